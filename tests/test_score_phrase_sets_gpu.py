"""score_phrases(phrase_sets=..., phrase_set_index=..., prompt_lengths=...) on the MI355X, end to end: the three models
of tests/test_score_phrases_gpu.py -- the tiny dense model (d = 128: the rows' LSE from i2t_gemm_bf16_lse's segments, no logits), a
decoder of width 64 (the fp32 lm_head + i2t_rows_lse) and the tiny Llama with a soft prompt --; B = 8 images, S = 3 sets of K = 5, 12 and
8 phrases of one to four tokens (prefixes and a duplicate among them), prompt lengths 1, 2 and 3 mixed.  The widest level of any set
holds 6 nodes, so a pass of 8 images runs 48 rows and the walk takes min p - 1 = 0 prefill steps and up to 3 + 4 + 1 - 1 = 7 walk steps.

``logprob[b, :K_s]`` is held against ``score`` through ``rerank`` on the image's OWN prompt and set.  The allowance per token is
MEASURED in the test from code that existed before the call did, exactly as tests/test_score_phrases_gpu.py does (its
``measured_allowance``: the largest |generate_captions greedy token log-prob - score at the same ids| per model, the larger of P = 1
and P = 3), times the phrase's tokens + 1 and that test's margin of 2.  ``best`` equals rerank's first choice wherever the score-side
gap between the best phrase and the best DIFFERENT phrase exceeds twice that allowance; at most 1 image of 8 may be excused.

Measured on the MI355X at the seeds below: per-token allowance tiny 0.0149, width-64 0.00286, Llama 0.00314; worst logprob error over
the allowance tiny 0.792, width-64 0.206, Llama 0.202; 0 of 8 images excused on every model; search_phrases (num_beams = 8, exhaustive)
names the same phrase on every image, its log-prob within 1.5e-4 of the allowance of score_phrases'."""
import numpy as np
import pytest
import torch

from image2text_amd.models.generation_utils import rerank
from image2text_amd.synth import reference_unit_test_config, synthetic_batch, tiny_config
from test_generate_captions_gpu import _ved
from test_score_phrases_gpu import EOS, PHRASES, measured_allowance

pytestmark = pytest.mark.gpu

B, PMAX = 8, 3
# set 0: a four-token phrase, [17 42] and [17 9] share a first token.  Levels: 1, 4, 4, 1, 1 nodes
SET0 = [[17, 42], [63], [77, 4, 4, 9], [17, 9], [88, 12]]
# set 1: the 12 phrases of tests/test_score_phrases_gpu.py (6 repeats 2; four prefix pairs).  Levels: 1, 5, 6, 4 nodes
SET1 = PHRASES
# set 2: 7 repeats 0; [31] < [31 7] < [31 7 19], [63 21] < [63 21 30], [90] < [90 2].  Levels: 1, 3, 3, 2 nodes
SET2 = [[31], [31, 7], [31, 7, 19], [63, 21], [63, 21, 30], [90], [90, 2], [31]]
SETS = [SET0, SET1, SET2]
INDEX = [0, 1, 2, 1, 0, 2, 1, 0]
PLEN = [1, 2, 3, 3, 1, 2, 1, 3]
KMAX, WMAX = 12, 6
# The input seed of every model: its images and prompts are synthetic_batch(B, ..., seed) / a torch generator of that seed, as in
# tests/test_score_phrases_gpu.py.  Chosen on the CPU from candidates 0 .. 15: ``phrase_set_scores_host`` over the oracle's forward
# (oracle/reference_model.forward for tiny and the width-64 decoder; oracle encode + the checkpoint's own transformers module in fp32 for
# the Llama) on the sets, indices and prompt lengths above, taking the seed with the largest smallest gap between an image's best phrase
# and its best different phrase; the oracle alone excuses 0 of 8 images at it.  Smallest oracle gap at the chosen seed: SEED_GAPS.
SEEDS = dict(tiny=9, dense64=3, llama=3)
SEED_GAPS = dict(tiny=3.329, dense64=0.2634, llama=0.2231)


def dev():
    return torch.device('cuda:0')


def inputs(name, seed, V):
    """the images [8, ...] and prompts [8, 3] of one model at one seed (the seed search on the CPU builds the same)"""
    if name == 'llama':
        g = torch.Generator().manual_seed(seed)
        return torch.randn(B, 3, 32, 32, generator=g), torch.randint(0, V, (B, PMAX), generator=g)
    images, labels = synthetic_batch(B, 32, 12, min(V, 384), seed=seed)
    return images, labels[:, :PMAX].clamp(min=0)


@pytest.fixture(scope='module', params=['tiny', 'dense64', 'llama'])
def model(request, tiny_weights, tmp_path_factory):
    """-> (name, model, images [8, ...], prompt [8, 3], pad id)"""
    name = request.param
    if name == 'llama':
        from test_hf_decoder_gpu import _llama_model
        mp = pytest.MonkeyPatch()
        request.addfinalizer(mp.undo)
        _, m, _, V = _llama_model(tmp_path_factory.mktemp('llama'), mp, 'llama')
        m = m.to(dev()).eval()
    else:
        m = _ved(tiny_config(), tiny_weights) if name == 'tiny' else _ved(tiny_config(dec_d=64, dec_heads=1))
        assert (m._engine.dec.d % 128 == 0) == (name == 'tiny')
        V = m._engine.dec.V
    assert V > 90
    images, prompt = inputs(name, SEEDS[name], V)
    return name, m, images.to(dev()), prompt.to(dev()), V - 1


_ALLOWANCE = {}


def per_token_allowance(name, m, images, full, pad):
    if name not in _ALLOWANCE:          # one value per model, over both prompt lengths, as tests/test_score_phrases_gpu.py takes it
        _ALLOWANCE[name] = max(measured_allowance(m, images, full[:, :p].contiguous(), pad) for p in (1, PMAX))
    assert 0 < _ALLOWANCE[name] < 0.5
    return _ALLOWANCE[name]


def ragged(m, images, prompt, **kw):
    return m.score_phrases(images, prompt, eos_token_id=EOS, phrase_sets=SETS, phrase_set_index=INDEX, prompt_lengths=PLEN, **kw)


def own_rerank(m, images, prompt, b):
    """rerank of image b's own set behind its own prompt -> (order [K], logprob [K])"""
    phrases, p = SETS[INDEX[b]], PLEN[b]
    L = p + max(len(ph) for ph in phrases) + 1
    cand = torch.full((1, len(phrases), L), EOS, dtype=torch.long, device=prompt.device)
    cand[0, :, :p] = prompt[b, :p]
    for k, ph in enumerate(phrases):
        cand[0, k, p:p + len(ph)] = torch.tensor(ph, device=prompt.device)
    order, ref = rerank(m, images[b:b + 1], cand, eos=EOS, prompt_len=p)
    return order[0], ref[0]


def test_one_set_for_all_images_is_score_phrases_bit_for_bit(model):
    """8 x 6 = 48 rows either way: the same GEMM routes"""
    name, m, images, prompt, pad = model
    old = m.score_phrases(images, prompt, SET1, EOS)
    new = m.score_phrases(images, prompt, eos_token_id=EOS, phrase_sets=[SET1], phrase_set_index=[0] * B)
    assert type(old).__name__ == 'PhraseScores' and type(new).__name__ == 'PhraseSetScores'
    assert tuple(new.logprob.shape) == (B, len(SET1)) and tuple(new.lengths.shape) == (1, len(SET1))
    assert torch.equal(old.logprob.view(torch.int32), new.logprob.view(torch.int32)), f'{name}: the one-set call differs from score_phrases'
    assert torch.equal(old.best, new.best) and torch.equal(old.lengths, new.lengths[0])
    again = m.score_phrases(images, prompt, phrases=SET1, eos_token_id=EOS)
    assert torch.equal(old.logprob.view(torch.int32), again.logprob.view(torch.int32)), 'the old call after the new one'


def test_ragged_sets_against_rerank_and_search_phrases(model):
    name, m, images, prompt, pad = model
    per_token = per_token_allowance(name, m, images, prompt, pad)
    res = ragged(m, images, prompt)
    assert tuple(res.logprob.shape) == (B, KMAX) and res.logprob.dtype == torch.float32 and res.best.dtype == torch.int64 and tuple(res.best.shape) == (B,)
    assert res.lengths.dtype == torch.int32 and res.lengths.tolist() == [[len(p) + 1 for p in s] + [0] * (KMAX - len(s)) for s in SETS]
    assert m._trie_scorer._score_state.W == WMAX
    beams = m.search_phrases(images, prompt, eos_token_id=EOS, num_beams=8, num_return_sequences=1, phrase_sets=SETS, phrase_set_index=INDEX,
                             prompt_lengths=PLEN)
    assert beams.exhaustive
    excused, worst, worst_beam = 0, 0.0, 0.0
    for b in range(B):
        phrases = SETS[INDEX[b]]
        K = len(phrases)
        lp = res.logprob[b]
        assert torch.isfinite(lp[:K]).all() and bool((lp[:K] < 0).all()) and torch.isneginf(lp[K:]).all(), f'{name}: image {b}: the padding is -inf'
        dup = [(i, j) for i in range(K) for j in range(i + 1, K) if phrases[i] == phrases[j]]
        assert all(lp[i].view(torch.int32) == lp[j].view(torch.int32) for i, j in dup), 'duplicate phrases get equal values'
        order, ref = own_rerank(m, images, prompt, b)
        allow = 2 * per_token * res.lengths[INDEX[b], :K].double()
        err = (lp[:K].double() - ref.double()).abs()
        worst = max(worst, float((err / allow).max()))
        assert bool((err <= allow).all()), f'{name}: image {b}: logprob vs score, worst error / allowance {float((err / allow).max()):.3g}'
        best = int(res.best[b])
        assert best == int(torch.nonzero(lp == lp.max())[0]) and best < K, 'best: the lowest index of the maximum, inside the own set'
        first = int(order[0])
        rivals = [k for k in range(K) if phrases[k] != phrases[first]]
        rival_k = max(rivals, key=lambda k: float(ref[k]))
        if not float(ref[first]) - float(ref[rival_k]) > 2 * float(max(allow[first], allow[rival_k])):
            excused += 1
        else:
            assert phrases[best] == phrases[first] and best == phrases.index(phrases[first]), f'{name}: image {b}: best {best}, rerank {first}'
            # the exhaustive trie beam names the same phrase, and reports the same quantity for it
            assert int(beams.phrase_index[b, 0]) == best, f'{name}: image {b}: search_phrases {int(beams.phrase_index[b, 0])}, score_phrases {best}'
        top = int(beams.phrase_index[b, 0])
        gap = abs(float(beams.logprob[b, 0]) - float(lp[top]))
        worst_beam = max(worst_beam, gap / float(allow[top]))
        assert gap <= float(allow[top]), f'{name}: image {b}: search_phrases logprob vs score_phrases {gap:.3g}'
        assert int(beams.lengths[b, 0]) == int(res.lengths[INDEX[b], top])
    print(f'{name}: measured per-token allowance {per_token:.3g}; logprob vs score worst error / allowance {worst:.3g}; search_phrases vs '
          f'score_phrases worst difference / allowance {worst_beam:.3g}; {excused} of {B} images decide inside the allowance')
    assert excused <= 1


def test_images_per_pass_changes_no_bit(model):
    """groups of 3, 3 and 2 images: 18 rows against one pass of 48, both on the weight-streaming GEMM route"""
    name, m, images, prompt, pad = model
    one = ragged(m, images, prompt, images_per_pass=B)
    assert m._trie_scorer.last_passes == 1
    three = ragged(m, images, prompt, images_per_pass=3)
    assert m._trie_scorer.last_passes == 3
    assert torch.equal(one.logprob.view(torch.int32), three.logprob.view(torch.int32)) and torch.equal(one.best, three.best)
    default = ragged(m, images, prompt)
    assert m._trie_scorer.last_passes == 1 and torch.equal(one.logprob.view(torch.int32), default.logprob.view(torch.int32))
    # what the caller leaves behind an image's prompt is not read
    noisy = prompt.clone()
    for b in range(B):
        noisy[b, PLEN[b]:] = 7
    assert torch.equal(one.logprob.view(torch.int32), ragged(m, images, noisy).logprob.view(torch.int32))


def test_refusals_from_the_model(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(2, 32, 12, 384, seed=7)
    images, prompt = images.to(dev()), labels[:, :PMAX].clamp(min=0).to(dev())
    sets = dict(phrase_sets=[SET0, SET2], phrase_set_index=[1, 0])
    with pytest.raises(ValueError, match='phrases and phrase_sets are both given'):
        m.score_phrases(images, prompt, SET1, EOS, **sets)
    with pytest.raises(ValueError, match='phrase_set_index without phrase_sets'):
        m.score_phrases(images, prompt, SET1, EOS, phrase_set_index=[0, 0])
    with pytest.raises(ValueError, match=r'needs phrase_sets.*phrase_sets=\[phrases\], phrase_set_index=\[0\] \* B'):
        m.score_phrases(images, prompt, SET1, EOS, prompt_lengths=[1, 2])
    with pytest.raises(ValueError, match='score_phrases needs phrases or phrase_sets'):
        m.score_phrases(images, prompt, eos_token_id=EOS)
    with pytest.raises(ValueError, match=r'prompt_lengths\[1\] = 4 exceeds the 3 columns'):
        m.score_phrases(images, prompt, eos_token_id=EOS, prompt_lengths=[1, 4], **sets)
    with pytest.raises(ValueError, match=r'phrase_set_index\[0\] = 2 is outside the 2 sets'):
        m.score_phrases(images, prompt, eos_token_id=EOS, phrase_sets=[SET0, SET2], phrase_set_index=[2, 0])
    with pytest.raises(ValueError, match='images_per_pass = 0'):
        m.score_phrases(images, prompt, eos_token_id=EOS, images_per_pass=0, **sets)
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match=rf'prompt \+ new tokens \({window + 1}\) exceed the text window \({window}\)'):
        m.score_phrases(images, prompt, eos_token_id=EOS, phrase_sets=[[[7] * (window - 2)], SET0], phrase_set_index=[0, 1], prompt_lengths=[2, 3])
    with pytest.raises(ValueError, match='need eos_token_id'):
        m.score_phrases(images, prompt, **sets)
    assert m._trie_scorer is None, 'a refused call ran something'
    nc = VisionEncoderDecoder(reference_unit_test_config()).to(dev()).eval()
    with pytest.raises(NotImplementedError, match='non-causal decoder'):
        nc.score_phrases(torch.zeros(2, 3, 128, 128, device=dev()), torch.zeros(2, 1, dtype=torch.long, device=dev()), eos_token_id=EOS,
                         phrase_sets=[[[3]]], phrase_set_index=[0, 0])
