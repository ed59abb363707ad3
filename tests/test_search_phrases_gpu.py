"""search_phrases on the MI355X, end to end.

EXHAUSTIVE (W = 8 >= the widest trie level, N = 4, penalty 0) on the three models, images, prompts and the K = 12 phrases of
tests/test_score_phrases_gpu.py: the result is held against ``score_phrases`` -- the same quantity from a walk that prunes nothing --
with that file's MEASURED per-token allowance (generate_captions' greedy token log-probs against ``score`` on the same model and
images, code older than both calls), times the phrase's tokens + 1 and its margin of 2.

PRUNED (W = 2, N = 2, penalties 0 and 1) on the tiny model: against ``phrase_beam_search_host`` driven by the model's own forward, the
``Case`` pattern of tests/test_caption_beams_gpu.py with its measured step-vs-forward logit difference: an image whose replica decided
everywhere on a gap above that difference must give equal phrases and lengths, and log-probs within the difference times tokens + 1;
at most a third of the images may decide inside it."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import phrase_beam_search_host, phrase_trie, trie_widest_level
from image2text_amd.synth import reference_unit_test_config, synthetic_batch, tiny_config
from test_caption_beams_gpu import Case
from test_generate_captions_gpu import GREEDY, _ved
from test_score_phrases_gpu import B, EOS, PHRASES, PMAX, T, dev, measured_allowance, model  # noqa: F401  (model: the fixture)

pytestmark = pytest.mark.gpu

K = len(PHRASES)
# The input seed of the pruned searches: images and prompts are synthetic_batch(6, ..., seed).  Chosen on the CPU from candidates
# 0 .. 15: ``phrase_beam_search_host`` (W = 2, N = 2, penalties 0 and 1) over the oracle's forward (oracle/reference_model.forward on the
# tiny weights), taking the seed with the largest smallest decision gap (``gaps`` and ``pool_gaps``) over its six images.
PRUNED_SEED = 14
PRUNED_SEED_GAP = 0.659                 # that smallest gap, on the oracle

_ALLOWANCE = {}


@pytest.mark.parametrize('P', [1, 3])
def test_exhaustive_search_against_score_phrases(model, P):
    name, m, images, full, pad = model
    prompt = full[:, :P].contiguous()
    if name not in _ALLOWANCE:          # one value per model, over both prompt lengths, as in tests/test_score_phrases_gpu.py
        _ALLOWANCE[name] = max(measured_allowance(m, images, full[:, :p].contiguous(), pad) for p in (1, PMAX))
    per_token = _ALLOWANCE[name]
    assert 0 < per_token < 0.5
    W, N = 8, 4
    res = m.search_phrases(images, prompt, PHRASES, EOS, num_beams=W, num_return_sequences=N)
    assert res.exhaustive is True and trie_widest_level(phrase_trie(PHRASES, EOS, m._engine.dec.V, 1 << 30)) == 6
    assert tuple(res.phrase_index.shape) == (B, N) and res.phrase_index.dtype == torch.int64
    assert res.logprob.dtype == torch.float32 and res.scores.dtype == torch.float32 and res.lengths.dtype == torch.int32
    assert torch.equal(res.scores.view(torch.int32), res.logprob.view(torch.int32)), 'penalty 0: the score is the log-prob'
    assert bool((res.scores[:, :-1] >= res.scores[:, 1:]).all()), 'best first'
    assert torch.isfinite(res.logprob).all() and bool((res.logprob < 0).all())
    sp = m.score_phrases(images, prompt, PHRASES, EOS)
    ref = sp.logprob.double().cpu().numpy()
    allow = 2 * per_token * sp.lengths.double().cpu().numpy()           # per phrase: (tokens + 1) . measured . margin 2
    idx, lp = res.phrase_index.cpu().numpy(), res.logprob.double().cpu().numpy()
    worst, excused = 0.0, 0
    for b in range(B):
        took = [PHRASES[k] for k in idx[b]]
        assert len({tuple(p) for p in took}) == N, 'distinct as token lists'
        assert all(k == PHRASES.index(PHRASES[k]) for k in idx[b]), 'a duplicate goes by the index the trie holds'
        assert res.lengths[b].tolist() == [len(p) + 1 for p in took]
        for n in range(N):
            err = abs(lp[b, n] - ref[b, idx[b, n]])
            worst = max(worst, err / allow[idx[b, n]])
            assert err <= allow[idx[b, n]], f'{name} P {P} image {b} entry {n}: logprob error {err:.3g} over allowance {allow[idx[b, n]]:.3g}'
        last = idx[b, N - 1]
        for k in range(K):
            if PHRASES[k] not in took:
                assert ref[b, k] - ref[b, last] <= allow[k] + allow[last], f'{name} P {P} image {b}: phrase {k} left out above the fourth'
        for n in range(N - 1):
            assert ref[b, idx[b, n + 1]] - ref[b, idx[b, n]] <= allow[idx[b, n]] + allow[idx[b, n + 1]], f'{name} P {P} image {b}: order at {n}'
        first = int(sp.best[b])
        rival_k = max((k for k in range(K) if PHRASES[k] != PHRASES[first]), key=lambda k: ref[b, k])
        if not ref[b, first] - ref[b, rival_k] > 2 * max(allow[first], allow[rival_k]):
            excused += 1
            continue
        assert idx[b, 0] == PHRASES.index(PHRASES[first]), f'{name} P {P}: image {b}: first {idx[b, 0]}, score_phrases {first}'
    print(f'{name} P {P}: per-token allowance {per_token:.3g}; worst logprob error / allowance {worst:.3g}; {excused} of {B} first choices '
          f'decide inside the allowance')
    assert excused <= 1


# ------------------------------------------------------------------------------------------------------ pruned, against the replica
@pytest.fixture(scope='module')
def tiny(tiny_weights):
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(6, 32, 12, 384, seed=PRUNED_SEED)
    return Case(m, images.to(dev()), labels[:, :2].clamp(min=0).to(dev()))


def check_against_replica(case, phrases, W, N, penalty, **kw):
    m = case.m
    trie = phrase_trie(phrases, EOS, case.V, 1 << 30)
    out = m.search_phrases(case.images, case.prompt, phrases, EOS, num_beams=W, num_return_sequences=N, length_penalty=penalty, **kw)
    assert out.exhaustive == (W >= trie_widest_level(trie)) and tuple(out.phrase_index.shape) == (case.B, N)
    idx, lens = out.phrase_index.cpu().numpy(), out.lengths.cpu().numpy()
    lp, sc = out.logprob.cpu().numpy(), out.scores.cpu().numpy()
    outside, smallest = 0, np.inf
    for b in range(case.B):
        want = phrase_beam_search_host(case.step_logits(b), case.prompt[b].tolist(), trie, EOS, W, N, penalty)
        margin = min(want.gaps + want.pool_gaps)
        smallest = min(smallest, margin)
        if not margin > case.diff:
            outside += 1
            continue
        assert np.array_equal(idx[b], want.phrase_index) and np.array_equal(lens[b], want.lengths), (b, idx[b], want.phrase_index)
        tol = case.diff * want.lengths
        assert (np.abs(lp[b] - want.logprob) <= tol).all() and (np.abs(sc[b] - want.scores) <= tol).all(), (b, lp[b], want.logprob)
    print(f'W={W} N={N} penalty={penalty}: {outside} of {case.B} images decide inside the measured difference {case.diff:.3g}; smallest '
          f'host decision gap {smallest:.3g} (on the oracle at this seed: {PRUNED_SEED_GAP})')
    assert outside * 3 <= case.B, f'{outside} of {case.B} images fall outside the margin rule'
    return out


@pytest.mark.parametrize('penalty', [0.0, 1.0])
def test_pruned_search_against_the_replica(tiny, penalty):
    out = check_against_replica(tiny, PHRASES, 2, 2, penalty)
    assert out.exhaustive is False


def test_graph_eager_and_polling_agree(tiny):
    m = tiny.m
    m.search_phrases(tiny.images, tiny.prompt, PHRASES, EOS)             # the model's own decoder exists
    dec = m._phrase_searcher
    trie = phrase_trie(PHRASES, EOS, tiny.V, 1 << 30)
    args = (tiny.images, tiny.prompt, trie, EOS, 4, 4, 1.0)
    want = dec.search(*args, poll_every=8)
    for kw in (dict(poll_every=0), dict(poll_every=1), dict(poll_every=8, use_graph=False), dict(poll_every=0, use_graph=False)):
        got = dec.search(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4])) and got.exhaustive == want.exhaustive, kw
        if kw['poll_every'] == 0:
            assert dec.last_replays == trie.longest + 1


def test_the_close_rule_saves_steps(tiny):
    """eight one-token phrases, each also the head of a six-token one: after the one-token phrases fill the pool no six-token
    continuation can reach it, and the image closes long before the longest phrase ends"""
    heads = [17, 63, 77, 88, 31, 9, 42, 21]
    phrases = [[t] for t in heads] + [[t, 90, 91, 92, 93, 94] for t in heads]
    out = check_against_replica(tiny, phrases, 2, 2, 0.0, poll_every=1)
    dec = tiny.m._phrase_searcher
    assert dec.last_replays < 6 + 1 and dec.last_replays < tiny.P - 1 + 6 + 1, dec.last_replays
    assert bool((out.lengths == 2).all())
    every = tiny.m.search_phrases(tiny.images, tiny.prompt, phrases, EOS, num_beams=2, num_return_sequences=2, poll_every=0)
    assert dec.last_replays == 7 and all(torch.equal(a, b) for a, b in zip(every[:4], out[:4])), 'the replays past the close change nothing'


def test_one_beam_is_the_greedy_walk(tiny):
    m = tiny.m
    walk = m.generate_captions(tiny.images, tiny.prompt, max_new_tokens=T, eos_token_id=EOS, pad_token_id=tiny.pad, phrases=PHRASES, **GREEDY)
    one = m.search_phrases(tiny.images, tiny.prompt, PHRASES, EOS, num_beams=1)
    assert one.exhaustive is False and torch.equal(one.phrase_index[:, 0], walk.phrase_index[:, 0].long())
    assert torch.equal(one.lengths[:, 0], walk.lengths[:, 0] - tiny.P)
    lps = walk.token_logprobs[:, 0].cpu().numpy()
    acc = np.zeros(tiny.B, dtype=np.float32)
    for t in range(lps.shape[1]):                               # in the search's order: the path sum takes one token at a time
        acc = (acc + lps[:, t]).astype(np.float32)
    assert np.array_equal(acc.view(np.int32), one.logprob[:, 0].cpu().numpy().view(np.int32)), (acc, one.logprob[:, 0])


def test_refusals_from_the_model(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = _ved(tiny_config(), tiny_weights)
    V = m._engine.dec.V
    images, labels = synthetic_batch(2, 32, 12, 384, seed=7)
    images, prompt = images.to(dev()), labels[:, :PMAX].clamp(min=0).to(dev())
    for bad, text in (([], 'phrases is empty'), ([[3], []], 'is empty'), ([[V]], 'outside the vocabulary'), ([[3, EOS]], 'holds eos_token_id')):
        with pytest.raises(ValueError, match=text):
            m.search_phrases(images, prompt, bad, EOS)
    with pytest.raises(ValueError, match='need eos_token_id'):
        m.search_phrases(images, prompt, PHRASES, None)
    with pytest.raises(ValueError, match='num_beams = 9'):
        m.search_phrases(images, prompt, PHRASES, EOS, num_beams=9)
    with pytest.raises(ValueError, match='num_return_sequences = 5 with num_beams = 4'):
        m.search_phrases(images, prompt, PHRASES, EOS, num_return_sequences=5)
    with pytest.raises(ValueError, match='length_penalty'):
        m.search_phrases(images, prompt, PHRASES, EOS, length_penalty=float('inf'))
    with pytest.raises(ValueError, match='poll_every = -1'):
        m.search_phrases(images, prompt, PHRASES, EOS, poll_every=-1)
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match=rf'prompt \+ new tokens \({window + 1}\) exceed the text window \({window}\)'):
        m.search_phrases(images, prompt, [[7] * (window - PMAX)], EOS)
    assert m._phrase_searcher is None, 'a refused call ran something'
    with pytest.raises(NotImplementedError, match='no trie state per hypothesis'):
        m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=EOS, phrases=PHRASES, num_beams=2)
    nc = VisionEncoderDecoder(reference_unit_test_config()).to(dev()).eval()
    with pytest.raises(NotImplementedError, match='non-causal decoder'):
        nc.search_phrases(torch.zeros(2, 3, 128, 128, device=dev()), torch.zeros(2, 1, dtype=torch.long, device=dev()), [[3]], EOS)
