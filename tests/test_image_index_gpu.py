"""``image_index`` on generate_captions / score_phrases_indexed / search_phrases on the MI355X: several prompts per image in one call.

The rule of tests/test_ragged_prompts_gpu.py holds here: where the call with ``image_index`` and the existing call have the same rows
and launch shapes, every kernel treats rows and images independently, so the results are held to BIT equality -- there is no
tolerance in legs (a), (b) and (d).
  (a) Q = 2 B, image_index = [0, 0, 1, 1], both queries of an image with its prompt, N = 1, against the existing call with
      num_return_sequences = 2, reshaped: the rows are (b, n) in both, and the sampling draw is keyed by (seed, step, row), so the
      seeds match by construction.  Greedy with N = 2 is refused by the existing checks (the rows would be identical), so the greedy
      leg's expectation is the existing call on images.repeat_interleave(2): the same Q rows, the encoder over Q images.
  (b) B = Q = 4, image_index = [2, 0, 2, 1] (a duplicate, image 3 unused), a prompt per query, against the existing call on
      images[image_index]: the encoder sees 4 images in both runs and the steps the same R rows.
  (c) Q = 5 over B = 2: shapes, the encoder's batch sizes, equal queries give bit-identical rows, and score_phrases' logprob against
      the existing call on images[image_index] -- the encoder then runs over 5 images, another launch shape -- within logits_tol, the
      bar tests/test_score_gpu.py holds two routes of one quantity to.  No ids are compared in that leg.
  (d) without, with, without on one model: the first and the third call are bit-equal (state and graph keying).
Models: the dense tiny decoder (d = 128, the segment-maxima head), its d = 64 one-head twin (fp32-logits head, one wave per
workgroup), the sparse / multi-query nano-mini family (the grouped-query kernel; score_phrases / search_phrases refuse it), a
Hugging Face GPT-2 with a soft prompt, whose prefix rows reach the rows of the head-major cache through the gather, and the tiny
Llama of tests/test_hf_decoder_gpu.py (no cross-attention: what it runs of this feature is the gather of the prefix rows into the
row-major cache, in _prepare_inputs' layer sink and in TrieScoreDecoder._load_group)."""
import pytest
import torch

from image2text_amd.synth import det_init_, mini_config, sharpen_gates_, synthetic_batch, tiny_config
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

F32 = torch.float32
EOS, T, P = 3, 6, 3
SET_A = [[7, 8], [7, 9, 10], [11], [12, 13]]
SET_B = [[20], [21, 22], [21, 23]]
INDEX = [2, 0, 2, 1]
PLEN = [1, 3, 2, 3]
CAPTION_FIELDS = ('ids', 'lengths', 'token_logprobs', 'logprob', 'prompt_lengths', 'beam_scores', 'phrase_index')


def dev():
    return torch.device('cuda:0')


def _ved(cfg, weights=None, sharpen=False):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(cfg)
    if weights is not None:
        m.load_state_dict(weights)
    else:
        det_init_(m, seed=0)
        if sharpen:
            sharpen_gates_(m)
    return m.to(dev()).eval()


def _model(name, tiny_weights, tmp_path, monkeypatch):
    """-> (model, images [4, ...], prompt [5, P]: a prompt per query, rows 0 and 2 equal)"""
    V = 384
    if name == 'tiny':
        m = _ved(tiny_config(), tiny_weights)
        assert m._engine.dec.d % 128 == 0
    elif name == 'dense64':
        m = _ved(tiny_config(dec_d=64, dec_heads=1))
    elif name == 'mini':
        m = _ved(mini_config(), sharpen=True)
        assert m._engine.dec.fam is not None and m._engine.dec.fam.sparse
    elif name == 'hf_llama':
        from test_hf_decoder_gpu import _llama_model
        _, m, _, V = _llama_model(tmp_path, monkeypatch, 'llama')
        m = m.to(dev()).eval()
        assert m._engine.dec.llama is not None and m._engine.dec.prefixed and not m._engine.cross_inputs
    else:
        from test_hf_decoder_gpu import _build
        _, m = _build(tmp_path, monkeypatch, True, True)
        m = m.to(dev()).eval()
        assert m._engine.dec.prefixed
        V = m._engine.dec.V
    images, labels = synthetic_batch(5, 32, 12, min(V, 384), seed=11)
    prompt = labels[:, :P].clamp(min=0)
    prompt[prompt == EOS] = EOS + 1
    prompt[2] = prompt[0]
    return m, images[:4].to(dev()), prompt.to(dev())


@pytest.fixture(params=['tiny', 'dense64', 'mini', 'hf_gpt2_soft', 'hf_llama'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    return (request.param,) + _model(request.param, tiny_weights, tmp_path, monkeypatch)


@pytest.fixture(params=['tiny', 'dense64', 'hf_gpt2_soft', 'hf_llama'])
def dense_model(request, tiny_weights, tmp_path, monkeypatch):
    """the models score_phrases / search_phrases run on (they refuse sparse nano-mini blocks)"""
    return (request.param,) + _model(request.param, tiny_weights, tmp_path, monkeypatch)


def bits(x):
    return x.view(torch.int32) if x.dtype == F32 else x


def same_captions(got, want, what, reshape=None):
    for f in CAPTION_FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), f'{what}: {f}'
        if g is not None:
            w = w if reshape is None or f == 'prompt_lengths' else w.reshape(reshape + w.shape[2:])
            assert g.shape == w.shape and torch.equal(bits(g), bits(w)), f'{what}: {f} differs'


def same_tuple(got, want, what):
    assert type(got) is type(want) and len(got) == len(want)
    for f, g, w in zip(got._fields, got, want):
        assert torch.equal(bits(g), bits(w)) if isinstance(g, torch.Tensor) else g == w, f'{what}: {f} differs'


def carries(out, index):
    assert out.image_index is not None and out.image_index.dtype == torch.int32 and out.image_index.tolist() == list(index)


# ------------------------------------------------------------------------------------------------------------------ (a)
def test_interleaved_queries_are_the_n_rows_of_an_image(model):
    name, m, images, prompt = model
    images, prompt = images[:2], prompt[:2]
    twice, index = prompt.repeat_interleave(2, dim=0), [0, 0, 1, 1]
    kw = dict(max_new_tokens=T, eos_token_id=EOS, temperature=1.2, top_k=30, seed=77)
    want = m.generate_captions(images, prompt, num_return_sequences=2, **kw)
    got = m.generate_captions(images, twice, image_index=index, **kw)
    assert want.image_index is None and tuple(got.ids.shape[:2]) == (4, 1)
    carries(got, index)
    same_captions(got, want, f'{name} sampling', reshape=(4, 1))
    kw = dict(max_new_tokens=T, eos_token_id=EOS, top_k=1)
    got = m.generate_captions(images, twice, image_index=index, **kw)
    same_captions(got, m.generate_captions(images.repeat_interleave(2, dim=0), twice, **kw), f'{name} greedy')
    assert torch.equal(got.ids[0], got.ids[1]) and torch.equal(bits(got.token_logprobs[2]), bits(got.token_logprobs[3]))


# ------------------------------------------------------------------------------------------------------------------ (b)
CAPTION_MODES = {
    'greedy': dict(top_k=1),
    'sampling_n2': dict(temperature=1.2, top_k=30, seed=5, num_return_sequences=2),
    'prompt_lengths': dict(top_k=1, prompt_lengths=PLEN),
    'phrase_sets_ragged': dict(top_k=1, phrase_sets=[SET_A, SET_B], phrase_set_index=[0, 1, 1, 0], prompt_lengths=PLEN),
    'processors': dict(top_k=1, repetition_penalty=1.3, min_new_tokens=3),
    'beams': dict(num_beams=3, num_return_sequences=2),
}


def test_a_map_with_duplicates_generate_captions(model):
    name, m, images, prompt = model
    prompt = prompt[:4]
    for mode, kw in CAPTION_MODES.items():
        kw = dict(kw, max_new_tokens=T, eos_token_id=EOS)
        want = m.generate_captions(images[INDEX], prompt, **kw)
        got = m.generate_captions(images, prompt, image_index=INDEX, **kw)
        same_captions(got, want, f'{name} {mode}')
        carries(got, INDEX)
        assert tuple(got.ids.shape[:2]) == (4, kw.get('num_return_sequences', 1))
    tensor_form = m.generate_captions(images, prompt, image_index=torch.tensor(INDEX, device=dev()), max_new_tokens=T, eos_token_id=EOS, top_k=1)
    same_captions(tensor_form, m.generate_captions(images, prompt, image_index=INDEX, max_new_tokens=T, eos_token_id=EOS, top_k=1), 'a tensor index')


def test_a_map_with_duplicates_phrase_calls(dense_model):
    name, m, images, prompt = dense_model
    prompt = prompt[:4]
    sets = dict(phrase_sets=[SET_A, SET_B], phrase_set_index=[0, 1, 1, 0], prompt_lengths=PLEN)
    for W in (2, 4):                                            # below, and at least, the widest level (3)
        for kw in (dict(phrases=SET_A), sets):
            kw = dict(kw, eos_token_id=EOS, num_beams=W, num_return_sequences=2)
            got = m.search_phrases(images, prompt, image_index=INDEX, **kw)
            same_tuple(got, m.search_phrases(images[INDEX], prompt, **kw), f'{name} search W={W}')
            carries(got, INDEX)
            assert got.exhaustive == (W >= 3)
    for kw in (dict(phrases=SET_A), sets):
        kw = dict(kw, eos_token_id=EOS)
        want = m.score_phrases(images[INDEX], prompt, **kw)
        for per_pass in (None, 1, 3):                           # the grouping does not change a bit
            got = m.score_phrases_indexed(images, prompt, INDEX, images_per_pass=per_pass, **kw)
            same_tuple(got, want, f'{name} score_phrases images_per_pass={per_pass}')
            carries(got, INDEX)


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_five_queries_over_two_images(model, monkeypatch):
    name, m, images, prompt = model
    images, index = images[:2], [1, 0, 1, 1, 0]                 # queries 0 and 2: the same image and the same prompt
    eng, calls = m._engine, []
    real = eng.encode
    monkeypatch.setattr(eng, 'encode', lambda im, save: (calls.append(int(im.shape[0])), real(im, save))[1])
    out = m.generate_captions(images, prompt, image_index=index, max_new_tokens=T, eos_token_id=EOS, temperature=1.1, top_k=20, seed=9,
                              num_return_sequences=2)
    assert calls == [2], 'the encoder ran once, over the 2 images'
    L = out.ids.shape[-1]
    assert tuple(out.ids.shape) == (5, 2, L) and tuple(out.lengths.shape) == (5, 2) and tuple(out.token_logprobs.shape) == (5, 2, L - P)
    assert tuple(out.logprob.shape) == (5, 2) and bool((out.ids[:, :, :P] == prompt[:, None]).all())
    carries(out, index)
    greedy = m.generate_captions(images, prompt, image_index=index, max_new_tokens=T, eos_token_id=EOS, top_k=1)
    assert torch.equal(greedy.ids[0], greedy.ids[2]) and torch.equal(bits(greedy.token_logprobs[0]), bits(greedy.token_logprobs[2]))
    beams = m.generate_captions(images, prompt, image_index=index, max_new_tokens=T, eos_token_id=EOS, num_beams=3, num_return_sequences=3)
    assert tuple(beams.ids.shape[:2]) == (5, 3) and torch.equal(beams.ids[0], beams.ids[2]) and torch.equal(bits(beams.beam_scores[0]), bits(beams.beam_scores[2]))
    if m._engine.dec.fam is not None and m._engine.dec.fam.sparse:
        return                                                  # score_phrases / search_phrases refuse sparse blocks, with or without the argument
    calls.clear()
    got = m.score_phrases_indexed(images, prompt, index, SET_A, EOS, images_per_pass=2)
    assert calls == [2] and tuple(got.logprob.shape) == (5, len(SET_A)) and tuple(got.best.shape) == (5,)
    assert torch.equal(bits(got.logprob[0]), bits(got.logprob[2]))
    want = m.score_phrases(images[index], prompt, SET_A, EOS)
    err, bar = float((got.logprob - want.logprob).abs().max()), logits_tol(want.logprob.cpu().numpy())
    print(f'{name}: score_phrases over 2 images vs over images[image_index]: max |err| {err:.4g}, bar {bar:.4g}')
    assert err <= bar
    found = m.search_phrases(images, prompt, SET_A, EOS, num_beams=4, num_return_sequences=2, image_index=index)
    assert tuple(found.phrase_index.shape) == (5, 2) and torch.equal(found.phrase_index[0], found.phrase_index[2])


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_calls_without_and_with_the_index_do_not_disturb_each_other(model):
    name, m, images, prompt = model
    prompt = prompt[:4]
    for kw in (dict(top_k=1), dict(temperature=1.2, top_k=30, seed=5, num_return_sequences=2), dict(num_beams=3)):
        kw = dict(kw, max_new_tokens=T, eos_token_id=EOS)
        first = m.generate_captions(images, prompt, **kw)
        with_index = m.generate_captions(images, prompt, image_index=INDEX, **kw)
        third = m.generate_captions(images, prompt, **kw)
        same_captions(third, first, f'{name} {sorted(kw)}')
        assert first.image_index is None and third.image_index is None
        # another number of memory rows: a state of its own (the encoder then runs over 3 images, another launch shape: no bits are compared)
        again = m.generate_captions(images[:3], prompt, image_index=INDEX, **kw)
        assert again.ids.shape[:2] == with_index.ids.shape[:2] and bool((again.ids[:, :, :P] == prompt[:, None]).all())
        same_captions(m.generate_captions(images, prompt, image_index=INDEX, **kw), with_index, f'{name} with, again {sorted(kw)}')


def test_non_causal_decoder_recomputes_over_the_gathered_images():
    from image2text_amd.synth import reference_unit_test_config
    m = _ved(reference_unit_test_config(), sharpen=True)
    assert not m._engine.dec.causal
    images, labels = synthetic_batch(2, 128, 12, 1024, seed=9)
    images, prompt = images.to(dev()), labels[:3, :2].clamp(min=0).repeat(2, 1)[:3].to(dev())
    index = [1, 0, 1]
    kw = dict(max_new_tokens=3, top_k=1)
    got = m.generate_captions(images, prompt, image_index=index, **kw)
    same_captions(got, m.generate_captions(images[index], prompt, **kw), 'non-causal')
    carries(got, index)


def test_rerank_takes_the_index(tiny_weights):
    from image2text_amd.models.generation_utils import rerank
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(3, 32, 12, 384, seed=11)
    images = images.to(dev())
    cand = labels[:4, :8].clamp(min=0).repeat(2, 1)[:4].view(4, 1, 8).repeat(1, 2, 1).to(dev())
    cand[:, 1, 3:] = (cand[:, 1, 3:] + 5) % 380
    cand[2] = cand[0]
    order, lp = rerank(m, images, cand, image_index=[2, 0, 2, 1])
    _, want_lp = rerank(m, images[[2, 0, 2, 1]], cand)          # the encoder over 4 gathered images: another launch shape, so a tolerance
    assert tuple(order.shape) == (4, 2) and float((lp - want_lp).abs().max()) <= logits_tol(want_lp.cpu().numpy())
    assert torch.equal(bits(lp[0]), bits(lp[2])), 'rows 0 and 2: the same image and candidates'
