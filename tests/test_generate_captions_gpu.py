"""VisionEncoderDecoder.generate_captions on the MI355X: generate() that stops at EOS, draws N captions per image and keeps the
log-prob of every token it chose.

Models: tiny (trained weights, d = 128: the segment form of the head), a decoder of width 64 (the fp32-logits form), the nano-mini
sparse / multi-query / MoE family at fixture size, and a Hugging Face GPT-2 decoder with a soft prompt.

The log-prob bar: token_logprobs against fp64 log_softmax(model(images_rep, ids).logits) at the generated ids, held to
4 . logits_tol(logits) (tests/test_model_gpu.py::logits_tol).  Step logits and forward logits are each held to logits_tol of the oracle
by existing tests, so they differ by at most 2 logits_tol; a log-prob is a logit minus a logsumexp that is 1-Lipschitz in the largest
change of a logit: 2 . 2 logits_tol.  For N > 1 the same comparison is the check that every row was conditioned on ITS image."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import apply_finish_rule
from image2text_amd.synth import det_init_, mini_config, sharpen_gates_, synthetic_batch, tiny_config
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

F32 = torch.float32
SAMPLING = dict(temperature=0.7, top_k=None, nucleus_p=0.6)
GREEDY = dict(top_k=1)


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


@pytest.fixture(params=['tiny', 'dense64', 'mini', 'hf_gpt2_soft'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    """-> (name, model, images [3, ...], prompt [3, 2])"""
    name = request.param
    V = 384
    if name == 'tiny':
        m = _ved(tiny_config(), tiny_weights)
        assert m._engine.dec.d % 128 == 0
    elif name == 'dense64':
        m = _ved(tiny_config(dec_d=64, dec_heads=1))
        assert m._engine.dec.d % 128 != 0
    elif name == 'mini':
        m = _ved(mini_config(), sharpen=True)
        assert m._engine.dec.fam is not None and m._engine.dec.fam.sparse
    else:
        from test_hf_decoder_gpu import _build
        _, m = _build(tmp_path, monkeypatch, True, True)
        m = m.to(dev()).eval()
        assert m._engine.dec.prefixed
        V = m._engine.dec.V
    images, labels = synthetic_batch(3, 32, 12, min(V, 384), seed=11)
    return name, m, images.to(dev()), labels[:, :2].clamp(min=0).to(dev())


def check_shapes(out, B, N, P):
    L = out.ids.shape[-1]
    assert tuple(out.ids.shape) == (B, N, L) and out.ids.dtype == torch.long
    assert tuple(out.lengths.shape) == (B, N) and out.lengths.dtype == torch.int32 and int(out.lengths.max()) == L
    assert tuple(out.token_logprobs.shape) == (B, N, L - P) and out.token_logprobs.dtype == F32
    assert tuple(out.logprob.shape) == (B, N) and torch.equal(out.logprob, out.token_logprobs.sum(dim=-1))


def check_logprobs(m, images, out, P, tag):
    """token_logprobs at the live positions against the model's own forward (fp64 log_softmax) and against score(): 4 . logits_tol"""
    B, N, L = out.ids.shape
    rep = images.repeat_interleave(N, dim=0)
    ids = out.ids.reshape(B * N, L)
    with torch.no_grad():
        logits = m(images=rep, ids=ids).logits
    assert logits.shape[1] == L
    bar = 4 * logits_tol(logits.float().cpu().numpy())
    ref = torch.log_softmax(logits.double(), dim=-1)[:, P - 1:L - 1].gather(-1, ids[:, P:, None])[..., 0]
    live = torch.arange(P, L, device=dev())[None, :] < out.lengths.reshape(B * N, 1)
    got = out.token_logprobs.reshape(B * N, L - P)
    err = float(((got.double() - ref).abs() * live).max())
    sc = m.score(rep, ids).token_logprobs[:, P - 1:L - 1]
    err_sc = float(((got - sc).abs() * live).max())
    print(f'{tag}: token_logprobs worst error / bar vs forward {err / bar:.3g}, vs score {err_sc / bar:.3g} (bar {bar:.3g})')
    assert torch.isfinite(got).all() and bool((got[live] <= bar).all()) and err <= bar and err_sc <= bar
    assert bool((got[~live] == 0).all())


@pytest.mark.parametrize('mode', [GREEDY, SAMPLING], ids=['greedy', 'sampling'])
def test_without_eos_it_is_generate(model, mode):
    """eos_token_id None, N = 1: the ids are generate()'s exactly (both draw their seed under the same torch.manual_seed)"""
    name, m, images, prompt = model
    B, P, T = images.shape[0], prompt.shape[1], 10
    torch.manual_seed(5)
    want = m.generate(images, prompt, max_new_tokens=T, **mode)
    torch.manual_seed(5)
    out = m.generate_captions(images, prompt, max_new_tokens=T, **mode)
    check_shapes(out, B, 1, P)
    assert torch.equal(out.ids[:, 0], want)
    assert bool((out.lengths == P + T).all())
    check_logprobs(m, images, out, P, f'{name} {"greedy" if mode is GREEDY else "sampling"}')
    torch.manual_seed(5)
    assert torch.equal(m.generate(images, prompt, max_new_tokens=T, **mode), want)          # generate() itself is undisturbed


def test_three_captions_per_image(model):
    """N = 3 sampled rows per image over ONE encoder pass and one cross K/V per image: each row's log-probs are those of the forward
    over its own image; a seed reproduces the call"""
    name, m, images, prompt = model
    B, P, T, N = images.shape[0], prompt.shape[1], 8, 3
    calls = []
    eng = m._engine
    real = eng.encode
    eng.encode = lambda im, save: (calls.append(int(im.shape[0])), real(im, save))[1]
    try:
        out = m.generate_captions(images, prompt, max_new_tokens=T, num_return_sequences=N, seed=1234, **SAMPLING)
    finally:
        del eng.encode
    assert calls == [B]
    check_shapes(out, B, N, P)
    assert bool((out.ids[:, :, :P] == prompt[:, None]).all())
    check_logprobs(m, images, out, P, f'{name} N=3')
    again = m.generate_captions(images, prompt, max_new_tokens=T, num_return_sequences=N, seed=1234, **SAMPLING)
    assert torch.equal(again.ids, out.ids) and torch.equal(again.token_logprobs, out.token_logprobs)


def test_eos_rule_early_stop_and_polling(tiny_weights):
    """with an EOS id the greedy run emits: the prefix up to each first EOS is unchanged, pads and exact zeros after it, lengths equal the
    host rule's, poll_every in {0, 1, 8} agree, and the replays launched stay within max(lengths) - P + poll_every"""
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(4, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :2].clamp(min=0).to(dev())
    P, T, PAD = 2, 24, 383
    free = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    raw = free.ids[:, 0].cpu().numpy()
    eos = int(raw[0, P + 3])                                  # row 0 emits it at its fourth step at the latest
    want_ids, want_len, want_lp = apply_finish_rule(raw, P, eos, PAD, free.token_logprobs[:, 0].cpu().numpy())
    outs = {}
    for poll in (8, 1, 0):
        out = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, pad_token_id=PAD, poll_every=poll, **GREEDY)
        replays = m._captioner.last_replays
        check_shapes(out, 4, 1, P)
        assert np.array_equal(out.ids[:, 0].cpu().numpy(), want_ids) and np.array_equal(out.lengths[:, 0].cpu().numpy(), want_len)
        assert np.array_equal(out.token_logprobs[:, 0].cpu().numpy(), want_lp)          # the EOS keeps its log-prob; 0.0 after it
        assert replays == T if poll == 0 else replays <= int(want_len.max()) - P + poll
        outs[poll] = out
    check_logprobs(m, images, outs[8], P, 'tiny eos')
    # one image: the row ends within four steps, and the loop with it
    out = m.generate_captions(images[:1], prompt[:1], max_new_tokens=T, eos_token_id=eos, poll_every=2, **GREEDY)
    assert int(out.lengths[0, 0]) <= P + 4 and out.ids.shape[-1] == int(out.lengths[0, 0]) and int(out.ids[0, 0, -1]) == eos
    assert m._captioner.last_replays <= int(out.lengths[0, 0]) - P + 2 < T
    # the default pad is the EOS id; an EOS inside the prompt finishes nothing
    out = m.generate_captions(images, torch.full_like(prompt, eos), max_new_tokens=6, eos_token_id=eos, **GREEDY)
    assert bool((out.lengths > P).all())
    tail = torch.arange(out.ids.shape[-1], device=dev())[None, :] >= out.lengths[:, 0, None]
    assert bool((out.ids[:, 0][tail] == eos).all())


def test_sampled_rows_with_eos_and_rerank(tiny_weights):
    from image2text_amd.models.generation_utils import rerank
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(2, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :1].clamp(min=0).to(dev())
    B, N, P, T = 2, 4, 1, 16
    SAMPLING = dict(temperature=1.5, top_k=20, nucleus_p=None)          # a wide draw: the rows of an image differ
    free = m.generate_captions(images, prompt, max_new_tokens=T, num_return_sequences=N, seed=7, **SAMPLING)
    raw = free.ids.reshape(B * N, -1).cpu().numpy()
    eos = int(np.bincount(raw[:, P:].ravel()).argmax())       # the token the free run emits most often
    want_ids, want_len, want_lp = apply_finish_rule(raw, P, eos, None, free.token_logprobs.reshape(B * N, -1).cpu().numpy())
    out = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, num_return_sequences=N, seed=7, **SAMPLING)
    check_shapes(out, B, N, P)
    # the draw of a step is a function of (seed, step, row): the rows are those of the free run up to their first EOS
    assert np.array_equal(out.ids.reshape(B * N, -1).cpu().numpy(), want_ids)
    assert np.array_equal(out.lengths.reshape(-1).cpu().numpy(), want_len)
    assert np.array_equal(out.token_logprobs.reshape(B * N, -1).cpu().numpy(), want_lp)
    print(f'lengths of the {B * N} sampled rows: {want_len.tolist()}')
    check_logprobs(m, images, out, P, 'tiny N=4 eos')
    order, lp = rerank(m, images, out.ids, eos)
    assert tuple(order.shape) == (B, N) and torch.equal(order.sort(dim=1).values, torch.arange(N, device=dev()).expand(B, N))


def test_n_captions_hold_one_cross_kv_per_image(tiny_weights):
    """N = 4: the allocator's peak rise stays below that of generate() on 4x repeated images, less three copies of the cross K/V"""
    B, N, T = 16, 4, 8
    images, labels = synthetic_batch(B, 32, 12, 384, seed=3)
    images, prompt = images.to(dev()), labels[:, :1].clamp(min=0).to(dev())
    rise = {}
    for form in ('captions', 'repeated'):
        m = _ved(tiny_config(), tiny_weights)
        m._engine.prepare(False)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if form == 'captions':
            out = m.generate_captions(images, prompt, max_new_tokens=T, num_return_sequences=N, seed=1, **SAMPLING)
            assert tuple(out.ids.shape) == (B, N, 1 + T)
        else:
            out = m.generate(images.repeat_interleave(N, dim=0), prompt.repeat_interleave(N, dim=0), max_new_tokens=T, **SAMPLING)
        torch.cuda.synchronize()
        rise[form] = torch.cuda.max_memory_allocated() - base
        dc, S = m._engine.dec, m._engine.enc.ncls
        n_cross = len(m._greedy._cross_layers()) if form == 'repeated' else len(m._captioner._cross_layers())
        kv = B * S * 2 * dc.d * 2 * n_cross                   # bf16 K | V of every cross layer, one copy
        del m, out
    print(f'peak rise: N = 4 captions {rise["captions"] / 2 ** 20:.2f} MiB, 4x repeated images {rise["repeated"] / 2 ** 20:.2f} MiB, '
          f'one cross K/V copy {kv / 2 ** 20:.3f} MiB')
    assert n_cross > 0 and rise['captions'] < rise['repeated'] - 3 * kv


def test_refusals(tiny_weights):
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(2, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :2].clamp(min=0).to(dev())
    with pytest.raises(ValueError, match='identical'):
        m.generate_captions(images, prompt, max_new_tokens=4, num_return_sequences=2, **GREEDY)
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match='text window'):
        m.generate_captions(images, prompt, max_new_tokens=window - 1, **GREEDY)
    out = m.generate_captions(images, prompt, max_new_tokens=window - 2, **GREEDY)          # the whole window is fine
    assert out.ids.shape[-1] == window
    ms = _ved(mini_config(use_soft_prompting=False), sharpen=True)                          # sparse blocks without >= 2 kept prompt positions
    with pytest.raises(NotImplementedError, match='kept positions'):
        ms.generate_captions(images, prompt, max_new_tokens=4, **GREEDY)


@pytest.mark.parametrize('mode', ['plain', 'ragged', 'beams'])
def test_model_call_and_decoder_shim_run_one_plan(tiny_weights, mode):
    """``m.generate_captions`` and the decoder's keyword ``generate_captions`` resolve equal arguments into equal plans: the second call
    returns the first one's result bit for bit, on the same state, and captures nothing"""
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(2, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :3].clamp(min=0).to(dev())
    T, eos = 4, 5
    if mode == 'beams':
        out = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, num_beams=2)
        dec = m._beam_captioner
        call = lambda: dec.generate_captions(images, prompt, T, 2, eos)
    else:
        plen = [2, 3] if mode == 'ragged' else None
        out = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, prompt_lengths=plen, **GREEDY)
        dec = m._captioner
        call = lambda: dec.generate_captions(images, prompt, T, eos, None, 1, None, prompt_lengths=plen)
    st, keys = dec._state, set(dec._state.graphs)
    again = call()
    assert dec._state is st and set(st.graphs) == keys
    for name in ('ids', 'lengths', 'token_logprobs'):
        assert torch.equal(getattr(again, name), getattr(out, name)), name
    if mode == 'beams':
        assert torch.equal(again.beam_scores, out.beam_scores)
    else:
        assert again.beam_scores is None and out.beam_scores is None
