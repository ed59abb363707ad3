"""generate_captions(repetition_penalty=, min_new_tokens=, suppress_tokens=) on the MI355X, end to end.

Models at fixture size: tiny (trained weights, d = 128: inactive calls take the segment-maxima head, active ones the fp32-logits head),
a decoder of width 64 (the fp32-logits head either way) and a Hugging Face GPT-2 decoder with a soft prompt; B = 3, P = 3, 8 new tokens.

Bars, all existing ones: token_logprobs within 4 . logits_tol of fp64 log_softmax of the model's own forward at the generated ids and of
score() (tests/test_generate_captions_gpu.py states why) -- here the check that the RAW definition survived the processed row; greedy
ids under the margin rule of DESIGN.md 4q: a token may differ from the teacher-forced expectation only where the top-2 margin of the
expectation's (processed, banned) row is below 2 . logits_tol."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import process_logits_host
from image2text_amd.synth import reference_unit_test_config, synthetic_batch, tiny_config
from oracle import reference_model as orc
from test_generate_captions_gpu import GREEDY, _ved, check_shapes
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

B, P, T = 3, 3, 8
SAMPLING = dict(temperature=1.2, top_k=30, nucleus_p=None)
PLEN = [1, 3, 2]


def dev():
    return torch.device('cuda:0')


@pytest.fixture(params=['tiny', 'dense64', 'hf_gpt2_soft'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    """-> (name, model, images [3, ...], prompt [3, 3])"""
    name = request.param
    V = 384
    if name == 'tiny':
        m = _ved(tiny_config(), tiny_weights)
        assert m._engine.dec.d % 128 == 0
    elif name == 'dense64':
        m = _ved(tiny_config(dec_d=64, dec_heads=1))
        assert m._engine.dec.d % 128 != 0
    else:
        from test_hf_decoder_gpu import _build
        _, m = _build(tmp_path, monkeypatch, True, True)
        m = m.to(dev()).eval()
        assert m._engine.dec.prefixed
        V = m._engine.dec.V
    images, labels = synthetic_batch(B, 32, 12, min(V, 384), seed=7)
    return name, m, images.to(dev()), labels[:, :P].clamp(min=0).to(dev())


def same(a, b):
    return (torch.equal(a.ids, b.ids) and torch.equal(a.lengths, b.lengths)
            and torch.equal(a.token_logprobs.view(torch.int32), b.token_logprobs.view(torch.int32)))


def forward_logits(m, images, out):
    Bn, N, L = out.ids.shape
    rep = images.repeat_interleave(N, dim=0)
    ids = out.ids.reshape(Bn * N, L)
    with torch.no_grad():
        return rep, ids, m(images=rep, ids=ids).logits.float()


def check_raw_logprobs(m, images, out, plen, tag):
    """token_logprobs at every emitted position (column >= the row's prompt length, < its length) against fp64 log_softmax of the
    model's own forward at the generated ids and against score(): 4 . logits_tol; exact zeros elsewhere"""
    Bn, N, L = out.ids.shape
    pmin = min(plen)
    rep, ids, logits = forward_logits(m, images, out)
    bar = 4 * logits_tol(logits.cpu().numpy())
    ref = torch.log_softmax(logits.double(), dim=-1)[:, pmin - 1:L - 1].gather(-1, ids[:, pmin:, None])[..., 0]
    col = torch.arange(pmin, L, device=dev())[None, :]
    p_rows = torch.tensor(plen, device=dev()).repeat_interleave(N)[:, None]
    live = (col >= p_rows) & (col < out.lengths.reshape(Bn * N, 1))
    got = out.token_logprobs.reshape(Bn * N, L - pmin)
    err = float(((got.double() - ref).abs() * live).max())
    sc = m.score(rep, ids).token_logprobs[:, pmin - 1:L - 1]
    err_sc = float(((got - sc).abs() * live).max())
    print(f'{tag}: raw token_logprobs worst error / bar vs forward {err / bar:.3g}, vs score {err_sc / bar:.3g} (bar {bar:.3g})')
    assert bool(live.any()) and torch.isfinite(got).all() and err <= bar and err_sc <= bar, f'{tag}: {err:.3g} / {err_sc:.3g} over {bar:.3g}'
    assert bool((got[~live] == 0).all())


def expected_rows(m, images, out, theta, suppress=(), eos=None, min_new=0):
    """teacher forcing: the forward's fp32 logits at the generated ids of a greedy N = 1 run through process_logits_host and the n-gram
    ban -> (processed rows [B, L - P, V], logits_tol of the forward)"""
    _, ids, logits = forward_logits(m, images, out)
    V = m._engine.dec.V
    L = ids.shape[1]
    ids_c, z = ids.cpu(), logits[..., :V].cpu()
    rows = torch.empty(ids.shape[0], L - P, V)
    for t in range(P, L):
        step = torch.stack([torch.from_numpy(process_logits_host(z[b, t - 1].numpy(), ids_c[b].numpy(), t, t - P, theta, suppress, eos, min_new))
                            for b in range(ids.shape[0])])
        rows[:, t - P] = orc.apply_ngram_ban(ids_c[:, :t], step, m.config.no_repeat_n_grams)
    return rows, logits_tol(logits.cpu().numpy())


def test_defaults_are_the_present_call(model):
    """defaults and suppress_tokens=[] are bit-equal to the call without the arguments, with equal replays and no 'proc' graph key; an
    active call in between changes nothing of a later inactive one"""
    name, m, images, prompt = model
    modes = (GREEDY, dict(seed=5, num_return_sequences=2, **SAMPLING))
    alone = []
    for mode in modes:
        old = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=7, **mode)
        alone.append(old)
        replays = m._captioner.last_replays
        for kw in (dict(repetition_penalty=1.0, min_new_tokens=0, suppress_tokens=None), dict(suppress_tokens=[]), dict(min_new_tokens=0)):
            new = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=7, **mode, **kw)
            assert same(old, new) and m._captioner.last_replays == replays, f'{name}: {kw}'
        st = m._captioner._state
        assert st.raw_lse is None and st.saved is None and st.suppress is None, 'an inactive call made a processor buffer'
        assert not any(isinstance(k, tuple) and k and k[0] == 'proc' for k in st.graphs), list(st.graphs)
    m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=7, repetition_penalty=1.4, suppress_tokens=[3], **GREEDY)
    assert any(isinstance(k, tuple) and k[0] == 'proc' for k in m._captioner._state.graphs)
    m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=7, min_new_tokens=3, seed=5, num_return_sequences=2, **SAMPLING)
    for mode, before in zip(modes, alone):                   # the same state has run processed steps meanwhile
        after = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=7, **mode)
        assert same(before, after), f'{name}: an inactive call after an active one differs from the inactive call alone'


@pytest.mark.parametrize('mode', ['greedy', 'sampling'])
def test_suppress_tokens(model, mode):
    """the free run's three most frequent emitted tokens, suppressed: none of them appears after the prompt; raw log-probs"""
    name, m, images, prompt = model
    kw = GREEDY if mode == 'greedy' else dict(seed=9, num_return_sequences=2, **SAMPLING)
    N = kw.get('num_return_sequences', 1)
    free = m.generate_captions(images, prompt, max_new_tokens=T, **kw)
    emitted = free.ids[..., P:].reshape(-1).cpu().numpy()
    top3 = [int(t) for t in np.argsort(-np.bincount(emitted), kind='stable')[:3]]
    out = m.generate_captions(images, prompt, max_new_tokens=T, suppress_tokens=top3 + top3[:1], **kw)
    check_shapes(out, B, N, P)
    assert bool((out.ids[..., :P] == prompt[:, None]).all())
    assert not np.isin(out.ids[..., P:].cpu().numpy(), top3).any(), f'{name} {mode}: a suppressed token was emitted'
    assert not torch.equal(out.ids, free.ids)
    check_raw_logprobs(m, images, out, [P] * B, f'{name} suppress {mode}')
    if mode == 'greedy':                                    # use_graph=False equals the graph run
        eager = m._captioner.generate_captions(images, prompt, T, None, None, 1, None, use_graph=False, suppress_tokens=top3)
        assert same(out, eager)


def test_min_new_tokens(model):
    """an EOS id at which some free row stops before its 5th token: with min_new_tokens = 5 no EOS before the 5th emitted token,
    lengths >= p_b + 5; the count is per row under prompt_lengths"""
    name, m, images, prompt = model
    free = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    eos = int(free.ids[0, 0, P + 1])                          # row 0 would stop at its second token at the latest
    short = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, **GREEDY)
    assert int(short.lengths.min()) <= P + 2
    out = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, min_new_tokens=5, **GREEDY)
    check_shapes(out, B, 1, P)
    assert bool((out.lengths >= P + 5).all()) and not bool((out.ids[:, 0, P:P + 4] == eos).any())
    check_raw_logprobs(m, images, out, [P] * B, f'{name} min_new')
    rag = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, min_new_tokens=5, prompt_lengths=PLEN, **GREEDY)
    ids = rag.ids[:, 0].cpu().numpy()
    for b, p in enumerate(PLEN):
        assert int(rag.lengths[b, 0]) >= p + 5 and eos not in ids[b, p:p + 4].tolist(), f'{name}: row {b} (prompt {p}) ended early'
        assert ids[b, :p].tolist() == prompt[b, :p].tolist()
    check_raw_logprobs(m, images, rag, PLEN, f'{name} min_new ragged')
    # sampling, N = 2: a row that would draw EOS first is not an empty caption
    smp = m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, min_new_tokens=5, seed=2, num_return_sequences=2, **SAMPLING)
    assert bool((smp.lengths >= P + 5).all()) and not bool((smp.ids[..., P:P + 4] == eos).any())
    check_raw_logprobs(m, images, smp, [P] * B, f'{name} min_new sampling')


def test_repetition_penalty_teacher_forced(tiny_weights):
    """tiny, greedy, theta = 1.5, images of seed 7 (the free run repeats a token there, and the penalised run differs from it): the
    argmax of the teacher-forced processed rows is the emitted token wherever their top-2 margin is >= 2 . logits_tol, and at most a
    quarter of the (row, column) cells may be excused by the margin.  The CPU oracle alone (oracle/reference_model.forward through
    process_logits_host and the ban, same weights and images) excuses 1 of 24 cells (4 %) at theta = 1.5 and 2 of 24 at theta = 1."""
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(B, 32, 12, 384, seed=7)
    images, prompt = images.to(dev()), labels[:, :P].clamp(min=0).to(dev())
    free = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    fr = free.ids[:, 0].cpu().numpy()
    assert any(len(set(r[P:].tolist())) < T or set(r[P:].tolist()) & set(r[:P].tolist()) for r in fr), 'the free run repeats no token'
    out = m.generate_captions(images, prompt, max_new_tokens=T, repetition_penalty=1.5, **GREEDY)
    check_shapes(out, B, 1, P)
    assert not torch.equal(out.ids, free.ids), 'the penalty changed no token'
    rows, tol = expected_rows(m, images, out, 1.5)
    t2 = torch.topk(rows, 2, dim=-1).values
    margin = t2[..., 0] - t2[..., 1]
    agree = rows.argmax(dim=-1) == out.ids[:, 0, P:].cpu()
    excused = margin < 2 * tol
    print(f'theta 1.5: {int(excused.sum())} of {excused.numel()} cells excused by the margin (2 logits_tol = {2 * tol:.3g}), '
          f'{int((~agree).sum())} cells differ')
    assert bool((agree | excused).all()), 'an emitted token differs from the processed argmax at a decided column'
    assert int(excused.sum()) * 4 <= excused.numel()
    check_raw_logprobs(m, images, out, [P] * B, 'tiny theta 1.5')
    eager = m._captioner.generate_captions(images, prompt, T, None, None, 1, None, use_graph=False, repetition_penalty=1.5)
    assert same(out, eager)


def test_all_three_with_prefill_pass(model):
    """every processor at once; prompt_prefill='pass' agrees with 'steps' under the margin rule: a row leaves the 'steps' run only at a
    column whose processed top-2 margin there is below 2 . logits_tol"""
    name, m, images, prompt = model
    free = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    eos = int(free.ids[1, 0, P + 2])
    sup = [int(free.ids[0, 0, P]), int(free.ids[2, 0, P + 1])]
    kw = dict(max_new_tokens=T, eos_token_id=eos, repetition_penalty=1.3, min_new_tokens=4, suppress_tokens=sup, **GREEDY)
    steps = m.generate_captions(images, prompt, prompt_prefill='steps', **kw)
    check_raw_logprobs(m, images, steps, [P] * B, f'{name} all three')
    ids = steps.ids[:, 0]
    assert not np.isin(ids[:, P:].cpu().numpy(), [s for s in sup if s != eos]).any() and bool((steps.lengths >= P + 4).all())
    got = m.generate_captions(images, prompt, prompt_prefill='pass', **kw)
    check_raw_logprobs(m, images, got, [P] * B, f'{name} all three, pass')
    rows, tol = expected_rows(m, images, steps, 1.3, sup, eos, 4)
    t2 = torch.topk(rows, 2, dim=-1).values
    margin = t2[..., 0] - t2[..., 1]
    Lc = min(ids.shape[1], got.ids.shape[-1])
    for b in range(B):
        live = min(int(steps.lengths[b, 0]), int(got.lengths[b, 0]), Lc)
        diff = (ids[b, :live] != got.ids[b, 0, :live]).nonzero().flatten()
        if diff.numel() == 0:
            continue
        c = int(diff[0])
        print(f'{name} row {b}: pass leaves steps at column {c}, processed margin {float(margin[b, c - P]):.3g} (2 logits_tol = {2 * tol:.3g})')
        assert c >= P and float(margin[b, c - P]) < 2 * tol


def test_non_causal_decoder_refuses_active_processors():
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(reference_unit_test_config()).to(dev()).eval()
    images, prompt = torch.zeros(2, 3, 128, 128, device=dev()), torch.zeros(2, 1, dtype=torch.long, device=dev())
    with pytest.raises(NotImplementedError, match='non-causal decoder'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match='non-causal decoder'):
        m.generate_captions(images, prompt, max_new_tokens=4, top_k=1, suppress_tokens=[5])
