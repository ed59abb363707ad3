"""generate_captions(top_logprobs=K) end to end on the MI355X: the dense tiny decoder (d = 128: K > 0 takes it off the
segment-maxima head), its d = 64 one-head twin (the fp32-logits head anyway), the sparse nano-mini family and the tiny Llama of
tests/test_hf_decoder_gpu.py, built as tests/test_image_index_gpu.py builds them; B = 3 images, N in {1, 2}, at most 6 new tokens, K = 5.

The reference of every step is the numpy statement decoding_host.top_logprobs_host on the DEVICE's own logits row, copied by the
``each`` hook after the step (plain greedy and plain sampled calls: their choosers do not write the row): tokens exactly, log-probs and
entropy within the bounds of tests/test_top_logprobs_kernel_gpu.py (lse_bound / entropy_bound, derived there).  Where the emitted
token is in the list, its entry and ``token_logprobs`` agree within the sum of the two kernels' bounds: the chooser's lse goes through
a reduction of another shape -- up to 1024 threads and 16 waves --, held here to the same form with n_m = ceil(V / 256) + 1 + 6 + 16
merges, which is no fewer than any chooser takes.  Everything else is bit equality: the kernel only reads, so a call with the argument
on a decoder or mode that takes the fp32-logits head anyway returns the ids, lengths and log-probs of the call without it; a replayed
graph is the eager step; a call under ``image_index`` is the call on the gathered images."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding_host import top_logprobs_host
from image2text_amd.synth import synthetic_batch, tiny_config
from test_image_index_gpu import _model, _ved, bits, dev
from test_top_logprobs_kernel_gpu import U, entropy_bound, lse_bound

pytestmark = pytest.mark.gpu

F32 = torch.float32
B, T, K, EOS = 3, 5, 5, 3
GREEDY = dict(top_k=1)
SAMPLED = dict(temperature=1.2, top_k=30, seed=5, num_return_sequences=2)
FIELDS = ('ids', 'lengths', 'token_logprobs', 'logprob', 'phrase_index', 'prompt_lengths')
TOP = ('top_tokens', 'top_logprobs', 'token_entropy')
SET_A = [[7, 8], [7, 9, 10], [11], [12, 13]]
SET_B = [[20], [21, 22], [21, 23]]


@pytest.fixture(params=['tiny', 'dense64', 'mini', 'hf_llama'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    m, images, prompt = _model(request.param, tiny_weights, tmp_path, monkeypatch)
    return request.param, m, images[:B], prompt[:B]


def same(got, want, fields, what):
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), f'{what}: {f}'
        assert g is None or (g.shape == w.shape and torch.equal(bits(g), bits(w))), f'{what}: {f} differs'


def shaped(out, N, K=K):
    cols = out.token_logprobs.shape[2]
    assert out.top_tokens.dtype == torch.int32 and out.top_logprobs.dtype == F32 and out.token_entropy.dtype == F32
    assert tuple(out.top_tokens.shape) == tuple(out.top_logprobs.shape) == (out.ids.shape[0], N, cols, K)
    assert tuple(out.token_entropy.shape) == (out.ids.shape[0], N, cols)


def recorded_call(m, images, prompt, K, use_graph=True, eos=None, **kw):
    """a call through the decoder that keeps, per full step, the device's raw logits rows and which rows had finished before it"""
    from image2text_amd.decoding import Sampling
    if m._captioner is None:
        m.generate_captions(images, prompt, max_new_tokens=1, top_k=1)                      # (makes the captioner)
    cap, V = m._captioner, m._engine.dec.V
    steps, before = [], [None]

    def each(i):
        st = cap._state
        was = torch.zeros_like(st.finished) if before[0] is None else before[0]
        steps.append((st.logits[:, :V].cpu().numpy().copy(), was.cpu().numpy().astype(bool)))
        before[0] = st.finished.clone()
    N = kw.get('num_return_sequences', 1)
    sampling = None if kw.get('top_k') == 1 else Sampling(kw['temperature'], kw['top_k'], None, kw['seed'])
    out = cap.generate_captions(images, prompt, T, eos, None, N, sampling, poll_every=0, use_graph=use_graph, top_logprobs=K, each=each)
    return out, steps, N


def held_to_the_replica(out, steps, N, P, K, what):
    """every step's column against the replica on that step's device logits -> the worst error / bound of the floats"""
    shaped(out, N, K)
    V = steps[0][0].shape[1]
    worst = 0.0
    chosen_n_m = (V + 255) // 256 + 1 + 6 + 16
    for i, (z, was_finished) in enumerate(steps[:out.token_logprobs.shape[2]]):
        tok = out.top_tokens[:, :, i].reshape(-1, K).cpu().numpy()
        lp = out.top_logprobs[:, :, i].reshape(-1, K).cpu().numpy().astype(np.float64)
        ent = out.token_entropy[:, :, i].reshape(-1).cpu().numpy().astype(np.float64)
        emitted = out.ids[:, :, P + i].reshape(-1).cpu().numpy()
        tlp = out.token_logprobs[:, :, i].reshape(-1).cpu().numpy().astype(np.float64)
        rtok, rlp, rent = top_logprobs_host(z, K)
        z64 = torch.from_numpy(z).double()
        _, dL = lse_bound(z64, V)
        _, hb = entropy_bound(z64, V, dL)
        _, dL_chooser = lse_bound(z64, V, chosen_n_m)
        for r in range(z.shape[0]):
            if was_finished[r]:
                assert (tok[r] == -1).all() and (lp[r] == 0).all() and ent[r] == 0, f'{what}: step {i} row {r}: a finished row was written'
                continue
            assert np.array_equal(tok[r], rtok[r]), f'{what}: step {i} row {r}: tokens {tok[r]} vs the replica {rtok[r]}'
            b = float(dL[r]) + U * np.abs(rlp[r])
            assert (np.abs(lp[r] - rlp[r]) <= b).all() and abs(ent[r] - rent[r]) <= float(hb[r]), f'{what}: step {i} row {r}'
            worst = max(worst, float((np.abs(lp[r] - rlp[r]) / b).max()), abs(ent[r] - rent[r]) / float(hb[r]))
            at = np.flatnonzero(tok[r] == emitted[r])
            if at.size:                                             # the two kernels' statements of one quantity
                both = float(dL[r]) + float(dL_chooser[r]) + 2 * U * abs(rlp[r, at[0]])
                assert abs(lp[r, at[0]] - tlp[r]) <= both, f'{what}: step {i} row {r}: {lp[r, at[0]]} in the list, token_logprobs {tlp[r]}'
    return worst


def test_every_step_is_the_replica_on_the_device_logits(model):
    name, m, images, prompt = model
    P = prompt.shape[1]
    for mode in (GREEDY, SAMPLED):
        out, steps, N = recorded_call(m, images, prompt, K, **mode)
        assert len(steps) == T and out.ids.shape[2] == P + T
        worst = held_to_the_replica(out, steps, N, P, K, f'{name} {sorted(mode)}')
        print(f'{name} N = {N}: worst error / bound over top_logprobs and token_entropy {worst:.3g}')
        assert bool((out.token_entropy > 0).all()) and bool((out.top_logprobs[..., :-1] >= out.top_logprobs[..., 1:]).all())
        # the kernel only reads: where the head is the fp32-logits one anyway, the call is the call without the argument
        if name == 'dense64' or mode is SAMPLED:
            same(out, m.generate_captions(images, prompt, max_new_tokens=T, **mode), FIELDS, f'{name}: with and without the argument')
        eager, _, _ = recorded_call(m, images, prompt, K, use_graph=False, **mode)
        same(eager, out, FIELDS + TOP, f'{name}: graph replay against the eager steps')
    plain = m.generate_captions(images, prompt, max_new_tokens=T, **GREEDY)
    assert plain.top_tokens is None and plain.top_logprobs is None and plain.token_entropy is None


def test_without_a_ban_the_first_entry_is_the_emitted_token():
    m = _ved(tiny_config(dec_d=64, dec_heads=1, no_repeat_n_grams=()))
    images, labels = synthetic_batch(B, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :3].clamp(min=0).to(dev())
    out = m.generate_captions(images, prompt, max_new_tokens=T, top_k=1, top_logprobs=K)
    assert torch.equal(out.top_tokens[..., 0].long(), out.ids[:, :, 3:])


def test_a_smaller_then_a_larger_k(model):
    name, m, images, prompt = model
    P = prompt.shape[1]
    outs = {}
    for k in (3, 8, 3):
        out, steps, N = recorded_call(m, images, prompt, k, **GREEDY)
        held_to_the_replica(out, steps, N, P, k, f'{name} K = {k}')
        st = m._captioner._state
        assert st.top_tok.shape[2] == max([k] + list(outs)) and any(key[-2:] == ('top_logprobs', k) for key in st.graphs if isinstance(key, tuple))
        if k in outs:
            same(out, outs[k], FIELDS + TOP, f'{name}: K = {k} again, on the larger buffers')
        outs[k] = out
    assert torch.equal(outs[3].top_tokens, outs[8].top_tokens[..., :3]) and torch.equal(bits(outs[3].token_entropy), bits(outs[8].token_entropy))


def test_fill_values_at_forced_columns_and_past_the_eos(model):
    name, m, images, prompt = model
    plen = [1, 3, 2]
    free = m.generate_captions(images, prompt, max_new_tokens=T, prompt_lengths=plen, **GREEDY)
    eos = int(free.ids[0, 0, plen[0] + 1])                           # row 0 emits it as its second token (or earlier)
    kw = dict(max_new_tokens=T, prompt_lengths=plen, eos_token_id=eos, **GREEDY)
    out = m.generate_captions(images, prompt, top_logprobs=K, **kw)
    shaped(out, 1)
    pmin, L = min(plen), out.ids.shape[2]
    assert int(out.lengths[0, 0]) <= plen[0] + 2 < L
    if name == 'dense64':
        same(out, m.generate_captions(images, prompt, **kw), FIELDS, name)
    for b in range(B):
        end = int(out.lengths[b, 0])
        for col in range(pmin, L):
            cell = (out.top_tokens[b, 0, col - pmin], out.top_logprobs[b, 0, col - pmin], out.token_entropy[b, 0, col - pmin])
            if col < plen[b] or col >= end:
                assert bool((cell[0] == -1).all()) and bool((cell[1] == 0).all()) and float(cell[2]) == 0.0, f'{name}: row {b} column {col}'
                assert float(out.token_logprobs[b, 0, col - pmin]) == 0.0
            else:                                                   # written, the column of the EOS included
                assert bool((cell[0] >= 0).all()) and bool((cell[1] < 0).all()) and float(cell[2]) > 0.0, f'{name}: row {b} column {col}'
    assert int(out.ids[0, 0, int(out.lengths[0, 0]) - 1]) == eos


def test_the_results_describe_the_raw_row(model):
    name, m, images, prompt = model
    P = prompt.shape[1]
    plain = m.generate_captions(images, prompt, max_new_tokens=T, top_logprobs=K, **GREEDY)
    first = lambda out: [getattr(out, f)[:, :, 0] for f in TOP]
    # a suppressed token is not emitted, and still leads the list: the first step's raw row is the plain call's
    t0 = plain.top_tokens[:, 0, 0, 0]
    sup = m.generate_captions(images, prompt, max_new_tokens=T, top_logprobs=K, suppress_tokens=t0.tolist(), repetition_penalty=1.3, **GREEDY)
    assert not bool((sup.ids[:, 0, P] == t0).any())
    for g, w in zip(first(sup), first(plain)):
        assert torch.equal(bits(g), bits(w)), f'{name}: the processors entered the first step\'s results'
    same(sup, m.generate_captions(images, prompt, max_new_tokens=T, suppress_tokens=t0.tolist(), repetition_penalty=1.3, **GREEDY), FIELDS,
         f'{name}: processors with and without the argument')
    # phrase_sets: the alternatives are the unconstrained model's
    kw = dict(max_new_tokens=T, eos_token_id=EOS, phrase_sets=[SET_A, SET_B], phrase_set_index=[0, 1, 0], **GREEDY)
    sets = m.generate_captions(images, prompt, top_logprobs=K, **kw)
    same(sets, m.generate_captions(images, prompt, **kw), FIELDS, f'{name}: phrase_sets with and without the argument')
    for g, w in zip(first(sets), first(plain)):
        assert torch.equal(bits(g), bits(w)), f'{name}: the trie mask entered the first step\'s results'
    allowed = {t for s in (SET_A, SET_B) for ph in s for t in ph} | {EOS}
    assert any(t not in allowed for t in sets.top_tokens[:, 0, 0].reshape(-1).tolist()), f'{name}: the list holds phrase tokens only'
    assert bool(torch.isfinite(sets.top_logprobs[sets.top_tokens >= 0]).all()), 'no masked (-inf) value reached the list'
    if name != 'mini':                                               # (the nano-mini family refuses the one-pass prefill)
        passed = m.generate_captions(images, prompt, max_new_tokens=T, top_logprobs=K, prompt_prefill='pass', **GREEDY)
        shaped(passed, 1)
        ref = m.generate_captions(images, prompt, max_new_tokens=T, prompt_prefill='pass', **SAMPLED)
        same(m.generate_captions(images, prompt, max_new_tokens=T, top_logprobs=K, prompt_prefill='pass', **SAMPLED), ref, FIELDS,
             f"{name}: prompt_prefill='pass' with and without the argument")
        assert bool((passed.top_tokens >= 0).all()) and bool((passed.token_entropy > 0).all())


def test_image_index_gives_per_query_results(model):
    name, m, images, prompt = model
    index = [0, 0, 1]
    assert not torch.equal(prompt[0], prompt[1])
    kw = dict(max_new_tokens=T, top_logprobs=K, **GREEDY)
    got = m.generate_captions(images, prompt, image_index=index, **kw)         # (three images in both calls: the encoder's launch shapes)
    shaped(got, 1)
    same(got, m.generate_captions(images[index], prompt, **kw), FIELDS + TOP, f'{name}: image_index against the gathered images')
    assert got.image_index.tolist() == index and not torch.equal(got.top_tokens[0], got.top_tokens[1])


def test_the_model_refuses():
    from image2text_amd.synth import reference_unit_test_config
    m = _ved(tiny_config(dec_d=64, dec_heads=1))
    images, labels = synthetic_batch(B, 32, 12, 384, seed=11)
    images, prompt = images.to(dev()), labels[:, :3].clamp(min=0).to(dev())
    with pytest.raises(ValueError, match='top_logprobs = 9: from 0'):
        m.generate_captions(images, prompt, max_new_tokens=T, top_k=1, top_logprobs=9)
    with pytest.raises(ValueError, match='top_logprobs = 2.0: a whole number'):
        m.generate_captions(images, prompt, max_new_tokens=T, top_k=1, top_logprobs=2.0)
    with pytest.raises(NotImplementedError, match='top_logprobs under num_beams > 1'):
        m.generate_captions(images, prompt, max_new_tokens=T, num_beams=2, top_logprobs=2)
    assert m._captioner is None and m._beam_captioner is None, 'a refused call made a decoder'
    nc = _ved(reference_unit_test_config(), sharpen=True)
    assert not nc._engine.dec.causal
    images, labels = synthetic_batch(2, 128, 12, 1024, seed=9)
    with pytest.raises(NotImplementedError, match='top_logprobs runs inside the KV-cache caption step'):
        nc.generate_captions(images.to(dev()), labels[:2, :2].clamp(min=0).to(dev()), max_new_tokens=2, top_k=1, top_logprobs=2)
