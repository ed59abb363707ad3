"""score(..., top_logprobs=K) end to end on the MI355X, on the four tiny decoders of tests/test_top_logprobs_gpu.py: the
dense d = 128 one (K > 0 takes it off the segment-statistics head), its d = 64 one-head twin, the sparse nano-mini family and the tiny
Llama; B = 3 captions of 6 tokens, K = 5, temperature in {1.0, 0.7}, default labels and explicit ones with ignored positions.

The device's own fp32 rows, copied through ``HotPath.token_top_logprobs``' ``each`` hook, go into the numpy statement
``decoding_host.score_top_logprobs_host``: tokens and rank exactly, log-probs, lse and entropy within lse_bound / entropy_bound of
tests/test_top_logprobs_kernel_gpu.py applied to v = fp32(row) * fp32(1 / temperature), as tests/test_score_top_logprobs_kernel_gpu.py
applies them.  A call whose SCORE_WS_BYTES holds 5 rows walks the 18 rows in four chunks and is bit-equal, field by field, to the
one-chunk call.  score(top_logprobs=0) is score() without the argument, bit for bit.

``token_logprobs`` and ``lse`` of the K > 0 call against fp64 log_softmax(forward(...).logits / T): the bound form of
tests/test_score_gpu.py::score_bound, restated (``top_score_bound``) for this path.  Per position, u = 2^-24, d the decoder width, h / w
the bf16 hidden row and head rows, z = forward's fp32 logits, it = 1 / T:
  * no bf16 logits exist on this path, so score_bound's 2^-8 term is absent;
  * the chunk's GEMM re-accumulates the logits in fp32, possibly in another order than forward's GEMM: d u sum_k |h| |w| per logit on each
    side -- 2 it d u S_t on the target and, through the logsumexp (1-Lipschitz in the largest change of a logit), 2 it d u max_c S_c;
  * the scale is fp32(1 / T), off by a relative u, and the product z * scale rounds once more: 2 u it |z| per column, on the target and
    on the row's largest column;
  * the row-form sum: score_bound's sum-and-log terms -- the rounded exponents (3 spread u), three roundings per merge, one addition per
    merge and up to V additions, one log, the final roundings -- with THIS kernel's merge count n_m = ceil(V / 256) + 1 + 6 + 4 (a
    thread's chain over its columns of 256-column strides, the first value, the 6-step xor tree, the 4 waves in order: the count
    tests/test_top_logprobs_kernel_gpu.py derives for the same reduction) in place of the segment form's 2 + ceil(nseg / 64) + 6;
  * the final subtraction and the reference's own gather: 2 u it |z_t|, as there."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding_host import score_top_logprobs_host
from image2text_amd.models.vision_encoder_decoder import next_token_labels
from image2text_amd.synth import synthetic_batch
from test_image_index_gpu import _model, bits, dev
from test_score_gpu import reference_logprobs
from test_top_logprobs_kernel_gpu import U, entropy_bound, lse_bound

pytestmark = pytest.mark.gpu

F32, I32, BF16 = torch.float32, torch.int32, torch.bfloat16
B, L, K = 3, 6, 5
IGNORE = -100
TUPLE = ('token_logprobs', 'lse', 'logprob')
TOP = ('top_tokens', 'top_logprobs', 'token_entropy', 'label_rank')


@pytest.fixture(params=['tiny', 'dense64', 'mini', 'hf_llama'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    m, images, _ = _model(request.param, tiny_weights, tmp_path, monkeypatch)
    _, labels = synthetic_batch(B, 32, 12, min(m._engine.dec.V, 384), seed=23)
    return request.param, m, images[:B], labels[:, :L].clamp(min=0).to(dev())


def recorded(m, monkeypatch, images, ids, **kw):
    """score(...) with the engine's ``each`` hook on -> (the result, the chunks [(r0, n)], the device's fp32 rows [B T, V])"""
    eng = m._engine
    real, chunks, rows = eng.token_top_logprobs, [], []

    def each(r0, n, logits):
        assert logits.dtype == F32 and logits.shape[0] == n and logits.shape[1] == eng.dec.Vp
        chunks.append((r0, n))
        rows.append(logits[:, :eng.dec.V].cpu().numpy().copy())

    with monkeypatch.context() as mp:
        mp.setattr(eng, 'token_top_logprobs', lambda *a, **k: real(*a, each=each, **k))
        out = m.score(images, ids, **kw)
    return out, chunks, np.concatenate(rows, axis=0)


def shaped(out, T):
    assert tuple(out.top_tokens.shape) == tuple(out.top_logprobs.shape) == (B, T, K)
    assert tuple(out.token_entropy.shape) == tuple(out.label_rank.shape) == tuple(out.token_logprobs.shape) == tuple(out.lse.shape) == (B, T)
    assert tuple(out.logprob.shape) == (B,)
    assert out.top_tokens.dtype == I32 and out.label_rank.dtype == I32
    assert all(getattr(out, f).dtype == F32 for f in TUPLE + ('top_logprobs', 'token_entropy'))
    a, b, c = out                                                       # still a tuple of three
    assert a is out.token_logprobs and b is out.lse and c is out.logprob and len(out) == 3
    assert torch.equal(out.logprob, out.token_logprobs.sum(dim=1))


def same(got, want, fields, what):
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and torch.equal(bits(g), bits(w)), f'{what}: {f} differs'


def held_to_the_replica(out, rows, labels, temperature, what):
    """every position against the replica on the device's own row -> the worst error / bound of the floats"""
    T, V = out.lse.shape[1], rows.shape[1]
    lab = labels[:, :T].reshape(-1).cpu().numpy()
    rtok, rlp, rent, rrank, rlse, rylp = score_top_logprobs_host(rows, lab, K, scale=1.0 / temperature, ignore_index=IGNORE)
    tok, rank = out.top_tokens.reshape(-1, K).cpu().numpy(), out.label_rank.reshape(-1).cpu().numpy()
    assert np.array_equal(tok, rtok), f'{what}: tokens differ from the replica\'s at rows {np.flatnonzero((tok != rtok).any(axis=1)).tolist()}'
    assert np.array_equal(rank, rrank), f'{what}: rank {rank.tolist()} vs the replica {rrank.tolist()}'
    v64 = torch.from_numpy(rows * np.float32(1.0 / temperature)).double()
    _, dL = lse_bound(v64, V)
    _, hb = entropy_bound(v64, V, dL)
    dL, hb = dL.numpy(), hb.numpy()
    lp = out.top_logprobs.reshape(-1, K).cpu().numpy().astype(np.float64)
    ylp, lse, ent = (getattr(out, f).reshape(-1).cpu().numpy().astype(np.float64) for f in ('token_logprobs', 'lse', 'token_entropy'))
    e_lp = np.abs(lp - rlp) / (dL[:, None] + U * np.abs(rlp))
    e_y = np.abs(ylp - rylp) / (dL + U * np.abs(rylp))
    e_lse, e_h = np.abs(lse - rlse) / dL, np.abs(ent - rent) / hb
    worst = max(float(e.max()) for e in (e_lp, e_y, e_lse, e_h))
    print(f'{what}: worst error / bound -- top_logprobs {float(e_lp.max()):.3g}, token_logprobs {float(e_y.max()):.3g}, lse {float(e_lse.max()):.3g}, '
          f'entropy {float(e_h.max()):.3g}')
    assert worst <= 1.0, what
    # the label inside the list: the same bits
    t32, y32 = out.top_logprobs.reshape(-1, K).cpu().numpy(), out.token_logprobs.reshape(-1).cpu().numpy()
    inside = np.flatnonzero((rank >= 0) & (rank < K))
    for r in inside:
        assert tok[r, rank[r]] == lab[r] and t32[r, rank[r]].view(np.int32) == y32[r].view(np.int32), f'{what}: row {r}'
    dead = rank < 0
    assert (y32[dead] == 0.0).all() and ((lab[dead] == IGNORE) | (lab[dead] < 0) | (lab[dead] >= V)).all()
    return worst, inside.size


def top_score_bound(m, out, labels, temperature):
    """the module docstring's bound, [B, T]"""
    eng = m._engine
    V, d = eng.dec.V, eng.dec.d
    z = out.logits.double()
    Bz, T = z.shape[:2]
    hb = out.hidden_state[:, -T:].reshape(Bz * T, d).to(BF16).double()
    W = eng.arena.W(eng.n_head)[:V].double()
    S = (hb.abs() @ W.abs().T).view(Bz, T, V)
    live = (labels >= 0) & (labels < V)
    col = torch.where(live, labels, torch.zeros_like(labels))[..., None]
    zt, St = z.gather(-1, col)[..., 0].abs(), S.gather(-1, col)[..., 0]
    zmax, Smax = z.abs().amax(dim=-1), S.amax(dim=-1)
    it = 1.0 / temperature
    n_m = (V + 255) // 256 + 1 + 6 + 4
    spread = it * (z.amax(dim=-1) - z.amin(dim=-1))
    sum_log = U * (3 * spread + 3 * (n_m + 1) + 64 + n_m + V) + 2 * U * np.log(V) + 3 * U * it * zmax
    return 2 * it * d * U * (St + Smax) + 2 * U * it * (zt + zmax) + sum_log + 2 * U * it * zt


def test_every_position_is_the_replica_on_the_device_rows(model, monkeypatch):
    name, m, images, ids = model
    with torch.no_grad():
        fwd = m(images=images, ids=ids)
    T, V = fwd.logits.shape[1], m._engine.dec.V
    labels = next_token_labels(ids, IGNORE)
    for temperature in (1.0, 0.7):
        what = f'{name} T={temperature}'
        out, chunks, rows = recorded(m, monkeypatch, images, ids, temperature=temperature, top_logprobs=K)
        shaped(out, T)
        assert chunks == [(0, B * T)] and rows.shape == (B * T, V)
        worst, inside = held_to_the_replica(out, rows, labels, temperature, what)
        assert bool((out.token_entropy > 0).all()) and bool((out.top_logprobs[..., :-1] >= out.top_logprobs[..., 1:]).all())
        dead = labels[:, :T] == IGNORE
        assert bool((out.label_rank[dead] == -1).all()) and bool((out.label_rank[~dead] >= 0).all()) and bool((out.token_logprobs[dead] == 0).all())
        assert bool((out.top_tokens >= 0).all()) and bool((out.top_tokens < V).all())
        # against the model's own forward
        ref, lse_ref = reference_logprobs(fwd.logits, labels[:, :T], temperature)
        bound = top_score_bound(m, fwd, labels[:, :T], temperature)
        err, err_lse = (out.token_logprobs.double() - ref).abs(), (out.lse.double() - lse_ref).abs()
        print(f'{what}: against forward, logprob worst error / bound {float((err / bound).max()):.3g} (abs {float(err.max()):.3g}), '
              f'lse {float((err_lse / bound).max()):.3g} (abs {float(err_lse.max()):.3g}); {inside} labels inside the top {K}')
        assert bool((err <= bound).all()) and bool((err_lse <= bound).all()), what
        # the argmax of forward's row leads the list wherever forward's two best logits are further apart than the re-accumulation
        top2 = fwd.logits.topk(2, dim=-1)
        clear = (top2.values[..., 0] - top2.values[..., 1]) > 1e-3
        assert torch.equal(out.top_tokens[..., 0][clear].long(), top2.indices[..., 0][clear])


def test_a_chunk_boundary_changes_no_bit(model, monkeypatch):
    name, m, images, ids = model
    eng = m._engine
    one, chunks, rows = recorded(m, monkeypatch, images, ids, temperature=0.7, top_logprobs=K)
    assert len(chunks) == 1
    M = chunks[0][1]
    monkeypatch.setattr(eng, 'SCORE_WS_BYTES', 5 * eng.dec.Vp * 4 + 3)          # five rows fit, far below the 256-row rounding
    cut, chunks, cut_rows = recorded(m, monkeypatch, images, ids, temperature=0.7, top_logprobs=K)
    assert len(chunks) >= 3 and chunks == [(r0, min(5, M - r0)) for r0 in range(0, M, 5)], chunks
    same(cut, one, TUPLE + TOP, f'{name}: {len(chunks)} chunks against one')
    assert np.array_equal(cut_rows.view(np.int32), rows.view(np.int32))
    monkeypatch.setattr(eng, 'SCORE_WS_BYTES', 1)                               # nothing fits: one row at a time, never zero
    single, chunks, _ = recorded(m, monkeypatch, images, ids, temperature=0.7, top_logprobs=K)
    assert chunks == [(r0, 1) for r0 in range(M)]
    same(single, one, TUPLE + TOP, f'{name}: one row per chunk against one chunk')


def test_explicit_labels_with_ignored_positions(model, monkeypatch):
    name, m, images, ids = model
    V = m._engine.dec.V
    default = m.score(images, ids, top_logprobs=K)
    T = default.lse.shape[1]
    lab = next_token_labels(ids, IGNORE)
    lab[:, ::3] = IGNORE
    lab[0, 1] = V                                                               # no token id
    lab[1, 2] = int(default.top_tokens[1, 2, 3])                                # a label known to stand at rank 3
    out, _, rows = recorded(m, monkeypatch, images, ids, labels=lab, top_logprobs=K)
    shaped(out, T)
    held_to_the_replica(out, rows, lab, 1.0, f'{name} explicit labels')
    off = (lab[:, :T] == IGNORE) | (lab[:, :T] >= V)
    assert bool((out.label_rank[off] == -1).all()) and bool((out.token_logprobs[off] == 0).all()) and bool((out.label_rank[~off] >= 0).all())
    assert int(out.label_rank[1, 2]) == 3
    assert bits(out.token_logprobs)[1, 2] == bits(default.top_logprobs)[1, 2, 3]
    # the alternatives, the entropy and the lse do not depend on a label
    same(out, default, ('lse', 'top_tokens', 'top_logprobs', 'token_entropy'), f'{name}: explicit against default labels')


def test_k_zero_is_the_call_without_the_argument(model):
    name, m, images, ids = model
    for kw in (dict(), dict(temperature=0.7)):
        plain, zero = m.score(images, ids, **kw), m.score(images, ids, top_logprobs=0, **kw)
        same(zero, plain, TUPLE, f'{name}: top_logprobs=0')
        assert type(zero) is type(plain) and all(getattr(zero, f) is None and getattr(plain, f) is None for f in TOP)


def test_the_model_refuses_before_it_launches(model, monkeypatch):
    name, m, images, ids = model
    monkeypatch.setattr(m._engine, 'encode', lambda *a, **k: pytest.fail('a refused call reached the encoder'))
    with pytest.raises(ValueError, match='top_logprobs = 9: from 0'):
        m.score(images, ids, top_logprobs=9)
    with pytest.raises(ValueError, match='temperature = 0 with top_logprobs = 5'):
        m.score(images, ids, temperature=0, top_logprobs=K)
    with pytest.raises(ValueError, match='temperature = -0.7 with top_logprobs = 5'):
        m.score(images, ids, temperature=-0.7, top_logprobs=K)
