"""The kernels of a generate_captions step against fp64 on the SAME bf16 operands, and against the kernels they extend:
ops.gemm_top2_lse (epilogue class 15), the three choosers that record the log-prob of their token (ops.top2_ngram_argmax_lp,
ops.ngram_ban_argmax_lp, ops.sample_token_lp), ops.caption_finish against decoding.apply_finish_rule, and a captured step replayed
past `done`.

Shapes: rows M in {1, 5, 300} (300: more than one 256-row tile, ragged), V in {64, 130, 50257} (one segment; a last segment of 2
columns; a last segment of 17), d in {128, 768}.  Planted rows: a row of large EQUAL logits (ties: columns 1, 2 and V - 1 at +40) and
a row whose logits spread over 180 (+90 at one column, -90 at two), so that exp underflows in every segment but one when the row's
segments are merged; with M = 1 the single row is the tie row (d = 128) or the spread row (d = 768).

Bounds (u = 2^-24): se is held to the segment bound of tests/test_lse_head_gpu.py, evaluated on the fp32 logits the GEMM kernel holds;
tok_lp to that file's lp_bound form -- d u sum|h||w| per re-accumulated logit on the target and on the row's worst column, the
rounded exponents, three roundings per merge a column's partial goes through, one addition per level, one log, the final roundings --
where the row forms (fp32 logits in, no segments) go through n_row = ceil(V / 512) + 6 + 16 merges (a thread's chain, the xor tree, the
waves) and, as tests/test_score_gpu.py counts it, up to V additions."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
MS, VS, DS = (1, 5, 300), (64, 130, 50257), (128, 768)
SHAPES = [(M, V, d) for M in MS for V in VS for d in DS]
ROWS = [(M, V) for M in MS for V in VS]
SID = lambda s: 'x'.join(map(str, s))
LEN, IDS_LD = 8, 12                      # tokens in every row before the step; columns of the id / log-prob rows
NGRAMS = (2, 3)


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


_CASES = {}


def case(ops, shape):
    """Operands, the fp32 logits of the persistent GEMM kernel, the fp64 products and the id rows (ban lists) of one shape -- built
    once, never changed."""
    if shape in _CASES:
        return _CASES[shape]
    M, V, d = shape
    g = torch.Generator(device=dev()).manual_seed(7 * V + d + M)
    W = torch.randn(V, d, generator=g, device=dev()) * (3.0 / math.sqrt(d))
    hid = torch.randn(M, d, generator=g, device=dev())
    hid[:, :2] = 0                                         # head columns 0 and 1 reach the planted rows only
    W[:, :2] *= 0.1
    tie_row = 0 if (M > 1 or d == 128) else None
    spread_row = 1 if M > 1 else (0 if d == 768 else None)
    ties, hi, lo = [1, 2, V - 1], 40 % V, [(40 + 5) % V, (3 * 64 + 5) % V]
    Wt = W
    if tie_row is not None:                                # the row is 8 e_0: logit 40 at the three tie columns, |z| < 2 elsewhere
        hid[tie_row] = 0
        hid[tie_row, 0] = 8.0
        Wt[ties, 0] = 5.0
    if spread_row is not None:                             # the row is 8 e_1: +90 at one column, -90 at two
        hid[spread_row] = 0
        hid[spread_row, 1] = 8.0
        Wt[hi, 1], Wt[lo[0], 1], Wt[lo[1], 1] = 11.25, -11.25, -11.25
    W, hid = Wt.to(BF16), hid.to(BF16)
    nseg = (V + 63) // 64
    Mp = max(M, 96)                                        # rows are independent: the padded rows only select the persistent kernel
    hp = torch.zeros(Mp, d, dtype=BF16, device=dev())
    hp[:M] = hid
    logits = torch.zeros(Mp, nseg * 64, device=dev())
    ops.gemm(hp, W, logits, Mp, V, d)
    z32 = torch.full((M, nseg * 64), float('-inf'), device=dev())
    z32[:, :V] = logits[:M, :V]
    z64 = hid.double() @ W.double().T
    S = hid.double().abs() @ W.double().abs().T
    if tie_row is not None:
        assert torch.equal(z32[tie_row, ties], torch.full((3,), 40.0, device=dev())) and float(z32[tie_row, :V].max()) == 40.0
    if spread_row is not None:
        assert float(z64[spread_row].max() - z64[spread_row].min()) > 80.0
    # id rows: LEN tokens each; row r % 3 == 0 bans nothing, == 1 bans the row's best token, == 2 bans the best and the runner-up of the
    # best's segment (the top2 form then re-evaluates that segment)
    zc = z32[:, :V].cpu()
    ids = torch.zeros(M, IDS_LD, dtype=torch.long)
    rng = np.random.default_rng(V + M)
    for r in range(M):
        a = int(zc[r].argmax())
        seg = zc[r, (a // 64) * 64:min((a // 64) * 64 + 64, V)].clone()
        seg[a % 64] = float('-inf')
        s2 = (a // 64) * 64 + int(seg.argmax())
        x = (a + 17) % V
        x = x if x != s2 else (x + 1) % V
        fill = [int(t) for t in rng.permutation(V)[:24] if t not in (x, a, s2)][:7]
        fill += [fill[0]] * (7 - len(fill))
        row = fill[:7] + [x]
        if r % 3 >= 1:
            row[1], row[2] = x, a
        if r % 3 == 2:
            row[3], row[4] = x, s2
        ids[r, :LEN] = torch.tensor(row)
        ids[r, LEN:] = -7
    c = dict(M=M, V=V, d=d, nseg=nseg, W=W, hid=hid, z32=z32, z64=z64, S=S, ids=ids.to(dev()), ties=ties, tie_row=tie_row,
             spread_row=spread_row, ngrams=torch.tensor(NGRAMS, dtype=torch.int32, device=dev()),
             len_ptr=torch.tensor([LEN], dtype=torch.int32, device=dev()))
    _CASES[shape] = c
    return c


def ulp(x):
    _, e = torch.frexp(x.abs().clamp(min=TINY))
    return torch.ldexp(torch.ones_like(x), e - 24)


def guarded(rows_before, rows, rows_after, width, dtype=F32, fill=float('nan')):
    buf = torch.full(((rows_before + rows + rows_after) * width,), fill, dtype=dtype, device=dev())
    return buf[rows_before * width:(rows_before + rows) * width], buf


def run_top2_lse(ops, c):
    M, nseg = c['M'], c['nseg']
    t2, t2buf = guarded(2, M, 256, nseg * 4)
    se, sebuf = guarded(2, M, 256, nseg)
    ops.gemm_top2_lse(c['hid'], c['W'], t2.view(M, nseg, 4), se.view(M, nseg), M, c['V'], c['d'])
    return t2.view(M, nseg, 4), se.view(M, nseg), t2buf, sebuf


@pytest.mark.parametrize('shape', SHAPES, ids=SID)
def test_gemm_top2_lse(ops, shape):
    """class 15: the top-2 words bit-equal to i2t_gemm_bf16_top2's, se within the segment bound, guards untouched, two launches equal"""
    c = case(ops, shape)
    M, V, d, nseg = c['M'], c['V'], c['d'], c['nseg']
    t2, se, t2buf, sebuf = run_top2_lse(ops, c)
    ref = torch.full((M, nseg, 4), float('nan'), device=dev())
    ops.gemm_top2(c['hid'], c['W'], ref, M, V, d)
    torch.cuda.synchronize()
    assert torch.equal(t2.view(torch.int32), ref.view(torch.int32)), 'top-2 words differ from i2t_gemm_bf16_top2'
    for buf, w in ((t2buf, nseg * 4), (sebuf, nseg)):
        assert torch.isnan(buf[:2 * w]).all() and torch.isnan(buf[(2 + M) * w:]).all(), 'a guard word was written'
    assert torch.isfinite(se).all()
    z = c['z32'].view(M, nseg, 64)
    mx = t2[..., 0]
    assert torch.equal(mx, z.amax(dim=-1)), 'v1 differs from the segment maximum of the fp32 logits'
    if c['tie_row'] is not None:                          # ties: the lower column first
        r = c['tie_row']
        assert t2[r, 0, 1:2].view(torch.int32).item() == 1 and t2[r, 0, 3:4].view(torch.int32).item() == 2
    # the segment bound of tests/test_lse_head_gpu.py at scale 1 (no product rounding): per column u (3 |a| + 6 + 2 + 64) e, a = z - mx
    a = z.double() - mx.double()[..., None]
    e = torch.exp(a)
    a0 = torch.where(torch.isfinite(a), a.abs(), torch.zeros_like(a))
    se_ref = e.sum(dim=-1)
    bound = U * ((3 * a0 + 6 + 2 + 64) * e).sum(dim=-1) + 64 * TINY
    err = (se.double() - se_ref).abs()
    print(f'{shape}: se worst error / bound {float((err / bound).max()):.3g}, worst relative error {float((err / se_ref).max()):.3g}')
    assert (err <= bound).all(), f'se: worst error / bound {float((err / bound).max()):.3g}'
    assert (se >= 1.0 - 80 * U).all()
    t2b, seb, _, _ = run_top2_lse(ops, c)
    assert torch.equal(t2.view(torch.int32), t2b.view(torch.int32)) and torch.equal(se.view(torch.int32), seb.view(torch.int32))


def lp_bound(c, tok, n_m, extra_adds):
    """the lp_bound form of tests/test_lse_head_gpu.py at scale 1 for the tokens `tok` [M]; -> (lp_ref, bound)"""
    d, v, S = c['d'], c['z64'], c['S']
    Kd = d * U
    lse_ref = torch.logsumexp(v, dim=-1)
    vmax = v.amax(dim=-1)
    a = v - vmax[:, None]
    e = torch.exp(a)
    rel_se = U * ((3 * a.abs() + 3 * (n_m + 1) + 64 + n_m + extra_adds) * e).sum(dim=-1) / e.sum(dim=-1)
    Smax = S.amax(dim=-1)
    lse_bound = Kd * Smax + U * v.abs().amax(dim=-1) + rel_se + 2 * U * (lse_ref - vmax).abs() + U * lse_ref.abs()
    zt, St = v.gather(1, tok[:, None])[:, 0], S.gather(1, tok[:, None])[:, 0]
    lp_ref = zt - lse_ref
    return lp_ref, Kd * (St + Smax) + lse_bound - Kd * Smax + U * zt.abs() + U * lp_ref.abs()


def lp_buffers(c):
    """id rows and log-prob rows of a chooser call, one guard row behind each"""
    M = c['M']
    ids = torch.full((M + 1, IDS_LD), -7, dtype=torch.long, device=dev())
    ids[:M] = c['ids']
    lp = torch.full((M + 1, IDS_LD), float('nan'), device=dev())
    return ids, lp


def check_chooser(c, tag, ids, lp, want_ids, n_m, extra_adds):
    M = c['M']
    torch.cuda.synchronize()
    assert torch.equal(ids[:M], want_ids), f'{tag}: chosen ids differ from the plain kernel'
    keep = torch.ones(IDS_LD, dtype=torch.bool, device=dev())
    keep[LEN] = False
    assert torch.equal(ids[:M, keep], c['ids'][:, keep]) and bool((ids[M] == -7).all()), f'{tag}: an id column other than len was written'
    assert torch.isnan(lp[:M, keep]).all() and torch.isnan(lp[M]).all(), f'{tag}: a log-prob column other than len was written'
    tok = ids[:M, LEN]
    ref, bound = lp_bound(c, tok, n_m, extra_adds)
    err = (lp[:M, LEN].double() - ref).abs()
    print(f'{tag}: tok_lp worst error / bound {float((err / bound).max()):.3g} (abs {float(err.max()):.3g})')
    assert torch.isfinite(lp[:M, LEN]).all() and (err <= bound).all(), f'{tag}: worst error / bound {float((err / bound).max()):.3g}'


def check_done(fn, M, extra=()):
    """with done = 1 and len == ids_ld (the next row's first column, or the guard row's) nothing is written"""
    ids = torch.randint(0, 50, (M + 1, IDS_LD), device=dev())
    lp = torch.full((M + 1, IDS_LD), 0.25, device=dev())
    len_ptr = torch.tensor([IDS_LD], dtype=torch.int32, device=dev())
    done = torch.ones(1, dtype=torch.int32, device=dev())
    before = [t.clone() for t in (ids, lp) + tuple(extra)]
    fn(ids, lp, len_ptr, done)
    torch.cuda.synchronize()
    for a, b in zip(before, (ids, lp) + tuple(extra)):
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)


@pytest.mark.parametrize('shape', SHAPES, ids=SID)
def test_top2_ngram_argmax_lp(ops, shape):
    c = case(ops, shape)
    M, V, d, nseg = c['M'], c['V'], c['d'], c['nseg']
    t2, se, _, _ = run_top2_lse(ops, c)
    ng, nn = c['ngrams'], len(NGRAMS)
    want = c['ids'].clone()
    ops.top2_ngram_argmax(t2, c['hid'], c['W'], want, IDS_LD, c['len_ptr'], ng, nn, M, V, d)
    ids, lp = lp_buffers(c)
    done = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.top2_ngram_argmax_lp(t2, se, c['hid'], c['W'], ids, IDS_LD, c['len_ptr'], ng, nn, M, V, d, done, lp)
    n_m = 2 + (nseg + 63) // 64 + 6
    check_chooser(c, f'top2 {shape}', ids, lp, want, n_m, 0)
    z = c['z32'][:, :V]
    banned = torch.tensor([r % 3 >= 1 for r in range(M)], device=dev())
    took_max = z.gather(1, ids[:M, LEN:LEN + 1])[:, 0] == z.amax(dim=-1)
    assert bool((took_max == ~banned).all()), 'the ban lists are not in play'
    check_done(lambda i, l, lenp, dn: ops.top2_ngram_argmax_lp(t2, se, c['hid'], c['W'], i, IDS_LD, lenp, ng, nn, M, V, d, dn, l), M)


@pytest.mark.parametrize('rows', ROWS, ids=SID)
def test_ngram_ban_argmax_lp(ops, rows):
    M, V = rows
    c = case(ops, (M, V, 128))
    ld = c['z32'].shape[1]
    logits = c['z32'].clone()
    logits[:, V:] = 1e30                                   # columns past V are not part of the row
    ng, nn = c['ngrams'], len(NGRAMS)
    want = c['ids'].clone()
    ops.ngram_ban_argmax(logits, ld, want, IDS_LD, c['len_ptr'], ng, nn, M, V)
    ids, lp = lp_buffers(c)
    done = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.ngram_ban_argmax_lp(logits, ld, ids, IDS_LD, c['len_ptr'], ng, nn, M, V, done, lp)
    check_chooser(c, f'ban {rows}', ids, lp, want, (V + 511) // 512 + 6 + 16, V)
    check_done(lambda i, l, lenp, dn: ops.ngram_ban_argmax_lp(logits, ld, i, IDS_LD, lenp, ng, nn, M, V, dn, l), M)


@pytest.mark.parametrize('mode', [(0.7, None, 0.6), (1.3, 40, None)], ids=['T0.7_p0.6', 'T1.3_k40'])
@pytest.mark.parametrize('rows', ROWS, ids=SID)
def test_sample_token_lp(ops, rows, mode):
    M, V = rows
    c = case(ops, (M, V, 128))
    ld = c['z32'].shape[1]
    logits = c['z32'].clone()
    logits[:, V:] = 1e30
    temperature, top_k, nucleus_p = mode
    ng, nn = c['ngrams'], len(NGRAMS)
    seed = torch.tensor([12345 + V, 678], dtype=torch.int32, device=dev())
    want = c['ids'].clone()
    ops.sample_token(logits, ld, want, IDS_LD, c['len_ptr'], ng, nn, M, V, temperature, top_k, nucleus_p, seed)
    ids, lp = lp_buffers(c)
    done = torch.zeros(1, dtype=torch.int32, device=dev())
    ops.sample_token_lp(logits, ld, ids, IDS_LD, c['len_ptr'], ng, nn, M, V, temperature, top_k, nucleus_p, seed, done, lp)
    check_chooser(c, f'sample {rows} {mode}', ids, lp, want, (V + 511) // 512 + 6 + 16, V)
    check_done(lambda i, l, lenp, dn: ops.sample_token_lp(logits, ld, i, IDS_LD, lenp, ng, nn, M, V, temperature, top_k, nucleus_p, seed,
                                                          dn, l), M)


@pytest.mark.parametrize('R', [1, 5, 3000])
def test_caption_finish_against_the_host_rule(ops, R):
    """a chooser's stream of tokens fed column by column, then i2t_caption_finish + i2t_beam_advance: ids, lengths and log-probs equal
    decoding.apply_finish_rule's exactly; two more steps after `done` change nothing"""
    from image2text_amd.decoding import apply_finish_rule
    P, T, EOS, PAD, ld = 3, 9, 4, 11, 14
    rng = np.random.default_rng(R)
    stream = rng.integers(0, 6, size=(R, P + T))
    stream[:, :P] = EOS                                    # an EOS in the prompt finishes nothing
    if R > 1:
        stream[1, P:] = 5
        stream[1, P + 6] = EOS                             # no row outlasts step 7: `done` is raised before the stream ends
        stream[:, P + 6] = np.where((stream[:, P:P + 6] == EOS).any(axis=1), stream[:, P + 6], EOS)
    else:
        stream[0, P:] = [1, 2, EOS, 3, EOS, 1, 1, 1, 1]
    lps = -rng.random((R, T)).astype(np.float32) - 0.5
    want_ids, want_len, want_lp = apply_finish_rule(stream, P, EOS, PAD, lps)
    L = want_ids.shape[1]
    assert L < P + T
    ids = torch.full((R + 1, ld), -7, dtype=torch.long, device=dev())
    ids[:R, :P] = EOS
    tok_lp = torch.full((R + 1, ld), float('nan'), device=dev())
    s_ids, s_lp = torch.from_numpy(stream).to(dev()), torch.from_numpy(lps).to(dev())
    i32 = dict(dtype=torch.int32, device=dev())
    finished, lengths = torch.zeros(R + 1, **i32), torch.full((R + 1,), P + T, **i32)
    counters, ctrl = torch.tensor([P - 1, P], **i32), torch.zeros(2, **i32)
    steps = 0
    for t in range(T):
        if int(ctrl[0]):
            break
        ids[:R, P + t], tok_lp[:R, P + t] = s_ids[:, P + t], s_lp[:, t]          # what a chooser writes at ids[r][len]
        ops.caption_finish(ids, ld, counters[1:2], EOS, PAD, finished, lengths, tok_lp, ctrl, R)
        if t == 0:
            assert int(ctrl[1]) == int((want_len > P + 1).sum())                  # rows still unfinished after the first step
        ops.beam_advance(counters, ctrl)
        steps += 1
    assert steps == L - P and int(ctrl[0]) == 1 and counters.tolist() == [P - 1 + steps, L]
    snap = [x.clone() for x in (ids, tok_lp, finished, lengths, counters)]
    for _ in range(2):
        ops.caption_finish(ids, ld, counters[1:2], EOS, PAD, finished, lengths, tok_lp, ctrl, R)
        ops.beam_advance(counters, ctrl)
    torch.cuda.synchronize()
    for a, b in zip(snap, (ids, tok_lp, finished, lengths, counters)):
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)
    assert np.array_equal(ids[:R, :L].cpu().numpy(), want_ids) and bool((ids[:R, L:] == -7).all()) and bool((ids[R] == -7).all())
    assert np.array_equal(lengths[:R].cpu().numpy(), want_len) and int(lengths[R]) == P + T and int(finished[R]) == 0
    assert np.array_equal(tok_lp[:R, P:L].cpu().numpy(), want_lp) and torch.isnan(tok_lp[:R, L:]).all() and torch.isnan(tok_lp[R]).all()
    assert bool((finished[:R] == 1).all())
    # no rule: nothing finishes, every row counts as unfinished
    ctrl.zero_()
    f2 = torch.zeros(R, **i32)
    ops.caption_finish(ids, ld, torch.tensor([P], **i32), None, PAD, f2, lengths, tok_lp, ctrl, R)
    assert ctrl.tolist() == [0, R] and int(f2.sum()) == 0


def test_captured_step_replayed_past_done(ops):
    """head -> choice -> finish -> advance captured into one graph; every row picks the EOS at the first replay, so `done` is up from
    then on and len == ids_ld: three more replays leave every buffer bit-equal"""
    from image2text_amd.decoding import _capture_launches
    M, V, d = 5, 130, 128
    c = case(ops, (M, V, d))
    nseg = c['nseg']
    hid = c['hid'][2:3].expand(M, d).contiguous()          # the same row M times: one argmax for all
    eos = int(c['z32'][2, :V].argmax())
    ld = LEN + 1
    ids = torch.full((M + 1, ld), -7, dtype=torch.long, device=dev())
    ids[:M, :LEN] = torch.arange(LEN, device=dev()) + 200  # no token of the vocabulary: nothing banned, and no EOS before the step
    i32 = dict(dtype=torch.int32, device=dev())
    tok_lp = torch.full((M + 1, ld), float('nan'), device=dev())
    finished, lengths = torch.zeros(M + 1, **i32), torch.full((M + 1,), 99, **i32)
    counters, ctrl = torch.tensor([LEN - 1, LEN], **i32), torch.zeros(2, **i32)
    t2, se = torch.zeros(M, nseg, 4, device=dev()), torch.zeros(M, nseg, device=dev())
    ng = c['ngrams']

    def step():
        ops.gemm_top2_lse(hid, c['W'], t2, se, M, V, d)
        ops.top2_ngram_argmax_lp(t2, se, hid, c['W'], ids, ld, counters[1:2], ng, len(NGRAMS), M, V, d, ctrl[0:1], tok_lp)
        ops.caption_finish(ids, ld, counters[1:2], eos, eos, finished, lengths, tok_lp, ctrl, M)
        ops.beam_advance(counters, ctrl)

    state = (ids, tok_lp, finished, lengths, counters, ctrl)
    init = [x.clone() for x in state]
    step()                                                 # eager once: code objects load before capture
    eager = [x.clone() for x in state]
    for x, x0 in zip(state, init):
        x.copy_(x0)
    graph = _capture_launches(dev(), step)
    graph.launch()
    torch.cuda.synchronize()
    assert ctrl.tolist() == [1, 0] and counters.tolist() == [LEN, ld] and bool((ids[:M, LEN] == eos).all())
    assert bool((lengths[:M] == ld).all()) and bool((finished[:M] == 1).all()) and torch.isfinite(tok_lp[:M, LEN]).all()
    snap = [x.clone() for x in state]
    for a, b in zip(eager, snap):
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)
    for _ in range(3):
        graph.launch()
    torch.cuda.synchronize()
    for a, b in zip(snap, state):
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b)
    assert bool((ids[M] == -7).all()) and torch.isnan(tok_lp[M]).all() and int(lengths[M]) == 99


def test_refusals(ops):
    from image2text_amd.lib import I2TError
    hid = torch.zeros(8, 192, dtype=BF16, device=dev())
    W = torch.zeros(100, 192, dtype=BF16, device=dev())
    with pytest.raises(I2TError, match='multiple of 128'):
        ops.gemm_top2_lse(hid, W, torch.zeros(8, 2, 4, device=dev()), torch.zeros(8, 2, device=dev()), 8, 100, 192)
    with pytest.raises(AssertionError):
        ops.gemm_top2_lse(hid[:, :128], W[:, :128], torch.zeros(8, 3, 4, device=dev()), torch.zeros(8, 2, device=dev()), 8, 100, 128)
