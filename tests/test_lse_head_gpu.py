"""Caption scoring's lm_head without its logits: ops.gemm_lse (the (max, sum exp) of every 64-column segment of a row, left by the
persistent GEMM kernel instead of the tile) and ops.lse_token_logprob (segments -> logsumexp, label logit re-evaluated, log-prob),
against fp64 statements of the same ops on the SAME bf16 operands.  Every tolerance below is built from unit round-offs
(u = 2^-24 for an fp32 operation, 2 u for a 1-ulp hardware exp / log) and the sizes of the quantities involved; none is tuned.

Shapes (M, V, d):
  (96, 1000, 128)     minimum K; V % 64 = 40: a partly valid last segment, and three segments wholly past V inside the last tile
  (300, 50257, 768)   two tile rows, the second ragged; 394 tiles > 256 CUs: the persistent loop takes a second round
  (96, 32000, 4096)   long K
  (96, 151936, 1536)  the widest vocabulary
Planted rows (every shape): row 0 holds a logit near +90 and two near -90 (one in the +90's segment, one elsewhere) and is labelled
with a -90 column; row 1 is labelled V - 1 (the last valid column of the last segment), row 2 is labelled 0, row 3 carries
ignore_index, rows 4 and 5 carry labels outside [0, V) (V and -5)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24                       # unit round-off of one fp32 operation
TINY = 2.0 ** -126                   # a result below it is flushed to zero
IGNORE = -100
SHAPES = [(96, 1000, 128), (300, 50257, 768), (96, 32000, 4096), (96, 151936, 1536)]
SCALES = [1.0, 1.0 / 0.7]
GUARD_BEFORE, GUARD_AFTER = 2, 256   # rows of NaN around the statistics (a tile is 256 rows: a store to a row >= M lands in the second)


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def f32_of(x: float) -> float:
    """the fp32 value a C float argument receives"""
    return float(torch.tensor(x, dtype=F32))


_CASES = {}


def case(ops, shape):
    """Operands, labels, the fp32 logits of the logits form (ops.gemm) and the fp64 products of one shape -- built once, never changed."""
    if shape in _CASES:
        return _CASES[shape]
    M, V, d = shape
    g = torch.Generator(device=dev()).manual_seed(V + d)
    W = torch.randn(V, d, generator=g, device=dev()) * (3.0 / math.sqrt(d))
    hid = torch.randn(M, d, generator=g, device=dev())
    hid[:, 0] = 0
    hi, lo_same, lo_far = 70, 75, 64 * 3 + 5           # segment 1, segment 1, segment 3
    hid[0] = 0
    hid[0, 0] = 8.0                                    # row 0: nothing but the planted column of the head
    W[:, 0] *= 0.1
    W[hi, 0], W[lo_same, 0], W[lo_far, 0] = 11.25, -11.25, -11.25
    W, hid = W.to(BF16), hid.to(BF16)
    labels = torch.randint(0, V, (M,), generator=g, device=dev())
    labels[0], labels[1], labels[2], labels[3], labels[4], labels[5] = lo_far, V - 1, 0, IGNORE, V, -5
    nseg = (V + 63) // 64
    logits = torch.zeros(M, nseg * 64, device=dev())
    ops.gemm(hid, W, logits, M, V, d)                  # fp32 output of the same persistent kernel (M > 64)
    z32 = torch.full((M, nseg * 64), float('-inf'), device=dev())
    z32[:, :V] = logits[:, :V]
    z64 = hid.double() @ W.double().T                  # [M, V]
    S = hid.double().abs() @ W.double().abs().T        # sum_k |h| |w|: the scale of a dot product's rounding errors
    assert 89.0 < float(z64[0, hi]) < 91.0 and -91.0 < float(z64[0, lo_same]) < -89.0 and -91.0 < float(z64[0, lo_far]) < -89.0
    c = dict(M=M, V=V, d=d, nseg=nseg, W=W, hid=hid, labels=labels, z32=z32, z64=z64, S=S, hi=hi, lo_far=lo_far)
    _CASES[shape] = c
    return c


def run_gemm_lse(ops, c, scale):
    """-> (stats [M, nseg, 2], the whole guarded buffer)"""
    M, nseg = c['M'], c['nseg']
    buf = torch.full(((GUARD_BEFORE + M + GUARD_AFTER) * nseg * 2,), float('nan'), device=dev())
    stats = buf[GUARD_BEFORE * nseg * 2:(GUARD_BEFORE + M) * nseg * 2].view(M, nseg, 2)
    ops.gemm_lse(c['hid'], c['W'], stats, M, c['V'], c['d'], scale=scale)
    return stats, buf


def ulp(x):
    """fp32 unit in the last place at the magnitude of the fp64 values x"""
    _, e = torch.frexp(x.abs().clamp(min=TINY))
    return torch.ldexp(torch.ones_like(x), e - 24)


def se_terms(v, mx):
    """fp64 [M, nseg, 64]: a = v - mx of every column (the segment's own maximum subtracted), exp(a); columns past V: a = -inf, exp = 0"""
    a = v - mx[..., None]
    return a, torch.exp(a)


def stats_case(ops, shape, scale):
    c = case(ops, shape)
    M, V, nseg = c['M'], c['V'], c['nseg']
    s = f32_of(scale)
    stats, buf = run_gemm_lse(ops, c, scale)
    torch.cuda.synchronize()
    # every (m < M, seg < nseg) entry written and finite, nothing else touched
    assert torch.isfinite(stats).all()
    assert torch.isnan(buf[:GUARD_BEFORE * nseg * 2]).all() and torch.isnan(buf[(GUARD_BEFORE + M) * nseg * 2:]).all()
    mx, se = stats[..., 0], stats[..., 1]
    z = c['z32'].view(M, nseg, 64)
    zmax = z.amax(dim=-1)
    if scale == 1.0:
        assert torch.equal(mx, zmax), 'segment maximum differs from the fp32 logits of the logits form'
    else:
        ref = s * zmax.double()
        err = (mx.double() - ref).abs()
        print(f'{shape} scale {scale}: mx worst error {float((err / ulp(ref)).max()):.3g} ulp')
        assert (err <= ulp(ref)).all()
    # se: v = s z (fp64 product of the fp32 values the kernel holds), a = v - mx (the kernel's own maximum).  Per column:
    #   the product s z is rounded (u |v|, scale != 1 only), the subtraction is rounded (u |a|), exp(a) = exp2(a log2 e) rounds the
    #   constant and the product (2 u |a| once the absolute error of the exponent turns into a relative one) and the hardware exp2 is
    #   good to 1 ulp (2 u).  A column's term is rescaled when its lane's partial joins the other lanes' (2 merges): the rescale factors
    #   are exp's of non-positive pieces that add up to a, so the |a| parts above are counted once; 3 exp's (6 u) and 2 products (2 u).
    #   Then the sum: no more than 64 fp32 additions above any term (64 u).  A term below 2^-126 may be flushed (64 TINY).
    v = s * z.double()
    a, e = se_terms(v, mx.double())
    se_ref = e.sum(dim=-1)
    a0 = torch.where(torch.isfinite(a), a.abs(), torch.zeros_like(a))
    v0 = torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v)) if scale != 1.0 else torch.zeros_like(a0)
    bound = U * ((3 * a0 + v0 + 6 + 2 + 64) * e).sum(dim=-1) + 64 * TINY
    err = (se.double() - se_ref).abs()
    print(f'{shape} scale {scale}: se worst error / bound {float((err / bound).max()):.3g}, worst relative error {float((err / se_ref).max()):.3g}')
    assert (err <= bound).all(), f'se: worst error / bound {float((err / bound).max()):.3g}'
    assert (se >= 1.0 - 80 * U).all()                    # the maximum's own term is exp(0)
    # a second launch: bit-identical
    stats2, _ = run_gemm_lse(ops, c, scale)
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gemm_lse_segment_stats(ops, shape):
    """scale = 1: mx bit-equal to the segment maxima of the fp32 logits ops.gemm leaves, se within the derived bound, guards untouched,
    two launches bit-identical"""
    stats_case(ops, shape, 1.0)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gemm_lse_segment_stats_scaled(ops, shape):
    """scale = 1 / 0.7: the same, with mx within one fp32 ulp of scale . (fp32 logit maximum)"""
    stats_case(ops, shape, 1.0 / 0.7)


@pytest.mark.parametrize('scale', SCALES, ids=['T1', 'T0.7'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_lse_token_logprob_vs_fp64(ops, shape, scale):
    """lse and logprob against fp64 logsumexp / log_softmax of scale . hid . W^T on the bf16 operands."""
    c = case(ops, shape)
    M, V, d, nseg, labels = c['M'], c['V'], c['d'], c['nseg'], c['labels']
    s = f32_of(scale)
    stats, _ = run_gemm_lse(ops, c, scale)
    out = torch.full((2, M + 8), float('nan'), device=dev())
    lse, lp = out[0, :M], out[1, :M]
    ops.lse_token_logprob(stats, c['hid'], c['W'], labels, lse, lp, M, V, d, scale=scale, ignore_index=IGNORE)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, M:]).all()
    assert torch.isfinite(lse).all() and torch.isfinite(lp).all()
    v = s * c['z64']
    lse_ref = torch.logsumexp(v, dim=-1)
    live = (labels != IGNORE) & (labels >= 0) & (labels < V)
    col = torch.where(live, labels, torch.zeros_like(labels))
    zt = v.gather(1, col[:, None])[:, 0]
    lp_ref = torch.where(live, zt - lse_ref, torch.zeros_like(zt))
    # every fp32 logit: K exact products, K additions -> |z32 - z64| <= K u sum_k |h| |w|; scaled, and rounded once more (u |v|).
    # logsumexp moves by no more than the largest change of a logit.  The sum of exp's: per column the terms of the segment bound
    # (3 |a| u for the rounded exponent, a = v - row maximum, counted once along the chain of rescales), one exp and one product per
    # merge the column's partial goes through (n_m merges: 2 in the GEMM epilogue, ceil(nseg / 64) + 6 in the row kernel; 3 u each)
    # and one addition per level (64 + ceil(nseg / 64) + 6).  Then one log (1 ulp: 2 u |log se|) and mx + log se (u |lse|).
    Kd = d * U * s
    S = c['S']
    Smax = S.amax(dim=-1)
    n_m = 2 + (nseg + 63) // 64 + 6
    a = v - v.amax(dim=-1, keepdim=True)
    e = torch.exp(a)
    rel_se = U * ((3 * a.abs() + 3 * (n_m + 1) + 64 + n_m) * e).sum(dim=-1) / e.sum(dim=-1)
    lse_bound = Kd * Smax + U * v.abs().amax(dim=-1) + rel_se + 2 * U * (lse_ref - v.amax(dim=-1)).abs() + U * lse_ref.abs()
    # the label's logit: d products and additions in fp32 (K u sum |h| |w_label|), scaled (u |z_t|), and the final subtraction (u |logprob|)
    St = S.gather(1, col[:, None])[:, 0]
    lp_bound = Kd * (St + Smax) + lse_bound - Kd * Smax + U * zt.abs() + U * lp_ref.abs()
    err_lse = (lse.double() - lse_ref).abs()
    err_lp = (lp.double() - lp_ref).abs()
    print(f'{shape} scale {scale}: lse worst error / bound {float((err_lse / lse_bound).max()):.3g} (abs {float(err_lse.max()):.3g}), '
          f'logprob worst error / bound {float((err_lp[live] / lp_bound[live]).max()):.3g} (abs {float(err_lp.max()):.3g})')
    assert (err_lse <= lse_bound).all(), f'lse: worst error / bound {float((err_lse / lse_bound).max()):.3g}'
    assert (err_lp[live] <= lp_bound[live]).all(), f'logprob: worst error / bound {float((err_lp[live] / lp_bound[live]).max()):.3g}'
    # ignored and out-of-range labels: exactly 0.0, their lse still held to the bound above
    dead = (~live).nonzero()[:, 0].tolist()
    assert dead == [3, 4, 5]
    assert torch.equal(lp[~live].view(torch.int32), torch.zeros(3, dtype=torch.int32, device=dev()))
    # the planted rows: row 0's label sits ~180 / T below the row maximum
    assert float(lp_ref[0]) < -179.0 * s and abs(float(lp[0]) - float(lp_ref[0])) <= float(lp_bound[0])
    assert int(labels[1]) == V - 1 and int(labels[2]) == 0 and bool(live[1]) and bool(live[2])
    # a second launch: bit-identical
    out2 = torch.empty(2, M, device=dev())
    ops.lse_token_logprob(stats, c['hid'], c['W'], labels, out2[0], out2[1], M, V, d, scale=scale, ignore_index=IGNORE)
    assert torch.equal(out2.view(torch.int32), out[:, :M].contiguous().view(torch.int32))


def test_refusals(ops):
    """the argument checks of i2t_gemm_bf16_top2: K % 128, nseg"""
    from image2text_amd.lib import I2TError
    hid = torch.zeros(8, 192, dtype=BF16, device=dev())
    W = torch.zeros(100, 192, dtype=BF16, device=dev())
    stats = torch.zeros(8, 2, 2, device=dev())
    with pytest.raises(I2TError, match='multiple of 128'):
        ops.gemm_lse(hid, W, stats, 8, 100, 192)
    with pytest.raises(AssertionError):
        ops.gemm_lse(hid[:, :128], W[:, :128], torch.zeros(8, 3, 2, device=dev()), 8, 100, 128)
