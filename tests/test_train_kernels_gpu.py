"""The training-step kernels of csrc/norm.hip (LayerNorm, LayerNormND) and the older half of csrc/elementwise.hip (embeddings,
cross-entropy, gradient normaliser, AdamW, dropout, the strided arena helpers) against the float64 statements of tests/train_ref.py,
by the rules of tests/test_row_kernels_gpu.py: per-element bounds, no element excluded, non-finite output fails, outputs start as
NaN, and every byte a kernel must not touch holds a non-zero sentinel compared with torch.equal.  The bounds and the way every k
was counted: DESIGN.md "Training-step kernels".

fp32 outputs: 1e-5 |ref| + k 2^-23 sum|terms| (k = fp32 operations on the longest path, stated at each comparison); bf16 outputs:
2^-7 |ref| + a; sums that land by float atomics add one operation per workgroup that adds into the address."""
import math

import numpy as np
import pytest
import torch

import train_ref as R
from test_row_kernels_gpu import BF16, E7, F32, SENT, TINY, U32, check, dev, nans, refused, rnd

pytestmark = pytest.mark.gpu

I16 = torch.int16


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def sent(*shape, dtype=F32):
    return torch.full(shape, SENT, dtype=dtype, device=dev())


def is_sent(t):
    return torch.equal(t, torch.full_like(t, SENT))


def keep_mask(key, n, thr, offset=0):
    from image2text_amd import rng
    return rng.keep_mask(key, n, thr, offset).to(dev())


def drop_args(seed, p=0.2):
    from image2text_amd import rng
    key, thr = rng.site_key(seed, 7), rng.threshold(p)
    return key, thr, rng.scale(thr)


def deterministic_twice(ops, run):
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        return run(), run()
    finally:
        ops.set_deterministic(was)


# --------------------------------------------------------------------------------------------------------- row LayerNorm
NARROW_D, WIDE_D = [4, 64, 252, 256, 260, 768, 1020, 1024], [1028, 4544, 8188, 8192]


def _ln_inputs(M, d, seed):
    """row scales 1e-3 .. 1e3, row means up to 100 standard deviations from zero; row 1 (when there is one) all zero"""
    x = rnd(M, d, seed=seed)
    if M > 1:
        x = (x + torch.linspace(0, 100, M, device=dev()).unsqueeze(1)) * torch.logspace(-3, 3, M, device=dev()).unsqueeze(1)
        x[1] = 0.0
    else:
        x = x + 100.0
    return x.contiguous(), (1.0 + 0.5 * rnd(d, seed=seed + 1)).contiguous(), rnd(d, seed=seed + 2).contiguous()


def _ln_k(d):
    """fp32 operations on the longest path of a row sum: a lane's serial chain (4 chunks x 4, wide: 8 x 4), the 6-step wave tree,
    the 4-wave LDS sum of the wide form, the division"""
    return 16 + 6 + 1 if d <= 1024 else 32 + 6 + 4 + 1


def _ln_fwd_case(ops, M, d):
    x, gamma, beta = _ln_inputs(M, d, seed=d + M)
    k = _ln_k(d) + 4                                        # + subtract, two products and the add of the affine map
    for eps in (1e-5, 1e-6):
        for b in (None, beta):
            r = R.ln_fwd(x, gamma, b, eps)
            tol_y = 1e-5 * r['y'].abs() + k * U32 * r['amp']
            tol_mean = 1e-5 * r['mean'].abs() + k * U32 * r['mean_abs']
            tol_rstd = r['rstd'] * (1e-5 + (k + 2) * U32 * (1 + r['mean_abs'] * r['rstd']))          # + rsqrtf
            ys = {}
            for ydt, null in ((F32, 'none'), (BF16, 'none'), (F32, 'mean'), (BF16, 'rstd')):
                y, mean, rstd = nans(M + 1, d, dtype=ydt), None if null == 'mean' else nans(M + 1), None if null == 'rstd' else nans(M + 1)
                for t in (y, mean, rstd):
                    if t is not None:
                        t[M:] = SENT
                ops.layernorm_fwd(x, gamma, b, y, mean, rstd, M, d, eps=eps)
                tag = f'ln_fwd M={M} d={d} eps={eps} beta={b is not None} y={ydt} null={null}'
                check(f'{tag} y', y[:M], r['y'], tol_y if ydt == F32 else E7 * r['y'].abs() + tol_y)
                assert is_sent(y[M:]), f'{tag}: rows past M'
                if mean is not None:
                    check(f'{tag} mean', mean[:M], r['mean'], tol_mean)
                    assert is_sent(mean[M:])
                if rstd is not None:
                    check(f'{tag} rstd', rstd[:M], r['rstd'], tol_rstd)
                    assert is_sent(rstd[M:])
                    if M > 1:                               # the all-zero row: rstd = eps^-1/2 within 2 ulp
                        want = 1.0 / math.sqrt(R.f32(eps))
                        assert abs(float(rstd[1]) - want) <= 2 * U32 * want, (tag, float(rstd[1]), want)
                if M > 1:                                   # ... and y == beta exactly
                    want = torch.zeros(d, device=dev()) if b is None else b
                    assert torch.equal(y[1], want.to(ydt)), f'{tag}: the all-zero row'
                ys.setdefault(ydt, y)
                if null != 'none':
                    assert torch.equal(y.view(I16 if ydt == BF16 else torch.int32), ys[ydt].view(I16 if ydt == BF16 else torch.int32)), f'{tag}: a null stat changed y'
            assert torch.equal(ys[BF16][:M], ys[F32][:M].to(BF16)), f'ln_fwd M={M} d={d}: the bf16 output is not the rounded fp32 output'


@pytest.mark.parametrize('M', [1, 3, 5, 33])
@pytest.mark.parametrize('d', NARROW_D)
def test_layernorm_fwd_narrow(ops, d, M):
    _ln_fwd_case(ops, M, d)


@pytest.mark.parametrize('M', [1, 2, 9])
@pytest.mark.parametrize('d', WIDE_D)
def test_layernorm_fwd_wide(ops, d, M):
    _ln_fwd_case(ops, M, d)


@pytest.mark.parametrize('M,d', [(4 * 8192 + 5, 64), (16384 + 3, 1028)])
def test_layernorm_fwd_grid_stride(ops, M, d):
    """one workgroup past the grid cap (8192 workgroups of 4 rows; 16384 of one row): the loops take a second trip"""
    _ln_fwd_case(ops, M, d)


def test_layernorm_fwd_refusals(ops):
    x, g, y = rnd(4, 8196), rnd(8196), nans(4, 8196)
    refused(lambda: ops.layernorm_fwd(x, g, None, y, None, None, 4, 6), 'i2t_layernorm_fwd')
    refused(lambda: ops.layernorm_fwd(x, g, None, y, None, None, 4, 8196), 'i2t_layernorm_fwd')
    refused(lambda: ops.layernorm_fwd(x, g, None, y, None, None, 0, 64), 'i2t_layernorm_fwd')
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


def _ln_bwd_setup(M, d, dy_dtype, seed):
    x, gamma, _ = _ln_inputs(M, d, seed=seed)
    f = R.ln_fwd(x, gamma, None, 1e-5)
    mean, rstd = f['mean'].float().contiguous(), f['rstd'].float().contiguous()          # the fp32 values the kernel reads
    return x, gamma, mean, rstd, rnd(M, d, seed=seed + 5, dtype=dy_dtype)


def _ln_bwd_tols(r, M, d, start_g=None, start_b=None):
    wide = d > 1024
    chain = 32 + 4 if wide else 16
    k_dx = 2 * chain + 6 + 1 + 6                            # the s2 chain (product + add per element), tree, division, 6 ops to dx (+ the accumulate)
    rows_per, blocks = (8, (M + 7) // 8) if wide else (8, (M + 31) // 32)
    k_w = 4 * rows_per + (0 if wide else 3) + blocks + 1    # a thread's rows (xhat: 2, product, add), the 4-wave sum, one atomic per workgroup, the start value
    tol_dx = 1e-5 * r['dx_unmasked'].abs() + k_dx * U32 * r['dx_terms']
    sg = 0.0 if start_g is None else start_g.double().abs()
    sb = 0.0 if start_b is None else start_b.double().abs()
    tol_dg = 1e-5 * r['dgamma'].abs() + k_w * U32 * (r['dgamma_terms'] + sg)
    tol_db = 1e-5 * r['dbeta'].abs() + k_w * U32 * (r['dbeta_terms'] + sb)
    return tol_dx, tol_dg, tol_db


def _ln_bwd_case(ops, M, d, dy_dtype):
    x, gamma, mean, rstd, dy = _ln_bwd_setup(M, d, dy_dtype, seed=3 * d + M)
    dx0, dg0, db0 = rnd(M, d, seed=7), rnd(d, seed=8), rnd(d, seed=9)
    for acc, with_bf, which in ((False, True, 'both'), (True, False, 'both'), (False, False, 'dgamma'), (True, True, 'dbeta'), (False, True, 'neither')):
        r = R.ln_bwd(dy, x, gamma, mean, rstd, dx0=dx0 if acc else None)
        tol_dx, tol_dg, tol_db = _ln_bwd_tols(r, M, d, dg0, db0)
        dx = nans(M + 1, d)
        dx[M:] = SENT
        if acc:
            dx[:M] = dx0
        dxb = nans(M + 1, d, dtype=BF16) if with_bf else None
        if with_bf:
            dxb[M:] = SENT
        dg = dg0.clone() if which in ('both', 'dgamma') else None
        db = db0.clone() if which in ('both', 'dbeta') else None
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, M, d, dx_accumulate=acc, dx_bf16=dxb)
        tag = f'ln_bwd M={M} d={d} dy={dy_dtype} acc={acc} bf={with_bf} {which}'
        check(f'{tag} dx', dx[:M], r['dx'], tol_dx)
        assert is_sent(dx[M:]), f'{tag}: rows past M'
        if with_bf:
            assert torch.equal(dxb[:M], dx[:M].to(BF16)), f'{tag}: dx_bf16 is not the rounded dx'
            assert is_sent(dxb[M:])
        if dg is not None:
            check(f'{tag} dgamma', dg, r['dgamma'] + dg0.double(), tol_dg)
        if db is not None:
            check(f'{tag} dbeta', db, r['dbeta'] + db0.double(), tol_db)


@pytest.mark.parametrize('dy_dtype', [F32, BF16])
@pytest.mark.parametrize('M', [1, 3, 31, 32, 33, 65])
@pytest.mark.parametrize('d', NARROW_D)
def test_layernorm_bwd_narrow(ops, d, M, dy_dtype):
    _ln_bwd_case(ops, M, d, dy_dtype)


@pytest.mark.parametrize('dy_dtype', [F32, BF16])
@pytest.mark.parametrize('M', [1, 7, 8, 9, 17])
@pytest.mark.parametrize('d', WIDE_D)
def test_layernorm_bwd_wide(ops, d, M, dy_dtype):
    _ln_bwd_case(ops, M, d, dy_dtype)


@pytest.mark.parametrize('extra', ['sumsq_out', 'dx_pre_sumsq', 'bf16_drop', 'dx_mask', 'all'])
@pytest.mark.parametrize('M,d', [(33, 64), (65, 260), (40, 1024)])
def test_layernorm_bwd_extras(ops, M, d, extra):
    x, gamma, mean, rstd, dy = _ln_bwd_setup(M, d, F32, seed=d + M + 1)
    dx0 = rnd(M, d, seed=17, scale=5.0)
    every = extra == 'all'
    kd, td, sd = drop_args(11)
    km, tm, sm = drop_args(12, p=0.3)
    use_ss, use_pre, use_drop, use_mask = every or extra == 'sumsq_out', every or extra == 'dx_pre_sumsq', every or extra == 'bf16_drop', every or extra == 'dx_mask'
    pre = torch.tensor([float(dx0.double().pow(2).sum()), SENT], device=dev()) if use_pre else None
    drop = keep_mask(kd, M * d, td).view(M, d) if use_drop else None
    mask = keep_mask(km, M * d, tm).view(M, d) if use_mask else None
    r = R.ln_bwd(dy, x, gamma, mean, rstd, dx0=dx0, pre_sumsq=pre, mask=mask, mask_scale=sm, drop=drop, drop_scale=sd)
    tol_dx, _, _ = _ln_bwd_tols(r, M, d)
    tol_dx = tol_dx + (4 * U32 * dx0.double().abs() if use_pre else 0.0)       # sqrtf, the add of 1e-6, the reciprocal, the product
    dx, dxb = dx0.clone(), nans(M + 1, d, dtype=BF16)
    dxb[M:] = SENT
    ss = torch.tensor([2.5, SENT], device=dev()) if use_ss else None
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, None, None, M, d, dx_accumulate=True, dx_bf16=dxb, bf16_drop=(1, kd, td, sd) if use_drop else None,
                      sumsq_out=ss, dx_pre_sumsq=pre, dx_mask=(1, km, tm, sm) if use_mask else None)
    tag = f'ln_bwd extras M={M} d={d} {extra}'
    scale_m, scale_d = (R.f32(sm) if use_mask else 1.0), (R.f32(sd) if use_drop else 1.0)
    # the masked / dropped value is the unmasked dx (bound tol_dx, which holds the 1e-5 |ref|) times the factor: one more rounding
    check(f'{tag} dx', dx, r['dx'], (tol_dx + U32 * r['dx_unmasked'].abs()) * scale_m)
    check(f'{tag} dx_bf16', dxb[:M], r['dx_bf16'], E7 * r['dx_bf16'].abs() + (tol_dx + U32 * r['dx_unmasked'].abs()) * scale_d)
    assert is_sent(dxb[M:])
    if use_mask:
        assert torch.equal(dx[~mask], torch.zeros_like(dx[~mask])), f'{tag}: a masked element is not zero'
    if use_drop:
        assert torch.equal(dxb[:M][~drop], torch.zeros_like(dxb[:M][~drop])), f'{tag}: a dropped element is not zero'
    if use_drop and not use_mask:                           # the copy is the f32 dx times the factor, rounded
        assert torch.equal(dxb[:M], torch.where(drop, dx * np.float32(sd), torch.zeros_like(dx)).to(BF16))
    if not use_drop and not use_mask:
        assert torch.equal(dxb[:M], dx.to(BF16))
    if use_pre:
        assert float(pre[1]) == SENT
    if use_ss:
        # a thread's chain of squares (8 rows x 4 chunks x 4 elements, product + add), trees, one atomic per workgroup; every dx
        # carries its own error twice (d(x^2) = 2 x dx)
        k_ss = 2 * 8 * 16 + 6 + 3 + (M + 31) // 32 + 1
        want = r['sumsq'] + 2.5
        tol_ss = 1e-5 * want + k_ss * U32 * want + 2 * (r['dx_unmasked'].abs() * tol_dx).sum()
        check(f'{tag} sumsq_out', ss[0], want, tol_ss)
        assert float(ss[1]) == SENT


@pytest.mark.parametrize('M,period,rows', [(33, 5, 1), (33, 5, 0), (33, 5, 5), (2 * 197, 197, 1)])
def test_layernorm_bwd_acc_period(ops, M, period, rows):
    """rows outside the accumulated set start as NaN in dx: they must come out finite and bit-equal to the plain backward (written,
    not read); the others equal the accumulating backward"""
    d = 64
    x, gamma, mean, rstd, dy = _ln_bwd_setup(M, d, F32, seed=period + rows)
    dx0 = rnd(M, d, seed=3, scale=3.0)
    accd = (torch.arange(M, device=dev()) % period) < rows
    dx = torch.where(accd.unsqueeze(1), dx0, nans(M, d))
    dxb = nans(M, d, dtype=BF16)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, None, None, M, d, dx_accumulate=True, dx_bf16=dxb, acc_period=period, acc_rows=rows)
    r = R.ln_bwd(dy, x, gamma, mean, rstd, dx0=dx0, acc_period=period, acc_rows=rows)
    tol_dx, _, _ = _ln_bwd_tols(r, M, d)
    check(f'ln_bwd acc_period={period} acc_rows={rows} M={M}', dx, r['dx'], tol_dx)
    assert torch.equal(dxb, dx.to(BF16))
    plain, full = nans(M, d), dx0.clone()
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, plain, None, None, M, d)
    ops.layernorm_bwd(dy, x, gamma, mean, rstd, full, None, None, M, d, dx_accumulate=True)
    assert torch.equal(dx[~accd], plain[~accd]) and torch.equal(dx[accd], full[accd])
    assert int(accd.sum()) == (M // period) * rows + min(M % period, rows)


def test_layernorm_bwd_refusals(ops):
    M = 4
    for d in (1028, 64):
        x, gamma, mean, rstd, dy = _ln_bwd_setup(M, d, F32, seed=1)
        dx, dxb, one = rnd(M, d), nans(M, d, dtype=BF16), torch.ones(1, device=dev())
        dx0 = dx.clone()
        call = lambda **kw: ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, None, None, M, d, **kw)
        if d > 1024:                                        # no extra on the wide form
            refused(lambda: call(dx_accumulate=True, dx_bf16=dxb, sumsq_out=one), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_accumulate=True, dx_bf16=dxb, dx_pre_sumsq=one), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_accumulate=True, dx_bf16=dxb, bf16_drop=(1, 5, 50, 1.25)), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_accumulate=True, dx_bf16=dxb, dx_mask=(1, 5, 50, 1.25)), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_accumulate=True, dx_bf16=dxb, acc_period=2, acc_rows=1), 'i2t_layernorm_bwd')
        else:
            refused(lambda: call(acc_period=2, acc_rows=1), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_accumulate=True, acc_period=2, acc_rows=3), 'i2t_layernorm_bwd')
            refused(lambda: call(bf16_drop=(1, 5, 50, 1.25)), 'i2t_layernorm_bwd')
            refused(lambda: call(dx_pre_sumsq=one), 'i2t_layernorm_bwd')
        torch.cuda.synchronize()
        assert torch.isnan(dxb.float()).all() and torch.equal(dx, dx0) and float(one) == 1.0


@pytest.mark.parametrize('d', [64, 1028])
def test_layernorm_bwd_deterministic(ops, d):
    M = 65
    x, gamma, mean, rstd, dy = _ln_bwd_setup(M, d, F32, seed=d)

    def run():
        dx, dg, db = nans(M, d), torch.zeros(d, device=dev()), torch.zeros(d, device=dev())
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, M, d)
        return dx, dg, db
    a, b = deterministic_twice(ops, run)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    r = R.ln_bwd(dy, x, gamma, mean, rstd)
    tol_dx, tol_dg, tol_db = _ln_bwd_tols(r, M, d)
    check(f'ln_bwd deterministic d={d} dx', a[0], r['dx'], tol_dx)
    check(f'ln_bwd deterministic d={d} dgamma', a[1], r['dgamma'], tol_dg)
    check(f'ln_bwd deterministic d={d} dbeta', a[2], r['dbeta'], tol_db)


# ----------------------------------------------------------------------------------------------------------- LayerNormND
STATS = 34
HEAD = 8                                                    # sentinel elements ahead of every slab of a strided buffer


def _lnnd_inputs(B, n, seed, far=0.0):
    """slabs with a ramp across them (the 16 splits have different means: the Chan combine's cross term matters), a different
    scale per image, and optionally a mean ``far`` standard deviations from zero"""
    x = rnd(B, n, seed=seed) + torch.linspace(-2, 2, n, device=dev()) + far * 1.5
    x = x * torch.logspace(-1, 1, B, device=dev()).unsqueeze(1) if B > 1 else x
    return x.contiguous(), (0.3 * rnd(n, seed=seed + 1)).contiguous(), (1.0 + 0.5 * rnd(n, seed=seed + 2)).contiguous(), rnd(n, seed=seed + 3).contiguous()


def _lnnd_k(n):
    """a thread's chain in its split (float4s of the split / 256 threads x 4), the workgroup tree (6 + 4), the 16-step Chan combine
    (4 operations a step), the affine map"""
    per = ((n >> 2) + 15) // 16
    return 4 * ((per + 255) // 256) + 10 + 64 + 4


def _strided(B, n, fill=None, seed=0):
    """[B][HEAD + n] buffer whose slabs start HEAD elements into each row: (buffer, the flat view the kernel gets, batch stride)"""
    buf = sent(B + 1, HEAD + n)
    if fill is not None:
        buf[:B, HEAD:] = fill
    return buf, buf.view(-1)[HEAD:], HEAD + n


def _lnnd_case(ops, B, rows, d, far=0.0):
    n = rows * d
    x, add, gamma, beta = _lnnd_inputs(B, n, seed=B + n, far=far)
    k = _lnnd_k(n)
    per = ((n >> 2) + 15) // 16
    k_b = 8 * ((per + 255) // 256) + 10 + 16 + 6            # the s2 chain (2 products + add), tree, the 16 partials, 6 ops to dx
    k_w = 2 * B + 16 + 2                                    # a thread's walk over its images (product + add), at most 16 slices' atomics, the start
    dyv = rnd(B, n, seed=B + n + 9)
    for a, b, strided in ((None, None, False), (add, None, True), (None, beta, True), (add, beta, True)):
        r = R.lnnd_fwd(x, a, gamma, b)
        ybuf, y, y_bs = _strided(B, n) if strided else (None, nans(B, n), n)
        if strided:
            ybuf[:B, HEAD:] = float('nan')
        stats = nans(B + 1, STATS)
        stats[B:] = SENT
        ops.layernorm_nd_fwd(x, a, gamma, b, y, y_bs, stats, B, rows, d)
        tag = f'lnnd B={B} {rows}x{d} add={a is not None} beta={b is not None} far={far}'
        got = ybuf[:B, HEAD:] if strided else y
        check(f'{tag} y', got, r['y'], 1e-5 * r['y'].abs() + k * U32 * r['amp'])
        check(f'{tag} mean', stats[:B, 0], r['mean'], 1e-5 * r['mean'].abs() + k * U32 * r['mean_abs'])
        check(f'{tag} rstd', stats[:B, 1], r['rstd'], r['rstd'] * (1e-5 + (k + 2) * U32 * (1 + r['mean_abs'] * r['rstd'])))
        assert is_sent(stats[B:]), f'{tag}: stats past B'
        if strided:
            assert is_sent(ybuf[:, :HEAD]) and is_sent(ybuf[B:]), f'{tag}: the rows ahead of the slab'
        # backward, from the mean / rstd the forward left (what the kernel reads)
        mean, rstd = stats[:B, 0].clone(), stats[:B, 1].clone()
        bw = R.lnnd_bwd(dyv, x, a, gamma, mean, rstd)
        dybuf, dy, dy_bs = _strided(B, n, fill=dyv)
        g0, b0, a0 = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3)
        nulls = ('none', 'dgamma', 'dbeta', 'dadd') if (a is not None and b is not None) else ('none' if a is not None else 'dadd',)
        for null in nulls:
            dx = nans(B + 1, n)
            dx[B:] = SENT
            dg, db, da = (None if null == 'dgamma' else g0.clone()), (None if null == 'dbeta' else b0.clone()), (None if null == 'dadd' else a0.clone())
            ops.layernorm_nd_bwd(dy, dy_bs, x, a, gamma, stats, dx, dg, db, da, B, rows, d)
            t2 = f'{tag} bwd null={null}'
            check(f'{t2} dx', dx[:B], bw['dx'], 1e-5 * bw['dx'].abs() + k_b * U32 * bw['dx_terms'] + bw['dx_add_err'])
            assert is_sent(dx[B:]) and torch.equal(dybuf[:B, HEAD:], dyv) and is_sent(dybuf[:, :HEAD])
            assert torch.equal(stats[:B, 0], mean) and torch.equal(stats[:B, 1], rstd) and is_sent(stats[B:])
            if dg is not None:
                check(f'{t2} dgamma', dg, bw['dgamma'] + g0.double(), 1e-5 * bw['dgamma'].abs() + k_w * U32 * (bw['dgamma_terms'] + g0.double().abs()) + bw['dgamma_add_err'])
            if db is not None:
                check(f'{t2} dbeta', db, bw['dbeta'] + b0.double(), 1e-5 * bw['dbeta'].abs() + k_w * U32 * (bw['dbeta_terms'] + b0.double().abs()))
            if da is not None:                              # dadd sums dx: every addend carries the error of its dx
                check(f'{t2} dadd', da, bw['dadd'] + a0.double(), 1e-5 * bw['dadd'].abs() + (k_w + k_b) * U32 * (bw['dadd_terms'] + a0.double().abs()) + bw['dx_add_err'].sum(0))


@pytest.mark.parametrize('B', [1, 2, 63, 64, 65, 130])
@pytest.mark.parametrize('rows,d', [(1, 4), (3, 20), (1, 64), (1, 68), (17, 964), (196, 512)])
def test_layernorm_nd(ops, rows, d, B):
    """(1, 4): one float4, 15 empty splits; (3, 20): 15 float4s, the last split empty; (1, 64): 16, one each; (1, 68): 17 float4s in
    splits of 2, so splits 9 .. 15 start past the end (c1 < c0)"""
    _lnnd_case(ops, B, rows, d)


def test_layernorm_nd_mean_far_from_zero(ops):
    _lnnd_case(ops, 3, 17, 964, far=1e3)


def test_layernorm_nd_fwd_drop(ops):
    B, rows, d = 3, 3, 20
    n, base = rows * d, 12
    x, add, gamma, beta = _lnnd_inputs(B, n, seed=5)
    key, thr, sc = drop_args(21)
    ybuf, y, y_bs = _strided(B, n)
    stats = nans(B, STATS)
    ops.layernorm_nd_fwd(x, add, gamma, beta, y, y_bs, stats, B, rows, d, drop=(1, key, thr, sc), drop_base=base)
    keep = keep_mask(key, B * y_bs, thr, offset=base).view(B, y_bs)[:, :n]          # element (b, i): index b * y_bs + drop_base + i
    r = R.lnnd_fwd(x, add, gamma, beta, keep=keep, keep_scale=sc)
    check('lnnd fwd drop y', ybuf[:B, HEAD:], r['y'], 1e-5 * r['y'].abs() + (_lnnd_k(n) + 1) * U32 * r['amp'])
    assert torch.equal(ybuf[:B, HEAD:][~keep], torch.zeros_like(ybuf[:B, HEAD:][~keep])) and 0 < int((~keep).sum()) < keep.numel()
    assert is_sent(ybuf[:, :HEAD]) and is_sent(ybuf[B:])


@pytest.mark.parametrize('B,rows,d', [(130, 3, 20), (65, 17, 964)])
def test_layernorm_nd_bwd_deterministic(ops, B, rows, d):
    n = rows * d
    x, add, gamma, beta = _lnnd_inputs(B, n, seed=B)
    stats, y, dy = nans(B, STATS), nans(B, n), rnd(B, n, seed=4)
    ops.layernorm_nd_fwd(x, add, gamma, beta, y, n, stats, B, rows, d)

    def run():
        dx, dg, db, da = nans(B, n), torch.zeros(n, device=dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
        ops.layernorm_nd_bwd(dy, n, x, add, gamma, stats, dx, dg, db, da, B, rows, d)
        return dx, dg, db, da
    a, b = deterministic_twice(ops, run)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    bw = R.lnnd_bwd(dy, x, add, gamma, stats[:, 0], stats[:, 1])
    check(f'lnnd deterministic B={B} dgamma', a[1], bw['dgamma'], 1e-5 * bw['dgamma'].abs() + (2 * B + 2) * U32 * bw['dgamma_terms'])


def test_layernorm_nd_refusals(ops):
    B = 2
    x, g, y, stats = rnd(B, 64), rnd(64), nans(B, 64), nans(B, STATS)
    refused(lambda: ops.layernorm_nd_fwd(x, None, g, None, y, 6, stats, B, 1, 6), 'i2t_layernorm_nd_fwd')
    refused(lambda: ops.layernorm_nd_fwd(x, None, g, None, y, 22, stats, B, 1, 20), 'i2t_layernorm_nd_fwd')
    refused(lambda: ops.layernorm_nd_fwd(x, None, g, None, y, 20, stats, B, 1, 20, drop=(1, 5, 50, 1.25), drop_base=2), 'i2t_layernorm_nd_fwd')
    refused(lambda: ops.layernorm_nd_bwd(x, 6, x, None, g, stats, y, None, None, None, B, 1, 6), 'i2t_layernorm_nd_bwd')
    refused(lambda: ops.layernorm_nd_bwd(x, 22, x, None, g, stats, y, None, None, None, B, 1, 20), 'i2t_layernorm_nd_bwd')
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(stats).all()


# ------------------------------------------------------------------------------------------------------------- embedding
VOCAB, NPOS_PAD = 50, 8


def _embed_ids(rows, seed):
    ids = torch.randint(0, VOCAB, (rows,), generator=torch.Generator().manual_seed(seed))
    edge = torch.tensor([VOCAB + 5, -3, VOCAB])             # clamped to vocab - 1, 0, vocab - 1
    ids[:min(rows, 3)] = edge[:min(rows, 3)]
    return ids.to(dev())


@pytest.mark.parametrize('B,T', [(1, 1), (3, 20), (1, 4096 + 3)])
@pytest.mark.parametrize('d', [4, 128, 1028])
def test_embed_fwd(ops, d, B, T):
    rows = B * T
    ids = _embed_ids(rows, seed=rows + d)
    wte, wpe = rnd(VOCAB + 1, d, seed=1), rnd(T + NPOS_PAD + 1, d, seed=2)
    wte[VOCAB], wpe[T + NPOS_PAD] = float('nan'), float('nan')          # the row behind each table: a read of it poisons the output
    pos = torch.randint(0, T, (rows,), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(dev())
    pos[:min(rows, 2)] = T - 1                              # repeats
    tok = ids.clamp(0, VOCAB - 1)
    for with_wpe in (True, False):
        for off in (0, 8):
            for p in (None, pos):
                x = nans(rows + 1, d)
                x[rows:] = SENT
                ops.embed_fwd(ids, wte, wpe if with_wpe else None, x, B, T, d, off, VOCAB, pos=p)
                prow = (p.long() if p is not None else torch.arange(rows, device=dev()) % T) + off
                want = wte[tok] + wpe[prow] if with_wpe else wte[tok]                      # the fp32 sum
                tag = f'embed_fwd d={d} rows={rows} wpe={with_wpe} off={off} pos={p is not None}'
                ref = R.embed_fwd(ids, wte, wpe if with_wpe else None, T, off, VOCAB, p)
                assert torch.equal(x[:rows], want), tag
                assert torch.equal(want, ref.float()), f'{tag}: reference'
                check(tag, x[:rows], ref.float(), 0.0)      # exact: the fp64 sum rounded to fp32
                assert is_sent(x[rows:]), f'{tag}: rows past the last'


def _sob_slices(rows, d, B, cap=32):
    """launch_sum_over_batch's slicing: (slices, batch entries a slice walks)"""
    col_blocks = (rows * (d >> 2) + 255) // 256
    s = 1
    while s < cap and col_blocks * s < 1024 and B // (s * 2) >= 32:
        s *= 2
    return s, (B + s - 1) // s


@pytest.mark.parametrize('mode', ['equal', 'distinct', 'packed', 'dwte_null', 'dwpe_null'])
@pytest.mark.parametrize('B', [3, 64, 131])
def test_embed_bwd(ops, B, mode):
    T, d, off = 5, 128, 8
    rows = B * T
    vocab = rows + 4 if mode == 'distinct' else VOCAB
    if mode == 'equal':
        ids = torch.full((rows,), 7, device=dev())          # every row collides on one address
    elif mode == 'distinct':
        ids = torch.randperm(rows, generator=torch.Generator().manual_seed(B)).to(dev())
    else:
        ids = _embed_ids(rows, seed=B)
    pos = (torch.arange(rows, device=dev()) % 3).to(torch.int32) if mode == 'packed' else None        # repeated positions
    dx = rnd(rows, d, seed=B + 1)
    npos = T + off
    w0, p0 = rnd(vocab + 1, d, seed=2), rnd(npos + 1, d, seed=3)
    w0[vocab], p0[npos] = SENT, SENT
    dwte, dwpe = (None if mode == 'dwte_null' else w0.clone()), (None if mode == 'dwpe_null' else p0.clone())
    ops.embed_bwd(ids, dx, dwte, dwpe, B, T, d, off, vocab, pos=pos)
    r = R.embed_bwd(ids, dx, vocab, npos, T, off, vocab, pos)
    tag = f'embed_bwd B={B} {mode}'
    if dwte is not None:                                    # k: one atomic per row that names the address, onto the start value
        kk = (r['dwte_count'].double() + 1).unsqueeze(1)
        want = r['dwte'] + w0[:vocab].double()
        check(f'{tag} dwte', dwte[:vocab], want, 1e-5 * want.abs() + kk * U32 * (r['dwte_terms'] + w0[:vocab].double().abs()))
        assert is_sent(dwte[vocab:])
        untouched = r['dwte_count'] == 0
        assert torch.equal(dwte[:vocab][untouched], w0[:vocab][untouched]), f'{tag}: a row no id names'
    if dwpe is not None:
        if pos is None:                                     # the sliced sum over the batch: a slice's walk, then one atomic per slice
            s, per = _sob_slices(T, d, B)
            kk = per + s + 1
        else:
            kk = (r['dwpe_count'].double() + 1).unsqueeze(1)
        want = r['dwpe'] + p0[:npos].double()
        check(f'{tag} dwpe', dwpe[:npos], want, 1e-5 * want.abs() + kk * U32 * (r['dwpe_terms'] + p0[:npos].double().abs()))
        assert is_sent(dwpe[npos:]) and torch.equal(dwpe[:off], p0[:off]), f'{tag}: rows outside the positions'


def test_embed_bwd_deterministic(ops):
    B, T, d = 131, 5, 128
    ids, dx = _embed_ids(B * T, seed=1), rnd(B * T, d, seed=2)
    pos = (torch.arange(B * T, device=dev()) % 3).to(torch.int32)

    def run():
        out = []
        for p in (None, pos):
            dwte, dwpe = torch.zeros(VOCAB, d, device=dev()), torch.zeros(T, d, device=dev())
            ops.embed_bwd(ids, dx, dwte, dwpe, B, T, d, 0, VOCAB, pos=p)
            out += [dwte, dwpe]
        return out
    a, b = deterministic_twice(ops, run)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    r = R.embed_bwd(ids, dx, VOCAB, T, T, 0, VOCAB, None)
    check('embed_bwd deterministic dwte', a[0], r['dwte'], 1e-5 * r['dwte'].abs() + (r['dwte_count'].double() + 1).unsqueeze(1) * U32 * r['dwte_terms'])
    check('embed_bwd deterministic dwpe', a[1], r['dwpe'], 1e-5 * r['dwpe'].abs() + (B + 1) * U32 * r['dwpe_terms'])


# --------------------------------------------------------------------------------------------------------- cross entropy
IGNORE = -100
CE_V = [1, 7, 8, 9, 13, 4096, 16384, 16392, 32768, 32775, 32776, 53248, 53255, 53256, 65536, 65543]
# __expf(x) = v_exp_f32(x log2 e): the instruction is accurate to 1 ulp, the product's rounding (2^-24 |x log2 e|) times ln 2 is a
# relative 2^-24 |x|; __logf = v_log_f32 (1 ulp) times ln 2
def expf_rel(arg_abs):
    return 2 * U32 + 0.5 * U32 * arg_abs


def _ce_logits(M, V, ld, seed):
    """row 0, 4: N(0, 4); row 1 constant (lse = z/T + log V); row 2 one +60 among -60s; row 3 all -100.  Pad columns: the sentinel"""
    z = sent(M + 1, ld, dtype=BF16)
    z[:M, :V] = rnd(M, V, seed=seed, scale=2.0, dtype=BF16)
    z[1, :V] = 1.75
    z[2, :V] = -60.0
    z[2, V // 2] = 60.0
    z[3, :V] = -100.0
    return z


def _ce_labels(V, variant):
    tail = V - 1 - (V & 7) // 2 if V & 7 else max(V - 3, 0)      # inside the V & 7 tail where there is one
    if variant == 0:
        lab, w = [0, V - 1, V // 2, IGNORE, -5], [0.3, 0.2, 0.25, 0.4, 0.15]             # row 2: the label on the +60 column (p - 1 cancels)
    else:
        lab, w = [V, V + 3, V // 2, tail, V - 1], [0.3, 0.2, 0.0, 0.25, 0.15]            # row 2: live, with w == 0; row 3 (all -100): live
    return torch.tensor(lab, device=dev()), torch.tensor(w, device=dev())


def _ce_tols(r, V):
    # lse = bm + log(bs): bs sums V exponentials -- a thread's chain (V / 512 threads), the wave and workgroup trees (6 + 8) -- each with
    # the relative error of its exp: the rounding of its argument, 2^-23 (|z/T| + |lse|), plus __expf's own; the log turns the
    # relative error of bs into an absolute one; + __logf, + the final add (2^-23 |lse| each)
    k_s = (V + 511) // 512 + 14
    arg = r['arg'].amax(-1)
    lse_abs = (k_s + 2) * U32 + U32 * arg + expf_rel(arg) + 2 * U32 * r['lse'].abs()
    lse_abs = torch.where(r['live'], lse_abs, torch.zeros_like(lse_abs))
    tol_lse = 1e-5 * r['lse'].abs() + lse_abs
    # the gradient coef (p - onehot), bf16: p = exp(z/T - lse) carries the absolute error of the fp32 lse and of its own argument as a
    # relative error, plus __expf's; 3 more roundings to the product; a p below 2^-126 is flushed to zero
    p_rel = lse_abs[:, None] + U32 * r['arg'] + expf_rel(r['arg'])
    a_grad = r['coef'].abs() * r['p'] * p_rel + 3 * U32 * r['gterms'] + TINY * r['coef'].abs()
    return tol_lse, lse_abs, E7 * r['grad'].abs() + a_grad


def _ce_case(ops, V, one_pass):
    M = 5
    ld0 = (V + 7) // 8 * 8
    runs = [(1.0, ld0, 0, 1.0), (1 / 0.7, ld0 + 8, 1, 0.5), (0.5, ld0, 1, 3.1), (1.0, ld0 + 8, 1, 3.1), (1 / 0.7, ld0, 0, 1.0), (0.5, ld0 + 8, 0, 0.5)]
    for inv_temp, ld, variant, gscale in runs:
        z0 = _ce_logits(M, V, ld, seed=V + ld)
        labels, w = _ce_labels(V, variant)
        start = 1.5
        tag = f'ce V={V} ld={ld} 1/T={inv_temp:.3f} labels={variant} g={gscale}'
        r1 = R.ce(z0[:M], V, labels, w, inv_temp, IGNORE)
        rg = R.ce(z0[:M], V, labels, w, inv_temp, IGNORE, gscale=gscale)
        tol_lse, lse_abs, tol_grad1 = _ce_tols(r1, V)
        _, _, tol_gradg = _ce_tols(rg, V)
        # the loss: one atomic per live row onto the start (k = M + 3 with the product and the subtraction), each term with the error of its lse
        tol_loss = 1e-5 * (r1['loss'] + start).abs() + (M + 3) * U32 * (r1['loss_abs'] + start) + (w.double().abs() * lse_abs).sum()
        dead = ~r1['live']
        assert int(dead.sum()) == 2 and (r1['lse'][dead] == 0).all()
        # two-pass form: gscale through the device scalar
        z, lse, loss = z0.clone(), nans(M + 1), torch.tensor([start, SENT], device=dev())
        lse[M:] = SENT
        ops.ce_fwd(z[:M], ld, labels, w, inv_temp, IGNORE, lse, loss, M, V)
        assert torch.equal(z.view(I16), z0.view(I16)), f'{tag}: ce_fwd wrote the logits'
        check(f'{tag} two-pass lse', lse[:M], r1['lse'], tol_lse)
        check(f'{tag} two-pass loss', loss[0], r1['loss'] + start, tol_loss)
        assert float(loss[1]) == SENT and is_sent(lse[M:]) and torch.equal(lse[:M][dead], torch.zeros_like(lse[:M][dead]))
        gs = torch.tensor([gscale, SENT], device=dev())
        ops.ce_bwd(z[:M], ld, labels, w, inv_temp, IGNORE, lse, gs, M, V)
        check(f'{tag} two-pass grad', z[:M, :V], rg['grad'], tol_gradg)
        assert torch.equal(z[:M, V:].view(I16), z0[:M, V:].view(I16)) and torch.equal(z[M:].view(I16), z0[M:].view(I16)), f'{tag}: pad columns / rows past M (two-pass)'
        assert torch.equal(z[:M, :V][dead], torch.zeros_like(z[:M, :V][dead])), f'{tag}: dead rows (two-pass)'
        if variant == 1:
            assert torch.equal(z[2, :V], torch.zeros_like(z[2, :V])), f'{tag}: the w == 0 row'
            assert bool(r1['live'][3]) and float(w[3]) > 0 and (V == 1 or float(rg['grad'][3].abs().max()) > 0), f'{tag}: the all -100 row must be live'
        if not one_pass:
            continue
        z1, lse1, loss1 = z0.clone(), nans(M + 1), torch.tensor([start, SENT], device=dev())
        lse1[M:] = SENT
        ops.ce_fwd_bwd(z1[:M], ld, labels, w, inv_temp, IGNORE, lse1, loss1, M, V)
        check(f'{tag} one-pass lse', lse1[:M], r1['lse'], tol_lse)
        check(f'{tag} one-pass loss', loss1[0], r1['loss'] + start, tol_loss)
        check(f'{tag} one-pass grad', z1[:M, :V], r1['grad'], tol_grad1)
        assert float(loss1[1]) == SENT and is_sent(lse1[M:])
        assert torch.equal(z1[:M, V:].view(I16), z0[:M, V:].view(I16)) and torch.equal(z1[M:].view(I16), z0[M:].view(I16)), f'{tag}: pad columns / rows past M (one-pass)'
        assert torch.equal(z1[:M, :V][dead], torch.zeros_like(z1[:M, :V][dead])) and torch.equal(lse1[:M][dead], torch.zeros_like(lse1[:M][dead]))
        # one-pass against two-pass at gscale 1.  Both evaluate coef (__expf(z/T - lse) - onehot) with coef = w/T, but not bit for bit:
        # (1) the streaming ce_bwd and the body of the one-pass kernel contract z * (1/T) - lse into one fma (the product un-rounded),
        # while the one-pass kernel's V & 7 tail keeps the ROUNDED product it took the maximum of, so the argument differs by up to
        # 2^-24 |z/T| (seen at V = 1 and V = 7 on the MI355X: the label column of a one-hot row gave 0 against coef x 1.9e-6);
        # (2) the two forms sum the exponentials in different orders, so a row's lse may differ in its last bits.  Either moves p by
        # the relative 2^-23 (|z/T| + |lse|) the bound already carries, visible where p - onehot cancels, or flips one bf16 rounding
        z2 = z0.clone()
        ops.ce_bwd(z2[:M], ld, labels, w, inv_temp, IGNORE, lse, torch.ones(1, device=dev()), M, V)
        differ = int((z2[:M, :V].view(I16) != z1[:M, :V].view(I16)).sum())
        print(f'DIFFER {tag}: {differ} of {M * V} elements')
        check(f'{tag} one-pass vs two-pass grad', z1[:M, :V], z2[:M, :V].double(),
              E7 * r1['grad'].abs() + r1['coef'].abs() * r1['p'] * (U32 * r1['arg'] + (lse[:M].double() - lse1[:M].double()).abs()[:, None]) + TINY * r1['coef'].abs())
        # the upstream gradient afterwards: scale_bf16 on the whole buffer (pad columns scale with it)
        ops.scale_bf16(z1[:M], M * ld, gs)
        # two bf16 roundings (the un-scaled gradient, then its product with gscale), half an ulp = 2^-8 each: (1 + 2^-8)^2 - 1 <=
        # 2^-7 (1 + 2^-8) relative; tol_gradg holds the 2^-7 |ref| and the absolute part, which the exact scaling carries along
        check(f'{tag} one-pass + scale_bf16', z1[:M, :V], rg['grad'], tol_gradg + E7 * 2.0 ** -8 * rg['grad'].abs())
        assert float(gs[1]) == SENT and torch.equal(z1[M:].view(I16), z0[M:].view(I16))


@pytest.mark.parametrize('V', CE_V)
def test_ce_one_pass_and_two_pass(ops, V):
    """nch = ceil((V >> 3) / 512) picks the instantiation: <4,8> up to V = 16391, <8,8> 16392 .. 32775, <13,6> 32776 .. 53255, <16,4>
    from 53256; the listed V sit on both sides of every boundary and on the V & 7 tails"""
    _ce_case(ops, V, one_pass=True)


def test_ce_two_pass_past_the_one_pass_limit(ops):
    _ce_case(ops, 70001, one_pass=False)


def test_ce_one_pass_refuses_65544_columns(ops):
    M, V = 2, 65544
    z = rnd(M, V, seed=1, dtype=BF16)
    z0 = z.clone()
    labels, w = torch.tensor([0, 5], device=dev()), torch.ones(M, device=dev())
    lse, loss = nans(M), nans(1)
    refused(lambda: ops.ce_fwd_bwd(z, V, labels, w, 1.0, IGNORE, lse, loss, M, V), 'one-pass')
    refused(lambda: ops.ce_fwd_bwd(z, V - 4, labels, w, 1.0, IGNORE, lse, loss, M, V - 4), 'i2t_ce_fwd_bwd')       # ld % 8
    torch.cuda.synchronize()
    assert torch.equal(z.view(I16), z0.view(I16)) and torch.isnan(lse).all() and torch.isnan(loss).all()


@pytest.mark.parametrize('tail', range(8))
def test_scale_bf16(ops, tail):
    for n in (tail, 4096 + tail, 2048 * 256 * 8 + 8 * 3 + tail):          # the last: one trip past the 2048-workgroup cap
        if n == 0:
            continue
        x = rnd(n + 8, seed=n % 9973, scale=3.0, dtype=BF16)
        x[n:] = SENT
        x0 = x.clone()
        ops.scale_bf16(x, n, torch.ones(1, device=dev()))
        assert torch.equal(x.view(I16), x0.view(I16)), f'scale_bf16 n={n}: the scale-1 launch changed the buffer'
        for sc in (0.5, 3.1):
            x = x0.clone()
            ops.scale_bf16(x, n, torch.tensor([sc], device=dev()))
            ref = R.scale_bf16(x0[:n], sc)
            check(f'scale_bf16 n={n} x{sc}', x[:n], ref, E7 * ref.abs())
            assert torch.equal(x[:n], (x0[:n].float() * np.float32(sc)).to(BF16)) and is_sent(x[n:])


# --------------------------------------------------------------------------------------------------- gradient normaliser
GN_BIG = 4 * 4 * 256 * 1024 + 3                             # past the 1024-workgroup cap, into the 4-way unrolled loop


def _sumsq_k(n, det=False):
    """operations behind sum(g^2), all terms positive: a thread's chain (product + add per element), the workgroup trees, one atomic
    per workgroup"""
    grid = 1 if det else min(1024, max(1, ((n >> 2) + 255) // 256))
    return 2 * 4 * (((n >> 2) + grid * 256 - 1) // (grid * 256)) + 2 + 10 + grid


def _gn_buffers(n, scale, seed, zero=False):
    g = rnd(n + 4, seed=seed, scale=scale)
    if zero:
        g[:] = 0.0
    g[n:] = SENT
    return g


@pytest.mark.parametrize('scale', [0.0, 1e-6, 1.0, 1e4])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, GN_BIG])
def test_grad_normalize(ops, n, scale):
    g0 = _gn_buffers(n, scale, seed=n % 9973, zero=scale == 0.0)
    key, thr, sc = drop_args(n % 97)
    keep = keep_mask(key, n, thr)
    k = _sumsq_k(n) // 2 + 4                                # sqrt halves the sum's relative error; sqrtf, + 1e-6, the reciprocal, the product
    plain = R.grad_normalize(g0[:n])
    tol = 1e-5 * plain['g'].abs() + k * U32 * plain['g'].abs()
    tag = f'grad_normalize n={n} scale={scale}'
    outs = {}
    for name, kw in (('plain', {}), ('bf16', dict(bf=True)), ('drop', dict(bf=True, drop=True)), ('presummed', dict(bf=True, pres=True)),
                     ('keep_f32', dict(bf=True, keepf=True)), ('keep_f32+drop+clear', dict(bf=True, keepf=True, drop=True, clear=True, pres=True))):
        g = g0.clone()
        gb = nans(n + 4, dtype=BF16) if kw.get('bf') else None
        if gb is not None:
            gb[n:] = SENT
        ws = torch.tensor([float('nan'), SENT], device=dev())
        if kw.get('pres'):
            ops.sumsq(g[:n], ws)
        clear = torch.tensor([5.0, SENT], device=dev()) if kw.get('clear') else None
        ops.grad_normalize(g[:n], ws, gb, bf16_drop=(1, key, thr, sc) if kw.get('drop') else None, presummed=bool(kw.get('pres')),
                           clear_after=clear, keep_f32=bool(kw.get('keepf')))
        t = f'{tag} {name}'
        assert is_sent(g[n:]) and float(ws[1]) == SENT, f'{t}: past n'
        check(f'{t} ws', ws[0], plain['g'].new_tensor(float(g0[:n].double().pow(2).sum())), (1e-5 + _sumsq_k(n) * U32) * float(g0[:n].double().pow(2).sum()))
        if kw.get('keepf'):
            assert torch.equal(g.view(torch.int32), g0.view(torch.int32)), f'{t}: keep_f32 touched g'
        else:
            check(f'{t} g', g[:n], plain['g'], tol)
            outs[name] = g
        if scale == 0.0:
            assert torch.equal(g[:n], torch.zeros_like(g[:n]))
        if gb is not None:
            ref = R.grad_normalize(g0[:n], keep=keep if kw.get('drop') else None, keep_scale=sc)['g_bf16']
            check(f'{t} g_bf16', gb[:n], ref, E7 * ref.abs() + tol * (R.f32(sc) if kw.get('drop') else 1.0))
            assert is_sent(gb[n:])
            gn = g[:n] if not kw.get('keepf') else outs['plain'][:n]
            want = torch.where(keep, gn * np.float32(sc), torch.zeros_like(gn)) if kw.get('drop') else gn
            if not kw.get('keepf') or (n <= 1024 and not kw.get('pres')):          # (across launches only where one workgroup sums: the atomics of several land in any order)
                assert torch.equal(gb[:n], want.to(BF16)), f'{t}: the bf16 copy is not the rounded (masked) result'
            if kw.get('drop'):
                assert torch.equal(gb[:n][~keep], torch.zeros_like(gb[:n][~keep])), f'{t}: a dropped element'
        if clear is not None:
            assert clear.tolist() == [0.0, SENT]


@pytest.mark.parametrize('n', [1020, 1021, 1022, 1023, 2052, 2053, 2054, 2055])
def test_grad_normalize_drop_tail_matches_body(ops, n):
    """the n & 3 tail takes its keep decision from dropout_keep, the body from dropout_keep4: one mask over the whole tensor"""
    g0 = _gn_buffers(n, 1.0, seed=n)
    g0[:n] = g0[:n].abs() + 0.5                             # no zero: the kept pattern is readable from the output
    key, thr, sc = drop_args(n, p=0.5)
    keep = keep_mask(key, n, thr)
    g, gb, ws = g0.clone(), nans(n + 4, dtype=BF16), nans(1)
    gb[n:] = SENT
    ops.grad_normalize(g[:n], ws, gb, bf16_drop=(1, key, thr, sc))
    assert torch.equal(gb[:n] != 0, keep), f'n={n}: kept pattern'
    assert torch.equal(gb[:n], torch.where(keep, g[:n] * np.float32(sc), torch.zeros_like(g[:n])).to(BF16)) and is_sent(gb[n:])
    ref = R.grad_normalize(g0[:n], keep=keep, keep_scale=sc)['g_bf16']
    check(f'grad_normalize drop tail n={n}', gb[:n], ref, E7 * ref.abs() + (_sumsq_k(n) // 2 + 5) * U32 * ref.abs())


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, GN_BIG])
def test_sumsq_accumulate(ops, n):
    g = _gn_buffers(n, 3.0, seed=n % 9973)
    g[n:] = float('nan')                                    # a read past n poisons the sum
    for start, acc in ((float('nan'), False), (2.5, True)):
        ws = torch.tensor([start, SENT], device=dev())
        ops.sumsq(g[:n], ws, accumulate=acc)
        want = R.sumsq(g[:n], start=2.5 if acc else None)
        check(f'sumsq n={n} accumulate={acc}', ws[0], want, (1e-5 + (_sumsq_k(n) + 1) * U32) * want)
        assert float(ws[1]) == SENT


def test_grad_normalize_deterministic(ops):
    n = GN_BIG
    g0 = _gn_buffers(n, 1.0, seed=5)

    def run():
        g, ws, gb = g0.clone(), nans(1), nans(n, dtype=BF16)
        ops.grad_normalize(g[:n], ws, gb)
        s2 = torch.tensor([2.5], device=dev())
        ops.sumsq(g0[:n], s2, accumulate=True)
        return g, ws, gb, s2
    a, b = deterministic_twice(ops, run)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    ref = R.grad_normalize(g0[:n])['g']
    check('grad_normalize deterministic g', a[0][:n], ref, (1e-5 + (_sumsq_k(n, det=True) // 2 + 4) * U32) * ref.abs())


# ----------------------------------------------------------------------------------------------------------------- AdamW
B1, B2, EPS = 0.9, 0.999, 1e-8
SEGMENTS = {1: ([1528], [3e-3], [0.1]),
            2: ([1000, 520], [3e-3, -1.0], [0.1, 0.0]),
            7: ([8, 1000, 520, 2048, 64, 8, 256], [1e-2, 3e-3, -1.0, 0.0, 1e-3, -1.0, 3e-3], [0.1, 0.0, 0.1, 0.1, 0.0, 0.0, 0.1])}


def _adamw_check(tag, ops, p, g, m, v, pb, ends, lrs, wds, step, gscale):
    """one launch against the reference evaluated from the state the launch starts from; frozen segments: bit-untouched"""
    n = p.numel()
    p0, m0, v0, pb0 = p.clone(), m.clone(), v.clone(), None if pb is None else pb.clone()
    dv = lambda xs, dt: torch.tensor(xs, dtype=dt, device=dev())
    ops.adamw_step(p, g, m, v, pb, n, dv(ends, torch.long), dv(lrs, F32), dv(wds, F32), len(ends), B1, B2, EPS, step, grad_scale=gscale)
    r = R.adamw(p0, g, m0, v0, ends, lrs, wds, B1, B2, EPS, step, grad_scale=gscale)
    b1, b2 = R.f32(B1), R.f32(B2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    # m: the scaled gradient, two products, (1 - beta1), the add: 5.  v: one product more: 6
    tol_m = 1e-5 * r['m'].abs() + 5 * U32 * r['m_terms']
    tol_v = 1e-5 * r['v'].abs() + 6 * U32 * r['v_terms']
    # p: the decay factor and product (3), the step lr / bc1 * m / (sqrt(v) / bc2s + eps) (7 operations), the subtraction; the step also
    # carries the relative errors of m, of sqrt(v) (half of v's) and of the two bias corrections, computed in fp32 on the host: powf to
    # 1 ulp and the subtraction from 1 leave 2^-23 absolute on 1 - beta^step, i.e. 2^-23 / (1 - beta^step) relative (halved by the root)
    rel = tol_m / r['m'].abs().clamp_min(1e-300) + 0.5 * tol_v / r['v'].abs().clamp_min(1e-300) * (r['sqrt_vhat'] / (r['sqrt_vhat'] + r['eps']))
    tol_p = 1e-5 * r['p'].abs() + 4 * U32 * r['p_terms'] + r['upd'] * (8 * U32 + U32 / bc1 + 0.5 * U32 / bc2 + rel)
    live = ~r['frozen']
    for name, got, tol in (('p', p, tol_p), ('m', m, tol_m), ('v', v, tol_v)):
        check(f'{tag} {name}', got[live], r[name][live], tol[live])
    fz = r['frozen']
    assert torch.equal(p[fz], p0[fz]) and torch.equal(m[fz], m0[fz]) and torch.equal(v[fz], v0[fz]), f'{tag}: a frozen segment changed'
    if pb is not None:
        assert torch.equal(pb[live], p[live].to(BF16)), f'{tag}: the bf16 shadow is not the rounded p'
        assert torch.equal(pb[fz].view(I16), pb0[fz].view(I16)), f'{tag}: the shadow of a frozen segment changed'
    lr_el = torch.tensor([R.f32(x) for x in lrs], device=dev())[torch.bucketize(torch.arange(n, device=dev()), dv(ends, torch.long), right=True)]
    assert torch.equal(p[lr_el == 0], p0[lr_el == 0]), f'{tag}: lr == 0 moved the parameters'
    return r


def _adamw_arena(n, seed, state='zero'):
    p = rnd(n, seed=seed)
    if state == 'zero':
        m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    else:
        m, v = rnd(n, seed=seed + 1, scale=0.1), rnd(n, seed=seed + 2, scale=0.1).pow(2)
    return p, m, v


def _set_frozen_sentinels(ends, lrs, *tensors):
    lo = 0
    for e, lr in zip(ends, lrs):
        if lr < 0:
            for t in tensors:
                if t is not None:
                    t[lo:e] = SENT
        lo = e


@pytest.mark.parametrize('with_bf', [True, False])
@pytest.mark.parametrize('gscale', [1.0, 1.0 / 64])
@pytest.mark.parametrize('nseg', [1, 2, 7])
def test_adamw_three_steps(ops, nseg, gscale, with_bf):
    sizes, lrs, wds = SEGMENTS[nseg]
    ends = np.cumsum(sizes).tolist()
    n = ends[-1]
    p, m, v = _adamw_arena(n, seed=nseg)
    pb = p.to(BF16) if with_bf else None
    _set_frozen_sentinels(ends, lrs, p, m, v, pb)
    for step in (1, 2, 3):
        g = rnd(n, seed=10 + step, scale=4.0 / gscale)
        g[40:120] = 0.0                                     # a range with zero gradient on zero state: no NaN, the decay alone
        _adamw_check(f'adamw nseg={nseg} g x{gscale:.4f} bf={with_bf} step {step}', ops, p, g, m, v, pb, ends, lrs, wds, step, gscale)
    if lrs[ends.index(next(e for e in ends if e > 40))] >= 0:
        assert torch.equal(m[40:120], torch.zeros_like(m[40:120])) and torch.equal(v[40:120], torch.zeros_like(v[40:120]))
    if nseg == 7:
        s = slice(ends[2], ends[3])                         # lr == 0: the moments advance
        assert float(m[s][120:].abs().min()) > 0 and float(v[s][120:].min()) > 0


@pytest.mark.parametrize('step', [1, 2, 1000, 100000])
def test_adamw_single_step_from_random_state(ops, step):
    sizes, lrs, wds = SEGMENTS[7]
    ends = np.cumsum(sizes).tolist()
    p, m, v = _adamw_arena(ends[-1], seed=step % 97, state='random')
    pb = p.to(BF16)
    _set_frozen_sentinels(ends, lrs, p, m, v, pb)
    _adamw_check(f'adamw step={step}', ops, p, rnd(ends[-1], seed=3, scale=2.0), m, v, pb, ends, lrs, wds, step, 1.0)


def test_adamw_grid_stride(ops):
    n = 4096 * 256 * 4 + 8                                  # two float4s past the 4096-workgroup cap; the last 8 elements frozen
    ends, lrs, wds = [n - 8, n], [3e-3, -1.0], [0.1, 0.0]
    p, m, v = _adamw_arena(n, seed=4, state='random')
    pb = p.to(BF16)
    _set_frozen_sentinels(ends, lrs, p, m, v, pb)
    _adamw_check('adamw grid stride', ops, p, rnd(n, seed=5), m, v, pb, ends, lrs, wds, 5, 1.0)


def test_adamw_refusals(ops):
    p, m, v = _adamw_arena(16, seed=1)
    p0 = p.clone()
    g = rnd(16)
    t = lambda xs, dt: torch.tensor(xs, dtype=dt, device=dev())
    refused(lambda: ops.adamw_step(p, g, m, v, None, 10, t([10], torch.long), t([1e-3], F32), t([0.0], F32), 1, B1, B2, EPS, 1), 'i2t_adamw_step')
    refused(lambda: ops.adamw_step(p, g, m, v, None, 16, t([16], torch.long), t([1e-3], F32), t([0.0], F32), 1, B1, B2, EPS, 0), 'i2t_adamw_step')
    torch.cuda.synchronize()
    assert torch.equal(p, p0)


# ------------------------------------------------------------------------------------------ dropout and the strided helpers
def _dropout_want(x0, rows, cols, mode, key, thr, sc):
    if mode == 1:
        keep = keep_mask(key, rows * cols, thr).view(rows, cols)
    else:
        keep = torch.stack([keep_mask((key + t) & 0xFFFFFFFF, rows, thr) for t in range(3)], 1).repeat_interleave(cols // 3, dim=1)
    f = torch.where(keep, torch.full((rows, cols), np.float32(sc), device=dev()), torch.zeros(rows, cols, device=dev()))
    return (x0.float() * f).to(x0.dtype), keep


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('rows,cols', [(5, 4), (5, 12), (5, 768), (2731, 768)])          # the last: one trip past the 2048-workgroup cap
def test_dropout_apply(ops, rows, cols, mode, dtype):
    from image2text_amd import rng
    if mode == 2 and cols % 12:
        x = rnd(rows, cols, dtype=dtype)
        x0 = x.clone()
        refused(lambda: ops.dropout_apply(x, rows, cols, (2, 1, 26, 1.1)), 'i2t_dropout_apply')
        assert torch.equal(x, x0)
        return
    key = rng.site_key(rows * cols, mode)
    for thr in (0, 1, 26, 255, 256):                        # both ends: nothing dropped (thr 0), everything (256)
        sc = rng.scale(thr)
        buf = rnd(rows * cols + 8, seed=cols + thr, dtype=dtype)
        buf[rows * cols:] = SENT
        x = buf[:rows * cols].view(rows, cols)
        x0 = x.clone()
        ops.dropout_apply(x, rows, cols, (mode, key, thr, sc))
        want, keep = _dropout_want(x0, rows, cols, mode, key, thr, sc)
        tag = f'dropout_apply {rows}x{cols} mode={mode} {dtype} thr={thr}'
        assert torch.equal(x, want), tag
        ref = R.dropout(x0, keep, sc)
        check(tag, x, ref, (E7 if dtype == BF16 else U32) * ref.abs())
        assert is_sent(buf[rows * cols:]), f'{tag}: past the tensor'
        if thr == 0:
            assert keep.all()
        if thr == 256:
            assert not keep.any() and torch.equal(x, torch.zeros_like(x))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('rows,d', [(1, 4), (5, 13108)])    # 5 x 13108 = 65536 + 4 elements: one float4 past the 64-workgroup cap
def test_bcast_and_copy_rows(ops, rows, d, B):
    n = rows * d
    src = rnd(rows, d, seed=n)
    ybuf, y, y_bs = _strided(B, n)
    ops.bcast_rows(src, y, y_bs, B, rows, d)
    assert torch.equal(ybuf[:B, HEAD:], src.view(1, n).expand(B, n)) and is_sent(ybuf[:, :HEAD]) and is_sent(ybuf[B:]), 'bcast_rows'
    key, thr, sc = drop_args(n + B)
    ybuf, y, y_bs = _strided(B, n)
    ops.bcast_rows(src, y, y_bs, B, rows, d, drop=(1, key, thr, sc))
    keep = keep_mask(key, B * y_bs, thr).view(B, y_bs)[:, :n]            # index b * y_bs + i: the rows head their slab
    want = torch.where(keep, src.view(1, n) * np.float32(sc), torch.zeros(B, n, device=dev()))
    assert torch.equal(ybuf[:B, HEAD:], want) and is_sent(ybuf[:, :HEAD]) and is_sent(ybuf[B:]), 'bcast_rows drop'
    check(f'bcast_rows drop {rows}x{d} B={B}', ybuf[:B, HEAD:], R.dropout(src.view(1, n).expand(B, n), keep, sc), U32 * want.double().abs())
    xbuf, x, x_bs = _strided(B, n, fill=rnd(B, n, seed=n + 1))
    for dt in (F32, BF16):
        ybuf = sent(B + 1, 2 * HEAD + n, dtype=dt)
        ops.copy_rows(x, x_bs, ybuf.view(-1)[2 * HEAD:], 2 * HEAD + n, B, rows, d)
        assert torch.equal(ybuf[:B, 2 * HEAD:], xbuf[:B, HEAD:].to(dt)) and is_sent(ybuf[:, :2 * HEAD]) and is_sent(ybuf[B:]), f'copy_rows {dt}'
        ref = xbuf[:B, HEAD:].double()
        check(f'copy_rows {rows}x{d} B={B} {dt}', ybuf[:B, 2 * HEAD:], ref, E7 * ref.abs() if dt == BF16 else 0.0)


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('B', [1, 3, 5, 63, 64, 131, 2048])
def test_sum_over_batch(ops, B, accumulate):
    rows, d = 5, 64
    n = rows * d
    xbuf = nans(B, HEAD + n)                                # NaN between the slabs: a read of a gap poisons the sum
    xbuf[:, HEAD:] = rnd(B, n, seed=B)
    dst0 = rnd(rows + 1, d, seed=1)
    dst0[rows:] = SENT
    if not accumulate:
        dst0[:rows] = float('nan')
    dst = dst0.clone()
    ops.sum_over_batch(xbuf.view(-1)[HEAD:], HEAD + n, dst, B, rows, d, accumulate=accumulate)
    ref, terms = R.sum_over_batch(xbuf[:, HEAD:].view(B, rows, d), start=dst0[:rows] if accumulate else None)
    s, per = _sob_slices(rows, d, B)
    assert s == {2048: 32, 131: 4, 64: 2}.get(B, 1)
    check(f'sum_over_batch B={B} accumulate={accumulate}', dst[:rows], ref, 1e-5 * ref.abs() + (per + s + 1) * U32 * terms)       # a slice's walk, one atomic per slice, the start
    assert is_sent(dst[rows:])


def test_sum_over_batch_deterministic(ops):
    B, rows, d = 2048, 5, 64
    x = rnd(B, rows * d, seed=2)

    def run():
        dst = nans(rows, d)
        ops.sum_over_batch(x, rows * d, dst, B, rows, d)
        return dst
    a, b = deterministic_twice(ops, run)
    assert torch.equal(a, b)
    ref, terms = R.sum_over_batch(x.view(B, rows, d))
    check('sum_over_batch deterministic', a, ref, 1e-5 * ref.abs() + (B + 1) * U32 * terms)


@pytest.mark.parametrize('tail', range(4))
def test_add(ops, tail):
    for n in (tail, 1024 + tail, 2048 * 256 * 4 + 12 + tail):
        if n == 0:
            continue
        dst, src = rnd(n + 4, seed=n % 9973), rnd(n + 4, seed=n % 9973 + 1)
        dst[n:] = SENT
        dst0 = dst.clone()
        ops.add_(dst[:n], src[:n])
        assert torch.equal(dst[:n], dst0[:n] + src[:n]) and is_sent(dst[n:]), f'add n={n}'
        check(f'add n={n}', dst[:n], dst0[:n].double() + src[:n].double(), U32 * (dst0[:n].double().abs() + src[:n].double().abs()))


@pytest.mark.parametrize('tail', range(8))
def test_cast_f32_bf16(ops, tail):
    special = torch.tensor([0.0, -0.0, float('inf'), float('-inf'), float('nan'), 1e-40, -1e-40, 3.4028234663852886e38, -3.4028234663852886e38,
                            1.00390625, 1.01171875, -1.00390625, 1.0039062, 1.0039063, 2.0 ** -126, 2.0 ** -133], device=dev())        # ties to even both ways and their neighbours
    for n in (tail, 2048 + tail, 2048 * 256 * 8 + 8 * 5 + tail):
        if n == 0:
            continue
        src = rnd(n, seed=n % 9973, scale=10.0)
        k = min(n, special.numel())
        src[n - k:] = special[:k]                           # in the tail and the last full vector
        src[:k] = special[:k]
        dst = nans(n + 8, dtype=BF16)
        dst[n:] = SENT
        ops.cast_f32_bf16(src, dst, n)
        want = src.to(BF16)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(dst[:n]), nan) and torch.equal(dst[:n][~nan].view(I16), want[~nan].view(I16)), f'cast n={n}'
        assert is_sent(dst[n:])
        fin = torch.isfinite(want)                          # (the largest finite fp32 rounds to inf, as torch's cast does)
        ref = src[fin].double()
        check(f'cast_f32_bf16 n={n}', dst[:n][fin], ref, E7 * ref.abs() + 2.0 ** -134)       # one rounding; half a bf16 subnormal step


@pytest.mark.parametrize('N', [8, 200])
@pytest.mark.parametrize('M', [1, 100, 5000])
def test_colsum(ops, M, N):
    ld = N + 8
    x = sent(M + 1, ld, dtype=BF16)
    x[:M, :N] = rnd(M, N, seed=M + N, dtype=BF16)
    x[:M, N:] = float('nan')                                # a read of a pad column poisons the sum
    col_blocks = (N + 511) // 512
    splits = max(1, min((M + 63) // 64, 512 // col_blocks))
    k = ((M + splits - 1) // splits + 3) // 4 + 3 + splits + 2       # a wave's rows, the 4-wave sum, one atomic per workgroup, the factor, the start
    ss = torch.tensor([7.5], device=dev())
    for acc, asq in ((False, None), (True, None), (False, ss), (True, ss)):
        out0 = rnd(N + 1, seed=3)
        out0[N:] = SENT
        if not acc:
            out0[:N] = float('nan')
        out = out0.clone()
        ops.colsum(x[:M], out, M, N, ld=ld, accumulate=acc, alpha_sumsq=asq)
        ref, terms = R.colsum(x[:M], N, start=out0[:N] if acc else None, alpha_sumsq=asq)
        check(f'colsum M={M} N={N} accumulate={acc} alpha_sumsq={asq is not None}', out[:N], ref, 1e-5 * ref.abs() + (k + (3 if asq is not None else 0)) * U32 * terms)
        assert is_sent(out[N:])
