"""ops.gemm_dw_colsum (include/i2t.h::i2t_gemm_dw_colsum_bf16): a linear layer's weight gradient C += f A^T . B and, from the same launch,
its bias gradient colsum[m] += f sum_k A[k][m], against float64 on the SAME bf16 operands.  In the GEMM's naming (M, N, K) = (layer N,
layer K, rows); A = dY [K, M], B = x [K, N].

Tolerance (the per-element rule of tests/test_row_kernels_gpu.py, fp32 outputs):
    |got - ref| <= 1e-5 |ref| + k 2^-23 sum|terms|
``terms``: the value the output held before the call and every addend of the sum (products a b f for C, a f for the column sums).
``k``: the addends on the longest fp32 path -- the K steps (64 rows each: the MFMA adds a step's exact products in fp32) of one
workgroup's K slice, then one float atomic per slice onto the value already there: k = steps per slice + slices, both restated from the
launch rule of csrc/gemm_route.h::dw_plan.  Outputs start from a non-zero pattern (the calls accumulate); the floats behind
colsum[M], the pad columns of C and the pad columns of dY hold sentinels / junk: what must not be written is compared bit for bit."""
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U32 = 2.0 ** -23
SENT = -7.75
GUARD = 24


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def check(name, got, ref, tol):
    got, ref, tol = got.detach().to(F64), ref.detach().to(F64), tol.to(F64)
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs()
    units = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = float(units.max())
    print(f'UNITS {name}: {worst:.4f}')
    bad = err > tol
    assert not bad.any(), f'{name}: {int(bad.sum())}/{bad.numel()} out of tolerance, worst {worst:.2f} x the bound'
    return worst


def path_len(M, N, K):
    """(K steps of one slice) + (slices): dw_plan's split of ceil(K / 64) K-tiles over the CUs the output tiles leave idle"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles, nk_all = ((M + 255) // 256) * ((N + 255) // 256), (K + 63) // 64
    per = max(8, ((nk_all + n_cu // tiles - 1) // (n_cu // tiles) + 1) & ~1)
    return per + (nk_all + per - 1) // per


def make_case(M, N, K, seed, with_sumsq=False):
    g = torch.Generator(device=dev()).manual_seed(seed)
    lda, ldb, ldc = M + 8, N + 8, N + 4
    dy = (torch.randn(K, lda, generator=g, device=dev()) * 0.5).to(BF16)
    dy[:, M:] = 3.0                                  # junk in the pad columns: rows >= M of the last row tile read it
    x = torch.randn(K, ldb, generator=g, device=dev()).to(BF16)
    c0 = torch.randn(M, ldc, generator=g, device=dev()) * 4.0
    c0[:, N:] = SENT
    cs0 = torch.randn(M + GUARD, generator=g, device=dev()) * 4.0
    cs0[M:] = SENT
    sumsq = torch.tensor([float(K) * M * 0.37], dtype=F32, device=dev()) if with_sumsq else None
    return SimpleNamespace(M=M, N=N, K=K, dy=dy, x=x, c0=c0, cs0=cs0, sumsq=sumsq)


def reference(c, alpha=1.0):
    """float64 results and sum|terms| of both outputs"""
    f = 1.0 / (torch.sqrt(c.sumsq.to(F64)) + 1e-6) if c.sumsq is not None else torch.ones(1, dtype=F64, device=dev())
    a, b = c.dy[:, :c.M].to(F64), c.x[:, :c.N].to(F64)
    prod, prod_abs = a.t() @ b, a.abs().t() @ b.abs()
    C0, S0 = c.c0[:, :c.N].to(F64), c.cs0[:c.M].to(F64)
    return SimpleNamespace(C=C0 + alpha * f * prod, C_terms=C0.abs() + abs(alpha) * f * prod_abs,
                           S=S0 + f * a.sum(0), S_terms=S0.abs() + f * a.abs().sum(0))


def run(ops, c, with_colsum=True, alpha=1.0):
    C, S = c.c0.clone(), c.cs0.clone()
    ops.gemm_dw_colsum(c.dy, c.x, C, S[:c.M] if with_colsum else None, c.M, c.N, c.K, alpha=alpha, alpha_sumsq=c.sumsq)
    torch.cuda.synchronize()
    return C, S


def verify(name, c, C, S, alpha=1.0, with_colsum=True):
    r, k = reference(c, alpha), path_len(c.M, c.N, c.K)
    check(f'{name} dW', C[:, :c.N], r.C, 1e-5 * r.C.abs() + k * U32 * r.C_terms)
    assert torch.equal(C[:, c.N:], c.c0[:, c.N:]), f'{name}: pad columns of dW were written'
    if with_colsum:
        check(f'{name} colsum', S[:c.M], r.S, 1e-5 * r.S.abs() + k * U32 * r.S_terms)
        assert torch.equal(S[c.M:], c.cs0[c.M:]), f'{name}: floats behind colsum[M] were written'
    else:
        assert torch.equal(S, c.cs0), f'{name}: colsum written without being asked for'


# (512, 256, 1000): two row tiles, one column tile (every K-tile is the work item's own), ragged K tail
# (256, 768, 4099): three column tiles share the K-tiles of a row tile, several slices, K no multiple of the K step
# (520, 512, 2048): ragged last row tile -- rows >= M of the tile see junk and must not be written
SHAPES = [(512, 256, 1000), (256, 768, 4099), (520, 512, 2048)]


@pytest.mark.parametrize('M,N,K', SHAPES)
def test_dw_and_colsum_vs_fp64(ops, M, N, K):
    c = make_case(M, N, K, seed=M + N + K)
    C, S = run(ops, c)
    verify(f'({M},{N},{K})', c, C, S)


def test_alpha_sumsq(ops):
    """the normaliser 1 / (sqrt(S) + 1e-6) scales both outputs; alpha scales dW only (i2t_colsum_bf16_ex has no alpha)"""
    c = make_case(256, 768, 4099, seed=11, with_sumsq=True)
    C, S = run(ops, c, alpha=0.75)
    verify('alpha_sumsq', c, C, S, alpha=0.75)


def test_without_colsum_is_the_plain_call(ops):
    """colsum_out = NULL: no column sums, and dW bit-equal to ops.gemm's -- in deterministic mode, where both are reproducible"""
    c = make_case(256, 768, 4099, seed=5)
    C, S = run(ops, c, with_colsum=False)
    verify('no colsum', c, C, S, with_colsum=False)
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        C1, S1 = run(ops, c, with_colsum=False)
        C2 = c.c0.clone()
        ops.gemm(c.dy, c.x, C2, c.M, c.N, c.K, a_kmajor=True, b_kmajor=True, accumulate=True)
        C3, S3 = run(ops, c)                         # deterministic mode with column sums: the ordered column-sum launch, same dW
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    assert torch.equal(C1, C2) and torch.equal(S1, c.cs0)
    assert torch.equal(C3, C2)
    r = reference(c)
    check('deterministic colsum', S3[:c.M], r.S, 1e-5 * r.S.abs() + (c.K // 4 + 5) * U32 * r.S_terms)     # (one wave's rows in order, 4 waves, 1 add)
    assert torch.equal(S3[c.M:], c.cs0[c.M:])


def test_site_bwd_fold_switch(ops):
    """engine_lora._site_bwd on a tiny plain site (weight and bias trainable): I2T_FOLD_COLSUM=1 (db from the dW launch) against =0 (the
    colsum launch + the plain dW GEMM), compared with each other.  Both sides carry their own error: the bound's k is the folded path's
    plus the column-sum kernel's (a wave's share of a 64-row slice in order = 16, 4 waves, one atomic per slice)."""
    from image2text_amd.engine_lora import LoraAdapters
    N, K, M = 256, 256, 1024
    g = torch.Generator(device=dev()).manual_seed(3)
    dY = (torch.randn(M, N, generator=g, device=dev()) * 0.5).to(BF16)
    x = torch.randn(M, K, generator=g, device=dev()).to(BF16)
    g0, gb0 = torch.randn(N, K, generator=g, device=dev()), torch.randn(N, generator=g, device=dev())
    host = SimpleNamespace(arena=SimpleNamespace(trainable=lambda n: True), _site_e4m3=lambda s: False)
    out = {}
    old = os.environ.get('I2T_FOLD_COLSUM')
    try:
        for mode in ('1', '0'):
            os.environ['I2T_FOLD_COLSUM'] = mode
            s = SimpleNamespace(names=('w',), bnames=('b',), W=None, G=g0.clone(), b=None, gb=gb0.clone(), N=N, K=K, lora=None, switch=None)
            assert LoraAdapters._site_bwd(host, s, None, dY, x, M) is None
            torch.cuda.synchronize()
            out[mode] = s
    finally:
        if old is None:
            os.environ.pop('I2T_FOLD_COLSUM', None)
        else:
            os.environ['I2T_FOLD_COLSUM'] = old
    a, b = dY.to(F64), x.to(F64)
    k_fold, slices = path_len(N, K, M), min((M + 63) // 64, 512)
    k_plain = 16 + 4 + slices
    gb_terms = gb0.to(F64).abs() + a.abs().sum(0)
    gw_terms = g0.to(F64).abs() + a.abs().t() @ b.abs()
    gb_ref, gw_ref = gb0.to(F64) + a.sum(0), g0.to(F64) + a.t() @ b
    check('site db fold vs plain', out['1'].gb, out['0'].gb, 1e-5 * gb_ref.abs() + (k_fold + k_plain) * U32 * gb_terms)
    check('site dW fold vs plain', out['1'].G, out['0'].G, 1e-5 * gw_ref.abs() + 2 * k_fold * U32 * gw_terms)
    check('site db fold vs fp64', out['1'].gb, gb_ref, 1e-5 * gb_ref.abs() + k_fold * U32 * gb_terms)
