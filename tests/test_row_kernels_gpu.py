"""The row, activation and loss-helper kernels (csrc/llama.hip, csrc/lora.hip, the distillation / arena helpers of
csrc/elementwise.hip and the small ones of csrc/vit.hip and csrc/family.hip) at the shapes the Llama-2 / Qwen2 / Falcon / LoRA /
momentum-distillation steps run them, each against a float64 statement of the same op (restated from include/i2t.h) on the SAME
rounded values the kernel reads.

The tolerance rule (DESIGN.md "Row, activation and loss-helper kernels"): every comparison is PER ELEMENT,
    bf16 output:  |got - ref| <= 2^-7 |ref| + a          fp32 output:  |got - ref| <= r |ref| + a
with r = 1e-5 for row ops and 2e-3 after a long reduction (tests/test_kernels_gpu.py), and ``a`` derived per element from the
operands: 2^-8 sum|terms| (bf16 outputs) or k 2^-23 sum|terms| (fp32 outputs, k = terms on the longest fp32 path).  No element
is excluded, non-finite outputs fail, outputs start as NaN and everything a kernel must not touch holds a sentinel that is
compared with torch.equal.  ``check`` prints the largest error in units of the bound for every comparison (pytest -rA shows it)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E8, E7 = 2.0 ** -8, 2.0 ** -7            # half an ulp / one ulp of bf16, relative
U32 = 2.0 ** -23                          # one ulp of fp32, relative
TINY = 2.0 ** -126                        # below this fp32 flushes to zero: the absolute error of a sigmoid / exp that underflowed
SENT = -7.75                              # sentinel (exact in bf16)
# erf by Abramowitz & Stegun 7.1.26 (csrc/common.h::erf_sqrt2_): |erf error| <= 1.5e-7, so Phi = (1 + erf) / 2 carries 7.5e-8 plus
# the fp32 roundings of 1 - poly e and 1 + erf (2 x 2^-25 on values <= 2, halved): 1.5e-7 absolute on Phi covers both
ERF_PHI_ERR = 1.5e-7


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def rnd(*shape, scale=1.0, seed=0, dtype=F32):
    g = torch.Generator(device=dev()).manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device=dev()) * scale).to(dtype)


def nans(*shape, dtype=F32):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev())


def check(name, got, ref, tol):
    """per element |got - ref| <= tol (float64 tensors of got's shape); returns the largest error in units of the bound"""
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    tol = torch.as_tensor(tol, dtype=F64, device=got.device).expand_as(ref)
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs()
    units = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = float(units.max()) if units.numel() else 0.0
    print(f'UNITS {name}: {worst:.4f}')
    bad = err > tol
    if bad.any():
        idx = np.unravel_index(int(units.argmax()), tuple(got.shape))
        raise AssertionError(f'{name}: {int(bad.sum())}/{bad.numel()} out of tolerance; worst at {idx}: got {got[idx].item():.9g} '
                             f'ref {ref[idx].item():.9g} tol {tol[idx].item():.3g} ({worst:.2f} x the bound)')
    return worst


def bf16_round(x64):
    """float64 -> nearest bf16 (through fp32: exact for values that are fp32 already), as float64"""
    return x64.to(F32).to(BF16).to(F64)


def refused(fn, what):
    from image2text_amd import lib as i2tlib
    with pytest.raises(i2tlib.I2TError, match=r'rc=-\d+') as e:
        fn()
    assert what in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------------------------ RMSNorm
def _rms_inputs(M, d, seed):
    """rows with a mean far from zero and scales from 1e-3 to 1e3; row 0 of a multi-row case is all zero"""
    x = rnd(M, d, seed=seed)
    sc = torch.logspace(-3, 3, M, device=dev()).unsqueeze(1) if M > 1 else torch.ones(1, 1, device=dev())
    x = (x + 3.0) * sc
    if M > 1:
        x[0] = 0.0
    w = 1.0 + 0.5 * rnd(d, seed=seed + 1)
    return x.contiguous(), w.contiguous()


def _rms_ref(x, w, eps):
    x64, w64 = x.double(), w.double()
    rstd = (x64.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return x64 * rstd * w64, rstd.squeeze(-1)


RMS_D = [256, 1536, 2048, 2052, 4096, 4544, 5120, 8192]


@pytest.mark.parametrize('M', [1, 3, 33])
@pytest.mark.parametrize('d', RMS_D)
def test_rmsnorm_fwd(ops, d, M):
    _rmsnorm_fwd_case(ops, M, d)


def test_rmsnorm_fwd_real_rows(ops):
    _rmsnorm_fwd_case(ops, 4096 + 5, 4096)


def _rmsnorm_fwd_case(ops, M, d):
    eps = 1e-6
    x, w = _rms_inputs(M, d, seed=d + M)
    yr, rr = _rms_ref(x, w, eps)
    k = d // 256 + 8                                        # a lane's serial chain of squares + the wave tree + the final products
    for skip in ('none', 'y', 'y_f32', 'rstd'):
        y = None if skip == 'y' else nans(M + 1, d, dtype=BF16)
        y32 = None if skip == 'y_f32' else nans(M + 1, d)
        rs = None if skip == 'rstd' else nans(M + 1)
        for t in (y, y32, rs):
            if t is not None:
                t[M:] = SENT
        ops.rmsnorm_fwd(x, w, y, rs, M, d, eps, y_f32=y32)
        tag = f'rms_fwd M={M} d={d} null={skip}'
        if rs is not None:
            check(f'{tag} rstd', rs[:M], rr, 1e-5 * rr.abs() + k * U32 * rr.abs())
            assert torch.equal(rs[M:], torch.full_like(rs[M:], SENT))
        if y32 is not None:
            check(f'{tag} y_f32', y32[:M], yr, 1e-5 * yr.abs() + k * U32 * yr.abs())
            assert torch.equal(y32[M:], torch.full_like(y32[M:], SENT))
        if y is not None:
            check(f'{tag} y', y[:M], yr, E7 * yr.abs())
            assert torch.equal(y[M:], torch.full_like(y[M:], SENT))
        if y is not None and y32 is not None:
            assert torch.equal(y[:M], y32[:M].to(BF16)), f'{tag}: the bf16 output is not the rounded fp32 output'
        if M > 1:                                           # the all-zero row: rstd = eps^-1/2, outputs exactly zero
            for t in (y, y32):
                if t is not None:
                    assert torch.equal(t[0], torch.zeros_like(t[0]))


def _rms_bwd_ref(dy, x, w, rstd):
    dy64, x64, w64, rs = dy.double(), x.double(), w.double(), rstd.double().unsqueeze(-1)
    g, xh = dy64 * w64, x64 * rs
    c2 = (g * xh).mean(-1, keepdim=True)
    dx = rs * (g - xh * c2)
    dx_terms = rs * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    return dx, dx_terms, (dy64 * xh).sum(0), (dy64 * xh).abs().sum(0)


def _rmsnorm_bwd_case(ops, M, d, dy_dtype):
    x, w = _rms_inputs(M, d, seed=3 * d + M)
    rstd = _rms_ref(x, w, 1e-6)[1].float().contiguous()             # the fp32 values the kernel reads
    dy = rnd(M, d, seed=5 * d + M, dtype=dy_dtype)
    dxr, dxt, dwr, dwt = _rms_bwd_ref(dy, x, w, rstd)
    k = d // 256 + 10
    kw = 12 + (M + 31) // 32                                # 8 rows per wave + 4 waves, then one atomic per workgroup
    tol_dx = 1e-5 * dxr.abs() + k * U32 * dxt
    tol_dw = 2e-3 * dwr.abs() + kw * U32 * dwt
    dx0, dw0 = rnd(M, d, seed=7), rnd(d, seed=8)
    for acc, with_dw, with_bf in ((False, True, True), (True, True, True), (False, False, True), (False, True, False), (True, False, False)):
        dx = nans(M + 1, d)
        dx[M:] = SENT
        if acc:
            dx[:M] = dx0
        dxb = nans(M + 1, d, dtype=BF16) if with_bf else None
        if with_bf:
            dxb[M:] = SENT
        dw = dw0.clone() if with_dw else None
        ops.rmsnorm_bwd(dy, x, w, rstd, dx, dw, M, d, dx_accumulate=acc, dx_bf16=dxb)
        tag = f'rms_bwd M={M} d={d} dy={dy_dtype} acc={acc} dw={with_dw} bf={with_bf}'
        ref = dxr + dx0.double() if acc else dxr
        check(f'{tag} dx', dx[:M], ref, tol_dx + (2 * U32 * dx0.double().abs() if acc else 0.0))
        assert torch.equal(dx[M:], torch.full_like(dx[M:], SENT))
        if with_bf:
            assert torch.equal(dxb[:M], dx[:M].to(BF16)), f'{tag}: dx_bf16 is not the rounded dx'
            assert torch.equal(dxb[M:], torch.full_like(dxb[M:], SENT))
        if with_dw:
            check(f'{tag} dw', dw, dwr + dw0.double(), tol_dw + 2 * U32 * dw0.double().abs())


@pytest.mark.parametrize('dy_dtype', [F32, BF16])
@pytest.mark.parametrize('M', [1, 3, 33])
@pytest.mark.parametrize('d', RMS_D)
def test_rmsnorm_bwd(ops, d, M, dy_dtype):
    _rmsnorm_bwd_case(ops, M, d, dy_dtype)


@pytest.mark.parametrize('dy_dtype', [F32, BF16])
def test_rmsnorm_bwd_real_rows(ops, dy_dtype):
    _rmsnorm_bwd_case(ops, 4096 + 5, 4096, dy_dtype)


def test_rmsnorm_bwd_deterministic_dw(ops):
    M, d = 133, 2052
    x, w = _rms_inputs(M, d, seed=11)
    rstd = _rms_ref(x, w, 1e-6)[1].float().contiguous()
    dy = rnd(M, d, seed=12)
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            dx, dw = nans(M, d), torch.zeros(d, device=dev())
            ops.rmsnorm_bwd(dy, x, w, rstd, dx, dw, M, d)
            outs.append((dx, dw))
    finally:
        ops.set_deterministic(was)
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    dxr, dxt, dwr, dwt = _rms_bwd_ref(dy, x, w, rstd)
    check('rms_bwd deterministic dw', outs[0][1], dwr, 2e-3 * dwr.abs() + (12 + (M + 31) // 32) * U32 * dwt)


# --------------------------------------------------------------------------------------------------------------------- RoPE
N_POS = 1030


def _rope_table(hd):
    """[N_POS][hd] fp32: cos(p f_i) | sin(p f_i), f_i = 10000^(-2 i / hd), built in fp64"""
    i = torch.arange(hd // 2, dtype=F64)
    ang = torch.arange(N_POS, dtype=F64).unsqueeze(1) * (10000.0 ** (-2.0 * i / hd)).unsqueeze(0)
    return torch.cat([ang.cos(), ang.sin()], 1).to(F32).to(dev()).contiguous()


def _rope_ref(x, col0, nh, hd, cs, p, inverse):
    """x bf16 [M][rs], p long [M] -> (fp64 reference of the rotated heads [M][nh][hd], sum |terms|)"""
    M = x.shape[0]
    v = x[:, col0:col0 + nh * hd].double().view(M, nh, hd)
    a, b = v[..., :hd // 2], v[..., hd // 2:]
    t = cs[p].double()
    c, s = t[:, None, :hd // 2], t[:, None, hd // 2:]
    if inverse:
        s = -s
    ref = torch.cat([a * c - b * s, b * c + a * s], -1)
    terms = torch.cat([a.abs() * c.abs() + b.abs() * s.abs(), b.abs() * c.abs() + a.abs() * s.abs()], -1)
    return ref, terms


def _rope_buffer(M, rs, seed):
    x = rnd(M + 1, rs, seed=seed, dtype=BF16)
    return x


ROPE_HEADS = [(128, 64), (128, 14), (64, 72), (128, 1), (64, 1), (16, 1), (16, 3)]     # (hd, heads): 32+32, 12+2, 71+1, 1


@pytest.mark.parametrize('col0', [0, 40])
@pytest.mark.parametrize('hd,nh', ROPE_HEADS)
def test_rope(ops, hd, nh, col0):
    cs = _rope_table(hd)
    rs = col0 + nh * hd + 24                                # the value columns of a fused qkv row stand behind the rotated heads
    per_row = nh * hd // 16                                 # threads per row
    Ms = sorted({1, 37, 300} | ({256 // per_row * 5 - 1, 256 // per_row * 5, 256 // per_row * 5 + 1} if per_row <= 256 and 256 % per_row == 0 else set()))
    g = torch.Generator().manual_seed(hd * 1000 + nh + col0)
    for M in Ms:
        T = 7 if M > 7 else M                               # M is not a multiple of T for the ragged Ms
        pos_rows = torch.randint(0, N_POS, (M,), generator=g)
        pos_rows[0] = N_POS - 1                             # the last table row, then descending and repeated entries
        if M > 3:
            pos_rows[1:4] = torch.tensor([900, 900, 3])
        sources = {'pos': dict(pos=pos_rows.to(torch.int32).to(dev())),
                   'pos_ptr': dict(pos_ptr=torch.tensor([1000], dtype=torch.int32, device=dev()), pos_offset=23),
                   'dense': dict(pos_offset=N_POS - T, T=T)}
        rows = {'pos': pos_rows, 'pos_ptr': torch.full((M,), 1023), 'dense': N_POS - T + torch.arange(M) % T}
        for name, kw in sources.items():
            for inverse in (False, True):
                x = _rope_buffer(M, rs, seed=M + nh)
                x0 = x.clone()
                ops.rope(x, rs, col0, nh, hd, cs, M, inverse=inverse, **kw)
                tag = f'rope hd={hd} nh={nh} col0={col0} M={M} {name} inv={inverse}'
                ref, terms = _rope_ref(x0[:M], col0, nh, hd, cs, rows[name].to(dev()), inverse)
                check(tag, x[:M, col0:col0 + nh * hd].reshape(M, nh, hd), ref, E7 * ref.abs() + E8 * terms)
                assert torch.equal(x[:M, :col0], x0[:M, :col0]) and torch.equal(x[:M, col0 + nh * hd:], x0[:M, col0 + nh * hd:]), f'{tag}: columns outside the heads'
                assert torch.equal(x[M:], x0[M:]), f'{tag}: rows past M'
                if not inverse:                             # inverse after forward: two bf16 roundings per element
                    fwd = x.clone()
                    ops.rope(x, rs, col0, nh, hd, cs, M, inverse=True, **kw)
                    _, t2 = _rope_ref(fwd[:M], col0, nh, hd, cs, rows[name].to(dev()), True)
                    orig = x0[:M, col0:col0 + nh * hd].double().view(M, nh, hd)
                    check(f'{tag} round trip', x[:M, col0:col0 + nh * hd].reshape(M, nh, hd), orig, (E8 * t2 + E8 * orig.abs()) * (1 + 2.0 ** -6))


def test_rope_position_zero_is_identity(ops):
    for hd, nh in ((128, 14), (64, 72), (16, 1)):
        cs = _rope_table(hd)
        M, rs = 19, nh * hd + 8
        x = rnd(M, rs, seed=hd, dtype=BF16)
        x0 = x.clone()
        for inverse in (False, True):
            ops.rope(x, rs, 0, nh, hd, cs, M, pos=torch.zeros(M, dtype=torch.int32, device=dev()), inverse=inverse)
            assert torch.equal(x.view(torch.int16), x0.view(torch.int16))
            ops.rope(x, rs, 0, nh, hd, cs, M, pos_offset=0, T=1, inverse=inverse)
            assert torch.equal(x.view(torch.int16), x0.view(torch.int16))


def test_rope_refuses_bad_arguments(ops):
    cs = _rope_table(64)
    x = rnd(4, 256, dtype=BF16)
    x0 = x.clone()
    cs24 = torch.zeros(N_POS, 24, device=dev())
    refused(lambda: ops.rope(x, 256, 0, 2, 24, cs24, 4, pos_offset=0, T=4), 'i2t_rope')                    # hd % 16 != 0
    refused(lambda: ops.rope(x, 256, 8, 4, 64, cs, 4, pos_offset=0, T=4), 'i2t_rope')                      # heads overrun the row
    refused(lambda: ops.rope(x, 256, 0, 4, 64, cs, 4, pos_offset=N_POS - 3, T=4), 'outside the table')     # dense range overruns the table
    refused(lambda: ops.rope(x, 256, 0, 4, 64, cs[:2], 4, pos_offset=0, T=4), 'outside the table')
    torch.cuda.synchronize()
    assert torch.equal(x, x0)


# ------------------------------------------------------------------------------------------------------------------- SwiGLU
EDGE_GATES = [0.0, -0.0, 20.0, -20.0, 50.0, -50.0, 90.0, -90.0, 200.0, -200.0]


def _swiglu_inputs(M, ff, ld, gate_scale, seed):
    gu = torch.full((M + 1, ld), SENT, dtype=BF16, device=dev())
    gu[:M, :ff] = rnd(M, ff, seed=seed, scale=gate_scale, dtype=BF16)
    gu[:M, ff:2 * ff] = rnd(M, ff, seed=seed + 1, dtype=BF16)
    ne = len(EDGE_GATES)
    for r in range(min(M, 3)):                              # the edge values, in the first rows and at the end of the last vector
        gu[r, :ne] = torch.tensor(EDGE_GATES, dtype=BF16, device=dev())
        gu[r, ff - ne:ff] = torch.tensor(EDGE_GATES, dtype=BF16, device=dev())
    return gu


def _swiglu_case(ops, M, ff, pad, gate_scale):
    ld = 2 * ff + pad
    gu = _swiglu_inputs(M, ff, ld, gate_scale, seed=ff + M + pad)
    gu0 = gu.clone()
    g, u = gu[:M, :ff].double(), gu[:M, ff:2 * ff].double()
    s = torch.sigmoid(g)
    tag = f'swiglu M={M} ff={ff} ld={ld} gate x{gate_scale}'
    # forward
    h = nans(M + 1, ff, dtype=BF16)
    h[M:] = SENT
    ops.swiglu_fwd(gu[:M], h, M, ff)
    href = g * s * u
    check(f'{tag} fwd', h[:M], href, E7 * href.abs() + TINY * (g * u).abs())
    assert torch.equal(h[M:], torch.full_like(h[M:], SENT)) and torch.equal(gu, gu0)
    # backward
    dh = rnd(M, ff, seed=ff + 3, dtype=BF16)
    dgu = nans(M + 1, ld, dtype=BF16)
    dgu[M:] = SENT
    dgu[:, 2 * ff:] = SENT
    ops.swiglu_bwd(dh, gu[:M], dgu[:M], M, ff)
    d = dh.double()
    dg_ref = d * u * (s + g * s * (1 - s))
    dg_terms = (d * u).abs() * (s + g.abs() * s * (1 - s))
    du_ref = d * g * s
    check(f'{tag} bwd d_gate', dgu[:M, :ff], dg_ref, E7 * dg_ref.abs() + E8 * dg_terms + TINY * (d * u).abs() * (1 + g.abs()))
    check(f'{tag} bwd d_up', dgu[:M, ff:2 * ff], du_ref, E7 * du_ref.abs() + TINY * (d * g).abs())
    assert torch.equal(dgu[M:], torch.full_like(dgu[M:], SENT)) and torch.equal(dgu[:, 2 * ff:], torch.full_like(dgu[:, 2 * ff:], SENT))
    assert torch.equal(gu, gu0)
    # the edge columns: the fp64 value rounded to bf16 -- silu(-200) = -0 / 0, silu(200) = 200, the gate factor 0 or 1
    ne = len(EDGE_GATES)
    for r in range(min(M, 3)):
        for c0 in (0, ff - ne):
            ge, ue, de = g[r, c0:c0 + ne], u[r, c0:c0 + ne], d[r, c0:c0 + ne]
            for j, gv in enumerate(EDGE_GATES):
                if abs(gv) >= 90:
                    want_h = 0.0 if gv < 0 else gv * float(ue[j])
                    assert abs(float(h[r, c0 + j]) - float(bf16_round(torch.tensor(want_h, dtype=F64)))) <= TINY * abs(gv * float(ue[j])), (tag, r, c0, gv)
                    want_g = 0.0 if gv < 0 else float(de[j] * ue[j])
                    assert abs(float(dgu[r, c0 + j]) - float(bf16_round(torch.tensor(want_g, dtype=F64)))) <= TINY * (1 + abs(gv)) * abs(float(de[j] * ue[j])), (tag, r, c0, gv)
            assert float(ge.abs().max()) == 200.0


@pytest.mark.parametrize('gate_scale', [1.0, 2.0])          # N(0, 1) and N(0, 4)
@pytest.mark.parametrize('pad', [0, 64])
@pytest.mark.parametrize('M,ff', [(1, 96), (37, 96), (4096, 96), (1, 8960), (37, 8960), (4096, 8960), (1, 11008), (37, 11008), (1, 13824), (37, 13824)])
def test_swiglu(ops, M, ff, pad, gate_scale):
    _swiglu_case(ops, M, ff, pad, gate_scale)


# ------------------------------------------------------------------------------------------------------------- GELU helpers
def _gelu_tanh64(x):
    """-> (gelu, gelu', sum |terms| of gelu', relative fp32 error of the sigmoid form, flush allowance of gelu'): x sigmoid(2u), u = sqrt(2/pi)(x + 0.044715 x^3)"""
    k0 = math.sqrt(2.0 / math.pi)
    u2 = 2.0 * k0 * (x + 0.044715 * x ** 3)
    s = torch.sigmoid(u2)
    du2 = 2.0 * k0 * (1 + 3 * 0.044715 * x * x)
    grad = s + x * s * (1 - s) * du2
    terms = s + (x * s * (1 - s) * du2).abs()
    flush = TINY * (1 + (x * du2).abs())                    # a sigmoid below 2^-126 is flushed to zero: its coefficient in gelu'
    # s = 1 / (1 + exp2(t)), t = x (c0 + c1 x^2) log2 e: four fp32 roundings reach t (2^-24 each), exp2 turns an absolute error of
    # t into a relative one (ln 2), plus the 1-ulp v_exp_f32 / v_rcp_f32 and the sum
    rel = 4 * 2.0 ** -24 * math.log(2.0) * (u2.abs() * 1.4426950408889634) + 4 * 2.0 ** -24
    return x * s, grad, terms, rel, flush


def _gelu_erf64(x):
    Phi = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * Phi, Phi + x * phi, Phi + (x * phi).abs()


def _gelu_inputs(n, seed):
    """|x| up to 12: N(0, 1) mixed with a uniform sweep of [-12, 12] so both tails of the derivative are reached"""
    x = rnd(n, seed=seed)
    x[::3] = torch.linspace(-12, 12, x[::3].numel(), device=dev())
    x[:8] = torch.tensor([0.0, -0.0, 12.0, -12.0, 5.0, -5.0, 0.5, -0.5], device=dev())[:min(n, 8)]
    return x


CAP4 = 65536 * 256 * 4 + 4 * 37                             # one vector-of-4 past 65536 workgroups: the second grid-stride trip, ragged


@pytest.mark.parametrize('erf', [False, True])
@pytest.mark.parametrize('n', [4, 8, 1000, 4096 * 3072, CAP4])
def test_dgelu_mul(ops, n, erf):
    pre = _gelu_inputs(n, seed=n % 9973).to(BF16)
    dh = rnd(n, seed=n % 9973 + 1)
    out = nans(n + 8, dtype=BF16)
    out[n:] = SENT
    ops.dgelu_mul(dh, pre, out[:n], erf=erf)
    x, d = pre.double(), dh.double()
    if erf:
        _, grad, terms = _gelu_erf64(x)
        a = ERF_PHI_ERR * d.abs()
    else:
        _, grad, terms, rel, flush = _gelu_tanh64(x)
        a = (rel * terms + flush) * d.abs()
    ref = d * grad
    check(f'dgelu_mul erf={erf} n={n}', out[:n], ref, E7 * ref.abs() + E8 * d.abs() * terms + a + TINY)
    assert torch.equal(out[n:], torch.full_like(out[n:], SENT))


@pytest.mark.parametrize('erf', [False, True])
@pytest.mark.parametrize('n', [8, 1000, 4096 * 3072, 2 * CAP4])
def test_gelu_fwd(ops, n, erf):
    pre = _gelu_inputs(n, seed=n % 9973 + 2).to(BF16)
    pre0 = pre.clone()
    out = nans(n + 8, dtype=BF16)
    out[n:] = SENT
    ops.gelu_fwd(pre, out[:n], erf=erf)
    x = pre.double()
    if erf:
        ref = _gelu_erf64(x)[0]
        a = ERF_PHI_ERR * x.abs()
    else:
        ref, _, _, rel, _ = _gelu_tanh64(x)
        a = rel * ref.abs() + TINY * x.abs()
    check(f'gelu_fwd erf={erf} n={n}', out[:n], ref, E7 * ref.abs() + a)
    assert torch.equal(out[n:], torch.full_like(out[n:], SENT)) and torch.equal(pre, pre0)


@pytest.mark.parametrize('with_lo', [True, False])
@pytest.mark.parametrize('act', [0, 1, 3])                  # I2T_ACT_NONE, I2T_ACT_GELU, I2T_ACT_GELU_ERF
@pytest.mark.parametrize('n', [1, 7, 1001, 4096 * 3072 + 1])
def test_split_f32(ops, n, act, with_lo):
    assert (ops.ACT_GELU, ops.ACT_GELU_ERF) == (1, 3)
    src = _gelu_inputs(n, seed=n % 9973 + 3) * (1.0 if act else 37.0)
    hi, lo = nans(n + 8, dtype=BF16), (nans(n + 8, dtype=BF16) if with_lo else None)
    hi[n:] = SENT
    if with_lo:
        lo[n:] = SENT
    ops.split_f32(src, hi, lo, n=n, act=act)
    x = src.double()
    if act == 0:
        ref, a = x, torch.zeros_like(x)
    elif act == 1:
        ref, _, _, rel, _ = _gelu_tanh64(x)
        a = rel * ref.abs() + TINY * x.abs()
    else:
        ref = _gelu_erf64(x)[0]
        a = ERF_PHI_ERR * x.abs() + 4 * 2.0 ** -24 * ref.abs()
    tag = f'split_f32 n={n} act={act} lo={with_lo}'
    check(f'{tag} hi', hi[:n], ref, (E7 if act else E8) * ref.abs() + a + TINY)
    assert torch.equal(hi[n:], torch.full_like(hi[n:], SENT))
    if act == 0:
        assert torch.equal(hi[:n], src.to(BF16))
    if with_lo:
        check(f'{tag} hi + lo', hi[:n].double() + lo[:n].double(), ref, 2.0 ** -16 * ref.abs() + a + 2 * TINY)
        assert torch.equal(lo[n:], torch.full_like(lo[n:], SENT))


def test_gelu_entry_points_refuse_ragged_sizes(ops):
    pre, dh, out = rnd(16, dtype=BF16), rnd(16), nans(16, dtype=BF16)
    refused(lambda: ops.dgelu_mul(dh[:6], pre[:6], out[:6]), 'multiple of 4')
    refused(lambda: ops.dgelu_mul(dh[:6], pre[:6], out[:6], erf=True), 'multiple of 4')
    refused(lambda: ops.gelu_fwd(pre[:12].clone(), out[:12].clone()), 'multiple of 8')
    refused(lambda: ops.split_f32(dh, out, None, act=2), 'act=2')
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()


# --------------------------------------------------------------------------------------------------------------- lora_stage
@pytest.mark.parametrize('M', [1, 33, 4096])
@pytest.mark.parametrize('K', [64, 768, 4096, 4544])
def test_lora_stage(ops, K, M):
    from image2text_amd import rng
    ldc = K + 64
    x = rnd(M, K, seed=K + M, dtype=BF16)
    x[x == 0] = 1.0
    x0 = x.clone()
    key, thr = rng.site_key(1234 + K, M), rng.threshold(0.1)
    drop = (1, key, thr, rng.scale(thr))
    for with_xd in (True, False):
        xcat = torch.full((M + 1, ldc), SENT, dtype=BF16, device=dev())
        xd = nans(M * K + 8, dtype=BF16) if with_xd else None
        if with_xd:
            xd[M * K:] = SENT
        ops.lora_stage(x, xcat[:M], xd[:M * K].view(M, K) if with_xd else None, M, K, drop if with_xd else None)
        assert torch.equal(xcat[:M, :K], x0) and torch.equal(x, x0)
        assert torch.equal(xcat[:M, K:], torch.full_like(xcat[:M, K:], SENT)) and torch.equal(xcat[M:], torch.full_like(xcat[M:], SENT))
        if with_xd:
            want = x0.clone()
            ops.dropout_apply(want, M, K, drop)
            got = xd[:M * K].view(M, K)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), 'xd differs from i2t_dropout_apply on a copy of x'
            assert torch.equal((got != 0).flatten().cpu(), rng.keep_mask(key, M * K, thr)), 'keep pattern'
            assert torch.equal(xd[M * K:], torch.full_like(xd[M * K:], SENT))


# ------------------------------------------------------------------------------------------------------- distillation loss
IGNORE = -100


def _distill_ref(z, t, labels, w, V, inv_temp, alpha, gscale):
    """fp64 from include/i2t.h: loss_row = lse(z/T) - (1 - alpha) z[label]/T - alpha/T sum_v softmax(t/T)[v] z[v];
    dz = g w/T (softmax(z/T) - (1 - alpha) onehot - alpha softmax(t/T)); dead rows (ignored / out-of-range label): zero."""
    z64, t64 = z[:, :V].double(), t[:, :V].double()
    live = (labels != IGNORE) & (labels >= 0) & (labels < V)
    lab = labels.clamp(0, V - 1)
    lse, lse_t = torch.logsumexp(z64 * inv_temp, -1), torch.logsumexp(t64 * inv_temp, -1)
    p, pt = torch.exp(z64 * inv_temp - lse[:, None]), torch.exp(t64 * inv_temp - lse_t[:, None])
    zl = z64.gather(1, lab[:, None]).squeeze(1)
    dot, dot_abs = (pt * z64).sum(-1), (pt * z64.abs()).sum(-1)
    w64 = w.double()
    rows = torch.where(live, w64 * (lse - (1 - alpha) * zl * inv_temp - alpha * inv_temp * dot), torch.zeros_like(lse))
    rows_abs = torch.where(live, w64.abs() * (lse.abs() + (1 - alpha) * (zl * inv_temp).abs() + alpha * inv_temp * dot_abs), torch.zeros_like(lse))
    onehot = torch.zeros_like(z64).scatter_(1, lab[:, None], 1.0)
    coef = torch.where(live, gscale * w64 * inv_temp, torch.zeros_like(w64))[:, None]
    grad = coef * (p - (1 - alpha) * onehot - alpha * pt)
    gterms = coef.abs() * (p + (1 - alpha) * onehot + alpha * pt)
    spread = ((z64 * inv_temp).amax(-1) - (z64 * inv_temp).amin(-1)).max().item()
    return dict(live=live, lse=torch.where(live, lse, torch.zeros_like(lse)), lse_t=torch.where(live, lse_t, torch.zeros_like(lse)),
                loss=rows.sum(), loss_abs=rows_abs.sum(), grad=grad, gterms=gterms, spread=spread)


@pytest.mark.parametrize('alpha', [0.0, 0.4, 1.0])
@pytest.mark.parametrize('temp', [1.0, 0.7])
@pytest.mark.parametrize('M,V,ld,ld_t', [(64, 50257, 50264, 50264), (19, 151936, 151936, 151944), (9, 13, 16, 24), (37, 1000, 1000, 1008)])
def test_ce_distill(ops, M, V, ld, ld_t, temp, alpha):
    inv_temp, gscale = 1.0 / temp, 0.37
    z = torch.full((M + 1, ld), SENT, dtype=BF16, device=dev())
    t = torch.full((M + 1, ld_t), SENT, dtype=BF16, device=dev())
    z[:M, :V] = rnd(M, V, seed=V + M, scale=2.0, dtype=BF16)
    t[:M, :V] = rnd(M, V, seed=V + M + 1, scale=2.0, dtype=BF16)
    g = torch.Generator().manual_seed(V + M)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[::5] = IGNORE                                    # every fifth label ignored, with weight zero
    labels[1] = V - 1                                       # in the V % 8 tail (or the last column)
    labels[2] = V + 3                                       # out of range: a dead row
    labels[3] = V // 8 * 8 if V % 8 else V - 8              # the first tail column
    w = (0.5 + torch.rand(M, generator=g)) / M
    w[::5] = 0.0
    labels, w = labels.to(dev()), w.to(dev())
    z0, t0 = z.clone(), t.clone()
    r = _distill_ref(z[:M], t[:M], labels, w, V, inv_temp, alpha, gscale)
    k = (V + 511) // 512 + 16                               # a thread's serial chain + the wave / block trees
    tag = f'ce_distill M={M} V={V} T={temp} alpha={alpha}'
    lse, lse_t, loss = nans(M), nans(M), torch.zeros(1, device=dev())
    ops.ce_distill_fwd(z[:M], ld, t[:M], ld_t, alpha, labels, w, inv_temp, IGNORE, lse, lse_t, loss, M, V)
    assert torch.equal(z, z0) and torch.equal(t, t0)
    tol_lse = lambda ref: 1e-5 * ref.abs() + (k + r['spread'] + 20) * U32              # a relative error of the sum is an absolute one of its log
    check(f'{tag} lse', lse, r['lse'], tol_lse(r['lse']))
    check(f'{tag} lse_t', lse_t, r['lse_t'], tol_lse(r['lse_t']))
    check(f'{tag} loss', loss[0], r['loss'], 2e-3 * r['loss'].abs() + (k + M + r['spread'] + 20) * U32 * r['loss_abs'])
    gs = torch.tensor([gscale], device=dev())
    ops.ce_distill_bwd(z[:M], ld, t[:M], ld_t, alpha, labels, w, inv_temp, IGNORE, lse, lse_t, gs, M, V)
    check(f'{tag} grad', z[:M, :V], r['grad'], E7 * r['grad'].abs() + E8 * r['gterms'])
    dead = ~r['live']
    assert torch.equal(z[:M, :V][dead], torch.zeros_like(z[:M, :V][dead])), f'{tag}: dead rows are not zero'
    assert torch.equal(z[:M, V:], z0[:M, V:]) and torch.equal(z[M:], z0[M:]), f'{tag}: pad columns / rows past M'
    assert torch.equal(t, t0), f'{tag}: the teacher was written'
    if alpha == 0.0:                                        # the plain cross entropy on the same logits, each against fp64 first
        z1 = z0.clone()
        lse1, loss1 = nans(M), torch.zeros(1, device=dev())
        ops.ce_fwd(z1[:M], ld, labels, w, inv_temp, IGNORE, lse1, loss1, M, V)
        check(f'{tag} ce_fwd lse', lse1, r['lse'], tol_lse(r['lse']))
        check(f'{tag} ce_fwd loss', loss1[0], r['loss'], 2e-3 * r['loss'].abs() + (k + M + r['spread'] + 20) * U32 * r['loss_abs'])
        ops.ce_bwd(z1[:M], ld, labels, w, inv_temp, IGNORE, lse1, gs, M, V)
        check(f'{tag} ce_bwd grad', z1[:M, :V], r['grad'], E7 * r['grad'].abs() + E8 * r['gterms'])
        check(f'{tag} distill vs ce grad', z[:M, :V], z1[:M, :V].double(), 2 * (E7 * r['grad'].abs() + E8 * r['gterms']))
        assert torch.equal(z1[:M, V:], z0[:M, V:]) and torch.equal(z1[M:], z0[M:])


# ------------------------------------------------------------------------------------------------------------ arena helpers
EMA_CAP = 4096 * 256 * 4 + 4 * 37                           # one vector past the launcher's 4096-workgroup cap


@pytest.mark.parametrize('with_bf', [True, False])
@pytest.mark.parametrize('momentum', [0.0, 1.0, 0.995])
@pytest.mark.parametrize('n', [4, 1000, EMA_CAP])
def test_ema_update(ops, n, momentum, with_bf):
    pm, p = rnd(n + 4, seed=n % 9973), rnd(n + 4, seed=n % 9973 + 1, scale=3.0)
    pm[n:] = SENT
    pm0 = pm.clone()
    pb = nans(n + 4, dtype=BF16) if with_bf else None
    if with_bf:
        pb[n:] = SENT
    ops.ema_update(pm, p, pb, n, momentum)
    m32 = np.float32(momentum)
    om32 = np.float32(1.0) - m32                            # the kernel's fp32 (1 - momentum)
    ta, tb = pm0[:n].double() * float(m32), p[:n].double() * float(om32)
    ref = ta + tb
    check(f'ema n={n} m={momentum} bf={with_bf}', pm[:n], ref, 1e-5 * ref.abs() + 3 * U32 * (ta.abs() + tb.abs()))
    assert torch.equal(pm[n:], pm0[n:])
    if momentum == 1.0:
        assert torch.equal(pm[:n], pm0[:n])
    if momentum == 0.0:
        assert torch.equal(pm[:n], p[:n])
    if with_bf:
        assert torch.equal(pb[:n], pm[:n].to(BF16)) and torch.equal(pb[n:], torch.full_like(pb[n:], SENT))


@pytest.mark.parametrize('n', [1, 2, 3, 4, 1001, 1002, 1003, 50_000_000])
def test_sumsq(ops, n):
    g = torch.Generator(device=dev()).manual_seed(n % 9973)
    x = torch.randn(n + 4, generator=g, device=dev()) * torch.pow(10.0, torch.rand(n + 4, generator=g, device=dev()) * 8 - 4)
    x[n:] = float('nan')                                    # a read past n poisons the sum
    ref = x[:n].double().pow(2).sum()
    # r = 1e-5: every partial sum is of non-negative terms, so the error is relative to the result
    for start, acc in ((float('nan'), False), (2.5, True)):
        ws = torch.tensor([start, SENT], device=dev())
        ops.sumsq(x[:n], ws, accumulate=acc)
        want = ref + (2.5 if acc else 0.0)
        check(f'sumsq n={n} accumulate={acc}', ws[0], want, 1e-5 * want.abs())
        assert float(ws[1]) == SENT


def test_snradam_step_segments(ops):
    """4 steps on a 3-segment arena against oracle.snradam_step in fp64: a live segment with weight decay, a frozen one (lr < 0:
    p, m, v and the bf16 shadow bit-unchanged) and one at lr == 0 (parameters unchanged, moments advance); grad_scale != 1"""
    from oracle import reference_model as orc
    sizes = [1000, 520, 2052]
    ends = np.cumsum(sizes)
    n = int(ends[-1])
    lrs, wds = [3e-3, -1.0, 0.0], [0.1, 0.0, 0.05]
    b1, b2, eps, gscale = 0.9, 0.999, 1e-8, 0.25
    b1f, b2f = float(np.float32(b1)), float(np.float32(b2))
    p = rnd(n, seed=1)
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    m[ends[0]:ends[1]], v[ends[0]:ends[1]] = 0.125, 0.5     # a frozen segment's state is not even read
    pb = p.to(BF16)
    seg_end = torch.tensor(ends, dtype=torch.long, device=dev())
    seg_lr, seg_wd = torch.tensor(lrs, device=dev()), torch.tensor(wds, device=dev())
    lr32, wd32 = seg_lr.double().cpu(), seg_wd.double().cpu()
    segs = [slice(0, ends[0]), slice(ends[0], ends[1]), slice(ends[1], ends[2])]
    ref_p = [p[s].double().cpu().clone() for s in segs]
    states = [{}, {}, {}]
    p_start, m_start, v_start, pb_start = p.clone(), m.clone(), v.clone(), pb.clone()
    for step in range(1, 5):
        g = rnd(n, seed=10 + step, scale=4.0)
        ops.snradam_step(p, g, m, v, pb, n, seg_end, seg_lr, seg_wd, 3, b1, b2, eps, step, grad_scale=gscale)
        for i in (0, 2):
            s, lr, wd = segs[i], float(lr32[i]), float(wd32[i])
            g64 = g[s].double().cpu() * float(np.float32(gscale))
            before, st = ref_p[i].clone(), states[i]
            m_prev = st['m'].clone() if st else torch.zeros_like(before)
            v_prev = st['v'].clone() if st else torch.zeros_like(before)
            orc.snradam_step(ref_p[i], g64, st, lr, (b1f, b2f), wd, float(np.float32(eps)))
            inv_prev = 1.0 if step == 1 else 1.0 / (1 - b1f ** (step - 1))
            tol_m = 1e-5 * st['m'].abs() + 4 * U32 * (b1f * m_prev.abs() + (1 - b1f) * g64.abs())
            tol_v = 1e-5 * st['v'].abs() + 6 * U32 * (b2f * v_prev + (1 - b2f) * (g64.abs() + m_prev.abs() * inv_prev) ** 2)
            upd = (before * (1 - lr * wd) - ref_p[i]).abs()                 # lr |m_hat / (sqrt(v_hat) + eps)|
            tol_p = (1e-5 * ref_p[i].abs() + 4 * U32 * (before.abs() + upd)
                     + upd * (tol_m / st['m'].abs().clamp_min(1e-300) + tol_v / st['v'].abs().clamp_min(1e-300)))
            tag = f'snradam step {step} segment {i}'
            check(f'{tag} m', m[s].cpu(), st['m'], tol_m)
            check(f'{tag} v', v[s].cpu(), st['v'], tol_v)
            check(f'{tag} p', p[s].cpu(), ref_p[i], tol_p)
            # the kernel's fp32 state is what the next step starts from: carry it, so each step is compared on its own
            st['m'], st['v'], ref_p[i] = m[s].double().cpu().clone(), v[s].double().cpu().clone(), p[s].double().cpu().clone()
        assert torch.equal(pb[segs[0]], p[segs[0]].to(BF16)) and torch.equal(pb[segs[2]], p[segs[2]].to(BF16))
        f = segs[1]
        assert torch.equal(p[f], p_start[f]) and torch.equal(m[f], m_start[f]) and torch.equal(v[f], v_start[f]) and torch.equal(pb[f], pb_start[f])
        assert torch.equal(p[segs[2]], p_start[segs[2]]), 'lr == 0 moved the parameters'
    assert float(m[segs[2]].abs().min()) > 0 and float(v[segs[2]].min()) > 0, 'lr == 0: the moments must advance'


# --------------------------------------------------------------------------------------------------------------- small ones
@pytest.mark.parametrize('B,R,C', [(3, 768, 196), (2, 197, 768), (130, 5, 7), (1, 1, 1)])
def test_transpose_last2(ops, B, R, C):
    src = rnd(B, R, C, seed=R)
    for which in ('both', 'f32', 'bf16'):
        dst = nans(B * C * R + 4) if which != 'bf16' else None
        dstb = nans(B * C * R + 4, dtype=BF16) if which != 'f32' else None
        for t in (dst, dstb):
            if t is not None:
                t[B * C * R:] = SENT
        ops.transpose_last2(src, dst, dstb, B, R, C)
        want = src.transpose(1, 2).contiguous().flatten()
        if dst is not None:
            assert torch.equal(dst[:-4], want) and torch.equal(dst[-4:], torch.full_like(dst[-4:], SENT))
        if dstb is not None:
            assert torch.equal(dstb[:-4], want.to(BF16)) and torch.equal(dstb[-4:], torch.full_like(dstb[-4:], SENT))


@pytest.mark.parametrize('M,N,K', [(3, 48, 768), (64, 96, 768), (1, 1, 1), (130, 50, 100)])
def test_gemm_f32(ops, M, N, K):
    """fp32 all the way: inputs with 24 significant bits (not bf16-representable) reach the output with no operand rounding"""
    x, P = rnd(M, K, seed=K), rnd(K, N, seed=N + 1)
    x, P = x * (1 + 2.0 ** -20), P * (1 - 2.0 ** -19)       # low mantissa bits in use
    assert not torch.equal(x, x.to(BF16).float())
    z = nans(M * N + 4)
    z[M * N:] = SENT
    ops.gemm_f32(x, P, z[:M * N].view(M, N), M, N, K)
    ref = x.double() @ P.double()
    bound = K * 2.0 ** -24 * (x.double().abs() @ P.double().abs())
    check(f'gemm_f32 {M}x{N}x{K}', z[:M * N].view(M, N), ref, bound)
    assert torch.equal(z[M * N:], torch.full_like(z[M * N:], SENT))


@pytest.mark.parametrize('n', [4, 1000, 1024 + 4, 16 * 1024])
@pytest.mark.parametrize('flag', [0, 1, 7])
def test_select_rows(ops, flag, n):
    a, b = rnd(n, seed=1), rnd(n, seed=2)
    out = nans(n + 4)
    out[n:] = SENT
    ops.select_rows(torch.tensor([flag], dtype=torch.int32, device=dev()), a, b, out, n)
    assert torch.equal(out[:n], a if flag else b) and torch.equal(out[n:], torch.full_like(out[n:], SENT))
    refused(lambda: ops.select_rows(torch.tensor([flag], dtype=torch.int32, device=dev()), a, b, out, n - 1), 'i2t_select_rows')


@pytest.mark.parametrize('L,tmax,off,max_block', [(12, 256, 64, 320), (2, 40, 8, 48)])       # nano-mini, its fixture-size twin
def test_sparse_step_setup(ops, L, tmax, off, max_block):
    """the rank / member tables as decoding.py builds them from a sparse decoder's kept-position sets (layers.py: the first n_cls
    positions always, then a seeded permutation; half of max_block kept), at the first, a middle and the last text position"""
    from image2text_amd import decoding
    rank, member = np.zeros((L, tmax), dtype=np.int32), np.zeros((L, tmax), dtype=np.int32)
    for l in range(L):
        gen = np.random.Generator(np.random.PCG64(seed=l))
        full = np.concatenate([np.arange(off), gen.permutation(max_block - off) + off])
        idx = np.sort(full[:max_block // 2])
        text = np.zeros(off + tmax, dtype=np.int32)
        text[idx[idx < off + tmax]] = 1
        member[l] = text[off:]
        rank[l] = np.cumsum(member[l]) - member[l]
    kpos = decoding.slot_positions(member)
    rk, mb = torch.from_numpy(rank).to(dev()), torch.from_numpy(member).to(dev())
    for pos in (0, tmax // 2 + 1, tmax - 1, tmax + 5):      # past the window: clamped to the last position
        lpos = torch.full((L + 2,), -9, dtype=torch.int32, device=dev())
        lmem = torch.full((L + 2,), -9, dtype=torch.int32, device=dev())
        ops.sparse_step_setup(torch.tensor([pos], dtype=torch.int32, device=dev()), rk, mb, lpos, lmem, L, tmax)
        q = min(pos, tmax - 1)
        lp, lm = lpos.cpu().numpy(), lmem.cpu().numpy()
        assert (lp[:L] == rank[:, q]).all() and (lm[:L] == member[:, q]).all()
        assert (lp[L:] == -9).all() and (lm[L:] == -9).all()
        for l in range(L):                                  # a kept position sits at the slot the setup names
            if member[l, q]:
                assert kpos[l, lp[l]] == q


def test_beam_advance(ops):
    """the step counters of the captured beam step: both advance while the search runs, ctrl[1] (a live beam was seen this step)
    is consumed, and a step that saw none raises the done flag, after which nothing moves"""
    i32 = lambda *xs: torch.tensor(xs, dtype=torch.int32, device=dev())
    for counters, ctrl, want_counters, want_ctrl in (((5, 9, -3), (0, 1, -3), (6, 10, -3), (0, 0, -3)),
                                                    ((5, 9, -3), (0, 0, -3), (6, 10, -3), (1, 0, -3)),
                                                    ((5, 9, -3), (1, 1, -3), (5, 9, -3), (1, 0, -3))):
        c, k = i32(*counters), i32(*ctrl)
        ops.beam_advance(c, k)
        assert c.tolist() == list(want_counters) and k.tolist() == list(want_ctrl), (counters, ctrl, c.tolist(), k.tolist())
