"""float64 statements of the convolution kernels (csrc/conv_mfma.hip, csrc/conv.hip) on the host, with the kernels' rounding points
restated, the per-element bounds that follow from them, and the case table of tests/test_conv_kernels_gpu.py.

Everything here is plain torch on the CPU in float64 (no MIOpen, nothing from the GPU), tensors are logical NCHW, and every
reference comes with S = the same sum over |terms|, so that a bound is derived per element from the operands:

    bf16 output:  |got - ref| <= 2^-8 |ref| + (n + 8) 2^-24 S + flip (+ the GELU' allowance of backward-data)
    fp32 output:  |got - ref| <= 2^-23 |ref| + (n + 8) 2^-24 S + flip

n = terms on the longest fp32 path (36 CP forward / backward-data, B H W backward-weight); ``flip`` is the one operand rounding
that float64 cannot reproduce bit for bit -- the kernel's fp32 gelu_tanh followed by the bf16 pack: an activation whose float64
GELU lies within the fp32 error of a bf16 rounding tie may come out one bf16 ulp away, and flip is the convolution of |W| (|dy|)
with that per-element ulp map.  DESIGN.md "Convolution kernels against fp64"."""
import itertools
import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from test_row_kernels_gpu import TINY, _gelu_tanh64, bf16_round

F32, F64 = torch.float32, torch.float64
E8, U32, U24 = 2.0 ** -8, 2.0 ** -23, 2.0 ** -24
# csrc/conv_route.h: TS, KS, NCHW_GRP (the MFMA kernels' tile edge, kernel size, NCHW store group) and TILE (the generic path's tile edge)
TS, KS, GRP = 16, 6, 4
TILE = 32
NCHW_F32, NCHW_BF16, NHWC_BF16 = 0, 1, 2                    # include/i2t.h layouts
II_MAX = 0.25                                               # condition (ii): median(bound) <= rms(ref) / (4 sqrt n)


def pad8(c):
    return 8 if c <= 8 else (16 if c <= 16 else 32)


# ------------------------------------------------------------------------------------------------------------ the three sums
def corr(a, w, before):
    """out[b][o][y][x] = sum_{i,ky,kx} w[o][i][ky][kx] a[b][i][y + ky - before][x + kx - before], zero outside the image"""
    k = w.shape[-1]
    B, _, H, W = a.shape
    ap = F.pad(a, (before, k - 1 - before, before, k - 1 - before))
    out = torch.zeros(B, w.shape[0], H, W, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum('oi,bihw->bohw', w[:, :, ky, kx], ap[:, :, ky:ky + H, kx:kx + W])
    return out


def mirrored(w):
    """backward-data weights: roles swapped, taps mirrored -- wt[i][o][ky][kx] = w[o][i][k-1-ky][k-1-kx]"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def wgrad(dy, a, before, k):
    """out[o][i][ky][kx] = sum_{b,y,x} dy[b][o][y][x] a[b][i][y + ky - before][x + kx - before]"""
    B, _, H, W = a.shape
    ap = F.pad(a, (before, k - 1 - before, before, k - 1 - before))
    out = torch.zeros(dy.shape[1], a.shape[1], k, k, dtype=F64)
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', dy, ap[:, :, ky:ky + H, kx:kx + W])
    return out


# ------------------------------------------------------------------------------------------------------------------ staging
def stage_image(x):
    """the fp32 image as the MFMA kernels stage it: rounded to bf16 -> (a, ulp map = 0)"""
    a = bf16_round(x.double())
    return a, torch.zeros_like(a)


def stage_gelu(pre):
    """stored bf16 pre-activation -> (a = bf16(gelu_tanh(pre)), per-element ulp map of the values the fp32 GELU may round the
    other way).  g = m 2^e with |m| in [0.5, 1): the bf16 ulp of g's binade is 2^(e - 8), the ties lie half an ulp from the grid."""
    x = pre.double()
    g, _, _, rel, _ = _gelu_tanh64(x)
    a = bf16_round(g)
    _, e = torch.frexp(g)
    ulp = torch.ldexp(torch.ones_like(g), e - 8)
    dist = ulp / 2 - (g - a).abs()
    umap = torch.where((dist <= rel * g.abs()) & (g != 0), ulp, torch.zeros_like(g))
    # a GELU this small comes from a sigmoid near the fp32 flush threshold: the kernel may store 0 or a few ulps away
    umap = torch.where((g != 0) & (g.abs() < 2.0 ** -100), g.abs() + TINY, umap)
    return a, umap


def stage_gelu_f32(pre):
    """csrc/conv.hip keeps gelu_tanh(pre) in fp32 (no bf16 pack) -> (a = float64 GELU, per-element absolute error of the fp32 one)"""
    g, _, _, rel, _ = _gelu_tanh64(pre.double())
    return g, (rel + U24) * g.abs() + TINY


# ------------------------------------------------------------------------------------------------ references with their bounds
def _res(ref, S, n, extra, f32_out=False):
    bound = (U32 if f32_out else E8) * ref.abs() + (n + 8) * U24 * S + extra
    return SimpleNamespace(ref=ref, S=S, n=n, extra=extra, bound=bound)


def forward(a, umap, w, bias, n=None, wround=True, before=None):
    """y = bias + sum W_b a (padding 2 before, 3 after at k = 6).  wround=False: fp32 weights (csrc/conv.hip)"""
    k = w.shape[-1]
    before = (k - 1) // 2 if before is None else before
    wb = bf16_round(w.double()) if wround else w.double()
    b = torch.zeros(w.shape[0], dtype=F64) if bias is None else bias.double()
    ref = corr(a, wb, before) + b.view(1, -1, 1, 1)
    S = corr(a.abs(), wb.abs(), before) + b.abs().view(1, -1, 1, 1)
    flip = corr(umap, wb.abs(), before) if bool((umap != 0).any()) else torch.zeros_like(ref)
    return _res(ref, S, 36 * pad8(a.shape[1]) if n is None else n, flip)


def backward_data(dy, w, pre, n=None, wround=True):
    """dx = gelu_tanh'(pre) sum_{co,taps} W_b[co][ci][ky][kx] dy[co][y - ky + 2][x - kx + 2]  (the mirrored sum: padding 3 before, 2
    after at k = 6); pre None: no GELU' epilogue (csrc/conv.hip with in_gelu = 0)"""
    k = w.shape[-1]
    wb = mirrored(bf16_round(w.double()) if wround else w.double())
    before = k - 1 - (k - 1) // 2
    v = corr(dy, wb, before)
    Sv = corr(dy.abs(), wb.abs(), before)
    n = 36 * pad8(dy.shape[1]) if n is None else n
    if pre is None:
        return _res(v, Sv, n, torch.zeros_like(v))
    _, grad, terms, rel, flush = _gelu_tanh64(pre.double())
    r = _res(v * grad, Sv * terms, n, v.abs() * (rel * terms + flush))
    r.v = v
    return r


def backward_weight(dy, a, umap, dw0, db0, k=KS, n=None):
    """dW = dW0 + sum_{b,y,x} dy a (padding (k-1)/2 before), db = db0 + sum dy -> (dW result, db result); fp32 outputs"""
    before = (k - 1) // 2
    n = dy.shape[0] * dy.shape[2] * dy.shape[3] if n is None else n
    flip = wgrad(dy.abs(), umap, before, k) if bool((umap != 0).any()) else 0.0
    rw = _res(dw0.double() + wgrad(dy, a, before, k), dw0.double().abs() + wgrad(dy.abs(), a.abs(), before, k), n, flip, f32_out=True)
    rb = None
    if db0 is not None:
        rb = _res(db0.double() + dy.sum((0, 2, 3)), db0.double().abs() + dy.abs().sum((0, 2, 3)), n, 0.0, f32_out=True)
    return rw, rb


def with_bias(r, bias):
    b = bias.double().view(1, -1, 1, 1)
    return _res(r.ref + b, r.S + b.abs(), r.n, r.extra)


def case_reference(c, d):
    """the reference of one MFMA case on inputs ``d``: forward -> result without bias (with_bias adds it); backward-data -> result;
    backward-weight -> (dW result, db result | None)"""
    if c.op == 'fwd':
        a, um = stage_image(d.x) if c.src == 'img' else stage_gelu(d.x)
        return forward(a, um, d.w, None)
    if c.op == 'bwd_data':
        return backward_data(d.dy.double(), d.w, d.x)
    a, um = stage_image(d.x) if c.src == 'img' else stage_gelu(d.x)
    return backward_weight(d.dy.double(), a, um, d.dw0, d.db0 if c.db else None)


def condition_ii(r):
    """median(bound) sqrt(n) / rms(ref): at most II_MAX, so the bound stays well under the size of one term"""
    rms = float(r.ref.pow(2).mean().sqrt())
    return float(torch.as_tensor(r.bound, dtype=F64).expand_as(r.ref).median()) * math.sqrt(r.n) / max(rms, 1e-300)


def kernel_rounded(r, f32_out=False):
    """the reference rounded where the kernel rounds its result"""
    return r.ref.to(F32).to(F64) if f32_out else bf16_round(r.ref)


# -------------------------------------------------------------------------------------------------------------------- cases
SHAPES = [(5, 7), (16, 16), (17, 33), (40, 24), (24, 66), (16, 64), (16, 80), (32, 128)]
WIDE = (16, 132)                                            # tiles_x = 9: two full store groups plus one
GRP_SHAPES = [(16, 64), (16, 80), (32, 128), WIDE, (17, 33), (5, 7)]      # tiles_x 4, 5, 8, 9, 3 (ragged, W % 4 = 1), 1
MAX_PIXELS = 2 * 40 * 72


def _case(op, **kw):
    c = SimpleNamespace(op=op, **kw)
    c.id = '-'.join([op] + ([kw['name']] if kw.get('name') else []) +
                    [f'{k}{v}' for k, v in kw.items() if k not in ('name', 'H', 'W', 'B')] + [f"B{kw['B']}x{kw['H']}x{kw['W']}"])
    return c


def _batch(i, H, W, cap=MAX_PIXELS):
    return max(1, min(1 + i % 3, cap // (H * W)))


def _fwd_cases():
    pairs = [('img', 1, 8, 'nhwc'), ('img', 3, 32, 'nhwc'), ('img', 4, 16, 'nhwc'), ('img', 5, 24, 'nhwc'), ('img', 8, 16, 'nhwc'),
             ('img', 8, 32, 'nhwc'), ('img', 3, 5, 'nchw'), ('img', 4, 32, 'nchw'), ('img', 5, 16, 'nchw'), ('img', 8, 32, 'nchw'),
             ('img', 1, 8, 'nchw'), ('img', 3, 8, 'nhwc'),
             ('nhwc', 8, 8, 'nhwc'), ('nhwc', 8, 24, 'nhwc'), ('nhwc', 16, 16, 'nhwc'), ('nhwc', 16, 32, 'nhwc'), ('nhwc', 32, 16, 'nhwc'),
             ('nhwc', 32, 32, 'nhwc'), ('nhwc', 32, 24, 'nhwc'), ('nhwc', 32, 8, 'nhwc'), ('nhwc', 8, 5, 'nchw'), ('nhwc', 8, 32, 'nchw'),
             ('nhwc', 16, 8, 'nchw'), ('nhwc', 16, 32, 'nchw'), ('nhwc', 32, 16, 'nchw'), ('nhwc', 32, 32, 'nchw'), ('nhwc', 32, 5, 'nchw')]
    out = []
    for i, (src, ci, co, dst) in enumerate(pairs):
        shapes = GRP_SHAPES if (dst == 'nchw' and pad8(ci) >= 16 and co in (8, 32, 16)) else [SHAPES[(3 * i + 2) % len(SHAPES)]]
        if src == 'nhwc' and ci == 32 and dst == 'nhwc' and co in (16, 32):
            shapes = [(17, 33), (24, 66)]                   # the swizzled forward: ragged row + column, W % 4 = 1 and 2
        for j, (H, W) in enumerate(shapes):
            out.append(_case('fwd', src=src, Cin=ci, Cout=co, dst=dst, B=_batch(i + j, H, W), H=H, W=W))
    return out


def _bwd_data_cases():
    out = [_case('bwd_data', name='production', dyl='nhwc', Cin=16, Cout=32, B=2, H=40, W=24)]
    combos = [('nhwc', 16, 32)] * 4 + [('nchw', ci, co) for co in (8, 12, 16, 24, 32) for ci in (8, 16)] + \
             [('nhwc', ci, co) for co in (8, 16, 32) for ci in (8, 16) if (ci, co) != (16, 32)]
    extra = [(17, 33), (24, 66), (5, 7), (16, 80)]
    for i, (dyl, ci, co) in enumerate(combos):
        H, W = extra[i] if i < 4 else SHAPES[(3 * i + 1) % len(SHAPES)]
        out.append(_case('bwd_data', dyl=dyl, Cin=ci, Cout=co, B=_batch(i, H, W), H=H, W=W))
    return out


# backward-weight: B H W <= 1700.  Its fp32 sum has n = B H W terms and (n + 8) 2^-24 S grows like n^2, so condition (ii) holds with
# margin only up to there (0.24 at 1 x 16 x 132); the wide shape is for the forward's store groups
BW_SHAPES_B3 = [(5, 7), (16, 16), (17, 33)]
BW_SHAPES_B1 = [(40, 24), (24, 66), (16, 64), (16, 80), (16, 16)]


def _bwd_weight_cases():
    out = [_case('bwd_weight', name='production', src='nhwc', dyl='nhwc', Cin=16, Cout=32, db=True, B=1, H=40, W=24)]
    i = 0
    for src, ci in (('img', 3), ('img', 5), ('img', 1), ('img', 4), ('img', 8), ('nhwc', 8), ('nhwc', 16)):
        for cop in (16, 32):
            for dyl in ('nchw', 'nhwc'):
                co = {('nchw', 16): (5, 12, 16), ('nchw', 32): (24, 32, 17), ('nhwc', 16): (8, 16, 16), ('nhwc', 32): (24, 32, 32)}[(dyl, cop)][i % 3]
                B = 3 if i % 2 else 1
                H, W = (BW_SHAPES_B3[(i // 2) % 3] if B == 3 else BW_SHAPES_B1[(i // 2) % 5])
                out.append(_case('bwd_weight', src=src, dyl=dyl, Cin=ci, Cout=co, db=(i % 4 != 2), B=B, H=H, W=W))
                i += 1
    return out


DET_CASES = [_case('bwd_weight', name='det', src='img', dyl='nchw', Cin=3, Cout=8, db=True, B=3, H=17, W=33),
             _case('bwd_weight', name='det', src='nhwc', dyl='nhwc', Cin=8, Cout=16, db=True, B=3, H=17, W=33),
             _case('bwd_weight', name='det', src='nhwc', dyl='nhwc', Cin=16, Cout=32, db=True, B=3, H=17, W=33)]
FWD_CASES, BWD_DATA_CASES, BWD_WEIGHT_CASES = _fwd_cases(), _bwd_data_cases(), _bwd_weight_cases()
# nchw_to_nhwc: (C, W, misaligned view)
T_CASES = [(C, W, False) for C in (8, 16, 24, 32) for W in (8, 63, 64, 65, 72)] + [(32, 72, True), (32, 8, True)]


def _src(layout):
    return {'img': 'SRC_NCHW_F32', 'nchw': 'SRC_NCHW_BF16', 'nhwc': 'SRC_NHWC_BF16'}[layout]


def route(c):
    """the kernel instantiation a case launches: csrc/conv_route.h (conv6_route, conv6_bwd_weight_route) restated;
    tests/test_conv_route_cpu.py holds the two together for every case.  The staging of an fp32 image is a run-time choice inside
    one instantiation (pixel chunks for <= 4 channels, planar otherwise): the /chunks | /planar suffix notes it, the header does not."""
    b = lambda v: 'true' if v else 'false'
    if c.op == 'fwd':
        cp, nt = pad8(c.Cin), 1 if c.Cout <= 16 else 2
        sub = ('/chunks' if c.Cin <= 4 else '/planar') if c.src == 'img' else ''
        return f"conv_mfma_kernel<{cp}, {nt}, {_src(c.src)}, {b(c.src == 'nhwc')}, false, {b(c.dst == 'nchw')}>{sub}"
    if c.op == 'bwd_data':                                   # roles swapped: reduction over the forward's Cout, NT = 1 (Cin <= 16)
        return f'conv_mfma_kernel<{pad8(c.Cout)}, 1, {_src(c.dyl)}, false, true, false>'
    if c.op == 'bwd_weight':
        sub = ('/chunks' if c.Cin <= 4 else '/planar') if c.src == 'img' else ''
        return (f"conv_mfma_bwd_weight_kernel<{pad8(c.Cin)}, {16 if c.Cout <= 16 else 32}, {_src(c.dyl)}, {_src(c.src)}, "
                f"{b(c.src == 'nhwc')}>{sub}")
    raise ValueError(c.op)


def transpose_route(C, W, aligned):
    return 'nchw_to_nhwc32_kernel' if (C == 32 and W % 8 == 0 and aligned) else 'nchw_to_nhwc_kernel'


def all_routes():
    """every instantiation i2t_conv6_fwd / i2t_conv6_bwd_data / i2t_conv6_bwd_weight / i2t_nchw_to_nhwc_bf16 can launch: the set the
    *_instantiated predicates of csrc/conv_route.h state (tests/test_conv_route_cpu.py compares the two), each image kernel once
    per staging form"""
    r = set()
    for nt, nchw, sub in itertools.product((1, 2), ('false', 'true'), ('/chunks', '/planar')):
        r.add(f'conv_mfma_kernel<8, {nt}, SRC_NCHW_F32, false, false, {nchw}>{sub}')
    for cp, nt, nchw in itertools.product((8, 16, 32), (1, 2), ('false', 'true')):
        r.add(f'conv_mfma_kernel<{cp}, {nt}, SRC_NHWC_BF16, true, false, {nchw}>')
    for cp, s in itertools.product((8, 16, 32), ('SRC_NCHW_BF16', 'SRC_NHWC_BF16')):
        r.add(f'conv_mfma_kernel<{cp}, 1, {s}, false, true, false>')
    for cop, s, sub in itertools.product((16, 32), ('SRC_NCHW_BF16', 'SRC_NHWC_BF16'), ('/chunks', '/planar')):
        r.add(f'conv_mfma_bwd_weight_kernel<8, {cop}, {s}, SRC_NCHW_F32, false>{sub}')
    for cp, cop, s in itertools.product((8, 16), (16, 32), ('SRC_NCHW_BF16', 'SRC_NHWC_BF16')):
        r.add(f'conv_mfma_bwd_weight_kernel<{cp}, {cop}, {s}, SRC_NHWC_BF16, true>')
    return r | {'nchw_to_nhwc32_kernel', 'nchw_to_nhwc_kernel'}


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(c, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((c.op, c.Cin, c.Cout, c.B, c.H, c.W, salt)).encode()) % (2 ** 31))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def inputs(c, mode='n01', k=KS):
    """CPU fp32 tensors in logical NCHW, every value already representable in the type the kernel reads it as.
    mode 'n01': N(0, 1) operands, weights scaled by 1 / sqrt(terms);  'lattice': small integers, every product and sum exact;
    'lattice_sparse' (backward-data): full-range integers, dy non-zero at one pixel in 7 x 7."""
    g = _gen(c, mode)
    B, H, W, ci, co = c.B, c.H, c.W, c.Cin, c.Cout
    r16 = lambda t: t.to(torch.bfloat16).to(F32)
    d = SimpleNamespace()
    if mode == 'n01':
        d.w = torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k)
        d.bias = 0.1 * torch.randn(co, generator=g)
        if c.op == 'bwd_data':
            d.w = d.w * math.sqrt(ci / co)                  # the reduction runs over the forward's Cout
        d.x = torch.randn(B, ci, H, W, generator=g)
        if getattr(c, 'src', 'nhwc') != 'img':
            d.x = r16(d.x)                                  # stored bf16 pre-activation
        d.dy = r16(torch.randn(B, co, H, W, generator=g))
        d.dw0, d.db0 = torch.randn(co, ci, k, k, generator=g), torch.randn(co, generator=g)
        return d
    small = c.op == 'bwd_data' and mode == 'lattice'        # the GELU' factor 0.5 must leave 8 significant bits: {-1, 0, 1}
    d.w = _ints(g, -1, 1, co, ci, k, k) if small else _ints(g, -3, 3, co, ci, k, k)
    d.bias = _ints(g, -3, 3, co)
    if getattr(c, 'src', 'nhwc') == 'img':
        d.x = _ints(g, -4, 4, B, ci, H, W)
    else:
        d.x = 4.0 * _ints(g, 0, 2, B, ci, H, W)             # {0, 4, 8}: gelu(4) and gelu(8) round to 4 and 8 in bf16
    d.dy = _ints(g, -1, 1, B, co, H, W) if small else _ints(g, -4, 4, B, co, H, W)
    if mode == 'lattice_sparse':
        m = torch.zeros(H, W)
        m[(c.B + 1) % 7::7, (c.Cout // 8) % 7::7] = 1
        d.dy = d.dy * m
    if c.op == 'bwd_data':
        d.x = torch.zeros(B, ci, H, W)                      # pre-activation 0: gelu'(0) = 1/2 exactly
    d.dw0, d.db0 = _ints(g, -3, 3, co, ci, k, k), _ints(g, -3, 3, co)
    return d


def lattice_stage(x, src):
    """staged values of a lattice input: the integers themselves (gelu(4) -> 4, gelu(8) -> 8 after the bf16 pack)"""
    if src != 'img':
        a, umap = stage_gelu(x)
        assert torch.equal(a, x.double()) and not bool((umap != 0).any()), 'lattice activations must survive the staging GELU exactly'
    return x.double()


def assert_exact(r, dgelu=False):
    """every partial sum of a lattice case stays below 2^24 (S bounds them all), and under the GELU' epilogue the value in front
    of the store has at most 8 significant bits, so that a factor 1 +- 1e-7 cannot move it across a bf16 tie"""
    assert float(torch.as_tensor(r.S).max()) < 2.0 ** 24
    if dgelu:
        assert float(r.S.max()) < 2.0 ** 24 and torch.equal(bf16_round(r.ref), r.ref), 'GELU\' case: pre-store values must be bf16 numbers'


IMPULSE_AT = lambda H, W: [(0, 0), (15, 15), (16, 16), (H - 1, W - 1), (3, 20), (H - 2, 5)]      # (y, x); x = 20, 5: bit 2 set


def impulse_fwd(Cout, H, W, y, x):
    """CP = 32 forward (staging GELU): one pixel with channel c at {0, 4, 8}[(c + c // 16) % 3] -- every channel differs from the one 16
    channels away, which is what a swapped chunk pair exchanges -- and weights that differ per (tap, channel, output)"""
    c = torch.arange(32)
    pre = torch.zeros(1, 32, H, W)
    pre[0, :, y, x] = 4.0 * ((c + c // 16) % 3)
    i = torch.arange(Cout * 32 * 36).view(Cout, 32, 6, 6)
    w = ((i * 5 + i // 36 + i // 1152) % 7 - 3).to(F32)
    return pre, w


def impulse_bwd_data(Cin, H, W, y, x):
    """CP = 32 backward-data: dy is one pixel whose 32 channels are 1 .. 32; W[co][ci][tap] is non-zero for ONE co per (tap, ci), so
    every output is a single product (<= 96, exact after the factor 1/2) that names the channel it read"""
    dy = torch.zeros(1, 32, H, W)
    dy[0, :, y, x] = torch.arange(1, 33).to(F32)
    w = torch.zeros(32, Cin, 6, 6)
    for ci in range(Cin):
        for tap in range(36):
            w[(5 * tap + 3 * ci) % 32, ci, tap // 6, tap % 6] = 1 + (tap + ci) % 3
    return dy, w
