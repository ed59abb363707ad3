"""The convolution kernels (csrc/conv_mfma.hip: every instantiation i2t_conv6_fwd / i2t_conv6_bwd_data / i2t_conv6_bwd_weight /
i2t_nchw_to_nhwc_bf16 can launch; csrc/conv.hip: the generic k = 4 / k = 6 path) against the float64 statements of tests/conv_ref.py.

Every case runs twice: N(0, 1) operands against the derived per-element bound (no free atol; DESIGN.md "Convolution kernels against
fp64"), and integer lattice operands, for which every product and partial sum is exact and the output must be bit-identical to the
rounded reference.  The swizzled 32-channel kernels also get single-pixel impulses.  Every operand is a view into a larger
allocation: NaN around the inputs (a vector load or clamped index that strays brings NaN into a result), a sentinel around and NaN
inside the outputs.  The case table names the instantiation of every case (conv_ref.route) and must cover the full list.
Worst error / bound per tensor goes to I2T_REPORT_DIR/parity_report_conv_kernels.json."""
import json
import os

import pytest
import torch

import conv_ref as R
from test_row_kernels_gpu import BF16, F32, F64, SENT, _gelu_tanh64, bf16_round, check, dev, nans, refused  # noqa: F401

pytestmark = pytest.mark.gpu

REPORT = {}
ID = lambda c: c.id


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


@pytest.fixture(scope='module', autouse=True)
def write_report():
    yield
    out = os.environ.get('I2T_REPORT_DIR', 'test_reports')
    os.makedirs(out, exist_ok=True)
    worst = {}
    for row in REPORT.values():
        for k, u in row.items():
            if not k.startswith('ii '):
                worst[k] = max(worst.get(k, 0.0), u)
    with open(os.path.join(out, 'parity_report_conv_kernels.json'), 'w') as fh:
        json.dump({'worst_error_over_bound': worst, 'cases': REPORT}, fh, indent=1, sort_keys=True)


# --------------------------------------------------------------------------------------------------------- guarded buffers
def _guard(row):
    return (max(64, row) + 15) // 16 * 16                   # at least one image row and 64 elements; keeps the view 32-byte aligned


class Out:
    """an output view with NaN inside and SENT around it"""

    def __init__(self, shape, dtype, row, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.g, self.n = _guard(row), n
        self.buf = torch.full((2 * self.g + n,), SENT, dtype=dtype, device=dev())
        self.v = self.buf[self.g:self.g + n].view(shape)
        self.v.copy_(fill.to(dtype)) if fill is not None else self.v.fill_(float('nan'))

    def intact(self):
        return bool((self.buf[:self.g] == SENT).all()) and bool((self.buf[self.g + self.n:] == SENT).all())


def guarded(t, dtype, row, shift=0):
    """an input view with NaN before and after it (shift: elements by which the view is moved off its alignment)"""
    g, n = _guard(row), t.numel()
    buf = nans(2 * g + n + shift, dtype=dtype)
    v = buf[g + shift:g + shift + n].view(t.shape)
    v.copy_(t.to(dtype))
    return v


@pytest.fixture(scope='module')
def ws():
    """weight workspace and backward-weight scratch, sized as engine.py sizes them, inside guards"""
    from image2text_amd import ops as _ops
    return Out((_ops.CONV6_WS_ELEMS,), F32, 64), Out((_ops.CONV6_SCRATCH_FLOATS,), F32, 64)


def lay(t, layout):
    """logical NCHW (CPU) -> the memory order of ``layout``"""
    return t.permute(0, 2, 3, 1).contiguous() if layout == 'nhwc' else t.contiguous()


def unlay(v, layout):
    t = v.detach().cpu().to(F64)
    return t.permute(0, 3, 1, 2) if layout == 'nhwc' else t


LAYOUT = {'img': R.NCHW_F32, 'nchw': R.NCHW_BF16, 'nhwc': R.NHWC_BF16}


def done(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.intact(), 'a guard region around an output was written'


def record(c, name, units, r=None):
    row = REPORT.setdefault(c if isinstance(c, str) else c.id, {})
    row[name] = max(row.get(name, 0.0), units)
    if r is not None:
        ii = R.condition_ii(r)
        row['ii ' + name] = ii
        assert ii <= R.II_MAX, f'{name}: condition (ii) {ii:.3f}'


def exact(name, got, r, f32_out=False):
    want = R.kernel_rounded(r, f32_out)
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    bad = got != want
    assert not bool(bad.any()), f'{name}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result; first at ' \
                                f'{tuple(bad.nonzero()[0].tolist())}: got {got[bad][0].item()} want {want[bad][0].item()}'


# ----------------------------------------------------------------------------------------------------------------- runners
def run_fwd(ops, ws, c, x, w, bias):
    B, H, W, ci, co = c.B, c.H, c.W, c.Cin, c.Cout
    xs = guarded(lay(x, 'nhwc' if c.src == 'nhwc' else 'nchw'), F32 if c.src == 'img' else BF16, W * ci)
    wd = guarded(w, F32, 64)
    bd = None if bias is None else guarded(bias, F32, 64)
    y = Out((B, co, H, W) if c.dst == 'nchw' else (B, H, W, co), BF16, W * co)
    ops.conv6_fwd(xs, LAYOUT[c.src], c.src == 'nhwc', wd, bd, y.v, c.dst == 'nchw', ws[0].v, B, ci, co, H, W)
    done(y, ws[0])
    return unlay(y.v, c.dst)


def run_bwd_data(ops, ws, c, dy, w, pre):
    B, H, W, ci, co = c.B, c.H, c.W, c.Cin, c.Cout
    dys = guarded(lay(dy, c.dyl), BF16, W * co)
    wd = guarded(w, F32, 64)
    ps = guarded(lay(pre, 'nhwc'), BF16, W * ci)
    dx = Out((B, H, W, ci), BF16, W * ci)
    ops.conv6_bwd_data(dys, LAYOUT[c.dyl], wd, ps, dx.v, ws[0].v, B, ci, co, H, W)
    done(dx, ws[0])
    return unlay(dx.v, 'nhwc')


def run_bwd_weight(ops, ws, c, d):
    B, H, W, ci, co = c.B, c.H, c.W, c.Cin, c.Cout
    dys = guarded(lay(d.dy, c.dyl), BF16, W * co)
    xs = guarded(lay(d.x, 'nhwc' if c.src == 'nhwc' else 'nchw'), F32 if c.src == 'img' else BF16, W * ci)
    dw = Out(tuple(d.dw0.shape), F32, 64, fill=d.dw0)
    db = Out((co,), F32, 64, fill=d.db0) if c.db else None
    ops.conv6_bwd_weight(dys, LAYOUT[c.dyl], xs, LAYOUT[c.src], c.src == 'nhwc', dw.v, None if db is None else db.v, ws[1].v, B, ci, co, H, W)
    done(dw, ws[1], *([db] if db is not None else []))
    return dw.v.detach().cpu().to(F64), (None if db is None else db.v.detach().cpu().to(F64))


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('c', R.FWD_CASES, ids=ID)
def test_conv6_fwd(ops, ws, c):
    d = R.inputs(c)
    r0 = R.case_reference(c, d)
    for bias in (None, d.bias):
        r = r0 if bias is None else R.with_bias(r0, bias)
        name = 'fwd y' + (' +bias' if bias is not None else '')
        record(c, name, check(f'{c.id} {name} [{R.route(c)}]', run_fwd(ops, ws, c, d.x, d.w, bias), r.ref, r.bound), r)
    d = R.inputs(c, 'lattice')
    R.lattice_stage(d.x, c.src)
    r0 = R.case_reference(c, d)
    for bias in (None, d.bias):
        r = r0 if bias is None else R.with_bias(r0, bias)
        R.assert_exact(r)
        exact(f'{c.id} lattice bias={bias is not None}', run_fwd(ops, ws, c, d.x, d.w, bias), r)


@pytest.mark.parametrize('co,dst', [(16, 'nhwc'), (32, 'nhwc'), (16, 'nchw'), (32, 'nchw')])
def test_conv6_fwd_impulse_swizzled(ops, ws, co, dst):
    H, W = 24, 40
    c = R._case('fwd', src='nhwc', Cin=32, Cout=co, dst=dst, B=1, H=H, W=W)
    for y, x in R.IMPULSE_AT(H, W):
        pre, w = R.impulse_fwd(co, H, W, y, x)
        a = R.lattice_stage(pre, 'nhwc')
        r = R.forward(a, torch.zeros_like(a), w, None)
        R.assert_exact(r)
        exact(f'{c.id} impulse at {(y, x)}', run_fwd(ops, ws, c, pre, w, None), r)


# ------------------------------------------------------------------------------------------------------------ backward-data
@pytest.mark.parametrize('c', R.BWD_DATA_CASES, ids=ID)
def test_conv6_bwd_data(ops, ws, c):
    d = R.inputs(c)
    r = R.case_reference(c, d)
    record(c, 'bwd_data dx', check(f'{c.id} dx [{R.route(c)}]', run_bwd_data(ops, ws, c, d.dy, d.w, d.x), r.ref, r.bound), r)
    for mode in ('lattice', 'lattice_sparse'):
        d = R.inputs(c, mode)
        r = R.case_reference(c, d)
        R.assert_exact(r, dgelu=True)
        exact(f'{c.id} {mode}', run_bwd_data(ops, ws, c, d.dy, d.w, d.x), r)


@pytest.mark.parametrize('ci,dyl', [(16, 'nhwc'), (8, 'nhwc'), (16, 'nchw')])
def test_conv6_bwd_data_impulse_swizzled(ops, ws, ci, dyl):
    H, W = 24, 40
    c = R._case('bwd_data', dyl=dyl, Cin=ci, Cout=32, B=1, H=H, W=W)
    pre = torch.zeros(1, ci, H, W)
    for y, x in R.IMPULSE_AT(H, W):
        dy, w = R.impulse_bwd_data(ci, H, W, y, x)
        r = R.backward_data(dy.double(), w, pre)
        R.assert_exact(r, dgelu=True)
        exact(f'{c.id} impulse at {(y, x)}', run_bwd_data(ops, ws, c, dy, w, pre), r)


# ---------------------------------------------------------------------------------------------------------- backward-weight
@pytest.mark.parametrize('c', R.BWD_WEIGHT_CASES, ids=ID)
def test_conv6_bwd_weight(ops, ws, c):
    assert not ops.deterministic()
    for mode in ('n01', 'lattice'):
        d = R.inputs(c, mode)
        if mode == 'lattice':
            R.lattice_stage(d.x, c.src)
        rw, rb = R.case_reference(c, d)
        dw, db = run_bwd_weight(ops, ws, c, d)
        if mode == 'n01':
            record(c, 'bwd_weight dW', check(f'{c.id} dW [{R.route(c)}]', dw, rw.ref, rw.bound), rw)
            if c.db:
                record(c, 'bwd_weight db', check(f'{c.id} db', db, rb.ref, rb.bound), rb)
        else:
            R.assert_exact(rw)
            exact(f'{c.id} lattice dW', dw, rw, f32_out=True)
            if c.db:
                R.assert_exact(rb)
                exact(f'{c.id} lattice db', db, rb, f32_out=True)


@pytest.mark.parametrize('c', R.DET_CASES, ids=ID)
def test_conv6_bwd_weight_deterministic(ops, ws, c):
    d = R.inputs(c)
    rw, rb = R.case_reference(c, d)
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        runs = [run_bwd_weight(ops, ws, c, d) for _ in range(2)]
    finally:
        ops.set_deterministic(was)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    record(c, 'bwd_weight dW deterministic', check(f'{c.id} dW [{R.route(c)}]', runs[0][0], rw.ref, rw.bound), rw)
    record(c, 'bwd_weight db deterministic', check(f'{c.id} db', runs[0][1], rb.ref, rb.bound), rb)


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize('C,W,misaligned', R.T_CASES)
def test_nchw_to_nhwc(ops, C, W, misaligned):
    B, H = 2, 3
    g = torch.Generator().manual_seed(C * 100 + W)
    src = torch.randn(B, C, H, W, generator=g).to(BF16)
    s = guarded(src, BF16, W * C, shift=1 if misaligned else 0)
    assert R.transpose_route(C, W, s.data_ptr() % 16 == 0) == ('nchw_to_nhwc_kernel' if misaligned or C != 32 or W % 8 else 'nchw_to_nhwc32_kernel')
    o = Out((B, H, W, C), BF16, W * C)
    ops.nchw_to_nhwc(s, o.v, B, C, H, W)
    done(o)
    assert torch.equal(o.v.cpu().view(torch.int16), src.permute(0, 2, 3, 1).contiguous().view(torch.int16))


def test_route_table_is_complete():
    cases = R.FWD_CASES + R.BWD_DATA_CASES + R.BWD_WEIGHT_CASES + R.DET_CASES
    got = {R.route(c) for c in cases} | {R.transpose_route(C, W, not mis) for C, W, mis in R.T_CASES}
    assert got == R.all_routes(), (sorted(R.all_routes() - got), sorted(got - R.all_routes()))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_conv6_refusals(ops, ws):
    B, H, W = 1, 16, 16
    x32 = torch.zeros(B * 40 * H * W, device=dev())
    xb = torch.zeros(B * 40 * H * W, dtype=BF16, device=dev())
    w = torch.zeros(40 * 40 * 36, device=dev())
    y = torch.full((B * 40 * H * W,), SENT, dtype=BF16, device=dev())
    dw = torch.full((40 * 40 * 36,), SENT, device=dev())
    db = torch.full((40,), SENT, device=dev())
    w_ws, scr = ws[0].v, ws[1].v
    w_ws.fill_(SENT)                                        # a refused call issues nothing: no repack, no memset
    scr.fill_(SENT)
    refused(lambda: ops.conv6_fwd(xb, 2, True, w, None, y, False, w_ws, B, 12, 16, H, W), 'NHWC input needs')
    refused(lambda: ops.conv6_fwd(xb, 2, True, w, None, y, False, w_ws, B, 24, 16, H, W), 'NHWC input needs')
    refused(lambda: ops.conv6_fwd(xb, 2, True, w, None, y, False, w_ws, B, 16, 12, H, W), 'NHWC output needs')
    refused(lambda: ops.conv6_fwd(x32, 0, False, w, None, y, False, w_ws, B, 3, 20, H, W), 'NHWC output needs')
    refused(lambda: ops.conv6_fwd(xb, 2, True, w, None, y, True, w_ws, B, 33, 16, H, W), 'i2t_conv6_fwd: bad args')
    refused(lambda: ops.conv6_fwd(xb, 2, True, w, None, y, True, w_ws, B, 16, 33, H, W), 'i2t_conv6_fwd: bad args')
    refused(lambda: ops.conv6_fwd(xb, 1, False, w, None, y, True, w_ws, B, 8, 16, H, W), 'unsupported layout combination')      # NCHW bf16 input
    refused(lambda: ops.conv6_fwd(xb, 2, False, w, None, y, True, w_ws, B, 8, 16, H, W), 'unsupported layout combination')      # NHWC without GELU
    refused(lambda: ops.conv6_fwd(x32, 0, True, w, None, y, True, w_ws, B, 3, 16, H, W), 'unsupported layout combination')      # image through GELU
    refused(lambda: ops.conv6_fwd(x32, 0, False, w, None, y, True, w_ws, B, 12, 16, H, W), 'unsupported layout combination')    # image, Cin > 8
    refused(lambda: ops.conv6_bwd_data(xb, 2, w, xb, y, w_ws, B, 32, 32, H, W), 'i2t_conv6_bwd_data: bad args')                  # Cin > 16
    refused(lambda: ops.conv6_bwd_data(xb, 2, w, xb, y, w_ws, B, 12, 32, H, W), 'i2t_conv6_bwd_data: bad args')
    refused(lambda: ops.conv6_bwd_data(xb, 2, w, xb, y, w_ws, B, 16, 33, H, W), 'i2t_conv6_bwd_data: bad args')
    refused(lambda: ops.conv6_bwd_data(xb, 2, w, xb, y, w_ws, B, 16, 24, H, W), 'dy layout')                                     # NHWC dy, 24 channels
    refused(lambda: ops.conv6_bwd_data(x32, 0, w, xb, y, w_ws, B, 16, 32, H, W), 'dy layout')
    refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, True, dw, db, scr, B, 32, 32, H, W), 'i2t_conv6_bwd_weight: bad args')    # Cin > 16
    refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, True, dw, db, scr, B, 16, 33, H, W), 'i2t_conv6_bwd_weight: bad args')
    refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, False, dw, db, scr, B, 16, 32, H, W), 'unsupported layout combination')
    refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, True, dw, db, scr, B, 12, 32, H, W), 'unsupported layout combination')
    refused(lambda: ops.conv6_bwd_weight(xb, 2, x32, 0, False, dw, db, scr, B, 12, 32, H, W), 'unsupported layout combination')
    refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, True, dw, db, scr, B, 16, 12, H, W), 'NHWC dy needs')
    refused(lambda: ops.conv_bwd_weight(xb, x32, False, dw, db, B, 3, 12, H, W, 6), 'unsupported')                               # generic: Cout
    refused(lambda: ops.conv_bwd_weight(xb, x32, False, dw, db, B, 3, 16, H, W, 5), 'unsupported')                               # generic: k
    refused(lambda: ops.conv_fwd(x32, False, w, None, y, w_ws, B, 3, 16, H, W, 5), 'kernel size 5 unsupported')
    refused(lambda: ops.conv_bwd_data(xb, w, None, False, y, w_ws, B, 3, 16, H, W, 3), 'kernel size 3 unsupported')
    for h, wd in ((0, W), (H, 0)):                                                                                               # an empty image
        refused(lambda: ops.conv6_fwd(x32, 0, False, w, None, y, True, w_ws, B, 3, 16, h, wd), 'i2t_conv6_fwd: bad args')
        refused(lambda: ops.conv6_bwd_weight(xb, 2, xb, 2, True, dw, db, scr, B, 16, 32, h, wd), 'i2t_conv6_bwd_weight: bad args')
        refused(lambda: ops.conv_fwd(x32, False, w, None, y, w_ws, B, 3, 16, h, wd, 6), 'i2t_conv_fwd: bad args')
    done(*ws)
    for t in (y, dw, db, w_ws, scr):
        assert bool((t == SENT).all())


# ------------------------------------------------------------------------------------------- the generic path (csrc/conv.hip)
# What it rounds, read from the kernels: weights stay fp32 (repacked, not rounded); the input is the fp32 image as it is, or the bf16
# tensor widened, passed through the fp32 gelu_tanh WITHOUT a bf16 pack; one fmaf chain over Cin k k terms (forward / backward-data,
# bias and GELU' after it), over the 1024 pixels of a 32 x 32 tile (backward-weight, then one atomic per tile and image); outputs
# bf16 (fwd, dX) or fp32 (dW, db).  All tensors NCHW.  The fp32 GELU's error enters as  sum |W| err  instead of a flip term.
GEN_SHAPES = [(17, 33), (40, 24)]
GEN_IN = ['f32', 'bf16+gelu', 'bf16', 'f32+gelu']


def _gen_stage(x, kind):
    if kind.endswith('+gelu'):
        return R.stage_gelu_f32(x)
    return x.double(), torch.zeros_like(x, dtype=F64)


def _gen_inputs(kind, B, ci, co, H, W, k, seed):
    c = R._case('gen', Cin=ci, Cout=co, B=B, H=H, W=W, k=k, seed=seed)
    c.src = 'img' if kind.startswith('f32') else 'nchw'
    return R.inputs(c, 'n01', k=k)


@pytest.mark.parametrize('k', [4, 6])
@pytest.mark.parametrize('kind', GEN_IN)
@pytest.mark.parametrize('co', [3, 8, 24])                 # COUT_T 4, 8 and 16 (two channel groups, the second ragged)
def test_generic_conv_fwd(ops, ws, co, kind, k):
    ci, B = 5, 2                                            # two input-channel chunks of 4, the second ragged
    H, W = GEN_SHAPES[(co + k + len(kind)) % 2]
    d = _gen_inputs(kind, B, ci, co, H, W, k, 1)
    a, err = _gen_stage(d.x, kind)
    r = R.forward(a, torch.zeros_like(a), d.w, d.bias, n=ci * k * k + 2, wround=False)
    r.bound = r.bound + R.corr(err, d.w.double().abs(), (k - 1) // 2)
    xs = guarded(d.x, F32 if kind.startswith('f32') else BF16, W)
    y = Out((B, co, H, W), BF16, W)
    ops.conv_fwd(xs, kind.endswith('+gelu'), guarded(d.w, F32, 64), guarded(d.bias, F32, 64), y.v, ws[0].v, B, ci, co, H, W, k)
    done(y, ws[0])
    record(f'generic fwd co={co} {kind} k={k}', f'generic fwd k={k}', check(f'generic fwd co={co} {kind} k={k} {H}x{W}', unlay(y.v, 'nchw'), r.ref, r.bound), r)


@pytest.mark.parametrize('k', [4, 6])
@pytest.mark.parametrize('dgelu', [True, False])
@pytest.mark.parametrize('ci', [3, 8, 16])                 # COUT_T 4, 8 and 16 (roles swapped: dX has Cin channels)
def test_generic_conv_bwd_data(ops, ws, ci, dgelu, k):
    co, B = 6, 2
    H, W = GEN_SHAPES[(ci + k + dgelu) % 2]
    d = _gen_inputs('bf16', B, ci, co, H, W, k, 2)
    d.w = d.w * (ci / co) ** 0.5
    r = R.backward_data(d.dy.double(), d.w, d.x if dgelu else None, n=co * k * k + 4, wround=False)
    dx = Out((B, ci, H, W), BF16, W)
    ops.conv_bwd_data(guarded(d.dy, BF16, W), guarded(d.w, F32, 64), guarded(d.x, BF16, W) if dgelu else None, dgelu, dx.v, ws[0].v, B, ci, co, H, W, k)
    done(dx, ws[0])
    record(f'generic bwd_data ci={ci} dgelu={dgelu} k={k}', f'generic bwd_data k={k}',
           check(f'generic bwd_data ci={ci} dgelu={dgelu} k={k} {H}x{W}', unlay(dx.v, 'nchw'), r.ref, r.bound), r)


@pytest.mark.parametrize('k', [4, 6])
@pytest.mark.parametrize('kind', ['f32', 'bf16+gelu', 'bf16'])
@pytest.mark.parametrize('co', [4, 8, 16, 32])
def test_generic_conv_bwd_weight(ops, co, kind, k):
    ci = 5
    H, W = GEN_SHAPES[(co // 4 + k + len(kind)) % 2]
    B = 1 if H * W > 600 else 3
    d = _gen_inputs(kind, B, ci, co, H, W, k, 3)
    a, err = _gen_stage(d.x, kind)
    tiles = ((H + R.TILE - 1) // R.TILE) * ((W + R.TILE - 1) // R.TILE)
    rw, rb = R.backward_weight(d.dy.double(), a, torch.zeros_like(a), d.dw0, d.db0, k=k, n=R.TILE * R.TILE + B * tiles + 2)
    rw.bound = rw.bound + R.wgrad(d.dy.double().abs(), err, (k - 1) // 2, k)
    dw, db = Out(tuple(d.dw0.shape), F32, 64, fill=d.dw0), Out((co,), F32, 64, fill=d.db0)
    ops.conv_bwd_weight(guarded(d.dy, BF16, W), guarded(d.x, F32 if kind == 'f32' else BF16, W), kind.endswith('+gelu'), dw.v, db.v, B, ci, co, H, W, k)
    done(dw, db)
    tag = f'generic bwd_weight co={co} {kind} k={k}'
    record(tag, f'generic bwd_weight dW k={k}', check(f'{tag} dW {H}x{W}', dw.v.cpu().double(), rw.ref, rw.bound))
    record(tag, f'generic bwd_weight db k={k}', check(f'{tag} db', db.v.cpu().double(), rb.ref, rb.bound))
