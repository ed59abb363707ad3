"""The GEMM kernels (csrc/gemm.hip: every instantiation gemm_bf16_impl, i2t_gemm_bf16_ws and i2t_colsum_bf16_ex can launch) against
the float64 statements of tests/gemm_ref.py.

Every case of gemm_ref.CASES names its instantiation (the route restated from csrc/gemm_route.h, evaluated for this device's CU count
and the pointers' real alignment) and runs in three input regimes: bf16-rounded N(0, 1) operands against the derived per-element
bound (no free atol; DESIGN.md "GEMM kernels against fp64"); an integer lattice and an address pattern (C[m][n] = B[n][m mod K]),
whose results are exact in fp32 whatever the order and must be bit-identical to the reference rounded once -- epilogues with a
transcendental keep the bound there.  Every operand is a view into a larger allocation: NaN around the inputs and in their pad
columns, a sentinel around the outputs and in theirs, NaN inside a non-accumulating output.  Worst error / bound per instantiation
goes to I2T_REPORT_DIR/parity_report_gemm_kernels.json."""
import contextlib
import json
import os

import pytest
import torch

import gemm_ref as R
from test_row_kernels_gpu import BF16, F32, F64, SENT, check, dev, refused

pytestmark = pytest.mark.gpu

REPORT = {}
ID = lambda c: c.id
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


@pytest.fixture(scope='module')
def n_cu(ops):
    return R.effective_cus(torch.cuda.get_device_properties(0).multi_processor_count, ops.gemm_reserved_cus())


@pytest.fixture(scope='module', autouse=True)
def write_report():
    yield
    out = os.environ.get('I2T_REPORT_DIR', 'test_reports')
    os.makedirs(out, exist_ok=True)
    worst = {}
    for row in REPORT.values():
        for inst in row['route'].split(' + '):
            worst[inst] = max([worst.get(inst, 0.0)] + [u for k, u in row.items() if k.startswith('units ')])
    with open(os.path.join(out, 'parity_report_gemm_kernels.json'), 'w') as fh:
        json.dump({'worst_error_over_bound': worst, 'cases': REPORT}, fh, indent=1, sort_keys=True)


# --------------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """a [rows][cols] view with row stride ld inside a larger allocation: ``pad`` in the columns cols .. ld, ``outer`` on both sides
    (at least max(64, one row) elements); shift moves the view off its 16-byte alignment by that many elements"""

    def __init__(self, data, rows, cols, ld, dtype, pad, outer, shift=0, fill=NAN, watch=True):
        g = (max(64, ld) + 15) // 16 * 16
        self.g, self.n = g + shift, rows * ld
        self.buf = torch.full((2 * g + shift + self.n,), outer, dtype=dtype, device=dev())
        body = self.buf[self.g:self.g + self.n].view(rows, ld)
        body.fill_(pad)
        self.v = torch.as_strided(self.buf, (rows, cols), (ld, 1), self.g)
        if data is None:
            self.v.fill_(fill)
        else:
            self.v.copy_(data.reshape(rows, cols).to(F32).to(dtype))
        if not watch:
            return
        self.keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=dev())
        torch.as_strided(self.keep, (rows, cols), (ld, 1), self.g).fill_(False)
        self.before = self.buf[self.keep].clone()

    def intact(self):
        it = torch.int16 if self.buf.dtype == BF16 else torch.int32
        return torch.equal(self.buf[self.keep].view(it), self.before.view(it))

    def host(self):
        return self.v.detach().cpu().to(F64)


def operand(t, kmajor, ld, zero_pad=False):
    """a bf16 GEMM operand, logical [rows, K]: stored as it is or k-major, NaN around it and in its pad columns (zero where the
    ABI lets the kernel read them, gemm_ref.zero_pad)"""
    s = t.t() if kmajor else t
    return Buf(s, s.shape[0], s.shape[1], ld, BF16, 0.0 if zero_pad else NAN, NAN, watch=False)


def vector(t, shift=0, out=False):
    return Buf(t, 1, t.numel(), t.numel(), F32, SENT if out else NAN, SENT if out else NAN, shift)


@contextlib.contextmanager
def switches(ops, c, reserve=0):
    env = R.env_of(c)
    old = {k: os.environ.get(k) for k in env}
    was_det, was_res = ops.deterministic(), ops.gemm_reserved_cus()
    os.environ.update(env)
    try:
        ops.set_deterministic(bool(c.det))
        ops.gemm_reserve_cus(reserve)
        yield
    finally:
        ops.gemm_reserve_cus(was_res)
        ops.set_deterministic(was_det)
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run(ops, c, d, n_cu, reserve=0, refuse=None):
    """one call of case c on inputs d -> ({name: float64 CPU result}, route); guards checked.  refuse: the call must fail with
    this text in its error"""
    M, N, K = c.M, c.N, c.K
    mis = c.misalign
    outs = {}
    asq = None if d.asq is None else torch.tensor([d.asq], dtype=F32, device=dev())
    if c.entry == 'colsum':
        X = Buf(d.A, M, N, R.r8(N) + 8, BF16, NAN, NAN)
        o = vector(d.C0 if c.acc else torch.full((N,), NAN, dtype=F64), out=True)
        with switches(ops, c):
            ops.colsum(X.v, o.v.view(-1), M, N, ld=X.v.stride(0), accumulate=bool(c.acc), alpha_sumsq=asq)
            torch.cuda.synchronize()
        assert o.intact(), 'a guard region around colsum_out was written'
        return {'colsum': o.host().view(-1)}, R.case_route(c)
    A = operand(d.A, c.ak, c.lda, R.zero_pad(c))
    B = operand(d.B, c.bk, c.ldb)
    cdt = F32 if c.f32 else BF16
    preload = d.C0 if (c.acc or c.resc) else None
    C = Buf(preload, M, N, c.ldc, cdt, SENT, SENT, shift=4 if (mis and not c.f32) else 0)
    outs['C'] = C
    bias = vector(d.bias, shift=mis) if c.bias else None
    res = Buf(d.res, M, N, c.ldr, F32, NAN, NAN, shift=mis) if c.res else None
    auxi = Buf(d.auxi, M, N, c.ldai, BF16, NAN, NAN, shift=4 * mis) if c.auxi else None
    auxo = Buf(None, M, N, c.ldao, BF16, SENT, SENT) if c.auxo else None
    if auxo:
        outs['aux_out'] = auxo
    cs = vector(d.cs0, out=True) if c.cso else None
    if cs:
        outs['colsum'] = cs
    call = R.call_of(c, c16=C.v.data_ptr() % 16 == 0, auxo16=auxo is None or auxo.v.data_ptr() % 16 == 0)
    route = R.route(call, R.knobs_of(c), n_cu, bool(c.det))
    ws = None
    with switches(ops, c, reserve):
        if c.entry == 'dw':
            dw = lambda: ops.gemm_dw_colsum(A.v, B.v, C.v, None if cs is None else cs.v.view(-1), M, N, K, alpha=d.alpha, alpha_sumsq=asq,
                                            lda=c.lda, ldb=c.ldb, ldc=c.ldc)
            refused(dw, refuse) if refuse else dw()
        else:
            kw = {}
            if c.entry == 'ws':
                ws = Buf(None, 1, R.ws_floats_of(c), R.ws_floats_of(c) + (-R.ws_floats_of(c)) % 4, F32, SENT, SENT)
                kw['workspace'] = ws.v.view(-1)
                if R.ws_splits(M, N, K, c.act, R.ws_floats_of(c)) > 1:
                    route = 'g128<0,0,1>+reduce'
            ops.gemm(A.v, B.v, C.v, M, N, K, a_kmajor=bool(c.ak), b_kmajor=bool(c.bk), lda=c.lda, ldb=c.ldb, ldc=c.ldc, alpha=d.alpha,
                     bias=None if bias is None else bias.v.view(-1), act=c.act, aux_in=None if auxi is None else auxi.v,
                     aux_out=None if auxo is None else auxo.v, residual=C.v if c.resc else (None if res is None else res.v),
                     ldr=c.ldr if (c.res or c.resc) else None, accumulate=bool(c.acc), drop=d.drop, alpha_sumsq=asq, **kw)
        torch.cuda.synchronize()
    for name, b in list(outs.items()) + ([('workspace', ws)] if ws else []):
        assert b.intact(), f'{c.id}: a guard region or pad column of {name} was written'
    got = {k: (b.host().view(-1) if k == 'colsum' else b.host()) for k, b in outs.items()}
    return got, route


def exact(name, got, r):
    want = R.kernel_rounded(r)
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    bad = got != want
    assert not bool(bad.any()), f'{name}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result; first at ' \
                                f'{tuple(bad.nonzero()[0].tolist())}: got {got[bad][0].item()} want {want[bad][0].item()}'


def compare(c, regime, got, res, route):
    row = REPORT.setdefault(c.id, {'route': route})
    assert set(got) == set(res)
    for name, r in res.items():
        tag = f'{c.id} {regime} {name} [{route}]'
        if R.is_exact(c, regime):
            R.assert_exact_inputs(c, res)
            exact(tag, got[name], r)
            continue
        u = check(tag, got[name], r.ref, r.bound.expand_as(r.ref))
        row[f'units {regime} {name}'] = u
        if regime == 'normal':
            ii = R.condition_ii(r)
            row[f'ii {name}'] = ii
            assert ii <= R.ii_max(r), f'{tag}: condition 2 {ii:.5f}'


# ------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize('c', R.CASES, ids=ID)
def test_gemm_case(ops, n_cu, c):
    for regime in R.REGIMES:
        if c.entry == 'colsum' and regime == 'address':
            continue
        d = R.inputs(c, regime)
        if c.drop and regime != 'normal' and d.drop[3] != 2.0:
            continue                                            # p = 0.5 must scale by exactly 2 to stay on the lattice
        res = R.reference(c, d, n_cu)
        got, route = run(ops, c, d, n_cu)
        assert route == R.case_route(c), f'{c.id}: the table says {R.case_route(c)}, this device takes {route}'
        compare(c, regime, got, res, route)
        if c.det and regime == 'normal':                        # deterministic mode: bit-equal twice
            again, _ = run(ops, c, d, n_cu)
            assert all(torch.equal(got[k], again[k]) for k in got), f'{c.id}: deterministic mode differs between two runs'
        if c.reserve and regime == 'normal':
            # g256_cus ignores a reservation that leaves fewer than 9 CUs: n_cu - 3 runs on every CU, n_cu - 9 on 9 workgroups that
            # walk all the tiles (tile hand-over and DMA chaining of the persistent loop); both bit-equal to the un-reserved run
            total = torch.cuda.get_device_properties(0).multi_processor_count
            for reserve in (total - 3, total - 9):
                few, _ = run(ops, c, d, n_cu, reserve=reserve)
                assert all(torch.equal(got[k], few[k]) for k in got), f'{c.id}: differs under gemm_reserve_cus({reserve})'
            assert ops.gemm_reserved_cus() == 0


def test_route_table_is_complete(n_cu):
    got, want = R.table_routes(n_cu=n_cu), R.all_routes()
    assert got == want, (sorted(want - got), sorted(got - want))


def test_report_names_every_instantiation():
    """runs after the cases (file order): every listed instantiation has a worst error / bound, none above 1"""
    if len(REPORT) < len(R.CASES):
        pytest.skip('needs every case of this file in one process, before it')
    seen = {}
    for row in REPORT.values():
        for inst in row['route'].split(' + '):
            inst = 'skinny ksplit>1' if ' ksplit=' in inst else inst
            seen[inst] = max([seen.get(inst, 0.0)] + [u for k, u in row.items() if k.startswith('units ')])
    assert set(seen) == R.all_routes()
    assert max(seen.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_gemm_refusals(ops):
    from image2text_amd import lib as L
    lib, s = L.load(), torch.cuda.current_stream().cuda_stream
    M = N = K = 64
    a = torch.zeros(M * K + 16, dtype=BF16, device=dev())
    b = torch.zeros(N * K + 16, dtype=BF16, device=dev())
    c16 = torch.full((M * N + 16,), SENT, dtype=BF16, device=dev())
    c32 = torch.full((M * N + 16,), SENT, dtype=F32, device=dev())
    aux = torch.full((M * N + 16,), SENT, dtype=BF16, device=dev())
    cs = torch.full((N + 16,), SENT, dtype=F32, device=dev())
    wsb = torch.full((8 * 130 * 72 + 16,), SENT, dtype=F32, device=dev())
    A, B, C, C32 = a.data_ptr(), b.data_ptr(), c16.data_ptr(), c32.data_ptr()

    def gemm(what, A=A, lda=K, ak=0, B=B, ldb=K, bk=0, C=C, ldc=N, f32=0, M=M, N=N, K=K, act=0, auxi=None, acc=0, drop=0):
        refused(lambda: L.check(lib.i2t_gemm_bf16(s, A, lda, ak, B, ldb, bk, C, ldc, f32, M, N, K, 1.0, None, act, auxi, N, None, 0, None, 0, acc,
                                                  drop, 1, 26, 1.0), 'i2t_gemm_bf16'), what)

    gemm('null operand', A=None)
    gemm('null operand', B=None)
    gemm('null operand', C=None)
    gemm('empty problem', M=0)
    gemm('empty problem', N=0)
    gemm('empty problem', K=0)
    gemm('must be multiples of 8', lda=68)
    gemm('must be multiples of 8', ldb=68)
    gemm('16-byte aligned', A=A + 2)
    gemm('16-byte aligned', B=B + 8)
    gemm('lda=56 too small', lda=56)
    gemm('lda=56 too small', lda=56, ak=1)
    gemm('ldb=56 too small', ldb=56)
    gemm('ldb=56 too small', ldb=56, bk=1)
    gemm('ldc=63 < N=64', ldc=63)
    gemm('accumulate needs an f32 C', acc=1)
    for act in (R.DGELU, R.DGELU_ERF, R.MUL_AUX):
        gemm('need aux_in', act=act)
    gemm('unknown act 7', act=7)
    gemm('unknown act -1', act=-1)
    gemm('C misaligned', C=C + 4)
    gemm('C misaligned', C=C32 + 8, f32=1)
    gemm('dropout mode 2 unsupported', drop=2)                  # N % 12 != 0
    gemm('dropout mode 3 unsupported', drop=3)
    # (drop_mode 1 with M N >= 2^32 needs no allocation: the check comes before any launch)
    refused(lambda: L.check(lib.i2t_gemm_bf16(s, A, 8, 0, B, 8, 0, C32, 65536, 1, 65536, 65536, 8, 1.0, None, 0, None, 0, None, 0, None, 0, 0,
                                              1, 1, 26, 1.0), 'i2t_gemm_bf16'), 'dropout mode 1 unsupported')
    refused(lambda: L.check(lib.i2t_gemm_dw_colsum_bf16(s, A, M, B, N, C32, N, M, N, K, 1.0, None, cs.data_ptr() + 2), 'dw'), 'colsum_out misaligned')
    refused(lambda: L.check(lib.i2t_gemm_dw_colsum_bf16(s, A, M, B, N, C32 + 8, N, M, N, K, 1.0, None, cs.data_ptr()), 'dw'), 'C misaligned')

    def ws(what, A=A, lda=3072, B=B, ldb=3072, C=C, ldc=72, f32=0, W=wsb.data_ptr()):
        refused(lambda: L.check(lib.i2t_gemm_bf16_ws(s, A, lda, B, ldb, C, ldc, f32, 130, 72, 3072, None, 0, None, 0, W, 8 * 130 * 72), 'ws'), what)

    assert R.ws_splits(130, 72, 3072, 0, 8 * 130 * 72) == 8
    ws('null operand', A=None)
    ws('null operand', C=None)
    ws('operand layout', lda=3076)
    ws('operand layout', ldb=3076)
    ws('operand layout', lda=3064)
    ws('operand layout', ldb=3064)
    ws('operand layout', A=A + 8)
    ws('operand layout', B=B + 2)
    ws('operand layout', ldc=71)
    ws('C / workspace misaligned', C=C + 4)
    ws('C / workspace misaligned', C=C32 + 8, f32=1)
    ws('C / workspace misaligned', W=wsb.data_ptr() + 4)

    def colsum(what, X=A, ld=64, M=8, N=64, out=cs.data_ptr()):
        refused(lambda: L.check(lib.i2t_colsum_bf16_ex(s, X, ld, M, N, out, 0, None), 'colsum'), what)

    colsum('bad args', X=None)
    colsum('bad args', out=None)
    colsum('bad args', M=0)
    colsum('bad args', N=0)
    colsum('16-byte aligned', ld=60)
    colsum('16-byte aligned', X=A + 2)
    refused(lambda: ops.gemm_reserve_cus(-1), 'negative count')
    torch.cuda.synchronize()
    for t in (c16, c32, aux, cs, wsb):
        assert bool((t == SENT).all()), 'a refused call wrote to an output'


def test_dw_chunk_error_leaves_the_first_chunk(ops, n_cu):
    """The 2^32 dW case outside deterministic mode: its 42112-row chunk runs as class 6, its 101-row tail has no large-tile form and
    the call is refused THERE (gemm.hip: the chunks before the failing one are launched).  Pinned: the error text, guards and pad
    columns of C intact, and C = its value before the call + alpha x the first chunk's sum -- bit-identical on the lattice."""
    big = next(c for c in R.CASES if c.name == 'dw2g')
    kw = dict(entry='dw', ak=1, bk=1, f32=1, acc=1, lda=big.lda, positive=1)
    c = R.case('dw2g_refused', big.M, big.N, big.K, **kw)
    r = R.gemm_route(R.call_of(c), R.knobs_of(c), n_cu, False)
    assert r.chunk_error and r.chunks == 1 and r.full[0] == 6
    first = R.case('dw2g_first_chunk', c.M, c.N, r.kc, **kw)
    assert R.case_route(first, n_cu) == 'g256dw<epi=6>'
    for regime in ('lattice', 'normal'):
        d = R.inputs(c, regime)
        d1 = R.NS(**vars(d))
        d1.A, d1.B = d.A[:, :r.kc], d.B[:, :r.kc]
        res = R.reference(first, d1, n_cu)
        got, route = run(ops, c, d, n_cu, refuse='has no large-tile form')
        assert route == 'g256dw<epi=6>'
        compare(first, regime, got, res, route)
