"""Every kernel of csrc/attention.hip and csrc/attention_g.hip called through ops.attention_fwd / _bwd and ops.gq_attention_fwd /
_bwd, each against the float64 statement of tests/attention_ref.py on the SAME values the kernel reads: the bf16 q, k, v, dO, and for
the backward the O and lse the forward kernel STORED (compared with float64 first, so the backward rests on checked values).

Bounds (DESIGN.md "Attention kernels against fp64"): per element, built from the operands -- the one bf16 rounding of P or dS (two
units of 2^-9) times the absolute-value product it enters, the bf16 store, the fp32 terms with their counts and the measured allowance of the raw
v_exp_f32.  No free atol.  Every comparison asserts (i) every element is compared and finite and (ii) the median bound is at most
a quarter of the rms of the reference tensor, so a bound cannot hide a failure by being wide.

Every case runs on GUARDED buffers: operands are views into larger allocations (8 filler columns before and after the heads, two
rows after the last, three packed rows after ``total``) whose filler is NaN on inputs -- 0 x NaN must not reach a result -- and a
fixed bit pattern on outputs, which must come back bit-identical.  The kernel a case runs on is part of the case: the dispatch rule
of i2t_attention_fwd / i2t_attention_bwd_ex is restated in ``attention_ref.route`` (the cases live there too) and asserted, and
tests/test_attention_route_cpu.py holds ``route`` against csrc/attention_route.h for every case and switch, so a later change of
dispatch cannot silently move a case to another kernel.  Worst error / bound per tensor goes to
I2T_REPORT_DIR/parity_report_attention_kernels.json."""
import functools
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch

import attention_ref as R
from attention_ref import BWD1, BWD3, BWD3_QSEQ, ENVS, FWD_TILED, FWD_V2, GQ, GQ_SPLIT, PAIR, SWITCHES, route
from test_row_kernels_gpu import BF16, F32, F64, SENT, check, dev, refused

pytestmark = pytest.mark.gpu

REPORT = {}
DROP_P, DROP_SEED, OD_P, OD_SEED = 0.2, 99, 0.1, 4242
PAD_C, PAD_R, PAD_T = 8, 2, 3                               # filler columns each side, rows after a dense block, rows after a pack
II_MAX = 0.25                                               # condition (ii)


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
    with open(os.path.join(out, 'parity_report_attention_kernels.json'), 'w') as fh:
        json.dump({'worst_error_over_bound': worst, 'cases': REPORT}, fh, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def default_routes(monkeypatch):
    for e in ENVS:
        monkeypatch.delenv(e, raising=False)


ID = lambda c: c.id


# ------------------------------------------------------------------------------------------------------------------ buffers
def guarded(c, packed_rows, T, width, fill, device):
    """(allocation, view): the view is [rows, width] of a pack or [B, T, width] of a dense block; everything else holds ``fill``"""
    W = PAD_C + width + PAD_C
    if packed_rows is not None:
        buf = torch.full((packed_rows + PAD_T, W), fill, dtype=BF16, device=device)
        return buf, buf[:packed_rows, PAD_C:PAD_C + width]
    buf = torch.full((c.B, T + PAD_R, W), fill, dtype=BF16, device=device)
    return buf, buf[:, :T, PAD_C:PAD_C + width]


def untouched(buf, view, fill):
    """everything of the allocation outside the view still holds the fill, bit for bit"""
    keep = view.clone()
    view.fill_(fill)
    ok = torch.equal(buf.view(torch.int16), torch.full_like(buf, fill).view(torch.int16))
    view.copy_(keep)
    return ok


def stat_buffer(n, device):
    flat = torch.full((n + 4,), SENT, dtype=F32, device=device)
    return flat, flat[:n]


def geometry(c):
    """per sequence: (Tq_b, Tk_b, q row offset in the pack or None, k row offset or None, first q token row, first k token row)"""
    out = []
    if c.lens is None:
        for b in range(c.B):
            out.append((c.Tq, c.Tk, None, None, b * (c.q_seq or c.Tq), b * c.Tk))
        return out
    s0 = 0
    for b, n in enumerate(c.lens):
        out.append((n, c.Tk, s0, None, s0, b * c.Tk) if c.cross else (n, n, s0, s0, s0, s0))
        s0 += n
    return out


def seq_rows(view, b, off, n, heads, hd):
    """rows of sequence b as float64 [heads, n, hd]"""
    r = view[b, :n] if off is None else view[off:off + n]
    return r.reshape(n, heads, hd).permute(1, 0, 2)


@functools.lru_cache(maxsize=2)
def _data(cid):
    return _build(CASE_BY_ID[cid])


def _build(c):
    """inputs on the device (guarded), the dropout masks and the float64 forward reference of every sequence; never modified"""
    from image2text_amd import rng
    d = dev()
    H, Hkv, hd = c.H, c.Hkv, c.hd
    geo = geometry(c)
    total = sum(c.lens) if c.lens is not None else None
    self_like = not c.cross
    nan = float('nan')
    x = SimpleNamespace(c=c, geo=geo, total=total, scale=1.0 / math.sqrt(hd))
    if self_like:                                           # one packed qkv buffer, heads at hd-column steps: the engine's c_attn output
        x.qkv_buf, qkv = guarded(c, total, c.Tq, (H + 2 * Hkv) * hd, nan, d)
        x.q, x.k, x.v = qkv[..., :H * hd], qkv[..., H * hd:(H + Hkv) * hd], qkv[..., (H + Hkv) * hd:]
    else:                                                   # queries of their own, k and v side by side (the cross-attention kv projection)
        x.q_buf, x.q = guarded(c, total, c.Tq, H * hd, nan, d)
        x.kv_buf, kv = guarded(c, None, c.Tk, 2 * Hkv * hd, nan, d)
        x.k, x.v = kv[..., :Hkv * hd], kv[..., Hkv * hd:]
    x.do_buf, x.do = guarded(c, total, c.Tq, H * hd, nan, d)
    x.cu = None if c.lens is None else torch.tensor([0] + list(torch.tensor(c.lens).cumsum(0)), dtype=torch.int32, device=d)
    gen = torch.Generator().manual_seed(1234 + sum(map(ord, c.id)))
    for b, (tq, tk, qo, ko, _, _) in enumerate(geo):
        q, k, v, do = R.make_sequence(gen, H, Hkv, hd, max(tq, 1), tk if tk else 1, c.causal, c.regime, c.plant)
        for view, t, n, off in ((x.q, q, tq, qo), (x.do, do, tq, qo), (x.k, k, tk, ko), (x.v, v, tk, ko)):
            if n:
                (view[b, :n] if off is None else view[off:off + n]).copy_(t[:n].reshape(n, -1).to(BF16))
    x.drop, x.keep = None, None
    if c.drop:
        key, thr = rng.site_key(DROP_SEED, 18), rng.threshold(DROP_P)
        x.drop = (1, key, thr, rng.scale(thr))
        x.keep = rng.keep_mask(key, c.B * H * c.Tq * c.Tk, thr).view(c.B, H, c.Tq, c.Tk).to(d)      # the kernels' index space
    x.od, x.mult = None, None
    if c.od:
        key, thr = rng.site_key(OD_SEED, 77), rng.threshold(OD_P)
        x.od = (2, key, thr, rng.scale(thr))
        nq = total if c.lens is not None else c.B * (c.q_seq or c.Tq)
        nk = total if (c.lens is not None and not c.cross) else c.B * c.Tk
        x.mult = [rng.keep_mask((key + t) & 0xFFFFFFFF, n, thr).to(d).to(F64) * rng.scale(thr) for t, n in ((0, nq), (1, nk), (2, nk))]
    x.fwd = []
    for b, (tq, tk, qo, ko, _, _) in enumerate(geo):
        if tq == 0 or tk == 0:
            x.fwd.append(None)
            continue
        q, k, v = seq_rows(x.q, b, qo, tq, H, hd).to(F64), seq_rows(x.k, b, ko, tk, Hkv, hd).to(F64), seq_rows(x.v, b, ko, tk, Hkv, hd).to(F64)
        vis = R.visible(tq, tk, c.causal, c.split, d)
        keep = None if x.keep is None else x.keep[b, :, :tq, :tk]
        f = R.forward(q, k, v, x.scale, vis, keep, x.drop[3] if x.drop else 1.0)
        f.q, f.k, f.v, f.vis, f.keep = q, k, v, vis, keep
        x.fwd.append(f)
    return x


def compare(rid, name, parts):
    """parts: (got, ref, bound) of every sequence -> one per-element check over the whole tensor, with conditions (i) and (ii)"""
    got, ref, bound = (torch.cat([p[i].reshape(-1).to(F64) for p in parts]) for i in range(3))
    assert got.numel() == ref.numel() == bound.numel() and got.numel() > 0                         # (i): nothing filtered
    rms = float(ref.pow(2).mean().sqrt())
    ii = float(bound.median()) / rms if rms > 0 else float('inf')
    print(f'II {name}: median bound / rms(ref) = {ii:.4f} (rms {rms:.4g})')
    units = check(name, got, ref, bound)
    REPORT.setdefault(rid, {})[name] = round(units, 4)
    REPORT[rid]['ii ' + name] = round(ii, 5)
    assert ii <= II_MAX, f'{name}: the median bound is {ii:.3f} of the rms of the reference (condition (ii): <= {II_MAX})'
    return units


def run_forward(ops, x, rid):
    """the forward kernel on guarded outputs, checked against float64 -> (o view, lse view)"""
    c, d = x.c, dev()
    o_buf, o = guarded(c, x.total, c.Tq, c.H * c.hd, SENT, d)
    n_stat = c.H * x.total if c.lens is not None else c.B * c.H * c.Tq
    lse_flat, lse = stat_buffer(n_stat, d)
    kw = dict(drop=x.drop)
    if c.lens is not None:
        kw.update(cu_q=x.cu, cu_k=None if c.cross else x.cu, total_q=x.total)
    if c.api == 'gq':
        ops.gq_attention_fwd(x.q, x.k, x.v, o, lse, c.B, c.H, c.Hkv, c.hd, c.Tq, c.Tk, c.causal, split=c.split, **kw)
    else:
        ops.attention_fwd(x.q, x.k, x.v, o, lse, c.B, c.H, c.Tq, c.Tk, c.causal, **kw)
    torch.cuda.synchronize()
    assert untouched(o_buf, o, SENT), 'the forward wrote outside its output rows / head columns'
    assert float(lse_flat[n_stat:].min()) == SENT == float(lse_flat[n_stat:].max()), 'the forward wrote past the end of lse'
    lse_v = lse.view(c.H, x.total) if c.lens is not None else lse.view(c.B, c.H, c.Tq)
    po, pl = [], []
    for b, (tq, tk, qo, ko, _, _) in enumerate(x.geo):
        f = x.fwd[b]
        if f is None:
            continue
        po.append((seq_rows(o, b, qo, tq, c.H, c.hd), f.O, f.o_bound))
        pl.append((lse_v[:, qo:qo + tq] if c.lens is not None else lse_v[b], f.lse, f.lse_bound))
    tag = route(c, {})[0] if c.api == 'mha' else 'gq_fwd'
    compare(rid, f'{tag} O', po)
    compare(rid, f'{tag} lse', pl)
    return o, lse


def run_backward(ops, x, o, lse, rid, tag):
    """the backward kernel(s) on guarded outputs against float64 from the stored o / lse -> {name: (got parts, bound parts)}"""
    c, d = x.c, dev()
    H, Hkv, hd = c.H, c.Hkv, c.hd
    if not c.cross:
        g_buf, g = guarded(c, x.total, c.Tq, (H + 2 * Hkv) * hd, SENT, d)
        dq, dk, dv = g[..., :H * hd], g[..., H * hd:(H + Hkv) * hd], g[..., (H + Hkv) * hd:]
        bufs = [(g_buf, g)]
    else:
        dq_buf, dq = guarded(c, x.total, c.Tq, H * hd, SENT, d)
        dkv_buf, dkv = guarded(c, None, c.Tk, 2 * Hkv * hd, SENT, d)
        dk, dv = dkv[..., :Hkv * hd], dkv[..., Hkv * hd:]
        bufs = [(dq_buf, dq), (dkv_buf, dkv)]
    n_stat = H * x.total if c.lens is not None else c.B * H * c.Tq
    ws_flat, ws = stat_buffer(n_stat, d)
    kw = dict(drop=x.drop, out_drop=x.od)
    if c.lens is not None:
        kw.update(cu_q=x.cu, cu_k=None if c.cross else x.cu, total_q=x.total)
    if c.api == 'gq':
        ops.gq_attention_bwd(x.q, x.k, x.v, o, x.do, lse, ws, dq, dk, dv, c.B, H, Hkv, hd, c.Tq, c.Tk, c.causal, **kw)
    else:
        ops.attention_bwd(x.q, x.k, x.v, o, x.do, lse, ws, dq, dk, dv, c.B, H, c.Tq, c.Tk, c.causal, out_drop_q_seq=c.q_seq, **kw)
    torch.cuda.synchronize()
    # what must not be written: filler and guard rows.  A self-attention pack writes exactly its ``total`` rows; dense and
    # cross-attention calls write every key row of every sequence (zeros where a sequence has no query row: checked below as values)
    for buf, view in bufs:
        assert untouched(buf, view, SENT), f'{tag}: the backward wrote outside its gradient rows / head columns'
    assert float(ws_flat[n_stat:].min()) == SENT == float(ws_flat[n_stat:].max()), f'{tag}: the backward wrote past the end of the delta workspace'
    lse_v = lse.view(H, x.total) if c.lens is not None else lse.view(c.B, H, c.Tq)
    parts = {'dq': [], 'dk': [], 'dv': []}
    for b, (tq, tk, qo, ko, gq0, gk0) in enumerate(x.geo):
        f = x.fwd[b]
        gk_, gv_ = seq_rows(dk, b, ko, tk, Hkv, hd), seq_rows(dv, b, ko, tk, Hkv, hd)
        if f is None:
            if tk:                                          # a sequence with no query row: its key rows' gradients are WRITTEN as zeros
                assert float(gk_.float().abs().max()) == 0.0 and float(gv_.float().abs().max()) == 0.0, f'{tag}: sequence {b} has no query, dk / dv must be zero'
            continue
        O_st = seq_rows(o, b, qo, tq, H, hd).to(F64)
        lse_st = (lse_v[:, qo:qo + tq] if c.lens is not None else lse_v[b]).to(F64)
        dO = seq_rows(x.do, b, qo, tq, H, hd).to(F64)
        fq = fk = fv = None
        if x.mult is not None:
            fq, fk, fv = x.mult[0][gq0:gq0 + tq], x.mult[1][gk0:gk0 + tk], x.mult[2][gk0:gk0 + tk]
        r = R.backward(f.q, f.k, f.v, x.scale, f.vis, f.keep, x.drop[3] if x.drop else 1.0, O_st, lse_st, dO, fq, fk, fv)
        parts['dq'].append((seq_rows(dq, b, qo, tq, H, hd), r.dq, r.dq_bound))
        parts['dk'].append((gk_, r.dk, r.dk_bound))
        parts['dv'].append((gv_, r.dv, r.dv_bound))
    for name, p in parts.items():
        compare(rid, f'{tag} {name}', p)
    return parts


def fwd_bwd(ops, c, request, env=None, monkeypatch=None, expect=None):
    """forward + backward of one case on the default route, then (env given) the backward again on the switched route: each against
    float64, and the two against each other within the sum of their bounds"""
    x = _data(c.id)
    rid = request.node.name
    if c.api == 'mha' and expect is not None:
        got = route(c, {})
        assert expect[0] is None or got[0].startswith(expect[0]), f'{c.id}: forward runs on {got[0]}, the case is meant for {expect[0]}'
        assert expect[1] is None or got[1].startswith(expect[1]), f'{c.id}: backward runs on {got[1]}, the case is meant for {expect[1]}'
        if c.lens is None and not c.causal:
            assert ops.attention_bwd_takes_q_seq(c.Tq, c.Tk, x.drop) == got[1].startswith('bwd3')
    o, lse = run_forward(ops, x, rid)
    if not c.bwd:
        return
    base = run_backward(ops, x, o, lse, rid, route(c, {})[1] if c.api == 'mha' else 'gq_bwd')
    if env:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        kernel = route(c, env)[1]
        assert kernel.startswith(expect[2]), f'{c.id}: with {env} the backward runs on {kernel}, the case is meant for {expect[2]}'
        if c.lens is None and not c.causal:
            assert ops.attention_bwd_takes_q_seq(c.Tq, c.Tk, x.drop) == kernel.startswith('bwd3')
        alt = run_backward(ops, x, o, lse, rid, kernel)
        for name in ('dq', 'dk', 'dv'):
            a, b, bound = (torch.cat([p[i].reshape(-1).to(F64) for p in side[name]]) for side, i in ((base, 0), (alt, 0), (base, 2)))
            REPORT[rid][f'{kernel} vs default {name}'] = round(check(f'{kernel} vs default {name}', b, a, 2 * bound), 4)


# ------------------------------------------------------------------------------------------------------------------ head_dim 64
CASE_BY_ID = {}


@pytest.mark.parametrize('c', FWD_TILED, ids=ID)
def test_tiled_forward(ops, c, request):
    """attn_fwd_kernel<DROP, EVEN> (and whatever backward the shape takes: bwd1 or the tiled pair)"""
    fwd_bwd(ops, c, request, expect=('fwd<', None))


@pytest.mark.parametrize('c', FWD_V2, ids=ID)
def test_resident_forward(ops, c, request):
    """attn_fwd2_kernel<DROP, PER = 1 .. 4>: PER changes at Tq = 112 / 113, 176 / 177, 240 / 241; the limit is 304"""
    per = ((c.Tq + 15) >> 4) >> 2
    assert per == {64: 1, 112: 1, 113: 2, 176: 2, 177: 3, 240: 3, 241: 4, 304: 4}[c.Tq]
    fwd_bwd(ops, c, request, expect=(f'fwd2<PER={per}>', None))


@pytest.mark.parametrize('c', BWD3 + BWD3_QSEQ, ids=ID)
def test_bwd3_default(ops, c, request):
    """attn_bwd3_kernel<DROP, 8>: CNT changes at Tk = 128 / 129 and 256 / 257; the limit is 288"""
    cnt = {16: 1, 17: 1, 128: 1, 129: 2, 196: 2, 197: 2, 256: 2, 257: 3, 272: 3, 288: 3}[c.Tk]
    fwd_bwd(ops, c, request, expect=('fwd2<', f'bwd3<8,CNT={cnt}>'))


# (I2T_ATTN_BWD2=0 is the same route as I2T_ATTN_BWD=0: one regime shows that the switch is read)
SWITCHED = [(c, s) for s in SWITCHES for c in BWD3 if s != 'bwd2off' or c.regime == 'n01']


@pytest.mark.parametrize('c,switch', SWITCHED, ids=[f'{s}-{c.id}' for c, s in SWITCHED])
def test_bwd3_shapes_on_the_switched_routes(ops, c, switch, request, monkeypatch):
    """the A/B baselines of the encoder backward: each against float64 and against the default route on the same inputs"""
    env, kernel = SWITCHES[switch]
    if kernel == 'pair<' and c.Tq <= 64 and c.Tk <= 64:      # without the resident kernels a single-tile shape is bwd1's, not the pair's
        kernel = 'bwd1<'
    fwd_bwd(ops, c, request, env=env, monkeypatch=monkeypatch, expect=('fwd2<', 'bwd3<8', kernel))


@pytest.mark.parametrize('c', BWD1, ids=ID)
def test_bwd1(ops, c, request):
    """attn_bwd1_kernel<DROP, EVEN>, then I2T_ATTN_BWD1=0: the tiled pair on the same single-tile inputs"""
    fwd_bwd(ops, c, request, expect=('fwd<', 'bwd1<'))


@pytest.mark.parametrize('c', BWD1, ids=ID)
def test_bwd1_shapes_on_the_tiled_pair(ops, c, request, monkeypatch):
    fwd_bwd(ops, c, request, env={'I2T_ATTN_BWD1': '0'}, monkeypatch=monkeypatch, expect=('fwd<', 'bwd1<', 'pair<'))


@pytest.mark.parametrize('c', PAIR, ids=ID)
def test_tiled_pair_default(ops, c, request):
    """attn_bwd_dq_kernel + attn_bwd_dkv_kernel where they are the default: Tq > 288, Tk > 288, causal multi-tile, packed"""
    fwd_bwd(ops, c, request, expect=(None, 'pair<'))


def test_q_seq_is_refused_off_the_one_pass_kernel(ops, monkeypatch):
    c = BWD3_QSEQ[0]
    x = _data(c.id)
    o, lse = torch.zeros_like(x.q), torch.zeros(c.B, c.H, c.Tq, device=dev())
    dq, dk, dv = torch.zeros_like(x.q), torch.zeros_like(x.k), torch.zeros_like(x.v)
    call = lambda: ops.attention_bwd(x.q, x.k, x.v, o, x.do, lse, torch.zeros_like(lse), dq, dk, dv, c.B, c.H, c.Tq, c.Tk, False, out_drop=x.od,
                                     out_drop_q_seq=c.q_seq)
    for env in ({'I2T_ATTN_BWD': '2'}, {'I2T_ATTN_BWD': '0'}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            refused(call, 'out_drop_q_seq')
    assert float(dq.abs().max()) == 0.0 and float(dk.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ grouped heads
@pytest.mark.parametrize('c', GQ, ids=ID)
def test_grouped_query(ops, c, request):
    """gattn_fwd_kernel / gattn_bwd_dq_kernel / gattn_bwd_dkv_kernel<D, DROP>: hd 16 .. 128, H / Hkv 1, 2, 8"""
    fwd_bwd(ops, c, request)


@pytest.mark.parametrize('c', GQ_SPLIT, ids=ID)
def test_grouped_query_split(ops, c, request):
    """rows >= split do not see keys < split (forward only: i2t_gq_attention_bwd has no split)"""
    fwd_bwd(ops, c, request)


def test_grouped_query_refusals(ops):
    """each refusal leaves lib.last_error text and launches nothing (the outputs keep their pattern)"""
    d = dev()
    B, H, Hkv, hd, T = 1, 4, 2, 32, 96
    q = torch.zeros(B, T, H * hd, dtype=BF16, device=d)
    kv = torch.zeros(B, T, 2 * Hkv * hd, dtype=BF16, device=d)
    k, v = kv[..., :Hkv * hd], kv[..., Hkv * hd:]
    o = torch.full_like(q, SENT)
    lse = torch.full((B, H, T), SENT, device=d)
    cu = torch.tensor([0, T], dtype=torch.int32, device=d)
    fwd = lambda **kw: ops.gq_attention_fwd(q, k, v, o, lse, **{**dict(B=B, H=H, Hkv=Hkv, hd=hd, Tq=T, Tk=T, causal=False), **kw})
    refused(lambda: fwd(causal=True, split=8), 'split needs dense non-causal self-attention')
    refused(lambda: fwd(cu_q=cu, cu_k=cu, total_q=T, split=8), 'split needs dense non-causal self-attention')
    refused(lambda: fwd(split=T), 'split needs dense non-causal self-attention')
    refused(lambda: fwd(hd=48), 'head_dim 48')
    refused(lambda: fwd(H=3), 'not a multiple of H_kv')
    refused(lambda: fwd(Tk=T - 1, causal=True), 'causal needs Tk >= Tq')
    dq, dk, dv = torch.full_like(q, SENT), torch.full_like(k, SENT), torch.full_like(v, SENT)
    bwd = lambda **kw: ops.gq_attention_bwd(q, k, v, o, q, lse, torch.zeros_like(lse), dq, dk, dv,
                                            **{**dict(B=B, H=H, Hkv=Hkv, hd=hd, Tq=T, Tk=T, causal=False), **kw})
    refused(lambda: bwd(hd=48), 'head_dim 48')
    refused(lambda: bwd(H=3), 'not a multiple of H_kv')
    refused(lambda: bwd(Tk=T - 1, causal=True), 'causal needs Tk >= Tq')
    torch.cuda.synchronize()
    for t in (o, dq, dk, dv, lse):
        assert float(t.float().min()) == SENT == float(t.float().max())


for _c in FWD_TILED + FWD_V2 + BWD3 + BWD3_QSEQ + BWD1 + PAIR + GQ + GQ_SPLIT:
    assert CASE_BY_ID.setdefault(_c.id, _c) is _c or vars(CASE_BY_ID[_c.id]) == vars(_c), _c.id
