"""The PEER and LSH head kernels of csrc/vit.hip (i2t_peer_lookup_fwd / _bwd, i2t_lsh_embed_fwd / _bwd) called through their ops
wrappers, each against a float64 statement of the same op (restated from include/i2t.h and the kernels' comments) on the SAME
rounded values the kernel reads: bf16 tables and inp_proj converted up, fp32 scores / z / tables as they are.

What is compared exactly (DESIGN.md "PEER and LSH head kernels"): the routing (sv.unit, sv.lr, order included) and the bucket rows,
for every row -- the kernel compares the same fp32 numbers as the reference, so the only condition is that the inputs hold no exact
tie, which every case ASSERTS on the reference (a separate case is built from ties and pins the tie rule: larger value, then
smaller index); and everything a kernel must not touch (tails, guard rows, filler between tables, gradient rows nobody named).
Values follow the rule of tests/test_row_kernels_gpu.py: per element, fp32 |got - ref| <= r |ref| + k 2^-23 sum|terms|, bf16
2^-7 |ref| + 2^-8 sum|terms|, plus what csrc/common.h states for gelu_tanh (``_gelu_tanh64``) and the measured allowance of the
softmax's expf (EXPF_ALLOW).  Inputs and references are built once per case on the host (the seeds are chosen so the asserted
conditions hold) and shared by the forward and backward tests."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from test_row_kernels_gpu import BF16, E7, E8, F32, F64, SENT, U32, _gelu_tanh64, check, dev, nans, refused

pytestmark = pytest.mark.gpu

I32 = torch.int32
ISENT = -7                                                  # sentinel of the int32 buffers
R32 = 1e-5                                                  # r of the fp32 bound (row ops)
# The softmax's expf: csrc/common.h states no figure for it.  Measured on the MI355X over every forward case below (ties included),
# the largest relative error of sv.score against float64 was 4.2e-7 (every case prints its own as MEAS); four times that is allowed
# on top of the fp32 bound, because the inputs are random and few.
EXPF_MEASURED = 4.2e-7
EXPF_ALLOW = 4 * EXPF_MEASURED


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def cuda(t):
    return t.to(dev()).contiguous()


def pattern(*shape):
    """a known non-zero fp32 pattern (multiples of 1/8 in [1/8, 7/8])"""
    n = math.prod(shape)
    return ((torch.arange(n, dtype=F64) % 7 + 1) * 0.125).to(F32).view(*shape)


def with_tail(t, rows=1, fill=SENT):
    """t with ``rows`` more leading-dim rows that hold the sentinel -> (whole buffer, view of the first rows)"""
    buf = torch.full((t.shape[0] + rows,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf, buf[:t.shape[0]]


def tail_ok(buf, n, fill=SENT):
    return torch.equal(buf[n:], torch.full_like(buf[n:], fill))


def gelu64(x):
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


# ------------------------------------------------------------------------------------------------------------------ PEER
#             (M, nhead, nq, topk, din, dout)
PEER_CASES = [(5, 2, 16, 4, 32, 64),                        # the fixture's twin
              (3, 1, 16, 16, 8, 4),                         # topk == nq == PEER_MAXK: all 256 sums are candidates; smallest din / dout
              (4, 2, 100, 8, 776, 260),                     # nq % 64 != 0, din past one 512 trip and ragged, dout / 4 = 65
              (2, 3, 1024, 16, 768, 768),                   # PEER_MAXQ: sixteen strided reads per lane
              (2, 1, 64, 4, 64, 8192),                      # the dout limit: every MAXC chunk in use
              (1, 1, 1, 1, 8, 4)]                           # minimal: the softmax of one value
PEER_BWD_CASES = [(33,) + c[1:] if i in (0, 2) else c for i, c in enumerate(PEER_CASES)]
PEER_TIE_CASES = [PEER_CASES[0], PEER_CASES[1], PEER_CASES[2], PEER_CASES[3]]
PEER_SEED = 0                                               # chosen on the host: no case below has an exact tie with it
PEER_ID = lambda c: 'x'.join(map(str, c))


def topk_stable(v, k):
    """larger value first, a tie goes to the smaller index (torch.topk leaves the tie order open)"""
    s, i = torch.sort(v, dim=-1, descending=True, stable=True)
    return s[..., :k], i[..., :k], s


def peer_route(S, nq, k):
    """fp32 selection of every (row, head): -> namespace(li, ri, ci [R][k] long; l, r, unit [R][k] long; the three sorted value lists)"""
    lv, li, ls = topk_stable(S[:, :nq], k)
    rv, ri, rs = topk_stable(S[:, nq:], k)
    cross = (lv[:, :, None] + rv[:, None, :]).reshape(-1, k * k)            # one IEEE fp32 add per candidate, j = a k + b
    assert cross.dtype == F32
    cv, ci, cs = topk_stable(cross, k)
    l, r = li.gather(1, ci // k), ri.gather(1, ci % k)
    return SimpleNamespace(li=li, ri=ri, ci=ci, l=l, r=r, unit=l * k + r, ls=ls, rs=rs, cs=cs)


def peer_ref(c, S, ip, res, e_in, e_out, rt, pin=None):
    """float64 statement of PeerLookup after its linear maps, the chosen indices ``rt`` held fixed; differentiable in S, ip, e_in, e_out.
    pin = (score, dot) evaluates the selected logits and the dots AT the fp32 values the backward kernel reads (gradients still flow)."""
    M, nh, nq, k, din, dout = c
    lv, rv = S[:, :nq].gather(1, rt.li), S[:, nq:].gather(1, rt.ri)
    cv = (lv[:, :, None] + rv[:, None, :]).reshape(-1, k * k).gather(1, rt.ci)
    dot = (e_in[rt.unit] * ip.view(M * nh, 1, din)).sum(-1)
    if pin is not None:
        cv = cv + (pin[0].log() - cv).detach()
        dot = dot + (pin[1] - dot).detach()
    score = torch.softmax(cv, -1)
    terms = (score * gelu64(dot))[:, :, None] * e_out[rt.unit]                # [R][k][dout]
    out = res + terms.view(M, nh * k, dout).sum(1)
    return SimpleNamespace(score=score, dot=dot, out=out, terms=terms)


@functools.lru_cache(maxsize=2)
def peer_case(c, ties=False):
    """host inputs of one case and their float64 forward reference (shared by the tests of that case, never modified)"""
    M, nh, nq, k, din, dout = c
    g = torch.Generator().manual_seed(PEER_SEED + sum(c) + (1000 if ties else 0))
    R, U = M * nh, (nq - 1) * k + nq                        # unit = l k + r < U: the rows the stride quirk can address
    if ties:                                                # a handful of repeated values: ties at the k-th place of all three selections
        S = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0, 1.5])[torch.randint(0, 6, (R, 2 * nq), generator=g)]
    else:                                                   # a common bias per index: a few l and r dominate across rows, so units collide;
        S = torch.randn(R, 2 * nq, generator=g)             # the hot l are consecutive and the hot r multiples of k, so that
        S[:, nq - k:nq] += 1.5                              # (l + 1, r) and (l, r + k) name the SAME unit within one (row, head)
        S[:, nq:][:, [r for r in range(0, nq, k)][:k]] += 1.5
    ip = torch.randn(M, nh * din, generator=g).to(BF16)
    res = torch.randn(M, dout, generator=g)
    e_in = (torch.randn(U, din, generator=g) * (2.0 / math.sqrt(din))).to(BF16)        # dots ~ N(0, 4): both GELU tails and its middle
    e_out = torch.randn(U, dout, generator=g).to(BF16)
    G = torch.randn(M, dout, generator=g)
    rt = peer_route(S, nq, k)
    with torch.no_grad():
        ref = peer_ref(c, S.double(), ip.double(), res.double(), e_in.double(), e_out.double(), rt)
    return SimpleNamespace(c=c, S=S, ip=ip, res=res, e_in=e_in, e_out=e_out, G=G, rt=rt, ref=ref, U=U)


def has_tie(sorted_desc):
    return bool((sorted_desc[..., 1:] == sorted_desc[..., :-1]).any())


def peer_dot_terms(p):
    M, nh, nq, k, din, dout = p.c
    return (p.e_in.double()[p.rt.unit] * p.ip.double().view(M * nh, 1, din)).abs().sum(-1)


def run_peer_fwd(ops, p):
    """device forward with NaN outputs, sentinel tails and guard rows -> (out, sv) on the device; checks what must not change"""
    M, nh, nq, k, din, dout = p.c
    ins = [cuda(with_tail(t, 2)[0]) for t in (p.S, p.ip, p.res, p.e_in, p.e_out)]
    keep = [t.clone() for t in ins]
    out = nans(M + 1, dout)
    out[M:] = SENT
    sv = SimpleNamespace(unit=torch.full((M + 1, nh, k), ISENT, dtype=I32, device=dev()), lr=torch.full((M + 1, nh, k, 2), ISENT, dtype=I32, device=dev()),
                         score=nans(M + 1, nh, k), dot=nans(M + 1, nh, k))
    sv.score[M:] = SENT
    sv.dot[M:] = SENT
    ops.peer_lookup_fwd(*ins, out, sv, M, nh, nq, k, din, dout)
    torch.cuda.synchronize()
    for a, b in zip(ins, keep):
        assert torch.equal(a, b), 'an input (or its guard rows) changed'
    assert tail_ok(out, M) and tail_ok(sv.score, M) and tail_ok(sv.dot, M) and tail_ok(sv.unit, M, ISENT) and tail_ok(sv.lr, M, ISENT)
    return out, sv, ins


def check_peer_fwd(ops, p, tag):
    M, nh, nq, k, din, dout = p.c
    rt, ref = p.rt, p.ref
    out, sv, _ = run_peer_fwd(ops, p)
    unit, lr = sv.unit[:M].cpu().view(-1, k).long(), sv.lr[:M].cpu().view(-1, k, 2).long()
    assert torch.equal(lr[..., 0], rt.l) and torch.equal(lr[..., 1], rt.r), f'{tag}: (l, r) differ in {int(((lr[..., 0] != rt.l) | (lr[..., 1] != rt.r)).sum())} places'
    assert torch.equal(unit, rt.unit), f'{tag}: units differ'
    score, dot = sv.score[:M].view(-1, k), sv.dot[:M].view(-1, k)
    assert torch.isfinite(score).all() and torch.isfinite(dot).all()
    rel_score = ((score.cpu().double() - ref.score).abs() / ref.score).max().item()
    print(f'MEAS {tag} score: largest relative error {rel_score:.3e}')
    # score = e_j / sum e: the subtraction, the k-term sum and the division are fp32 (k + 2 roundings), expf adds its own
    tol_score = (R32 + (k + 2) * U32 + EXPF_ALLOW) * ref.score
    check(f'{tag} score', score, cuda(ref.score), cuda(tol_score))
    dterms = peer_dot_terms(p)
    check(f'{tag} dot', dot, cuda(ref.dot), cuda(R32 * ref.dot.abs() + din * U32 * dterms))
    # out = residual + sum_h sum_j score_j gelu(dot_j) e_out[unit_j]: nh k + 1 fp32 terms; each term also carries the relative error of
    # its score (the bound above), of gelu_tanh (csrc/common.h: _gelu_tanh64's rel) and of the fp32 dot it is evaluated at -- a
    # lane's serial chain of 8 products per 512-column trip plus the 6-step wave tree, through |gelu'| <= 1.13
    gl, _, _, rel_gelu, _ = _gelu_tanh64(ref.dot)
    kdot = 8 * ((din + 511) // 512) + 7
    tol_dot = R32 * ref.dot.abs() + kdot * U32 * dterms
    eo = p.e_out.double()[rt.unit].abs()
    err_terms = (ref.terms.abs() * (tol_score / ref.score + rel_gelu)[:, :, None] + (ref.score * 1.13 * tol_dot)[:, :, None] * eo).view(M, nh * k, dout).sum(1)
    sum_terms = p.res.double().abs() + ref.terms.abs().view(M, nh * k, dout).sum(1)
    check(f'{tag} out', out[:M], cuda(ref.out), cuda(R32 * ref.out.abs() + (nh * k + 1) * U32 * sum_terms + err_terms))
    return sv


@pytest.mark.parametrize('c', PEER_CASES, ids=PEER_ID)
def test_peer_lookup_fwd(ops, c):
    p = peer_case(c)
    assert not has_tie(p.rt.ls) and not has_tie(p.rt.rs) and not has_tie(p.rt.cs), 'the inputs hold an exact tie: choose another PEER_SEED'
    check_peer_fwd(ops, p, f'peer_fwd {PEER_ID(c)}')


@pytest.mark.parametrize('c', PEER_TIE_CASES, ids=PEER_ID)
def test_peer_lookup_fwd_ties(ops, c):
    """ties at the k-th place of the left, the right and the k x k selection: the larger value wins, a tie goes to the smaller index"""
    M, nh, nq, k, din, dout = c
    p = peer_case(c, True)
    at_kth = lambda s: bool((s[:, k - 1] == s[:, k]).any())
    assert at_kth(p.rt.cs) and has_tie(p.rt.ls[:, :k]) and has_tie(p.rt.rs[:, :k])
    if k < nq:
        assert at_kth(p.rt.ls) and at_kth(p.rt.rs)
    check_peer_fwd(ops, p, f'peer_fwd ties {PEER_ID(c)}')


def test_peer_lookup_fwd_refusals(ops):
    def call(M=2, nh=1, nq=16, k=4, din=8, dout=4):
        z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev())
        sv = SimpleNamespace(unit=z(64, dt=I32), lr=z(128, dt=I32), score=z(64), dot=z(64))
        return lambda: ops.peer_lookup_fwd(z(64), z(64, dt=BF16), z(64), z(64, dt=BF16), z(64, dt=BF16), z(64), sv, M, nh, nq, k, din, dout)
    for kw in (dict(nq=1025), dict(nq=32, k=17), dict(nq=3, k=4), dict(din=12), dict(dout=6), dict(dout=8196)):
        refused(call(**kw), 'i2t_peer_lookup_fwd: bad args (nq=')
    torch.cuda.synchronize()


# ---- backward
def gelu_grad_terms(t):
    _, grad, terms, rel, flush = _gelu_tanh64(t)
    return grad, rel * terms + flush                         # gelu'(t) and the absolute error csrc/common.h's sigmoid form leaves on it


@functools.lru_cache(maxsize=2)
def peer_bwd_case(c):
    p = peer_case(c)
    M, nh, nq, k, din, dout = c
    rt, R = p.rt, M * nh
    cnt = torch.zeros(p.U, dtype=torch.long).index_add_(0, rt.unit.reshape(-1), torch.ones(R * k, dtype=torch.long))
    return SimpleNamespace(p=p, cnt=cnt, touched=cnt > 0)


def peer_bwd_ref(p, score32, dot32):
    """float64 autograd of the forward restatement (indices fixed, evaluated at the sv values the kernel reads), loss = sum(out G);
    -> gradients and, per element, the sum of |terms| / the error allowances of the sums the kernel forms"""
    M, nh, nq, k, din, dout = p.c
    rt, R = p.rt, M * nh
    S, ip, e_in, e_out = (t.double().requires_grad_() for t in (p.S, p.ip, p.e_in, p.e_out))
    sc, t = score32.double(), dot32.double()
    f = peer_ref(p.c, S, ip, p.res.double(), e_in, e_out, rt, pin=(sc, t))
    (f.out * p.G.double()).sum().backward()
    # softmax(log sc) = sc / sum sc: what the reference's score differs from the kernel's input by, relative (from the INPUT sv.score)
    norm = float((sc.sum(-1) - 1).abs().max())
    Gr = p.G.double().repeat_interleave(nh, 0)                               # [R][dout]
    eo, ei, ipr = p.e_out.double()[rt.unit], p.e_in.double()[rt.unit], p.ip.double().view(R, din)
    ge, _, _, rel_ge, _ = _gelu_tanh64(t)
    gp, err_gp = gelu_grad_terms(t)
    adfw = (eo * Gr[:, None, :]).abs().sum(-1)                               # sum |e_out G| of every <dout, e_out[unit_j]>
    ads = adfw * ge.abs()
    add = sc * (ads + (sc * ads).sum(-1, keepdim=True))                      # |terms| of dd_j = sc_j (ds_j - sum_i sc_i ds_i)
    tS = torch.zeros(R, 2 * nq, dtype=F64).scatter_add_(1, rt.l, add).scatter_add_(1, nq + rt.r, add)
    eS = torch.zeros(R, 2 * nq, dtype=F64).scatter_add_(1, rt.l, add * rel_ge).scatter_add_(1, nq + rt.r, add * rel_ge)
    adt = adfw * sc * gp.abs()
    edt = adfw * sc * err_gp
    t_ip = (adt[:, :, None] * ei.abs()).sum(1)
    flat = rt.unit.reshape(-1)
    a_in = (adt[:, :, None] * ipr.abs()[:, None, :]).reshape(R * k, din)
    e_inn = (edt[:, :, None] * ipr.abs()[:, None, :]).reshape(R * k, din)
    t_gin = torch.zeros(p.U, din, dtype=F64).index_add_(0, flat, a_in)
    e_gin = torch.zeros(p.U, din, dtype=F64).index_add_(0, flat, e_inn)
    a_out = ((sc * ge).abs()[:, :, None] * Gr.abs()[:, None, :]).reshape(R * k, dout)
    t_gout = torch.zeros(p.U, dout, dtype=F64).index_add_(0, flat, a_out)
    e_gout = torch.zeros(p.U, dout, dtype=F64).index_add_(0, flat, a_out * rel_ge.reshape(R * k, 1))
    return SimpleNamespace(dS=S.grad, dip=ip.grad.view(M, nh * din), gin=e_in.grad, gout=e_out.grad, tS=tS, eS=eS + 3 * norm * tS,
                           t_ip=t_ip.view(M, nh * din), t_gin=t_gin, e_gin=e_gin + 3 * norm * t_gin, t_gout=t_gout, e_gout=e_gout + 3 * norm * t_gout)


def run_peer_bwd(ops, p, ins, sv, tables=True):
    """one device backward on pre-filled accumulators -> (dS, dip, g_in, g_out) whole buffers (guard rows included)"""
    M, nh, nq, k, din, dout = p.c
    S, ip, res, e_in, e_out = ins
    G, _ = with_tail(cuda(p.G))
    dS, _ = with_tail(cuda(pattern(M * nh, 2 * nq)))
    dip = nans(M + 1, nh * din, dtype=BF16)
    dip[M:] = SENT
    gin = with_tail(cuda(pattern(p.U, din)), 2)[0] if tables else None
    gout = with_tail(cuda(pattern(p.U, dout)), 2)[0] if tables else None
    keep = [t.clone() for t in (G, ip, e_in, e_out, sv.unit, sv.lr, sv.score, sv.dot)]
    ops.peer_lookup_bwd(G, ip, e_in, e_out, sv, dS, dip, gin, gout, M, nh, nq, k, din, dout)
    torch.cuda.synchronize()
    for a, b in zip((G, ip, e_in, e_out, sv.unit, sv.lr, sv.score, sv.dot), keep):
        assert torch.equal(a, b), 'an input changed'
    return dS, dip, gin, gout


def check_peer_bwd(p, b, r, got, tag):
    M, nh, nq, k, din, dout = p.c
    dS, dip, gin, gout = got
    R = M * nh
    # dS: pattern + ref; k = topk addends (+ 1 for the pattern) over |terms| taken down to the products of <dout, e_out>
    pS = pattern(R, 2 * nq).double()
    untouched = cuda(r.tS == 0)
    assert torch.equal(dS[:R][untouched], cuda(pattern(R, 2 * nq))[untouched]), f'{tag}: dS of an unchosen index changed'
    assert tail_ok(dS, R)
    check(f'{tag} dS', dS[:R], cuda(pS + r.dS), cuda(R32 * r.dS.abs() + (k + 1) * U32 * (r.tS + pS) + r.eS))
    assert tail_ok(dip, M)
    check(f'{tag} dip', dip[:M], cuda(r.dip), cuda(E7 * r.dip.abs() + E8 * r.t_ip))
    if gin is None:
        return
    for name, g, ref, terms, extra, w in (('g_emb_in', gin, r.gin, r.t_gin, r.e_gin, din), ('g_emb_out', gout, r.gout, r.t_gout, r.e_gout, dout)):
        pt = pattern(p.U, w)
        assert tail_ok(g, p.U), f'{tag}: the guard rows of {name} changed'
        assert torch.equal(g[:p.U][cuda(~b.touched)], cuda(pt)[cuda(~b.touched)]), f'{tag}: a {name} row that no candidate named changed'
        kk = (b.cnt + 1).double()[:, None]                   # the addends that reach the element, and the pattern under them
        check(f'{tag} {name}', g[:p.U], cuda(pt.double() + ref), cuda(R32 * ref.abs() + kk * U32 * (terms + pt.double()) + extra))


def cross_wave_collision(rt, k):
    """(row, head)s in which two candidates of different j % 4 -- different waves of the backward -- name the same unit"""
    same = rt.unit[:, :, None] == rt.unit[:, None, :]
    j = torch.arange(k)
    return (same & ((j[:, None] % 4) != (j[None, :] % 4))).any(-1).any(-1)


@pytest.mark.parametrize('c', PEER_BWD_CASES, ids=PEER_ID)
def test_peer_lookup_bwd(ops, c):
    M, nh, nq, k, din, dout = c
    b = peer_bwd_case(c)
    p, rt = b.p, b.p.rt
    assert not has_tie(rt.ls) and not has_tie(rt.rs) and not has_tie(rt.cs)
    if k > 1:                                               # several j share one l / one r: the += scatter into dS is exercised
        shared = lambda i: torch.tensor([len(set(row.tolist())) < k for row in i]).double().mean().item()
        assert shared(rt.l) > 0.5 and shared(rt.r) > 0.5
    assert int(b.cnt.max()) >= M / 2, 'no unit collects M / 2 contributions: the atomics would go untested'
    _, sv, ins = run_peer_fwd(ops, p)
    assert torch.equal(sv.unit[:M].cpu().view(-1, k).long(), rt.unit)
    r = peer_bwd_ref(p, sv.score[:M].cpu().view(-1, k), sv.dot[:M].cpu().view(-1, k))
    got = run_peer_bwd(ops, p, ins, sv)
    check_peer_bwd(p, b, r, got, f'peer_bwd {PEER_ID(c)}')
    frozen = run_peer_bwd(ops, p, ins, sv, tables=False)      # the frozen-table path: dS and dip bit-equal to the first run's
    assert torch.equal(frozen[0], got[0]) and torch.equal(frozen[1], got[1])


def test_peer_lookup_bwd_deterministic(ops):
    c = PEER_BWD_CASES[2]
    M, nh, nq, k, din, dout = c
    b = peer_bwd_case(c)
    p = b.p
    assert bool(cross_wave_collision(p.rt, k).any()), 'no (row, head) has two candidates of different waves on one unit'
    _, sv, ins = run_peer_fwd(ops, p)
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        runs = [run_peer_bwd(ops, p, ins, sv) for _ in range(2)]
    finally:
        ops.set_deterministic(was)
    for x, y in zip(*runs):
        assert torch.equal(x, y), 'two deterministic backward passes differ'
    r = peer_bwd_ref(p, sv.score[:M].cpu().view(-1, k), sv.dot[:M].cpu().view(-1, k))
    check_peer_bwd(p, b, r, runs[0], f'peer_bwd deterministic {PEER_ID(c)}')


def test_peer_lookup_bwd_refusals(ops):
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev())
    sv = SimpleNamespace(unit=z(64, dt=I32), lr=z(128, dt=I32), score=z(64), dot=z(64))
    dipb = z(72, dt=BF16)

    def call(M=2, nh=1, nq=16, k=4, din=8, dout=4, dip=dipb):
        return lambda: ops.peer_lookup_bwd(z(64), z(64, dt=BF16), z(64, dt=BF16), z(64, dt=BF16), sv, z(64), dip, None, None, M, nh, nq, k, din, dout)
    for kw in (dict(nq=3, k=4), dict(nq=1025), dict(nq=32, k=17), dict(din=12), dict(dout=6), dict(dout=8196), dict(dip=dipb[1:])):
        refused(call(**kw), 'i2t_peer_lookup_bwd: bad args (nq=')
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- LSH
#            (B, n_cls, bins, n_proj, dout, grid)
LSH_CASES = [(3, 3, (4, 8, 20), 32, 64, 'uniform'),         # the fixture's twin
             (2, 1, (1,), 1, 4, 'uniform'),                 # minimal; n_cls == 1: slot_stride == 0
             (2, 2, (7,) * 8, 128, 1028, 'uniform'),        # nK n_proj == 1024: the rid[] limit; dout > 1024: the column loop's second trip
             (4, 5, (5, 20), 16, 768, 'uniform'),           # odd nb: the grid holds zero
             (3, 3, (4, 8, 20), 32, 64, 'ragged')]          # a sorted non-uniform grid, as a checkpoint could load
LSH_BWD_CASES = [(70,) + LSH_CASES[0][1:]] + LSH_CASES[1:]
LSH_ID = lambda c: f'{c[0]}x{c[1]}x{"-".join(map(str, c[2])) if len(set(c[2])) > 1 else f"{len(c[2])}of{c[2][0]}"}x{c[3]}x{c[4]}-{c[5]}'
LEAD = 4                                                    # unrelated floats in front of slot 0


def lsh_grid(nb, kind, g):
    if kind == 'uniform':                                   # the module's: linspace(-1, 1, nb + 1)[:-1] + 1 / nb
        return (torch.linspace(-1, 1, nb + 1)[:-1] + 1 / nb).to(F32)
    v = torch.sort(torch.rand(nb, generator=g) * 2 - 1).values.to(F32)
    v[v.abs().argmin()] = 0.0                               # the point nearest zero becomes zero: still sorted
    return v


def lsh_layout(c):
    """the arena's layout: LEAD filler floats, then per slot the nK tables with 4 (k + 1) filler floats after table k; the slot stride
    is a multiple of 4 (0 for a single slot) -> (tab_off, stride, total floats, [(start, rows)] of slot 0's tables)"""
    B, ncls, bins, npj, dout, _ = c
    off, toff, spans = 0, [], []
    for kk, nb in enumerate(bins):
        toff.append(off)
        spans.append((off, (nb + 1) * npj))
        off += (nb + 1) * npj * dout + 4 * (kk + 1)
    stride = off if ncls > 1 else 0
    return toff, stride, LEAD + off * ncls, spans


@functools.lru_cache(maxsize=2)
def lsh_case(c):
    B, ncls, bins, npj, dout, kind = c
    nK = len(bins)
    g = torch.Generator().manual_seed(17 + B + ncls + npj + dout + sum(bins))
    grids = [lsh_grid(nb, kind, g) for nb in bins]
    assert all(bool((gr[1:] > gr[:-1]).all()) for gr in grids)
    toff, stride, total, spans = lsh_layout(c)
    arena = torch.full((total,), SENT, dtype=F32)
    is_table = torch.zeros(total, dtype=torch.bool)
    for s in range(ncls):
        for (st, rows) in spans:
            a0 = LEAD + s * (stride or 0) + st
            arena[a0:a0 + rows * dout] = torch.randn(rows * dout, generator=g)
            is_table[a0:a0 + rows * dout] = True
    # z: random values (N(0, 1/16)), and for every resolution every grid value, its two neighbours, values outside the grid, +-0 and +-1, planted at
    # random (image, slot, projection) places; a shape too small to hold them all takes several batches of z
    specials = []
    for gr in grids:
        sp = torch.cat([gr, torch.nextafter(gr, torch.tensor(2.0)), torch.nextafter(gr, torch.tensor(-2.0)),
                        torch.tensor([-1.5, gr[0].item() - 1e-3, gr[-1].item() + 1e-3, 1.5, 0.0, -0.0, 1.0, -1.0])])
        specials.append(sp.to(F32))
    places = B * ncls * npj
    rounds = max((len(sp) + places - 1) // places for sp in specials)
    zs = []
    for rd in range(rounds):
        z = (torch.randn(B, ncls, nK, npj, generator=g) * 0.25).to(F32)        # narrow: many images share the middle buckets
        for kk, sp in enumerate(specials):
            chunk = sp[rd * places:(rd + 1) * places]
            where = torch.randperm(places, generator=g)[:len(chunk)]
            zk = z[:, :, kk, :].reshape(-1)
            zk[where] = chunk
            z[:, :, kk, :] = zk.view(B, ncls, npj)
        zs.append(z.view(B, ncls * nK * npj).contiguous())
    dy = torch.randn(B * ncls, dout, generator=g)
    return SimpleNamespace(c=c, grids=grids, toff=toff, stride=stride, total=total, spans=spans, arena=arena, is_table=is_table, zs=zs, dy=dy,
                           specials=specials)


def lsh_rows_ref(q, z):
    """bucket = number of grid points strictly below z (fp32 compare); row = bucket + (nb + 1) j -> long [B][n_cls][nK][n_proj]"""
    B, ncls, bins, npj, dout, _ = q.c
    z = z.view(B, ncls, len(bins), npj)
    j = torch.arange(npj)
    return torch.stack([(q.grids[kk][None, None, None, :] < z[:, :, kk, :, None]).sum(-1) + (nb + 1) * j for kk, nb in enumerate(bins)], 2)


def lsh_flat_index(q, rows):
    """[B][n_cls][nK][n_proj] rows -> the arena index of column 0 of every named table row"""
    B, ncls, bins, npj, dout, _ = q.c
    s = torch.arange(ncls)[None, :, None, None]
    off = torch.tensor(q.toff)[None, None, :, None]
    return LEAD + s * q.stride + off + rows * dout


def lsh_device_args(q):
    goff = [0]
    for gr in q.grids[:-1]:
        goff.append(goff[-1] + len(gr))
    return SimpleNamespace(toff=cuda(torch.tensor(q.toff, dtype=torch.int64)), nbins=cuda(torch.tensor(q.c[2], dtype=I32)),
                           grids=cuda(torch.cat(q.grids + [torch.full((3,), SENT)])), goff=cuda(torch.tensor(goff, dtype=I32)))


def run_lsh_fwd(ops, q, z):
    B, ncls, bins, npj, dout, _ = q.c
    nK, a = len(bins), lsh_device_args(q)
    arena, zb = cuda(q.arena), cuda(with_tail(z)[0])
    keep = [t.clone() for t in (arena, zb, a.grids, a.toff, a.nbins, a.goff)]
    out = nans(B * ncls + 1, dout)
    out[B * ncls:] = SENT
    rows = torch.full((B * ncls + 1, nK, npj), ISENT, dtype=I32, device=dev())
    ops.lsh_embed_fwd(zb, arena[LEAD:], q.stride, a.toff, a.nbins, a.grids, a.goff, out, rows, B, ncls, nK, npj, dout)
    torch.cuda.synchronize()
    for x, y in zip((arena, zb, a.grids, a.toff, a.nbins, a.goff), keep):
        assert torch.equal(x, y), 'an input (the filler between tables included) changed'
    assert tail_ok(out, B * ncls) and tail_ok(rows, B * ncls, ISENT)
    return out, rows


@pytest.mark.parametrize('c', LSH_CASES, ids=LSH_ID)
def test_lsh_embed_fwd(ops, c):
    B, ncls, bins, npj, dout, kind = c
    q = lsh_case(c)
    nK = len(bins)
    seen = [set() for _ in bins]
    for rd, z in enumerate(q.zs):
        zz = z.view(B, ncls, nK, npj)
        for kk in range(nK):
            seen[kk] |= {v.item() for v in zz[:, :, kk].reshape(-1).view(I32)}
        rr = lsh_rows_ref(q, z)
        out, rows = run_lsh_fwd(ops, q, z)
        assert torch.equal(rows[:B * ncls].cpu().long().view(B, ncls, nK, npj), rr), f'lsh_fwd {LSH_ID(c)}: bucket rows differ'
        idx = lsh_flat_index(q, rr)[..., None] + torch.arange(dout)            # [B][n_cls][nK][n_proj][dout]
        vals = q.arena.double()[idx]
        ref = vals.sum((2, 3)) / npj
        terms = vals.abs().sum((2, 3)) / npj
        check(f'lsh_fwd {LSH_ID(c)} z{rd} out', out[:B * ncls], cuda(ref.view(B * ncls, dout)),
              cuda((R32 * ref.abs() + nK * npj * U32 * terms).view(B * ncls, dout)))
    for kk, sp in enumerate(q.specials):                    # every grid value, both neighbours, the outside values, +-0, +-1: bit patterns
        assert {v.item() for v in sp.view(I32)} <= seen[kk], 'a special z value was not planted'


def test_lsh_embed_fwd_refusals(ops):
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=dev())

    def call(nK=2, npj=4, dout=8, stride=64):
        return lambda: ops.lsh_embed_fwd(z(4096), z(4096), stride, z(32, dt=torch.int64), z(32, dt=I32), z(64), z(32, dt=I32), z(64), z(4096, dt=I32), 1, 1,
                                         nK, npj, dout)
    refused(call(nK=25, npj=41), 'i2t_lsh_embed_fwd: bad args (nK * n_proj = 1025')
    refused(call(dout=6), 'i2t_lsh_embed_fwd: bad args')
    refused(call(stride=66), 'i2t_lsh_embed_fwd: bad args')
    refused(lambda: ops.lsh_embed_bwd(z(64), z(4096, dt=I32), z(4096), 64, z(32, dt=torch.int64), 1, 1, 25, 41, 8), 'i2t_lsh_embed_bwd: bad args (nK * n_proj = 1025')
    torch.cuda.synchronize()


def lsh_bwd_ref(q, rr):
    """g_table_k[row] += dy / n_proj in float64 for every (b, s, k, j) -> (sum, sum |terms|, addends) over the whole arena"""
    B, ncls, bins, npj, dout, _ = q.c
    idx = (lsh_flat_index(q, rr)[..., None] + torch.arange(dout)).reshape(-1)
    add = (q.dy.double() / npj).view(B, ncls, 1, 1, dout).expand(B, ncls, len(bins), npj, dout).reshape(-1)
    ref = torch.zeros(q.total, dtype=F64).index_add_(0, idx, add)
    terms = torch.zeros(q.total, dtype=F64).index_add_(0, idx, add.abs())
    cnt = torch.zeros(q.total, dtype=F64).index_add_(0, idx, torch.ones_like(add))
    return ref, terms, cnt


def run_lsh_bwd(ops, q, rows):
    B, ncls, bins, npj, dout, _ = q.c
    a = lsh_device_args(q)
    g0 = torch.where(q.is_table, pattern(q.total), torch.full((q.total,), SENT))
    g, dy = cuda(g0), cuda(with_tail(q.dy)[0])
    keep = dy.clone()
    ops.lsh_embed_bwd(dy, rows, g[LEAD:], q.stride, a.toff, B, ncls, len(bins), npj, dout)
    torch.cuda.synchronize()
    assert torch.equal(dy, keep)
    return g, g0


def check_lsh_bwd(q, ref, terms, cnt, g, g0, tag):
    named = cuda(cnt > 0)
    assert torch.equal(g[~named], cuda(g0)[~named]), f'{tag}: a table row that no bucket named, or the filler between tables, changed'
    assert bool((q.is_table | (cnt == 0)).all())
    p0 = torch.where(q.is_table, g0, torch.zeros(())).double()
    got, want = g[named], cuda(p0 + ref)[named]
    check(f'{tag} g_tables', got, want, (R32 * want.abs() + cuda((cnt + 1) * U32 * (terms + p0.abs()))[named]))


@pytest.mark.parametrize('c', LSH_BWD_CASES, ids=LSH_ID)
def test_lsh_embed_bwd(ops, c):
    B, ncls = c[:2]
    q = lsh_case(c)
    _, rows = run_lsh_fwd(ops, q, q.zs[0])
    rr = lsh_rows_ref(q, q.zs[0])
    assert torch.equal(rows[:B * ncls].cpu().long().view(rr.shape), rr)
    ref, terms, cnt = lsh_bwd_ref(q, rr)
    assert cnt.max().item() >= B / 2, 'no table row collects B / 2 addends: the atomics would go untested'
    g, g0 = run_lsh_bwd(ops, q, rows)
    check_lsh_bwd(q, ref, terms, cnt, g, g0, f'lsh_bwd {LSH_ID(c)}')


def test_lsh_embed_bwd_deterministic(ops):
    c = LSH_BWD_CASES[0]
    q = lsh_case(c)
    _, rows = run_lsh_fwd(ops, q, q.zs[0])
    rr = lsh_rows_ref(q, q.zs[0])
    ref, terms, cnt = lsh_bwd_ref(q, rr)
    assert cnt.max().item() >= c[0] / 2
    was = ops.deterministic()
    ops.set_deterministic(True)
    try:
        runs = [run_lsh_bwd(ops, q, rows) for _ in range(2)]
    finally:
        ops.set_deterministic(was)
    assert torch.equal(runs[0][0], runs[1][0]), 'two deterministic backward passes differ'
    check_lsh_bwd(q, ref, terms, cnt, *runs[0], f'lsh_bwd deterministic {LSH_ID(c)}')
