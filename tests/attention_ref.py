"""Float64 statement of the attention kernels (csrc/attention.hip, csrc/attention_g.hip) and the per-element error bounds of
DESIGN.md "Attention kernels against fp64" -- a plain helper module of tests/test_attention_kernels_gpu.py (no kernel is called
here).  Everything works on ONE sequence at a time: q / dO / O [H, Tq, hd], k / v [Hkv, Tk, hd] (float64 copies of the bf16
values the kernel reads), the visibility mask [Tq, Tk] and the dropout keep mask [H, Tq, Tk].

The rounding points, read out of the kernels (they are the same in every variant):
  forward   p~ = exp2(s c - m) in fp32 (raw v_exp_f32) -> bf16 MFMA operand (ONE rounding) -> fp32 accumulation over the keys
            -> x 1 / l (l summed in fp32 from the UNROUNDED p~) -> bf16 store (ONE rounding);
  backward  p = exp2(s c - lse c') in fp32; delta and dP in fp32; dS = p (mask sc dP - delta) in fp32 -> bf16 operand (ONE rounding)
            of dQ = dS K and dK = dS^T Q; p mask -> bf16 operand (ONE rounding) of dV = P^T dO; fp32 accumulation; bf16 store.
ONE round-to-nearest to bf16 (8 significant bits) errs by half an ulp = 2^-9 of the binade's UPPER end, i.e. up to 2^-8 of the
value: RN = 2 units of 2^-9.  So c_q = c_k = c_v = 2 and the gradients' store costs 2 x 2^-9 |dX|.  The output keeps the form
c_o 2^-9 sum p |v| + 2^-9 |O| with c_o = 3: two units for the rounding of P and one for the half of the store's worst case that
2^-9 |O| leaves open (|O| <= sum p |v|).  What is left are fp32 terms, written out below with their counts."""
import math
from types import SimpleNamespace

import torch

F64 = torch.float64
E9 = 2.0 ** -9                     # the unit of the bf16 terms
RN = 2                             # one round-to-nearest to bf16, in units of E9
C_O = RN + 1                       # the output's count (module docstring)
U24 = 2.0 ** -24                   # half an ulp of fp32, relative
FLUSH = 2.0 ** -110                # a probability below 2^-126 is flushed to zero: x |operand| < 2^7 x keys < 2^9
# The raw v_exp_f32 against float64 exp2: largest relative error measured on the MI355X over the arguments these tests produce
# (every multiple of 2^-14 in [-126, 0]: the arguments are s c - m <= 0 and s c - lse c' <= 0): 8.14e-8, at x = -0.938171.  Four times
# that is allowed.
EXP2_MEASURED = 8.2e-8
EXP2_ALLOW = 4 * EXP2_MEASURED
LSE_ULPS = 5                       # m c (2 roundings: product, constant), log2f(l) (1 ulp), their sum, x ln 2 (2): <= 4.5 ulp of the largest


def visible(Tq, Tk, causal, split, device):
    """bool [Tq, Tk]: key j is visible to row i (causal with offset Tk - Tq; split: rows >= split do not see keys < split)"""
    i = torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    vis = torch.ones(Tq, Tk, dtype=torch.bool, device=device)
    if causal:
        vis &= j <= i + (Tk - Tq)
    if split:
        vis &= ~((i >= split) & (j < split))
    return vis


def _p_eps(S0, ref_abs, A):
    """relative error of ONE fp32 probability exp2(s c - x): the hardware exp, the argument's roundings (the fp32 constant
    SCALE LOG2E and the fma: 2^-24 (|s| + |x|) each, x = the running maximum or lse, both <= ref_abs) and the fp32 accumulation of
    the score (<= 8 roundings of sum |q_d k_d| scale = A); the argument is in log2 units, d p / p = ln 2 d arg: natural units here"""
    return EXP2_ALLOW + U24 * (4 * (S0.abs() + ref_abs[..., None]) + 8 * A)


def forward(q, k, v, scale, vis, keep, sc):
    """-> namespace(S0, A, lse, m, P, O, o_bound, lse_bound): the forward and its bounds.  k, v are [Hkv, Tk, hd]: expanded here."""
    H, Tq, hd = q.shape
    G, Tk = H // k.shape[0], k.shape[1]
    kx, vx = k.repeat_interleave(G, 0), v.repeat_interleave(G, 0)
    S0 = (q @ kx.transpose(1, 2)) * scale
    A = (q.abs() @ kx.abs().transpose(1, 2)) * scale
    S0 = torch.where(vis, S0, torch.zeros_like(S0))
    S = S0.masked_fill(~vis, float('-inf'))
    lse = torch.logsumexp(S, -1)
    m = S.max(-1).values
    P = torch.exp(S - lse[..., None])
    M = torch.ones_like(P) if keep is None else keep.to(F64) * sc
    Pd = P * M
    O = Pd @ vx
    ref_abs = torch.maximum(lse.abs(), m.abs())
    eps = _p_eps(S0, ref_abs, torch.where(vis, A, torch.zeros_like(A)))
    ebar = (P * eps).sum(-1) + Tk * U24                     # relative error of the fp32 denominator l
    relP = eps + ebar[..., None]
    PV = Pd @ vx.abs()
    # bf16 P and half the store (c_o = 3) and P's fp32 error | fp32 accumulation over the keys, the per-tile rescales, 1 / l and the product | the store
    o_bound = ((C_O * E9 + relP) * Pd) @ vx.abs() + (Tk + 8) * U24 * PV + E9 * O.abs() + FLUSH
    Amax = torch.where(vis, A, torch.zeros_like(A)).max(-1).values
    lse_bound = LSE_ULPS * 2 * U24 * torch.maximum(ref_abs, torch.ones_like(ref_abs)) + ebar + 8 * U24 * Amax
    return SimpleNamespace(S0=S0, A=torch.where(vis, A, torch.zeros_like(A)), lse=lse, m=m, P=P, O=O, o_bound=o_bound, lse_bound=lse_bound, kx=kx, vx=vx)


def backward(q, k, v, scale, vis, keep, sc, O_st, lse_st, dO, fq=None, fk=None, fv=None):
    """The backward from the values the kernels read: the STORED O (bf16) and lse (fp32) and dO.  fq [Tq], fk, fv [Tk]: the out_drop
    multipliers (None: 1).  -> namespace(dq [H, Tq, hd], dk, dv [Hkv, Tk, hd] and *_bound)."""
    H, Tq, hd = q.shape
    Hkv, Tk = k.shape[0], k.shape[1]
    G = H // Hkv
    kx, vx = k.repeat_interleave(G, 0), v.repeat_interleave(G, 0)
    zero = torch.zeros(H, Tq, Tk, dtype=F64, device=q.device)
    S0 = torch.where(vis, (q @ kx.transpose(1, 2)) * scale, zero)
    A = torch.where(vis, (q.abs() @ kx.abs().transpose(1, 2)) * scale, zero)
    P = torch.where(vis, torch.exp(S0 - lse_st[..., None]), zero)
    M = torch.ones_like(P) if keep is None else keep.to(F64) * sc
    delta, Dabs = (dO * O_st).sum(-1), (dO.abs() * O_st.abs()).sum(-1)
    dP, DPabs = dO @ vx.transpose(1, 2), dO.abs() @ vx.abs().transpose(1, 2)
    dS = P * (M * dP - delta[..., None])
    eps = _p_eps(S0, lse_st.abs(), A)
    # fp32 error of dS before its rounding: p's own | the fma and the product (2 roundings) | dP's accumulation (<= 8) | delta's
    # (hd / 4 products per lane summed one by one, then the shuffles: hd / 4 + 4)
    e32 = P * ((eps + 2 * U24) * (M * dP.abs() + delta.abs()[..., None]) + 8 * U24 * M * DPabs + (hd // 4 + 4) * U24 * Dabs[..., None])
    errS = RN * E9 * dS.abs() + e32                               # c_q = c_k = 2: one bf16 rounding of dS
    Pd = P * M
    errP = (RN * E9 + eps) * Pd                                   # c_v = 2: one bf16 rounding of P mask (sc rides on the accumulator)
    dq = scale * (dS @ kx)
    dq_bound = scale * (errS @ kx.abs()) + (Tk + 8) * U24 * scale * (dS.abs() @ kx.abs())
    dkh = scale * (dS.transpose(1, 2) @ q)                   # per query head; the group's heads are summed in the same accumulator
    dkh_bound = scale * (errS.transpose(1, 2) @ q.abs()) + (G * Tq + 8) * U24 * scale * (dS.abs().transpose(1, 2) @ q.abs())
    dvh = Pd.transpose(1, 2) @ dO
    dvh_bound = errP.transpose(1, 2) @ dO.abs() + (G * Tq + 8) * U24 * (Pd.transpose(1, 2) @ dO.abs())
    grp = lambda t: t.view(Hkv, G, Tk, hd).sum(1)            # the sum over the group's query heads goes INSIDE the absolute product
    dk, dk_bound, dv, dv_bound = grp(dkh), grp(dkh_bound), grp(dvh), grp(dvh_bound)
    if fq is not None:
        dq, dq_bound = dq * fq[None, :, None], dq_bound * fq[None, :, None]
        dk, dk_bound = dk * fk[None, :, None], dk_bound * fk[None, :, None]
        dv, dv_bound = dv * fv[None, :, None], dv_bound * fv[None, :, None]
    return SimpleNamespace(dq=dq, dk=dk, dv=dv, dq_bound=dq_bound + RN * E9 * dq.abs() + FLUSH, dk_bound=dk_bound + RN * E9 * dk.abs() + FLUSH,
                           dv_bound=dv_bound + RN * E9 * dv.abs() + FLUSH)


# ------------------------------------------------------------------------------------------------------------ input regimes
NCODE = 9                                                   # head dims 0 .. 8 carry a +-1 code of the key index (512 codes > any Tk here)
RISE_DIM, OFF_DIM = 9, 10                                   # the dim of the rising component and of the shared offset (hd >= 16)
PLANTS = ('first', 'last', 'tail', 'diag', 'rising')


def _code(j):
    bits = (j[:, None] >> torch.arange(NCODE)[None, :]) & 1
    return bits.to(torch.float32) * 2 - 1


def plant_target(plant, Tq, Tk, causal):
    """the key each query row is pointed at (long [Tq])"""
    i = torch.arange(Tq)
    shift = Tk - Tq
    if plant == 'first':
        t = i % min(64, Tk)
    elif plant == 'last':
        s0 = ((Tk - 1) // 64) * 64
        t = s0 + i % (Tk - s0)
    elif plant == 'tail':
        t = torch.full((Tq,), Tk - 1)
    else:                                                   # 'diag': the causal diagonal (the last visible key of the row)
        t = (i + shift).clamp(0, Tk - 1) if shift >= 0 else i % Tk
    if causal:
        t = torch.minimum(t, i + shift)
    return t


def make_sequence(gen, H, Hkv, hd, Tq, Tk, causal, regime, plant):
    """fp32 q [Tq, H, hd], k, v [Tk, Hkv, hd], dO [Tq, H, hd] of one sequence (the caller rounds them to bf16).
    regime 'n01': N(0, 1).  'peak': scores of standard deviation ~6 and one dominant key per row, planted by a code both sides carry
    (the same code scores 36, a code one bit off 28); plant 'rising' instead lifts every 64-key tile 12 nats over the one before it, so
    that every rescale of the running softmax has alpha = e^-12.  'offset': a component shared by ALL keys, so that every score of a
    row moves by +60 (even rows) or -60 (odd rows): lse ~ +-60, the probabilities unchanged."""
    scale = 1.0 / math.sqrt(hd)
    q = torch.randn(Tq, H, hd, generator=gen)
    k = torch.randn(Tk, Hkv, hd, generator=gen)
    v = torch.randn(Tk, Hkv, hd, generator=gen)
    do = torch.randn(Tq, H, hd, generator=gen)
    if regime == 'peak' and plant == 'rising':
        q[:, :, RISE_DIM] = 4.0
        k[:, :, RISE_DIM] = ((torch.arange(Tk) // 64).float() * (3.0 / scale))[:, None]
    elif regime == 'peak':
        g = math.sqrt(4.0 / scale)
        q[:, :, NCODE:] *= 6.0
        k[:, :, :NCODE] = g * _code(torch.arange(Tk))[:, None, :]
        q[:, :, :NCODE] = g * _code(plant_target(plant, Tq, Tk, causal))[:, None, :]
    elif regime == 'offset':
        sign = (1 - 2 * (torch.arange(Tq) % 2)).float()
        k[:, :, OFF_DIM] = 16.0
        q[:, :, OFF_DIM] = (sign * (60.0 / (16.0 * scale)))[:, None]
    return q, k, v, do


# ------------------------------------------------------------------------------------------------------------------ cases
# The cases of tests/test_attention_kernels_gpu.py and the kernel each one is meant for.  They live here, in a module that imports
# without a device, so that tests/test_attention_route_cpu.py can hold ``route`` against csrc/attention_route.h for every one of them.
ENVS = ('I2T_ATTN_V2', 'I2T_ATTN_BWD', 'I2T_ATTN_BWD2', 'I2T_ATTN_BWD1', 'I2T_ATTN_BWD3_WAVES')


def C(api='mha', B=1, H=2, Hkv=None, hd=64, Tq=64, Tk=None, causal=False, drop=False, lens=None, cross=False, split=0, od=False,
      q_seq=0, regime='n01', plant='first', bwd=True):
    """one case.  lens: packed queries (cu_q; with cross=False the keys are packed the same way, cu_k = cu_q); q_seq: the queries are
    the first Tq rows of sequences of q_seq rows (out_drop_q_seq); od: out_drop on."""
    Tk = Tq if Tk is None else Tk
    Hkv = H if Hkv is None else Hkv
    if lens is not None:
        B = len(lens)
    c = SimpleNamespace(api=api, B=B, H=H, Hkv=Hkv, hd=hd, Tq=Tq, Tk=Tk, causal=causal, drop=drop, lens=lens, cross=cross or Tq != Tk,
                        split=split, od=od, q_seq=q_seq, regime=regime, plant=plant if regime == 'peak' else '-', bwd=bwd)
    c.id = (f'{api}-B{B}H{H}' + (f'kv{Hkv}d{hd}' if api == 'gq' else '') + f'-{Tq}x{Tk}' + ('-causal' if causal else '') +
            ('-drop' if drop else '') + (f'-lens{"_".join(map(str, lens))}' + ('x' if c.cross else 's') if lens is not None else '') +
            (f'-split{split}' if split else '') + ('-od' if od else '') + (f'-qseq{q_seq}' if q_seq else '') +
            f'-{regime}' + (f'_{plant}' if regime == 'peak' else ''))
    return c


def regimes(bases):
    """every base case in the three input regimes; the planted key's place rotates over the cases"""
    out, n = [], 0
    for kw in bases:
        for regime in ('n01', 'peak', 'offset'):
            plants = ('first', 'diag', 'rising') if kw.get('causal') else ('first', 'last', 'tail', 'rising')
            out.append(C(regime=regime, plant=plants[n % len(plants)], **kw))
            n += regime == 'peak'
    return out


def v2_applies(c, env):
    """csrc/attention_route.h::attn_resident"""
    return (env.get('I2T_ATTN_V2', '1')[:1] != '0' and not c.causal and c.lens is None and c.Tk <= 288 and 64 <= c.Tq <= 304 and
            (not c.drop or c.Tk % 4 == 0))


def drop_variant(c):
    return 'nodrop' if not c.drop else ('even' if c.Tk % 4 == 0 else 'odd')


def route(c, env):
    """(forward kernel, backward kernel) of a head_dim-64 call: csrc/attention_route.h::attn_fwd_route / attn_bwd_route restated
    (tests/test_attention_route_cpu.py holds the two together).  CNT, the key blocks per wave, is chosen inside attn_bwd3_kernel."""
    v2 = v2_applies(c, env)
    fwd = f'fwd2<PER={((c.Tq + 15) >> 4) >> 2}>' if v2 else f'fwd<{drop_variant(c)}>'
    mode = 0 if env.get('I2T_ATTN_BWD2', '1')[:1] == '0' else int(env.get('I2T_ATTN_BWD', '3'))
    nkb = (c.Tk + 15) >> 4
    if mode == 3 and v2 and c.Tq <= 288:
        nwv = 9 if env.get('I2T_ATTN_BWD3_WAVES') == '9' else 8
        bwd = f'bwd3<{nwv},CNT={min(-(-nkb // nwv), 2 if nwv == 9 else 3)}>'
    elif mode != 0 and v2 and c.Tq <= 288:
        bwd = 'bwd2'
    elif c.Tq <= 64 and c.Tk <= 64 and env.get('I2T_ATTN_BWD1', '1')[:1] != '0':
        bwd = f'bwd1<{drop_variant(c)}>'
    else:
        bwd = f'pair<{drop_variant(c)}>'
    return fwd, bwd


# head_dim 64 (the smallest sizes that reach each branch; B, H > 1 in at least one case per kernel)
FWD_TILED = regimes(
    [dict(Tq=1, causal=True, bwd=False), dict(B=2, H=3, Tq=16, causal=True), dict(Tq=37, causal=True), dict(B=2, Tq=64, causal=True),
     dict(Tq=65, causal=True), dict(B=2, H=2, Tq=130, causal=True), dict(B=2, H=1, Tq=33, Tk=131, causal=True), dict(B=2, Tq=1, Tk=50, causal=True),
     dict(B=2, H=1, Tq=5, Tk=9), dict(B=2, H=1, Tq=24), dict(Tq=70, Tk=320), dict(B=2, H=3, Tq=320, Tk=40),
     dict(Tq=70, Tk=37, drop=True), dict(B=2, H=3, Tq=100, Tk=131, drop=True), dict(B=2, Tq=130, causal=True, drop=True),
     dict(H=2, Tq=65, lens=(0, 1, 64, 65, 5), causal=True), dict(H=2, Tq=65, lens=(0, 1, 64, 65, 5), causal=True, drop=True),
     dict(H=2, Tq=65, Tk=130, lens=(5, 64, 0, 65, 1), cross=True), dict(H=3, Tq=65, Tk=197, lens=(5, 64, 0, 65, 1), cross=True),
     dict(H=2, Tq=65, Tk=197, lens=(5, 64, 0, 65, 1), cross=True, drop=True, od=True)])
FWD_V2 = regimes(
    [dict(B=2, H=3, Tq=64, Tk=9), dict(Tq=112, Tk=64), dict(Tq=113, Tk=197), dict(Tq=176, Tk=288), dict(Tq=177, Tk=64, drop=True),
     dict(B=2, Tq=240, Tk=197), dict(Tq=241, Tk=9), dict(Tq=241, Tk=288, drop=True), dict(B=2, H=2, Tq=304, Tk=288), dict(Tq=304, Tk=64, drop=True)])
BWD3 = regimes(
    [dict(B=2, H=3, Tq=64, Tk=16), dict(Tq=197, Tk=17), dict(Tq=288, Tk=128), dict(Tq=64, Tk=129), dict(B=2, Tq=197, Tk=197),
     dict(Tq=288, Tk=256), dict(Tq=64, Tk=257), dict(Tq=197, Tk=272), dict(Tq=288, Tk=288),
     dict(Tq=64, Tk=16, drop=True), dict(B=2, Tq=288, Tk=128, drop=True), dict(Tq=197, Tk=272, drop=True), dict(Tq=288, Tk=288, drop=True, od=True),
     dict(B=2, Tq=197, Tk=197, od=True)])
BWD3_QSEQ = regimes([dict(B=2, H=2, Tq=64, Tk=197, od=True, q_seq=197), dict(B=2, H=2, Tq=64, Tk=196, od=True, q_seq=196, drop=True)])
BWD1 = regimes(
    [dict(B=2, H=3, Tq=64, causal=True), dict(Tq=37, causal=True), dict(Tq=16, causal=True), dict(Tq=33, Tk=50, causal=True), dict(B=2, H=1, Tq=5, Tk=9),
     dict(Tq=24), dict(Tq=40, Tk=64), dict(B=2, Tq=64, causal=True, drop=True), dict(Tq=24, drop=True), dict(Tq=37, causal=True, drop=True),
     dict(B=2, Tq=5, Tk=9, drop=True), dict(B=2, Tq=40, causal=True, od=True),
     dict(H=2, Tq=64, lens=(0, 1, 64, 37), causal=True), dict(H=2, Tq=64, lens=(0, 1, 64, 37), causal=True, drop=True, od=True),
     dict(H=2, Tq=64, Tk=24, lens=(5, 0, 64, 16), cross=True), dict(H=2, Tq=64, Tk=37, lens=(5, 0, 64, 16), cross=True, drop=True)])
PAIR = [c for c in FWD_TILED if c.bwd and route(c, {})[1].startswith('pair')] + regimes([dict(B=2, H=2, Tq=304, Tk=288), dict(Tq=304, Tk=64, drop=True)])

# the A/B switches of the encoder backward: name -> (environment, the kernel the BWD3 shapes then run on)
SWITCHES = {'waves9': ({'I2T_ATTN_BWD3_WAVES': '9'}, 'bwd3<9'), 'bwd2': ({'I2T_ATTN_BWD': '2'}, 'bwd2'), 'bwd0': ({'I2T_ATTN_BWD': '0'}, 'pair<'),
            'bwd2off': ({'I2T_ATTN_BWD2': '0'}, 'pair<')}

# grouped heads
GQ = regimes(
    [dict(api='gq', B=2, H=8, Hkv=1, hd=16, Tq=70, causal=True), dict(api='gq', H=8, Hkv=1, hd=16, Tq=33, Tk=131),
     dict(api='gq', B=2, H=4, Hkv=2, hd=32, Tq=130, causal=True), dict(api='gq', H=4, Hkv=2, hd=32, Tq=257), dict(api='gq', H=2, Hkv=2, hd=32, Tq=1, Tk=50, causal=True),
     dict(api='gq', B=2, H=2, Hkv=2, hd=64, Tq=65, causal=True), dict(api='gq', H=8, Hkv=1, hd=64, Tq=70, Tk=37, drop=True),
     dict(api='gq', H=2, Hkv=1, hd=128, Tq=257, causal=True), dict(api='gq', B=2, H=2, Hkv=2, hd=128, Tq=64, Tk=130),
     dict(api='gq', H=2, Hkv=1, hd=128, Tq=100, Tk=131, drop=True, od=True), dict(api='gq', B=2, H=4, Hkv=2, hd=16, Tq=40, Tk=37, drop=True),
     dict(api='gq', H=4, Hkv=2, hd=32, Tq=65, lens=(0, 1, 64, 65, 5), causal=True), dict(api='gq', H=4, Hkv=2, hd=64, Tq=65, lens=(0, 1, 64, 65, 5), causal=True, drop=True, od=True),
     dict(api='gq', H=8, Hkv=1, hd=64, Tq=65, Tk=130, lens=(5, 64, 0, 65), cross=True), dict(api='gq', B=2, H=4, Hkv=2, hd=64, Tq=96, od=True)])
GQ_SPLIT = regimes([dict(api='gq', B=B, H=H, Hkv=Hkv, hd=hd, Tq=T, split=s, bwd=False)
                    for T, (B, H, Hkv, hd) in ((96, (2, 4, 2, 32)), (130, (1, 2, 1, 64))) for s in (1, 63, 64, 65, T - 1)])
