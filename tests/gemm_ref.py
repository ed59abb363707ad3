"""float64 statements of the GEMM kernels (csrc/gemm.hip: every instantiation i2t_gemm_bf16* / i2t_gemm_dw_colsum_bf16 /
i2t_gemm_bf16_ws / i2t_colsum_bf16_ex can launch, the fp8 / top2 / lse / fused cross-attention classes apart) on the host, with
the kernels' rounding points restated, the per-element bounds that follow from them, the routing rule of csrc/gemm_route.h
restated in Python and the case table of tests/test_gemm_kernels_gpu.py.  Plain torch on the CPU, nothing from the GPU.

Rounding points: operands are bf16 numbers; products are exact and summed in fp32 by the MFMA (one 64-wide K step = two
16x16x32 instructions); K slices are combined by float atomics (g128 split-K, skinny K-split, dW classes 6 / 13), by a fixed-order
sum of fp32 planes (ws + reduce) or by read-add-write (dW class 5 chunks); the epilogue runs in fp32 (alpha, bias, activation,
dropout multiplier, residual, accumulate); ONE rounding at a bf16 store (C and aux_out each).

    fp32 output:  |got - ref| <= 2^-23 |ref| + k 2^-23 S + extra          bf16 output:  2^-8 |ref| + k 2^-23 S + extra

S = the same expression over |terms| (every product times |alpha f|, |bias|, |residual|, |C before the call|); k = 64-wide K steps
on the longest fp32 path + slices / atomics / planes combined + additions of the epilogue (``fp32_k``, from the restated route);
extra = the activation's allowance (GELU: |gelu'(v)| dv + rel |gelu(v)| + flush, from _gelu_tanh64 / ERF_PHI_ERR).
DESIGN.md "GEMM kernels against fp64"."""
import math
import zlib
from types import SimpleNamespace as NS

import torch

from test_row_kernels_gpu import ERF_PHI_ERR, TINY, _gelu_erf64, _gelu_tanh64, bf16_round

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
E8, U32 = 2.0 ** -8, 2.0 ** -23
NONE, GELU, DGELU, GELU_ERF, DGELU_ERF, GELU_DOUT, MUL_AUX = range(7)          # include/i2t.h I2T_ACT_*
II_BF16, II_F32 = 1 / 128, 1 / 256                              # condition 2: median(bound) <= rms(ref) x this
N_CU = 256                                                      # MI355X; the GPU test passes the device's own count


def r8(x):
    return (x + 7) & ~7


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------- csrc/gemm_route.h, restated
CALL_DEFAULTS = dict(f32=0, acc=0, act=0, drop=0, bias=0, auxi=0, auxo=0, res=0, alpha1=1, cso=0, c16=1, auxo16=1, resc=0, ak=0, bk=0)
CALL_DEFAULTS['as'] = 0
KNOB_DEFAULTS = dict(no_g256=0, min_tiles=40, gemm3=0, narrow=0, ksplit=0, fold=1, dw_splits=0, gn=8, stagger=0, stagger_groups=2,
                     g256_dbg=0, g3_dbg=0, fp8_g256=1, log=0)


def parse_call(text):
    """'M=17 N=72 K=136 bias=1 ...' (the line format of tests/gemm_route_cli.cpp) -> (call, knobs, n_cu, deterministic)"""
    v = {k: int(x) for k, x in (f.split('=') for f in text.split())}
    knobs = {k: v.pop(k, d) for k, d in KNOB_DEFAULTS.items()}
    n_cu, det = v.pop('n_cu', N_CU), bool(v.pop('det', 0))
    c = dict(CALL_DEFAULTS)
    c.update(v)
    c['lda'] = v.get('lda', r8(c['M'] if c['ak'] else c['K']))
    c['ldb'] = v.get('ldb', r8(c['N'] if c['bk'] else c['K']))
    c['ldc'] = v.get('ldc', c['N'])
    for k in ('ldai', 'ldao', 'ldr'):
        c[k] = v.get(k, c['ldc'])
    return NS(**c), NS(**knobs), n_cu, det


def epilogue_class(c):
    fast4 = c.ldc % 4 == 0 and (not c.res or c.ldr % 4 == 0) and (not c.auxi or c.ldai % 4 == 0) and (not c.auxo or c.ldao % 4 == 0)
    none = c.act == NONE and not c.auxo
    if fast4 and c.N % 4 and none and not c.bias and not c.res and not c.acc and not c.drop:
        return 7
    if not fast4 or c.N % 4:
        return 0
    plain = not c.drop and not c.res and not c.acc
    if not c.f32 and none and not c.res and not c.acc and c.drop != 1:
        return 1
    if not c.f32 and c.act == GELU and plain:
        return 2
    if not c.f32 and c.act == GELU_DOUT and plain:
        return 10
    if not c.f32 and c.act == MUL_AUX and not c.bias and not c.auxo and plain:
        return 11
    if c.f32 and none and not c.acc and c.drop != 2 and (c.res or c.bias or c.drop):
        return 3
    if not c.f32 and c.act == DGELU and not c.bias and not c.auxo and plain:
        return 4
    if c.f32 and none and not c.bias and not c.res and not c.drop:
        return 5
    return 0


def dw_plan(M, N, kchunk, class5, cso, knobs, n_cu, det):
    """-> (cls, splits, per, colsum) with colsum in 'none' | 'folded' | 'before'; cls 0: no large-tile form"""
    tiles, nk_all = cdiv(M, 256) * cdiv(N, 256), (kchunk + 63) >> 6
    own = 'before' if cso else 'none'
    if tiles >= n_cu or n_cu // tiles < 2 or det:
        return (5, 1, (nk_all + 1) & ~1, own) if class5 else (0, 0, 0, 'none')
    splits = knobs.dw_splits or n_cu // tiles
    per = max(8, (cdiv(nk_all, splits) + 1) & ~1)
    splits = cdiv(nk_all, per)
    if splits < 2:
        return (0, 0, 0, 'none')
    return (13, splits, per, 'folded') if cso and knobs.fold else (6, splits, per, own)


def gemm_route(c, knobs, n_cu=N_CU, det=False):
    if c.M <= 64 and not c.ak and not c.bk and not c.auxo and c.act <= GELU and not c.acc and not c.drop:
        ks, ntiles = 1, cdiv(c.N, 16)
        if knobs.ksplit and c.f32 and c.resc and c.ldr == c.ldc and c.act == NONE:
            while ntiles * ks < 256 and (c.K // 64) // (ks * 2) >= 2 and ks < 16:
                ks *= 2
        return NS(kind='skinny', mt=min(cdiv(c.M, 16), 4), ksplit=ks, colsum='none')
    if (not knobs.no_g256 and c.ak and c.bk and c.acc and c.f32 and not c.bias and c.act == NONE and not c.auxo and not c.res and not c.drop
            and c.M >= 256 and c.N >= 256 and c.ldc % 4 == 0 and c.N % 4 == 0):
        k_fit = (1 << 32) // (2 * max(c.lda, c.ldb)) - 512
        if k_fit >= 1024:
            class5 = epilogue_class(c) == 5
            kc = c.K if c.K <= k_fit else (k_fit // 128) * 128
            n_full, k_tail = c.K // kc, c.K % kc
            full = dw_plan(c.M, c.N, kc, class5, c.cso, knobs, n_cu, det)
            if full[0]:
                r = NS(kind='dw', kc=kc, chunks=n_full, chunk_error=False, full=full, tail=None)
                if k_tail:
                    r.tail = dw_plan(c.M, c.N, k_tail, class5, c.cso, knobs, n_cu, det)
                    if r.tail[0]:
                        r.chunks += 1
                    else:
                        r.chunk_error = True
                return r
    colsum = 'before' if c.cso else 'none'
    splits = 1
    if c.acc and c.f32 and not c.bias and c.act == NONE and not c.auxo and not c.res and not c.drop:
        tiles, nk_all = cdiv(c.M, 128) * cdiv(c.N, 128), cdiv(c.K, 64)
        while tiles * splits < 384 and nk_all // (splits * 2) >= 4 and splits < 64:
            splits *= 2
        if det:
            splits = 1
    cls = epilogue_class(c)
    if (knobs.gemm3 and splits == 1 and not c.ak and not c.bk and c.K % 64 == 0 and c.alpha1 and not getattr(c, 'as') and c.N % 8 == 0
            and c.ldc % 8 == 0 and c.c16
            and ((cls == 1 and c.K >= 320) or (cls == 2 and c.K >= 512 and (not c.auxo or (c.ldao % 8 == 0 and c.auxo16))))
            and cdiv(c.M, 256) * cdiv(c.N, 128) >= 2 * knobs.min_tiles):
        return NS(kind='gemm3', cls=cls, overlap=knobs.gemm3 == 2, colsum=colsum)
    g256_ok = ((c.K % 128 == 0 or c.bk) and (not c.ak or (c.K + 512) * c.lda * 2 < (1 << 32))
               and (not c.bk or (c.K + 512) * c.ldb * 2 < (1 << 32)))
    if (splits == 1 and not knobs.no_g256 and g256_ok and not c.ak and (c.N > 128 or knobs.narrow)
            and cdiv(c.M, 256) * cdiv(c.N, 256) >= knobs.min_tiles):
        not_built = cls in (2, 3, 7, 10) if c.bk else cls in (4, 11)
        return NS(kind='g256', cls=0 if not_built else cls, colsum=colsum)
    return NS(kind='g128', splits=splits, colsum=colsum)


def cli_text(r, c):
    """the line tests/gemm_route_cli.cpp prints for this route"""
    plan = lambda p: '%d/%d/%d/%s' % p
    if r.kind == 'skinny':
        t = f'skinny mt={r.mt} ksplit={r.ksplit}'
    elif r.kind == 'dw':
        t = f'dw kc={r.kc} chunks={r.chunks} full={plan(r.full)}' + (f' tail={plan(r.tail)}' if c.K % r.kc else '') + (' error' if r.chunk_error else '')
    elif r.kind == 'gemm3':
        t = f'gemm3 cls={r.cls} overlap={int(r.overlap)}'
    elif r.kind == 'g256':
        t = f'g256 cls={r.cls}'
    else:
        t = f'g128 splits={r.splits}'
    return t if r.kind == 'dw' else t + f' colsum={r.colsum}'


def colsum_paths(N):
    """colsum_kernel's two run-time paths: 16-byte loads where 8 columns fit, element loads for the last N % 8"""
    return (['colsum_kernel/full'] if N >= 8 else []) + (['colsum_kernel/tail'] if N % 8 else [])


def instantiations(r, c):
    """the kernel instantiations a route launches, in launch order"""
    if r.kind == 'dw':
        plans = ([r.full] if r.chunks - (1 if r.tail and r.tail[0] else 0) > 0 else []) + ([r.tail] if r.tail and r.tail[0] else [])
        out = []
        for p in plans:
            out += (colsum_paths(c.M) if p[3] == 'before' else []) + [f'g256dw<epi={p[0]}>']
        return out
    pre = colsum_paths(c.M) if r.colsum == 'before' else []
    if r.kind == 'skinny':
        return pre + [f'skinny<{r.mt}>' + (f' ksplit={r.ksplit}' if r.ksplit > 1 else '')]
    if r.kind == 'gemm3':
        return pre + [f"gemm3<{r.cls},{'overlap' if r.overlap else 'plain'}>"]
    if r.kind == 'g256':
        return pre + [f'g256<bk={int(c.bk)},epi={r.cls}>']
    return pre + [f'g128<ak={int(c.ak)},bk={int(c.bk)},splitk={int(r.splits > 1)}>']


def route(call, knobs, n_cu=N_CU, deterministic=False):
    """the instantiation name(s) of one i2t_gemm_bf16 / i2t_gemm_dw_colsum_bf16 call, ' + ' between launches"""
    return ' + '.join(instantiations(gemm_route(call, knobs, n_cu, deterministic), call))


def ws_splits(M, N, K, act, ws_floats):
    """i2t_gemm_bf16_ws's split rule: K slices of the two-launch form, or 1 = the call falls through to i2t_gemm_bf16"""
    tiles, nk_all, splits = cdiv(M, 128) * cdiv(N, 128), cdiv(K, 64), 1
    while tiles * splits < 256 and nk_all // (splits * 2) >= 4 and splits < 32:
        splits *= 2
    while splits > 1 and splits * M * N > ws_floats:
        splits >>= 1
    return 1 if (M <= 64 or M > 2048 or not ws_floats or act not in (NONE, GELU)) else splits


def effective_cus(n_cu, reserved):
    """csrc/gemm.hip::g256_cus: a reservation that would leave fewer than 9 CUs is ignored"""
    return n_cu - reserved if 0 < reserved < n_cu - 8 else n_cu


def all_routes():
    """every instantiation gemm_bf16_impl, i2t_gemm_bf16_ws and i2t_colsum_bf16_ex can launch, written out from their launch lines
    (launch_g128, launch_g256, launch_g256_dw, launch_g3, launch_skinny); 'skinny ksplit>1' stands for any one K-split skinny launch"""
    r = {f'g128<ak={a},bk={b},splitk={s}>' for a in (0, 1) for b in (0, 1) for s in (0, 1)}
    r |= {f'g256<bk={b},epi={e}>' for b in (0, 1) for e in (0, 1, 5)}
    r |= {f'g256<bk=0,epi={e}>' for e in (2, 3, 7, 10)} | {f'g256<bk=1,epi={e}>' for e in (4, 11)}
    r |= {f'g256dw<epi={e}>' for e in (5, 6, 13)}
    r |= {f'gemm3<{c},{o}>' for c in (1, 2) for o in ('plain', 'overlap')}
    r |= {f'skinny<{m}>' for m in (1, 2, 3, 4)} | {'skinny ksplit>1', 'g128<0,0,1>+reduce', 'colsum_kernel/full', 'colsum_kernel/tail'}
    return r


# ------------------------------------------------------------------------------------------------------------------- cases
BIG = 10 ** 9
_DEF = dict(entry='gemm', ak=0, bk=0, f32=0, acc=0, act=NONE, drop=0, bias=0, auxi=0, auxo=0, res=0, resc=0, alpha=1.0, asq=0, cso=0,
            ldc=None, ldr=None, ldai=None, ldao=None, lda=None, ldb=None, env=None, det=0, reserve=0, misalign=0, ws_short=0, positive=0, kpad=0)
_ENV = dict(min_tiles='I2T_G256_MIN_TILES', gemm3='I2T_GEMM3', ksplit='I2T_SKINNY_KSPLIT', fold='I2T_FOLD_COLSUM', dw_splits='I2T_DW_SPLITS')


def case(name, M, N, K, **kw):
    d = dict(_DEF)
    d.update(kw)
    c = NS(name=name, M=M, N=N, K=K, **d)
    c.env = dict(c.env or {})
    c.ldc = c.ldc or N
    c.ldr, c.ldai, c.ldao = c.ldr or c.ldc, c.ldai or c.ldc, c.ldao or c.ldc
    # kpad: 8 NaN pad columns behind the reduction index of a row-major operand (K % 8 == 0 everywhere: the ABI asks for no zeros)
    c.lda = c.lda or r8(M if c.ak else K) + (0 if c.ak else c.kpad)
    c.ldb = c.ldb or r8(N if c.bk else K) + (0 if c.bk else c.kpad)
    if c.bk and not c.ak and K % 128 and c.lda == r8(K):
        c.lda += 8                                              # zero pad columns, then the next row's head (see ``zero_pad``)
    bits = [f'{k}{getattr(c, k)}' for k in ('ak', 'bk', 'f32', 'acc', 'act', 'drop', 'bias', 'auxi', 'auxo', 'res', 'resc', 'asq', 'cso', 'det',
                                            'reserve', 'misalign', 'kpad') if getattr(c, k)]
    c.id = '-'.join([name, f'{M}x{N}x{K}'] + bits + ([f'alpha{c.alpha}'] if c.alpha != 1 else []) + ([f'ldc{c.ldc}'] if c.ldc != N else []) +
                    [f'{k}{v}' for k, v in sorted(c.env.items()) if v != BIG])
    return c


def zero_pad(c):
    """row-major A on the 256^2 kernel beside a k-major B with K % 128 != 0: the kernel reads A up to the K tile's end and multiplies
    by the zeros the range check returns for B rows >= K, so whatever follows A's K columns must be finite: the pad columns hold
    zero (gemm_route.h: "its zero pads, then the head of the next row") instead of NaN"""
    return bool(c.bk and not c.ak and c.K % 128 and gemm_route(call_of(c), knobs_of(c)).kind == 'g256')


def call_of(c, c16=None, auxo16=True):
    """the GemmCall of a case (c16: 16-byte alignment of C as the test lays it out)"""
    if c16 is None:
        c16 = bool(c.f32 or not c.misalign)
    d = dict(M=c.M, N=c.N, K=c.K, lda=c.lda, ldb=c.ldb, ldc=c.ldc, ak=c.ak, bk=c.bk, f32=c.f32, acc=c.acc, act=c.act, drop=c.drop, bias=c.bias,
             auxi=c.auxi, auxo=c.auxo, res=int(c.res or c.resc), resc=c.resc, ldai=c.ldai, ldao=c.ldao, ldr=c.ldr, alpha1=int(c.alpha == 1.0),
             cso=c.cso, c16=int(c16), auxo16=int(auxo16))
    d['as'] = c.asq
    return NS(**d)


def knobs_of(c):
    k = dict(KNOB_DEFAULTS)
    k.update(c.env)
    return NS(**k)


def cli_line(c):
    call, k = call_of(c), knobs_of(c)
    f = [f'{a}={int(b)}' for a, b in vars(call).items()] + [f'{a}={b}' for a, b in vars(k).items()] + [f'det={c.det}']
    return ' '.join(f)


def env_of(c):
    """the per-call environment switches of a case: {variable: value}"""
    return {_ENV[k]: str(v) for k, v in c.env.items()}


def case_route(c, n_cu=N_CU):
    if c.entry == 'colsum':
        return ' + '.join(colsum_paths(c.N))
    if c.entry == 'ws':
        s = ws_splits(c.M, c.N, c.K, c.act, ws_floats_of(c))
        if s > 1:
            return 'g128<0,0,1>+reduce'
    return route(call_of(c), knobs_of(c), n_cu, bool(c.det))


def ws_floats_of(c):
    full = ws_splits(c.M, c.N, c.K, c.act, 1 << 40)
    return full * c.M * c.N - (1 if c.ws_short else 0)


def _cases():
    out = []
    g256 = lambda name, M, N, K, **kw: out.append(case(name, M, N, K, env=dict(min_tiles=1, **kw.pop('env', {})), **kw))
    g128 = lambda name, M, N, K, **kw: out.append(case(name, M, N, K, env=dict(min_tiles=BIG), **kw))
    Ms, Ns, Ks = [257, 300, 520], [264, 520, 2312], [128, 256, 384]
    sh = lambda i: (Ms[i % 3], Ns[(i + i // 3) % 3], Ks[(i + i // 9) % 3])
    # --- 256^2, B^T form.  class 1: bias, alpha != 1, alpha_sumsq, drop_mode 2 (N % 12 == 0), each present and absent
    for i, kw in enumerate([{}, dict(bias=1), dict(alpha=0.37), dict(asq=1, bias=1), dict(drop=2), dict(drop=2, bias=1, alpha=-2.0)]):
        M, N, K = sh(i)
        g256('c1', M, 264 if kw.get('drop') else N, K, **kw)
    for i, (act, nm) in enumerate([(GELU, 'c2'), (GELU_DOUT, 'c10')]):
        for j, kw in enumerate([dict(bias=1, auxo=1), dict(auxo=1), dict(bias=1), {}]):
            g256(nm, *sh(2 * i + j + 1), act=act, **kw)
    for j, kw in enumerate([dict(bias=1), dict(res=1), dict(drop=1), dict(bias=1, res=1, drop=1), dict(res=1, ldr=2316)]):
        M, N, K = sh(j + 2)
        g256('c3', M, 2312 if kw.get('ldr') else N, K, f32=1, **kw)
    g256('c5', *sh(0), f32=1)
    g256('c5', *sh(4), f32=1, acc=1)
    g256('c7', 257, 1022, 128, ldc=1024)
    g256('c7', 520, 1022, 384, ldc=1024, f32=1)
    # generic class on the 256^2 kernel: residual + accumulate, the erf flavours, GELU_DOUT without aux_out at an odd ld, and every
    # class-k combination at a leading dimension that is no multiple of 4
    g256('c0', *sh(1), f32=1, res=1, acc=1, bias=1)
    g256('c0', *sh(2), act=GELU_ERF, bias=1)
    g256('c0', *sh(3), act=DGELU_ERF, auxi=1)
    g256('c0', 257, 1022, 256, ldc=1022)
    odd = [dict(bias=1, drop=2, N=264), dict(act=GELU, bias=1, auxo=1), dict(f32=1, bias=1, res=1, drop=1), dict(act=DGELU, auxi=1, bk=1),
           dict(f32=1, acc=1), dict(act=GELU_DOUT, bias=1, auxo=1), dict(act=MUL_AUX, auxi=1, bk=1), dict(act=GELU_DOUT, bias=1)]
    for i, kw in enumerate(odd):
        M, N, K = sh(i)
        N = kw.pop('N', N)
        g256('c0odd', M, N, K, ldc=N + 2, **kw)
    # --- 256^2, B form (k-major B): any K, the zero-range path past K
    for i, K in enumerate([128, 256, 384, 72, 200, 1000]):
        M, N, _ = sh(i)
        g256('c4', M, N, K, bk=1, act=DGELU, auxi=1, ldai=N + 8)
        g256('c11', Ms[(i + 1) % 3], N, K, bk=1, act=MUL_AUX, auxi=1, ldai=N + 8)
        kw = [dict(bias=1), dict(f32=1), dict(f32=1, acc=1), dict(act=GELU, bias=1, auxo=1), {}, dict(f32=1, res=1)][i]
        g256('bk', Ms[(i + 2) % 3], N, K, bk=1, **kw)
    # --- one case per class under a CU reservation (12 tiles or more: the persistent loop hands tiles over) and one misaligned
    per_class = [('c1', dict(bias=1)), ('c2', dict(act=GELU, bias=1, auxo=1)), ('c10', dict(act=GELU_DOUT, bias=1, auxo=1)),
                 ('c3', dict(f32=1, bias=1, res=1, drop=1)), ('c5', dict(f32=1, acc=1)), ('c7', dict(N=1022, ldc=1024)), ('c0', dict(f32=1, res=1, acc=1)),
                 ('c4', dict(bk=1, act=DGELU, auxi=1, K=200)), ('c11', dict(bk=1, act=MUL_AUX, auxi=1, K=72)), ('bk5', dict(bk=1, f32=1, acc=1, K=200))]
    for nm, kw in per_class:
        kw = dict(kw)
        N, K = kw.pop('N', 2312), kw.pop('K', 256)
        g256(nm, 520, N, K, reserve=1, **kw)
        g256(nm, 300, N if N == 1022 else 520, K, misalign=1, **kw)
    # --- gemm3 (I2T_GEMM3 = 1 | 2): class 1 from K = 320, class 2 from K = 512
    for mode in (1, 2):
        g256('g3', 300 if mode == 1 else 520, 264 if mode == 1 else 520, 384, bias=1, env=dict(gemm3=mode))
        g256('g3', 520 if mode == 1 else 257, 2312 if mode == 1 else 264, 512, act=GELU, bias=1, auxo=1, env=dict(gemm3=mode))
    # --- dW on the 256^2 kernel (classes 5 / 6 / 13)
    dw = lambda name, M, N, K, **kw: out.append(case(name, M, N, K, entry='dw', ak=1, bk=1, f32=1, acc=1, **kw))
    for i, (M, N) in enumerate([(256, 256), (264, 520), (520, 256)]):
        for j, K in enumerate([1024, 1000, 4099]):
            kw = [dict(), dict(cso=1), dict(cso=1, asq=1, alpha=0.37), dict(cso=1, env=dict(fold=0)), dict(cso=1, det=1), dict(det=1),
                  dict(alpha=-2.0), dict(cso=1, alpha=0.5), dict(asq=1)][3 * i + j]
            dw('dw', M, N, K, **kw)
    dw('dw', 264, 520, 4099, cso=1, env=dict(dw_splits=4))         # 65 K-tiles in slices of 18, 18, 18, 11
    # (K + 512) ld 2 >= 2^32 at ld = 50264: two chunks, 42112 rows and a 101-row tail with its own plan.  Outside deterministic
    # mode the tail has no large-tile form (test_gemm_route_cpu 'dw_later_chunk_error'): the call is refused after the first chunk
    # positive: |N(0, 1)| operands in the first regime, so that condition 2 holds over 660 K steps.  S ~ |ref| ~ 130 then puts the
    # bound near 0.01 against a product of ~0.003: in THIS case a lost product shows in the lattice regime only
    dw('dw2g', 256, 256, 42213, lda=50264, det=1, positive=1)
    # --- 128^2: all four layouts, ragged M / N / K, every epilogue flag of the generic class
    shapes = [(1, 8, None), (65, 72, None), (128, 128, None), (129, 136, None), (200, 130, 130)]
    epi = [dict(bias=1), dict(act=GELU, bias=1, auxo=1), dict(f32=1, res=1, ldr=140), dict(f32=1, acc=1, bias=1), dict(act=DGELU, auxi=1),
           dict(f32=1, drop=1, res=1), dict(act=GELU_DOUT, bias=1), dict(act=GELU_ERF, bias=1), dict(act=MUL_AUX, auxi=1, alpha=0.5),
           dict(alpha=-2.0, bias=1, f32=1), dict(act=DGELU_ERF, auxi=1), dict(act=GELU_DOUT, bias=1, auxo=1), dict(f32=1, res=1, acc=1),
           dict(auxo=1, bias=1), dict(f32=1, asq=1, bias=1)]
    i = 0
    for ak in (0, 1):
        for bk in (0, 1):
            for s, (M, N, ldc) in enumerate(shapes):
                K = [8, 64, 72, 200, 1000][(s + 2 * ak + bk) % 5]
                kw = dict(epi[i % len(epi)])
                if kw.get('ldr') and ldc:
                    kw.pop('ldr')
                if M <= 64 and not ak and not bk:
                    kw = dict(f32=1, acc=1, bias=1)             # (anything the skinny kernel does not take)
                g128('g128', M, N, K, ak=ak, bk=bk, ldc=ldc, kpad=8 * (s % 2), **kw)
                i += 1
            g128('g128sk', 128, 136, 8192, ak=ak, bk=bk, f32=1, acc=1, alpha=1.0 if ak else 0.5)
    g128('g128sk', 128, 136, 8192, ak=1, bk=1, f32=1, acc=1, det=1)
    g128('g128', 129, 136, 200, misalign=1, bias=1, res=1, f32=1)
    g128('g128', 129, 136, 200, misalign=1, act=DGELU, auxi=1)
    # --- skinny (M <= 64, both row-major): K % 64 != 0 runs both half-step guards
    sk = lambda name, M, N, K, **kw: out.append(case(name, M, N, K, **kw))
    sM, sN, sK = [1, 16, 17, 33, 49, 64], [(8, None), (24, None), (72, None), (770, 776)], [8, 40, 64, 136, 3072]
    sepi = [dict(bias=1), dict(act=GELU, bias=1), dict(f32=1, res=1), dict(f32=1, resc=1, bias=1), dict(), dict(res=1, bias=1)]
    for i, M in enumerate(sM):
        for j in range(2):
            N, ldc = sN[(i + 2 * j) % 4]
            sk('skinny', M, N, sK[(i + 3 * j) % 5], ldc=ldc, kpad=8 * j, **sepi[(i + j) % 6])
    for i, M in enumerate([1, 17, 33, 64]):
        N, ldc = sN[(i + 1) % 4]
        for env in ({}, dict(ksplit=1)):
            sk('skinny_inplace', M, N, 3072, ldc=ldc, f32=1, resc=1, bias=i % 2, kpad=8 * (i // 2), env=env)
    sk('skinny', 17, 72, 136, misalign=1, bias=1, res=1, f32=1)
    # --- ws + reduce
    for i, (M, N) in enumerate([(65, 72), (65, 770), (130, 72), (130, 770)]):
        kw = [dict(bias=1), dict(act=GELU, bias=1, f32=1), dict(res=1, f32=1), dict(res=1, bias=1, act=GELU)][i]
        out.append(case('ws', M, N, 3072, entry='ws', **kw))
        out.append(case('ws', M, N, 3072, entry='ws', ws_short=1, **[dict(f32=1), dict(bias=1), dict(bias=1, res=1), dict(f32=1, bias=1)][i]))
    # --- colsum
    for M, N in [(5, 8), (63, 520), (200, 1030)]:
        for kw in (dict(), dict(acc=1), dict(acc=1, asq=1), dict(det=1, acc=1)):
            out.append(case('colsum', M, N, 1, entry='colsum', f32=1, **kw))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()


def table_routes(cases=None, n_cu=N_CU):
    got = set()
    for c in cases or CASES:
        for r in case_route(c, n_cu).split(' + '):
            got.add('skinny ksplit>1' if ' ksplit=' in r else r)
    return got


# ------------------------------------------------------------------------------------------------------------------ inputs
REGIMES = ('normal', 'lattice', 'address')


def _gen(c, salt):
    return torch.Generator().manual_seed(zlib.crc32(repr((c.id, salt)).encode()) % (2 ** 31))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def has_transcendental(c):
    return c.act in (GELU, DGELU, GELU_ERF, DGELU_ERF, GELU_DOUT)


def is_exact(c, regime):
    """lattice and address inputs give a result that is exact in fp32 whatever the order: bit-identity is required, unless the
    epilogue evaluates a transcendental or divides by sqrt(alpha_sumsq) + 1e-6 (then the bound of the normal regime)"""
    return regime != 'normal' and not has_transcendental(c) and not c.asq


def inputs(c, regime='normal'):
    """float64 CPU tensors, logical A [M, K], B [N, K], every value representable in the type the kernel reads it as"""
    g = _gen(c, regime)
    M, N, K = c.M, c.N, c.K
    d = NS(alpha=float(c.alpha), asq=None, drop=None)
    rb = lambda t: bf16_round(t.double())
    r32 = lambda t: t.to(F32).to(F64)
    if c.entry == 'colsum':
        d.A = rb(torch.randn(M, N, generator=g)) if regime == 'normal' else _ints(g, -4, 4, M, N)
        d.C0 = r32(torch.randn(N, generator=g)) if regime == 'normal' else _ints(g, -8, 8, N)
        d.asq = 7.3 if c.asq else None
        return d
    if regime == 'normal':
        d.A = rb(torch.randn(M, K, generator=g))
        d.B = rb(torch.randn(N, K, generator=g) / math.sqrt(K))
        if c.positive:                                        # K = 42213 into fp32: sum |terms| ~ |ref| keeps condition 2
            d.A, d.B = d.A.abs(), d.B.abs()
        d.bias, d.res, d.C0 = r32(0.5 * torch.randn(N, generator=g)), r32(torch.randn(M, N, generator=g)), r32(torch.randn(M, N, generator=g))
        d.auxi = rb(torch.randn(M, N, generator=g))
        d.cs0 = r32(torch.randn(M, generator=g))
        thr = 26                                              # p = 0.1
    else:
        if regime == 'lattice':
            d.A, d.B = _ints(g, -4, 4, M, K), _ints(g, -4, 4, N, K)
            d.bias, d.res = _ints(g, -8, 8, N), _ints(g, -8, 8, M, N)
        else:
            m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
            d.A = (k[None, :] == (m % K)[:, None]).to(F64)
            d.B = (((131 * n[:, None] + 7 * k[None, :]) % 251) - 125).to(F64)
            d.bias = (256 * (n % 3)).to(F64)
            d.res = (512 * (m % 5)).to(F64)[:, None].expand(M, N).contiguous()
        d.C0, d.cs0 = _ints(g, -8, 8, M, N), _ints(g, -8, 8, M)
        d.auxi = _ints(g, -2, 2, M, N) if c.act == MUL_AUX else rb(torch.randn(M, N, generator=g))
        d.alpha = {1.0: 1.0, 0.5: 0.5, -2.0: -2.0}.get(c.alpha, 0.5)
        thr = 128                                             # p = 0.5: scale exactly 2
    if c.asq:
        d.asq = 7.3
    if c.drop:
        from image2text_amd import rng
        thr = rng.threshold(0.5) if regime != 'normal' else thr
        d.drop = (c.drop, 0x1234567 + 77 * M + N, thr, float(torch.tensor(rng.scale(thr), dtype=F32)))
    return d


def drop_multiplier(c, d):
    """[M, N] multipliers (0 or scale) of include/i2t.h's two dropout rules, from image2text_amd.rng"""
    from image2text_amd import rng
    mode, key, thr, scale = d.drop
    M, N = c.M, c.N
    if mode == 1:
        keep = rng.keep_mask(key, M * N, thr).view(M, N)
    else:
        third = torch.arange(N) // (N // 3)
        cols = [rng.keep_mask((key + t) & 0xFFFFFFFF, M, thr) for t in range(int(third.max()) + 1)]
        keep = torch.stack(cols, 1)[:, third]
    return keep.to(F64) * scale


# ----------------------------------------------------------------------------------------------- references with their bounds
def norm_factor(asq):
    """f = 1 / (sqrt(alpha_sumsq) + 1e-6) as eff_alpha evaluates it in fp32 (three roundings: counted in k)"""
    return 1.0 if asq is None else 1.0 / (math.sqrt(asq) + 1e-6)


def fp32_k(c, n_cu=N_CU):
    """(k of the pre-activation, k of the stored value, k of colsum_out): 64-wide K steps on the longest fp32 path + slices / atomic adds /
    planes combined + the epilogue's operations, restated from the route"""
    nk = cdiv(c.K, 64)
    kcs = 0
    if c.entry == 'colsum':
        cb = cdiv(c.N, 512)
        splits = 1 if c.det else max(1, min(cdiv(c.M, 64), 512 // cb))
        return 0, 0, cdiv(cdiv(c.M, splits), 4) + 3 + splits + 1 + c.acc + (3 if c.asq else 0)
    if c.entry == 'ws' and ws_splits(c.M, c.N, c.K, c.act, ws_floats_of(c)) > 1:
        s = ws_splits(c.M, c.N, c.K, c.act, ws_floats_of(c))
        steps, adds = cdiv(nk, s), s
    else:
        r = gemm_route(call_of(c), knobs_of(c), n_cu, bool(c.det))
        if r.kind == 'skinny':
            steps, adds = cdiv(cdiv(nk, r.ksplit), 4), 3 + (r.ksplit if r.ksplit > 1 else 0)
        elif r.kind == 'g128':
            steps, adds = cdiv(nk, r.splits), (r.splits if r.splits > 1 else 0)
        elif r.kind == 'dw':
            plans = [r.full] * (r.chunks - (1 if r.tail and r.tail[0] else 0)) + ([r.tail] if r.tail and r.tail[0] else [])
            steps, adds = max(p[2] for p in plans), sum(p[1] for p in plans)
            rows = min(r.kc, c.K)
            cb = cdiv(c.M, 512)
            cs_splits = 1 if c.det else max(1, min(cdiv(rows, 64), 512 // cb))
            kcs = max(steps + adds, cdiv(cdiv(rows, cs_splits), 4) + 3 + cs_splits * len(plans)) + 2 + (3 if c.asq else 0)
        else:
            steps, adds = (nk + 1) & ~1, 0
        if c.cso and not kcs:
            cb = cdiv(c.M, 512)
            cs_splits = 1 if c.det else max(1, min(cdiv(c.K, 64), 512 // cb))
            kcs = cdiv(cdiv(c.K, cs_splits), 4) + 3 + cs_splits + 2 + (3 if c.asq else 0)
    kv = steps + adds + 1 + (3 if c.asq else 0) + c.bias
    return kv, kv + 1 + (1 if c.drop else 0) + (1 if (c.res or c.resc) else 0) + c.acc, kcs


def _gelu2(v):
    """gelu_tanh''(v) by autograd on the float64 derivative"""
    x = v.clone().requires_grad_(True)
    _gelu_tanh64(x)[1].sum().backward()
    return x.grad.detach()


def _out(ref, S, k, extra, f32):
    bound = (U32 if f32 else E8) * ref.abs() + k * U32 * S + extra
    return NS(ref=ref, S=S, k=k, extra=extra, bound=bound, f32=bool(f32))


def reference(c, d, n_cu=N_CU, acc_of=None):
    """{'C': .., 'aux_out': .., 'colsum': ..} -> NS(ref, S, k, extra, bound, f32); include/i2t.h's epilogue order in float64.
    acc_of(A, B) -> (sum of products, sum of |products|) replaces the exact sums (the emulation of test_gemm_ref_cpu.py)"""
    kv, kc, kcs = fp32_k(c, n_cu)
    f = norm_factor(d.asq)
    res = {}
    if c.entry == 'colsum':
        ref, S = d.A.sum(0) * f, d.A.abs().sum(0) * f
        if c.acc:
            ref, S = ref + d.C0, S + d.C0.abs()
        return {'colsum': _out(ref, S, kcs, 0.0, True)}
    acc, S = acc_of(d.A, d.B) if acc_of else (d.A @ d.B.t(), d.A.abs() @ d.B.abs().t())
    a = d.alpha * f
    v, S = a * acc, abs(a) * S
    if c.bias:
        v, S = v + d.bias[None, :], S + d.bias.abs()[None, :]
    dv = kv * U32 * S                                           # what the fp32 pre-activation may be off by
    extra = torch.zeros_like(v)
    if c.auxo and c.act != GELU_DOUT:
        res['aux_out'] = _out(v, S, kv, 0.0, False)
    if c.act == GELU:
        g, grad, _, rel, _ = _gelu_tanh64(v)
        v, S, extra = g, g.abs(), grad.abs() * dv + rel * g.abs() + TINY * (1 + v.abs())
    elif c.act == GELU_ERF:
        g, grad, _ = _gelu_erf64(v)
        v, S, extra = g, g.abs(), grad.abs() * dv + ERF_PHI_ERR * v.abs()
    elif c.act == GELU_DOUT:
        g, grad, terms, rel, flush = _gelu_tanh64(v)
        if c.auxo:
            res['aux_out'] = _out(grad, terms, 4, _gelu2(v).abs() * dv + rel * terms + flush, False)
        v, S, extra = g, g.abs(), grad.abs() * dv + rel * g.abs() + TINY * (1 + v.abs())
    elif c.act == DGELU:
        _, grad, terms, rel, flush = _gelu_tanh64(d.auxi)
        extra, v, S = v.abs() * (rel * terms + flush), v * grad, S * terms
    elif c.act == DGELU_ERF:
        _, grad, terms = _gelu_erf64(d.auxi)
        # gelu_erf'(x) = Phi + x phi: Phi carries ERF_PHI_ERR; phi = exp(-x^2 / 2) / sqrt(2 pi) in fp32 turns the rounding of its
        # argument (x^2 / 2 ulps) into a relative error, plus a few roundings of the product
        x = d.auxi
        xphi = (x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)).abs()
        extra = v.abs() * (ERF_PHI_ERR + (4 + x * x) * 2.0 ** -24 * xphi + 2.0 ** -23 * terms)
        v, S = v * grad, S * terms
    elif c.act == MUL_AUX:
        v, S = v * d.auxi, S * d.auxi.abs()
    if c.drop:
        mult = drop_multiplier(c, d)
        v, S, extra = v * mult, S * mult, extra * mult
    if c.res or c.resc:
        r_ = d.C0 if c.resc else d.res
        v, S = v + r_, S + r_.abs()
    if c.acc:
        v, S = v + d.C0, S + d.C0.abs()
    res['C'] = _out(v, S, kc, extra, c.f32)
    if c.cso:
        ref, Sc = d.cs0 + f * d.A.sum(1), d.cs0.abs() + f * d.A.abs().sum(1)
        res['colsum'] = _out(ref, Sc, kcs, 0.0, True)
    return res


def condition_ii(r):
    """median(bound) / rms(ref): at most 1/128 (bf16 outputs) or 1/256 (fp32 outputs)"""
    rms = float(r.ref.pow(2).mean().sqrt())
    return float(r.bound.expand_as(r.ref).median()) / max(rms, 1e-300)


def ii_max(r):
    return II_F32 if r.f32 else II_BF16


def kernel_rounded(r):
    """the reference rounded where the kernel rounds its result"""
    return r.ref.to(F32).to(F64) if r.f32 else bf16_round(r.ref)


def assert_exact_inputs(c, res):
    """every partial sum of an exact case stays below 2^24 (S bounds them all) and is an integer multiple of 1/2"""
    for name, r in res.items():
        assert float(r.S.max()) < 2.0 ** 24, (c.id, name)
        assert torch.equal(r.ref * 2, (r.ref * 2).round()), (c.id, name)
