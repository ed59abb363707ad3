"""Tensor-level wrappers over the C ABI: stride marshalling and shape checks only, one function per entry point.

PyTorch supplies device memory and the current HIP stream; every op below launches hand-written gfx950 kernels
through ``libi2t_hip.so`` and raises ``I2TError`` on any failure (no fallback).  A kernel entry point is reached through ``_k`` alone:
``_k.i2t_x(...)`` adds the stream, refuses a pointer operand that is not a device tensor of the dtype ``lib.SIGNATURES`` gives that
position, passes its address, and checks the return code.  A wrapper keeps what the table cannot know: shapes, strides, contiguity,
and the dtype of a ``void*`` operand.
"""
import os
import weakref
from typing import Optional

import torch

from . import lib as _l

BF16 = torch.bfloat16
F32 = torch.float32
NO_CPU_PATH = 'image2text_amd ops need tensors on the MI355X (cuda) device; there is no CPU path'


def _lib():
    return _l.load()


def operand_error(kind, is_cuda, dtype):
    """Why a tensor on that device, of that dtype, may not stand behind a pointer of this kind (lib.POINTER_DTYPE); None: it may."""
    if not is_cuda:
        return NO_CPU_PATH
    want = _l.POINTER_DTYPE[kind]
    if want is not None and dtype != want:
        return f'wants {want}, got {dtype}'
    return None


class _Kernels:
    """The checked callers of the entry points whose first argument is the stream, one per entry point, built from its row of
    lib.SIGNATURES on first use (``load`` gives the library then)."""

    def __init__(self, load):
        self._load = load

    def __getattr__(self, name):            # the first use only: the caller then stands in the instance's __dict__
        if name not in _l.SIGNATURES:
            raise AttributeError(name)
        fn, check, current_stream = getattr(self._load(), name), _l.check, torch.cuda.current_stream
        ptrs = tuple((i, kind, _l.POINTER_DTYPE[kind]) for i, kind in enumerate(_l.SIGNATURES[name][1:]) if issubclass(kind, _l.P))

        def call(*args):
            args = list(args)
            try:
                for i, kind, want in ptrs:
                    t = args[i]
                    if t is not None:
                        if not t.is_cuda or (want is not None and t.dtype is not want):          # operand_error(...) is not None, inlined
                            why = operand_error(kind, t.is_cuda, t.dtype)
                            raise _l.I2TError(why if why is NO_CPU_PATH else f'{name}: argument {i} ({kind.__doc__}) {why}')
                        args[i] = t.data_ptr()
            except AttributeError:
                raise _l.I2TError(f'{name}: argument {i} wants a tensor or None, got {type(t).__name__}') from None
            rc = fn(current_stream().cuda_stream, *args)
            if rc:
                check(rc, name)

        setattr(self, name, call)
        return call


_k = _Kernels(_l.load)


def _drop(drop):
    """drop = None | (mode, key, thr, scale) -> the four trailing dropout arguments of the C ABI."""
    return (0, 0, 0, 1.0) if drop is None else (int(drop[0]), int(drop[1]), int(drop[2]), float(drop[3]))


# ------------------------------------------------------------------------------------------------------------------------------
# I2T_PRECISE=1 -- the opt-in PARITY mode of the teacher-forced forward (never part of a measured step).  Every
# bf16 GEMM operand this module produces from fp32 data (LayerNorm rows, fp32 -> bf16 casts, the parameter shadow, activated GEMM
# outputs) is written as TWO bf16 terms, hi = bf16(x) and lo = bf16(x - hi); ``lo`` rides on the hi tensor object (``_i2t_lo``), so a
# tensor that lost it (a view, an attention output, the conv stack's bf16 patches) simply counts as exact: never wrong, only one
# term short.  gemm() then runs hi.hi + lo.hi + hi.lo through the SAME MFMA kernels (the second and third product through the
# accumulate class) into fp32, and applies bias / GELU / the bf16 rounding of its output afterwards.  Attention keeps bf16 q, k, v, P
# and the conv stack its bf16 operands: the oracle with exactly those two roundings left deviates by 5e-3 on the nano-224 logits
# (tools/diag_precision.py), the shipped one-term pipeline by 1.7e-2.
# ------------------------------------------------------------------------------------------------------------------------------
PRECISE_CALLS = {'gemm': 0, 'products': 0, 'splits': 0}
_SHADOWS = []            # weak references to bf16 parameter shadows that carry a low-order term (engine.ParamArena.refresh_shadow)


def precise() -> bool:
    return os.environ.get('I2T_PRECISE', '0') not in ('', '0')


def split_f32(src: torch.Tensor, hi: torch.Tensor, lo: Optional[torch.Tensor], n: Optional[int] = None, act: int = 0):
    """hi = bf16(f(src)), lo = bf16(f(src) - hi) over the first n elements (include/i2t.h::i2t_split_f32_bf16)"""
    assert hi.dtype == BF16 and (lo is None or lo.dtype == BF16)
    _k.i2t_split_f32_bf16(src, hi, lo, src.numel() if n is None else n, int(act))
    PRECISE_CALLS['splits'] += 1
    return hi


def register_shadow(shadow: torch.Tensor):
    """the bf16 parameter shadow (whose ``_i2t_lo`` a precise cast just wrote): weight VIEWS of it find their low-order term by address"""
    _SHADOWS[:] = [r for r in _SHADOWS if r() is not None and r() is not shadow]
    _SHADOWS.append(weakref.ref(shadow))


def _lo_of(t: torch.Tensor):
    lo = getattr(t, '_i2t_lo', None)
    if lo is not None:
        return lo
    for r in _SHADOWS:
        sh = r()
        if sh is None or getattr(sh, '_i2t_lo', None) is None:
            continue
        off = t.data_ptr() - sh.data_ptr()
        if 0 <= off < 2 * sh.numel():
            return torch.as_strided(sh._i2t_lo, t.size(), t.stride(), off // 2)
    return None


def _gemm_precise(a, b, out, M, N, K, *, a_kmajor, b_kmajor, lda, ldb, ldc, alpha, bias, act, aux_in, aux_out, residual, ldr, accumulate,
                  drop, alpha_sumsq):
    if drop is not None or aux_in is not None or aux_out is not None or alpha_sumsq is not None or act not in (0, ACT_GELU, ACT_GELU_ERF):
        raise _l.I2TError('I2T_PRECISE=1 covers inference forwards only (no dropout, no saved pre-activations, no backward epilogues)')
    direct = out.dtype == F32 and act == 0
    if not direct and (residual is not None or accumulate or not out.is_contiguous() or (ldc is not None and ldc != out.stride(0))):
        raise _l.I2TError('I2T_PRECISE=1: a bf16 / activated GEMM output must be a plain contiguous buffer')
    acc = out if direct else torch.zeros(M, out.shape[-1], dtype=F32, device=out.device)          # (pad columns stay zero)
    kw = dict(a_kmajor=a_kmajor, b_kmajor=b_kmajor, alpha=alpha)
    ldacc = ldc if direct else None
    _gemm(a, b, acc, M, N, K, lda=lda, ldb=ldb, ldc=ldacc, bias=bias, residual=residual, ldr=ldr, accumulate=accumulate, **kw)
    n = 1
    a_lo, b_lo = _lo_of(a), _lo_of(b)
    if a_lo is not None:
        _gemm(a_lo, b, acc, M, N, K, lda=lda, ldb=ldb, ldc=ldacc, accumulate=True, **kw)
        n += 1
    if b_lo is not None:
        _gemm(a, b_lo, acc, M, N, K, lda=lda, ldb=ldb, ldc=ldacc, accumulate=True, **kw)
        n += 1
    PRECISE_CALLS['gemm'] += 1
    PRECISE_CALLS['products'] += n
    if not direct:
        if out.dtype == F32:
            raise _l.I2TError('I2T_PRECISE=1: an activated GEMM writes bf16 operands')
        lo = torch.empty_like(out)
        split_f32(acc, out, lo, act=act)
        out._i2t_lo = lo
    return out


def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, *, a_kmajor=False, b_kmajor=False,
         lda=None, ldb=None, ldc=None, alpha=1.0, bias=None, act=0, aux_in=None, aux_out=None, residual=None,
         ldr=None, accumulate=False, drop=None, workspace=None, alpha_sumsq=None, colsum_out=None):
    """out[M,N] = epilogue(alpha * op(a) . op(b)); see include/i2t.h::i2t_gemm_bf16.  workspace (fp32, decode steps): the
    deterministic split-K form i2t_gemm_bf16_ws when the problem has few tiles and a long K.  alpha_sumsq (1-float device tensor):
    alpha is further divided by sqrt(alpha_sumsq) + 1e-6 on the device (i2t_gemm_bf16_ex: a folded gradient normaliser).
    colsum_out (fp32 [M], the dW form a_kmajor = b_kmajor = accumulate only): the bias gradient beside the weight gradient, see
    ``gemm_dw_colsum``.  Under I2T_PRECISE=1: the three-product form of the parity mode (above)."""
    if colsum_out is not None:
        assert a_kmajor and b_kmajor and accumulate and bias is None and not act and aux_out is None and residual is None and drop is None
        return gemm_dw_colsum(a, b, out, colsum_out, M, N, K, alpha=alpha, alpha_sumsq=alpha_sumsq, lda=lda, ldb=ldb, ldc=ldc)
    if precise():
        return _gemm_precise(a, b, out, M, N, K, a_kmajor=a_kmajor, b_kmajor=b_kmajor, lda=lda, ldb=ldb, ldc=ldc, alpha=alpha, bias=bias,
                             act=act, aux_in=aux_in, aux_out=aux_out, residual=residual, ldr=ldr, accumulate=accumulate, drop=drop,
                             alpha_sumsq=alpha_sumsq)
    return _gemm(a, b, out, M, N, K, a_kmajor=a_kmajor, b_kmajor=b_kmajor, lda=lda, ldb=ldb, ldc=ldc, alpha=alpha, bias=bias, act=act,
                 aux_in=aux_in, aux_out=aux_out, residual=residual, ldr=ldr, accumulate=accumulate, drop=drop, workspace=workspace,
                 alpha_sumsq=alpha_sumsq)


def _gemm(a, b, out, M, N, K, *, a_kmajor=False, b_kmajor=False, lda=None, ldb=None, ldc=None, alpha=1.0, bias=None, act=0, aux_in=None,
          aux_out=None, residual=None, ldr=None, accumulate=False, drop=None, workspace=None, alpha_sumsq=None):
    assert a.dtype == BF16 and b.dtype == BF16 and out.dtype in (BF16, F32)
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    ldc = out.stride(0) if ldc is None else ldc
    if workspace is not None and not (a_kmajor or b_kmajor or accumulate or drop is not None or aux_in is not None
                                      or aux_out is not None or alpha != 1.0 or act not in (0, 1)):
        ldr_ = (residual.stride(0) if residual is not None else 0) if ldr is None else ldr
        _k.i2t_gemm_bf16_ws(a, lda, b, ldb, out, ldc, int(out.dtype == F32), M, N, K, bias, int(act), residual, ldr_, workspace, workspace.numel())
        return out
    ld_ai = aux_in.stride(0) if aux_in is not None else 0
    ld_ao = aux_out.stride(0) if aux_out is not None else 0
    ldr = (residual.stride(0) if residual is not None else 0) if ldr is None else ldr
    if alpha_sumsq is not None:
        _k.i2t_gemm_bf16_ex(a, lda, int(a_kmajor), b, ldb, int(b_kmajor), out, ldc, int(out.dtype == F32), M, N, K, float(alpha), bias, int(act),
                            aux_in, ld_ai, aux_out, ld_ao, residual, ldr, int(accumulate), *_drop(drop), alpha_sumsq)
        return out
    _k.i2t_gemm_bf16(a, lda, int(a_kmajor), b, ldb, int(b_kmajor), out, ldc, int(out.dtype == F32), M, N, K, float(alpha), bias, int(act), aux_in,
                     ld_ai, aux_out, ld_ao, residual, ldr, int(accumulate), *_drop(drop))
    return out


def set_deterministic(on: bool):
    """Fixed-order reductions on the gradient path (include/i2t.h::i2t_set_deterministic): slow, bit-reproducible backward passes."""
    _l.check(_lib().i2t_set_deterministic(int(bool(on))), 'i2t_set_deterministic')


def deterministic() -> bool:
    return bool(_lib().i2t_deterministic())


def gemm_reserve_cus(n: int):
    """Leave n CUs free in later persistent-GEMM launches (0 = use all); see include/i2t.h::i2t_gemm_reserve_cus."""
    _l.check(_lib().i2t_gemm_reserve_cus(int(n)), 'i2t_gemm_reserve_cus')


def gemm_reserved_cus() -> int:
    return int(_lib().i2t_gemm_reserved_cus())


def colsum(x: torch.Tensor, out: torch.Tensor, M: int, N: int, ld=None, accumulate=False, alpha_sumsq=None):
    _k.i2t_colsum_bf16_ex(x, x.stride(0) if ld is None else ld, M, N, out, int(accumulate), alpha_sumsq)
    return out


def gemm_dw_colsum(dy: torch.Tensor, x: torch.Tensor, gw: torch.Tensor, gb, N: int, K: int, M: int, *, alpha=1.0, alpha_sumsq=None,
                   lda=None, ldb=None, ldc=None):
    """gw[N, K] += alpha f dy^T . x and gb[N] += f sum_rows(dy) (f: the folded gradient normaliser of ``gemm`` / ``colsum``) for dy bf16
    [M, N], x bf16 [M, K]: a linear layer's weight and bias gradients from one read of dy (include/i2t.h::i2t_gemm_dw_colsum_bf16;
    I2T_FOLD_COLSUM=0: the two launches it replaces).  gb None: the GEMM alone.  Under I2T_PRECISE=1: the separate calls."""
    if precise():
        if gb is not None:
            colsum(dy, gb, M, N, ld=lda, accumulate=True, alpha_sumsq=alpha_sumsq)
        return gemm(dy, x, gw, N, K, M, a_kmajor=True, b_kmajor=True, lda=lda, ldb=ldb, ldc=ldc, alpha=alpha, accumulate=True, alpha_sumsq=alpha_sumsq)
    assert dy.dtype == BF16 and x.dtype == BF16
    _k.i2t_gemm_dw_colsum_bf16(dy, dy.stride(0) if lda is None else lda, x, x.stride(0) if ldb is None else ldb, gw,
                               gw.stride(0) if ldc is None else ldc, N, K, M, float(alpha), alpha_sumsq, gb)
    return gw


def layernorm_fwd(x, gamma, beta, y, mean, rstd, M, d, eps=None):
    """eps None: the reference's LayerNorm (1e-5); torchvision's ViT blocks pass 1e-6."""
    if y.dtype == BF16 and precise():          # parity mode: the row in fp32, then its two bf16 terms
        y32 = torch.empty(y.shape, dtype=F32, device=y.device)
        layernorm_fwd(x, gamma, beta, y32, mean, rstd, M, d, eps)
        y._i2t_lo = torch.empty_like(y)
        return split_f32(y32, y, y._i2t_lo)
    if eps is not None:
        _k.i2t_layernorm_fwd_eps(x, gamma, beta, y, int(y.dtype == F32), mean, rstd, M, d, float(eps))
        return y
    _k.i2t_layernorm_fwd(x, gamma, beta, y, int(y.dtype == F32), mean, rstd, M, d)
    return y


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, M, d, dx_accumulate=False, dx_bf16=None, bf16_drop=None,
                  sumsq_out=None, dx_pre_sumsq=None, dx_mask=None, acc_period=0, acc_rows=0):
    """bf16_drop = (1, key, thr, scale): elementwise dropout mask applied to the bf16 copy only; dx_mask = (1, key, thr, scale): the
    same kind of mask on the f32 dx this call stores; acc_period / acc_rows: accumulate onto the first acc_rows rows of every period only
    (see include/i2t.h::i2t_layernorm_bwd_ex)."""
    assert (bf16_drop is None or int(bf16_drop[0]) == 1) and (dx_mask is None or int(dx_mask[0]) == 1)
    _k.i2t_layernorm_bwd_ex(dy, int(dy.dtype == F32), x, gamma, mean, rstd, dx, int(dx_accumulate), dx_bf16, dgamma, dbeta, M, d,
                            *_drop(bf16_drop)[1:], sumsq_out, dx_pre_sumsq, *_drop(dx_mask)[1:], int(acc_period), int(acc_rows))
    return dx


LNND_STATS_STRIDE = 34


def layernorm_nd_fwd(x, add, gamma, beta, y, y_batch_stride, stats, B, rows, d, drop=None, drop_base=0):
    """drop = (1, key, thr, scale) + drop_base: the elementwise dropout of the tensor y is a slab of, applied while writing
    (include/i2t.h::i2t_layernorm_nd_fwd_drop)"""
    assert drop is None or int(drop[0]) == 1
    _k.i2t_layernorm_nd_fwd_drop(x, add, gamma, beta, y, y_batch_stride, stats, B, rows, d, *_drop(drop)[1:], int(drop_base))
    return y


def layernorm_nd_bwd(dy, dy_batch_stride, x, add, gamma, stats, dx, dgamma, dbeta, dadd, B, rows, d):
    _k.i2t_layernorm_nd_bwd(dy, dy_batch_stride, x, add, gamma, stats, dx, dgamma, dbeta, dadd, B, rows, d)
    return dx


def _bs_rs(t: torch.Tensor):
    """(batch stride, row stride) in elements of a [B, T, *] view whose last dim is contiguous; a packed [rows, *] view
    has no batch stride (0)."""
    assert t.stride(-1) == 1
    return (0, t.stride(0)) if t.dim() == 2 else (t.stride(0), t.stride(1))


def attention_fwd(q, k, v, o, lse, B, H, Tq, Tk, causal, drop=None, cu_q=None, cu_k=None, total_q=0):
    """q,k,v,o: bf16 [B, T, >=64H] views (last dim contiguous; heads at 64-column steps), or packed [rows, >=64H] views
    together with cu_q / cu_k (device int32 [B+1])."""
    qb, qr = _bs_rs(q); kb, kr = _bs_rs(k); vb, vr = _bs_rs(v); ob, orr = _bs_rs(o)
    _k.i2t_attention_fwd(q, qb, qr, k, kb, kr, v, vb, vr, o, ob, orr, lse, B, H, Tq, Tk, int(causal), *_drop(drop)[1:], cu_q, cu_k, int(total_q))
    return o


def attention_bwd(q, k, v, o, do, lse, delta_ws, dq, dk, dv, B, H, Tq, Tk, causal, drop=None, cu_q=None, cu_k=None, total_q=0,
                  out_drop=None, out_drop_q_seq=0):
    """out_drop = (2, key, thr, scale): the forward's per-token q/k/v multipliers applied to dq/dk/dv on the way out;
    out_drop_q_seq: the queries are the first Tq rows of sequences of that many rows (i2t_attention_bwd_ex)."""
    qb, qr = _bs_rs(q); kb, kr = _bs_rs(k); vb, vr = _bs_rs(v); ob, orr = _bs_rs(o); gb, gr = _bs_rs(do)
    dqb, dqr = _bs_rs(dq); dkb, dkr = _bs_rs(dk); dvb, dvr = _bs_rs(dv)
    _k.i2t_attention_bwd_ex(q, qb, qr, k, kb, kr, v, vb, vr, o, ob, orr, do, gb, gr, lse, delta_ws, dq, dqb, dqr, dk, dkb, dkr, dv, dvb, dvr, B, H,
                            Tq, Tk, int(causal), *_drop(drop)[1:], cu_q, cu_k, int(total_q), *_drop(out_drop)[1:], int(out_drop_q_seq))


def attention_bwd_takes_q_seq(Tq: int, Tk: int, drop) -> bool:
    """whether a dense, non-causal attention_bwd of these sizes runs on the one-pass resident-operand kernel, the only one that takes
    out_drop_q_seq: csrc/attention_route.h::attn_bwd_route says attn_bwd3_kernel (tests/test_attention_route_cpu.py holds the two
    together over every size up to 320 and every switch; the C side refuses loudly otherwise)"""
    if os.environ.get('I2T_ATTN_V2', '1')[:1] == '0' or os.environ.get('I2T_ATTN_BWD2', '1')[:1] == '0' or os.environ.get('I2T_ATTN_BWD', '3') != '3':
        return False
    return 64 <= Tq <= 288 and Tk <= 288 and (drop is None or Tk % 4 == 0)


def conv_stack_takes_mfma(chans, k: int) -> bool:
    """whether the engine runs a ConvMLP stack of these channel widths (image, gates ..., output) on the 6x6 MFMA entry points: the
    kernel is 6x6, every intermediate width is 8 / 16 / 32 channels, the image has at most 8, the output at most 32 and every layer's
    input at most 16.  csrc/conv_route.h accepts every call encode / encode_backward then make (tests/test_conv_route_cpu.py holds
    the two together); any other stack takes the generic conv_* path."""
    return (k == 6 and all(c in (8, 16, 32) for c in chans[1:-1]) and chans[0] <= 8 and chans[-1] <= 32
            and all(c <= 16 for c in chans[:-1]))


def gq_attention_fwd(q, k, v, o, lse, B, H, Hkv, hd, Tq, Tk, causal, drop=None, cu_q=None, cu_k=None, total_q=0, split=0):
    """Grouped-query attention (include/i2t.h::i2t_gq_attention_fwd): H query heads of width hd on Hkv shared key/value heads."""
    qb, qr = _bs_rs(q); kb, kr = _bs_rs(k); vb, vr = _bs_rs(v); ob, orr = _bs_rs(o)
    _k.i2t_gq_attention_fwd(q, qb, qr, k, kb, kr, v, vb, vr, o, ob, orr, lse, B, H, Hkv, hd, Tq, Tk, int(causal), *_drop(drop)[1:], cu_q, cu_k,
                            int(total_q), int(split))
    return o


def gq_attention_bwd(q, k, v, o, do, lse, delta_ws, dq, dk, dv, B, H, Hkv, hd, Tq, Tk, causal, drop=None, cu_q=None, cu_k=None,
                     total_q=0, out_drop=None):
    qb, qr = _bs_rs(q); kb, kr = _bs_rs(k); vb, vr = _bs_rs(v); ob, orr = _bs_rs(o); gb, gr = _bs_rs(do)
    dqb, dqr = _bs_rs(dq); dkb, dkr = _bs_rs(dk); dvb, dvr = _bs_rs(dv)
    _k.i2t_gq_attention_bwd(q, qb, qr, k, kb, kr, v, vb, vr, o, ob, orr, do, gb, gr, lse, delta_ws, dq, dqb, dqr, dk, dkb, dkr, dv, dvb, dvr, B, H,
                            Hkv, hd, Tq, Tk, int(causal), *_drop(drop)[1:], cu_q, cu_k, int(total_q), *_drop(out_drop)[1:])


def row_sections_dropout(x, rows, cols, section, drop, key_offset=0):
    """drop = (2, key, thr, scale): x[m, n] *= multiplier(key + key_offset + n // section, m)  (bf16 [rows, ld], in place)."""
    if drop is None:
        return x
    assert x.dtype == BF16 and x.stride(-1) == 1
    _k.i2t_row_sections_dropout(x, x.stride(-2), rows, cols, section, (int(drop[1]) + key_offset) & 0xFFFFFFFF, int(drop[2]), float(drop[3]))
    return x


def gather_rows(src, idx, n, d, out_f32=None, out_bf16=None):
    _k.i2t_gather_rows(src, idx, out_f32, out_bf16, n, d)


def scatter_rows(src, idx, dst, n, d):
    _k.i2t_scatter_rows(src, idx, dst, n, d)


def moe_gate_fwd(U, wg2, bg2, A, gates, wsel, M, E, P, G, top_k, inv_sqrt_in):
    assert A.dtype == BF16
    _k.i2t_moe_gate_fwd(U, U.stride(0), wg2, bg2, A, A.stride(0), gates, wsel, M, E, P, G, top_k, float(inv_sqrt_in))


def moe_gate_bwd_blocks(M: int) -> int:
    return _lib().i2t_moe_gate_bwd_blocks(M)


def moe_gate_bwd(dA, U, gates, wsel, wg2, D1, dwg2, dbg2, part_ws, M, E, P, G, top_k, inv_sqrt_in):
    assert dA.dtype == BF16 and D1.dtype == BF16
    _k.i2t_moe_gate_bwd(dA, dA.stride(0), U, U.stride(0), gates, wsel, wg2, D1, D1.stride(0), dwg2, dbg2, part_ws, M, E, P, G, top_k,
                        float(inv_sqrt_in))


def moe_pack_w2(l2w, l2b, W, out, E, P):
    assert l2w.dtype == BF16 and W.dtype == BF16
    _k.i2t_moe_pack_w2(l2w, l2b, W, out, E, P, W.stride(0))


def moe_unpack_dw2(dW, gw, gb, out, E, P):
    _k.i2t_moe_unpack_dw2(dW, gw, gb, out, E, P, dW.stride(0))


def gq_decode_attention(q, k_new, v_new, kcache, vcache, cache_bs, cache_rs, out, pos_ptr, n_keys_fixed, max_keys, B, H, Hkv, hd):
    """Decode-step attention of the family (include/i2t.h::i2t_gq_decode_attention); q / k_new / v_new / out are row-major 2-D views."""
    kv_rs = k_new.stride(0) if k_new is not None else 0
    _k.i2t_gq_decode_attention(q, q.stride(0), k_new, v_new, kv_rs, kcache, vcache, cache_bs, cache_rs, out, out.stride(0), pos_ptr, n_keys_fixed,
                               max_keys, B, H, Hkv, hd)
    return out


def beam_decode_attention(q, q_rs, kcache, vcache, cache_bs, cache_rs, o, o_rs, pos, n_keys_fixed, R, H, hist=None, rows_per_mem=1,
                          append_dm=0, cache_hs=64):
    """decode_attention with key t of row r read from cache row hist[r][t] (hist None: row r // rows_per_mem) -- include/i2t.h::
    i2t_beam_decode_attention"""
    assert hist is None or hist.stride(1) == 1
    _k.i2t_beam_decode_attention(q, q_rs, kcache, vcache, cache_bs, cache_rs, cache_hs, o, o_rs, pos, n_keys_fixed, append_dm, hist,
                                 0 if hist is None else hist.stride(0), rows_per_mem, R, H)


def beam_gq_decode_attention(q, k_new, v_new, kcache, vcache, cache_bs, cache_rs, out, pos_ptr, n_keys_fixed, max_keys, R, H, Hkv, hd,
                             hist=None, rows_per_mem=1, slot_pos=None):
    """gq_decode_attention with the same history indirection (include/i2t.h::i2t_beam_gq_decode_attention); slot_pos (int32
    [max_keys], sparse layers): key s of row r is read from cache row hist[r][slot_pos[s]]"""
    assert hist is None or hist.stride(1) == 1
    assert slot_pos is None or (hist is not None and slot_pos.is_contiguous() and slot_pos.numel() >= max_keys)
    kv_rs = k_new.stride(0) if k_new is not None else 0
    _k.i2t_beam_gq_decode_attention(q, q.stride(0), k_new, v_new, kv_rs, kcache, vcache, cache_bs, cache_rs, out, out.stride(0), pos_ptr,
                                    n_keys_fixed, max_keys, hist, 0 if hist is None else hist.stride(0), slot_pos, rows_per_mem, R, H, Hkv, hd)
    return out


def _mem_index(mem_index, R):
    """the row -> memory-row table of the two calls below: int32 [>= R], contiguous.  Its VALUES are the caller's to check against
    n_mem before the upload (caption_plan.check_image_index): the kernels do not scan them."""
    assert mem_index is None or (mem_index.dim() == 1 and mem_index.is_contiguous() and mem_index.numel() >= R), \
        f'mem_index: one contiguous int32 word per row ({R} rows)'
    return mem_index


def mem_decode_attention(q, q_rs, kmem, vmem, mem_bs, mem_rs, o, o_rs, n_keys, mem_index, n_mem, R, H):
    """Cross-attention of R rows over a memory stored once per image: row r attends to the n_keys keys of memory row mem_index[r], heads
    of 64 in decode_attention's token-major layout (include/i2t.h::i2t_mem_decode_attention)."""
    _k.i2t_mem_decode_attention(q, q_rs, kmem, vmem, mem_bs, mem_rs, o, o_rs, n_keys, _mem_index(mem_index, R), n_mem, R, H)


def mem_gq_decode_attention(q, kmem, vmem, mem_bs, mem_rs, out, n_keys, mem_index, n_mem, R, H, Hkv, hd):
    """mem_decode_attention for Hkv key/value heads of width hd under H query heads (include/i2t.h::i2t_mem_gq_decode_attention); q /
    out are row-major 2-D views."""
    _k.i2t_mem_gq_decode_attention(q, 0 if q is None else q.stride(0), kmem, vmem, mem_bs, mem_rs, out, 0 if out is None else out.stride(0), n_keys,
                                   _mem_index(mem_index, R), n_mem, R, H, Hkv, hd)
    return out


# the host's copy of csrc/common.h::LONG_CHUNK_KEYS, the keys per wave of the split-key decode attention
# (tests/test_long_decode_host_cpu.py reads the header against it)
LONG_CHUNK_KEYS = 256


def gq_decode_long_workspace_floats(R: int, H: int, max_keys: int, hd: int) -> int:
    """fp32 elements of the workspace of gq_decode_attention_long / beam_gq_decode_attention_long over R rows, H query heads of width hd
    and caches of max_keys slots: R * H * NC * (hd + 2), NC = ceil(max_keys / LONG_CHUNK_KEYS) -- per (row, head, chunk) the
    unnormalised sum [hd], then the chunk's maximum and sum of exponentials (include/i2t.h::i2t_gq_decode_attention_long)."""
    return R * H * (-(-max_keys // LONG_CHUNK_KEYS)) * (hd + 2)


def gq_decode_attention_long(q, k_new, v_new, kcache, vcache, cache_bs, cache_rs, out, pos_ptr, n_keys_fixed, max_keys, B, H, Hkv, hd, ws):
    """gq_decode_attention over caches past 1024 keys, the keys split across workgroups (include/i2t.h::i2t_gq_decode_attention_long);
    ws: fp32, at least gq_decode_long_workspace_floats(B, H, max_keys, hd) elements."""
    assert ws.is_contiguous()
    kv_rs = k_new.stride(0) if k_new is not None else 0
    _k.i2t_gq_decode_attention_long(q, q.stride(0), k_new, v_new, kv_rs, kcache, vcache, cache_bs, cache_rs, out, out.stride(0), pos_ptr,
                                    n_keys_fixed, max_keys, B, H, Hkv, hd, ws, ws.numel())
    return out


def beam_gq_decode_attention_long(q, k_new, v_new, kcache, vcache, cache_bs, cache_rs, out, pos_ptr, n_keys_fixed, max_keys, R, H, Hkv, hd,
                                  ws, hist):
    """gq_decode_attention_long with key t of row r read from cache row hist[r][t] (int32 [R][>= max_keys];
    include/i2t.h::i2t_beam_gq_decode_attention_long)"""
    assert ws.is_contiguous() and hist.stride(1) == 1
    kv_rs = k_new.stride(0) if k_new is not None else 0
    _k.i2t_beam_gq_decode_attention_long(q, q.stride(0), k_new, v_new, kv_rs, kcache, vcache, cache_bs, cache_rs, out, out.stride(0), pos_ptr,
                                         n_keys_fixed, max_keys, hist, hist.stride(0), R, H, Hkv, hd, ws, ws.numel())
    return out


def beam_candidates(logits, ids, len_ptr, ctrl, ngram_sizes, R, V, E, temperature, top_k, eos, log_boost, seed, cand_tok, cand_lp,
                    raw_tok=None):
    """E candidates per beam row after ban / crop / EOS rule (include/i2t.h::i2t_beam_candidates); top_k None/0 = no crop, eos None/-1
    = no EOS rule"""
    _k.i2t_beam_candidates(logits, logits.stride(0), ids, ids.stride(0), len_ptr, ctrl, ngram_sizes,
                           0 if ngram_sizes is None else ngram_sizes.numel(), R, V, E, float(temperature), int(top_k or 0),
                           -1 if eos is None else int(eos), float(log_boost), seed, cand_tok, cand_lp, raw_tok)


def beam_consolidate(cand_tok, cand_lp, scores, ids, hist, has_eos, parent, pos_ptr, len_ptr, ctrl, B, W, E, temperature, eos, seed,
                     raw_pick=None):
    """W survivors per caption, ids / history rows moved to the children (include/i2t.h::i2t_beam_consolidate)"""
    _k.i2t_beam_consolidate(cand_tok, cand_lp, scores, ids, ids.stride(0), hist, hist.stride(0), has_eos, parent, pos_ptr, len_ptr, ctrl, B, W, E,
                            float(temperature), -1 if eos is None else int(eos), seed, raw_pick)


def beam_pool_select(cand_tok, cand_lp, scores, ids, hist, tok_lp, pool_ids, pool_lp, pool_score, pool_sum, pool_len, pool_n, closed, pos_ptr,
                     len_ptr, ctrl, B, W, P, max_new, eos, pad, length_penalty, early_stopping):
    """the selection step of generate_captions(num_beams = W): finished pool, running children, close test
    (include/i2t.h::i2t_beam_pool_select); pool_ids [B, W, ids_ld] and pool_lp [B, W, lp_ld] share the row strides of ids and tok_lp"""
    assert cand_tok.shape == (B * W, 2 * W) and cand_lp.shape == (B * W, 2 * W) and cand_tok.is_contiguous() and cand_lp.is_contiguous()
    assert pool_ids.is_contiguous() and pool_lp.is_contiguous() and pool_ids.shape == (B, W, ids.stride(0)) and pool_lp.shape == (B, W, tok_lp.stride(0))
    assert ids.shape[0] == B * W and hist.shape[0] == B * W and tok_lp.shape[0] == B * W and scores.numel() == B * W
    assert pool_score.numel() == B * W and pool_sum.numel() == B * W and pool_len.numel() == B * W and pool_n.numel() == B and closed.numel() == B
    _k.i2t_beam_pool_select(cand_tok, cand_lp, scores, ids, ids.stride(0), hist, hist.stride(0), tok_lp, tok_lp.stride(0), pool_ids, pool_lp,
                            pool_score, pool_sum, pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, B, W, P, max_new, -1 if eos is None else int(eos),
                            int(pad), float(length_penalty), int(bool(early_stopping)))


def beam_advance(counters, ctrl):
    _k.i2t_beam_advance(counters, ctrl)


def sparse_step_setup(pos_ptr, rank, member, lpos, lmem, L, tmax):
    _k.i2t_sparse_step_setup(pos_ptr, rank, member, lpos, lmem, L, tmax)


def select_rows(flag, a, b, out, n):
    _k.i2t_select_rows(flag, a, b, out, n)


def grouped_gemm(mode, a, b, c, N, K, *, b_group_stride=0, c_group_stride=0, bias=None, bias_group_stride=0, act=0, aux_in=None,
                 aux_out=None, residual=None, accumulate=False, seg=None, n_groups=1, max_rows=0, group_ptr=None, group0=0):
    """One GEMM per group (position) in one launch; see include/i2t.h::i2t_grouped_gemm for the three modes."""
    assert a.dtype == BF16 and b.dtype == BF16 and c.dtype in (BF16, F32)
    aux = aux_in if aux_in is not None else aux_out
    _k.i2t_grouped_gemm(mode, a, a.stride(0), b, b.stride(0), b_group_stride, c, c.stride(0), c_group_stride, int(c.dtype == F32), bias,
                        bias_group_stride, int(act), aux_in, aux_out, aux.stride(0) if aux is not None else 0, residual,
                        residual.stride(0) if residual is not None else 0, int(accumulate), seg, n_groups, max_rows, group_ptr, group0, N, K)
    return c


def grouped_colsum(x, seg, n_groups, out, out_group_stride, group0, N):
    _k.i2t_grouped_colsum(x, x.stride(0), seg, n_groups, out, out_group_stride, group0, N)


def xattn_kv_fused(mem, w_kv, bias_kv, q, kv, o, lse, B, S, H, Tq, drop=None, cu_q=None, total_q=0):
    """Fused cross-attention forward (include/i2t.h::i2t_xattn_kv_fused): kv = mem . w_kv^T + bias written once, attention of every
    (image, head) out of the projection's accumulators.  q / o: [B, Tq, >= 64 H] views or packed [rows, >= 64 H] with cu_q.
    S (memory tokens per image) is 64, or 8 / 16 / 32 (64 / S whole images per wave); H even; any other S raises I2TError."""
    qb, qr = _bs_rs(q); ob, orr = _bs_rs(o)
    assert mem.dtype == BF16 and w_kv.dtype == BF16 and q.dtype == BF16 and kv.dtype == BF16 and o.dtype == BF16
    _k.i2t_xattn_kv_fused(mem, mem.stride(0), w_kv, w_kv.stride(0), bias_kv, q, qb, qr, cu_q, int(total_q), kv, kv.stride(-2), o, ob, orr, lse, B, S,
                          H, Tq, *_drop(drop)[1:])
    return o


def embed_fwd(ids, wte, wpe, x, B, T, d, pos_offset, vocab, pos=None):
    _k.i2t_embed_fwd(ids, wte, wpe, x, B, T, d, pos_offset, vocab, pos)
    return x


def embed_bwd(ids, dx, dwte, dwpe, B, T, d, pos_offset, vocab, pos=None):
    _k.i2t_embed_bwd(ids, dx, dwte, dwpe, B, T, d, pos_offset, vocab, pos)


def ce_fwd(logits, ld, labels, w, inv_temp, ignore_index, lse, loss, M, V):
    _k.i2t_ce_fwd(logits, ld, labels, w, float(inv_temp), int(ignore_index), lse, loss, M, V)


def ce_bwd(logits, ld, labels, w, inv_temp, ignore_index, lse, gscale, M, V):
    _k.i2t_ce_bwd(logits, ld, labels, w, float(inv_temp), int(ignore_index), lse, gscale, M, V)


def ce_fwd_bwd(logits, ld, labels, w, inv_temp, ignore_index, lse, loss, M, V):
    """One pass: lse / loss as ce_fwd, and the rows overwritten with the un-scaled gradient (include/i2t.h::i2t_ce_fwd_bwd)."""
    _k.i2t_ce_fwd_bwd(logits, ld, labels, w, float(inv_temp), int(ignore_index), lse, loss, M, V)


CE_ONE_PASS_MAX_V = 8 * 16 * 512


def scale_bf16(x, n, scale):
    """x[0 .. n) *= scale[0] in place (bf16 x, device scalar); a no-op launch when the scale is exactly 1."""
    assert x.dtype == BF16
    _k.i2t_scale_bf16(x, int(n), scale)


def ce_distill_fwd(logits, ld, teacher, ld_t, alpha, labels, w, inv_temp, ignore_index, lse, lse_t, loss, M, V):
    _k.i2t_ce_distill_fwd(logits, ld, teacher, ld_t, float(alpha), labels, w, float(inv_temp), int(ignore_index), lse, lse_t, loss, M, V)


def ce_distill_bwd(logits, ld, teacher, ld_t, alpha, labels, w, inv_temp, ignore_index, lse, lse_t, gscale, M, V):
    _k.i2t_ce_distill_bwd(logits, ld, teacher, ld_t, float(alpha), labels, w, float(inv_temp), int(ignore_index), lse, lse_t, gscale, M, V)


def ema_update(pm, p, pm_bf16, n, momentum):
    _k.i2t_ema_update(pm, p, pm_bf16, int(n), float(momentum))


def lm_inputs(labels, ids, B, L, bos, eos, mask_id, vocab, ignore_index, mask_fraction=0.0, random_fraction=0.0, seed=0):
    """ids = [BOS, labels[:-1]] with ignored labels -> EOS and the optional MLM corruption (include/i2t.h::i2t_lm_inputs)."""
    assert labels.is_contiguous() and ids.is_contiguous()
    _k.i2t_lm_inputs(labels, ids, B, L, int(bos), int(eos), int(-1 if mask_id is None else mask_id), int(vocab), int(ignore_index),
                     float(mask_fraction), float(random_fraction), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return ids


def grad_normalize(g: torch.Tensor, ws: torch.Tensor, g_bf16=None, bf16_drop=None, presummed=False, clear_after=None,
                   keep_f32=False):
    """presummed: ws already holds sum(g^2) (layernorm_bwd's sumsq_out); clear_after: 1-float tensor zeroed afterwards;
    keep_f32: g stays un-normalised, only the bf16 copy is written (the first layernorm_bwd onto g passes dx_pre_sumsq=ws)."""
    assert bf16_drop is None or int(bf16_drop[0]) == 1
    _k.i2t_grad_normalize(g, g.numel(), ws, g_bf16, *_drop(bf16_drop)[1:], int(bool(presummed)) | (2 if keep_f32 else 0), clear_after)
    return g


def rmsnorm_fwd(x, w, y, rstd, M, d, eps, y_f32=None):
    _k.i2t_rmsnorm_fwd(x, w, y, y_f32, rstd, M, d, float(eps))
    return y


def rmsnorm_bwd(dy, x, w, rstd, dx, dw, M, d, dx_accumulate=False, dx_bf16=None):
    _k.i2t_rmsnorm_bwd(dy, int(dy.dtype == F32), x, w, rstd, dx, int(dx_accumulate), dx_bf16, dw, M, d)
    return dx


def rope(x, rs, col0, n_heads, hd, cos_sin, M, pos=None, pos_ptr=None, pos_offset=0, T=0, inverse=False):
    """in place on bf16 rows (include/i2t.h::i2t_rope)"""
    _k.i2t_rope(x, rs, col0, n_heads, hd, cos_sin, cos_sin.shape[0], pos, pos_ptr, pos_offset, T, M, int(inverse))
    return x


def swiglu_fwd(gate_up, h, M, ff):
    _k.i2t_swiglu_fwd(gate_up, gate_up.stride(0), h, M, ff)
    return h


def swiglu_bwd(dh, gate_up, d_gate_up, M, ff):
    _k.i2t_swiglu_bwd(dh, gate_up, gate_up.stride(0), d_gate_up, M, ff)
    return d_gate_up


def dgelu_mul(dh, pre, out, erf=False):
    """out (bf16) = dh (fp32) * gelu'(pre (bf16)), contiguous; tanh form (include/i2t.h::i2t_dgelu_mul) or exact (i2t_dgelu_erf_mul)"""
    assert pre.dtype == BF16 and out.dtype == BF16 and dh.is_contiguous() and pre.is_contiguous() and out.is_contiguous()
    if erf:
        _k.i2t_dgelu_erf_mul(dh, pre, out, dh.numel())
    else:
        _k.i2t_dgelu_mul(dh, pre, out, dh.numel())
    return out


def gelu_fwd(pre, out, erf=False):
    """out (bf16) = gelu(pre (bf16)), contiguous (include/i2t.h::i2t_gelu_fwd)"""
    assert pre.dtype == BF16 and out.dtype == BF16 and pre.is_contiguous() and out.is_contiguous()
    _k.i2t_gelu_fwd(pre, out, pre.numel(), int(bool(erf)))
    return out


def lora_stage(x, xcat, xd, M, K, drop):
    """xcat[:, :K] = x and (xd not None) xd = dropout(x): include/i2t.h::i2t_lora_stage; drop = (1, key, thr, scale) | None"""
    assert x.is_contiguous() and (drop is None) == (xd is None) and (drop is None or int(drop[0]) == 1)
    _k.i2t_lora_stage(x, xcat, xcat.stride(0), xd, M, K, *_drop(drop)[1:])


def sumsq(g: torch.Tensor, ws: torch.Tensor, accumulate=False):
    """ws[0] (+)= sum(g^2)  (include/i2t.h::i2t_sumsq)"""
    _k.i2t_sumsq(g, g.numel(), ws, int(accumulate))
    return ws


def conv_fwd(x, in_gelu, w, bias, y, w_ws, B, Cin, Cout, H, W, k):
    _k.i2t_conv_fwd(x, int(x.dtype == F32), int(in_gelu), w, bias, y, w_ws, B, Cin, Cout, H, W, k)
    return y


def conv_bwd_data(dy, w, x_pre, in_gelu, dx, w_ws, B, Cin, Cout, H, W, k):
    _k.i2t_conv_bwd_data(dy, w, x_pre, int(in_gelu), dx, w_ws, B, Cin, Cout, H, W, k)
    return dx


def conv_bwd_weight(dy, x, in_gelu, dw, db, B, Cin, Cout, H, W, k):
    _k.i2t_conv_bwd_weight(dy, x, int(x.dtype == F32), int(in_gelu), dw, db, B, Cin, Cout, H, W, k)


LAYOUT_NCHW_F32, LAYOUT_NCHW_BF16, LAYOUT_NHWC_BF16 = 0, 1, 2
# The workspaces of the conv6_* calls, at the largest instantiation (csrc/conv_route.h: ws_elems, scratch_bytes; held to it by
# tests/test_conv_route_cpu.py): the repacked weights, 32 rows x 36 taps x 32 channels, and the dW scratch, 32 x 36 x 16 floats
CONV6_WS_ELEMS = 32 * 36 * 32
CONV6_SCRATCH_FLOATS = 32 * 36 * 16


def conv6_fwd(x, x_layout, in_gelu, w, bias, y, y_nchw, w_ws, B, Cin, Cout, H, W):
    _k.i2t_conv6_fwd(x, x_layout, int(in_gelu), w, bias, y, int(y_nchw), w_ws, B, Cin, Cout, H, W)
    return y


def conv6_bwd_data(dy, dy_layout, w, x_pre, dx, w_ws, B, Cin, Cout, H, W):
    _k.i2t_conv6_bwd_data(dy, dy_layout, w, x_pre, dx, w_ws, B, Cin, Cout, H, W)
    return dx


def conv6_bwd_weight(dy, dy_layout, x, x_layout, in_gelu, dw, db, scratch, B, Cin, Cout, H, W):
    _k.i2t_conv6_bwd_weight(dy, dy_layout, x, x_layout, int(in_gelu), dw, db, scratch, B, Cin, Cout, H, W)


def dropout_apply(x, rows, cols, drop):
    """in place; drop = (mode, key, thr, scale)"""
    _k.i2t_dropout_apply(x, int(x.dtype == F32), rows, cols, *_drop(drop))
    return x


def nchw_to_nhwc(src, dst, B, C, H, W):
    _k.i2t_nchw_to_nhwc_bf16(src, dst, B, C, H, W)
    return dst


def cast_f32_bf16(src, dst, n=None):
    if precise():
        dst._i2t_lo = torch.zeros_like(dst)
        return split_f32(src, dst, dst._i2t_lo, n)
    _k.i2t_cast_f32_bf16(src, dst, src.numel() if n is None else n)
    return dst


def adamw_step(p, g, m, v, p_bf16, n, seg_end, seg_lr, seg_wd, nseg, beta1, beta2, eps, step, grad_scale=1.0):
    _k.i2t_adamw_step(p, g, m, v, p_bf16, n, seg_end, seg_lr, seg_wd, nseg, float(beta1), float(beta2), float(eps), int(step), float(grad_scale))


def snradam_step(p, g, m, v, p_bf16, n, seg_end, seg_lr, seg_wd, nseg, beta1, beta2, eps, step, grad_scale=1.0):
    _k.i2t_snradam_step(p, g, m, v, p_bf16, n, seg_end, seg_lr, seg_wd, nseg, float(beta1), float(beta2), float(eps), int(step), float(grad_scale))


def bcast_rows(src, y, y_batch_stride, B, rows, d, drop=None):
    assert drop is None or int(drop[0]) == 1
    _k.i2t_bcast_rows_drop(src, y, y_batch_stride, B, rows, d, *_drop(drop)[1:])


def sum_over_batch(x, x_batch_stride, dst, B, rows, d, accumulate=False):
    _k.i2t_sum_over_batch(x, x_batch_stride, dst, B, rows, d, int(accumulate))


def copy_rows(x, x_bs, y, y_bs, B, rows, d):
    _k.i2t_copy_rows(x, x_bs, y, y_bs, int(y.dtype == BF16), B, rows, d)


def add_(dst, src):
    _k.i2t_add_f32(dst, src, dst.numel())
    return dst


def decode_attention(q, q_rs, kcache, vcache, cache_bs, cache_rs, o, o_rs, pos, n_keys_fixed, B, H, append_dm=0, cache_hs=64):
    """cache_hs = 64: token-major cache rows [t][H][64]; cache_hs = tmax * 64 with cache_rs = 64: head-major [H][t][64]"""
    _k.i2t_decode_attention(q, q_rs, kcache, vcache, cache_bs, cache_rs, cache_hs, o, o_rs, pos, n_keys_fixed, append_dm, B, H)


def kv_append(qkv, qkv_rs, kcache, vcache, cache_bs, cache_rs, pos, B, d):
    _k.i2t_kv_append(qkv, qkv_rs, kcache, vcache, cache_bs, cache_rs, pos, B, d)


def kv_prefill(src, src_ld, k_off, v_off, src_T, src_t0, m, kcache, vcache, cache_bs, cache_rs, cache_hs, hd, w, slot0, B, N):
    """The K / V rows a forward pass saved for m tokens of B images into slots slot0 .. slot0 + m - 1 of the N cache rows of every image
    (include/i2t.h::i2t_kv_prefill); cache_rs / cache_hs as decode_attention (head-major) and gq_decode_attention (row-major: w, hd)."""
    _k.i2t_kv_prefill(src, src_ld, k_off, v_off, src_T, src_t0, m, kcache, vcache, cache_bs, cache_rs, cache_hs, hd, w, slot0, B, N)


def ngram_ban_argmax(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, margin_out=None):
    _k.i2t_ngram_ban_argmax(logits, ld, int(logits.dtype == F32), ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, margin_out)


def gemm_top2(a, b, top2, M, N, K):
    """the two largest of every 64-column segment of a . b^T, not the product (include/i2t.h::i2t_gemm_bf16_top2); top2 f32 [M, ceil(N/64), 4]"""
    assert a.dtype == BF16 and b.dtype == BF16 and top2.is_contiguous() and top2.shape[-2] == (N + 63) // 64
    _k.i2t_gemm_bf16_top2(a, a.stride(0), b, b.stride(0), M, N, K, top2, (N + 63) // 64)
    return top2


def top2_ngram_argmax(top2, hidden, w_head, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, d):
    """n-gram ban + argmax over gemm_top2's segments (include/i2t.h::i2t_top2_ngram_argmax)"""
    _k.i2t_top2_ngram_argmax(top2, (V + 63) // 64, hidden, hidden.stride(0), w_head, w_head.stride(0), d, ids, ids_ld, len_ptr, ngram_sizes, n_sizes,
                             B, V)


def sample_token(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, temperature, top_k, nucleus_p, seed, dist_out=None):
    """One sampling step (include/i2t.h::i2t_sample_token); top_k None/0 = no crop, nucleus_p None = no cut."""
    assert seed.numel() >= 2
    _k.i2t_sample_token(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, float(temperature), int(top_k or 0),
                        float(-1.0 if nucleus_p is None else nucleus_p), seed, dist_out, 0 if dist_out is None else dist_out.stride(0))


def embed_step(ids, ids_ld, len_ptr, wte, wpe, x, B, d, pos_offset, vocab):
    _k.i2t_embed_step(ids, ids_ld, len_ptr, wte, wpe, x, B, d, pos_offset, vocab)


def advance(counters, delta=1):
    _k.i2t_advance(counters, counters.numel(), delta)


def gemm_top2_lse(a, b, top2, se, M, N, K):
    """gemm_top2 that also leaves se f32 [M, ceil(N/64)]: the segment's sum of exp(z - v1) (include/i2t.h::i2t_gemm_bf16_top2_lse)"""
    nseg = (N + 63) // 64
    assert a.dtype == BF16 and b.dtype == BF16 and top2.is_contiguous() and se.is_contiguous()
    assert top2.shape[-1] == 4 and top2.shape[-2] == nseg and top2.numel() >= M * nseg * 4 and se.shape[-1] == nseg and se.numel() >= M * nseg
    assert a.stride(-1) == 1 and b.stride(-1) == 1 and a.shape[0] >= M and b.shape[0] >= N
    _k.i2t_gemm_bf16_top2_lse(a, a.stride(0), b, b.stride(0), M, N, K, top2, se, nseg)
    return top2, se


def _lp_args(ids, ids_ld, done, tok_lp, B):
    """the shared checks of the caption-step choosers: tok_lp f32 rows addressed like the id rows, done an int32 device word"""
    assert done.numel() >= 1 and tok_lp.stride(-1) == 1 and tok_lp.shape[0] >= B and tok_lp.shape[1] >= ids_ld


def top2_ngram_argmax_lp(top2, se, hidden, w_head, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, d, done, tok_lp):
    """top2_ngram_argmax + tok_lp[b][len] = log-prob of the chosen token; no write once *done (include/i2t.h::i2t_top2_ngram_argmax_lp)"""
    _lp_args(ids, ids_ld, done, tok_lp, B)
    assert hidden.dtype == BF16 and w_head.dtype == BF16
    _k.i2t_top2_ngram_argmax_lp(top2, se, (V + 63) // 64, hidden, hidden.stride(0), w_head, w_head.stride(0), d, ids, ids_ld, len_ptr, ngram_sizes,
                                n_sizes, B, V, done, tok_lp, tok_lp.stride(0))


def ngram_ban_argmax_lp(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, done, tok_lp):
    """ngram_ban_argmax over fp32 logits + tok_lp[b][len]; no write once *done (include/i2t.h::i2t_ngram_ban_argmax_lp)"""
    _lp_args(ids, ids_ld, done, tok_lp, B)
    _k.i2t_ngram_ban_argmax_lp(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, done, tok_lp, tok_lp.stride(0))


def sample_token_lp(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, temperature, top_k, nucleus_p, seed, done, tok_lp,
                    dist_out=None):
    """sample_token + tok_lp[b][len] = log-prob of the drawn token under the RAW row; no write once *done (i2t_sample_token_lp)"""
    _lp_args(ids, ids_ld, done, tok_lp, B)
    assert seed.numel() >= 2
    _k.i2t_sample_token_lp(logits, ld, ids, ids_ld, len_ptr, ngram_sizes, n_sizes, B, V, float(temperature), int(top_k or 0),
                           float(-1.0 if nucleus_p is None else nucleus_p), seed, dist_out, 0 if dist_out is None else dist_out.stride(0), done,
                           tok_lp, tok_lp.stride(0))


def caption_finish(ids, ids_ld, len_ptr, eos, pad, finished, lengths, tok_lp, ctrl, R):
    """the finish rule of a caption step (include/i2t.h::i2t_caption_finish); eos None/-1 = no rule"""
    assert tok_lp.stride(-1) == 1 and finished.numel() >= R and lengths.numel() >= R and ctrl.numel() >= 2
    _k.i2t_caption_finish(ids, ids_ld, len_ptr, -1 if eos is None else int(eos), int(pad), finished, lengths, tok_lp, tok_lp.stride(0), ctrl, R)


def caption_finish_ragged(ids, ids_ld, len_ptr, prompt, plen, N, max_new, eos, pad, finished, lengths, tok_lp, ctrl, R):
    """the finish rule of a caption step whose rows have prompts of different lengths: forced while len < plen[r // N], the budget
    of max_new emitted tokens counted per row (include/i2t.h::i2t_caption_finish_ragged); prompt int64 [B, ld], plen int32 [B]"""
    assert tok_lp.stride(-1) == 1 and finished.numel() >= R and lengths.numel() >= R and ctrl.numel() >= 2
    assert prompt.dim() == 2 and prompt.stride(-1) == 1 and plen.is_contiguous()
    assert N >= 1 and R % N == 0 and prompt.shape[0] >= R // N and plen.numel() >= R // N
    _k.i2t_caption_finish_ragged(ids, ids_ld, len_ptr, prompt, prompt.stride(0), plen, N, int(max_new), -1 if eos is None else int(eos), int(pad),
                                 finished, lengths, tok_lp, tok_lp.stride(0), ctrl, R)


def caption_logits_process(logits, ld, ids, ids_ld, len_ptr, plen, P, N, suppress, n_suppress, eos, min_new, theta, inv_theta, done, raw_lse,
                           saved, R, V):
    """the logits processors of a caption step on fp32 logits rows, in place, before the chooser: repetition penalty over
    ids[r][0 .. len), the suppress list (int32, the first n_suppress entries; None: none), EOS below min_new emitted tokens (plen int32
    [R / N], or None: every prompt P long); raw_lse [R] and saved [R, >= ids_ld] keep what caption_raw_logprob needs; no write once
    *done (include/i2t.h::i2t_caption_logits_process).  inv_theta: 1 / theta rounded to fp32 by the caller"""
    assert saved.dim() == 2 and saved.stride(-1) == 1 and saved.shape[0] >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    assert plen is None or (plen.is_contiguous() and N >= 1 and plen.numel() >= R // N)
    assert suppress is None or (suppress.is_contiguous() and suppress.numel() >= n_suppress)
    assert suppress is not None or n_suppress == 0
    _k.i2t_caption_logits_process(logits, ld, ids, ids_ld, len_ptr, plen, int(P), int(N), suppress, int(n_suppress), -1 if eos is None else int(eos),
                                  int(min_new), float(theta), float(inv_theta), done, raw_lse, saved, saved.stride(0), R, V)


def caption_raw_logprob(ids, ids_ld, len_ptr, raw_lse, saved, logits, ld, done, tok_lp, R, V):
    """after the chooser of a processed step: tok_lp[r][len] = raw z[ids[r][len]] - raw_lse[r], the raw logit from ``saved`` when the
    token occurs in ids[r][0 .. len), else from ``logits``; no write once *done (include/i2t.h::i2t_caption_raw_logprob)"""
    assert tok_lp.dim() == 2 and tok_lp.stride(-1) == 1 and tok_lp.shape[0] >= R
    assert saved.dim() == 2 and saved.stride(-1) == 1 and saved.shape[0] >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    _k.i2t_caption_raw_logprob(ids, ids_ld, len_ptr, raw_lse, saved, saved.stride(0), logits, ld, done, tok_lp, tok_lp.stride(0), R, V)


def caption_top_logprobs(logits, ld, len_ptr, plen, N, finished, done, top_tok, top_lp, entropy, K, R, V):
    """the alternatives of a caption step on RAW fp32 logits rows, which are only read: column *len_ptr of top_tok (int32 [R, out_ld, K]:
    the K best columns by (z descending, id ascending)), top_lp (f32, same shape: z - the row's rows_lse value) and entropy (f32 [R,
    out_ld]); nothing for a finished row, a row in a forced column (plen int32 [R / N], or None: no row is), a column outside the
    outputs, or once *done (include/i2t.h::i2t_caption_top_logprobs)"""
    assert top_tok.dim() == 3 and top_tok.is_contiguous() and top_lp.is_contiguous() and top_tok.shape == top_lp.shape
    assert top_tok.shape[0] >= R and top_tok.shape[2] == K and entropy.is_contiguous() and tuple(entropy.shape) == tuple(top_tok.shape[:2])
    assert finished.is_contiguous() and finished.numel() >= R
    assert plen is None or (plen.is_contiguous() and (N < 1 or plen.numel() >= -(-R // N)))
    _k.i2t_caption_top_logprobs(logits, ld, len_ptr, plen, int(N), finished, done, top_tok, top_lp, entropy, top_tok.shape[1], int(K), R, V)


def score_top_logprobs(logits, ld, labels, top_tok, top_lp, entropy, rank, lse, logprob, K, R, V, scale=1.0, ignore_index=-100):
    """the alternatives, entropy, lse and label rank / log-prob of R teacher-forced fp32 logits rows, which are only read, on v = z * scale
    (one fp32 rounding per column): top_tok (int32 [R, K]: the K best columns by (v descending, id ascending)), top_lp (f32 [R, K]: v -
    lse), entropy / lse / logprob (f32 [R]) and rank (int32 [R]: columns strictly ahead of labels[r], -1 and logprob 0 for an ignored
    or out-of-range label) (include/i2t.h::i2t_score_top_logprobs)"""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.stride(0) == ld and logits.shape[0] >= R
    assert top_tok.dim() == 2 and top_tok.is_contiguous() and top_lp.is_contiguous() and top_tok.shape == top_lp.shape
    assert top_tok.shape[0] >= R and top_tok.shape[1] == K and labels.is_contiguous() and labels.numel() >= R
    for t in (entropy, rank, lse, logprob):
        assert t.is_contiguous() and t.numel() >= R
    _k.i2t_score_top_logprobs(logits, ld, float(scale), labels, int(ignore_index), top_tok, top_lp, entropy, rank, lse, logprob, int(K), R, V)


def _trie_args(child_off, child_tok, term, child_next=None):
    """the shared checks of the trie kernels: int32 CSR arrays on the device -> (nodes, edges) the arrays hold"""
    arrays = (child_off, child_tok, term) + (() if child_next is None else (child_next,))
    assert all(t.is_contiguous() for t in arrays)
    assert child_off.numel() == term.numel() + 1 and (child_next is None or child_next.numel() == child_tok.numel())
    return term.numel(), child_tok.numel()


def caption_trie_mask(logits, ld, node, child_off, child_tok, term, eos, done, raw_lse, kept, R, V):
    """the pre-pass of a phrase-constrained caption step on fp32 logits rows, in place, before the chooser: -inf everywhere in [0, V)
    except the children of node[r] and, at a node that ends a phrase, EOS; raw_lse [R] and kept [R, >= max fan-out + 1] take the raw
    row's log-sum-exp and the raw allowed logits; no write once *done (include/i2t.h::i2t_caption_trie_mask)"""
    nodes, edges = _trie_args(child_off, child_tok, term)
    assert kept.dim() == 2 and kept.stride(-1) == 1 and kept.shape[0] >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    assert node.is_contiguous() and node.numel() >= R
    _k.i2t_caption_trie_mask(logits, ld, node, child_off, child_tok, term, nodes, edges, int(eos), done, raw_lse, kept, kept.stride(0), R, V)


def caption_trie_advance(ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok, child_next, term, eos, done, node,
                         phrase_index, tok_lp, R, V):
    """the post-pass of a phrase-constrained caption step, after the chooser: a row that is not finished moves to the chosen child or,
    on EOS at a node that ends a phrase, takes that phrase's index; tok_lp[r][len] = logits[r][chosen] - raw_lse[r]; no write once
    *done (include/i2t.h::i2t_caption_trie_advance)"""
    nodes, edges = _trie_args(child_off, child_tok, term, child_next)
    assert node.is_contiguous() and phrase_index.is_contiguous()
    assert node.numel() >= R and phrase_index.numel() >= R and finished.numel() >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    assert tok_lp.dim() == 2 and tok_lp.stride(-1) == 1 and tok_lp.shape[0] >= R
    _k.i2t_caption_trie_advance(ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok, child_next, term, nodes, edges, int(eos),
                                done, node, phrase_index, tok_lp, tok_lp.stride(0), R, V)


def caption_trie_mask_ragged(logits, ld, node, child_off, child_tok, term, eos, done, raw_lse, kept, len_ptr, plen, N, R, V):
    """caption_trie_mask under ``prompt_lengths``: row r belongs to image r // N, and while *len_ptr < plen[r // N] (plen int32 [R / N])
    its logits row stays raw and raw_lse[r] / kept[r] are not written (include/i2t.h::i2t_caption_trie_mask_ragged)"""
    nodes, edges = _trie_args(child_off, child_tok, term)
    assert kept.dim() == 2 and kept.stride(-1) == 1 and kept.shape[0] >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    assert node.is_contiguous() and node.numel() >= R
    assert plen is None or (plen.is_contiguous() and (N < 1 or plen.numel() >= R // N))
    _k.i2t_caption_trie_mask_ragged(logits, ld, node, child_off, child_tok, term, nodes, edges, int(eos), done, raw_lse, kept, kept.stride(0),
                                    len_ptr, plen, int(N), R, V)


def caption_trie_advance_ragged(ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok, child_next, term, eos, done, node,
                                phrase_index, tok_lp, plen, N, R, V):
    """caption_trie_advance under ``prompt_lengths``: a row in a forced column (*len_ptr < plen[r // N]) keeps node, phrase_index and
    tok_lp[r][len] (include/i2t.h::i2t_caption_trie_advance_ragged)"""
    nodes, edges = _trie_args(child_off, child_tok, term, child_next)
    assert node.is_contiguous() and phrase_index.is_contiguous()
    assert node.numel() >= R and phrase_index.numel() >= R and finished.numel() >= R and raw_lse.is_contiguous() and raw_lse.numel() >= R
    assert tok_lp.dim() == 2 and tok_lp.stride(-1) == 1 and tok_lp.shape[0] >= R
    assert plen is None or (plen.is_contiguous() and (N < 1 or plen.numel() >= R // N))
    _k.i2t_caption_trie_advance_ragged(ids, ids_ld, len_ptr, finished, logits, ld, raw_lse, child_off, child_tok, child_next, term, nodes, edges,
                                       int(eos), done, node, phrase_index, tok_lp, tok_lp.stride(0), plen, int(N), R, V)


def rows_lse(logits, ld, lse, R, V):
    """lse[r] = the log-sum-exp of columns [0, V) of fp32 logits row r, in caption_trie_mask's reduction order; the rows are only read
    (include/i2t.h::i2t_rows_lse)"""
    assert lse.is_contiguous() and lse.numel() >= R
    _k.i2t_rows_lse(logits, ld, lse, R, V)
    return lse


class TrieLevelTables:
    """One level's tables of trie_level_expand on the device (int32, one allocation each): child_parent / child_tok [n_child] -- the next
    level's row j takes token child_tok[j] behind the parent in row child_parent[j] of this level --, term_row [n_term], term_off
    [n_term + 1], term_phrase [n_term_phrases]: row term_row[j] ends the phrases term_phrase[term_off[j] .. term_off[j + 1])."""

    def __init__(self, child_parent, child_tok, term_row, term_off, term_phrase, n_child, n_term, n_term_phrases):
        self.child_parent, self.child_tok, self.term_row, self.term_off, self.term_phrase = child_parent, child_tok, term_row, term_off, term_phrase
        self.n_child, self.n_term, self.n_term_phrases = n_child, n_term, n_term_phrases


def trie_level_tables(child_parent, child_tok, term_row, term_off, term_phrase, W: int, V: int, K: int, device) -> TrieLevelTables:
    """The host-built tables of one level (integer sequences or numpy arrays), checked BEFORE upload -- the kernel cannot refuse what it
    reads from device memory -- and uploaded: I2TError for a parent or terminal row outside [0, W), more children or terminal rows than
    W, a token outside [0, V), offsets that do not ascend from 0 to len(term_phrase), a phrase index outside [0, K)."""
    import numpy as np
    arr = lambda a: np.asarray(a, dtype=np.int64).reshape(-1)
    child_parent, child_tok, term_row, term_off, term_phrase = (arr(a) for a in (child_parent, child_tok, term_row, term_off, term_phrase))
    bad = lambda a, hi: bool(a.size) and (int(a.min()) < 0 or int(a.max()) >= hi)
    if child_parent.shape != child_tok.shape or term_off.shape != (term_row.shape[0] + 1,):
        raise _l.I2TError(f'trie_level_tables: {child_parent.shape[0]} parent rows for {child_tok.shape[0]} tokens, {term_off.shape[0]} offsets for '
                          f'{term_row.shape[0]} terminal rows')
    if child_parent.shape[0] > W or term_row.shape[0] > W:
        raise _l.I2TError(f'trie_level_tables: {child_parent.shape[0]} child rows, {term_row.shape[0]} terminal rows exceed the W = {W} rows of an image')
    if bad(child_parent, W):
        raise _l.I2TError(f'trie_level_tables: a parent row outside [0, {W})')
    if bad(term_row, W):
        raise _l.I2TError(f'trie_level_tables: a terminal row outside [0, {W})')
    if bad(child_tok, V):
        raise _l.I2TError(f'trie_level_tables: a token outside the vocabulary [0, {V})')
    if int(term_off[0]) != 0 or int(term_off[-1]) != term_phrase.shape[0] or bool((np.diff(term_off) < 0).any()):
        raise _l.I2TError(f'trie_level_tables: term_off does not ascend from 0 to the {term_phrase.shape[0]} phrase indices')
    if bad(term_phrase, K):
        raise _l.I2TError(f'trie_level_tables: a phrase index outside [0, {K})')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate((a, np.zeros(1, np.int64))).astype(np.int32))).to(device)
    return TrieLevelTables(up(child_parent), up(child_tok), up(term_row), up(term_off), up(term_phrase), int(child_tok.shape[0]),
                           int(term_row.shape[0]), int(term_phrase.shape[0]))


def trie_level_expand(tables: TrieLevelTables, lse, path_in, path_out, ids, ids_ld, len_ptr, logprob, eos, B, W, V, *, hidden=None,
                      w_head=None, d=0, scale=1.0, logits=None, ld=0):
    """one level of score_phrases' walk over ``tables`` (trie_level_tables): the next level's path sums and tokens, and the log-probs of
    the phrases that end at this level; z from ``logits`` [B W, ld] when given, else re-evaluated from ``hidden`` [B W, d] and ``w_head``
    [V, d] (include/i2t.h::i2t_trie_level_expand)"""
    assert all(t.is_contiguous() and t.numel() >= B * W for t in (lse, path_in, path_out)) and ids.shape[0] >= B * W
    assert logprob.dim() == 2 and logprob.stride(-1) == 1 and logprob.shape[0] >= B
    assert logits is None or logits.shape[0] >= B * W
    assert logits is not None or (hidden.dtype == BF16 and w_head.dtype == BF16 and hidden.stride(-1) == 1 and w_head.stride(-1) == 1
                                  and hidden.shape[0] >= B * W and w_head.shape[0] >= V)
    t = tables
    _k.i2t_trie_level_expand(hidden, 0 if hidden is None else hidden.stride(0), w_head, 0 if w_head is None else w_head.stride(0), int(d),
                             float(scale), logits, int(ld), lse, path_in, path_out, t.child_parent, t.child_tok, t.n_child, t.term_row, t.term_off,
                             t.term_phrase, t.n_term, t.n_term_phrases, ids, ids_ld, len_ptr, logprob, logprob.stride(0), int(eos), B, W, V)


class TrieSetTables:
    """The level tables of every (set, level) of a score_phrases(phrase_sets=...) call on the device, end to end (int32, one allocation
    each; trie_set_tables), with the sizes trie_level_expand_sets hands the kernel."""

    def __init__(self, child_parent, child_tok, term_row, term_off, term_phrase, n_child_all, n_term_all, n_off_all, n_term_phrases, kmax):
        self.child_parent, self.child_tok, self.term_row, self.term_off, self.term_phrase = child_parent, child_tok, term_row, term_off, term_phrase
        self.n_child_all, self.n_term_all, self.n_off_all, self.n_term_phrases, self.kmax = n_child_all, n_term_all, n_off_all, n_term_phrases, kmax


def trie_set_tables(tabs, W: int, V: int, device) -> TrieSetTables:
    """``phrase_trie.set_level_tables``' arrays, checked BEFORE upload as trie_level_tables checks one level's, segment by segment:
    I2TError for a segment outside its arrays or wider than W, a parent or terminal row outside [0, W), a token outside [0, V), a
    segment's offsets that do not ascend inside term_phrase, a phrase index outside [0, kmax)."""
    import numpy as np
    arr = lambda a: np.asarray(a, dtype=np.int64).reshape(-1)
    cp, ct, tr, to, tp = (arr(a) for a in (tabs.child_parent, tabs.child_tok, tabs.term_row, tabs.term_off, tabs.term_phrase))
    seg = [arr(a) for a in (tabs.child_at, tabs.n_child, tabs.term_at, tabs.n_term, tabs.off_at)]
    kmax = int(tabs.kmax)
    bad = lambda a, hi: bool(a.size) and (int(a.min()) < 0 or int(a.max()) >= hi)
    if cp.shape != ct.shape or len({a.shape for a in seg}) != 1 or kmax < 1:
        raise _l.I2TError(f'trie_set_tables: {cp.shape[0]} parent rows for {ct.shape[0]} tokens, segment arrays of {[a.shape[0] for a in seg]}, kmax = {kmax}')
    for g, (ca, nc, ta, nt, oa) in enumerate(zip(*(a.tolist() for a in seg))):
        if min(ca, nc, ta, nt, oa) < 0 or ca + nc > cp.shape[0] or ta + nt > tr.shape[0] or oa + nt + 1 > to.shape[0]:
            raise _l.I2TError(f'trie_set_tables: segment {g} lies outside its tables')
        if nc > W or nt > W:
            raise _l.I2TError(f'trie_set_tables: segment {g}: {nc} child rows, {nt} terminal rows exceed the W = {W} rows of an image')
        off = to[oa:oa + nt + 1]
        if int(off[0]) < 0 or int(off[-1]) > tp.shape[0] or bool((np.diff(off) < 0).any()):
            raise _l.I2TError(f'trie_set_tables: segment {g}: term_off does not ascend inside the {tp.shape[0]} phrase indices')
    if bad(cp, W):
        raise _l.I2TError(f'trie_set_tables: a parent row outside [0, {W})')
    if bad(tr, W):
        raise _l.I2TError(f'trie_set_tables: a terminal row outside [0, {W})')
    if bad(ct, V):
        raise _l.I2TError(f'trie_set_tables: a token outside the vocabulary [0, {V})')
    if bad(tp, kmax):
        raise _l.I2TError(f'trie_set_tables: a phrase index outside [0, {kmax})')
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate((a, np.zeros(1, np.int64))).astype(np.int32))).to(device)
    return TrieSetTables(up(cp), up(ct), up(tr), up(to), up(tp), int(cp.shape[0]), int(tr.shape[0]), int(to.shape[0]), int(tp.shape[0]), kmax)


class TrieSetState:
    """The per-image state of one trie_level_expand_sets launch on the device (int32 [B, 8]; trie_set_state) and the entries per image
    its two parts need."""

    def __init__(self, state, e_child, e_term, B):
        self.state, self.e_child, self.e_term, self.B = state, e_child, e_term, B


def trie_set_state(tables: TrieSetTables, state, W: int, V: int, ids_ld: int, device) -> TrieSetState:
    """One step's per-image state (``phrase_trie.set_step_state``: int [B, 8] = level or -1, forced token or -1, child start and count,
    terminal start and count, offset start, id column), checked BEFORE upload -- the entry point cannot read device memory --:
    I2TError for a level below -1, a forced token outside [-1, V), a range of an image at a level outside the tables or wider than W,
    a column outside [0, ids_ld)."""
    import numpy as np
    st = np.asarray(state, dtype=np.int64)
    if st.ndim != 2 or st.shape[1] != 8 or st.shape[0] < 1:
        raise _l.I2TError(f'trie_set_state: a state of shape {tuple(st.shape)}: 8 integers per image')
    level, forced, ca, nc, ta, nt, oa, col = st.T
    at = level >= 0
    if bool((level < -1).any()):
        raise _l.I2TError('trie_set_state: a level below -1')
    if bool(((forced < -1) | (forced >= V))[~at].any()):
        raise _l.I2TError(f'trie_set_state: a forced token outside [-1, {V})')
    t = tables
    if bool(((ca < 0) | (nc < 0) | (nc > W) | (ca + nc > t.n_child_all) | (ta < 0) | (nt < 0) | (nt > W) | (ta + nt > t.n_term_all) | (oa < 0)
             | (oa + nt + 1 > t.n_off_all))[at].any()):
        raise _l.I2TError(f"trie_set_state: an image's table ranges lie outside the tables or exceed the W = {W} rows of an image")
    if bool(((col < 0) | (col >= ids_ld)).any()):
        raise _l.I2TError(f'trie_set_state: an id column outside [0, {ids_ld})')
    e_child = max(int(nc[at].max(initial=0)), W if bool((~at & (forced >= 0)).any()) else 0)
    return TrieSetState(torch.from_numpy(np.ascontiguousarray(st.astype(np.int32))).to(device), e_child, int(nt[at].max(initial=0)), int(st.shape[0]))


def trie_level_expand_sets(tables: TrieSetTables, state: TrieSetState, lse, path_in, path_out, ids, ids_ld, logprob, eos, W, V, *, hidden=None,
                           w_head=None, d=0, scale=1.0, logits=None, ld=0):
    """one step of score_phrases(phrase_sets=...)'s walk: trie_level_expand with every image at its own level of its own set's tables
    (``tables``: trie_set_tables), in a forced prompt column or finished (``state``: trie_set_state); logprob [B, >= kmax]
    (include/i2t.h::i2t_trie_level_expand_sets)"""
    B = state.B
    assert all(t.is_contiguous() and t.numel() >= B * W for t in (lse, path_in, path_out)) and ids.shape[0] >= B * W
    assert logprob.dim() == 2 and logprob.stride(-1) == 1 and logprob.shape[0] >= B and logprob.shape[1] >= tables.kmax
    assert logits is None or logits.shape[0] >= B * W
    assert logits is not None or (hidden.dtype == BF16 and w_head.dtype == BF16 and hidden.stride(-1) == 1 and w_head.stride(-1) == 1
                                  and hidden.shape[0] >= B * W and w_head.shape[0] >= V)
    t = tables
    _k.i2t_trie_level_expand_sets(hidden, 0 if hidden is None else hidden.stride(0), w_head, 0 if w_head is None else w_head.stride(0), int(d),
                                  float(scale), logits, int(ld), lse, path_in, path_out, t.child_parent, t.child_tok, t.n_child_all, t.term_row,
                                  t.n_term_all, t.term_off, t.n_off_all, t.term_phrase, t.n_term_phrases, state.state, state.e_child, state.e_term,
                                  ids, ids_ld, logprob, logprob.stride(0), t.kmax, int(eos), B, W, V)


def trie_beam_candidates(logits, ld, node, path, child_off, child_tok, term, eos, ctrl, cand_edge, cand_total, fin_total, R, W, V, lse=None):
    """the candidates of search_phrases' step on fp32 logits rows: per live row (node[r] a trie node) the W best children by
    path + (z[token] - lse) as edge indices and totals, and the total of ending here at a node that ends a phrase; lse (optional, f32
    [R]) takes the rows' log-sum-exp, rows_lse's value; no write once ctrl[0] (include/i2t.h::i2t_trie_beam_candidates)"""
    nodes, edges = _trie_args(child_off, child_tok, term)
    assert node.is_contiguous() and path.is_contiguous() and node.numel() >= R and path.numel() >= R and ctrl.numel() >= 2
    assert cand_edge.is_contiguous() and cand_total.is_contiguous() and cand_edge.shape == (R, W) and cand_total.shape == (R, W)
    assert fin_total.is_contiguous() and fin_total.numel() >= R and (lse is None or (lse.is_contiguous() and lse.numel() >= R))
    assert logits.shape[0] >= R and logits.stride(-1) == 1
    _k.i2t_trie_beam_candidates(logits, int(ld), node, path, child_off, child_tok, term, nodes, edges, int(eos), ctrl, cand_edge, cand_total,
                                fin_total, lse, R, W, V)


def trie_beam_select(cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, eos, ids, hist, pool_phrase, pool_sum,
                     pool_score, pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, B, W, P, longest, length_penalty):
    """the selection step of search_phrases: the rows' offers into the pool of finished phrases, the W best children as the image's next
    rows (node, path, token, history), the close test (include/i2t.h::i2t_trie_beam_select)"""
    assert child_tok.is_contiguous() and child_next.is_contiguous() and term.is_contiguous() and child_next.numel() == child_tok.numel()
    assert cand_edge.is_contiguous() and cand_total.is_contiguous() and cand_edge.shape == (B * W, W) and cand_total.shape == (B * W, W)
    assert all(t.is_contiguous() and t.numel() == B * W for t in (fin_total, node, path, pool_phrase, pool_sum, pool_score, pool_len))
    assert pool_n.numel() == B and closed.numel() == B and ctrl.numel() >= 2
    assert ids.shape[0] == B * W and hist.shape[0] == B * W and ids.stride(-1) == 1 and hist.stride(-1) == 1
    _k.i2t_trie_beam_select(cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, term.numel(), child_tok.numel(), int(eos),
                            ids, ids.stride(0), hist, hist.stride(0), pool_phrase, pool_sum, pool_score, pool_len, pool_n, closed, pos_ptr,
                            len_ptr, ctrl, B, W, int(P), int(longest), float(length_penalty))


def trie_beam_select_sets(cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, eos, ids, hist, pool_phrase, pool_sum,
                          pool_score, pool_len, pool_n, closed, pos_ptr, len_ptr, ctrl, B, W, P, plen, longest_of, length_penalty):
    """trie_beam_select with a prompt length and a longest phrase per image: plen int32 [B] (None: every prompt P long), longest_of
    int32 [B]; an image whose prompt reaches past the column only records the identity history column
    (include/i2t.h::i2t_trie_beam_select_sets)"""
    assert child_tok.is_contiguous() and child_next.is_contiguous() and term.is_contiguous() and child_next.numel() == child_tok.numel()
    assert cand_edge.is_contiguous() and cand_total.is_contiguous() and cand_edge.shape == (B * W, W) and cand_total.shape == (B * W, W)
    assert all(t.is_contiguous() and t.numel() == B * W for t in (fin_total, node, path, pool_phrase, pool_sum, pool_score, pool_len))
    assert pool_n.numel() == B and closed.numel() == B and ctrl.numel() >= 2
    assert ids.shape[0] == B * W and hist.shape[0] == B * W and ids.stride(-1) == 1 and hist.stride(-1) == 1
    assert plen is None or (plen.is_contiguous() and plen.numel() >= B)
    assert longest_of is None or (longest_of.is_contiguous() and longest_of.numel() >= B)
    _k.i2t_trie_beam_select_sets(cand_edge, cand_total, fin_total, node, path, child_tok, child_next, term, term.numel(), child_tok.numel(),
                                 int(eos), ids, ids.stride(0), hist, hist.stride(0), pool_phrase, pool_sum, pool_score, pool_len, pool_n, closed,
                                 pos_ptr, len_ptr, ctrl, B, W, int(P), plen, longest_of, float(length_penalty))


def gemm_lse(a, b, stats, M, N, K, scale=1.0):
    """(max, sum exp) of every 64-column segment of scale . a . b^T, not the product (include/i2t.h::i2t_gemm_bf16_lse); stats f32 [M, ceil(N/64), 2]"""
    assert a.dtype == BF16 and b.dtype == BF16 and stats.is_contiguous()
    assert stats.shape[-1] == 2 and stats.shape[-2] == (N + 63) // 64 and stats.numel() >= M * stats.shape[-2] * 2
    assert a.stride(-1) == 1 and b.stride(-1) == 1 and a.shape[0] >= M and b.shape[0] >= N
    _k.i2t_gemm_bf16_lse(a, a.stride(0), b, b.stride(0), M, N, K, float(scale), stats, (N + 63) // 64)
    return stats


def lse_token_logprob(stats, hidden, w_head, labels, lse, logprob, M, V, d, scale=1.0, ignore_index=-100):
    """lse[m] and logprob[m] = scale . hidden[m] . w_head[labels[m]] - lse[m] from gemm_lse's segments (include/i2t.h::i2t_lse_token_logprob)"""
    assert hidden.dtype == BF16 and w_head.dtype == BF16
    assert labels.is_contiguous() and lse.is_contiguous() and logprob.is_contiguous() and stats.is_contiguous()
    assert stats.shape[-1] == 2 and stats.shape[-2] == (V + 63) // 64 and stats.numel() >= M * stats.shape[-2] * 2
    assert hidden.stride(-1) == 1 and w_head.stride(-1) == 1 and hidden.shape[0] >= M and w_head.shape[0] >= V
    assert labels.numel() >= M and lse.numel() >= M and logprob.numel() >= M
    _k.i2t_lse_token_logprob(stats, (V + 63) // 64, hidden, hidden.stride(0), w_head, w_head.stride(0), d, float(scale), labels, int(ignore_index),
                             lse, logprob, M, V)
    return logprob, lse


class Graph:
    """hipGraph captured from the launches issued between ``begin()`` and ``end()`` on the current stream."""

    def __init__(self):
        self._exec = None
        self._stream = None

    def begin(self):
        self._stream = torch.cuda.current_stream().cuda_stream
        _l.check(_lib().i2t_graph_capture_begin(self._stream), 'i2t_graph_capture_begin')

    def end(self):
        import ctypes as C
        h = C.c_void_p()
        _l.check(_lib().i2t_graph_capture_end(self._stream, C.byref(h)), 'i2t_graph_capture_end')
        self._exec = h

    def launch(self):
        _l.check(_lib().i2t_graph_launch(self._exec, torch.cuda.current_stream().cuda_stream), 'i2t_graph_launch')

    def __del__(self):
        if self._exec is not None:
            try:
                _lib().i2t_graph_destroy(self._exec)
            except Exception:
                pass


# ---- PretrainedViT pieces (csrc/vit.hip)
ACT_NONE, ACT_GELU, ACT_DGELU, ACT_GELU_ERF, ACT_DGELU_ERF, ACT_GELU_DOUT, ACT_MUL_AUX = 0, 1, 2, 3, 4, 5, 6


def patchify(images, out, B, C, H, W, p):
    assert out.dtype == BF16 and images.is_contiguous()
    _k.i2t_patchify(images, out, B, C, H, W, p)
    return out


def vit_tokens(proj, cls, pos, x, B, T, d):
    _k.i2t_vit_tokens(proj, cls, pos, x, B, T, d)
    return x


def l2norm_fwd(x, y, y_bf16, inv_norm, M, d):
    _k.i2t_l2norm_fwd(x, y, y_bf16, inv_norm, M, d)


def l2norm_bwd(dy, x, inv_norm, dx, M, d, accumulate=False):
    _k.i2t_l2norm_bwd(dy, x, inv_norm, dx, int(accumulate), M, d)
    return dx


def transpose_last2(src, dst, dst_bf16, B, R, C):
    assert src.is_contiguous()
    _k.i2t_transpose_last2(src, dst, dst_bf16, B, R, C)


def peer_lookup_fwd(scores, inp_proj, residual, emb_in, emb_out, out, sv, M, nhead, nq, topk, din, dout):
    """sv: namespace(unit int32 [M, nhead, topk], lr int32 [M, nhead, topk, 2], score f32, dot f32)."""
    assert inp_proj.dtype == BF16 and emb_in.dtype == BF16 and emb_out.dtype == BF16
    _k.i2t_peer_lookup_fwd(scores, inp_proj, residual, emb_in, emb_out, out, sv.unit, sv.lr, sv.score, sv.dot, M, nhead, nq, topk, din, dout)
    return out


def peer_lookup_bwd(dout, inp_proj, emb_in, emb_out, sv, dscores, dinp_proj, g_emb_in, g_emb_out, M, nhead, nq, topk, din, dout_w):
    _k.i2t_peer_lookup_bwd(dout, inp_proj, emb_in, emb_out, sv.unit, sv.lr, sv.score, sv.dot, dscores, dinp_proj, g_emb_in, g_emb_out, M, nhead, nq,
                           topk, din, dout_w)


def gemm_f32(x, P, z, M, N, K):
    assert x.is_contiguous() and P.is_contiguous() and z.is_contiguous()
    _k.i2t_gemm_f32(x, P, z, M, N, K)
    return z


def lsh_embed_fwd(z, tables, slot_stride, tab_off, nbins, grids, grid_off, out, rows, B, n_cls, nK, n_proj, dout):
    _k.i2t_lsh_embed_fwd(z, tables, int(slot_stride), tab_off, nbins, grids, grid_off, out, rows, B, n_cls, nK, n_proj, dout)
    return out


def lsh_embed_bwd(dy, rows, g_tables, slot_stride, tab_off, B, n_cls, nK, n_proj, dout):
    _k.i2t_lsh_embed_bwd(dy, rows, g_tables, int(slot_stride), tab_off, B, n_cls, nK, n_proj, dout)


def l2norm_groups_fwd(x, group_off, y, inv_norm, G, rows, d):
    """l2norm_fwd over G matrices of ``rows`` rows at x + group_off[g] (int64 element offsets); y / inv_norm contiguous"""
    assert group_off.numel() >= G and y.is_contiguous()
    _k.i2t_l2norm_groups_fwd(x, group_off, y, inv_norm, G, rows, d)
    return y


def l2norm_groups_bwd(dy, x, group_off, inv_norm, dx, G, rows, d, accumulate=False):
    assert group_off.numel() >= G and dy.is_contiguous()
    _k.i2t_l2norm_groups_bwd(dy, x, group_off, inv_norm, dx, int(accumulate), G, rows, d)
    return dx


def lsh_soft_fwd(c, params, slot_stride, mean_off, nbins, col_off, z, inv_norm, B, n_cls, nK, n_proj, Ktot):
    """Gaussian-kernel activations of the learnable LSH head, normalised, bf16, slot-major (include/i2t.h::i2t_lsh_soft_fwd)"""
    assert z.dtype == BF16 and c.is_contiguous() and z.is_contiguous() and col_off.numel() == nK + 1
    assert c.numel() == B * n_cls * nK * n_proj == inv_norm.numel() and z.numel() == B * n_cls * Ktot
    _k.i2t_lsh_soft_fwd(c, params, int(slot_stride), mean_off, nbins, col_off, z, inv_norm, B, n_cls, nK, n_proj, Ktot)
    return z


def lsh_soft_bwd(dz, c, inv_norm, params, g_params, slot_stride, mean_off, nbins, col_off, dc, t_ws, B, n_cls, nK, n_proj, Ktot):
    """dz f32 [n_cls B, Ktot] -> dc (c's layout) and g_params (+)= d/d(mean) (None: frozen); include/i2t.h::i2t_lsh_soft_bwd"""
    assert dz.is_contiguous() and dz.numel() == B * n_cls * Ktot and col_off.numel() == nK + 1
    assert c.numel() == B * n_cls * nK * n_proj == inv_norm.numel() == dc.numel() == t_ws.numel()
    _k.i2t_lsh_soft_bwd(dz, c, inv_norm, params, g_params, int(slot_stride), mean_off, nbins, col_off, dc, t_ws, B, n_cls, nK, n_proj, Ktot)
    return dc


# ---- fp8 (e4m3) operand path for frozen weights (csrc/fp8.hip)
def quant_rows_fp8(x, out, scale, M, K):
    """x bf16 / f32 [M, >= K] -> out uint8 [M, ld_out] (e4m3 bytes, zero pad), scale f32 [M] (amax / 448)."""
    assert out.dtype == torch.uint8 and x.dtype in (BF16, F32) and x.stride(-1) == 1
    _k.i2t_quant_rows_fp8(x, int(x.dtype == F32), x.stride(0), out, out.stride(0), scale, M, K)
    return out


def quant_cols_fp8(w, out, scale, N, K):
    """W bf16 [N, K] -> out uint8 [K, ld_out] = W^T quantised per k, scale f32 [K]."""
    assert w.dtype == BF16 and out.dtype == torch.uint8
    _k.i2t_quant_cols_fp8(w, w.stride(0), out, out.stride(0), scale, N, K)
    return out


def rmsnorm_fwd_fp8(x, w, y8, scale, rstd, M, d, eps, y_bf16=None):
    """y8 (e4m3 [M, ld8]) , scale [M] = quantised RMSNorm(x); rstd [M] or None; y_bf16: optional contiguous bf16 copy  (include/i2t.h)"""
    assert y_bf16 is None or (y_bf16.dtype == BF16 and y_bf16.is_contiguous())
    _k.i2t_rmsnorm_fwd_fp8(x, w, y8, y8.stride(0), scale, rstd, M, d, float(eps), y_bf16)
    return y8


def swiglu_fwd_fp8(gate_up, h8, scale, M, ff, h_bf16=None):
    assert h_bf16 is None or (h_bf16.dtype == BF16 and h_bf16.is_contiguous())
    _k.i2t_swiglu_fwd_fp8(gate_up, gate_up.stride(0), h8, h8.stride(0), scale, M, ff, h_bf16)
    return h8


def swiglu_bwd_fp8(dh, gate_up, dgu8, scale, M, ff, dgu_bf16=None):
    assert dh.is_contiguous() and (dgu_bf16 is None or (dgu_bf16.dtype == BF16 and dgu_bf16.is_contiguous()))
    _k.i2t_swiglu_bwd_fp8(dh, gate_up, gate_up.stride(0), dgu8, dgu8.stride(0), scale, M, ff, dgu_bf16)
    return dgu8


def gemm_fp8(a8, sa, b8, sb, out, M, N, K, bias=None, residual=None, act=0):
    """out[M, N] = act((a8[M, K] . b8[N, K]^T) * sa[m] * sb[n] (+ bias)) (+ residual f32); include/i2t.h::i2t_gemm_fp8."""
    assert a8.dtype == torch.uint8 and b8.dtype == torch.uint8 and out.dtype in (BF16, F32)
    _k.i2t_gemm_fp8(a8, a8.stride(0), sa, b8, b8.stride(0), sb, out, out.stride(0), int(out.dtype == F32), M, N, K, bias, int(act), residual,
                    residual.stride(0) if residual is not None else 0)
    return out


# ---- image preprocessing (csrc/preprocess.hip)
def preprocess_images(data, offsets, shapes, out, a, b, max_side, antialias=True):
    """data uint8 (packed images + 16 bytes of tail pad), offsets int64 [B], shapes int32 [B, 3] = (h, w, c) -> out f32 [B, 3, H, W] =
    resize(image) * a[k] + b[k]; ``max_side``: the largest side in ``shapes``.  include/i2t.h::i2t_preprocess_images; the shapes and
    offsets are the caller's to get right (preprocess.py::pack_images): the kernel writes NaN for an image they do not cover."""
    B = offsets.numel()
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
    assert out.dim() == 4 and out.shape[0] == B and out.shape[1] == 3 and out.is_contiguous()
    assert tuple(shapes.shape) == (B, 3) and shapes.is_contiguous() and len(a) == 3 and len(b) == 3
    _k.i2t_preprocess_images(data, data.numel(), offsets, shapes, B, int(max_side), out, out.shape[2], out.shape[3], float(a[0]), float(a[1]),
                             float(a[2]), float(b[0]), float(b[1]), float(b[2]), int(bool(antialias)))
    return out


def preprocess_regions(data, offsets, shapes, regions, out, a, b, max_side, antialias=True):
    """``preprocess_images`` over boxes: regions int32 [R, 6] = (src, top, left, bh, bw, flip) on the device -> out f32 [R, 3, H, W], row r
    the box of image src resized to H x W, mirrored when flip is 1.  include/i2t.h::i2t_preprocess_regions; the regions are the
    caller's to get right (preprocess.py::preprocess_images): the kernel writes NaN for a region its arguments do not cover."""
    B, R = offsets.numel(), regions.shape[0]
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
    assert regions.dim() == 2 and regions.shape[1] == 6 and regions.is_contiguous()
    assert out.dim() == 4 and out.shape[0] == R and out.shape[1] == 3 and out.is_contiguous()
    assert tuple(shapes.shape) == (B, 3) and shapes.is_contiguous() and len(a) == 3 and len(b) == 3
    _k.i2t_preprocess_regions(data, data.numel(), offsets, shapes, B, int(max_side), regions, R, out, out.shape[2], out.shape[3], float(a[0]),
                              float(a[1]), float(a[2]), float(b[0]), float(b[1]), float(b[2]), int(bool(antialias)))
    return out
