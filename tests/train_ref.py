"""float64 statements of the training-step kernels of csrc/norm.hip and the older half of csrc/elementwise.hip, restated from
include/i2t.h on the SAME rounded values the kernels read (bf16 / fp32 inputs are upcast exactly).  Plain torch on whatever device the
operands live on; nothing here loads the library.  Every function returns, beside the result, the per-element quantity its bound
needs (tests/test_row_kernels_gpu.py's rule): sum |terms| of the reduction the element sits behind, or the magnitude of an exp's
argument.  Dropout masks are arguments (bool tensors from image2text_amd/rng.py::keep_mask); there is no second replica here."""
import numpy as np
import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NORM_EPS = 1e-6                                            # the gradient normaliser's 1 / (||g|| + 1e-6)


def f32(v):
    """the fp32 value a float argument reaches the kernel as"""
    return float(np.float32(v))


def d64(t):
    return None if t is None else t.detach().to(F64)


# ----------------------------------------------------------------------------------------------------------- row LayerNorm
def ln_fwd(x, gamma, beta, eps):
    """x [M][d] -> dict(y, mean, rstd) and the bound quantities: ``amp`` [M][d], what one relative rounding of the mean's sum costs y
    (mean|x| rstd |gamma| (1 + xhat^2): through x - mean and through rstd) plus the terms of the affine map; ``mean_abs`` = mean|x|"""
    x, g, b = d64(x), d64(gamma), d64(beta)
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = (xc.pow(2).mean(-1, keepdim=True) + f32(eps)).rsqrt()
    xh = xc * rstd
    y = xh * g + (b if b is not None else 0.0)
    mean_abs = x.abs().mean(-1, keepdim=True)
    amp = mean_abs * rstd * g.abs() * (1 + xh.pow(2)) + (xh * g).abs() + (b.abs() if b is not None else 0.0)
    return dict(y=y, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), amp=amp, mean_abs=mean_abs.squeeze(-1), xhat=xh)


def ln_bwd(dy, x, gamma, mean, rstd, dx0=None, acc_period=0, acc_rows=0, pre_sumsq=None, mask=None, mask_scale=1.0,
           drop=None, drop_scale=1.0):
    """i2t_layernorm_bwd_ex.  dx0: the dx accumulated onto (None: dx_accumulate off); acc_period / acc_rows: only rows r with
    r % acc_period < acc_rows are added onto; pre_sumsq: dx0 is multiplied by 1 / (sqrt(pre_sumsq) + 1e-6) while adding; mask /
    mask_scale (dx_mask): on the f32 dx only; drop / drop_scale (bf16_drop): on the bf16 copy only.
    -> dx (the f32 result), dx_unmasked, dx_bf16 (the value the bf16 copy rounds), sumsq (of the unmasked dx), dgamma, dbeta, and
    dx_terms / dgamma_terms / dbeta_terms / sumsq_terms = sum |terms|"""
    dy, x, g = d64(dy), d64(x), d64(gamma)
    mu, rs = d64(mean).unsqueeze(-1), d64(rstd).unsqueeze(-1)
    xh = (x - mu) * rs
    gg = dy * g
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    dx = rs * (gg - c1 - xh * c2)
    terms = rs * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
    if dx0 is not None:
        pre = 1.0 if pre_sumsq is None else 1.0 / (float(d64(pre_sumsq).reshape(-1)[0]) ** 0.5 + NORM_EPS)
        old = d64(dx0) * pre
        if acc_period:
            rows = torch.arange(x.shape[0], device=x.device)
            old = torch.where((rows % acc_period < acc_rows).unsqueeze(-1), old, torch.zeros_like(old))
        dx, terms = dx + old, terms + old.abs()
    unmasked = dx
    out = dict(dx_unmasked=unmasked, sumsq=unmasked.pow(2).sum(), sumsq_terms=unmasked.pow(2).sum(), dx_terms=terms,
               dgamma=(dy * xh).sum(0), dgamma_terms=(dy * xh).abs().sum(0), dbeta=dy.sum(0), dbeta_terms=dy.abs().sum(0))
    out['dx'] = unmasked if mask is None else torch.where(mask, unmasked * f32(mask_scale), torch.zeros_like(unmasked))
    out['dx_bf16'] = unmasked if drop is None else torch.where(drop, unmasked * f32(drop_scale), torch.zeros_like(unmasked))
    return out


# ------------------------------------------------------------------------------------------------------------- LayerNormND
def lnnd_fwd(x, add, gamma, beta, eps=1e-5, keep=None, keep_scale=1.0):
    """x [B][n], add / gamma / beta [n] (add, beta nullable): one normalisation per slab.  keep [B][n] bool: the elementwise dropout
    of the tensor y is a slab of.  -> y, mean [B], rstd [B], amp (as ln_fwd)"""
    x, a, g, b = d64(x), d64(add), d64(gamma), d64(beta)
    v = x + a if a is not None else x
    r = ln_fwd(v, g, b, eps)
    if keep is not None:
        r['y'] = torch.where(keep, r['y'] * f32(keep_scale), torch.zeros_like(r['y']))
        r['amp'] = r['amp'] * f32(keep_scale)
    return r


def lnnd_bwd(dy, x, add, gamma, mean, rstd):
    """-> dx [B][n], dgamma, dbeta, dadd [n] (dadd = sum_b dx) and their sum |terms|"""
    x, a = d64(x), d64(add)
    v = x + a if a is not None else x
    r = ln_bwd(dy, v, gamma, mean, rstd)
    r['dadd'], r['dadd_terms'] = r['dx'].sum(0), r['dx_terms'].sum(0)
    # the kernel forms x + add in fp32: half an ulp of |x + add|, times rstd, is an absolute error e of xhat (nothing when add is
    # NULL: x is exact).  dx = rstd (g - c1 - xhat c2) moves by rstd e (|c2| + |xhat| mean|g|), dgamma = sum dy xhat by sum |dy| e
    rs, dy64, g = d64(rstd).unsqueeze(-1), d64(dy), d64(dy) * d64(gamma)
    e = (2.0 ** -24 * v.abs() * rs) if a is not None else torch.zeros_like(v)
    xh = (v - d64(mean).unsqueeze(-1)) * rs
    r['dx_add_err'] = rs * e.amax(-1, keepdim=True) * ((g * xh).mean(-1, keepdim=True).abs() + xh.abs() * g.abs().mean(-1, keepdim=True))
    r['dgamma_add_err'] = (dy64.abs() * e).sum(0)
    return r


# --------------------------------------------------------------------------------------------------------------- embedding
def embed_rows(ids, vocab, T, pos_offset, pos=None):
    """(clamped token row, position row) of every flat row: ids are clamped to [0, vocab) as the kernels do; the position is
    pos[row] (packed batches) or row % T, plus pos_offset"""
    ids = ids.reshape(-1).long()
    rows = torch.arange(ids.numel(), device=ids.device)
    p = pos.long() if pos is not None else rows % T
    return ids.clamp(0, vocab - 1), p + pos_offset


def embed_fwd(ids, wte, wpe, T, pos_offset, vocab, pos=None):
    tok, p = embed_rows(ids, vocab, T, pos_offset, pos)
    x = d64(wte)[tok]
    return x + d64(wpe)[p] if wpe is not None else x


def embed_bwd(ids, dx, n_wte, n_wpe, T, pos_offset, vocab, pos=None):
    """-> dwte [n_wte][d], dwpe [n_wpe][d], their sum |terms|, and the number of addends that reach every row of each"""
    tok, p = embed_rows(ids, vocab, T, pos_offset, pos)
    dx = d64(dx).reshape(tok.numel(), -1)
    out = {}
    for name, idx, n in (('dwte', tok, n_wte), ('dwpe', p, n_wpe)):
        z = torch.zeros(n, dx.shape[1], dtype=F64, device=dx.device)
        out[name] = z.clone().index_add_(0, idx, dx)
        out[name + '_terms'] = z.clone().index_add_(0, idx, dx.abs())
        out[name + '_count'] = torch.bincount(idx, minlength=n)
    return out


# ----------------------------------------------------------------------------------------------------------- cross entropy
def ce(z, V, labels, w, inv_temp, ignore_index, gscale=1.0):
    """z bf16 [M][>= V]: F.cross_entropy(z / T, labels, reduction='none') * w with the kernels' dead-row rule (ignore_index, any
    label < 0, any label >= V: lse 0, no loss term, zero gradient).  gscale: the two-pass form's device scalar (1: the one-pass
    form's un-scaled gradient).  -> live, lse, rows (loss terms), loss, loss_abs, grad, gterms (sum |terms| of grad), p, and arg =
    |z/T| + |lse|, the magnitude of the exp's argument terms"""
    it = f32(inv_temp)
    zt = d64(z)[:, :V] * it
    labels = labels.long()
    live = (labels != ignore_index) & (labels >= 0) & (labels < V)
    lab = labels.clamp(0, V - 1)
    lse = torch.logsumexp(zt, -1)
    p = torch.exp(zt - lse[:, None])
    zl = zt.gather(1, lab[:, None]).squeeze(1)
    w64 = d64(w)
    zero = torch.zeros_like(lse)
    rows = torch.where(live, w64 * (lse - zl), zero)
    rows_abs = torch.where(live, w64.abs() * (lse.abs() + zl.abs()), zero)
    onehot = torch.zeros_like(zt).scatter_(1, lab[:, None], 1.0)
    coef = torch.where(live, f32(gscale) * w64 * it, zero)[:, None]
    return dict(live=live, lse=torch.where(live, lse, zero), rows=rows, loss=rows.sum(), loss_abs=rows_abs.sum(), grad=coef * (p - onehot),
                gterms=coef.abs() * (p + onehot), p=p, arg=zt.abs() + lse.abs()[:, None], coef=coef)


def scale_bf16(x, scale):
    """x bf16 -> x * scale (fp64; the kernel rounds it to bf16); scale exactly 1 leaves the bits alone"""
    return d64(x) * f32(scale)


# ----------------------------------------------------------------------------------------------------- gradient normaliser
def sumsq(g, start=None):
    s = d64(g).pow(2).sum()
    return s + float(start) if start is not None else s


def grad_normalize(g, ws=None, keep=None, keep_scale=1.0, keep_f32=False):
    """g <- g / (||g|| + 1e-6).  ws: presummed sum(g^2) as the fp32 the kernel reads (None: computed here); keep / keep_scale: the
    bf16 copy's dropout; keep_f32: g itself stays as it is.  -> g (the f32 result), g_bf16 (the value the bf16 copy rounds), inv"""
    g = d64(g)
    ss = float(d64(ws).reshape(-1)[0]) if ws is not None else float(g.pow(2).sum())
    inv = 1.0 / (ss ** 0.5 + NORM_EPS)
    gn = g * inv
    gb = gn if keep is None else torch.where(keep, gn * f32(keep_scale), torch.zeros_like(gn))
    return dict(g=g if keep_f32 else gn, g_bf16=gb, inv=inv)


# ------------------------------------------------------------------------------------------------------------------- AdamW
def adamw(p, g, m, v, seg_end, seg_lr, seg_wd, beta1, beta2, eps, step, grad_scale=1.0):
    """torch.optim.AdamW's arithmetic (decoupled decay first, bias corrections from ``step``, eps added to sqrt(v_hat)) over a flat
    arena with a segment table; a segment with lr < 0 is frozen (nothing changes), one at lr == 0 advances its moments only.
    -> p, m, v (fp64) and frozen (bool [n]) and the bound quantities p_terms, m_terms, v_terms, upd (the step taken)"""
    p, g, m, v = d64(p), d64(g) * f32(grad_scale), d64(m), d64(v)
    n = p.numel()
    b1, b2, e = f32(beta1), f32(beta2), f32(eps)
    ends = [int(s) for s in seg_end]
    seg = torch.bucketize(torch.arange(n, device=p.device), torch.tensor(ends, device=p.device), right=True).clamp_max(len(ends) - 1)
    lr = torch.tensor([f32(s) for s in seg_lr], dtype=F64, device=p.device)[seg]
    wd = torch.tensor([f32(s) for s in seg_wd], dtype=F64, device=p.device)[seg]
    frozen = lr < 0
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    upd = lr * (m1 / bc1) / ((v1 / bc2).sqrt() + e)
    p1 = p * (1 - lr * wd) - upd
    out = dict(p=torch.where(frozen, p, p1), m=torch.where(frozen, m, m1), v=torch.where(frozen, v, v1), frozen=frozen, upd=upd.abs(),
               p_terms=p.abs() + upd.abs(), m_terms=(b1 * m).abs() + ((1 - b1) * g).abs(), v_terms=b2 * v.abs() + (1 - b2) * g * g,
               sqrt_vhat=(v1 / bc2).sqrt(), eps=e)
    return out


# ------------------------------------------------------------------------------------------------------- strided helpers
def sum_over_batch(x, start=None):
    """x [B][rows][d] -> (sum_b x (+ start), sum |terms|)"""
    x = d64(x)
    s, t = x.sum(0), x.abs().sum(0)
    return (s + d64(start), t + d64(start).abs()) if start is not None else (s, t)


def colsum(x, N, start=None, alpha_sumsq=None):
    """x bf16 [M][>= N] -> (out[n] (+)= f sum_m x[m][n], sum |terms|), f = 1 / (sqrt(alpha_sumsq) + 1e-6) or 1"""
    x = d64(x)[:, :N]
    f = 1.0 if alpha_sumsq is None else 1.0 / (float(d64(alpha_sumsq).reshape(-1)[0]) ** 0.5 + NORM_EPS)
    s, t = x.sum(0) * f, x.abs().sum(0) * f
    return (s + d64(start), t + d64(start).abs()) if start is not None else (s, t)


def dropout(x, keep, scale):
    """x * (keep ? scale : 0) with the sign of x kept on a dropped element (the kernels multiply by the factor)"""
    return d64(x) * torch.where(keep, torch.full_like(d64(x), f32(scale)), torch.zeros_like(d64(x)))
