"""i2t_caption_top_logprobs alone, through ops.caption_top_logprobs, on the MI355X.

Shapes: R = 3 rows and a guard row behind them, V in {70, 257, 50257} (fewer columns than the 256 threads; a tail off a multiple of 4;
the real vocabulary), ld = round_up(V, 4) + 4 with NaN in the padding (read once, it would poison every result), K in {1, 5, 8}, outputs
of OUT_LD = 6 columns pre-filled with a sentinel, the step at column LEN = 2.  Two sets of rows: (a Gaussian row, a lattice row of
multiples of 0.25 with many exact ties, a row with one dominant logit: entropy near 0) and (a constant row: entropy log V and K equal
list entries, a row whose only finite entries are 6 columns, so that K = 8 reaches two -inf columns, a Gaussian row with -inf sprinkled
over it).

Expectation.  Tokens: decoding_host.top_logprobs_host's, exactly.  top_lp: bit-equal to fp32(z[tok]) - ops.rows_lse(...) formed in fp32
on the host, and within the lp_bound form of tests/test_caption_kernels_gpu.py of the fp64 value -- restated here as
tests/test_logits_processors_gpu.py restates it for rows that ARE the fp32 inputs (u = 2^-24): the rounded exponents (3 |a| u per
column), three roundings per merge a column's partial goes through, n_m = ceil(V / 256) + 1 + 6 + 4 merges for 256 threads (a
thread's chain, the xor tree, the waves), one addition per merge and up to V additions, one log, the final roundings; plus u |lp| for
the subtraction.  Call that bound on the lse dL.

The entropy bound, from the kernel's operation count.  Per finite column the kernel forms d^ = fl(lse^ - z), p^ = __expf(-d^), and adds
p^ d^ to the thread's sum.  With d = lse - z exact and p = exp(-d):
  * |d^ - d| <= dd = dL + u d (the lse's error, the subtraction's rounding);
  * __expf(x) is exp2(fl(x log2e)) on v_exp_f32: the constant and the product each round once, a relative error of 2 |x| u in the
    result, and the instruction is good to 1 ulp = 2 u; 4 u is allowed.  So p^ <= p exp(dd) (1 + (2 (d + dd) + 4) u);
  * the product rounds once (not at all as an fma): the term is at most p exp(dd) (1 + (2 (d + dd) + 4) u) (d + dd) (1 + u), and its
    deviation below p d is no larger than the one above (every factor deviates symmetrically to first order, and the second-order part
    is positive above);
  * a term goes through at most n_a = 4 ceil(V / 1024) + 1 + 6 + 3 additions (a thread's chain of 16-byte groups and one tail column,
    the xor tree, the waves in order), all terms non-negative: n_a u times the sum of the computed terms;
  * exp flushes below 2^-126, where d > 87: under 1e-36 per column.
bound = sum_c (upper term - p d) (1 + n_a u) + n_a u H + V 1e-36.  It is dominated by dL (H + 1), and dL by its V u term: at V = 50257
about 3e-3 (H + 1), so the bound is loose by what the lp_bound form is loose by; the test prints worst error / bound.

Guards: only column LEN of the active rows changes; the guard row, every other column, and everything under done = 1, for a finished
row, for a forced row (plen with N = 2, so that r / N matters) and at *len_ptr == out_ld keeps the sentinel.  Every refusal returns an
error with the outputs untouched."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding_host import top_logprobs_host

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
R, OUT_LD, LEN = 3, 6, 2
VS, KS = (70, 257, 50257), (1, 5, 8)
TOK_SENTINEL, F_SENTINEL = -7, -777.0
FINITE = (3, 11, 12, 40, 41, 69)         # the finite columns of the sparse row: two fewer than K = 8


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


_CASES = {}


def case(ops, V, which):
    """the logits [R + 1, ld] of one vocabulary and row set, the replica's answer for every K up to 8, the kernel's own lse and the fp64
    statistics -- built once, never changed"""
    if (V, which) in _CASES:
        return _CASES[V, which]
    rng = np.random.default_rng(1000 * which + V)
    ld = (V + 3) // 4 * 4 + 4
    z = np.full((R + 1, ld), np.nan, dtype=np.float32)
    if which == 0:
        z[0, :V] = rng.standard_normal(V) * 3
        z[1, :V] = rng.integers(-12, 13, size=V) * 0.25
        z[2, :V] = rng.standard_normal(V)
        z[2, V // 3] = 40.0
    else:
        z[0, :V] = 1.75
        z[1, :V] = -np.inf
        z[1, list(FINITE)] = [0.5, -1.0, 0.5, 2.0, -3.0, 0.5]
        z[2, :V] = rng.standard_normal(V) * 2
        z[2, np.flatnonzero(rng.random(V) < 0.3)] = -np.inf
        z[2, V - 1] = -np.inf
    z[R, :V] = rng.standard_normal(V)                            # the guard row: a valid row that no workgroup may take
    z_dev = torch.from_numpy(z).to(dev())
    tok, lp, ent = top_logprobs_host(z[:R, :V], 8)
    lse = torch.zeros(4, dtype=F32, device=dev())
    ops.rows_lse(z_dev, ld, lse, R, V)
    torch.cuda.synchronize()
    c = dict(V=V, ld=ld, z=z, z_dev=z_dev, tok=tok, lp=lp, ent=ent, lse=lse.cpu().numpy()[:R], z64=torch.from_numpy(z[:R, :V]).double())
    _CASES[V, which] = c
    return c


def lse_bound(z64, V, n_m=None):
    """-> (lse fp64 [R], bound [R]): the lp_bound form at scale 1 with exact inputs; n_m: the merges a column's partial goes through,
    by default this kernel's (256 threads)"""
    n_m, extra_adds = (V + 255) // 256 + 1 + 6 + 4 if n_m is None else n_m, V
    vmax = z64.amax(dim=-1)
    a = z64 - vmax[:, None]
    e = torch.exp(a)
    a0 = torch.where(torch.isfinite(a), a.abs(), torch.zeros_like(a))
    rel_se = U * ((3 * a0 + 3 * (n_m + 1) + 64 + n_m + extra_adds) * e).sum(dim=-1) / e.sum(dim=-1)
    lse = torch.logsumexp(z64, dim=-1)
    zabs = torch.where(torch.isfinite(z64), z64.abs(), torch.zeros_like(z64)).amax(dim=-1)
    return lse, U * zabs + rel_se + 2 * U * (lse - vmax).abs() + U * lse.abs()


def entropy_bound(z64, V, dL):
    """-> (entropy fp64 [R], bound [R]): the module docstring's derivation; dL: the bound on the lse's error"""
    lse = torch.logsumexp(z64, dim=-1)
    fin = torch.isfinite(z64)
    zero = torch.zeros_like(z64)
    d = torch.where(fin, lse[:, None] - z64, zero)
    p = torch.where(fin, torch.exp(-d), zero)
    H = (p * d).sum(dim=-1)
    dd = dL[:, None] + U * d
    upper = p * torch.exp(dd) * (1 + (2 * (d + dd) + 4) * U) * (d + dd) * (1 + U)
    n_a = 4 * ((V + 1023) // 1024) + 1 + 6 + 3
    return H, (upper - p * d).sum(dim=-1) * (1 + n_a * U) + n_a * U * H + V * 1e-36


def outputs(K, rows=R + 1):
    return (torch.full((rows, OUT_LD, K), TOK_SENTINEL, dtype=I32, device=dev()), torch.full((rows, OUT_LD, K), F_SENTINEL, dtype=F32, device=dev()),
            torch.full((rows, OUT_LD), F_SENTINEL, dtype=F32, device=dev()))


def untouched(outs, rows=slice(None), cols=slice(None)):
    tok, lp, ent = outs
    return bool((tok[rows, cols] == TOK_SENTINEL).all() and (lp[rows, cols] == F_SENTINEL).all() and (ent[rows, cols] == F_SENTINEL).all())


def i32(*v):
    return torch.tensor(v, dtype=I32, device=dev())


def bits(t):
    return t.contiguous().view(I32)


def launch(ops, c, K, outs, ln=LEN, plen=None, N=1, finished=(0, 0, 0), done=0):
    ops.caption_top_logprobs(c['z_dev'], c['ld'], i32(ln), None if plen is None else i32(*plen), N, i32(*finished, 0), i32(done), *outs, K, R, c['V'])
    torch.cuda.synchronize()


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('V', VS)
def test_tokens_logprobs_and_entropy(ops, V, K):
    worst_lp = worst_h = 0.0
    for which in (0, 1):
        c = case(ops, V, which)
        outs = outputs(K)
        launch(ops, c, K, outs)
        again = outputs(K)
        launch(ops, c, K, again)
        for a, b in zip(outs, again):
            assert torch.equal(bits(a), bits(b)), 'two launches differ'
        keep = [j for j in range(OUT_LD) if j != LEN]
        assert untouched(outs, slice(0, R), keep) and untouched(outs, slice(R, R + 1)), 'a cell outside column LEN of the active rows was written'
        tok, lp, ent = (t[:R, LEN].cpu().numpy() for t in outs)
        assert np.array_equal(tok, c['tok'][:, :K]), f'set {which}: tokens {tok.tolist()} vs the replica {c["tok"][:, :K].tolist()}'
        # one fp32 subtraction from the bits rows_lse gives
        own = np.take_along_axis(c['z'][:R, :V], c['tok'][:, :K].astype(np.int64), axis=1) - c['lse'][:, None]
        assert own.dtype == np.float32 and np.array_equal(lp.view(np.int32), own.view(np.int32)), f'set {which}: top_lp is not z[tok] - rows_lse'
        lse_ref, dL = lse_bound(c['z64'], V)
        assert bool((torch.from_numpy(c['lse']).double() - lse_ref).abs().le(dL).all())
        ref = c['lp'][:, :K]
        fin = np.isfinite(ref)
        assert np.array_equal(lp[~fin], ref[~fin]), 'a -inf column in the list has log-prob -inf'
        bound = (dL.numpy()[:, None] + U * np.abs(np.where(fin, ref, 0.0))) * np.ones_like(ref)
        err = np.abs(np.where(fin, lp.astype(np.float64) - np.where(fin, ref, 0.0), 0.0))
        assert (err <= bound).all(), f'set {which}: top_lp worst error / bound {float((err / bound).max()):.3g}'
        worst_lp = max(worst_lp, float((err / bound).max()))
        H, hb = entropy_bound(c['z64'], V, dL)
        assert np.allclose(H.numpy(), c['ent'], rtol=1e-12, atol=1e-12), 'the bound\'s entropy is the replica\'s'
        herr = np.abs(ent.astype(np.float64) - c['ent'])
        assert (herr <= hb.numpy()).all(), f'set {which}: entropy {ent.tolist()} vs {c["ent"].tolist()}, worst error / bound {float((herr / hb.numpy()).max()):.3g}'
        worst_h = max(worst_h, float((herr / hb.numpy()).max()))
        if which == 0:
            assert ent[2] < 1e-6 * V, 'one dominant logit: entropy near 0'
        else:
            assert abs(float(ent[0]) - np.log(V)) <= float(hb[0]) and tok[0].tolist() == list(range(K)), 'a constant row: log V, ids ascending'
            want = [40, 3, 12, 69, 11, 41] + [0, 1]
            assert tok[1].tolist() == want[:K] and bool(np.isneginf(lp[1, 6:]).all()), 'six finite columns, then -inf columns by ascending id'
    print(f'V {V} K {K}: top_lp worst error / bound {worst_lp:.3g}, entropy worst error / bound {worst_h:.3g}')


@pytest.mark.parametrize('V', VS)
def test_rows_that_are_not_written(ops, V):
    c, K = case(ops, V, 0), 5
    want = c['tok'][:, :K]
    outs = outputs(K)
    launch(ops, c, K, outs, done=1)
    assert untouched(outs), 'written under done = 1'
    launch(ops, c, K, outs, finished=(0, 1, 0))
    assert untouched(outs, 1) and untouched(outs, R), 'a finished row was written'
    assert np.array_equal(outs[0][[0, 2], LEN].cpu().numpy(), want[[0, 2]])
    outs = outputs(K)
    launch(ops, c, K, outs, ln=OUT_LD)
    assert untouched(outs), 'written at *len_ptr == out_ld'
    # N = 2: rows 0 and 1 belong to image 0, row 2 to image 1; only image 0 has reached its emitting columns
    outs = outputs(K)
    launch(ops, c, K, outs, plen=(LEN, LEN + 1), N=2)
    assert untouched(outs, 2) and untouched(outs, R), 'a row inside its prompt was written'
    assert np.array_equal(outs[0][:2, LEN].cpu().numpy(), want[:2])
    outs = outputs(K)
    launch(ops, c, K, outs, plen=(LEN + 1, LEN), N=2)
    assert untouched(outs, slice(0, 2)) and np.array_equal(outs[0][2, LEN].cpu().numpy(), want[2])
    outs = outputs(K)                                            # the last column there is
    launch(ops, c, K, outs, ln=OUT_LD - 1)
    assert untouched(outs, slice(None), slice(0, OUT_LD - 1)) and np.array_equal(outs[0][:R, OUT_LD - 1].cpu().numpy(), want)


def test_refusals(ops):
    from image2text_amd.lib import I2TError
    c, K = case(ops, 70, 0), 5
    V, ld, z = 70, c['ld'], c['z_dev']
    outs = outputs(K)
    ln, fin, done = i32(LEN), i32(0, 0, 0, 0), i32(0)
    call = ops._k.i2t_caption_top_logprobs                       # the wrapper's own assertions would stop some of these before the entry point
    good = [z, ld, ln, None, 1, fin, done, *outs, OUT_LD, K, R, V]
    call(*good)
    torch.cuda.synchronize()
    assert not untouched(outs, slice(0, R), LEN)
    outs = outputs(K)
    good[7:10] = outs

    def refused(text, **change):
        names = ['logits', 'ld', 'len_ptr', 'plen', 'N', 'finished', 'done', 'top_tok', 'top_lp', 'entropy', 'out_ld', 'K', 'R', 'V']
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        with pytest.raises(I2TError) as e:
            call(*args)
        assert 'i2t_caption_top_logprobs' in str(e.value) and text in str(e.value), str(e.value)

    for name in ('logits', 'len_ptr', 'finished', 'done', 'top_tok', 'top_lp', 'entropy'):
        refused('null pointer', **{name: None})
    refused('ld = 68', ld=68)
    refused('ld = 74', ld=74)
    refused('misaligned base pointer', logits=z.view(-1)[1:])
    refused('K = 0', K=0)
    refused('K = 9', K=9)
    refused('K = 5 alternatives of a vocabulary of 4', V=4)
    refused('out_ld = 0', out_ld=0)
    refused('N = 0', N=0)
    refused('R = 0', R=0)
    torch.cuda.synchronize()
    assert untouched(outs), 'a refused call wrote an output'
    with pytest.raises(I2TError, match='wants torch.int32'):
        ops.caption_top_logprobs(z, ld, ln, None, 1, fin, done, outs[0].float(), outs[1], outs[2], K, R, V)
