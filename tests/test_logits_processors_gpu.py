"""The two kernels of a generate_captions step with logits processors, directly through ops.caption_logits_process and
ops.caption_raw_logprob, on the MI355X.

Shapes: R = 3 rows; V in {70, 257, 50257} with ld = V rounded up to 64 columns (engine.VOCAB_PAD: what the decoder's logits buffer
uses), the pad columns holding 1e30 (not part of the row); id rows of 320 columns; len in {1, 2, 255, 256, 257, 319}: the kernel walks a
row's ids in chunks of 256, so the j loop runs on both sides of one block.  Every row holds EOS at column 0, a token that is also
suppressed at column 1, a token whose logit is exactly 0 at column 2, one whose logit is -inf at column 3, and ONE token at columns 5
and 261 (the same token in two chunks); random logits of both signs elsewhere.  theta in {1.3, 0.8, 1.0}; the min-length rule with the
scalar P and with a plen table at N = 1 and N = 3, min_new on both sides of len - p.

Expectation: the processed row is decoding.process_logits_host's, bit for bit (one fp32 multiply on either side); saved holds the raw
gathers; raw_lse and tok_lp are held to the lp_bound form of tests/test_caption_kernels_gpu.py, restated here for rows that ARE the
fp32 inputs (no GEMM in front: the d u sum|h||w| terms of that form are zero): the rounded exponents (3 |a| u per column), three
roundings per merge a column's partial goes through, n_m = ceil(V / 256) + 1 + 6 + 4 merges for 256 threads (a thread's chain, the
xor tree, the waves), one addition per merge and -- as that file counts the row forms -- up to V additions, one log, the final
roundings; tok_lp adds the rounding of its subtraction.  Guard words behind logits, saved, raw_lse and tok_lp stay untouched."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import process_logits_host

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32
U = 2.0 ** -24
R, IDS_LD = 3, 320
VS, LENS, THETAS = (70, 257, 50257), (1, 2, 255, 256, 257, 319), (1.3, 0.8, 1.0)
SUP, SUP_UNSEEN, FREE = 3, 5, 4          # a token that is seen and suppressed, one suppressed only, one that no row ever holds
ZERO_TOK, NINF_TOK = 8, 9                # seen tokens whose raw logits are exactly 0 and -inf
PAD_VALUE = 1e30


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def pad64(V):
    return (V + 63) // 64 * 64


_CASES = {}


def case(V):
    """the raw logits [R, ld], the id rows and the fp64 statistics of one vocabulary -- built once, never changed"""
    if V in _CASES:
        return _CASES[V]
    rng = np.random.default_rng(V)
    ld, eos = pad64(V), V - 3
    ids = rng.integers(10, V - 8, size=(R, IDS_LD))
    ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3] = eos, SUP, ZERO_TOK, NINF_TOK
    ids[:, 261] = ids[:, 5]
    z = (rng.standard_normal((R, ld)) * 3).astype(np.float32)
    z[:, V:] = PAD_VALUE
    z[:, eos] = [2.5, 0.0, -4.0]
    z[:, SUP] = [-1.5, 0.0, 3.0]
    z[:, ZERO_TOK], z[:, NINF_TOK], z[:, 6] = 0.0, -np.inf, -np.inf
    assert not (ids == FREE).any() and not (ids == SUP_UNSEEN).any()
    z64 = torch.from_numpy(z[:, :V]).double()
    c = dict(V=V, ld=ld, eos=eos, ids=ids, z=z, z64=z64, ids_dev=torch.from_numpy(ids).to(dev()), z_dev=torch.from_numpy(z).to(dev()),
             suppress=[SUP, SUP_UNSEEN, SUP])
    _CASES[V] = c
    return c


def lse_bound(z64, V):
    """-> (lse fp64 [R], bound [R]): the lp_bound form at scale 1 with exact inputs"""
    n_m, extra_adds = (V + 255) // 256 + 1 + 6 + 4, V
    vmax = z64.amax(dim=-1)
    a = z64 - vmax[:, None]
    e = torch.exp(a)
    a0 = torch.where(torch.isfinite(a), a.abs(), torch.zeros_like(a))
    rel_se = U * ((3 * a0 + 3 * (n_m + 1) + 64 + n_m + extra_adds) * e).sum(dim=-1) / e.sum(dim=-1)
    lse = torch.logsumexp(z64, dim=-1)
    zabs = torch.where(torch.isfinite(z64), z64.abs(), torch.zeros_like(z64)).amax(dim=-1)
    return lse, U * zabs + rel_se + 2 * U * (lse - vmax).abs() + U * lse.abs()


def guarded(rows, width, fill=float('nan'), dtype=F32):
    """[rows, width] inside a buffer with one guard row of the fill before and two behind -> (view, whole buffer)"""
    buf = torch.full((rows + 3, width), fill, dtype=dtype, device=dev())
    return buf[1:1 + rows], buf


def guards_untouched(buf, rows):
    g = torch.cat([buf[:1].reshape(-1), buf[1 + rows:].reshape(-1)])
    return bool(torch.isnan(g).all())


def bits(t):
    return t.contiguous().view(I32) if t.dtype == F32 else t


def min_length_configs(ln):
    """(plen table or None, P, N, min_new) -> the rule on both sides of len - p; the emitted count of row r is len - p(r)"""
    p = max(ln - 2, 1)
    e = ln - p                                                # 0 at len 1, 1 at len 2, else 2
    return [(None, p, 1, 0), (None, p, 1, e), (None, p, 1, e + 1), (None, ln + 1, 1, 1),
            ([ln, max(ln - 1, 1), ln + 1], 0, 1, 1),           # per row: emitted 0 (banned), 1 or 0, -1 (a forced column: banned)
            ([p], 7, 3, e), ([p], 7, 3, e + 1)]                # N = 3: all three rows belong to image 0; P is not read


@pytest.mark.parametrize('ln', LENS)
@pytest.mark.parametrize('V', VS)
def test_logits_process_and_raw_logprob(ops, V, ln):
    c = case(V)
    ld, eos, ids_np = c['ld'], c['eos'], c['ids']
    sup = torch.tensor(c['suppress'] + [0] * 5, dtype=I32, device=dev())          # (entries past n_suppress are not read)
    n_sup = len(c['suppress'])
    len_ptr = torch.tensor([ln], dtype=I32, device=dev())
    done = torch.zeros(1, dtype=I32, device=dev())
    lse_ref, bound = lse_bound(c['z64'], V)
    raw_gather = np.take_along_axis(c['z'], ids_np[:, :ln], axis=1)
    # the chosen tokens of the post-pass: row 0 the row's latest token (seen), row 1 a token no row holds, row 2 the two-chunk token
    # (seen once below column 5, twice from 262 on) or -- while it is unseen -- itself an unseen token
    chosen = [int(ids_np[0, ln - 1]), FREE, int(ids_np[2, 5])]
    ids = c['ids_dev'].clone()
    ids[:, ln] = torch.tensor(chosen, device=dev())
    ids_before = ids.clone()
    lp_ref = c['z64'][torch.arange(R), torch.tensor(chosen)] - lse_ref
    worst = 0.0
    for theta in THETAS:
        inv = float(np.float32(1.0) / np.float32(theta))
        for plen, P, N, min_new in min_length_configs(ln):
            z, zbuf = guarded(R, ld)
            z.copy_(c['z_dev'])
            saved, sbuf = guarded(R, IDS_LD)
            lse, lbuf = guarded(1, 4)
            lse = lse.view(-1)[:R]
            lse4_before = lbuf[1, 3:].clone()
            plen_dev = None if plen is None else torch.tensor(plen, dtype=I32, device=dev())
            ops.caption_logits_process(z, ld, ids, IDS_LD, len_ptr, plen_dev, P, N, sup, n_sup, eos, min_new, theta, inv, done, lse, saved, R, V)
            tok_lp, tbuf = guarded(R, IDS_LD)
            ops.caption_raw_logprob(ids, IDS_LD, len_ptr, lse, saved, z, ld, done, tok_lp, R, V)
            torch.cuda.synchronize()
            tag = f'V {V} len {ln} theta {theta} plen {plen} P {P} N {N} min_new {min_new}'
            got = z.cpu().numpy()
            for r in range(R):
                p = P if plen is None else plen[r // N]
                want = process_logits_host(c['z'][r, :V], ids_np[r], ln, ln - p, theta, c['suppress'], eos, min_new)
                assert np.array_equal(got[r, :V].view(np.int32), want.view(np.int32)), f'{tag}: row {r} differs from process_logits_host'
                assert (want[eos] == -np.inf) == (ln - p < min_new or c['z'][r, eos] == -np.inf) and want[SUP] == -np.inf
            assert np.array_equal(got[:, V:], c['z'][:, V:]), f'{tag}: a pad column was written'
            assert guards_untouched(zbuf, R) and guards_untouched(sbuf, R) and guards_untouched(tbuf, R), f'{tag}: a guard word was written'
            assert guards_untouched(lbuf, 1) and torch.equal(bits(lbuf[1, 3:]), bits(lse4_before)), f'{tag}: a word behind raw_lse was written'
            assert np.array_equal(saved[:, :ln].cpu().numpy().view(np.int32), raw_gather.view(np.int32)), f'{tag}: saved is not the raw gather'
            assert bool(torch.isnan(saved[:, ln:]).all()), f'{tag}: saved was written past len'
            err = (lse.double().cpu() - lse_ref).abs()
            assert bool((err <= bound).all()), f'{tag}: raw_lse worst error / bound {float((err / bound).max()):.3g}'
            worst = max(worst, float((err / bound).max()))
            assert torch.equal(ids, ids_before), f'{tag}: an id was written'
            keep = torch.ones(IDS_LD, dtype=torch.bool, device=dev())
            keep[ln] = False
            assert bool(torch.isnan(tok_lp[:, keep]).all()), f'{tag}: a log-prob column other than len was written'
            lp = tok_lp[:, ln].double().cpu()
            lp_err, lp_bnd = (lp - lp_ref).abs(), bound + U * lp_ref.abs()
            fin = torch.isfinite(lp_ref)
            assert bool(torch.equal(lp[~fin], lp_ref[~fin])) and bool((lp_err[fin] <= lp_bnd[fin]).all()), \
                f'{tag}: tok_lp {lp.tolist()} vs fp64 {lp_ref.tolist()} (bound {lp_bnd.tolist()})'
            worst = max(worst, float((lp_err[fin] / lp_bnd[fin]).max()))
    print(f'V {V} len {ln}: worst raw_lse / tok_lp error over bound {worst:.3g}')
    if ln > 5:
        assert chosen[2] in ids_np[2, :ln].tolist() and chosen[0] in ids_np[0, :ln].tolist() and FREE not in ids_np[1, :ln].tolist()


@pytest.mark.parametrize('V', VS)
def test_first_column_and_two_launches_equal(ops, V):
    """len = 0: nothing is seen -- the penalty touches nothing, saved stays as it was, the chosen token's raw logit comes from the
    logits row -- and two launches on the same inputs are bit-equal (no atomics, fixed reduction order)"""
    c = case(V)
    ld, eos = c['ld'], c['eos']
    sup = torch.tensor(c['suppress'], dtype=I32, device=dev())
    len_ptr, done = torch.zeros(1, dtype=I32, device=dev()), torch.zeros(1, dtype=I32, device=dev())
    ids = c['ids_dev'].clone()
    chosen = [int(c['eos']), FREE, ZERO_TOK]
    ids[:, 0] = torch.tensor(chosen, device=dev())
    outs = []
    for _ in range(2):
        z = c['z_dev'].clone()
        saved, sbuf = guarded(R, IDS_LD)
        lse = torch.zeros(4, device=dev())
        tok_lp, tbuf = guarded(R, IDS_LD)
        ops.caption_logits_process(z, ld, ids, IDS_LD, len_ptr, None, 0, 1, sup, len(c['suppress']), eos, 0, 1.3, float(np.float32(1) / np.float32(1.3)),
                                   done, lse, saved, R, V)
        ops.caption_raw_logprob(ids, IDS_LD, len_ptr, lse, saved, z, ld, done, tok_lp, R, V)
        torch.cuda.synchronize()
        assert bool(torch.isnan(sbuf).all()) and guards_untouched(tbuf, R)
        outs.append((z, lse, tok_lp[:, 0].clone()))
    for a, b in zip(*outs):
        assert torch.equal(bits(a), bits(b))
    z, lse, lp = outs[0]
    for r in range(R):
        want = process_logits_host(c['z'][r, :V], c['ids'][r], 0, 0, 1.3, c['suppress'], eos, 0)
        assert np.array_equal(z[r, :V].cpu().numpy().view(np.int32), want.view(np.int32))
    lse_ref, bound = lse_bound(c['z64'], V)
    lp_ref = c['z64'][torch.arange(R), torch.tensor(chosen)] - lse_ref
    err = (lp.double().cpu() - lp_ref).abs()
    assert bool((err <= bound + U * lp_ref.abs()).all()), f'tok_lp at len 0: error / bound {float((err / (bound + U * lp_ref.abs())).max()):.3g}'


def test_nothing_is_written_past_done(ops):
    """done = 1 and len == ids_ld (the next row's first column), as the existing past-`done` test of the choosers: neither kernel writes"""
    c = case(257)
    V, ld, eos = c['V'], c['ld'], c['eos']
    z = c['z_dev'].clone()
    ids = c['ids_dev'].clone()
    saved = torch.full((R + 1, IDS_LD), 0.25, device=dev())
    lse, tok_lp = torch.full((4,), 0.5, device=dev()), torch.full((R + 1, IDS_LD), 0.75, device=dev())
    sup = torch.tensor(c['suppress'], dtype=I32, device=dev())
    len_ptr, done = torch.tensor([IDS_LD], dtype=I32, device=dev()), torch.ones(1, dtype=I32, device=dev())
    state = (z, ids, saved, lse, tok_lp)
    before = [t.clone() for t in state]
    ops.caption_logits_process(z, ld, ids, IDS_LD, len_ptr, None, 2, 1, sup, 3, eos, 400, 1.3, float(np.float32(1) / np.float32(1.3)), done, lse,
                               saved, R, V)
    ops.caption_raw_logprob(ids, IDS_LD, len_ptr, lse, saved, z, ld, done, tok_lp, R, V)
    torch.cuda.synchronize()
    for a, b in zip(before, state):
        assert torch.equal(bits(a), bits(b))


def test_entry_point_refusals(ops):
    """every check the entry points make without the device: an error with its message, and the outputs as they were"""
    from image2text_amd import lib as i2tlib
    lib = i2tlib.load()
    c = case(70)
    V, ld, eos = c['V'], c['ld'], c['eos']
    z, ids = c['z_dev'].clone(), c['ids_dev'].clone()
    saved, lse, tok_lp = torch.full((R, IDS_LD), 0.25, device=dev()), torch.full((4,), 0.5, device=dev()), torch.full((R, IDS_LD), 0.75, device=dev())
    sup = torch.tensor(c['suppress'], dtype=I32, device=dev())
    len_ptr, done = torch.tensor([4], dtype=I32, device=dev()), torch.zeros(1, dtype=I32, device=dev())
    plen = torch.tensor([2], dtype=I32, device=dev())
    state = (z, ids, saved, lse, tok_lp)
    before = [t.clone() for t in state]
    stream = torch.cuda.current_stream().cuda_stream
    pre = dict(stream=stream, logits=z.data_ptr(), ld=ld, ids=ids.data_ptr(), ids_ld=IDS_LD, len_ptr=len_ptr.data_ptr(), plen=plen.data_ptr(), P=2,
               N=3, suppress=sup.data_ptr(), n_suppress=3, eos=eos, min_new=1, theta=1.3, inv_theta=1 / 1.3, done=done.data_ptr(),
               raw_lse=lse.data_ptr(), saved=saved.data_ptr(), saved_ld=IDS_LD, R=R, V=V)
    post = dict(stream=stream, ids=ids.data_ptr(), ids_ld=IDS_LD, len_ptr=len_ptr.data_ptr(), raw_lse=lse.data_ptr(), saved=saved.data_ptr(),
                saved_ld=IDS_LD, logits=z.data_ptr(), ld=ld, done=done.data_ptr(), tok_lp=tok_lp.data_ptr(), lp_ld=IDS_LD, R=R, V=V)

    def refused(fn, args, change, text):
        rc = getattr(lib, fn)(*{**args, **change}.values())
        assert rc == -1 and text in i2tlib.last_error() and fn in i2tlib.last_error(), (fn, change, rc, i2tlib.last_error())

    for name in ('logits', 'ids', 'len_ptr', 'done', 'raw_lse', 'saved'):
        refused('i2t_caption_logits_process', pre, {name: None}, 'null pointer')
    refused('i2t_caption_logits_process', pre, dict(suppress=None), 'without a list')
    refused('i2t_caption_logits_process', pre, dict(ld=V - 1), 'ld = 69')
    refused('i2t_caption_logits_process', pre, dict(ld=V + 1), 'ld = 71')
    refused('i2t_caption_logits_process', pre, dict(saved_ld=IDS_LD - 1), 'saved_ld = 319')
    refused('i2t_caption_logits_process', pre, dict(n_suppress=-1), 'n_suppress = -1')
    refused('i2t_caption_logits_process', pre, dict(n_suppress=V), f'n_suppress = {V}')
    refused('i2t_caption_logits_process', pre, dict(eos=V), f'eos = {V}')
    refused('i2t_caption_logits_process', pre, dict(min_new=-1), 'min_new = -1')
    refused('i2t_caption_logits_process', pre, dict(theta=0.0), 'theta = 0')
    refused('i2t_caption_logits_process', pre, dict(theta=-1.3), 'theta = -1.3')
    refused('i2t_caption_logits_process', pre, dict(inv_theta=float('inf')), '1 / theta = inf')
    refused('i2t_caption_logits_process', pre, dict(N=2), 'in groups of 2')
    refused('i2t_caption_logits_process', pre, dict(R=0), 'R = 0')
    for name in ('logits', 'saved', 'raw_lse', 'ids'):
        refused('i2t_caption_logits_process', pre, {name: pre[name] + 4}, 'misaligned')
    for name in ('ids', 'len_ptr', 'raw_lse', 'saved', 'logits', 'done', 'tok_lp'):
        refused('i2t_caption_raw_logprob', post, {name: None}, 'null pointer')
    refused('i2t_caption_raw_logprob', post, dict(ld=V - 1), 'ld = 69')
    refused('i2t_caption_raw_logprob', post, dict(saved_ld=IDS_LD - 1), 'saved_ld = 319')
    refused('i2t_caption_raw_logprob', post, dict(lp_ld=0), 'lp_ld = 0')
    for name in ('logits', 'saved', 'raw_lse', 'ids'):
        refused('i2t_caption_raw_logprob', post, {name: post[name] + 4}, 'misaligned')
    # through the wrappers the same error surfaces as I2TError
    narrow = torch.zeros(R, IDS_LD - 8, device=dev())
    with pytest.raises(i2tlib.I2TError, match='saved_ld'):
        ops.caption_logits_process(z, ld, ids, IDS_LD, len_ptr, None, 2, 1, sup, 3, eos, 1, 1.3, 1 / 1.3, done, lse, narrow, R, V)
    with pytest.raises(i2tlib.I2TError, match='saved_ld'):
        ops.caption_raw_logprob(ids, IDS_LD, len_ptr, lse, narrow, z, ld, done, tok_lp, R, V)
    torch.cuda.synchronize()
    for a, b in zip(before, state):
        assert torch.equal(bits(a), bits(b))
