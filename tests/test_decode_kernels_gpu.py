"""The decode-step kernels at the shapes greedy / sampled captioning runs them (GPT-2 50257, Llama 32000, Falcon 65024 and
Qwen2 151936 vocabularies, up to 1024 cached keys, 1 ... 71 heads), each against a plain fp64 statement of the same op on the
SAME bf16 / fp32 values the kernel reads.  The n-gram ban and the sampling filters come from oracle.reference_model."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, scale=1.0, seed=0, dtype=F32):
    g = torch.Generator(device=dev()).manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g, device=dev()) * scale).to(dtype)


def check(name, got, ref, atol, rtol):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    if bad.any():
        idx = np.unravel_index(int((err - tol).argmax()), tuple(got.shape))
        raise AssertionError(f'{name}: {int(bad.sum())}/{bad.numel()} out of tolerance; worst at {idx}: got {got[idx].item():.6g} '
                             f'ref {ref[idx].item():.6g} (max abs err {err.max().item():.3g}, ref absmax {ref.abs().max().item():.3g})')


def i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=dev())


def ban_history(targets, L, last, filler):
    """An id row of length L that ends in ``last`` and holds the pair (last, t) for every t of ``targets``: the 2-gram rule bans
    exactly ``targets`` (plus whatever follows ``last`` in the filler, which never contains it)."""
    body = []
    for t in targets:
        body += [last, int(t)]
    body.append(last)
    assert len(body) <= L
    return list(filler[:L - len(body)]) + body


def ref_ban(ids_rows, logits, sizes):
    """fp64 logits with the oracle's n-gram ban applied (ids_rows: (B, len) on the host)"""
    from oracle import reference_model as orc
    return orc.apply_ngram_ban(ids_rows.cpu(), logits.double().cpu().clone(), sizes)


# ------------------------------------------------------------------------------------------------------ a. ngram_ban_argmax
def _logit_buffer(x, layout):
    """x (B, V) in its kernel dtype -> (view the kernel reads, ld): rows padded to 8 (the vec4 path), an odd ld, or rows padded to
    8 behind a base pointer 4 bytes off 16-byte alignment (both scalar paths)"""
    B, V = x.shape
    ld = {'pad8': (V + 7) // 8 * 8, 'odd': V | 1 if V % 2 == 0 else V + 2, 'offset': (V + 7) // 8 * 8}[layout]
    skip = (4 // x.element_size()) if layout == 'offset' else 0
    buf = torch.full((B * ld + skip + 8,), float('nan'), dtype=x.dtype, device=dev())
    view = buf[skip:skip + B * ld].view(B, ld)
    view[:, :V] = x.to(dev())
    return view, ld


def _run_ban_argmax(ops, logits, layout, rows, sizes, cur=None):
    """one i2t_ngram_ban_argmax call; -> (tokens, margins, reference fp64 banned logits)"""
    B, V = logits.shape
    L = rows.shape[1]
    cur = L if cur is None else cur
    view, ld = _logit_buffer(logits, layout)
    ids = torch.full((B, L + 2), -7, dtype=torch.long, device=dev())
    ids[:, :L] = rows.to(dev())
    before = ids.clone()
    margin = torch.full((B,), float('nan'), device=dev())
    ops.ngram_ban_argmax(view, ld, ids, L + 2, i32([cur]), i32(sizes), len(sizes), B, V, margin)
    assert torch.equal(ids[:, :cur], before[:, :cur]) and torch.equal(ids[:, cur + 1:], before[:, cur + 1:])
    ref = ref_ban(rows[:, :cur], logits.float(), sizes)
    return ids[:, cur].cpu(), margin.cpu(), ref


def _check_ban_argmax(tag, tok, margin, ref):
    want = ref.argmax(-1)
    assert torch.equal(tok, want), f'{tag}: tokens {tok.tolist()} vs {want.tolist()}'
    t2 = torch.topk(ref, 2, dim=-1).values
    check(f'{tag} margin', margin, t2[:, 0] - t2[:, 1], 1e-6, 1e-6)


@pytest.mark.parametrize('layout', ['pad8', 'odd', 'offset'])
@pytest.mark.parametrize('V', [384, 32000, 50257, 65024, 151936])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_ngram_ban_argmax_shapes(ops, dtype, V, layout):
    """ties across lanes / waves (lowest column wins), the top 1 ... 50 columns banned, n-gram sizes with 1 and sizes past len + 1"""
    B, L = 8, 128
    g = gen(V + (dtype == BF16))
    x = (torch.randn(B, V, generator=g) * 2).to(dtype)
    # rows 0 / 1: an exact tie at the row maximum between columns in different lanes and waves of both scan forms (row 1: the
    # lowest member is banned, the next one must win)
    ties = sorted({7, 65, V // 7 + 1, V // 2 + 3, V - 2, (V - 2) // 4 * 4 + 1})
    for r in (0, 1):
        x[r, ties] = (x[r].float().max() + 1).to(dtype)
    order = torch.argsort(x.float(), dim=-1, descending=True, stable=True)
    hist = []
    for r in range(B):
        alphabet = order[r, V - 60:]                       # the row's 60 lowest columns: none of its top 50, nor a tie member
        last = int(alphabet[0])
        filler = [int(t) for t in alphabet[1 + torch.randint(0, 59, (L,), generator=g)]]
        targets = {1: [ties[0]], 2: [], 3: order[r, :1], 4: order[r, :3], 5: order[r, :10], 6: order[r, :25], 7: order[r, :50]}.get(r, [])
        hist.append(ban_history([int(t) for t in targets if int(t) != last], L, last, filler))
    rows = torch.tensor(hist, dtype=torch.long)
    for sizes in ((2,), (2, 3, 4), (1, 2), (3, L, L + 1, L + 2), (1, L + 5)):
        tok, margin, ref = _run_ban_argmax(ops, x, layout, rows, sizes)
        _check_ban_argmax(f'{dtype} V={V} {layout} sizes={sizes}', tok, margin, ref)
        if sizes == (2,):
            assert int(tok[0]) == ties[0] and int(tok[1]) == ties[1]
            banned = torch.isinf(ref) & (ref < 0)
            for r, m in ((3, 1), (4, 3), (5, 10), (6, 25), (7, 50)):
                assert bool(banned[r, order[r, :m]].all()), (r, m)
    for cur in (1, 2):                                     # sizes past len + 1 are skipped, n = len + 1 has no candidate
        tok, margin, ref = _run_ban_argmax(ops, x, layout, rows, (1, 2, 3, 4), cur=cur)
        _check_ban_argmax(f'{dtype} V={V} {layout} cur={cur}', tok, margin, ref)


@pytest.mark.parametrize('sizes', [(1, 2, 3), (3, 2, 1)])
@pytest.mark.parametrize('V', [50257, 151936])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_ngram_ban_argmax_many_matches(ops, dtype, V, sizes):
    """A ~1000-token history over an almost constant alphabet: well over 1024 n-gram matches (duplicates included).  200 distinct
    tokens, each banned by exactly one match (the 1-gram rule), hold the 200 highest logits: un-banning any of them changes the
    argmax, whichever matches a capped list would have dropped."""
    B, L = 3, 1001
    g = gen(V + 11 * (dtype == BF16) + sizes[0])
    x = torch.randn(B, V, generator=g).to(dtype)
    rows = []
    for r in range(B):
        perm = torch.randperm(V, generator=g)
        f, gg, D = int(perm[0]), int(perm[1]), [int(t) for t in perm[2:202]]
        body = []
        for t in D:                                        # g d f f f: g (never f) before every d, so only the 1-gram rule bans d
            body += [gg, t, f, f, f]
        row = body + [f]
        assert len(row) == L
        rows.append(row)
        top = torch.linspace(20, 10, len(D))
        x[r, D] = top.to(dtype)
        x[r, [f, gg]] = torch.tensor([30.0, 25.0]).to(dtype)   # banned too (1- and 2-gram rules)
    rows = torch.tensor(rows, dtype=torch.long)
    from oracle import reference_model as orc
    assert sum(len(orc.banned_next_tokens(rows[0].tolist(), n)) for n in sizes) > 1800
    for layout in ('pad8', 'odd'):
        tok, margin, ref = _run_ban_argmax(ops, x, layout, rows, sizes)
        assert bool((ref.max(-1).values < 10).all())       # the fp64 winner is none of the 202 banned ones
        _check_ban_argmax(f'{dtype} V={V} {layout} sizes={sizes}', tok, margin, ref)


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('V', [37, 384])
def test_ngram_ban_argmax_all_banned(ops, dtype, V):
    """every column banned (1-gram rule over a history holding all V ids): token 0 (torch.argmax of a row of -inf), margin 0"""
    B = 3
    g = gen(V)
    rows = torch.stack([torch.cat([torch.randperm(V, generator=g), torch.randperm(V, generator=g)]) for _ in range(B)])
    x = torch.randn(B, V, generator=g).to(dtype)
    for layout in ('pad8', 'odd', 'offset'):
        tok, margin, ref = _run_ban_argmax(ops, x, layout, rows, (1, 2))
        assert bool(torch.isinf(ref).all()) and torch.equal(ref.argmax(-1), torch.zeros(B, dtype=torch.long))
        assert torch.equal(tok, torch.zeros(B, dtype=torch.long)), tok.tolist()
        assert torch.equal(margin, torch.zeros(B)), margin.tolist()


# ------------------------------------------------------------------------------------------------------ b. gemm_top2 + top2 argmax
@pytest.mark.parametrize('V,d', [(50257, 768), (32000, 4096), (151936, 1536), (64 * 700 + 1, 256)])
def test_top2_ngram_argmax_shapes(ops, V, d):
    """Segment maxima bit-exact against a stable sort of the fp32 logits; the token against the fp64 argmax of the banned logits.
    Rows 0 .. nr-1 are built so that 100 - 300 segments have BOTH leaders banned (each such row gets its own planted columns:
    head rows kappa * e_r, hidden row 4 * e_r + noise), with the true winner in the highest-numbered one of them.  96 rows: the
    logits form of the lm_head takes its skinny path (another summation order) at 64 rows and fewer."""
    B = 96
    nseg = (V + 63) // 64
    Vp = nseg * 64
    g = torch.Generator(device=dev()).manual_seed(V + d)
    nr = min(4, (nseg - 1) // 100)
    per = [min(300, 100 + 60 * r, (nseg - 1) // nr) for r in range(nr)]
    W = torch.randn(V, d, generator=g, device=dev()) * (0.7 / math.sqrt(d))
    hid = torch.randn(B, d, generator=g, device=dev())
    hid[:, :nr] = 0
    segs = torch.randperm(nseg - 1, generator=gen(V))   # the last (partial) segment is never planted
    gh = gen(V + 1)
    R, winner_seg = [], []
    for r in range(nr):
        hid[r, r] = 4.0
        Rr = sorted(int(s) for s in segs[sum(per[:r]):sum(per[:r + 1])])
        R.append(set(Rr))
        winner_seg.append(Rr[-1])
        for s in Rr:
            cols = s * 64 + torch.randperm(64, generator=gh)[:3]
            k3 = 2.0 if s == Rr[-1] else 1.5 + 0.25 * float(torch.rand(1, generator=gh))
            for c, k in zip(cols.tolist(), (3.0, 2.75, k3)):
                W[c] *= 0.1
                W[c, r] = k
    W, hid = W.to(BF16), hid.to(BF16)
    # the logits form and its stable per-segment sort
    logits = torch.zeros(B, Vp, device=dev())
    ops.gemm(hid, W, logits, B, V, d)
    top2 = torch.zeros(B, nseg, 4, device=dev())
    ops.gemm_top2(hid, W, top2, B, V, d)
    lg = torch.full((B, Vp), float('-inf'), device=dev())
    lg[:, :V] = logits[:, :V]
    v, i = lg.view(B, -1, 64).sort(dim=-1, descending=True, stable=True)
    assert torch.equal(top2[..., 0], v[..., 0]) and torch.equal(top2[..., 2], v[..., 1])
    cols = i + (torch.arange(nseg, device=dev()) * 64)[None, :, None]
    assert torch.equal(top2[..., 1].contiguous().view(torch.int32), cols[..., 0].int())
    assert torch.equal(top2[:, :-1, 3].contiguous().view(torch.int32), cols[:, :-1, 1].int())
    # histories: planted rows ban the two leaders of every planted segment through the 1-gram rule; the other rows draw from a
    # 40-token alphabet (many repeated 2- and 3-grams)
    L = 2 * max(per) + 1 if nr else 64
    sizes = (1, 2, 3)
    rows = []
    for r in range(B):
        if r < nr:
            lead = [int(cols[r, s, k]) for s in sorted(R[r]) for k in (0, 1)]
            rows.append((lead * (L // len(lead) + 1))[:L])
        else:                                              # the row's 20 best columns among them: one or both leaders banned
            alpha = torch.cat([logits[r, :V].topk(20).indices.cpu(), torch.randperm(V, generator=gen(V + r))[:20]])
            rows.append(alpha[torch.randint(0, 40, (L,), generator=gen(r))].tolist())
    rows = torch.tensor(rows, dtype=torch.long)
    ids = torch.full((B, L + 1), -7, dtype=torch.long, device=dev())
    ids[:, :L] = rows.to(dev())
    ops.top2_ngram_argmax(top2, hid, W, ids, L + 1, i32([L]), i32(sizes), len(sizes), B, V, d)
    got = ids[:, L].cpu()
    assert torch.equal(ids[:, :L].cpu(), rows)
    ref = ref_ban(rows, (hid.double() @ W.double().t()), sizes)
    want = ref.argmax(-1)
    t2 = torch.topk(ref, 2, dim=-1).values
    clear = (t2[:, 0] - t2[:, 1]) > 1e-4 * ref.masked_fill(torch.isinf(ref), 0).abs().amax(-1)
    print(f'V={V} d={d}: {int((~clear).sum())} of {B} rows within the near-tie gap; redo segments per planted row {per}')
    assert bool(clear[:nr].all())
    bad = (got != want) & clear
    assert not bool(bad.any()), f'rows {bad.nonzero().flatten().tolist()}: got {got[bad].tolist()} want {want[bad].tolist()}'
    banned = torch.zeros(B, Vp, dtype=torch.bool)
    banned[:, :V] = torch.isinf(ref) & (ref < 0)
    for r in range(nr):                                    # the construction: both leaders banned in exactly the planted segments
        both = banned[r, cols[r, :, 0].cpu()] & banned[r, cols[r, :, 1].cpu()] & torch.isfinite(top2[r, :, 2].cpu())
        assert set(both.nonzero().flatten().tolist()) == R[r] and int(want[r]) // 64 == winner_seg[r]


def test_top2_ngram_argmax_all_banned(ops):
    """every column banned: token 0"""
    B, V, d = 2, 1000, 128
    hid, W = rnd(B, d, dtype=BF16, seed=1), rnd(V, d, dtype=BF16, seed=2)
    nseg = (V + 63) // 64
    top2 = torch.zeros(B, nseg, 4, device=dev())
    ops.gemm_top2(hid, W, top2, B, V, d)
    rows = torch.stack([torch.randperm(V, generator=gen(b)) for b in range(B)])
    ids = torch.full((B, V + 1), 5, dtype=torch.long, device=dev())
    ids[:, :V] = rows.to(dev())
    ops.top2_ngram_argmax(top2, hid, W, ids, V + 1, i32([V]), i32((1,)), 1, B, V, d)
    assert torch.equal(ids[:, V].cpu(), torch.zeros(B, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------ c. sample_token
SEED = (0x2345_6789 << 32) | 0x1357_9BDF


def _sample(ops, x, rows, sizes, V, **kw):
    """one i2t_sample_token call with dist_out -> (tokens, dist)"""
    B, L = rows.shape
    ids = torch.full((B, L + 1), -7, dtype=torch.long, device=dev())
    ids[:, :L] = rows.to(dev())
    ld = (V + 7) // 8 * 8
    buf = torch.zeros(B, ld, device=dev())
    buf[:, :V] = x.to(dev())
    dist = torch.full((B, V), float('nan'), device=dev())
    seed = torch.tensor([SEED & 0xFFFFFFFF, SEED >> 32], dtype=torch.int32, device=dev())
    ops.sample_token(buf, ld, ids, L + 1, i32([L]), i32(sizes), len(sizes), B, V, kw.get('temperature', 1.0), kw.get('top_k'),
                     kw.get('nucleus_p'), seed, dist_out=dist)
    assert torch.equal(ids[:, :L].cpu(), rows)
    return ids[:, L].cpu(), dist.cpu()


def _check_sample(tag, x, rows, sizes, tok, dist, **kw):
    from image2text_amd import rng
    from oracle import reference_model as orc
    want = orc.sampling_distribution(x, rows, sizes, **kw)
    got = dist.numpy()
    w = want.numpy()
    diff = (got > 0) != (w > 0)
    assert diff.sum(axis=1).max() <= 1, (tag, diff.sum(axis=1))       # at most one entry per row within float noise of the cut
    assert np.abs(got - w)[~diff].max() <= 1e-5 + 1e-3 * w.max(), (tag, float(np.abs(got - w)[~diff].max()))
    L = rows.shape[1]
    u = torch.tensor([rng.sample_uniform(SEED, L, b) for b in range(rows.shape[0])], dtype=torch.float64)
    ref_tok = orc.inverse_cdf_token(want, u)
    cdf = torch.cumsum(want.double(), -1)
    near = ((cdf / cdf[:, -1:] - u[:, None]).abs() < 1e-5).any(-1) | torch.from_numpy(diff.any(1))
    assert bool(((tok == ref_tok) | near).all()), (tag, tok.tolist(), ref_tok.tolist())
    assert int((~near).sum()) >= 1, tag
    return want


SAMPLE_MODES = {'plain': dict(), 'temperature': dict(temperature=0.7), 'top_k': dict(top_k=40, temperature=1.3),
                'nucleus': dict(nucleus_p=0.8), 'top_k+nucleus': dict(top_k=200, nucleus_p=0.6, temperature=0.9)}


@pytest.mark.parametrize('V', [1000, 1024, 1025, 8192, 8193, 32000, 32769, 50257, 51201, 65024, 65536])
def test_sample_token_widths(ops, V):
    """every template width (EPT 2 / 16 / 64 / 100 / 128) and both sides of each boundary, every filter mode, with banned tokens
    among the top-k"""
    B, L, sizes = 4, 64, (2, 3)
    g = gen(V)
    x = torch.randn(B, V, generator=g) * 3
    order = torch.argsort(x, -1, descending=True)
    rows = []
    for r in range(B):
        last = int(order[r, -1])
        filler = torch.randint(0, V, (L,), generator=g).tolist()
        rows.append(ban_history([int(t) for t in order[r, r:r + 8 * (r + 1):r + 1]], L, last, [t for t in filler if t != last] * 2))
    rows = torch.tensor(rows, dtype=torch.long)
    for tag, kw in SAMPLE_MODES.items():
        tok, dist = _sample(ops, x, rows, sizes, V, **kw)
        want = _check_sample(f'V={V} {tag}', x, rows, sizes, tok, dist, **kw)
        assert bool((want[torch.arange(B)[:, None], rows[:, -8:-1:2]] == 0).all())      # banned ids inside the top-k stay out


@pytest.mark.parametrize('V', [8193, 50257, 65024])
def test_sample_token_ties(ops, V):
    """(1) top-k whose k-th value is shared by several columns: all of them stay; (2) a nucleus cut inside a group of exactly equal
    probabilities (the boundary-group branch): the group's members sit in one lane across slots, in several waves and, where V
    allows, above column 32768; exactly the oracle's number of members is kept, every kept one from the group, all equal."""
    from image2text_amd import rng
    from oracle import reference_model as orc
    B, L = 2, 8
    g = gen(V)
    rows = torch.zeros(B, L, dtype=torch.long)
    # (1)
    x = torch.randn(B, V, generator=g)
    order = torch.argsort(x, -1, descending=True)
    k = 10
    for r in range(B):
        x[r, order[r, k - 3:k + 4]] = float(x[r, order[r, k - 3]])               # 7 columns share the k-th value
    kw = dict(top_k=k)
    tok, dist = _sample(ops, x, rows, (), V, **kw)
    want = _check_sample(f'V={V} top-k ties', x, rows, (), tok, dist, **kw)
    assert bool(((dist > 0).sum(-1) == k + 4).all()) and bool(((want > 0).sum(-1) == k + 4).all())
    # (2)
    ST = 512
    lanes = [(5, s) for s in (0, 3, 10, 12, 40, 70, 90, 120)] + [(199, 1), (199, 65), (300, 2), (450, 15), (477, 80), (511, 64)]
    group = sorted({s * ST + t for t, s in lanes if s * ST + t < V})
    assert len(group) >= 6 and (V < 32768 + ST or max(group) >= 32768)
    x = torch.randn(B, V, generator=g) * 0.5 - 6
    hi = [11, 257, V - 3]
    x[:, hi] = torch.tensor([5.0, 4.5, 4.0])
    x[:, group] = 3.0
    p = torch.softmax(x.double(), -1)[0]
    m_hi, q = float(p[hi].sum()), float(p[group[0]])
    for c in (1, 3, len(group) - 2):
        nucleus_p = m_hi + (c + 0.5) * q
        kw = dict(nucleus_p=nucleus_p)
        want = orc.sampling_distribution(x, rows, (), **kw)
        assert bool(((want > 0).sum(-1) == len(hi) + c).all())
        tok, dist = _sample(ops, x, rows, (), V, **kw)
        kept = dist > 0
        other = torch.ones(V, dtype=torch.bool)
        other[group] = False                               # outside the group: the oracle's kept set and probabilities
        assert torch.equal(kept[:, other], (want > 0)[:, other])
        check(f'V={V} nucleus tie c={c}', dist[:, other], want[:, other], 1e-5, 1e-3)
        u = torch.tensor([rng.sample_uniform(SEED, L, b) for b in range(B)], dtype=torch.float64)
        assert torch.equal(tok, orc.inverse_cdf_token(dist, u))     # the draw over the kernel's own kept set
        assert bool((kept.sum(-1) == len(hi) + c).all()), kept.sum(-1).tolist()
        assert bool(kept[:, hi].all()) and bool((kept[:, group].sum(-1) == c).all())
        gk = dist[:, group][kept[:, group]].view(B, c)
        assert torch.equal(gk, gk[:, :1].expand(B, c))
        check(f'V={V} nucleus tie c={c} kept mass', dist[:, group].sum(-1), want[:, group].sum(-1).double(), 1e-6, 1e-5)


def test_sample_token_refuses_large_vocab(ops):
    """V = 65537 is past the register-resident row: the host check refuses it (nothing is launched)"""
    from image2text_amd.lib import I2TError
    V = 65537
    x = torch.zeros(1, V + 7, device=dev())
    ids = torch.zeros(1, 4, dtype=torch.long, device=dev())
    seed = torch.zeros(2, dtype=torch.int32, device=dev())
    with pytest.raises(I2TError, match='exceeds the register-resident row'):
        ops.sample_token(x, V + 7, ids, 4, i32([2]), i32(()), 0, 1, V, 1.0, None, None, seed)
    torch.cuda.synchronize()
    assert bool((ids == 0).all())


# ------------------------------------------------------------------------------------------------------ d. decode_attention
KEY_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 129, 197, 511, 1000, 1024]


def ref_attn(q, k, v, scale, G=1):
    """q (B, H, hd), k / v (B, n, Hkv, hd) -> fp64 (B, H, hd); query head h reads key/value head h // G"""
    q, k, v = q.double(), k.double().repeat_interleave(G, dim=2), v.double().repeat_interleave(G, dim=2)
    s = torch.einsum('bhe,bnhe->bhn', q, k) * scale
    return torch.einsum('bhn,bnhe->bhe', torch.softmax(s, -1), v)


@pytest.mark.parametrize('head_major', [False, True])
@pytest.mark.parametrize('H', [1, 3, 12, 16])
def test_decode_attention_key_counts(ops, H, head_major):
    B, T = 2, 1024
    d = 64 * H
    kt, vt = rnd(B, T, H, 64, dtype=BF16, seed=10 + H), rnd(B, T, H, 64, dtype=BF16, seed=20 + H)

    def cache(t):                                          # token-major [B][T][H][64] or head-major [B][H][T][64]
        return t.permute(0, 2, 1, 3).contiguous() if head_major else t.clone()

    def tok_view(c):
        return c.permute(0, 2, 1, 3) if head_major else c

    rs, hs = (64, T * 64) if head_major else (d, 64)
    o = torch.empty(B, d, dtype=BF16, device=dev())
    for qscale, tag in ((8.0, 'one-hot'), (0.0, 'flat'), (1.0, 'mixed')):
        for n in KEY_COUNTS:
            qkv = rnd(B, 3 * d, dtype=BF16, seed=1000 * n + H)
            qkv[:, :d] = (qkv[:, :d].float() * qscale).to(BF16)
            q = qkv[:, :d].view(B, H, 64)
            # appended through pos_ptr: slot n - 1 written by the launch, attended to with keys 0 .. n - 2
            kc, vc = cache(kt), cache(vt)
            pos = i32([n - 1])
            ops.decode_attention(qkv, 3 * d, kc, vc, T * d, rs, o, d, pos, 0, B, H, append_dm=d, cache_hs=hs)
            ke, ve = kt.clone(), vt.clone()
            ke[:, n - 1], ve[:, n - 1] = qkv[:, d:2 * d].view(B, H, 64), qkv[:, 2 * d:].view(B, H, 64)
            assert torch.equal(tok_view(kc), ke) and torch.equal(tok_view(vc), ve), f'append n={n}: the cache differs'
            check(f'append H={H} n={n} {tag}', o.view(B, H, 64), ref_attn(q, ke[:, :n], ve[:, :n], 0.125), 1e-4, 1 / 200)
            if n == 1:
                assert torch.equal(o.view(B, H, 64), ve[:, 0])
            # cached through pos_ptr, and a fixed key count
            kc, vc = cache(kt), cache(vt)
            want = ref_attn(q, kt[:, :n], vt[:, :n], 0.125)
            ops.decode_attention(qkv, 3 * d, kc, vc, T * d, rs, o, d, pos, 0, B, H, cache_hs=hs)
            check(f'cached H={H} n={n} {tag}', o.view(B, H, 64), want, 1e-4, 1 / 200)
            o2 = torch.empty_like(o)
            ops.decode_attention(qkv, 3 * d, kc, vc, T * d, rs, o2, d, None, n, B, H, cache_hs=hs)
            assert torch.equal(o2, o), f'fixed H={H} n={n}'
            assert torch.equal(tok_view(kc), kt) and torch.equal(tok_view(vc), vt)


def test_kv_append(ops):
    B, H, T = 3, 12, 40
    d = 64 * H
    kc, vc = rnd(B, T, d, dtype=BF16, seed=1), rnd(B, T, d, dtype=BF16, seed=2)
    for p in (0, 17, T - 1):
        qkv = rnd(B, 3 * d, dtype=BF16, seed=3 + p)
        ke, ve = kc.clone(), vc.clone()
        ke[:, p], ve[:, p] = qkv[:, d:2 * d], qkv[:, 2 * d:]
        ops.kv_append(qkv, 3 * d, kc, vc, T * d, d, i32([p]), B, d)
        assert torch.equal(kc, ke) and torch.equal(vc, ve), p


# ------------------------------------------------------------------------------------------------------ e. gq_decode_attention
@pytest.mark.parametrize('H,Hkv', [(4, 4), (12, 2), (32, 32), (71, 1)])
@pytest.mark.parametrize('hd', [16, 32, 64, 128])
def test_gq_decode_attention(ops, hd, H, Hkv):
    B, T = 2, 1024
    G = H // Hkv
    w = Hkv * hd
    kpp = 64 // (hd // 8)
    scale = hd ** -0.5
    kt, vt = rnd(B, T, Hkv, hd, dtype=BF16, seed=hd + H), rnd(B, T, Hkv, hd, dtype=BF16, seed=2 * hd + H)
    out = torch.empty(B, H * hd, dtype=BF16, device=dev())
    for n in sorted({1, kpp - 1, kpp, kpp + 1, 2 * kpp + 1, 1024} - {0}):
        q = rnd(B, H * hd, dtype=BF16, seed=n, scale=2.0)
        kvn = rnd(B, 2 * w, dtype=BF16, seed=n + 1)
        kc, vc = kt.clone(), vt.clone()
        ops.gq_decode_attention(q, kvn[:, :w], kvn[:, w:], kc, vc, T * w, w, out, i32([n - 1]), 0, T, B, H, Hkv, hd)
        ke, ve = kt.clone(), vt.clone()
        ke[:, n - 1], ve[:, n - 1] = kvn[:, :w].view(B, Hkv, hd), kvn[:, w:].view(B, Hkv, hd)
        assert torch.equal(kc, ke) and torch.equal(vc, ve), f'append n={n}: the cache differs'
        check(f'gq append hd={hd} H={H}/{Hkv} n={n}', out.view(B, H, hd), ref_attn(q.view(B, H, hd), ke[:, :n], ve[:, :n], scale, G),
              1e-4, 1 / 200)
        ops.gq_decode_attention(q, None, None, kc, vc, T * w, w, out, i32([n - 1]), 0, T, B, H, Hkv, hd)
        check(f'gq cached hd={hd} H={H}/{Hkv} n={n}', out.view(B, H, hd), ref_attn(q.view(B, H, hd), ke[:, :n], ve[:, :n], scale, G),
              1e-4, 1 / 200)
    # the decoder's cross form: K and V interleaved in one row of 2 * Hkv * hd, a fixed memory of S keys
    for S in (64, 197):
        kv = rnd(B, S, 2 * w, dtype=BF16, seed=S + hd)
        q = rnd(B, H * hd, dtype=BF16, seed=S)
        ops.gq_decode_attention(q, None, None, kv, kv.view(-1)[w:], S * 2 * w, 2 * w, out, None, S, S, B, H, Hkv, hd)
        want = ref_attn(q.view(B, H, hd), kv[..., :w].reshape(B, S, Hkv, hd), kv[..., w:].reshape(B, S, Hkv, hd), scale, G)
        check(f'gq cross hd={hd} H={H}/{Hkv} S={S}', out.view(B, H, hd), want, 1e-4, 1 / 200)


# ------------------------------------------------------------------------------------------------------ f. embed_step
def test_embed_step(ops):
    B, V, d, P = 5, 1000, 768, 300
    wte, wpe = rnd(V, d, seed=1), rnd(P, d, seed=2)
    ln = 9
    ids = torch.randint(0, V, (B, 16), generator=gen(3)).to(dev())
    ids[:, ln - 1] = torch.tensor([0, V - 1, -5, V + 7, 123], device=dev())
    want_id = torch.tensor([0, V - 1, 0, V - 1, 123], device=dev())
    x = torch.full((B, d), float('nan'), device=dev())
    for off, pe in ((0, wpe), (17, wpe), (5, None)):
        ops.embed_step(ids, 16, i32([ln]), wte, pe, x, B, d, off, V)
        want = wte[want_id] + pe[ln - 1 + off] if pe is not None else wte[want_id]
        assert torch.equal(x, want), (off, pe is None)


# ------------------------------------------------------------------------------------------------------ g. operand refusal
def test_select_rows_refuses_an_int64_flag(ops):
    """flag is an int* of i2t_select_rows: an int64 device tensor is refused on the host, by dtype, and nothing is launched"""
    from image2text_amd.lib import I2TError
    a, b = torch.arange(4., device=dev()), -torch.arange(4., device=dev())
    out = torch.tensor([float('nan'), -0.0, 3e38, 1e-45], device=dev())
    before = out.clone().view(torch.int32)
    with pytest.raises(I2TError, match=r'i2t_select_rows.*torch\.int32.*torch\.int64'):
        ops.select_rows(torch.ones(1, dtype=torch.int64, device=dev()), a, b, out, 4)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before)
