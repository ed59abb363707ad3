"""i2t_trie_level_expand_sets, directly through ops.trie_level_expand_sets, on the MI355X.

Shapes: B = 3 images of W = 70 rows in three different states in ONE launch -- image 0 in a forced prompt column, image 1 at level 1
of a 1 -> 5 -> 70 set (70 child waves, 2 terminal rows that end 1 and 3 phrases), image 2 at the terminal level of a second set (no
children; 2 terminal rows that end 1 and 3 duplicates) --; V in {70, 257, 50257}; the bf16 form at d in {64, 128} (scale 1 and 0.5)
and the fp32-logits form (ld = V rounded up to 64 columns, the pad columns holding 1e30); Kmax = 9 in logprob rows of 12 columns.

Expectation: the ids cells equal; path_out and logprob BIT-equal to the fp32 restatement path_in[p] + (z - lse[p]) in numpy, fed the
kernel's own z -- read back from a launch with zero path sums and zero lse, as tests/test_trie_expand_gpu.py does --, the forced
image's rows path_out = path_in and its prompt token in every one of its W rows; with one set and every image at one level every
output buffer bit-equal to i2t_trie_level_expand on the same inputs; NaN / -7 guards around every buffer and every cell the state does
not name untouched; the input path buffer unchanged; two launches bit-equal; a finished image's logprob, path and id rows untouched;
every refusal -- the entry point's and the host checks' of what it cannot read -- an error that writes nothing."""
import types

import numpy as np
import pytest
import torch

from test_logits_processors_gpu import PAD_VALUE, bits, guarded, pad64

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
B, W, KMAX, LP_LD, IDS_LD, COL = 3, 70, 9, 12, 8, 5
R = B * W
R_PAD = (R + 3) // 4 * 4
VS = (70, 257, 50257)
FORMS = (('logits', 0, 1.0), ('bf16', 64, 1.0), ('bf16', 128, 0.5))
FORCED_TOK = 11


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


_DATA = {}


def data(V, form, d):
    """the operands of one (vocabulary, form): built once, never changed.  Segments: 0 = set X level 0 (1 -> 5), 1 = set X level 1
    (5 -> 70, rows 1 and 3 end phrases [2] and [0 5 7]), 2 = set Y's last level (rows 0 and 2 end phrases [1] and [3 4 6])."""
    key = (V, form, d)
    if key in _DATA:
        return _DATA[key]
    g = torch.Generator().manual_seed(V * 11 + d)
    rng = np.random.default_rng(V + d + 1)
    eos = V - 3
    toks = np.setdiff1d(np.arange(V), [eos])
    tok0, tok1 = rng.choice(toks, 5, replace=False), rng.choice(toks, W, replace=V < 2 * W)
    tabs = types.SimpleNamespace(
        child_parent=np.concatenate([np.zeros(5, dtype=np.int64), np.arange(W) % 5]), child_tok=np.concatenate([tok0, tok1]),
        term_row=np.array([1, 3, 0, 2]), term_off=np.array([0, 0, 1, 4, 4, 5, 8]), term_phrase=np.array([2, 0, 5, 7, 1, 3, 4, 6]),
        child_at=np.array([0, 5, 5 + W]), n_child=np.array([5, W, 0]), term_at=np.array([0, 0, 2]), n_term=np.array([0, 2, 2]),
        off_at=np.array([0, 1, 4]), kmax=KMAX)
    c = dict(V=V, eos=eos, tabs=tabs, lse=(torch.randn(R, generator=g) + 6).to(dev()), path=(torch.randn(R, generator=g) * 3 - 4).to(dev()))
    if form == 'logits':
        ld = pad64(V)
        z = torch.randn(R, ld, generator=g) * 3
        z[:, V:] = PAD_VALUE
        c.update(ld=ld, logits=z.to(dev()))
    else:
        c.update(hidden=torch.randn(R, d, generator=g).to(BF16).to(dev()), w_head=(torch.randn(V, d, generator=g) * 0.3).to(BF16).to(dev()))
    _DATA[key] = c
    return c


def seg_state(tabs, g, level, col=COL):
    return [level, -1, int(tabs.child_at[g]), int(tabs.n_child[g]), int(tabs.term_at[g]), int(tabs.n_term[g]), int(tabs.off_at[g]), col]


def mixed_state(tabs, first):
    """image 0 forced (or, ``first`` = -1, finished), image 1 at segment 1, image 2 at segment 2"""
    return np.array([[-1, first, 0, 0, 0, 0, 0, COL], seg_state(tabs, 1, 1), seg_state(tabs, 2, 2)])


def zkw(c, form, d, scale):
    return dict(logits=c['logits'], ld=c['ld']) if form == 'logits' else dict(hidden=c['hidden'], w_head=c['w_head'], d=d, scale=scale)


def outputs():
    path_row, pbuf = guarded(1, R_PAD)                          # the row padded so that it starts on 16 bytes behind its guard row
    path_out = path_row.view(-1)[:R]
    ids, ibuf = guarded(R, IDS_LD, fill=-7, dtype=torch.long)
    logprob, lbuf = guarded(B, LP_LD)
    return (path_out, ids, logprob), (pbuf, ibuf, lbuf)


def guards_clean(pbuf, ibuf, lbuf):
    return bool(torch.isnan(pbuf[0]).all() and torch.isnan(pbuf[1, R:]).all() and torch.isnan(pbuf[2:]).all() and torch.isnan(lbuf[0]).all() and torch.isnan(lbuf[1 + B:]).all()
                and (ibuf[0] == -7).all() and (ibuf[1 + R:] == -7).all())


@pytest.mark.parametrize('form,d,scale', FORMS)
@pytest.mark.parametrize('V', VS)
def test_three_states_in_one_launch(ops, V, form, d, scale):
    c = data(V, form, d)
    tabs, eos = c['tabs'], c['eos']
    tables = ops.trie_set_tables(tabs, W, V, dev())
    state_np = mixed_state(tabs, FORCED_TOK)
    state = ops.trie_set_state(tables, state_np, W, V, IDS_LD, dev())
    assert (state.e_child, state.e_term, state.B) == (W, 2, B)
    kw = zkw(c, form, d, scale)
    zero = torch.zeros(R, device=dev())
    (z_path, _, z_lp), _ = outputs()
    ops.trie_level_expand_sets(tables, state, zero, zero.clone(), z_path, torch.zeros(R, IDS_LD, dtype=torch.long, device=dev()), IDS_LD, z_lp, eos, W, V, **kw)
    path_in = c['path'].clone()
    (path_out, ids, logprob), bufs = outputs()
    ops.trie_level_expand_sets(tables, state, c['lse'], path_in, path_out, ids, IDS_LD, logprob, eos, W, V, **kw)
    (again, again_ids, again_lp), _ = outputs()
    ops.trie_level_expand_sets(tables, state, c['lse'], path_in, again, again_ids, IDS_LD, again_lp, eos, W, V, **kw)
    torch.cuda.synchronize()
    tag = f'V {V} {form} d {d}'
    assert torch.equal(bits(path_in), bits(c['path'])), f'{tag}: the input path buffer was written'
    assert guards_clean(*bufs), f'{tag}: a guard was written'
    assert torch.equal(bits(path_out), bits(again)) and torch.equal(bits(logprob), bits(again_lp)) and torch.equal(ids, again_ids), f'{tag}: two launches differ'
    zc, zt = z_path.cpu().numpy(), z_lp.cpu().numpy()
    lse, pin = c['lse'].cpu().numpy(), c['path'].cpu().numpy()
    want_path = np.full(R, np.nan, dtype=np.float32)
    want_ids = np.full((R, IDS_LD), -7, dtype=np.int64)
    want_lp = np.full((B, LP_LD), np.nan, dtype=np.float32)
    want_path[:W], want_ids[:W, COL] = pin[:W], FORCED_TOK       # image 0: forced
    assert np.array_equal(zc[:W], np.zeros(W, dtype=np.float32)), 'a forced row copies its path sum: 0 in the z launch'
    for b in (1, 2):
        _, _, ca, nc, ta, nt, oa, _ = state_np[b].tolist()
        for j in range(nc):
            p, cell = b * W + int(tabs.child_parent[ca + j]), b * W + j
            want_path[cell] = np.float32(pin[p] + np.float32(zc[cell] - lse[p]))
            want_ids[cell, COL] = int(tabs.child_tok[ca + j])
        for j in range(nt):
            p = b * W + int(tabs.term_row[ta + j])
            mine = tabs.term_phrase[tabs.term_off[oa + j]:tabs.term_off[oa + j + 1]].tolist()
            assert len(mine) == (1, 3)[j]
            for k in mine:
                assert zt[b, k] == zt[b, mine[0]], 'the duplicates of a node share its z'
                want_lp[b, k] = np.float32(pin[p] + np.float32(zt[b, k] - lse[p]))
            if form == 'logits':
                assert zt[b, mine[0]] == float(c['logits'][p, eos]), f'{tag}: z is not the logits cell'
    if form == 'logits':
        _, _, ca, nc = state_np[1, :4].tolist()
        rows = torch.tensor([W + int(tabs.child_parent[ca + j]) for j in range(nc)])
        assert torch.equal(bits(torch.from_numpy(zc[W:W + nc].copy())), bits(c['logits'].cpu()[rows, torch.from_numpy(tabs.child_tok[ca:ca + nc])]))
    assert np.array_equal(ids.cpu().numpy(), want_ids), f'{tag}: ids'
    assert np.array_equal(path_out.cpu().numpy().view(np.int32), want_path.view(np.int32)), f'{tag}: path_out is not the fp32 restatement, bit for bit'
    assert np.array_equal(logprob.cpu().numpy().view(np.int32), want_lp.view(np.int32)), f'{tag}: logprob is not the fp32 restatement, bit for bit'
    # a finished image: nothing of its rows is written
    (f_path, f_ids, f_lp), f_bufs = outputs()
    ops.trie_level_expand_sets(tables, ops.trie_set_state(tables, mixed_state(tabs, -1), W, V, IDS_LD, dev()), c['lse'], path_in, f_path, f_ids,
                               IDS_LD, f_lp, eos, W, V, **kw)
    torch.cuda.synchronize()
    assert guards_clean(*f_bufs)
    assert torch.isnan(f_lp[0]).all() and torch.isnan(f_path[:W]).all() and bool((f_ids[:W] == -7).all()), f'{tag}: a finished image was written'
    assert torch.equal(bits(f_path[W:]), bits(path_out[W:])) and torch.equal(bits(f_lp[1:]), bits(logprob[1:])) and torch.equal(f_ids[W:], ids[W:])


@pytest.mark.parametrize('form,d,scale', FORMS)
@pytest.mark.parametrize('V', VS)
def test_one_set_one_level_equals_trie_level_expand(ops, V, form, d, scale):
    c = data(V, form, d)
    tabs, eos = c['tabs'], c['eos']
    tables = ops.trie_set_tables(tabs, W, V, dev())
    kw = zkw(c, form, d, scale)
    len_ptr = torch.tensor([COL], dtype=I32, device=dev())
    for g in (0, 1):                                            # both levels of set X, every image at the level
        ca, nc, ta, nt, oa = (int(a[g]) for a in (tabs.child_at, tabs.n_child, tabs.term_at, tabs.n_term, tabs.off_at))
        off = tabs.term_off[oa:oa + nt + 1]
        old = ops.trie_level_tables(tabs.child_parent[ca:ca + nc], tabs.child_tok[ca:ca + nc], tabs.term_row[ta:ta + nt], off - off[0],
                                    tabs.term_phrase[off[0]:off[-1]], W, V, KMAX, dev())
        path_in = c['path'].clone()
        (o_path, o_ids, o_lp), o_bufs = outputs()
        ops.trie_level_expand(old, c['lse'], path_in, o_path, o_ids, IDS_LD, len_ptr, o_lp, eos, B, W, V, **kw)
        state = ops.trie_set_state(tables, np.array([seg_state(tabs, g, g)] * B), W, V, IDS_LD, dev())
        (n_path, n_ids, n_lp), n_bufs = outputs()
        ops.trie_level_expand_sets(tables, state, c['lse'], path_in, n_path, n_ids, IDS_LD, n_lp, eos, W, V, **kw)
        torch.cuda.synchronize()
        for old_buf, new_buf in zip(o_bufs, n_bufs):
            assert torch.equal(bits(old_buf), bits(new_buf)), f'V {V} {form} d {d} segment {g}: a buffer differs from i2t_trie_level_expand, guards included'
        assert torch.equal(bits(path_in), bits(c['path']))


def test_refusals(ops):
    from image2text_amd import lib as i2tlib
    lib = i2tlib.load()
    V, d = 70, 64
    cl, cb = data(V, 'logits', 0), data(V, 'bf16', d)
    tabs = cl['tabs']
    t = ops.trie_set_tables(tabs, W, V, dev())
    st = ops.trie_set_state(t, mixed_state(tabs, FORCED_TOK), W, V, IDS_LD, dev())
    path_in = cl['path'].clone()
    (path_out, ids, logprob), bufs = outputs()
    before = [x.clone() for x in (*bufs, path_in)]
    args = dict(stream=torch.cuda.current_stream().cuda_stream, hidden=cb['hidden'].data_ptr(), ld_hidden=d, w_head=cb['w_head'].data_ptr(), ld_w=d,
                d=d, scale=1.0, logits=None, ld=0, lse=cl['lse'].data_ptr(), path_in=path_in.data_ptr(), path_out=path_out.data_ptr(),
                child_parent=t.child_parent.data_ptr(), child_tok=t.child_tok.data_ptr(), n_child_all=t.n_child_all, term_row=t.term_row.data_ptr(),
                n_term_all=t.n_term_all, term_off=t.term_off.data_ptr(), n_off_all=t.n_off_all, term_phrase=t.term_phrase.data_ptr(),
                n_term_phrases=t.n_term_phrases, image_state=st.state.data_ptr(), e_child=st.e_child, e_term=st.e_term, ids=ids.data_ptr(),
                ids_ld=IDS_LD, logprob=logprob.data_ptr(), lp_ld=LP_LD, kmax=KMAX, eos=cl['eos'], B=B, W=W, V=V)
    with_logits = {**args, 'hidden': None, 'w_head': None, 'logits': cl['logits'].data_ptr(), 'ld': cl['ld']}
    fn = 'i2t_trie_level_expand_sets'

    def refused(a, change, text):
        rc = getattr(lib, fn)(*{**a, **change}.values())
        assert rc == -1 and text in i2tlib.last_error() and fn in i2tlib.last_error(), (change, rc, i2tlib.last_error())

    for a in (args, with_logits):
        # what i2t_trie_level_expand refuses
        for name in ('lse', 'path_in', 'path_out', 'ids', 'logprob', 'child_parent', 'child_tok', 'term_row', 'term_off', 'term_phrase'):
            refused(a, {name: None}, 'null pointer')
        refused(a, dict(n_child_all=-1), 'n_child_all = -1')
        refused(a, dict(n_term_all=-1), 'n_term_all = -1')
        refused(a, dict(eos=V), f'eos = {V}')
        refused(a, dict(eos=-1), 'eos = -1')
        refused(a, dict(B=0), 'B = 0')
        refused(a, dict(path_out=a['path_in']), 'one buffer')
        for name in ('lse', 'path_in', 'path_out', 'child_parent', 'child_tok', 'term_row', 'term_off', 'term_phrase', 'logprob'):
            refused(a, {name: a[name] + 4}, 'misaligned')
        refused(a, dict(ids=a['ids'] + 8), 'misaligned')
        # its own
        refused(a, dict(image_state=None), 'null image_state')
        refused(a, dict(image_state=a['image_state'] + 4), 'misaligned image_state')
        refused(a, dict(kmax=0), 'kmax = 0')
        refused(a, dict(kmax=LP_LD + 1), f'kmax = {LP_LD + 1}')
        refused(a, dict(e_child=W + 1), f'e_child = {W + 1}')
        refused(a, dict(e_term=-1), 'e_term = -1')
        refused(a, dict(n_off_all=t.n_term_all), f'n_off_all = {t.n_term_all}')
    refused(args, dict(hidden=None), 'null pointer')
    refused(args, dict(w_head=None), 'null pointer')
    refused(args, dict(d=60), 'd = 60')
    refused(args, dict(ld_hidden=d - 8), 'd = 64')
    refused(args, dict(hidden=args['hidden'] + 2), 'misaligned')
    refused(args, dict(scale=float('inf')), 'scale must be finite')
    refused(with_logits, dict(ld=V - 2), 'ld = 68')
    refused(with_logits, dict(ld=V + 1), 'ld = 71')
    refused(with_logits, dict(logits=with_logits['logits'] + 4), 'misaligned')
    # what the entry point cannot read is refused on the host before upload: the tables ...
    def changed(**kw):
        return types.SimpleNamespace(**{**vars(tabs), **kw})
    for kw, text in ((dict(child_parent=np.concatenate([[W], tabs.child_parent[1:]])), 'a parent row outside'),
                     (dict(child_tok=np.concatenate([[V], tabs.child_tok[1:]])), 'a token outside'),
                     (dict(term_row=np.array([1, W, 0, 2])), 'a terminal row outside'),
                     (dict(term_off=np.array([0, 0, 5, 4, 4, 5, 8])), 'segment 1: term_off does not ascend'),
                     (dict(term_off=np.array([0, 0, 1, 4, 4, 5, 9])), 'segment 2: term_off does not ascend'),
                     (dict(term_phrase=np.array([2, 0, 5, 7, 1, 3, 4, KMAX])), 'a phrase index outside'),
                     (dict(child_at=np.array([0, 5, 6 + W])), 'segment 2 lies outside'), (dict(n_term=np.array([0, 2, 3])), 'segment 2 lies outside'),
                     (dict(kmax=0), 'kmax = 0')):
        with pytest.raises(i2tlib.I2TError, match=text):
            ops.trie_set_tables(changed(**kw), W, V, dev())
    with pytest.raises(i2tlib.I2TError, match='exceed the W = 4 rows'):
        ops.trie_set_tables(tabs, 4, V, dev())
    # ... and every image's level and offsets
    good = mixed_state(tabs, FORCED_TOK)
    for (b, at), value, text in (((0, 0), -2, 'a level below -1'), ((0, 1), V, 'a forced token outside'), ((1, 2), t.n_child_all, 'table ranges lie outside'),
                                 ((1, 3), W + 1, 'table ranges lie outside'), ((2, 4), 3, 'table ranges lie outside'), ((2, 6), 5, 'table ranges lie outside'),
                                 ((1, 2), -1, 'table ranges lie outside'), ((2, 7), IDS_LD, 'an id column outside'), ((0, 7), -1, 'an id column outside')):
        bad = good.copy()
        bad[b, at] = value
        with pytest.raises(i2tlib.I2TError, match=text):
            ops.trie_set_state(t, bad, W, V, IDS_LD, dev())
    with pytest.raises(i2tlib.I2TError, match='8 integers per image'):
        ops.trie_set_state(t, good[:, :7], W, V, IDS_LD, dev())
    with pytest.raises(i2tlib.I2TError, match='one buffer'):
        ops.trie_level_expand_sets(t, st, cl['lse'], path_in, path_in, ids, IDS_LD, logprob, cl['eos'], W, V, logits=cl['logits'], ld=cl['ld'])
    torch.cuda.synchronize()
    for x, y in zip(before, (*bufs, path_in)):
        assert torch.equal(bits(x), bits(y)), 'a refused call wrote something'
