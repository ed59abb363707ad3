"""The two kernels of score_phrases, directly through ops.trie_level_expand and ops.rows_lse, on the MI355X.

Shapes: B = 2 images of W = 70 rows; V in {70, 257, 50257}; the bf16 form at d in {64, 128} (scale 1 and 0.5) and the fp32-logits form
(ld = V rounded up to 64 columns, the pad columns holding 1e30).  Two levels: 1 -> 5 rows (one workgroup) and 5 -> 70 rows (140 child
waves and 4 terminal waves: 36 workgroups), the second with two terminal rows that end 1 and 3 phrases of K = 9.

Expectation: the ids cells equal; path_out and logprob BIT-equal to the fp32 restatement path_in[p] + (z - lse[p]) in numpy, fed the
kernel's own z -- read back from a launch with zero path sums and zero lse, which leaves z itself in every cell -- and the lse it was
given; z against fp64 of the bf16 operands within d u sum|h||w| + u|z|, the bound tests/test_lse_head_gpu.py holds
i2t_lse_token_logprob's re-evaluated logit to (bit-equal to the logits cell in the other form); the row LSE inside ``lse_bound`` of
tests/test_logits_processors_gpu.py (the lp_bound form for this reduction shape); NaN guards around every output and every cell the
tables do not name untouched; the input path buffer unchanged; every refusal an error that writes nothing."""
import numpy as np
import pytest
import torch

from test_logits_processors_gpu import PAD_VALUE, U, bits, case, guarded, guards_untouched, lse_bound, pad64

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
B, W, K, LP_LD, IDS_LD, LEN = 2, 70, 9, 12, 8, 5
R = B * W
VS = (70, 257, 50257)
FORMS = (('logits', 0, 1.0), ('bf16', 64, 1.0), ('bf16', 128, 0.5))


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
    """the operands of one (vocabulary, form): built once, never changed"""
    key = (V, form, d)
    if key in _DATA:
        return _DATA[key]
    g = torch.Generator().manual_seed(V * 7 + d)
    rng = np.random.default_rng(V + d)
    eos = V - 3
    toks = np.setdiff1d(np.arange(V), [eos])
    levels = [dict(child_parent=np.zeros(5, dtype=np.int64), child_tok=rng.choice(toks, 5, replace=False), term_row=[], term_off=[0], term_phrase=[]),
              dict(child_parent=np.arange(W) % 5, child_tok=rng.choice(toks, W, replace=V < 2 * W), term_row=[1, 3], term_off=[0, 1, 4],
                   term_phrase=[2, 0, 5, 7])]
    c = dict(V=V, eos=eos, levels=levels, lse=(torch.randn(R, generator=g) + 6).to(dev()), path=(torch.randn(R, generator=g) * 3 - 4).to(dev()))
    if form == 'logits':
        ld = pad64(V)
        z = torch.randn(R, ld, generator=g) * 3
        z[:, V:] = PAD_VALUE
        c.update(ld=ld, logits=z.to(dev()))
    else:
        c.update(hidden=torch.randn(R, d, generator=g).to(BF16).to(dev()), w_head=(torch.randn(V, d, generator=g) * 0.3).to(BF16).to(dev()))
    _DATA[key] = c
    return c


def launch(ops, c, tables, form, d, scale, lse, path_in, path_out, ids, logprob, len_ptr):
    kw = dict(logits=c['logits'], ld=c['ld']) if form == 'logits' else dict(hidden=c['hidden'], w_head=c['w_head'], d=d, scale=scale)
    ops.trie_level_expand(tables, lse, path_in, path_out, ids, IDS_LD, len_ptr, logprob, c['eos'], B, W, c['V'], **kw)


def outputs():
    path_out, pbuf = guarded(1, R)
    ids, ibuf = guarded(R, IDS_LD, fill=-7, dtype=torch.long)
    logprob, lbuf = guarded(B, LP_LD)
    return (path_out.view(-1), ids, logprob), (pbuf, ibuf, lbuf)


@pytest.mark.parametrize('form,d,scale', FORMS)
@pytest.mark.parametrize('V', VS)
def test_level_expand(ops, V, form, d, scale):
    c = data(V, form, d)
    eos = c['eos']
    len_ptr = torch.tensor([LEN], dtype=I32, device=dev())
    zero = torch.zeros(R, device=dev())
    worst = 0.0
    for lv in c['levels']:
        tables = ops.trie_level_tables(lv['child_parent'], lv['child_tok'], lv['term_row'], lv['term_off'], lv['term_phrase'], W, V, K, dev())
        n_child = len(lv['child_tok'])
        (z_path, _, z_lp), _ = outputs()
        launch(ops, c, tables, form, d, scale, zero, zero, z_path, torch.zeros(R, IDS_LD, dtype=torch.long, device=dev()), z_lp, len_ptr)
        path_in = c['path'].clone()
        (path_out, ids, logprob), (pbuf, ibuf, lbuf) = outputs()
        launch(ops, c, tables, form, d, scale, c['lse'], path_in, path_out, ids, logprob, len_ptr)
        (again, _, again_lp), _ = outputs()
        launch(ops, c, tables, form, d, scale, c['lse'], path_in, again, torch.zeros(R, IDS_LD, dtype=torch.long, device=dev()), again_lp, len_ptr)
        torch.cuda.synchronize()
        tag = f'V {V} {form} d {d} level of {n_child} children'
        assert torch.equal(bits(path_in), bits(c['path'])), f'{tag}: the input path buffer was written'
        assert torch.isnan(pbuf[0]).all() and torch.isnan(pbuf[2:]).all() and torch.isnan(lbuf[0]).all() and torch.isnan(lbuf[1 + B:]).all()
        assert bool((ibuf[0] == -7).all()) and bool((ibuf[1 + R:] == -7).all()), f'{tag}: a guard row of ids was written'
        assert torch.equal(bits(path_out), bits(again)) and torch.equal(bits(logprob), bits(again_lp)), f'{tag}: two launches differ'
        zc, zt = z_path.cpu().numpy(), z_lp.cpu().numpy()
        lse, pin = c['lse'].cpu().numpy(), c['path'].cpu().numpy()
        got_path, got_ids, got_lp = path_out.cpu().numpy(), ids.cpu().numpy(), logprob.cpu().numpy()
        want_path = np.full(R, np.nan, dtype=np.float32)
        want_ids = np.full((R, IDS_LD), -7, dtype=np.int64)
        want_lp = np.full((B, LP_LD), np.nan, dtype=np.float32)
        ref_rows, ref_toks, zs = [], [], []
        for b in range(B):
            for j in range(n_child):
                p, cell = b * W + int(lv['child_parent'][j]), b * W + j
                want_path[cell] = np.float32(pin[p] + np.float32(zc[cell] - lse[p]))
                want_ids[cell, LEN] = int(lv['child_tok'][j])
                ref_rows.append(p), ref_toks.append(int(lv['child_tok'][j])), zs.append(zc[cell])
            for j, w in enumerate(lv['term_row']):
                p = b * W + w
                for k in lv['term_phrase'][lv['term_off'][j]:lv['term_off'][j + 1]]:
                    assert zt[b, k] == zt[b, lv['term_phrase'][lv['term_off'][j]]], 'the duplicates of a node share its z'
                    want_lp[b, k] = np.float32(pin[p] + np.float32(zt[b, k] - lse[p]))
                ref_rows.append(p), ref_toks.append(eos), zs.append(zt[b, lv['term_phrase'][lv['term_off'][j]]])
        assert np.array_equal(got_ids, want_ids), f'{tag}: ids'
        assert np.array_equal(got_path.view(np.int32), want_path.view(np.int32)), f'{tag}: path_out is not the fp32 restatement, bit for bit'
        assert np.array_equal(got_lp.view(np.int32), want_lp.view(np.int32)), f'{tag}: logprob is not the fp32 restatement, bit for bit'
        # z itself
        rows, toks, zs = torch.tensor(ref_rows), torch.tensor(ref_toks), torch.tensor(np.array(zs, dtype=np.float32))
        if form == 'logits':
            assert torch.equal(bits(zs), bits(c['logits'].cpu()[rows, toks])), f'{tag}: z is not the logits cell'
        else:
            h, w = c['hidden'].cpu().double()[rows], c['w_head'].cpu().double()[toks]
            ref, S = scale * (h * w).sum(dim=-1), (h.abs() * w.abs()).sum(dim=-1)
            bound = d * U * scale * S + U * ref.abs()
            err = (zs.double() - ref).abs()
            assert bool((err <= bound).all()), f'{tag}: z worst error / bound {float((err / bound).max()):.3g}'
            worst = max(worst, float((err / bound).max()))
    print(f'V {V} {form} d {d}: worst z error over bound {worst:.3g}')


@pytest.mark.parametrize('V', VS)
def test_rows_lse(ops, V):
    c = case(V)                                                 # three rows with -inf cells and exact zeros (test_logits_processors_gpu)
    rows = c['z_dev'].shape[0]
    lse_ref, bound = lse_bound(c['z64'], V)
    outs = []
    for _ in range(2):
        z = c['z_dev'].clone()
        buf = torch.full((3, 4), float('nan'), device=dev())
        ops.rows_lse(z, c['ld'], buf[1, :rows], rows, V)
        torch.cuda.synchronize()
        assert torch.equal(bits(z), bits(c['z_dev'])), 'the logits were written'
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[2]).all() and torch.isnan(buf[1, rows:]).all()
        outs.append(buf[1, :rows].clone())
    assert torch.equal(bits(outs[0]), bits(outs[1])), 'two launches differ'
    err = (outs[0].double().cpu() - lse_ref).abs()
    print(f'V {V}: rows_lse worst error over bound {float((err / bound).max()):.3g}')
    assert bool((err <= bound).all())


def test_refusals(ops):
    from image2text_amd import lib as i2tlib
    lib = i2tlib.load()
    V, d = 70, 64
    cl, cb = data(V, 'logits', 0), data(V, 'bf16', d)
    lv = cl['levels'][1]
    t = ops.trie_level_tables(lv['child_parent'], lv['child_tok'], lv['term_row'], lv['term_off'], lv['term_phrase'], W, V, K, dev())
    path_in, len_ptr = cl['path'].clone(), torch.tensor([LEN], dtype=I32, device=dev())
    (path_out, ids, logprob), (pbuf, ibuf, lbuf) = outputs()
    before = [x.clone() for x in (pbuf, ibuf, lbuf, path_in)]
    args = dict(stream=torch.cuda.current_stream().cuda_stream, hidden=cb['hidden'].data_ptr(), ld_hidden=d, w_head=cb['w_head'].data_ptr(), ld_w=d,
                d=d, scale=1.0, logits=None, ld=0, lse=cl['lse'].data_ptr(), path_in=path_in.data_ptr(), path_out=path_out.data_ptr(),
                child_parent=t.child_parent.data_ptr(), child_tok=t.child_tok.data_ptr(), n_child=t.n_child, term_row=t.term_row.data_ptr(),
                term_off=t.term_off.data_ptr(), term_phrase=t.term_phrase.data_ptr(), n_term=t.n_term, n_term_phrases=t.n_term_phrases,
                ids=ids.data_ptr(), ids_ld=IDS_LD, len_ptr=len_ptr.data_ptr(), logprob=logprob.data_ptr(), lp_ld=LP_LD, eos=cl['eos'], B=B, W=W, V=V)
    with_logits = {**args, 'hidden': None, 'w_head': None, 'logits': cl['logits'].data_ptr(), 'ld': cl['ld']}

    def refused(a, change, text, fn='i2t_trie_level_expand'):
        rc = getattr(lib, fn)(*{**a, **change}.values())
        assert rc == -1 and text in i2tlib.last_error() and fn in i2tlib.last_error(), (change, rc, i2tlib.last_error())

    for a in (args, with_logits):
        for name in ('lse', 'path_in', 'path_out', 'ids', 'len_ptr', 'logprob', 'child_parent', 'child_tok', 'term_row', 'term_off', 'term_phrase'):
            refused(a, {name: None}, 'null pointer')
        refused(a, dict(n_child=-1), 'n_child = -1')
        refused(a, dict(n_term=-1), 'n_term = -1')
        refused(a, dict(n_child=W + 1), f'n_child = {W + 1}')
        refused(a, dict(n_term=W + 1), f'n_term = {W + 1}')
        refused(a, dict(eos=V), f'eos = {V}')
        refused(a, dict(eos=-1), 'eos = -1')
        refused(a, dict(B=0), 'B = 0')
        refused(a, dict(path_out=a['path_in']), 'one buffer')
        for name in ('lse', 'path_in', 'path_out', 'child_parent', 'child_tok', 'term_row', 'term_off', 'term_phrase', 'logprob'):
            refused(a, {name: a[name] + 4}, 'misaligned')
        refused(a, dict(ids=a['ids'] + 8), 'misaligned')
    refused(args, dict(hidden=None), 'null pointer')
    refused(args, dict(w_head=None), 'null pointer')
    refused(args, dict(d=60), 'd = 60')
    refused(args, dict(ld_hidden=d - 8), 'd = 64')
    refused(args, dict(hidden=args['hidden'] + 2), 'misaligned')
    refused(args, dict(scale=float('inf')), 'scale must be finite')
    refused(with_logits, dict(ld=V - 2), 'ld = 68')
    refused(with_logits, dict(ld=V + 1), 'ld = 71')
    refused(with_logits, dict(logits=with_logits['logits'] + 4), 'misaligned')
    lse_args = dict(stream=args['stream'], logits=cl['logits'].data_ptr(), ld=cl['ld'], lse=path_out.data_ptr(), R=R, V=V)
    refused(lse_args, dict(logits=None), 'null pointer', 'i2t_rows_lse')
    refused(lse_args, dict(lse=None), 'null pointer', 'i2t_rows_lse')
    refused(lse_args, dict(ld=V - 2), 'ld = 68', 'i2t_rows_lse')
    refused(lse_args, dict(ld=V + 1), 'ld = 71', 'i2t_rows_lse')
    refused(lse_args, dict(R=0), 'R = 0', 'i2t_rows_lse')
    refused(lse_args, dict(lse=lse_args['lse'] + 4), 'misaligned', 'i2t_rows_lse')
    # the tables are host-built: their contents are refused before upload
    good = (lv['child_parent'], lv['child_tok'], lv['term_row'], lv['term_off'], lv['term_phrase'])
    for at, value, text in ((0, [W] + [0] * (W - 1), 'a parent row outside'), (0, [-1] + [0] * (W - 1), 'a parent row outside'),
                            (1, [V] + [1] * (W - 1), 'a token outside'), (2, [1, W], 'a terminal row outside'),
                            (3, [0, 5, 4], 'does not ascend'), (3, [1, 1, 4], 'does not ascend'), (4, [2, 0, 5, K], 'a phrase index outside'),
                            (0, [0] * (W + 1), 'parent rows for')):
        bad = list(good)
        bad[at] = value
        with pytest.raises(i2tlib.I2TError, match=text):
            ops.trie_level_tables(*bad, W, V, K, dev())
    with pytest.raises(i2tlib.I2TError, match='exceed the W = 4 rows'):
        ops.trie_level_tables(*good, 4, V, K, dev())
    with pytest.raises(i2tlib.I2TError, match='one buffer'):
        ops.trie_level_expand(t, cl['lse'], path_in, path_in, ids, IDS_LD, len_ptr, logprob, cl['eos'], B, W, V, logits=cl['logits'], ld=cl['ld'])
    torch.cuda.synchronize()
    for x, y in zip(before, (pbuf, ibuf, lbuf, path_in)):
        assert torch.equal(bits(x), bits(y)), 'a refused call wrote something'
