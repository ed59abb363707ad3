"""The two kernels of a phrase-constrained generate_captions step, directly through ops.caption_trie_mask and
ops.caption_trie_advance, on the MI355X.

Shapes: R = 3 rows; V in {70, 257, 50257} with ld = V rounded up to 64 columns (what the decoder's logits buffer uses), the pad columns
holding 1e30 (not part of the row).  One trie per vocabulary, built by ``phrase_trie`` from two-token phrases [a_j, t]: the node behind
a_j has a fan-out of f_j for every f_j in {1, 2, 255, 256, 257, V - 1} below V -- the gather and scatter loops of the mask kernel walk a
node's children in chunks of 256 threads, so they run on both sides of one chunk, and V - 1 is every token but the EOS --; [a_j] is
itself a phrase for every other j, so the set holds terminal and non-terminal nodes with children, and its leaves end a phrase and allow
the EOS alone.  The rows of a launch sit at three different nodes.  The raw rows hold -inf at a few columns, children among them.

Expectation: the masked row is decoding.trie_mask_host's, bit for bit; kept holds the raw gathers; node and phrase_index after the
advance kernel are decoding.trie_advance_host's; raw_lse and tok_lp are held to the bound tests/test_logits_processors_gpu.py derives
for caption_logits_process_kernel's reduction (``lse_bound``, imported: the same 256-thread chain, xor tree and wave order; tok_lp adds
the rounding of its subtraction).  Guard words around logits, kept, raw_lse and tok_lp stay untouched."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import phrase_trie, trie_advance_host, trie_mask_host
from test_logits_processors_gpu import PAD_VALUE, U, bits, guarded, guards_untouched, lse_bound, pad64

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
R, IDS_LD, LEN = 3, 24, 5
VS, FANOUTS = (70, 257, 50257), (1, 2, 255, 256, 257)


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


_CASES = {}


def case(V):
    """the trie, the nodes under test, the raw logits [R, ld] and their fp64 statistics of one vocabulary -- built once, never changed"""
    if V in _CASES:
        return _CASES[V]
    rng = np.random.default_rng(V)
    ld, eos = pad64(V), V - 3
    fans = [f for f in FANOUTS if f < V - 1] + [V - 1]
    firsts = [10 + j for j in range(len(fans))]
    allowed = np.setdiff1d(np.arange(V), [eos])
    phrases, kids = [], {}
    for j, (a, f) in enumerate(zip(firsts, fans)):
        kids[a] = np.sort(rng.permutation(allowed)[:f]) if f < V - 1 else allowed
        if j % 2 == 0:
            phrases.append([a])                                 # a phrase that is a prefix of others: a terminal node with children
        phrases += [[a, int(t)] for t in kids[a]]
    trie = phrase_trie(phrases, eos, V, 3)
    assert trie.max_fanout == V - 1 and trie.nodes == 1 + len(fans) + sum(fans)
    root_toks, root_next = trie.children(0)
    node_of = {int(t): int(n) for t, n in zip(root_toks, root_next)}
    leaf = int(trie.children(node_of[firsts[0]])[1][0])
    nodes = [0] + [node_of[a] for a in firsts] + [leaf]
    assert [int(np.diff(trie.child_off)[n]) for n in nodes] == [len(fans)] + fans + [0]
    assert [bool(trie.term[n] >= 0) for n in nodes] == [False] + [j % 2 == 0 for j in range(len(fans))] + [True]
    z = (rng.standard_normal((R, ld)) * 3).astype(np.float32)
    z[:, V:] = PAD_VALUE
    z[:, eos] = [2.5, 0.0, -4.0]
    z[:, 6] = -np.inf
    for a in firsts:                                            # a raw -inf at a child of every node, and an exact zero at another
        z[:, kids[a][0]] = -np.inf
        z[:, kids[a][-1]] = 0.0
    z[:, eos] = [2.5, 0.0, -4.0]
    keys = ('child_off', 'child_tok', 'child_next', 'term')
    c = dict(V=V, ld=ld, eos=eos, trie=trie, nodes=nodes, z=z, z64=torch.from_numpy(z[:, :V]).double(), z_dev=torch.from_numpy(z).to(dev()),
             kept_ld=(trie.max_fanout + 1 + 3) // 4 * 4, **{k: torch.from_numpy(getattr(trie, k)).to(dev()) for k in keys})
    _CASES[V] = c
    return c


def groups(nodes):
    """the nodes under test, three rows at a time (the last group wraps round)"""
    return [[nodes[(i + r) % len(nodes)] for r in range(R)] for i in range(0, len(nodes), R)]


def mask(ops, c, z, node, done, lse, kept):
    ops.caption_trie_mask(z, c['ld'], node, c['child_off'], c['child_tok'], c['term'], c['eos'], done, lse, kept, R, c['V'])


def advance(ops, c, ids, len_ptr, finished, z, lse, done, node, phrase, tok_lp):
    ops.caption_trie_advance(ids, IDS_LD, len_ptr, finished, z, c['ld'], lse, c['child_off'], c['child_tok'], c['child_next'], c['term'],
                             c['eos'], done, node, phrase, tok_lp, R, c['V'])


def lse_buffer():
    buf, whole = guarded(1, 4)
    return buf.view(-1)[:R], whole, whole[1, 3:].clone()


@pytest.mark.parametrize('V', VS)
def test_mask_kernel(ops, V):
    c = case(V)
    trie, eos, ld = c['trie'], c['eos'], c['ld']
    done = torch.zeros(1, dtype=I32, device=dev())
    lse_ref, bound = lse_bound(c['z64'], V)
    worst = 0.0
    for rows in groups(c['nodes']):
        node = torch.tensor(rows, dtype=I32, device=dev())
        outs = []
        for _ in range(2):
            z, zbuf = guarded(R, ld)
            z.copy_(c['z_dev'])
            kept, kbuf = guarded(R, c['kept_ld'])
            lse, lbuf, behind = lse_buffer()
            mask(ops, c, z, node, done, lse, kept)
            torch.cuda.synchronize()
            outs.append((z, lse, kept))
            assert guards_untouched(zbuf, R) and guards_untouched(kbuf, R) and guards_untouched(lbuf, 1), f'V {V} nodes {rows}: a guard word was written'
            assert torch.equal(bits(lbuf[1, 3:]), bits(behind)), 'a word behind raw_lse was written'
        for a, b in zip(*outs):                                 # no atomics, a fixed reduction order: two launches agree in every bit
            assert torch.equal(bits(a), bits(b)), f'V {V} nodes {rows}: two launches differ'
        z, lse, kept = outs[0]
        got, kp = z.cpu().numpy(), kept.cpu().numpy()
        assert np.array_equal(got[:, V:], c['z'][:, V:]), 'a pad column was written'
        assert torch.equal(node.cpu(), torch.tensor(rows, dtype=I32))
        for r, n in enumerate(rows):
            want = trie_mask_host(c['z'][r, :V], n, trie, eos)
            assert np.array_equal(got[r, :V].view(np.int32), want.view(np.int32)), f'V {V} node {n}: row {r} differs from trie_mask_host'
            toks, _ = trie.children(n)
            fan, terminal = toks.shape[0], bool(trie.term[n] >= 0)
            assert int((want > -np.inf).sum()) <= fan + terminal
            assert np.array_equal(kp[r, :fan].view(np.int32), c['z'][r, toks].view(np.int32)), f'V {V} node {n}: kept is not the raw gather'
            if terminal:
                assert kp[r, fan] == c['z'][r, eos]
            assert np.isnan(kp[r, fan + terminal:]).all(), f'V {V} node {n}: kept was written past the node\'s entries'
        err = (lse.double().cpu() - lse_ref).abs()
        assert bool((err <= bound).all()), f'V {V} nodes {rows}: raw_lse worst error / bound {float((err / bound).max()):.3g}'
        worst = max(worst, float((err / bound).max()))
    print(f'V {V}: worst raw_lse error over bound {worst:.3g}')


@pytest.mark.parametrize('V', VS)
def test_advance_kernel(ops, V):
    """after the pre-pass, per group of nodes and per kind of chosen token: the first, a middle and the last child; the EOS (a phrase
    index at a terminal node, nothing elsewhere); a token the node does not allow (nothing); and one finished row (skipped)"""
    c = case(V)
    trie, eos, ld = c['trie'], c['eos'], c['ld']
    done, len_ptr = torch.zeros(1, dtype=I32, device=dev()), torch.tensor([LEN], dtype=I32, device=dev())
    lse_ref, bound = lse_bound(c['z64'], V)
    worst, named, moved = 0.0, 0, 0
    for rows in groups(c['nodes']):
        node0 = torch.tensor(rows, dtype=I32, device=dev())
        z = c['z_dev'].clone()
        lse, kept = torch.zeros(4, device=dev()), torch.zeros(R, c['kept_ld'], device=dev())
        mask(ops, c, z, node0, done, lse[:R], kept)
        for kind in ('first', 'middle', 'last', 'eos', 'other', 'finished'):
            chosen = []
            for n in rows:
                toks, _ = trie.children(n)
                pick = dict(first=0, middle=toks.shape[0] // 2, last=-1).get(kind, 0)
                chosen.append(eos if kind == 'eos' or toks.shape[0] == 0 else 7 if kind == 'other' else int(toks[pick]))
            fin = [0, 1, 0] if kind == 'finished' else [0, 0, 0]
            ids = torch.full((R, IDS_LD), 5, dtype=torch.long, device=dev())
            ids[:, LEN] = torch.tensor(chosen, device=dev())
            ids_before = ids.clone()
            node, phrase = node0.clone(), torch.full((4,), -7, dtype=I32, device=dev())
            tok_lp, tbuf = guarded(R, IDS_LD)
            advance(ops, c, ids, len_ptr, torch.tensor(fin, dtype=I32, device=dev()), z, lse[:R], done, node, phrase[:R], tok_lp)
            torch.cuda.synchronize()
            tag = f'V {V} nodes {rows} {kind}'
            assert torch.equal(ids, ids_before) and guards_untouched(tbuf, R) and int(phrase[3]) == -7, f'{tag}: a word outside was written'
            keep = torch.ones(IDS_LD, dtype=torch.bool, device=dev())
            keep[LEN] = False
            assert bool(torch.isnan(tok_lp[:, keep]).all()), f'{tag}: a log-prob column other than len was written'
            for r, n in enumerate(rows):
                nxt, ph, ok = trie_advance_host(n, chosen[r], trie, eos)
                lp = float(tok_lp[r, LEN])
                if fin[r] or not ok:
                    assert int(node[r]) == n and int(phrase[r]) == -7 and np.isnan(lp), f'{tag}: row {r} was not left as it was'
                    continue
                assert int(node[r]) == nxt and int(phrase[r]) == (ph if ph >= 0 else -7), f'{tag}: row {r} differs from trie_advance_host'
                named, moved = named + (ph >= 0), moved + (nxt != n)
                ref = float(c['z64'][r, chosen[r]] - lse_ref[r])
                if not np.isfinite(ref):
                    assert lp == ref, f'{tag}: row {r}'
                    continue
                bnd = float(bound[r]) + U * abs(ref)
                assert abs(lp - ref) <= bnd, f'{tag}: row {r} tok_lp {lp} vs fp64 {ref} (bound {bnd:.3g})'
                worst = max(worst, abs(lp - ref) / bnd)
    assert named >= 3 and moved >= 9
    print(f'V {V}: worst tok_lp error over bound {worst:.3g}')


def test_nothing_is_written_past_done(ops):
    c = case(257)
    z, node = c['z_dev'].clone(), torch.tensor(c['nodes'][:R], dtype=I32, device=dev())
    lse, kept = torch.full((4,), 0.5, device=dev()), torch.full((R, c['kept_ld']), 0.25, device=dev())
    ids = torch.full((R + 1, IDS_LD), int(c['trie'].child_tok[0]), dtype=torch.long, device=dev())
    phrase, tok_lp = torch.full((4,), -7, dtype=I32, device=dev()), torch.full((R + 1, IDS_LD), 0.75, device=dev())
    done, fin = torch.ones(1, dtype=I32, device=dev()), torch.zeros(R, dtype=I32, device=dev())
    state = (z, node, lse, kept, ids, phrase, tok_lp)
    before = [t.clone() for t in state]
    mask(ops, c, z, node, done, lse[:R], kept)
    advance(ops, c, ids, torch.tensor([LEN], dtype=I32, device=dev()), fin, z, lse[:R], done, node, phrase[:R], tok_lp)
    torch.cuda.synchronize()
    for a, b in zip(before, state):
        assert torch.equal(bits(a), bits(b))


def test_entry_point_refusals(ops):
    """every check the entry points make without the device: an error with its message, and the outputs as they were"""
    from image2text_amd import lib as i2tlib
    lib = i2tlib.load()
    c = case(70)
    V, ld, eos, trie = c['V'], c['ld'], c['eos'], c['trie']
    z, node = c['z_dev'].clone(), torch.tensor(c['nodes'][:R] + [0], dtype=I32, device=dev())
    lse, kept = torch.full((4,), 0.5, device=dev()), torch.full((R, c['kept_ld']), 0.25, device=dev())
    ids = torch.full((R, IDS_LD), int(trie.child_tok[0]), dtype=torch.long, device=dev())
    phrase, tok_lp = torch.full((4,), -7, dtype=I32, device=dev()), torch.full((R, IDS_LD), 0.75, device=dev())
    done, fin, len_ptr = torch.zeros(1, dtype=I32, device=dev()), torch.zeros(4, dtype=I32, device=dev()), torch.tensor([LEN], dtype=I32, device=dev())
    state = (z, node, lse, kept, ids, phrase, tok_lp)
    before = [t.clone() for t in state]
    stream = torch.cuda.current_stream().cuda_stream
    tr = {k: c[k].data_ptr() for k in ('child_off', 'child_tok', 'child_next', 'term')}
    pre = dict(stream=stream, logits=z.data_ptr(), ld=ld, node=node.data_ptr(), child_off=tr['child_off'], child_tok=tr['child_tok'],
               term=tr['term'], nodes=trie.nodes, edges=trie.edges, eos=eos, done=done.data_ptr(), raw_lse=lse.data_ptr(),
               kept=kept.data_ptr(), kept_ld=c['kept_ld'], R=R, V=V)
    post = dict(stream=stream, ids=ids.data_ptr(), ids_ld=IDS_LD, len_ptr=len_ptr.data_ptr(), finished=fin.data_ptr(), logits=z.data_ptr(),
                ld=ld, raw_lse=lse.data_ptr(), child_off=tr['child_off'], child_tok=tr['child_tok'], child_next=tr['child_next'],
                term=tr['term'], nodes=trie.nodes, edges=trie.edges, eos=eos, done=done.data_ptr(), node=node.data_ptr(),
                phrase_index=phrase.data_ptr(), tok_lp=tok_lp.data_ptr(), lp_ld=IDS_LD, R=R, V=V)

    def refused(fn, args, change, text):
        rc = getattr(lib, fn)(*{**args, **change}.values())
        assert rc == -1 and text in i2tlib.last_error() and fn in i2tlib.last_error(), (fn, change, rc, i2tlib.last_error())

    for fn, args in (('i2t_caption_trie_mask', pre), ('i2t_caption_trie_advance', post)):
        for name, value in args.items():
            if name != 'stream' and value is not None and value > 1 << 20:              # every pointer argument
                refused(fn, args, {name: None}, 'null pointer')
        refused(fn, args, dict(ld=V - 1), 'ld = 69')
        refused(fn, args, dict(ld=V + 1), 'ld = 71')
        refused(fn, args, dict(eos=V), f'eos = {V}')
        refused(fn, args, dict(eos=-1), 'eos = -1')
        refused(fn, args, dict(nodes=0), 'nodes = 0')
        refused(fn, args, dict(edges=-1), 'edges = -1')
        refused(fn, args, dict(R=0), 'R = 0')
        for name in ('logits', 'raw_lse', 'node', 'child_off', 'child_tok', 'term'):
            refused(fn, args, {name: args[name] + 4}, 'misaligned')
    refused('i2t_caption_trie_mask', pre, dict(kept_ld=0), 'kept_ld = 0')
    refused('i2t_caption_trie_mask', pre, dict(kept=pre['kept'] + 4), 'misaligned')
    refused('i2t_caption_trie_advance', post, dict(lp_ld=0), 'lp_ld = 0')
    for name in ('ids', 'child_next', 'phrase_index'):
        refused('i2t_caption_trie_advance', post, {name: post[name] + 4}, 'misaligned')
    # through the wrappers the same error surfaces as I2TError
    with pytest.raises(i2tlib.I2TError, match='eos = 70'):
        ops.caption_trie_mask(z, ld, node, c['child_off'], c['child_tok'], c['term'], V, done, lse, kept, R, V)
    with pytest.raises(i2tlib.I2TError, match='eos = 70'):
        ops.caption_trie_advance(ids, IDS_LD, len_ptr, fin, z, ld, lse, c['child_off'], c['child_tok'], c['child_next'], c['term'], V, done, node,
                                 phrase, tok_lp, R, V)
    torch.cuda.synchronize()
    for a, b in zip(before, state):
        assert torch.equal(bits(a), bits(b))
