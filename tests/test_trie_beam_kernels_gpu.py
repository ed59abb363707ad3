"""The two kernels of search_phrases, directly through ops.trie_beam_candidates and ops.trie_beam_select, on the MI355X:
each against its numpy replica (decoding_host.trie_beam_candidates_host / trie_beam_select_host), bit for bit, on random state.  The
candidates kernel's log-sum-exp is held to ops.rows_lse on the same rows, bit for bit, and the replica is then given that value: what
is compared is everything the kernel does with it.  One figure is not compared by its bits: pool_score passes through one powf, the
device's against numpy's, and gets 2 ulp (tests/test_caption_beams_gpu.py does the same); every decision that hangs on it is exact in
the cases below (lengths 1 and 4)."""
import numpy as np
import pytest
import torch

from image2text_amd.caption_plan import BEAM_DEAD
from image2text_amd.decoding_host import beam_advance_host, trie_beam_candidates_host, trie_beam_select_host
from image2text_amd.phrase_trie import PhraseTrie, phrase_trie

pytestmark = pytest.mark.gpu

THREADS = 256                                   # the candidates kernel's workgroup (csrc/constrain.hip::TRIE_THREADS)
f32, i32 = np.float32, np.int32


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(i32)


# ------------------------------------------------------------------------------------------------------ candidates
def fan_trie(V, W, eos, g):
    """a CSR table (not a tree: child_next is arbitrary, the kernel never follows it) whose nodes have the fan-outs under test, every
    second one ending a phrase -> (trie, fans)"""
    fans = sorted({0, 1, W - 1, W, V - 1} | ({THREADS + 44} if V - 1 > THREADS + 44 else set()))
    fans = fans + fans                          # each fan-out once at a node that ends a phrase and once at one that does not
    off, tok, term = [0], [], []
    allowed = np.setdiff1d(np.arange(V), [eos])
    for n, fan in enumerate(fans):
        tok += sorted(g.choice(allowed, size=fan, replace=False).tolist())
        off.append(len(tok))
        term.append(n if n < len(fans) // 2 else -1)
    nxt = g.integers(0, len(fans), len(tok))
    return PhraseTrie(np.array(off, dtype=i32), np.array(tok, dtype=i32), nxt.astype(i32), np.array(term, dtype=i32), max(fans), 1), fans


@pytest.mark.parametrize('W', [2, 8])
@pytest.mark.parametrize('R,V,ld', [(3, 67, 68), (16, 515, 516)])
def test_candidates_against_the_replica(ops, R, V, ld, W):
    eos = 5
    g = np.random.default_rng(R * 1000 + V + W)
    trie, fans = fan_trie(V, W, eos, g)
    assert {0, 1, W - 1, W, V - 1} <= set(fans) and (V < 300 or max(f for f in fans if f < V - 1) > THREADS)
    t_off, t_tok, t_term = up(trie.child_off), up(trie.child_tok), up(trie.term)
    ctrl = torch.zeros(2, dtype=torch.int32, device=dev())
    seen_ties = 0
    for start in range(0, trie.nodes, R - 1):   # every node gets a row; the last row of every launch is dead
        node = np.array([(start + i) % trie.nodes for i in range(R - 1)] + [-1 if start % 2 == 0 else trie.nodes], dtype=i32)
        path = (-g.random(R, dtype=f32) * 5).astype(f32)
        z = (g.standard_normal((R, ld)) * 3).astype(f32)
        z[:, V:] = 1e30                         # the padding columns take no part
        for r in range(R - 1):                  # ties: equal logits on two children
            toks, _ = trie.children(int(node[r]))
            if toks.shape[0] >= 2:
                z[r, toks[-1]] = z[r, toks[0]] = 4.0 if toks.shape[0] <= W else z[r, toks[0]]
                seen_ties += 1
        dz = up(z)
        out_e, out_t = torch.full((R, W), 77, dtype=torch.int32, device=dev()), torch.full((R, W), 7.0, device=dev())
        out_f, out_l = torch.full((R,), 7.0, device=dev()), torch.full((R,), 7.0, device=dev())
        ops.trie_beam_candidates(dz, ld, up(node), up(path), t_off, t_tok, t_term, eos, ctrl, out_e, out_t, out_f, R, W, V, lse=out_l)
        ref = torch.zeros(R, device=dev())
        ops.rows_lse(dz, ld, ref, R, V)
        live = (node >= 0) & (node < trie.nodes)
        got_l = out_l.cpu().numpy()
        assert np.array_equal(bits(got_l[live]), bits(ref.cpu().numpy()[live])), 'lse: bit-equal to rows_lse on the same rows'
        assert got_l[~live].tolist() == [7.0] * int((~live).sum()), 'a dead row writes no lse'
        assert torch.equal(dz, up(z)), 'the rows are only read'
        want_e, want_t, want_f, _ = trie_beam_candidates_host(z, np.where(live, node, -1), path, trie, eos, W, V=V, lse=got_l)
        got_e, got_t, got_f = out_e.cpu().numpy(), out_t.cpu().numpy(), out_f.cpu().numpy()
        assert np.array_equal(got_e, want_e), (start, got_e, want_e)
        assert np.array_equal(bits(got_t), bits(want_t)) and np.array_equal(bits(got_f), bits(want_f))
        assert (got_e[~live] == -1).all() and np.isneginf(got_t[~live]).all() and np.isneginf(got_f[~live]).all()
        for r in np.flatnonzero(live):
            fan = int(trie.child_off[node[r] + 1] - trie.child_off[node[r]])
            assert int((got_e[r] >= 0).sum()) == min(fan, W) and np.isneginf(got_f[r]) == (trie.term[node[r]] < 0)
            assert bool((got_t[r] <= 0.0).all()), 'log-probs stay at or below 0 in fp32'
    assert seen_ties > 0
    ctrl[0] = 1                                 # ctrl[0] set: nothing is written
    out_e.fill_(77)
    out_f.fill_(7.0)
    ops.trie_beam_candidates(dz, ld, up(node), up(path), t_off, t_tok, t_term, eos, ctrl, out_e, out_t, out_f, R, W, V, lse=out_l)
    assert bool((out_e == 77).all()) and bool((out_f == 7.0).all())


# ------------------------------------------------------------------------------------------------------ select
V, LD, EOS, P = 67, 68, 5, 2
ROOTS = list(range(10, 22))
# twelve one-token phrases, each also the prefix of two longer ones (nodes that end a phrase AND have children); a chain 40 -> 41 -> 42 of
# single-child nodes that end nothing before its leaf
PHRASES = [[t] for t in ROOTS] + [[t, 30] for t in ROOTS] + [[t, 31, 32] for t in ROOTS] + [[40, 41, 42]]
SCENARIOS = ('random', 'one_parent', 'few', 'leaves', 'bound', 'closed', 'tie')
INTS = ('node', 'ids', 'hist', 'pool_phrase', 'pool_len', 'pool_n', 'closed', 'counters', 'ctrl')
EXACT = ('path', 'pool_sum')


def _nodes_by_kind(trie):
    fan = np.diff(trie.child_off)
    return dict(leaf=np.flatnonzero((fan == 0) & (trie.term >= 0)), inner=np.flatnonzero(fan > 0), single=np.flatnonzero(fan == 1),
                both=np.flatnonzero((fan > 0) & (trie.term >= 0)))


def _select_state(B, W, pos, t, penalty, shift, seed):
    g = np.random.default_rng(seed)
    trie = phrase_trie(PHRASES, EOS, V, 1 << 30)
    kinds = _nodes_by_kind(trie)
    R, ids_ld, hist_ld = B * W, P + trie.longest + 1 + 3, 333
    s = dict(node=np.zeros(R, dtype=i32), path=(-g.random(R, dtype=f32) * 4).astype(f32), ids=g.integers(0, V, (R, ids_ld)).astype(np.int64),
             hist=g.integers(0, R, (R, hist_ld)).astype(i32), pool_phrase=np.full((B, W), -1, dtype=i32), pool_sum=np.zeros((B, W), dtype=f32),
             pool_score=np.full((B, W), BEAM_DEAD, dtype=f32), pool_len=np.zeros((B, W), dtype=i32), pool_n=np.zeros(B, dtype=i32),
             closed=np.zeros(B, dtype=i32), counters=np.array([pos, P + t], dtype=i32), ctrl=np.zeros(2, dtype=i32))
    z = (g.standard_normal((R, LD)) * 2).astype(f32)
    names = []
    for b in range(B):
        name = SCENARIOS[(b + shift) % len(SCENARIOS)]
        names.append(name)
        rows = slice(b * W, (b + 1) * W)
        n = int(g.integers(0, W + 1)) if name in ('random', 'closed', 'tie') else (W if name == 'bound' else int(g.integers(0, W)))
        s['pool_n'][b] = n
        s['pool_score'][b, :n] = -np.sort(g.random(n, dtype=f32)) * 6 - (1e6 if name == 'random' else 0.5)
        s['pool_sum'][b, :n] = s['pool_score'][b, :n] * 2
        s['pool_len'][b, :n], s['pool_phrase'][b, :n] = 2, g.integers(100, 200, n)
        if name in ('random', 'closed', 'tie'):
            s['node'][rows] = g.choice(np.concatenate([kinds['inner'], kinds['leaf'], [-1]]), W)
            s['node'][b * W] = kinds['both'][b % kinds['both'].shape[0]]
            if name == 'tie':                   # the other rows' offers score far below the first row's
                s['path'][b * W + 1:(b + 1) * W] = -60.0
        elif name == 'one_parent':              # the last row sits at the root with the best path: it feeds every child, child 0 included
            s['node'][rows] = g.choice(kinds['single'], W)
            s['node'][b * W + W - 1], s['path'][b * W + W - 1] = 0, 0.0
            s['path'][b * W:b * W + W - 1] = -50.0
        elif name == 'few':                     # one live row with one child, the rest dead
            s['node'][rows] = -1
            s['node'][b * W + (W - 1) // 2] = kinds['single'][0]
        elif name == 'leaves':                  # every row ends a phrase and has no child: the image closes for want of rows
            s['node'][rows] = g.choice(kinds['leaf'], W)
        elif name == 'bound':                   # a full pool of scores no running row can reach
            s['node'][rows] = g.choice(kinds['inner'], W)
            s['pool_score'][b] = -np.sort(g.random(W, dtype=f32)) * 1e-3
        if name == 'closed':
            s['closed'][b] = 1
    cand = trie_beam_candidates_host(z, s['node'], s['path'], trie, EOS, W, V=V)
    with np.errstate(all='ignore'):
        denom = np.power(f32(t + 1), f32(penalty)).astype(f32)
    for b, name in enumerate(names):            # a pool entry with exactly the score the image's first offer will have: it stays in front
        if name == 'tie':
            s['pool_n'][b] = max(1, s['pool_n'][b])
            s['pool_score'][b, 0], s['pool_phrase'][b, 0] = f32(cand[2][b * W] / denom), 777
            s['pool_score'][b, 1:s['pool_n'][b]] = s['pool_score'][b, 0] - 1 - np.arange(s['pool_n'][b] - 1, dtype=f32)
    return trie, s, cand[:3], names


@pytest.mark.parametrize('penalty', [0.0, 1.0, -0.5])
@pytest.mark.parametrize('pos', [0, 300])
@pytest.mark.parametrize('B,W', [(1, 2), (3, 4), (2, 8)])
def test_select_against_the_replica(ops, B, W, pos, penalty):
    t = 0 if pos == 0 else 3                    # t + 1 = 1 or 4: the offers' powf is exact for every penalty here
    seen = set()
    for shift in range(len(SCENARIOS)):
        trie, s, (edge, total, fin), names = _select_state(B, W, pos, t, penalty, shift, seed=B * 100 + W * 10 + shift)
        seen |= set(names)
        d = {k: up(v) for k, v in s.items()}
        t_tok, t_nxt, t_term = up(trie.child_tok), up(trie.child_next), up(trie.term)
        call = lambda: ops.trie_beam_select(up(edge), up(total), up(fin), d['node'], d['path'], t_tok, t_nxt, t_term, EOS, d['ids'], d['hist'],
                                            d['pool_phrase'], d['pool_sum'], d['pool_score'], d['pool_len'], d['pool_n'], d['closed'],
                                            d['counters'][0:1], d['counters'][1:2], d['ctrl'], B, W, P, trie.longest, penalty)
        before = {k: v.copy() for k, v in s.items()}
        trie_beam_select_host(edge, total, fin, s['node'], s['path'], trie, EOS, s['ids'], s['hist'], s['pool_phrase'], s['pool_sum'],
                              s['pool_score'], s['pool_len'], s['pool_n'], s['closed'], s['counters'], s['ctrl'], W, P, trie.longest, penalty)
        call()
        for step in ('select', 'advance'):
            for k in INTS:
                assert np.array_equal(d[k].cpu().numpy(), s[k]), (names, step, k)
            for k in EXACT:
                assert np.array_equal(bits(d[k].cpu().numpy()), bits(s[k])), (names, step, k)
            got = d['pool_score'].cpu().numpy()
            assert bool((np.abs(got.astype(np.float64) - s['pool_score']) <= 2 * np.spacing(np.abs(s['pool_score']))).all()), (names, step)
            if step == 'select':
                beam_advance_host(s['counters'], s['ctrl'])
                ops.beam_advance(d['counters'], d['ctrl'])
        for b, name in enumerate(names):        # the scenarios did what they are there for
            rows = slice(b * W, (b + 1) * W)
            if name == 'closed':
                assert all(np.array_equal(s[k][rows], before[k][rows]) for k in ('node', 'path', 'ids', 'hist')), 'a closed image is left untouched'
                assert np.array_equal(s['pool_score'][b], before['pool_score'][b])
            elif name == 'one_parent':
                assert (s['hist'][rows, pos] == b * W + W - 1).all() and (s['node'][rows] > 0).all(), 'one parent feeds every child'
                assert np.array_equal(s['hist'][rows, :pos], np.repeat(before['hist'][b * W + W - 1:b * W + W, :pos], W, axis=0))
            elif name == 'few':
                assert int((s['node'][rows] >= 0).sum()) == 1 and s['node'][b * W] >= 0 and (s['ids'][b * W + 1:(b + 1) * W, P + t] == EOS).all()
                assert np.isneginf(s['path'][b * W + 1:(b + 1) * W]).all() and (s['hist'][b * W + 1:(b + 1) * W, pos] == np.arange(b * W + 1, (b + 1) * W)).all()
                assert s['closed'][b] == 0
            elif name == 'leaves':
                assert s['closed'][b] == 1 and (s['node'][rows] == -1).all() and s['pool_n'][b] > before['pool_n'][b]
            elif name == 'bound':
                assert s['closed'][b] == 1 and (s['node'][rows] >= 0).all(), 'closed at the bound with every row live'
            elif name == 'tie':
                assert s['pool_phrase'][b, 0] == 777 and s['pool_score'][b, 1] == s['pool_score'][b, 0], 'a held entry before a new one of equal score'
        # with ctrl[0] set nothing changes
        d['ctrl'][0] = 1
        d['closed'].zero_()
        d['counters'].copy_(torch.tensor([pos, P + t], dtype=torch.int32))
        keep = {k: v.clone() for k, v in d.items()}
        call()
        assert all(torch.equal(d[k], keep[k]) for k in d)
        # counters outside the call's columns: nothing is written either
        d['ctrl'].zero_()
        d['counters'].copy_(torch.tensor([pos, P + trie.longest + 1], dtype=torch.int32))
        keep = {k: v.clone() for k, v in d.items()}
        call()
        assert all(torch.equal(d[k], keep[k]) for k in d)
    assert seen == set(SCENARIOS)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_both_kernels(ops):
    from image2text_amd import lib as i2tlib
    trie = phrase_trie(PHRASES, EOS, V, 1 << 30)
    R, W = 4, 2
    z = torch.zeros(R, LD, device=dev())
    I = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    F = lambda *s: torch.zeros(*s, device=dev())
    base = dict(logits=z, ld=LD, node=I(R), path=F(R), child_off=up(trie.child_off), child_tok=up(trie.child_tok), term=up(trie.term), eos=EOS,
                ctrl=I(2), cand_edge=I(R, W), cand_total=F(R, W), fin_total=F(R), R=R, W=W, V=V, lse=F(R))

    def refused(fn, args, change, text, name):
        with pytest.raises(i2tlib.I2TError, match=text) as e:
            fn(**{**args, **change})
        assert name in str(e.value)
    cand = 'i2t_trie_beam_candidates'
    refused(ops.trie_beam_candidates, base, dict(W=9, cand_edge=I(R, 9), cand_total=F(R, 9)), 'W = 9', cand)
    refused(ops.trie_beam_candidates, base, dict(ld=V - 1), 'ld = 66', cand)
    refused(ops.trie_beam_candidates, base, dict(ld=V + 2), 'ld = 69', cand)
    refused(ops.trie_beam_candidates, base, dict(eos=V), 'eos = 67', cand)
    refused(ops.trie_beam_candidates, base, dict(V=0), 'V = 0', cand)
    with pytest.raises(i2tlib.I2TError, match='null pointer'):
        ops._k.i2t_trie_beam_candidates(z, LD, base['node'], None, base['child_off'], base['child_tok'], base['term'], trie.nodes, trie.edges, EOS,
                                        base['ctrl'], base['cand_edge'], base['cand_total'], base['fin_total'], None, R, W, V)
    refused(ops.trie_beam_candidates, base, dict(fin_total=F(R + 1)[1:]), 'misaligned', cand)
    ids, hist = torch.zeros(R, 8, dtype=torch.long, device=dev()), I(R, 16)
    sel = dict(cand_edge=I(R, W), cand_total=F(R, W), fin_total=F(R), node=I(R), path=F(R), child_tok=up(trie.child_tok),
               child_next=up(trie.child_next), term=up(trie.term), eos=EOS, ids=ids, hist=hist, pool_phrase=I(2, W), pool_sum=F(2, W),
               pool_score=F(2, W), pool_len=I(2, W), pool_n=I(2), closed=I(2), pos_ptr=I(1), len_ptr=I(1), ctrl=I(2), B=2, W=W, P=P, longest=3,
               length_penalty=0.0)
    name = 'i2t_trie_beam_select'
    refused(ops.trie_beam_select, sel, dict(P=5), 'ids_ld = 8', name)                    # 5 + 3 + 1 = 9 columns in rows of 8
    refused(ops.trie_beam_select, sel, dict(length_penalty=float('nan')), 'length_penalty', name)
    refused(ops.trie_beam_select, sel, dict(length_penalty=float('inf')), 'length_penalty', name)
    refused(ops.trie_beam_select, sel, dict(longest=0), 'longest = 0', name)
    refused(ops.trie_beam_select, sel, dict(P=0), 'P = 0', name)
    refused(ops.trie_beam_select, sel, dict(eos=-1), 'eos = -1', name)
    with pytest.raises(i2tlib.I2TError, match='null pointer'):
        ops._k.i2t_trie_beam_select(sel['cand_edge'], sel['cand_total'], sel['fin_total'], sel['node'], sel['path'], sel['child_tok'],
                                    sel['child_next'], sel['term'], trie.nodes, trie.edges, EOS, ids, 8, hist, 16, sel['pool_phrase'],
                                    sel['pool_sum'], sel['pool_score'], sel['pool_len'], sel['pool_n'], None, sel['pos_ptr'], sel['len_ptr'],
                                    sel['ctrl'], 2, W, P, 3, 0.0)
    big = dict(sel, B=1, W=9, cand_edge=I(9, 9), cand_total=F(9, 9), fin_total=F(9), node=I(9), path=F(9), ids=torch.zeros(9, 8, dtype=torch.long, device=dev()),
               hist=I(9, 16), pool_phrase=I(1, 9), pool_sum=F(1, 9), pool_score=F(1, 9), pool_len=I(1, 9), pool_n=I(1), closed=I(1))
    refused(ops.trie_beam_select, big, {}, 'W = 9', name)
