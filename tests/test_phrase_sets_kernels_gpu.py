"""The three entry points of ``phrase_sets`` directly through ops.caption_trie_mask_ragged, ops.caption_trie_advance_ragged
and ops.trie_beam_select_sets, on the MI355X, each against its host statement (decoding_host.trie_mask_ragged_host /
trie_advance_ragged_host / trie_beam_select_sets_host); every device buffer a kernel writes carries guard words behind it.

Mask / advance: R = 6 rows, N = 2 rows per image, prompt lengths 1 / 5 / 3, a forest of two sets (images 0 and 2 answer from set 0,
image 1 from set 1, whose root is not node 0), walked column by column behind a scripted chooser that also writes a tempting token
and a log-prob into the forced rows.  V in {70, 257} as the issue sets them; a node that holds every token but the EOS has V - 1
children, which is 256 at V = 257 -- exactly one pass of the 256-thread gather.  So that the strided gather wraps, V = 515 is run as
well, with a node of 257 children beside the one of 514.  Select: B = 3 images, W in {2, 8}, three sets with longest 1 / 3 / 2 and
prompt lengths 1 / 4 / 2, every step of a search from the first column to the last."""
import numpy as np
import pytest
import torch

from image2text_amd.caption_plan import BEAM_DEAD
from image2text_amd.decoding_host import (beam_advance_host, trie_advance_ragged_host, trie_beam_candidates_host, trie_beam_select_sets_host,
                                          trie_mask_host, trie_mask_ragged_host)
from image2text_amd.phrase_trie import phrase_forest, phrase_trie

pytestmark = pytest.mark.gpu

f32, i32 = np.float32, np.int32
GUARD = 64                                      # guard words behind every buffer


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


class Guarded:
    """a device copy of a numpy array with GUARD sentinel words behind it"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.sentinel = {np.dtype(f32): 12345.5, np.dtype(i32): -77777, np.dtype(np.int64): -77777}[a.dtype]
        self.whole = torch.full((a.size + GUARD,), self.sentinel, dtype=torch.from_numpy(a).dtype, device=dev())
        self.t = self.whole[:a.size].view(a.shape)
        self.t.copy_(torch.from_numpy(a))

    def intact(self):
        return bool((self.whole[-GUARD:] == self.sentinel).all())

    def np(self):
        return self.t.cpu().numpy()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(i32)


# ------------------------------------------------------------------------------------------------------ mask / advance
R, N, PLEN, SET_OF = 6, 2, (1, 5, 3), (0, 1, 0)
IDS_LD = 12
CHOOSER_LP = 123.0                              # what the scripted chooser leaves in tok_lp: the advance kernel writes over it, or not


def walk_case(V):
    """the forest, the rows' scripts and the prompts of one vocabulary"""
    eos = V - 3
    allowed = np.setdiff1d(np.arange(V), [eos])
    A, Bt, C = 10, 11, 12                       # set 0's first tokens: A a node with every token but the EOS below it, Bt a phrase of its own
    set0 = [[Bt]] + [[A, int(t)] for t in allowed]
    if V > 300:                                 # a node of 257 children: one pass of the 256 threads and one thread more
        set0 += [[C, int(t)] for t in allowed[:257]]
    set1 = [[3], [3, 4], [5, 6, 7]]
    forest = phrase_forest([set0, set1], eos, V)
    assert forest.max_fanout == V - 1 and int(forest.roots[1]) > 0
    wide = [C, int(allowed[256])] if V > 300 else [A, int(allowed[5])]
    scripts = [[A, int(allowed[-1]), eos], [Bt, eos],           # image 0 (set 0, prompt 1)
               [3, 4, eos], [5, 6, 7, eos],                     # image 1 (set 1, prompt 5)
               wide + [eos], [A, int(allowed[0]), eos]]         # image 2 (set 0, prompt 3)
    return forest, eos, scripts


@pytest.mark.parametrize('V', [70, 257, 515])
def test_mask_and_advance_walk(ops, V):
    forest, eos, scripts = walk_case(V)
    ld = (V + 63) // 64 * 64
    g = np.random.default_rng(V)
    plen_rows = np.repeat(np.array(PLEN, dtype=i32), N)
    roots = np.repeat(forest.roots[list(SET_OF)], N).astype(i32)
    prompt = g.integers(0, V, (R, IDS_LD)).astype(np.int64)
    t_off, t_tok, t_nxt, t_term = (up(a) for a in (forest.child_off, forest.child_tok, forest.child_next, forest.term))
    kept_ld = (forest.max_fanout + 1 + 3) // 4 * 4
    plen_dev, done = up(np.array(PLEN, dtype=i32)), torch.zeros(1, dtype=torch.int32, device=dev())
    ids = np.zeros((R, IDS_LD), dtype=np.int64)
    ids[:, 0] = prompt[:, 0]
    node, phrase, finished = roots.copy(), np.full(R, -1, dtype=i32), np.zeros(R, dtype=i32)
    tok_lp = np.zeros((R, IDS_LD), dtype=f32)
    seen_forced = seen_wrap = 0
    for ln in range(1, max(PLEN) + 5):
        forced = ln < plen_rows
        z = (g.standard_normal((R, ld)) * 3).astype(f32)
        z[:, V:] = 1e30
        z[:, 6] = -np.inf
        zr, zp = Guarded(z), Guarded(z)
        lse_r, lse_p = Guarded(np.full(R, 55.5, dtype=f32)), Guarded(np.full(R, 55.5, dtype=f32))
        kept_r, kept_p = Guarded(np.full((R, kept_ld), 66.5, dtype=f32)), Guarded(np.full((R, kept_ld), 66.5, dtype=f32))
        len_ptr = up(np.array([ln], dtype=i32))
        node_r, node_p = Guarded(node), Guarded(node)
        ops.caption_trie_mask_ragged(zr.t, ld, node_r.t, t_off, t_tok, t_term, eos, done, lse_r.t, kept_r.t, len_ptr, plen_dev, N, R, V)
        ops.caption_trie_mask(zp.t, ld, node_p.t, t_off, t_tok, t_term, eos, done, lse_p.t, kept_p.t, R, V)
        got, plain = zr.np(), zp.np()
        for r in range(R):
            want = trie_mask_ragged_host(z[r, :V], int(node[r]), forest, eos, ln, int(plen_rows[r]))
            assert np.array_equal(bits(got[r, :V]), bits(want)), (ln, r)
            if forced[r]:
                assert np.array_equal(bits(got[r]), bits(z[r])), 'a forced row stays raw'
                assert lse_r.np()[r] == f32(55.5) and (kept_r.np()[r] == f32(66.5)).all(), 'raw_lse and kept of a forced row are not written'
            else:
                assert np.array_equal(bits(got[r]), bits(plain[r])) and np.array_equal(bits(lse_r.np()[r]), bits(lse_p.np()[r]))
                assert np.array_equal(bits(kept_r.np()[r]), bits(kept_p.np()[r])), 'the other rows: the plain kernel, bit for bit'
                assert np.array_equal(bits(got[r, :V]), bits(trie_mask_host(z[r, :V], int(node[r]), forest, eos)))
                seen_wrap += int(np.diff(forest.child_off)[node[r]] > 256)
        assert np.array_equal(bits(got[:, V:]), bits(z[:, V:])), 'the pad columns are not touched'
        # the scripted chooser: the row's next token, or -- forced or finished -- a child of the row's node, to tempt the advance kernel
        for r in range(R):
            k = ln - int(plen_rows[r])
            toks = forest.children(int(node[r]))[0]
            ids[r, ln] = scripts[r][k] if 0 <= k < len(scripts[r]) else (int(toks[0]) if toks.size else eos)
            tok_lp[r, ln] = CHOOSER_LP
        ids_r, lp_r, ph_r, fin = Guarded(ids), Guarded(tok_lp), Guarded(phrase), up(finished)
        lp_p, ph_p = Guarded(tok_lp), Guarded(phrase)
        ops.caption_trie_advance_ragged(ids_r.t, IDS_LD, len_ptr, fin, zr.t, ld, lse_r.t, t_off, t_tok, t_nxt, t_term, eos, done, node_r.t, ph_r.t,
                                        lp_r.t, plen_dev, N, R, V)
        ops.caption_trie_advance(ids_r.t, IDS_LD, len_ptr, fin, zp.t, ld, lse_p.t, t_off, t_tok, t_nxt, t_term, eos, done, node_p.t, ph_p.t, lp_p.t,
                                 R, V)
        for r in range(R):
            if finished[r]:
                want_node, want_ph, wrote = int(node[r]), int(phrase[r]), False
            else:
                want_node, want_ph, wrote = trie_advance_ragged_host(int(node[r]), int(ids[r, ln]), forest, eos, ln, int(plen_rows[r]))
                want_ph = want_ph if want_ph >= 0 else int(phrase[r])
            assert int(node_r.np()[r]) == want_node and int(ph_r.np()[r]) == want_ph, (ln, r)
            if forced[r]:
                seen_forced += 1
                assert not wrote and want_node == int(node[r]) == int(roots[r]), 'a forced row holds its trie state still'
                assert lp_r.np()[r, ln] == f32(CHOOSER_LP), 'tok_lp of a forced row is left to the finish rule'
            else:
                assert int(node_r.np()[r]) == int(node_p.np()[r]) and int(ph_r.np()[r]) == int(ph_p.np()[r])
                assert np.array_equal(bits(lp_r.np()[r]), bits(lp_p.np()[r])), 'the other rows: the plain kernel, bit for bit'
                assert (lp_r.np()[r, ln] != f32(CHOOSER_LP)) == wrote
        assert np.array_equal(bits(np.delete(lp_r.np(), ln, axis=1)), bits(np.delete(tok_lp, ln, axis=1))), 'only column len is written'
        assert all(b.intact() for b in (zr, zp, lse_r, lse_p, kept_r, kept_p, node_r, node_p, ids_r, lp_r, ph_r, lp_p, ph_p)), ln
        # what i2t_caption_finish_ragged does next: the prompt over a forced column, EOS finishes a row
        node, phrase, tok_lp = node_r.np().copy(), ph_r.np().copy(), lp_r.np().copy()
        for r in range(R):
            if forced[r]:
                ids[r, ln], tok_lp[r, ln] = prompt[r, ln], 0.0
            elif finished[r]:
                ids[r, ln], tok_lp[r, ln] = eos, 0.0
            elif ids[r, ln] == eos:
                finished[r] = 1
    assert finished.all() and seen_forced == N * sum(p - 1 for p in PLEN)
    assert seen_wrap > 0 or V <= 257
    # every row named a phrase of ITS OWN set: [3, 4] and [5, 6, 7] are phrases 1 and 2 of set 1, [Bt] is phrase 0 of set 0
    assert phrase[2] == 1 and phrase[3] == 2 and phrase[1] == 0 and phrase[0] > 0 and phrase[4] > 0 and phrase[5] > 0
    # nothing is written under done
    done.fill_(1)
    zr, lse_r, kept_r, node_r = Guarded(z), Guarded(np.full(R, 55.5, dtype=f32)), Guarded(np.full((R, kept_ld), 66.5, dtype=f32)), Guarded(roots)
    lp_r, ph_r = Guarded(tok_lp), Guarded(np.full(R, -1, dtype=i32))
    len_ptr = up(np.array([max(PLEN)], dtype=i32))
    ops.caption_trie_mask_ragged(zr.t, ld, node_r.t, t_off, t_tok, t_term, eos, done, lse_r.t, kept_r.t, len_ptr, plen_dev, N, R, V)
    ops.caption_trie_advance_ragged(up(ids), IDS_LD, len_ptr, up(np.zeros(R, dtype=i32)), zr.t, ld, lse_r.t, t_off, t_tok, t_nxt, t_term, eos, done,
                                    node_r.t, ph_r.t, lp_r.t, plen_dev, N, R, V)
    assert np.array_equal(bits(zr.np()), bits(z)) and (lse_r.np() == f32(55.5)).all() and (kept_r.np() == f32(66.5)).all()
    assert np.array_equal(node_r.np(), roots) and (ph_r.np() == -1).all() and np.array_equal(bits(lp_r.np()), bits(tok_lp))


def test_mask_and_advance_refusals(ops):
    from image2text_amd import lib as i2tlib
    V = 70
    forest, eos, _ = walk_case(V)
    ld = 128
    I = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    F = lambda *s: torch.zeros(*s, device=dev())
    t_off, t_tok, t_nxt, t_term = (up(a) for a in (forest.child_off, forest.child_tok, forest.child_next, forest.term))
    m = dict(logits=F(R, ld), ld=ld, node=I(R), child_off=t_off, child_tok=t_tok, term=t_term, eos=eos, done=I(1), raw_lse=F(R), kept=F(R, 72),
             len_ptr=I(1), plen=I(4), N=N, R=R, V=V)
    a = dict(ids=torch.zeros(R, IDS_LD, dtype=torch.long, device=dev()), ids_ld=IDS_LD, len_ptr=I(1), finished=I(R), logits=F(R, ld), ld=ld,
             raw_lse=F(R), child_off=t_off, child_tok=t_tok, child_next=t_nxt, term=t_term, eos=eos, done=I(1), node=I(R), phrase_index=I(R),
             tok_lp=F(R, IDS_LD), plen=I(4), N=N, R=R, V=V)
    for fn, base, name in ((ops.caption_trie_mask_ragged, m, 'i2t_caption_trie_mask_ragged'),
                           (ops.caption_trie_advance_ragged, a, 'i2t_caption_trie_advance_ragged')):
        for change, text in ((dict(N=0), 'N = 0'), (dict(N=4), 'not whole groups of N = 4'), (dict(plen=None), 'null plen'),
                             (dict(plen=I(8)[1:5]), 'misaligned plen'), (dict(eos=V), 'eos = 70'), (dict(ld=V - 1), 'ld = 69')):
            with pytest.raises(i2tlib.I2TError, match=text) as e:
                fn(**{**base, **change})
            assert name in str(e.value)


# ------------------------------------------------------------------------------------------------------ select
SV, SLD, SEOS = 67, 68, 5
SETS = [[[10], [11], [12], [13]],                                                           # longest 1
        [[10, 20, 30], [10, 20, 31], [10, 21], [13], [14, 22, 32], [14, 22], [15, 23, 33], [16], [17, 24, 34], [18, 25]],   # longest 3
        [[10, 20], [15], [16, 23], [10], [17, 26], [18, 27], [19, 28]]]                     # longest 2
SPLEN = (1, 4, 2)
INTS = ('node', 'ids', 'hist', 'pool_phrase', 'pool_len', 'pool_n', 'closed', 'counters', 'ctrl')
EXACT = ('path', 'pool_sum')


def _search_state(B, W, ids_ld, hist_ld, roots, g):
    Rr = B * W
    node = np.full((B, W), -1, dtype=i32)
    node[:, 0] = roots
    return dict(node=node.reshape(-1), path=np.zeros(Rr, dtype=f32), ids=g.integers(0, SV, (Rr, ids_ld)).astype(np.int64),
                hist=g.integers(0, Rr, (Rr, hist_ld)).astype(i32), pool_phrase=np.full((B, W), -1, dtype=i32), pool_sum=np.zeros((B, W), dtype=f32),
                pool_score=np.full((B, W), BEAM_DEAD, dtype=f32), pool_len=np.zeros((B, W), dtype=i32), pool_n=np.zeros(B, dtype=i32),
                closed=np.zeros(B, dtype=i32), counters=np.array([0, 1], dtype=i32), ctrl=np.zeros(2, dtype=i32))


@pytest.mark.parametrize('penalty', [0.0, 1.0])
@pytest.mark.parametrize('W', [2, 8])
def test_select_sets_over_a_search(ops, W, penalty):
    B = 3
    forest = phrase_forest(SETS, SEOS, SV)
    assert forest.longest.tolist() == [1, 3, 2]
    plen, longest_of = np.array(SPLEN, dtype=i32), forest.longest.astype(i32)
    pmax = int(plen.max())
    ids_ld, hist_ld = pmax + int(longest_of.max()) + 1 + 2, 40
    g = np.random.default_rng(W * 10 + int(penalty))
    s = _search_state(B, W, ids_ld, hist_ld, forest.roots, g)
    d = {k: Guarded(v) for k, v in s.items()}
    t_tok, t_nxt, t_term = up(forest.child_tok), up(forest.child_next), up(forest.term)
    plen_dev, longest_dev = up(plen), up(longest_of)
    forced_seen = 0
    for step in range(pmax - 1 + int(longest_of.max()) + 1):
        ln, pos = int(s['counters'][1]), int(s['counters'][0])
        if s['ctrl'][0]:
            break
        z = (g.standard_normal((B * W, SLD)) * 2).astype(f32)
        edge, total, fin, _ = trie_beam_candidates_host(z, s['node'], s['path'], forest, SEOS, W, V=SV)
        before = {k: v.copy() for k, v in s.items()}
        trie_beam_select_sets_host(edge, total, fin, s['node'], s['path'], forest, SEOS, s['ids'], s['hist'], s['pool_phrase'], s['pool_sum'],
                                   s['pool_score'], s['pool_len'], s['pool_n'], s['closed'], s['counters'], s['ctrl'], W, pmax, plen, longest_of,
                                   penalty)
        ops.trie_beam_select_sets(up(edge), up(total), up(fin), d['node'].t, d['path'].t, t_tok, t_nxt, t_term, SEOS, d['ids'].t, d['hist'].t,
                                  d['pool_phrase'].t, d['pool_sum'].t, d['pool_score'].t, d['pool_len'].t, d['pool_n'].t, d['closed'].t,
                                  d['counters'].t[0:1], d['counters'].t[1:2], d['ctrl'].t, B, W, pmax, plen_dev, longest_dev, penalty)
        for phase in ('select', 'advance'):
            for k in INTS:
                assert np.array_equal(d[k].np(), s[k]), (step, phase, k)
            for k in EXACT:
                assert np.array_equal(bits(d[k].np()), bits(s[k])), (step, phase, k)
            got = d['pool_score'].np()
            assert bool((np.abs(got.astype(np.float64) - s['pool_score']) <= 2 * np.spacing(np.abs(s['pool_score']))).all()), (step, phase)
            if phase == 'select':
                for b in range(B):
                    rows = slice(b * W, (b + 1) * W)
                    if ln < plen[b]:                            # a forced image: the identity history column, everything else as it was
                        forced_seen += 1
                        assert s['hist'][rows, pos].tolist() == list(range(b * W, (b + 1) * W)) and s['ctrl'][1] == 1
                        assert all(np.array_equal(s[k][rows], before[k][rows]) for k in ('node', 'path', 'ids'))
                        assert np.array_equal(np.delete(s['hist'][rows], pos, axis=1), np.delete(before['hist'][rows], pos, axis=1))
                        assert s['pool_n'][b] == 0 and s['closed'][b] == 0
                beam_advance_host(s['counters'], s['ctrl'])
                ops.beam_advance(d['counters'].t, d['ctrl'].t)
    assert forced_seen == sum(p - 1 for p in SPLEN)
    assert s['closed'].all(), 'every image ran to its end'
    assert all(v.intact() for v in d.values())
    n = np.minimum(s['pool_n'], W)
    for b in range(B):                                          # phrase indices are the sets' own
        assert n[b] >= 1 and (s['pool_phrase'][b, :n[b]] < len(SETS[b])).all() and (s['pool_len'][b, :n[b]] <= longest_of[b] + 1).all()


@pytest.mark.parametrize('W', [2, 8])
def test_select_sets_with_a_null_plen_is_the_plain_kernel(ops, W):
    B, P = 3, 2
    trie = phrase_trie(SETS[1], SEOS, SV, 1 << 30)
    g = np.random.default_rng(W)
    t_tok, t_nxt, t_term = up(trie.child_tok), up(trie.child_next), up(trie.term)
    longest_dev = up(np.full(B, trie.longest, dtype=i32))
    for t in range(trie.longest + 1):
        s = _search_state(B, W, P + trie.longest + 3, 16, np.zeros(B, dtype=i32), g)
        live = np.flatnonzero(np.diff(trie.child_off) > 0)
        s['node'] = g.choice(np.concatenate([live, np.arange(trie.nodes), [-1]]), B * W).astype(i32)
        s['path'] = (-g.random(B * W, dtype=f32) * 4).astype(f32)
        s['counters'] = np.array([3, P + t], dtype=i32)
        z = (g.standard_normal((B * W, SLD)) * 2).astype(f32)
        edge, total, fin, _ = trie_beam_candidates_host(z, s['node'], s['path'], trie, SEOS, W, V=SV)
        a, b = {k: Guarded(v) for k, v in s.items()}, {k: Guarded(v) for k, v in s.items()}
        ops.trie_beam_select_sets(up(edge), up(total), up(fin), a['node'].t, a['path'].t, t_tok, t_nxt, t_term, SEOS, a['ids'].t, a['hist'].t,
                                  a['pool_phrase'].t, a['pool_sum'].t, a['pool_score'].t, a['pool_len'].t, a['pool_n'].t, a['closed'].t,
                                  a['counters'].t[0:1], a['counters'].t[1:2], a['ctrl'].t, B, W, P, None, longest_dev, 1.0)
        ops.trie_beam_select(up(edge), up(total), up(fin), b['node'].t, b['path'].t, t_tok, t_nxt, t_term, SEOS, b['ids'].t, b['hist'].t,
                             b['pool_phrase'].t, b['pool_sum'].t, b['pool_score'].t, b['pool_len'].t, b['pool_n'].t, b['closed'].t,
                             b['counters'].t[0:1], b['counters'].t[1:2], b['ctrl'].t, B, W, P, trie.longest, 1.0)
        for k in s:
            assert torch.equal(a[k].whole, b[k].whole), (t, k)
        assert not np.array_equal(a['node'].np(), s['node']), 'the step did something'


def test_select_sets_refusals_and_done(ops):
    from image2text_amd import lib as i2tlib
    forest = phrase_forest(SETS, SEOS, SV)
    B, W = 2, 2
    Rr = B * W
    I = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev())
    F = lambda *s: torch.zeros(*s, device=dev())
    sel = dict(cand_edge=I(Rr, W), cand_total=F(Rr, W), fin_total=F(Rr), node=I(Rr), path=F(Rr), child_tok=up(forest.child_tok),
               child_next=up(forest.child_next), term=up(forest.term), eos=SEOS, ids=torch.zeros(Rr, 8, dtype=torch.long, device=dev()), hist=I(Rr, 16),
               pool_phrase=I(B, W), pool_sum=F(B, W), pool_score=F(B, W), pool_len=I(B, W), pool_n=I(B), closed=I(B), pos_ptr=I(1), len_ptr=I(1),
               ctrl=I(2), B=B, W=W, P=2, plen=I(4), longest_of=I(4), length_penalty=0.0)
    for change, text in ((dict(longest_of=None), 'null longest_of'), (dict(plen=I(8)[1:5]), 'misaligned'), (dict(longest_of=I(8)[1:5]), 'misaligned'),
                         (dict(P=0), 'P = 0'), (dict(P=7), 'ids_ld = 8'), (dict(eos=-1), 'eos = -1'), (dict(length_penalty=float('nan')), 'length_penalty')):
        with pytest.raises(i2tlib.I2TError, match=text) as e:
            ops.trie_beam_select_sets(**{**sel, **change})
        assert 'i2t_trie_beam_select_sets' in str(e.value)
    # ctrl[0] set: a forced image writes nothing either
    sel['ctrl'][0] = 1
    sel['plen'].fill_(5)
    sel['longest_of'].fill_(2)
    sel['hist'].fill_(9)
    ops.trie_beam_select_sets(**sel)
    assert bool((sel['hist'] == 9).all()) and sel['ctrl'].tolist() == [1, 0]
