"""The host side of ``phrase_sets`` without a GPU: ``phrase_forest``, the three host statements of the new kernels, the
whole searches from a root that is not node 0, every refusal with its text and place, and the graph keys."""
import numpy as np
import pytest

from image2text_amd.caption_plan import (BEAM_DEAD, CaptionFacts, caption_graph_key, check_phrase_search_args, check_phrase_sets,
                                         phrase_beam_sets_graph_key, plan_captions)
from image2text_amd.decoding_host import (beam_advance_host, constrained_decode_host, phrase_beam_search_host, trie_advance_host,
                                          trie_advance_ragged_host, trie_beam_candidates_host, trie_beam_select_host, trie_beam_select_sets_host,
                                          trie_mask_host, trie_mask_ragged_host)
from image2text_amd.phrase_trie import PhraseForest, phrase_forest, phrase_trie

f32, i32 = np.float32, np.int32
V, EOS = 40, 5
# shared prefixes inside a set, a phrase that is a prefix of another (1 extends 0), a duplicate (4 repeats 2); [7, 8] also in set 1; a
# single-token set
SETS = [[[7, 8], [7, 8, 9], [7, 10], [11], [7, 10]], [[12, 13, 14], [7, 8], [12]], [[20]]]
FACTS = CaptionFacts(V, True, None, 64, 0, 64, False)


def test_forest_lays_the_tries_end_to_end():
    f = phrase_forest(SETS, EOS, V)
    tries = [phrase_trie(s, EOS, V, 1 << 30) for s in SETS]
    assert isinstance(f, PhraseForest) and f.sets == 3 and f.roots.tolist() == [0, tries[0].nodes, tries[0].nodes + tries[1].nodes]
    assert f.nodes == sum(t.nodes for t in tries) and f.edges == sum(t.edges for t in tries)
    assert f.longest.tolist() == [3, 3, 1] and f.widest.tolist() == [2, 2, 1] and f.max_fanout == 2 and f.distinct.tolist() == [4, 3, 1]
    assert all(a.dtype == i32 for a in (f.child_off, f.child_tok, f.child_next, f.term, f.roots, f.longest, f.widest))
    for s, (t, phrases) in enumerate(zip(tries, SETS)):
        for k, ph in enumerate(phrases):        # walking a phrase from the set's root ends at a node whose term is the index WITHIN the set
            nd, own = int(f.roots[s]), 0
            for tok in ph:
                toks, nxt = f.children(nd)
                assert np.all(np.diff(toks) > 0), 'child_tok ascends within a node'
                nd = int(nxt[toks.tolist().index(tok)])
                own = int(t.children(own)[1][t.children(own)[0].tolist().index(tok)])
            assert nd == own + int(f.roots[s]) and int(f.term[nd]) == phrases.index(ph) == int(t.term[own])
        lo, hi = int(f.roots[s]), int(f.roots[s]) + t.nodes
        assert np.all((f.child_next[f.child_off[lo]:f.child_off[hi]] >= lo) & (f.child_next[f.child_off[lo]:f.child_off[hi]] < hi)), 'no edge leaves its set'
    one = phrase_forest([SETS[0]], EOS, V)
    for name in ('child_off', 'child_tok', 'child_next', 'term'):
        assert np.array_equal(getattr(one, name), getattr(tries[0], name)) and getattr(one, name).dtype == getattr(tries[0], name).dtype, name
    assert one.roots.tolist() == [0] and one.max_fanout == tries[0].max_fanout and int(one.longest[0]) == tries[0].longest


def test_forest_refusals_name_the_set():
    for sets, text in (([], 'phrase_sets is empty'), ([SETS[0], []], r'phrase_sets\[1\]: phrases is empty'),
                       ([SETS[0], [[7], []]], r'phrase_sets\[1\]: phrases\[1\] is empty'), ([[[7, EOS]]], r'phrase_sets\[0\]: phrases\[0\] holds eos_token_id'),
                       ([SETS[0], SETS[1], [[V]]], r'phrase_sets\[2\]: phrases\[0\] holds 40: outside the vocabulary')):
        with pytest.raises(ValueError, match=text):
            phrase_forest(sets, EOS, V)
    with pytest.raises(ValueError, match=r'phrase_sets\[0\]: phrases need eos_token_id'):
        phrase_forest(SETS, None, V)
    with pytest.raises(ValueError, match=r'phrase_sets\[0\]: max_new_tokens = 3 is below the longest phrase \+ 1 = 4'):
        phrase_forest(SETS, EOS, V, 3)


def test_ragged_mask_and_advance_statements():
    f = phrase_forest(SETS, EOS, V)
    z = np.random.default_rng(0).standard_normal(V).astype(f32)
    root1 = int(f.roots[1])
    raw = trie_mask_ragged_host(z, root1, f, EOS, 2, 3)
    assert np.array_equal(raw.view(i32), z.view(i32)) and raw is not z, 'a forced column leaves the row raw'
    for ln in (3, 4):
        m = trie_mask_ragged_host(z, root1, f, EOS, ln, 3)
        assert np.array_equal(m.view(i32), trie_mask_host(z, root1, f, EOS).view(i32))
        assert np.flatnonzero(m > -np.inf).tolist() == [7, 12]
    assert trie_advance_ragged_host(root1, 12, f, EOS, 2, 3) == (root1, -1, False), 'a forced column holds the node still'
    nd, ph, ok = trie_advance_ragged_host(root1, 12, f, EOS, 3, 3)
    assert (nd, ph, ok) == trie_advance_host(root1, 12, f, EOS) and ok and nd != root1
    assert trie_advance_ragged_host(nd, EOS, f, EOS, 4, 3) == (nd, 2, True), 'term is the index within the set: [12] is phrase 2 of set 1'
    assert trie_advance_ragged_host(nd, EOS, f, EOS, 4, 5) == (nd, -1, False)


def _state(B, W, ids_ld, roots, g):
    node = np.full((B, W), -1, dtype=i32)
    node[:, 0] = roots
    return dict(node=node.reshape(-1), path=np.zeros(B * W, dtype=f32), ids=g.integers(0, V, (B * W, ids_ld)).astype(np.int64),
                hist=g.integers(0, B * W, (B * W, 12)).astype(i32), pool_phrase=np.full((B, W), -1, dtype=i32), pool_sum=np.zeros((B, W), dtype=f32),
                pool_score=np.full((B, W), BEAM_DEAD, dtype=f32), pool_len=np.zeros((B, W), dtype=i32), pool_n=np.zeros(B, dtype=i32),
                closed=np.zeros(B, dtype=i32), counters=np.array([0, 1], dtype=i32), ctrl=np.zeros(2, dtype=i32))


def _select(fn, s, cand, trie, W, *tail):
    fn(*cand, s['node'], s['path'], trie, EOS, s['ids'], s['hist'], s['pool_phrase'], s['pool_sum'], s['pool_score'], s['pool_len'], s['pool_n'],
       s['closed'], s['counters'], s['ctrl'], W, *tail)


def test_select_sets_statement():
    f = phrase_forest(SETS, EOS, V)
    B, W = 3, 2
    plen, longest_of = np.array([1, 3, 2], dtype=i32), f.longest.astype(i32)
    g = np.random.default_rng(1)
    s = _state(B, W, 8, f.roots, g)
    for step in range(6):
        if s['ctrl'][0]:
            break
        ln, pos = int(s['counters'][1]), int(s['counters'][0])
        z = g.standard_normal((B * W, V)).astype(f32)
        cand = trie_beam_candidates_host(z, s['node'], s['path'], f, EOS, W)[:3]
        before = {k: v.copy() for k, v in s.items()}
        # an image that is not forced: the plain statement on that image alone, with its own P and longest
        alone = {b: {k: v.copy() for k, v in s.items()} for b in range(B) if ln >= plen[b]}
        _select(trie_beam_select_sets_host, s, cand, f, W, int(plen.max()), plen, longest_of, 1.0)
        for b in range(B):
            rows = slice(b * W, (b + 1) * W)
            if ln < plen[b]:
                assert s['hist'][rows, pos].tolist() == list(range(b * W, (b + 1) * W)) and s['ctrl'][1] == 1
                assert all(np.array_equal(s[k][rows], before[k][rows]) for k in ('node', 'path', 'ids'))
                assert np.array_equal(np.delete(s['hist'][rows], pos, 1), np.delete(before['hist'][rows], pos, 1))
                assert all(np.array_equal(s[k][b], before[k][b]) for k in ('pool_phrase', 'pool_sum', 'pool_score', 'pool_len', 'pool_n', 'closed'))
            else:
                a = alone[b]
                a['closed'][:] = 1
                a['closed'][b] = before['closed'][b]
                a['ctrl'][:] = 0
                _select(trie_beam_select_host, a, cand, f, W, int(plen[b]), int(longest_of[b]), 1.0)
                assert all(np.array_equal(s[k][rows], a[k][rows]) for k in ('node', 'ids', 'hist')), (step, b)
                assert np.array_equal(s['path'][rows].view(i32), a['path'][rows].view(i32))
                for k in ('pool_phrase', 'pool_sum', 'pool_score', 'pool_len', 'pool_n', 'closed'):
                    assert np.array_equal(np.asarray(s[k][b]), np.asarray(a[k][b])), (step, b, k)
        beam_advance_host(s['counters'], s['ctrl'])
    assert s['closed'].all() and (s['pool_n'] >= 1).all()
    for b in range(B):
        assert (s['pool_phrase'][b, :s['pool_n'][b]] < len(SETS[b])).all() and (s['pool_len'][b, :s['pool_n'][b]] <= longest_of[b] + 1).all()
    # a null plen with equal longest_of is the plain statement
    t = phrase_trie(SETS[0], EOS, V, 1 << 30)
    a, b2 = _state(B, W, 8, np.zeros(B, dtype=i32), np.random.default_rng(2)), _state(B, W, 8, np.zeros(B, dtype=i32), np.random.default_rng(2))
    for s2 in (a, b2):
        s2['counters'][:] = [2, 3]
    cand = trie_beam_candidates_host(np.random.default_rng(3).standard_normal((B * W, V)).astype(f32), a['node'], a['path'], t, EOS, W)[:3]
    _select(trie_beam_select_sets_host, a, cand, t, W, 3, None, np.full(B, t.longest), 0.5)
    _select(trie_beam_select_host, b2, cand, t, W, 3, t.longest, 0.5)
    assert all(np.array_equal(a[k], b2[k]) for k in a) and not np.array_equal(a['node'], _state(B, W, 8, np.zeros(B, dtype=i32), np.random.default_rng(2))['node'])


def _scripted(seed):
    """step_logits of a scripted model: the row depends on the whole sequence, deterministically"""
    def f(seq):
        return np.random.default_rng([seed] + [int(t) for t in seq]).standard_normal(V).astype(f32) * 2
    return f


@pytest.mark.parametrize('s', [1, 2, 0])
def test_searches_from_a_root_equal_the_sets_own_trie(s):
    f = phrase_forest(SETS, EOS, V)
    own = phrase_trie(SETS[s], EOS, V, 1 << 30)
    root = int(f.roots[s])
    assert root > 0 or s == 0
    for seed in range(4):
        a = constrained_decode_host(_scripted(seed), [3, 4], f, EOS, 0, 5, start=root)
        b = constrained_decode_host(_scripted(seed), [3, 4], own, EOS, 0, 5)
        assert a.ids.tolist() == b.ids.tolist() and a.phrase_index == b.phrase_index and a.gaps == b.gaps
        assert np.array_equal(a.token_logprobs.view(i32), b.token_logprobs.view(i32))
        for W in (1, 2, 4):
            N = min(W, int(f.distinct[s]))
            x = phrase_beam_search_host(_scripted(seed), [3, 4], f, EOS, W, N, 0.5, start=root, longest=int(f.longest[s]))
            y = phrase_beam_search_host(_scripted(seed), [3, 4], own, EOS, W, N, 0.5)
            assert x.phrase_index.tolist() == y.phrase_index.tolist() and x.lengths.tolist() == y.lengths.tolist() and x.steps == y.steps
            assert np.array_equal(x.logprob.view(i32), y.logprob.view(i32)) and np.array_equal(x.scores.view(i32), y.scores.view(i32))


def plan(B=3, P=3, **kw):
    kw = {**dict(max_new_tokens=4, eos_token_id=EOS, top_k=1), **kw}
    return plan_captions(FACTS, B, P, **kw)


def test_plan_carries_the_forest():
    p = plan(phrase_sets=SETS, prompt_lengths=[1, 3, 2])
    assert p.trie is None and p.sets.index.tolist() == [0, 1, 2] and p.sets.roots.tolist() == p.sets.forest.roots.tolist()
    assert p.sets.longest.tolist() == [3, 3, 1] and p.plen.tolist() == [1, 3, 2] and (p.pmin, p.pmax) == (1, 3) and p.mode == 'cache'
    p = plan(phrase_sets=SETS, phrase_set_index=[2, 2, 2], max_new_tokens=2)       # only the sets in use count: set 2's longest phrase is 1
    assert p.sets.longest.tolist() == [1, 1, 1] and p.sets.widest == 1 and p.sets.smallest == 1 and p.plen is None
    p = plan(phrase_sets=SETS, phrase_set_index=[0, 0, 1], num_return_sequences=3, top_k=None, prompt_prefill='pass', prompt_lengths=[2, 3, 3])
    assert p.N == 3 and p.m == 1 and p.sets.index.tolist() == [0, 0, 1]
    with pytest.raises(AttributeError):
        p.sets = None                           # frozen
    assert plan().sets is None and plan(phrases=SETS[0]).sets is None and plan(phrases=SETS[0]).trie is not None


def test_refusals_texts_and_order():
    both = dict(phrases=SETS[0], phrase_sets=SETS)
    with pytest.raises(ValueError, match='phrases and phrase_sets are both given'):
        plan(**both, phrase_set_index=[9, 9, 9], num_beams=2)                      # before the index, before NotImplementedError
    with pytest.raises(ValueError, match='phrase_set_index without phrase_sets'):
        plan(phrase_set_index=[0, 0, 0])
    with pytest.raises(ValueError, match=r'phrase_sets\[1\]: phrases\[0\] is empty'):
        plan(phrase_sets=[SETS[0], [[]]], phrase_set_index=[0, 0, 7], num_beams=2)     # set refusals first
    with pytest.raises(ValueError, match=r'phrase_set_index\[2\] = 3 is outside the 3 sets'):
        plan(phrase_sets=SETS, phrase_set_index=[0, 1, 3])
    with pytest.raises(ValueError, match=r'phrase_set_index\[0\] = -1'):
        plan(phrase_sets=SETS, phrase_set_index=[-1, 1, 2])
    with pytest.raises(ValueError, match=r'phrase_set_index of shape \(2,\) for 3 images'):
        plan(phrase_sets=SETS, phrase_set_index=[0, 1])
    with pytest.raises(ValueError, match='integers are needed'):
        plan(phrase_sets=SETS, phrase_set_index=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match='one set per image: 3 sets for 4 images'):
        plan(B=4, phrase_sets=SETS)
    with pytest.raises(ValueError, match=r'max_new_tokens = 3 is below the longest phrase \+ 1 = 4 of the sets in use'):
        plan(phrase_sets=SETS, max_new_tokens=3, num_beams=2)                      # ValueError before NotImplementedError
    with pytest.raises(ValueError, match='repetition_penalty = -1'):
        plan(phrase_sets=SETS, repetition_penalty=-1, num_beams=2)                 # the processors' own ValueError before it too
    with pytest.raises(NotImplementedError, match='phrase_sets with repetition_penalty / min_new_tokens / suppress_tokens'):
        plan(phrase_sets=SETS, suppress_tokens=[3], num_beams=2)
    with pytest.raises(NotImplementedError, match='phrase_sets under num_beams > 1: the beam step has no trie state per hypothesis'):
        plan(phrase_sets=SETS, num_beams=2)
    with pytest.raises(NotImplementedError, match='phrase_sets run inside the KV-cache caption step; a non-causal decoder'):
        plan_captions(FACTS._replace(causal=False), 3, 3, 4, EOS, top_k=1, phrase_sets=SETS)
    # the pinned refusal of the old keyword stays
    with pytest.raises(NotImplementedError, match='phrases with prompt_lengths: a forced prompt column would have to hold the trie still'):
        plan(phrases=SETS[0], prompt_lengths=[1, 2, 3])


def search(**kw):
    kw = {**dict(phrases=None, eos=EOS, vocab=V, P=3, window=64, B=3), **kw}
    return check_phrase_search_args(**kw)


def test_search_refusals_and_result():
    sets, W, N, plen = search(phrase_sets=SETS, phrase_set_index=[0, 1, 1], prompt_lengths=[1, 3, 2], num_beams=4, num_return_sequences=3)
    assert (W, N) == (4, 3) and plen.tolist() == [1, 3, 2] and plen.dtype == i32 and sets.widest == 2 and sets.smallest == 3
    assert search(phrase_sets=SETS)[3] is None
    trie, W, N = check_phrase_search_args(SETS[0], EOS, V, 3, 64)                  # the old call, the old triple
    assert (W, N) == (4, 1) and trie.longest == 3
    with pytest.raises(ValueError, match='phrases and phrase_sets are both given'):
        search(phrases=SETS[0], phrase_sets=SETS)
    with pytest.raises(ValueError, match='needs phrase_sets'):
        search(phrases=SETS[0], prompt_lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='num_return_sequences = 2 with num_beams = 4 and 1 distinct phrases'):
        search(phrase_sets=SETS, num_return_sequences=2)                           # the smallest set in use holds one phrase
    with pytest.raises(ValueError, match='num_return_sequences = 5 with num_beams = 4'):
        search(phrase_sets=SETS, phrase_set_index=[0, 0, 0], num_return_sequences=5)
    with pytest.raises(ValueError, match=r'prompt_lengths\[1\] = 4 exceeds the 3 columns'):
        search(phrase_sets=SETS, prompt_lengths=[1, 4, 2])
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(7\) exceed the text window \(6\)'):
        search(phrase_sets=SETS, window=6, causal=False)                           # ValueError before NotImplementedError
    assert search(phrase_sets=SETS, phrase_set_index=[2, 2, 2], window=5)[0].longest.tolist() == [1, 1, 1]      # the sets in use
    with pytest.raises(NotImplementedError, match='search_phrases runs its beam over the trie on the KV cache'):
        search(phrase_sets=SETS, causal=False)
    with pytest.raises(NotImplementedError, match='search_phrases on sparse nano-mini decoder blocks'):
        search(phrase_sets=SETS, sparse=True)
    with pytest.raises(ValueError, match=r'phrase_sets\[2\]: phrases\[0\] holds eos_token_id = 5'):
        check_phrase_sets(None, [SETS[0], SETS[1], [[5]]], None, 3, EOS, V)


def test_graph_keys():
    plain, rag = caption_graph_key('greedy', EOS, 0), caption_graph_key('greedy', EOS, 0, 6)
    assert caption_graph_key('greedy', EOS, 0, sets=True) == ('trie_sets', EOS) + plain
    assert caption_graph_key('greedy', EOS, 0, 6, sets=True) == ('trie_sets', EOS) + rag == ('trie_sets', EOS, 'ragged', 'greedy', EOS, 0, 6)
    assert caption_graph_key('greedy', EOS, 0, trie=True) == ('trie', EOS) + plain, 'a phrases call keeps its key'
    assert caption_graph_key('greedy', EOS, 0, trie=True, sets=True)[0] == 'trie_sets'
    assert phrase_beam_sets_graph_key(4, 3, EOS, 0.5) == ('phrase_beam_sets', 4, 3, EOS, 0.5)
    assert len({caption_graph_key('greedy', EOS, 0, sets=True), caption_graph_key('greedy', EOS, 0, trie=True), plain, rag}) == 4
