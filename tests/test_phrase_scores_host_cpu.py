"""Host side of score_phrases, no GPU: ``trie_levels`` and its static history tables on hand-written sets (against a
brute-force ancestor walk), ``level_expand_tables``, ``phrase_scores_host`` -- the normative replica -- against a direct per-phrase sum
in fp64, the hand-written case in which the greedy walk of ``constrained_decode_host`` ends at a phrase that is not the most likely one
(the case the call exists for), every refusal with its text, and the replica over the CPU oracle's forward against the oracle's own
per-caption log-likelihood on the tiny model."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import (PhraseScores, PhraseTrie, check_phrase_score_args, constrained_decode_host, level_expand_tables,
                                     phrase_node_csr, phrase_scores_host, phrase_trie, trie_levels)

V, EOS = 12, 11
# 0: [3 5]   1: [3 5 7] (0 is its prefix)   2: [3 2]   3: [9] (one token)   4: [3 5] again   5: [1 4 4]
SET = [[3, 5], [3, 5, 7], [3, 2], [9], [3, 5], [1, 4, 4]]
WIDE_FIRST = [[4], [2], [7], [2, 3]]            # three nodes at depth 1, one at depth 2
SETS = (SET, WIDE_FIRST, [[6]], [[1, 2, 3, 4]], [[5], [5]])


def walk(trie, phrase):
    n = 0
    for t in phrase:
        toks, nxt = trie.children(n)
        n = int(nxt[toks.tolist().index(t)])
    return n


def parents_by_scan(trie):
    """node -> (parent, token), from the CSR arrays alone"""
    out = {}
    for n in range(trie.nodes):
        toks, nxt = trie.children(n)
        for t, c in zip(toks.tolist(), nxt.tolist()):
            out[c] = (n, t)
    return out


def depth_of(node, up):
    d = 0
    while node:
        node, d = up[node][0], d + 1
    return d


def test_trie_levels_on_hand_written_sets():
    trie = phrase_trie(SET, EOS, V, 4)
    lv = trie_levels(trie)
    assert len(lv.levels) == trie.longest + 1 == 4 and lv.wmax == 3
    assert [l.nodes.shape[0] for l in lv.levels] == [1, 3, 3, 2], 'level 2 is wider than its successor'
    n = lambda p: walk(trie, p)
    assert lv.levels[0].nodes.tolist() == [0] and lv.levels[0].parent_rows.tolist() == [-1] and lv.levels[0].tokens.tolist() == [-1]
    assert sorted(lv.levels[1].nodes.tolist()) == sorted([n([3]), n([9]), n([1])])
    assert sorted(lv.levels[2].nodes.tolist()) == sorted([n([3, 5]), n([3, 2]), n([1, 4])])
    assert sorted(lv.levels[3].nodes.tolist()) == sorted([n([3, 5, 7]), n([1, 4, 4])])
    for l in lv.levels:
        assert all(a.dtype == np.int32 for a in l[:6])
        assert (np.diff(l.nodes) > 0).all() and l.rows.tolist() == list(range(l.nodes.shape[0])), 'node order, row = rank'
        assert np.array_equal(l.term, trie.term[l.nodes])
    # the prefix phrase and its duplicate end at one node of level 2; the one-token phrase at level 1
    l1, l2 = lv.levels[1], lv.levels[2]
    assert l2.term[l2.nodes.tolist().index(n([3, 5]))] == 0 and l1.term[l1.nodes.tolist().index(n([9]))] == 3
    off, idx = phrase_node_csr(trie)
    assert idx[off[n([3, 5])]:off[n([3, 5]) + 1]].tolist() == [0, 4] and idx[off[n([9])]:off[n([9]) + 1]].tolist() == [3]
    assert off[0] == off[1] == 0 and off[-1] == len(SET) and sorted(idx.tolist()) == list(range(len(SET)))
    wide = trie_levels(phrase_trie(WIDE_FIRST, EOS, V, 3))
    assert [l.nodes.shape[0] for l in wide.levels] == [1, 3, 1] and wide.wmax == 3
    one = trie_levels(phrase_trie([[6]], EOS, V, 2))
    assert [l.nodes.tolist() for l in one.levels] == [[0], [1]] and one.wmax == 1


@pytest.mark.parametrize('phrases', SETS)
def test_parent_rows_tokens_and_history_against_an_ancestor_walk(phrases):
    trie = phrase_trie(phrases, EOS, V, 8)
    lv = trie_levels(trie)
    up = parents_by_scan(trie)
    row_of = {int(nd): (t, w) for t, l in enumerate(lv.levels) for w, nd in enumerate(l.nodes.tolist())}
    assert len(row_of) == trie.nodes and all(depth_of(nd, up) == t for nd, (t, _) in row_of.items())
    assert lv.wmax == max(l.nodes.shape[0] for l in lv.levels)
    first, clen = 5, 5 + trie.longest + 3
    for t, l in enumerate(lv.levels):
        hist = lv.history(t, first, clen)
        assert hist.shape == (lv.wmax, clen) and hist.dtype == np.int32 and l.anc.shape == (lv.wmax, t + 1)
        for w in range(lv.wmax):
            want = np.full(clen, w)
            if w < l.nodes.shape[0]:
                nd = int(l.nodes[w])
                if t:
                    assert (int(l.nodes[w]), int(l.tokens[w])) == (nd, up[nd][1]) and row_of[up[nd][0]] == (t - 1, int(l.parent_rows[w]))
                at = nd
                for j in range(t, -1, -1):                      # the depth-j ancestor wrote slot first + j in the row it held
                    assert row_of[at] == (j, int(l.anc[w, j]))
                    if 0 < j < t:
                        want[first + j] = row_of[at][1]
                    at = up[at][0] if j else at
            else:
                assert l.anc[w].tolist() == [w] * (t + 1), 'a row without a node keeps the identity'
            assert hist[w].tolist() == want.tolist(), f'level {t} row {w}'


@pytest.mark.parametrize('phrases', SETS)
def test_level_expand_tables(phrases):
    trie = phrase_trie(phrases, EOS, V, 8)
    lv = trie_levels(trie)
    seen = []
    for t in range(trie.longest + 1):
        cp, ct, tr, to, tp = level_expand_tables(trie, lv, t)
        assert all(a.dtype == np.int32 for a in (cp, ct, tr, to, tp)) and to.shape == (tr.shape[0] + 1,) and to[0] == 0 and to[-1] == tp.shape[0]
        if t < trie.longest:
            nxt = lv.levels[t + 1]
            assert np.array_equal(cp, nxt.parent_rows) and np.array_equal(ct, nxt.tokens) and cp.max() < lv.levels[t].nodes.shape[0]
        else:
            assert cp.size == 0 and ct.size == 0
        for j, w in enumerate(tr.tolist()):
            nd = int(lv.levels[t].nodes[w])
            mine = tp[to[j]:to[j + 1]].tolist()
            assert mine and all(walk(trie, phrases[k]) == nd for k in mine) and int(trie.term[nd]) == min(mine)
            seen += mine
    assert sorted(seen) == list(range(len(phrases))), 'every phrase, duplicates included, ends in exactly one table'


def table_logits(seed, vocab, scale):
    """a logits function that is a fixed random row per token sequence"""
    rows = {}

    def f(seq):
        key = tuple(int(t) for t in seq)
        if key not in rows:
            rng = np.random.default_rng([seed, len(key)] + [t + 1 for t in key])
            rows[key] = (rng.uniform(-1, 1, vocab) * scale).astype(np.float32)
        return rows[key]
    return f


@pytest.mark.parametrize('seed', range(8))
def test_phrase_scores_host_against_a_direct_sum(seed):
    """to 1e-6 absolute: the sets hold at most two tokens per phrase (three terms with the EOS) over 6 tokens with logits in [-0.5, 0.5],
    so a term is about -1.8 and a sum stays below 8 in magnitude -- fp32 carries it to a few 1e-7"""
    vocab, eos = 6, 5
    phrases = [[0], [0, 1], [2, 3], [2, 4], [0, 1], [3]]
    f = table_logits(seed, vocab, 0.5)
    prompt = [1, 2]
    got = phrase_scores_host(f, phrase_trie(phrases, eos, vocab, 4), eos, prompt=prompt)
    assert got.logprob.dtype == np.float32 and got.lengths.tolist() == [len(p) + 1 for p in phrases]
    want = []
    for ph in phrases:
        total, seq = 0.0, list(prompt)
        for t in ph + [eos]:
            z = f(seq).astype(np.float64)
            total += z[t] - np.log(np.exp(z).sum())
            seq.append(t)
        want.append(total)
    err = np.abs(got.logprob.astype(np.float64) - np.array(want))
    assert err.max() <= 1e-6, err
    assert got.logprob[1] == got.logprob[4], 'duplicate phrases get equal values'
    assert got.best == int(np.argmax(want)) or np.sort(want)[-1] - np.sort(want)[-2] < 2e-6


def test_greedy_walk_misses_the_most_likely_phrase():
    """Two phrases over 8 tokens.  At the root token 1 leads token 3 by 0.1, so the greedy walk takes [1 ...] and can never come back;
    behind 1 the model wants token 5, which the set does not hold, and [1 2] pays for it, while behind 3 the EOS is nearly certain."""
    vocab, eos = 8, 7
    phrases = [[1, 2], [3]]
    rows = {(0,): [0, 2.0, 0, 1.9, 0, 0, 0, 0], (0, 1): [0, 0, -3.0, 0, 0, 3.0, 0, 0], (0, 1, 2): [0, 0, 0, 0, 0, 0, 0, 0.5],
            (0, 3): [0, 0, 0, 0, 0, 0, 0, 5.0]}
    f = lambda seq: np.array(rows[tuple(seq)], dtype=np.float32)
    trie = phrase_trie(phrases, eos, vocab, 3)
    greedy = constrained_decode_host(f, [0], trie, eos, eos, 3)
    exact = phrase_scores_host(f, trie, eos, prompt=[0])
    assert greedy.phrase_index == 0 and greedy.ids.tolist() == [0, 1, 2, eos]
    assert exact.best == 1 and exact.logprob[1] > exact.logprob[0] + 5
    # both report the same quantity for the phrase the greedy walk took
    assert abs(float(greedy.logprob) - float(exact.logprob[0])) <= 1e-6


def test_refusals():
    ok = dict(eos=EOS, vocab=V, P=2, window=16)
    for bad, text in (([], 'phrases is empty'), ([[3], []], 'is empty'), ([[V]], 'outside the vocabulary'), ([[3, EOS]], 'holds eos_token_id'),
                      ([[2.5]], 'token ids are integers')):
        with pytest.raises(ValueError, match=text):
            check_phrase_score_args(bad, **ok)
    with pytest.raises(ValueError, match='need eos_token_id'):
        check_phrase_score_args(SET, **{**ok, 'eos': None})
    with pytest.raises(ValueError, match=r'eos_token_id = 12 outside the vocabulary'):
        check_phrase_score_args(SET, **{**ok, 'eos': V})
    with pytest.raises(NotImplementedError, match='a non-causal decoder has none'):
        check_phrase_score_args(SET, **ok, causal=False)
    with pytest.raises(NotImplementedError, match=r'sparse nano-mini decoder blocks.*slot_pos'):
        check_phrase_score_args(SET, **ok, sparse=True)
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(6\) exceed the text window \(5\)'):
        check_phrase_score_args(SET, **{**ok, 'window': 5})
    assert check_phrase_score_args(SET, **{**ok, 'window': 6}).longest == 3
    for n in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='images_per_pass = '):
            check_phrase_score_args(SET, **ok, images_per_pass=n)
    trie = check_phrase_score_args(SET, **ok, images_per_pass=3)
    assert isinstance(trie, PhraseTrie) and trie.phrase_node.tolist() == [walk(trie, p) for p in SET]
    assert check_phrase_score_args(trie, **ok) is trie, 'a trie is taken as it is'
    with pytest.raises(ValueError, match='built for another call'):
        check_phrase_score_args(trie, **{**ok, 'eos': 3})
    with pytest.raises(ValueError, match='without phrase_node'):
        check_phrase_score_args(trie._replace(phrase_node=None), **ok)
    assert PhraseScores._fields == ('logprob', 'best', 'lengths')


def test_replica_over_the_oracle_forward_equals_the_oracle_score(tiny_weights):
    """``phrase_scores_host`` fed the CPU oracle's forward, one prefix at a time, against the oracle's log-likelihood of the whole
    caption prompt + phrase + EOS from ONE forward.  Both are fp32 evaluations of the same causal function; they differ by the rounding
    of differently shaped products, some 1e-6 of logits of magnitude ~10: 1e-4 per scored token."""
    from image2text_amd.synth import synthetic_batch, tiny_config
    from oracle import reference_model as orc
    cfg = tiny_config()
    vocab = cfg.decoder_config.vocab_size
    sd = dict(tiny_weights)
    sd.setdefault('decoder.lm_head.weight', sd['decoder.transformer.wte.weight'])
    images, labels = synthetic_batch(2, 32, 12, min(vocab, 384), seed=0)
    prompt = labels[:, :2].clamp(min=0)
    eos = 5
    phrases = [[17, 42], [17, 42, 8], [17, 9], [63], [17, 9]]
    trie = phrase_trie(phrases, eos, vocab, 4)
    with torch.no_grad():
        for b in range(2):
            enc = orc.encode(sd, cfg, images[b:b + 1])
            f = lambda seq: orc.forward(sd, cfg, None, torch.tensor([seq]), encoder_output=enc)[1][0, -1].float().numpy()
            got = phrase_scores_host(f, trie, eos, prompt=prompt[b].tolist())
            for k, ph in enumerate(phrases):
                ids = torch.tensor([prompt[b].tolist() + ph + [eos]])
                lp = torch.log_softmax(orc.forward(sd, cfg, None, ids, encoder_output=enc)[1][0].double(), dim=-1)
                want = float(sum(lp[i - 1, ids[0, i]] for i in range(2, ids.shape[1])))
                assert abs(float(got.logprob[k]) - want) <= 1e-4 * (len(ph) + 1), (b, k, float(got.logprob[k]), want)
            assert got.logprob[2] == got.logprob[4]
