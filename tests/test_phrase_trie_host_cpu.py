"""Host side of generate_captions(phrases=...), no GPU: ``phrase_trie`` on hand-written sets, ``trie_mask_host`` /
``trie_advance_host`` -- the normative statements of the two kernels -- on a hand-made table, ``constrained_decode_host`` on a scripted
``step_logits`` whose answer is known by hand, every refusal with its text, and the graph key."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import (GeneratedCaptions, Processors, caption_graph_key, check_phrase_caption_args, constrained_decode_host,
                                     phrase_trie, trie_advance_host, trie_mask_host)

V, EOS = 12, 11
# 0: [3 5]   1: [3 5 7] (0 is its prefix)   2: [3 2]   3: [9]   4: [3 5] again   5: [1 4 4]
SET = [[3, 5], [3, 5, 7], [3, 2], [9], [3, 5], [1, 4, 4]]


def walk(trie, phrase):
    n = 0
    for t in phrase:
        toks, nxt = trie.children(n)
        assert t in toks.tolist()
        n = int(nxt[toks.tolist().index(t)])
    return n


def well_formed(trie):
    assert all(a.dtype == np.int32 for a in (trie.child_off, trie.child_tok, trie.child_next, trie.term))
    assert trie.child_off.shape == (trie.nodes + 1,) and trie.child_off[0] == 0 and trie.child_off[-1] == trie.edges
    assert trie.child_next.shape == trie.child_tok.shape and (np.diff(trie.child_off) >= 0).all()
    assert int(np.diff(trie.child_off).max()) == trie.max_fanout
    for n in range(trie.nodes):
        toks, nxt = trie.children(n)
        assert (np.diff(toks) > 0).all(), f'node {n}: children not ascending'
        assert ((nxt > 0) & (nxt < trie.nodes)).all()
        assert toks.size or trie.term[n] >= 0, f'node {n}: a leaf that ends no phrase'
    assert sorted(trie.child_next.tolist()) == list(range(1, trie.nodes)), 'every node but the root has one parent'


def test_shared_prefixes_prefix_phrases_and_duplicates():
    trie = phrase_trie(SET, EOS, V, 4)
    well_formed(trie)
    assert trie.nodes == 9 and trie.edges == 8 and trie.max_fanout == 3            # root: 1, 3, 9
    assert trie.children(0)[0].tolist() == [1, 3, 9]
    assert trie.children(walk(trie, [3]))[0].tolist() == [2, 5]
    n35 = walk(trie, [3, 5])
    assert trie.term[n35] == 0, 'the duplicate keeps the lowest index'
    assert trie.children(n35)[0].tolist() == [7] and trie.term[walk(trie, [3, 5, 7])] == 1
    assert trie.term[walk(trie, [3, 2])] == 2 and trie.term[walk(trie, [9])] == 3 and trie.term[walk(trie, [1, 4, 4])] == 5
    assert trie.term[0] == -1 and trie.term[walk(trie, [3])] == -1 and trie.term[walk(trie, [1, 4])] == -1
    assert sorted(t for t in trie.term.tolist() if t >= 0) == [0, 1, 2, 3, 5]
    # tensors and tuples are taken as lists are
    same = phrase_trie([torch.tensor(p) for p in SET], EOS, V, 4)
    assert all(np.array_equal(a, b) for a, b in zip(trie[:4], same[:4])) and same.max_fanout == 3


def test_single_token_phrases_and_a_full_root():
    trie = phrase_trie([[4], [2], [7]], EOS, V, 2)
    well_formed(trie)
    assert trie.nodes == 4 and trie.max_fanout == 3 and trie.child_tok.tolist() == [2, 4, 7]
    assert [int(trie.term[n]) for n in trie.child_next] == [1, 0, 2]
    # a root fan-out of V - 1: every token but the EOS, given in descending order
    full = phrase_trie([[t] for t in range(V - 1, -1, -1) if t != EOS], EOS, V, 2)
    well_formed(full)
    assert full.max_fanout == V - 1 and full.child_tok.tolist() == [t for t in range(V) if t != EOS]
    assert [int(full.term[n]) for n in full.child_next] == [V - 1 - t - (1 if t < EOS else 0) for t in range(V) if t != EOS]


def test_mask_and_advance_on_a_hand_made_table():
    trie = phrase_trie(SET, EOS, V, 4)
    z = np.arange(V, dtype=np.float32) - 5
    z[2] = -np.inf
    inf = -np.inf

    def want(cols):
        out = np.full(V, inf, dtype=np.float32)
        out[cols] = z[cols]
        return out
    root = trie_mask_host(z, 0, trie, EOS)
    assert root.dtype == np.float32 and np.array_equal(root, want([1, 3, 9])) and root is not z
    n3, n35 = walk(trie, [3]), walk(trie, [3, 5])
    assert np.array_equal(trie_mask_host(z, n3, trie, EOS), want([2, 5]))                      # (the raw -inf of column 2 stays)
    assert np.array_equal(trie_mask_host(z, n35, trie, EOS), want([7, EOS])), 'a node that ends one phrase and continues another'
    assert np.array_equal(trie_mask_host(z, walk(trie, [9]), trie, EOS), want([EOS])), 'a leaf allows the EOS alone'
    assert z[0] == -5 and z[EOS] == 6, 'the input row is not written'
    # advance: a child moves the row, EOS at a terminal node names the phrase, anything else changes nothing
    assert trie_advance_host(0, 3, trie, EOS) == (n3, -1, True)
    assert trie_advance_host(n3, 5, trie, EOS) == (n35, -1, True)
    assert trie_advance_host(n35, EOS, trie, EOS) == (n35, 0, True)
    assert trie_advance_host(n35, 7, trie, EOS) == (walk(trie, [3, 5, 7]), -1, True)
    assert trie_advance_host(walk(trie, [3, 5, 7]), EOS, trie, EOS) == (walk(trie, [3, 5, 7]), 1, True)
    assert trie_advance_host(n3, EOS, trie, EOS) == (n3, -1, False), 'EOS where no phrase ends'
    assert trie_advance_host(0, 5, trie, EOS) == (0, -1, False) and trie_advance_host(n3, 10, trie, EOS) == (n3, -1, False)


def scripted(table):
    """step_logits from {sequence after the prompt: {token: logit}}; every other column -9, and the unconstrained best is token 0"""
    calls = []

    def f(seq):
        calls.append(tuple(seq))
        z = np.full(V, -9.0, dtype=np.float32)
        z[0] = 50.0                                             # what a free argmax would take: never allowed
        for t, v in table[tuple(seq[2:])].items():
            z[t] = v
        return z
    return f, calls


def lp_of(z, c):
    z = z.astype(np.float64)
    return z[c] - (z.max() + np.log(np.exp(z - z.max()).sum()))


def test_constrained_decode_on_a_script():
    trie = phrase_trie(SET, EOS, V, 4)
    # a child beats the EOS at [3 5]: -> [3 5 7] = phrase 1.  Gaps by hand: root 3 (4.0) vs 9 (1.5); [3]: 5 (2.0) vs 2 (-1.0);
    # [3 5]: 7 (0.5) vs EOS (0.25); [3 5 7]: the EOS alone
    f, calls = scripted({(): {3: 4.0, 9: 1.5, 1: -2.0, 5: 30.0}, (3,): {5: 2.0, 2: -1.0, 9: 40.0}, (3, 5): {7: 0.5, EOS: 0.25},
                         (3, 5, 7): {EOS: -3.0, 3: 20.0}})
    out = constrained_decode_host(f, [8, 8], trie, EOS, 0, 4)
    assert out.ids.tolist() == [8, 8, 3, 5, 7, EOS] and out.length == 6 and out.phrase_index == 1 and out.steps == 4
    assert out.gaps == [2.5, 3.0, 0.25, float('inf')]
    assert calls == [(8, 8), (8, 8, 3), (8, 8, 3, 5), (8, 8, 3, 5, 7)]
    want = [lp_of(f(list(c)), t) for c, t in zip(calls[:4], [3, 5, 7, EOS])]
    assert out.token_logprobs.dtype == np.float32 and np.allclose(out.token_logprobs, want, atol=1e-5)
    assert out.logprob == out.token_logprobs.sum(dtype=np.float32) and (out.token_logprobs < -10).all(), 'the RAW row: token 0 holds the mass'
    # the EOS beats the child at [3 5]: -> [3 5] = phrase 0 (the lowest index of the duplicates)
    f, _ = scripted({(): {3: 4.0, 9: 1.5}, (3,): {5: 2.0, 2: -1.0}, (3, 5): {7: 0.25, EOS: 0.5}})
    out = constrained_decode_host(f, [8, 8], trie, EOS, 0, 4)
    assert out.ids.tolist() == [8, 8, 3, 5, EOS] and out.phrase_index == 0 and out.gaps == [2.5, 3.0, 0.25]
    # a tie between two children: the lower id
    f, _ = scripted({(): {9: 1.0, 1: 1.0, 3: 0.0}, (1,): {4: 0.0}, (1, 4): {4: 0.0}, (1, 4, 4): {EOS: 0.0}})
    out = constrained_decode_host(f, [8, 8], trie, EOS, 0, 4)
    assert out.ids.tolist() == [8, 8, 1, 4, 4, EOS] and out.phrase_index == 5 and out.gaps[0] == 0.0


@pytest.mark.parametrize('phrases,eos,max_new,text', [
    ([], EOS, 4, 'phrases is empty'),
    ([[3], []], EOS, 4, r'phrases\[1\] is empty'),
    ([[3, V]], EOS, 4, rf'phrases\[0\] holds {V}: outside the vocabulary \[0, {V}\)'),
    ([[3], [-1]], EOS, 4, r'phrases\[1\] holds -1: outside the vocabulary'),
    ([[3, EOS, 2]], EOS, 4, rf'phrases\[0\] holds eos_token_id = {EOS}'),
    ([[3]], None, 4, 'phrases need eos_token_id'),
    ([[3]], V, 4, rf'eos_token_id = {V} outside the vocabulary'),
    ([[3, 5, 7], [2]], EOS, 3, r'max_new_tokens = 3 is below the longest phrase \+ 1 = 4'),
    ([[3.5]], EOS, 4, 'token ids are integers'),
])
def test_value_errors(phrases, eos, max_new, text):
    with pytest.raises(ValueError, match=text):
        phrase_trie(phrases, eos, V, max_new)
    with pytest.raises(ValueError, match=text):
        check_phrase_caption_args(phrases, eos, V, max_new, prompt_lengths=[1], num_beams=2)      # the set's own refusals come first


def test_max_new_tokens_at_the_bound_passes():
    assert phrase_trie([[3, 5, 7], [2]], EOS, V, 4).nodes == 5


@pytest.mark.parametrize('kw,text', [
    (dict(prompt_lengths=[1, 2]), 'phrases with prompt_lengths'),
    (dict(processors_active=True), 'phrases with repetition_penalty / min_new_tokens / suppress_tokens'),
    (dict(num_beams=2), 'phrases under num_beams > 1'),
    (dict(causal=False), 'non-causal decoder'),
])
def test_not_implemented_combinations(kw, text):
    with pytest.raises(NotImplementedError, match=text):
        check_phrase_caption_args(SET, EOS, V, 4, **kw)
    assert check_phrase_caption_args(SET, EOS, V, 4, num_beams=1).nodes == 9


def test_a_built_trie_is_taken_as_it_is_and_held_against_the_call():
    trie = phrase_trie(SET, EOS, V, 4)
    assert trie.longest == 3
    assert check_phrase_caption_args(trie, EOS, V, 4) is trie, 'the trie the model built is not built again'
    for eos, vocab, max_new in ((None, V, 4), (EOS, V, 3), (7, V, 4), (EOS, 9, 4), (V, V, 4)):
        with pytest.raises(ValueError, match='a PhraseTrie built for another call'):
            check_phrase_caption_args(trie, eos, vocab, max_new)
    with pytest.raises(NotImplementedError, match='phrases under num_beams > 1'):
        check_phrase_caption_args(trie, EOS, V, 4, num_beams=3)


def test_graph_key_and_result_field():
    assert caption_graph_key('greedy', 7, 0) == ('greedy', 7, 0)
    proc = Processors(1.3, 1 / 1.3, 2, (5,))
    for args in (('greedy', 7, 0), ('greedy_top2', 7, 0), ('greedy', 7, 0, 12), ('greedy', 7, 0, None, proc, 3)):
        key = caption_graph_key(*args)
        assert 'trie' not in key, 'a call without phrases never sees a trie key'
        assert caption_graph_key(*args, trie=True) == ('trie', 7) + key
    z = torch.zeros(1)
    out = GeneratedCaptions(z, z, z, z)
    assert out.phrase_index is None and GeneratedCaptions._fields == ('ids', 'lengths', 'token_logprobs', 'logprob')
    with_index = GeneratedCaptions(z, z, z, z, phrase_index=z + 2)
    assert with_index.phrase_index is not None and with_index.beam_scores is None and len(with_index) == 4
