"""search_phrases on the host: ``phrase_beam_search_host`` -- the normative statement of the beam over the phrase trie --
against a brute-force enumeration of the set, with and without its close rule, and every refusal of ``check_phrase_search_args``.
Logits are random fp32 rows that depend on the token sequence alone, so the replica, ``phrase_scores_host`` and the enumeration see the
same numbers."""
import zlib

import numpy as np
import pytest

from image2text_amd.caption_plan import CaptionFacts, PhraseBeams, check_phrase_search_args, plan_captions, trie_widest_level
from image2text_amd.decoding_host import phrase_beam_search_host, phrase_scores_host, trie_beam_candidates_host
from image2text_amd.phrase_trie import phrase_trie

V, EOS = 64, 5
f32 = np.float32


def logits_fn(seed):
    """fp32 logits [V] as a function of the sequence: a generator keyed by (seed, the sequence)"""
    def f(seq):
        key = zlib.crc32(np.asarray([seed] + [int(t) for t in seq], dtype=np.int64).tobytes())
        return (np.random.default_rng(key).standard_normal(V) * 2.5).astype(f32)
    return f


def random_phrases(seed, K, depth):
    """K phrases of 1 .. depth tokens over a small alphabet, so that they share prefixes, some are prefixes of others and some repeat"""
    g = np.random.default_rng(seed)
    alphabet = [t for t in range(8, 8 + int(g.integers(3, 7))) if t != EOS]
    return [[int(t) for t in g.choice(alphabet, size=int(g.integers(1, depth + 1)))] for _ in range(K)]


def brute_force(step, trie, phrases, prompt, penalty):
    """every distinct phrase's (score, logprob, length, index the trie holds), best first: ``phrase_scores_host``'s numbers, the score
    one fp32 power and one fp32 division"""
    ref = phrase_scores_host(step, trie, EOS, prompt)
    rows = []
    for k in sorted(set(int(t) for t in trie.term if t >= 0)):
        lp, n = ref.logprob[k], int(ref.lengths[k])
        rows.append((f32(lp / np.power(f32(n), f32(penalty))), lp, n, k))
    rows.sort(key=lambda r: (-r[0], r[3]))
    return rows


@pytest.mark.parametrize('penalty', [0.0, 1.0, -0.5])
@pytest.mark.parametrize('seed', range(6))
def test_exhaustive_search_is_the_brute_force_top_n(seed, penalty):
    phrases = random_phrases(seed, K=10 + 6 * seed, depth=2 + seed % 3)
    assert len(phrases) <= 40
    trie = phrase_trie(phrases, EOS, V, 1 << 30)
    step, prompt = logits_fn(seed), [3, 1 + seed]
    want = brute_force(step, trie, phrases, prompt, penalty)
    W = max(trie_widest_level(trie), 2)
    N = min(4, len(want))
    got = phrase_beam_search_host(step, prompt, trie, EOS, W, N, penalty)
    assert got.phrase_index.tolist() == [r[3] for r in want[:N]], 'the same phrases in the same order'
    assert got.lengths.tolist() == [r[2] for r in want[:N]]
    assert got.logprob.dtype == f32 and got.logprob.tobytes() == np.array([r[1] for r in want[:N]], dtype=f32).tobytes(), 'logprob: bit-equal'
    assert got.scores.tobytes() == np.array([r[0] for r in want[:N]], dtype=f32).tobytes()
    assert got.steps <= trie.longest + 1
    if penalty == 0.0:
        assert got.scores.tobytes() == got.logprob.tobytes()
    # the whole pool, too: W entries or every distinct phrase
    full = phrase_beam_search_host(step, prompt, trie, EOS, W, min(W, len(want)), penalty)
    assert full.phrase_index.tolist() == [r[3] for r in want[:min(W, len(want))]]


@pytest.mark.parametrize('penalty', [0.0, 1.0, -0.5])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_the_close_rule_changes_no_pool(W, penalty):
    done, seed = 0, 100 * W
    while done < 5:
        seed += 1
        phrases = random_phrases(seed, K=30, depth=4)
        trie = phrase_trie(phrases, EOS, V, 1 << 30)
        N = min(W, int((trie.term >= 0).sum()))
        step, prompt = logits_fn(seed), [7]
        off = phrase_beam_search_host(step, prompt, trie, EOS, W, N, penalty, close_rule=False)
        if off.gaps + off.pool_gaps and min(off.gaps + off.pool_gaps) <= 1e-4:
            continue                                            # neighbouring totals closer than 1e-4: draw the next case
        on = phrase_beam_search_host(step, prompt, trie, EOS, W, N, penalty)
        assert on.steps <= off.steps <= trie.longest + 1 and on.pool_n == off.pool_n
        for name in ('phrase_index', 'logprob', 'scores', 'lengths'):
            assert getattr(on, name).tobytes() == getattr(off, name).tobytes(), (seed, name)
        done += 1


def test_small_fan_out_a_terminal_with_children_and_duplicates():
    phrases = [[9], [9, 11], [12], [9], [9, 11, 13]]            # 0 and 3 repeat; [9] ends a phrase and runs on; the root has 2 children
    trie = phrase_trie(phrases, EOS, V, 1 << 30)
    assert trie_widest_level(trie) == 2 and int((trie.term >= 0).sum()) == 4
    step = logits_fn(77)
    z = np.stack([step([4])] * 4)
    node, path = np.array([0, -1, 0, -1], dtype=np.int32), np.array([0.0, 0.0, -1.5, 0.0], dtype=f32)
    edge, total, fin, lse = trie_beam_candidates_host(z, node, path, trie, EOS, 4)
    assert (edge[[1, 3]] == -1).all() and np.isneginf(total[[1, 3]]).all() and np.isneginf(fin).all(), 'dead rows; the root ends no phrase'
    assert (edge[0, 2:] == -1).all() and np.isneginf(total[0, 2:]).all() and (edge[0, :2] >= 0).all(), 'fewer than W children'
    assert total[0, 0] >= total[0, 1] and np.array_equal(edge[0], edge[2]) and lse[0] == lse[2]
    assert total[2, :2].tobytes() == (f32(-1.5) + total[0, :2]).astype(f32).tobytes(), 'path + (z - lse), the path added last'
    z2 = z.copy()
    z2[0, 9] = z2[0, 12] = 1.25                                 # equal logits on the two children: the lower edge first
    edge2, total2, _, _ = trie_beam_candidates_host(z2, node, path, trie, EOS, 4)
    assert total2[0, 0] == total2[0, 1] and edge2[0, 0] < edge2[0, 1]
    for penalty in (0.0, 1.0, -0.5):
        want = brute_force(step, trie, phrases, [4], penalty)
        got = phrase_beam_search_host(step, [4], trie, EOS, 4, 4, penalty)
        assert got.phrase_index.tolist() == [r[3] for r in want] and 3 not in got.phrase_index.tolist(), 'a duplicate goes by its lowest index'
        assert got.logprob.tobytes() == np.array([r[1] for r in want], dtype=f32).tobytes()
        assert sorted(got.lengths.tolist()) == [2, 2, 3, 4]


def test_every_refusal_with_its_text():
    ok = [[9], [9, 11], [12]]
    check = lambda phrases=ok, eos=EOS, **kw: check_phrase_search_args(phrases, eos, V, kw.pop('P', 2), kw.pop('window', 32), **kw)
    trie, W, N = check()
    assert (W, N) == (4, 1) and trie.longest == 2
    assert check(trie, num_beams=8, num_return_sequences=3, length_penalty=-0.5, poll_every=0)[1:] == (8, 3)
    for bad, text in (([], 'phrases is empty'), ([[3], []], 'is empty'), ([[V]], 'outside the vocabulary'), ([[3, EOS]], 'holds eos_token_id'),
                      ([[2.5]], 'token ids are integers')):
        with pytest.raises(ValueError, match=text):
            check(bad)
    with pytest.raises(ValueError, match='need eos_token_id'):
        check(eos=None)
    with pytest.raises(ValueError, match=r'eos_token_id = 64 outside the vocabulary'):
        check(eos=V)
    with pytest.raises(ValueError, match='a PhraseTrie built for another call: eos_token_id = 9, vocabulary 64'):
        check(trie, eos=9)
    with pytest.raises(ValueError, match='a PhraseTrie built for another call'):
        check_phrase_search_args(trie, EOS, 12, 2, 32)
    for bad in (0, 9, 2.5, True):
        with pytest.raises(ValueError, match=r'num_beams = .*: a whole number from 1 to 8'):
            check(num_beams=bad)
    for bad, text in ((0, 'from 1 to 3'), (4, 'from 1 to 3'), (1.5, 'from 1 to 3')):
        with pytest.raises(ValueError, match=rf'num_return_sequences = .* with num_beams = 4 and 3 distinct phrases: {text}'):
            check(num_return_sequences=bad)
    with pytest.raises(ValueError, match=r'num_return_sequences = 3 with num_beams = 2 and 3 distinct phrases: from 1 to 2'):
        check(num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match=r'with num_beams = 4 and 1 distinct phrases: from 1 to 1'):
        check([[9], [9]], num_return_sequences=2)
    for bad in (float('nan'), float('inf'), None, 'x'):
        with pytest.raises(ValueError, match='length_penalty = .*: a finite number is needed'):
            check(length_penalty=bad)
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(33\) exceed the text window \(32\)'):
        check(P=30)
    assert check(P=29)[0].longest == 2
    with pytest.raises(ValueError, match=r'poll_every = -1: it may not be negative'):
        check(poll_every=-1)
    with pytest.raises(NotImplementedError, match='a non-causal decoder has none'):
        check(causal=False)
    with pytest.raises(NotImplementedError, match='sparse nano-mini decoder blocks'):
        check(sparse=True)
    # the order: the set first, the window before poll_every, every ValueError before a NotImplementedError
    with pytest.raises(ValueError, match='phrases is empty'):
        check([], num_beams=0, causal=False)
    with pytest.raises(ValueError, match='num_beams'):
        check(num_beams=0, num_return_sequences=0, causal=False)
    with pytest.raises(ValueError, match='text window'):
        check(P=30, poll_every=-1, sparse=True)
    assert PhraseBeams._fields == ('phrase_index', 'logprob', 'scores', 'lengths', 'exhaustive')


def test_generate_captions_still_refuses_phrases_under_beams():
    facts = CaptionFacts(V, True, None, 32, 0)
    with pytest.raises(NotImplementedError, match='phrases under num_beams > 1: the beam step has no trie state per hypothesis'):
        plan_captions(facts, 2, 2, max_new_tokens=4, eos_token_id=EOS, phrases=[[9], [9, 11]], num_beams=2)
