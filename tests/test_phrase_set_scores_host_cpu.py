"""Host side of score_phrases(phrase_sets=..., prompt_lengths=...), no GPU: the sets' level tables laid end to end and
the per-step state of every image (forced / at a level / finished) with its history table, on hand-written forests against a
brute-force ancestor walk; ``phrase_set_scores_host`` -- the normative replica -- bit-equal to ``phrase_scores_host`` for one set and
equal lengths, and on ragged sets against a direct per-phrase sum in fp64 (1e-6, the bound of tests/test_phrase_scores_host_cpu.py);
the -inf padding, ``best`` on ties, ``lengths``; every new refusal with its text; the replica over the CPU oracle's forward against
the oracle's own per-caption log-likelihood on the tiny model."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import (PhraseSetScores, check_phrase_set_score_args, phrase_scores_host, phrase_set_scores_host, phrase_trie,
                                     set_level_tables, set_step_state)
from test_phrase_scores_host_cpu import depth_of, parents_by_scan, table_logits, walk

V, EOS = 12, 11
# A: depth 3, widest level 3; a prefix phrase ([3 5] of [3 5 7]), a duplicate ([3 5] twice), a one-token phrase ([9])
A = [[3, 5], [3, 5, 7], [3, 2], [9], [3, 5], [1, 4, 4]]
# B: depth 1, widest level 4: wider and shallower than A
B_SET = [[4], [2], [7], [8]]
# C: one phrase of one token
C = [[6]]
SETS = (A, B_SET, C)
PROMPTS = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 1, 2, 3], [4, 5, 6, 7], [8, 9, 1, 2]]
PLEN = [1, 3, 4, 3, 1]                            # lengths {1, 3, 4} in one batch
INDEX = [0, 1, 0, 2, 1]


def tries_of(sets, vocab=V, eos=EOS):
    return [phrase_trie(s, eos, vocab, 8) for s in sets]


def test_combined_tables_hold_every_sets_levels():
    tries = tries_of(SETS)
    tabs = set_level_tables(tries)
    assert tabs.wmax == 4 and tabs.kmax == 6 and tabs.level_at.tolist() == [0, 4, 6, 8]
    assert all(a.dtype == np.int32 for a in tabs[:11]) and tabs.lengths.dtype == np.int32
    assert tabs.lengths.tolist() == [[3, 4, 3, 2, 3, 4], [2, 2, 2, 2, 0, 0], [2, 0, 0, 0, 0, 0]]
    seen = {s: [] for s in range(3)}
    for s, trie in enumerate(tries):
        up = parents_by_scan(trie)
        lv = tabs.levels[s]
        for t in range(trie.longest + 1):
            g = int(tabs.level_at[s]) + t
            ca, nc, ta, nt, oa = (int(a[g]) for a in (tabs.child_at, tabs.n_child, tabs.term_at, tabs.n_term, tabs.off_at))
            here = lv.levels[t].nodes.tolist()
            nxt = lv.levels[t + 1].nodes.tolist() if t < trie.longest else []
            assert nc == len(nxt)
            for j, nd in enumerate(nxt):                         # the child in row j: its parent's row and its token, by a scan of the CSR
                assert here[int(tabs.child_parent[ca + j])] == up[nd][0] and int(tabs.child_tok[ca + j]) == up[nd][1]
            for j in range(nt):
                nd = here[int(tabs.term_row[ta + j])]
                mine = tabs.term_phrase[tabs.term_off[oa + j]:tabs.term_off[oa + j + 1]].tolist()
                assert mine and all(walk(trie, SETS[s][k]) == nd for k in mine) and depth_of(nd, up) == t
                seen[s] += mine
    assert all(sorted(seen[s]) == list(range(len(SETS[s]))) for s in range(3)), 'every phrase of every set ends in exactly one segment'


def test_step_states_and_histories_against_an_ancestor_walk():
    tries = tries_of(SETS)
    tabs = set_level_tables(tries)
    W, prefix, clen = tabs.wmax, 2, 16
    last = max(PLEN[b] + tries[INDEX[b]].longest for b in range(5))
    assert last == 7, 'image 2: a prompt of 4 and the set of depth 3'
    kinds = []
    for col in range(min(PLEN), last + 1):
        st = set_step_state(tabs, INDEX, PLEN, PROMPTS, col)
        assert st.shape == (5, 8) and st.dtype == np.int32 and (st[:, 7] == col).all()
        row = []
        for b in range(5):
            s, trie, t = INDEX[b], tries[INDEX[b]], col - PLEN[b]
            if t < 0:
                assert st[b, 0] == -1 and st[b, 1] == PROMPTS[b][col], 'forced: the prompt token of this column'
                row.append('F')
            elif t > trie.longest:
                assert st[b, 0] == -1 and st[b, 1] == -1, 'finished'
                row.append('.')
            else:
                g = int(tabs.level_at[s]) + t
                assert st[b, :7].tolist() == [t, -1, tabs.child_at[g], tabs.n_child[g], tabs.term_at[g], tabs.n_term[g], tabs.off_at[g]]
                row.append(str(t))
                # the history table of the image's rows: its own level, its own first slot
                up = parents_by_scan(trie)
                lv = tabs.levels[s]
                first = prefix + PLEN[b] - 1
                hist = lv.history(t, first, clen)
                row_of = {int(nd): (d, w) for d, l in enumerate(lv.levels) for w, nd in enumerate(l.nodes.tolist())}
                for w, nd in enumerate(lv.levels[t].nodes.tolist()):
                    want, at = np.full(clen, w), nd
                    for j in range(t, -1, -1):
                        if 0 < j < t:
                            want[first + j] = row_of[at][1]
                        at = up[at][0] if j else at
                    assert hist[w].tolist() == want.tolist(), (col, b, w)
                assert first + t == prefix + col - 1, 'the slot this step writes is the same for every image'
        kinds.append(''.join(row))
    assert kinds == ['0FFF0', '1FFF1', '20F0.', '3101.', '..1..', '..2..', '..3..'], kinds


def test_one_set_and_equal_lengths_is_phrase_scores_host_bit_for_bit():
    f = table_logits(3, V, 2.0)
    trie = phrase_trie(A, EOS, V, 8)
    prompts = [[1, 2], [4, 7], [2, 2]]
    got = phrase_set_scores_host(lambda b, seq: f(seq), [A], [0, 0, 0], EOS, prompts)
    assert got.logprob.dtype == np.float32 and got.logprob.shape == (3, len(A)) and got.lengths.shape == (1, len(A))
    for b, p in enumerate(prompts):
        one = phrase_scores_host(f, trie, EOS, prompt=p)
        assert np.array_equal(got.logprob[b].view(np.int32), one.logprob.view(np.int32)), b
        assert int(got.best[b]) == one.best and got.lengths[0].tolist() == one.lengths.tolist()
    assert got.steps == trie.longest + 1


@pytest.mark.parametrize('seed', range(8))
def test_ragged_sets_against_a_direct_sum(seed):
    """to 1e-6 absolute: at most three tokens per phrase (four terms with the EOS) over 12 tokens with logits in [-0.5, 0.5]: a term is
    about -2.5, a sum stays below 11 in magnitude -- fp32 carries it to a few 1e-7 (the bound of test_phrase_scores_host_cpu)"""
    f = table_logits(seed, V, 0.5)
    fb = lambda b, seq: f([100 + b] + list(seq))                 # every image its own function
    got = phrase_set_scores_host(fb, SETS, INDEX, EOS, PROMPTS, PLEN)
    assert got.logprob.shape == (5, 6) and got.steps == 7
    for b in range(5):
        phrases = SETS[INDEX[b]]
        want = []
        for ph in phrases:
            total, seq = 0.0, PROMPTS[b][:PLEN[b]]
            for t in ph + [EOS]:
                z = fb(b, seq).astype(np.float64)
                total += z[t] - np.log(np.exp(z).sum())
                seq = seq + [t]
            want.append(total)
        err = np.abs(got.logprob[b, :len(phrases)].astype(np.float64) - np.array(want))
        assert err.max() <= 1e-6, (b, err)
        assert np.isneginf(got.logprob[b, len(phrases):]).all(), 'the padding is -inf'
        assert int(got.best[b]) == int(np.argmax(want)) or np.sort(want)[-1] - np.sort(want)[-2] < 2e-6 or phrases[int(got.best[b])] == phrases[int(np.argmax(want))]
        assert int(got.best[b]) < len(phrases)
    assert got.logprob[0, 0] == got.logprob[0, 4] and got.logprob[2, 0] == got.logprob[2, 4], 'duplicate phrases tie exactly'
    assert got.lengths.tolist() == [[3, 4, 3, 2, 3, 4], [2, 2, 2, 2, 0, 0], [2, 0, 0, 0, 0, 0]]


def test_best_takes_the_lowest_index_on_ties():
    flat = lambda b, seq: np.zeros(V, dtype=np.float32)          # every token equally likely: phrases of one length tie exactly
    got = phrase_set_scores_host(flat, [[[3], [4], [3]], [[1, 2], [5]]], [0, 1], EOS, [[0], [0]])
    assert got.best.tolist() == [0, 1] and got.best.dtype == np.int64
    assert got.logprob[0, 0] == got.logprob[0, 1] == got.logprob[0, 2] and got.logprob[1, 1] > got.logprob[1, 0]
    assert np.isneginf(got.logprob[1, 2]) and got.lengths.tolist() == [[2, 2, 2], [3, 2, 0]]


def test_refusals():
    ok = dict(eos=EOS, vocab=V, B=3, P=4, window=16)
    sets, idx = [A, B_SET], [0, 1, 0]
    check = lambda phrases=None, phrase_sets=None, phrase_set_index=None, prompt_lengths=None, **kw: check_phrase_set_score_args(
        phrases, phrase_sets, phrase_set_index, prompt_lengths, **{**ok, **kw})
    with pytest.raises(ValueError, match='phrases and phrase_sets are both given'):
        check(A, sets, idx)
    with pytest.raises(ValueError, match='phrase_set_index without phrase_sets'):
        check(None, None, idx)
    with pytest.raises(ValueError, match=r'score_phrases\(prompt_lengths=\.\.\.\) needs phrase_sets.*phrase_sets=\[phrases\], phrase_set_index=\[0\] \* B'):
        check(A, None, None, [1, 2, 3])
    with pytest.raises(ValueError, match=r'phrase_sets\[1\]: phrases\[0\] is empty'):
        check(None, [A, [[]]], idx)
    with pytest.raises(ValueError, match=r'phrase_set_index\[1\] = 2 is outside the 2 sets'):
        check(None, sets, [0, 2, 0])
    with pytest.raises(ValueError, match='phrase_set_index = None needs one set per image'):
        check(None, sets, None)
    with pytest.raises(ValueError, match=r'prompt_lengths\[2\] = 5 exceeds the 4 columns'):
        check(None, sets, idx, [1, 2, 5])
    with pytest.raises(ValueError, match=r'prompt_lengths\[0\] = 0'):
        check(None, sets, idx, [0, 2, 3])
    with pytest.raises(ValueError, match='integers are needed'):
        check(None, sets, idx, torch.tensor([1.0, 2.0, 3.0]))
    # the window is held against max_b (p_b + longest phrase of b's set + 1): image 2, 4 + 3 + 1
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(8\) exceed the text window \(7\)'):
        check(None, sets, idx, [1, 4, 4], window=7)
    check(None, sets, idx, [1, 4, 4], window=8)
    check(None, sets, idx, [3, 4, 3], window=7)                  # the long prompt on the shallow set: 4 + 1 + 1 and 3 + 3 + 1
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(8\) exceed the text window \(7\)'):
        check(None, sets, idx, None, window=7)
    for n in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='images_per_pass = '):
            check(None, sets, idx, images_per_pass=n)
    with pytest.raises(NotImplementedError, match='a non-causal decoder has none'):
        check(None, sets, idx, causal=False)
    with pytest.raises(NotImplementedError, match=r'sparse nano-mini decoder blocks.*slot_pos'):
        check(None, sets, idx, sparse=True)
    tries, index, plen = check(None, sets, torch.tensor(idx), torch.tensor([1, 2, 4]), images_per_pass=2)
    assert len(tries) == 2 and tries[0].phrase_node.tolist() == [walk(tries[0], p) for p in A]
    assert index.dtype == np.int32 and index.tolist() == idx and plen.dtype == np.int32 and plen.tolist() == [1, 2, 4]
    assert check(None, sets, idx)[2] is None
    assert PhraseSetScores._fields == ('logprob', 'best', 'lengths')


def test_the_model_call_takes_the_new_keywords():
    import inspect
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    names = list(inspect.signature(VisionEncoderDecoder.score_phrases).parameters)
    assert names == ['self', 'images', 'prompt_ids', 'phrases', 'eos_token_id', 'images_per_pass', 'phrase_sets', 'phrase_set_index', 'prompt_lengths']


def test_replica_over_the_oracle_forward_equals_the_oracle_score(tiny_weights):
    """``phrase_set_scores_host`` fed the CPU oracle's forward against the oracle's log-likelihood of the whole caption own prompt +
    phrase + EOS from ONE forward, to 1e-4 per scored token (tests/test_phrase_scores_host_cpu.py states why)."""
    from image2text_amd.synth import synthetic_batch, tiny_config
    from oracle import reference_model as orc
    cfg = tiny_config()
    vocab = cfg.decoder_config.vocab_size
    sd = dict(tiny_weights)
    sd.setdefault('decoder.lm_head.weight', sd['decoder.transformer.wte.weight'])
    images, labels = synthetic_batch(3, 32, 12, min(vocab, 384), seed=0)
    prompt = labels[:, :3].clamp(min=0)
    eos = 5
    sets = [[[17, 42], [17, 42, 8], [17, 9], [63], [17, 9]], [[88], [31, 7]]]
    index, plen = [0, 1, 0], [1, 3, 2]
    with torch.no_grad():
        encs = [orc.encode(sd, cfg, images[b:b + 1]) for b in range(3)]
        f = lambda b, seq: orc.forward(sd, cfg, None, torch.tensor([seq]), encoder_output=encs[b])[1][0, -1].float().numpy()
        got = phrase_set_scores_host(f, sets, index, eos, prompt.tolist(), plen)
        for b in range(3):
            p = plen[b]
            for k, ph in enumerate(sets[index[b]]):
                ids = torch.tensor([prompt[b, :p].tolist() + ph + [eos]])
                lp = torch.log_softmax(orc.forward(sd, cfg, None, ids, encoder_output=encs[b])[1][0].double(), dim=-1)
                want = float(sum(lp[i - 1, ids[0, i]] for i in range(p, ids.shape[1])))
                assert abs(float(got.logprob[b, k]) - want) <= 1e-4 * (len(ph) + 1), (b, k, float(got.logprob[b, k]), want)
            assert np.isneginf(got.logprob[b, len(sets[index[b]]):]).all()
    assert got.logprob[0, 2] == got.logprob[0, 4]
