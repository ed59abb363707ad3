"""``top_logprobs`` on the host: the numpy statement ``decoding_host.top_logprobs_host`` against a direct fp64 computation on
hand-written rows (the tie rule, the -inf rule, V == K); what ``plan_captions`` makes of the keyword -- every refusal with its text and
its place among the others, the mode, the plan's field --; the graph key, unchanged at K = 0 and distinct at K > 0 across the ragged /
proc / trie / sets forms; the result type's three attributes and the model method's signature.  No device, no library."""
import inspect
import math

import numpy as np
import pytest
import torch

from image2text_amd.caption_plan import (MAX_TOP_LOGPROBS, CaptionFacts, CaptionPlan, GeneratedCaptions, Processors, caption_graph_key,
                                         check_top_logprobs, plan_captions)
from image2text_amd.decoding_host import top_logprobs_host

V, WINDOW, EOS = 50, 20, 0
FACTS = CaptionFacts(V, True, None, WINDOW, 0)
NONCAUSAL = CaptionFacts(V, False, None, WINDOW, 0)
B, P = 3, 2
NINF = -np.inf


def plan(facts=FACTS, **kw):
    kw.setdefault('max_new_tokens', 4)
    kw.setdefault('top_k', 1)
    return plan_captions(facts, B, P, **kw)


# ------------------------------------------------------------------------------------------------------------------ the replica
def direct(row, K):
    """the definition, written out with math.* over Python floats: the order by sorted(), the sums one term at a time"""
    order = sorted(range(len(row)), key=lambda c: (-row[c], c))
    fin = [float(v) for v in row if v != NINF]
    m = max(fin)
    lse = m + math.log(sum(math.exp(v - m) for v in fin))
    ent = sum(math.exp(v - lse) * (lse - v) for v in fin)
    return order[:K], [float(row[c]) - lse if row[c] != NINF else NINF for c in order[:K]], ent


def held(rows, K):
    tok, lp, ent = top_logprobs_host(np.asarray(rows), K)
    assert tok.dtype == np.int32 and tok.shape == (len(rows), K) and lp.shape == (len(rows), K) and ent.shape == (len(rows),)
    assert lp.dtype == np.float64 and ent.dtype == np.float64
    for r, row in enumerate(rows):
        t, l, e = direct(list(row), K)
        assert tok[r].tolist() == t, (r, tok[r], t)
        for got, want in zip(lp[r], l):
            assert got == want if want == NINF else abs(got - want) <= 1e-12 * max(1.0, abs(want)), (r, lp[r], l)
        assert abs(ent[r] - e) <= 1e-12 * max(1.0, e), (r, ent[r], e)
    return tok, lp, ent


def test_equal_values_go_by_ascending_id():
    tok, lp, ent = held([[1.5] * 7], 4)
    assert tok[0].tolist() == [0, 1, 2, 3]
    assert np.allclose(lp[0], -math.log(7), rtol=0, atol=1e-15) and abs(ent[0] - math.log(7)) < 1e-15
    # ties inside the list and at its edge: 2.0 at ids 5 and 1, then the 0.25s by id
    tok, _, _ = held([[0.25, 2.0, 0.25, -1.0, 0.25, 2.0, 3.0]], 5)
    assert tok[0].tolist() == [6, 1, 5, 0, 2]


def test_fewer_finite_entries_than_k():
    K = 5                                                                       # K - 2 = 3 finite entries
    row = [NINF, 0.5, NINF, NINF, -2.0, NINF, 0.5, NINF]
    tok, lp, ent = held([row], K)
    assert tok[0].tolist() == [1, 6, 4, 0, 2], 'the -inf columns follow the finite ones, by ascending id'
    assert np.isfinite(lp[0, :3]).all() and (lp[0, 3:] == NINF).all()
    p = np.exp(lp[0, :3])
    assert abs(p.sum() - 1) < 1e-15 and abs(ent[0] + (p * lp[0, :3]).sum()) < 1e-15, 'a -inf column adds 0 to the entropy'


def test_v_equals_k_and_fp32_rows_are_read_as_given():
    rows = np.array([[0.1, -0.3, 7.0, 7.0, 2.5], [-1.0, -1.0, -1.0, -1.0, -1.0]], dtype=np.float32)
    tok, lp, ent = held(rows, 5)
    assert tok[0].tolist() == [2, 3, 4, 0, 1] and tok[1].tolist() == [0, 1, 2, 3, 4]
    assert abs(np.exp(lp[0]).sum() - 1) < 1e-15, 'with V == K the list is the whole distribution'
    assert abs(ent[0] + (np.exp(lp[0]) * lp[0]).sum()) < 1e-15
    held(rows, 1)
    with pytest.raises(AssertionError):
        top_logprobs_host(rows, 6)
    with pytest.raises(AssertionError):
        top_logprobs_host(np.full((1, 4), NINF), 2)


# ------------------------------------------------------------------------------------------------------------------ the planner
def test_the_plan_carries_k_and_stays_a_cache_plan():
    assert CaptionPlan._fields[-1] == 'top_logprobs' and CaptionPlan._field_defaults['top_logprobs'] == 0
    assert plan().top_logprobs == 0 and plan(top_logprobs=0) == plan()
    for K in (1, 5, MAX_TOP_LOGPROBS, np.int64(3)):
        p = plan(top_logprobs=K)
        assert p.mode == 'cache' and p.top_logprobs == int(K) and type(p.top_logprobs) is int
        assert p._replace(top_logprobs=0) == plan()
    # every 'cache' form: sampled with N rows, ragged, both prefill settings, processors, phrases, phrase_sets, image_index
    forms = [dict(top_k=20, num_return_sequences=2, seed=1), dict(prompt_lengths=[1, 2, 2]), dict(prompt_prefill='pass'),
             dict(repetition_penalty=1.3, eos_token_id=EOS), dict(phrases=[[1, 2], [3]], eos_token_id=EOS),
             dict(phrase_sets=[[[1, 2], [3]]], phrase_set_index=[0, 0, 0], eos_token_id=EOS, prompt_lengths=[1, 2, 2]),
             dict(image_index=[0, 0, 1], images=2)]
    for kw in forms:
        p = plan(top_logprobs=5, **kw)
        assert p.mode == 'cache' and p.top_logprobs == 5 and repr(p._replace(top_logprobs=0)) == repr(plan(**kw)), kw      # (repr: the plans hold arrays)
    assert inspect.signature(plan_captions).parameters['top_logprobs'].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(plan_captions).parameters)[-2:] == ['images', 'top_logprobs']


@pytest.mark.parametrize('K, text', [
    (1.0, 'top_logprobs = 1.0: a whole number of alternatives per step, from 0 (none) to 8'),
    ('3', "top_logprobs = '3': a whole number of alternatives per step, from 0 (none) to 8"),
    (True, 'top_logprobs = True: a whole number of alternatives per step, from 0 (none) to 8'),
    (None, 'top_logprobs = None: a whole number of alternatives per step, from 0 (none) to 8'),
    (-1, 'top_logprobs = -1: from 0 (none) to 8 alternatives per step'),
    (9, 'top_logprobs = 9: from 0 (none) to 8 alternatives per step'),
])
def test_what_k_refuses_about_itself(K, text):
    with pytest.raises(ValueError) as e:
        plan(top_logprobs=K)
    assert text in str(e.value)
    with pytest.raises(ValueError) as e2:
        check_top_logprobs(K, V)
    assert str(e2.value) == str(e.value)


def test_more_alternatives_than_tokens():
    small = CaptionFacts(6, True, None, WINDOW, 0)
    assert plan(small, top_logprobs=6).top_logprobs == 6
    with pytest.raises(ValueError) as e:
        plan(small, top_logprobs=7)
    assert str(e.value) == 'top_logprobs = 7 alternatives of a vocabulary of 6 tokens'
    with pytest.raises(ValueError) as e:                                        # the range comes before the vocabulary
        plan(small, top_logprobs=9)
    assert 'from 0 (none) to 8' in str(e.value)


def test_beams_and_a_non_causal_decoder_are_refused():
    with pytest.raises(NotImplementedError) as e:
        plan(top_k=None, num_beams=2, top_logprobs=3)
    assert str(e.value).startswith("top_logprobs under num_beams > 1: the beam step's quantity is the row AFTER the n-gram ban")
    with pytest.raises(NotImplementedError) as e:
        plan(NONCAUSAL, top_logprobs=3)
    assert str(e.value).startswith('top_logprobs runs inside the KV-cache caption step; a non-causal decoder generates by re-evaluation')
    # K = 0 is the call without the argument in both
    assert plan(top_k=None, num_beams=2, top_logprobs=0).mode == 'beam' and plan(NONCAUSAL, top_logprobs=0).mode == 'recompute'


def test_the_order_of_the_refusals():
    # image_index's ValueErrors come first, then K's own, then everything else
    with pytest.raises(ValueError, match='image_index of shape'):
        plan(top_logprobs=9, image_index=[0], images=2)
    with pytest.raises(ValueError, match='top_logprobs = 9'):
        plan(top_logprobs=9, num_beams=99)
    with pytest.raises(ValueError, match='top_logprobs = 9'):
        plan(top_logprobs=9, max_new_tokens=4, min_new_tokens=7)
    with pytest.raises(ValueError, match='top_logprobs = 9'):
        plan(NONCAUSAL, top_logprobs=9, phrases=[[1]], eos_token_id=EOS)
    # under beams: the beam arguments' own refusals, then K's, then the beam window
    with pytest.raises(ValueError, match='num_beams = 99'):
        plan(top_k=None, top_logprobs=3, num_beams=99)
    with pytest.raises(ValueError, match='deterministic beam search'):
        plan(top_k=5, top_logprobs=3, num_beams=2)
    with pytest.raises(NotImplementedError, match='prompt_lengths under num_beams > 1'):
        plan(top_k=None, top_logprobs=3, num_beams=2, prompt_lengths=[1, 2, 2])
    with pytest.raises(NotImplementedError, match='top_logprobs under num_beams > 1'):
        plan(top_k=None, top_logprobs=3, num_beams=2, max_new_tokens=WINDOW)
    # on a non-causal decoder: the caption arguments' ValueErrors and the processors' refusal, then K's, then prefill_plan's and the window
    with pytest.raises(ValueError, match='greedy decoding with num_return_sequences = 2'):
        plan(NONCAUSAL, top_logprobs=3, num_return_sequences=2)
    with pytest.raises(NotImplementedError, match='repetition_penalty / min_new_tokens / suppress_tokens run inside'):
        plan(NONCAUSAL, top_logprobs=3, repetition_penalty=1.3)
    with pytest.raises(NotImplementedError, match='top_logprobs runs inside'):
        plan(NONCAUSAL, top_logprobs=3, prompt_prefill='nonsense')
    with pytest.raises(NotImplementedError, match='top_logprobs runs inside'):
        plan(NONCAUSAL, top_logprobs=3, max_new_tokens=WINDOW)
    with pytest.raises(ValueError, match='exceed the text window'):
        plan(top_logprobs=3, max_new_tokens=WINDOW)


# ------------------------------------------------------------------------------------------------------------------ the graph key
def test_the_graph_key():
    proc = Processors(1.5, 1 / 1.5, 2, (3, 4))
    forms = [dict(), dict(ragged_max_new=6), dict(proc=proc, P=3), dict(ragged_max_new=6, proc=proc, P=3), dict(trie=True), dict(sets=True),
             dict(ragged_max_new=6, sets=True)]
    seen = set()
    for head in ('greedy', (0.7, 0, 0.6)):
        for kw in forms:
            base = caption_graph_key(head, EOS, 4, **kw)
            assert caption_graph_key(head, EOS, 4, top_logprobs=0, **kw) == base, 'K = 0 is the key without the argument'
            for K in (1, 5):
                key = caption_graph_key(head, EOS, 4, top_logprobs=K, **kw)
                assert key == tuple(base) + ('top_logprobs', K) and key[0] == base[0], 'the key keeps its first tag: the pair stands at the end'
                seen.add(key)
            seen.add(base)
    assert len(seen) == 2 * len(forms) * 3
    assert list(inspect.signature(caption_graph_key).parameters)[-1] == 'top_logprobs'
    # the keys other tests pin, once more
    assert caption_graph_key('greedy_top2', 4, 4) == ('greedy_top2', 4, 4)
    assert caption_graph_key('greedy', 4, 4, 8, proc, P=3) == ('proc', 1.5, 2, 2, 0, 'ragged', 'greedy', 4, 4, 8)
    assert caption_graph_key('greedy', EOS, 0, 6, sets=True) == ('trie_sets', EOS, 'ragged', 'greedy', EOS, 0, 6)


def test_stale_graphs_are_found_by_either_tag():
    from types import SimpleNamespace
    from image2text_amd.decoding import GreedyDecoder
    proc = Processors(1.5, 1 / 1.5, 2, (3, 4))
    keys = [None, caption_graph_key('greedy', EOS, 4), caption_graph_key('greedy', EOS, 4, top_logprobs=5),
            caption_graph_key('greedy', EOS, 4, proc=proc, P=3), caption_graph_key('greedy', EOS, 4, proc=proc, P=3, top_logprobs=5),
            caption_graph_key((0.7, 0, 0.6), EOS, 4, 6, trie=True, top_logprobs=2), caption_graph_key('greedy', None, 0, 6)]
    st = SimpleNamespace(graphs={k: i for i, k in enumerate(keys)})
    GreedyDecoder._drop_graphs(st, 'top_logprobs')
    assert list(st.graphs.values()) == [0, 1, 3, 6]
    st = SimpleNamespace(graphs={k: i for i, k in enumerate(keys)})
    GreedyDecoder._drop_graphs(st, 'proc')
    assert list(st.graphs.values()) == [0, 1, 2, 5, 6], 'a K > 0 step that points at the suppress list goes with it'
    st = SimpleNamespace(graphs={k: i for i, k in enumerate(keys)})
    GreedyDecoder._drop_graphs(st, ('trie', 'trie_sets'))
    assert list(st.graphs.values()) == [0, 1, 2, 3, 4, 6]


# ------------------------------------------------------------------------------------------------------------------ the result and the signature
def test_the_result_type():
    t = torch.zeros(2)
    out = GeneratedCaptions(t, t, t, t)
    assert out.top_tokens is None and out.top_logprobs is None and out.token_entropy is None
    assert GeneratedCaptions._fields == ('ids', 'lengths', 'token_logprobs', 'logprob') and len(out) == 4
    a, b, c = torch.ones(1), torch.ones(2), torch.ones(3)
    out = GeneratedCaptions(t, t, t, t, top_tokens=a, top_logprobs=b, token_entropy=c)
    assert out.top_tokens is a and out.top_logprobs is b and out.token_entropy is c and out.image_index is None and len(out) == 4
    names = list(inspect.signature(GeneratedCaptions.__new__).parameters)
    assert names[8] == 'image_index' and names[9:] == ['top_tokens', 'top_logprobs', 'token_entropy'], 'image_index keeps its positional slot'
    assert GeneratedCaptions(t, t, t, t, None, None, None, a).image_index is a


def test_the_signatures():
    from image2text_amd.decoding import CaptionDecoder
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    for fn in (VisionEncoderDecoder.generate_captions, CaptionDecoder.generate_captions):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ['top_logprobs', 'image_index'] and p['top_logprobs'].default == 0 and p['image_index'].default is None
    assert 'top_logprobs' not in inspect.signature(VisionEncoderDecoder.generate).parameters
    doc = VisionEncoderDecoder.generate_captions.__doc__
    assert 'top_logprobs' in doc and 'segment-maxima' in doc
