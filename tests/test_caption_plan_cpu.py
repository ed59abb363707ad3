"""``plan_captions`` (image2text_amd/caption_plan.py): which refusal wins when two apply, what W = 1 looks at, what a plan holds, that
every check is entered once, and that ``decoding`` still exports what it did.  Host only: no library is loaded, no GPU is used.  The
expected texts are those of the commit before ``plan_captions`` existed, read off the model method's call order."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from image2text_amd import caption_plan
from image2text_amd.caption_plan import CaptionFacts, CaptionPlan, Processors, Sampling, plan_captions
from image2text_amd.phrase_trie import PhraseTrie, phrase_trie

V, WINDOW, B, P = 50, 20, 2, 3
FACTS = CaptionFacts(V, True, None, WINDOW, 0)
NON_CAUSAL = FACTS._replace(causal=False)
NANO_MINI = FACTS._replace(fam=object())
PHRASES = dict(phrases=[[1, 2], [3]], eos_token_id=0)


def plan(facts=FACTS, **kw):
    kw.setdefault('max_new_tokens', 4)
    return plan_captions(facts, B, P, **kw)


# (what applies, the facts, the arguments, the exception and the text that wins)
PRECEDENCE = [
    ('phrases + beams', FACTS, dict(PHRASES, num_beams=2),
     NotImplementedError, 'phrases under num_beams > 1: the beam step has no trie state per hypothesis'),
    ('phrases + active processor', FACTS, dict(PHRASES, repetition_penalty=1.5),
     NotImplementedError, 'phrases with repetition_penalty / min_new_tokens / suppress_tokens: the phrase set says'),
    ('phrases + active processor + beams', FACTS, dict(PHRASES, suppress_tokens=[4], num_beams=2),
     NotImplementedError, 'phrases with repetition_penalty / min_new_tokens / suppress_tokens: the phrase set says'),
    ('phrases + prompt_lengths', FACTS, dict(PHRASES, prompt_lengths=[2, 3]),
     NotImplementedError, 'phrases with prompt_lengths: a forced prompt column would have to hold the trie still'),
    ('phrases + prompt_lengths + active processor', FACTS, dict(PHRASES, prompt_lengths=[2, 3], repetition_penalty=1.5),
     NotImplementedError, 'phrases with prompt_lengths: a forced prompt column would have to hold the trie still'),
    ('phrases + non-causal', NON_CAUSAL, dict(PHRASES),
     NotImplementedError, 'phrases run inside the KV-cache caption step; a non-causal decoder generates by re-evaluation'),
    ('a bad processor value + phrases', FACTS, dict(PHRASES, repetition_penalty=0),
     ValueError, 'repetition_penalty = 0: a finite value above 0 is needed (1.0: none)'),
    ('a bad processor value + a bad phrase set', FACTS, dict(phrases=[], eos_token_id=0, min_new_tokens=9),
     ValueError, 'min_new_tokens = 9 exceeds max_new_tokens = 4'),
    ('a bad phrase set + beams', FACTS, dict(phrases=[[]], eos_token_id=0, num_beams=9),
     ValueError, 'phrases[0] is empty: a phrase holds at least one token'),
    ('beams + sampling argument', FACTS, dict(num_beams=2, top_k=5),
     ValueError, 'num_beams > 1 is deterministic beam search: temperature, top_k, nucleus_p and seed must stay at their defaults'),
    ('beams + sampling argument + prompt_lengths', FACTS, dict(num_beams=2, seed=1, prompt_lengths=[2, 3]),
     ValueError, 'num_beams > 1 is deterministic beam search: temperature, top_k, nucleus_p and seed must stay at their defaults'),
    ('beams + prompt_lengths', FACTS, dict(num_beams=2, prompt_lengths=[2, 3]),
     NotImplementedError, 'prompt_lengths under num_beams > 1: the beam step has no forcing table for ragged prompts'),
    ('beams + a ragged length out of range', FACTS, dict(num_beams=2, prompt_lengths=[0, 9]),
     NotImplementedError, 'prompt_lengths under num_beams > 1: the beam step has no forcing table for ragged prompts'),
    ("beams + 'pass'", FACTS, dict(num_beams=2, prompt_prefill='pass'),
     NotImplementedError, "prompt_prefill='pass' under num_beams > 1: the beam rows are prefilled step by step"),
    ("beams + prompt_lengths + 'pass'", FACTS, dict(num_beams=2, prompt_lengths=[2, 3], prompt_prefill='pass'),
     NotImplementedError, 'prompt_lengths under num_beams > 1: the beam step has no forcing table for ragged prompts'),
    ('beams + active processor', FACTS, dict(num_beams=2, repetition_penalty=1.5),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens under num_beams > 1: the beam step has no'),
    ('beams + active processor + prompt_lengths', FACTS, dict(num_beams=2, suppress_tokens=[4], prompt_lengths=[2, 3]),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens under num_beams > 1: the beam step has no'),
    ('beams + a bad processor value + a bad N', FACTS, dict(num_beams=2, num_return_sequences=3, repetition_penalty=0),
     ValueError, 'num_return_sequences = 3 with num_beams = 2: from 1 to num_beams captions per image'),
    ('beams + non-causal', NON_CAUSAL, dict(num_beams=2),
     NotImplementedError, 'num_beams > 1 needs a causal decoder: a non-causal one has no KV cache to run the beams on'),
    ('beams + active processor + non-causal', NON_CAUSAL, dict(num_beams=2, repetition_penalty=1.5),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens under num_beams > 1: the beam step has no'),
    ('beams + prompt past the window', FACTS, dict(num_beams=2, max_new_tokens=18),
     ValueError, 'prompt + new tokens (21) exceed the text window (20)'),
    ('beams + prompt past the window + non-causal', NON_CAUSAL, dict(num_beams=2, max_new_tokens=18),
     NotImplementedError, 'num_beams > 1 needs a causal decoder: a non-causal one has no KV cache to run the beams on'),
    ('2 W > V', FACTS._replace(V=6), dict(num_beams=4),
     ValueError, 'num_beams = 4 needs 2 * num_beams candidates per row: the vocabulary holds 6 tokens'),
    ('2 W > V + prompt past the window', FACTS._replace(V=6), dict(num_beams=4, max_new_tokens=18),
     ValueError, 'prompt + new tokens (21) exceed the text window (20)'),
    ('ragged length out of range + bad N', FACTS, dict(prompt_lengths=[0, 3], num_return_sequences=0),
     ValueError, 'num_return_sequences = 0: at least one caption per image'),
    ('ragged length out of range + a bad processor value', FACTS, dict(prompt_lengths=[0, 3], repetition_penalty=0),
     ValueError, 'repetition_penalty = 0: a finite value above 0 is needed (1.0: none)'),
    ('ragged length out of range + prompt past the window', FACTS, dict(prompt_lengths=[2, 4], max_new_tokens=30),
     ValueError, 'prompt_lengths[1] = 4 exceeds the 3 columns of prompt_ids'),
    ('a bad processor value + a bad N', FACTS, dict(num_return_sequences=0, repetition_penalty=0),
     ValueError, 'num_return_sequences = 0: at least one caption per image'),
    ('active processor + non-causal', NON_CAUSAL, dict(repetition_penalty=1.5),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens run inside the KV-cache caption step; a non-causal'),
    ('active processor + non-causal + prompt past the window', NON_CAUSAL, dict(suppress_tokens=[4], max_new_tokens=18),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens run inside the KV-cache caption step; a non-causal'),
    ('active processor + non-causal + a bad prefill mode', NON_CAUSAL, dict(suppress_tokens=[4], prompt_prefill='all'),
     NotImplementedError, 'repetition_penalty / min_new_tokens / suppress_tokens run inside the KV-cache caption step; a non-causal'),
    ("'pass' on the nano-mini family", NANO_MINI, dict(prompt_prefill='pass'),
     NotImplementedError, "prompt_prefill='pass' is not available for the nano-mini decoder family: a sparse layer caches"),
    ("'pass' on the nano-mini family + prompt past the window", NANO_MINI, dict(prompt_prefill='pass', max_new_tokens=18),
     NotImplementedError, "prompt_prefill='pass' is not available for the nano-mini decoder family: a sparse layer caches"),
    ('a bad prefill mode + prompt past the window', FACTS, dict(prompt_prefill='all', max_new_tokens=18),
     ValueError, "prompt_prefill = 'all': one of ('steps', 'pass')"),
    ('window overflow with ragged pmax', FACTS, dict(prompt_lengths=[1, 2], max_new_tokens=19),
     ValueError, 'prompt + new tokens (21) exceed the text window (20)'),
    ('window overflow without prompt_lengths', FACTS, dict(max_new_tokens=18),
     ValueError, 'prompt + new tokens (21) exceed the text window (20)'),
]


@pytest.mark.parametrize('what, facts, kw, exc, text', PRECEDENCE, ids=[row[0] for row in PRECEDENCE])
def test_the_refusal_that_wins(what, facts, kw, exc, text):
    with pytest.raises(exc) as e:
        plan(facts, **kw)
    assert type(e.value) is exc and str(e.value).startswith(text), str(e.value)


def test_ragged_pmax_not_P_is_held_against_the_window():
    """P + max_new_tokens = 21 is past the window, the longest prompt + max_new_tokens = 20 is not"""
    p = plan(prompt_lengths=[1, 2], max_new_tokens=18)
    assert (p.mode, p.pmin, p.pmax) == ('cache', 1, 2)


def test_one_beam_is_the_call_without_the_beam_arguments():
    p = plan(num_beams=1, temperature=0.7, top_k=5, seed=3, num_return_sequences=2, prompt_lengths=[2, 3], prompt_prefill='pass',
             repetition_penalty=1.3, eos_token_id=7)
    assert (p.mode, p.W, p.N) == ('cache', 1, 2)
    assert p.sampling == Sampling(0.7, 5, None, 3) and p.proc is not None and p.plen is not None and p.m == 1
    assert plan(NON_CAUSAL, num_beams=1, top_k=5).mode == 'recompute'
    assert plan(num_beams=np.int64(1)).W == 1
    for kw, text in ((dict(length_penalty=float('nan')), 'length_penalty = nan: a finite number is needed'),
                     (dict(length_penalty='long'), "length_penalty = 'long': a finite number is needed"),
                     (dict(early_stopping='never'), 'early_stopping = \'never\': False or True ("never" is not supported)'),
                     (dict(num_beams=0), 'num_beams = 0: a whole number from 1 to 8'),
                     (dict(num_beams=True), 'num_beams = True: a whole number from 1 to 8'),
                     (dict(num_beams=9, num_return_sequences=0), 'num_beams = 9: a whole number from 1 to 8')):
        with pytest.raises(ValueError) as e:
            plan(**kw)
        assert str(e.value).startswith(text), str(e.value)


def test_plan_contents():
    p = plan(top_k=1)                                           # plain greedy
    assert isinstance(p, CaptionPlan) and p == CaptionPlan('cache', 1, 1, None, None, 0, 8, 4, None, 3, 3, 'steps', 0, (0, 1), None, None, 1.0, False)
    with pytest.raises(AttributeError):
        p.mode = 'beam'
    p = plan(num_return_sequences=3, temperature=0.7, top_k=5, seed=9, eos_token_id=7, poll_every=2)        # N > 1, sampled
    assert (p.mode, p.N, p.W, p.eos, p.pad, p.poll_every, p.max_new) == ('cache', 3, 1, 7, 7, 2, 4)
    assert p.sampling == Sampling(0.7, 5, None, 9) and isinstance(p.sampling, Sampling)
    assert plan(eos_token_id=7, pad_token_id=4).pad == 4 and plan(pad_token_id=4).pad == 4 and plan().sampling == Sampling(1.0, None, None, None)
    assert plan(sampling=None).sampling is None and plan(top_k=1, sampling=Sampling(0.5)).sampling == Sampling(0.5)
    prefixed = FACTS._replace(prefix=5)
    for lengths in ([2, 3], np.array([2, 3]), torch.tensor([2, 3])):                                         # ragged
        p = plan(prefixed, prompt_lengths=lengths, top_k=1)
        assert p.plen.dtype == np.int32 and p.plen.tolist() == [2, 3] and (p.pmin, p.pmax, p.m, p.start) == (2, 3, 0, (5, 1))
    p = plan(prefixed, prompt_prefill='pass', top_k=1)                                                       # 'pass': m = pmin - 1 columns
    assert (p.prompt_prefill, p.pmin, p.pmax, p.m, p.start) == ('pass', 3, 3, 2, (7, 3))
    p = plan(prefixed, prompt_prefill='pass', prompt_lengths=[2, 3])
    assert (p.pmin, p.pmax, p.m, p.start) == (2, 3, 1, (6, 2))
    assert plan(prefixed, top_k=1).start == (5, 1)
    assert plan().proc is None and plan(suppress_tokens=[]).proc is None and plan(min_new_tokens=2).proc is None     # no EOS id: no rule
    p = plan(repetition_penalty=1.5, min_new_tokens=2, suppress_tokens=[4, 4, 9], eos_token_id=7)            # processors
    assert isinstance(p.proc, Processors) and (p.proc.theta, p.proc.min_new, p.proc.suppress) == (1.5, 2, (4, 9))
    assert p.proc.inv_theta == float(np.float32(1.0) / np.float32(1.5))
    trie = phrase_trie([[1, 2], [3]], 0, V, 4)                                                               # phrases
    p = plan(phrases=trie, eos_token_id=0, top_k=1)
    assert p.trie is trie and p.mode == 'cache' and p.proc is None
    p = plan(**PHRASES)
    assert isinstance(p.trie, PhraseTrie) and p.trie.longest == 2 and p.trie.nodes == 4
    assert plan(top_k=1).trie is None
    p = plan(num_beams=3, num_return_sequences=2, eos_token_id=7, length_penalty=2, early_stopping=np.True_)  # beams
    assert p == CaptionPlan('beam', 2, 3, None, 7, 7, 8, 4, None, 3, 3, 'steps', 0, (0, 1), None, None, 2.0, True)
    assert type(p.length_penalty) is float and type(p.early_stopping) is bool and type(p.pad) is int
    assert plan(prefixed, num_beams=2).start == (5, 1) and plan(num_beams=2).pad == 0
    p = plan(NON_CAUSAL, prompt_prefill='pass', prompt_lengths=[2, 3], eos_token_id=7, top_k=1)              # non-causal: nothing to prefill
    assert (p.mode, p.m, p.start, p.pmin, p.pmax, p.pad, p.sampling) == ('recompute', 0, (0, 1), 2, 3, 7, None)


@pytest.mark.parametrize('kw', [dict(top_k=1), dict(PHRASES), dict(num_beams=2), dict(prompt_lengths=[2, 3], repetition_penalty=1.5),
                                dict(prompt_prefill='pass', suppress_tokens=[4])], ids=['plain', 'phrases', 'beams', 'ragged', 'pass'])
def test_every_check_is_entered_once(monkeypatch, kw):
    calls = {}
    for name in ('caption_processors', 'prefill_plan', 'check_beam_caption_args', 'check_caption_args', 'check_ragged_caption_args',
                 'check_phrase_caption_args'):
        def counted(*a, _fn=getattr(caption_plan, name), _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(caption_plan, name, counted)
    plan(**kw)
    assert calls['caption_processors'] == 1 and calls['check_beam_caption_args'] == 1 and calls.get('prefill_plan', 0) <= 1
    # check_ragged_caption_args is check_caption_args and the lengths: the one call of the former makes the one call of the latter
    assert calls.get('check_caption_args', 0) <= 1 and calls.get('check_ragged_caption_args', 0) <= 1 and calls.get('check_phrase_caption_args', 0) <= 1
    assert all(n == 1 for n in calls.values()), calls


PARENT_NAMES = [
    'ENC_CHUNK', 'TOP2_HEAD', 'PREFILL_ROWS', 'Sampling', 'DECODE_MAX_KEYS', 'text_window', 'LONG_CHUNK_KEYS', 'DECODE_LONG_MAX_KEYS',
    'LONG_HEAD_DIMS', 'takes_long_cache', 'decode_window', 'cache_plan', 'split_attention_host', 'PROMPT_PREFILL_MODES', 'prefill_plan',
    'kv_prefill_host', 'slot_positions', 'GreedyDecoder', 'BeamSpec', 'BeamDecoder', 'GeneratedCaptions', 'apply_finish_rule',
    'apply_finish_rule_ragged', 'Processors', 'caption_processors', 'process_logits_host', 'caption_graph_key', 'PhraseTrie', 'phrase_trie',
    'check_phrase_caption_args', 'trie_mask_host', 'trie_advance_host', 'constrained_decode_host', 'PhraseScores', 'TrieLevel',
    'TrieLevels', 'trie_levels', 'phrase_node_csr', 'level_expand_tables', 'phrase_scores_host', 'check_phrase_score_args',
    'CaptionDecoder', 'check_caption_args', 'check_ragged_caption_args', 'MAX_CAPTION_BEAMS', 'BEAM_DEAD', 'check_beam_caption_args',
    'beam_pool_select_host', 'beam_advance_host', 'banned_log_softmax_host', 'beam_search_host', 'CaptionBeamDecoder', 'TRIE_SCORE_BYTES',
    'TrieScoreDecoder', 'generate_by_recompute', 'ConcurrentGreedyDecoder',
    '_finish_rows', '_draw_seed', '_set_seed', '_capture_launches',                    # private, but tests and tools import some of them
]


def test_decoding_exports_what_it_did():
    from image2text_amd import decoding, decoding_host, phrase_trie as trie_module
    missing = [n for n in PARENT_NAMES if not hasattr(decoding, n)]
    assert not missing, missing
    for name in PARENT_NAMES:                                   # one object under both names, not a copy
        for home in (caption_plan, decoding_host, trie_module):
            if hasattr(home, name):
                assert getattr(decoding, name) is getattr(home, name), name
    for knob in ('ENC_CHUNK', 'TOP2_HEAD', 'PREFILL_ROWS', 'TRIE_SCORE_BYTES'):      # the knobs are decoding's own: the drivers read them there
        assert not any(hasattr(home, knob) for home in (caption_plan, decoding_host, trie_module)), knob
    assert decoding.LONG_CHUNK_KEYS == decoding.ops.LONG_CHUNK_KEYS == 256


def test_the_siblings_import_without_the_library_or_decoding():
    code = ('import sys\n'
            'import image2text_amd.caption_plan, image2text_amd.phrase_trie, image2text_amd.decoding_host\n'
            'bad = [m for m in ("image2text_amd.lib", "image2text_amd.ops", "image2text_amd.engine", "image2text_amd.decoding") if m in sys.modules]\n'
            'assert not bad, bad\n')
    done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=str(__import__('pathlib').Path(__file__).resolve().parents[1]))
    assert done.returncode == 0, done.stderr
