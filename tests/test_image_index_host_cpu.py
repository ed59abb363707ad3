"""``image_index`` on the host: what the three planners of caption_plan.py make of it -- the row -> image table for
N = 1, N > 1 and beams --, every refusal with its text and the ValueError-before-NotImplementedError order, ``phrase_set_index`` None
meaning S == Q, and plans without the argument that are what they were before it existed.  No device, no library."""
import numpy as np
import pytest
import torch

from image2text_amd.caption_plan import (CaptionFacts, CaptionPlan, ClosedSet, GeneratedCaptions, PhraseBeams, PhraseScores, PhraseSetScores,
                                         Sampling, check_image_index, plan_captions, plan_phrase_scores, plan_phrase_search, row_images)

V, WINDOW, EOS = 50, 20, 0
FACTS = CaptionFacts(V, True, None, WINDOW, 0)
Q, P, IMAGES = 5, 3, 2
INDEX = [1, 0, 1, 1, 0]
SETS = [[[1, 2], [3]], [[4], [5, 6, 7]]]


def captions(index=INDEX, images=IMAGES, facts=FACTS, q=Q, **kw):
    kw.setdefault('max_new_tokens', 4)
    return plan_captions(facts, q, P, image_index=index, images=images, **kw)


def scores(index=INDEX, images=IMAGES, q=Q, **kw):
    kw = dict(dict(phrases=[[1, 2], [3]], phrase_sets=None, phrase_set_index=None, prompt_lengths=None), **kw)
    return plan_phrase_scores(kw.pop('phrases'), kw.pop('phrase_sets'), kw.pop('phrase_set_index'), kw.pop('prompt_lengths'), EOS, V, q, P, WINDOW,
                              image_index=index, images=images, **kw)


def search(index=INDEX, images=IMAGES, q=Q, **kw):
    kw = dict(dict(phrases=[[1, 2], [3]], phrase_sets=None, phrase_set_index=None, prompt_lengths=None), **kw)
    return plan_phrase_search(kw.pop('phrases'), kw.pop('phrase_sets'), kw.pop('phrase_set_index'), kw.pop('prompt_lengths'), EOS, V, q, P, WINDOW,
                              image_index=index, images=images, **kw)


PLANNERS = [captions, scores, search]


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('index', [INDEX, tuple(INDEX), np.array(INDEX), np.array(INDEX, dtype=np.uint8), torch.tensor(INDEX),
                                   torch.tensor(INDEX, dtype=torch.int32)], ids=['list', 'tuple', 'int64', 'uint8', 'tensor', 'tensor32'])
def test_the_index_is_taken_in_every_integer_form(index):
    got = check_image_index(index, Q, IMAGES)
    assert got.dtype == np.int32 and got.tolist() == INDEX
    for plan in (captions(index, top_k=1), scores(index), search(index)[0]):
        assert plan.image_index.dtype == np.int32 and plan.image_index.tolist() == INDEX


def test_the_row_to_image_table():
    p = captions(top_k=1)                                                       # N = 1: a row per query
    assert (p.mode, p.N, p.rows_per_query) == ('cache', 1, 1) and p.row_images.tolist() == INDEX and p.row_images.dtype == np.int32
    p = captions(num_return_sequences=3, top_k=20, seed=1)                      # N > 1: rows (query, n)
    assert (p.mode, p.N) == ('cache', 3) and p.row_images.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    p = captions(num_beams=2, num_return_sequences=1)                           # beams: rows (query, w), whatever N
    assert (p.mode, p.N, p.W, p.rows_per_query) == ('beam', 1, 2, 2) and p.row_images.tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 0, 0]
    assert captions(None, Q, top_k=1).row_images is None and captions(None, None, top_k=1).image_index is None
    # everything that was per image is per query: Q prompt lengths, Q set indices, the result of a planner is Q long
    p = captions(top_k=1, prompt_lengths=[1, 2, 3, 2, 1], phrase_sets=SETS, phrase_set_index=[0, 1, 1, 0, 0], eos_token_id=EOS)
    assert p.plen.tolist() == [1, 2, 3, 2, 1] and p.sets.index.tolist() == [0, 1, 1, 0, 0] and p.image_index.tolist() == INDEX
    one = scores(phrases=None, phrase_sets=SETS, phrase_set_index=[0, 1, 1, 0, 0], prompt_lengths=[1, 2, 3, 2, 1])
    assert isinstance(one, ClosedSet) and one.index.tolist() == [0, 1, 1, 0, 0] and one.plen.tolist() == [1, 2, 3, 2, 1] and one.roots.shape == (Q,)
    one, W, N = search(phrases=None, phrase_sets=SETS, phrase_set_index=[0, 1, 1, 0, 0], num_beams=2)
    assert (W, N) == (2, 1) and one.longest.shape == (Q,) and one.image_index.tolist() == INDEX
    assert check_image_index([], 0, 3).shape == (0,)
    # the one derivation: what CaptionPlan.row_images gives is what the drivers upload (decoding._set_mem_index takes it as it stands;
    # search_phrases' rows come from the same function over its ClosedSet's table)
    assert row_images(None, 3) is None and row_images(one.image_index, W).tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 0, 0]
    assert row_images(one.image_index, W).dtype == np.int32 and np.array_equal(p.row_images, row_images(p.image_index, 1))


def test_no_set_index_means_a_set_per_query():
    five = [[[1]], [[2]], [[3]], [[4]], [[5, 6]]]
    for one in (captions(top_k=1, phrase_sets=five, eos_token_id=EOS).sets, scores(phrases=None, phrase_sets=five),
                search(phrases=None, phrase_sets=five, num_beams=1)[0]):
        assert one.index.tolist() == [0, 1, 2, 3, 4]
    for call in (lambda: captions(top_k=1, phrase_sets=SETS, eos_token_id=EOS), lambda: scores(phrases=None, phrase_sets=SETS),
                 lambda: search(phrases=None, phrase_sets=SETS)):
        with pytest.raises(ValueError, match='phrase_set_index = None needs one set per image: 2 sets for 5 images'):
            call()                                                              # S == the images, not the queries: refused


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('planner', PLANNERS, ids=lambda f: f.__name__)
def test_what_the_index_refuses_about_itself(planner):
    with pytest.raises(ValueError, match=r'image_index of shape \(4,\) for prompt_ids of 5 rows: one image per prompt, shape \(5,\)'):
        planner(INDEX[:4])
    with pytest.raises(ValueError, match=r'image_index of shape \(5, 1\)'):
        planner(np.array(INDEX)[:, None])
    with pytest.raises(ValueError, match=r'image_index\[3\] = 2 is outside the 2 images: \[0, 2\)'):
        planner([1, 0, 1, 2, 0])
    with pytest.raises(ValueError, match=r'image_index\[1\] = -1 is outside the 2 images'):
        planner([1, -1, 1, 1, 0])
    for bad, text in ((np.array(INDEX, dtype=np.float32), 'image_index of type float32: integers are needed'),
                      (torch.tensor(INDEX, dtype=torch.float16), 'image_index of dtype torch.float16: integers are needed'),
                      (torch.tensor(INDEX) > 0, 'image_index of dtype torch.bool: integers are needed'),
                      ([1.0, 0.0, 1.0, 1.0, 0.0], 'image_index of type float64: integers are needed')):
        with pytest.raises(ValueError, match=text):
            planner(bad)
    with pytest.raises(ValueError, match='5 prompts for 2 images: without image_index row b of prompt_ids is asked of image b'):
        planner(None)                                                           # silently mishandled before: the first 2 prompts' images only / past the end
    with pytest.raises(ValueError, match='2 prompts for 5 images'):
        planner(None, 5, q=2)
    planner(None, None)                                                         # a caller that does not know the images checks no count
    with pytest.raises(ValueError, match=r'image_index\[0\] = -3: an image index cannot be negative'):
        planner([-3, 0, 1, 1, 0], None)


def test_value_errors_come_before_not_implemented_errors():
    non_causal, nano_mini = FACTS._replace(causal=False), FACTS._replace(fam=object())
    # the index's own ValueErrors win over every NotImplementedError of the call
    for kw in (dict(prompt_prefill='pass'), dict(num_beams=2, prompt_prefill='pass'), dict(phrases=[[1]], eos_token_id=EOS, num_beams=2)):
        with pytest.raises(ValueError, match='image_index of shape'):
            captions(INDEX[:4], **kw)
    with pytest.raises(ValueError, match='image_index of shape'):
        captions(INDEX[:4], facts=non_causal, repetition_penalty=2.0)
    for planner in (scores, search):
        for kw in (dict(causal=False), dict(sparse=True)):
            with pytest.raises(ValueError, match=r'image_index\[0\] = 7 is outside'):
                planner([7, 0, 0, 0, 0], **kw)
            with pytest.raises(NotImplementedError):
                planner(**kw)
    # its NotImplementedError comes after every ValueError of the call
    with pytest.raises(NotImplementedError, match="image_index with prompt_prefill='pass': the prefill pass is one causal sequence per IMAGE"):
        captions(prompt_prefill='pass', top_k=1)
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(23\) exceed the text window \(20\)'):
        captions(prompt_prefill='pass', top_k=1, max_new_tokens=20)
    with pytest.raises(ValueError, match='prompt_prefill = \'ahead\''):
        captions(prompt_prefill='ahead', top_k=1)
    with pytest.raises(ValueError, match='min_new_tokens = 9 exceeds'):
        captions(prompt_prefill='pass', min_new_tokens=9)
    with pytest.raises(NotImplementedError, match="prompt_prefill='pass' is not available for the nano-mini decoder family"):
        captions(facts=nano_mini, prompt_prefill='pass', top_k=1)               # the mode's own refusal keeps its place and text
    with pytest.raises(NotImplementedError, match="prompt_prefill='pass' under num_beams > 1"):
        captions(num_beams=2, prompt_prefill='pass')
    assert captions(facts=non_causal, prompt_prefill='pass', top_k=1).mode == 'recompute'      # no cache: the mode is checked and ignored
    assert captions(None, Q, prompt_prefill='pass', top_k=1).m == 2             # without the index 'pass' is what it was
    assert captions(facts=nano_mini, top_k=1).image_index.tolist() == INDEX     # a nano-mini decoder takes the index: its slot tables are per layer


# ------------------------------------------------------------------------------------------------------------------ unchanged
def test_plans_without_the_index_are_what_they_were():
    plan = lambda **kw: plan_captions(FACTS, 2, P, **dict(dict(max_new_tokens=4), **kw))
    assert plan(top_k=1) == CaptionPlan('cache', 1, 1, None, None, 0, 8, 4, None, 3, 3, 'steps', 0, (0, 1), None, None, 1.0, False)
    assert plan(top_k=1) == plan(top_k=1, image_index=None, images=2) and plan(top_k=1).image_index is None
    p = plan(num_return_sequences=3, temperature=0.7, top_k=5, seed=9, eos_token_id=7, poll_every=2)
    assert p == CaptionPlan('cache', 3, 1, Sampling(0.7, 5, None, 9), 7, 7, 2, 4, None, 3, 3, 'steps', 0, (0, 1), None, None, 1.0, False, None)
    p = plan(num_beams=3, num_return_sequences=2, eos_token_id=7, length_penalty=2, early_stopping=True)
    assert p == CaptionPlan('beam', 2, 3, None, 7, 7, 8, 4, None, 3, 3, 'steps', 0, (0, 1), None, None, 2.0, True)
    p = plan_captions(FACTS._replace(prefix=5), 2, P, 4, prompt_prefill='pass', prompt_lengths=[2, 3])
    assert (p.pmin, p.pmax, p.m, p.start, p.plen.tolist(), p.image_index) == (2, 3, 1, (6, 2), [2, 3], None)
    one = plan_phrase_scores([[1, 2], [3]], None, None, None, EOS, V, 2, P, WINDOW)
    assert len(one) == len(ClosedSet._fields) and one.image_index is None and not one.per_image and one.roots.tolist() == [0, 0]
    one, W, N = plan_phrase_search(None, SETS, None, [1, 3], EOS, V, 2, P, WINDOW, num_beams=3, num_return_sequences=2)
    assert (W, N, one.image_index, one.index.tolist(), one.plen.tolist()) == (3, 2, None, [0, 1], [1, 3])


def test_the_result_types_carry_the_index_beside_the_tuple():
    t = torch.zeros(2)
    for cls, n in ((PhraseScores, 3), (PhraseSetScores, 3), (PhraseBeams, 5)):
        fields = (t,) * n
        out = cls(*fields)
        assert out.image_index is None and len(out) == n and 'image_index' not in cls._fields and tuple(out) == fields
        assert cls(*fields, image_index=t).image_index is t
    out = GeneratedCaptions(t, t, t, t)
    assert out.image_index is None and len(out) == 4 and GeneratedCaptions._fields == ('ids', 'lengths', 'token_logprobs', 'logprob')
    assert GeneratedCaptions(t, t, t, t, None, None, None, t).image_index is t and GeneratedCaptions(t, t, t, t, image_index=t).prompt_lengths is None


def test_the_model_methods_and_rerank_take_the_keyword():
    import inspect
    from image2text_amd.models.generation_utils import rerank
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    for fn in (VisionEncoderDecoder.generate_captions, VisionEncoderDecoder.search_phrases, rerank):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == 'image_index' and p['image_index'].default is None, fn.__name__
    # score_phrases' parameter list is pinned as it stands (tests/test_phrase_set_scores_host_cpu.py): the table goes through a method of
    # its own, whose other arguments are score_phrases' in score_phrases' order
    old = list(inspect.signature(VisionEncoderDecoder.score_phrases).parameters)
    new = list(inspect.signature(VisionEncoderDecoder.score_phrases_indexed).parameters)
    assert 'image_index' not in old and new == old[:3] + ['image_index'] + old[3:]
