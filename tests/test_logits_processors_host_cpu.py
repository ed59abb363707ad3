"""The host side of generate_captions' logits processors that needs no GPU: decoding.process_logits_host -- the numpy
fp32 statement of what i2t_caption_logits_process leaves of a row, which the GPU tests use as their expectation -- on a hand-written
table and against transformers' own processors; decoding.caption_processors' refusals, texts written out; and the routing rule
(inactive: the old graph key; active: a 'proc' key and the fp32-logits head)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from image2text_amd import decoding
from image2text_amd.decoding import (CaptionDecoder, Processors, Sampling, caption_graph_key, caption_processors, check_caption_args,
                                     check_ragged_caption_args, process_logits_host)

NINF = -np.inf
f32 = np.float32


def test_process_logits_host_on_a_table():
    """V = 8, theta = 2 (its fp32 reciprocal 0.5 is exact, so the table is too).  Row: token 1 seen twice (penalised ONCE), token 2 with
    a negative logit (multiplied), token 3 with logit 0 (stays 0), token 4 seen and suppressed, EOS = 6 seen in the prompt; token 7
    is in the row only at column `length` and beyond, which are not read."""
    z = np.array([1.0, 4.0, -3.0, 0.0, 5.0, 2.0, 6.0, -1.0], dtype=f32)
    ids = [1, 2, 1, 3, 4, 6, 7, 7]
    want = np.array([1.0, 2.0, -6.0, 0.0, NINF, 2.0, 3.0, -1.0], dtype=f32)
    got = process_logits_host(z, ids, 6, emitted=2, theta=2.0, suppress=[4], eos=6, min_new=2)          # emitted == min_new: EOS allowed
    assert got.dtype == f32 and np.array_equal(got, want)
    assert z[1] == 4.0, 'the input row was written'
    want[6] = NINF
    assert np.array_equal(process_logits_host(z, ids, 6, emitted=1, theta=2.0, suppress=[4], eos=6, min_new=2), want)      # one short: banned
    assert np.array_equal(process_logits_host(z, ids, 6, 1, 2.0, [4, 6], 6, 2), want)                   # the same -inf twice
    assert np.array_equal(process_logits_host(z, ids, 6, 1, 2.0, [4, 4], None, 2)[6], f32(3.0))        # no EOS id: no rule
    # theta < 1 rewards: positive up, negative towards 0
    assert np.array_equal(process_logits_host(z, ids, 3, 0, 0.5, None, None, 0), np.array([1, 8, -1.5, 0, 5, 2, 6, -1], dtype=f32))
    # nothing active: the row; length 0: nothing is seen; ids outside the vocabulary take no part
    assert np.array_equal(process_logits_host(z, ids, 6, 5, 1.0, [], 6, 0), z)
    assert np.array_equal(process_logits_host(z, ids, 0, 0, 2.0, [], None, 0), z)
    assert np.array_equal(process_logits_host(z, [-1, 8, 99], 3, 0, 2.0, [-1, 8], None, 0), z)
    # a raw -inf stays -inf under either factor; the multiply is ONE fp32 operation with fp32(1 / theta)
    zi = np.array([NINF, 3.0], dtype=f32)
    got = process_logits_host(zi, [0, 1], 2, 0, 1.3, [], None, 0)
    assert got[0] == NINF and got[1] == f32(3.0) * (f32(1.0) / f32(1.3))


def test_against_the_transformers_processors():
    """Random fp32 rows through transformers' RepetitionPenaltyLogitsProcessor -> SuppressTokensLogitsProcessor ->
    MinNewTokensLengthLogitsProcessor, whichever of them the installed version exports (a missing class is left out by name), theta in
    {1.3, 0.8}.  transformers DIVIDES a positive score by the penalty where the device multiplies by the fp32 reciprocal: the two are
    not bit-equal on every input (a correctly rounded quotient against a product with a rounded reciprocal differ by at most 1 ulp),
    so the comparison is torch.equal where it holds and otherwise assert_allclose at 1 ulp of fp32 (rtol 2^-23); -inf entries and
    everything the penalty multiplies (negative scores) must agree exactly."""
    lp = pytest.importorskip('transformers.generation.logits_process')
    names = ('RepetitionPenaltyLogitsProcessor', 'SuppressTokensLogitsProcessor', 'MinNewTokensLengthLogitsProcessor')
    have = {n: getattr(lp, n, None) for n in names}
    print('transformers processors compared:', [n for n in names if have[n] is not None], 'missing:', [n for n in names if have[n] is None])
    if all(v is None for v in have.values()):
        pytest.skip('the installed transformers exports none of the three processors')
    V, B, L, P, EOS = 97, 6, 12, 3, 5
    g = torch.Generator().manual_seed(3)
    suppress = [7, 11, 11, 40]
    n_exact = n_all = 0
    for theta in (1.3, 0.8):
        for min_new in (0, L - P, L - P + 1):
            scores = torch.randn(B, V, generator=g) * 4
            ids = torch.randint(0, V, (B, L), generator=g)
            ids[0, :2] = EOS                                # EOS seen in the prompt
            ids[1, 4] = 7                                   # a seen token that is also suppressed
            scores[2, int(ids[2, 0])] = 0.0
            want = scores.clone()
            ours_theta, ours_sup, ours_min = 1.0, [], 0
            if have[names[0]] is not None:
                want = have[names[0]](penalty=theta)(ids, want)
                ours_theta = theta
            if have[names[1]] is not None:
                want = have[names[1]](suppress, device='cpu')(ids, want)
                ours_sup = suppress
            if have[names[2]] is not None and min_new:
                want = have[names[2]](P, min_new, EOS, device='cpu')(ids, want)
                ours_min = min_new
            got = torch.stack([torch.from_numpy(process_logits_host(scores[b].numpy(), ids[b].numpy(), L, L - P, ours_theta, ours_sup, EOS, ours_min))
                               for b in range(B)])
            assert got.dtype == torch.float32 and torch.equal(torch.isinf(got), torch.isinf(want))
            n_exact += int(torch.equal(got, want))
            n_all += 1
            fin = torch.isfinite(want)
            np.testing.assert_allclose(got[fin].numpy(), want[fin].numpy(), rtol=2.0 ** -23, atol=0)
            mult = fin & (scores < 0)                       # transformers multiplies there too: the same single fp32 product
            assert torch.equal(got[mult], want[mult])
    print(f'bit-equal to transformers in {n_exact} of {n_all} batches; the rest within 1 ulp at divided entries')


def test_refusal_texts():
    ok = dict(repetition_penalty=1.3, min_new_tokens=2, suppress_tokens=[3, 5], max_new_tokens=8, eos=4, vocab=100)

    def refused(text, **change):
        with pytest.raises(ValueError, match=text):
            caption_processors(**{**ok, **change})
        kw = {k: v for k, v in {**ok, **change}.items() if k not in ('max_new_tokens', 'eos')}
        with pytest.raises(ValueError, match=text):           # check_caption_args carries them
            check_caption_args(1, None, {**ok, **change}['eos'], None, 8, {**ok, **change}['max_new_tokens'], **kw)
        with pytest.raises(ValueError, match=text):
            check_ragged_caption_args([1, 2], 2, 3, 1, None, {**ok, **change}['eos'], None, 8, {**ok, **change}['max_new_tokens'], **kw)

    refused(r'repetition_penalty = 0: a finite value above 0 is needed \(1\.0: none\)', repetition_penalty=0)
    refused(r'repetition_penalty = -1\.5: a finite value above 0 is needed', repetition_penalty=-1.5)
    refused(r'repetition_penalty = inf: a finite value above 0 is needed', repetition_penalty=float('inf'))
    refused(r'repetition_penalty = nan: a finite value above 0 is needed', repetition_penalty=float('nan'))
    refused(r'repetition_penalty = 1e-40: neither it nor its reciprocal is a positive finite fp32 number', repetition_penalty=1e-40)
    refused(r'min_new_tokens = -1: a whole number of tokens, 0 or more', min_new_tokens=-1)
    refused(r'min_new_tokens = 2\.5: a whole number of tokens, 0 or more', min_new_tokens=2.5)
    refused(r'min_new_tokens = 9 exceeds max_new_tokens = 8', min_new_tokens=9)
    refused(r'suppress_tokens holds 100: outside the vocabulary \[0, 100\)', suppress_tokens=[3, 100])
    refused(r'suppress_tokens holds -1: outside the vocabulary \[0, 100\)', suppress_tokens=[-1])
    refused(r'suppress_tokens holds 1\.5: token ids are integers', suppress_tokens=[1.5])
    refused(r'suppress_tokens covers the whole vocabulary of 4 tokens: nothing is left to emit', suppress_tokens=[0, 1, 2, 3, 3], vocab=4, eos=None)
    # allowed: EOS in the list together with min_new_tokens > 0; min_new_tokens == max_new_tokens; duplicates (dropped, order kept)
    p = caption_processors(1.3, 8, [4, 3, 4, 3], 8, 4, 100)
    assert p == Processors(1.3, float(f32(1.0) / f32(1.3)), 8, (4, 3)) and p.key() == (1.3, 8, 2)
    assert caption_processors(1.0, 0, torch.tensor([9, 9]), 8, None, 100).suppress == (9,)
    assert check_caption_args(1, None, 4, None, 8, 8) is None


def test_inactive_settings_are_none():
    """defaults, an empty list, and a min length without an EOS id to ban: no Processors -- the call is the present one"""
    assert caption_processors(1.0, 0, None, 8, 4, 100) is None
    assert caption_processors(1.0, 0, [], 8, 4, 100) is None
    assert caption_processors(1, 0, (), 8, None, None) is None
    assert caption_processors(1.0, 3, None, 8, None, 100) is None
    assert caption_processors(1.0, 3, None, 8, 4, 100) == Processors(1.0, 1.0, 3, ())
    assert caption_processors(1.0, 3, [2], 8, None, 100) == Processors(1.0, 1.0, 0, (2,))          # no EOS: the min length drops out


def test_routing_rule():
    """inactive -> the graph keys generate_captions has always used, and the head _greedy_head chose; active -> a 'proc' key around
    them and the fp32-logits head whatever the width"""
    proc = caption_processors(1.5, 2, [3, 5], 8, 4, 100)
    assert caption_graph_key('greedy_top2', 4, 4) == ('greedy_top2', 4, 4)
    assert caption_graph_key('greedy', None, 0, ragged_max_new=8) == ('ragged', 'greedy', None, 0, 8)
    assert caption_graph_key('greedy', 4, 4, None, None, P=3) == ('greedy', 4, 4)
    assert caption_graph_key('greedy', 4, 4, None, proc, P=3) == ('proc', 1.5, 2, 2, 3, 'greedy', 4, 4)
    assert caption_graph_key('greedy', 4, 4, 8, proc, P=3) == ('proc', 1.5, 2, 2, 0, 'ragged', 'greedy', 4, 4, 8)
    key = Sampling(0.7, None, 0.6).key()
    assert caption_graph_key(key, 4, 4, None, proc, P=1)[:5] == ('proc', 1.5, 2, 2, 1) and caption_graph_key(key, 4, 4, None, proc, P=1)[5:] == (key, 4, 4)
    # the head: d % 128 == 0 takes the segment-maxima head when inactive, the logits head when a processor is active
    for d, inactive in ((128, 'greedy_top2'), (64, 'greedy')):
        me = SimpleNamespace(eng=SimpleNamespace(dec=SimpleNamespace(d=d, V=100)))
        st = SimpleNamespace(top2=object(), seg_se=object())
        assert CaptionDecoder._greedy_head(me, st, None, logits=False, lse=True) == (inactive == 'greedy_top2', inactive) or not decoding.TOP2_HEAD
        assert CaptionDecoder._greedy_head(me, st, None, logits=True, lse=True) == (False, 'greedy')
        assert CaptionDecoder._greedy_head(me, st, Sampling(0.7, None, 0.6), logits=True, lse=True) == (False, key)


def test_model_refuses_before_touching_the_device():
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import reference_unit_test_config, tiny_config
    m = VisionEncoderDecoder(tiny_config())
    images, prompt = torch.zeros(2, 3, 32, 32), torch.zeros(2, 1, dtype=torch.long)
    kw = dict(max_new_tokens=4, top_k=1)
    with pytest.raises(ValueError, match='repetition_penalty = 0'):
        m.generate_captions(images, prompt, repetition_penalty=0, **kw)
    with pytest.raises(ValueError, match='min_new_tokens = 5 exceeds max_new_tokens = 4'):
        m.generate_captions(images, prompt, min_new_tokens=5, eos_token_id=3, **kw)
    with pytest.raises(ValueError, match=r'suppress_tokens holds 384: outside the vocabulary \[0, 384\)'):
        m.generate_captions(images, prompt, suppress_tokens=[384], prompt_lengths=[1, 1], **kw)
    with pytest.raises(ValueError, match='covers the whole vocabulary of 384 tokens'):
        m.generate_captions(images, prompt, suppress_tokens=range(384), **kw)
    nc = VisionEncoderDecoder(reference_unit_test_config())
    images = torch.zeros(2, 3, 128, 128)
    for active in (dict(repetition_penalty=1.2), dict(suppress_tokens=[1]), dict(min_new_tokens=2, eos_token_id=3)):
        with pytest.raises(NotImplementedError, match='non-causal decoder generates by re-evaluation'):
            nc.generate_captions(images, prompt, **kw, **active)
