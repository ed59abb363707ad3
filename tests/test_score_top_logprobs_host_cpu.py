"""``score(..., top_logprobs=K)`` on the host: the numpy statement ``decoding_host.score_top_logprobs_host`` against
hand-worked rows -- ties, a constant row, fewer than K finite columns, a label on a -inf column, ignored and out-of-range labels, a
scale --; the result record, which stays a three-field tuple; the model method's signature; the refusals' texts through the pure
checker the method calls and through a model on the CPU that is never run.  No device, no library."""
import inspect
import math

import numpy as np
import pytest
import torch

from image2text_amd.caption_plan import check_score_top_logprobs, check_top_logprobs
from image2text_amd.decoding_host import score_top_logprobs_host, top_logprobs_host
from image2text_amd.object_models import CaptionScores

NINF = -np.inf
IGNORE = -100


def one(row, label, K, **kw):
    """the replica on one row -> its six results, the row axis dropped; dtypes and shapes checked on the way"""
    out = score_top_logprobs_host(np.asarray([row], dtype=np.float32), [label], K, **kw)
    tok, lp, ent, rank, lse, lab = out
    assert tok.dtype == np.int32 and rank.dtype == np.int32 and all(a.dtype == np.float64 for a in (lp, ent, lse, lab))
    assert tok.shape == lp.shape == (1, K) and ent.shape == rank.shape == lse.shape == lab.shape == (1,)
    return tok[0].tolist(), lp[0], float(ent[0]), int(rank[0]), float(lse[0]), float(lab[0])


# ------------------------------------------------------------------------------------------------------------------ the replica
def test_ties_go_by_ascending_id_and_so_does_the_rank():
    row = [0.25, 2.0, 0.25, -1.0, 0.25, 2.0, 3.0]
    order = [6, 1, 5, 0, 2, 4, 3]                                      # 3.0; the 2.0s by id; the 0.25s by id; -1.0
    lse = math.log(sum(math.exp(v) for v in row))
    for label in range(7):
        tok, lp, ent, rank, got_lse, lab = one(row, label, 5)
        assert tok == order[:5] and rank == order.index(label), (label, tok, rank)
        assert abs(got_lse - lse) < 1e-12 and abs(lab - (row[label] - lse)) < 1e-12
        if rank < 5:
            assert tok[rank] == label and lp[rank] == lab, 'inside the list the label stands at its rank, with the list\'s value'
    # the two 2.0s: the one of lower id is ahead of the other, not the other way round
    assert one(row, 1, 1)[3] == 1 and one(row, 5, 1)[3] == 2


def test_a_constant_row():
    V, K = 11, 4
    for label in (0, 3, 10):
        tok, lp, ent, rank, lse, lab = one([1.75] * V, label, K)
        assert tok == [0, 1, 2, 3] and rank == label, 'equal everywhere: ids ascending, the label behind the ids below it'
        assert abs(ent - math.log(V)) < 1e-12 and np.allclose(lp, -math.log(V), rtol=0, atol=1e-12)
        assert abs(lse - (1.75 + math.log(V))) < 1e-12 and abs(lab + math.log(V)) < 1e-12


def test_fewer_finite_columns_than_k():
    row = [NINF, 0.5, NINF, NINF, -2.0, NINF, 0.5, NINF]
    tok, lp, ent, rank, lse, lab = one(row, 4, 5)
    assert tok == [1, 6, 4, 0, 2] and rank == 2
    assert np.isfinite(lp[:3]).all() and (lp[3:] == NINF).all(), '-inf log-probs at the tail'
    p = np.exp(lp[:3])
    assert abs(p.sum() - 1) < 1e-12 and abs(ent + (p * lp[:3]).sum()) < 1e-12, 'a -inf column adds 0 to the entropy'
    assert lp[2] == lab


def test_a_label_on_a_minus_inf_column():
    row = [NINF, 0.5, NINF, NINF, -2.0, NINF, 0.5, NINF]              # three finite columns
    for label, below in ((0, 0), (2, 1), (3, 2), (5, 3), (7, 4)):      # below: the -inf ids under the label
        tok, lp, ent, rank, lse, lab = one(row, label, 8)
        assert lab == NINF and rank == 3 + below, (label, rank)
        assert tok[rank] == label and lp[rank] == NINF


def test_ignored_and_out_of_range_labels():
    row = [0.1, -0.3, 7.0, 7.0, 2.5]
    want = one(row, 2, 3)
    for label in (IGNORE, 5, 8, -1, -7):
        tok, lp, ent, rank, lse, lab = one(row, label, 3)
        assert rank == -1 and lab == 0.0, label
        assert tok == want[0] and np.array_equal(lp, want[1]) and ent == want[2] and lse == want[4], 'the alternatives do not depend on a label'
    tok, lp, ent, rank, lse, lab = one(row, 3, 3, ignore_index=3)      # another ignore_index: that id is then no label
    assert rank == -1 and lab == 0.0
    assert one(row, IGNORE + 105, 3, ignore_index=7)[3] == -1 and one(row, 4, 3, ignore_index=7)[3] == 2


def test_a_scale_is_the_result_on_the_scaled_row():
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((4, 37)) * 3).astype(np.float32)
    z[1, ::5] = NINF
    labels = [5, 6, IGNORE, 36]
    got = score_top_logprobs_host(z, labels, 6, scale=0.5)
    want = score_top_logprobs_host(z * np.float32(0.5), labels, 6)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # a scale that rounds: the row is formed in fp32, one rounding per column, and read in fp64 from there
    s = np.float32(1 / 0.7)
    got = score_top_logprobs_host(z, labels, 6, scale=1 / 0.7)
    v = z * s
    assert v.dtype == np.float32
    tok, lp, ent = top_logprobs_host(v, 6)
    assert np.array_equal(got[0], tok) and np.array_equal(got[1], lp) and np.array_equal(got[2], ent)
    assert not np.array_equal(v.astype(np.float64), z.astype(np.float64) * (1 / 0.7)), '(the fp32 product does round here)'
    lse = np.array([np.log(np.exp(r[np.isfinite(r)].astype(np.float64)).sum()) for r in v])
    assert np.allclose(got[4], lse, rtol=0, atol=1e-12)
    assert got[5][0] == float(v[0, 5]) - got[4][0] and got[5][2] == 0.0
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(AssertionError):
            score_top_logprobs_host(z, labels, 6, scale=bad)


def test_the_rank_agrees_with_the_full_order():
    rng = np.random.default_rng(4)
    z = (rng.integers(-4, 5, size=(8, 29)) * 0.25).astype(np.float32)  # a lattice: many ties
    z[rng.random(z.shape) < 0.2] = NINF
    z[:, 0] = 0.0                                                      # (a finite column in every row)
    labels = rng.integers(0, 29, size=8)
    tok, lp, ent, rank, lse, lab = score_top_logprobs_host(z, labels, 8)
    for r in range(8):
        order = sorted(range(29), key=lambda c: (-z[r, c], c))
        assert tok[r].tolist() == order[:8] and rank[r] == order.index(labels[r])


# ------------------------------------------------------------------------------------------------------------------ the record
def test_the_result_record():
    a, b, c = torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(2)
    r = CaptionScores(a, b, c)
    assert CaptionScores._fields == ('token_logprobs', 'lse', 'logprob') and len(r) == 3
    x, y, z = r
    assert x is a and y is b and z is c and r.lse is r[1]
    assert r.top_tokens is None and r.top_logprobs is None and r.token_entropy is None and r.label_rank is None
    kw = CaptionScores(token_logprobs=a, lse=b, logprob=c)
    assert kw.token_logprobs is a and kw.logprob is c and kw.label_rank is None
    t, l, e, k = torch.ones(1), torch.ones(2), torch.ones(3), torch.ones(4)
    full = CaptionScores(a, b, c, top_tokens=t, top_logprobs=l, token_entropy=e, label_rank=k)
    assert full.top_tokens is t and full.top_logprobs is l and full.token_entropy is e and full.label_rank is k
    assert len(full) == 3 and tuple(full) == (a, b, c)
    # _replace and _make build the three fields only, as GeneratedCaptions' do
    rep = full._replace(lse=a)
    assert isinstance(rep, CaptionScores) and rep.lse is a and rep.token_logprobs is a and rep.top_tokens is None and len(rep) == 3
    made = CaptionScores._make([a, b, c])
    assert isinstance(made, CaptionScores) and made.logprob is c and made.label_rank is None
    assert full._asdict() == {'token_logprobs': a, 'lse': b, 'logprob': c}
    names = list(inspect.signature(CaptionScores.__new__).parameters)
    assert names[1:] == ['token_logprobs', 'lse', 'logprob', 'top_tokens', 'top_logprobs', 'token_entropy', 'label_rank']


# ------------------------------------------------------------------------------------------------------------------ the signature
def test_the_signatures():
    from image2text_amd.engine import HotPath
    from image2text_amd.models.generation_utils import rerank
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    p = inspect.signature(VisionEncoderDecoder.score).parameters
    assert list(p)[-1] == 'top_logprobs' and p['top_logprobs'].kind is inspect.Parameter.KEYWORD_ONLY and p['top_logprobs'].default == 0
    assert list(p)[:-1] == ['self', 'images', 'ids', 'labels', 'temperature', 'encoder_output', 'ignore_index'], 'the positional part is as it was'
    assert 'top_logprobs' not in inspect.signature(rerank).parameters
    doc = VisionEncoderDecoder.score.__doc__
    assert 'top_logprobs' in doc and 'label_rank' in doc and 'not bit-equal' in doc
    e = inspect.signature(HotPath.token_top_logprobs).parameters
    assert list(e) == ['self', 'hb', 'labels', 'M', 'K', 'inv_temp', 'ignore_index', 'each'] and e['each'].default is None
    assert list(inspect.signature(HotPath.token_logprobs).parameters) == ['self', 'hb', 'labels', 'M', 'inv_temp', 'ignore_index']


# ------------------------------------------------------------------------------------------------------------------ the refusals
V = 50


@pytest.mark.parametrize('K, text', [
    (1.0, 'top_logprobs = 1.0: a whole number of alternatives per step, from 0 (none) to 8'),
    (True, 'top_logprobs = True: a whole number of alternatives per step, from 0 (none) to 8'),
    (None, 'top_logprobs = None: a whole number of alternatives per step, from 0 (none) to 8'),
    (-1, 'top_logprobs = -1: from 0 (none) to 8 alternatives per step'),
    (9, 'top_logprobs = 9: from 0 (none) to 8 alternatives per step'),
    (51, 'top_logprobs = 51: from 0 (none) to 8 alternatives per step'),
])
def test_what_k_refuses_about_itself(K, text):
    with pytest.raises(ValueError) as e:
        check_score_top_logprobs(K, 1.0, V)
    assert text in str(e.value)
    with pytest.raises(ValueError) as e2:                              # generate_captions' rule, word for word
        check_top_logprobs(K, V)
    assert str(e2.value) == str(e.value)
    with pytest.raises(ValueError) as e3:                              # K's own refusals come before the temperature's
        check_score_top_logprobs(K, 0.0, V)
    assert str(e3.value) == str(e.value)


def test_more_alternatives_than_tokens():
    assert check_score_top_logprobs(6, 1.0, 6) == 6
    with pytest.raises(ValueError) as e:
        check_score_top_logprobs(7, 1.0, 6)
    assert str(e.value) == 'top_logprobs = 7 alternatives of a vocabulary of 6 tokens'


@pytest.mark.parametrize('t', [0.0, -0.7, float('inf'), float('-inf'), float('nan'), 1e-60, 1e60, 'warm', None])
def test_a_temperature_that_is_not_finite_and_positive(t):
    with pytest.raises(ValueError) as e:
        check_score_top_logprobs(3, t, V)
    assert str(e.value).startswith(f'temperature = {t!r} with top_logprobs = 3: a finite positive number')
    assert check_score_top_logprobs(0, t, V) == 0, 'the call without the argument takes what it took'


def test_what_is_accepted():
    for K in (0, 1, 8, np.int64(5)):
        for t in (1.0, 0.7, 3, np.float32(0.25), 1e-30, 1e30):
            got = check_score_top_logprobs(K, t, V)
            assert got == int(K) and type(got) is int


def test_the_model_refuses_before_any_device_work():
    """a model on the CPU, never run: the ops have no CPU path, so a call that got past the checker would raise something else"""
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import tiny_config
    m = VisionEncoderDecoder(tiny_config(dec_d=64, dec_heads=1)).eval()
    vocab = m._engine.dec.V
    images, ids = torch.zeros(2, 3, 32, 32), torch.zeros(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match='top_logprobs = 9: from 0'):
        m.score(images, ids, top_logprobs=9)
    with pytest.raises(ValueError, match='top_logprobs = 2.0: a whole number'):
        m.score(images, ids, top_logprobs=2.0)
    with pytest.raises(ValueError, match=r'temperature = 0.0 with top_logprobs = 2'):
        m.score(images, ids, temperature=0.0, top_logprobs=2)
    with pytest.raises(ValueError, match=r"temperature = nan with top_logprobs = 2"):
        m.score(images, ids, temperature=float('nan'), top_logprobs=2)
    assert vocab > 8
    with pytest.raises(TypeError):
        m.score(images, ids, None, 1.0, None, -100, 2)                 # keyword-only
