"""generate_captions(num_beams=W) on the host: the numpy replicas of the selection step and of the whole search, and the
refusals.  ``beam_search_host`` is held to transformers' own ``generate(num_beams=W, do_sample=False)`` on a tiny random GPT-2: equal
sequences, ``sequences_scores`` within 1e-5 (fp32 sums of at most 12 terms).  torch's tie order is unspecified, so every case must
keep a gap above 1e-4 between neighbouring totals of the top 2 W and to the next one, at every step; the seeds are chosen so."""
import itertools

import numpy as np
import pytest
import torch

from image2text_amd.decoding import (BEAM_DEAD, GeneratedCaptions, banned_log_softmax_host, beam_advance_host, beam_pool_select_host,
                                     beam_search_host, check_beam_caption_args)

F32, I32 = np.float32, np.int32
V, EOS, PAD = 40, 7, 39
PROMPTS = {1: [3], 3: [5, 11, 2]}
MODEL_SEED = 0


@pytest.fixture(scope='module')
def gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel
    torch.manual_seed(MODEL_SEED)
    cfg = GPT2Config(vocab_size=V, n_positions=32, n_embd=32, n_layer=2, n_head=2, bos_token_id=0, eos_token_id=None, pad_token_id=None)
    m = GPT2LMHeadModel(cfg).float().eval()
    with torch.no_grad():                                     # wider logits than the 0.02 initialisation gives: distinct totals, EOS in reach
        for p in m.parameters():
            p.mul_(6.0) if p.dim() > 1 else None
    cache = {}

    def step_logits(seq):
        key = tuple(seq)
        if key not in cache:
            with torch.no_grad():
                cache[key] = m(torch.tensor([list(seq)])).logits[0, -1].float().numpy().copy()
        return cache[key]
    return m, step_logits


GRID = list(itertools.product((2, 4, 8), (False, True), (0.0, 1.0, 2.0), (False, True), (None, EOS), (1, 6, 12), (1, 3)))


@pytest.mark.parametrize('W,full,lp,early,eos,max_new,plen', GRID)
def test_search_matches_transformers(gpt2, W, full, lp, early, eos, max_new, plen):
    m, step_logits = gpt2
    N = W if full else 1
    prompt = PROMPTS[plen]
    got = beam_search_host(step_logits, prompt, W, N, max_new, eos, PAD, lp, early, ())
    # the totals a decision hung on are more than 1e-4 apart: the comparison does not rest on a tie order
    assert got.gaps and min(got.gaps) > 1e-4, min(got.gaps)
    with torch.no_grad():
        out = m.generate(torch.tensor([prompt]), num_beams=W, do_sample=False, num_return_sequences=N, length_penalty=lp, early_stopping=early,
                         eos_token_id=eos, pad_token_id=PAD, max_new_tokens=max_new, return_dict_in_generate=True, output_scores=True,
                         attention_mask=torch.ones(1, plen, dtype=torch.long))
    want = out.sequences.numpy()
    assert want.shape[0] == N
    L = got.ids.shape[1]
    assert want.shape[1] >= L or not (want[:, L:] != PAD).any()
    width = max(L, want.shape[1])
    a, b = np.full((N, width), PAD), np.full((N, width), PAD)
    a[:, :L], b[:, :want.shape[1]] = got.ids, want
    assert np.array_equal(a, b), (a, b)
    assert np.abs(got.beam_scores - out.sequences_scores.numpy()).max() <= 1e-5
    for n in range(N):
        ln = int(got.lengths[n])
        assert (got.ids[n, ln:] == PAD).all() and (got.token_logprobs[n, ln - plen:] == 0).all()
        assert ln == plen + max_new or got.ids[n, ln - 1] == EOS


def test_ngram_ban_in_the_replica():
    """Vocabulary of 6, bigram ban.  Token 1 always leads, so the unbanned search emits 1 1 1 ...; with the ban the bigram (1, 1) may
    not recur: after 1 1 the best allowed token is 2.  Scores by hand: log-softmax over the allowed tokens only."""
    z = np.array([0.0, 3.0, 2.0, 1.0, 0.5, -1.0], dtype=F32)
    step = lambda seq: z
    free = beam_search_host(step, [1], 2, 1, 3, None, 0, 0.0, False, ())
    assert free.ids[0].tolist() == [1, 1, 1, 1]
    banned = beam_search_host(step, [1], 2, 2, 3, None, 0, 0.0, False, (2,))
    for row in banned.ids.tolist():
        grams = [tuple(row[i:i + 2]) for i in range(len(row) - 1)]
        assert len(grams) == len(set(grams)), row
    lse = lambda mask: np.log(np.exp(z.astype(np.float64))[mask].sum())
    every = np.ones(6, dtype=bool)
    no1 = every.copy()
    no1[1] = False
    # step 1 (after [1]): nothing banned -> 1;  step 2 (after [1, 1]): (1, 1) exists, 1 banned -> 2;  step 3 (after [1, 1, 2]): the tail
    # 2 has no successor yet -> 1
    want = (3.0 - lse(every)) + (2.0 - lse(no1)) + (3.0 - lse(every))
    assert banned.ids[0].tolist() == [1, 1, 2, 1]
    assert abs(float(banned.beam_scores[0]) - want) < 1e-5 and abs(float(banned.logprob[0]) - want) < 1e-5
    lp = banned_log_softmax_host(z, [1, 1], (2,))
    assert lp[1] == -np.inf and abs(float(lp[2]) - (2.0 - lse(no1))) < 1e-6


def _state(B, W, P, max_new, ld=None, pad=9):
    ld = ld or P + max_new
    R = B * W
    s = dict(scores=np.zeros(R, dtype=F32), ids=np.zeros((R, ld), dtype=np.int64), hist=np.repeat(np.arange(R, dtype=I32)[:, None], ld, 1),
             tok_lp=np.zeros((R, ld), dtype=F32), pool_ids=np.full((B, W, ld), pad, dtype=np.int64), pool_lp=np.zeros((B, W, ld), dtype=F32),
             pool_score=np.full((B, W), BEAM_DEAD, dtype=F32), pool_sum=np.zeros((B, W), dtype=F32), pool_len=np.zeros((B, W), dtype=I32),
             pool_n=np.zeros(B, dtype=I32), closed=np.zeros(B, dtype=I32), counters=np.array([P - 1, P], dtype=I32),
             ctrl=np.zeros(2, dtype=I32))
    return s


def _select(s, tok, lp, W, P, max_new, eos, pad, penalty, early):
    beam_pool_select_host(np.asarray(tok, dtype=I32), np.asarray(lp, dtype=F32), s['scores'], s['ids'], s['hist'], s['tok_lp'], s['pool_ids'],
                          s['pool_lp'], s['pool_score'], s['pool_sum'], s['pool_len'], s['pool_n'], s['closed'], s['counters'], s['ctrl'], W, P,
                          max_new, eos, pad, penalty, early)


def test_pool_select_eos_rank_rules():
    """W = 2, E = 4.  Row 0 leads.  EOS (token 5) at rank 1 (< W) enters the pool; in the second case it sits at rank 2 (>= W) and is
    dropped without a trace; the two best other candidates run on either way."""
    W, P, T = 2, 1, 8
    s = _state(1, W, P, T)
    s['ids'][:, 0] = 4
    s['scores'][:] = [-1.0, -2.0]
    tok = [[1, 5, 2, 3], [1, 2, 3, 6]]
    lp = [[-0.1, -0.2, -3.0, -4.0], [-0.5, -3.5, -4.5, -5.5]]           # totals: -1.1, -1.2(eos), -4, -5 | -2.5, -5.5, ...
    _select(s, tok, lp, W, P, T, 5, 9, 1.0, False)
    assert s['pool_n'][0] == 1 and s['pool_ids'][0, 0].tolist() == [4, 5] + [9] * 7 and s['pool_len'][0, 0] == 2
    assert s['pool_score'][0, 0] == F32(-1.2) / F32(1.0) and s['pool_sum'][0, 0] == F32(F32(-1.0) + F32(-0.2))
    assert s['pool_lp'][0, 0, 1] == F32(-0.2) and (s['pool_lp'][0, 0, 2:] == 0).all()
    assert s['ids'][:, :2].tolist() == [[4, 1], [4, 1]] and s['hist'][:, 0].tolist() == [0, 1]
    assert np.array_equal(s['scores'], np.array([-1.1, -2.5], dtype=F32)) and s['tok_lp'][:, 1].tolist() == [F32(-0.1), F32(-0.5)]
    assert s['closed'][0] == 0 and s['ctrl'][1] == 1
    s = _state(1, W, P, T)
    s['scores'][:] = [-1.0, -1.05]
    tok = [[1, 2, 5, 3], [1, 2, 3, 6]]
    lp = [[-0.1, -0.2, -0.3, -4.0], [-0.1, -3.5, -4.5, -5.5]]           # ranks: -1.1, -1.15 (row 1), -1.2, -1.3 (eos: rank 3)
    _select(s, tok, lp, W, P, T, 5, 9, 1.0, False)
    assert s['pool_n'][0] == 0 and (s['pool_ids'] == 9).all() and s['ids'][:, 1].tolist() == [1, 1] and s['hist'][:, 0].tolist() == [0, 1]


def test_pool_select_full_pool_and_close_rules():
    """a full pool gives up its worst entry only to a better score (an equal one stays out); the close rule for both early_stopping
    values; nothing is offered to a closed image"""
    W, P, T = 2, 1, 8
    tok = [[5, 1, 2, 3], [1, 2, 3, 6]]
    lp = [[-0.5, -0.6, -3.0, -4.0], [-0.7, -3.5, -4.5, -5.5]]           # the EOS at rank 0, total -0.5; the best running total -0.6

    def full(worst):
        s = _state(1, W, P, T)
        s['scores'][:] = [0.0, -1.0]
        s['pool_n'][0] = 2
        s['pool_score'][0] = [-0.25, worst]
        s['pool_ids'][0, :, :2] = [[4, 7], [4, 8]]
        s['pool_len'][0] = [2, 2]
        return s
    s = full(-0.75)
    _select(s, tok, lp, W, P, T, 5, 9, 0.0, False)                       # penalty 0: the offer scores -0.5 and replaces the worst
    assert s['pool_score'][0].tolist() == [-0.25, -0.5] and s['pool_ids'][0, :, 1].tolist() == [7, 5]
    assert s['closed'][0] == 1                                           # the best running total -0.6 does not exceed the worst -0.5
    s = full(-0.5)
    _select(s, tok, lp, W, P, T, 5, 9, 0.0, False)                       # an equal score: the entry the pool holds goes first
    assert s['pool_score'][0].tolist() == [-0.25, -0.5] and s['pool_ids'][0, :, 1].tolist() == [7, 8]
    s = full(-0.75)
    s['pool_score'][0] = [-0.25, -0.75]
    lp2 = [[-0.8, -0.6, -3.0, -4.0], [-0.7, -3.5, -4.5, -5.5]]          # the EOS at rank 1 scores -0.8: worse than the worst, stays out
    tok2 = [[5, 1, 2, 3], [1, 2, 3, 6]]
    _select(s, tok2, lp2, W, P, T, 5, 9, 0.0, False)
    assert s['pool_score'][0].tolist() == [-0.25, -0.75] and s['closed'][0] == 0 and s['ctrl'][1] == 1   # -0.6 > -0.75: stays open
    before = {k: v.copy() for k, v in s.items()}
    s['closed'][0] = 1
    s['ctrl'][1] = 0
    before['closed'][0] = 1
    before['ctrl'][1] = 0
    _select(s, tok, lp, W, P, T, 5, 9, 0.0, False)
    assert all(np.array_equal(s[k], before[k]) for k in s), 'a closed image is left alone'
    # early_stopping=True: a pool that fills closes the image whatever the running beams could reach
    s = _state(1, W, P, T)
    s['scores'][:] = [0.0, -0.01]
    tok3 = [[5, 1, 2, 3], [5, 2, 3, 6]]
    lp3 = [[-0.5, -3.6, -4.0, -5.0], [-0.6, -3.5, -4.5, -5.5]]
    for early, want in ((True, 1), (False, 1)):
        s = _state(1, W, P, T)
        s['scores'][:] = [0.0, -0.01]
        _select(s, tok3, lp3, W, P, T, 5, 9, 1.0, early)
        assert s['pool_n'][0] == 2 and s['closed'][0] == want            # both EOS enter; the best running -3.51 is below the worst
    lp4 = [[-3.0, -0.1, -4.0, -5.0], [-3.1, -0.2, -4.5, -5.5]]          # the running beams lead: EOS at ranks 2 and 3 are dropped
    s = _state(1, W, P, T)
    s['scores'][:] = [0.0, -0.01]
    s['pool_n'][0] = 2
    s['pool_score'][0] = [-1.0, -2.0]
    _select(s, [[5, 1, 2, 3], [5, 2, 3, 6]], lp4, W, P, T, 5, 9, 1.0, False)
    assert s['closed'][0] == 0                                           # -0.1 / 1 > -2: improvement is possible
    s['closed'][0] = 0
    s2 = _state(1, W, P, T)
    s2['scores'][:] = [0.0, -0.01]
    s2['pool_n'][0] = 2
    s2['pool_score'][0] = [-1.0, -2.0]
    _select(s2, [[5, 1, 2, 3], [5, 2, 3, 6]], lp4, W, P, T, 5, 9, 1.0, True)
    assert s2['closed'][0] == 1                                          # a full pool closes under early_stopping


def test_pool_select_at_the_bound_every_candidate_hits():
    """the max_new-th token: every candidate hits, the W best enter the pool at total / max_new ** penalty, the image closes, the rows
    stay, and the advance raises the done flag"""
    W, P, T = 2, 2, 3
    s = _state(1, W, P, T)
    s['ids'][:, :4] = [[4, 4, 1, 2], [4, 4, 3, 6]]
    s['tok_lp'][:, 2:4] = [[-0.5, -0.5], [-0.7, -0.8]]
    s['scores'][:] = [-1.0, -1.5]
    s['counters'][:] = [3, 4]
    ids0, hist0 = s['ids'].copy(), s['hist'].copy()
    tok = [[1, 2, 3, 6], [1, 2, 3, 6]]
    lp = [[-0.5, -2.0, -3.0, -4.0], [-0.25, -3.5, -4.5, -5.5]]          # totals -1.5, -1.75, ...
    _select(s, tok, lp, W, P, T, None, 9, 2.0, False)
    assert s['pool_n'][0] == 2 and s['closed'][0] == 1 and s['ctrl'][1] == 0
    assert np.array_equal(s['pool_score'][0], np.array([-1.5, -1.75], dtype=F32) / F32(9.0))
    assert s['pool_ids'][0].tolist() == [[4, 4, 1, 2, 1], [4, 4, 3, 6, 1]] and s['pool_len'][0].tolist() == [5, 5]
    assert s['pool_lp'][0].tolist() == [[0, 0, -0.5, -0.5, -0.5], [0, 0, F32(-0.7), F32(-0.8), -0.25]]
    assert np.array_equal(s['ids'], ids0) and np.array_equal(s['hist'], hist0)
    beam_advance_host(s['counters'], s['ctrl'])
    assert s['ctrl'].tolist() == [1, 0] and s['counters'].tolist() == [4, 5]


def test_refusals():
    ok = dict(num_beams=3, num_return_sequences=2, length_penalty=1.0, early_stopping=False)
    assert check_beam_caption_args(**ok) == 3
    assert check_beam_caption_args(1, 1, 1.0, False, temperature=0.7, top_k=5, seed=3, prompt_lengths=[1]) == 1      # W = 1: not this path
    for bad in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=2.5), dict(num_return_sequences=4), dict(num_return_sequences=0),
                dict(length_penalty=float('nan')), dict(length_penalty=float('inf')), dict(early_stopping='never'), dict(early_stopping=1),
                dict(temperature=0.7), dict(top_k=1), dict(top_k=50), dict(nucleus_p=0.9), dict(seed=1), dict(eos=-2), dict(poll_every=-1)):
        with pytest.raises(ValueError):
            check_beam_caption_args(**{**ok, **bad})
    for bad, word in ((dict(prompt_lengths=[1, 2]), 'prompt_lengths'), (dict(prompt_prefill='pass'), 'pass'),
                      (dict(repetition_penalty=1.2), 'repetition_penalty'), (dict(min_new_tokens=1, eos=3), 'min_new_tokens'),
                      (dict(suppress_tokens=[4]), 'suppress_tokens'), (dict(causal=False), 'causal')):
        with pytest.raises(NotImplementedError, match=word):
            check_beam_caption_args(**{**ok, **bad})


def test_generated_captions_gains_a_defaulted_field():
    z = torch.zeros(1)
    four = GeneratedCaptions(z, z, z, z)
    assert four.beam_scores is None and four.prompt_lengths is None and len(four) == 4 and GeneratedCaptions._fields == ('ids', 'lengths', 'token_logprobs', 'logprob')
    six = GeneratedCaptions(z, z, z, z, None, z + 1)
    a, b, c, d = six
    assert six.beam_scores is not None and six.prompt_lengths is None
