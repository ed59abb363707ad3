"""generate_captions / search_phrases with ``phrase_sets``, ``phrase_set_index`` and ``prompt_lengths`` on the MI355X, end to end (DESIGN.md
4x): the tiny dense model (trained weights) and the tiny Llama with a soft prompt; B = 6 images, P = 3 prompt columns, prompt lengths
2 / 3 / 1 / 3 / 2 / 1.

Ragged versus equal length is held bit for bit (4p's argument: the two runs have the same rows and launch shapes, every kernel of a
step treats rows independently, and a forced full step runs the body a prefill step runs).  Per-image sets are held bit for bit
against one-set calls.  ``logprob`` is held to score() at 4 . logits_tol, the bound of tests/test_generate_captions_phrases_gpu.py;
greedy ids to ``constrained_decode_host`` from the image's root over the model's own forward under that file's gap rule: the
step-vs-forward logit difference is MEASURED here, an image whose replica decided every step on a gap above it must agree in ids,
length, phrase index and token log-probs, and at most 1 image in 8 may fall outside (at B = 6: none)."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import constrained_decode_host, phrase_forest
from image2text_amd.synth import synthetic_batch, tiny_config
from test_generate_captions_gpu import GREEDY, _ved
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

B, P, T, EOS = 6, 3, 6, 5
PLEN = [2, 3, 1, 3, 2, 1]
SETS = [[[17, 42], [17, 42, 8], [17, 9], [63], [63, 21, 30], [77, 4, 4], [17, 9]],     # 4u's set: 1 extends 0; 6 repeats 2
        [[63], [21]],                                                                  # yes / no
        [[30, 31, 32], [30, 33], [17, 42], [40], [41], [44, 45]]]                      # shares [17, 42] with set 0, under another index
INDEX = [0, 1, 2, 2, 0, 1]
SIX = SETS + [[[50], [51, 52]], [[17, 9], [17, 42]], [[60, 61, 62], [60], [64]]]      # one set per image
# The input seed of each model (images and prompts as tests/test_generate_captions_phrases_gpu.py makes them, the first 6 of 8).  Chosen
# on the CPU from candidates 0 .. 15: ``constrained_decode_host`` from every image's root over the oracle's forward
# (oracle/reference_model.forward for tiny; oracle encode + the checkpoint's own transformers module in fp32 for the Llama), taking a
# seed whose smallest decision gap over the 6 images and all steps is the largest (tiny) or among the largest (Llama) and above the
# step-vs-forward difference this file measures.  Oracle gaps per image at the chosen seed -- tiny seed 10: [0.568, 7.445, 0.099,
# 0.141, 0.541, 9.995] (smallest 0.0993; the runners-up 6: 0.0772, 5: 0.0554; seed 0, 4u's, has 0.0260); llama seed 7: [0.412, 0.717,
# 0.0925, 0.134, 0.729, 0.171] (smallest 0.0925; seed 9: 0.0930, seed 3: 0.0010).  The oracle alone excuses 0 of 6 images on each model.
SEEDS = dict(tiny=10, llama=7)
SAMPLED = dict(seed=11, num_return_sequences=2, temperature=1.3, top_k=40)


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module', params=['tiny', 'llama'])
def model(request, tiny_weights, tmp_path_factory):
    """-> (name, model, images [6, ...], prompt [6, 3], pad id, a function that builds the model again)"""
    name = request.param
    if name == 'llama':
        from test_hf_decoder_gpu import _llama_model
        mp = pytest.MonkeyPatch()
        request.addfinalizer(mp.undo)

        def fresh():
            return _llama_model(tmp_path_factory.mktemp('llama'), mp, 'llama')[1].to(dev()).eval()
        m = fresh()
        V = m._engine.dec.V
        g = torch.Generator().manual_seed(SEEDS[name])
        images, prompt = torch.randn(8, 3, 32, 32, generator=g)[:B], torch.randint(0, V, (8, P), generator=g)[:B]
    else:
        fresh = lambda: _ved(tiny_config(), tiny_weights)
        m = fresh()
        V = m._engine.dec.V
        images, labels = synthetic_batch(8, 32, 12, min(V, 384), seed=SEEDS[name])
        images, prompt = images[:B], labels[:B, :P].clamp(min=0)
    assert V > 90
    return name, m, images.to(dev()), prompt.to(dev()), V - 1, fresh


def bit(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def rows_equal(a, b, ia, ib, pa, pb, pmin_a, pmin_b):
    """image ia of GeneratedCaptions a against image ib of b, bit for bit: ids up to the row's length, lengths, phrase index and the
    emitted tokens' log-probs (column-aligned: entry t of a call belongs to column pmin + t).  ``logprob`` is by definition the call's
    own ``token_logprobs.sum(dim=-1)``, which is held bit for bit inside each call; across calls it is held bit for bit whenever the
    two calls' rows have the same width and the same first column (every comparison but ragged against equal length, and per-image
    sets against a one-set call that ends on another column).  Where they differ, equal entries sit at other offsets of a row of
    another width, torch's reduction associates a row's entries by position, and the sums may be neighbouring fp32 numbers (seen on
    the MI355X: -31.3858 against -31.3857): the emitted entries themselves are what is compared there."""
    for out in (a, b):
        if not torch.equal(bit(out.logprob), bit(out.token_logprobs.sum(dim=-1))):
            return False
    same_layout = a.token_logprobs.shape[-1] == b.token_logprobs.shape[-1] and pmin_a == pmin_b
    if same_layout and not torch.equal(bit(a.logprob[ia]), bit(b.logprob[ib])):
        return False
    for n in range(a.ids.shape[1]):
        la, lb = int(a.lengths[ia, n]), int(b.lengths[ib, n])
        if la != lb or a.ids[ia, n, :la].tolist() != b.ids[ib, n, :lb].tolist() or int(a.phrase_index[ia, n]) != int(b.phrase_index[ib, n]):
            return False
        ta, tb = a.token_logprobs[ia, n, pa - pmin_a:la - pmin_a], b.token_logprobs[ib, n, pb - pmin_b:lb - pmin_b]
        if not torch.equal(bit(ta), bit(tb)):
            return False
        if bool((a.token_logprobs[ia, n, :pa - pmin_a] != 0).any()) or bool((a.token_logprobs[ia, n, la - pmin_a:] != 0).any()):
            return False
    return True


def beams_equal(a, b, ia, ib):
    return all(torch.equal(bit(x[ia]), bit(y[ib])) for x, y in zip(a[:4], b[:4]))


def check_rows(out, prompt, plen, index, sets, pad, N):
    """every row is its prompt + a phrase of ITS OWN set + EOS, then pad; phrase_index names the lowest duplicate"""
    ids, lens, idx = out.ids.cpu().numpy(), out.lengths.cpu().numpy(), out.phrase_index.cpu().numpy()
    assert tuple(idx.shape) == (B, N) and out.phrase_index.dtype == torch.int32
    for b in range(B):
        mine = sets[index[b]]
        for n in range(N):
            k = int(idx[b, n])
            assert 0 <= k < len(mine) and mine.index(mine[k]) == k, (b, n, k)
            row = prompt[b, :plen[b]].tolist() + mine[k] + [EOS]
            assert int(lens[b, n]) == len(row) and ids[b, n, :len(row)].tolist() == row and (ids[b, n, len(row):] == pad).all(), (b, n, ids[b, n])


def test_ragged_against_equal_length(model):
    name, m, images, prompt, pad, _ = model
    kw = dict(max_new_tokens=T, eos_token_id=EOS, pad_token_id=pad, phrase_sets=SETS, phrase_set_index=INDEX)
    pmin = min(PLEN)
    for mode, N in ((GREEDY, 1), (SAMPLED, 2)):
        for prefill in ('steps', 'pass'):
            rag = m.generate_captions(images, prompt, **kw, **mode, prompt_lengths=PLEN, prompt_prefill=prefill)
            assert rag.prompt_lengths.tolist() == PLEN and m._captioner.last_prefill_steps == (pmin - 1 if prefill == 'steps' else 0)
            check_rows(rag, prompt, PLEN, INDEX, SETS, pad, N)
            if prefill == 'pass':
                assert torch.equal(rag.ids, steps.ids) and torch.equal(rag.phrase_index, steps.phrase_index), "'pass' = 'steps' in ids"
                continue
            steps = rag
            for p in sorted(set(PLEN)):
                eq = m.generate_captions(images, prompt[:, :p], **kw, **mode)
                assert eq.prompt_lengths is None
                for b in (b for b in range(B) if PLEN[b] == p):
                    assert rows_equal(rag, eq, b, b, p, p, pmin, p), f'{name} {mode}: image {b} (p = {p}) ragged vs equal length'
    W = 3
    skw = dict(eos_token_id=EOS, num_beams=W, num_return_sequences=2, length_penalty=0.7, phrase_sets=SETS, phrase_set_index=INDEX)
    rag = m.search_phrases(images, prompt, **skw, prompt_lengths=PLEN)
    assert rag.exhaustive is False and tuple(rag.phrase_index.shape) == (B, 2)
    for p in sorted(set(PLEN)):
        eq = m.search_phrases(images, prompt[:, :p], **skw)
        for b in (b for b in range(B) if PLEN[b] == p):
            assert beams_equal(rag, eq, b, b), f'{name}: search, image {b} (p = {p}) ragged vs equal length'
    for b in range(B):
        assert all(0 <= int(k) < len(SETS[INDEX[b]]) for k in rag.phrase_index[b]) and len(set(rag.phrase_index[b].tolist())) == 2
        for n in range(2):
            assert int(rag.lengths[b, n]) == len(SETS[INDEX[b]][int(rag.phrase_index[b, n])]) + 1


def test_per_image_sets_against_one_set(model):
    name, m, images, prompt, pad, _ = model
    kw = dict(max_new_tokens=T, eos_token_id=EOS, pad_token_id=pad)
    skw = dict(eos_token_id=EOS, num_beams=5, num_return_sequences=2)
    for mode in (GREEDY, SAMPLED):
        one = m.generate_captions(images, prompt, **kw, **mode, phrases=SETS[0])
        zero = m.generate_captions(images, prompt, **kw, **mode, phrase_sets=SETS, phrase_set_index=[0] * B)
        assert all(rows_equal(zero, one, b, b, P, P, P, P) for b in range(B)), f'{name} {mode}: index all zero vs phrases=sets[0]'
        six = m.generate_captions(images, prompt, **kw, **mode, phrase_sets=SIX)
        for b in range(B):
            alone = m.generate_captions(images, prompt, **kw, **mode, phrases=SIX[b])
            assert rows_equal(six, alone, b, b, P, P, P, P), f'{name} {mode}: image {b} of six sets vs phrases=sets[{b}]'
    one = m.search_phrases(images, prompt, SETS[0], **skw)
    zero = m.search_phrases(images, prompt, **skw, phrase_sets=SETS, phrase_set_index=[0] * B)
    assert all(beams_equal(zero, one, b, b) for b in range(B)) and zero.exhaustive == one.exhaustive
    six = m.search_phrases(images, prompt, **dict(skw, num_return_sequences=2), phrase_sets=SIX)
    for b in range(B):
        alone = m.search_phrases(images, prompt, SIX[b], **skw)
        assert beams_equal(six, alone, b, b), f'{name}: search, image {b} of six sets vs phrases=sets[{b}]'
    assert six.exhaustive is True, 'five rows hold the widest level of every one of the six sets (five first tokens in set 2)'
    assert m.search_phrases(images, prompt, **dict(skw, num_beams=4), phrase_sets=SIX).exhaustive is False


def test_logprob_against_score_and_ids_against_the_replica(model):
    name, m, images, prompt, pad, _ = model
    V = m._engine.dec.V
    m.generate_captions(images[:1], prompt[:1], T, EOS, pad, **GREEDY, phrase_sets=SETS, phrase_set_index=[0])
    cap = m._captioner
    pmin, pmax = min(PLEN), max(PLEN)
    plen_dev = torch.tensor(PLEN, device=dev())
    # the step-vs-forward difference, measured on the rows that emit: each(i) runs after full step i, column pmin + i
    rows, worst, ended = [None], [0.0], [torch.zeros(B, dtype=torch.bool, device=dev())]

    def each(i):
        st = cap._state
        col = pmin + i
        emits = (plen_dev <= col) & ~ended[0]
        for b in torch.nonzero(emits).flatten().tolist():
            with torch.no_grad():
                fwd = m(images=images[b:b + 1], ids=st.ids[b:b + 1, :col]).logits[0, -1].float()[:V]
            step = st.logits[b, :V]
            live = torch.isfinite(step)
            worst[0] = max(worst[0], float((step - fwd).abs()[live].max()))
        ended[0] = st.finished.bool().clone()
    out = cap.generate_captions(images, prompt, T, EOS, pad, 1, None, poll_every=0, use_graph=False, prompt_lengths=PLEN, phrase_sets=SETS,
                                phrase_set_index=INDEX, each=each)
    diff = worst[0]
    check_rows(out, prompt, PLEN, INDEX, SETS, pad, 1)
    ids = out.ids[:, 0]
    L = ids.shape[1]
    with torch.no_grad():
        logits = m(images=images, ids=ids).logits.float()
    tol = logits_tol(logits.cpu().numpy())
    col = torch.arange(pmin, L, device=dev())[None, :]
    live = (col >= plen_dev[:, None]) & (col < out.lengths.reshape(B, 1))
    sc = m.score(images, ids).token_logprobs[:, pmin - 1:L - 1]
    err = float(((out.token_logprobs[:, 0] - sc).abs() * live).max())
    err_sum = float((out.logprob[:, 0] - (sc * live).sum(dim=-1)).abs().max())
    print(f'{name}: measured step-vs-forward logit difference {diff:.3g}; logits_tol {tol:.3g}; token_logprobs vs score {err:.3g}, '
          f'logprob vs score {err_sum:.3g} (bar {4 * tol:.3g})')
    assert 0 < diff < 0.5
    assert err <= 4 * tol and err_sum <= 4 * tol
    # search_phrases reports the same quantity
    beams = m.search_phrases(images, prompt, eos_token_id=EOS, num_beams=8, num_return_sequences=1, phrase_sets=SETS, phrase_set_index=INDEX,
                             prompt_lengths=PLEN)
    for b in range(B):
        seq = prompt[b, :PLEN[b]].tolist() + SETS[INDEX[b]][int(beams.phrase_index[b, 0])] + [EOS]
        t = torch.tensor([seq], device=dev())
        want = float(m.score(images[b:b + 1], t).token_logprobs[0, PLEN[b] - 1:].sum())
        assert abs(float(beams.logprob[b, 0]) - want) <= 4 * tol, (b, float(beams.logprob[b, 0]), want)
    # the replica over the model's own forward, from the image's root
    forest = phrase_forest(SETS, EOS, V)
    cache, outside, gaps = {}, 0, []

    def step_logits(b):
        def f(seq):
            if (b, tuple(seq)) not in cache:
                with torch.no_grad():
                    z = m(images=images[b:b + 1], ids=torch.tensor([list(seq)], device=dev())).logits[0, -1].float()
                cache[(b, tuple(seq))] = z.cpu().numpy()[:V].copy()
            return cache[(b, tuple(seq))]
        return f
    for b in range(B):
        want = constrained_decode_host(step_logits(b), prompt[b, :PLEN[b]].tolist(), forest, EOS, pad, T, start=int(forest.roots[INDEX[b]]))
        gaps.append(min(want.gaps))
        if not min(want.gaps) > diff:
            outside += 1
            continue
        assert int(out.lengths[b, 0]) == want.length and ids[b, :want.length].tolist() == want.ids.tolist(), f'{name}: image {b}'
        assert int(out.phrase_index[b, 0]) == want.phrase_index
        lp = out.token_logprobs[b, 0, PLEN[b] - pmin:PLEN[b] - pmin + want.steps].cpu().numpy()
        assert np.abs(lp - want.token_logprobs).max() <= 4 * tol
    print(f'{name}: {outside} of {B} images decide inside the measured difference; smallest gaps {[round(g, 4) for g in gaps]}')
    assert outside * 8 <= B, f'{outside} of {B} images fall outside the gap rule'


def test_robustness(model):
    name, m, images, prompt, pad, fresh = model
    kw = dict(max_new_tokens=T, eos_token_id=EOS, pad_token_id=pad)
    sets_kw = dict(phrase_sets=SETS, phrase_set_index=INDEX, prompt_lengths=PLEN)
    skw = dict(eos_token_id=EOS, num_beams=3, num_return_sequences=2)
    clean = fresh()
    # calls without the keyword: no 'trie_sets' / 'phrase_beam_sets' key and none of the new buffers
    free = clean.generate_captions(images, prompt, **kw, **GREEDY)
    old = clean.generate_captions(images, prompt, **kw, **GREEDY, phrases=SETS[0])
    old_rag = clean.generate_captions(images, prompt, **kw, **GREEDY, prompt_lengths=PLEN)
    old_beams = clean.search_phrases(images, prompt, SETS[0], **skw)
    cst, sst = clean._captioner._state, clean._phrase_searcher._state
    assert not [k for k in cst.graphs if isinstance(k, tuple) and k and k[0] == 'trie_sets'] and cst.node_init is None
    assert not [k for k in sst.graphs if isinstance(k, tuple) and k and k[0] == 'phrase_beam_sets']
    assert sst.set_node_init is None and sst.set_plen is None and sst.set_longest is None
    # interleaved on one model = each on a model of its own
    a1 = m.generate_captions(images, prompt, **kw, **GREEDY, **sets_kw)
    a2 = m.generate_captions(images, prompt, **kw, **GREEDY, phrases=SETS[0])
    a3 = m.search_phrases(images, prompt, **skw, **sets_kw)
    a4 = m.generate_captions(images, prompt, **kw, **GREEDY, prompt_lengths=PLEN)
    a5 = m.generate_captions(images, prompt, **kw, **GREEDY, **sets_kw)
    a6 = m.search_phrases(images, prompt, SETS[0], **skw)
    a7 = m.generate_captions(images, prompt, **kw, **GREEDY)
    a8 = m.search_phrases(images, prompt, **skw, **sets_kw)
    pm = min(PLEN)
    assert all(rows_equal(a1, a5, b, b, PLEN[b], PLEN[b], pm, pm) for b in range(B)) and all(beams_equal(a3, a8, b, b) for b in range(B))
    other = fresh()
    b1 = other.generate_captions(images, prompt, **kw, **GREEDY, **sets_kw)
    b3 = other.search_phrases(images, prompt, **skw, **sets_kw)
    assert all(rows_equal(a1, b1, b, b, PLEN[b], PLEN[b], pm, pm) for b in range(B)), f'{name}: interleaved vs fresh, generate'
    assert all(beams_equal(a3, b3, b, b) for b in range(B)), f'{name}: interleaved vs fresh, search'
    assert all(rows_equal(a2, old, b, b, P, P, P, P) for b in range(B)) and all(beams_equal(a6, old_beams, b, b) for b in range(B))
    assert torch.equal(a4.ids, old_rag.ids) and torch.equal(bit(a4.token_logprobs), bit(old_rag.token_logprobs))
    assert torch.equal(a7.ids, free.ids) and torch.equal(bit(a7.token_logprobs), bit(free.token_logprobs))
    st = m._captioner._state
    assert any(isinstance(k, tuple) and k[0] == 'trie_sets' and 'ragged' in k for k in st.graphs)
    assert any(isinstance(k, tuple) and k[0] == 'phrase_beam_sets' for k in m._phrase_searcher._state.graphs)
    # eager = graph, every poll_every
    cap, srch = m._captioner, m._phrase_searcher
    from image2text_amd.decoding import caption_facts, check_phrase_search_args
    facts = caption_facts(m)
    for call in (dict(use_graph=False), dict(poll_every=0), dict(poll_every=1), dict(poll_every=8), dict(poll_every=0, use_graph=False)):
        got = cap.generate_captions(images, prompt, T, EOS, pad, 1, None, **sets_kw, **call)
        assert all(rows_equal(a1, got, b, b, PLEN[b], PLEN[b], pm, pm) for b in range(B)), f'{name}: generate {call}'
        if call.get('poll_every') == 0:
            assert cap.last_replays == max(PLEN) - pm + T
        if call.get('poll_every') == 1:
            assert cap.last_replays <= max(PLEN) - pm + 4, 'the longest phrase has three tokens'
        sets, W, N, plen = check_phrase_search_args(None, EOS, facts.V, P, facts.cache_window, 3, 2, 0.0, call.get('poll_every', 8), facts.causal,
                                                    facts.sparse, SETS, INDEX, PLEN, B)
        got = srch.search_sets(images, prompt, sets, EOS, W, N, 0.0, plen=plen, **call)
        assert all(beams_equal(a3, got, b, b) for b in range(B)), f'{name}: search {call}'
        if call.get('poll_every') == 0:
            assert srch.last_replays == max(PLEN) - pm + 3 + 1
    # the refusals reach the caller from the model, before anything runs
    with pytest.raises(ValueError, match='phrases and phrase_sets are both given'):
        m.generate_captions(images, prompt, **kw, **GREEDY, phrases=SETS[0], phrase_sets=SETS, phrase_set_index=INDEX)
    with pytest.raises(ValueError, match=r'phrase_set_index\[3\] = 3'):
        m.search_phrases(images, prompt, eos_token_id=EOS, phrase_sets=SETS, phrase_set_index=[0, 1, 2, 3, 0, 1])
    with pytest.raises(ValueError, match='one set per image: 3 sets for 6 images'):
        m.generate_captions(images, prompt, **kw, **GREEDY, phrase_sets=SETS)
    with pytest.raises(ValueError, match=r'phrase_sets\[1\]: phrases\[0\] is empty'):
        m.search_phrases(images, prompt, eos_token_id=EOS, phrase_sets=[SETS[0], [[]]], phrase_set_index=[0] * B)
    with pytest.raises(NotImplementedError, match='phrase_sets under num_beams > 1'):
        m.generate_captions(images, prompt, **kw, phrase_sets=SETS, phrase_set_index=INDEX, num_beams=2)
    with pytest.raises(NotImplementedError, match='phrase_sets with repetition_penalty'):
        m.generate_captions(images, prompt, **kw, **GREEDY, phrase_sets=SETS, phrase_set_index=INDEX, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match='phrases with prompt_lengths'):
        m.generate_captions(images, prompt, **kw, **GREEDY, phrases=SETS[0], prompt_lengths=PLEN)
    with pytest.raises(ValueError, match='num_return_sequences = 3'):
        m.search_phrases(images, prompt, eos_token_id=EOS, num_beams=4, num_return_sequences=3, phrase_sets=SETS, phrase_set_index=INDEX)
