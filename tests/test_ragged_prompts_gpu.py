"""generate_captions(prompt_lengths=...) on the MI355X: prompts of different lengths in one batch.

Kernel level: ops.caption_finish_ragged driven column by column behind a scripted chooser, against decoding.apply_finish_rule_ragged
after every step, exactly.

End to end: for every distinct prompt length p the expectation is the EXISTING equal-length generate_captions on the same images with
prompt_ids[:, :p], compared at the rows whose length is p.  Both runs have the same rows and launch shapes and every kernel of a step
treats rows independently, so ids, lengths and token_logprobs (shifted by p - Pmin columns) are held to BIT equality; there is no
tolerance in this file."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import Sampling, apply_finish_rule_ragged
from image2text_amd.synth import det_init_, reference_unit_test_config, sharpen_gates_, synthetic_batch, tiny_config

pytestmark = pytest.mark.gpu

F32 = torch.float32
GREEDY = dict(top_k=1)
SAMPLING = dict(temperature=1.2, top_k=30, nucleus_p=None, seed=77, num_return_sequences=2)
PLEN, P, T = (1, 3, 5, 3), 5, 8


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def bits(x):
    return x.view(torch.int32) if x.dtype == F32 else x


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('eos', [4, None], ids=['eos', 'budget'])
def test_caption_finish_ragged_against_the_host_rule(ops, eos):
    """R = 6 rows of 3 images (N = 2), prompts of 1, 5 and 3 tokens in 5 columns, 4 new tokens.  The scripted chooser writes a token and a
    log-prob at EVERY row -- an EOS at the forced ones, which must neither stay nor finish the row.  'eos': every row ends before
    Pmax + max_new (one of them on its budget, one on both at once) and `done` rises early; 'budget': no EOS id, rows end on their
    budgets and the last step raises `done`.  Guard rows and words behind every buffer survive."""
    EOS, PAD, G = 4, 11, 99
    B, N, R, MAX_NEW, ld = 3, 2, 6, 4, 11
    plen = np.array([1, 5, 3])
    rows = np.repeat(plen, N)
    pmin, pmax = 1, 5
    total = pmax + MAX_NEW
    prompt = np.array([[7, G, G, G, G], [7, EOS, 8, EOS, 6], [7, 8, EOS, G, G]])          # G: columns nothing may read
    table = np.array([[7, 1, EOS, 5, 5, 5, 5, 5, 5],               # ends at column 2
                      [7, 1, 2, 3, 5, 5, 5, 5, 5],                 # no EOS in its 4 tokens: ends on the budget at column 4
                      [7, EOS, 8, EOS, 6, 2, EOS, 5, 5],           # the EOS's of its prompt finish nothing; ends at column 6
                      [7, EOS, 8, EOS, 6, EOS, 5, 5, 5],           # its first emitted token
                      [7, 8, EOS, 1, 2, 3, EOS, 5, 5],             # EOS as its 4th token
                      [7, 8, EOS, EOS, 5, 5, 5, 5, 5]])
    assert all((table[r, :rows[r]] == prompt[r // N, :rows[r]]).all() for r in range(R))
    rng = np.random.default_rng(3)
    lps = -rng.random((R, total - pmin)).astype(np.float32) - 0.5
    want_ids, want_len, want_lp = apply_finish_rule_ragged(table, rows, MAX_NEW, eos, PAD, lps)
    L = want_ids.shape[1]
    assert want_len.tolist() == ([3, 5, 7, 6, 7, 4] if eos is not None else [5, 5, 9, 9, 7, 7])
    n_full = pmax - pmin + MAX_NEW
    forced = np.arange(total)[None, :] < rows[:, None]
    stream = torch.from_numpy(np.where(forced, EOS, table)).to(dev())
    s_lp = torch.from_numpy(lps).to(dev())

    i32 = dict(dtype=torch.int32, device=dev())
    ids = torch.full((R + 1, ld), -7, dtype=torch.long, device=dev())
    ids[:R, :1] = 7                                               # the first column is every row's prompt; the rest the kernel forces
    tok_lp = torch.full((R + 1, ld), float('nan'), device=dev())
    finished, lengths = torch.zeros(R + 1, **i32), torch.full((R + 1,), -3, **i32)
    lengths[:R] = torch.from_numpy(rows + MAX_NEW).to(dev())
    prm = torch.full((B + 1, P), -9, dtype=torch.long, device=dev())
    prm[:B] = torch.from_numpy(prompt).to(dev())
    pl = torch.full((B + 1,), 1000, **i32)
    pl[:B] = torch.from_numpy(plen).to(dev())
    counters, ctrl = torch.tensor([pmin - 1, pmin, -5], **i32), torch.tensor([0, 0, -5], **i32)
    state = (ids, tok_lp, finished, lengths, counters, ctrl, prm, pl)

    def finish():
        ops.caption_finish_ragged(ids, ld, counters[1:2], prm, pl, N, MAX_NEW, eos, PAD, finished, lengths, tok_lp, ctrl, R)

    for step in range(L - pmin):
        c = pmin + step
        assert counters.tolist() == [c - 1, c, -5] and ctrl.tolist() == [0, 0, -5]
        ids[:R, c], tok_lp[:R, c] = stream[:, c], s_lp[:, c - pmin]          # what a chooser writes at ids[r][len], on every row
        finish()
        fin = want_len <= c + 1
        assert np.array_equal(ids[:R, :c + 1].cpu().numpy(), want_ids[:, :c + 1]), f'ids after column {c}'
        assert np.array_equal(tok_lp[:R, pmin:c + 1].cpu().numpy(), want_lp[:, :c + 1 - pmin]), f'tok_lp after column {c}'
        assert np.array_equal(finished[:R].cpu().numpy(), fin.astype(np.int32)), f'finished after column {c}'
        assert np.array_equal(lengths[:R].cpu().numpy(), np.where(fin, want_len, rows + MAX_NEW)), f'lengths after column {c}'
        assert ctrl.tolist() == [0, int((~fin).sum()), -5], f'ctrl after column {c}'
        assert bool((ids[:R, c + 1:] == -7).all()) and torch.isnan(tok_lp[:R, c + 1:]).all() and torch.isnan(tok_lp[:R, :pmin]).all()
        ops.beam_advance(counters, ctrl)
    assert ctrl.tolist() == [1, 0, -5] and counters.tolist() == [L - 1, L, -5]
    assert (L - pmin < n_full) == (eos is not None)               # 'eos': `done` rose before the last step a host would launch
    snap = [x.clone() for x in state]
    for _ in range(2):                                            # past `done` nothing is written, whatever the column holds
        finish()
        ops.beam_advance(counters, ctrl)
    torch.cuda.synchronize()
    for a, b in zip(snap, state):
        assert torch.equal(bits(a), bits(b))
    assert bool((finished[:R] == 1).all()) and np.array_equal(lengths[:R].cpu().numpy(), want_len)
    assert not bool((ids[:R, :L] == G).any())
    # the guards: the row behind the ids and the log-probs, the words behind finished / lengths / ctrl / counters, the inputs
    assert bool((ids[R] == -7).all()) and bool((ids[:R, L:] == -7).all()) and torch.isnan(tok_lp[R]).all()
    assert int(finished[R]) == 0 and int(lengths[R]) == -3 and int(ctrl[2]) == -5
    assert bool((prm[B] == -9).all()) and np.array_equal(prm[:B].cpu().numpy(), prompt) and pl.tolist() == [1, 5, 3, 1000]


def test_caption_finish_ragged_refusals(ops):
    from image2text_amd.lib import I2TError
    i32 = dict(dtype=torch.int32, device=dev())
    ids, lp = torch.zeros(4, 8, dtype=torch.long, device=dev()), torch.zeros(4, 8, device=dev())
    fin, ln, ctrl, cnt = torch.zeros(4, **i32), torch.zeros(4, **i32), torch.ones(2, **i32), torch.ones(2, **i32)
    prm, pl = torch.zeros(2, 3, dtype=torch.long, device=dev()), torch.ones(2, **i32)
    with pytest.raises(I2TError, match='max_new 0'):
        ops.caption_finish_ragged(ids, 8, cnt[1:2], prm, pl, 2, 0, 3, 0, fin, ln, lp, ctrl, 4)
    with pytest.raises(AssertionError):
        ops.caption_finish_ragged(ids, 8, cnt[1:2], prm, pl, 3, 2, 3, 0, fin, ln, lp, ctrl, 4)          # 4 rows in groups of 3


# ---------------------------------------------------------------------------------------------------------------- end to end
def _tiny(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(tiny_config())
    m.load_state_dict(tiny_weights)
    return m.to(dev()).eval()


def _inputs(V):
    images, labels = synthetic_batch(4, 32, 12, min(V, 384), seed=11)
    return images.to(dev()), labels[:, :P].clamp(min=0).to(dev())


@pytest.fixture(params=['tiny', 'hf_gpt2_soft'])
def model(request, tiny_weights, tmp_path, monkeypatch):
    """-> (name, model, images [4, ...], prompt [4, 5]): the dense decoder with a soft prompt and a Hugging Face GPT-2 with a prefix"""
    if request.param == 'tiny':
        m = _tiny(tiny_weights)
        assert m.config.use_soft_prompting and m._engine.dec.causal
    else:
        from test_hf_decoder_gpu import _build
        _, m = _build(tmp_path, monkeypatch, True, True)
        m = m.to(dev()).eval()
        assert m._engine.dec.prefixed
    return (request.param, m) + _inputs(m._engine.dec.V)


def by_column(out, pad):
    """-> (ids [R, Pmax + T] padded with `pad`, lengths [R], token_logprobs by COLUMN [R, Pmax + T], 0.0 where none was recorded)"""
    B, N, L = out.ids.shape
    plen = out.prompt_lengths
    first = L - out.token_logprobs.shape[-1]                      # the column of entry 0: Pmin, or P on the equal-length path
    assert first == (int(plen.min()) if plen is not None else first)
    ids = torch.full((B * N, P + T), pad, dtype=torch.long, device=dev())
    ids[:, :L] = out.ids.reshape(B * N, L)
    lp = torch.zeros(B * N, P + T, device=dev())
    lp[:, first:L] = out.token_logprobs.reshape(B * N, L - first)
    return ids, out.lengths.reshape(-1), lp


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def check_against_equal_length_runs(m, images, prompt, out, pad, **kw):
    """every row of `out` against the equal-length call with its prompt length, bit for bit; -> the rows compared"""
    N = out.ids.shape[1]
    got = by_column(out, pad)
    rows = torch.tensor(PLEN, device=dev()).repeat_interleave(N)
    seen = 0
    for p in sorted(set(PLEN)):
        ref = m.generate_captions(images, prompt[:, :p].contiguous(), max_new_tokens=T, **kw)
        assert ref.prompt_lengths is None and ref.token_logprobs.shape[-1] == ref.ids.shape[-1] - p
        sel = rows == p
        want = by_column(ref, pad)
        for name, g, w in zip(('ids', 'lengths', 'token_logprobs'), got, want):
            assert torch.equal(bits(g[sel]), bits(w[sel])), f'{name} of the rows with a prompt of {p} differ from the equal-length call'
        seen += int(sel.sum())
    assert seen == rows.numel()
    return seen


def check_shapes(out, N):
    B, L = len(PLEN), out.ids.shape[-1]
    plen = torch.tensor(PLEN, dtype=torch.int32, device=dev())
    assert tuple(out.ids.shape) == (B, N, L) and out.ids.dtype == torch.long
    assert tuple(out.lengths.shape) == (B, N) and out.lengths.dtype == torch.int32 and int(out.lengths.max()) == L
    assert tuple(out.token_logprobs.shape) == (B, N, L - min(PLEN)) and out.token_logprobs.dtype == F32
    assert torch.equal(out.logprob, out.token_logprobs.sum(dim=-1))
    assert out.prompt_lengths.dtype == torch.int32 and torch.equal(out.prompt_lengths, plen)
    assert bool((out.lengths > plen[:, None]).all()) and bool((out.lengths <= plen[:, None] + T).all())
    col = torch.arange(L, device=dev())
    live = (col >= plen[:, None, None]) & (col < out.lengths[..., None])             # [B, N, L]: the emitted tokens
    lp = torch.zeros(B, N, L, device=dev())
    lp[..., min(PLEN):] = out.token_logprobs
    assert bool((lp[~live] == 0).all()) and torch.isfinite(lp).all() and bool((lp[live] <= 0).all()) and bool((lp[live] < 0).any())


@pytest.mark.parametrize('mode', [GREEDY, SAMPLING], ids=['greedy', 'sampling_n2'])
def test_rows_equal_the_equal_length_calls(model, mode):
    """B = 4, lengths (1, 3, 5, 3) in 5 columns, 8 new tokens, without an EOS id and with one the run emits: each row is bit-equal to
    the equal-length call on prompt_ids[:, :p]; what the ignored columns hold changes nothing; without the graph the same"""
    name, m, images, prompt = model
    N = mode.get('num_return_sequences', 1)
    V = m._engine.dec.V
    free = m.generate_captions(images, prompt, max_new_tokens=T, prompt_lengths=PLEN, **mode)
    check_shapes(free, N)
    assert bool((free.lengths == torch.tensor(PLEN, device=dev())[:, None] + T).all()) and free.ids.shape[-1] == P + T
    for b, p in enumerate(PLEN):
        assert bool((free.ids[b, :, :p] == prompt[b, :p]).all())
    check_against_equal_length_runs(m, images, prompt, free, 0, **mode)
    # the third token row (0, 0) emits as the EOS id: that row ends by its third step, the others where they emit it, or on their budget
    eos = int(free.ids[0, 0, PLEN[0] + 2])
    pad = (eos + 1) % V
    kw = dict(eos_token_id=eos, pad_token_id=pad, **mode)
    out = m.generate_captions(images, prompt, max_new_tokens=T, prompt_lengths=torch.tensor(PLEN), **kw)
    check_shapes(out, N)
    assert bool((out.lengths < torch.tensor(PLEN, device=dev())[:, None] + T).any()), 'no row ended on the EOS id'
    print(f'{name}: eos {eos}, lengths {out.lengths.reshape(-1).tolist()} for prompts {PLEN} x {N}')
    check_against_equal_length_runs(m, images, prompt, out, pad, **kw)
    # the host rule on the free run's rows gives the same table
    R = len(PLEN) * N
    w_ids, w_len, w_lp = apply_finish_rule_ragged(free.ids.reshape(R, -1).cpu().numpy(), np.repeat(PLEN, N), T, eos, pad,
                                                  free.token_logprobs.reshape(R, -1).cpu().numpy())
    assert np.array_equal(out.ids.reshape(R, -1).cpu().numpy(), w_ids) and np.array_equal(out.lengths.reshape(-1).cpu().numpy(), w_len)
    assert np.array_equal(out.token_logprobs.reshape(R, -1).cpu().numpy(), w_lp)
    # columns at or past p_b: two kinds of garbage, one of them the EOS id
    ignored = torch.arange(P, device=dev())[None, :] >= torch.tensor(PLEN, device=dev())[:, None]
    for junk in (eos, V - 1):
        again = m.generate_captions(images, torch.where(ignored, junk, prompt), max_new_tokens=T, prompt_lengths=list(PLEN), **kw)
        assert same(again, out) and torch.equal(again.prompt_lengths, out.prompt_lengths), f'ignored columns filled with {junk} changed the result'
    # step by step without the captured graph
    sampling = None if mode is GREEDY else Sampling(mode['temperature'], mode['top_k'], mode['nucleus_p'], mode['seed'])
    eager = m._captioner.generate_captions(images, prompt, T, eos, pad, N, sampling, use_graph=False, prompt_lengths=PLEN)
    assert same(eager, out), 'use_graph=False differs from the captured step'


def test_graph_keys_keep_ragged_and_equal_length_calls_apart(tiny_weights):
    """a ragged call, an equal-length call and a ragged call again on one model; the reverse order on a second: every call reproduces
    what it gives as the first call of a fresh model (same EOS id, pad id and mode on both paths: only the key's 'ragged' differs)"""
    images, prompt = _inputs(384)
    kw = dict(max_new_tokens=T, eos_token_id=5, pad_token_id=2, **GREEDY)
    ragged = lambda m: m.generate_captions(images, prompt, prompt_lengths=PLEN, **kw)
    equal = lambda m: m.generate_captions(images, prompt, **kw)
    a, b = _tiny(tiny_weights), _tiny(tiny_weights)
    a_r1, a_e, a_r2 = ragged(a), equal(a), ragged(a)
    b_e1, b_r, b_e2 = equal(b), ragged(b), equal(b)
    assert same(a_r2, a_r1) and same(b_r, a_r1), 'a ragged call is disturbed by an equal-length call before it'
    assert same(b_e2, b_e1) and same(a_e, b_e1), 'an equal-length call is disturbed by a ragged call before it'
    keys = [k for k in a._captioner._state.graphs if k is not None]
    assert len(keys) == 2 and sum(k[0] == 'ragged' for k in keys) == 1
    # another budget is another captured step (max_new_tokens is a kernel argument)
    short = a.generate_captions(images, prompt, prompt_lengths=PLEN, **dict(kw, max_new_tokens=3))
    assert len(a._captioner._state.graphs) == 4 and int(short.lengths.max()) <= P + 3
    assert same(ragged(a), a_r1)


def test_none_is_the_old_path_and_equal_lengths_agree_with_it(tiny_weights):
    m = _tiny(tiny_weights)
    images, prompt = _inputs(384)
    kw = dict(max_new_tokens=T, eos_token_id=5, **GREEDY)
    old = m.generate_captions(images, prompt, **kw)
    none = m.generate_captions(images, prompt, prompt_lengths=None, **kw)
    assert type(none)._fields == ('ids', 'lengths', 'token_logprobs', 'logprob') and len(none) == 4
    assert none.prompt_lengths is None and old.prompt_lengths is None and same(none, old)
    assert all(k is None or k[0] != 'ragged' for k in m._captioner._state.graphs)
    ids, lengths, lp, total = none                                # unpacks as it did
    full = m.generate_captions(images, prompt, prompt_lengths=[P] * 4, **kw)          # every length P: the same rows through the new kernel
    assert same(full, old) and full.prompt_lengths.tolist() == [P] * 4
    # nothing to emit: the prompts, padded
    zero = m.generate_captions(images, prompt, max_new_tokens=0, pad_token_id=9, prompt_lengths=PLEN, **GREEDY)
    assert tuple(zero.ids.shape) == (4, 1, P) and zero.lengths[:, 0].tolist() == list(PLEN) and tuple(zero.token_logprobs.shape) == (4, 1, P - 1)
    for b, p in enumerate(PLEN):
        assert torch.equal(zero.ids[b, 0, :p], prompt[b, :p]) and bool((zero.ids[b, 0, p:] == 9).all())
    window = m.decoder.block_size - m.space_for_prompt
    with pytest.raises(ValueError, match='text window'):
        m.generate_captions(images, prompt, max_new_tokens=window - P + 1, prompt_lengths=PLEN, **GREEDY)


def test_the_loop_stops_once_every_row_has_ended(tiny_weights):
    """one image four times, the prompts prefixes of ITS greedy caption: every row continues that caption, so an EOS id taken from it
    ends all rows at one column, and with poll_every = 1 the host launches no step past it"""
    m = _tiny(tiny_weights)
    images, prompt = _inputs(384)
    images = images[:1].expand(4, -1, -1, -1).contiguous()
    s = m.generate_captions(images, prompt[:1, :1].expand(4, 1).contiguous(), max_new_tokens=P - 1 + T, **GREEDY).ids[0, 0]
    prompts = s[:P].expand(4, P).contiguous()
    free = m.generate_captions(images, prompts, max_new_tokens=T, prompt_lengths=PLEN, **GREEDY)
    for b, p in enumerate(PLEN):
        assert torch.equal(free.ids[b, 0, :p + T], s[:p + T]), 'a forced row does not continue the caption it is a prefix of'
    sl = s.tolist()
    fresh = [c for c in range(P, min(PLEN) + T) if sl[c] not in sl[1:c]]          # columns EVERY row emits, holding a token not seen before
    assert fresh, f'the caption {sl} has no first occurrence in columns {P} .. {min(PLEN) + T - 1}'
    c = fresh[0]
    n_full = max(PLEN) - min(PLEN) + T
    for poll, most in ((1, c), (4, c + 3), (0, n_full)):
        out = m.generate_captions(images, prompts, max_new_tokens=T, eos_token_id=sl[c], poll_every=poll, prompt_lengths=PLEN, **GREEDY)
        assert bool((out.lengths == c + 1).all()) and out.ids.shape[-1] == c + 1 and bool((out.ids[:, 0] == s[:c + 1]).all())
        replays = m._captioner.last_replays
        assert (replays == n_full) if poll == 0 else (c + 1 - min(PLEN) <= replays <= most), (poll, replays)
    assert c + 1 - min(PLEN) < n_full


def test_non_causal_decoder_recomputes_once_per_length():
    """no cache to share: ids and lengths are those of the equal-length fallback on the rows of each length (the same launches), the
    log-probs are score()'s on the returned table at the emitted columns -- conditioned, as that fallback's are, on the whole row --
    and exactly 0.0 elsewhere"""
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(reference_unit_test_config())
    det_init_(m, seed=0)
    sharpen_gates_(m)
    m = m.to(dev()).eval()
    assert not m._engine.dec.causal
    images, labels = synthetic_batch(3, 128, 12, 1024, seed=9)
    images, prompt = images.to(dev()), labels[:, :3].clamp(min=0).to(dev())
    plen, Tn, PADID = (1, 3, 1), 4, 1023
    free = m.generate_captions(images, prompt, max_new_tokens=Tn, prompt_lengths=plen, **GREEDY)
    assert free.lengths[:, 0].tolist() == [p + Tn for p in plen] and tuple(free.token_logprobs.shape) == (3, 1, 3 + Tn - 1)
    eos = int(free.ids[0, 0, 2])                                  # row 0 ends at its second token
    kw = dict(max_new_tokens=Tn, eos_token_id=eos, pad_token_id=PADID, **GREEDY)
    out = m.generate_captions(images, prompt, prompt_lengths=plen, **kw)
    assert m._captioner is None and out.prompt_lengths.tolist() == list(plen) and int(out.lengths[0, 0]) <= 3
    L = out.ids.shape[-1]
    assert int(out.lengths.max()) == L and tuple(out.token_logprobs.shape) == (3, 1, L - 1)
    for p in sorted(set(plen)):
        sel = torch.tensor([q == p for q in plen], device=dev())
        ref = m.generate_captions(images[sel], prompt[sel, :p].contiguous(), **kw)
        assert torch.equal(out.lengths[sel], ref.lengths), f'lengths of the rows with a prompt of {p}'
        Lp = ref.ids.shape[-1]
        assert torch.equal(out.ids[sel][..., :Lp], ref.ids) and bool((out.ids[sel][..., Lp:] == PADID).all()), f'ids of the rows with a prompt of {p}'
    sc = m.score(images, out.ids[:, 0]).token_logprobs            # [3, L]: entry c is the log-prob of the token at column c + 1
    col = torch.arange(1, L, device=dev())[None, :]
    live = (col >= torch.tensor(plen, device=dev())[:, None]) & (col < out.lengths)
    got = out.token_logprobs[:, 0]
    assert torch.equal(bits(got[live]), bits(sc[:, :L - 1][live])) and bool((got[~live] == 0).all()) and bool((got[live] < 0).all())
    assert torch.equal(out.logprob, out.token_logprobs.sum(dim=-1))
