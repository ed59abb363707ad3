"""generate_captions(num_beams=W) on the MI355X: i2t_beam_pool_select against its numpy replica, and whole searches
against ``beam_search_host`` run over the model's own forward.

The decode step and the forward differ by their bf16 GEMM and attention shapes, so a search is compared the way the existing beam
tests compare (tests/test_beam_cache_gpu.py): the largest difference between the step's logits and the forward's logits on the same
rows is MEASURED in the test; an image whose replica never decided on a gap below that difference must give equal ids and lengths,
and log-probs and beam scores within that difference times the number of steps; at most one third of the images may fall outside."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import BEAM_DEAD, beam_advance_host, beam_pool_select_host, beam_search_host
from image2text_amd.synth import det_init_, mini_config, sharpen_gates_, synthetic_batch, tiny_config

pytestmark = pytest.mark.gpu

F32 = torch.float32


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


# ------------------------------------------------------------------------------------------------------ the kernel against its replica
FLOATS = ('scores', 'tok_lp', 'pool_lp', 'pool_score', 'pool_sum')
INTS = ('ids', 'hist', 'pool_ids', 'pool_len', 'pool_n', 'closed', 'counters', 'ctrl')


def _random_state(B, W, P, max_new, ids_ld, hist_ld, eos, pad, seed):
    g = np.random.default_rng(seed)
    R = B * W
    s = dict(scores=-g.random(R, dtype=np.float32) * 3, ids=g.integers(0, 50, (R, ids_ld)), hist=g.integers(0, R, (R, hist_ld), dtype=np.int32),
             tok_lp=-g.random((R, ids_ld), dtype=np.float32), pool_ids=np.full((B, W, ids_ld), pad, dtype=np.int64),
             pool_lp=np.zeros((B, W, ids_ld), dtype=np.float32), pool_score=np.full((B, W), BEAM_DEAD, dtype=np.float32),
             pool_sum=np.zeros((B, W), dtype=np.float32), pool_len=np.zeros((B, W), dtype=np.int32), pool_n=np.zeros(B, dtype=np.int32),
             closed=np.zeros(B, dtype=np.int32), counters=np.array([P + 2, P], dtype=np.int32), ctrl=np.zeros(2, dtype=np.int32))
    s['ids'] = s['ids'].astype(np.int64)
    s['tok_lp'][:, :P] = 0
    for b in range(B):                                        # a partly filled pool: b % W entries, sorted, with rows of their own
        n = b % W if B > 1 else 1
        s['pool_n'][b] = n
        s['pool_score'][b, :n] = -np.sort(g.random(n, dtype=np.float32)) * 2 - 0.2
        s['pool_sum'][b, :n] = s['pool_score'][b, :n] * 2
        s['pool_len'][b, :n] = P + 1
        s['pool_ids'][b, :n, :P + 1] = g.integers(0, 50, (n, P + 1))
        s['pool_lp'][b, :n, P] = -g.random(n, dtype=np.float32)
    return s, g


def _candidates(g, R, W, eos):
    E = 2 * W
    tok = np.stack([g.permutation(np.setdiff1d(np.arange(50), [eos]))[:E] for _ in range(R)]).astype(np.int32)
    lp = -np.sort(g.random((R, E), dtype=np.float32) * 4, axis=1)
    for r in range(R):                                        # an EOS among most rows' candidates, early or late in the row
        if g.random() < 0.75:
            tok[r, g.integers(0, E)] = eos
    tok[0, 0] = eos                                           # and one that leads its row
    return tok, lp


def _to_dev(s):
    return {k: torch.from_numpy(v.copy()).to(dev()) for k, v in s.items()}


def _call(ops, d, tok, lp, B, W, P, max_new, eos, pad, penalty, early):
    ops.beam_pool_select(torch.from_numpy(tok).to(dev()), torch.from_numpy(lp).to(dev()), d['scores'], d['ids'], d['hist'], d['tok_lp'],
                         d['pool_ids'], d['pool_lp'], d['pool_score'], d['pool_sum'], d['pool_len'], d['pool_n'], d['closed'],
                         d['counters'][0:1], d['counters'][1:2], d['ctrl'], B, W, P, max_new, eos, pad, penalty, early)


def _same(d, s, tag):
    for k in INTS:
        assert np.array_equal(d[k].cpu().numpy(), s[k]), f'{tag}: {k}'
    for k in FLOATS:
        got, want = d[k].cpu().numpy().astype(np.float64), s[k].astype(np.float64)
        assert bool((np.abs(got - want) <= 2 * np.spacing(np.abs(s[k]).astype(np.float32))).all()), f'{tag}: {k}'


@pytest.mark.parametrize('B,W', [(1, 2), (3, 4), (2, 8)])
@pytest.mark.parametrize('max_new,penalty,early', [(6, 1.0, False), (3, 2.0, False), (6, 0.0, True), (6, 0.7, True)])
def test_pool_select_against_the_replica(ops, B, W, max_new, penalty, early):
    """three consecutive calls with i2t_beam_advance between them, on random candidates with EOS seeded at ranks below and above W and a
    partly filled pool; ids_ld = 37 and hist_ld = 41 are no multiple of anything; max_new = 3 puts the third call at the bound"""
    P, eos, pad, ids_ld, hist_ld = 2, 7, 49, 37, 41
    s, g = _random_state(B, W, P, max_new, ids_ld, hist_ld, eos, pad, seed=B * 100 + W)
    d = _to_dev(s)
    entered = 0
    for call in range(3):
        tok, lp = _candidates(g, B * W, W, eos)
        before = s['pool_n'].sum()
        beam_pool_select_host(tok, lp, s['scores'], s['ids'], s['hist'], s['tok_lp'], s['pool_ids'], s['pool_lp'], s['pool_score'], s['pool_sum'],
                              s['pool_len'], s['pool_n'], s['closed'], s['counters'], s['ctrl'], W, P, max_new, eos, pad, penalty, early)
        entered += int(s['pool_n'].sum() - before)
        _call(ops, d, tok, lp, B, W, P, max_new, eos, pad, penalty, early)
        _same(d, s, f'call {call} select')
        beam_advance_host(s['counters'], s['ctrl'])
        ops.beam_advance(d['counters'], d['ctrl'])
        _same(d, s, f'call {call} advance')
    assert entered > 0, 'the case never filled a pool slot'
    # with ctrl[0] set nothing changes
    d['ctrl'][0] = 1
    d['closed'].zero_()
    d['counters'].copy_(torch.tensor([P + 2, P], dtype=torch.int32))
    keep = {k: v.clone() for k, v in d.items()}
    tok, lp = _candidates(g, B * W, W, eos)
    _call(ops, d, tok, lp, B, W, P, max_new, eos, pad, penalty, early)
    assert all(torch.equal(d[k], keep[k]) for k in d)


def test_pool_select_refusals(ops):
    from image2text_amd import lib as i2tlib
    s, g = _random_state(1, 2, 2, 4, 8, 8, 7, 9, seed=1)
    d = _to_dev(s)
    tok, lp = _candidates(g, 2, 2, 7)
    with pytest.raises(i2tlib.I2TError, match='ids_ld'):
        _call(ops, d, tok, lp, 1, 2, 2, 7, 7, 9, 1.0, False)          # P + max_new = 9 columns in rows of 8
    with pytest.raises(i2tlib.I2TError, match='length_penalty'):
        _call(ops, d, tok, lp, 1, 2, 2, 4, 7, 9, float('nan'), False)
    rc = i2tlib.load().i2t_beam_pool_select(None, *([d['ctrl'].data_ptr()] * 4), 8, d['ctrl'].data_ptr(), 8, d['ctrl'].data_ptr(), 8,
                                            *([d['ctrl'].data_ptr()] * 10), 1, 9, 2, 4, 7, 9, 1.0, 0)
    assert rc == -1 and 'beam width' in i2tlib.last_error()


# ------------------------------------------------------------------------------------------------------ whole searches
def _ved(cfg, weights=None, sharpen=False):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(cfg)
    if weights is not None:
        m.load_state_dict(weights)
    else:
        det_init_(m, seed=0)
        if sharpen:
            sharpen_gates_(m)
    return m.to(dev()).eval()


class Case:
    """a model, B = 3 images with prompts, an EOS id the free search emits, the forward as ``step_logits`` (cached per image and
    sequence, shared by every test of the model) and the measured step-vs-forward logit difference"""

    def __init__(self, m, images, prompt, T=8):
        self.m, self.images, self.prompt, self.T = m, images, prompt, T
        self.B, self.P = prompt.shape
        self.V = m._engine.dec.V
        self.ngrams = tuple(int(n) for n in m.config.no_repeat_n_grams)
        self.cache = {}
        free = m.generate_captions(images, prompt, max_new_tokens=T, num_beams=2)
        self.eos = int(free.ids[0, 0, self.P + 2])             # image 0's best caption holds it as its third token
        self.pad = self.V - 1
        self.diff = self._measure()

    def step_logits(self, b):
        def f(seq):
            key = (b, tuple(seq))
            if key not in self.cache:
                with torch.no_grad():
                    z = self.m(images=self.images[b:b + 1], ids=torch.tensor([list(seq)], device=dev())).logits[0, -1].float()
                self.cache[key] = z.cpu().numpy()[:self.V].copy()
            return self.cache[key]
        return f

    def _measure(self):
        """the largest |step logit - forward logit| over every row and step of one W = 2 search without an EOS: each(i) runs after
        step i, so the rows that produced step i's logits are the ids left by step i - 1"""
        dec, W = self.m._beam_captioner, 2
        rows, worst = [self.prompt.repeat_interleave(W, dim=0)], [0.0]
        imgs = self.images.repeat_interleave(W, dim=0)

        def each(i):
            st = dec._state
            with torch.no_grad():
                fwd = self.m(images=imgs, ids=rows[0]).logits[:, -1].float()[:, :self.V]
            worst[0] = max(worst[0], float((st.logits[:, :self.V] - fwd).abs().max()))
            rows[0] = st.ids[:, :self.P + i + 1].clone()
        dec.generate_captions(self.images, self.prompt, self.T, W, None, self.pad, 1, 1.0, False, poll_every=0, use_graph=False, each=each)
        print(f'measured step-vs-forward logit difference: {worst[0]:.3g}')
        assert 0 < worst[0] < 0.5
        return worst[0]

    def check(self, W, N, penalty, early, eos='own', **kw):
        eos = self.eos if eos == 'own' else eos
        out = self.m.generate_captions(self.images, self.prompt, max_new_tokens=self.T, eos_token_id=eos, pad_token_id=self.pad,
                                       num_return_sequences=N, num_beams=W, length_penalty=penalty, early_stopping=early, **kw)
        B, P, T = self.B, self.P, self.T
        L = out.ids.shape[-1]
        assert tuple(out.ids.shape) == (B, N, L) and tuple(out.lengths.shape) == (B, N) and int(out.lengths.max()) == L
        assert tuple(out.token_logprobs.shape) == (B, N, L - P) and tuple(out.beam_scores.shape) == (B, N) and out.beam_scores.dtype == F32
        assert out.prompt_lengths is None and torch.equal(out.logprob, out.token_logprobs.sum(dim=-1))
        assert bool((out.beam_scores[:, :-1] >= out.beam_scores[:, 1:]).all()), 'best first'
        ids, lens, lps = out.ids.cpu().numpy(), out.lengths.cpu().numpy(), out.token_logprobs.cpu().numpy()
        for b in range(B):                                    # lengths, padding and zeros past the end: exact
            for n in range(N):
                ln = int(lens[b, n])
                assert (ids[b, n, :P] == self.prompt[b].cpu().numpy()).all() and (ids[b, n, ln:] == self.pad).all() and (lps[b, n, ln - P:] == 0).all()
                assert ln == P + T or (eos is not None and ids[b, n, ln - 1] == eos and not (ids[b, n, P:ln - 1] == eos).any())
                assert (lps[b, n, :ln - P] <= 0).all() and np.isfinite(lps[b, n]).all()
        outside = 0
        for b in range(B):
            want = beam_search_host(self.step_logits(b), self.prompt[b].tolist(), W, N, T, eos, self.pad, penalty, early, self.ngrams)
            margin = min(want.decision_gaps + want.pool_gaps)       # every gap between a chosen and the next total, at every selection
            if not margin > self.diff:
                outside += 1
                continue
            Lb = want.ids.shape[1]
            assert np.array_equal(lens[b], want.lengths) and np.array_equal(ids[b, :, :Lb], want.ids) and (ids[b, :, Lb:] == self.pad).all(), b
            tol = self.diff * T
            assert np.abs(lps[b, :, :Lb - P] - want.token_logprobs).max() <= tol
            assert np.abs(out.beam_scores[b].cpu().numpy() - want.beam_scores).max() <= tol
        print(f'W={W} N={N} penalty={penalty} early={early}: {outside} of {B} images decide inside the measured difference {self.diff:.3g}')
        assert outside * 3 <= B, f'{outside} of {B} images fall outside the margin rule'
        return out


@pytest.fixture(scope='module')
def tiny(tiny_weights):
    m = _ved(tiny_config(), tiny_weights)
    images, labels = synthetic_batch(3, 32, 12, 384, seed=11)
    return Case(m, images.to(dev()), labels[:, :2].clamp(min=0).to(dev()))


@pytest.mark.parametrize('early', [False, True])
@pytest.mark.parametrize('penalty', [0.0, 1.0])
@pytest.mark.parametrize('W,N', [(2, 1), (2, 2), (4, 1), (4, 4)])
def test_search_against_the_replica(tiny, W, N, penalty, early):
    tiny.check(W, N, penalty, early)


def test_sparse_nano_mini_family():
    m = _ved(mini_config(), sharpen=True)
    assert m._engine.dec.fam is not None and m._engine.dec.fam.sparse
    # the deterministic initialisation leaves this family's next-token distribution nearly flat, so most searches decide somewhere on a
    # gap below the step-vs-forward difference (about 5e-3); input seed 2 is one whose replica margins, computed from the forward
    # alone, clear it for two of the three images
    images, labels = synthetic_batch(3, 32, 12, 384, seed=2)
    case = Case(m, images.to(dev()), labels[:, :2].clamp(min=0).to(dev()))
    case.check(3, 2, 0.0, True)


def test_llama_family(tmp_path, monkeypatch):
    from test_hf_decoder_gpu import _llama_model
    cfg, m, _, V = _llama_model(tmp_path, monkeypatch, 'llama')
    m = m.to(dev()).eval()
    # a randomly initialised decoder: nearly flat next-token distributions, so the input seed is one whose replica margins, computed
    # from the forward alone, clear the step-vs-forward difference (about 6e-3) for two of the three images
    g = torch.Generator().manual_seed(1)
    images = torch.randn(3, 3, 32, 32, generator=g).to(dev())
    prompt = torch.randint(0, V, (3, 2), generator=g).to(dev())
    case = Case(m, images, prompt)
    case.check(3, 2, 0.0, True)


def test_one_beam_is_the_call_without_the_arguments(tiny):
    m, kw = tiny.m, dict(max_new_tokens=8, eos_token_id=tiny.eos, pad_token_id=tiny.pad)
    for mode in (dict(top_k=1), dict(temperature=0.7, nucleus_p=0.6, seed=12, num_return_sequences=2)):
        want = m.generate_captions(tiny.images, tiny.prompt, **kw, **mode)
        got = m.generate_captions(tiny.images, tiny.prompt, **kw, **mode, num_beams=1, length_penalty=2.0, early_stopping=True)
        assert got.beam_scores is None and want.beam_scores is None and got.prompt_lengths is None
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match='num_beams'):
        m.generate_captions(tiny.images, tiny.prompt, num_beams=9, **kw)
    with pytest.raises(NotImplementedError, match='prompt_lengths'):
        m.generate_captions(tiny.images, tiny.prompt, num_beams=2, prompt_lengths=[1, 2, 2], **kw)


def test_graph_eager_and_polling_agree(tiny):
    dec = tiny.m._beam_captioner
    args = (tiny.images, tiny.prompt, 8, 4, tiny.eos, tiny.pad, 4, 1.0, True)
    want = dec.generate_captions(*args, poll_every=8)
    for kw in (dict(poll_every=0), dict(poll_every=1), dict(poll_every=8, use_graph=False), dict(poll_every=0, use_graph=False)):
        got = dec.generate_captions(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.equal(got.beam_scores, want.beam_scores), kw
        if kw.get('poll_every') == 0:
            assert dec.last_replays == 8
