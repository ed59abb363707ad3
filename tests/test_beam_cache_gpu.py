"""Beam search on the static KV cache (csrc/beam.hip, decoding.BeamDecoder, BeamSearchTokenGenerator(kv_cache=True)).

Kernels against plain torch statements of the same step on the same inputs (real vocabularies and head shapes), the device draws
against their distribution and the host replica of their uniforms, then whole searches: the reference's recorded runs
(tests/golden/tiny_beam.npz), beam = greedy at W = E = 1, and the self-consistency of a nano-224-shaped search."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from image2text_amd.synth import det_init_, nano224_config, tiny_config
from test_oracle_golden import BEAM_RUNS

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def dev():
    return torch.device('cuda:0')


def rnd(*shape, scale=1.0, seed=0, dtype=F32):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev()) * scale).to(dtype)


def i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=dev())


def ref_attn_rows(q, k, v, scale, G=1):
    """q (R, H, hd), k / v (R, n, Hkv, hd) -> fp64 (R, H, hd)"""
    q, k, v = q.double(), k.double().repeat_interleave(G, dim=2), v.double().repeat_interleave(G, dim=2)
    s = torch.einsum('bhe,bnhe->bhn', q, k) * scale
    return torch.einsum('bhn,bnhe->bhe', torch.softmax(s, -1), v)


def close(name, got, ref, atol=1e-4, rtol=1 / 200):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    assert bool((err <= atol + rtol * ref.abs()).all()), f'{name}: max abs err {err.max().item():.3g}'


# ------------------------------------------------------------------------------------------------------ attention through the history
@pytest.mark.parametrize('H', [12, 3])
def test_beam_decode_attention(ops, H):
    """Dense head-major cache [R][H][T][64]: identity table bit-equal to decode_attention, random tables against fp64, cross mode."""
    R, T, d = 6, 1024, 64 * H
    kt, vt = rnd(R, H, T, 64, dtype=BF16, seed=1), rnd(R, H, T, 64, dtype=BF16, seed=2)
    ident = torch.arange(R, dtype=torch.int32, device=dev()).unsqueeze(1).expand(R, T).contiguous()
    g = torch.Generator(device=dev()).manual_seed(3)
    for n in (1, 33, 200, 1024):
        qkv = rnd(R, 3 * d, dtype=BF16, seed=n)
        pos = i32([n - 1])
        o0, o1 = torch.empty(R, d, dtype=BF16, device=dev()), torch.empty(R, d, dtype=BF16, device=dev())
        k0, v0, k1, v1 = kt.clone(), vt.clone(), kt.clone(), vt.clone()
        ops.decode_attention(qkv, 3 * d, k0, v0, T * d, 64, o0, d, pos, 0, R, H, append_dm=d, cache_hs=T * 64)
        ops.beam_decode_attention(qkv, 3 * d, k1, v1, T * d, 64, o1, d, pos, 0, R, H, hist=ident, append_dm=d, cache_hs=T * 64)
        assert torch.equal(o0, o1) and torch.equal(k0, k1) and torch.equal(v0, v1), f'identity table n={n}'
        hist = torch.randint(0, R, (R, T), generator=g, device=dev(), dtype=torch.int32)
        k2, v2 = kt.clone(), vt.clone()
        ops.beam_decode_attention(qkv, 3 * d, k2, v2, T * d, 64, o1, d, pos, 0, R, H, hist=hist, append_dm=d, cache_hs=T * 64)
        kn, vn = qkv[:, d:2 * d].view(R, H, 64), qkv[:, 2 * d:].view(R, H, 64)
        assert torch.equal(k2[:, :, n - 1], kn) and torch.equal(v2[:, :, n - 1], vn), 'the new key goes to the row itself'
        rows = hist[:, :n - 1].long()
        ar = torch.arange(n - 1, device=dev())
        kk = torch.cat([kt.permute(0, 2, 1, 3)[rows, ar], kn.unsqueeze(1)], 1)    # (R, n, H, 64)
        vv = torch.cat([vt.permute(0, 2, 1, 3)[rows, ar], vn.unsqueeze(1)], 1)
        close(f'hist n={n}', o1.view(R, H, 64), ref_attn_rows(qkv[:, :d].view(R, H, 64), kk, vv, 0.125))
    # cross: beam row r reads memory row r // W of a token-major [B][S][2d] K|V memory
    W, S = 3, 197
    B = R // W
    kv = rnd(B, S, 2 * d, dtype=BF16, seed=7)
    q = rnd(R, d, dtype=BF16, seed=8)
    o0, o1 = torch.empty(R, d, dtype=BF16, device=dev()), torch.empty(R, d, dtype=BF16, device=dev())
    kvx = kv.repeat_interleave(W, 0).contiguous()
    ops.decode_attention(q, d, kvx, kvx.view(-1)[d:], S * 2 * d, 2 * d, o0, d, None, S, R, H)
    ops.beam_decode_attention(q, d, kv, kv.view(-1)[d:], S * 2 * d, 2 * d, o1, d, None, S, R, H, rows_per_mem=W)
    assert torch.equal(o0, o1)


@pytest.mark.parametrize('H,Hkv,hd', [(32, 32, 128), (32, 8, 128), (12, 12, 64), (12, 1, 64)])
def test_beam_gq_decode_attention(ops, H, Hkv, hd):
    R, T = 4, 1024
    w, G, scale = Hkv * hd, H // Hkv, hd ** -0.5
    kt, vt = rnd(R, T, Hkv, hd, dtype=BF16, seed=1), rnd(R, T, Hkv, hd, dtype=BF16, seed=2)
    ident = torch.arange(R, dtype=torch.int32, device=dev()).unsqueeze(1).expand(R, T).contiguous()
    g = torch.Generator(device=dev()).manual_seed(4)
    for n in (1, 65, 1024):
        q = rnd(R, H * hd, dtype=BF16, seed=n, scale=2.0)
        kvn = rnd(R, 2 * w, dtype=BF16, seed=n + 1)
        pos = i32([n - 1])
        o0, o1 = torch.empty(R, H * hd, dtype=BF16, device=dev()), torch.empty(R, H * hd, dtype=BF16, device=dev())
        k0, v0, k1, v1 = kt.clone(), vt.clone(), kt.clone(), vt.clone()
        ops.gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k0, v0, T * w, w, o0, pos, 0, T, R, H, Hkv, hd)
        ops.beam_gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k1, v1, T * w, w, o1, pos, 0, T, R, H, Hkv, hd, hist=ident)
        assert torch.equal(o0, o1) and torch.equal(k0, k1) and torch.equal(v0, v1), f'identity table n={n}'
        hist = torch.randint(0, R, (R, T), generator=g, device=dev(), dtype=torch.int32)
        k2, v2 = kt.clone(), vt.clone()
        ops.beam_gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k2, v2, T * w, w, o1, pos, 0, T, R, H, Hkv, hd, hist=hist)
        rows, ar = hist[:, :n - 1].long(), torch.arange(n - 1, device=dev())
        kk = torch.cat([kt[rows, ar], kvn[:, :w].view(R, 1, Hkv, hd)], 1)
        vv = torch.cat([vt[rows, ar], kvn[:, w:].view(R, 1, Hkv, hd)], 1)
        close(f'gq hist n={n}', o1.view(R, H, hd), ref_attn_rows(q.view(R, H, hd), kk, vv, scale, G))
    W, S = 2, 64
    kv = rnd(R // W, S, 2 * w, dtype=BF16, seed=9)
    q = rnd(R, H * hd, dtype=BF16, seed=10)
    kvx = kv.repeat_interleave(W, 0).contiguous()
    o0, o1 = torch.empty(R, H * hd, dtype=BF16, device=dev()), torch.empty(R, H * hd, dtype=BF16, device=dev())
    ops.gq_decode_attention(q, None, None, kvx, kvx.view(-1)[w:], S * 2 * w, 2 * w, o0, None, S, S, R, H, Hkv, hd)
    ops.beam_gq_decode_attention(q, None, None, kv, kv.view(-1)[w:], S * 2 * w, 2 * w, o1, None, S, S, R, H, Hkv, hd, rows_per_mem=W)
    assert torch.equal(o0, o1)


# ------------------------------------------------------------------------------------------------------ candidates
def cand_buffers(R, E):
    return (torch.zeros(R, E, dtype=torch.int32, device=dev()), torch.zeros(R, E, dtype=F32, device=dev()),
            torch.zeros(R, E, dtype=torch.int32, device=dev()))


def seed_buf(seed):
    from image2text_amd.decoding import _set_seed
    s = torch.zeros(2, dtype=torch.int32, device=dev())
    _set_seed(s, seed)
    return s


@pytest.mark.parametrize('V,top_k', [(50257, None), (32000, 7), (151936, None), (151936, 50)])
def test_beam_candidates_deterministic(ops, V, top_k):
    import oracle.reference_model as orc
    R, E, L, eos, boost = 8, 4, 40, 11, math.log(1.5)
    Vp = (V + 7) // 8 * 8
    logits = rnd(R, Vp, scale=3.0, seed=V)
    logits[:, :64] += 6.0                                                   # the ids' alphabet leads: the ban decides the candidates
    g = torch.Generator().manual_seed(V)
    ids = torch.randint(0, 64, (R, L + 4), generator=g)                     # small alphabet: many repeated n-grams
    ids[:, L - 1] = torch.tensor([eos, 5, eos, 6, eos, 7, 8, eos])          # rows ending in EOS
    ids[2, :L - 1] = torch.arange(L - 1) % 3                                 # a heavily banned row
    ngrams = (2, 3)
    for eos_id in (None, eos):
        tok, lp, raw = cand_buffers(R, E)
        ops.beam_candidates(logits, ids.to(dev()), i32([L]), i32([0, 0]), i32(ngrams), R, V, E, 0.0, top_k, eos_id, boost if eos_id else 0.0,
                            seed_buf(1), tok, lp, raw)
        s = orc.apply_ngram_ban(ids[:, :L], logits[:, :V].double().cpu().clone(), ngrams)
        if top_k is not None:
            kth = torch.topk(s, top_k, dim=-1).values[:, -1:]
            s[s < kth] = -float('inf')
        logp = s.log_softmax(-1)
        nxt = s.topk(E, dim=-1).indices
        want_lp = logp.gather(-1, nxt)
        assert torch.equal(raw.cpu().long(), nxt), (raw.cpu(), nxt)
        if eos_id is not None:
            ended = ids[:, L - 1:L] == eos_id
            stay = ended & (want_lp + boost < 0)
            nxt = torch.where(stay, torch.full_like(nxt, eos_id), nxt)
            want_lp = torch.where(stay, torch.zeros_like(want_lp), want_lp + boost)
        assert torch.equal(tok.cpu().long(), nxt)
        close(f'lp V={V}', lp, want_lp, atol=1e-5, rtol=1e-5)


def test_beam_candidates_ties_and_gumbel_replica(ops):
    """Ties: lower id first.  Sampled draws: the top-E of score / T + Gumbel noise over rng.beam_uniform, exactly."""
    from image2text_amd import rng
    R, V, E, L = 4, 50257, 4, 9
    Vp = (V + 7) // 8 * 8
    logits = torch.zeros(R, Vp, device=dev())
    logits[:, [900, 17, 4000, 33]] = 5.0                                    # four tied leaders
    logits[:, 70] = 6.0
    ids = torch.full((R, L + 1), 1, dtype=torch.long, device=dev())
    tok, lp, raw = cand_buffers(R, E)
    ops.beam_candidates(logits, ids, i32([L]), i32([0, 0]), i32(()), R, V, E, 0.0, None, None, 0.0, seed_buf(1), tok, lp, raw)
    assert tok.cpu().tolist() == [[70, 17, 33, 900]] * R
    T, seed = 1.7, 0x1234567890ABCDEF
    logits = rnd(R, Vp, scale=2.0, seed=5)
    ops.beam_candidates(logits, ids, i32([L]), i32([0, 0]), i32(()), R, V, E, T, None, None, 0.0, seed_buf(seed), tok, lp, raw)
    y = logits[:, :V].double().cpu() / T
    for r in range(R):
        u = rng.beam_uniform(seed, L, r, torch.arange(V), 0)
        key = y[r] - torch.log(-torch.log(u))
        assert tok[r].cpu().long().tolist() == key.topk(E).indices.tolist(), r
    close('sampled lp', lp, y.log_softmax(-1).gather(-1, tok.cpu().long()), atol=1e-5, rtol=1e-5)


def test_beam_draw_distributions(ops):
    """Ordered pairs of draws without replacement: P(i, j) = p_i p_j / (1 - p_i), within 5 sigma, for the candidate draws and for
    the consolidation draws."""
    V, E, R = 6, 2, 8192
    x = torch.tensor([1.0, 0.3, -0.5, 0.8, -2.0, 0.0], dtype=torch.float64)
    T = 0.8
    p = (x / T).softmax(-1)
    want = p.unsqueeze(1) * p.unsqueeze(0) / (1 - p.unsqueeze(1))
    want.fill_diagonal_(0)
    logits = torch.zeros(R, 8, device=dev())
    logits[:, :V] = x.float().to(dev())
    ids = torch.zeros(R, 4, dtype=torch.long, device=dev())
    counts = torch.zeros(V, V, dtype=torch.float64)
    n = 0
    for seed in range(4):
        tok, lp, raw = cand_buffers(R, E)
        ops.beam_candidates(logits, ids, i32([1 + seed % 3]), i32([0, 0]), i32(()), R, V, E, T, None, None, 0.0, seed_buf(seed), tok, lp, raw)
        t = tok.cpu().long()
        counts.index_put_((t[:, 0], t[:, 1]), torch.ones(R, dtype=torch.float64), accumulate=True)
        n += R
    sigma = (want * (1 - want) / n).sqrt()
    assert bool(((counts / n - want).abs() <= 5 * sigma + 1e-12).all()), (counts / n, want)
    # consolidation: B captions of W = 2 beams x E = 3 candidates, totals = scores + cand_lp, W draws from softmax(total / ct)
    B, W, E = 8192, 2, 3
    ct = 1.3
    tot = torch.tensor([0.2, -0.4, 0.9, -1.0, 0.5, 0.0], dtype=torch.float64)
    q = (tot / ct).softmax(-1)
    want = q.unsqueeze(1) * q.unsqueeze(0) / (1 - q.unsqueeze(1))
    want.fill_diagonal_(0)
    counts = torch.zeros(W * E, W * E, dtype=torch.float64)
    n = 0
    for seed in range(4):
        R = B * W
        scores = torch.zeros(R, dtype=F32, device=dev())
        cand_lp = tot.float().view(1, W, E).expand(B, W, E).reshape(R, E).contiguous().to(dev())
        cand_tok = torch.arange(R * E, dtype=torch.int32, device=dev()).view(R, E) % 5
        ids = torch.zeros(R, 4, dtype=torch.long, device=dev())
        hist = torch.zeros(R, 4, dtype=torch.int32, device=dev())
        has_eos, parent, pick = (torch.zeros(R, dtype=torch.int32, device=dev()) for _ in range(3))
        ops.beam_consolidate(cand_tok, cand_lp, scores, ids, hist, has_eos, parent, i32([1]), i32([1 + seed]), i32([0, 0]), B, W, E, ct, None,
                             seed_buf(100 + seed), pick)
        pk = pick.view(B, W).cpu().long()
        counts.index_put_((pk[:, 0], pk[:, 1]), torch.ones(B, dtype=torch.float64), accumulate=True)
        n += B
    sigma = (want * (1 - want) / n).sqrt()
    assert bool(((counts / n - want).abs() <= 5 * sigma + 1e-12).all()), (counts / n, want)


def test_beam_consolidate_ties_gather_history(ops):
    B, W, E, L, pos, T = 3, 3, 2, 7, 9, 16
    R = B * W
    scores = torch.tensor([0.0, -1.0, -1.0] * B, device=dev())
    cand_lp = torch.tensor([[-1.0, -2.0], [0.0, -3.0], [0.0, -0.5]] * B, device=dev())
    # totals per caption: [-1, -2, -1, -4, -1, -1.5] -> flat 0, 2, 4 (three-way tie at -1, lower flat index first)
    cand_tok = torch.arange(R * E, dtype=torch.int32, device=dev()).view(R, E) + 100
    ids = torch.arange(R * (L + 2), device=dev()).view(R, L + 2).clone()
    hist = torch.arange(R * T, dtype=torch.int32, device=dev()).view(R, T).clone()
    ids0, hist0 = ids.clone(), hist.clone()
    has_eos = torch.tensor([0, 1, 0] * B, dtype=torch.int32, device=dev())
    parent, pick = torch.zeros(R, dtype=torch.int32, device=dev()), torch.zeros(R, dtype=torch.int32, device=dev())
    ctrl = i32([0, 0])
    ops.beam_consolidate(cand_tok, cand_lp, scores, ids, hist, has_eos, parent, i32([pos]), i32([L]), ctrl, B, W, E, 0.0, 101, seed_buf(0), pick)
    assert pick.view(B, W).cpu().tolist() == [[0, 2, 4]] * B
    par = torch.tensor([[b * W + 0, b * W + 1, b * W + 2] for b in range(B)]).view(-1)
    assert parent.cpu().long().tolist() == par.tolist()
    assert torch.equal(scores.cpu(), torch.full((R,), -1.0))
    assert torch.equal(ids[:, :L].cpu(), ids0[par, :L].cpu()) and torch.equal(ids[:, L].cpu(), cand_tok.cpu().long().view(-1)[par * E + torch.tensor([0, 0, 0] * B)])
    assert torch.equal(hist[:, :pos].cpu(), hist0[par, :pos].cpu()) and torch.equal(hist[:, pos].cpu().long(), par)
    assert torch.equal(hist[:, pos + 1:].cpu(), hist0[:, pos + 1:].cpu()) and torch.equal(ids[:, L + 1:].cpu(), ids0[:, L + 1:].cpu())
    assert int(ctrl[1].item()) == B                  # no caption has eos in every beam
    # a parent permutation: caption 0 keeps beam 2 twice and beam 0 (the kernel moves the rows through registers, no aliasing)
    ids, hist = ids0.clone(), hist0.clone()
    scores = torch.tensor([-5.0, -9.0, 0.0] * B, device=dev())
    cand_lp = torch.zeros(R, E, device=dev())
    ops.beam_consolidate(cand_tok, cand_lp, scores, ids, hist, has_eos, parent, i32([pos]), i32([L]), ctrl, B, W, E, 0.0, None, seed_buf(0), pick)
    par = torch.tensor([[b * W + 2, b * W + 2, b * W + 0] for b in range(B)]).view(-1)
    assert parent.cpu().long().tolist() == par.tolist()
    assert torch.equal(ids[:, :L].cpu(), ids0[par, :L].cpu()) and torch.equal(hist[:, :pos].cpu(), hist0[par, :pos].cpu())


# ------------------------------------------------------------------------------------------------------ whole searches
def tiny_model(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(tiny_config())
    m.load_state_dict(tiny_weights)
    return m.to(dev()).eval()


@pytest.mark.parametrize('tag', list(BEAM_RUNS))
def test_cached_beam_search_matches_the_reference_runs(tiny_weights, tag):
    """det / det_eos outright; smp / smp_eos: the cached path's own draws replayed through the oracle call by call (beam-major)."""
    import oracle.reference_model as orc
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    g = load_golden('tiny_beam.npz')
    kw = dict(BEAM_RUNS[tag])
    kw['eos_token_id'] = int(g[kw['eos_token_id']])
    W, E = kw['beam_width'], kw['beam_expansion_factor']
    images, prompt = torch.from_numpy(g['images']), torch.from_numpy(g['prompt'])
    B = images.shape[0]
    gen = BeamSearchTokenGenerator(tiny_model(tiny_weights), kv_cache=True, seed=1234 + len(tag), **kw)
    if tag.startswith('det'):
        ids, scores = gen(images.to(dev()), prompt.to(dev()))
        want_ids, want_scores = g[f'{tag}.ids'], g[f'{tag}.scores']
    else:
        ids, scores, draws = gen.search_cached(images.to(dev()), prompt.to(dev()), record=True)
        seq = []
        for raw_tok, pick in draws:
            seq.append(raw_tok.cpu().long().view(B, W, E).permute(1, 0, 2).reshape(W * B, E))
            seq.append(pick.cpu().long())
        it = iter(seq)

        def draw(probs, n, *a, **k):
            r = next(it)
            assert r.shape == (probs.shape[0], n)
            assert bool((probs.gather(1, r) > 0).all())
            return r
        want_ids, want_scores = orc.beam_search(tiny_weights, tiny_config(), images, prompt, draw=draw, **kw)
        assert next(it, None) is None, 'the oracle stopped before the cached path'
        want_ids, want_scores = want_ids.numpy(), want_scores.numpy()
    ids, scores = ids.cpu().numpy(), scores.float().cpu().numpy()
    assert ids.shape == want_ids.shape and np.array_equal(ids, want_ids), (ids[0].tolist(), want_ids[0].tolist())
    err = float(np.abs(scores - want_scores).max())
    assert err <= 2e-2 * (ids.shape[-1] - 1), err


def nano_model(seed=0):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=seed)
    return m.to(dev()).eval()


@pytest.fixture(scope='module')
def nano():
    return nano_model()


def nano_inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 224, 224, generator=g).to(dev()), torch.full((B, 1), 50256, dtype=torch.long, device=dev())


def test_beam_width_one_is_greedy_nano224(nano):
    from image2text_amd.decoding import BeamDecoder, BeamSpec, GreedyDecoder
    images, prompt = nano_inputs(64)
    N = 32
    want, _ = GreedyDecoder(nano).generate(images, prompt, N, return_margins=True)
    spec = BeamSpec(1, 1, 0.0, None, 0.0, None, 0.0, tuple(nano.config.no_repeat_n_grams))
    ids, scores = BeamDecoder(nano).search(images, prompt, 1 + N, spec)
    assert torch.equal(ids[:, 0], want)


def test_beam_width_one_is_greedy_llama(tmp_path, monkeypatch):
    from test_hf_decoder_gpu import _llama_model
    from image2text_amd.decoding import BeamDecoder, BeamSpec, GreedyDecoder
    cfg, m, _, V = _llama_model(tmp_path, monkeypatch, 'llama')
    m = m.to(dev()).eval()
    g = torch.Generator().manual_seed(5)
    images = torch.randn(16, 3, 32, 32, generator=g).to(dev())
    prompt = torch.randint(0, V, (16, 2), generator=g).to(dev())
    want, _ = GreedyDecoder(m).generate(images, prompt, 12, return_margins=True)
    spec = BeamSpec(1, 1, 0.0, None, 0.0, None, 0.0, tuple(cfg.no_repeat_n_grams))
    ids, _ = BeamDecoder(m).search(images, prompt, 2 + 12, spec)
    assert torch.equal(ids[:, 0], want)


def rescore(model, images, ids, P, ngrams, W):
    """teacher-forced score of every beam: sum over its generated tokens of the banned log_softmax of the full forward"""
    B, Wd, L = ids.shape
    flat = ids.reshape(B * Wd, L)
    imgs = images.repeat_interleave(Wd, 0)
    logits = model(images=imgs, ids=flat[:, :-1]).logits.float()[:, -(L - 1):]        # the text positions (after any soft prompt)
    import oracle.reference_model as orc
    tot = torch.zeros(B * Wd, dtype=torch.float64)
    for t in range(P, L):
        s = orc.apply_ngram_ban(flat[:, :t].cpu(), logits[:, t - 1].double().cpu().clone(), ngrams)
        tot += s.log_softmax(-1).gather(-1, flat[:, t:t + 1].cpu()).squeeze(1)
    return tot.view(B, Wd)


def test_nano224_beam_self_consistency(nano):
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    import oracle.reference_model as orc
    images, prompt = nano_inputs(64, seed=1)
    ngrams = (2, 3, 4)
    gen = BeamSearchTokenGenerator(nano, beam_width=3, temperature=0.0, max_new_tokens=24, no_repeat_n_grams=ngrams, beam_expansion_factor=4,
                                   consolidation_temperature=0.0, kv_cache=True)
    ids, scores = gen(images, prompt)
    assert ids.shape == (64, 3, 24)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), 'beams are sorted by score'
    for row in ids.reshape(-1, 24).tolist():
        for n in ngrams:
            grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
            assert len(grams) == len(set(grams)), (n, row)
    want = rescore(nano, images[:16], ids[:16], 1, ngrams, 3)
    err = (scores[:16].double().cpu() - want).abs().max().item()
    assert err <= 2e-2 * 23, err
    eager, escores = gen.search_cached(images, prompt, use_graph=False)
    assert torch.equal(eager, ids) and torch.equal(escores, scores)
    # sampled: same seed -> same output, another seed -> another
    kw = dict(beam_width=3, temperature=1.0, max_new_tokens=16, no_repeat_n_grams=ngrams, beam_expansion_factor=4, consolidation_temperature=1.0,
              kv_cache=True)
    a = BeamSearchTokenGenerator(nano, seed=7, **kw)(images[:8], prompt[:8])[0]
    b = BeamSearchTokenGenerator(nano, seed=7, **kw)(images[:8], prompt[:8])[0]
    c = BeamSearchTokenGenerator(nano, seed=8, **kw)(images[:8], prompt[:8])[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    torch.manual_seed(3)
    d = BeamSearchTokenGenerator(nano, **kw)(images[:8], prompt[:8])[0]
    torch.manual_seed(3)
    e = BeamSearchTokenGenerator(nano, **kw)(images[:8], prompt[:8])[0]
    assert torch.equal(d, e)
    # a prompt that already holds EOS in every beam returns at once
    ids, scores = BeamSearchTokenGenerator(nano, eos_token_id=50256, **kw)(images[:4], prompt[:4])
    assert ids.shape == (4, 3, 1) and bool((scores == 0).all())
    with pytest.raises(ValueError, match='top_k'):
        BeamSearchTokenGenerator(nano, top_k=2, **kw)(images[:4], prompt[:4])
    del orc
