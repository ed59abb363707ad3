"""Beam search on the static KV cache through sparse decoder blocks (the nano-mini family; decoding.BeamDecoder with st.kpos, the
slot_pos argument of i2t_beam_gq_decode_attention).

A sparse layer caches only the positions it keeps: slot s of the layer holds text position kpos[l][s], so key s of beam r is read
from cache row hist[r][kpos[l][s]].  Tests: the kernel at the real head shapes (identity table bit-equal to gq_decode_attention,
random tables against fp64), W = E = 1 against greedy, sampled searches replayed through the oracle, and the self-consistency of a
full-size search."""
import numpy as np
import pytest
import torch

from image2text_amd.synth import det_init_, mini_config, nano_mini_config, sharpen_gates_
from test_beam_cache_gpu import close, i32, ref_attn_rows, rescore, rnd
from test_family_oracle import variant_config

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


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('R,H,Hkv,hd', [(6, 8, 1, 128), (4, 2, 1, 128)])        # nano-mini, mini
def test_beam_gq_decode_attention_slot_pos(ops, R, H, Hkv, hd):
    S, T = 96, 192                                  # cache slots of the layer, history width (text positions)
    w, G, scale = Hkv * hd, H // Hkv, hd ** -0.5
    kt, vt = rnd(R, S, Hkv, hd, dtype=BF16, seed=21), rnd(R, S, Hkv, hd, dtype=BF16, seed=22)
    ident = torch.arange(R, dtype=torch.int32, device=dev()).unsqueeze(1).expand(R, T).contiguous()
    g = torch.Generator().manual_seed(100 * R + H)
    gd = torch.Generator(device=dev()).manual_seed(100 * R + H)
    for lpos in (0, 1, 40, S - 1):
        slot_pos = torch.randperm(T, generator=g)[:S].sort().values.to(torch.int32).to(dev())     # strictly increasing
        q = rnd(R, H * hd, dtype=BF16, seed=lpos + 1, scale=2.0)
        kvn = rnd(R, 2 * w, dtype=BF16, seed=lpos + 2)
        pos = i32([lpos])
        o0, o1 = torch.empty(R, H * hd, dtype=BF16, device=dev()), torch.empty(R, H * hd, dtype=BF16, device=dev())
        k0, v0, k1, v1 = kt.clone(), vt.clone(), kt.clone(), vt.clone()
        ops.gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k0, v0, S * w, w, o0, pos, 0, S, R, H, Hkv, hd)
        ops.beam_gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k1, v1, S * w, w, o1, pos, 0, S, R, H, Hkv, hd, hist=ident,
                                     slot_pos=slot_pos)
        assert torch.equal(o0, o1) and torch.equal(k0, k1) and torch.equal(v0, v1), f'identity table lpos={lpos}'
        hist = torch.randint(0, R, (R, T), generator=gd, device=dev(), dtype=torch.int32)
        k2, v2 = kt.clone(), vt.clone()
        ops.beam_gq_decode_attention(q, kvn[:, :w], kvn[:, w:], k2, v2, S * w, w, o1, pos, 0, S, R, H, Hkv, hd, hist=hist,
                                     slot_pos=slot_pos)
        kn, vn = kvn[:, :w].view(R, Hkv, hd), kvn[:, w:].view(R, Hkv, hd)
        assert torch.equal(k2[:, lpos], kn) and torch.equal(v2[:, lpos], vn), 'the new key goes to (r, lpos)'
        rest = torch.arange(S, device=dev()) != lpos
        assert torch.equal(k2[:, rest], kt[:, rest]) and torch.equal(v2[:, rest], vt[:, rest]), 'nothing else is written'
        rows = hist[:, slot_pos[:lpos].long()].long()                       # (R, lpos): row of key s = hist[r][slot_pos[s]]
        ar = torch.arange(lpos, device=dev())
        kk = torch.cat([kt[rows, ar], kn.unsqueeze(1)], 1)
        vv = torch.cat([vt[rows, ar], vn.unsqueeze(1)], 1)
        close(f'slot_pos hist lpos={lpos}', o1.view(R, H, hd), ref_attn_rows(q.view(R, H, hd), kk, vv, scale, G))


def test_slot_pos_needs_a_history_table(ops):
    from image2text_amd import lib as i2tlib
    R, H, hd, S = 2, 2, 128, 8
    q, out = torch.zeros(R, H * hd, dtype=BF16, device=dev()), torch.zeros(R, H * hd, dtype=BF16, device=dev())
    kc, vc = torch.zeros(R, S, hd, dtype=BF16, device=dev()), torch.zeros(R, S, hd, dtype=BF16, device=dev())
    sp, pos = torch.arange(S, dtype=torch.int32, device=dev()), i32([0])
    rc = i2tlib.load().i2t_beam_gq_decode_attention(None, q.data_ptr(), H * hd, None, None, 0, kc.data_ptr(), vc.data_ptr(), S * hd, hd,
                                                    out.data_ptr(), H * hd, pos.data_ptr(), 0, S, None, 0, sp.data_ptr(), 1, R, H, 1, hd)
    assert rc == -1 and 'slot_pos' in i2tlib.last_error()


# ------------------------------------------------------------------------------------------------------ whole searches
def family_model(cfg):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = sharpen_gates_(det_init_(VisionEncoderDecoder(cfg), seed=0))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(dev()).eval(), sd


def nano_mini_dense_config():
    """gpu/nano-mini.yaml's shape (synth.nano_mini_config's arguments) with plain MLP rotators instead of MoE"""
    from image2text_amd import synth
    return synth._family_config(img=128, num_patches=16, conv_gates=(8, 16), conv_out=32, kernel=6, n_cls=64, d=1024, heads=8,
                                enc_layers=12, dec_layers=12, block_size=256, vocab=50258, dropout=0.0, experts=4, proj=16,
                                gate_sizes=(32,), enc_ff=2, dec_ff=4, enc_top_k=2, dec_top_k=1, sparsity=0.5, moe=False)


def inputs(B, img, V, P, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, img, img, generator=g)
    prompt = torch.full((B, 1), 50256, dtype=torch.long) if V > 50256 and P == 1 else torch.randint(0, V, (B, P), generator=g)
    return images, prompt


@pytest.mark.parametrize('name,B,P,N', [('mini', 8, 2, 24), ('nano_mini', 16, 1, 24)])
def test_beam_width_one_is_greedy_sparse(name, B, P, N):
    """W = E = 1, temperature 0: the beam step runs the greedy step's kernels on an identity history, so the ids are equal"""
    from image2text_amd.decoding import BeamDecoder, BeamSpec, GreedyDecoder
    cfg = {'mini': mini_config, 'nano_mini': nano_mini_config}[name]()
    m, _ = family_model(cfg)
    assert m._engine.dec.fam.sparse and m._engine.dec.fam.mqa and m._engine.dec.fam.moe is not None
    images, prompt = inputs(B, cfg.vision_encoder_config.input.width, cfg.decoder_config.vocab_size, P, seed=3)
    images, prompt = images.to(dev()), prompt.to(dev())
    want, _ = GreedyDecoder(m).generate(images, prompt, N, return_margins=True)
    spec = BeamSpec(1, 1, 0.0, None, 0.0, None, 0.0, tuple(cfg.no_repeat_n_grams))
    ids, _ = BeamDecoder(m).search(images, prompt, P + N, spec)
    assert ids.shape == (B, 1, P + N)
    assert torch.equal(ids[:, 0], want)


@pytest.mark.parametrize('name', ['sparse_only', 'mq_sparse'])
def test_sparse_cached_beam_search_replays_through_the_oracle(name):
    """Sampled searches (W = 3, E = 4, temperature 1, consolidation temperature 1), without and with an EOS id: the cached path's own
    draws replayed through oracle.reference_model.beam_search call by call (beam-major), as
    test_beam_cache_gpu::test_cached_beam_search_matches_the_reference_runs does.  The second run's EOS id is the token the first
    run generated most often (not in the prompt); both runs share the seed, so the second follows the first until that token
    appears and the EOS rule takes part."""
    import oracle.reference_model as orc
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    cfg = variant_config('sparse_only') if name == 'sparse_only' else mini_config(moe=False)
    m, sd = family_model(cfg)
    assert m._engine.dec.fam.sparse and m._engine.dec.fam.moe is None
    W, E, B, N = 3, 4, 4, 20
    images, prompt = inputs(B, cfg.vision_encoder_config.input.width, cfg.decoder_config.vocab_size, 1, seed=7)
    base = dict(beam_width=W, beam_expansion_factor=E, temperature=1.0, consolidation_temperature=1.0, top_k=None, max_new_tokens=N,
                no_repeat_n_grams=tuple(cfg.no_repeat_n_grams), length_boost=1.0)
    eos = None
    for run in range(2):
        kw = dict(base, eos_token_id=eos)
        gen = BeamSearchTokenGenerator(m, kv_cache=True, seed=4321, **kw)
        ids, scores, draws = gen.search_cached(images.to(dev()), prompt.to(dev()), record=True)
        seq = []
        for raw_tok, pick in draws:
            seq.append(raw_tok.cpu().long().view(B, W, E).permute(1, 0, 2).reshape(W * B, E))
            seq.append(pick.cpu().long())
        it = iter(seq)

        def draw(probs, n, *a, **k):
            r = next(it)
            assert r.shape == (probs.shape[0], n)
            assert bool((probs.gather(1, r) > 0).all()), 'a replayed draw has oracle probability 0'
            return r
        # the oracle compares ids with its eos_token_id and has no None case: an id outside the vocabulary never matches, which is
        # the cached path's eos None (no EOS rule, no early stop)
        want_ids, want_scores = orc.beam_search(sd, cfg, images, prompt, draw=draw, **dict(kw, eos_token_id=-1 if eos is None else eos))
        assert next(it, None) is None, 'the oracle stopped before the cached path'
        ids, scores = ids.cpu().numpy(), scores.float().cpu().numpy()
        want_ids, want_scores = want_ids.numpy(), want_scores.numpy()
        assert ids.shape == want_ids.shape and np.array_equal(ids, want_ids), (run, ids[0].tolist(), want_ids[0].tolist())
        err = float(np.abs(scores - want_scores).max())
        print(f'{name} run {run} (eos {eos}): L = {ids.shape[-1]}, max |score - oracle| = {err:.4g}, '
              f'bound {2e-2 * (ids.shape[-1] - 1):.4g}')
        assert err <= 2e-2 * (ids.shape[-1] - 1), err
        if eos is None:
            counts = np.bincount(ids[..., 1:].reshape(-1), minlength=cfg.decoder_config.vocab_size)
            counts[prompt.numpy().reshape(-1)] = 0
            eos = int(counts.argmax())
        else:
            print(f'{name}: EOS {eos} in {int((ids == eos).any(-1).sum())} of {B * W} beams')


def test_nano_mini_dense_ffn_beam_self_consistency():
    """gpu/nano-mini.yaml's shape without MoE, B = 16, deterministic W = 3, E = 4, 24 new tokens"""
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    cfg = nano_mini_dense_config()
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = det_init_(VisionEncoderDecoder(cfg), seed=0).to(dev()).eval()
    assert m._engine.dec.fam.sparse and m._engine.dec.fam.moe is None
    B, N = 16, 24
    images, prompt = inputs(B, 128, cfg.decoder_config.vocab_size, 1, seed=1)
    images, prompt = images.to(dev()), prompt.to(dev())
    ngrams = tuple(cfg.no_repeat_n_grams)
    assert ngrams == (2, 3, 4, 5)
    gen = BeamSearchTokenGenerator(m, beam_width=3, temperature=0.0, max_new_tokens=N + 1, no_repeat_n_grams=ngrams, beam_expansion_factor=4,
                                   consolidation_temperature=0.0, kv_cache=True)
    ids, scores = gen(images, prompt)
    L = N + 1
    assert ids.shape == (B, 3, L)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), 'beams are sorted by score'
    for row in ids.reshape(-1, L).tolist():
        for n in ngrams:
            grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
            assert len(grams) == len(set(grams)), (n, row)
    want = rescore(m, images, ids, 1, ngrams, 3)
    err = (scores.double().cpu() - want).abs().max().item()
    print(f'nano-mini dense: max |score - teacher-forced rescore| = {err:.4g}, bound {2e-2 * N:.4g}')
    assert err <= 2e-2 * N, err
    eager, escores = gen.search_cached(images, prompt, use_graph=False)
    assert torch.equal(eager, ids) and torch.equal(escores, scores)
    kw = dict(beam_width=3, temperature=1.0, max_new_tokens=16, no_repeat_n_grams=ngrams, beam_expansion_factor=4, consolidation_temperature=1.0,
              kv_cache=True)
    a = BeamSearchTokenGenerator(m, seed=7, **kw)(images[:8], prompt[:8])[0]
    b = BeamSearchTokenGenerator(m, seed=7, **kw)(images[:8], prompt[:8])[0]
    c = BeamSearchTokenGenerator(m, seed=8, **kw)(images[:8], prompt[:8])[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
