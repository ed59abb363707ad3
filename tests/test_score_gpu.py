"""VisionEncoderDecoder.score / generation_utils.rerank on the MI355X: the log-likelihood of given captions on every decoder the
forward runs on, against fp64 log_softmax(forward(...).logits / T) gathered at the labels.

The bound (per position; u = 2^-24, K = the decoder width, h / w the bf16 hidden row and head rows, z = forward's fp32 logits):
  * the fallback form scores bf16 logits: 2^-8 |z| relative per logit, which moves the target by 2^-8 |z_t| / T and the logsumexp by
    no more than 2^-8 max_c |z_c| / T;
  * the fused form re-accumulates the logits in fp32, possibly in another order than forward's GEMM: K u sum_k |h| |w| per logit on
    each side, on the target and (through the logsumexp, 1-Lipschitz in the largest change of a logit) on the row's worst column;
  * the sum of exp's, one log, the final roundings: the terms tests/test_lse_head_gpu.py derives (and V additions for the row form).
Where a golden holds the reference's logits (tests/golden/tiny_forward.npz, mini_forward.npz) the log-probs derived from those in fp64
are held to the bar of that golden's logits-parity test (tests/test_model_gpu.py::test_tiny_forward: max |err| <= logits_tol;
tests/test_family_gpu.py::test_mini_forward_against_reference_and_oracle: 0.9-quantile of |err| <= logits_tol)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from image2text_amd.synth import det_init_, mini_config, reference_unit_test_config, sharpen_gates_, synthetic_batch, tiny_config
from test_model_gpu import logits_tol

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
IGNORE = -100


def dev():
    return torch.device('cuda:0')


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


def reference_logprobs(logits, labels, temperature, ignore=IGNORE):
    """fp64 log_softmax(logits / T) gathered at the labels; 0 where the label is ignored.  -> (logprob [B, T], lse [B, T])"""
    z = torch.as_tensor(logits).to(dev()).double() / temperature
    labels = labels.to(dev())
    live = (labels != ignore) & (labels >= 0) & (labels < z.shape[-1])
    col = torch.where(live, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(z, dim=-1)
    lp = z.gather(-1, col[..., None])[..., 0] - lse
    return torch.where(live, lp, torch.zeros_like(lp)), lse


def score_bound(m, out, labels, temperature):
    """the derived bound of the module docstring, [B, T]"""
    eng = m._engine
    V, K = eng.dec.V, eng.dec.d
    z = out.logits.double()
    B, T = z.shape[:2]
    hb = out.hidden_state[:, -T:].reshape(B * T, K).to(BF16).double()
    W = eng.arena.W(eng.n_head)[:V].double()
    S = (hb.abs() @ W.abs().T).view(B, T, V)
    live = (labels >= 0) & (labels < V)
    col = torch.where(live, labels, torch.zeros_like(labels))[..., None]
    zt, St = z.gather(-1, col)[..., 0].abs(), S.gather(-1, col)[..., 0]
    zmax, Smax = z.abs().amax(dim=-1), S.amax(dim=-1)
    it = 1.0 / temperature
    nseg = (V + 63) // 64
    n_m = 2 + (nseg + 63) // 64 + 6
    spread = it * (z.amax(dim=-1) - z.amin(dim=-1))
    sum_log = U * (3 * spread + 3 * (n_m + 1) + 64 + n_m + V) + 2 * U * np.log(V) + 3 * U * it * zmax
    return it * 2.0 ** -8 * (zt + zmax) + 2 * it * K * U * (St + Smax) + sum_log + 2 * U * it * zt


def check_score(m, images, ids, tag):
    """the contract of score() against the model's own forward, T in {1, 0.7}; -> the T = 1 record"""
    images, ids = images.to(dev()), ids.to(dev())
    with torch.no_grad():
        out = m(images=images, ids=ids)
    B, T = out.logits.shape[:2]
    from image2text_amd.models.vision_encoder_decoder import next_token_labels
    labels = next_token_labels(ids, IGNORE)
    first = None
    for temperature in (1.0, 0.7):
        sc = m.score(images, ids, temperature=temperature)
        assert tuple(sc.token_logprobs.shape) == (B, T) and tuple(sc.lse.shape) == (B, T) and tuple(sc.logprob.shape) == (B,)
        assert sc.token_logprobs.dtype == F32 and sc.lse.dtype == F32 and sc.logprob.dtype == F32
        ref, lse_ref = reference_logprobs(out.logits, labels[:, :T], temperature)
        bound = score_bound(m, out, labels[:, :T], temperature)
        err, err_lse = (sc.token_logprobs.double() - ref).abs(), (sc.lse.double() - lse_ref).abs()
        print(f'{tag} T={temperature}: logprob worst error / bound {float((err / bound).max()):.3g} (abs {float(err.max()):.3g}), '
              f'lse {float((err_lse / bound).max()):.3g} (abs {float(err_lse.max()):.3g})')
        assert torch.isfinite(sc.token_logprobs).all() and (err <= bound).all() and (err_lse <= bound).all()
        dead = labels[:, :T] == IGNORE
        assert dead[:, -1].all() or T < ids.shape[1]
        assert torch.equal(sc.token_logprobs[dead], torch.zeros_like(sc.token_logprobs[dead]))
        assert torch.equal(sc.logprob, sc.token_logprobs.sum(dim=1))
        # explicit labels equal to the default shift, and an explicit encoder output: identical
        sc2 = m.score(images, ids, labels=labels, temperature=temperature)
        sc3 = m.score(None, ids, temperature=temperature, encoder_output=m.encode(images))
        for other in (sc2, sc3):
            assert torch.equal(other.token_logprobs, sc.token_logprobs) and torch.equal(other.lse, sc.lse) and torch.equal(other.logprob, sc.logprob)
        first = first or sc
    # labels of the caller: some ignored, one out of range
    lab = labels.clone()
    lab[:, ::3] = IGNORE
    lab[0, 1] = m._engine.dec.V
    sc = m.score(images, ids, labels=lab)
    ref, _ = reference_logprobs(out.logits, lab[:, :T], 1.0)
    assert ((sc.token_logprobs.double() - ref).abs() <= score_bound(m, out, lab[:, :T], 1.0)).all()
    off = (lab[:, :T] == IGNORE) | (lab[:, :T] >= m._engine.dec.V)
    assert torch.equal(sc.token_logprobs[off], torch.zeros_like(sc.token_logprobs[off])) and torch.equal(sc.lse, first.lse)
    return first


def test_dense_decoder_fused_path_and_reference_golden(tiny_weights, tiny_forward):
    """tiny_config: d = 128 -> the fused form.  Also against the log-probs of the reference's own logits."""
    m = _ved(tiny_config(), tiny_weights)
    assert m._engine.dec.d % 128 == 0
    f = tiny_forward
    images, ids = torch.from_numpy(f['images']), torch.from_numpy(f['ids'])
    sc = check_score(m, images, ids, 'tiny')
    from image2text_amd.models.vision_encoder_decoder import next_token_labels
    T = sc.token_logprobs.shape[1]
    ref, _ = reference_logprobs(f['nomask.logits'], next_token_labels(ids, IGNORE)[:, :T], 1.0)
    err = float((sc.token_logprobs.double() - ref).abs().max())
    print(f'tiny vs the reference golden: max |err| {err:.4g}, bar {logits_tol(f["nomask.logits"]):.4g}')
    assert err <= logits_tol(f['nomask.logits'])


def test_dense_decoder_fallback_path():
    """a decoder of width 64: d % 128 != 0 -> bf16 logits + ce_fwd + gather"""
    m = _ved(tiny_config(dec_d=64, dec_heads=1))
    assert m._engine.dec.d % 128 != 0
    images, labels = synthetic_batch(3, 32, 12, 384, seed=5)
    check_score(m, images, labels.clamp(min=0), 'dense64')


def test_nano_mini_sparse_mqa_decoder_and_reference_golden():
    """mini_config: multi-query attention, MoE rotators, sparse token subsets.  Also against the reference golden."""
    f = load_golden('mini_forward.npz')
    m = _ved(mini_config(), sharpen=True)
    assert m._engine.dec.fam is not None and m._engine.dec.fam.sparse
    images, ids = torch.from_numpy(f['images']), torch.from_numpy(f['ids'])
    sc = check_score(m, images, ids, 'mini')
    from image2text_amd.models.vision_encoder_decoder import next_token_labels
    T = sc.token_logprobs.shape[1]
    ref, _ = reference_logprobs(f['logits'], next_token_labels(ids, IGNORE)[:, :T], 1.0)
    err = (sc.token_logprobs.double() - ref).abs()[:, :-1].flatten().cpu().numpy()          # (the last column is ignored: 0 on both sides)
    print(f'mini vs the reference golden: 0.9-quantile |err| {float(np.quantile(err, 0.9)):.4g}, bar {logits_tol(f["logits"]):.4g}')
    assert float(np.quantile(err, 0.9)) <= logits_tol(f['logits'])


def test_gpt2_hf_decoder_with_soft_prompt(tmp_path, monkeypatch):
    """Hugging Face GPT-2 plugin + soft prompt: engine.decode_prefixed"""
    from test_hf_decoder_gpu import _build
    _, m = _build(tmp_path, monkeypatch, True, True)
    m = m.to(dev()).eval()
    assert m._engine.dec.prefixed
    images, labels = synthetic_batch(3, 32, 12, 384, seed=17)
    check_score(m, images, labels.clamp(min=0), 'hf_gpt2.soft')


def test_gpt2_hf_decoder_without_soft_prompt(tmp_path, monkeypatch):
    """Hugging Face GPT-2 plugin, ids only: engine.decode_segment"""
    from test_hf_decoder_gpu import _build
    _, m = _build(tmp_path, monkeypatch, True, False)
    m = m.to(dev()).eval()
    assert not m._engine.dec.prefixed
    images, labels = synthetic_batch(3, 32, 12, 384, seed=17)
    check_score(m, images, labels.clamp(min=0), 'hf_gpt2.ids')


def test_llama_shaped_decoder(tmp_path, monkeypatch):
    from test_hf_decoder_gpu import _llama_model
    _, m, _, V = _llama_model(tmp_path, monkeypatch, 'llama')
    m = m.to(dev()).eval()
    assert m._engine.dec.llama is not None
    images, labels = synthetic_batch(3, 32, 12, V, seed=17)
    check_score(m, images, labels.clamp(min=0), 'hf_llama')


def test_non_causal_decoder():
    m = _ved(reference_unit_test_config(), sharpen=True)
    assert not m._engine.dec.causal
    images, labels = synthetic_batch(2, 128, 12, 1024, seed=9)
    check_score(m, images, labels.clamp(min=0), 'noncausal')


def test_block_size_crop():
    """ids longer than block_size - n_cls: T is cropped as forward crops it, the last kept position is labelled with the next token"""
    m = _ved(tiny_config(block_size=20))
    images, labels = synthetic_batch(2, 32, 16, 384, seed=3)
    ids = labels.clamp(min=0)
    sc = check_score(m, images, ids, 'crop')
    assert sc.token_logprobs.shape[1] == 12 and bool((sc.token_logprobs[:, -1] != 0).all())


def test_fused_form_does_not_materialise_the_logits():
    """one decoder layer of width 128 under a 50257-token head, 8192 rows: the rise of the allocator's peak across score() stays under
    the M x Vp x 2 bytes of the bf16 logits the fused form avoids.  The d = 64 twin (fallback form) runs the same call; not held to it."""
    B, T = 128, 64
    g = torch.Generator().manual_seed(1)
    images = torch.randn(B, 3, 32, 32, generator=g).to(dev())
    ids = torch.randint(0, 50257, (B, T), generator=g).to(dev())
    for d, heads in ((128, 2), (64, 1)):
        m = _ved(tiny_config(dec_layers=1, dec_d=d, dec_heads=heads, vocab=50257, block_size=T + 8))
        m.score(images, ids)                                  # warm-up: cached workspaces, the parameter arena
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sc = m.score(images, ids)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        logits_bytes = B * T * m._engine.dec.Vp * 2
        print(f'd={d}: peak rise {rise / 2 ** 20:.1f} MiB, bf16 logits would be {logits_bytes / 2 ** 20:.1f} MiB')
        assert torch.isfinite(sc.token_logprobs).all() and bool((sc.token_logprobs[:, :-1] < 0).all())
        if d % 128 == 0:
            assert rise < logits_bytes
        del m, sc


def test_rerank(tiny_weights, tiny_forward, monkeypatch):
    from image2text_amd.models.generation_utils import rerank
    m = _ved(tiny_config(), tiny_weights)
    V = 384
    eos = V - 1
    images = torch.from_numpy(tiny_forward['images'])[:2].to(dev())
    B, W = images.shape[0], 3
    prompt = torch.full((B, 1), eos, dtype=torch.long, device=dev())              # BOS = EOS, as a GPT-2 tokenizer has it
    greedy = m.generate(images, prompt, max_new_tokens=10, top_k=1)
    greedy[:, 1:] = torch.where(greedy[:, 1:] == eos, torch.full_like(greedy[:, 1:], 5), greedy[:, 1:])      # (no EOS of its own)
    L = greedy.shape[1]
    cand = greedy[:, None].repeat(1, W, 1)
    cand[:, 1, 3] = (cand[:, 1, 3] + 7) % (V - 1)                                 # one token replaced
    cand[:, 2, 2::2] = (cand[:, 2, 2::2] + 11) % (V - 1)                          # every other token replaced ...
    cand[:, 2, 6] = eos                                                           # ... and an EOS in the middle: what follows is not scored
    calls = []
    eng = m._engine
    real = eng.encode
    monkeypatch.setattr(eng, 'encode', lambda images, save: (calls.append(int(images.shape[0])), real(images, save))[1])
    order, lp = rerank(m, images, cand, eos=eos)
    assert calls == [B]                                                           # the encoder ran once, over the B images
    assert tuple(order.shape) == (B, W) and tuple(lp.shape) == (B, W)
    assert torch.equal(order.sort(dim=1).values, torch.arange(W, device=dev()).expand(B, W))
    ranked = lp.gather(1, order)
    assert bool((ranked[:, :-1] >= ranked[:, 1:]).all())
    # the same numbers from score() on the flattened rows, labels masked by hand
    flat = cand.reshape(B * W, L)
    labels = torch.full_like(flat, IGNORE)
    for r in range(B * W):
        row = flat[r].tolist()
        for t in range(L - 1):
            if eos not in row[1:t + 1]:
                labels[r, t] = row[t + 1]
    assert int((labels[2] != IGNORE).sum()) == 6                                  # tokens 1 .. 6 of the row with the EOS at column 6
    enc = m.encode(images)
    enc = enc[:, None].expand(B, W, *enc.shape[1:]).reshape(B * W, *enc.shape[1:])
    want = m.score(None, flat, labels=labels, encoder_output=enc)
    assert torch.equal(lp.reshape(-1), want.logprob)
    assert bool((want.token_logprobs[labels == IGNORE] == 0).all())


def test_scoring_kernels_replay_from_a_graph():
    """gemm_lse + lse_token_logprob captured on a side stream and replayed: bit-identical to the eager launches"""
    from image2text_amd import ops
    from image2text_amd.decoding import _capture_launches
    M, V, d = 96, 1000, 128
    g = torch.Generator(device=dev()).manual_seed(4)
    hid = torch.randn(M, d, generator=g, device=dev()).to(BF16)
    W = (torch.randn(V, d, generator=g, device=dev()) * 0.3).to(BF16)
    labels = torch.randint(0, V, (M,), generator=g, device=dev())
    labels[3] = IGNORE
    nseg = (V + 63) // 64

    def launches(stats, lse, lp):
        ops.gemm_lse(hid, W, stats, M, V, d, scale=1.0 / 0.7)
        ops.lse_token_logprob(stats, hid, W, labels, lse, lp, M, V, d, scale=1.0 / 0.7, ignore_index=IGNORE)

    eager = [torch.zeros(M, nseg, 2, device=dev()), torch.zeros(M, device=dev()), torch.zeros(M, device=dev())]
    launches(*eager)
    bufs = [torch.zeros_like(t) for t in eager]
    graph = _capture_launches(dev(), lambda: launches(*bufs))
    for t in bufs:
        t.fill_(float('nan'))
    graph.launch()
    torch.cuda.synchronize()
    for a, b in zip(eager, bufs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
