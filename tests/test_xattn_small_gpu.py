"""Fused cross-attention for 8 / 16 / 32 memory tokens per image (epilogue class 16 of the 256^2 GEMM kernel, the small-S form of
i2t_xattn_kv_fused): the kernel against fp64 and against the un-fused pair, isolation between the images that share a wave, the
accepted values of S, and the model-level switch I2T_XATTN_FUSED_SMALL on the reference-run goldens.

Bounds: those of test_kernels_gpu.py::test_xattn_kv_fused (the project's bar for this kernel) and of test_model_gpu.py."""
import numpy as np
import pytest
import torch

from image2text_amd.lib import I2TError
from image2text_amd.synth import det_init_, synthetic_batch, tiny_config
from test_kernels_gpu import check, dev, rnd
from test_model_gpu import _wrapper, check_all_grads, grad_close, hidden_tol, logits_tol, maxerr

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 3.0


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def _xattn_reference(mem, w_kv, bias, q_rows, lens, H, S, mask=None, sc=1.0):
    """fp64 reference on the bf16-rounded K / V the kernel stores: per image b (S memory rows), queries q_rows[b] (n_b x d)."""
    B, S_, d = mem.shape
    assert S_ == S
    kv = (mem.double().reshape(B * S, d) @ w_kv.double().t() + bias.double()).reshape(B, S, 2 * d)
    kvb = kv.to(BF16).double()
    outs, lses = [], []
    for b in range(B):
        n = lens[b]
        qh = q_rows[b].double().reshape(n, H, 64).permute(1, 0, 2)                 # (H, n, 64)
        kh = kvb[b, :, :d].reshape(S, H, 64).permute(1, 0, 2)
        vh = kvb[b, :, d:].reshape(S, H, 64).permute(1, 0, 2)
        s = qh @ kh.transpose(-1, -2) / 8.0
        lses.append(torch.logsumexp(s, -1))                                        # (H, n)
        p = torch.softmax(s, -1)
        if mask is not None:
            p = p * mask[b][:, :n].double() * sc
        outs.append((p @ vh).permute(1, 0, 2).reshape(n, d))
    return kv, outs, lses


def _lens(B, packed, T):
    if not packed:
        return [T] * B
    lens = [int(x) for x in torch.randint(1, 65, (B,), generator=torch.Generator().manual_seed(7))]
    lens[0], lens[1], lens[2], lens[3] = 64, 0, 17, 1         # images 0..3: one wave at S = 8 / 16, two neighbouring pairs at S = 32
    return lens


def _run_fused(ops, mem, w_in, b_in, q, lens, cu, B, S, H, T, packed, dr, pad_rows=256):
    """One fused call into pre-filled buffers: kv with pad_rows sentinel rows behind its B S rows, o with 16 rows of 7.0 behind its own."""
    d = 64 * H
    total = sum(lens)
    kv_all = torch.full((B * S + pad_rows, 2 * d), SENTINEL, dtype=BF16, device=dev())
    kv = kv_all[:B * S].view(B, S, 2 * d)
    o_all = torch.full((q.reshape(-1, d).shape[0] + 16, d), 7.0, dtype=BF16, device=dev())
    o = o_all[:-16].view(q.shape)
    lse = torch.zeros(H * total if packed else B * H * T, device=dev())
    ops.xattn_kv_fused(mem.view(B * S, d), w_in[d:], b_in[d:], q, kv, o, lse, B, S, H, T, drop=dr,
                       cu_q=cu if packed else None, total_q=total if packed else 0)
    torch.cuda.synchronize()
    return kv_all, kv, o_all, o, lse


# S, B, H: one full workgroup tile + a wave with 5 of 8 images live | 2 full waves + a wave with 1 of 4 live | a wave with 1 of 2 live |
# exactly one tile, nothing partial
SHAPES = [(8, 37, 2), (16, 9, 12), (32, 5, 4), (16, 16, 2)]


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('packed', [True, False])
@pytest.mark.parametrize('S,B,H', SHAPES)
def test_xattn_kv_fused_small(ops, S, B, H, packed, drop):
    """test_xattn_kv_fused with S < 64: stored K/V, output and lse against fp64; K/V against ops.gemm, output against
    ops.attention_fwd, attention_bwd on the fused outputs against attention_bwd on the un-fused ones.  Packed ragged queries (64, 0,
    17 and 1 rows on images that share a wave) and dense T = 100 (seven query blocks), with and without probability dropout on
    i2t_attention_fwd's index space (Tk = S).  Nothing outside the live rows may be written."""
    from image2text_amd import rng
    d = 64 * H
    mem = rnd(B, S, d, dtype=BF16, seed=400)
    w_in = rnd(3 * d, d, dtype=BF16, seed=401, scale=d ** -0.5)
    b_in = rnd(3 * d, seed=402, scale=0.3)
    T = 64 if packed else 100
    lens = _lens(B, packed, T)
    total = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev())
    q = rnd(total, d, dtype=BF16, seed=403) if packed else rnd(B, T, d, dtype=BF16, seed=403)
    key, thr = rng.site_key(31337, 4100), rng.threshold(0.1)
    sc = rng.scale(thr)
    dr = (1, key, thr, sc) if drop else None
    kv_all, kv, o_all, o, lse = _run_fused(ops, mem, w_in, b_in, q, lens, cu, B, S, H, T, packed, dr)
    assert bool((kv_all[B * S:] == SENTINEL).all()), 'a kv row at or past B S was written'
    assert bool((o_all[-16:] == 7.0).all()), 'an output row past the last query was written'
    q_rows = [q[int(cu[b]):int(cu[b + 1])] for b in range(B)] if packed else [q[b] for b in range(B)]
    mask = None
    if drop:
        mask = rng.keep_mask(key, B * H * T * S, thr).view(B, H, T, S).to(dev())
    kv_ref, o_ref, lse_ref = _xattn_reference(mem, w_in[d:], b_in[d:], q_rows, lens, H, S, mask, sc)
    check('fused kv', kv, kv_ref, 2e-2, 1 / 128)
    for b in range(B):
        n = lens[b]
        if n == 0:
            continue
        ob = o[int(cu[b]):int(cu[b + 1])] if packed else o[b]
        check(f'fused o[{b}]', ob, o_ref[b], 1e-2, 1 / 64)
        for h in range(H):
            got = lse[h * total + int(cu[b]):h * total + int(cu[b]) + n] if packed else lse.view(B, H, T)[b, h]
            check(f'fused lse[{b},{h}]', got, lse_ref[b][h], 2e-3, 1e-3)
    # the same call through the un-fused kernels (GEMM + attention_fwd)
    cuq, tq = (cu if packed else None), (total if packed else 0)
    kv2 = torch.empty(B, S, 2 * d, dtype=BF16, device=dev())
    ops.gemm(mem.view(B * S, d), w_in[d:], kv2.view(B * S, 2 * d), B * S, 2 * d, d, bias=b_in[d:])
    o2, lse2 = torch.zeros_like(q), torch.zeros_like(lse)
    ops.attention_fwd(q, kv2[..., :d], kv2[..., d:], o2, lse2, B, H, T, S, False, drop=dr, cu_q=cuq, total_q=tq)
    assert float((kv.float() - kv2.float()).abs().max()) <= 2.0 ** -7 * float(kv2.float().abs().max())
    check('fused vs unfused o', o.reshape(-1, d), o2.reshape(-1, d), 2e-2, 1 / 32)
    # backward of the fused forward = the un-fused backward kernels on its saved tensors
    do = rnd(*q.shape, dtype=BF16, seed=404)
    oc = o.contiguous()
    dq, dkv = torch.zeros_like(q), torch.zeros(B, S, 2 * d, dtype=BF16, device=dev())
    ops.attention_bwd(q, kv[..., :d], kv[..., d:], oc, do, lse, torch.empty_like(lse), dq, dkv[..., :d], dkv[..., d:], B, H, T, S, False,
                      drop=dr, cu_q=cuq, total_q=tq)
    dq2, dkv2 = torch.zeros_like(q), torch.zeros_like(dkv)
    ops.attention_bwd(q, kv2[..., :d], kv2[..., d:], o2, do, lse2, torch.empty_like(lse), dq2, dkv2[..., :d], dkv2[..., d:], B, H, T, S, False,
                      drop=dr, cu_q=cuq, total_q=tq)
    check('bwd dq on fused outputs', dq, dq2, 3e-2 * float(do.float().abs().max()), 1 / 16)
    check('bwd dkv on fused outputs', dkv, dkv2, 3e-2 * float(do.float().abs().max()), 1 / 16)


@pytest.mark.parametrize('S', [8, 16, 32])
def test_neighbouring_images_of_a_wave_are_isolated(ops, S):
    """Images b and b + 1 share a wave (at S = 8 even one 16-key score block).  Scaling image b + 1's memory rows by 50 must leave
    image b's output, lse and stored K/V rows BIT-equal (and those of every other image): a key of the neighbour that leaked into
    the row maximum, the denominator or P V would move them -- a slip that bf16 tolerances could hide."""
    B, H, T = 4, 2, 64
    d = 64 * H
    mem = rnd(B, S, d, dtype=BF16, seed=410)
    w_in = rnd(3 * d, d, dtype=BF16, seed=411, scale=d ** -0.5)
    b_in = rnd(3 * d, seed=412, scale=0.3)
    lens = [20, 33, 5, 16]
    total = sum(lens)
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev())
    q = rnd(total, d, dtype=BF16, seed=413)
    _, kv_a, _, o_a, lse_a = _run_fused(ops, mem, w_in, b_in, q, lens, cu, B, S, H, T, True, None)
    for nb in (1, 2):                                # the scaled image; its neighbours on both sides must not move
        mem2 = mem.clone()
        mem2[nb] = (mem2[nb].float() * 50).to(BF16)
        _, kv_b, _, o_b, lse_b = _run_fused(ops, mem2, w_in, b_in, q, lens, cu, B, S, H, T, True, None)
        assert not torch.equal(o_a[int(cu[nb]):int(cu[nb + 1])], o_b[int(cu[nb]):int(cu[nb + 1])])      # (the scaling did reach the kernel)
        for b in range(B):
            if b == nb:
                continue
            r0, r1 = int(cu[b]), int(cu[b + 1])
            assert torch.equal(o_a[r0:r1], o_b[r0:r1]), f'S={S}: o of image {b} moved with image {nb}'
            assert torch.equal(kv_a[b], kv_b[b]), f'S={S}: K/V rows of image {b} moved with image {nb}'
            for h in range(H):
                assert torch.equal(lse_a[h * total + r0:h * total + r1], lse_b[h * total + r0:h * total + r1]), f'S={S}: lse of image {b} moved'


def test_accepted_memory_token_counts(ops):
    """S = 24 and S = 128 are refused; S = 64 still runs (class 8, untouched) and reproduces ops.gemm + ops.attention_fwd."""
    B, H, T = 3, 2, 20
    d = 64 * H
    w_in = rnd(3 * d, d, dtype=BF16, seed=421, scale=d ** -0.5)
    b_in = rnd(3 * d, seed=422, scale=0.3)
    q = rnd(B, T, d, dtype=BF16, seed=423)
    for S in (24, 128):
        mem = rnd(B, S, d, dtype=BF16, seed=420)
        kv = torch.zeros(B, S, 2 * d, dtype=BF16, device=dev())
        with pytest.raises(I2TError):
            ops.xattn_kv_fused(mem.view(B * S, d), w_in[d:], b_in[d:], q, kv, torch.zeros_like(q), torch.zeros(B * H * T, device=dev()), B, S, H, T)
    S = 64
    mem = rnd(B, S, d, dtype=BF16, seed=420)
    kv, o, lse = torch.zeros(B, S, 2 * d, dtype=BF16, device=dev()), torch.zeros_like(q), torch.zeros(B * H * T, device=dev())
    ops.xattn_kv_fused(mem.view(B * S, d), w_in[d:], b_in[d:], q, kv, o, lse, B, S, H, T)
    kv2, o2, lse2 = torch.empty_like(kv), torch.zeros_like(q), torch.zeros_like(lse)
    ops.gemm(mem.view(B * S, d), w_in[d:], kv2.view(B * S, 2 * d), B * S, 2 * d, d, bias=b_in[d:])
    ops.attention_fwd(q, kv2[..., :d], kv2[..., d:], o2, lse2, B, H, T, S, False)
    assert float((kv.float() - kv2.float()).abs().max()) <= 2.0 ** -7 * float(kv2.float().abs().max())
    check('S = 64 fused vs unfused o', o, o2, 2e-2, 1 / 32)
    check('S = 64 fused vs unfused lse', lse, lse2, 2e-3, 1e-3)


# ------------------------------------------------------------------------------------------------ model level
class _Calls:
    """Counts the fused launches and the un-fused cross-attention launches (ops.attention_fwd, not causal, over S keys)."""

    def __init__(self, monkeypatch, S):
        from image2text_amd import ops as _ops
        self.fused = self.unfused = 0
        fused0, attn0 = _ops.xattn_kv_fused, _ops.attention_fwd

        def fused(*a, **k):
            self.fused += 1
            return fused0(*a, **k)

        def attn(*a, **k):
            if a[8] == S and a[9] is False:
                self.unfused += 1
            return attn0(*a, **k)

        monkeypatch.setattr(_ops, 'xattn_kv_fused', fused)
        monkeypatch.setattr(_ops, 'attention_fwd', attn)

    def take(self):
        r = (self.fused, self.unfused)
        self.fused = self.unfused = 0
        return r


def _tiny(tiny_weights, **kw):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(tiny_config(**kw))
    m.load_state_dict(tiny_weights)
    return m.to(dev()).eval()


def _n_cross(model):
    return sum(bool(c) for c in model._engine.dec_cross)


@pytest.mark.parametrize('tag,kw', [('nomask', {}), ('cross_only', dict(use_soft_prompting=False))])
def test_tiny_forward_with_the_switch(tiny_weights, tiny_forward, monkeypatch, tag, kw):
    """The tiny model (n_cls = 8, 2 heads of 64) on the reference-run goldens with I2T_XATTN_FUSED_SMALL=1: the checks of
    test_tiny_forward[nomask] / test_tiny_forward_modes[cross_only]; the fused launch replaces every un-fused cross-attention
    launch, and runs zero times with the switch unset."""
    f = tiny_forward
    calls = _Calls(monkeypatch, 8)
    msk = None if tag == 'nomask' else torch.from_numpy(f['row_mask']).to(dev())
    images, ids = torch.from_numpy(f['images']).to(dev()), torch.from_numpy(f['ids']).to(dev())
    monkeypatch.delenv('I2T_XATTN_FUSED_SMALL', raising=False)
    off = _tiny(tiny_weights, **kw)
    assert not off._engine.xattn_fused_small
    with torch.no_grad():
        off(images=images, ids=ids, attn_msk=msk)
    fused_off, unfused_off = calls.take()
    assert fused_off == 0 and unfused_off >= _n_cross(off) >= 1 and unfused_off % _n_cross(off) == 0
    monkeypatch.setenv('I2T_XATTN_FUSED_SMALL', '1')
    m = _tiny(tiny_weights, **kw)
    assert m._engine.xattn_fused_small
    with torch.no_grad():
        out = m(images=images, ids=ids, attn_msk=msk)
    assert calls.take() == (unfused_off, 0)
    if tag == 'cross_only':
        assert unfused_off == _n_cross(m)               # one decoder segment: once per cross layer
    if tag == 'nomask':
        assert tuple(out.logits.shape) == f[f'{tag}.logits'].shape and tuple(out.hidden_state.shape) == f[f'{tag}.hidden_state'].shape
        maxerr(f'tiny_small.{tag}.encoder_output', out.encoder_output, f[f'{tag}.encoder_output'], 2e-2)
    maxerr(f'tiny_small.{tag}.logits', out.logits, f[f'{tag}.logits'], logits_tol(f[f'{tag}.logits']))
    maxerr(f'tiny_small.{tag}.hidden_state', out.hidden_state, f[f'{tag}.hidden_state'], hidden_tol(f[f'{tag}.hidden_state']))
    if tag == 'nomask':
        assert (out.logits.argmax(-1).cpu().numpy() == f[f'{tag}.logits'].argmax(-1)).mean() > 0.97


def test_tiny_train_step_with_the_switch(tiny_weights, tiny_forward, tiny_train, monkeypatch):
    """test_tiny_train_step_loss_and_every_gradient with the fused small-S forward: the un-fused backward runs on its saved kv, co, lse."""
    calls = _Calls(monkeypatch, 8)
    monkeypatch.setenv('I2T_XATTN_FUSED_SMALL', '1')
    w = _wrapper(tiny_config(), tiny_weights).train()
    f = tiny_forward
    images, labels = torch.from_numpy(f['images']).to(dev()), torch.from_numpy(f['labels']).to(dev())
    loss, metrics = w.train_step(images, labels)
    assert calls.take() == (_n_cross(w.model), 0)       # the training path runs the text segment only: once per cross layer
    loss.backward()
    ref = float(tiny_train['loss'])
    assert abs(float(loss.detach()) - ref) <= 1e-2 * max(1.0, ref)
    assert 'train_loss_lm' in metrics
    check_all_grads('tiny_small', w.model, tiny_train, rel=0.15, cos=0.985)
    with torch.no_grad():
        vloss, _ = w.eval().val_step(images, labels)
    assert abs(float(vloss) - float(tiny_train['val_loss'])) <= 1e-2 * max(1.0, float(tiny_train['val_loss']))


@pytest.mark.parametrize('n_cls,dropout', [(16, 0.1), (32, 0.0)])
def test_switch_on_against_off_at_16_and_32_tokens(monkeypatch, n_cls, dropout):
    """tiny_config(n_cls = 16 / 32), random weights: forward logits and one train step's gradients with the switch on against the
    switch off on the same state dict.  The two differ only in the cross-attention forward's bf16 rounding.  With dropout 0.1 the
    same step seed gives both the same masks: the un-fused backward has to regenerate the fused forward's mask."""
    cfg = tiny_config(dropout=dropout, n_cls=n_cls)
    images, labels = synthetic_batch(4, 32, 16, cfg.decoder_config.vocab_size, seed=9)
    images, labels = images.to(dev()), labels.to(dev())
    calls = _Calls(monkeypatch, n_cls)
    res = {}
    sd = None
    for mode in ('off', 'on'):
        if mode == 'on':
            monkeypatch.setenv('I2T_XATTN_FUSED_SMALL', '1')
        else:
            monkeypatch.delenv('I2T_XATTN_FUSED_SMALL', raising=False)
        w = _wrapper(cfg)
        if sd is None:
            det_init_(w.model, seed=0)
            sd = {k: v.detach().cpu().clone() for k, v in w.model.state_dict().items()}
        else:
            w.model.load_state_dict(sd)
        w.eval()
        with torch.no_grad():
            logits = w.model(images=images, ids=labels.clamp(min=0)).logits.detach().float().cpu().numpy()
        n_fwd = calls.take()
        w.train()
        torch.manual_seed(20240917)                     # the step seed (hence every dropout mask) derives from torch's seed
        loss, _ = w.train_step(images, labels)
        n_train = calls.take()
        loss.backward()
        nc = _n_cross(w.model)
        if mode == 'on':
            assert n_fwd[0] >= nc and n_fwd[1] == 0 and n_train == (nc, 0)
        else:
            assert n_fwd[0] == 0 and n_fwd[1] >= nc and n_train == (0, nc)
        res[mode] = (logits, float(loss.detach()), {n: p.grad.detach().float().cpu().numpy() for n, p in w.model.named_parameters()})
    maxerr(f'tiny_small.n_cls{n_cls}.logits', res['on'][0], res['off'][0], logits_tol(res['off'][0]))
    assert abs(res['on'][1] - res['off'][1]) <= 1e-2 * max(1.0, res['off'][1])
    fails = []
    for name, ref in res['off'][2].items():
        try:
            grad_close(f'tiny_small.n_cls{n_cls}.{name}', torch.from_numpy(res['on'][2][name]), ref)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, f'{len(fails)} gradients out of tolerance: ' + '; '.join(fails[:6])
