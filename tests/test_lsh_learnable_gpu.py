"""The learnable LSH head (``lsh_config.learnable: True``) on the MI355X: its four kernels against fp64 statements of the same
arithmetic, the head against the reference's fixture (tests/golden/vit_head_lsh_learnable.npz) and, at the shipped width, against
the fp64 restatement (tests/lsh_learnable_ref.py); a whole train step, optimizer step and the three decoders; deterministic mode.

Bars.  The cosines and their gradient run in fp32 (``i2t_gemm_f32``); the only bf16 operands are z, emb.weight and the output
cotangent of the slot-grouped GEMMs.  The project's bars for bf16 heads (tests/test_vit_gpu.py) are output within 1e-2 of its scale,
gradients rel-L2 6e-2 / cosine 0.995.  Measured on the MI355X (REPORT entries): output 2.3e-3 (fixture) and 2.4e-3
(shipped width) of its scale, worst gradient rel-L2 3.2e-3, worst cosine 1 - 4.9e-6.  The head cases therefore hold four times the
measured figures: output 1e-2 of its scale (unchanged), gradients rel-L2 1.2e-2 / cosine 0.99998.  The whole-model case keeps the
existing whole-model bars.  Every figure is printed and kept in REPORT before its assertion.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lsh_learnable_ref as rs
from conftest import load_golden
from image2text_amd.synth import det_init_, fake_tokenizer, synthetic_batch
from test_lsh_learnable_cpu import SPEC, build_encoder, fixture_state
from test_model_gpu import grad_close
from test_vit_gpu import dev, vit_model_config

os.environ.setdefault('I2T_VIT_B16_CHECKPOINT', 'random')
pytestmark = pytest.mark.gpu
REPORT = {}
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OUT_TOL, GRAD_REL, GRAD_COS = 1e-2, 1.2e-2, 0.99998


@pytest.fixture(scope='module', autouse=True)
def write_report():
    yield
    out = os.environ.get('I2T_REPORT_DIR', 'test_reports')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'parity_report_lsh_learnable.json'), 'w') as fh:
        json.dump(REPORT, fh, indent=1, sort_keys=True)


def close(name, got, ref, rel, cos):
    """grad_close with the figures printed and kept before the assertion"""
    g, r = got.detach().double().cpu().numpy().ravel(), np.asarray(ref, dtype=np.float64).ravel()
    e = float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-300))
    c = float(g @ r / (np.linalg.norm(g) * np.linalg.norm(r) + 1e-300))
    REPORT[name] = {'rel_l2': e, 'cos': c, 'bar_rel': rel, 'bar_cos': cos}
    print(f'{name}: rel_l2 {e:.3e} cos {c:.8f}')
    grad_close(name, got, np.asarray(ref), rel=rel, cos=cos)


# ------------------------------------------------------------------------------------------------------------ kernels
def test_l2norm_groups_kernels():
    """rows of G matrices that sit apart in one buffer (and a zero row: the 1e-12 floor) vs F.normalize in fp64"""
    from image2text_amd import ops
    g = torch.Generator().manual_seed(3)
    G, rows, d = 5, 7, 768
    offs = torch.tensor([8, 3 * rows * d + 40, rows * d + 16, 6 * rows * d + 64, 4 * rows * d + 48], dtype=torch.int64)      # unordered, gaps
    buf = torch.randn(8 * rows * d, generator=g) * 2
    buf[int(offs[1]):int(offs[1]) + d] = 0
    x = torch.stack([buf[int(o):int(o) + rows * d].view(rows, d) for o in offs]).double().requires_grad_(True)
    gy = torch.randn(G * rows, d, generator=g)
    yr = F.normalize(x, p=2.0, dim=-1).view(G * rows, d)
    (yr * gy.double()).sum().backward()
    y, inv = torch.empty(G * rows, d, device=dev()), torch.empty(G * rows, device=dev())
    ops.l2norm_groups_fwd(buf.to(dev()), offs.to(dev()), y, inv, G, rows, d)
    assert float((y.cpu().double() - yr.detach()).abs().max()) <= 1e-6
    base = torch.randn(buf.shape, generator=g)
    for acc in (False, True):
        dx = base.clone().to(dev())
        ops.l2norm_groups_bwd(gy.to(dev()), buf.to(dev()), offs.to(dev()), inv, dx, G, rows, d, accumulate=acc)
        dx, want, touched = dx.cpu(), base.clone().double(), torch.zeros(buf.shape, dtype=torch.bool)
        for i, o in enumerate(offs.tolist()):
            want[o:o + rows * d] = (want[o:o + rows * d] if acc else 0) + x.grad[i].reshape(-1)
            touched[o:o + rows * d] = True
        touched[int(offs[1]):int(offs[1]) + d] = False                 # the zero row: the floor's gradient convention is the kernel's own
        assert torch.equal(dx[~touched & (buf != 0)], base[~touched & (buf != 0)])      # nothing outside the groups is written
        assert float((dx.double() - want)[touched].abs().max()) <= 1e-5 * max(1.0, float(want[touched].abs().max()))


def soft_problem(B, n_cls, bins, n_proj, seed):
    """a parameter buffer with the means of every (slot, resolution) at a constant slot stride, and the kernel's tables"""
    g = torch.Generator().manual_seed(seed)
    nK = len(bins)
    sizes = [n_proj * nb for nb in bins]
    moff, o = [], 24
    for sz in sizes:
        moff.append(o)
        o += sz + 40                                                    # other parameters sit between the means
    stride = o + 8
    par = torch.randn(n_cls * stride, generator=g)
    means = [[2 * torch.rand(n_proj, nb, generator=g) - 1 for nb in bins] for _ in range(n_cls)]
    for s in range(n_cls):
        for k in range(nK):
            par[s * stride + moff[k]:s * stride + moff[k] + sizes[k]] = means[s][k].reshape(-1)
    c = (torch.rand(B, n_cls, nK, n_proj, generator=g) * 1.8 - 0.9)
    koff = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    return par, means, c, moff, stride, koff


@pytest.mark.parametrize('B,n_cls,bins,n_proj', [(5, 3, (4, 8, 20), 16), (70, 2, (1, 3, 70), 6), (300, 8, (4, 8, 20), 32)],
                         ids=['fixture', 'odd-bins', 'shipped'])
def test_lsh_soft_kernels_match_fp64(B, n_cls, bins, n_proj):
    """i2t_lsh_soft_fwd / _bwd vs autograd in fp64 on the same cosines and means: z within bf16 rounding (2^-8 relative), the saved
    inverse norms, dc and dmean within fp32 rounding of sums of a few hundred terms (1e-4 of the largest entry); bins of 1, odd and
    more than 64 included"""
    from image2text_amd import ops
    par, means, c, moff, stride, koff = soft_problem(B, n_cls, bins, n_proj, seed=11)
    nK, Ktot, ncol = len(bins), int(koff[-1]), n_cls * len(bins) * n_proj
    cd = c.double().requires_grad_(True)
    md = [[m.double().requires_grad_(True) for m in row] for row in means]
    zs, invs = [], []
    for s in range(n_cls):
        parts = []
        for k, nb in enumerate(bins):
            diff = cd[:, s, k, :, None] - md[s][k][None]
            a = torch.exp(-0.5 * diff * diff / (2.0 / nb) ** 2)
            invs.append((s, k, 1.0 / a.norm(dim=-1).clamp_min(1e-12)))
            parts.append(F.normalize(a, p=2.0, dim=-1).reshape(B, -1))
        zs.append(torch.cat(parts, dim=1))
    zr = torch.stack(zs)                                                # (n_cls, B, Ktot): slot-major rows
    gz = torch.randn(n_cls, B, Ktot, generator=torch.Generator().manual_seed(12))
    (zr * gz.double()).sum().backward()
    d = dev()
    tabs = (torch.tensor(moff, dtype=torch.int64, device=d), torch.tensor(bins, dtype=torch.int32, device=d), torch.from_numpy(koff).to(d))
    z, inv = torch.empty(n_cls * B, Ktot, dtype=BF16, device=d), torch.empty(B, ncol, device=d)
    cg, pg = c.reshape(B, ncol).contiguous().to(d), par.to(d)
    ops.lsh_soft_fwd(cg, pg, stride, *tabs, z, inv, B, n_cls, nK, n_proj, Ktot)
    ez = float((z.float().cpu().double().view(n_cls, B, Ktot) - zr.detach()).abs().max())
    print('z max abs err', ez)
    assert ez <= 2.0 ** -8
    inv_c = inv.cpu().double().view(B, n_cls, nK, n_proj)
    for s, k, r in invs:
        assert float(((inv_c[:, s, k] - r.detach()) / r.detach()).abs().max()) <= 5e-5      # exponents up to ~50: a few fp32 roundings of them
    gpar0 = torch.randn(par.shape, generator=torch.Generator().manual_seed(13))
    gpar, dc, tws = gpar0.clone().to(d), torch.empty(B, ncol, device=d), torch.empty(B, ncol, device=d)
    ops.lsh_soft_bwd(gz.view(n_cls * B, Ktot).contiguous().to(d), cg, inv, pg, gpar, stride, *tabs, dc, tws, B, n_cls, nK, n_proj, Ktot)
    want_dc = cd.grad.reshape(B, ncol)
    edc = float((dc.cpu().double() - want_dc).abs().max()) / max(1.0, float(want_dc.abs().max()))
    print('dc err / scale', edc)
    assert edc <= 1e-4
    got = (gpar.cpu() - gpar0).double()
    mask = torch.zeros(par.shape, dtype=torch.bool)
    scale = max(float(m.grad.abs().max()) for row in md for m in row)
    for s in range(n_cls):
        for k, nb in enumerate(bins):
            o = s * stride + moff[k]
            mask[o:o + n_proj * nb] = True
            e = float((got[o:o + n_proj * nb] - md[s][k].grad.reshape(-1)).abs().max()) / max(1.0, scale)
            assert e <= 1e-4, (s, k, e)
    assert torch.equal(gpar.cpu()[~mask], gpar0[~mask])                 # only the means' gradient slots are written (accumulated)


# ------------------------------------------------------------------------------------------------------------ head
def head_engine(kw, head_sd):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    enc = build_encoder(kw)
    with torch.no_grad():
        for n, t in head_sd.items():
            enc.get_parameter(n).copy_(t)
    model = VisionEncoderDecoder(vit_model_config(kw), encoder=enc).to(dev()).train()
    eng = model._engine
    assert eng.enc.head == 'lsh_soft'
    return model, eng, eng.prepare(True)


def check_head(tag, eng, a, feats, ref_out, G, ref_grads):
    B = feats.shape[0]
    y, hctx = eng._vit_head_lsh_soft_fwd(feats.to(dev()), B, True)
    _, nothing = eng._vit_head_lsh_soft_fwd(feats.to(dev()), B, False)
    assert nothing is None                                              # save=False (generation, validation) keeps nothing
    scale = max(1.0, float(np.abs(ref_out).max()))
    err = float(np.abs(y.view(ref_out.shape).cpu().double().numpy() - ref_out).max())
    REPORT[f'{tag}.output'] = {'max_abs_err': err, 'tol': OUT_TOL * scale, 'ref_absmax': float(np.abs(ref_out).max())}
    print(f'{tag}.output: max abs err {err:.3e} of scale {scale:.3g}')
    assert err <= OUT_TOL * scale
    a.begin_backward()
    dfeat = eng._vit_head_lsh_soft_bwd(hctx, G.reshape(B * eng.enc.ncls, -1).to(dev()).contiguous(), B)
    assert dfeat is None
    worst = {}
    for name, r in ref_grads.items():
        leaf = name.split('.emb.', 1)[1].split('.', 1)[1]
        got = a.G(f'{eng.ep}{name}')
        close(f'{tag}.{name}', got, r, rel=GRAD_REL, cos=GRAD_COS)
        w = worst.setdefault(leaf, {'rel_l2': 0.0, 'cos': 1.0})
        w['rel_l2'], w['cos'] = max(w['rel_l2'], REPORT[f'{tag}.{name}']['rel_l2']), min(w['cos'], REPORT[f'{tag}.{name}']['cos'])
    REPORT[f'{tag}.worst'] = worst
    print(f'{tag}.worst', worst)
    assert set(worst) == {'mean', 'proj.weight', 'emb.weight'}
    return hctx


def test_head_matches_the_reference_fixture():
    """(a) output and the gradients of every proj.weight, mean and emb.weight of loss = sum(output * G) against the reference's run"""
    g = load_golden(rs.FIXTURE)
    sd, feats = fixture_state(g)
    model, eng, a = head_engine(rs.CASE, sd)
    grads = {k[len('grad.'):]: v for k, v in g.items() if k.startswith('grad.')}
    assert len(grads) == 27
    check_head('fixture', eng, a, feats, g['output'].astype(np.float64), torch.from_numpy(g['G']), grads)


def test_head_backward_is_bit_reproducible_in_deterministic_mode():
    """(c) two backward passes under i2t_set_deterministic(1): bit-equal gradients for all three parameter kinds"""
    from image2text_amd import ops
    g = load_golden(rs.FIXTURE)
    sd, feats = fixture_state(g)
    model, eng, a = head_engine(rs.CASE, sd)
    B = feats.shape[0]
    denc = torch.from_numpy(g['G']).reshape(B * eng.enc.ncls, -1).to(dev()).contiguous()
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            _, hctx = eng._vit_head_lsh_soft_fwd(feats.to(dev()), B, True)
            a.begin_backward()
            eng._vit_head_lsh_soft_bwd(hctx, denc, B)
            runs.append({n: a.G(f'{eng.ep}{n}').clone() for n in sd})
    finally:
        ops.set_deterministic(False)
    kinds = set()
    for n in sd:
        assert torch.equal(runs[0][n], runs[1][n]), n
        assert float(runs[0][n].abs().max()) > 0, n
        kinds.add(n.split('.emb.', 1)[1].split('.', 1)[1])
    assert kinds == {'mean', 'proj.weight', 'emb.weight'}
    close('deterministic.mean.vs_fixture', runs[0]['lsh_emb.1.emb.2.mean'], g['grad.lsh_emb.1.emb.2.mean'], rel=GRAD_REL, cos=GRAD_COS)


def test_head_at_the_shipped_width_matches_fp64():
    """(d) n_cls 8, 768 outputs, bins (4, 8, 20), 32 projections, B = 256 against the restatement in fp64 on the CPU.  Features and
    projection rows share an 8-dimensional subspace (plus noise), so the cosines spread over the bins (asserted below)."""
    kw = dict(n_cls=8, n_embd_out_vit=768, refine_base_model=False, lsh_config=dict(num_bins=(4, 8, 20), num_proj=32, learnable=True))
    B, g = 256, torch.Generator().manual_seed(41)
    Q = torch.randn(8, 768, generator=g)
    feats = 1.5 * (torch.randn(B, 8, generator=g) @ Q + torch.randn(B, 768, generator=g)) / 27.7
    sd = {}
    for s in range(8):
        for k, nb in enumerate((4, 8, 20)):
            q = f'lsh_emb.{s}.emb.{k}.'
            sd[q + 'proj.weight'] = (torch.randn(32, 8, generator=g) @ Q + torch.randn(32, 768, generator=g)) / 83.0
            sd[q + 'mean'] = 2 * torch.rand(1, 1, 32, nb, generator=g) - 1
            sd[q + 'emb.weight'] = torch.randn(768, 32 * nb, generator=g) / (32 * nb) ** 0.5
    sd64 = {n: t.double().requires_grad_(True) for n, t in sd.items()}
    cs = torch.cat([rs.cosines(sd64, feats.double(), s, k).detach().reshape(-1) for s in range(8) for k in range(3)])
    norms = torch.cat([rs.activations(sd64, feats.double(), s, k)[0].detach().norm(dim=-1).reshape(-1) for s in range(8) for k in range(3)])
    REPORT['shipped.inputs'] = {'std_c': float(cs.std()), 'min_norm_a': float(norms.min())}
    print('shipped inputs', REPORT['shipped.inputs'])
    assert float(cs.std()) >= 0.25 and float(norms.min()) >= 1e-6       # conditions on the inputs, as the fixture's generator asserts
    y = rs.head_lsh_learnable(sd64, feats.double(), 8)
    G = torch.randn(y.shape, generator=g)
    (y * G.double()).sum().backward()
    model, eng, a = head_engine(kw, sd)
    check_head('shipped', eng, a, feats, y.detach().numpy(), G, {n: t.grad.numpy() for n, t in sd64.items()})


# ------------------------------------------------------------------------------------------------------------ whole model
def test_train_step_optimizer_and_decoders_with_the_learnable_lsh_head(monkeypatch):
    """(b) ModelTrainerWrapper.train_step through a 2-layer backbone + the nanoGPT decoder: loss (1 %) and every trainable gradient
    (rel 0.12 / cos 0.985, the whole-model bars) against oracle.reference_model.lm_step, the oracle's encoder routed to the
    restatement for this head and pinned to the device's own backbone features: with sigma = 2 / nb the bf16 backbone's feature error
    (a few 1e-3 in a cosine) is a relative error of |c - mean| delta / sigma^2 -- tens of percent -- in the tails of the 20-bin
    activations, which is the backbone's error and not the head's (the head is checked at fixed features above)."""
    from image2text_amd.configs.trainer import TrainerWrapperConfig
    from image2text_amd.models.encoder import PretrainedViT
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    from image2text_amd.training.optim import FusedAdamW
    from image2text_amd.training.wrapper import ModelTrainerWrapper
    from oracle import reference_model as orc
    from oracle import vit as ovit
    spec = dict(image_size=32, patch_size=16, num_layers=2, num_heads=12, hidden_dim=768, mlp_dim=256)
    lc = dict(num_bins=(4, 8, 20), num_proj=32, learnable=True)
    vit_kw = dict(n_cls=8, n_embd_out_vit=128, refine_base_model=False, lsh_config=lc)
    cfg = vit_model_config(vit_kw)
    V = cfg.decoder_config.vocab_size
    tok = fake_tokenizer(V)
    old = PretrainedViT.backbone_spec
    PretrainedViT.backbone_spec = spec
    try:
        w = ModelTrainerWrapper(cfg, tok, TrainerWrapperConfig(), ignore_index=-100)
    finally:
        PretrainedViT.backbone_spec = old
    det_init_(w.model, seed=2)
    images, labels = synthetic_batch(4, 32, 16, V, seed=3)
    ep = 'encoder.0.' if w.model.has_bridge else 'encoder.'
    with torch.no_grad():       # head weights that exercise the bins: projections mixed from (approximately) this batch's features
        bsd = {k[len(ep):]: v.detach() for k, v in w.model.state_dict().items() if k.startswith(ep + 'model.')}
        hw = rs.seeded_weights(ovit.vit_backbone(bsd, images), 8, lc['num_bins'], 32, 128, seed=5)
        gm = torch.Generator().manual_seed(6)
        for n, p in w.model.named_parameters():
            if n.startswith(ep + 'lsh_emb.'):
                p.copy_(2 * torch.rand(p.shape, generator=gm) - 1 if n.endswith('.mean') else hw[n[len(ep):]])
    sd = {k: v.detach().clone() for k, v in w.model.state_dict().items()}
    w = w.to(dev()).train()
    eng = w.model._engine
    assert eng.enc.head == 'lsh_soft' and not eng.enc.refine
    osd = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items() if k != 'decoder.lm_head.weight'}
    osd['decoder.lm_head.weight'] = osd['decoder.transformer.wte.weight']
    loss, _ = w.train_step(images.to(dev()), labels.to(dev()))
    loss.backward()
    with torch.no_grad():
        dfeat = eng.vit_backbone_fwd(images.to(dev()), False)[0].cpu()
    cs = torch.cat([rs.cosines({k[len(ep):]: v for k, v in sd.items()}, dfeat, s, k).reshape(-1) for s in range(8) for k in range(3)])
    REPORT['model.inputs'] = {'std_c': float(cs.std())}
    assert float(cs.std()) >= 0.25
    monkeypatch.setattr(ovit, 'vit_backbone', lambda sd_, images_, spec=None, pfx='model.': dfeat)
    monkeypatch.setattr(ovit, 'pretrained_vit', rs.pretrained_vit(ovit.pretrained_vit))
    oloss = orc.lm_step(osd, cfg, images, labels, tok, training=True)
    oloss.backward()
    REPORT['model.loss'] = {'got': float(loss.detach()), 'ref': float(oloss)}
    print('model.loss', REPORT['model.loss'])
    assert abs(float(loss.detach()) - float(oloss)) <= 1e-2 * float(oloss)
    n_checked = n_none = n_head = 0
    for name, p in w.model.named_parameters():
        ref = osd[name].grad if name in osd else None
        if name.startswith(eng.ep + 'model.'):
            assert p.grad is None and ref is None, name                 # the frozen backbone: .grad stays None
            n_none += 1
            continue
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        if ref is None:
            assert float(p.grad.abs().max()) == 0.0, name
            continue
        close(f'model.{name}', p.grad, ref.numpy(), rel=0.12, cos=0.985)
        n_checked += 1
        n_head += name.startswith(eng.ep + 'lsh_emb.')
    assert n_head == 72 and n_checked > n_head and n_none >= 20
    before = {n: p.detach().clone() for n, p in w.model.named_parameters()}
    opt = FusedAdamW(w.model.parameters(), w.model, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.1)
    opt.step()
    opt.zero_grad()
    for n, p in w.model.named_parameters():
        moved = not torch.equal(p.detach(), before[n])
        frozen = n.startswith(eng.ep + 'model.') or not p.requires_grad
        assert moved != frozen or float(before[n].abs().max()) == 0.0, (n, moved, frozen)
    w.eval()
    prompt = torch.full((4, 1), tok.bos_token_id, dtype=torch.long)
    ids = w.model.generate(images.to(dev()), prompt.to(dev()), max_new_tokens=6, top_k=1)
    assert ids.shape == (4, 7)
    torch.manual_seed(0)
    ids = w.model.generate(images.to(dev()), prompt.to(dev()), max_new_tokens=6, temperature=0.9, top_k=5)
    assert ids.shape == (4, 7) and int(ids.min()) >= 0 and int(ids.max()) < V
    gen = BeamSearchTokenGenerator(w.model, beam_width=3, temperature=0.0, max_new_tokens=6, no_repeat_n_grams=(2, 3), beam_expansion_factor=4,
                                   consolidation_temperature=0.0, kv_cache=True)
    bids, scores = gen(images.to(dev()), prompt.to(dev()))
    assert bids.shape[:2] == (4, 3) and bool((scores[:, :-1] >= scores[:, 1:]).all())
