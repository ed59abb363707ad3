"""TEST INFRASTRUCTURE ONLY: a plain-PyTorch restatement of the learnable LSH head (``lsh_config.learnable: True``; reference
models/layers.py:147-219 used through models/encoder.py:117) as pure functions over a state dict, in whatever dtype the state dict
and the features carry (fp32 against the fixture, fp64 as the yardstick of the shipped-width case).  Pinned to the reference by
tests/test_lsh_learnable_cpu.py on tests/golden/vit_head_lsh_learnable.npz (tools/gen_goldens_lsh_learnable.py).

Per slot s and resolution k (nb bins, P projections), feature x:
    c = normalize(x) @ normalize(proj.weight, dim=-1).T                  (B, P)
    a = exp(-0.5 (c[..., None] - mean)^2 / (2 / nb)^2)                   (B, P, nb)
    z = a / max(||a||_2 over the bins, 1e-12)
    y_s += z.view(B, P nb) @ emb.weight.T
"""
import torch
import torch.nn.functional as F

FIXTURE = 'vit_head_lsh_learnable.npz'
CASE = dict(n_cls=3, n_embd_out_vit=32, refine_base_model=True, lsh_config=dict(num_bins=(4, 8, 20), num_proj=16, learnable=True))
WEIGHT_SEED = 77


def cosines(sd, feat, slot: int, k: int, pfx: str = 'lsh_emb.'):
    w = sd[f'{pfx}{slot}.emb.{k}.proj.weight']
    return F.normalize(feat, p=2.0, dim=-1) @ F.normalize(w, p=2.0, dim=-1).t()


def activations(sd, feat, slot: int, k: int, pfx: str = 'lsh_emb.'):
    """-> (a, z): the Gaussian bin activations (B, P, nb) before and after the L2 normalisation over the bins"""
    mean = sd[f'{pfx}{slot}.emb.{k}.mean']
    P, nb = mean.shape[-2], mean.shape[-1]
    diff = cosines(sd, feat, slot, k, pfx).unsqueeze(-1) - mean.reshape(1, P, nb)
    a = torch.exp(-0.5 * diff * diff / (2.0 / nb) ** 2)
    return a, F.normalize(a, p=2.0, dim=-1)


def head_lsh_learnable(sd, feat, n_cls: int, pfx: str = 'lsh_emb.'):
    """-> (B, n_cls, out)"""
    outs = []
    for s in range(n_cls):
        acc, k = None, 0
        while f'{pfx}{s}.emb.{k}.emb.weight' in sd:
            _, z = activations(sd, feat, s, k, pfx)
            y = z.reshape(z.shape[0], -1) @ sd[f'{pfx}{s}.emb.{k}.emb.weight'].t()
            acc = y if acc is None else acc + y
            k += 1
        outs.append(acc)
    return torch.stack(outs, dim=1)


def pretrained_vit(original):
    """``oracle.vit.pretrained_vit`` with the learnable LSH case routed here (the oracle refuses it); everything else is the oracle's."""
    from oracle import vit as ovit

    def run(sd, cfg, images=None, spec=None, features=None, trace=None):
        if cfg.peer_config is None and cfg.lsh_config is not None and cfg.lsh_config.learnable:
            if features is None:
                with torch.no_grad():                              # LSH forces refine off (encoder.py:73)
                    features = ovit.vit_backbone(sd, images, spec)
            return head_lsh_learnable(sd, features, cfg.n_cls)
        return original(sd, cfg, images, spec, features, trace)
    return run


def seeded_weights(features, n_cls: int, num_bins, n_proj: int, out: int, seed: int = WEIGHT_SEED):
    """The fixture's proj.weight / emb.weight, regenerated instead of stored.  Cosines of random 768-vectors are ~ +-0.04, where the
    head is nearly constant in x: every projection row is a random mixture of the normalised FEATURE rows plus unit-norm noise, which
    spreads its cosines over the bins (std(c) ~ 0.35).  emb.weight ~ N(0, 1 / fan_in).  -> {'lsh_emb.s.emb.k.<leaf>': tensor}"""
    g = torch.Generator().manual_seed(seed)
    xn = F.normalize(features.float(), p=2.0, dim=-1)
    d, out_sd = features.shape[1], {}
    for s in range(n_cls):
        for k, nb in enumerate(num_bins):
            mix = torch.randn(n_proj, features.shape[0], generator=g)
            noise = torch.randn(n_proj, d, generator=g) / d ** 0.5
            out_sd[f'lsh_emb.{s}.emb.{k}.proj.weight'] = 0.5 * (mix @ xn + noise)
            out_sd[f'lsh_emb.{s}.emb.{k}.emb.weight'] = torch.randn(out, n_proj * nb, generator=g) / (n_proj * nb) ** 0.5
    return out_sd
