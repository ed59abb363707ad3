"""The learnable LSH head (``lsh_config.learnable: True``) without a GPU: the test-local restatement (tests/lsh_learnable_ref.py)
against the reference's fixture, and the module tree ``Encoder.from_config`` builds for the flag."""
import os

import numpy as np
import torch
import yaml

import lsh_learnable_ref as rs
from conftest import GOLDEN, load_golden
from image2text_amd.configs.models import PretrainedViTConfig

os.environ.setdefault('I2T_VIT_B16_CHECKPOINT', 'random')
SPEC = dict(image_size=32, patch_size=16, num_layers=1, num_heads=12, hidden_dim=768, mlp_dim=64)


def fixture_state(g):
    """the fixture's head weights: the stored means + the regenerated proj.weight / emb.weight"""
    lc = rs.CASE['lsh_config']
    feats = torch.from_numpy(g['features'])
    sd = rs.seeded_weights(feats, rs.CASE['n_cls'], lc['num_bins'], lc['num_proj'], rs.CASE['n_embd_out_vit'])
    sd.update({k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')})
    return sd, feats


def fixture_keys(g):
    out = []
    for row in g['keys']:
        name, shape = str(row).split(' ')
        out.append((name, tuple(int(v) for v in shape.split(','))))
    return out


def build_encoder(kw, spec=SPEC):
    from image2text_amd.models.encoder import Encoder, PretrainedViT
    old = PretrainedViT.backbone_spec
    PretrainedViT.backbone_spec = spec
    try:
        return Encoder.from_config(PretrainedViTConfig.model_validate(kw))
    finally:
        PretrainedViT.backbone_spec = old


def test_restatement_reproduces_the_reference_fixture():
    g = load_golden(rs.FIXTURE)
    sd, feats = fixture_state(g)
    assert sorted(sd) == sorted(n for n, _ in fixture_keys(g))
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    y = rs.head_lsh_learnable(sd, feats, rs.CASE['n_cls'])
    err = float((y.detach() - torch.from_numpy(g['output'])).abs().max())
    print('output max abs err', err)
    assert err <= 2e-5
    (y * torch.from_numpy(g['G'])).sum().backward()
    for name, t in sd.items():
        e = float((t.grad - torch.from_numpy(g[f'grad.{name}'])).abs().max())
        print(name, 'grad max abs err', e)
        assert e <= 2e-5, name
    # the conditions the generator asserted on the inputs hold for what the tests regenerate
    cs = torch.cat([rs.cosines(sd, feats, s, k).detach().reshape(-1) for s in range(3) for k in range(3)])
    norms = torch.cat([rs.activations(sd, feats, s, k)[0].detach().norm(dim=-1).reshape(-1) for s in range(3) for k in range(3)])
    assert float(cs.std()) >= 0.25 and float(norms.min()) >= 1e-6


def test_module_tree_has_the_reference_keys_and_shapes():
    g = load_golden(rs.FIXTURE)
    enc = build_encoder(rs.CASE)
    got = [(n, tuple(t.shape)) for n, t in enc.state_dict().items() if n.startswith('lsh_emb.')]
    assert got == fixture_keys(g)
    params = dict(enc.named_parameters())
    for n, _ in got:
        assert params[n].requires_grad, n
    assert enc.refine is False                                   # LSH forces the backbone frozen (encoder.py:73)
    for comp in enc.lsh_emb:
        for mod, nb in zip(comp.emb, rs.CASE['lsh_config']['num_bins']):
            assert mod.top_k is None and abs(mod.sigma2 - (2.0 / nb) ** 2) < 1e-15
            assert float(mod.mean.detach().min()) >= -1.0 and float(mod.mean.detach().max()) <= 1.0      # 2 U(0, 1) - 1


def test_nano_yaml_encoder_builds_with_the_flag_flipped():
    with open(os.path.join(GOLDEN, 'training_configs', 'local', 'nano.yaml')) as fh:
        doc = yaml.safe_load(fh)

    def find(node):
        if isinstance(node, dict):
            if 'lsh_config' in node and isinstance(node['lsh_config'], dict):
                return node
            for v in node.values():
                r = find(v)
                if r is not None:
                    return r
        return None
    ecfg = find(doc)
    assert ecfg is not None and ecfg['lsh_config']['learnable'] is False
    ecfg = dict(ecfg, lsh_config=dict(ecfg['lsh_config'], learnable=True))
    enc = build_encoder(ecfg)
    lc = ecfg['lsh_config']
    names = {n for n, _ in enc.named_parameters()}
    for s in range(ecfg['n_cls']):
        for k, nb in enumerate(lc['num_bins']):
            q = f'lsh_emb.{s}.emb.{k}.'
            assert {q + 'mean', q + 'proj.weight', q + 'emb.weight'} <= names
            assert tuple(enc.lsh_emb[s].emb[k].emb.weight.shape) == (ecfg['n_embd_out_vit'], lc['num_proj'] * nb)


def test_refusals_name_their_reason():
    import pytest
    from image2text_amd.models.layers import LearnableCosineVectorEmbedding
    with pytest.raises(NotImplementedError, match='top_k'):
        LearnableCosineVectorEmbedding(768, 32, n_proj=16, num_bins=20, top_k=4)
    with pytest.raises(NotImplementedError, match='multiples of 32'):
        build_encoder(dict(rs.CASE, lsh_config=dict(num_bins=(4, 8, 20), num_proj=6, learnable=True)))
