"""Host-side pieces of the KV-cache beam search (no GPU): the uniform replica of csrc/beam.hip and the generator's switch."""
import pytest
import torch

from image2text_amd import rng
from image2text_amd.synth import tiny_config


def _uniform_scalar(seed, step, row, index, salt):
    """csrc/beam.hip::beam_uniform restated on python integers, one element"""
    m = rng.M32
    h2 = rng.lowbias32(rng.lowbias32((seed & m) ^ ((row * 0x9E3779B9) & m)) + ((seed >> 32) & m) + step * 0x85EBCA6B + salt * 0x27D4EB2F)
    h = rng.lowbias32((h2 + index * 0x165667B1) & m)
    return ((h >> 9) + 0.5) / 2 ** 23


def test_beam_uniform_replica():
    seed = 0xDEADBEEF12345678
    idx = torch.arange(0, 151936, 997)
    u = rng.beam_uniform(seed, 17, 5, idx, 0)
    assert u.dtype == torch.float64 and bool(((u > 0) & (u < 1)).all())
    assert u.tolist() == [_uniform_scalar(seed, 17, 5, int(i), 0) for i in idx]
    assert torch.equal(u.float().double(), u), 'every value is exact in fp32'
    assert not torch.equal(u, rng.beam_uniform(seed, 17, 5, idx, 1)) and not torch.equal(u, rng.beam_uniform(seed, 18, 5, idx, 0))
    assert not torch.equal(u, rng.beam_uniform(seed, 17, 6, idx, 0)) and not torch.equal(u, rng.beam_uniform(seed + 1, 17, 5, idx, 0))
    big = rng.beam_uniform(7, 3, 0, torch.arange(200000), 0)
    assert abs(big.mean().item() - 0.5) < 5e-3 and big.unique().numel() > 190000


def test_generator_kv_cache_switch(monkeypatch):
    from image2text_amd.decoding import BeamSpec
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    m = VisionEncoderDecoder(tiny_config())
    monkeypatch.delenv('I2T_BEAM_KV_CACHE', raising=False)
    gen = BeamSearchTokenGenerator(m, beam_width=2, beam_expansion_factor=3, eos_token_id=5, length_boost=2.0, no_repeat_n_grams=(2,))
    assert not gen.uses_kv_cache()
    monkeypatch.setenv('I2T_BEAM_KV_CACHE', '1')
    assert gen.uses_kv_cache()
    assert not BeamSearchTokenGenerator(m, kv_cache=False).uses_kv_cache()
    monkeypatch.setenv('I2T_BEAM_KV_CACHE', '0')
    assert BeamSearchTokenGenerator(m, kv_cache=True, seed=3).uses_kv_cache()
    spec = gen.beam_spec()
    assert spec == BeamSpec(2, 3, 1.0, None, 1.0, 5, pytest.approx(0.6931471805599453), (2,))
