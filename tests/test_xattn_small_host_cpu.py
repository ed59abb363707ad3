"""The routing rule of a decoder block's cross-attention forward (engine.xattn_route): which of the LoRA, fused and un-fused forms
runs, for every combination of its inputs.  No GPU."""
import itertools

import pytest

from image2text_amd.engine import xattn_route

S_VALUES = (8, 16, 24, 32, 64, 257)
# (H, d): even heads of 64 | odd head count | d != 64 H (heads of 32) | d != 64 H (heads of 128)
SHAPES = ((2, 128), (12, 768), (3, 192), (1, 64), (4, 128), (2, 256))
CASES = list(itertools.product(S_VALUES, SHAPES, (False, True), (False, True), (False, True), (False, True)))


def _old_rule(S, H, d, fused, lora, precise):
    """engine.py's if / elif / else before the helper existed, written out literally."""
    if lora:
        return 'lora'
    elif fused and S == 64 and H % 2 == 0 and d == 64 * H and not precise:
        return 'fused'
    else:
        return 'unfused'


@pytest.mark.parametrize('S,shape,fused,small,lora,precise', CASES)
def test_route(S, shape, fused, small, lora, precise):
    H, d = shape
    got = xattn_route(S, H, d, fused, small, lora, precise)
    assert got in ('lora', 'fused', 'unfused')
    if not small:
        assert got == _old_rule(S, H, d, fused, lora, precise)      # switch off: today's routing, whatever the inputs
        return
    if lora:
        assert got == 'lora'                                        # an adapted K/V projection never fuses
    elif fused and not precise and H % 2 == 0 and d == 64 * H and S in (8, 16, 32, 64):
        assert got == 'fused'
    else:
        assert got == 'unfused'                                     # S = 24 (64 % S != 0), S = 257 (> 64), odd H, d != 64 H, precise, I2T_XATTN_FUSED=0


def test_the_switch_only_adds_the_three_small_sizes():
    """Across all cases the two settings of the switch differ exactly where S is 8 / 16 / 32 and every other condition holds."""
    moved = {(S, shape) for S, shape, fused, small, lora, precise in CASES
             if xattn_route(S, *shape, fused, True, lora, precise) != xattn_route(S, *shape, fused, False, lora, precise)}
    assert moved == {(S, shape) for S in (8, 16, 32) for shape in ((2, 128), (12, 768))}


def test_the_switch_is_read_from_the_environment(monkeypatch):
    """HotPath reads I2T_XATTN_FUSED_SMALL next to I2T_XATTN_FUSED when a model is built: '1' turns it on, anything else leaves it off."""
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import tiny_config
    monkeypatch.delenv('I2T_XATTN_FUSED', raising=False)
    for value, want in ((None, False), ('0', False), ('1', True)):
        if value is None:
            monkeypatch.delenv('I2T_XATTN_FUSED_SMALL', raising=False)
        else:
            monkeypatch.setenv('I2T_XATTN_FUSED_SMALL', value)
        eng = VisionEncoderDecoder(tiny_config())._engine
        assert eng.xattn_fused_small is want and eng.xattn_fused is True
