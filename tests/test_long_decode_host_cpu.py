"""Host side of decoding past 1024 cached keys: which cache a call gets (decoding.cache_plan), the numpy statement of the
split-key attention and its combine against a one-pass fp64 softmax, and the workspace formula.  No library, no device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from image2text_amd import ops
from image2text_amd.decoding import (DECODE_LONG_MAX_KEYS, DECODE_MAX_KEYS, LONG_CHUNK_KEYS, LONG_HEAD_DIMS, GreedyDecoder, cache_plan,
                                     decode_window, split_attention_host, takes_long_cache, text_window)

CH = LONG_CHUNK_KEYS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_copies_match_the_header():
    """ops.LONG_CHUNK_KEYS and decoding.DECODE_LONG_MAX_KEYS are the values csrc/common.h compiles in"""
    src = open(os.path.join(ROOT, 'image2text_amd', 'csrc', 'common.h')).read()
    chunk = re.search(r'^#ifndef LONG_CHUNK_KEYS\n#define LONG_CHUNK_KEYS (\d+)\n#endif', src, flags=re.M)
    cap = re.search(r'^constexpr int DECODE_LONG_MAX_KEYS = (\d+);', src, flags=re.M)
    assert chunk and cap
    assert int(chunk.group(1)) == ops.LONG_CHUNK_KEYS == CH and int(cap.group(1)) == DECODE_LONG_MAX_KEYS == 32768
    assert CH % 64 == 0 and 64 <= CH <= DECODE_MAX_KEYS                 # csrc/common.h's static_assert


def _decoder(hd, block=4096, ncls=8):
    """GreedyDecoder over a stub of what its cache routing reads: a prefixed Llama-family decoder with heads of ``hd`` (None: dense)"""
    dec = SimpleNamespace(block=block, prefixed=hd is not None, llama=None if hd is None else SimpleNamespace(hd=hd))
    eng = SimpleNamespace(enc=SimpleNamespace(ncls=ncls), dec=dec)
    return GreedyDecoder(SimpleNamespace(_engine=eng, config=SimpleNamespace(use_soft_prompting=True)))


def test_only_heads_the_split_kernels_are_built_for_take_the_long_cache():
    """the plugins accept heads of 16 and 32 too (block 4096 whatever the width): such a decoder keeps the classic window and its
    refusal, as does every decoder that is not of the Llama family"""
    assert LONG_HEAD_DIMS == (64, 128)
    assert [takes_long_cache(SimpleNamespace(hd=hd)) for hd in (16, 32, 64, 128)] == [False, False, True, True]
    assert not takes_long_cache(None)
    for hd in (64, 128):
        d = _decoder(hd)
        assert d._cache_args() == (4096, 8, 8, True) and decode_window(*d._cache_args()) == 4088
        assert cache_plan(*d._cache_args()[:3], 1100, d._cache_args()[3])[1] is True
    built = []
    for hd, prefix in ((16, 8), (32, 8), (None, 0)):
        d = _decoder(hd)
        assert d._cache_args() == (4096, 8, prefix, False) and decode_window(*d._cache_args()) == 1024 - prefix
        for total in (1024 - prefix + 1, 1100, 4000):
            with pytest.raises(ValueError, match=rf'prompt \+ new tokens \({total}\) exceed the text window \({1024 - prefix}\)$'):
                d._state_for(2, total, built.append)
        assert d._state is None and d._long_state is None and not built          # refused before any buffer is made


@pytest.mark.parametrize('llama', [False, True])
def test_cache_plan_keeps_the_classic_window(llama):
    """every tuple of test_host_cpu.py::test_decode_text_window_keeps_the_attention_key_bound: a total that fits gets today's cache"""
    for block, off, prefix in ((1024, 0, 0), (1024, 197, 0), (4096, 0, 0), (4096, 197, 197), (64, 8, 8)):
        tmax = text_window(block, off, prefix)
        for total in (1, tmax - 1, tmax):
            if total >= 1:
                assert cache_plan(block, off, prefix, total, llama) == (tmax + prefix, False)
    for block, off, prefix in ((2048, 1024, 1024), (4096, 1100, 1100)):          # no room in the classic window at all
        if not llama:
            with pytest.raises(ValueError, match='at most 1024 keys'):
                cache_plan(block, off, prefix, 1, llama)


def test_cache_plan_long():
    clen, long = cache_plan(4096, 8, 8, 1100, True)
    assert long and clen % CH == 0 and clen >= 1108 and clen - CH < 1108
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(1100\) exceed the text window \(1016\)') as e:
        cache_plan(4096, 8, 8, 1100, False)
    assert str(e.value) == 'prompt + new tokens (1100) exceed the text window (1016)'
    # the first total past the classic window, and the last one of the model's
    assert cache_plan(4096, 8, 8, 1016, True) == (1024, False)
    assert cache_plan(4096, 8, 8, 1017, True) == (-(-1025 // CH) * CH, True)
    assert cache_plan(4096, 8, 8, 4088, True) == (4096, True)
    assert cache_plan(4100, 8, 8, 4092, True) == (4100, True)                    # the model's window is no multiple of the chunk
    with pytest.raises(ValueError, match=r'prompt \+ new tokens \(4089\) exceed the text window \(4088\)$'):
        cache_plan(4096, 8, 8, 4089, True)
    # a Llama-family block inside the classic window: the same refusal whether or not the decoder takes the long cache
    for llama in (False, True):
        with pytest.raises(ValueError, match=r'prompt \+ new tokens \(121\) exceed the text window \(120\)$'):
            cache_plan(128, 8, 8, 121, llama)
    # a cached prompt that fills the classic window leaves room in the long one
    assert cache_plan(4096, 1100, 1100, 10, True) == (-(-1110 // CH) * CH, True)
    # the cap
    big = 1 << 20
    assert cache_plan(big, 0, 0, DECODE_LONG_MAX_KEYS, True) == (DECODE_LONG_MAX_KEYS, True)
    assert cache_plan(big, 8, 8, DECODE_LONG_MAX_KEYS - 8, True) == (DECODE_LONG_MAX_KEYS, True)
    with pytest.raises(ValueError, match=rf'exceed the text window \({DECODE_LONG_MAX_KEYS - 8}\)'):
        cache_plan(big, 8, 8, DECODE_LONG_MAX_KEYS - 7, True)
    with pytest.raises(ValueError, match='text window'):
        cache_plan(big, 8, 8, DECODE_LONG_MAX_KEYS - 7, False)


def _one_pass(q, k, v, scale):
    s = (k @ q) * scale
    p = np.exp(s - s.max())
    return (p / p.sum()) @ v


def test_split_attention_host_is_the_softmax():
    """n on both sides of every chunk boundary of a 4-chunk row; rows whose maximum sits in the first, a middle and the last chunk"""
    rng = np.random.default_rng(0)
    hd, chunk = 16, 32
    counts = sorted({1, 2} | {c * chunk + d for c in (1, 2, 3, 4) for d in (-1, 0, 1)})
    worst = 0.0
    for n in counts:
        k, v = rng.standard_normal((n, hd)), rng.standard_normal((n, hd))
        for qscale in (0.0, 1.0, 8.0):
            q = rng.standard_normal(hd) * qscale
            for win in (None, 0, n // 2, n - 1):           # a planted winner: chunk 0, a middle chunk, the last live chunk
                kk = k.copy()
                if win is not None:
                    kk[win] = 3.0 * q / max(np.linalg.norm(q), 1e-9) * np.sqrt(hd)
                got, want = split_attention_host(q, kk, v, hd ** -0.5, chunk), _one_pass(q, kk, v, hd ** -0.5)
                worst = max(worst, float(np.abs(got - want).max()))
                if win is not None and qscale == 8.0:
                    assert int(np.argmax(kk @ q)) == win
    print(f'split_attention_host vs one-pass fp64 softmax: worst abs error {worst:.3g} (bound 1e-12)')
    assert worst <= 1e-12
    # the package's chunk size, a row of 4 chunks and a bit
    n = 4 * CH + 3
    q, k, v = rng.standard_normal(hd), rng.standard_normal((n, hd)), rng.standard_normal((n, hd))
    assert np.abs(split_attention_host(q, k, v, 0.25) - _one_pass(q, k, v, 0.25)).max() <= 1e-12


def test_workspace_formula():
    f = ops.gq_decode_long_workspace_floats
    assert f(1, 1, 1, 64) == 66 and f(1, 1, CH, 64) == 66 and f(1, 1, CH + 1, 64) == 132
    assert f(2, 71, 9 * CH, 64) == 2 * 71 * 9 * 66
    assert f(8, 32, 4096, 128) == 8 * 32 * (-(-4096 // CH)) * 130
    assert f(3, 12, DECODE_LONG_MAX_KEYS, 128) == 3 * 12 * (DECODE_LONG_MAX_KEYS // CH) * 130
