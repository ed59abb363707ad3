"""i2t_kv_prefill on the MI355X: the K / V rows of a forward pass into the decode cache, both layouts, N cache rows per
image.  It is a copy: tolerance 0.  The source holds a distinct 16-bit pattern per (row, column) in packed q | k | v rows wider than
k | v; the caches start as a sentinel pattern no source element has, with guard elements before and behind each buffer.  Every slot in
range must equal ``kv_prefill_host`` (decoding.py, numpy), every other element of caches and guards the sentinel, the N rows of an
image each other; every refusal returns an error and writes nothing."""
import numpy as np
import pytest
import torch

from image2text_amd.decoding import kv_prefill_host

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENTINEL = -21846           # 0xAAAA as int16: above every source pattern below
GUARD = 64                  # elements (128 bytes) on either side of a cache: keeps the cache base 16-byte aligned


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def _source(rows, src_ld):
    n = rows * src_ld
    assert n < 0xAAAA, 'the source patterns must stay distinct and below the sentinel'
    return torch.arange(n, dtype=torch.int32).to(torch.int16).view(rows, src_ld)


def _guarded(n):
    """-> (int16 buffer [GUARD | n | GUARD] of sentinels on the device, its bf16 view of the middle n elements)"""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int16, device=dev())
    return buf, buf[GUARD:GUARD + n].view(BF16)


def _run_and_check(ops, src, k_off, v_off, src_T, src_t0, m, R, cache_bs, cache_rs, cache_hs, hd, w, slot0, B, N):
    kbuf, kc = _guarded(R * cache_bs)
    vbuf, vc = _guarded(R * cache_bs)
    ops.kv_prefill(src.to(dev()).view(BF16), src.shape[1], k_off, v_off, src_T, src_t0, m, kc, vc, cache_bs, cache_rs, cache_hs, hd, w, slot0, B, N)
    torch.cuda.synchronize()
    want_k, want_v = (np.full(R * cache_bs, SENTINEL, dtype=np.int16) for _ in range(2))
    kv_prefill_host(src.numpy(), k_off, v_off, src_T, src_t0, m, want_k, want_v, cache_bs, cache_rs, cache_hs, hd, w, slot0, B, N)
    assert int((want_k != SENTINEL).sum()) == B * N * m * w == int((want_v != SENTINEL).sum())          # the host rule wrote every slot in range
    for name, buf, want in (('K', kbuf, want_k), ('V', vbuf, want_v)):
        got = buf.cpu()
        assert bool((got[:GUARD] == SENTINEL).all()) and bool((got[-GUARD:] == SENTINEL).all()), f'{name}: a guard element was written'
        # slots in range equal the host rule; everything else in the cache is still the sentinel (the host array holds it there)
        assert torch.equal(got[GUARD:-GUARD], torch.from_numpy(want)), f'{name} cache differs from kv_prefill_host'
        rows = got[GUARD:GUARD + B * N * cache_bs].view(B, N, cache_bs)
        for n in range(1, N):
            assert torch.equal(rows[:, n], rows[:, 0]), f'{name}: row {n} of an image differs from its row 0'
    return kbuf, vbuf


@pytest.mark.parametrize('B,N,H,m,clen,slot0,src_T,src_t0', [(3, 2, 2, 5, 37, 0, 5, 0), (2, 3, 12, 1, 40, 3, 9, 4), (1, 1, 2, 37, 37, 0, 37, 0)],
                         ids=['b3n2', 'one_token_12_heads', 'full_cache'])
def test_head_major(ops, B, N, H, m, clen, slot0, src_T, src_t0):
    """[R][H][clen][64] (the dense decoder's cache): packed q | k | v rows of width 3 d; one cache row more than B * N, never written"""
    d = 64 * H
    R = B * N + 1
    _run_and_check(ops, _source(B * src_T, 3 * d), d, 2 * d, src_T, src_t0, m, R, clen * d, 64, clen * 64, 64, d, slot0, B, N)


@pytest.mark.parametrize('Hkv,hd', [(1, 64), (2, 128), (4, 64)], ids=['mqa_64', 'gqa_2x128', 'gqa_4x64'])
def test_row_major(ops, Hkv, hd):
    """[R][clen][Hkv hd] (the Llama family's cache): packed rows of 2 Hkv query heads | Hkv key heads | Hkv value heads"""
    B, N, m, clen, slot0, src_T, src_t0 = 3, 2, 5, 21, 4, 7, 1
    w = Hkv * hd
    _run_and_check(ops, _source(B * src_T, 4 * w), 2 * w, 3 * w, src_T, src_t0, m, B * N + 1, clen * w, w, hd, hd, w, slot0, B, N)


def test_refusals_write_nothing(ops):
    from image2text_amd.lib import I2TError
    B, N, H, m, clen, src_T = 2, 2, 2, 3, 8, 4
    d = 64 * H
    src = _source(B * src_T, 3 * d).to(dev()).view(BF16)
    kbuf, kc = _guarded(B * N * clen * d)
    vbuf, vc = _guarded(B * N * clen * d)
    # the good call, as keyword arguments: every refusal below changes one or two of them
    good = dict(src=src, src_ld=3 * d, k_off=d, v_off=2 * d, src_T=src_T, src_t0=0, m=m, kcache=kc, vcache=vc, cache_bs=clen * d, cache_rs=64,
                cache_hs=clen * 64, hd=64, w=d, slot0=0, B=B, N=N)
    row_major = dict(cache_rs=d, cache_hs=64)
    odd = src.view(-1)[8:8 + 2 * 3 * d + 4].view(-1)                # a source whose rows are 3 d + 2 apart: src_ld % 8 != 0
    cases = [
        (dict(src=None), 'null pointer'), (dict(kcache=None), 'null pointer'), (dict(vcache=None), 'null pointer'),
        (dict(w=d - 4, hd=4), 'w = 124'), (dict(hd=4), 'hd = 4'), (dict(hd=48), 'hd = 48'),
        (dict(src=odd, src_ld=3 * d + 2, src_T=1, m=1, B=2), 'src_ld = 386'),
        (dict(k_off=d + 4), 'k_off = 132'), (dict(v_off=2 * d + 8), 'inside src_ld'),
        (dict(src=src.view(-1)[1:]), 'misaligned base'), (dict(kcache=kc.view(-1)[4:]), 'misaligned base'),
        (dict(vcache=vc.view(-1)[1:]), 'misaligned base'), (dict(cache_bs=clen * d + 4), 'cache strides'),
        (dict(m=0), 'm = 0'), (dict(m=-2), 'm = -2'), (dict(B=0), 'B = 0'), (dict(N=0), 'N = 0'),
        (dict(src_t0=2), r'src_t0 \+ m = 2 \+ 3 exceeds src_T = 4'), (dict(src_t0=-1), 'exceeds src_T'), (dict(m=src_T + 1), 'exceeds src_T'),
        (dict(slot0=clen - m + 1), r'slot0 \+ m = 6 \+ 3 exceeds the slots'), (dict(slot0=-1), 'exceeds the slots'),
        (dict(slot0=clen - m + 1, **row_major), 'exceeds the slots'), (dict(cache_bs=(clen - 1) * d, slot0=clen - m, **row_major), 'exceeds the slots'),
        (dict(cache_hs=clen * 64 - 64, slot0=clen - m), 'exceeds the slots'),          # a head's run one slot short
        (dict(cache_bs=clen * d - 64), 'exceeds the slots'),                           # a cache row that does not hold H runs
    ]
    for change, msg in cases:
        with pytest.raises(I2TError, match=msg):
            ops.kv_prefill(**{**good, **change})
    torch.cuda.synchronize()
    assert bool((kbuf == SENTINEL).all()) and bool((vbuf == SENTINEL).all()), 'a refused call wrote to a cache'
    ops.kv_prefill(**good)                                            # ... and the good call is accepted, in both layouts
    ops.kv_prefill(**{**good, **row_major})
    torch.cuda.synchronize()
    assert bool((kbuf[:GUARD] == SENTINEL).all()) and bool((kbuf[-GUARD:] == SENTINEL).all()) and int((kbuf != SENTINEL).sum()) > 0
