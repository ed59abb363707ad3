"""i2t_mem_decode_attention / i2t_mem_gq_decode_attention through ops.mem_decode_attention / ops.mem_gq_decode_attention:
cross-attention of R query rows over a memory stored once per image, row r over memory row mem_index[r].

R = 5 rows over n_mem = 3 memory rows, mem_index = [2, 0, 2, 1, 0] (a duplicate, every row used, not sorted); n_keys 1 (a single
key), 8 (one group of 8 lanes-per-key keys), 33 (a partial 32-key trip), 64 (the default memory), 257 (ViT-B/16's).  Each case is held
  * against the float64 statement below, with the per-element bound of tests/attention_ref.py::forward -- the derivation
    tests/test_attention_kernels_gpu.py uses, on one query row per sequence.  That bound allows for a bf16 rounding of P, which these
    kernels do not make (P stays fp32), so it is not tight here, only valid: what it has to cover are the fp32 terms and the bf16
    store.  Condition (ii) of that file is asserted too: the median bound is at most a quarter of the reference's rms;
  * BIT for bit against ops.decode_attention / ops.gq_decode_attention on the host-gathered memory kv[mem_index];
  * BIT for bit, with mem_index[r] = r // W, against ops.beam_decode_attention / ops.beam_gq_decode_attention(rows_per_mem=W).
Guard rows behind the output and guard words behind mem_index come back untouched; the host refusals return -1 with a message.  The
index values are the caller's to validate: every table built here is checked against n_mem on the host before it is uploaded."""
import numpy as np
import pytest
import torch

import attention_ref
from test_row_kernels_gpu import BF16, F64, SENT, check, dev, refused

pytestmark = pytest.mark.gpu

R, N_MEM, MEM_INDEX = 5, 3, [2, 0, 2, 1, 0]
N_KEYS = [1, 8, 33, 64, 257]
GUARD_ROWS, GUARD_WORDS, GUARD_WORD = 2, 3, 0x7FFFFFF0
II_MAX = 0.25


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device=dev()).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev()) * scale).to(BF16)


def table(index, n_mem):
    """the row -> memory-row table on the device behind GUARD_WORDS guard words; validated HERE, on the host, before the upload"""
    index = np.asarray(index, dtype=np.int64)
    assert index.min() >= 0 and index.max() < n_mem, 'no out-of-range index is ever sent to the device'
    buf = torch.full((len(index) + GUARD_WORDS,), GUARD_WORD, dtype=torch.int32, device=dev())
    buf[:len(index)] = torch.from_numpy(index.astype(np.int32)).to(dev())
    return buf, buf[:len(index)]


def guarded_out(rows, width):
    buf = torch.full((rows + GUARD_ROWS, width), SENT, dtype=BF16, device=dev())
    return buf, buf[:rows]


def intact(obuf, rows, ibuf, n):
    assert bool((obuf[rows:] == SENT).all()), 'a guard row behind the output was written'
    assert bool((ibuf[n:] == GUARD_WORD).all()), 'a guard word behind mem_index was written'


def fp64_rows(q, kv, index, H, Hkv, hd, n_keys):
    """-> (O, bound) float64 [R, H * hd]: softmax(q k^T / sqrt(hd)) v of row r over memory row index[r], and attention_ref's bound"""
    w = Hkv * hd
    O, bound = [], []
    for r, m in enumerate(index):
        k = kv[m, :n_keys, :w].double().view(n_keys, Hkv, hd).transpose(0, 1)
        v = kv[m, :n_keys, w:].double().view(n_keys, Hkv, hd).transpose(0, 1)
        f = attention_ref.forward(q[r].double().view(H, 1, hd), k, v, hd ** -0.5, torch.ones(1, n_keys, dtype=torch.bool, device=dev()), None, 1.0)
        O.append(f.O.reshape(-1))
        bound.append(f.o_bound.reshape(-1))
    return torch.stack(O), torch.stack(bound)


def held(name, got, ref, bound):
    check(name, got.to(F64), ref, bound)
    rms = float(ref.pow(2).mean().sqrt())
    assert float(bound.median()) <= II_MAX * rms, f'{name}: median bound {float(bound.median()):.3g} against rms {rms:.3g}'


@pytest.mark.parametrize('n_keys', N_KEYS)
@pytest.mark.parametrize('H', [12, 3])
def test_mem_decode_attention(ops, H, n_keys):
    d = 64 * H
    kv = rnd(N_MEM, n_keys, 2 * d, seed=7 + n_keys)                             # token-major K | V memory, as the cross K/V GEMM writes it
    q = rnd(R, d, seed=8 + n_keys, scale=2.0)
    ibuf, index = table(MEM_INDEX, N_MEM)
    obuf, o = guarded_out(R, d)
    ops.mem_decode_attention(q, d, kv, kv.view(-1)[d:], n_keys * 2 * d, 2 * d, o, d, n_keys, index, N_MEM, R, H)
    intact(obuf, R, ibuf, R)
    ref, bound = fp64_rows(q, kv, MEM_INDEX, H, H, 64, n_keys)
    held(f'mem H={H} n={n_keys}', o, ref, bound)
    gathered = kv[torch.tensor(MEM_INDEX, device=dev())].contiguous()
    o0 = torch.empty(R, d, dtype=BF16, device=dev())
    ops.decode_attention(q, d, gathered, gathered.view(-1)[d:], n_keys * 2 * d, 2 * d, o0, d, None, n_keys, R, H)
    assert torch.equal(o0, o), 'bit-equal to decode_attention on the gathered memory'


@pytest.mark.parametrize('n_keys', N_KEYS)
@pytest.mark.parametrize('H,Hkv,hd', [(32, 32, 128), (32, 8, 128), (12, 12, 64), (12, 1, 64)])
def test_mem_gq_decode_attention(ops, H, Hkv, hd, n_keys):
    w = Hkv * hd
    kv = rnd(N_MEM, n_keys, 2 * w, seed=9 + n_keys)
    q = rnd(R, H * hd, seed=10 + n_keys, scale=2.0)
    ibuf, index = table(MEM_INDEX, N_MEM)
    obuf, o = guarded_out(R, H * hd)
    ops.mem_gq_decode_attention(q, kv, kv.view(-1)[w:], n_keys * 2 * w, 2 * w, o, n_keys, index, N_MEM, R, H, Hkv, hd)
    intact(obuf, R, ibuf, R)
    ref, bound = fp64_rows(q, kv, MEM_INDEX, H, Hkv, hd, n_keys)
    held(f'mem gq H={H} Hkv={Hkv} hd={hd} n={n_keys}', o, ref, bound)
    gathered = kv[torch.tensor(MEM_INDEX, device=dev())].contiguous()
    o0 = torch.empty(R, H * hd, dtype=BF16, device=dev())
    ops.gq_decode_attention(q, None, None, gathered, gathered.view(-1)[w:], n_keys * 2 * w, 2 * w, o0, None, n_keys, n_keys, R, H, Hkv, hd)
    assert torch.equal(o0, o), 'bit-equal to gq_decode_attention on the gathered memory'


@pytest.mark.parametrize('hd', [16, 32])
def test_mem_gq_decode_attention_narrow_heads(ops, hd):
    """the nano-mini family's head widths: 4 and 2 lanes per key"""
    H, n_keys = 6, 33
    w = H * hd
    kv, q = rnd(N_MEM, n_keys, 2 * w, seed=21), rnd(R, w, seed=22, scale=2.0)
    ibuf, index = table(MEM_INDEX, N_MEM)
    obuf, o = guarded_out(R, w)
    ops.mem_gq_decode_attention(q, kv, kv.view(-1)[w:], n_keys * 2 * w, 2 * w, o, n_keys, index, N_MEM, R, H, H, hd)
    intact(obuf, R, ibuf, R)
    held(f'mem gq hd={hd}', o, *fp64_rows(q, kv, MEM_INDEX, H, H, hd, n_keys))
    gathered = kv[torch.tensor(MEM_INDEX, device=dev())].contiguous()
    o0 = torch.empty(R, w, dtype=BF16, device=dev())
    ops.gq_decode_attention(q, None, None, gathered, gathered.view(-1)[w:], n_keys * 2 * w, 2 * w, o0, None, n_keys, n_keys, R, H, H, hd)
    assert torch.equal(o0, o)


@pytest.mark.parametrize('n_keys', [33, 257])
def test_division_table_is_the_beam_form(ops, n_keys):
    """mem_index[r] = r // W: bit-equal to the beam kernels' rows_per_mem = W"""
    W, B = 3, 2
    rows = B * W
    ibuf, index = table([r // W for r in range(rows)], B)
    H, d = 12, 768
    kv, q = rnd(B, n_keys, 2 * d, seed=31), rnd(rows, d, seed=32)
    o0, o1 = torch.empty(rows, d, dtype=BF16, device=dev()), torch.empty(rows, d, dtype=BF16, device=dev())
    ops.beam_decode_attention(q, d, kv, kv.view(-1)[d:], n_keys * 2 * d, 2 * d, o0, d, None, n_keys, rows, H, rows_per_mem=W)
    ops.mem_decode_attention(q, d, kv, kv.view(-1)[d:], n_keys * 2 * d, 2 * d, o1, d, n_keys, index, B, rows, H)
    assert torch.equal(o0, o1)
    for H, Hkv, hd in [(12, 12, 64), (32, 8, 128), (6, 6, 32)]:
        w = Hkv * hd
        kv, q = rnd(B, n_keys, 2 * w, seed=33), rnd(rows, H * hd, seed=34)
        o0, o1 = torch.empty(rows, H * hd, dtype=BF16, device=dev()), torch.empty(rows, H * hd, dtype=BF16, device=dev())
        ops.beam_gq_decode_attention(q, None, None, kv, kv.view(-1)[w:], n_keys * 2 * w, 2 * w, o0, None, n_keys, n_keys, rows, H, Hkv, hd,
                                     rows_per_mem=W)
        ops.mem_gq_decode_attention(q, kv, kv.view(-1)[w:], n_keys * 2 * w, 2 * w, o1, n_keys, index, B, rows, H, Hkv, hd)
        assert torch.equal(o0, o1), (H, Hkv, hd)
    assert bool((ibuf[rows:] == GUARD_WORD).all()), 'a guard word behind mem_index was written'


def test_host_refusals(ops):
    H, d, n = 12, 768, 8
    kv, q, o = rnd(N_MEM, n, 2 * d, seed=41), rnd(R, d, seed=42), torch.empty(R, d, dtype=BF16, device=dev())
    _, index = table(MEM_INDEX, N_MEM)
    k, v = kv, kv.view(-1)[d:]
    dense = lambda **kw: ops.mem_decode_attention(*[kw.get(a, b) for a, b in (('q', q), ('q_rs', d), ('k', k), ('v', v), ('bs', n * 2 * d), ('rs', 2 * d),
                                                                               ('o', o), ('o_rs', d), ('n', n), ('index', index), ('n_mem', N_MEM),
                                                                               ('R', R), ('H', H))])
    gq = lambda **kw: ops.mem_gq_decode_attention(*[kw.get(a, b) for a, b in (('q', q), ('k', k), ('v', v), ('bs', n * 2 * d), ('rs', 2 * d), ('o', o),
                                                                              ('n', n), ('index', index), ('n_mem', N_MEM), ('R', R), ('H', H),
                                                                              ('Hkv', H), ('hd', 64))])
    for call, name in ((dense, 'i2t_mem_decode_attention'), (gq, 'i2t_mem_gq_decode_attention')):
        call()                                                                  # the arguments as they stand are taken
        for arg in ('q', 'k', 'v', 'o'):
            refused(lambda: call(**{arg: None}), f'{name}: null operand')
        refused(lambda: call(index=None), f'{name}: mem_index is required')
        refused(lambda: call(n=0), 'key count out of range')
        refused(lambda: call(n=1025), 'key count out of range')
        refused(lambda: call(n_mem=0), 'at least one memory row')
    refused(lambda: gq(hd=48), 'head_dim 48')
    refused(lambda: gq(Hkv=5), 'heads over Hkv')
    refused(lambda: dense(rs=2 * d + 4), 'misaligned')
