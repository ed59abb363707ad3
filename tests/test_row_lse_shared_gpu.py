"""The four 256-thread kernels that take a raw fp32 row's log-sum-exp call one pair of helpers (csrc/select_common.h:
row_lse_partials / lse_waves_merge), so for the same row they give the same bits: raw_lse of i2t_caption_trie_mask, the output of
i2t_rows_lse, lse of i2t_trie_beam_candidates and raw_lse of i2t_caption_logits_process.  The host replicas and the bit-exact tests
of the decoding modes rely on that.

V = 3 (the tail loop only), 67, 257, 1027 (a second trip of the 16-byte loop and a tail); ld the next multiple of 4; R = 3: row 0 holds
some -inf columns, row 1 is all -inf (every kernel gives -inf), row 2 has its maximum in the last column.  A two-node trie (the root,
one child that ends a phrase), every row at the root, done = 0; the processors run with no ids, no suppress list and no EOS rule.
Every output is also held against the fp64 logsumexp within tests/test_logits_processors_gpu.py's raw_lse bound."""
import numpy as np
import pytest
import torch

from test_logits_processors_gpu import bits, lse_bound

pytestmark = pytest.mark.gpu

F32, I32, I64 = torch.float32, torch.int32, torch.int64
R, VS = 3, (3, 67, 257, 1027)


@pytest.fixture(scope='module')
def ops():
    from image2text_amd import ops as _ops
    from image2text_amd.build import build_library
    build_library()
    return _ops


def rows(V):
    ld = (V + 3) // 4 * 4
    rng = np.random.default_rng(V)
    z = np.full((R, ld), 1e30, np.float32)                   # the pad columns: read by no kernel
    z[:, :V] = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    z[0, :V:3] = -np.inf
    z[1, :V] = -np.inf
    z[2, V - 1] = 20.0
    return z, ld


@pytest.mark.parametrize('V', VS)
def test_four_kernels_one_row_lse(ops, V):
    dev = torch.device('cuda:0')
    z, ld = rows(V)
    i32 = lambda a: torch.tensor(a, dtype=I32, device=dev)
    child_off, child_tok, term = i32([0, 1, 1]), i32([1]), i32([-1, 0])     # root -token 1-> node 1, which ends phrase 0
    eos, node, done = 0, i32([0] * R), i32([0])
    out = {k: torch.full((R,), float('nan'), dtype=F32, device=dev) for k in ('trie_mask', 'rows_lse', 'trie_beam_candidates', 'logits_process')}
    fresh = lambda: torch.from_numpy(z).to(dev)

    ops.caption_trie_mask(fresh(), ld, node, child_off, child_tok, term, eos, done, out['trie_mask'], torch.zeros(R, 4, device=dev), R, V)
    ops.rows_lse(fresh(), ld, out['rows_lse'], R, V)
    ops.trie_beam_candidates(fresh(), ld, node, torch.zeros(R, device=dev), child_off, child_tok, term, eos, i32([0, 0]),
                             torch.zeros(R, 1, dtype=I32, device=dev), torch.zeros(R, 1, device=dev), torch.zeros(R, device=dev), R, 1, V,
                             lse=out['trie_beam_candidates'])
    ops.caption_logits_process(fresh(), ld, torch.zeros(R, 4, dtype=I64, device=dev), 4, i32([0]), None, 0, 1, None, 0, None, 0, 1.0, 1.0, done,
                               out['logits_process'], torch.zeros(R, 4, device=dev), R, V)
    torch.cuda.synchronize()

    ref, bound = lse_bound(torch.from_numpy(z[:, :V]).double(), V)
    for name, got in out.items():
        assert torch.equal(bits(got), bits(out['rows_lse'])), f'V {V}: {name} {got.tolist()} is not rows_lse {out["rows_lse"].tolist()} bit for bit'
        got = got.double().cpu()
        assert got[1] == -np.inf and ref[1] == -np.inf, f'V {V}: {name}: the all -inf row gives {float(got[1])}'
        err = (got - ref).abs()[[0, 2]]
        print(f'V {V} {name}: worst error / bound {float((err / bound[[0, 2]]).max()):.3g}')
        assert bool((err <= bound[[0, 2]]).all()), f'V {V}: {name} {got.tolist()} vs fp64 {ref.tolist()} (bound {bound.tolist()})'
