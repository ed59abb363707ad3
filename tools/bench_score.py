#!/usr/bin/env python3
"""Caption scoring's head: the fused pair (ops.gemm_lse + ops.lse_token_logprob, row chunks of HotPath.SCORE_WS_BYTES of segment
statistics) against the logits form (bf16 logits by ops.gemm + ops.ce_fwd) at the benchmark's head shape and at one decode batch.

    python tools/bench_score.py [out.txt]

Both forms run in one process on the same operands, alternating, ROUNDS times after a warm-up of each; times are device events
around a window of back-to-back calls, reported as the median and the range over the rounds.  Bytes written are counted from the shapes."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd import ops  # noqa: E402
from image2text_amd.engine import HotPath  # noqa: E402

dev = torch.device('cuda:0')
BF16, F32 = torch.bfloat16, torch.float32
SHAPES = [(110592, 50257, 768), (4096, 50257, 768)]
ROUNDS, ROWS_PER_WINDOW = 5, 3 * 110592       # every timed window covers at least this many rows (>= 3 calls)
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    assert torch.cuda.is_available(), 'bench_score.py measures on the MI355X; there is nothing to report without one'
    say(f'device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating rounds, device events around >= {ROWS_PER_WINDOW} rows of calls; median [min .. max] ms')
    for M, V, d in SHAPES:
        g = torch.Generator(device=dev).manual_seed(M + V)
        hid = torch.randn(M, d, generator=g, device=dev).to(BF16)
        W = (torch.randn(V, d, generator=g, device=dev) * (3.0 / d ** 0.5)).to(BF16)
        labels = torch.randint(0, V, (M,), generator=g, device=dev)
        nseg, Vp = (V + 63) // 64, (V + 7) // 8 * 8
        chunk = max(256, HotPath.SCORE_WS_BYTES // (nseg * 8) // 256 * 256)
        stats = torch.zeros(min(chunk, M), nseg, 2, device=dev)
        lse_f, lp_f = torch.empty(M, device=dev), torch.empty(M, device=dev)
        logits = torch.zeros(M, Vp, dtype=BF16, device=dev)
        lse_l, loss, ones = torch.empty(M, device=dev), torch.zeros(1, device=dev), torch.ones(M, device=dev)

        def fused():
            for r0 in range(0, M, chunk):
                n = min(chunk, M - r0)
                ops.gemm_lse(hid[r0:r0 + n], W, stats[:n], n, V, d)
                ops.lse_token_logprob(stats[:n], hid[r0:r0 + n], W, labels[r0:r0 + n], lse_f[r0:r0 + n], lp_f[r0:r0 + n], n, V, d)

        def logits_form():
            ops.gemm(hid, W, logits, M, V, d)
            ops.ce_fwd(logits, Vp, labels, ones, 1.0, -100, lse_l, loss, M, V)

        forms = (('fused (gemm_lse + lse_token_logprob)', fused, M * nseg * 8 + 8 * M),
                 ('logits (gemm bf16 + ce_fwd)', logits_form, M * Vp * 2 + 4 * M))
        for _, fn, _ in forms:              # warm-up: code objects, both shapes of the chunk loop
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in forms}
        for _ in range(ROUNDS):
            for name, fn, _ in forms:
                times[name].append(timed(fn, max(3, ROWS_PER_WINDOW // M)))
        say(f'M = {M}, V = {V}, d = {d}   (2 M V d = {2.0 * M * V * d / 1e12:.2f} TFLOP; fused rows per chunk {min(chunk, M)})')
        for name, _, written in forms:
            t = times[name]
            med = statistics.median(t)
            say(f'  {name:38s} {med:8.3f} [{min(t):8.3f} .. {max(t):8.3f}] ms   {2.0 * M * V * d / med / 1e9:7.1f} TFLOP/s   '
                f'writes {written / 2 ** 20:9.1f} MiB')
        diff = float((lse_f - lse_l).abs().max())
        say(f'  max |lse fused - lse logits form| = {diff:.3g}   (the logits form rounds its logits to bf16)')
        del logits, stats
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
