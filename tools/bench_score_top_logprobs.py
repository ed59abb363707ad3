#!/usr/bin/env python3
"""What ``score(..., top_logprobs=K)`` costs at the head: ``HotPath.token_logprobs`` (K = 0: the segment-statistics head, ops.gemm_lse +
ops.lse_token_logprob) against ``HotPath.token_top_logprobs`` (K = 8: the fp32 lm_head into a chunk of scratch + ops.score_top_logprobs)
on the benchmark decoder's head shape, rows x 50257 x 768 with rows = 4096 captions x 64 positions.

    python tools/bench_score_top_logprobs.py [--captions 4096] [--positions 64] [--k 8] [--temperature 1.0] [--rounds 5] [out.txt]

The two methods are the engine's own, run on a stand-in that holds what they read of an engine (the head weight, V, Vp, d), so the chunk
arithmetic timed is the one ``score`` runs.  Both forms run in one process on the same operands, alternating, ROUNDS times after a
warm-up of each; times are device events around a window of back-to-back calls, reported as the median and the range over the rounds.
Bytes written are counted from the shapes: what passes through the chunk scratch, and what the call leaves behind."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.engine import VOCAB_PAD, HotPath  # noqa: E402

dev = torch.device('cuda:0')
BF16 = torch.bfloat16
V, D = 50257, 768
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


class Head:
    """what the two scoring heads read of a HotPath"""
    SCORE_WS_BYTES = HotPath.SCORE_WS_BYTES
    _empty, _score_ws = HotPath._empty, HotPath._score_ws
    token_logprobs, token_top_logprobs = HotPath.token_logprobs, HotPath.token_top_logprobs

    def __init__(self, W):
        self.arena = SimpleNamespace(device=dev, W=lambda name: W)
        self.dec = SimpleNamespace(d=D, V=V, Vp=(V + VOCAB_PAD - 1) // VOCAB_PAD * VOCAB_PAD)
        self.n_head = 'head'


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--captions', type=int, default=4096)
    ap.add_argument('--positions', type=int, default=64)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3, help='calls per timed window')
    ap.add_argument('out', nargs='?')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_score_top_logprobs.py measures on the MI355X; there is nothing to report without one'
    M, K, inv = a.captions * a.positions, a.k, 1.0 / a.temperature
    g = torch.Generator(device=dev).manual_seed(M + V)
    hid = torch.randn(M, D, generator=g, device=dev).to(BF16)
    W = (torch.randn(V, D, generator=g, device=dev) * (3.0 / D ** 0.5)).to(BF16)
    labels = torch.randint(0, V, (M,), generator=g, device=dev)
    head = Head(W)
    Vp, nseg = head.dec.Vp, (V + 63) // 64
    rows_stats = min(M, max(256, Head.SCORE_WS_BYTES // (nseg * 8) // 256 * 256))
    rows_top = Head.SCORE_WS_BYTES // (Vp * 4)
    rows_top = min(M, rows_top // 256 * 256 if rows_top >= 256 else max(1, rows_top))
    forms = ((f'K = 0 (gemm_lse + lse_token_logprob)', lambda: head.token_logprobs(hid, labels, M, inv), rows_stats, M * nseg * 8, 8 * M),
             (f'K = {K} (gemm fp32 + score_top_logprobs)', lambda: head.token_top_logprobs(hid, labels, M, K, inv), rows_top, M * Vp * 4,
              M * (8 * K + 16)))
    say(f'device: {torch.cuda.get_device_name(0)}; {a.captions} captions x {a.positions} positions = {M} rows x {V} x {D}, temperature '
        f'{a.temperature}; {a.rounds} alternating rounds, device events around {a.reps} calls; median [min .. max] ms')
    for _, fn, _, _, _ in forms:              # warm-up: code objects, the scratch, both shapes of the chunk loop
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, *_ in forms}
    for _ in range(a.rounds):
        for name, fn, *_ in forms:
            times[name].append(timed(fn, a.reps))
    base = statistics.median(times[forms[0][0]])
    for name, _, rows, scratch, left in forms:
        t = times[name]
        med = statistics.median(t)
        say(f'  {name:42s} {med:8.3f} [{min(t):8.3f} .. {max(t):8.3f}] ms  x{med / base:.3f}  {2.0 * M * V * D / med / 1e9:7.1f} TFLOP/s of the GEMM  '
            f'{rows} rows per chunk; through the scratch {scratch / 2 ** 20:9.1f} MiB, left behind {left / 2 ** 20:7.1f} MiB')
    lp0, lse0 = head.token_logprobs(hid, labels, M, inv)
    lp8, lse8 = head.token_top_logprobs(hid, labels, M, K, inv)[:2]
    say(f'  max |lse K = {K} - lse K = 0| = {float((lse8 - lse0).abs().max()):.3g}, max |token_logprobs K = {K} - K = 0| = '
        f'{float((lp8 - lp0).abs().max()):.3g}   (close, not bit-equal: segment statistics against fp32 rows)')
    say(f'  forward(...).logits would hold {M * V * 4 / 2 ** 30:.1f} GiB')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
