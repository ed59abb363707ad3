#!/usr/bin/env python3
"""Decode-step self-attention over long row-major caches, the launch alone, under hipGraph replay.

    python tools/bench_long_decode.py [--rows 8 128 1024] [--keys 1024 2048 4096] [--models llama2-7b qwen2-1.5b falcon-7b]
                                      [--variant CHUNK=LIBRARY ...] [--json out.json]

Per (model shape, rows R, cached keys n): the split-key form (i2t_gq_decode_attention_long) and, at n <= 1024, the classic kernel
(i2t_gq_decode_attention) on the same buffers, both in the append form the decode step uses.  A graph of ``--launches`` launches is
replayed in windows of at least ``--window`` seconds between device events.  All kernels of a shape are captured first and then timed
in ``--rounds`` alternating rounds of ``--windows`` windows each (A B C A B C ...), in ONE process: the figure is the median over all
windows of a kernel, with their minimum and maximum beside it, so the spread that a comparison has to exceed is on the same line.
GB/s counts the algorithmic K/V bytes -- R * n * Hkv * hd * 2 tensors * 2 bytes -- and nothing else (the G query heads of a group
read their K/V head once each; that re-read is not counted, so the column is not a bandwidth for a grouped model).  These are
graph-replay times per launch (the partial and the combine kernel together), not kernel times.

A/B of the chunk size: ``tools/build_variant.sh ch128 family.hip -DLONG_CHUNK_KEYS=128`` builds a second library of the same ABI;
``--variant 128=image2text_amd/csrc/libi2t_ch128.so`` loads it beside the package's own and times it in the same rounds (the
workspace is sized for the smallest chunk, which every larger one fits).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SHAPES = {'llama2-7b': (32, 32, 128), 'qwen2-1.5b': (12, 2, 128), 'falcon-7b': (71, 1, 64)}          # H, Hkv, hd


def kv_bytes(R, n, Hkv, hd):
    return R * n * Hkv * hd * 2 * 2


def load_variant(path):
    """a second library of the package's ABI, bound like lib.load() binds the first"""
    from image2text_amd import lib as i2tlib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ('i2t_abi_version', 'i2t_gq_decode_attention_long'):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = i2tlib.SIGNATURES[name], ctypes.c_int
    if lib.i2t_abi_version() != i2tlib.ABI_VERSION:
        sys.exit(f'{path}: ABI {lib.i2t_abi_version()}, the package binds {i2tlib.ABI_VERSION}')
    return lib


def reps_for(graph, window_s):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        graph.launch()
    torch.cuda.synchronize()
    start.record()
    graph.launch()
    end.record()
    torch.cuda.synchronize()
    return max(1, int(window_s / max(start.elapsed_time(end) * 1e-3, 1e-6)))


def window(graph, reps):
    """seconds per replay over one window of ``reps`` replays"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        graph.launch()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', nargs='+', default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument('--rows', nargs='+', type=int, default=[8, 128, 1024])
    ap.add_argument('--keys', nargs='+', type=int, default=[1024, 2048, 4096])
    ap.add_argument('--variant', nargs='*', default=[], metavar='CHUNK=LIBRARY', help='further libraries built with another LONG_CHUNK_KEYS')
    ap.add_argument('--launches', type=int, default=8, help='launches per captured graph')
    ap.add_argument('--window', type=float, default=1.0, help='seconds per timed window')
    ap.add_argument('--windows', type=int, default=2, help='windows per kernel and round')
    ap.add_argument('--rounds', type=int, default=2, help='alternating rounds over the kernels of a shape')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    variants = [(int(c), p) for c, p in (v.split('=', 1) for v in args.variant)]
    if not torch.cuda.is_available():
        sys.exit('bench_long_decode: no GPU visible; this tool has no CPU path')
    from image2text_amd import lib as i2tlib, ops
    from image2text_amd.decoding import DECODE_MAX_KEYS, _capture_launches
    dev = torch.device('cuda:0')
    libs = [(ops.LONG_CHUNK_KEYS, i2tlib.load())] + [(c, load_variant(p)) for c, p in variants]
    ch_min = min(c for c, _ in libs)
    T = max(args.keys)
    rows = []
    print(f'# chunk sizes {[c for c, _ in libs]}, {args.launches} launches per graph, {args.rounds} alternating rounds of {args.windows} windows '
          f'of >= {args.window} s: median [min .. max] over all windows')
    print(f'{"model":12s} {"R":>5s} {"n":>5s} {"kernel":10s} {"us/launch":>26s} {"GB/s":>8s}')
    for name in args.models:
        H, Hkv, hd = SHAPES[name]
        w = Hkv * hd
        for R in args.rows:
            kc = torch.randn(R, T, w, device=dev, dtype=torch.bfloat16)
            vc = torch.randn(R, T, w, device=dev, dtype=torch.bfloat16)
            q = torch.randn(R, H * hd, device=dev, dtype=torch.bfloat16)
            kvn = torch.randn(R, 2 * w, device=dev, dtype=torch.bfloat16)
            out = torch.empty(R, H * hd, device=dev, dtype=torch.bfloat16)
            ws = torch.empty(R * H * (-(-T // ch_min)) * (hd + 2), device=dev, dtype=torch.float32)     # the formula, at the smallest chunk
            for n in args.keys:
                pos = torch.tensor([n - 1], dtype=torch.int32, device=dev)
                a = (q, kvn[:, :w], kvn[:, w:], kc, vc, T * w, w, out, pos, 0)

                def split(lib):
                    def fn():
                        i2tlib.check(lib.i2t_gq_decode_attention_long(
                            torch.cuda.current_stream().cuda_stream, q.data_ptr(), q.stride(0), kvn.data_ptr(), kvn[:, w:].data_ptr(),
                            kvn.stride(0), kc.data_ptr(), vc.data_ptr(), T * w, w, out.data_ptr(), out.stride(0), pos.data_ptr(), 0, T, R, H,
                            Hkv, hd, ws.data_ptr(), ws.numel()), 'i2t_gq_decode_attention_long')
                    return fn
                kinds = [(f'split{c}', c, split(lib)) for c, lib in libs]
                if n <= DECODE_MAX_KEYS:
                    kinds.append(('classic', 0, lambda: ops.gq_decode_attention(*a, DECODE_MAX_KEYS, R, H, Hkv, hd)))
                graphs = []
                for kind, c, fn in kinds:
                    fn()                                    # code objects are loaded before the capture
                    torch.cuda.synchronize()
                    graph = _capture_launches(dev, lambda fn=fn: [fn() for _ in range(args.launches)])
                    graphs.append((kind, c, graph, reps_for(graph, args.window), []))
                for _ in range(args.rounds):                # A B C A B C: drift and neighbours hit every kernel alike
                    for kind, c, graph, reps, times in graphs:
                        times.extend(window(graph, reps) / args.launches for _ in range(args.windows))
                for kind, c, graph, reps, times in graphs:
                    med, lo, hi = statistics.median(times), min(times), max(times)
                    gbs = kv_bytes(R, n, Hkv, hd) / med / 1e9
                    rows.append(dict(model=name, R=R, n=n, kernel=kind, chunk=c, us=med * 1e6, us_min=lo * 1e6, us_max=hi * 1e6, gbs=gbs))
                    print(f'{name:12s} {R:5d} {n:5d} {kind:10s} {med * 1e6:9.1f} [{lo * 1e6:.1f} .. {hi * 1e6:.1f}] {gbs:8.0f}', flush=True)
                del graphs
            del kc, vc, ws
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
