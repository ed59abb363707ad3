#!/usr/bin/env python3
"""Beam search throughput: the KV-cache path (BeamSearchTokenGenerator(kv_cache=True), decoding.BeamDecoder) against the
re-evaluating path on a nano-224-shaped model (random weights), W = 3 beams, E = 4 candidates, 32 new tokens, deterministic.
--config nano-mini runs the same protocol on gpu/nano-mini.yaml's shape (synth.nano_mini_config: 128x128 images, sparse decoder
blocks, multi-query attention, MoE rotators).

    python tools/bench_beam.py [--config {nano224,nano-mini}] [--batches 64 1024] [--reps 3] [--legacy-max 1024]
                               [--profile B [--profile-dir DIR]]

Prints one JSON line per (path, batch): beams / s = B * W / seconds per search (encoder included, median of --reps timed runs
after one warm-up).  --profile B reruns the cached search at batch B as a child process under ``rocprofv3 --kernel-trace
--stats`` and prints the per-kernel split of one step: every kernel of two searches, encoder and prompt prefill included, divided
by their number of cached steps."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, E, NEW = 3, 4, 32


def model_and_inputs(B, config='nano224'):
    import torch
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import det_init_, nano224_config, nano_mini_config, sharpen_gates_
    if config == 'nano224':
        m, img = VisionEncoderDecoder(nano224_config()), 224
        det_init_(m, seed=0)
    else:
        m, img = VisionEncoderDecoder(nano_mini_config()), 128
        sharpen_gates_(det_init_(m, seed=0))         # decisive, input-dependent expert routing (as the family fixtures)
    m = m.to('cuda').eval()
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, img, img, generator=g).to('cuda')
    prompt = torch.full((B, 1), 50256, dtype=torch.long, device='cuda')
    return m, images, prompt


def generator(m, kv_cache):
    from image2text_amd.models.generation_utils import BeamSearchTokenGenerator
    return BeamSearchTokenGenerator(m, beam_width=W, temperature=0.0, max_new_tokens=NEW + 1, no_repeat_n_grams=(2, 3, 4),
                                    beam_expansion_factor=E, consolidation_temperature=0.0, kv_cache=kv_cache)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', choices=('nano224', 'nano-mini'), default='nano224', help='model shape (random weights)')
    ap.add_argument('--batches', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--legacy-max', type=int, default=1024, help='largest batch the re-evaluating path is timed at')
    ap.add_argument('--legacy-reps', type=int, default=1)
    ap.add_argument('--profile', type=int, default=0, help='kernel split of the cached step at this batch (rocprofv3 child)')
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profile_out', 'beam_prof'),
                    help='where rocprofv3 writes its trace (git ignores profile_out/)')
    ap.add_argument('--inner', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.inner:                                   # the profiled child: one warm-up search, one more search
        m, images, prompt = model_and_inputs(a.inner, a.config)
        gen = generator(m, True)
        gen(images, prompt)
        gen(images, prompt)
        return
    import torch
    for B in a.batches:
        m, images, prompt = model_and_inputs(B, a.config)
        for kv_cache in (True, False):
            if not kv_cache and B > a.legacy_max:
                continue
            gen = generator(m, kv_cache)
            out = {}

            def run():
                out['ids'] = gen(images, prompt)[0]
            s = timed(run, a.reps if kv_cache else a.legacy_reps)
            assert out['ids'].shape == (B, W, NEW + 1)
            print(json.dumps({'config': a.config, 'path': 'kv_cache' if kv_cache else 'recompute', 'batch': B, 'beam_width': W, 'expansion': E,
                              'new_tokens': NEW, 'seconds': round(s, 4), 'beams_per_s': round(B * W / s, 1)}), flush=True)
        del m, images, prompt
        torch.cuda.empty_cache()
    if a.profile:
        out_dir = os.path.abspath(a.profile_dir)
        os.makedirs(out_dir, exist_ok=True)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', out_dir, '-o', 'beam', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--config', a.config, '--inner', str(a.profile)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
        import csv
        import glob
        path = sorted(glob.glob(os.path.join(out_dir, '**', 'beam_kernel_stats.csv'), recursive=True))[-1]
        rows = list(csv.DictReader(open(path)))
        steps = 2 * NEW                                # two searches of NEW cached steps each
        total = sum(float(r['TotalDurationNs']) for r in rows)
        print(f'# {a.config}: kernel split of one cached beam step, B = {a.profile} captions x W = {W} (all kernels of 2 searches / {steps} steps)')
        for r in rows:
            name = r['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
            ns = float(r['TotalDurationNs'])
            print(f"{name[:72]:72s} {float(r['Calls']) / steps:6.1f}/step {ns / 1e6 / steps:8.3f} ms/step {100 * ns / total:5.1f} %")
        print(f'# all kernels: {total / 1e6 / steps:.3f} ms per step')


if __name__ == '__main__':
    main()
