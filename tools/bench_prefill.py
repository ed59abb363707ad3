#!/usr/bin/env python3
"""generate_captions(prompt_prefill='steps') against prompt_prefill='pass' on the benchmark decoder (nano-224 shape, random weights;
DESIGN.md 4q).

    python tools/bench_prefill.py [--rows 4096] [--rounds 5] [--new 16] [--prompts 1,8,32] [--samples 1,4]

For every prompt length P and every N (captions per image; B = rows / N images) both modes run on the SAME model, images and prompt
in one process: one warm-up call of each (graphs captured, code objects loaded), then ROUNDS rounds that alternate the two.  A call is
timed with device events around it (it ends in the host's read of the lengths, so the window holds all of its device work: encoder,
cross K/V, prompt, NEW full steps).  N = 1 is greedy, N > 1 samples.  Prints per mode the median [min .. max] ms, the prefill
replays launched, and the ratio of the medians -- 'steps' in the same run is the only parent a time here has.  P = 1 leaves nothing
to prefill: there the two modes are the same launches and the ratio shows the run's noise."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder  # noqa: E402
from image2text_amd.synth import det_init_, nano224_config  # noqa: E402

SAMPLING = dict(temperature=0.7, top_k=None, nucleus_p=0.6, seed=3)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def fmt(ts):
    return f'{statistics.median(ts):8.1f} [{min(ts):.1f} .. {max(ts):.1f}] ms'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096, help='B * N')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--new', type=int, default=16)
    ap.add_argument('--prompts', default='1,8,32')
    ap.add_argument('--samples', default='1,4')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_prefill.py measures on the MI355X; there is nothing to report without one'
    R, T = a.rows, a.new
    Ps, Ns = [int(p) for p in a.prompts.split(',')], [int(n) for n in a.samples.split(',')]
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    V = m._engine.dec.V
    g = torch.Generator().manual_seed(0)
    all_images = torch.randn(R // min(Ns), 3, 224, 224, generator=g).to('cuda')
    all_prompts = torch.randint(0, V, (R // min(Ns), max(Ps)), generator=g).to('cuda')
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, B * N = {R} rows, {T} new tokens, {a.rounds} alternating '
          f'rounds after one warm-up call of each mode', flush=True)
    for N in Ns:
        assert R % N == 0
        B = R // N
        images = all_images[:B]
        mode = dict(top_k=1) if N == 1 else dict(num_return_sequences=N, **SAMPLING)
        for P in Ps:
            prompt = all_prompts[:B, :P].contiguous()
            call = {k: (lambda k=k: m.generate_captions(images, prompt, max_new_tokens=T, prompt_prefill=k, **mode)) for k in ('steps', 'pass')}
            ts, launched = {k: [] for k in call}, {}
            for k, fn in call.items():
                fn()
            for _ in range(a.rounds):
                for k, fn in call.items():
                    t, _ = timed(fn)
                    ts[k].append(t)
                    launched[k] = (m._captioner.last_prefill_steps, m._captioner.last_replays)
            ratio = statistics.median(ts['steps']) / statistics.median(ts['pass'])
            print(f'P = {P:3d}, N = {N} (B = {B} images, {"greedy" if N == 1 else "sampling"}):', flush=True)
            for k in call:
                print(f'  {k:5s}  {fmt(ts[k])}   prefill replays {launched[k][0]}, full replays {launched[k][1]}', flush=True)
            print(f'  steps / pass = {ratio:.3f}', flush=True)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
