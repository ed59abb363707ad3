#!/usr/bin/env python3
"""generate_captions(num_beams=W) throughput on a nano-224-shaped model (random weights): captions / s at W in {3, 5}, N = 1,
length_penalty 1, 32 new tokens, with an EOS id picked from a free run so that searches end early, against greedy generate_captions.

    python tools/bench_caption_beams.py [--batch 256] [--new 32] [--reps 3] [--beams 3 5]

Prints one JSON line per mode: captions / s = B / seconds per call (encoder included, median of --reps timed calls after one warm-up)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--new', type=int, default=32)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--beams', type=int, nargs='+', default=[3, 5])
    args = ap.parse_args()
    import torch
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import det_init_, nano224_config
    dev = torch.device('cuda:0')
    m = det_init_(VisionEncoderDecoder(nano224_config()), seed=0).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    images = torch.randn(args.batch, 3, 224, 224, generator=g).to(dev)
    prompt = torch.full((args.batch, 1), 50256, dtype=torch.long, device=dev)
    free = m.generate_captions(images, prompt, max_new_tokens=args.new, top_k=1)
    eos = int(free.ids[0, 0, 1 + args.new // 2])

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]
    t = timed(lambda: m.generate_captions(images, prompt, max_new_tokens=args.new, eos_token_id=eos, top_k=1))
    print(json.dumps({'mode': 'greedy', 'batch': args.batch, 'new_tokens': args.new, 'captions_per_s': round(args.batch / t, 1)}))
    for W in args.beams:
        t = timed(lambda: m.generate_captions(images, prompt, max_new_tokens=args.new, eos_token_id=eos, num_beams=W))
        print(json.dumps({'mode': f'num_beams={W}', 'batch': args.batch, 'new_tokens': args.new, 'captions_per_s': round(args.batch / t, 1),
                          'replays': m._beam_captioner.last_replays}))


if __name__ == '__main__':
    main()
