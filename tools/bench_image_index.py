#!/usr/bin/env python3
"""Q questions per image in one call: ``image_index`` against ``images.repeat_interleave(Q)`` on the benchmark decoder (nano-224
shape, random weights).

    python tools/bench_image_index.py [--images 64] [--rounds 5] [--questions 1,4,10] [--prompt 8]

For every Q both forms run on the SAME model, images, prompts and phrase sets in one process -- B images, Q * B queries, query q asked
of image q // Q: one warm-up call of each (graphs captured, code objects loaded), then ROUNDS rounds that alternate the two.  A call is
timed with device events around it (it ends in a host read, so the window holds all of its device work: the encoder over B or Q * B
images, the cross K/V, the prompt and the steps).  Two calls are timed: generate_captions(phrase_sets=[answers], greedy) and
score_phrases(phrases=answers).  Prints per form the median [min .. max] ms and the ratio of the medians, repeat / index -- the
repeat form in the same run is the only parent a time here has.  Q = 1 with the identity table is the same work but for the
cross-attention kernel and the state it runs on: its ratio shows the run's noise."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder  # noqa: E402
from image2text_amd.synth import det_init_, nano224_config  # noqa: E402


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
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--questions', default='1,4,10')
    ap.add_argument('--prompt', type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_image_index.py measures on the MI355X; there is nothing to report without one'
    B, P = a.images, a.prompt
    Qs = [int(q) for q in a.questions.split(',')]
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    V = m._engine.dec.V
    eos = V - 1
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, 224, 224, generator=g).to('cuda')
    answers = [torch.randint(0, V - 1, (n,), generator=g).tolist() for n in (1, 2, 2, 3, 1, 2, 3, 1)]       # 8 answers of 1 to 3 tokens
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, prompts of {P} tokens, 8 answers of 1 to 3 '
          f'tokens, {a.rounds} alternating rounds after one warm-up call of each form', flush=True)
    for Q in Qs:
        prompt = torch.randint(0, V - 1, (B * Q, P), generator=g).to('cuda')
        index = torch.arange(B).repeat_interleave(Q)
        repeated = images.repeat_interleave(Q, dim=0) if Q > 1 else images
        calls = {
            'generate_captions(phrase_sets)': {
                'index': lambda: m.generate_captions(images, prompt, max_new_tokens=4, eos_token_id=eos, top_k=1, phrase_sets=[answers],
                                                     phrase_set_index=[0] * (B * Q), image_index=index),
                'repeat': lambda: m.generate_captions(repeated, prompt, max_new_tokens=4, eos_token_id=eos, top_k=1, phrase_sets=[answers],
                                                      phrase_set_index=[0] * (B * Q))},
            'score_phrases': {
                'index': lambda: m.score_phrases_indexed(images, prompt, index, answers, eos),
                'repeat': lambda: m.score_phrases(repeated, prompt, answers, eos)},
        }
        print(f'Q = {Q} ({B * Q} queries):', flush=True)
        for what, forms in calls.items():
            ts = {k: [] for k in forms}
            for fn in forms.values():
                fn()
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    ts[k].append(timed(fn)[0])
            for k in forms:
                print(f'  {what:32s} {k:6s} {fmt(ts[k])}', flush=True)
            print(f'  {what:32s} repeat / index = {statistics.median(ts["repeat"]) / statistics.median(ts["index"]):.3f}', flush=True)
        del repeated
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
