#!/usr/bin/env python3
"""score_phrases against rerank on the same phrase set, on a nano-224-shaped model with random weights.

    python tools/bench_score_phrases.py [--batch 16] [--phrases 3000] [--phrase-len 3] [--rounds 3] [--images-per-pass N]

K random phrases of phrase-len tokens (as tools/bench_generate_captions.py --phrases draws them), a one-token prompt.  The two calls
alternate ROUNDS times in one process after a warm-up of both; score_phrases includes building the trie and its level tables on the
host and copying them to the device, rerank building nothing (its candidates tensor is made once, outside the timing).  Prints wall
time per call (median [min .. max] ms, synchronised), the widest trie level, the image groups score_phrases ran, and the largest
difference between the two results."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.decoding import phrase_trie, trie_levels  # noqa: E402
from image2text_amd.models.generation_utils import rerank  # noqa: E402
from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder  # noqa: E402
from image2text_amd.synth import det_init_, nano224_config  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--phrases', type=int, default=3000)
    ap.add_argument('--phrase-len', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--images-per-pass', type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_score_phrases.py measures on the MI355X; there is nothing to report without one'
    B, K, T, eos = a.batch, a.phrases, a.phrase_len, 50256
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    g = torch.Generator().manual_seed(1)
    phrases = torch.randint(0, eos, (K, T), generator=g)
    images = torch.randn(B, 3, 224, 224, generator=g).to('cuda')
    prompt = torch.full((B, 1), eos, dtype=torch.long, device='cuda')
    cand = torch.cat((prompt[:, None].expand(B, K, 1), phrases.to('cuda')[None].expand(B, K, T), torch.full((B, K, 1), eos, device='cuda')), dim=-1)
    wmax = trie_levels(phrase_trie(phrases.tolist(), eos, m._engine.dec.V, T + 1)).wmax
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {K} phrases of {T} tokens (widest trie level '
          f'{wmax} rows per image), {a.rounds} alternating rounds', flush=True)
    forms = {'score_phrases': lambda: m.score_phrases(images, prompt, phrases.tolist(), eos, images_per_pass=a.images_per_pass).logprob,
             'rerank': lambda: rerank(m, images, cand, eos=eos, prompt_len=1)[1]}
    ts, outs = {k: [] for k in forms}, {}
    for fn in forms.values():
        fn()
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t, outs[k] = wall(fn)
            ts[k].append(t)
    for k in forms:
        print(f'  {k:14s} {statistics.median(ts[k]):9.1f} [{min(ts[k]):.1f} .. {max(ts[k]):.1f}] ms', flush=True)
    print(f'  image groups of score_phrases: {m._trie_scorer.last_passes}; largest |score_phrases - rerank| over the {B * K} log-probs: '
          f'{float((outs["score_phrases"] - outs["rerank"]).abs().max()):.3g}', flush=True)


if __name__ == '__main__':
    main()
