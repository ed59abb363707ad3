#!/usr/bin/env python3
"""score_phrases against rerank on the same phrase set, on a nano-224-shaped model with random weights.

    python tools/bench_score_phrases.py [--batch 16] [--phrases 3000] [--phrase-len 3] [--rounds 3] [--images-per-pass N]
    python tools/bench_score_phrases.py --sets S [--ragged] [...]

K random phrases of phrase-len tokens (as tools/bench_generate_captions.py --phrases draws them), a one-token prompt.  The two calls
alternate ROUNDS times in one process after a warm-up of both; score_phrases includes building the trie and its level tables on the
host and copying them to the device, rerank building nothing (its candidates tensor is made once, outside the timing).  Prints wall
time per call (median [min .. max] ms, synchronised), the widest trie level, the image groups score_phrases ran, and the largest
difference between the two results.

--sets S: S sets of K random phrases each, image b answering from set b % S; --ragged: prompts of 1, 2 and 3 tokens,
image b's (b // S) % 3 + 1 long.  Then the ONE score_phrases(phrase_sets=..., phrase_set_index=..., prompt_lengths=...) call is timed
against what it replaces, one score_phrases(phrases=...) call per distinct (set, prompt length) pair over that pair's images, the two
forms alternating ROUNDS times after a warm-up of both; prints the wall times, the pairs and the largest difference between the
two results."""
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
    ap.add_argument('--sets', type=int, default=0, help='S phrase sets, image b answering from set b %% S, in one call against one call per (set, length)')
    ap.add_argument('--ragged', action='store_true', help='with --sets: prompts of 1, 2 and 3 tokens in one batch')
    a = ap.parse_args()
    assert not a.ragged or a.sets, '--ragged times the phrase_sets call: give --sets S'
    assert torch.cuda.is_available(), 'bench_score_phrases.py measures on the MI355X; there is nothing to report without one'
    B, K, T, eos = a.batch, a.phrases, a.phrase_len, 50256
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    if a.sets:
        return sets_against_one_call_per_pair(a, m, B, K, T, eos)
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


def sets_against_one_call_per_pair(a, m, B, K, T, eos):
    S = a.sets
    g = torch.Generator().manual_seed(1)
    sets = [torch.randint(0, eos, (K, T), generator=g).tolist() for _ in range(S)]
    images = torch.randn(B, 3, 224, 224, generator=g).to('cuda')
    prompt = torch.randint(0, eos, (B, 3), generator=g).to('cuda')
    index = [b % S for b in range(B)]
    plen = [(b // S) % 3 + 1 if a.ragged else 1 for b in range(B)]
    pairs = sorted({(index[b], plen[b]) for b in range(B)})
    members = {pr: torch.tensor([b for b in range(B) if (index[b], plen[b]) == pr], device='cuda') for pr in pairs}
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {S} sets of {K} phrases of {T} tokens, prompt '
          f'lengths {sorted(set(plen))}: {len(pairs)} distinct (set, length) pairs, {a.rounds} alternating rounds', flush=True)

    def one_call():
        return m.score_phrases(images, prompt, eos_token_id=eos, images_per_pass=a.images_per_pass, phrase_sets=sets, phrase_set_index=index,
                               prompt_lengths=plen).logprob

    def per_pair():
        out = torch.empty(B, K, device='cuda')
        for (s, p), rows in members.items():
            out[rows] = m.score_phrases(images[rows], prompt[rows, :p].contiguous(), sets[s], eos, images_per_pass=a.images_per_pass).logprob
        return out
    forms = {'one call': one_call, f'{len(pairs)} calls': per_pair}
    ts, outs = {k: [] for k in forms}, {}
    for fn in forms.values():
        fn()
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t, outs[k] = wall(fn)
            ts[k].append(t)
    for k in forms:
        print(f'  {k:14s} {statistics.median(ts[k]):9.1f} [{min(ts[k]):.1f} .. {max(ts[k]):.1f}] ms', flush=True)
    a_, b_ = outs.values()
    print(f'  largest |one call - per-pair calls| over the {B * K} log-probs: {float((a_ - b_).abs().max()):.3g}', flush=True)


if __name__ == '__main__':
    main()
