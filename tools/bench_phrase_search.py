#!/usr/bin/env python3
"""search_phrases against score_phrases on the same phrase set, on a nano-224-shaped model with random weights.

    python tools/bench_phrase_search.py [--batch 16] [--phrases 1000] [--first 300] [--rounds 3] [--images-per-pass N]

K synthetic phrases of one to three tokens whose first tokens come from a pool of --first ids, so the widest trie level holds some
hundreds of nodes (printed).  score_phrases and search_phrases (W = 4 and W = 8, N = W, penalty 0) alternate ROUNDS times in one process
on the same model and images after a warm-up of each; every call includes building its trie on the host and copying it to the device.
Prints wall time per call (median [min .. max] ms, synchronised), each search's time over score_phrases', the full steps it replayed,
and how many of score_phrases' first choices lead the search's result.  Nothing is asserted about a time.

    python tools/bench_phrase_search.py --phrase-sets 8 [--batch 16] [--phrases 1000] [--first 300] [--rounds 3]

The comparison is instead: search_phrases(phrases=set 0), one set for all images, against
search_phrases(phrase_sets=S synthetic sets of K phrases each, image b answering from set b mod S), W = 4 and W = 8, alternating in one
process after a warm-up of each; both calls include building their tries on the host and copying them to the device."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.decoding import phrase_trie, trie_levels  # noqa: E402
from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder  # noqa: E402
from image2text_amd.synth import det_init_, nano224_config  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def synthetic_phrases(K, first, eos, g):
    """K distinct phrases of 1 .. 3 tokens below ``eos``, the first token of each from a pool of ``first`` ids"""
    pool = torch.randperm(eos, generator=g)[:first].tolist()
    seen = set()
    while len(seen) < K:
        n = int(torch.randint(1, 4, (1,), generator=g))
        rest = torch.randint(0, eos, (n - 1,), generator=g).tolist()
        seen.add((pool[int(torch.randint(0, first, (1,), generator=g))],) + tuple(rest))
    return [list(p) for p in sorted(seen)]


def phrase_sets_comparison(a, m, images, prompt, eos, g):
    B, K, S = a.batch, a.phrases, a.phrase_sets
    sets = [synthetic_phrases(K, a.first, eos, g) for _ in range(S)]
    index = [b % S for b in range(B)]
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {S} sets of {K} phrases of 1 .. 3 tokens, '
          f'{a.rounds} alternating rounds', flush=True)
    forms = {}
    for W in (4, 8):
        forms[f'W={W} one set'] = lambda W=W: m.search_phrases(images, prompt, sets[0], eos, num_beams=W, num_return_sequences=W)
        forms[f'W={W} {S} sets, per image'] = lambda W=W: m.search_phrases(images, prompt, eos_token_id=eos, num_beams=W, num_return_sequences=W,
                                                                           phrase_sets=sets, phrase_set_index=index)
    ts, replays = {k: [] for k in forms}, {}
    for fn in forms.values():
        fn()
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t, _ = wall(fn)
            ts[k].append(t)
            replays[k] = m._phrase_searcher.last_replays
    for k in forms:
        print(f'  {k:26s} {statistics.median(ts[k]):9.1f} [{min(ts[k]):.1f} .. {max(ts[k]):.1f}] ms   {replays[k]} full steps', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--phrase-sets', type=int, default=None, help='S: compare phrases=one set against phrase_sets=S sets (DESIGN.md 4x)')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--phrases', type=int, default=1000)
    ap.add_argument('--first', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--images-per-pass', type=int, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_phrase_search.py measures on the MI355X; there is nothing to report without one'
    B, K, eos = a.batch, a.phrases, 50256
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    g = torch.Generator().manual_seed(1)
    phrases = synthetic_phrases(K, a.first, eos, g)
    images = torch.randn(B, 3, 224, 224, generator=g).to('cuda')
    prompt = torch.full((B, 1), eos, dtype=torch.long, device='cuda')
    if a.phrase_sets:
        return phrase_sets_comparison(a, m, images, prompt, eos, g)
    wmax = trie_levels(phrase_trie(phrases, eos, m._engine.dec.V, 4)).wmax
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {K} phrases of 1 .. 3 tokens (widest trie '
          f'level {wmax} rows per image), {a.rounds} alternating rounds', flush=True)
    forms = {'score_phrases': lambda: m.score_phrases(images, prompt, phrases, eos, images_per_pass=a.images_per_pass)}
    for W in (4, 8):
        forms[f'search_phrases W={W}'] = lambda W=W: m.search_phrases(images, prompt, phrases, eos, num_beams=W, num_return_sequences=W)
    ts, outs, replays = {k: [] for k in forms}, {}, {}
    for fn in forms.values():
        fn()
    for _ in range(a.rounds):
        for k, fn in forms.items():
            t, outs[k] = wall(fn)
            ts[k].append(t)
            if k != 'score_phrases':
                replays[k] = m._phrase_searcher.last_replays
    base = statistics.median(ts['score_phrases'])
    for k in forms:
        med = statistics.median(ts[k])
        print(f'  {k:20s} {med:9.1f} [{min(ts[k]):.1f} .. {max(ts[k]):.1f}] ms' + ('' if k == 'score_phrases' else f'   x{med / base:.3f} of score_phrases, '
              f'{replays[k]} full steps, first choice = score_phrases\' best on '
              f'{int((outs[k].phrase_index[:, 0] == outs["score_phrases"].best).sum())} of {B} images'), flush=True)
    print(f'  image groups of score_phrases: {m._trie_scorer.last_passes}', flush=True)


if __name__ == '__main__':
    main()
