#!/usr/bin/env python3
"""generate() for 64 tokens against generate_captions() with an EOS id at which the rows end, on a nano-224-shaped model with random
weights.

    python tools/bench_generate_captions.py [--batch 256] [--rounds 3] [--new 64]

Two comparisons, each alternating its two forms ROUNDS times in one process after a warm-up of both:
  N = 1   generate(images, 64 tokens, greedy)                      vs  generate_captions(images, eos, greedy)
  N = 4   generate(images repeated 4 times, 64 tokens, sampling)   vs  generate_captions(images, eos, N = 4, sampling)
The EOS id is taken from a free run: the token whose first emission, over all rows, comes earliest at the latest row -- the rows of
random weights do end, if late.  Prints wall time per call (median [min .. max] ms, synchronised), the replays launched, the mean
length, and the rise of the allocator's peak across a call of each form (decoder state included: measured on a fresh model).

    python tools/bench_generate_captions.py --repetition-penalty 1.3 [--min-new-tokens 8] [--suppress 0,1,2]

With any of the three flags the comparison is instead: generate_captions as it is against generate_captions with the
logits processors, greedy N = 1 and sampling N = 4, no EOS id unless --min-new-tokens needs one (50256; every call then runs all
steps that its rows need), alternating in one process -- first with the segment-maxima head in play (nano-224: d % 128 == 0, so the
processors also cost the switch to the fp32-logits head), then with I2T_DECODE_TOP2's effect switched off in the process (both forms on
the fp32-logits head: the difference is the two new launches alone).

    python tools/bench_generate_captions.py --phrases 3000 [--phrase-len 3]

The comparison is instead: generate_captions without phrases for phrase-len + 1 new tokens against
generate_captions(phrases=K random phrases of phrase-len tokens), greedy N = 1 and sampling N = 4, alternating in one process; the
constrained call includes building the trie on the host and copying it to the device.

    python tools/bench_generate_captions.py --phrase-sets 8 [--phrases 3000] [--phrase-len 3]

The comparison is instead: generate_captions(phrases=set 0), one set for all images, against
generate_captions(phrase_sets=S sets of K random phrases each, image b answering from set b mod S), greedy N = 1 and sampling N = 4,
alternating in one process; both calls include building their tries on the host and copying them to the device."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder  # noqa: E402
from image2text_amd.synth import det_init_, nano224_config  # noqa: E402

SAMPLING = dict(temperature=0.7, top_k=None, nucleus_p=0.6)


def fresh(B):
    m = VisionEncoderDecoder(nano224_config())
    det_init_(m, seed=0)
    m = m.to('cuda').eval()
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, 224, 224, generator=g).to('cuda')
    prompt = torch.full((B, 1), 50256, dtype=torch.long, device='cuda')
    return m, images, prompt


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_rise(B, call):
    m, images, prompt = fresh(B)
    m._engine.prepare(False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    call(m, images, prompt)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del m
    torch.cuda.empty_cache()
    return rise / 2 ** 20


def pick_eos(ids, P):
    """the token whose first emission comes earliest at the latest row; -> (id, that step)"""
    new = ids[:, P:]
    best, best_step = None, new.shape[1] + 1
    for tok in new[0].unique().tolist():
        hit = new == tok
        if not bool(hit.any(dim=1).all()):
            continue
        step = int(hit.float().argmax(dim=1).max()) + 1
        if step < best_step:
            best, best_step = tok, step
    return best, best_step


def fmt(ts):
    return f'{statistics.median(ts):8.1f} [{min(ts):.1f} .. {max(ts):.1f}] ms'


def processors_comparison(a, procs):
    from image2text_amd import decoding
    B, T = a.batch, a.new
    eos = 50256 if procs.get('min_new_tokens') else None
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {T} new tokens, {a.rounds} alternating rounds; '
          f'processors {procs}, eos id {eos}', flush=True)
    for top2 in (True, False):
        decoding.TOP2_HEAD = top2
        m, images, prompt = fresh(B)
        print(f'inactive greedy head: {"segment maxima (the processors switch it to fp32 logits)" if top2 else "fp32 logits (both forms)"}', flush=True)
        for N, mode in ((1, dict(top_k=1)), (4, SAMPLING)):
            kw = dict(max_new_tokens=T, eos_token_id=eos, num_return_sequences=N, seed=3, **mode)
            forms = {'as it is': lambda: m.generate_captions(images, prompt, **kw),
                     'with processors': lambda: m.generate_captions(images, prompt, **kw, **procs)}
            ts, replays = {k: [] for k in forms}, {}
            for fn in forms.values():
                fn()
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    t, _ = wall(fn)
                    ts[k].append(t)
                    replays[k] = m._captioner.last_replays
            for k in forms:
                print(f'  N = {N} {"greedy  " if N == 1 else "sampling"} {k:16s} {fmt(ts[k])}   replays {replays[k]}', flush=True)
        del m
        torch.cuda.empty_cache()


def phrases_comparison(a):
    """generate_captions without phrases (--phrase-len + 1 new tokens, no EOS id: as many steps as the constrained call needs at the
    most) against generate_captions(phrases=K random phrases of --phrase-len tokens), greedy N = 1 and sampling N = 4"""
    B, K, T = a.batch, a.phrases, a.phrase_len
    eos = 50256
    g = torch.Generator().manual_seed(1)
    phrases = torch.randint(0, eos, (K, T), generator=g).tolist()
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {K} phrases of {T} tokens, {a.rounds} '
          f'alternating rounds', flush=True)
    m, images, prompt = fresh(B)
    for N, mode in ((1, dict(top_k=1)), (4, SAMPLING)):
        kw = dict(max_new_tokens=T + 1, num_return_sequences=N, seed=3, **mode)
        forms = {'as it is': lambda: m.generate_captions(images, prompt, **kw),
                 'with phrases': lambda: m.generate_captions(images, prompt, eos_token_id=eos, phrases=phrases, **kw)}
        ts, replays = {k: [] for k in forms}, {}
        for fn in forms.values():
            fn()
        for _ in range(a.rounds):
            for k, fn in forms.items():
                t, _ = wall(fn)
                ts[k].append(t)
                replays[k] = m._captioner.last_replays
        for k in forms:
            print(f'  N = {N} {"greedy  " if N == 1 else "sampling"} {k:13s} {fmt(ts[k])}   replays {replays[k]}', flush=True)


def phrase_sets_comparison(a):
    """generate_captions(phrases=set 0) against generate_captions(phrase_sets=S sets, image b from set b mod S), greedy N = 1 and
    sampling N = 4"""
    B, K, T, S = a.batch, a.phrases or 3000, a.phrase_len, a.phrase_sets
    eos = 50256
    g = torch.Generator().manual_seed(1)
    sets = [torch.randint(0, eos, (K, T), generator=g).tolist() for _ in range(S)]
    index = [b % S for b in range(B)]
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {S} sets of {K} phrases of {T} tokens, '
          f'{a.rounds} alternating rounds', flush=True)
    m, images, prompt = fresh(B)
    for N, mode in ((1, dict(top_k=1)), (4, SAMPLING)):
        kw = dict(max_new_tokens=T + 1, eos_token_id=eos, num_return_sequences=N, seed=3, **mode)
        forms = {'one set': lambda: m.generate_captions(images, prompt, phrases=sets[0], **kw),
                 f'{S} sets, per image': lambda: m.generate_captions(images, prompt, phrase_sets=sets, phrase_set_index=index, **kw)}
        ts, replays = {k: [] for k in forms}, {}
        for fn in forms.values():
            fn()
        for _ in range(a.rounds):
            for k, fn in forms.items():
                t, _ = wall(fn)
                ts[k].append(t)
                replays[k] = m._captioner.last_replays
        for k in forms:
            print(f'  N = {N} {"greedy  " if N == 1 else "sampling"} {k:20s} {fmt(ts[k])}   replays {replays[k]}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--phrase-sets', type=int, default=None, help='S: compare phrases=one set against phrase_sets=S sets (DESIGN.md 4x)')
    ap.add_argument('--phrases', type=int, default=None, help='K: compare against generate_captions(phrases=K random phrases) (DESIGN.md 4u)')
    ap.add_argument('--phrase-len', type=int, default=3)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--new', type=int, default=64)
    ap.add_argument('--repetition-penalty', type=float, default=None)
    ap.add_argument('--min-new-tokens', type=int, default=None)
    ap.add_argument('--suppress', type=str, default=None, help='comma-separated token ids')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_generate_captions.py measures on the MI355X; there is nothing to report without one'
    if a.phrase_sets:
        return phrase_sets_comparison(a)
    if a.phrases:
        return phrases_comparison(a)
    procs = {}
    if a.repetition_penalty is not None:
        procs['repetition_penalty'] = a.repetition_penalty
    if a.min_new_tokens is not None:
        procs['min_new_tokens'] = a.min_new_tokens
    if a.suppress:
        procs['suppress_tokens'] = [int(t) for t in a.suppress.split(',') if t.strip()]
    if procs:
        return processors_comparison(a, procs)
    B, T = a.batch, a.new
    print(f'device: {torch.cuda.get_device_name(0)}; nano-224 shape, random weights, {B} images, {T} new tokens, {a.rounds} alternating rounds',
          flush=True)
    m, images, prompt = fresh(B)
    for N, mode in ((1, dict(top_k=1)), (4, SAMPLING)):
        rep_i, rep_p = (images.repeat_interleave(N, dim=0), prompt.repeat_interleave(N, dim=0)) if N > 1 else (images, prompt)
        free = m.generate_captions(images, prompt, max_new_tokens=T, num_return_sequences=N, seed=3, **mode)
        eos, step = pick_eos(free.ids.reshape(B * N, -1), 1)
        if eos is None:
            print(f'N = {N}: no token is emitted by every row within {T} steps; generate_captions runs all {T} steps', flush=True)
        forms = {'generate': lambda: m.generate(rep_i, rep_p, max_new_tokens=T, **mode),
                 'generate_captions': lambda: m.generate_captions(images, prompt, max_new_tokens=T, eos_token_id=eos, num_return_sequences=N,
                                                                  seed=3, **mode)}
        for fn in forms.values():
            fn()
        ts = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                t, out = wall(fn)
                ts[k].append(t)
        print(f'N = {N} ({"greedy" if N == 1 else "sampling T 0.7 / p 0.6"}), eos id {eos} (every row has emitted it by step {step}):', flush=True)
        print(f'  generate, {B * N} rows x {T} tokens      {fmt(ts["generate"])}', flush=True)
        print(f'  generate_captions                   {fmt(ts["generate_captions"])}   replays {m._captioner.last_replays}, '
              f'mean length {float(out.lengths.float().mean()):.1f}, L {out.ids.shape[-1]}', flush=True)
        torch.cuda.empty_cache()
        r_gen = peak_rise(B, lambda mm, im, pr: mm.generate(im.repeat_interleave(N, dim=0) if N > 1 else im,
                                                            pr.repeat_interleave(N, dim=0) if N > 1 else pr, max_new_tokens=T, **mode))
        r_cap = peak_rise(B, lambda mm, im, pr: mm.generate_captions(im, pr, max_new_tokens=T, eos_token_id=eos, num_return_sequences=N, seed=3,
                                                                     **mode))
        print(f'  peak memory rise: generate {r_gen:.0f} MiB, generate_captions {r_cap:.0f} MiB', flush=True)


if __name__ == '__main__':
    main()
