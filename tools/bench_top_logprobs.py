#!/usr/bin/env python3
"""What ``generate_captions(top_logprobs=K)`` costs: greedy captions/s at ``bench.py --full``'s decode shape (4096 captions, a prompt of
one token, 64 new tokens, no EOS; random weights) for K in {0, 1, 5, 8}.

    python tools/bench_top_logprobs.py [--model nano|nano704] [--ks 0,1,5,8] [--captions 4096] [--rounds 3] [--root DIR]

``--model nano`` is the benchmark model (12 x 768 decoder): K = 0 takes the segment-maxima head, K > 0 the fp32-logits head, so its
rows hold the head switch AND the kernel.  ``--model nano704`` is the same model with a 704-wide decoder (11 heads of 64, d % 128 != 0),
which takes the fp32-logits head anyway: its rows show the kernel's own cost alone.  One process, one model: one warm-up call per K
(graphs captured, code objects loaded), then ROUNDS rounds that alternate the Ks; a call is timed with device events around it (it ends
in a host read, so the window holds the encoder, the cross K/V and the 64 steps).  Prints per K the median [min .. max] ms, captions/s
at the median and the ratio to K = 0.  ``--root DIR``: import the package from another checkout (the parent commit's, with ``--ks 0``:
the argument is not passed at K = 0), so that alternating processes compare two trees on one machine."""
import argparse
import os
import statistics
import sys

import torch


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('nano', 'nano704'), default='nano')
    ap.add_argument('--ks', default='0,1,5,8')
    ap.add_argument('--captions', type=int, default=4096)
    ap.add_argument('--new-tokens', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from image2text_amd import synth
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    assert torch.cuda.is_available(), 'bench_top_logprobs.py measures on the MI355X; there is nothing to report without one'
    Ks = [int(k) for k in a.ks.split(',')]
    cfg = synth.nano224_config()
    if a.model == 'nano704':            # the benchmark model as it stands, with only the decoder's width and heads replaced
        dc = cfg.decoder_config
        tf = dc.transformer_config
        attn = tf.attn_config.model_copy(update=dict(n_embd=704, n_head=11))
        cfg = cfg.model_copy(update=dict(decoder_config=dc.model_copy(update=dict(transformer_config=tf.model_copy(update=dict(attn_config=attn))))))
    m = VisionEncoderDecoder(cfg)
    synth.det_init_(m, seed=0)
    m = m.to('cuda').eval()
    V, B, T = m._engine.dec.V, a.captions, a.new_tokens
    images = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to('cuda')
    prompt = torch.full((B, 1), V - 1, dtype=torch.long, device='cuda')
    call = lambda K: m.generate_captions(images, prompt, max_new_tokens=T, top_k=1, poll_every=0, **({'top_logprobs': K} if K else {}))
    print(f'device: {torch.cuda.get_device_name(0)}; package: {os.path.abspath(a.root)}; {a.model} (decoder width {m._engine.dec.d}), {B} captions x '
          f'{T} new tokens, greedy, {a.rounds} alternating rounds after one warm-up call per K', flush=True)
    ts = {K: [] for K in Ks}
    for K in Ks:
        call(K)
    for _ in range(a.rounds):
        for K in Ks:
            ts[K].append(timed(lambda: call(K))[0])
    base = statistics.median(ts[Ks[0]])
    for K in Ks:
        med = statistics.median(ts[K])
        print(f'K = {K}: {med:8.1f} [{min(ts[K]):.1f} .. {max(ts[K]):.1f}] ms  {B / med * 1e3:9.0f} captions/s  x{med / base:.3f} of K = {Ks[0]}', flush=True)


if __name__ == '__main__':
    main()
