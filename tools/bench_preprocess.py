#!/usr/bin/env python3
"""Image preprocessing (uint8 pixels -> normalised fp32 [B, 3, 224, 224]) three ways, in images/s:

  (a) preprocess.preprocess_images (csrc/preprocess.hip): 3072 images of mixed Flickr-like sizes around 500 x 375, one launch;
      packed buffer already on the device (the kernel alone), and from host tensors (join + one upload + the kernel)
  (b) the same transform as torch ops on the device: equal-size images only (torch cannot batch ragged ones), 500 x 375, in chunks
  (c) the torch CPU pipeline, image by image, on 16 threads (the reference's ToTensor -> Resize -> Normalize)

    python tools/bench_preprocess.py [out.txt] [--images N]
    python tools/bench_preprocess.py [out.txt] [--images N] --regions R

With ``--regions R`` it measures boxes instead: R random-resized-crop boxes of each of N images (default 64), half of
them flipped, as ONE launch over the batch uploaded once, against what a caller without boxes does -- slice every box on the host and
hand the list of N R crops to preprocess_images, which joins and uploads every crop's pixels.

Device times are events around a window of back-to-back calls after a warm-up, ROUNDS windows, median [min .. max].  The kernel's
share of the HBM roof counts its own bytes (source bytes + 12 H W per image) against 6.29 TB/s, the measured copy rate of the card."""
import concurrent.futures
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image2text_amd import preprocess as pp  # noqa: E402

dev = torch.device('cuda:0')
SIZE = (224, 224)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_ROOF = 6.29e12
ROUNDS, WINDOW, CPU_IMAGES, CPU_THREADS, TORCH_CHUNK = 5, 20, 256, 16, 256
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def flickr_like(n, seed=0):
    """n uint8 images: landscape 500 x (333 .. 375 .. 400) and portrait (333 .. 375) x 500, one in twelve gray"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        short = int(torch.randint(300, 401, (1,), generator=g))
        h, w = (short, 500) if i % 4 else (500, short)
        out.append(torch.randint(0, 256, (h, w, 1 if i % 12 == 11 else 3), generator=g, dtype=torch.uint8))
    return out


def windows(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms), min(ms), max(ms)


def torch_chain(x_u8, mean, std):
    """[B, h, w, 3] uint8 on any device -> [B, 3, H, W] fp32: ToTensor, Resize (antialiased), Normalize as torch ops"""
    x = x_u8.permute(0, 3, 1, 2).float() / 255.0
    y = F.interpolate(x, size=SIZE, mode='bilinear', align_corners=False, antialias=True)
    return (y - mean) / std


def host_clock(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def regions_mode(n, per_image):
    """R boxes per image in one launch against slicing on the host"""
    say(f'device: {torch.cuda.get_device_name(0)}; {n} images x {per_image} boxes -> {SIZE[0]}x{SIZE[1]}, antialiased')
    ims = flickr_like(n)
    g = torch.Generator().manual_seed(2)
    index = torch.arange(n).repeat_interleave(per_image)
    boxes = pp.random_resized_crop_boxes([ims[i].shape for i in index.tolist()], generator=g)
    flip = pp.random_flips(len(index), generator=g)
    R = len(index)
    src_bytes = sum(im.numel() for im in ims)
    crop_bytes = int(sum(bh * bw * ims[i].shape[2] for i, (_, _, bh, bw) in zip(index.tolist(), boxes.tolist())))
    out = torch.empty(R, 3, *SIZE, device=dev)
    packed = pp.pack_images(ims, dev)
    med, lo, hi = windows(lambda: pp.preprocess_images(packed, SIZE, MEAN, STD, out=out, boxes=boxes, box_index=index, flip=flip), WINDOW)
    say(f'(r1) {R} boxes of the packed batch on the device, one launch (validation and the {24 * R} bytes of regions included): '
        f'{med:.3f} [{lo:.3f} .. {hi:.3f}] ms = {R / med * 1e3:,.0f} outputs/s')
    dt = host_clock(lambda: pp.preprocess_images(ims, SIZE, MEAN, STD, out=out, boxes=boxes, box_index=index, flip=flip))
    say(f'(r2) the same from host tensors (join + one upload of {src_bytes / 1e6:.1f} MB + the launch), host clock: {dt * 1e3:.2f} ms = '
        f'{R / dt:,.0f} outputs/s')
    got = out.clone()

    def sliced():
        crops = [ims[i][t:t + bh, l:l + bw] for i, (t, l, bh, bw) in zip(index.tolist(), boxes.tolist())]
        return pp.preprocess_images(crops, SIZE, MEAN, STD, out=out)

    dt_s = host_clock(sliced)
    say(f'(r3) slicing the boxes on the host and preprocess_images on the {R} crops (join + upload of {crop_bytes / 1e6:.1f} MB + the launch), '
        f'host clock: {dt_s * 1e3:.2f} ms = {R / dt_s:,.0f} outputs/s ({dt_s / dt:.2f} x the time of (r2))')
    want = torch.where(flip.to(dev)[:, None, None, None], torch.flip(out, [-1]), out)          # the parent has no flip: mirrored here
    say(f'    the two results are {"bit-equal" if torch.equal(got, want) else "NOT bit-equal: max |diff| %.3e" % float((got - want).abs().max())}')


def main():
    assert torch.cuda.is_available(), 'bench_preprocess.py measures on the MI355X; there is nothing to report without one'
    if '--regions' in sys.argv:
        i = sys.argv.index('--regions')
        per_image = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        n = 64
        if '--images' in sys.argv:
            i = sys.argv.index('--images')
            n = int(sys.argv[i + 1])
            del sys.argv[i:i + 2]
        regions_mode(n, per_image)
        if len(sys.argv) > 1:
            with open(sys.argv[1], 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
        return
    n = int(sys.argv[sys.argv.index('--images') + 1]) if '--images' in sys.argv else 3072
    say(f'device: {torch.cuda.get_device_name(0)}; {n} images -> {SIZE[0]}x{SIZE[1]}, antialiased; {ROUNDS} windows, median [min .. max]')
    ims = flickr_like(n)
    src_bytes = sum(im.numel() for im in ims)
    own_bytes = src_bytes + 12 * SIZE[0] * SIZE[1] * n

    # (a) the kernel
    packed = pp.pack_images(ims, dev)
    out = torch.empty(n, 3, *SIZE, device=dev)
    med, lo, hi = windows(lambda: pp.preprocess_images(packed, SIZE, MEAN, STD, out=out), WINDOW)
    say(f'(a) preprocess_images, packed on the device: {med:.3f} [{lo:.3f} .. {hi:.3f}] ms = {n / med * 1e3:,.0f} images/s; '
        f'{own_bytes / 1e6:.0f} MB of its own bytes ({src_bytes / 1e6:.0f} source) = {own_bytes / med / 1e9:.2f} TB/s = '
        f'{own_bytes / (med * 1e-3) / HBM_ROOF:.1%} of the {HBM_ROOF / 1e12:.2f} TB/s roof')
    med_p, lo_p, hi_p = windows(lambda: pp.preprocess_images(packed, SIZE, MEAN, STD, antialias=False, out=out), WINDOW)
    say(f'    plain (antialias=False): {med_p:.3f} [{lo_p:.3f} .. {hi_p:.3f}] ms = {n / med_p * 1e3:,.0f} images/s')
    t0 = time.perf_counter()
    for _ in range(3):
        pp.preprocess_images(ims, SIZE, MEAN, STD, out=out)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    say(f'    from host tensors (join on the host + one upload of {src_bytes / 1e6:.0f} MB + the kernel), host clock: {dt * 1e3:.1f} ms = '
        f'{n / dt:,.0f} images/s')

    # (b) torch ops on the device, equal sizes
    mean_d, std_d = (torch.tensor(v, device=dev)[None, :, None, None] for v in (MEAN, STD))
    g = torch.Generator().manual_seed(1)
    same = torch.randint(0, 256, (TORCH_CHUNK, 375, 500, 3), generator=g, dtype=torch.uint8).to(dev)
    med_t, lo_t, hi_t = windows(lambda: torch_chain(same, mean_d, std_d), WINDOW)
    say(f'(b) torch ops on the device, {TORCH_CHUNK} equal 375x500 images per call: {med_t:.3f} [{lo_t:.3f} .. {hi_t:.3f}] ms = '
        f'{TORCH_CHUNK / med_t * 1e3:,.0f} images/s')
    same_packed = pp.pack_images(same)
    out_s = torch.empty(TORCH_CHUNK, 3, *SIZE, device=dev)
    med_s, lo_s, hi_s = windows(lambda: pp.preprocess_images(same_packed, SIZE, MEAN, STD, out=out_s), WINDOW)
    say(f'    preprocess_images on the same {TORCH_CHUNK} images: {med_s:.3f} [{lo_s:.3f} .. {hi_s:.3f}] ms = {TORCH_CHUNK / med_s * 1e3:,.0f} images/s '
        f'({med_t / med_s:.2f} x the torch ops)')
    diff = float((torch_chain(same, mean_d, std_d) - out_s).abs().max())
    say(f'    max |torch ops - kernel| on them: {diff:.2e}')

    # (c) the CPU pipeline
    torch.set_num_threads(1)
    mean_c, std_c = (torch.tensor(v)[None, :, None, None] for v in (MEAN, STD))
    rgb = [im for im in ims if im.shape[2] == 3][:CPU_IMAGES]

    def one(im):
        return torch_chain(im[None], mean_c, std_c)

    with concurrent.futures.ThreadPoolExecutor(CPU_THREADS) as pool:
        list(pool.map(one, rgb[:CPU_THREADS]))
        t0 = time.perf_counter()
        list(pool.map(one, rgb))
        dt = time.perf_counter() - t0
    say(f'(c) torch CPU pipeline, {CPU_THREADS} threads, one image per call: {len(rgb)} images in {dt * 1e3:.0f} ms = {len(rgb) / dt:,.0f} images/s '
        f'({dt / len(rgb) * CPU_THREADS * 1e3:.2f} ms per image per thread)')
    if len(sys.argv) > 1 and not sys.argv[1].startswith('--'):
        with open(sys.argv[1], 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
