"""Decoded uint8 pixels -> the fp32 [B, 3, H, W] tensor every entry point of the package takes, on the device, in one launch.

The reference does this on the host, per image (trainer.py: ``ToTensor -> Resize((S, S)) -> Normalize(mean, std)``).  Here:

    out[k] = (resize(u[..., k] / 255) - mean[k]) / std[k]

with ``resize = torch.nn.functional.interpolate(x, size=(H, W), mode='bilinear', align_corners=False, antialias=antialias)``, the call
torchvision's ``Resize`` makes on a float tensor.  ``pack_images`` concatenates a batch of images of different sizes into one buffer
(one upload), ``preprocess_images`` launches csrc/preprocess.hip on it, ``preprocess_images_host`` restates the semantics in numpy
float64 and is what the kernel is held to (tests/test_preprocess_gpu.py).  DESIGN.md section 4y.
"""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MAX_SIDE = 16384          # csrc/preprocess.hip: a source row (3 * 16384 bytes) must fit an LDS row buffer; outputs share the cap
TAIL_PAD = 16             # the kernel reads rows with 16-byte loads aligned down: the last one may run this far past the last image


class PackedImages(tuple):
    """(data, offsets, shapes) of a batch, with ``max_side`` (the largest h or w, known on the host) riding along:
    data uint8 [total + TAIL_PAD], the images end to end, each as [h, w, c] rows; offsets int64 [B], the byte at which image b starts;
    shapes int32 [B, 3], (h, w, c) per image."""

    def __new__(cls, data: torch.Tensor, offsets: torch.Tensor, shapes: torch.Tensor, max_side: int):
        self = super().__new__(cls, (data, offsets, shapes))
        self.max_side = int(max_side)
        return self

    data = property(lambda self: self[0])
    offsets = property(lambda self: self[1])
    shapes = property(lambda self: self[2])

    def to(self, device) -> 'PackedImages':
        return self if self.data.device == device else PackedImages(*(t.to(device) for t in self), self.max_side)


# ---- the resize, one axis at a time (normative; the kernel evaluates the same expressions in fp64)
def resize_taps(n: int, m: int, antialias: bool) -> Tuple[np.ndarray, np.ndarray]:
    """Axis weights of ``n`` source -> ``m`` output samples: (lo, hi) int [m] and the dense float64 matrix [m, n] whose row i holds the
    weights of output sample i on source samples lo[i] <= j < hi[i] (zero elsewhere)."""
    scale = n / m
    lo, hi, mat = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros((m, n), dtype=np.float64)
    for i in range(m):
        if antialias:
            support = max(scale, 1.0)
            inv = 1.0 / scale if scale >= 1.0 else 1.0
            c = scale * (i + 0.5)
            lo[i], hi[i] = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)          # int(): toward zero
            j = np.arange(lo[i], hi[i], dtype=np.float64)
            w = np.maximum(0.0, 1.0 - np.abs((j - c + 0.5) * inv))
            total = 0.0
            for x in w:                                   # in index order, as the kernel sums them
                total += float(x)
            mat[i, lo[i]:hi[i]] = w / total
        else:
            s = max(scale * (i + 0.5) - 0.5, 0.0)
            j0 = min(int(s), n - 1)
            j1 = min(j0 + 1, n - 1)
            lo[i], hi[i] = j0, j1 + 1
            if j1 == j0:
                mat[i, j0] = 1.0                          # both taps on the clamped last sample: (1 - l) + l
            else:
                mat[i, j0], mat[i, j1] = 1.0 - (s - j0), s - j0
    return np.stack([lo, hi], axis=1), mat


def normalisation(mean, std) -> Tuple[np.ndarray, np.ndarray]:
    """(a, b) fp32 [3] with out = v * a + b on raw 0..255 values: a = 1 / (255 std), b = -mean / std, formed in fp64, rounded once."""
    mean, std = _three(mean, 'mean'), _three(std, 'std')
    if np.any(std == 0.0):
        raise ValueError(f'std must not contain 0, got {tuple(std)}')
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def _three(v, what) -> np.ndarray:
    try:
        arr = np.asarray([float(x) for x in v], dtype=np.float64)
    except TypeError:
        raise ValueError(f'{what} must be three numbers, got {v!r}') from None
    if arr.shape != (3,):
        raise ValueError(f'{what} must be three numbers, got {len(arr)}')
    if not np.all(np.isfinite(arr)):
        raise ValueError(f'{what} must be finite, got {tuple(arr)}')
    return arr


def _size(size) -> Tuple[int, int]:
    ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) and s > 0
                                                                    for s in size)
    if not ok:
        raise ValueError(f'size must be two positive ints (H, W), got {size!r}')
    if max(size) > MAX_SIDE:
        raise ValueError(f'size {tuple(size)} exceeds the cap of {MAX_SIDE} per side')
    return int(size[0]), int(size[1])


def _image_list(images) -> Sequence[torch.Tensor]:
    """a uint8 tensor [B, h, w, c] or a sequence of uint8 tensors [h, w, c] -> the list of images, every refusal made"""
    if isinstance(images, PackedImages):
        raise ValueError('images are packed already')
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError(f'a batch tensor must be [B, h, w, c], got {tuple(images.shape)}')
        images = list(images.unbind(0))
    images = list(images)
    if not images:
        raise ValueError('no images')
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor):
            raise ValueError(f'image {i}: want a uint8 tensor [h, w, c], got {type(im).__name__}')
        if im.dtype != torch.uint8:
            raise ValueError(f'image {i}: want uint8 pixels, got {im.dtype}')
        if im.dim() != 3:
            raise ValueError(f'image {i}: want [h, w, c], got {tuple(im.shape)}')
        h, w, c = im.shape
        if c not in (1, 3):
            raise ValueError(f'image {i}: {c} channels (1 or 3 are supported)')
        if h == 0 or w == 0:
            raise ValueError(f'image {i} is empty: {tuple(im.shape)}')
        if max(h, w) > MAX_SIDE:
            raise ValueError(f'image {i}: {h}x{w} exceeds the cap of {MAX_SIDE} per side')
    return images


def pack_images(images, device=None) -> PackedImages:
    """One concatenated uint8 buffer (plus TAIL_PAD bytes), the byte offsets and the (h, w, c) rows of a batch: a uint8 tensor
    [B, h, w, c] or a sequence of uint8 [h_b, w_b, c_b] tensors, on the CPU or a device, c in {1, 3}.  Host images are joined on the
    host and uploaded once; ``device=None`` leaves the result where the images are."""
    images = _image_list(images)
    device = torch.device(device) if device is not None else images[0].device
    shapes = torch.tensor([list(im.shape) for im in images], dtype=torch.int32)
    sizes = shapes.to(torch.int64).prod(dim=1)
    offsets = torch.cumsum(sizes, 0) - sizes
    parts = [im.contiguous().view(-1) for im in images]
    pad = torch.zeros(TAIL_PAD, dtype=torch.uint8, device=parts[0].device)
    if all(p.device == parts[0].device for p in parts):
        data = torch.cat(parts + [pad]).to(device)
    else:
        data = torch.cat([p.to(device) for p in parts] + [pad.to(device)])
    return PackedImages(data, offsets.to(device), shapes.to(device), int(shapes[:, :2].max()))


def preprocess_images(images, size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), antialias: bool = True, device=None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 images (what ``pack_images`` takes, or its result) -> fp32 [B, 3, H, W] on the device, ``size = (H, W)``: each image
    resized (bilinear, antialiased by default as in torchvision) and normalised, in one launch.  A one-channel image is replicated to
    the three channels.  Every refusal is a ValueError raised before anything is launched."""
    from . import ops
    H, W = _size(size)
    a, b = normalisation(mean, std)
    if not isinstance(images, PackedImages):
        images = _image_list(images)
    B = images.offsets.numel() if isinstance(images, PackedImages) else len(images)
    if device is None:                                    # where the images are, if that is a device; else the current one
        first = images.data if isinstance(images, PackedImages) else images[0]
        device = first.device if first.is_cuda else torch.device('cuda')
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'preprocess_images runs on the device; got device={device} (preprocess_images_host is the host form)')
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous float32 tensor of shape {(B, 3, H, W)}')
        if out.device.type != 'cuda' or (device.index is not None and out.device.index != device.index):
            raise ValueError(f'out is on {out.device}, the images go to {device}')
        device = out.device
    elif device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    packed = images.to(device) if isinstance(images, PackedImages) else pack_images(images, device)
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        ops.preprocess_images(packed.data, packed.offsets, packed.shapes, out, a, b, packed.max_side, antialias)
    return out


def preprocess_images_host(images, size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), antialias: bool = True) -> np.ndarray:
    """The semantics of ``preprocess_images`` in numpy float64 -> [B, 3, H, W] float64 (width first, then height)."""
    H, W = _size(size)
    mean, std = _three(mean, 'mean'), _three(std, 'std')
    if np.any(std == 0.0):
        raise ValueError(f'std must not contain 0, got {tuple(std)}')
    images = _image_list(images)
    out = np.empty((len(images), 3, H, W), dtype=np.float64)
    taps = {}
    for b, im in enumerate(images):
        u = im.cpu().numpy().astype(np.float64) / 255.0
        h, w, c = u.shape
        for n, m in ((w, W), (h, H)):
            if (n, m) not in taps:
                taps[(n, m)] = resize_taps(n, m, antialias)[1]
        for k in range(3):
            plane = np.ascontiguousarray(u[:, :, k if c == 3 else 0])          # (one layout: a gray image and its RGB copy agree bit for bit)
            out[b, k] = (taps[(h, H)] @ (plane @ taps[(w, W)].T) - mean[k]) / std[k]
    return out


def tap_counts(shape, size, antialias: bool) -> Tuple[int, int]:
    """(n_h, n_v): the most taps one output sample of an [h, w] image resized to ``size`` has along the width and the height"""
    (h, w), (H, W) = shape, size
    th, tv = resize_taps(w, W, antialias)[0], resize_taps(h, H, antialias)[0]
    return int((th[:, 1] - th[:, 0]).max()), int((tv[:, 1] - tv[:, 0]).max())


__all__ = ['MAX_SIDE', 'PackedImages', 'pack_images', 'preprocess_images', 'preprocess_images_host', 'normalisation', 'resize_taps',
           'tap_counts']
