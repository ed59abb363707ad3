"""Decoded uint8 pixels -> the fp32 [B, 3, H, W] tensor every entry point of the package takes, on the device, in one launch.

The reference does this on the host, per image (trainer.py: ``ToTensor -> Resize((S, S)) -> Normalize(mean, std)``).  Here:

    out[k] = (resize(u[..., k] / 255) - mean[k]) / std[k]

with ``resize = torch.nn.functional.interpolate(x, size=(H, W), mode='bilinear', align_corners=False, antialias=antialias)``, the call
torchvision's ``Resize`` makes on a float tensor.  ``pack_images`` concatenates a batch of images of different sizes into one buffer
(one upload), ``preprocess_images`` launches csrc/preprocess.hip on it, ``preprocess_images_host`` restates the semantics in numpy
float64 and is what the kernel is held to (tests/test_preprocess_gpu.py).  DESIGN.md section 4y.

Boxes and flips.  With ``boxes`` / ``box_index`` / ``flip``, output r names a source image, an integer box inside it
and a flip bit; the batch is uploaded once and R outputs (R need not be B) come out of one launch:

    crop   = image[src][top : top + bh, left : left + bw, :]            # inside the image, bh, bw >= 1
    y      = normalise(resize(crop / 255, (H, W)))                      # exactly preprocess_images_host([crop], ...)
    out[r] = y[..., ::-1] if flip else y                                # the flip is taken AFTER the resize

-- torchvision's ``resized_crop(img, top, left, height, width, size)`` followed by ``hflip``.  Taps clamp at the BOX's edges, never the
image's: pixels outside the box do not contribute.  ``preprocess_regions_host`` is these three lines over ``preprocess_images_host``;
``full_boxes``, ``center_boxes``, ``random_resized_crop_boxes`` and ``random_flips`` make the boxes and flips of the usual transforms
(whole image, ``CenterCrop``, ``RandomResizedCrop``, ``RandomHorizontalFlip``) from the image shapes, on the host.
"""
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MAX_SIDE = 16384          # csrc/preprocess.hip: a source row (3 * 16384 bytes) must fit an LDS row buffer; outputs share the cap
TAIL_PAD = 16             # the kernel reads rows with 16-byte loads aligned down: the last one may run this far past the last image


class PackedImages(tuple):
    """(data, offsets, shapes) of a batch, with ``max_side`` (the largest h or w, known on the host) and ``host_shapes`` (the rows of
    ``shapes`` as a tuple of (h, w, c), on the host: what validating boxes needs) riding along:
    data uint8 [total + TAIL_PAD], the images end to end, each as [h, w, c] rows; offsets int64 [B], the byte at which image b starts;
    shapes int32 [B, 3], (h, w, c) per image."""

    def __new__(cls, data: torch.Tensor, offsets: torch.Tensor, shapes: torch.Tensor, max_side: int, host_shapes=None):
        self = super().__new__(cls, (data, offsets, shapes))
        self.max_side = int(max_side)
        self._host_shapes = None if host_shapes is None else tuple(tuple(int(v) for v in row) for row in host_shapes)
        return self

    data = property(lambda self: self[0])
    offsets = property(lambda self: self[1])
    shapes = property(lambda self: self[2])

    @property
    def host_shapes(self):
        if self._host_shapes is None:                     # built by hand without them: read back once, then kept
            self._host_shapes = tuple(tuple(row) for row in self.shapes.cpu().tolist())
        return self._host_shapes

    def to(self, device) -> 'PackedImages':
        return self if self.data.device == device else PackedImages(*(t.to(device) for t in self), self.max_side, self._host_shapes)


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
    return PackedImages(data, offsets.to(device), shapes.to(device), int(shapes[:, :2].max()), shapes.tolist())


def _int_array(v, what, cols=None) -> np.ndarray:
    """an int tensor, array or sequence -> int64 numpy [R] (``cols=None``) or [R, cols]; bools and floats are refused"""
    if isinstance(v, torch.Tensor):
        if v.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f'{what} must hold integers, got {v.dtype}')
        arr = v.detach().cpu().numpy()
    else:
        try:
            arr = np.asarray(v)
        except Exception:
            raise ValueError(f'{what} must be a tensor or a sequence of integers, got {type(v).__name__}') from None
        if arr.size and arr.dtype.kind not in 'iu':
            raise ValueError(f'{what} must hold integers, got {arr.dtype}')
    want = (arr.ndim == 1) if cols is None else (arr.ndim == 2 and arr.shape[1] == cols)
    if not want:
        raise ValueError(f'{what} must be [R{"" if cols is None else f", {cols}"}], got {tuple(arr.shape)}')
    return arr.astype(np.int64)


def _hw(shapes) -> np.ndarray:
    """the image shapes of a batch -> int64 numpy [B, 2] = (h, w): a ``PackedImages``, or an int tensor, array or sequence [B, 2] of
    (h, w) or [B, 3] of (h, w, c)"""
    if isinstance(shapes, PackedImages):
        shapes = shapes.host_shapes
    if isinstance(shapes, torch.Tensor):
        shapes = shapes.detach().cpu().numpy()
    arr = np.asarray(shapes)
    if arr.ndim != 2 or arr.shape[0] == 0 or arr.shape[1] not in (2, 3) or arr.dtype.kind not in 'iu':
        raise ValueError(f'shapes must be integers [B, 2] (h, w) or [B, 3] (h, w, c), B >= 1, got {arr.dtype} {tuple(arr.shape)}')
    arr = arr[:, :2].astype(np.int64)
    if (arr < 1).any():
        raise ValueError('shapes must be positive')
    return arr


def _regions(shapes, boxes, box_index, flip) -> np.ndarray:
    """The rows (src, top, left, bh, bw, flip) the kernel takes, int32 numpy [R, 6], from the public arguments, every refusal made.
    ``shapes``: the (h, w[, c]) rows of the batch, on the host."""
    hw = _hw(shapes)
    B = len(hw)
    if boxes is None:
        if box_index is not None:
            raise ValueError('box_index without boxes')
        boxes = np.concatenate([np.zeros_like(hw), hw], axis=1)          # flip alone: the whole of every image
    else:
        boxes = _int_array(boxes, 'boxes', 4)
    R = len(boxes)
    if R == 0:
        raise ValueError('no boxes')
    if box_index is None:
        if R != B:
            raise ValueError(f'{R} boxes for {B} images: box_index must say which image each box is of')
        box_index = np.arange(B, dtype=np.int64)
    else:
        box_index = _int_array(box_index, 'box_index')
        if len(box_index) != R:
            raise ValueError(f'box_index has {len(box_index)} entries for {R} boxes')
        if ((box_index < 0) | (box_index >= B)).any():
            raise ValueError(f'box_index must lie in [0, {B}), got {box_index[(box_index < 0) | (box_index >= B)][0]}')
    if flip is None:
        flip = np.zeros(R, dtype=np.int64)
    else:
        if isinstance(flip, torch.Tensor):
            flip = flip.detach().cpu().numpy()
        try:
            flip = np.asarray(flip)
        except Exception:
            raise ValueError(f'flip must be a tensor or a sequence of bools, got {type(flip).__name__}') from None
        if flip.ndim != 1 or (flip.size and flip.dtype.kind not in 'biu'):
            raise ValueError(f'flip must be [R] bools, got {flip.dtype} {tuple(flip.shape)}')
        if len(flip) != R:
            raise ValueError(f'flip has {len(flip)} entries for {R} boxes')
        flip = flip.astype(np.int64)
        if ((flip != 0) & (flip != 1)).any():
            raise ValueError('flip must hold bools (0 or 1)')
    top, left, bh, bw = boxes.T
    h, w = hw[box_index].T
    bad = (top < 0) | (left < 0) | (bh < 1) | (bw < 1) | (top + bh > h) | (left + bw > w)
    if bad.any():
        r = int(np.argmax(bad))
        raise ValueError(f'box {r} (top, left, height, width) = {tuple(int(v) for v in boxes[r])} is not inside its {h[r]} x {w[r]} image')
    return np.concatenate([box_index[:, None], boxes, flip[:, None]], axis=1).astype(np.int32)


def preprocess_images(images, size, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), antialias: bool = True, device=None,
                      out: Optional[torch.Tensor] = None, boxes=None, box_index=None, flip=None) -> torch.Tensor:
    """uint8 images (what ``pack_images`` takes, or its result) -> fp32 [B, 3, H, W] on the device, ``size = (H, W)``: each image
    resized (bilinear, antialiased by default as in torchvision) and normalised, in one launch.  A one-channel image is replicated to
    the three channels.  Every refusal is a ValueError raised before anything is launched.

    ``boxes``: an int [R, 4] tensor or sequence of (top, left, height, width), torchvision's order -- output r is that box of image
    ``box_index[r]`` (int [R]; default ``arange(B)``, which needs R == B) resized to ``size``, and mirrored left to right where
    ``flip[r]`` ([R] bools) is set; ``flip`` alone mirrors whole images.  The result and ``out`` are then [R, 3, H, W]; the images are
    uploaded once however many boxes name them (module docstring).  A box must lie inside its image."""
    from . import ops
    H, W = _size(size)
    a, b = normalisation(mean, std)
    if not isinstance(images, PackedImages):
        images = _image_list(images)
    regions = None
    if boxes is not None or flip is not None:
        host_shapes = images.host_shapes if isinstance(images, PackedImages) else [tuple(im.shape) for im in images]
        regions = _regions(host_shapes, boxes, box_index, flip)
    elif box_index is not None:
        raise ValueError('box_index without boxes')
    B = len(regions) if regions is not None else images.offsets.numel() if isinstance(images, PackedImages) else len(images)
    if device is None:                                   # where the images are, if that is a device; else the current one
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
        if regions is None:
            ops.preprocess_images(packed.data, packed.offsets, packed.shapes, out, a, b, packed.max_side, antialias)
        else:
            ops.preprocess_regions(packed.data, packed.offsets, packed.shapes, torch.from_numpy(regions).to(device), out, a, b,
                                   packed.max_side, antialias)
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


def preprocess_regions_host(images, size, boxes, box_index=None, flip=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                            antialias: bool = True) -> np.ndarray:
    """The semantics of ``preprocess_images(..., boxes=, box_index=, flip=)`` in numpy float64 -> [R, 3, H, W] float64: the three lines
    of the module docstring over ``preprocess_images_host`` on the slices, so the two replicas cannot drift apart."""
    _size(size)
    images = _image_list(images)
    regions = _regions([tuple(im.shape) for im in images], boxes, box_index, flip)
    rows = []
    for src, top, left, bh, bw, fl in regions.tolist():
        y = preprocess_images_host([images[src][top:top + bh, left:left + bw, :]], size, mean, std, antialias)[0]
        rows.append(y[..., ::-1] if fl else y)
    return np.ascontiguousarray(np.stack(rows))


# ---- boxes and flips of the usual transforms: pure functions of the image shapes, on the host
def full_boxes(shapes) -> torch.Tensor:
    """int64 [B, 4]: (0, 0, h, w), the whole of every image.  ``shapes``: a ``PackedImages``, or [B, 2] (h, w) / [B, 3] (h, w, c)."""
    hw = _hw(shapes)
    return torch.from_numpy(np.concatenate([np.zeros_like(hw), hw], axis=1))


def center_boxes(shapes, size, fraction: float = 1.0) -> torch.Tensor:
    """int64 [B, 4]: the largest centred box of every image with the aspect ratio of ``size = (H, W)``, its sides scaled by ``fraction``
    (0.875 is the usual 224 / 256) -- ``Resize`` of the short side followed by ``CenterCrop``, as one box.  Per image (h, w):

        (fh, fw) = (h, h W / H) if w H >= W h else (w H / W, w)         # the image is wider than the target, or taller
        bh = min(h, max(1, int(round(fraction fh)))),  bw = min(w, max(1, int(round(fraction fw))))
        top = (h - bh) // 2,  left = (w - bw) // 2

    (``round`` is Python's: halves go to the even integer.)"""
    H, W = _size(size)
    fraction = float(fraction)
    if not (math.isfinite(fraction) and fraction > 0.0):
        raise ValueError(f'fraction must be a positive number, got {fraction}')
    out = []
    for h, w in _hw(shapes).tolist():
        fh, fw = (h, h * W / H) if w * H >= W * h else (w * H / W, w)
        bh, bw = min(h, max(1, int(round(fraction * fh)))), min(w, max(1, int(round(fraction * fw))))
        out.append(((h - bh) // 2, (w - bw) // 2, bh, bw))
    return torch.tensor(out, dtype=torch.int64)


def _range(v, what) -> Tuple[float, float]:
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be two numbers (low, high), got {v!r}') from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f'{what} must be 0 < low <= high, got {(lo, hi)}')
    return lo, hi


def rrc_fallback_box(h: int, w: int, ratio=(3 / 4, 4 / 3)) -> Tuple[int, int, int, int]:
    """the box ``random_resized_crop_boxes`` takes when none of its ten attempts fits: central, the whole image clipped to the ratio range"""
    r0, r1 = _range(ratio, 'ratio')
    if w / h < r0:
        bw, bh = w, int(round(w / r0))
    elif w / h > r1:
        bh, bw = h, int(round(h * r1))
    else:
        bh, bw = h, w
    bh, bw = min(h, max(1, bh)), min(w, max(1, bw))
    return (h - bh) // 2, (w - bw) // 2, bh, bw


def random_resized_crop_boxes(shapes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int64 [B, 4]: one random box per image by the algorithm of torchvision's ``RandomResizedCrop.get_params`` -- up to ten attempts of
    area = U(scale) h w and aspect ratio (w / h) log-uniform over ``ratio``, sides ``bw = round(sqrt(area aspect))``,
    ``bh = round(sqrt(area / aspect))`` accepted if 0 < bw <= w and 0 < bh <= h, then placed at a uniform integer position; after ten
    misses the central box of the whole image clipped to the ratio range (``rrc_fallback_box``).  The DISTRIBUTION is torchvision's; the
    random STREAM is not: all draws come from ``generator`` as one ``torch.rand(B, 10, 4)`` in float64 (area, aspect, top, left of each
    attempt; a position is ``int(u (h - bh + 1))``), so equal seeds give equal boxes here and boxes that differ from torchvision's."""
    s0, s1 = _range(scale, 'scale')
    r0, r1 = _range(ratio, 'ratio')
    hw = _hw(shapes).tolist()
    u = torch.rand(len(hw), 10, 4, generator=generator, dtype=torch.float64).numpy()
    l0, l1 = math.log(r0), math.log(r1)
    out = []
    for (h, w), draws in zip(hw, u):
        box = None
        for ua, ur, ui, uj in draws.tolist():
            area = h * w * (s0 + (s1 - s0) * ua)
            aspect = math.exp(l0 + (l1 - l0) * ur)
            bw, bh = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < bw <= w and 0 < bh <= h:
                box = (min(int(ui * (h - bh + 1)), h - bh), min(int(uj * (w - bw + 1)), w - bw), bh, bw)
                break
        out.append(box if box is not None else rrc_fallback_box(h, w, (r0, r1)))
    return torch.tensor(out, dtype=torch.int64)


def random_flips(n: int, p: float = 0.5, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """bool [n]: True with probability ``p`` (``RandomHorizontalFlip``), drawn from ``generator``"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f'n must be a positive int, got {n!r}')
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f'p must lie in [0, 1], got {p}')
    return torch.rand(int(n), generator=generator, dtype=torch.float64) < p


def tap_counts(shape, size, antialias: bool) -> Tuple[int, int]:
    """(n_h, n_v): the most taps one output sample of an [h, w] image resized to ``size`` has along the width and the height"""
    (h, w), (H, W) = shape, size
    th, tv = resize_taps(w, W, antialias)[0], resize_taps(h, H, antialias)[0]
    return int((th[:, 1] - th[:, 0]).max()), int((tv[:, 1] - tv[:, 0]).max())


__all__ = ['MAX_SIDE', 'PackedImages', 'pack_images', 'preprocess_images', 'preprocess_images_host', 'preprocess_regions_host',
           'normalisation', 'resize_taps', 'tap_counts', 'full_boxes', 'center_boxes', 'random_resized_crop_boxes', 'rrc_fallback_box',
           'random_flips']
