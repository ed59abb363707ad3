"""csrc/preprocess.hip on the MI355X against the float64 replica (image2text_amd/preprocess.py::preprocess_images_host), on the
smallest shapes at which it can go wrong, with a bound derived from the tap counts, bit-exact cases, and torch's own float32 result.

The bound.  u = 2^-24 (fp32 unit roundoff), values v <= 255, weights w >= 0 that sum to 1 per axis.
  * A weight is evaluated in fp64 and rounded once: w~ = w (1 + d), |d| <= u.
  * The horizontal sum of n_h taps is a chain of n_h fp32 fmas: every term meets at most n_h roundings besides its weight's, so
    |s~ - s| <= (n_h + 1) u sum(w v) <= (n_h + 1) u 255, to first order.
  * The vertical sum adds w~ s~ for the n_v source rows of the output row's tap range (rows outside it add an exact 0): likewise
    (n_v + 1) u 255 on top.  Before the normalisation: |acc~ - acc| <= (n_h + n_v + 2) u 255.
  * out = fl(acc~ a~ + b~), a~ = a (1 + d_a), b~ = b (1 + d_b): |a| times the above, + u 255 |a| (a's rounding) + u |b| (b's) +
    u (255 |a| + |b|) (the fma's one rounding of a result that is at most 255 |a| + |b|).
  * One more unit of u 255 |a| covers the second-order terms and the replica's own float64 error (~1e-13 of it).
  bound_k = u ((n_h + n_v + 5) 255 |a_k| + 2 |b_k|)
With |b_k| <= 255 |a_k| (mean <= 1, as here) this is below (n_h + n_v + 8) u 255 |a_k|, the figure the feature was specified with;
the test asserts that too.  n_h, n_v: the most taps any output sample has on that axis (preprocess.tap_counts)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image2text_amd import ops
from image2text_amd import preprocess as pp
from image2text_amd.lib import I2TError

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UNIT = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255,) * 3)           # a = 1, b = 0: the raw resized values

# (h, w, c) -> (H, W).  What each is there for:
CASES = {
    '1x1': ((1, 1, 3), (4, 4)),                      # one source pixel: every tap clamps
    '2x3_up': ((2, 3, 3), (8, 8)),                   # upscale with edge clamps
    '5x9': ((5, 9, 3), (16, 16)),                    # two bands of output rows
    '37x53': ((37, 53, 3), (16, 16)),                # odd width: rows start at every byte residue
    '300x7': ((300, 7, 3), (8, 8)),                  # 75 vertical taps
    '7x300': ((7, 300, 3), (8, 8)),                  # 75 horizontal taps: more than the LDS weight table holds, weights evaluated per use
    '33x41': ((33, 41, 3), (12, 20)),                # non-square output, 12 rows: the second band is half empty
    'gray_9x13': ((9, 13, 1), (16, 16)),             # one channel, replicated
    '12x300_wide_out': ((12, 300, 3), (9, 300)),     # 300 output columns: two column tiles, the second one partly empty
    '2x16384': ((2, 16384, 3), (3, 40)),             # the side cap: row buffers of 48 KB each (more than 64 KB of LDS in all)
    '375x500': ((375, 500, 3), (224, 224)),          # the real shape
}
RAGGED = ['1x1', '2x3_up', 'gray_9x13', '5x9', '37x53', 'gray_7x11', '300x7', '33x41', '7x300', '375x500', 'gray_5x9']
RAGGED_SHAPES = {'gray_7x11': (7, 11, 1), 'gray_5x9': (5, 9, 1)}


def dev():
    return torch.device('cuda:0')


def image(shape, seed=0):
    h, w, c = shape
    g = torch.Generator().manual_seed(seed * 7919 + h * 131 + w * 17 + c)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def bound(shape, size, antialias, mean=MEAN, std=STD):
    """[3, 1, 1] float64: the derived bound per channel (module docstring)"""
    n_h, n_v = pp.tap_counts(shape[:2], size, antialias)
    a, b = (x.astype(np.float64) for x in pp.normalisation(mean, std))
    out = U * ((n_h + n_v + 5) * 255.0 * np.abs(a) + 2.0 * np.abs(b))
    assert (out <= (n_h + n_v + 8) * U * 255.0 * np.abs(a)).all()          # never looser than the specified figure
    return out[:, None, None]


@pytest.fixture(scope='module')
def refs():
    """name -> (image, size, {antialias: float64 replica [3, H, W]}), computed once"""
    out = {}
    for name, (shape, size) in CASES.items():
        im = image(shape)
        out[name] = (im, size, {aa: pp.preprocess_images_host([im], size, MEAN, STD, aa)[0] for aa in (True, False)})
    return out


def check(name, got, ref, bnd):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bnd).max())
    print(f'{name}: max |err| {err.max():.3e}, {worst:.3f} of the bound ({float(bnd.max()):.3e})')
    assert np.isfinite(got).all(), f'{name}: non-finite output'
    assert worst <= 1.0, f'{name}: max |err| {err.max():.3e} is {worst:.2f} x the bound'


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
@pytest.mark.parametrize('name', list(CASES))
def test_one_image_against_the_float64_replica(refs, name, antialias):
    im, size, ref = refs[name]
    got = pp.preprocess_images([im], size, MEAN, STD, antialias, device=dev())                 # B = 1
    assert got.shape == (1, 3) + size and got.dtype == torch.float32 and got.device == dev()
    check(f'{name}.{"aa" if antialias else "plain"}', got[0].cpu().numpy(), ref[antialias], bound(im.shape, size, antialias))


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
def test_a_ragged_batch_in_one_launch(antialias):
    shapes = [CASES[n][0] if n in CASES else RAGGED_SHAPES[n] for n in RAGGED]
    ims = [image(s, seed=3) for s in shapes]
    packed = pp.pack_images(ims, dev())
    assert set((packed.offsets % 4).tolist()) == {0, 1, 2, 3} and len(set((packed.offsets % 16).tolist())) >= 6
    size = (20, 24)
    got = pp.preprocess_images(packed, size, MEAN, STD, antialias)
    ref = pp.preprocess_images_host(ims, size, MEAN, STD, antialias)
    assert got.shape == (len(ims), 3) + size
    for i, (n, s) in enumerate(zip(RAGGED, shapes)):
        check(f'ragged.{n}', got[i].cpu().numpy(), ref[i], bound(s, size, antialias))
    unit = pp.preprocess_images(packed, size, antialias=antialias, **UNIT)
    for i, s in enumerate(shapes):                                          # a gray image: three equal planes before the normalisation
        if s[2] == 1:
            assert torch.equal(unit[i, 0], unit[i, 1]) and torch.equal(unit[i, 0], unit[i, 2])
            assert not torch.equal(unit[i - 1, 0], unit[i - 1, 1])          # (its RGB neighbour's differ)
    # the same images one at a time, and as the list: bit-equal (the position in the buffer changes the loads' alignment, not the sums)
    assert torch.equal(pp.preprocess_images(ims, size, MEAN, STD, antialias, device=dev()), got)
    for i in (2, 4, 9):
        assert torch.equal(pp.preprocess_images([ims[i]], size, MEAN, STD, antialias, device=dev())[0], got[i])


def test_an_equal_size_batch_tensor_and_an_out_buffer():
    batch = torch.stack([image((37, 53, 3), seed=s) for s in range(5)])
    ref = pp.preprocess_images_host(batch, (16, 16), MEAN, STD, True)
    out = torch.full((5, 3, 16, 16), float('nan'), device=dev())
    got = pp.preprocess_images(batch, (16, 16), MEAN, STD, out=out)
    assert got is out
    check('batch_tensor', out.cpu().numpy(), ref, bound((37, 53, 3), (16, 16), True)[None])
    assert torch.equal(pp.preprocess_images(batch.to(dev()), (16, 16), MEAN, STD), out)        # images on the device already
    with pytest.raises(ValueError):
        pp.preprocess_images(batch, (16, 16), out=torch.empty(5, 3, 16, 16, device=dev(), dtype=torch.float16))
    with pytest.raises(ValueError):
        pp.preprocess_images(batch, (16, 16), out=torch.empty(5, 3, 16, 18, device=dev())[..., :16])


def raw(im, size, antialias):
    return pp.preprocess_images([im], size, antialias=antialias, device=dev(), **UNIT)[0].cpu()


def test_exact_cases_are_bit_equal():
    im = image((24, 40, 3), seed=5)
    u = im.permute(2, 0, 1).to(torch.float64)
    for antialias in (True, False):                                         # identity size: the pixels themselves
        assert torch.equal(raw(im, (24, 40), antialias), u.float()), antialias
    g = image((6, 10, 1), seed=5)
    assert torch.equal(raw(g, (6, 10), True), g.permute(2, 0, 1).float().expand(3, -1, -1))
    # plain 2x and 4x downscale: lambda = 1/2 on both axes, the mean of the 2 x 2 samples at (f i + f/2 - 1, f i + f/2)
    for f in (2, 4):
        r0, r1 = u[:, f // 2 - 1::f], u[:, f // 2::f]
        want = (r0[:, :, f // 2 - 1::f] + r0[:, :, f // 2::f] + r1[:, :, f // 2 - 1::f] + r1[:, :, f // 2::f]) / 4
        assert torch.equal(raw(im, (24 // f, 40 // f), False), want.float()), f
    # antialiased 2x downscale, interior rows and columns: weights (1 3 3 1) / 8 on samples 2 i - 1 .. 2 i + 2 of each axis
    got = raw(im, (12, 20), True)
    k = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64) / 8
    want = F.conv2d(u[:, None, 1:, 1:], (k[:, None] * k[None, :])[None, None], stride=2)[:, 0]          # outputs 1 .. m - 2 of each axis
    assert torch.equal(got[:, 1:-1, 1:-1], want.float())


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
@pytest.mark.parametrize('name', ['37x53', '33x41', '375x500'])
def test_torch_float32_is_within_its_own_error_of_the_kernel(refs, name, antialias):
    """torch computes tap positions in float32: the distance between its float32 and its float64 result is the reference's error,
    measured here on the same inputs, and the kernel may differ from torch float32 by no more than that plus its own bound."""
    im, size, _ = refs[name]

    def chain(dtype):
        x = im.permute(2, 0, 1).to(dtype) / 255.0
        y = F.interpolate(x[None], size=size, mode='bilinear', align_corners=False, antialias=antialias)[0]
        return ((y - torch.tensor(MEAN, dtype=dtype)[:, None, None]) / torch.tensor(STD, dtype=dtype)[:, None, None]).numpy().astype(np.float64)

    t32, t64 = chain(torch.float32), chain(torch.float64)
    dist = np.abs(t32 - t64).max(axis=(1, 2), keepdims=True)
    got = pp.preprocess_images([im], size, MEAN, STD, antialias, device=dev())[0].cpu().numpy().astype(np.float64)
    bnd = bound(im.shape, size, antialias)
    diff = np.abs(got - t32)
    print(f'{name}.{"aa" if antialias else "plain"}: torch f32 vs f64 {float(dist.max()):.3e} (normalised; x std = '
          f'{float((dist[:, 0, 0] * np.array(STD)).max()):.3e} of the 0..1 range), kernel vs torch f32 {diff.max():.3e}, kernel vs torch f64 '
          f'{np.abs(got - t64).max():.3e}, bound {float(bnd.max()):.3e}')
    assert (diff <= bnd + dist).all()


def test_the_entry_point_through_its_wrapper():
    """ops.preprocess_images directly: its refusals, and an image its arguments do not cover is left unread (NaN), the rest untouched"""
    ims = [image((5, 9, 3)), image((4, 6, 1)), image((3, 3, 3))]
    data, offsets, shapes = pp.pack_images(ims, dev())
    a, b = pp.normalisation(MEAN, STD)
    ref = pp.preprocess_images_host(ims, (8, 8), MEAN, STD, True)
    out = torch.empty(3, 3, 8, 8, device=dev())
    ops.preprocess_images(data, offsets, shapes, out, a, b, 9, True)
    for i, im in enumerate(ims):
        check(f'ops.{i}', out[i].cpu().numpy(), ref[i], bound(im.shape, (8, 8), True))
    good = out.clone()
    bad = shapes.clone()
    bad[1, 2] = 2                                                           # a channel count the kernel has no path for
    ops.preprocess_images(data, offsets, bad, out, a, b, 9, True)
    assert bool(out[1].isnan().all()) and torch.equal(out[0], good[0]) and torch.equal(out[2], good[2])
    far = offsets.clone()
    far[2] = data.numel() - 20                                              # 27 bytes of image do not fit before the tail pad
    ops.preprocess_images(data, far, shapes, out, a, b, 9, True)
    assert bool(out[2].isnan().all()) and torch.equal(out[:2], good[:2])
    ops.preprocess_images(data, offsets, shapes, out, a, b, 8, True)        # max_side below image 0's width: that image is refused
    assert bool(out[0].isnan().all()) and torch.equal(out[1:], good[1:])
    for kw in (dict(max_side=pp.MAX_SIDE + 1), dict(max_side=0)):
        with pytest.raises(I2TError, match='max_side'):
            ops.preprocess_images(data, offsets, shapes, out, a, b, kw['max_side'], True)
    with pytest.raises(I2TError, match='aligned'):
        ops.preprocess_images(data[1:], offsets, shapes, out, a, b, 9, True)
    with pytest.raises(I2TError, match='torch.int32'):
        ops.preprocess_images(data, offsets, shapes.long(), out, a, b, 9, True)


def test_the_model_method_feeds_encode(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import tiny_config
    cfg = tiny_config()
    m = VisionEncoderDecoder(cfg)
    m.load_state_dict(tiny_weights)
    m = m.to(dev()).eval()
    spec = cfg.vision_encoder_config.input
    ims = [image(s, seed=9) for s in ((37, 53, 3), (64, 48, 3), (9, 13, 1), (spec.height, spec.width, 3))]
    x = m.preprocess_images(ims, mean=MEAN, std=STD)
    assert x.shape == (4, 3, spec.height, spec.width) and x.dtype == torch.float32 and x.device == dev()
    ref = pp.preprocess_images_host(ims, (spec.height, spec.width), MEAN, STD, True)
    got, want = m.encode(x), m.encode(torch.from_numpy(ref).float().to(dev()))
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert float((got - want).abs().max()) <= 2e-2                          # the encoder's parity tolerance (tests/test_model_gpu.py)
    assert m.preprocess_images(ims, size=(16, 24), antialias=False).shape == (4, 3, 16, 24)
