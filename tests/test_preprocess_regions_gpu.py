"""Boxes and flips of csrc/preprocess.hip (i2t_preprocess_regions) on the MI355X against the float64 replica
(image2text_amd/preprocess.py::preprocess_regions_host), on the smallest shapes at which the kernel can go wrong, with the bound of the
whole-image kernel taken over the BOX's tap counts, and bit-exact cases.

The bound.  u = 2^-24 (fp32 unit roundoff), values v <= 255, weights w >= 0 that sum to 1 per axis.
  * A weight is evaluated in fp64 and rounded once: w~ = w (1 + d), |d| <= u.
  * The horizontal sum of n_h taps is a chain of n_h fp32 fmas: every term meets at most n_h roundings besides its weight's, so
    |s~ - s| <= (n_h + 1) u 255, to first order.  The vertical sum adds w~ s~ for the n_v source rows of the output row's tap range
    (rows outside it add an exact 0): likewise (n_v + 1) u 255 on top.  Before the normalisation: (n_h + n_v + 2) u 255.
  * out = fl(acc~ a~ + b~), a~ = a (1 + d_a), b~ = b (1 + d_b): |a| times the above, + u 255 |a| (a's rounding) + u |b| (b's) +
    u (255 |a| + |b|) (the fma's rounding).  One more unit of u 255 |a| covers second-order terms and the replica's float64 error.
  bound_k = u ((n_h + n_v + 5) 255 |a_k| + 2 |b_k|)
n_h, n_v: the most taps any output sample has on that axis, ``tap_counts((bh, bw), size, antialias)`` -- the box only renames the
axis length n, and the flip permutes output columns: a flipped column is the mirrored column's sum, term for term, so neither enters
the derivation."""
import numpy as np
import pytest
import torch

from image2text_amd import ops
from image2text_amd import preprocess as pp
from image2text_amd.lib import I2TError

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
UNIT = dict(mean=(0.0, 0.0, 0.0), std=(1 / 255,) * 3)           # a = 1, b = 0: the raw resized values

# image (h, w, c), boxes (top, left, bh, bw), size (H, W), the flips the case is held to its bound under.  What each is there for:
CASES = {
    'corner_pixel': ((5, 9, 3), [(4, 8, 1, 1)], (4, 4), (0, 1)),               # a one-pixel box in the far corner: every tap clamps to it
    'upscale_inside': ((5, 9, 3), [(1, 2, 3, 5)], (8, 8), (0, 1)),             # upscale, edges strictly inside the image: clamps at the box
    'odd_37x53': ((37, 53, 3), [(3, 5, 20, 31)], (16, 16), (0, 1)),            # odd width and odd left: row starts at every byte residue
    'gray_9x13': ((9, 13, 1), [(2, 3, 6, 7)], (16, 16), (0, 1)),               # gray; the three planes are equal before the normalisation
    '7x300': ((7, 300, 3), [(1, 3, 5, 290)], (8, 8), (0, 1)),                  # 73 horizontal taps, past the LDS weight table, under a flip
    '300x7': ((300, 7, 3), [(4, 1, 290, 5)], (8, 8), (0,)),                    # many vertical taps from a row offset
    '12x300_wide_out': ((12, 300, 3), [(0, 10, 12, 280)], (9, 300), (0, 1)),   # two column tiles, the second partly empty, the span backwards
    '2x16384': ((2, 16384, 3), [(0, 0, 2, 16384), (1, 8000, 1, 8384)], (3, 40), (1,)),          # the side cap and its > 64 KB LDS request
    '375x500': ((375, 500, 3), [(40, 60, 224, 300)], (224, 224), (0, 1)),      # the real shape
}
# the ragged batch of tests/test_preprocess_gpu.py, restated: (h, w, c)
RAGGED = [(1, 1, 3), (2, 3, 3), (9, 13, 1), (5, 9, 3), (37, 53, 3), (7, 11, 1), (300, 7, 3), (33, 41, 3), (7, 300, 3), (375, 500, 3), (5, 9, 1)]


def dev():
    return torch.device('cuda:0')


def image(shape, seed=0):
    h, w, c = shape
    g = torch.Generator().manual_seed(seed * 7919 + h * 131 + w * 17 + c)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def bound(box_hw, size, antialias, mean=MEAN, std=STD):
    """[3, 1, 1] float64: the derived bound per channel (module docstring) for a box of (bh, bw) pixels"""
    n_h, n_v = pp.tap_counts(box_hw, size, antialias)
    a, b = (x.astype(np.float64) for x in pp.normalisation(mean, std))
    out = U * ((n_h + n_v + 5) * 255.0 * np.abs(a) + 2.0 * np.abs(b))
    assert (out <= (n_h + n_v + 8) * U * 255.0 * np.abs(a)).all()          # never looser than the figure the whole-image kernel was specified with
    return out[:, None, None]


@pytest.fixture(scope='module')
def refs():
    """name -> (image, {antialias: float64 replica [n_boxes, 3, H, W], unflipped}), computed once; a flipped reference is its mirror
    (the replica's definition, held to torch in tests/test_preprocess_regions_host_cpu.py)"""
    out = {}
    for name, (shape, boxes, size, _) in CASES.items():
        im = image(shape)
        out[name] = (im, {aa: pp.preprocess_regions_host([im], size, boxes, [0] * len(boxes), None, MEAN, STD, aa) for aa in (True, False)})
    return out


def check(name, got, ref, bnd):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bnd).max())
    print(f'{name}: max |err| {err.max():.3e}, {worst:.3f} of the bound ({float(bnd.max()):.3e})')
    assert np.isfinite(got).all(), f'{name}: non-finite output'
    assert worst <= 1.0, f'{name}: max |err| {err.max():.3e} is {worst:.2f} x the bound'


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
@pytest.mark.parametrize('name', list(CASES))
def test_boxes_against_the_float64_replica(refs, name, antialias):
    shape, boxes, size, flips = CASES[name]
    im, ref = refs[name]
    n = len(boxes)
    # every box unflipped, then every box flipped, in one launch
    got = pp.preprocess_images([im], size, MEAN, STD, antialias, device=dev(), boxes=boxes * 2, box_index=[0] * (2 * n),
                               flip=[False] * n + [True] * n)
    assert got.shape == (2 * n, 3) + size and got.dtype == torch.float32 and got.device == dev()
    tag = f'{name}.{"aa" if antialias else "plain"}'
    for i, box in enumerate(boxes):
        bnd = bound(box[2:], size, antialias)
        if 0 in flips:
            check(f'{tag}.box{i}', got[i].cpu().numpy(), ref[antialias][i], bnd)
        if 1 in flips:
            check(f'{tag}.box{i}.flipped', got[n + i].cpu().numpy(), ref[antialias][i][..., ::-1], bnd)
        # the flip is taken on the output: the same sums, column for column
        assert torch.equal(got[n + i], torch.flip(got[i], [-1])), f'{tag}.box{i}: flipped != mirrored'
    if shape[2] == 1:
        unit = pp.preprocess_images([im], size, antialias=antialias, device=dev(), boxes=boxes, flip=[True] * n, **UNIT)
        assert torch.equal(unit[0, 0], unit[0, 1]) and torch.equal(unit[0, 0], unit[0, 2])


def test_a_box_of_the_output_size_is_the_pixels():
    im = image((24, 40, 3), seed=5)
    top, left, H, W = 5, 7, 12, 20
    want = im[top:top + H, left:left + W].permute(2, 0, 1).float()
    for antialias in (True, False):
        got = pp.preprocess_images([im], (H, W), antialias=antialias, device=dev(), boxes=[(top, left, H, W)] * 2, box_index=[0, 0],
                                   flip=[False, True], **UNIT).cpu()
        assert torch.equal(got[0], want) and torch.equal(got[1], torch.flip(want, [-1])), antialias
    g = image((6, 10, 1), seed=5)
    got = pp.preprocess_images([g], (4, 5), device=dev(), boxes=[(2, 5, 4, 5)], flip=[True], **UNIT).cpu()
    assert torch.equal(got[0], torch.flip(g[2:6, 5:10].permute(2, 0, 1).float(), [-1]).expand(3, -1, -1))


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
def test_full_boxes_are_the_whole_image_entry_point_bit_for_bit(antialias):
    ims = [image(s, seed=3) for s in RAGGED]
    packed = pp.pack_images(ims, dev())
    size = (20, 24)
    want = pp.preprocess_images(packed, size, MEAN, STD, antialias)
    got = pp.preprocess_images(packed, size, MEAN, STD, antialias, boxes=pp.full_boxes(RAGGED))
    assert torch.equal(got, want)
    assert torch.equal(pp.preprocess_images(packed, size, MEAN, STD, antialias, boxes=pp.full_boxes(packed), flip=[False] * len(ims)), want)
    # flip alone mirrors whole images
    flips = [i % 2 == 1 for i in range(len(ims))]
    got = pp.preprocess_images(packed, size, MEAN, STD, antialias, flip=flips)
    for i, f in enumerate(flips):
        assert torch.equal(got[i], torch.flip(want[i], [-1]) if f else want[i]), i


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
def test_many_regions_of_one_upload(antialias):
    ims = [image((37, 53, 3), seed=1), image((64, 48, 3), seed=1), image((21, 30, 1), seed=1)]          # image 1 is named by no region
    boxes = [(3, 5, 20, 31), (0, 0, 21, 30), (10, 20, 27, 33), (4, 9, 12, 8), (3, 5, 20, 31), (20, 29, 1, 1), (0, 0, 37, 53), (1, 1, 19, 28),
             (4, 9, 12, 8)]
    index = [0, 2, 0, 2, 0, 2, 0, 2, 2]                                     # unsorted; image 0 four times, image 2 five times
    flip = [False, True, True, False, True, False, False, True, True]       # rows 0 / 4 and 3 / 8: the same box, once flipped and once not
    assert index.count(0) == 4 and 1 not in index and boxes[0] == boxes[4] and flip[0] != flip[4]
    size = (16, 24)
    got = pp.preprocess_images(ims, size, MEAN, STD, antialias, device=dev(), boxes=boxes, box_index=index, flip=flip)
    assert got.shape == (9, 3) + size
    ref = pp.preprocess_regions_host(ims, size, boxes, index, flip, MEAN, STD, antialias)
    for r, box in enumerate(boxes):
        check(f'regions.{r}', got[r].cpu().numpy(), ref[r], bound(box[2:], size, antialias))
    assert torch.equal(got[4], torch.flip(got[0], [-1])) and torch.equal(got[8], torch.flip(got[3], [-1]))
    # one at a time: the source image alone, another position in the buffer
    for r, (box, i, f) in enumerate(zip(boxes, index, flip)):
        alone = pp.preprocess_images([ims[i]], size, MEAN, STD, antialias, device=dev(), boxes=[box], flip=[f])
        assert torch.equal(alone[0], got[r]), r
    # the packed form, with tensors for the arguments, and an out buffer
    packed = pp.pack_images(ims, dev())
    out = torch.full((9, 3) + size, float('nan'), device=dev())
    res = pp.preprocess_images(packed, size, MEAN, STD, antialias, boxes=torch.tensor(boxes), box_index=torch.tensor(index, dtype=torch.int32),
                               flip=torch.tensor(flip), out=out)
    assert res is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        pp.preprocess_images(packed, size, boxes=boxes, box_index=index, out=torch.empty((3, 3) + size, device=dev()))


def test_the_entry_point_through_its_wrapper():
    """ops.preprocess_regions directly: a region its arguments do not cover is left unread (NaN), the others untouched; its refusals"""
    ims = [image((5, 9, 3)), image((4, 6, 1)), image((3, 3, 3))]
    data, offsets, shapes = pp.pack_images(ims, dev())
    a, b = pp.normalisation(MEAN, STD)
    rows = [[0, 1, 2, 3, 5, 0], [1, 0, 0, 4, 6, 1], [2, 1, 1, 2, 2, 0], [0, 0, 0, 5, 9, 1]]
    regions = torch.tensor(rows, dtype=torch.int32, device=dev())
    ref = pp.preprocess_regions_host(ims, (8, 8), [r[1:5] for r in rows], [r[0] for r in rows], [r[5] for r in rows], MEAN, STD, True)
    out = torch.empty(4, 3, 8, 8, device=dev())
    ops.preprocess_regions(data, offsets, shapes, regions, out, a, b, 9, True)
    for i, r in enumerate(rows):
        check(f'ops.{i}', out[i].cpu().numpy(), ref[i], bound(r[3:5], (8, 8), True))
    good = out.clone()
    bads = {'src = B': (1, 0, 3), 'src = -1': (2, 0, -1), 'one column past the image': (0, 2, 5), 'bh = 0': (3, 3, 0), 'flip = 2': (1, 5, 2),
            'a negative left': (2, 2, -1), 'one row past the image': (1, 1, 1), 'a width that wraps int32': (0, 4, 2 ** 31 - 1)}
    for what, (r, col, value) in bads.items():
        bad = regions.clone()
        bad[r, col] = value
        out.fill_(7.0)
        ops.preprocess_regions(data, offsets, shapes, bad, out, a, b, 9, True)
        assert bool(out[r].isnan().all()), what
        keep = [i for i in range(4) if i != r]
        assert torch.equal(out[keep], good[keep]), what
    odd = shapes.clone()
    odd[1, 2] = 2                                                           # an image the existing check refuses: its regions only
    ops.preprocess_regions(data, offsets, odd, regions, out, a, b, 9, True)
    assert bool(out[1].isnan().all()) and torch.equal(out[[0, 2, 3]], good[[0, 2, 3]])
    ops.preprocess_regions(data, offsets, shapes, regions, out, a, b, 8, True)        # max_side below image 0's width
    assert bool(out[[0, 3]].isnan().all()) and torch.equal(out[1:3], good[1:3])
    for max_side in (pp.MAX_SIDE + 1, 0):
        with pytest.raises(I2TError, match='max_side'):
            ops.preprocess_regions(data, offsets, shapes, regions, out, a, b, max_side, True)
    with pytest.raises(I2TError, match='aligned'):
        ops.preprocess_regions(data[1:], offsets, shapes, regions, out, a, b, 9, True)
    with pytest.raises(I2TError, match='torch.int32'):
        ops.preprocess_regions(data, offsets, shapes, regions.long(), out, a, b, 9, True)
    with pytest.raises(I2TError, match='torch.int32'):
        ops.preprocess_regions(data, offsets, shapes.long(), regions, out, a, b, 9, True)
    with pytest.raises(I2TError, match='no CPU path'):
        ops.preprocess_regions(data, offsets, shapes, regions.cpu(), out, a, b, 9, True)


def test_the_model_method_takes_boxes(tiny_weights):
    from image2text_amd.models.vision_encoder_decoder import VisionEncoderDecoder
    from image2text_amd.synth import fake_tokenizer, tiny_config
    cfg = tiny_config()
    m = VisionEncoderDecoder(cfg)
    m.load_state_dict(tiny_weights)
    m = m.to(dev()).eval()
    spec = cfg.vision_encoder_config.input
    size = (spec.height, spec.width)
    ims = [image(s, seed=9) for s in ((37, 53, 3), (64, 48, 3), (9, 13, 1))]
    boxes = pp.center_boxes([im.shape for im in ims], size, 0.875)
    x = m.preprocess_images(ims, mean=MEAN, std=STD, boxes=boxes)
    assert x.shape == (3, 3) + size and x.dtype == torch.float32 and x.device == dev()
    ref = pp.preprocess_regions_host(ims, size, boxes, mean=MEAN, std=STD)
    got, want = m.encode(x), m.encode(torch.from_numpy(ref).float().to(dev()))
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    assert float((got - want).abs().max()) <= 2e-2                          # the encoder's parity tolerance (tests/test_model_gpu.py)
    # R = 6 regions of 2 images -> six captions in one batch; rows 0 and 5 are the same region
    regions = [(0, 0, 37, 53), (5, 5, 30, 40), (0, 0, 64, 48), (10, 8, 40, 32), (32, 24, 32, 24), (0, 0, 37, 53)]
    x6 = m.preprocess_images(ims[:2], mean=MEAN, std=STD, boxes=regions, box_index=[0, 0, 1, 1, 1, 0], flip=[False, True, False, False, True, False])
    assert x6.shape == (6, 3) + size and torch.equal(x6[0], x6[5])
    tok = fake_tokenizer(cfg.decoder_config.vocab_size)
    prompt = torch.full((6, 1), tok.bos_token_id, dtype=torch.long, device=dev())
    caps = m.generate_captions(x6, prompt, max_new_tokens=4, top_k=1)
    assert caps.ids.shape[:2] == (6, 1) and caps.ids.shape[2] <= 5 and bool(torch.isfinite(caps.logprob).all())
    assert torch.equal(caps.ids[0], caps.ids[5])
