"""Boxes and flips of image2text_amd/preprocess.py without a GPU: the float64 replica ``preprocess_regions_host`` against torch's float64
``interpolate`` on the slice, the clamp at the box's (not the image's) edge, every refusal of the public call before a launch, and the
host helpers that make boxes and flips (``full_boxes``, ``center_boxes``, ``random_resized_crop_boxes``, ``random_flips``)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image2text_amd import preprocess as pp

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# (h, w, c), (top, left, bh, bw), (H, W)
CASES = [((5, 9, 3), (4, 8, 1, 1), (4, 4)), ((5, 9, 3), (1, 2, 3, 5), (8, 8)), ((37, 53, 3), (3, 5, 20, 31), (16, 16)),
         ((9, 13, 1), (2, 3, 6, 7), (16, 16)), ((7, 300, 3), (1, 3, 5, 290), (8, 8)), ((300, 7, 3), (4, 1, 290, 5), (8, 8)),
         ((33, 41, 3), (0, 0, 33, 41), (12, 20)), ((375, 500, 3), (40, 60, 224, 300), (224, 224))]


def image(shape, seed=0):
    h, w, c = shape
    g = torch.Generator().manual_seed(seed * 7919 + h * 131 + w * 17 + c)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def torch_chain(im, box, size, mean, std, antialias, flip):
    """resized_crop -> hflip -> Normalize as torch ops in float64 -> [3, H, W]"""
    top, left, bh, bw = box
    x = im.permute(2, 0, 1).to(torch.float64) / 255.0
    if x.shape[0] == 1:
        x = x.expand(3, -1, -1)
    y = F.interpolate(x[None, :, top:top + bh, left:left + bw], size=size, mode='bilinear', align_corners=False, antialias=antialias)[0]
    y = (y - torch.tensor(mean, dtype=torch.float64)[:, None, None]) / torch.tensor(std, dtype=torch.float64)[:, None, None]
    return (torch.flip(y, [-1]) if flip else y).numpy()


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
@pytest.mark.parametrize('shape,box,size', CASES, ids=lambda p: 'x'.join(map(str, p)))
def test_the_replica_is_torch_float64_interpolate_on_the_slice(shape, box, size, antialias):
    im = image(shape)
    for flip in (False, True):
        got = pp.preprocess_regions_host([im], size, [box], flip=[flip], antialias=antialias)
        assert got.shape == (1, 3) + size and got.dtype == np.float64
        assert np.abs(got[0] - torch_chain(im, box, size, (0, 0, 0), (1, 1, 1), antialias, flip)).max() <= 1e-12
        got = pp.preprocess_regions_host([im], size, [box], None, [flip], MEAN, STD, antialias)
        assert np.abs(got[0] - torch_chain(im, box, size, MEAN, STD, antialias, flip)).max() <= 1e-12 / min(STD)


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
def test_taps_clamp_at_the_box_not_at_the_image(antialias):
    """A box whose right and bottom edges lie strictly inside the image.  A replica that clamped at the IMAGE's edge would let the taps
    of the last output column and row run on past the box: it would compute the resize, at the same scale, of the box grown to the
    image's edges (the wrong slice), cut to the box's outputs.  The two agree in the interior and differ on the last row and column."""
    im = image((13, 16, 3), seed=2)
    top, left, bh, bw = box = (1, 2, 6, 8)
    assert top + bh < 13 and left + bw < 16
    grown = (top, left, 13 - top, 16 - left)                                # 12 x 14
    unit = ((0, 0, 0), (1, 1, 1))
    # an upscale by 2: the last output's second tap is the sample past the box, clamped away (both modes).  A downscale by 1.5 x 2:
    # the antialiased taps of the last output reach one sample past the box (the plain ones, two per axis, do not).
    for size, grown_size in [((12, 16), (24, 28))] + ([((4, 4), (8, 7))] if antialias else []):
        H, W = size
        got = pp.preprocess_regions_host([im], size, [box], antialias=antialias)[0]
        assert np.abs(got - torch_chain(im, box, size, *unit, antialias, False)).max() <= 1e-12
        wrong = torch_chain(im, grown, grown_size, *unit, antialias, False)[:, :H, :W]
        assert np.abs(got[:, :H - 1, :W - 1] - wrong[:, :H - 1, :W - 1]).max() <= 1e-12          # the same taps in the interior
        assert np.abs(got[:, :, W - 1] - wrong[:, :, W - 1]).max() > 1e-3 and np.abs(got[:, H - 1] - wrong[:, H - 1]).max() > 1e-3
        # the same box of an image that differs only OUTSIDE the box: the same result, bit for bit
        other = image((13, 16, 3), seed=3)
        other[top:top + bh, left:left + bw] = im[top:top + bh, left:left + bw]
        assert not torch.equal(other, im)
        assert np.array_equal(pp.preprocess_regions_host([other], size, [box], antialias=antialias)[0], got)


def test_the_replica_is_the_whole_image_replica_on_the_slices():
    ims = [image((9, 13, 3)), image((6, 5, 1)), image((4, 4, 3))]
    boxes, index, flip = [(2, 3, 6, 7), (0, 0, 6, 5), (1, 1, 3, 4), (2, 3, 6, 7)], [0, 1, 0, 0], [False, True, False, True]
    got = pp.preprocess_regions_host(ims, (5, 6), boxes, index, flip, MEAN, STD)
    assert got.shape == (4, 3, 5, 6)
    for r, ((t, l, bh, bw), i, f) in enumerate(zip(boxes, index, flip)):
        want = pp.preprocess_images_host([ims[i][t:t + bh, l:l + bw]], (5, 6), MEAN, STD)[0]
        assert np.array_equal(got[r], want[..., ::-1] if f else want)
    assert np.array_equal(got[3], got[0][..., ::-1])
    whole = pp.preprocess_regions_host(ims, (5, 6), pp.full_boxes([im.shape for im in ims]), mean=MEAN, std=STD)
    assert np.array_equal(whole, pp.preprocess_images_host(ims, (5, 6), MEAN, STD))
    assert np.array_equal(pp.preprocess_regions_host(ims, (5, 6), None, flip=[True] * 3, mean=MEAN, std=STD), whole[..., ::-1])
    # tensors are taken as well as sequences
    t = pp.preprocess_regions_host(ims, (5, 6), torch.tensor(boxes), torch.tensor(index, dtype=torch.int32), torch.tensor(flip), MEAN, STD)
    assert np.array_equal(t, got)


GOOD = [image((4, 5, 3)), image((6, 7, 1))]
REFUSALS = {
    'boxes_rank_1': dict(boxes=[0, 0, 4, 5]),
    'boxes_rank_3': dict(boxes=[[[0, 0, 4, 5]], [[0, 0, 6, 7]]]),
    'boxes_five_columns': dict(boxes=[[0, 0, 4, 5, 0], [0, 0, 6, 7, 0]]),
    'boxes_float_tensor': dict(boxes=torch.tensor([[0., 0., 4., 5.], [0., 0., 6., 7.]])),
    'boxes_non_integral': dict(boxes=[[0, 0, 3.5, 5], [0, 0, 6, 7]]),
    'boxes_bool': dict(boxes=torch.ones(2, 4, dtype=torch.bool)),
    'boxes_not_numbers': dict(boxes=[['a', 0, 4, 5], [0, 0, 6, 7]]),
    'no_boxes': dict(boxes=torch.zeros(0, 4, dtype=torch.int64), box_index=[]),
    'more_boxes_than_images_without_an_index': dict(boxes=[[0, 0, 4, 5], [0, 0, 6, 7], [0, 0, 1, 1]]),
    'fewer_boxes_than_images_without_an_index': dict(boxes=[[0, 0, 4, 5]]),
    'index_at_B': dict(boxes=[[0, 0, 4, 5], [0, 0, 1, 1]], box_index=[0, 2]),
    'index_negative': dict(boxes=[[0, 0, 4, 5], [0, 0, 1, 1]], box_index=[0, -1]),
    'index_float': dict(boxes=[[0, 0, 4, 5], [0, 0, 1, 1]], box_index=[0.0, 1.0]),
    'index_rank_2': dict(boxes=[[0, 0, 4, 5], [0, 0, 1, 1]], box_index=[[0], [1]]),
    'index_length': dict(boxes=[[0, 0, 4, 5], [0, 0, 1, 1]], box_index=[0, 1, 1]),
    'index_without_boxes': dict(box_index=[0, 1]),
    'index_without_boxes_with_a_flip': dict(box_index=[0, 1], flip=[True, False]),
    'box_past_the_right_edge': dict(boxes=[[0, 1, 4, 5], [0, 0, 6, 7]]),
    'box_past_the_bottom_edge': dict(boxes=[[0, 0, 4, 5], [1, 0, 6, 7]]),
    'box_of_the_other_image': dict(boxes=[[0, 0, 6, 7], [0, 0, 6, 7]]),                  # inside image 1, not inside image 0
    'box_negative_top': dict(boxes=[[-1, 0, 4, 5], [0, 0, 6, 7]]),
    'box_negative_left': dict(boxes=[[0, -1, 4, 5], [0, 0, 6, 7]]),
    'box_zero_height': dict(boxes=[[0, 0, 0, 5], [0, 0, 6, 7]]),
    'box_zero_width': dict(boxes=[[0, 0, 4, 0], [0, 0, 6, 7]]),
    'box_beyond_int32': dict(boxes=[[0, 0, 2 ** 32 + 4, 5], [0, 0, 6, 7]]),
    'flip_length': dict(flip=[True]),
    'flip_length_with_boxes': dict(boxes=[[0, 0, 1, 1]] * 3, box_index=[0, 1, 1], flip=[True, False]),
    'flip_float': dict(flip=[0.0, 1.0]),
    'flip_two': dict(flip=[0, 2]),
    'flip_rank_2': dict(flip=[[True], [False]]),
    'flip_scalar': dict(flip=True),
    'out_has_B_rows_not_R': dict(boxes=[[0, 0, 1, 1]] * 3, box_index=[0, 1, 1], out=torch.empty(2, 3, 8, 8)),
}


@pytest.mark.parametrize('packed', [False, True], ids=['list', 'packed'])
@pytest.mark.parametrize('name', REFUSALS)
def test_refusals_are_value_errors_before_any_launch(name, packed, monkeypatch):
    from image2text_amd import ops
    monkeypatch.setattr(ops, 'preprocess_regions', lambda *a, **k: pytest.fail('launched'))
    monkeypatch.setattr(ops, 'preprocess_images', lambda *a, **k: pytest.fail('launched'))
    kw = dict(images=pp.pack_images(GOOD) if packed else GOOD, size=(8, 8))
    kw.update(REFUSALS[name])
    with pytest.raises(ValueError):
        pp.preprocess_images(**kw)
    if not packed and 'out' not in REFUSALS[name]:                          # the replica shares the refusals
        kw.setdefault('boxes', None)
        with pytest.raises(ValueError):
            pp.preprocess_regions_host(**kw)


def test_packed_images_carry_their_shapes_on_the_host():
    packed = pp.pack_images(GOOD)
    data, offsets, shapes = packed                                          # still the documented 3-tuple
    assert packed.host_shapes == ((4, 5, 3), (6, 7, 1)) and shapes.tolist() == [[4, 5, 3], [6, 7, 1]]
    assert packed.to(torch.device('cpu')) is packed
    by_hand = pp.PackedImages(data, offsets, shapes, 7)                     # built without them: read from the tensor, once
    assert by_hand.host_shapes == packed.host_shapes and by_hand.host_shapes is by_hand.host_shapes
    assert pp.full_boxes(packed).tolist() == [[0, 0, 4, 5], [0, 0, 6, 7]]


def test_full_and_center_boxes():
    assert pp.full_boxes([(375, 500, 3), (7, 9, 1)]).tolist() == [[0, 0, 375, 500], [0, 0, 7, 9]]
    assert pp.full_boxes(torch.tensor([[375, 500]])).dtype == torch.int64
    # (375, 500) -> (224, 224): the image is wider than the target, so the box is h x h = 375 x 375, left = (500 - 375) // 2 = 62
    assert pp.center_boxes([(375, 500)], (224, 224)).tolist() == [[0, 62, 375, 375]]
    # at 0.875: round(328.125) = 328 per side, top = (375 - 328) // 2 = 23, left = (500 - 328) // 2 = 86
    assert pp.center_boxes([(375, 500)], (224, 224), 0.875).tolist() == [[23, 86, 328, 328]]
    # a portrait image: w x w, top = 62
    assert pp.center_boxes([(500, 375, 3)], (224, 224)).tolist() == [[62, 0, 375, 375]]
    assert pp.center_boxes([(500, 375, 3)], (224, 224), 0.875).tolist() == [[86, 23, 328, 328]]
    # a 1 x 1 image: max(1, round(0.875)) = 1
    assert pp.center_boxes([(1, 1)], (224, 224)).tolist() == [[0, 0, 1, 1]]
    assert pp.center_boxes([(1, 1)], (224, 224), 0.875).tolist() == [[0, 0, 1, 1]]
    assert pp.center_boxes([(1, 1)], (224, 224), 0.1).tolist() == [[0, 0, 1, 1]]
    # a non-square target (H, W) = (100, 200) on 375 x 500: taller than the target, so bw = 500, bh = 500 * 100 / 200 = 250, top = 62
    assert pp.center_boxes([(375, 500)], (100, 200)).tolist() == [[62, 0, 250, 500]]
    # ... and on 100 x 500: wider, bh = 100, bw = 200, left = 150; a fraction above 1 is clipped to the image
    assert pp.center_boxes([(100, 500)], (100, 200)).tolist() == [[0, 150, 100, 200]]
    assert pp.center_boxes([(100, 500)], (100, 200), 4.0).tolist() == [[0, 0, 100, 500]]
    got = pp.center_boxes([(375, 500), (500, 375), (1, 1)], (224, 224), 0.875)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 4)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            pp.center_boxes([(375, 500)], (224, 224), bad)
    for bad in ([], [(0, 5)], [(4.5, 5.0)], [(4, 5, 3, 1)], [4, 5]):
        with pytest.raises(ValueError):
            pp.full_boxes(bad)


SHAPES = [(375, 500), (7, 300), (1, 1)]
DRAWS = 2000


def draw(seed, **kw):
    shapes = [s for s in SHAPES for _ in range(DRAWS)]
    return shapes, pp.random_resized_crop_boxes(shapes, generator=torch.Generator().manual_seed(seed), **kw)


def test_random_resized_crop_boxes():
    scale, ratio = (0.08, 1.0), (3 / 4, 4 / 3)
    shapes, boxes = draw(0)
    assert boxes.dtype == torch.int64 and tuple(boxes.shape) == (3 * DRAWS, 4)
    top, left, bh, bw = boxes.T
    h, w = torch.tensor(shapes).T
    assert bool(((top >= 0) & (left >= 0) & (bh >= 1) & (bw >= 1) & (top + bh <= h) & (left + bw <= w)).all())
    assert torch.equal(draw(0)[1], boxes) and not torch.equal(draw(1)[1], boxes)
    accepted = 0
    for (hh, ww), box in zip(shapes, boxes.tolist()):
        if tuple(box) == pp.rrc_fallback_box(hh, ww, ratio):
            continue
        accepted += 1
        t, l, y, x = box
        # the sides are real numbers with area / (h w) in scale and x / y in ratio, each rounded: off by at most half a pixel
        assert (x - 0.5) * (y - 0.5) <= scale[1] * hh * ww and (x + 0.5) * (y + 0.5) >= scale[0] * hh * ww, box
        assert (x - 0.5) / (y + 0.5) <= ratio[1] and (x + 0.5) / (y - 0.5) >= ratio[0], box
    # 375 x 500 accepts nearly always; on 7 x 300 the smallest height an attempt asks for, sqrt(0.08 * 2100 / (4 / 3)) = 11.2, never
    # fits, and the fallback is 7 rows by round(7 * 4 / 3) = 9 columns in the centre; 1 x 1 has one box
    assert accepted >= 0.95 * DRAWS
    assert boxes[DRAWS:2 * DRAWS].unique(dim=0).tolist() == [[0, 145, 7, 9]] == [list(pp.rrc_fallback_box(7, 300))]
    assert boxes[2 * DRAWS:].unique(dim=0).tolist() == [[0, 0, 1, 1]]
    first = boxes[:DRAWS]
    assert len(first.unique(dim=0)) > 0.9 * DRAWS                       # the boxes do vary, and so do the positions
    assert int(first[:, 0].min()) == 0 and int((first[:, 0] + first[:, 2]).max()) == 375 and int((first[:, 1] + first[:, 3]).max()) == 500
    # the area fraction is uniform over (0.08, 1) before the misfits are redrawn: its mean over accepted boxes lies well inside
    frac = (first[:, 2] * first[:, 3]).double() / (375 * 500)
    assert 0.3 < float(frac.mean()) < 0.6


def test_random_resized_crop_falls_back_when_nothing_fits():
    # area = h w with aspect 1 asks for a square of side sqrt(375 * 500) = 433 > 375: ten misses, then the centre clipped to ratio 1
    boxes = pp.random_resized_crop_boxes([(375, 500)] * DRAWS, scale=(1, 1), ratio=(1, 1), generator=torch.Generator().manual_seed(4))
    assert boxes.unique(dim=0).tolist() == [[0, 62, 375, 375]]
    boxes = pp.random_resized_crop_boxes([(500, 375)] * 50, scale=(1, 1), ratio=(1, 1))           # the global generator
    assert boxes.unique(dim=0).tolist() == [[62, 0, 375, 375]]
    assert pp.rrc_fallback_box(300, 400) == (0, 0, 300, 400)           # a ratio inside the range: the whole image
    assert pp.rrc_fallback_box(300, 7) == (145, 0, 9, 7)               # narrower than 3 / 4: bh = round(7 / (3 / 4)) = 9
    for kw in (dict(scale=(0.5, 0.2)), dict(scale=(0.0, 1.0)), dict(ratio=(2.0, 1.0)), dict(ratio=(1.0,)), dict(scale='ab')):
        with pytest.raises(ValueError):
            pp.random_resized_crop_boxes([(375, 500)], **kw)


def test_random_flips():
    g = torch.Generator().manual_seed(7)
    f = pp.random_flips(4000, generator=g)
    assert f.dtype == torch.bool and tuple(f.shape) == (4000,)
    assert abs(float(f.double().mean()) - 0.5) < 4 * math.sqrt(0.25 / 4000)                       # four standard deviations
    assert torch.equal(pp.random_flips(4000, generator=torch.Generator().manual_seed(7)), f)
    assert not torch.equal(pp.random_flips(4000, generator=torch.Generator().manual_seed(8)), f)
    assert not pp.random_flips(100, p=0.0).any() and pp.random_flips(100, p=1.0).all()
    for bad in (dict(n=0), dict(n=2.0), dict(n=4, p=1.5), dict(n=4, p=-0.1)):
        with pytest.raises(ValueError):
            pp.random_flips(**bad)


def test_the_names_are_exported():
    for name in ('preprocess_regions_host', 'full_boxes', 'center_boxes', 'random_resized_crop_boxes', 'random_flips'):
        assert name in pp.__all__ and callable(getattr(pp, name))
