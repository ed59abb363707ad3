"""image2text_amd/preprocess.py without a GPU: the float64 replica against torch's float64 ``interpolate`` (the CPU oracle of the
semantics), gray replication, the packing, the coefficient pair of the normalisation and every refusal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from image2text_amd import preprocess as pp

# (h, w) -> (H, W): the nine pairs the semantics were stated on
PAIRS = [((1, 1), (4, 4)), ((2, 3), (8, 8)), ((16, 16), (16, 16)), ((37, 53), (16, 16)), ((300, 7), (8, 8)), ((5, 9), (16, 16)),
         ((375, 500), (224, 224)), ((33, 41), (12, 20)), ((224, 224), (128, 128))]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def image(h, w, c=3, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + h * 131 + w * 17 + c)
    return torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8)


def torch_chain(im, size, mean, std, antialias, dtype):
    """ToTensor -> Resize(size) -> Normalize(mean, std) as torch ops in ``dtype`` -> [3, H, W]"""
    x = im.permute(2, 0, 1).to(dtype) / 255.0
    if x.shape[0] == 1:
        x = x.expand(3, -1, -1)
    y = F.interpolate(x[None], size=size, mode='bilinear', align_corners=False, antialias=antialias)[0]
    return (y - torch.tensor(mean, dtype=dtype)[:, None, None]) / torch.tensor(std, dtype=dtype)[:, None, None]


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
@pytest.mark.parametrize('src,dst', PAIRS, ids=lambda p: f'{p[0]}x{p[1]}')
def test_the_replica_is_torch_float64_interpolate(src, dst, antialias):
    im = image(*src)
    got = pp.preprocess_images_host([im], dst, antialias=antialias)[0]
    ref = torch_chain(im, dst, (0, 0, 0), (1, 1, 1), antialias, torch.float64).numpy()
    assert got.shape == (3,) + dst and got.dtype == np.float64
    assert np.abs(got - ref).max() <= 1e-12
    got = pp.preprocess_images_host([im], dst, MEAN, STD, antialias)[0]
    ref = torch_chain(im, dst, MEAN, STD, antialias, torch.float64).numpy()
    assert np.abs(got - ref).max() <= 1e-12 / min(STD)


@pytest.mark.parametrize('antialias', [True, False], ids=['aa', 'plain'])
def test_weights_are_non_negative_and_sum_to_one(antialias):
    for (h, w), (H, W) in PAIRS:
        for n, m in ((h, H), (w, W)):
            span, mat = pp.resize_taps(n, m, antialias)
            assert (mat >= 0).all() and np.abs(mat.sum(1) - 1).max() <= 1e-14
            assert (span[:, 0] >= 0).all() and (span[:, 1] <= n).all() and (span[:, 1] > span[:, 0]).all()
            assert (np.diff(span[:, 0]) >= 0).all() and (np.diff(span[:, 1]) >= 0).all()          # the kernel's tile span relies on it
            for i in range(m):
                assert not mat[i, :span[i, 0]].any() and not mat[i, span[i, 1]:].any()
    assert pp.tap_counts((300, 7), (8, 8), True) == (2, 75)


def test_a_gray_image_is_replicated_to_three_channels():
    g = image(9, 13, 1)
    for antialias in (True, False):
        got = pp.preprocess_images_host([g], (6, 5), MEAN, STD, antialias)
        rgb = pp.preprocess_images_host([g.expand(-1, -1, 3)], (6, 5), MEAN, STD, antialias)
        assert np.array_equal(got, rgb)
        ref = torch_chain(g, (6, 5), MEAN, STD, antialias, torch.float64).numpy()
        assert np.abs(got[0] - ref).max() <= 1e-12 / min(STD)


def test_pack_images_offsets_and_shapes():
    ims = [image(2, 3), image(5, 9, 1), image(1, 1), image(37, 53), image(4, 4, 1)]
    packed = pp.pack_images(ims)
    data, offsets, shapes = packed                              # a 3-tuple, as documented
    assert data.dtype == torch.uint8 and offsets.dtype == torch.int64 and shapes.dtype == torch.int32
    assert shapes.tolist() == [[2, 3, 3], [5, 9, 1], [1, 1, 3], [37, 53, 3], [4, 4, 1]]
    assert offsets.tolist() == [0, 18, 63, 66, 66 + 37 * 53 * 3]
    assert data.numel() == 66 + 37 * 53 * 3 + 16 + pp.TAIL_PAD and packed.max_side == 53
    assert not data[-pp.TAIL_PAD:].any()
    for im, off in zip(ims, offsets.tolist()):
        assert torch.equal(data[off:off + im.numel()], im.reshape(-1))
    batch = torch.stack([image(4, 6, 3, seed=s) for s in range(3)])
    data, offsets, shapes = pp.pack_images(batch)               # a [B, h, w, c] tensor
    assert offsets.tolist() == [0, 72, 144] and shapes.tolist() == [[4, 6, 3]] * 3
    assert torch.equal(data[:216], batch.reshape(-1))
    sliced = image(8, 8)[::2, 1:6]                              # a non-contiguous view is packed by value
    assert torch.equal(pp.pack_images([sliced]).data[:sliced.numel()], sliced.reshape(-1))


def test_the_normalisation_pair_is_formed_in_fp64_and_rounded_once():
    a, b = pp.normalisation(MEAN, STD)
    assert a.dtype == np.float32 and b.dtype == np.float32
    for k in range(3):
        assert a[k] == np.float32(1.0 / (255.0 * STD[k])) and b[k] == np.float32(-MEAN[k] / STD[k])
        assert abs(float(a[k]) * 255.0 * STD[k] - 1.0) <= 2.0 ** -24 and abs(float(b[k]) * STD[k] + MEAN[k]) <= 2.0 ** -24 * MEAN[k]
    a, b = pp.normalisation((0, 0, 0), (1 / 255,) * 3)
    assert a.tolist() == [1.0, 1.0, 1.0] and b.tolist() == [0.0, 0.0, 0.0]
    a, b = pp.normalisation((0, 0, 0), (1, 1, 1))
    assert a.tolist() == [float(np.float32(1 / 255))] * 3 and not b.any()


GOOD = [image(4, 5)]
REFUSALS = {
    'dtype': dict(images=[image(4, 5).float()]),
    'dtype_in_batch_tensor': dict(images=torch.zeros(2, 4, 5, 3, dtype=torch.int16)),
    'two_channels': dict(images=[torch.zeros(4, 5, 2, dtype=torch.uint8)]),
    'four_channels': dict(images=[image(4, 5), torch.zeros(4, 5, 4, dtype=torch.uint8)]),
    'no_channel_axis': dict(images=[torch.zeros(4, 5, dtype=torch.uint8)]),
    'empty_image': dict(images=[torch.zeros(0, 5, 3, dtype=torch.uint8)]),
    'empty_width': dict(images=[torch.zeros(4, 0, 1, dtype=torch.uint8)]),
    'no_images': dict(images=[]),
    'side_above_the_cap': dict(images=[torch.zeros(1, pp.MAX_SIDE + 1, 1, dtype=torch.uint8)]),
    'std_zero': dict(std=(0.2, 0.0, 0.2)),
    'std_nan': dict(std=(0.2, float('nan'), 0.2)),
    'std_inf': dict(std=(float('inf'), 1, 1)),
    'mean_inf': dict(mean=(0.0, float('-inf'), 0.0)),
    'mean_nan': dict(mean=(float('nan'), 0, 0)),
    'mean_two_values': dict(mean=(0.5, 0.5)),
    'size_one_int': dict(size=16),
    'size_three': dict(size=(16, 16, 3)),
    'size_zero': dict(size=(16, 0)),
    'size_negative': dict(size=(-16, 16)),
    'size_float': dict(size=(16.0, 16)),
    'size_above_the_cap': dict(size=(8, pp.MAX_SIDE + 1)),
    'out_shape': dict(out=torch.empty(1, 3, 8, 9)),
    'out_batch': dict(out=torch.empty(2, 3, 8, 8)),
    'out_dtype': dict(out=torch.empty(1, 3, 8, 8, dtype=torch.float64)),
    'out_on_the_host': dict(out=torch.empty(1, 3, 8, 8)),
    'host_device': dict(device='cpu'),
}


@pytest.mark.parametrize('name', REFUSALS)
def test_refusals_are_value_errors_before_any_launch(name, monkeypatch):
    from image2text_amd import ops
    monkeypatch.setattr(ops, 'preprocess_images', lambda *a, **k: pytest.fail('launched'))
    kw = dict(images=GOOD, size=(8, 8))
    kw.update(REFUSALS[name])
    with pytest.raises(ValueError):
        pp.preprocess_images(**kw)
    if not any(k in REFUSALS[name] for k in ('out', 'device')):          # the replica shares the refusals it can meet
        with pytest.raises(ValueError):
            pp.preprocess_images_host(**kw)


def test_pack_images_makes_the_image_refusals_itself():
    for name in ('dtype', 'two_channels', 'no_channel_axis', 'empty_image', 'no_images', 'side_above_the_cap'):
        with pytest.raises(ValueError):
            pp.pack_images(REFUSALS[name]['images'])
