"""Host-only checks of tests/conv_ref.py: the bounds of the convolution tests bite.  A dropped (tap, channel) term, two swapped
8-channel chunks at the pixels the LDS swizzle keys on, and a halo shifted by one pixel on the last tile column all exceed the
per-element bound; the reference rounded as the kernel rounds stays inside it; and conditions (i) (finite, every element bounded)
and (ii) (median bound <= rms / (4 sqrt n)) hold for every case of the table on the reference alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

F64 = torch.float64
ALL_CASES = R.FWD_CASES + R.BWD_DATA_CASES + R.BWD_WEIGHT_CASES + R.DET_CASES


def _layer(cin, cout, H=24, W=40):
    c = R._case('fwd', src='img' if cin < 8 else 'nhwc', Cin=cin, Cout=cout, dst='nhwc', B=1, H=H, W=W)
    d = R.inputs(c)
    a, um = R.stage_image(d.x) if c.src == 'img' else R.stage_gelu(d.x)
    return c, d, a, um, R.with_bias(R.forward(a, um, d.w, None), d.bias)


@pytest.mark.parametrize('cin,cout', [(3, 8), (8, 16), (16, 32), (32, 16)])         # 108, 288, 576 and 1152 terms
def test_perturbations_exceed_the_bound(cin, cout):
    c, d, a, um, r = _layer(cin, cout)
    wb = R.bf16_round(d.w.double())
    H, W = c.H, c.W
    # (a) one (tap, channel) term dropped: at every output pixel in turn.  The term of median size must show, and so must most
    ap = torch.nn.functional.pad(a, (2, 3, 2, 3))
    for co, ci, ky, kx in ((0, 0, 0, 0), (cout - 1, cin - 1, 5, 5), (cout // 2, cin // 2, 2, 3)):
        term = (wb[co, ci, ky, kx] * ap[0, ci, ky:ky + H, kx:kx + W]).abs()[3:H - 3, 3:W - 3]      # where the tap reads the image
        over = term > r.bound[0, co, 3:H - 3, 3:W - 3]
        sel = term.flatten().argsort()[term.numel() // 2]
        assert bool(over.flatten()[sel]), f'a dropped median-size term hides inside the bound (n = {36 * cin})'
        # (a GELU output near zero times a small weight is smaller than the output's own rounding: no bound can show that one)
        assert float(over.double().mean()) >= 0.6, float(over.double().mean())
    # (b) CP = 32: chunks ch and ch ^ 2 exchanged at the patch pixels with (px >> 2) & 1 set (patch px = x - x0 + 2)
    if cin == 32:
        x = torch.arange(W)
        hit = ((((x % R.TS) + 2) >> 2) & 1).bool()
        a2 = a.clone()
        a2[:, :, :, hit] = a[:, :, :, hit].view(1, 2, 16, H, int(hit.sum())).flip(1).reshape(1, 32, H, int(hit.sum()))
        diff = (R.corr(a2, wb, 2) + d.bias.double().view(1, -1, 1, 1) - r.ref).abs()
        assert float((diff > r.bound).double().mean()) >= 0.95
    # (c) the halo of the last tile column read one pixel to the side
    x0 = ((W - 1) // R.TS) * R.TS
    diff = (R.corr(torch.roll(a, 1, 3), wb, 2) + d.bias.double().view(1, -1, 1, 1) - r.ref).abs()[..., x0:]
    assert float((diff > r.bound[..., x0:]).double().mean()) >= 0.95
    # the reference itself, rounded as the kernel rounds its output, is inside
    assert bool(((R.kernel_rounded(r) - r.ref).abs() <= r.bound).all())


def _results(c, mode='n01'):
    d = R.inputs(c, mode)
    r = R.case_reference(c, d)
    if c.op == 'fwd':
        return d, [('y', r, False), ('y+bias', R.with_bias(r, d.bias), False)]
    if c.op == 'bwd_data':
        return d, [('dx', r, False)]
    return d, [('dW', r[0], True)] + ([('db', r[1], True)] if r[1] is not None else [])


@pytest.mark.parametrize('c', ALL_CASES, ids=lambda c: c.id)
def test_conditions_on_the_reference_alone(c):
    _, res = _results(c)
    for name, r, f32_out in res:
        b = torch.as_tensor(r.bound, dtype=F64).expand_as(r.ref)
        assert bool(torch.isfinite(r.ref).all()) and bool(torch.isfinite(b).all()) and bool((b > 0).all()), name      # (i)
        assert bool(((R.kernel_rounded(r, f32_out) - r.ref).abs() <= b).all()), name
        assert R.condition_ii(r) <= R.II_MAX, (name, R.condition_ii(r))                                                 # (ii)


@pytest.mark.parametrize('c', ALL_CASES, ids=lambda c: c.id)
def test_lattice_cases_are_exact(c):
    for mode in ('lattice',) + (('lattice_sparse',) if c.op == 'bwd_data' else ()):
        d, res = _results(c, mode)
        if c.op != 'bwd_data':
            R.lattice_stage(d.x, c.src)
        for name, r, f32_out in res:
            R.assert_exact(r, dgelu=c.op == 'bwd_data')
            assert torch.equal(r.ref, r.ref.round() if c.op != 'bwd_data' else (2 * r.ref).round() / 2), name
            assert not bool((torch.as_tensor(r.extra) != 0).any()) or c.op == 'bwd_data', name       # no uncertain GELU roundings
    if c.op == 'bwd_data':
        assert bool((d.dy != 0).any())


def test_impulses_are_exact():
    for y, x in R.IMPULSE_AT(24, 40):
        pre, w = R.impulse_fwd(16, 24, 40, y, x)
        a = R.lattice_stage(pre, 'nhwc')
        r = R.forward(a, torch.zeros_like(a), w, None)
        assert float(r.S.max()) < 2.0 ** 24 and len(torch.unique(w)) == 7
        c = torch.arange(32)
        assert bool((pre[0, c, y, x] != pre[0, c ^ 16, y, x]).all())
        dy, w = R.impulse_bwd_data(16, 24, 40, y, x)
        r = R.backward_data(dy.double(), w, torch.zeros(1, 16, 24, 40))
        R.assert_exact(r, dgelu=True)
        assert int((r.ref != 0).sum()) > 0
    assert any((((x % 16) + 3) >> 2) & 1 for _, x in R.IMPULSE_AT(24, 40)[4:])


def test_route_table_is_complete():
    got = {R.route(c) for c in ALL_CASES} | {R.transpose_route(C, W, not mis) for C, W, mis in R.T_CASES}
    assert got == R.all_routes(), (sorted(R.all_routes() - got), sorted(got - R.all_routes()))
    assert R.route(R.BWD_DATA_CASES[0]) == 'conv_mfma_kernel<32, 1, SRC_NHWC_BF16, false, true, false>'
    assert R.route(R.BWD_WEIGHT_CASES[0]) == 'conv_mfma_bwd_weight_kernel<16, 32, SRC_NHWC_BF16, SRC_NHWC_BF16, true>'
    assert {(c.W + 15) // 16 for c in R.FWD_CASES if c.dst == 'nchw' and c.Cin >= 16} >= {1, 3, 4, 5, 8, 9}
    assert {c.W % 4 for c in ALL_CASES} == {0, 1, 2, 3}
