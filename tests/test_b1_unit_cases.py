"""The helper of the block-1 unit kernel's tests (tests/b1_unit_cases.py) on the host: what tests/test_gpu_b1_unit_kernel.py relies on without
saying so.  (a) the float32 emulation of the chain stays inside the device bound on every grid, so a device result outside it is a
kernel finding; (b) no grid's outputs are so small that an all-zero result would pass; (c) the saturation inputs saturate what they are
named after, in some elements and in fewer than half; (d) the known-answer inputs and answers are exactly representable; (e) the NaN
cases poison exactly the neighbourhoods the device test exempts.  No GPU."""
import numpy as np
import pytest

import b1_unit_cases as B
from test_gpu_f16x3 import _split_round


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.GRIDS, ids=B.grid_id)
def test_float32_emulation_stays_inside_the_device_bound(grid, form):
    """(a), (b).  Measured (profiles/b1_unit_sweep.log): trunk max |err| <= 4.3e-6 with max |ref| 4-11, h1' <= 4.2e-6 with max |ref| 2-9; the
    bound is 2e-5 max(1, max |ref|) = 0.8-2.3e-4."""
    f, d = B.filters(form), B.operands(grid, form)
    trunk, h1 = B.emulate(f, d)
    et, eh = B.errors(trunk, h1, f, d)
    print("emulation %-9s %-8s trunk max |err| %.3e (max |ref| %.3e)   h1' max |err| %.3e (max |ref| %.3e)" % ((B.grid_id(grid), form) + et + eh))
    assert trunk.shape == (grid[0] * grid[1] * grid[2], 256) and h1.shape == (trunk.shape[0], 64)
    assert B.inside(et) and B.inside(eh), (et, eh)
    assert et[0] > 0 and eh[0] > 0                                         # float32 noise, not the reference compared with itself
    assert et[1] > 1.0 and eh[1] > 0.1
    assert np.abs(trunk).max() > 1.0 and np.abs(h1).max() > 0.1


@pytest.mark.parametrize("form", B.FORMS)
def test_emulation_of_the_descriptor_options(form):
    """relu1 = 0 leaves negative h1' values, shift3 = NULL moves the trunk by the bias: both inside the bound in float32"""
    f, d = B.filters(form), B.operands(B.FLAG_GRID, form)
    t0, h0 = B.emulate(f, d)
    t, h = B.emulate(f, d, relu1=False)
    assert np.array_equal(t, t0) and h.min() < -0.1 and np.array_equal(np.maximum(h, 0), h0)
    assert all(B.inside(e) for e in B.errors(t, h, f, d, relu1=False))
    t, h = B.emulate(f, d, bias=False)
    assert np.abs(t - t0).max() > 0.1
    assert all(B.inside(e) for e in B.errors(t, h, f, d, bias=False))
    assert not B.inside(B.errors(t, h, f, d)[0])                           # ... and the bound notices a missing bias


@pytest.mark.parametrize("form", B.FORMS)
def test_saturation_inputs_saturate_what_they_are_named_after(form):
    """(c): at least one element beyond 65504 and fewer than half, in float64"""
    some = lambda x: 0 < B.beyond_range(x)[0] < B.beyond_range(x)[1] / 2
    f, d = B.saturating_trunk(form)
    h2, trunk = B.reference(f, d)
    print("saturating trunk %-8s: %d of %d beyond the range, max h2 %.0f" % ((form,) + B.beyond_range(trunk) + (h2.max(),)))
    assert some(trunk) and B.beyond_range(h2)[0] == 0 and all(np.abs(v).max() <= 6e4 for v in d.values())
    for lower in (False, True):
        f, d, relu1 = B.saturating_h1(form, lower)
        h2, trunk = B.reference(f, d)
        h = B.reference_h1(f, B.emulate(f, d, relu1)[0], relu1)
        print("saturating h1' %-8s lower %d: %d of %d beyond the range" % ((form, lower) + B.beyond_range(h)))
        assert some(h) and B.beyond_range(trunk)[0] == 0 and B.beyond_range(h2)[0] == 0
        assert (h.min() < -B.SPLIT_MAX and h.max() < B.SPLIT_MAX and not relu1) if lower else (h.max() > B.SPLIT_MAX and relu1)
    f, d = B.saturating_h2(form)
    h2 = B.reference(f, d)[0]
    print("saturating h2 %-8s: %d of %d beyond the range" % ((form,) + B.beyond_range(h2)))
    assert some(h2)
    clean = B.reference(B.filters(form), B.operands(B.FLAG_GRID, form))
    assert B.beyond_range(clean[0])[0] == 0 and B.beyond_range(clean[1])[0] == 0


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.KNOWN_GRIDS, ids=B.grid_id)
def test_known_answers_are_exactly_representable(grid, form):
    """(d): operands and expected values survive the split unchanged (22 bits, inside the fp16 range), the filters are powers of two, and
    the float64 reference of these inputs IS the indexed answer -- for every tap"""
    d = B.known_operands(grid, form)
    for v in d.values():
        assert np.array_equal(_split_round(v), v.astype(np.float64))
    assert grid[1] != grid[2] or grid == (1, 56, 56)
    assert len(np.unique(d["h1"].reshape(-1, 64)[:, 0])) == grid[0] * grid[1] * grid[2]      # distinct per pixel ...
    assert all(len(np.unique(row)) == 64 for row in d["h1"].reshape(-1, 64)[:: 97])          # ... and per channel
    for ky in range(3):
        for kx in range(3):
            f = B.known_filters(ky, kx, form)
            for k in ("w2", "w3", "w1", "wsc"):
                if k in f:
                    nz = f[k][f[k] != 0]
                    assert np.array_equal(np.exp2(np.round(np.log2(nz))), nz)
            trunk, h1 = B.known_expected(grid, form, ky, kx)
            assert np.abs(trunk).max() < B.SPLIT_MAX and np.array_equal(_split_round(trunk), trunk) and np.array_equal(_split_round(h1), h1)
            if grid[1] * grid[2] <= 64 or (ky, kx) in ((0, 0), (1, 2)):                     # (the large grid: two taps are enough here)
                _, ref = B.reference(f, d)
                assert np.array_equal(ref, trunk.reshape(-1, 256))
                assert np.array_equal(B.reference_h1(f, ref), h1.reshape(-1, 64))
    # the taps differ from one another, and the border is where the zeros are
    t00, t22 = B.known_expected(grid, form, 0, 0)[0], B.known_expected(grid, form, 2, 2)[0]
    assert not np.array_equal(t00, t22)
    if form == "folded":
        xp4 = np.tile(d["xp"].astype(np.float64), 4)
        assert not (t00 - xp4)[:, 0].any() and not (t00 - xp4)[:, :, 0].any() and (t00 - xp4)[:, 1:, 1:].all()
        assert not (t22 - xp4)[:, -1].any() and not (t22 - xp4)[:, :, -1].any() and (t22 - xp4)[:, :-1, :-1].all()


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.NAN_GRIDS, ids=B.grid_id)
def test_nan_cases_poison_exactly_their_neighbourhoods(grid, form):
    """(e): in float64 the rows of the trunk that are not finite are the in-image 3 x 3 neighbourhoods of the three poisoned pixels, clipped
    by the image borders (each of the three sits in a corner: 4 pixels, 2 where the image is one pixel wide)"""
    n, h, w = grid
    pix = B.poisoned_pixels(grid)
    assert pix[0] == 0 and pix[1] == n * h * w - 1 and 0 < pix[2] < n * h * w - 1 and pix[2] % (h * w) == w - 1
    mask = B.poisoned_neighbourhood(grid)
    assert mask.sum() == 12 and mask[list(pix)].all()
    assert not mask[h * w: (n // 2) * h * w].any() and not mask[2 * w: h * w - 2 * w].any()      # nothing crosses into another image
    d = B.poisoned(grid, form)
    assert np.isnan(d["h1"]).sum() == 3 and not np.isnan(B.operands(grid, form)["h1"]).any()
    _, trunk = B.reference(B.filters(form), d)
    assert np.array_equal(~np.isfinite(trunk).all(axis=1), mask)
    clean = B.reference(B.filters(form), B.operands(grid, form))[1]
    assert np.array_equal(trunk[~mask], clean[~mask])
