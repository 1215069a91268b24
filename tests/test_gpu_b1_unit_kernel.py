"""csrc/b1_unit.hip ALONE (engine.B1UnitCall -> hmmr_bottleneck_tail with a unit_stream), both forms -- identity shortcut (RES) and folded
shortcut (KC3B = 4) -- against (1) the three hmmr_conv_gemm launches it replaces on the same device operands (conv2 with k_order = 2,
conv3 with the shortcut, the fused-preact conv1), bit for bit, and (2) the float64 reference of tests/b1_unit_cases.py on the operands as
stored.  h1, xp and res carry trailing rows of NaN halves; trunk and h1' start as a sentinel word everywhere and carry trailing guard
rows: a read or a store past row M shows (hmmr_run_flags / the sentinel).  The library's b1_unit launch counter proves which kernel ran.

    a  grid shapes: M = 1, one-pixel images, one-row and one-column images, H != W, odd widths, ragged and whole tiles
    b  tile counts around the XCD remap, more tiles than two workgroups per CU hold at once
    c  exact known answers: one-hot conv2 taps, every tap, the pixel and the tap named on failure
    d  descriptor values the ResNet never passes: a shortcut row stride > 256, relu1 = 0, shift3 = NULL
    e  run flags (saturation of h2, of the trunk, of h1' at either clamp; NaN operands) and the independence of images
    f  what the entry refuses queues nothing (the messages alone: tests/test_abi.py)

What the host half of this relies on (the float32 emulation inside the bound, the saturation and NaN inputs, the known answers'
exactness) is asserted in tests/test_b1_unit_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import b1_unit_cases as B
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 3
# grids the reference's conv2 launch (hmmr_conv_gemm with k_order = 2) refuses: those keep float64 and the sentinels only.  None today --
# its limits (an image at most 56 pixels wide, whole images) are the unit kernel's own
REFERENCE_REFUSES = ()
_streams, _cases = {}, {}


def _grid_id(g):
    return B.grid_id(g) + ("-float64_only" if g in REFERENCE_REFUSES else "")


def _flags():
    """read and clear hmmr_run_flags"""
    fl = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(fl), 1), "hmmr_run_flags")
    return fl.value


def _upload(d, dev):
    from human_dynamics_amd import packing
    return {k: packing.to_split(torch.from_numpy(v).to(dev)) for k, v in d.items()}


def _call(f, ops, dev, three=False, skey="", relu1=True, bias=True, res_ld=0):
    """the B1UnitCall of filter set f on the (uploaded) operands; the filter stream is packed once per (form, skey) -- host work"""
    from human_dynamics_amd import engine as E
    folded = "xp" in ops
    shortcut = (ops["xp"], f["wsc"], f["bsc"] if bias else None) if folded else None
    stream = None
    if not three:
        key = ("folded" if folded else "identity", skey)
        if key not in _streams:
            _streams[key] = E.pack_b1_unit((f["w2"],), f["w3"], f["w1"], shortcut).to(dev)
        stream = _streams[key]
    return E.B1UnitCall(ops["h1"], (f["w2"],) + tuple(f["bn2"]), f["w3"], f["b3"] if bias else None, f["pre"], f["w1"], f["bn1"], res=ops.get("res"),
                        shortcut=shortcut, relu1=relu1, res_ld=res_ld, guard_rows=GUARD, stream=stream, three_launches=three, device=dev)


def _unit(f, ops, dev, **kw):
    """the unit kernel, once: (trunk, h1', flags); the launch counters prove which kernel ran"""
    c = _call(f, ops, dev, **kw)
    _flags()
    L.launch_counts(clear=True)
    c.run()
    torch.cuda.synchronize(dev)
    n = L.launch_counts(clear=True)
    assert n["b1_unit"] == 1 and n["conv3x3_stream"] == 0, n
    return c.trunk, c.h1, _flags()


def _three(f, ops, dev, **kw):
    """the three hmmr_conv_gemm launches the unit replaces, on the same operands"""
    c = _call(f, ops, dev, three=True, **kw)
    _flags()
    L.launch_counts(clear=True)
    c.run()
    torch.cuda.synchronize(dev)
    n = L.launch_counts(clear=True)
    assert n["b1_unit"] == 0 and n["conv3x3_stream"] == 1, n
    return c.trunk, c.h1, _flags()


def _case(grid, form, dev, name="", **kw):
    """host operands, their upload and their three-launch reference (None where the reference refuses the grid): made once, left unchanged"""
    key = (grid, form, name, tuple(sorted(kw.items())))
    if key not in _cases:
        d = B.operands(grid, form, name)
        ops = _upload(d, dev)
        _cases[key] = (d, ops, None if grid in REFERENCE_REFUSES else _three(B.filters(form), ops, dev, **kw))
    return _cases[key]


def _sentinels(got, m, what):
    """the guard rows still hold the sentinel, no word of a valid row does"""
    from human_dynamics_amd import engine as E
    for name, a, c in (("trunk", got[0], 256), ("h1'", got[1], 64)):
        assert tuple(a.shape) == (m + GUARD, c), (what, name, a.shape)
        assert bool((a[m:] == E.PAIR_SENTINEL).all()), "%s %s: a store past row %d" % (what, name, m)
        left = (a[:m] == E.PAIR_SENTINEL).any(dim=1).nonzero()[:, 0]
        assert left.numel() == 0, "%s %s: %d valid rows were not stored (first %s)" % (what, name, left.numel(), left[:8].tolist())


def _same(got, want, m, what):
    """outputs equal bit for bit, guard rows (still the sentinel in both) included"""
    from human_dynamics_amd import packing
    _sentinels(got, m, what)
    _sentinels(want, m, what + " (three launches)")
    for name, a, b in (("trunk", got[0], want[0]), ("h1'", got[1], want[1])):
        if not torch.equal(a, b):
            bad = torch.unique((a != b).nonzero()[:, 0])
            raise AssertionError("%s %s: %d rows differ (first %s), max |diff| %.3e" % (
                what, name, bad.numel(), bad[:8].tolist(), float((packing.from_split(a[:m]) - packing.from_split(b[:m])).abs().max())))


def _values(t, m):
    from human_dynamics_amd import packing
    return packing.from_split(t[:m]).double().cpu().numpy()


def _float64(f, d, got, m, what, relu1=True, bias=True):
    """trunk against the float64 chain on the operands as stored, h1' against float64 from the trunk the kernel STORED.  Bound: 2e-5
    max(1, max |ref|), that of every split kernel's test."""
    et, eh = B.errors(_values(got[0], m), _values(got[1], m), f, d, relu1=relu1, bias=bias)
    print("device %-9s %-22s trunk max |err| %.3e (max |ref| %.3e)   h1' max |err| %.3e (max |ref| %.3e)" % ((what[0], what[1]) + et + eh))
    assert et[1] > 1.0 and eh[1] > 0.1
    assert B.inside(et), (what, "trunk", et)
    assert B.inside(eh), (what, "h1'", eh)


def _m(grid):
    return grid[0] * grid[1] * grid[2]


# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.GRIDS, ids=_grid_id)
def test_b1_unit_grid_shapes(grid, form, gpu_device):
    """1x1x1: M = 1.  129x1x1: every pixel is all four borders, a wave with one valid row, 129 images in two tiles.  5x1x56: top == bot
    at the widest row.  3x56x1: lef == rig, a halo of 2 rows.  7x3x5: several whole images inside one wave's 32 pixels.  1x3x11: M = 33.
    1x4x8: one wave.  4x8x4: one tile exactly.  2x16x40 / 2x40x16: H != W on whole tiles.  1x56x55 / 1x55x56: an odd width against the
    patch swizzle (r >> 2) & 3, an odd height.  1x8x8, 5x24x24, 3x56x56: the shapes of tests/test_gpu_b1_unit.py.
    Measured on an MI355X (profiles/b1_unit_sweep.log): trunk max |err| <= 4.2e-6 with max |ref| 4-11, h1' <= 3.6e-6 with max |ref| 2-9;
    the bound is 2e-5 max(1, max |ref|) = 0.8-2.3e-4."""
    f, m = B.filters(form), _m(grid)
    d, ops, want = _case(grid, form, gpu_device)
    got = _unit(f, ops, gpu_device)
    what = (B.grid_id(grid), form)
    if want is not None:
        _same(got, want, m, "%s %s" % what)
        assert want[2] == 0, want[2]
    else:
        with pytest.raises(L.HmmrError):
            _three(f, ops, gpu_device)
        _sentinels(got, m, "%s %s" % what)
    assert got[2] == 0, got[2]
    _float64(f, d, got, m, what)


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("n", B.TILE_COUNTS)
def test_b1_unit_tile_counts_around_the_xcd_remap(n, form, gpu_device):
    """n images of 8 x 16 = n tiles: below, at and above the 8 XCDs and twice that; xcd_remap covers every tile once for every count (a
    tile computed twice shows nowhere, a tile left out keeps the sentinel)"""
    grid = (n,) + B.TILE_GRID
    d, ops, want = _case(grid, form, gpu_device)
    got = _unit(B.filters(form), ops, gpu_device)
    _same(got, want, _m(grid), "%d tiles %s" % (n, form))
    assert got[2] == 0 and want[2] == 0


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_more_tiles_than_fit_at_once(form, gpu_device):
    """22 x 56 x 56 = 539 tiles (more images where the device has more than 269 CUs): more than two workgroups per CU hold at once, the
    last tile half empty.  Twice: the same bytes."""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    n = max(22, -(-(2 * cus + 1) * 128 // (56 * 56)))
    grid, f = (n, 56, 56), B.filters(form)
    assert -(-_m(grid) // 128) > 2 * cus
    ops = _upload(B.operands.__wrapped__(grid, form), gpu_device)
    want = _three(f, ops, gpu_device)
    got = _unit(f, ops, gpu_device)
    _same(got, want, _m(grid), "%s %s" % (B.grid_id(grid), form))
    assert got[2] == 0 and want[2] == 0
    del want
    again = _unit(f, ops, gpu_device)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and again[2] == 0


# ------------------------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.KNOWN_GRIDS, ids=B.grid_id)
def test_b1_unit_known_answers_of_every_tap(grid, form, gpu_device):
    """w2 one-hot at tap (ky, kx), identities and powers of two behind it, integer operands: trunk channel c of pixel (y, x) EQUALS
    s(c) h1[y + ky - 1, x + kx - 1, c % 64] (0 outside the image) + the shortcut, h1' = relu(trunk[..., :64]).  2x9x4: H > W, so a swapped
    H / W in the wrapper or the kernel shows."""
    n, h, w = grid
    m = _m(grid)
    ops = _upload(B.known_operands(grid, form), gpu_device)
    for ky in range(3):
        for kx in range(3):
            got = _unit(B.known_filters(ky, kx, form), ops, gpu_device, skey="known %d %d" % (ky, kx), bias=False)
            assert got[2] == 0, (ky, kx, got[2])
            _sentinels(got, m, "tap (%d, %d)" % (ky, kx))
            for name, t, e in zip(("trunk", "h1'"), got[:2], B.known_expected(grid, form, ky, kx)):
                v = _values(t, m)
                e = e.reshape(m, -1)
                if not np.array_equal(v, e):
                    bad = np.argwhere(v != e)
                    p, c = bad[0]
                    raise AssertionError("tap (ky %d, kx %d) %s: %d values differ; the first at image %d, y %d, x %d, channel %d: got %r, expected %r" % (
                        ky, kx, name, len(bad), p // (h * w), p % (h * w) // w, p % w, c, v[p, c], e[p, c]))


# ------------------------------------------------------------------------------------------------------------------ d
def test_b1_unit_shortcut_row_stride_above_256(gpu_device):
    """ldr = 320: the shortcut is a view into a wider buffer whose other columns are NaN -- never read (no flag), the same bits"""
    grid, f = B.FLAG_GRID, B.filters("identity")
    d, ops, want = _case(grid, "identity", gpu_device)
    got = _unit(f, ops, gpu_device, res_ld=320)
    _same(got, want, _m(grid), "ldr 320")
    assert got[2] == 0, got[2]
    dense = _unit(f, ops, gpu_device)
    assert torch.equal(got[0], dense[0]) and torch.equal(got[1], dense[1])
    _float64(f, d, got, _m(grid), ("ldr 320", "identity"))


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_without_relu1(form, gpu_device):
    """relu1 = 0: h1' is clamped at -65504 instead of 0"""
    grid, f = B.FLAG_GRID, B.filters(form)
    d, ops, want = _case(grid, form, gpu_device, relu1=False)
    got = _unit(f, ops, gpu_device, relu1=False)
    _same(got, want, _m(grid), form + " relu1=0")
    assert got[2] == 0 and want[2] == 0
    _float64(f, d, got, _m(grid), ("relu1=0", form), relu1=False)
    assert _values(got[1], _m(grid)).min() < -0.1


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_without_bias3(form, gpu_device):
    """shift3 = NULL: the kernel's sB3 = 0 branch"""
    grid, f = B.FLAG_GRID, B.filters(form)
    d, ops, want = _case(grid, form, gpu_device, bias=False)
    got = _unit(f, ops, gpu_device, bias=False)
    _same(got, want, _m(grid), form + " shift3=NULL")
    assert got[2] == 0 and want[2] == 0
    _float64(f, d, got, _m(grid), ("shift3=NULL", form), bias=False)
    assert not torch.equal(_case(grid, form, gpu_device)[2][0], want[0])


# ------------------------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_saturation_flags(form, gpu_device):
    """a clean run raises nothing; a saturating trunk, h1' (upper clamp; lower clamp with relu1 = 0) and h2 raise SATURATED -- the bits and
    the flags of the three launches"""
    dev, m = gpu_device, _m(B.FLAG_GRID)
    d, ops, want = _case(B.FLAG_GRID, form, dev)
    clean = _unit(B.filters(form), ops, dev)
    assert clean[2] == 0 and want[2] == 0
    _same(clean, want, m, form)

    def saturated(f, d_, what, **kw):
        o = _upload(d_, dev) if d_ is not d else ops
        w_, g_ = _three(f, o, dev, **kw), _unit(f, o, dev, **kw)
        assert g_[2] == L.FLAG_SATURATED and w_[2] == L.FLAG_SATURATED, (what, g_[2], w_[2])
        _same(g_, w_, m, "%s %s" % (form, what))
        return g_

    f, big = B.saturating_trunk(form)
    g = saturated(f, big, "saturated trunk")
    assert np.abs(_values(g[0], m)).max() == 65504.0
    f, d_, relu1 = B.saturating_h1(form)
    g = saturated(f, d, "saturated h1'")
    assert _values(g[1], m).max() == 65504.0 and np.abs(_values(g[0], m)).max() < 100 and torch.equal(g[0], clean[0])
    f, d_, relu1 = B.saturating_h1(form, lower=True)
    assert not relu1
    g = saturated(f, d, "h1' at the lower clamp", relu1=False)
    assert _values(g[1], m).min() == -65504.0 and _values(g[1], m).max() < 0 and torch.equal(g[0], clean[0])
    f, d_ = B.saturating_h2(form)
    saturated(f, d, "saturated h2")
    # (every _unit / _three call above read AND cleared the flags) a clean run after all that raises nothing and gives the clean bits
    again = _unit(B.filters(form), ops, dev)
    assert again[2] == 0 and torch.equal(again[0], clean[0]) and torch.equal(again[1], clean[1])


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", B.NAN_GRIDS, ids=B.grid_id)
def test_b1_unit_nan_operands_stay_in_their_neighbourhoods(grid, form, gpu_device):
    """a NaN half in h1 at pixel 0, at pixel M - 1 (the two pixels the patch clamp re-reads for rows outside the tensor) and at a corner
    of the middle image: the NAN flag, and every output pixel OUTSIDE the in-image 3 x 3 neighbourhoods has the clean run's bits (nothing
    is asserted inside them)"""
    dev, m, f = gpu_device, _m(grid), B.filters(form)
    d, ops, want = _case(grid, form, dev)
    clean = _unit(f, ops, dev)
    assert clean[2] == 0
    bad = _upload(B.poisoned(grid, form), dev)
    got = _unit(f, bad, dev)
    assert got[2] & L.FLAG_NAN, got[2]
    _sentinels(got, m, "NaN operands")
    keep = torch.from_numpy(np.concatenate([~B.poisoned_neighbourhood(grid), np.ones(GUARD, bool)])).to(dev)
    assert int(keep.sum()) == m + GUARD - 12
    for name, a, b in (("trunk", got[0], clean[0]), ("h1'", got[1], clean[1])):
        rows = ((a != b).any(dim=1) & keep).nonzero()[:, 0]
        assert rows.numel() == 0, "%s: a NaN reached %d pixels outside the neighbourhoods (first %s)" % (name, rows.numel(), rows[:8].tolist())
    if want is not None:
        assert _three(f, bad, dev)[2] & L.FLAG_NAN


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_images_are_independent(form, gpu_device):
    """image 2 of 6: its rows do not change when the other five images are replaced by other data"""
    from human_dynamics_amd import packing
    grid, dev, f = B.FLAG_GRID, gpu_device, B.filters(form)
    n, h, w = grid
    d, ops, want = _case(grid, form, dev)
    other = {k: v.copy() for k, v in B.operands(grid, form, "other").items()}
    for k in other:
        assert not np.array_equal(other[k][1], d[k][1]) and not np.array_equal(other[k][3], d[k][3])
        other[k][2] = d[k][2]
    a, b = _unit(f, ops, dev), _unit(f, _upload(other, dev), dev)
    rows = slice(2 * h * w, 3 * h * w)
    assert torch.equal(a[0][rows], b[0][rows]) and torch.equal(a[1][rows], b[1][rows])
    assert not torch.equal(a[0][:rows.start], b[0][:rows.start]) and not torch.equal(a[0][rows.stop:], b[0][rows.stop:])
    assert float(packing.from_split(a[0][rows]).abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------------------------ f
def test_b1_unit_refusals_queue_nothing(gpu_device):
    """every check of hmmr_b1_unit_split: refused with its message, the sentinel outputs untouched, and the good call that follows gives
    the reference bits"""
    from human_dynamics_amd import engine as E
    dev, grid = gpu_device, B.FLAG_GRID
    m = _m(grid)
    assert len(B.REFUSALS) >= 21
    for name, form, fields, words in B.REFUSALS:
        f = B.filters(form)
        d, ops, want = _case(grid, form, dev)
        c = _call(f, ops, dev)
        B.apply_refusal(c.descs[0], fields, c.trunk.data_ptr())
        with pytest.raises(L.HmmrError, match=words):
            c.run()
        torch.cuda.synchronize(dev)
        assert bool((c.trunk == E.PAIR_SENTINEL).all()) and bool((c.h1 == E.PAIR_SENTINEL).all()), "%s: refused, yet something was stored" % name
        got = _unit(f, ops, dev)
        _same(got, want, m, "after the refusal of '%s'" % name)
        assert got[2] == 0, (name, got[2])
