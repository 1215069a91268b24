"""hmmr_tail_desc_t.trunk_keep_stride: the block-1 unit (csrc/b1_unit.hip, both forms) and the unit pair (csrc/unit_pair.hip: the two
shapes with a shortcut tensor, as one wave per SIMD, as persistent workgroups forced on, and wave-specialised) ALONE, each case run once
with keep stride 2 and once with stride 0 on the same operands, and the whole ResNet with and without hmmr_debug_t.keep_dead_rows.

`out` starts as a sentinel word everywhere and is followed by guard rows, the inputs are followed by rows of NaN halves
(engine.B1UnitCall / engine.UnitPairCall with guard_rows).  Per case:

    live rows (y % 2 == 0 and x % 2 == 0 inside their image)   bit-equal between the two runs
    dead rows                                                  still the sentinel in every word: never stored
    h1'                                                        bit-equal everywhere, no sentinel left in a valid row
    guard rows                                                 intact in both runs
    hmmr_run_flags                                             equal
    hmmr_trunk_keep_launches                                   1 against 0: which path ran

The stride-0 run is the parent's kernel path, which tests/test_gpu_b1_unit_kernel.py and tests/test_gpu_unit_pair.py hold against the
launches it replaces and against float64; nothing here repeats that.

The pair's third shape (the shortcut folded into conv3's K) has no shortcut tensor, is never followed by a stride-2 unit and is REFUSED a
keep stride (its kernel compiles to the parent's instructions): it appears among the refusals, not among the cases."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import b1_unit_cases as B
from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets

pytestmark = pytest.mark.gpu

GUARD = 3
# (images, H, W).  1x1 and 2x2 images; odd sizes keep rows and columns 0, 2, 4 as x[::2, ::2] does; 4x6; 14x14; 7 x (3x5): several
# images inside one wave's 32 pixels; 3 x (7x9) = 63-pixel images: an image straddles the 32-pixel wave tiles and the 128-pixel
# workgroup tile; M = 1, 33, 129 one-pixel images: every row is live, in one wave, two waves, two workgroups
GRIDS = ((1, 1, 1), (33, 1, 1), (129, 1, 1), (3, 2, 2), (2, 3, 5), (2, 5, 3), (2, 4, 6), (2, 14, 14), (7, 3, 5), (3, 7, 9))
PAIR_SHAPES = {"b3": (256, 1024, 256), "b2": (128, 512, 128)}                  # c_mid, depth, n2
# form -> (shape, hmmr_debug_t.pair_form, pair_two_tile_min): the persistent geometry exists for the block-2 shape only
PAIR_FORMS = {"b3": ("b3", 0, 0), "b2": ("b2", 0, 0), "b2_persistent": ("b2", 0, 1), "b3_ws": ("b3", 2, 0), "b2_ws": ("b2", 2, 0)}
_pair_filters = {}


def _gid(g):
    return "%dx%dx%d" % g


def _flags():
    """read and clear hmmr_run_flags"""
    fl = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(fl), 1), "hmmr_run_flags")
    return fl.value


def _keep_launches():
    return int(L.load().hmmr_trunk_keep_launches(1))


def _live(grid, s, dev):
    """[M] bool: the rows x[:, ::s, ::s] reads"""
    n, h, w = grid
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    one = (y % s == 0) & (x % s == 0)
    assert one.sum() == -(-h // s) * -(-w // s)
    return torch.from_numpy(np.tile(one.reshape(-1), n)).to(dev)


def _run(call, dev, want_keep):
    """(trunk, h1', flags) of one launch; the counter says whether a keep stride was in force"""
    _flags()
    _keep_launches()
    call.run()
    torch.cuda.synchronize(dev)
    assert _keep_launches() == want_keep
    return call.trunk, call.h1, _flags()


def _check(kept, full, grid, dev, what, stride=2):
    from human_dynamics_amd import engine as E
    m = grid[0] * grid[1] * grid[2]
    live = _live(grid, stride, dev)
    S = E.PAIR_SENTINEL
    for name, t in (("trunk", kept[0]), ("h1'", kept[1]), ("trunk (stride 0)", full[0]), ("h1' (stride 0)", full[1])):
        assert t.shape[0] == m + GUARD and bool((t[m:] == S).all()), "%s %s: a store into the guard rows" % (what, name)
    assert not bool((full[0][:m] == S).any()) and not bool((full[1][:m] == S).any()), "%s: stride 0 left a valid row unstored" % what
    assert torch.equal(kept[0][:m][live], full[0][:m][live]), "%s: a live trunk row differs" % what
    dead = kept[0][:m][~live]
    assert bool((dead == S).all()), "%s: %d of %d dead trunk rows were stored" % (what, int((dead != S).any(dim=1).sum()), dead.shape[0])
    assert torch.equal(kept[1], full[1]), "%s: h1' differs" % what
    assert kept[2] == full[2], "%s: run flags %r with the keep stride, %r without" % (what, kept[2], full[2])


# ------------------------------------------------------------------------------------------------------------------ block-1 unit
def _b1_call(form, ops, dev, keep, f=None):
    from human_dynamics_amd import engine as E
    f = f or B.filters(form)
    shortcut = (ops["xp"], f["wsc"], f["bsc"]) if form == "folded" else None
    return E.B1UnitCall(ops["h1"], (f["w2"],) + tuple(f["bn2"]), f["w3"], f["b3"], f["pre"], f["w1"], f["bn1"], res=ops.get("res"),
                        shortcut=shortcut, guard_rows=GUARD, keep_stride=keep, device=dev)


def _b1_ops(d, dev):
    from human_dynamics_amd import packing
    return {k: packing.to_split(torch.from_numpy(v).to(dev)) for k, v in d.items()}


@pytest.mark.parametrize("form", B.FORMS)
@pytest.mark.parametrize("grid", GRIDS, ids=_gid)
def test_b1_unit_stores_only_live_rows(grid, form, gpu_device):
    ops = _b1_ops(B.operands(grid, form, "dead rows"), gpu_device)
    full = _run(_b1_call(form, ops, gpu_device, 0), gpu_device, 0)
    kept = _run(_b1_call(form, ops, gpu_device, 2), gpu_device, 1)
    _check(kept, full, grid, gpu_device, "b1 %s %s" % (form, _gid(grid)))
    assert full[2] == 0


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_other_strides_and_the_switch(form, gpu_device):
    """stride 1 is stride 0; stride 3 keeps rows and columns 0, 3; hmmr_debug_t.keep_dead_rows stores every row whatever the field says"""
    from human_dynamics_amd import engine as E
    grid, dev = (2, 5, 7), gpu_device
    ops = _b1_ops(B.operands(grid, form, "dead rows"), dev)
    full = _run(_b1_call(form, ops, dev, 0), dev, 0)
    one = _run(_b1_call(form, ops, dev, 1), dev, 0)
    assert torch.equal(one[0], full[0]) and torch.equal(one[1], full[1])
    _check(_run(_b1_call(form, ops, dev, 3), dev, 1), full, grid, dev, "b1 %s stride 3" % form, stride=3)
    try:
        E.set_debug(keep_dead_rows=1)
        forced = _run(_b1_call(form, ops, dev, 2), dev, 0)
    finally:
        E.set_debug()
    assert torch.equal(forced[0], full[0]) and torch.equal(forced[1], full[1]) and forced[2] == full[2]


@pytest.mark.parametrize("form", B.FORMS)
def test_b1_unit_saturating_trunk_raises_the_flag_with_either_stride(form, gpu_device):
    """the clamp and the flag come before the store: dead rows saturate the flag as live ones do"""
    f, big = B.saturating_trunk(form)
    ops = _b1_ops(big, gpu_device)
    full = _run(_b1_call(form, ops, gpu_device, 0, f), gpu_device, 0)
    kept = _run(_b1_call(form, ops, gpu_device, 2, f), gpu_device, 1)
    assert full[2] == L.FLAG_SATURATED and kept[2] == L.FLAG_SATURATED, (full[2], kept[2])
    _check(kept, full, B.FLAG_GRID, gpu_device, "b1 %s saturating" % form)


# ------------------------------------------------------------------------------------------------------------------ unit pair
def _pair_filter_set(shape, dev):
    if shape not in _pair_filters:
        from human_dynamics_amd import packing
        cm, depth, n2 = PAIR_SHAPES[shape]
        g = torch.Generator(device="cpu").manual_seed(zlib.crc32(("dead rows/" + shape).encode()))
        rnd = lambda *s: torch.randn(*s, generator=g)
        f = {"W3": (rnd(depth, cm) / cm ** 0.5).numpy(), "W1": (rnd(n2, depth) / depth ** 0.5).numpy(), "b3": rnd(depth).numpy(),
             "pre": ((torch.rand(depth, generator=g) + 0.5).numpy(), (rnd(depth) * 0.3).numpy()),
             "bn1": ((torch.rand(n2, generator=g) + 0.5).numpy(), (rnd(n2) * 0.3).numpy())}
        f["stream"] = packing.pack_pair_stream(f["W3"], f["W1"]).to(dev)
        _pair_filters[shape] = f
    return _pair_filters[shape]


def _pair_rows(shape, m, dev, scale_h2=1.0, scale_res=1.0):
    """ReLU'd normal h2, normal res, as split device tensors (made on the device: the largest case has 65 k rows)"""
    from human_dynamics_amd import packing
    cm, depth, n2 = PAIR_SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(("dead rows/%s/%d" % (shape, m)).encode()))
    h2 = torch.randn(m, cm, generator=g, device=dev).clamp_(min=0) * scale_h2
    res = (torch.randn(m, depth, generator=g, device=dev) * scale_res).clamp_(-6e4, 6e4)
    return packing.to_split(h2), packing.to_split(res)


def _pair_call(shape, rows, grid, dev, keep):
    from human_dynamics_amd import engine as E
    f = _pair_filter_set(shape, dev)
    return E.UnitPairCall(rows[0], f["W3"], f["b3"], f["pre"], f["W1"], f["bn1"], res=rows[1], guard_rows=GUARD, stream=f["stream"],
                          grid=grid[1:], keep_stride=keep, device=dev)


def _pair_both(form, grid, dev, rows=None):
    """(kept, full) of the pair in `form`; the unit_pair counter proves the kernel, the keep counter the path"""
    from human_dynamics_amd import engine as E
    shape, pair_form, two_min = PAIR_FORMS[form]
    m = grid[0] * grid[1] * grid[2]
    rows = rows or _pair_rows(shape, m, dev)
    try:
        E.set_debug(pair_form=pair_form, pair_two_tile_min=two_min)
        L.launch_counts(clear=True)
        full = _run(_pair_call(shape, rows, grid, dev, 0), dev, 0)
        kept = _run(_pair_call(shape, rows, grid, dev, 2), dev, 1)
        assert L.launch_counts(clear=True)["unit_pair"] == 2
    finally:
        E.set_debug()
    return kept, full


@pytest.mark.parametrize("form", list(PAIR_FORMS))
@pytest.mark.parametrize("grid", GRIDS, ids=_gid)
def test_unit_pair_stores_only_live_rows(grid, form, gpu_device):
    kept, full = _pair_both(form, grid, gpu_device)
    _check(kept, full, grid, gpu_device, "pair %s %s" % (form, _gid(grid)))
    assert full[2] == 0


@pytest.mark.parametrize("tiles", ["1", "3", "cus+1", "2cus+1"])
def test_unit_pair_persistent_geometries(tiles, gpu_device):
    """persistent workgroups forced on, images of 8 x 16 = one 128-pixel tile each: one tile, an odd count below the CU count (two
    tiles per workgroup, the last workgroup one), one more tile than CUs, and 2 CUs + 1 (three rounds, the last a single tile) -- the
    live mask and the dead-row line are set up again for every tile of a workgroup"""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    n = {"1": 1, "3": 3, "cus+1": cus + 1, "2cus+1": 2 * cus + 1}[tiles]
    grid = (n, 8, 16)
    kept, full = _pair_both("b2_persistent", grid, gpu_device)
    _check(kept, full, grid, gpu_device, "pair b2 persistent, %d tiles" % n)
    assert full[2] == 0


@pytest.mark.parametrize("form", list(PAIR_FORMS))
def test_unit_pair_saturating_trunk_raises_the_flag_with_either_stride(form, gpu_device):
    grid, dev = (6, 5, 7), gpu_device
    rows = _pair_rows(PAIR_FORMS[form][0], 6 * 5 * 7, dev, scale_h2=3e3, scale_res=5e4)
    kept, full = _pair_both(form, grid, dev, rows=rows)
    assert full[2] == L.FLAG_SATURATED and kept[2] == L.FLAG_SATURATED, (full[2], kept[2])
    _check(kept, full, grid, dev, "pair %s saturating" % form)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_queue_nothing(gpu_device):
    """hmmr_bottleneck_tail refuses the field where it cannot hold -- before anything is queued: the outputs keep the sentinel, no
    launch is counted -- and the good call that follows stores the live rows"""
    from human_dynamics_amd import engine as E
    from human_dynamics_amd import packing
    dev, grid = gpu_device, (2, 4, 6)
    m = 2 * 4 * 6
    rows = _pair_rows("b2", m, dev)
    some = torch.zeros(64, dtype=torch.int32, device=dev)

    def pair(**fields):
        c = _pair_call("b2", rows, grid, dev, 2)
        for k, v in fields.items():
            setattr(c.descs[0], k, v)
        return c

    def folded():
        f = _pair_filter_set("b2", dev)
        xp = packing.to_split(torch.randn(m, 256, device=dev).clamp_(min=0))
        wsc = (np.random.default_rng(1).normal(size=(512, 256)) / 16).astype(np.float32)
        return E.UnitPairCall(rows[0], f["W3"], f["b3"], f["pre"], f["W1"], f["bn1"], shortcut=(xp, wsc), guard_rows=GUARD, grid=grid[1:],
                              keep_stride=2, device=dev)

    def b1(**fields):
        c = _b1_call("identity", _b1_ops(B.operands(grid, "identity", "dead rows"), dev), dev, 2)
        for k, v in fields.items():
            setattr(c.descs[0], k, v)
        return c

    cases = [("out_pre beside it (pair)", pair(out_pre=some.data_ptr()), "trunk_keep_stride 2 needs"),
             ("out_pre beside it (block-1 unit)", b1(out_pre=some.data_ptr()), "trunk_keep_stride 2 needs"),
             ("the LDS-panel tail (no stream)", pair(pair_stream=None, w3=some.data_ptr(), w1=some.data_ptr()), "trunk_keep_stride 2 needs"),
             ("a bf16 tail", pair(dtype=L.HMMR_BF16, pair_stream=None, w3=some.data_ptr(), w1=some.data_ptr()), "trunk_keep_stride 2 needs"),
             ("a negative stride", pair(trunk_keep_stride=-2), "trunk_keep_stride -2 needs"),
             ("the folded pair", folded(), "needs a shortcut tensor"),
             ("a pair without its image grid", pair(ho=0, wo=0), "whole ho x wo images"),
             ("a pair on part of an image", pair(ho=5, wo=5), "whole ho x wo images")]
    for name, c, words in cases:
        _keep_launches()
        with pytest.raises(L.HmmrError, match=words):
            c.run()
        torch.cuda.synchronize(dev)
        assert bool((c.trunk == E.PAIR_SENTINEL).all()) and bool((c.h1 == E.PAIR_SENTINEL).all()), "%s: refused, yet something was stored" % name
        assert _keep_launches() == 0, name
    kept, full = _pair_both("b2", grid, dev, rows=rows)
    _check(kept, full, grid, dev, "after the refusals")


# ------------------------------------------------------------------------------------------------------------------ whole ResNet
@pytest.fixture(scope="module")
def f16x3_engine(weights, gpu_device):
    from human_dynamics_amd import engine as E
    return E.HmmrEngine(weights, None, dtype="f16x3", device=gpu_device, autotune=False)


def _phi(eng, frames, **debug):
    """(phi, keep-stride launches, unit_pair launches) of one pass with the pairs forced on"""
    from human_dynamics_amd import engine as E
    try:
        E.set_debug(pair_min_pixels=1, **debug)
        _keep_launches()
        L.launch_counts(clear=True)
        phi = eng.resnet(frames, parts=1).clone()
        torch.cuda.synchronize()
        return phi, _keep_launches(), L.launch_counts(clear=True)["unit_pair"]
    finally:
        E.set_debug()


@pytest.mark.parametrize("n", [3, 5])
def test_resnet_features_do_not_depend_on_the_dead_rows(n, f16x3_engine):
    frames = assets.make_synthetic_frames(n, seed=11)
    want, keep0, pairs0 = _phi(f16x3_engine, frames, keep_dead_rows=1)
    got, keep1, pairs1 = _phi(f16x3_engine, frames)
    assert (keep1, keep0) == (3, 0) and pairs0 == pairs1 == 8, (keep1, keep0, pairs1, pairs0)
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1


def test_resnet_on_two_concurrent_streams(f16x3_engine, gpu_device):
    """3 and 5 frames at once on two streams (each pass its own workspace; both launches aim their dead rows at the same region): the
    features of the sequential keep_dead_rows passes"""
    from human_dynamics_amd import engine as E
    eng = f16x3_engine
    fa, fb = eng.to_device(assets.make_synthetic_frames(3, seed=11)), eng.to_device(assets.make_synthetic_frames(5, seed=12))
    want_a, want_b = _phi(eng, fa, keep_dead_rows=1)[0], _phi(eng, fb, keep_dead_rows=1)[0]
    sa, sb = torch.cuda.Stream(device=gpu_device), torch.cuda.Stream(device=gpu_device)
    torch.cuda.synchronize()
    try:
        E.set_debug(pair_min_pixels=1)
        _keep_launches()
        with torch.cuda.stream(sa):
            got_a = eng.resnet(fa, parts=1, ws_key="dead_rows_a")
        with torch.cuda.stream(sb):
            got_b = eng.resnet(fb, parts=1, ws_key="dead_rows_b")
        torch.cuda.synchronize()
        assert _keep_launches() == 6
    finally:
        E.set_debug()
    assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
