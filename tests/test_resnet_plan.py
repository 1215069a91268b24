"""The ResNet unit schedule as a value (hmmr_resnet50_plan, include/hmmr_hip.h): which launches a packed unit table gives every unit,
decided on the host before anything is queued.  The expected plans below are written down from the header's description of
hmmr_resnet_unit_t.fuse_tail and from the launch counts the GPU tests of the same configurations assert (test_gpu_b1_unit.py,
test_gpu_conv1x1_stream.py) -- not read off the planner.  The GPU test closes the loop: the counters after a pass equal the plan's."""
import ctypes as C

import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets, packing

INT_MAX = 2 ** 31 - 1
# ResNet-50's 16 units: blocks of 3, 4, 6, 3; a block's last unit has stride 2 (not block 4's), its first a conv shortcut
BLOCK1, BLOCK2, BLOCK3, BLOCK4 = [0, 1, 2], [3, 4, 5, 6], [7, 8, 9, 10, 11, 12], [13, 14, 15]
STRIDE2 = [2, 6, 12]


def _pack(weights, dtype, **kw):
    store = packing.DeviceStore("cpu")
    return packing.pack_resnet(weights, dtype, store, **kw), store


def _set_debug(**kw):
    d = L.Debug()
    for k, v in kw.items():
        setattr(d, k, v)
    L.load().hmmr_set_debug(C.byref(d))


def _ends(plan, kind):
    return [u for u, p in enumerate(plan) if p.end == kind]


def predicted_counts(rw, plan):
    """hmmr_launch_counts_t of one pass, from its plan and the K order the packer gave each launched layer"""
    c = dict.fromkeys([k for k, _ in L.LaunchCounts._fields_], 0)
    for u, p in enumerate(plan):
        U = rw.unit[u]
        c["unit_pair"] += p.end == L.END_UNIT_PAIR
        c["b1_unit"] += p.end == L.END_B1_UNIT
        c["tail_split"] += p.end == L.END_TAIL_SPLIT
        c["conv3x3_stream"] += p.conv2 == L.CONV2_LAUNCH and U.conv2.k_order == 2
        conv3 = U.c3sc if p.shortcut == L.SC_IN_CONV3 else U.conv3
        c["conv1x1_stream"] += ((p.shortcut == L.SC_LAUNCH_WITH_CONV1 and U.sc_c1.k_order == 2) + (p.conv1 == L.CONV1_LAUNCH and U.conv1.k_order == 2) +
                                (p.end == L.END_CONV3_LAUNCH and conv3.k_order == 2))
    return c


@pytest.fixture(autouse=True)
def _product_debug_state():
    yield
    L.load().hmmr_set_debug(None)


def test_f16x3_shipped_plan(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    for n in (20, 67):       # block 2: 15 680 / 52 528 pixels (pairs), block 3: 3 920 / 13 132, below its 14 000 (the two launches)
        plan = L.resnet_plan(rw, n)
        assert _ends(plan, L.END_B1_UNIT) == [0, 1]
        assert _ends(plan, L.END_UNIT_PAIR) == BLOCK2[:3]
        assert [u for u, p in enumerate(plan) if p.pair_demoted] == BLOCK3[:5]
        assert _ends(plan, L.END_TAIL_SPLIT) == [] and len(_ends(plan, L.END_CONV3_LAUNCH)) == 16 - 2 - 3
        c = predicted_counts(rw, plan)
        assert (c["b1_unit"], c["unit_pair"], c["tail_split"], c["conv1x1_stream"]) == (2, 3, 0, 8), c
    _set_debug(pair_min_pixels=1)
    plan = L.resnet_plan(rw, 20)
    assert _ends(plan, L.END_UNIT_PAIR) == BLOCK2[:3] + BLOCK3[:5] and not any(p.pair_demoted for p in plan)
    # a pair leaves the next unit's conv1 behind, and so does the stem (conv1_frag) and each block-1 unit
    assert [u for u, p in enumerate(plan) if p.conv1 == L.CONV1_READY] == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert plan[7].shortcut == L.SC_LAUNCH_WITH_CONV1          # (block3/unit_1 keeps its shortcut as a launch, with conv1 as extra columns)
    assert predicted_counts(rw, plan)["conv1x1_stream"] == 8
    _set_debug(pair_min_pixels=INT_MAX)
    plan = L.resnet_plan(rw, 300)
    assert _ends(plan, L.END_UNIT_PAIR) == [] and sum(p.pair_demoted for p in plan) == 8
    assert predicted_counts(rw, plan)["b1_unit"] == 2


def test_f16x3_development_schedules(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3, fuse_tail=False)
    plan = L.resnet_plan(rw, 7)
    assert _ends(plan, L.END_CONV3_LAUNCH) == list(range(16))
    assert all(p.conv2 == L.CONV2_LAUNCH and not p.leaves_h1 and not p.swaps_t1_t2 for p in plan)
    c = predicted_counts(rw, plan)
    assert c["conv3x3_stream"] == 13 and c["b1_unit"] == c["unit_pair"] == c["tail_split"] == 0, c      # 11 + block 1's two
    rw, _keep = _pack(weights, L.HMMR_F16X3, b1_unit=False)
    plan = L.resnet_plan(rw, 7)
    assert _ends(plan, L.END_TAIL_SPLIT) == [0, 1] and _ends(plan, L.END_B1_UNIT) == []
    assert [plan[u].conv2 for u in (0, 1)] == [L.CONV2_IN_TAIL] * 2 and [plan[u].swaps_t1_t2 for u in (0, 1)] == [1, 1]
    rw, _keep = _pack(weights, L.HMMR_F16X3, stream_1x1=False)
    assert predicted_counts(rw, L.resnet_plan(rw, 7))["conv1x1_stream"] == 0


def test_bf16_and_f32_shipped_plans(weights):
    rw, _keep = _pack(weights, L.HMMR_BF16)
    plan = L.resnet_plan(rw, 9)
    # hmmr_resnet_unit_t.fuse_tail: 3 = block1/unit_1 (conv2 and the conv shortcut inside the tail), 2 = the other stride-1 units of
    # blocks 1-2, 4 = their stride-2 last units; blocks 3-4 launch layer by layer
    assert (plan[0].shortcut, plan[0].conv2, plan[0].end) == (L.SC_IN_TAIL, L.CONV2_IN_TAIL, L.END_TAIL_BF16)
    assert _ends(plan, L.END_TAIL_BF16) == [0, 1, 3, 4, 5]
    assert _ends(plan, L.END_TAIL_BF16_STRIDE2) == [2, 6]
    assert _ends(plan, L.END_CONV3_LAUNCH) == BLOCK3 + BLOCK4
    assert [u for u, p in enumerate(plan) if p.conv2 == L.CONV2_IN_TAIL] == [0, 1, 2, 3, 4, 5, 6]
    # conv1 without a launch: after the stem, after every tail with a next conv1, and with the shortcut launch of blocks 3-4 (sc_c1)
    assert [u for u, p in enumerate(plan) if p.conv1 == L.CONV1_READY] == [0, 1, 2, 4, 5, 6, 7, 13]
    assert [plan[u].shortcut for u in (3, 7, 13)] == [L.SC_LAUNCH, L.SC_LAUNCH_WITH_CONV1, L.SC_LAUNCH_WITH_CONV1]
    assert [u for u, p in enumerate(plan) if p.swaps_t1_t2] == [0, 1, 3, 4, 5] and not any(p.pair_demoted for p in plan)
    c = predicted_counts(rw, plan)
    assert c["unit_pair"] == c["b1_unit"] == c["tail_split"] == c["conv1x1_stream"] == 0
    _set_debug(stem_no_conv1=1)
    assert L.resnet_plan(rw, 9)[0].conv1 == L.CONV1_LAUNCH
    _set_debug()
    rw, _keep = _pack(weights, L.HMMR_F32)
    plan = L.resnet_plan(rw, 9)
    assert _ends(plan, L.END_CONV3_LAUNCH) == list(range(16))
    assert all(p.conv2 == L.CONV2_LAUNCH and not p.leaves_h1 for p in plan)
    # blocks 3-4 run the shortcut and conv1 of their first unit as one column-split GEMM (sc_c1), blocks 1-2 as two launches
    assert [p.shortcut for p in plan] == [{0: L.SC_LAUNCH, 3: L.SC_LAUNCH, 7: L.SC_LAUNCH_WITH_CONV1, 13: L.SC_LAUNCH_WITH_CONV1}.get(u, L.SC_NONE)
                                          for u in range(16)]
    assert [u for u, p in enumerate(plan) if p.conv1 == L.CONV1_READY] == [7, 13]
    # a block's first unit reads a stored pre-activated tensor (fuse_preact 0): its predecessor writes that instead of the raw trunk
    assert [u for u, p in enumerate(plan) if p.writes_pre] == STRIDE2 and [u for u, p in enumerate(plan) if not p.writes_raw] == STRIDE2
    assert [u for u, p in enumerate(plan) if not p.reads_fused_preact] == [0, 3, 7, 13]
    assert predicted_counts(rw, plan) == dict.fromkeys(predicted_counts(rw, plan), 0)


def test_an_inconsistent_table_is_refused_with_the_unit_named(weights):
    lib = L.load()
    out = (L.UnitPlan * L.RESNET_UNITS)()
    rw, _keep = _pack(weights, L.HMMR_BF16)
    assert rw.unit[5].fuse_tail == 2 and rw.unit[6].fuse_preact == 1
    rw.unit[5].fuse_tail = 1
    assert lib.hmmr_resnet50_plan(C.byref(rw), 4, out) == 0
    rw.unit[6].fuse_preact = 0                    # the tail of unit 5 would pre-activate for a unit that reads a stored tensor
    assert lib.hmmr_resnet50_plan(C.byref(rw), 4, out) == -1
    assert lib.hmmr_last_error() == b"resnet: unit 5 cannot fuse its tail"
    with pytest.raises(L.HmmrError, match="unit 5 cannot fuse its tail"):
        L.resnet_plan(rw, 4)
    rw, _keep = _pack(weights, L.HMMR_F32)
    rw.unit[9].fuse_tail = 1                      # no fused tail is built for fp32 operands
    assert lib.hmmr_resnet50_plan(C.byref(rw), 4, out) == -1 and b"unit 9 cannot fuse its tail" in lib.hmmr_last_error()
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    rw.unit[13].fuse_preact = 1                   # a folded shortcut (c3sc) reads the stored pre-activated tensor
    assert lib.hmmr_resnet50_plan(C.byref(rw), 4, out) == -1 and b"unit 13 cannot fold its shortcut into conv3" in lib.hmmr_last_error()
    assert lib.hmmr_resnet50_plan(None, 4, out) == -1 and lib.hmmr_resnet50_plan(C.byref(rw), 0, out) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,debug", [("f16x3", {}), ("f16x3", {"pair_min_pixels": 1}), ("bf16", {})],
                         ids=["f16x3_default", "f16x3_pairs_forced", "bf16"])
def test_launch_counters_equal_the_plan(weights, gpu_device, dtype, debug):
    """3 frames + 1 zero frame (blocks 3-4 end in ragged tiles: 784 / 196 pixels): the five launch counters after one pass are
    the ones the plan of the same table, frame count and debug state predicts."""
    import torch
    from human_dynamics_amd import engine as E
    eng = E.HmmrEngine(weights, None, dtype=dtype, device=gpu_device, autotune=False)
    frames = assets.make_synthetic_frames(3, seed=7)
    try:
        E.set_debug(**debug)
        want = predicted_counts(eng.rw, L.resnet_plan(eng.rw, 4))
        L.launch_counts(clear=True)
        phi = eng.resnet(frames, n_zero=1, parts=1)
        torch.cuda.synchronize()
        got = L.launch_counts(clear=True)
    finally:
        E.set_debug()
    print(dtype, debug, "plan:", want, "counters:", got)
    assert got == want
    assert sum(want.values()) > 0 and bool(torch.isfinite(phi).all()) and float(phi.abs().max()) > 0.1
    if debug:
        assert want["unit_pair"] == 8
