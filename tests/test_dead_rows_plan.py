"""hmmr_unit_plan_t.trunk_keep_stride (host only): which units of the ResNet-50 table the plan tells to store only the trunk rows the
next unit's strided identity shortcut reads.  The rule (csrc/resnet.hip, plan_unit, next to writes_raw): the next unit has stride 2, takes
its shortcut as the strided identity (HMMR_SC_NONE), and the raw trunk has no other reader -- the unit's end computed the next conv1
(leaves_h1) -- and the end is one of the two kernels that honour the field (the unit pair, the block-1 unit).

Expected, written down from the unit table: units 2, 6, 12 (block1/unit_3, block2/unit_4, block3/unit_6) have stride 2 and an identity
shortcut; their producers are units 1, 5, 11 -- b1_unit_kernel, unit_pair 128 -> 512 -> 128, unit_pair 256 -> 1024 -> 256."""
import ctypes as C

import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import packing

INT_MAX = 2 ** 31 - 1
PRODUCERS = [1, 5, 11]


def _pack(weights, dtype, **kw):
    store = packing.DeviceStore("cpu")
    return packing.pack_resnet(weights, dtype, store, **kw), store


def _set_debug(**kw):
    d = L.Debug()
    for k, v in kw.items():
        setattr(d, k, v)
    L.load().hmmr_set_debug(C.byref(d))


def _kept(plan):
    return {u: p.trunk_keep_stride for u, p in enumerate(plan) if p.trunk_keep_stride}


@pytest.fixture(autouse=True)
def _product_debug_state():
    yield
    L.load().hmmr_set_debug(None)


def test_the_table_has_the_three_stride_2_identity_units(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    assert [u for u in range(L.RESNET_UNITS) if rw.unit[u].stride == 2] == [2, 6, 12]
    assert all(not rw.unit[u].shortcut.w and not rw.unit[u].c3sc.w for u in (2, 6, 12))


def test_f16x3_marks_exactly_the_three_producers(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    # 257 frames, the default switches: every pair is on (block 3 has 50 372 pixels)
    plan = L.resnet_plan(rw, 257)
    assert _kept(plan) == {1: 2, 5: 2, 11: 2}
    assert [plan[u].end for u in PRODUCERS] == [L.END_B1_UNIT, L.END_UNIT_PAIR, L.END_UNIT_PAIR]
    # what makes the rows dead: the consumer launches neither a conv1 nor a shortcut, so x[:, ::2, ::2] is the trunk's one reader
    for u in PRODUCERS:
        assert plan[u].leaves_h1 and plan[u].writes_raw and not plan[u].writes_pre
        assert plan[u + 1].conv1 == L.CONV1_READY and plan[u + 1].shortcut == L.SC_NONE
    # 20 frames: block 3's pairs are demoted to the two launches (3 920 pixels), which store every row
    assert _kept(L.resnet_plan(rw, 20)) == {1: 2, 5: 2}
    _set_debug(pair_min_pixels=1)
    assert _kept(L.resnet_plan(rw, 3)) == {1: 2, 5: 2, 11: 2}


def test_none_without_the_kernels_that_honour_it(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    _set_debug(pair_min_pixels=INT_MAX)                      # pairs switched off: only the block-1 unit is left
    assert _kept(L.resnet_plan(rw, 257)) == {1: 2}
    _set_debug()
    rw, _keep = _pack(weights, L.HMMR_F16X3, b1_unit=False)    # block 1 ends in the LDS-panel tail
    plan = L.resnet_plan(rw, 257)
    assert plan[1].end == L.END_TAIL_SPLIT and _kept(plan) == {5: 2, 11: 2}
    _set_debug(pair_min_pixels=INT_MAX)
    assert _kept(L.resnet_plan(rw, 257)) == {}
    _set_debug()
    rw, _keep = _pack(weights, L.HMMR_F16X3, fuse_tail=False)  # layer by layer: every end is a conv3 launch
    assert _kept(L.resnet_plan(rw, 257)) == {}


def test_none_when_the_successor_reads_more_of_the_trunk(weights):
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    for u in (2, 6, 12):
        assert rw.unit[u].stride == 2
        rw.unit[u].stride = 1                                # a stride-1 successor reads every row
    assert _kept(L.resnet_plan(rw, 257)) == {}
    rw, _keep = _pack(weights, L.HMMR_F16X3)
    plan = L.resnet_plan(rw, 257)
    # the units in front of a block's FIRST unit (conv shortcut: it pre-activates the whole trunk) are the stride-2 units themselves,
    # which end in a conv3 launch; and no unit followed by a conv-shortcut unit is marked
    for u in range(L.RESNET_UNITS - 1):
        if rw.unit[u + 1].shortcut.w or rw.unit[u + 1].c3sc.w:
            assert plan[u].trunk_keep_stride == 0, u


def test_none_in_bf16_and_fp32(weights):
    for dtype in (L.HMMR_BF16, L.HMMR_F32):
        rw, _keep = _pack(weights, dtype)
        assert _kept(L.resnet_plan(rw, 257)) == {}, dtype
