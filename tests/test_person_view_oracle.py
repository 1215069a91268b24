"""tests/person_view_oracle.py (the float64 restatement of hmmr_video_bbox) against tests/golden/reference_video_bbox.npz, which
tests/golden/make_video_bbox_golden.py wrote by executing the reference's compute_video_bbox and visualize_mesh_og."""
import os

import numpy as np
import pytest

import person_view_oracle as PV
from conftest import GOLDEN


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_video_bbox.npz")))


def camera_bound(want):
    """one fp32 rounding of the result (half an ulp <= 2^-24 |ref|; 2^-23 leaves room for a result one fp64 ulp to the other side
    of a rounding boundary) plus the fp64 error of the cancelling terms o12 - S / (2 o0), which are of order 1e3 (1e3 2^-52 = 2e-13)"""
    return 2.0 ** -23 * np.abs(want.astype(np.float64)) + 1e-12


def test_fixture_holds_the_cases_the_issue_names(ref):
    meta, off = ref["meta"], ref["offsets"]
    assert sorted(set(map(tuple, meta[:, :2]))) == [(240, 320), (720, 1280), (1080, 810)]
    assert sorted(set(np.diff(off))) == [1, 7, 40] and sorted(set(meta[:, 2])) == [0, 10, 25]
    assert ref["kps"].shape[1:] == (25, 2) and ref["cams"].dtype == ref["kps"].dtype == ref["cams_crop"].dtype == np.float32
    assert 0.4 <= ref["proc"][:, 0].min() and ref["proc"][:, 0].max() <= 2.5
    raw, hw = ref["bbox_raw"], meta[:, :2]
    binds = np.stack([raw[:, 0] == 0, raw[:, 1] == hw[:, 0] - 1, raw[:, 2] == 0, raw[:, 3] == hw[:, 1] - 1], 1)
    assert binds.any(0).all()                                            # each of the four clamps binds in some case
    free = ~binds
    assert (np.abs(raw - np.rint(raw))[free] >= 1e-6).all()              # truncation is not a matter of the last bit
    trapped = np.array([ref["trap"][a:b].any() for a, b in zip(off[:-1], off[1:])])
    assert trapped.sum() >= 2 and (~trapped).sum() >= 2
    S = np.maximum(ref["bbox"][:, 1] - ref["bbox"][:, 0], ref["bbox"][:, 3] - ref["bbox"][:, 2])
    assert S.min() >= 16


def test_restatement_equals_the_reference_track_by_track(ref):
    off = ref["offsets"]
    worst = 0.0
    for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
        h, w, margin = (int(x) for x in ref["meta"][t])
        got = PV.video_bbox(ref["cams"][a:b], ref["kps"][a:b], ref["proc"][a:b], 224., [0, b - a], h, w, margin)
        assert np.array_equal(got["bbox"][0], ref["bbox"][t]), (t, got["bbox"], ref["bbox"][t])
        assert np.array_equal(got["trap"], ref["trap"][a:b]), t
        assert got["status"][0] == (PV.BEYOND_START if ref["trap"][a:b].any() else 0)
        want = ref["cams_crop"][a:b]
        err = np.abs(got["cams_crop"].astype(np.float64) - want)
        worst = max(worst, float((err / camera_bound(want)).max()))
        assert (err <= camera_bound(want)).all(), (t, float(err.max()))
    print("restatement vs reference: largest camera difference %.3f of the bound" % worst)


def test_one_ragged_call_equals_the_single_tracks(ref):
    """tracks that share a frame size and a margin in one call (the margin is per call): the same answers"""
    off = ref["offsets"]
    for t in range(len(off) - 1):
        a, b = int(off[t]), int(off[t + 1])
        h, w, margin = (int(x) for x in ref["meta"][t])
        rows = np.r_[a:b, a:b][: 2 * (b - a) - 1]                       # the track, an empty track, the track without its last frame
        got = PV.video_bbox(ref["cams"][rows], ref["kps"][rows], ref["proc"][rows], 224., [0, b - a, b - a, len(rows)], h, w, margin)
        assert np.array_equal(got["bbox"][0], ref["bbox"][t]) and got["status"][1] == PV.EMPTY and not got["bbox"][1].any()
        assert np.array_equal(got["cams_crop"][:b - a], PV.video_bbox(ref["cams"][a:b], ref["kps"][a:b], ref["proc"][a:b], 224., [0, b - a], h, w,
                                                                       margin)["cams_crop"])


def test_status_rules_of_the_restatement(ref):
    a, b = int(ref["offsets"][4]), int(ref["offsets"][5])
    h, w, margin = (int(x) for x in ref["meta"][4])
    cams, kps, proc = ref["cams"][a:b].copy(), ref["kps"][a:b].copy(), ref["proc"][a:b].copy()
    bad = kps.copy()
    bad[3, 7, 1] = np.nan
    got = PV.video_bbox(cams, bad, proc, 224., [0, b - a], h, w, margin)
    assert got["status"][0] == PV.NOT_FINITE and not got["bbox"].any() and np.isnan(got["cams_crop"]).all()
    far = proc.copy()
    far[:, 1] = 1e13                                                     # an extreme no int32 holds (xmin; xmax is clamped)
    got = PV.video_bbox(cams, kps, far, 224., [0, b - a], h, w, margin)
    assert got["status"][0] == PV.NOT_FINITE
    flat = np.zeros_like(kps)                                            # a point person with no margin, left of the frame: xmin = xmax = 0, ymin = ymax
    shifted = proc.copy()
    shifted[:, 1:3] = 0
    got = PV.video_bbox(cams, flat, shifted, 224., [0, b - a], h, w, 0)
    assert got["status"][0] & PV.DEGENERATE


def test_visualize_mesh_og_sizes_follow_resize_img(ref):
    """image_size of the box branch is clip_size's longer side; the recorded camera of that branch is the crop camera itself"""
    for m, cam in zip(ref["og_meta"], ref["og_cam"]):
        case, row, h, w, max_img, deg, boxed, size = (int(x) for x in m)
        if boxed:
            assert PV.clip_size(ref["bbox"][case], max_img)[2] == size
            assert np.array_equal(cam, ref["cams_crop"][row])
        else:
            s = max_img / float(max(h, w)) if max(h, w) > max_img else 1.0
            assert size == (max(int(np.floor(h * s)), int(np.floor(w * s))) if s != 1.0 else max(h, w))
