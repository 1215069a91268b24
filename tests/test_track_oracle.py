"""The track front end without a GPU: the NumPy restatement (tests/track_oracle.py) against what the reference's smooth_bbox.py
returned with SciPy (tests/golden/reference_tracks.npz), the PoseFlow reader against the reference's lists, the packing helper,
the new symbols and what the entry points refuse before they launch anything."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import track_oracle as TO
from conftest import GOLDEN, ROOT
from human_dynamics_amd import _lib
from human_dynamics_amd.evaluation import tracks as T

RECORDED = ("k25", "mixed", "bad_rows", "short")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_tracks.npz")))


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.maximum(1, np.abs(want))
    assert (err <= 1e-12).all(), err.max()


def _recorded_tracks(ref, name):
    return T.unpack_tracks(ref[name + "/kps"], ref[name + "/present"], ref[name + "/offsets"])


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_agrees_with_the_reference(ref, name):
    vis = float(ref["vis_thresh"])
    for t, trk in enumerate(_recorded_tracks(ref, name)):
        raw, start, end = TO.get_all_bbox_params(trk, vis)
        assert [start, end] == ref["%s/%d/range" % (name, t)].tolist()
        _close(raw, ref["%s/%d/raw" % (name, t)])
        if start < 0:
            with pytest.raises(ValueError):
                TO.get_smooth_bbox_params(trk, vis)
            continue
        smooth, s2, e2 = TO.get_smooth_bbox_params(trk, vis)
        assert (s2, e2) == (start, end) and not smooth[:start].any()
        _close(smooth, ref["%s/%d/smooth" % (name, t)])


def test_the_seeded_cases_are_the_recorded_ones(ref):
    """the fixture was recorded from track_oracle.seeded_cases(): the generator still gives the same tracks"""
    cases = TO.seeded_cases()
    for name in ("k25", "mixed", "bad_rows"):
        kps, present, offsets = T.pack_tracks(cases[name][2])
        assert np.array_equal(kps, ref[name + "/kps"]) and np.array_equal(present, ref[name + "/present"])
        assert np.array_equal(offsets, ref[name + "/offsets"]) and list(cases[name][:2]) == ref[name + "/hw"].tolist()
    assert [len(t) for t in cases["lengths"][2]] == list(TO.LENGTHS) and TO.TILE == _lib.TRACK_TILE


def test_filters_alone(ref):
    keys = sorted(k[:-3] for k in ref if k.startswith("filters/") and k.endswith("/in"))
    assert len(keys) == 12
    for key in keys:
        n, ks, sigma = key.split("/")[1].split("_")
        _close(TO.smooth_bbox_params(ref[key + "/in"], int(ks), float(sigma)), ref[key + "/out"])
    assert not ref["filters/5_11_3/out"].any()              # fewer than six rows: the median is padding
    from human_dynamics_amd.util import smooth_bbox
    for sigma in (0.5, 3, 8, 16):
        w, r = smooth_bbox.gaussian_weights(sigma)
        w2, r2 = TO.gaussian_weights(sigma)
        assert r == r2 == int(4 * sigma + 0.5) and np.array_equal(w, w2) and abs(w.sum() - 1) < 1e-15


def test_no_recorded_row_is_a_near_tie(ref):
    for name in RECORDED:
        h, w = ref[name + "/hw"]
        n_tracks = len(ref[name + "/offsets"]) - 1
        for t in range(n_tracks):
            start = ref["%s/%d/range" % (name, t)][0]
            for b in ref["%s/%d/smooth" % (name, t)][max(start, 0):]:
                assert TO.rounding_margin(h, w, b) >= float(ref["margin"])


def test_oracle_geometry_is_crop_geometry(ref):
    """the status word is non-zero exactly where run_video.crop_geometry raises; elsewhere the integers are its integers"""
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    seen = set()
    for name in RECORDED:
        h, w = (int(v) for v in ref[name + "/hw"])
        for t in range(len(ref[name + "/offsets"]) - 1):
            start = ref["%s/%d/range" % (name, t)][0]
            for b in ref["%s/%d/smooth" % (name, t)][max(start, 0):]:
                st, geom, info = TO.crop_geometry(h, w, b)
                seen.add(st)
                if st:
                    with pytest.raises(ValueError):
                        crop_geometry(h, w, b)
                    assert geom.tolist() == [h, w, 0, 0] and not info.any()
                else:
                    g = crop_geometry(h, w, b)
                    assert geom.tolist() == [g["hs"], g["ws"], g["u0"], g["v0"]]
                    assert info.tolist() == [g["start_pt"][0], g["start_pt"][1], g["center"][0], g["center"][1], g["scale"]]
    assert {0, TO.EMPTY, TO.CLIPPED} <= seen
    assert TO.crop_geometry(96, 128, [-400., 50., 1.5])[0] == TO.BEFORE_ORIGIN
    assert TO.crop_geometry(96, 128, [np.nan, 50., 1.5])[0] == TO.crop_geometry(96, 128, [10., 50., np.inf])[0] == TO.NOT_FINITE
    assert (TO.EMPTY, TO.BEFORE_ORIGIN, TO.CLIPPED, TO.NOT_FINITE) == (_lib.TRACK_EMPTY, _lib.TRACK_BEFORE_ORIGIN, _lib.TRACK_CLIPPED,
                                                                       _lib.TRACK_NOT_FINITE)


@pytest.mark.parametrize("name", ["full", "full_min20", "holes"])
def test_get_labels_poseflow_equals_the_reference(ref, tmp_path, name):
    path = tmp_path / (name + ".json")
    path.write_bytes(ref["poseflow/%s/json" % name].tobytes())
    num_frames, min_count = (int(v) for v in ref["poseflow/%s/args" % name])
    assert int(ref["poseflow/%s/stopped" % name]) == 0
    got = T.get_labels_poseflow(str(path), num_frames, min_count)
    want = T.unpack_tracks(*(ref["poseflow/%s/%s" % (name, k)] for k in ("kps", "present", "offsets")))
    assert len(got) == len(want) >= 1
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and np.array_equal(a, b)))
    if name == "full":
        assert len(got) == 5 and got[0][0] is not None and got[1][0] is None          # the longest first; None before the first appearance
        assert len(T.get_labels_poseflow(str(path), num_frames)) == 1                 # the default min_kp_count is 20


def test_get_labels_poseflow_raises_where_the_reference_stops(ref, tmp_path):
    path = tmp_path / "late.json"
    path.write_bytes(ref["poseflow/late/json"].tobytes())
    assert int(ref["poseflow/late/stopped"]) == 1 and min(json.loads(path.read_text())) == "00002.png"
    with pytest.raises(ValueError, match="first frame"):
        T.get_labels_poseflow(str(path), 30, 5)


def test_pack_tracks_round_trips():
    rng = np.random.default_rng(3)
    trks = [[None, rng.normal(size=(17, 3)), None, rng.normal(size=(17, 3))], [rng.normal(size=(17, 3))], [None, None], []]
    kps, present, offsets = T.pack_tracks(trks)
    assert kps.shape == (7, 17, 3) and kps.dtype == np.float64 and present.dtype == np.uint8 and offsets.dtype == np.int32
    assert present.tolist() == [0, 1, 0, 1, 1, 0, 0] and offsets.tolist() == [0, 4, 5, 7, 7] and not kps[present == 0].any()
    back = T.unpack_tracks(kps, present, offsets)
    assert [len(t) for t in back] == [4, 1, 2, 0]
    for t, b in zip(trks, back):
        for a, c in zip(t, b):
            assert (a is None and c is None) or np.array_equal(a, c)
    assert T.pack_tracks([[None, None]])[0].shape == (2, 1, 3)
    with pytest.raises(ValueError):
        T.pack_tracks([[np.zeros((17, 3)), np.zeros((25, 3))]])
    with pytest.raises(ValueError):
        T.pack_tracks([[np.zeros((17, 2))]])


def test_new_symbols_are_declared_bound_and_exported():
    names = ("hmmr_track_workspace_bytes", "hmmr_track_bbox", "hmmr_track_smooth", "hmmr_track_crop_geom")
    header = open(os.path.join(ROOT, "include", "hmmr_hip.h")).read()
    lib = _lib.load()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    assert lib.hmmr_abi_version() == 19
    for macro, value in (("HMMR_TRACK_MAX_KPS", _lib.TRACK_MAX_KPS), ("HMMR_TRACK_MAX_KERNEL", _lib.TRACK_MAX_KERNEL),
                         ("HMMR_TRACK_MAX_RADIUS", _lib.TRACK_MAX_RADIUS), ("HMMR_TRACK_TILE", _lib.TRACK_TILE)):
        assert int(re.search(r"#define %s (\d+)" % macro, header).group(1)) == value
    assert lib.hmmr_track_workspace_bytes(1000, 3) >= 1000 * (3 * 3 * 8 + 2 * 4)
    assert lib.hmmr_track_workspace_bytes(-1, 1) == 0 and lib.hmmr_track_workspace_bytes(10, 0) == 0


def test_track_entry_points_refuse_bad_arguments():
    """dummy, never dereferenced device pointers: everything is refused before a launch, with a message"""
    lib = _lib.load()
    P = [0x1000 * (i + 1) for i in range(8)]
    i32 = lambda v: np.asarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    w = np.ones(129) / 129.
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    big = 1 << 20

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc == -1 and msg, (rc, msg)
        for word in words:
            assert word in msg, (word, msg)

    def bbox(**kw):
        a = dict(kps=P[0], present=P[1], off=[0, 10, 30], nt=2, k=17, thr=0.1, ks=11, w=wp, r=12, raw=None, smooth=P[2], range=P[3], ws=P[4],
                 wsb=big)
        a.update(kw)
        return lib.hmmr_track_bbox(a["kps"], a["present"], i32(a["off"]) if a["off"] is not None else None, a["nt"], a["k"], a["thr"], a["ks"],
                                   a["w"], a["r"], a["raw"], a["smooth"], a["range"], a["ws"], a["wsb"], None)

    for name in ("kps", "present", "smooth", "range", "ws"):
        refused(bbox(**{name: None}), b"hmmr_track_bbox", b"null")
    refused(bbox(off=None), b"null offsets")
    refused(bbox(w=None), b"null gauss_w")
    refused(bbox(off=[0, 30, 10]), b"hmmr_track_bbox", b"not monotone")
    refused(bbox(off=[-1, 10, 30]), b"negative")
    refused(bbox(nt=0), b"n_tracks")
    refused(bbox(k=0), b"1 <= k <= 64")
    refused(bbox(k=65), b"1 <= k <= 64")
    for ks in (0, -1, 2, 10, 33, 32):
        refused(bbox(ks=ks), b"kernel_size")
    refused(bbox(r=65), b"gauss_radius")
    refused(bbox(r=-1), b"gauss_radius")
    refused(bbox(wsb=lib.hmmr_track_workspace_bytes(30, 2) - 1), b"workspace")

    def smooth(**kw):
        a = dict(p=P[0], off=[0, 10], nt=1, ks=11, w=wp, r=12, out=P[1], ws=P[2], wsb=big)
        a.update(kw)
        return lib.hmmr_track_smooth(a["p"], i32(a["off"]), a["nt"], a["ks"], a["w"], a["r"], a["out"], a["ws"], a["wsb"], None)

    refused(smooth(p=None), b"hmmr_track_smooth", b"null")
    refused(smooth(out=None), b"null")
    refused(smooth(ks=4), b"kernel_size")
    refused(smooth(r=100), b"gauss_radius")
    refused(smooth(wsb=8), b"workspace")
    refused(smooth(off=[5, 2]), b"not monotone")

    def geom(**kw):
        a = dict(box=P[0], off=[0, 10, 30], range=P[1], nt=2, h=96, w=128, geom=P[2], info=P[3], status=P[4])
        a.update(kw)
        return lib.hmmr_track_crop_geom(a["box"], i32(a["off"]), a["range"], a["nt"], a["h"], a["w"], a["geom"], a["info"], a["status"], None)

    for name in ("box", "geom", "status"):
        refused(geom(**{name: None}), b"hmmr_track_crop_geom", b"null")
    refused(geom(h=0), b"h >= 1")
    refused(geom(w=0), b"w >= 1")
    refused(geom(off=[0, 40, 30]), b"not monotone")
    with pytest.raises(_lib.HmmrError):
        _lib.check(geom(h=-3), "hmmr_track_crop_geom")


def test_the_track_front_end_does_not_import_scipy():
    for rel in ("util/smooth_bbox.py", "evaluation/tracks.py", "evaluation/run_video.py", "_lib.py", "__init__.py", "util/__init__.py"):
        path = os.path.join(ROOT, "human_dynamics_amd", rel)
        assert not re.search(r"^\s*(import|from)\s+scipy\b", open(path).read(), flags=re.M), path
