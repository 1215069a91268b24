"""The scene view's host side (include/hmmr_hip.h: hmmr_render_scene, csrc/render.hip): the C ABI and every refusal it makes
before a launch (dummy, never dereferenced device pointers), the workspace query, and the laws of the NumPy spec
(tests/scene_oracle.py) that tests/test_gpu_scene.py holds the kernel to -- among them the ambiguity cap of its seeded
cases, which is a condition on the cases, asserted here, not a measurement of the kernel.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_oracle as O
import scene_oracle as SO
from human_dynamics_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_scene_symbols_are_bound_and_abi_unchanged():
    lib = _lib.load()
    for name in ("hmmr_render_scene", "hmmr_render_scene_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.hmmr_abi_version() == 19 and _lib.SCENE_MAX_TRACKS == 16


def _header_fields(first, struct):
    hdr = open(os.path.join(ROOT, "include", "hmmr_hip.h")).read()
    end = hdr.index("} %s;" % struct)
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex(first, 0, end):end], flags=re.S)
    names = []
    for decl in body.replace("\n", " ").split(";"):
        for part in decl.split(","):
            m = re.search(r"\*?\s*([a-z_0-9]+)\s*(\[\d+\])?\s*$", part.strip())
            if m:
                names.append(m.group(1))
    return names


def test_scene_structs_match_the_header_field_order():
    assert _header_fields("const float* verts; int64_t ld_verts;", "hmmr_scene_track_t") == [f for f, _ in _lib.SceneTrack._fields_]
    assert _header_fields("const hmmr_scene_track_t* tracks;", "hmmr_scene_desc_t") == [f for f, _ in _lib.SceneDesc._fields_]
    assert "#define HMMR_SCENE_MAX_TRACKS 16" in open(os.path.join(ROOT, "include", "hmmr_hip.h")).read()


def test_scene_workspace_query():
    lib = _lib.load()
    q = lib.hmmr_render_scene_workspace_bytes
    for bad in ((0, 1, 10, 10), (4097, 1, 10, 10), (4, 0, 10, 10), (4, 17, 10, 10), (4, 2, 0, 10), (4, 2, 10, 0), (4, 2, 10, 65537)):
        assert q(*bad) == 0
    # slabs of max(1, 64 // n_tracks) frames: the workspace does not grow with n_frames past one slab
    for n_tracks in (1, 3, 16):
        slab = max(1, 64 // n_tracks)
        assert q(slab + 1, n_tracks, 6890, 13776) == q(4096, n_tracks, 6890, 13776) == q(slab, n_tracks, 6890, 13776)
        assert 0 < q(1, n_tracks, 6890, 13776) <= q(slab, n_tracks, 6890, 13776)
        # at most 64 instances: no more than hmmr_render_mesh's own 64-frame slab
        assert q(4096, n_tracks, 6890, 13776) <= lib.hmmr_render_workspace_bytes(64, 6890, 13776)
    assert q(1, 1, 6890, 13776) == lib.hmmr_render_workspace_bytes(1, 6890, 13776)


def _desc(n_tracks=2, n_frames=6, size=64):
    """a valid call with dummy device pointers; returns (desc, tracks) -- the host array must outlive the call"""
    arr = (_lib.SceneTrack * max(n_tracks, 1))()
    for i in range(max(n_tracks, 1)):
        t = arr[i]
        t.verts, t.ld_verts, t.cams, t.ld_cam = 0x1000, 30, 0x2000, 3
        t.start, t.end = i % 2, n_frames - i % 2
    d = _lib.SceneDesc()
    d.tracks, d.n_tracks, d.faces, d.rgb, d.ws = arr, n_tracks, 0x3000, 0x4000, 0x5000
    d.nv, d.nf, d.n_frames, d.size = 10, 8, n_frames, size
    d.out_h = d.out_w = size
    d.ws_bytes = _lib.load().hmmr_render_scene_workspace_bytes(n_frames, max(min(n_tracks, 16), 1), 10, 8)
    return d, arr


def test_a_valid_descriptor_passes_validation_up_to_the_workspace():
    """the dummy descriptor is refused ONLY for what each case below breaks: with a short workspace as its one fault it
    gets as far as the last check"""
    lib = _lib.load()
    d, keep = _desc()
    d.ws_bytes -= 1
    assert lib.hmmr_render_scene(C.byref(d), None) == -1 and b"workspace" in lib.hmmr_last_error()


@pytest.mark.parametrize("field,value,msg", [
    ("tracks", None, b"NULL operand"), ("faces", None, b"NULL operand"), ("rgb", None, b"NULL operand"), ("ws", None, b"NULL operand"),
    ("n_tracks", 0, b"n_tracks = 0"), ("n_tracks", 17, b"n_tracks = 17"), ("n_frames", 0, b"n_frames = 0"),
    ("n_frames", 4097, b"n_frames = 4097"), ("size", 15, b"size = 15"), ("size", 1025, b"size = 1025"), ("nf", 0, b"nf = 0"),
    ("nf", 65537, b"nf = 65537"), ("nv", 2, b"nv = 2"), ("out_h", 65, b"output"), ("out_w", 0, b"output"),
    ("bg_mode", 1, b"bg_mode"), ("bg_mode", 3, b"bg_mode"), ("bg_mode", 2, b"without bg_image"), ("ws_bytes", 100, b"workspace"),
])
def test_render_scene_validates_before_any_launch(field, value, msg):
    lib = _lib.load()
    d, keep = _desc(n_tracks=17 if (field, value) == ("n_tracks", 17) else 2)
    setattr(d, field, value)
    assert lib.hmmr_render_scene(C.byref(d), None) == -1
    assert msg in lib.hmmr_last_error(), lib.hmmr_last_error()
    assert lib.hmmr_render_scene(None, None) == -1


@pytest.mark.parametrize("field,value,msg", [
    ("verts", None, b"NULL operand in track 1"), ("cams", None, b"NULL operand in track 1"),
    ("start", -1, b"track 1 covers"), ("start", 5, b"track 1 covers"), ("start", 6, b"track 1 covers"), ("end", 7, b"track 1 covers"),
    ("ld_verts", 29, b"row strides of track 1"), ("ld_cam", 2, b"row strides of track 1"),
])
def test_render_scene_validates_every_track(field, value, msg):
    lib = _lib.load()
    d, arr = _desc()                                   # track 1 covers [1, 5) of 6 frames
    setattr(arr[1], field, value)
    assert lib.hmmr_render_scene(C.byref(d), None) == -1
    assert msg in lib.hmmr_last_error(), lib.hmmr_last_error()


def test_render_scene_refuses_a_frame_background_without_its_size():
    lib = _lib.load()
    d, keep = _desc()
    d.bg_mode, d.bg_image = 2, 0x6000
    assert lib.hmmr_render_scene(C.byref(d), None) == -1 and b"frame size" in lib.hmmr_last_error()


def test_python_front_refuses_bad_track_lists():
    from human_dynamics_amd.util.render import raster
    f = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError):
        raster.render_scene([], f, 32, 4)
    with pytest.raises(ValueError):
        raster.render_scene([{}] * 17, f, 32, 4)
    assert raster.scene_color(0) == raster.COLORS['blue'] and raster.scene_color(1) == raster.COLORS['pink']
    assert raster.scene_color(len(raster.SCENE_COLORS)) == raster.COLORS['blue']            # the cycle
    assert raster.scene_color(1, ['red', (0.1, 0.2, 0.3)]) == [0.1, 0.2, 0.3]
    assert set(raster.SCENE_COLORS) == set(raster.COLORS)


# ------------------------------------------------------------------------------------------------ the spec's laws
def test_one_track_is_the_mesh_renderer():
    c = SO.case("three80")
    trk = dict(c["tracks"][1], range=(0, 5))
    got = SO.render([trk], c["faces"], c["S"], 5, frames=c["frames"][:5], out_hw=c["out_hw"])
    for r in (0, 4):
        cam, _ = SO.frame_camera(trk["cams"][r], trk["geom"][r])
        bg = O.resize_frame(c["frames"][r], *c["out_hw"])
        ref = O.render(O.project(trk["verts"][r], cam), c["faces"], c["S"], color=trk["color"], bg=bg, bg_kind='frame', out_hw=c["out_hw"])
        for k in ("rgb", "alpha", "index", "ambiguous", "pixel_ambiguous"):
            assert np.array_equal(got[r][k], ref[k]), k
        assert np.array_equal(got[r]["owner"] >= 0, ref["index"] >= 0) and got[r]["owner"].max() == 0


def test_frame_camera_is_the_handoff_formula():
    from oracle import handoff_oracle as HO
    c = SO.case("three48")
    trk = c["tracks"][0]
    p = trk["params"][0]
    h, w = c["out_hw"]
    new_cam, _, _ = HO.orig_camera(trk["cams"][0], np.zeros((1, 2), np.float32), p["start_pt"], 1.0 / trk["geom"][0][0], 224, (h, w), 10 ** 6)
    cam, scale = SO.frame_camera(trk["cams"][0], trk["geom"][0])
    assert np.allclose(cam, new_cam, rtol=1e-6, atol=1e-6) and abs(scale - cam[0]) <= 1e-6 * scale


def test_order_rules():
    assert SO._order([(0, 1.0), (1, 2.0), (2, 1.5)]) == [1, 2, 0]                       # descending
    assert SO._order([(0, 1.0), (1, 1.0), (2, 3.0)]) == [2, 0, 1]                       # ties: lower track first
    assert SO._order([(0, float("nan")), (1, -5.0), (2, float("inf")), (3, 0.0)]) == [3, 1, 0, 2]   # non-finite last


def test_layering_beats_local_depth_and_ranges_use_their_own_rows():
    c = SO.case("three48")
    ref = SO.reference("three48")
    assert [r["order"] for r in ref] == [[0], [0, 1], [0, 1], [0, 1, 2], [1, 2], [1]]
    r = ref[3]
    i0, p0 = r["solo"][0]
    i1, p1 = r["solo"][1]
    both = (i0 >= 0) & (i1 >= 0) & ~r["ambiguous"]
    assert both.sum() > 100 and (r["owner"][both] == 0).all()
    z0, z1 = SO.depth_at(p0, c["faces"], c["S"], i0), SO.depth_at(p1, c["faces"], c["S"], i1)
    assert (z0[both] > z1[both]).all()                     # the owner is the FARTHER one in local z everywhere they overlap
    # rows differ per frame, so using row f instead of f - start would show
    t1 = c["tracks"][1]
    assert not np.array_equal(t1["verts"][0], t1["verts"][1]) and not np.array_equal(t1["geom"][0], t1["geom"][1])


def test_default_keys_are_well_separated():
    for name in ("three48", "three80", "pair80", "edges48"):
        c = SO.case(name)
        for f in range(c["n_frames"]):
            keys = sorted(SO.frame_camera(t["cams"][f - t["range"][0]], t["geom"][f - t["range"][0]])[1]
                          for t in c["tracks"] if t["range"][0] <= f < t["range"][1])
            for a, b in zip(keys, keys[1:]):
                assert b - a > 1e-3 * b


@pytest.mark.parametrize("name,mode,reverse", SO.ORACLE_CASES)
def test_seeded_cases_stay_under_the_ambiguity_cap(name, mode, reverse):
    """A condition on the cases: were 1 % or more of the raster ambiguous, the GPU comparison could hide a failure."""
    ref = SO.reference(name, mode, reverse)
    S2 = 2 * SO.case(name)["S"]
    for r in ref:
        assert r["ambiguous"].shape == (S2, S2) and r["ambiguous"].mean() < 0.01, r["ambiguous"].mean()
    assert any((r["owner"] >= 0).any() for r in ref)
