"""Workspaces are caller-owned, and a stage's layout is stated once (csrc/workspace.h): every *_workspace_bytes query against
an independent NumPy restatement of its layout, to the byte; every entry point that carves a workspace refuses one byte too few before
anything is queued (dummy pointers, no GPU); and the carver alone, as a program of its own."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import build

from test_video_plan import _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [L.HMMR_F32, L.HMMR_BF16, L.HMMR_F16X3]
SIZES = np.array([1, 2, 3, 5, 7, 8, 20, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, 255, 256, 257, 300, 1000], dtype=np.int64)
P = [0x10000 * (i + 1) for i in range(8)]                        # dummy device pointers, 256-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return L.load()


# ---- the layouts, restated: every buffer starts on a multiple of 256 bytes, so a layout is the sum of its rounded sizes
def r256(x):
    return (np.asarray(x, dtype=np.int64) + 255) // 256 * 256


def esize(dt):
    return 2 if dt == L.HMMR_BF16 else 4


def splitk(m, cout, k):
    return k * m * ((cout + 127) // 128 * 128) * 4               # k fp32 partial planes [m][cout rounded to 128]


def temporal(b, t, dt):
    m = b * t                                                    # h (operand dtype), h1 and two trunk buffers (fp32), 5 split-K planes
    return r256(m * 2048 * esize(dt)) + 3 * r256(m * 2048 * 4) + r256(splitk(m, 2048, 5))


def hallucinator(m, dt):
    return 3 * r256(m * 2048 * esize(dt)) + r256(splitk(m, 2048, 5))


def ief(m, regressors, dt):
    g = max(regressors - 1, 1)                                   # one set of buffers per delta regressor, each set's members rounded
    return (r256(m * 2048 * esize(dt)) + 3 * r256(g * r256(m * 1024 * esize(dt))) + 2 * r256(g * r256(m * 128 * 4)) +
            r256(g * splitk(m, 1024, 4)))


def resnet_stem(n, dt):
    return r256(n * 230 * 232 * 4 * esize(dt)) + r256(n * 112 * 112 * 64 * esize(dt))       # the padded RGBX image, the 7x7 conv map


def resnet(n, dt):
    return resnet_stem(n, dt) + 4 * r256(n * 56 * 56 * 256 * esize(dt)) + 2 * r256(n * 56 * 56 * 64 * esize(dt))


def smpl(m):
    mp = (m + 31) // 32 * 32                                     # whole groups of IBM = 32 instances
    return r256(mp * 224 * 4) + r256(mp * 24 * 12 * 4)


def raster_slab(ch, nv, nf):
    return r256(ch * nv * 16) + r256(ch * 16) + r256(ch * nf * 8) + r256(ch * nf * 48) + r256(ch * nf * 16)


def render(n, nv, nf):
    return raster_slab(np.minimum(n, 64), nv, nf)


def scene(n_frames, n_tracks, nv, nf):
    return raster_slab(np.minimum(n_frames, max(64 // n_tracks, 1)) * n_tracks, nv, nf)


def predict_video(n, mf, mw, dt, hal, T=20, g=8, R=3):
    n = max(n, 1)                                                # (an empty video reports what one frame takes)
    nw = min(-(-n // g), mw)                                     # the first tail pass is the largest: windows, and the rows it keeps
    keep = min(nw * g, n)
    movie = hallucinator(nw * T, dt) if hal else temporal(nw, T, dt)
    tail = (2 * r256(nw * T * 2048 * 4) + r256(keep * 2048 * 4) + r256(R * keep * 85 * 4) + r256(movie) + r256(ief(keep, R, dt)) +
            r256(smpl(R * keep)))
    return r256((n + 1) * 2048 * 4) + max(tail, r256(resnet(min(n, mf) + 1, dt)))


def test_stage_queries_equal_the_restated_layouts(lib):
    for dt in DTYPES:
        for n in SIZES:
            n = int(n)
            assert lib.hmmr_resnet50_workspace_bytes(n, dt) == resnet(n, dt), (n, dt)
            assert lib.hmmr_hallucinator_workspace_bytes(n, dt) == hallucinator(n, dt), (n, dt)
            for t in (1, 13, 20):
                assert lib.hmmr_temporal_workspace_bytes(n, t, dt) == temporal(n, t, dt), (n, t, dt)
            for r in range(1, 9):
                assert lib.hmmr_ief_workspace_bytes(n, r, dt) == ief(n, r, dt), (n, r, dt)
        for args in ((0, dt), (-1, dt)):
            assert lib.hmmr_resnet50_workspace_bytes(*args) == 0 and lib.hmmr_hallucinator_workspace_bytes(*args) == 0
            assert lib.hmmr_temporal_workspace_bytes(args[0], 20, dt) == 0 and lib.hmmr_temporal_workspace_bytes(8, args[0], dt) == 0
            assert lib.hmmr_ief_workspace_bytes(args[0], 3, dt) == 0
    for m in range(1, 200):
        assert lib.hmmr_smpl_workspace_bytes(m) == smpl(m), m
    assert lib.hmmr_smpl_workspace_bytes(0) == 0 and lib.hmmr_smpl_workspace_bytes(-3) == 0
    assert smpl(32) < smpl(33) == smpl(64) < smpl(65)            # (the restatement steps where the groups do)


def test_stem_query_is_the_front_of_the_resnet_layout_on_the_unfused_route_and_zero_on_the_fused(lib):
    try:
        for route in (0, 1, 2):                                  # hmmr_debug_t.stem_route: by dtype (fp32 unfused), unfused, fused
            dbg = L.Debug()
            dbg.stem_route = route
            lib.hmmr_set_debug(C.byref(dbg))
            for dt in DTYPES:
                rw = L.ResnetWeights()
                rw.dtype = dt
                unfused = route == 1 or (route == 0 and dt == L.HMMR_F32)
                for n in (1, 2, 3, 21, 65):
                    assert lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), n) == (resnet_stem(n, dt) if unfused else 0), (route, dt, n)
                assert lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), 0) == 0
    finally:
        lib.hmmr_set_debug(C.byref(L.Debug()))


def test_rasteriser_queries_are_one_slab_of_at_most_64_instances(lib):
    for nv, nf in ((3, 1), (10, 8), (6890, 13776)):
        for n in list(range(1, 70)) + [128, 4096]:
            assert lib.hmmr_render_workspace_bytes(n, nv, nf) == render(n, nv, nf), (n, nv, nf)
        for k in (1, 2, 3, 5, 16):
            for n in list(range(1, 70)) + [4096]:
                assert lib.hmmr_render_scene_workspace_bytes(n, k, nv, nf) == scene(n, k, nv, nf), (n, k, nv, nf)
    assert render(64, 10, 8) == render(65, 10, 8) > render(63, 10, 8) and scene(21, 3, 10, 8) == scene(22, 3, 10, 8) > scene(20, 3, 10, 8)
    assert lib.hmmr_render_workspace_bytes(0, 10, 8) == 0 and lib.hmmr_render_workspace_bytes(4097, 10, 8) == 0
    assert lib.hmmr_render_scene_workspace_bytes(8, 0, 10, 8) == 0 and lib.hmmr_render_scene_workspace_bytes(8, 17, 10, 8) == 0


def test_track_query_is_eighty_bytes_per_row(lib):
    for n in [0, 1, 2, 7, 255, 256, 257, 1000, L.TRACK_MAX_ROWS]:
        for k in (1, 5):
            assert lib.hmmr_track_workspace_bytes(n, k) == 80 * max(n, 1), (n, k)
    assert lib.hmmr_track_workspace_bytes(-1, 1) == 0 and lib.hmmr_track_workspace_bytes(L.TRACK_MAX_ROWS + 1, 1) == 0
    assert lib.hmmr_track_workspace_bytes(7, 0) == 0


@pytest.mark.parametrize("hal", [False, True])
def test_whole_video_query_is_phi_plus_the_larger_of_the_tail_and_the_resnet(lib, hal):
    for dt in DTYPES:
        m = _model(dtype=dt, hal=hal)
        for mf, mw in ((1024, 128), (8, 2), (1, 1)):
            for n in (0, 1, 7, 8, 9, 16, 17, 24, 100, 257):
                want = predict_video(n, mf, mw, dt, hal)
                assert lib.hmmr_predict_video_workspace_bytes(C.byref(m), n, mf, mw) == want, (dt, mf, mw, n)
                off = (C.c_int32 * 2)(0, n)
                assert lib.hmmr_predict_tracks_workspace_bytes(C.byref(m), off, 1, mf, mw) == want, (dt, mf, mw, n)


# ---- one byte too few is refused by name, with dummy pointers: the refusal precedes every launch
def _refused(lib, rc):
    assert rc == -1 and b"workspace" in lib.hmmr_last_error(), (rc, lib.hmmr_last_error())


@pytest.mark.parametrize("dt", DTYPES)
def test_f_movie_and_ief_refuse_a_workspace_one_byte_short(lib, dt):
    tw, hw, iw = L.TemporalWeights(), L.HallucinatorWeights(), L.IefWeights()
    tw.dtype = hw.dtype = iw.dtype = dt
    tw.num_blocks = 3
    iw.num_regressors, iw.num_stages = 3, 3
    iw.reg[0].nd, iw.reg[1].nd, iw.reg[2].nd = 85, 72, 72
    for b in (1, 2):
        need = lib.hmmr_temporal_workspace_bytes(b, 20, dt)
        _refused(lib, lib.hmmr_temporal_fwd(C.byref(tw), P[0], b, 20, P[1], P[2], need - 1, None))
    need = lib.hmmr_hallucinator_workspace_bytes(3, dt)
    _refused(lib, lib.hmmr_hallucinator_fwd(C.byref(hw), P[0], 3, P[1], P[2], need - 1, None))
    for r in (1, 3):
        iw.num_regressors = r
        need = lib.hmmr_ief_workspace_bytes(3, r, dt)
        _refused(lib, lib.hmmr_ief_fwd(C.byref(iw), P[0], 3, P[1], P[2], need - 1, None))


def test_smpl_refuses_a_workspace_one_byte_short(lib):
    sc = L.SmplConsts()
    sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = 100, 25, 4, 128
    for m in (5, 33):
        need = lib.hmmr_smpl_workspace_bytes(m)
        _refused(lib, lib.hmmr_smpl_fwd(C.byref(sc), P[0], 72, P[1], 10, P[2], 3, m, P[3], P[4], P[5], P[6], P[7], need - 1, None))


def test_rasteriser_refuses_a_workspace_one_byte_short(lib):
    nv, nf, size = 10, 8, 16
    for n in (1, 65):
        d = L.RenderDesc()
        d.verts, d.ld_verts, d.cams, d.ld_cam, d.faces, d.rgb, d.ws = P[0], 3 * nv, P[1], 3, P[2], P[3], P[4]
        d.n, d.nv, d.nf, d.size, d.out_h, d.out_w, d.bg_mode = n, nv, nf, size, size, size, L.RENDER_BG_COLOR
        d.ws_bytes = lib.hmmr_render_workspace_bytes(n, nv, nf) - 1
        _refused(lib, lib.hmmr_render_mesh(C.byref(d), None))
    tracks = (L.SceneTrack * 3)()
    for k in range(3):
        tracks[k].verts, tracks[k].ld_verts, tracks[k].cams, tracks[k].ld_cam, tracks[k].start, tracks[k].end = P[0], 3 * nv, P[1], 3, 0, 23
    s = L.SceneDesc()
    s.tracks, s.n_tracks, s.faces, s.nv, s.nf, s.n_frames, s.size, s.out_h, s.out_w = tracks, 3, P[2], nv, nf, 23, size, size, size
    s.bg_mode, s.rgb, s.ws = L.RENDER_BG_COLOR, P[3], P[4]
    s.ws_bytes = lib.hmmr_render_scene_workspace_bytes(23, 3, nv, nf) - 1
    _refused(lib, lib.hmmr_render_scene(C.byref(s), None))


def test_track_front_end_refuses_a_workspace_one_byte_short(lib):
    off = (C.c_int32 * 3)(0, 7, 7)                               # two tracks of 7 and 0 rows
    gauss = (C.c_double * 3)(0.5, 0.2, 0.05)
    need = lib.hmmr_track_workspace_bytes(7, 2)
    _refused(lib, lib.hmmr_track_bbox(P[0], P[1], off, 2, 25, 0.1, 5, gauss, 2, P[2], P[3], P[4], P[5], need - 1, None))
    assert b"hmmr_track_bbox" in lib.hmmr_last_error()
    _refused(lib, lib.hmmr_track_smooth(P[0], off, 2, 5, gauss, 2, P[1], P[2], need - 1, None))
    assert b"hmmr_track_smooth" in lib.hmmr_last_error()


@pytest.mark.parametrize("dt", DTYPES)
def test_resnet_and_the_whole_video_call_refuse_a_workspace_one_byte_short(lib, dt):
    m = _model(dtype=dt)
    need = lib.hmmr_resnet50_workspace_bytes(1, dt)
    _refused(lib, lib.hmmr_resnet50_fwd(m.resnet, P[0], 1, 0, P[1], P[2], need - 1, None, None))
    offs, ld = (C.c_int32 * 21)(), C.c_int64(0)
    assert lib.hmmr_record_layout(25, 6890, 3, offs, C.byref(ld)) == 0
    for hal in (False, True):
        m = _model(dtype=dt, hal=hal)
        need = lib.hmmr_predict_video_workspace_bytes(C.byref(m), 9, 4, 1)
        _refused(lib, lib.hmmr_predict_video(C.byref(m), P[0], 9, P[1], ld.value, offs, 4, 1, P[2], need - 1, None))


def test_the_carver_alone(tmp_path):
    """csrc/workspace.h with a main of its own: aligned, monotone, non-overlapping offsets and total() = the last end, over the stages'
    grids, mixed alignments and zero-byte takes (tests/c_abi/workspace_carver.cpp)"""
    cxx = shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path / "workspace_carver")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", build.CSRC, os.path.join(ROOT, "tests", "c_abi", "workspace_carver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
