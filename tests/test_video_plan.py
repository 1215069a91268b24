"""The host side of the whole-video call (include/hmmr_hip.h: hmmr_video_plan, hmmr_record_layout, hmmr_predict_video_workspace_bytes):
the sliding-window plan against the reference's recorded windows, the record layout against dist.record_layout, the workspace query and
the refusals -- no GPU -- and tests/c_abi/predict_video.c compiles and links against the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import build, dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 8), (24, 2), (64, 8), (65, 8), (100, 3), (256, 8)]      # (N, B) of tests/golden/reference_windows.npz: T = 20, fov = 13
PASSES = [(1024, 128), (8, 2), (1, 1)]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return L.load()


@pytest.fixture(scope="module")
def windows():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_windows.npz")))


def _plan(lib, n, T=20, fov=13, max_frames=1024, max_windows=128):
    p = L.VideoPlan()
    rc = lib.hmmr_video_plan(n, T, fov, max_frames, max_windows, C.byref(p))
    return rc, p


@pytest.mark.parametrize("N,B", CASES)
def test_video_plan_reproduces_the_reference_windows(lib, windows, N, B):
    fed, kept = windows["fed_n%d_b%d" % (N, B)], windows["kept_n%d_b%d" % (N, B)]
    for max_frames, max_windows in PASSES:
        rc, p = _plan(lib, N, max_frames=max_frames, max_windows=max_windows)
        assert rc == 0
        assert (p.n, p.T, p.fov, p.margin, p.g) == (N, 20, 13, 6, 8)
        assert p.n_windows == -(-N // 8) <= fed.shape[0]
        assert (p.max_frames, p.max_windows) == (max_frames, max_windows)
        assert p.resnet_passes == -(-N // max_frames) and p.tail_passes == -(-p.n_windows // max_windows)
    # the header's index rule gives every slot the reference fed (frame numbers from 1, -1 = the zero image) ...
    w, t = np.meshgrid(np.arange(fed.shape[0]), np.arange(20), indexing="ij")
    f = w * p.g + t - p.margin
    assert np.array_equal(np.where((f >= 0) & (f < N), f + 1, -1), fed)
    # ... the kept slots of the first n_windows windows are frames 1 .. N in order, and the windows beyond keep none
    centre = (f + 1)[:, p.margin:p.margin + p.g]
    assert np.array_equal(centre[:p.n_windows].reshape(-1)[:N], kept) and np.array_equal(kept, np.arange(1, N + 1))
    assert (centre[p.n_windows:] > N).all()


def test_video_plan_of_an_empty_video_has_no_pass(lib):
    rc, p = _plan(lib, 0)
    assert rc == 0 and (p.n_windows, p.resnet_passes, p.tail_passes) == (0, 0, 0)


@pytest.mark.parametrize("kw,word", [(dict(T=10, fov=13), b"keeps none"), (dict(fov=12), b"odd"), (dict(fov=0), b"odd"), (dict(fov=-1), b"odd"),
                                     (dict(T=12, fov=13), b"keeps none"), (dict(n=-1), b"n=-1"), (dict(max_frames=0), b"max_frames=0"),
                                     (dict(max_windows=0), b"max_windows=0")])
def test_video_plan_refusals(lib, kw, word):
    args = dict(n=24)
    args.update(kw)
    rc, _ = _plan(lib, **args)
    assert rc == -1 and word in lib.hmmr_last_error()
    assert lib.hmmr_video_plan(24, 20, 13, 8, 2, None) == -1
    assert _plan(lib, 24, T=13, fov=13)[0] == 0                  # g = 1 is the smallest window that keeps a frame


@pytest.mark.parametrize("K,V,D", [(25, 6890, 2), (14, 6890, 0), (25, 100, 1)])
def test_record_layout_equals_the_python_layout(lib, K, V, D):
    fields = (("cams", (3,)), ("joints", (K, 3)), ("kps", (K, 2)), ("poses", (24, 3, 3)), ("shapes", (10,)), ("verts", (V, 3)), ("omegas", (85,)))
    layout, rec_len = dist.record_layout(D, fields)
    off = {k: (o, sz) for k, shp, o, sz in layout}
    want = [[off[k][0] for k, _ in fields]]
    for d in range(D):                                           # (Tester.records_from_omegas)
        want.append([off[k + "_delta"][0] + d * (off[k + "_delta"][1] // D) for k, _ in fields])
    got, ld = (C.c_int32 * ((D + 1) * 7))(), C.c_int64(0)
    assert lib.hmmr_record_layout(K, V, D + 1, got, C.byref(ld)) == 0
    assert ld.value == rec_len and [list(got[r * 7:r * 7 + 7]) for r in range(D + 1)] == want
    assert lib.hmmr_record_layout(K, V, D + 1, None, C.byref(ld)) == 0 and ld.value == rec_len
    for bad in ((0, V, D + 1), (K, 0, D + 1), (K, V, 0), (K, V, L.MAX_REGRESSORS + 1)):
        assert lib.hmmr_record_layout(*bad, got, C.byref(ld)) == -1 and b"hmmr_record_layout" in lib.hmmr_last_error()
    assert lib.hmmr_record_layout(K, V, D + 1, None, None) == -1


def _model(dtype=L.HMMR_F16X3, hal=False):
    """a model of dummy, never dereferenced device pointers: the query and the refusals read the host structs only"""
    rw, tw, hw, iw, sc = L.ResnetWeights(), L.TemporalWeights(), L.HallucinatorWeights(), L.IefWeights(), L.SmplConsts()
    rw.dtype = tw.dtype = hw.dtype = iw.dtype = dtype
    rw.unit[0].c_in, rw.unit[15].depth = 64, 2048
    tw.num_blocks = 3
    iw.num_regressors, iw.num_stages = 3, 3
    iw.reg[0].nd, iw.reg[1].nd, iw.reg[2].nd = 85, 72, 72
    sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = 6890, 25, 4, 6912
    m = L.Model()
    m.resnet, m.ief, m.smpl = C.pointer(rw), C.pointer(iw), C.pointer(sc)
    if hal:
        m.hallucinator = C.pointer(hw)
    else:
        m.temporal = C.pointer(tw)
    m.sequence_length, m.fov = 20, 13
    m._keep = (rw, tw, hw, iw, sc)
    return m


@pytest.mark.parametrize("hal", [False, True])
def test_workspace_query_needs_no_gpu_and_never_shrinks(lib, hal):
    m = _model(hal=hal)
    q = lambda n, mf=1024, mw=128: lib.hmmr_predict_video_workspace_bytes(C.byref(m), n, mf, mw)
    sizes = [q(n) for n in range(0, 300)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    # phi [n + 1][2048], the ResNet workspace of n + 1 frames and the tail's buffers all fit
    assert sizes[24] >= 25 * 2048 * 4 + lib.hmmr_resnet50_workspace_bytes(25, L.HMMR_F16X3)
    assert sizes[24] >= 25 * 2048 * 4 + 2 * 3 * 20 * 2048 * 4 + lib.hmmr_ief_workspace_bytes(24, 3, L.HMMR_F16X3) + lib.hmmr_smpl_workspace_bytes(72)
    # bounded passes bound the workspace: past max_frames only phi grows
    small = [q(n, 8, 2) for n in (24, 100, 1000)]
    assert small[0] < sizes[24] and small[2] - small[1] == 900 * 2048 * 4
    assert all(b >= a for a, b in zip(small, small[1:]))


def test_workspace_query_returns_zero_for_a_bad_model(lib):
    q = lambda m, n=24, mf=1024, mw=128: lib.hmmr_predict_video_workspace_bytes(C.byref(m) if m is not None else None, n, mf, mw)
    assert q(None) == 0
    m = _model()
    m.hallucinator = C.pointer(m._keep[2])                       # both f_movie forms
    assert q(m) == 0 and b"exactly one" in lib.hmmr_last_error()
    m = _model()
    m.temporal = None                                            # neither
    assert q(m) == 0 and b"exactly one" in lib.hmmr_last_error()
    m = _model()
    m.ief = None
    assert q(m) == 0
    m = _model()
    m.fov = 12
    assert q(m) == 0 and b"odd" in lib.hmmr_last_error()
    m = _model()
    m._keep[3].reg[1].nd = 75                                    # a 75-wide delta regressor without no_optcam
    assert q(m) == 0 and b"regressor 1" in lib.hmmr_last_error()
    m = _model()
    assert q(m, n=-1) == 0 and q(m, mf=0) == 0 and q(m, mw=0) == 0 and q(m) > 0


def test_copies_refuse_bad_arguments_before_any_launch(lib):
    """dummy, never dereferenced pointers: no device is needed"""
    P = [0x10000, 0x20000, 0x30000]
    gather = lambda phi=P[0], n=24, zero=P[1], w0=0, nw=3, T=20, margin=6, g=8, c=2048, out=P[2]: \
        lib.hmmr_gather_windows(phi, n, zero, w0, nw, T, margin, g, c, out, None)
    keep = lambda strips=P[0], w0=0, nw=3, T=20, margin=6, g=8, c=2048, n_total=24, out=P[2], ld=2048: \
        lib.hmmr_keep_rows(strips, w0, nw, T, margin, g, c, n_total, out, ld, None)
    for bad in (dict(c=6), dict(c=0), dict(n=-1), dict(w0=-1), dict(nw=-1), dict(g=0), dict(margin=13), dict(T=0), dict(phi=None), dict(zero=None),
                dict(out=None), dict(phi=P[0] + 4), dict(out=P[2] + 8)):
        assert gather(**bad) == -1 and b"hmmr_gather_windows" in lib.hmmr_last_error(), bad
    for bad in (dict(c=6), dict(ld=2044), dict(ld=2050), dict(n_total=-1), dict(w0=-1), dict(nw=-1), dict(g=0), dict(margin=13), dict(strips=None),
                dict(out=None), dict(strips=P[0] + 4)):
        assert keep(**bad) == -1 and b"hmmr_keep_rows" in lib.hmmr_last_error(), bad
    # nothing to do is not an error, and launches nothing
    assert gather(n=0) == 0 and gather(nw=0) == 0 and keep(n_total=0) == 0 and keep(nw=0) == 0 and keep(w0=3, n_total=24) == 0


def test_predict_video_program_compiles_against_the_header(lib, tmp_path):
    """no GPU: the Python-free whole-video program compiles (hipcc, host code only) and links against libhmmr_hip.so"""
    pkg = os.path.join(ROOT, "human_dynamics_amd")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-x", "hip", os.path.join(ROOT, "tests", "c_abi", "predict_video.c"),
                        "-I", os.path.join(ROOT, "include"), "-L", pkg, "-lhmmr_hip", "-Wl,-rpath," + pkg, "-o", str(tmp_path / "predict_video")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
