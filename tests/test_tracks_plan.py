"""The host side of the call over several tracks (include/hmmr_hip.h: hmmr_tracks_plan, hmmr_tracks_window_owner, hmmr_tracks_window_rows,
hmmr_tracks_tail_pass, hmmr_predict_tracks_workspace_bytes): the ragged plan against a NumPy restatement and against per-track
hmmr_video_plan, the index rule against the reference's recorded windows, the tail passes' tiling of the output rows, and every refusal --
no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import build
from tracks_rule import FOV, G, LENGTHS, MARGIN, T, offsets as _offsets, ragged_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = [(1024, 128), (8, 2), (1, 1)]
CASES = [(1, 8), (24, 2), (64, 8), (65, 8), (100, 3), (256, 8)]      # (N, B) of tests/golden/reference_windows.npz


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return L.load()


def _p(off):
    return off.ctypes.data_as(C.POINTER(C.c_int32))


def _plan(lib, off, T=T, fov=FOV, max_frames=1024, max_windows=128, n_tracks=None):
    p = L.TracksPlan()
    rc = lib.hmmr_tracks_plan(_p(off) if off is not None else None, len(off) - 1 if n_tracks is None else n_tracks, T, fov, max_frames, max_windows,
                              C.byref(p))
    return rc, p


@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_tracks_plan_equals_the_restatement_and_the_per_track_plans(lib, name):
    off = _offsets(LENGTHS[name])
    fed, owner, kept = ragged_rule(off)
    for max_frames, max_windows in PASSES:
        rc, p = _plan(lib, off, max_frames=max_frames, max_windows=max_windows)
        assert rc == 0, lib.hmmr_last_error()
        assert (p.n_tracks, p.T, p.fov, p.margin, p.g) == (len(off) - 1, T, FOV, MARGIN, G)
        assert p.n_frames == int(off[-1]) and p.n_windows == len(owner)
        assert (p.max_frames, p.max_windows) == (max_frames, max_windows)
        assert p.resnet_passes == -(-p.n_frames // max_frames) and p.tail_passes == -(-p.n_windows // max_windows)
        # the windows are the sum of what the one-video plan gives every track
        total = 0
        for k in range(len(off) - 1):
            v = L.VideoPlan()
            assert lib.hmmr_video_plan(int(off[k + 1] - off[k]), T, FOV, max_frames, max_windows, C.byref(v)) == 0
            total += v.n_windows
        assert total == p.n_windows
        # the tail passes tile [0, n_frames) in order, without gap or overlap, and hold the rows the rule keeps for their windows
        row = 0
        for i in range(p.tail_passes):
            w0, nw, o0, keep = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
            assert lib.hmmr_tracks_tail_pass(_p(off), len(off) - 1, C.byref(p), i, C.byref(w0), C.byref(nw), C.byref(o0), C.byref(keep)) == 0
            assert w0.value == i * max_windows and nw.value == min(max_windows, p.n_windows - w0.value)
            rows = [r for w in range(w0.value, w0.value + nw.value) for _, r in kept[w]]
            assert o0.value == row and keep.value == len(rows) >= nw.value and rows == list(range(row, row + len(rows)))
            row += keep.value
        assert row == p.n_frames
        for bad in (-1, p.tail_passes):
            assert lib.hmmr_tracks_tail_pass(_p(off), len(off) - 1, C.byref(p), bad, None, None, None, None) == -1
            assert b"hmmr_tracks_tail_pass" in lib.hmmr_last_error()
    # every global window has the owner the rule gives it; the window behind the last has none
    k, lw = C.c_int(-1), C.c_int(-1)
    for w, (wk, wl) in enumerate(owner):
        assert lib.hmmr_tracks_window_owner(_p(off), len(off) - 1, G, w, C.byref(k), C.byref(lw)) == 0 and (k.value, lw.value) == (wk, wl)
    assert lib.hmmr_tracks_window_owner(_p(off), len(off) - 1, G, len(owner), C.byref(k), C.byref(lw)) == -1
    assert b"beyond" in lib.hmmr_last_error()
    # any window range: the rows are those the rule keeps (ranges that start inside a track or span empty tracks included)
    o0, keep = C.c_int(-1), C.c_int(-1)
    for w0 in range(0, len(owner), 3):
        for nw in (1, 2, 5, len(owner) - w0):
            if w0 + nw > len(owner):
                continue
            rows = [r for w in range(w0, w0 + nw) for _, r in kept[w]]
            assert lib.hmmr_tracks_window_rows(_p(off), len(off) - 1, G, w0, nw, C.byref(o0), C.byref(keep)) == 0
            assert (o0.value, keep.value) == (rows[0], len(rows)) and rows == list(range(rows[0], rows[0] + len(rows)))
    assert lib.hmmr_tracks_window_rows(_p(off), len(off) - 1, G, 0, len(owner) + 1, C.byref(o0), C.byref(keep)) == -1
    assert lib.hmmr_tracks_window_rows(_p(off), len(off) - 1, G, 0, 0, C.byref(o0), C.byref(keep)) == -1


@pytest.mark.parametrize("N,B", CASES)
def test_ragged_rule_of_a_track_between_two_others_is_the_reference_s_windows(lib, N, B):
    """the rule restricted to one track reproduces what the reference fed and kept for a video of that length: pinned to the recorded
    windows, not to a restatement.  The owner / row helpers of the library say the same as the rule for this track's windows."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_windows.npz"))
    ref_fed, ref_kept = z["fed_n%d_b%d" % (N, B)], z["kept_n%d_b%d" % (N, B)]      # frame numbers from 1; -1 = the zero image
    off = _offsets([11, N, 5])
    fed, owner, kept = ragged_rule(off)
    mine = [w for w, (k, _) in enumerate(owner) if k == 1]
    nw = -(-N // G)
    assert len(mine) == nw and mine[0] == 2                        # 11 frames in front: two windows
    local = np.where(fed[mine] >= 0, fed[mine] - off[1] + 1, -1)
    assert np.array_equal(local, ref_fed[:nw])
    assert ((fed[mine] < 0) | ((fed[mine] >= off[1]) & (fed[mine] < off[2]))).all()          # never a neighbour's frame
    rows = np.array([r for w in mine for _, r in kept[w]])
    slots = np.array([local[i, s] for i, w in enumerate(mine) for s, _ in kept[w]])
    assert np.array_equal(rows - off[1] + 1, ref_kept) and np.array_equal(slots, ref_kept)
    o0, keep = C.c_int(-1), C.c_int(-1)
    assert lib.hmmr_tracks_window_rows(_p(off), 3, G, mine[0], nw, C.byref(o0), C.byref(keep)) == 0
    assert (o0.value, keep.value) == (11, N)
    rc, p = _plan(lib, off)
    assert rc == 0 and p.n_windows == 2 + nw + 1 and p.n_frames == 16 + N


def test_tracks_plan_refusals(lib):
    good = _offsets([3, 0, 9])

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc == -1 and b"hmmr_tracks_plan" in msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    refused(_plan(lib, None, n_tracks=3)[0], b"null track_offsets")
    refused(_plan(lib, None, n_tracks=0)[0], b"null track_offsets")
    refused(_plan(lib, good, n_tracks=-1)[0], b"n_tracks=-1")
    refused(_plan(lib, np.array([4, 7, 7, 16], np.int32))[0], b"track_offsets[0]=4", b"must be 0")
    refused(_plan(lib, np.array([0, 3, 2, 12], np.int32))[0], b"must not decrease", b"track_offsets[1]=3", b"track_offsets[2]=2")
    refused(_plan(lib, np.array([0, 5, 2 ** 31 - 1], np.int32))[0], b"32-bit row numbers")
    refused(_plan(lib, good, fov=12)[0], b"odd")
    refused(_plan(lib, good, fov=0)[0], b"odd")
    refused(_plan(lib, good, T=12)[0], b"keeps none")
    refused(_plan(lib, good, max_frames=0)[0], b"max_frames=0")
    refused(_plan(lib, good, max_windows=0)[0], b"max_windows=0")
    assert lib.hmmr_tracks_plan(_p(good), 3, T, FOV, 8, 2, None) == -1
    assert _plan(lib, good)[0] == 0 and _plan(lib, good, T=13)[0] == 0 and _plan(lib, np.array([0, 5, 2 ** 31 - 2], np.int32))[0] == 0
    # the helpers and the two copies check the offsets the same way, under their own names, before anything else (dummy pointers: no device)
    bad = np.array([0, 3, 2, 12], np.int32)
    k = C.c_int(0)
    assert lib.hmmr_tracks_window_owner(_p(bad), 3, G, 0, C.byref(k), None) == -1 and b"hmmr_tracks_window_owner: track_offsets must not" in lib.hmmr_last_error()
    assert lib.hmmr_tracks_window_owner(_p(good), 3, 0, 0, C.byref(k), None) == -1 and b"g=0" in lib.hmmr_last_error()
    assert lib.hmmr_tracks_window_owner(_p(good), 3, G, -1, C.byref(k), None) == -1


def test_ragged_copies_refuse_bad_arguments_before_any_launch(lib):
    """dummy, never dereferenced pointers: no device is needed"""
    P = [0x10000, 0x20000, 0x30000]
    good = _offsets([3, 0, 9])                                     # 1 + 0 + 2 windows
    gather = lambda phi=P[0], zero=P[1], off=good, nt=3, w0=0, nw=3, T=20, margin=6, g=8, c=2048, out=P[2]: \
        lib.hmmr_gather_windows_tracks(phi, zero, _p(off) if off is not None else None, nt, w0, nw, T, margin, g, c, out, None)
    keep = lambda strips=P[0], off=good, nt=3, w0=0, nw=3, T=20, margin=6, g=8, c=2048, out=P[2], ld=2048: \
        lib.hmmr_keep_rows_tracks(strips, _p(off) if off is not None else None, nt, w0, nw, T, margin, g, c, out, ld, None)
    shared = (dict(off=None), dict(off=np.array([0, 3, 2, 12], np.int32)), dict(off=np.array([1, 3, 3, 12], np.int32)), dict(nt=-1), dict(c=6), dict(c=0),
              dict(w0=-1), dict(nw=-1), dict(g=0), dict(margin=13), dict(T=0), dict(out=None), dict(out=P[2] + 8), dict(nw=4), dict(w0=3, nw=1),
              dict(w0=2, nw=2))
    for bad in shared + (dict(phi=None), dict(zero=None), dict(phi=P[0] + 4)):
        assert gather(**bad) == -1 and b"hmmr_gather_windows_tracks" in lib.hmmr_last_error(), bad
    for bad in shared + (dict(strips=None), dict(strips=P[0] + 4), dict(ld=2044), dict(ld=2050)):
        rc, msg = keep(**bad), lib.hmmr_last_error()
        assert rc == -1 and (b"hmmr_keep_rows_tracks" in msg or b"hmmr_tracks_window" in msg), (bad, msg)
    # nothing to do is not an error, and launches nothing
    assert gather(nw=0) == 0 and keep(nw=0) == 0 and gather(off=_offsets([]), nt=0, nw=0) == 0 and keep(off=_offsets([0, 0]), nt=2, nw=0) == 0


def _model(dtype=L.HMMR_F16X3):
    """a model of dummy, never dereferenced device pointers (as tests/test_video_plan.py): the queries read the host structs only"""
    rw, tw, iw, sc = L.ResnetWeights(), L.TemporalWeights(), L.IefWeights(), L.SmplConsts()
    rw.dtype = tw.dtype = iw.dtype = dtype
    rw.unit[0].c_in, rw.unit[15].depth = 64, 2048
    tw.num_blocks = 3
    iw.num_regressors, iw.num_stages = 3, 3
    iw.reg[0].nd, iw.reg[1].nd, iw.reg[2].nd = 85, 72, 72
    sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = 6890, 25, 4, 6912
    m = L.Model()
    m.resnet, m.temporal, m.ief, m.smpl = C.pointer(rw), C.pointer(tw), C.pointer(iw), C.pointer(sc)
    m.sequence_length, m.fov = 20, 13
    m._keep = (rw, tw, iw, sc)
    return m


def test_tracks_workspace_query_needs_no_gpu(lib):
    m = _model()
    q = lambda lengths, mf=1024, mw=128: lib.hmmr_predict_tracks_workspace_bytes(C.byref(m), _p(_offsets(lengths)), len(lengths), mf, mw)
    one = lambda n, mf=1024, mw=128: lib.hmmr_predict_video_workspace_bytes(C.byref(m), n, mf, mw)
    # one track: the one-video call's workspace, whatever the pass sizes (the shared carve)
    for n in (1, 9, 24, 100):
        for mf, mw in PASSES:
            assert q([n], mf, mw) == one(n, mf, mw) > 0
    assert q([]) == q([0, 0]) == one(0) > 0
    # several tracks: phi of all frames, the ResNet workspace of all of them in one pass, the tail's buffers for every window
    mixed = LENGTHS["mixed"]
    n, nw = sum(mixed), sum(-(-x // G) for x in mixed)
    assert q(mixed) >= (n + 1) * 2048 * 4 + lib.hmmr_resnet50_workspace_bytes(n + 1, L.HMMR_F16X3)
    assert q(mixed) >= (n + 1) * 2048 * 4 + 2 * nw * 20 * 2048 * 4 + lib.hmmr_ief_workspace_bytes(n, 3, L.HMMR_F16X3) + lib.hmmr_smpl_workspace_bytes(3 * n)
    assert q(mixed, 8, 2) < q(mixed)
    # refusals give 0 and a message
    assert lib.hmmr_predict_tracks_workspace_bytes(C.byref(m), None, 2, 1024, 128) == 0 and b"null track_offsets" in lib.hmmr_last_error()
    bad = np.array([0, 3, 2], np.int32)
    assert lib.hmmr_predict_tracks_workspace_bytes(C.byref(m), _p(bad), 2, 1024, 128) == 0 and b"must not decrease" in lib.hmmr_last_error()
    assert q(mixed, 0, 2) == 0 and q(mixed, 8, 0) == 0 and lib.hmmr_predict_tracks_workspace_bytes(None, _p(bad), 2, 8, 2) == 0
    m.fov = 12
    assert q(mixed) == 0 and b"odd" in lib.hmmr_last_error()


def test_predict_tracks_program_compiles_against_the_header(lib, tmp_path):
    """no GPU: the Python-free program for several tracks compiles (hipcc, host code only) and links against libhmmr_hip.so"""
    pkg = os.path.join(ROOT, "human_dynamics_amd")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-x", "hip", os.path.join(ROOT, "tests", "c_abi", "predict_tracks.c"),
                        "-I", os.path.join(ROOT, "include"), "-L", pkg, "-lhmmr_hip", "-Wl,-rpath," + pkg, "-o", str(tmp_path / "predict_tracks")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
