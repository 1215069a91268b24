"""Every *_workspace_bytes export of two builds of the library side by side, on the CPU: no kernel runs, so both can be loaded.

    python tools/workspace_sizes.py OTHER_LIB [THIS_LIB]      (THIS_LIB defaults to the in-tree build)

Grids: ResNet, temporal, hallucinator, IEF over three dtypes and sizes 0, negative, 1..300 and a few large ones (1..8 regressors
for IEF); SMPL around the multiples of 32; the rasteriser and the scene view around their slab boundary at 64 instances, with 1, 2,
3, 5, 16 and 17 tracks; the track front end from 0 rows; the stem query on both routes; the whole-video and the all-tracks query on
the dummy model of tests/test_video_plan.py, both f_movie forms, three pass sizes, n = 0..300.  Prints the number of points and how
many differ; exit status 1 if any does."""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from human_dynamics_amd import _lib as L  # noqa: E402

SIZES = [0, -1, -7] + list(range(1, 301)) + [1000, 4096, 4097, 100000]
DTYPES = [L.HMMR_F32, L.HMMR_BF16, L.HMMR_F16X3]
PASSES = [(1024, 128), (8, 2), (1, 1)]


def bind(path):
    import torch  # noqa: F401  (the HIP runtime the library links against, as in _lib.load)
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in L.SIGNATURES.items():
        if name.endswith("workspace_bytes") or name in ("hmmr_set_debug", "hmmr_abi_version"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def points():
    """(label, function name, arguments as a callable of the library) for every point of the grids"""
    from test_video_plan import _model
    for n, dt in itertools.product(SIZES, DTYPES):
        yield "resnet", lambda lib, n=n, dt=dt: lib.hmmr_resnet50_workspace_bytes(n, dt)
        yield "hallucinator", lambda lib, n=n, dt=dt: lib.hmmr_hallucinator_workspace_bytes(n, dt)
        for t in (0, -1, 1, 13, 20):
            yield "temporal", lambda lib, n=n, t=t, dt=dt: lib.hmmr_temporal_workspace_bytes(n, t, dt)
        for r in range(0, 10):
            yield "ief", lambda lib, n=n, r=r, dt=dt: lib.hmmr_ief_workspace_bytes(n, r, dt)
    for m in SIZES:
        yield "smpl", lambda lib, m=m: lib.hmmr_smpl_workspace_bytes(m)
    for n, nv, nf in itertools.product([0, -1] + list(range(1, 131)) + [4096, 4097], (0, 3, 10, 6890), (0, 1, 8, 13776, 65536, 65537)):
        yield "render", lambda lib, n=n, nv=nv, nf=nf: lib.hmmr_render_workspace_bytes(n, nv, nf)
    for k, n, (nv, nf) in itertools.product((0, 1, 2, 3, 5, 16, 17), [0, -1] + list(range(1, 71)) + [4096, 4097], ((10, 8), (6890, 13776), (0, 8), (10, 0))):
        yield "scene", lambda lib, k=k, n=n, nv=nv, nf=nf: lib.hmmr_render_scene_workspace_bytes(n, k, nv, nf)
    for n, k in itertools.product(SIZES + [1 << 27, (1 << 27) + 1], (0, 1, 5)):
        yield "track", lambda lib, n=n, k=k: lib.hmmr_track_workspace_bytes(n, k)
    for route, dt, n in itertools.product((0, 1, 2), DTYPES + [7], SIZES):           # hmmr_debug_t.stem_route: default, unfused, fused
        def stem(lib, route=route, dt=dt, n=n):
            dbg, rw = L.Debug(), L.ResnetWeights()
            dbg.stem_route, rw.dtype = route, dt
            lib.hmmr_set_debug(C.byref(dbg))
            got = lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), n)
            lib.hmmr_set_debug(C.byref(L.Debug()))
            return got
        yield "stem", stem
    for hal, dt, (mf, mw) in itertools.product((False, True), DTYPES, PASSES):
        m = _model(dtype=dt, hal=hal)
        for n in range(0, 301):
            yield "predict_video", lambda lib, m=m, n=n, mf=mf, mw=mw: lib.hmmr_predict_video_workspace_bytes(C.byref(m), n, mf, mw)
            off = (C.c_int32 * 4)(0, n // 3, n // 3, n)                                   # three tracks, the middle one empty
            yield "predict_tracks", lambda lib, m=m, off=off, mf=mf, mw=mw: lib.hmmr_predict_tracks_workspace_bytes(C.byref(m), off, 3, mf, mw)


def main():
    other = bind(sys.argv[1])
    this = bind(sys.argv[2] if len(sys.argv) > 2 else L.LIB_PATH)
    assert other._handle != this._handle, "the two paths name one library"
    count, differ, zero = {}, {}, {}
    for label, f in points():
        a, b = f(other), f(this)
        count[label] = count.get(label, 0) + 1
        differ[label] = differ.get(label, 0) + (a != b)
        zero[label] = zero.get(label, 0) + (b == 0)
    for label in count:
        print("%-15s %6d points, %d differ (%d of them report 0: refused arguments)" % (label, count[label], differ[label], zero[label]))
    print("all *_workspace_bytes exports, %s against %s: %d points, %d differ" % (sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "this tree",
                                                                                sum(count.values()), sum(differ.values())))
    return 1 if sum(differ.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
