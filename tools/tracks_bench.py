"""Every tracked person in one call, measured: one hmmr_predict_tracks call against the loop of one hmmr_predict_video call per
track, device crops in and device records out, for crowds of equal tracks:

    16 x 40, 8 x 100, 4 x 256 and 1 x 640 frames      (tracks x frames per track; the last row is the control: one track either way)

Both routes run on ONE stream with one workspace and one record buffer, on the Tester's packed model (synthetic weights).  Per shape:
two warm-up calls of each route, then REPS repetitions, the two routes alternating; every repetition is timed with a pair of device
events around the whole route (a route takes milliseconds, a pair of events about 10 us).  Reported per route: median, min and max of
the repetitions in ms, and frames per second at the median; per shape the ratio loop / one call at the medians and whether the two
record buffers hold the same bytes.

With a library that has no hmmr_predict_tracks (a build of the commit before it) only the loop is measured: that is how the loop's
time is taken from the parent commit, and the loop measured here beside the one call cross-checks that the shared workspace carve
changed nothing for hmmr_predict_video.  Recorded, not gated.

    python tools/tracks_bench.py [--dtype f16x3] [--reps 9] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from human_dynamics_amd import _lib as L  # noqa: E402
from human_dynamics_amd import assets  # noqa: E402

SHAPES = [(16, 40), (8, 100), (4, 256), (1, 640)]


class Config(object):
    def __init__(self):
        self.load_path, self.smpl_model_path = "synthetic:0", "synthetic:2"
        self.batch_size, self.sequence_length, self.pred_mode, self.num_conv_layers = 8, 20, "pred", 3
        self.delta_t_values, self.num_kps = ["-5", "5"], 25


def stats(ms, frames):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": round(med, 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3), "frames_per_s": round(frames / med * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16x3")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracks_bench needs the GPU: there is nothing to measure without one")
    dev = "cuda:0"
    if not hasattr(C.CDLL(L.LIB_PATH), "hmmr_predict_tracks"):        # a build of the parent commit: bind what it has, measure the loop
        for name in [k for k in L.SIGNATURES if "tracks" in k and not k.startswith("hmmr_track_")]:
            del L.SIGNATURES[name]
    lib = L.load()
    has_tracks = "hmmr_predict_tracks" in L.SIGNATURES
    from human_dynamics_amd.evaluation.tester import Tester
    t = Tester(Config(), weights=assets.make_synthetic_weights(0), smpl=assets.make_synthetic_smpl(2), dtype=a.dtype, device=dev)
    eng, model = t.engine, t.native_model()
    R = eng.iw.num_regressors
    offs, ld = (C.c_int32 * (R * 7))(), C.c_int64(0)
    L.check(lib.hmmr_record_layout(eng.num_kps, eng.num_verts, R, offs, C.byref(ld)), "hmmr_record_layout")
    rec_len = ld.value
    mf, mw = Tester.MAX_DEVICE_FRAMES, Tester.MAX_TAIL_WINDOWS
    n_max = max(k * n for k, n in SHAPES)
    gen = torch.Generator(device=dev).manual_seed(0)
    frames = (torch.rand((n_max, 224, 224, 3), generator=gen, device=dev) * 2 - 1).contiguous()       # crops as process_tracks leaves them: on the device
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "reps": a.reps, "max_frames": mf, "max_windows": mw,
           "has_predict_tracks": has_tracks, "shapes": []}
    print("%s, %s operands, %d repetitions per route, passes of %d frames / %d windows" % (res["device"], a.dtype, a.reps, mf, mw), flush=True)
    for n_tracks, per in SHAPES:
        n = n_tracks * per
        off = (np.arange(n_tracks + 1, dtype=np.int32) * per).astype(np.int32)
        off_p = off.ctypes.data_as(C.POINTER(C.c_int32))
        nbytes = lib.hmmr_predict_video_workspace_bytes(C.byref(model), per, mf, mw)
        if has_tracks:
            nbytes = max(nbytes, lib.hmmr_predict_tracks_workspace_bytes(C.byref(model), off_p, n_tracks, mf, mw))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rec = {k: torch.empty((n, rec_len), dtype=torch.float32, device=dev) for k in ("loop", "one_call")}

        def loop():
            for k in range(n_tracks):
                L.check(lib.hmmr_predict_video(C.byref(model), frames[k * per:].data_ptr(), per, rec["loop"][k * per:].data_ptr(), rec_len, offs, mf, mw,
                                               ws.data_ptr(), nbytes, stream), "hmmr_predict_video")

        def one_call():
            L.check(lib.hmmr_predict_tracks(C.byref(model), frames.data_ptr(), off_p, n_tracks, rec["one_call"].data_ptr(), rec_len, offs, mf, mw,
                                            ws.data_ptr(), nbytes, stream), "hmmr_predict_tracks")

        routes = [("loop", loop)] + ([("one_call", one_call)] if has_tracks else [])
        for _ in range(2):
            for _, run in routes:
                run()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in routes}
        for _ in range(a.reps):
            for name, run in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        row = {"tracks": n_tracks, "frames_per_track": per}
        for name, _ in routes:
            row[name] = stats(ms[name], n)
            print("%2d x %3d  %-8s median %8.3f ms  (min %8.3f, max %8.3f)  %8.1f frames/s" % (
                n_tracks, per, name, row[name]["median_ms"], row[name]["min_ms"], row[name]["max_ms"], row[name]["frames_per_s"]), flush=True)
        if has_tracks:
            row["same_bytes"] = bool(torch.equal(rec["loop"].view(torch.int32), rec["one_call"].view(torch.int32)))
            row["loop_over_one_call"] = round(row["loop"]["median_ms"] / row["one_call"]["median_ms"], 3)
            print("%2d x %3d  loop / one call = %.3f at the medians; same bytes: %s" % (n_tracks, per, row["loop_over_one_call"], row["same_bytes"]),
                  flush=True)
        res["shapes"].append(row)
        del ws, rec
    flags = C.c_uint(0)
    L.check(lib.hmmr_run_flags(C.byref(flags), 0), "hmmr_run_flags")
    res["run_flags"] = int(flags.value)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
