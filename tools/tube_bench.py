"""The tube augmentor in front of the feature extractor, measured:

  kernel   hmmr_tube_augment on 64 frames of 300x300 at S = 224: float32 / uint8 frames, with / without rotation.  Time per
           launch = device events around LAUNCHES back-to-back launches on frames that already lie on the device; GB/s =
           (the frames read once + the crops written) / that time -- the bytes the algorithm needs, not what the caches moved.
  new      FeatureExtractor.compute_all_phis_augmented on a uint8 tube of 256 frames of 300x300 (upload, augmentation,
           ResNet in batches of 64, download of the phis; the crops stay on the device), frames per second, wall clock
           around a synchronise.
  today    the parent's path in the same run: compute_all_phis fed with READY host float32 crops of the same tube (the
           augmentation already paid for elsewhere), frames per second.  This is the yardstick: the new path must not be
           slower than it by more than the yardstick's own spread (REPS repetitions, max - min).

The two paths alternate, REPS repetitions each after one warm-up each.  Prints lines and one JSON object; recorded, not gated.

    python tools/tube_bench.py [--frames 256] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from human_dynamics_amd import _lib as L  # noqa: E402
from human_dynamics_amd import assets  # noqa: E402
from human_dynamics_amd.datasets.resnet_extractor import FeatureExtractor  # noqa: E402
from human_dynamics_amd.util.tube_augmentation import TubePreprocessorDriver  # noqa: E402

LAUNCHES = 1000


def kernel_rows(dev, rng):
    n, H, W, S = 64, 300, 300, 224
    pre = TubePreprocessorDriver(rotate_max=0.4, delta_rotate_max=0.1, device=dev).preprocessor
    u8 = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    sizes = np.tile(np.array([[H, W]], np.int32), (n, 1))
    centers = np.tile(np.array([[W // 2, H // 2]], np.int32), (n, 1))
    walks = pre.draw_walks(n, np.random.default_rng(1))
    _, geom, rot = pre.host_side(sizes, np.zeros((n, 3, 25), np.float32), centers, np.zeros((n, 72), np.float32),
                                 np.zeros((n, 14, 3), np.float32), walks, True)
    frames = {"uint8": torch.from_numpy(u8).to(dev), "float32": torch.from_numpy(u8.astype(np.float32) / np.float32(255)).to(dev)}
    out = torch.empty((n, S, S, 3), dtype=torch.float32, device=dev)
    lib = L.load()
    rows = []
    for kind, fr in frames.items():
        for r in (None, rot):
            # the Python wrapper uploads its operands on every call: time the C entry point itself on operands that lie on the device
            g = torch.from_numpy(geom).to(dev)
            fl = torch.ones(n, dtype=torch.uint8, device=dev)
            rt = None if r is None else torch.from_numpy(r).to(dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            launch = lambda: L.check(lib.hmmr_tube_augment(fr.data_ptr(), int(kind == "uint8"), n, H, W, g.data_ptr(), fl.data_ptr(), L.ptr(rt), S,
                                                           out.data_ptr(), st), "hmmr_tube_augment")
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / LAUNCHES
            nbytes = fr.numel() * fr.element_size() + out.numel() * 4
            rows.append({"frames": kind, "rotation": r is not None, "us_per_launch": round(us, 2), "gb_per_s": round(nbytes / us / 1e3, 1),
                         "bytes": nbytes})
            print("kernel  %-7s frames, rotation %-5s %9.2f us / launch of 64 frames %8.1f GB/s" % (kind, r is not None, us, nbytes / us / 1e3),
                  flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tube_bench needs the GPU: there is nothing to measure without one")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "reps": a.reps, "kernel": kernel_rows(dev, rng)}

    T, H, W = a.frames, 300, 300
    fe = FeatureExtractor("synthetic:0", batch_size=64, weights=assets.make_synthetic_weights(0), device=dev)
    drv = TubePreprocessorDriver(device=dev)
    tube = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    sizes = np.tile(np.array([[H, W]], np.int32), (T, 1))
    labels = rng.uniform(0, 300, (T, 3, 25)).astype(np.float32)
    centers = np.tile(np.array([[W // 2, H // 2]], np.int32), (T, 1))
    poses, gt3ds = np.zeros((T, 72), np.float32), np.zeros((T, 14, 3), np.float32)
    walks = drv.preprocessor.draw_walks(T, np.random.default_rng(2))
    ready = drv(tube, sizes, labels, centers, poses, gt3ds, walks=walks, flip=False)["images"]        # host float32 crops

    def new():
        return fe.compute_all_phis_augmented(drv, tube, sizes, labels, centers, poses, gt3ds, walks=walks, flip=False, keep_images=False)["phis"]

    def today():
        return fe.compute_all_phis(ready)

    paths = (("today", today), ("new", new))
    outs = {}
    for name, run in paths:
        outs[name] = run()                                   # warm-up of every shape
    res["same_phis"] = bool(np.array_equal(outs["today"], outs["new"]))
    fps = {name: [] for name, _ in paths}
    for _ in range(a.reps):
        for name, run in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            fps[name].append(T / (time.perf_counter() - t0))
    for name, _ in paths:
        v = fps[name]
        res[name] = {"frames_per_s": [round(x, 1) for x in v], "min": round(min(v), 1), "max": round(max(v), 1), "mean": round(sum(v) / len(v), 1)}
        print("%-6s %s frames/s (mean %.1f, spread %.1f)" % (name, ["%.1f" % x for x in v], sum(v) / len(v), max(v) - min(v)), flush=True)
    spread = max(fps["today"]) - min(fps["today"])
    short = sum(fps["today"]) / a.reps - sum(fps["new"]) / a.reps
    res["yardstick_spread"] = round(spread, 1)
    res["new_minus_today_mean"] = round(-short, 1)
    res["verdict"] = "new path not slower than the yardstick" if short <= spread else "new path SLOWER than the yardstick by more than its spread"
    print("phis of the two paths identical: %s; %s (today - new = %.1f frames/s, allowed %.1f)" % (res["same_phis"], res["verdict"], short, spread))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
