"""Wall time of the track front end for several person tracks of one video, two ways (evaluation/run_video.py):

  process_tracks   keypoints -> smoothed boxes -> crop integers -> crops on the device, one download of the info at the end;
  host_smoothing   what a caller did before: the smoothing on the host per track, then process_images per track, which derives
                   the crop integers in a Python loop and uploads them.  --host-smoother scipy (the default where SciPy can be
                   imported) filters with scipy.signal.medfilt and scipy.ndimage.gaussian_filter1d, as the reference does;
                   numpy uses the restatement of tests/track_oracle.py, whose per-row np.sort median is slower than SciPy's.
                   The boxes and the gap filling are the restatement's in both.  The JSON names the smoother that was timed.

The uint8 frames are on the device before the clock starts.  Warm; events around the whole call, the info download included.
Reports both times and the bytes each moves over PCIe, counted where the copies are made (Tensor.to / Tensor.cpu /
torch.tensor(...).to wrapped for one call of each leg).  Prints one JSON object; `--out FILE` also writes it.  Recorded, not gated.

    python tools/track_bench.py [--tracks 8] [--frames 1000] [--height 720] [--width 1280] [--out profiles/track_bench.json]
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import track_oracle as TO  # noqa: E402
from human_dynamics_amd.evaluation.run_video import process_images, process_tracks  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) / 1e3)
    return float(np.median(times)), times


@contextlib.contextmanager
def pcie_bytes(moved):
    """Adds to moved['up'] / moved['down'] the size of every tensor that Tensor.to / Tensor.cpu carries across."""
    to, cpu = torch.Tensor.to, torch.Tensor.cpu

    def counted_to(self, *args, **kw):
        out = to(self, *args, **kw)
        if out.is_cuda != self.is_cuda:
            moved["up" if out.is_cuda else "down"] += out.numel() * out.element_size()
        return out

    def counted_cpu(self, *args, **kw):
        if self.is_cuda:
            moved["down"] += self.numel() * self.element_size()
        return cpu(self, *args, **kw)

    torch.Tensor.to, torch.Tensor.cpu = counted_to, counted_cpu
    try:
        yield moved
    finally:
        torch.Tensor.to, torch.Tensor.cpu = to, cpu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-smoother", choices=("scipy", "numpy"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    smoother = a.host_smoother
    if smoother is None:
        try:
            import scipy.signal  # noqa: F401
            smoother = "scipy"
        except ImportError:
            smoother = "numpy"
    if smoother == "scipy":
        from scipy.ndimage import gaussian_filter1d
        from scipy.signal import medfilt

        def host_smooth(rows):
            return np.stack([gaussian_filter1d(medfilt(rows[:, c], 11), 3) for c in range(3)], axis=1)
    else:
        def host_smooth(rows):
            return TO.smooth_bbox_params(rows, 11, 3)
    rng = np.random.default_rng(0)
    h, w, n = a.height, a.width, a.frames
    tracks = [TO.make_track(rng, n, 17, h, w, holes=set(rng.choice(np.arange(1, n - 1), n // 20, replace=False).tolist())) for _ in range(a.tracks)]
    # one second of distinct frames, repeated: the kernels read every frame either way, the host does not have to make gigabytes of noise
    base = torch.from_numpy(rng.integers(0, 256, (25, h, w, 3), dtype=np.uint8)).to("cuda:0")
    frames = base.repeat((n + 24) // 25, 1, 1, 1)[:n].contiguous()
    del base

    def on_device():
        return process_tracks(frames, tracks, vis_thresh=0.1)

    def on_host():
        out = []
        for trk in tracks:
            rows, start, end = TO.get_all_bbox_params(trk, 0.1)
            smooth = np.vstack([np.zeros((start, 3)), host_smooth(rows)])
            crops, infos = process_images(frames[start:end], smooth[start:end])
            out.append((crops, (start, end), infos))
        torch.cuda.current_stream().synchronize()
        return out

    with pcie_bytes({"up": 0, "down": 0}) as dev_moved:
        got = on_device()
    with pcie_bytes({"up": 0, "down": 0}) as host_moved:
        want = on_host()
    same = all(torch.equal(g[0], x[0]) and g[1] == x[1] for g, x in zip(got, want))
    del got, want
    dev_s, dev_all = timed(on_device, a.reps)
    host_s, host_all = timed(on_host, a.reps)
    leg = lambda seconds, every, moved: {"seconds": round(seconds, 5), "all_seconds": [round(t, 5) for t in every], "pcie_bytes": moved["up"] + moved["down"],
                                         "pcie_bytes_up": moved["up"], "pcie_bytes_down": moved["down"]}
    res = {"device": torch.cuda.get_device_name(0), "tracks": a.tracks, "frames": n, "frame": [h, w], "reps": a.reps, "host_smoother": smoother,
           "process_tracks": leg(dev_s, dev_all, dev_moved), "host_smoothing_then_process_images": leg(host_s, host_all, host_moved),
           "crops_bit_identical": bool(same)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
