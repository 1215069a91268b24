"""Wall time of scoring one tube with compute_mesh=True, two ways (evaluation/eval.py):

  records   eval.score_records on the packed per-frame records where Tester.predict_records left them;
  host      what a user did before: download the dictionary predict_all_images returns, score it with the NumPy restatement
            (tests/eval_oracle.py), the meshes from engine.smpl downloaded to the host.

Warm, repeated until a leg has run for more than a second; reports both times and the bytes each moves over PCIe.  The bytes are
counted where the copies are made: for one call of each leg, Tensor.to and Tensor.cpu are wrapped and every transfer between
host and device adds its size.  Prints one JSON object; `--out FILE` also writes it.  Recorded, not gated.

    python tools/eval_bench.py [--frames 1000] [--out profiles/eval_bench.json]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_oracle as EO  # noqa: E402
from human_dynamics_amd import assets  # noqa: E402
from human_dynamics_amd.dist import unpack_outputs  # noqa: E402
from human_dynamics_amd.evaluation import eval as ev  # noqa: E402
from human_dynamics_amd.evaluation.tester import Tester  # noqa: E402


class Cfg(object):
    load_path, batch_size, sequence_length, pred_mode, num_conv_layers = "synthetic:0", 8, 20, "pred", 3
    delta_t_values, smpl_model_path, num_kps = ["-5", "5"], "synthetic:2", 25


def timed(fn, min_seconds=1.0):
    fn()
    torch.cuda.synchronize()
    reps, t0 = 0, time.perf_counter()
    while reps < 2 or time.perf_counter() - t0 < min_seconds:
        fn()
        torch.cuda.synchronize()
        reps += 1
    return (time.perf_counter() - t0) / reps, reps


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
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.frames
    t = Tester(Cfg(), weights=assets.make_synthetic_weights(0), smpl=assets.make_synthetic_smpl(2), dtype="f32", device="cuda:0")
    rng = np.random.default_rng(0)
    strips = torch.as_tensor(rng.normal(0, 1, (n, 2048)).astype(np.float32), device="cuda:0")
    rec = t.predict_records(strips)
    layout, rec_len = t.record_layout()
    kps = np.concatenate([rng.uniform(40, 180, (n, 25, 2)), rng.uniform(size=(n, 25, 1)) < 0.8], axis=2).astype(np.float32)
    data = {"kps": kps, "gt3ds": rng.normal(0, 0.3, (n, 14, 3)).astype(np.float32),
            "poses": rng.normal(0, 0.3, (n, 72)).astype(np.float32), "shape": rng.normal(0, 1, 10).astype(np.float32)}

    def on_device():
        return ev.score_records(rec, layout, data, has_3d=True, min_visible=6, compute_mesh=True, engine=t.engine)

    def host_smpl(poses, shapes):
        return ev.compute_gpu_smpl(poses.astype(np.float32), shapes.astype(np.float32), engine=t.engine).cpu().numpy().astype(np.float64)

    def on_host():
        preds = {k: v.cpu().numpy() for k, v in unpack_outputs(rec, layout).items()}       # the dictionary predict_all_images returns
        return EO.score_old_way(preds, data, host_smpl, min_visible=6)

    with pcie_bytes({"up": 0, "down": 0}) as dev_moved:
        a_out = on_device()
    with pcie_bytes({"up": 0, "down": 0}) as host_moved:
        b_out = on_host()
    worst = max(float(np.nanmax(np.abs(np.asarray(a_out[k], np.float64) - np.asarray(b_out[k], np.float64)))) for k in a_out
                if np.ndim(a_out[k]) > 0)
    dev_s, dev_reps = timed(on_device)
    host_s, host_reps = timed(on_host)
    leg = lambda seconds, reps, moved: {"seconds": round(seconds, 5), "reps": reps, "pcie_bytes": moved["up"] + moved["down"],
                                        "pcie_bytes_up": moved["up"], "pcie_bytes_down": moved["down"]}
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "compute_mesh": True,
           "score_records": leg(dev_s, dev_reps, dev_moved), "download_and_numpy": leg(host_s, host_reps, host_moved),
           "max_abs_difference_between_the_two": worst}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
