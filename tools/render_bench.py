"""hipEvent timing of util/render/video.render_views (csrc/render.hip) on 256 frames, per panel:
the 224x224 crop view, the original-frame view of a 720x1280 frame (-> 405x720 at max_img_size = 720) and the rotated
view, for the SMPL-sized closed mesh at a person-like scale and for the synthetic SMPL's triangle soup (worst case:
most faces span most of the image).  Prints one JSON object; `--out FILE` also writes it.

    python tools/render_bench.py [--frames 256] [--reps 10] [--out profiles/render_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from human_dynamics_amd import assets  # noqa: E402
from human_dynamics_amd.util.render import mesh, video  # noqa: E402
from human_dynamics_amd.util.render.raster import MeshFaces  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--soup-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    v, f = mesh.deformed_sphere(seed=0)
    faces = MeshFaces(f)
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "faces": len(f), "verts": len(v), "views": {}}

    def inputs(n, verts_np):
        cams = np.stack([rng.uniform(0.8, 1.0, n), rng.uniform(-.1, .1, n), rng.uniform(-.1, .1, n)], 1).astype(np.float32)
        verts = torch.as_tensor(verts_np + rng.normal(0, 0.01, (n, 1, 3)).astype(np.float32), device=dev)
        preds = {"cams": torch.as_tensor(cams, device=dev), "verts": verts}
        frames = torch.as_tensor(rng.integers(0, 256, (n, 720, 1280, 3), dtype=np.uint8), device=dev)
        crops = torch.as_tensor(rng.uniform(-1, 1, (n, 224, 224, 3)).astype(np.float32), device=dev)
        params = [{"start_pt": np.array([640 + 30 * rng.standard_normal(), 360 + 30 * rng.standard_normal()]),
                   "scale": 224 / 500.0, "im_shape": [224, 224]} for _ in range(n)]
        return preds, frames, crops, params

    soup_v = assets.make_synthetic_smpl(2)["v_template"]
    for name, verts_np, n in (("closed", v, a.frames), ("soup", soup_v, a.soup_frames)):
        preds, frames, crops, params = inputs(n, verts_np)
        for view in ("crop", "orig", "rotated"):
            run = lambda: video.render_views(preds, None, frames, params, faces, crops=crops, views=(view,))
            for _ in range(2):
                out = run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = a.reps if name == "closed" else max(2, a.reps // 4)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            shape = list(out[view].shape)
            res["views"]["%s/%s" % (name, view)] = {"frames": n, "ms": round(ms, 4), "frames_per_s": round(n / ms * 1e3, 1),
                                                     "out_shape": shape,
                                                     "coverage": round(float((out[view] != 255).any(-1).float().mean()), 4)
                                                     if view == "rotated" else None}
            print("%-16s %4d frames %9.3f ms %10.1f frames/s  %s" % (name + "/" + view, n, ms, n / ms * 1e3, shape), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
