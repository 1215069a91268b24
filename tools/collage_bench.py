"""The demo's finished frames two ways, on 256 frames of 720x1280 (-> 405x720 at max_img_size = 720):

  device  util/render/video.render_views(..., views=('collage',)) and one download of the uint8 collage frames
  host    today's way: render_views' three mesh panels, downloaded with the crops and keypoints, then the skeleton and the
          collage in NumPy (tests/collage_oracle.py, standing in for cv2 on the host)

Wall-clock frames per second of each (synchronised), and the bytes that cross PCIe at the copy sites.  Prints one JSON
object; `--out FILE` also writes it.  Recorded, not gated.

    python tools/collage_bench.py [--frames 256] [--reps 3] [--out profiles/collage_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collage_oracle as CO  # noqa: E402
from human_dynamics_amd.util.render import mesh, video  # noqa: E402
from human_dynamics_amd.util.render.raster import MeshFaces  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, S = a.frames, 224
    v, f = mesh.deformed_sphere(seed=0)
    faces = MeshFaces(f)
    rng = np.random.default_rng(0)
    cams = np.stack([rng.uniform(0.8, 1.0, n), rng.uniform(-.1, .1, n), rng.uniform(-.1, .1, n)], 1).astype(np.float32)
    preds = {"cams": torch.as_tensor(cams, device=dev), "kps": torch.as_tensor(rng.uniform(-0.8, 0.8, (n, 25, 2)).astype(np.float32), device=dev),
             "verts": torch.as_tensor(v + rng.normal(0, 0.01, (n, 1, 3)).astype(np.float32), device=dev)}
    frames = torch.as_tensor(rng.integers(0, 256, (n, 720, 1280, 3), dtype=np.uint8), device=dev)
    crops = torch.as_tensor(rng.uniform(-1, 1, (n, S, S, 3)).astype(np.float32), device=dev)
    params = [{"start_pt": np.array([640 + 30 * rng.standard_normal(), 360 + 30 * rng.standard_normal()]), "scale": S / 500.0,
               "im_shape": [S, S]} for _ in range(n)]

    def device_path():
        out = video.render_views(preds, None, frames, params, faces, crops=crops, views=('collage',))
        host = out["collage"].cpu().numpy()
        return host, host.nbytes

    def host_path():
        out = video.render_views(preds, None, frames, params, faces, crops=crops)
        got = {k: t.cpu().numpy() for k, t in out.items()}
        cr, kp = crops.cpu().numpy(), preds["kps"].cpu().numpy()
        moved = sum(x.nbytes for x in got.values()) + cr.nbytes + kp.nbytes
        res = []
        for i in range(n):
            skel = CO.draw_skeleton(((cr[i] + 1) * 0.5) * 255., ((kp[i] + 1) * 0.5) * S)[0].astype(np.uint8)
            res.append(CO.compose(got["crop"][i], skel, got["orig"][i], got["rotated"][i]))
        return np.stack(res), moved

    res = {"device": torch.cuda.get_device_name(0), "frames": n}
    for name, run, reps in (("device", device_path, a.reps), ("host", host_path, 1)):
        run() if name == "device" else None                  # warm-up (the host path is too slow to repeat)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out, moved = run()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res[name] = {"s": round(dt, 4), "frames_per_s": round(n / dt, 1), "pcie_bytes_per_frame": int(moved // n),
                     "out_shape": list(out.shape)}
        print("%-7s %8.3f s %9.1f frames/s %9d bytes/frame over PCIe" % (name, dt, n / dt, moved // n), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
