"""hipEvent timing of the scene view against what could be done before it: for T = 1, 2, 4 and 8 SMPL-sized tracks over the
same frames of a 720x1280 video (-> 405x720 at S = 720), one hmmr_render_scene call against T chained hmmr_render_mesh
calls, each of which takes the previous call's uint8 frames as its background (so the chain re-quantises T times and
layers the persons in call order, not by key: it is a cost comparison, not an equivalence).  Inputs are on the device
before the clock starts; warm; events around the calls.  The ratio chain / scene is recorded, not gated.  Prints one JSON
object; `--out FILE` also writes it.

    python tools/scene_bench.py [--frames 64] [--reps 10] [--out profiles/scene_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from human_dynamics_amd import _lib as L  # noqa: E402
from human_dynamics_amd.util.render import mesh, raster, video  # noqa: E402
from human_dynamics_amd.util.render.handoff import orig_image_geometry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    n, frame_hw = a.frames, (720, 1280)
    h, w, S = video.orig_output_size(frame_hw, 720)
    v, f = mesh.deformed_sphere(seed=0)
    faces = raster.MeshFaces(f)
    rng = np.random.default_rng(0)
    frames = torch.as_tensor(rng.integers(0, 256, (n,) + frame_hw + (3,), dtype=np.uint8), device=dev)
    props = torch.cuda.get_device_properties(0)
    res = {"device": props.name, "nominal_clock_mhz": getattr(props, "clock_rate", 0) / 1e3 or None, "frames": n, "size": S,
           "out_hw": [h, w], "faces": len(f), "verts": len(v), "reps": a.reps, "tracks": {}}

    def track(i, n_tracks):
        """person i of n_tracks, spread across the frame's width, 500-pixel boxes (scale 224 / 500) that overlap from T = 4 on"""
        cams = np.stack([rng.uniform(0.8, 1.0, n), rng.uniform(-.1, .1, n), rng.uniform(-.1, .1, n)], 1).astype(np.float32)
        cx = 1280 * (i + 1) / (n_tracks + 1.0)
        params = [{"start_pt": np.array([cx + 10 * rng.standard_normal(), 360 + 10 * rng.standard_normal()]) * (224 / 500.0) + 112,
                   "scale": 224 / 500.0, "im_shape": [224, 224]} for _ in range(n)]
        return {"verts": torch.as_tensor(v[None] + rng.normal(0, 0.01, (n, 1, 3)).astype(np.float32), device=dev),
                "cams": torch.as_tensor(cams, device=dev), "range": (0, n),
                "geom": np.stack([orig_image_geometry(p, frame_hw, 720) for p in params])}

    def timed(run, reps):
        for _ in range(2):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for n_tracks in (1, 2, 4, 8):
        tracks = [track(i, n_tracks) for i in range(n_tracks)]

        def scene():
            return raster.render_scene(tracks, faces, S, n, bg_mode=L.RENDER_BG_FRAME, bg_image=frames, out_hw=(h, w))["rgb"]

        def chain():
            bg = frames
            for i, t in enumerate(tracks):
                bg = raster.render_mesh(t["verts"], t["cams"], faces, S, geom=t["geom"], color=raster.scene_color(i),
                                        bg_mode=L.RENDER_BG_FRAME, bg_image=bg, out_hw=(h, w))["rgb"]
            return bg
        # alternate the two so that neither has the quieter half of the run
        ms = {"scene": [], "chain": []}
        for _ in range(3):
            ms["scene"].append(timed(scene, a.reps))
            ms["chain"].append(timed(chain, a.reps))
        s, c = float(np.median(ms["scene"])), float(np.median(ms["chain"]))
        res["tracks"][str(n_tracks)] = {"scene_ms": round(s, 4), "chain_ms": round(c, 4), "chain_over_scene": round(c / s, 3),
                                        "scene_ms_runs": [round(x, 4) for x in ms["scene"]],
                                        "chain_ms_runs": [round(x, 4) for x in ms["chain"]],
                                        "scene_frames_per_s": round(n / s * 1e3, 1)}
        print("T = %d: scene %9.3f ms, chain %9.3f ms, chain / scene %.3f" % (n_tracks, s, c, c / s), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
