"""One timing of the person-centred view's box step, recorded and not gated: 8 tracks x 100 frames of packed per-frame records
(SMPL-sized: 6 890 vertices, the layout of human_dynamics_amd.dist.record_layout) in one buffer on the device.

  device   util/render/video.video_bboxes: cams / kps read in place inside the records by one hmmr_video_bbox call; the
           {scale, start} rows go up, the boxes and status words come down
  host     what a user had to do before: download cams and kps of every frame, run the NumPy float64 restatement
           (tests/person_view_oracle.py, imported by putting tests/ on sys.path; the reference's arithmetic vectorised -- the reference's own per-frame Python loop is
           slower still) per track, upload the cameras
Both start from the same inputs: the record buffer on the device and process_image's dicts on the host.

Host clock around calls that end in a synchronisation (both paths end in one), warm, alternated; and device events around the
hmmr_video_bbox call alone.  The bytes over PCIe are counted where the copies are made.  Prints one JSON object; `--out FILE`
also writes it.

    python tools/person_clip_bench.py [--tracks 8] [--frames 100] [--reps 20] [--out profiles/person_clip_bench.log]
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
import person_view_oracle as PV  # noqa: E402
from human_dynamics_amd.dist import record_layout  # noqa: E402
from human_dynamics_amd.util.render import person_view, video  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=8)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("person_clip_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    T, n_t, hw, margin, k = a.tracks, a.frames, (720, 1280), 10, 25
    n = T * n_t
    layout, rec_len = record_layout(2)
    get = {key: (off, size) for key, _, off, size in layout}
    rng = np.random.default_rng(0)
    rec = torch.zeros((n, rec_len), dtype=torch.float32, device=dev)
    cams = np.stack([rng.uniform(0.5, 1.2, n), rng.uniform(-.3, .3, n), rng.uniform(-.3, .3, n)], 1).astype(np.float32)
    kps = rng.uniform(-0.85, 0.85, (n, 2 * k)).astype(np.float32)
    rec[:, get["cams"][0]:get["cams"][0] + 3] = torch.as_tensor(cams, device=dev)
    rec[:, get["kps"][0]:get["kps"][0] + 2 * k] = torch.as_tensor(kps, device=dev)
    tracks, counted = [], {"device": {"up": 0, "down": 0}, "host": {"up": 0, "down": 0}}
    for t in range(T):
        scale = rng.uniform(0.5, 1.5) * rng.uniform(0.97, 1.03, n_t)
        centre = np.array([1280 * (t + 1) / (T + 1.0), 360.]) + np.cumsum(rng.normal(0, 2, (n_t, 2)), 0)
        params = [{"scale": float(scale[i]), "start_pt": (np.round(centre[i] * scale[i]) + 112).astype(int), "im_shape": [224, 224]}
                  for i in range(n_t)]
        tracks.append((rec[t * n_t:(t + 1) * n_t], layout, (0, n_t), params))
    assert video._records_in_place(tracks) is not None
    oc, ok = get["cams"][0], get["kps"][0]
    proc_host = [person_view.proc_rows(p) for _, _, _, p in tracks]

    def device_path():
        bbox, crops, status = video.video_bboxes(tracks, hw, margin)          # ends in its one download
        return bbox, crops, status

    def host_path():
        c = rec[:, oc:oc + 3].cpu().numpy()                                   # (each .cpu() waits for the device)
        kp = rec[:, ok:ok + 2 * k].cpu().numpy()
        counted["host"]["down"] = c.nbytes + kp.nbytes
        boxes, out = [], []
        for t in range(T):
            proc_t = person_view.proc_rows(tracks[t][3])                      # (both paths start from process_image's dicts)
            r = PV.video_bbox(c[t * n_t:(t + 1) * n_t], kp[t * n_t:(t + 1) * n_t].reshape(n_t, k, 2), proc_t, 224., [0, n_t], hw[0], hw[1], margin)
            boxes.append(r["bbox"][0])
            out.append(r["cams_crop"])
        up = np.concatenate(out)
        counted["host"]["up"] = up.nbytes
        crops = torch.as_tensor(up, device=dev)
        torch.cuda.synchronize()
        return np.stack(boxes), crops

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    bd, cd, sd = device_path()
    bh, ch = host_path()
    same_boxes = bool(np.array_equal(bd, bh))
    cam_diff = float((torch.cat(cd) - ch).abs().max())
    counted["device"]["up"] = sum(p.nbytes for p in proc_host)
    counted["device"]["down"] = bd.nbytes + sd.nbytes
    ms = {"device": [], "host": []}
    for _ in range(5):                                                        # alternate, so that neither has the quieter half of the run
        ms["device"].append(clock(device_path))
        ms["host"].append(clock(host_path))
    # the C call alone, inputs in place, device events
    proc = torch.as_tensor(np.concatenate(proc_host), device=dev)
    offsets = (n_t * np.arange(T + 1)).astype(np.int32)
    call = lambda: person_view.video_bbox(rec[:, oc:oc + 3], rec[:, ok:ok + 2 * k], k, proc, offsets, hw, margin)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        call()
    e1.record()
    torch.cuda.synchronize()
    props = torch.cuda.get_device_properties(0)
    d, h = float(np.median(ms["device"])), float(np.median(ms["host"]))
    res = {"device": props.name, "tracks": T, "frames_per_track": n_t, "record_floats": rec_len, "reps": a.reps,
           "video_bboxes_ms": round(d, 4), "video_bboxes_ms_runs": [round(x, 4) for x in ms["device"]],
           "download_numpy_upload_ms": round(h, 4), "download_numpy_upload_ms_runs": [round(x, 4) for x in ms["host"]],
           "host_over_device": round(h / d, 2),
           "hmmr_video_bbox_call_ms": round(e0.elapsed_time(e1) / 200, 5),
           "note_call": "200 back-to-back calls between two events (each allocates its three outputs): enqueue-bound, not the kernel's time",
           "pcie_bytes": counted, "boxes_equal": same_boxes, "largest_camera_difference": cam_diff}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
