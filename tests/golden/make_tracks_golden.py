"""Golden vectors for the track front end (csrc/track.hip, human_dynamics_amd/util/smooth_bbox.py, evaluation/tracks.py),
produced by EXECUTING the reference's own code:

  reference_tracks.npz
      * src/util/smooth_bbox.py, loaded by path, with the real SciPy: get_all_bbox_params and get_smooth_bbox_params
        (vis_thresh 0.1, the demo's call) on the recorded seeded tracks of tests/track_oracle.seeded_cases(), and
        smooth_bbox_params alone over a few (length, kernel_size, sigma) combinations, tracks shorter than either filter among
        them;
      * get_labels_poseflow, lifted out of demo_video.py with `ast` (the module needs absl, ipdb and the tracker) and executed on
        synthetic PoseFlow files written here; the files' text (as bytes) is stored next to the lists it gave.
    Only inputs and results are stored.  This maker is the only file that reads the reference tree; tests read the .npz.

Near ties: the crop integers are floor / round of float64 values whose last bits depend on the summation order.  For every
recorded AND every seeded row the maker asserts that each floor / round argument lies at least 1e-6 from its decision boundary
(track_oracle.rounding_margin); if one does not, change the seed in track_oracle.seeded_cases, do not mask the row.  It also
asserts that the NumPy restatement agrees with the reference on every seeded case, recorded or not.

    python tests/golden/make_tracks_golden.py <reference tree>
"""
import ast
import importlib.util
import json
import os
import re
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HMMR_REFERENCE", "")
if not os.path.isdir(REF):
    sys.exit("usage: python tests/golden/make_tracks_golden.py <reference tree>   (or HMMR_REFERENCE)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import track_oracle as TO                                              # noqa: E402
from human_dynamics_amd.evaluation.tracks import pack_tracks           # noqa: E402

RECORDED = ("k25", "mixed", "bad_rows")                               # the seeded cases whose reference results the fixture carries
SHORT = 11                                                             # ... and the first SHORT tracks of 'lengths' (1 .. 26 rows)
MARGIN = 1e-6
FILTERS = ((1, 11, 3), (3, 11, 3), (5, 11, 3), (6, 11, 3), (12, 11, 3), (13, 11, 3), (40, 1, 0.5), (40, 3, 8), (40, 31, 3), (40, 11, 16),
           (7, 5, 16), (200, 11, 3))                                  # (rows, kernel_size, sigma); sigma 16: radius 64


def reference_smooth_bbox():
    spec = importlib.util.spec_from_file_location("reference_smooth_bbox", os.path.join(REF, "src", "util", "smooth_bbox.py"))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


class Stopped(Exception):
    pass


def reference_get_labels_poseflow():
    def set_trace():
        raise Stopped()
    tree = ast.parse(open(os.path.join(REF, "demo_video.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_labels_poseflow"]
    assert len(body) == 1
    ns = {"json": json, "re": re, "np": np, "ipdb": types.SimpleNamespace(set_trace=set_trace), "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=body, type_ignores=[]), "demo_video.py", "exec"), ns)
    return ns["get_labels_poseflow"]


def poseflow_files(rng):
    """name -> (text of a PoseFlow result file, num_frames, min_kp_count)"""
    def person(idx, k=5):
        kp = np.round(rng.uniform(0, 256, (k, 3)) * 8) / 8
        kp[:, 2] = np.round(rng.uniform(0, 1, k) * 256) / 256
        return {"keypoints": [float(v) for v in kp.reshape(-1)], "idx": idx, "scores": 1.5}
    spans = {3: range(0, 30), 7: range(4, 22), 1: list(range(10, 16)) + list(range(20, 30)), 12: range(25, 29), 5: range(2, 20),
             9: range(12, 30)}                                                               # 5 and 9: both 18 detections (a tie)
    full = {"%05d.png" % f: [person(idx) for idx in spans if f in spans[idx]] for f in range(30)}
    holes = {name: people for name, people in full.items() if name not in ("00005.png", "00017.png")}       # frames without people
    late = {name: people for name, people in full.items() if int(name[:5]) >= 2}                           # nobody in frames 0, 1
    dump = lambda d: json.dumps(d, sort_keys=False)
    return {"full": (dump(full), 30, 5), "full_min20": (dump(full), 30, 20), "holes": (dump(holes), 30, 5), "late": (dump(late), 30, 5)}


def main():
    ref, labels = reference_smooth_bbox(), reference_get_labels_poseflow()
    out = {"vis_thresh": np.array(TO.VIS_THRESH), "margin": np.array(MARGIN)}
    cases = TO.seeded_cases()
    recorded = {name: cases[name] for name in RECORDED}
    recorded["short"] = cases["lengths"][:2] + (cases["lengths"][2][:SHORT],)
    warnings.simplefilter("ignore")                                      # medfilt: 'kernel_size exceeds volume extent'
    worst = np.inf
    for name, (h, w, tracks) in list(cases.items()) + [("short", recorded["short"])]:
        for t, trk in enumerate(tracks):
            raw, start, end = ref.get_all_bbox_params(trk, TO.VIS_THRESH)
            o_raw, o_start, o_end = TO.get_all_bbox_params(trk, TO.VIS_THRESH)
            assert (start, end) == (o_start, o_end) and raw.shape == o_raw.shape, (name, t)
            if start < 0:
                smooth = np.zeros((0, 3))
            else:
                smooth, s2, e2 = ref.get_smooth_bbox_params(trk, vis_thresh=TO.VIS_THRESH)
                assert (s2, e2) == (start, end) and smooth.shape == (end, 3) and not smooth[:start].any()
                o_smooth = TO.get_smooth_bbox_params(trk, TO.VIS_THRESH)[0]
                for got, want in ((o_raw, raw), (o_smooth, smooth)):
                    assert (np.abs(got - want) <= 1e-12 * np.maximum(1, np.abs(want))).all(), (name, t)
                m = min([np.inf] + [TO.rounding_margin(h, w, b) for b in smooth[start:]])
                assert m >= MARGIN, "case %s track %d: a floor / round argument lies %.2e from its boundary: change the seed" % (name, t, m)
                worst = min(worst, m)
            if name in recorded:
                out["%s/%d/raw" % (name, t)], out["%s/%d/smooth" % (name, t)] = raw.astype(np.float64), smooth
                out["%s/%d/range" % (name, t)] = np.array([start, end], np.int32)
    print("smallest distance of a floor / round argument from its boundary: %.3e" % worst)
    for name, (h, w, tracks) in recorded.items():
        out[name + "/kps"], out[name + "/present"], out[name + "/offsets"] = pack_tracks(tracks)
        out[name + "/hw"] = np.array([h, w], np.int32)
    # ---- the two filters alone
    rng = np.random.default_rng(7)
    for n, ks, sigma in FILTERS:
        x = rng.uniform(20, 300, (n, 3)) * np.array([1, 1, 0.01])
        key = "filters/%d_%d_%g" % (n, ks, sigma)
        out[key + "/in"], out[key + "/out"] = x, ref.smooth_bbox_params(x, ks, sigma)
        got = TO.smooth_bbox_params(x, ks, sigma)
        assert (np.abs(got - out[key + "/out"]) <= 1e-12 * np.maximum(1, np.abs(out[key + "/out"]))).all(), key
    assert not out["filters/5_11_3/out"].any() and out["filters/6_11_3/out"].all()      # fewer than six rows smooth to zeros
    # ---- get_labels_poseflow
    with tempfile.TemporaryDirectory() as tmp:
        for name, (text, num_frames, min_count) in poseflow_files(np.random.default_rng(11)).items():
            path = os.path.join(tmp, name + ".json")
            with open(path, "w") as f:
                f.write(text)
            out["poseflow/%s/json" % name] = np.frombuffer(text.encode("ascii"), np.uint8)
            out["poseflow/%s/args" % name] = np.array([num_frames, min_count], np.int32)
            try:
                lists = labels(path, num_frames, min_count)
            except Stopped:
                out["poseflow/%s/stopped" % name] = np.array(1)
                continue
            out["poseflow/%s/stopped" % name] = np.array(0)
            if lists:
                kps, present, offsets = pack_tracks(lists)
            else:
                kps, present, offsets = np.zeros((0, 1, 3)), np.zeros(0, np.uint8), np.zeros(1, np.int32)
            out["poseflow/%s/kps" % name], out["poseflow/%s/present" % name], out["poseflow/%s/offsets" % name] = kps, present, offsets
            print("poseflow %s: %d tracks of lengths %s" % (name, len(lists), [int(present[a:b].sum()) for a, b in zip(offsets[:-1], offsets[1:])]))
    path = os.path.join(HERE, "reference_tracks.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
