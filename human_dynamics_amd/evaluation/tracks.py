"""Person tracks on the host: the PoseFlow reader of the reference's demo_video.py (`get_labels_poseflow`, :61-121) and the
packing of its list-of-lists into the arrays the device front end reads (csrc/track.hip, util/smooth_bbox.py).

    all_kps = get_labels_poseflow(json_path, num_frames)      # [person][frame] -> (K, 3) array or None, longest track first
    kps, present, offsets = pack_tracks(all_kps)              # float64 [N, K, 3], uint8 [N], int32 [n_tracks + 1]
"""
from __future__ import annotations

import json
import re

import numpy as np


def get_labels_poseflow(json_path, num_frames, min_kp_count=20):
    """The poses of every person tracklet in an AlphaPose / PoseFlow result file.

    Returns a list over people; each entry is a list over the file's frames (sorted by name) holding the (num_kp, 3) array
    (x, y, score) of the person in that frame, or None where the person is not seen -- before the first appearance included.
    Tracklets with fewer than min_kp_count detections are dropped; the rest are ordered by np.argsort(counts)[::-1], longest
    first.  Where the reference stops in a debugger (no person in the first frame) this raises ValueError."""
    with open(json_path, "r") as f:
        data = json.load(f)
    names = sorted(data.keys())
    if len(names) != num_frames and names:
        first = int(re.findall(r"\d+", names[0])[0])
        if first != 0:
            raise ValueError("PoseFlow found nobody in the first frame (the first frame with people is %d of %d): "
                             "the frame numbering of the tracks would be off" % (first, num_frames))
    tracks, counts = {}, {}
    for i, name in enumerate(names):
        seen = []
        for person in data[name]:
            idx = int(person["idx"])
            if idx not in tracks:
                tracks[idx], counts[idx] = [None] * i, 0
            tracks[idx].append(np.array(person["keypoints"]).reshape(-1, 3))
            counts[idx] += 1
            seen.append(idx)
        for idx in set(tracks).difference(seen):
            tracks[idx].append(None)
    kept = [idx for idx in tracks if counts[idx] >= min_kp_count]
    order = np.argsort([counts[idx] for idx in kept])[::-1]
    return [tracks[kept[j]] for j in order]


def pack_tracks(tracks):
    """[track][frame] -> (K, 3) or None  ==>  kps float64 [N, K, 3] (zeros where None), present uint8 [N], offsets int32
    [n_tracks + 1]: the tracks one after the other.  Every keypoint array of the call must have the same K (K = 1 if there is
    none at all)."""
    shapes = {np.shape(kp) for trk in tracks for kp in trk if kp is not None}
    if len(shapes) > 1 or any(len(s) != 2 or s[1] != 3 for s in shapes):
        raise ValueError("keypoints must all be (K, 3) arrays with one K, got shapes %s" % sorted(shapes))
    k = shapes.pop()[0] if shapes else 1
    if k < 1:
        raise ValueError("keypoints must be (K, 3) arrays with K >= 1")
    offsets = np.zeros(len(tracks) + 1, np.int32)
    offsets[1:] = np.cumsum([len(trk) for trk in tracks])
    n = int(offsets[-1])
    kps, present = np.zeros((n, k, 3), np.float64), np.zeros(n, np.uint8)
    row = 0
    for trk in tracks:
        for kp in trk:
            if kp is not None:
                kps[row], present[row] = kp, 1
            row += 1
    return kps, present, offsets


def unpack_tracks(kps, present, offsets):
    """The inverse of pack_tracks."""
    return [[kps[r].copy() if present[r] else None for r in range(offsets[t], offsets[t + 1])] for t in range(len(offsets) - 1)]
