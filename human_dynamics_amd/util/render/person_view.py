"""ctypes front of the person-centred view (csrc/person_view.hip, include/hmmr_hip.h: hmmr_video_bbox): the box that holds
a person over a whole track and every frame's camera relative to it -- the reference's compute_video_bbox
(src/util/render/nmr_renderer.py:519-634) for any number of tracks in one call.  The drop-in of that name is in
nmr_renderer.py; the whole-video drivers are video.video_bboxes and video.render_person_clips.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib as L

BBOX_SKIP = L.BBOX_EMPTY | L.BBOX_NOT_FINITE | L.BBOX_DEGENERATE      # no clip can be rendered for such a track


def status_words(status):
    """'EMPTY|BEYOND_START' for a status word (0: 'ok')"""
    names = [n for n, b in (("EMPTY", L.BBOX_EMPTY), ("NOT_FINITE", L.BBOX_NOT_FINITE), ("DEGENERATE", L.BBOX_DEGENERATE),
                            ("BEYOND_START", L.BBOX_BEYOND_START)) if int(status) & b]
    return "|".join(names) or "ok"


def proc_rows(image_og_params):
    """process_image's dicts (scale, start_pt) -> float64 [n, 3] = {scale, start_x, start_y}, the `proc` rows of hmmr_video_bbox"""
    out = np.empty((len(image_og_params), 3), np.float64)
    for i, p in enumerate(image_og_params):
        s, start = p["scale"], p["start_pt"]
        out[i, 0] = s if isinstance(s, float) else float(np.asarray(s).reshape(-1)[0])
        out[i, 1], out[i, 2] = start[0], start[1]
    return out


def clip_size(bbox, max_img_size=300):
    """(h', w', S): the window [ymin:ymax, xmin:xmax] of a box after visualize_mesh_og's optional down-scale to max_img_size
    (resize_img's floor, src/util/common.py:8) and the side of the square it is rendered in (make_square)."""
    h, w = int(bbox[1]) - int(bbox[0]), int(bbox[3]) - int(bbox[2])
    if max(h, w) > max_img_size:
        s = max_img_size / float(max(h, w))
        h, w = int(np.floor(h * s)), int(np.floor(w * s))
    return h, w, max(h, w)


def video_bbox(cams, kps, k, proc, offsets, frame_hw, margin=10, proc_size=224, stream=None):
    """One hmmr_video_bbox call.  cams [N, >= 3] and kps [N, >= 2k] float32 device rows with unit column stride, read in place
    (any row stride: views into packed records); proc float64 [N, 3] on the device; offsets: n_tracks + 1 HOST row numbers.
    -> (bbox int32 [T, 4] = {ymin, ymax, xmin, xmax}, cams_crop float32 [N, 3], status int32 [T]) on the device; nothing waits."""
    lib = L.load()
    dev = cams.device
    if dev.type != "cuda":
        raise L.HmmrError("video_bbox needs device tensors (the HIP library has no CPU path)")
    for name, t, dt in (("cams", cams, torch.float32), ("kps", kps, torch.float32), ("proc", proc, torch.float64)):
        if t.dim() != 2 or t.dtype != dt or (t.shape[0] > 0 and t.stride(1) != 1):
            raise ValueError("%s must be %s rows [N, width] with unit column stride" % (name, dt))
    offsets = np.ascontiguousarray(offsets, np.int32)
    n_tracks, n = len(offsets) - 1, int(offsets[-1]) if len(offsets) else 0
    if n_tracks < 1 or not (cams.shape[0] == kps.shape[0] == proc.shape[0] == n) or proc.shape[1] != 3 or not proc.is_contiguous():
        raise ValueError("%d tracks over %d rows for cams %s, kps %s and proc %s" % (n_tracks, n, tuple(cams.shape), tuple(kps.shape),
                                                                                  tuple(proc.shape)))
    ld = lambda t: t.stride(0) if t.shape[0] > 1 else t.shape[1]      # a single row may carry any stride
    if cams.shape[1] < 3 or kps.shape[1] < 2 * int(k):
        raise ValueError("rows of %d and %d floats for a camera and %d keypoints" % (cams.shape[1], kps.shape[1], k))
    bbox = torch.empty((n_tracks, 4), dtype=torch.int32, device=dev)
    status = torch.empty((n_tracks,), dtype=torch.int32, device=dev)
    crop = torch.empty((n, 3), dtype=torch.float32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    # an array without rows has no address worth passing: any non-null value is never dereferenced (every track is empty)
    p = lambda t: t.data_ptr() if t.numel() else bbox.data_ptr()
    L.check(lib.hmmr_video_bbox(p(cams), ld(cams), p(kps), ld(kps), int(k), p(proc), float(proc_size),
                                offsets.ctypes.data_as(L.C.POINTER(L.C.c_int32)), n_tracks, int(frame_hw[0]), int(frame_hw[1]), float(margin),
                                bbox.data_ptr(), p(crop), status.data_ptr(), st), "hmmr_video_bbox")
    return bbox, crop, status
