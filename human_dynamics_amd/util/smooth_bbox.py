"""Device mirror of src/util/smooth_bbox.py: the reference's four names with its signatures and return values, run by the
kernels of csrc/track.hip (hmmr_track_bbox, hmmr_track_smooth) in float64 -- no SciPy.

    smoothed, start, end = get_smooth_bbox_params(kps, vis_thresh=0.1)        # kps: list of (K, 3) arrays or None

`smooth_tracks` is the batched form: any number of tracks in one call, the results left on the device if asked
(evaluation/run_video.process_tracks goes on from there to the crops without a host step).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..evaluation.tracks import pack_tracks


def gaussian_weights(sigma, truncate=4.0):
    """The weights scipy.ndimage.gaussian_filter1d(x, sigma) correlates with, in float64, and their radius."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return np.ascontiguousarray(w / w.sum(), np.float64), radius


def _filters(kernel_size, sigma):
    w, radius = gaussian_weights(sigma)
    if int(kernel_size) != kernel_size:
        raise ValueError("kernel_size must be an odd integer")
    return int(kernel_size), w.ctypes.data_as(C.POINTER(C.c_double)), radius, w            # w: keeps the buffer alive


def _offsets(offsets):
    off = np.ascontiguousarray(offsets, np.int32)
    return off, off.ctypes.data_as(C.POINTER(C.c_int32))


def _workspace(lib, n, n_tracks, device):
    nbytes = lib.hmmr_track_workspace_bytes(n, n_tracks)
    if nbytes == 0:
        raise L.HmmrError("hmmr_track_workspace_bytes(%d, %d): bad arguments" % (n, n_tracks))
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def track_boxes(kps, present, offsets, vis_thresh, kernel_size=11, sigma=3, want_raw=False):
    """hmmr_track_bbox on DEVICE tensors kps float64 [N, K, 3] and present uint8 [N] with the host int32 offsets
    [n_tracks + 1]: returns device tensors (bbox_smooth [N, 3], range [n_tracks, 2], bbox_raw [N, 3] or None).  Launches on
    the current stream and does not wait for it."""
    lib = L.load()
    assert kps.is_cuda and kps.dtype == torch.float64 and kps.dim() == 3 and kps.shape[2] == 3 and kps.is_contiguous(), "kps: float64 [N,K,3] on the device"
    assert present.is_cuda and present.dtype == torch.uint8 and present.shape == kps.shape[:1], "present: uint8 [N] on the device"
    off, off_p = _offsets(offsets)
    n, n_tracks, dev = kps.shape[0], len(off) - 1, kps.device
    assert off[-1] == n and off[0] == 0, "offsets must cover the rows of kps"
    ks, w_p, radius, _keep = _filters(kernel_size, sigma)
    smooth = torch.empty((n, 3), dtype=torch.float64, device=dev)
    raw = torch.empty((n, 3), dtype=torch.float64, device=dev) if want_raw else None
    rng = torch.empty((max(n_tracks, 1), 2), dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace(lib, n, n_tracks, dev)
    L.check(lib.hmmr_track_bbox(kps.data_ptr(), present.data_ptr(), off_p, n_tracks, kps.shape[1], float(vis_thresh), ks, w_p, radius,
                                L.ptr(raw), smooth.data_ptr(), rng.data_ptr(), ws.data_ptr(), ws_bytes,
                                torch.cuda.current_stream(dev).cuda_stream), "hmmr_track_bbox")
    return smooth, rng, raw


def smooth_tracks(tracks, vis_thresh=2, kernel_size=11, sigma=3, device="cuda:0", keep_device=False, want_raw=False):
    """get_smooth_bbox_params for several tracks in one call.  tracks: [track][frame] -> (K, 3) array or None.

    Returns one (smoothed float64 [end, 3], start, end) per track, as get_smooth_bbox_params does; a track without a valid frame
    gives (empty [0, 3], -1, 0).  keep_device=True returns instead the dict of what the call left on the device, without
    waiting for it: 'bbox_smooth' [N, 3], 'range' [n_tracks, 2], 'bbox_raw' (want_raw) and the host 'offsets'."""
    kps, present, offsets = pack_tracks(tracks)
    if len(tracks) == 0:
        return {} if keep_device else []
    smooth, rng, raw = track_boxes(torch.from_numpy(kps).to(device), torch.from_numpy(present).to(device), offsets, vis_thresh,
                                   kernel_size, sigma, want_raw)
    if keep_device:
        return {"bbox_smooth": smooth, "range": rng, "bbox_raw": raw, "offsets": offsets}
    smooth, rng = smooth.cpu().numpy(), rng.cpu().numpy()
    raw = raw.cpu().numpy() if want_raw else None
    out = []
    for t in range(len(tracks)):
        o, start, end = int(offsets[t]), int(rng[t][0]), int(rng[t][1])
        item = (smooth[o:o + end].copy(), start, end)
        out.append(item + (raw[o + max(start, 0):o + end].copy(),) if want_raw else item)
    return out


def get_smooth_bbox_params(kps, vis_thresh=2, kernel_size=11, sigma=3):
    """Smooth bounding box parameters from keypoints: the box that scales the person to about 150 px per frame, linear
    interpolation over frames without one, an 11-tap median, a Gaussian.

    kps: list of (K, 3) arrays or None.  Returns (smoothed [end, 3] = [cx, cy, scale] with zero rows in front of `start`,
    start (inclusive), end (exclusive)).  A list without a single valid frame raises ValueError, as the reference does."""
    smoothed, start, end = smooth_tracks([list(kps)], vis_thresh, kernel_size, sigma)[0]
    if start < 0:
        raise ValueError("no frame of the track has a bounding box (start = -1): nothing to stack the smoothed boxes on")
    return smoothed, start, end


def _raw_boxes(kps, vis_thresh, device="cuda:0"):
    """(rows [end - start, 3], start, end) of one track: only bbox_raw and the range are downloaded"""
    packed, present, offsets = pack_tracks([list(kps)])
    _, rng, raw = track_boxes(torch.from_numpy(packed).to(device), torch.from_numpy(present).to(device), offsets, vis_thresh, 1, 3,
                              want_raw=True)
    start, end = (int(v) for v in rng.cpu().numpy()[0])
    return raw[max(start, 0):end].cpu().numpy(), start, end


def kp_to_bbox_param(kp, vis_thresh):
    """[center_x, center_y, scale] of one frame's (K, 3) keypoints, or None if the frame has no box."""
    if kp is None:
        return None
    raw, start, _ = _raw_boxes([kp], vis_thresh)
    return None if start < 0 else raw[0]


def get_all_bbox_params(kps, vis_thresh=2):
    """(bbox_params [end - start, 3] with the gaps interpolated, start_index (incl), end_index (excl)); (-1, 0) and no rows
    when no frame has a box."""
    return _raw_boxes(kps, vis_thresh)


def smooth_bbox_params(bbox_params, kernel_size=11, sigma=8, device="cuda:0"):
    """Median then Gaussian filtering of bounding box parameters [N, 3] -> [N, 3] (hmmr_track_smooth)."""
    lib = L.load()
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(bbox_params, np.float64).reshape(-1, 3))).to(device)
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, 3))
    off, off_p = _offsets([0, n])
    ks, w_p, radius, _keep = _filters(kernel_size, sigma)
    out = torch.empty_like(p)
    ws, ws_bytes = _workspace(lib, n, 1, p.device)
    L.check(lib.hmmr_track_smooth(p.data_ptr(), off_p, 1, ks, w_p, radius, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                  torch.cuda.current_stream(p.device).cuda_stream), "hmmr_track_smooth")
    return out.cpu().numpy()
