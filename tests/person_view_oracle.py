"""NumPy float64 restatement of hmmr_video_bbox (include/hmmr_hip.h; csrc/person_view.hip): compute_video_bbox of
src/util/render/nmr_renderer.py (:519-634) over ragged tracks, with this project's status word in place of the reference's
breakpoint and undefined cases.  tests/test_person_view_oracle.py pins it to the reference-executed fixture; the GPU tests
use it for shapes the fixture does not hold.
"""
import numpy as np

EMPTY, NOT_FINITE, DEGENERATE, BEYOND_START = 1, 2, 4, 8


def frame_extremes(kps, proc, proc_size, img_h, img_w, margin):
    """kps [n,k,2], proc [n,3] = {scale, start_x, start_y} -> [n,4] = {ymin, ymax, xmin, xmax} of every frame, before any cast"""
    kps, proc = np.asarray(kps, np.float64), np.asarray(proc, np.float64)
    with np.errstate(all="ignore"):
        undo = 1. / proc[:, 0]
        p = ((kps + 1) * 0.5) * proc_size
        q = ((p + proc[:, None, 1:3]) - proc_size) * undo[:, None, None]
        x, y = q[:, :, 0], q[:, :, 1]
        return np.stack([np.maximum(0., y.min(1) - margin), np.minimum(float(img_h - 1), y.max(1) + margin),
                         np.maximum(0., x.min(1) - margin), np.minimum(float(img_w - 1), x.max(1) + margin)], 1)


def crop_cameras(cams, proc, proc_size, bbox):
    """cams [n,3], proc [n,3], one bbox {ymin, ymax, xmin, xmax} -> (float64 cameras [n,3] before the one rounding to fp32,
    trap [n]: the frames at which the reference stops in its breakpoint)"""
    cams, proc = np.asarray(cams, np.float64), np.asarray(proc, np.float64)
    off = np.array([bbox[2], bbox[0]], np.float64)
    S = max(int(bbox[1]) - int(bbox[0]), int(bbox[3]) - int(bbox[2]))
    with np.errstate(all="ignore"):
        scale, start = proc[:, 0], proc[:, 1:3]
        undo = 1. / scale
        start2 = start - off[None] * scale[:, None]
        trap = np.sqrt(start[:, 0] * start[:, 0] + start[:, 1] * start[:, 1]) < np.sqrt(off[0] * off[0] + off[1] * off[1])
        c0 = (proc_size * cams[:, 0]) * 0.5
        c12 = cams[:, 1:3] + ((2. / cams[:, 0]) * 0.5)[:, None]
        o0 = c0 * undo
        o12 = c12 + (start2 - proc_size) / c0[:, None]
        k = np.float64(2.) / np.float64(S)
        new = np.concatenate([(o0 * k)[:, None], o12 - (1. / (k * o0))[:, None]], 1)
    return new, trap


def video_bbox(cams, kps, proc, proc_size, offsets, img_h, img_w, margin):
    """cams [N,3], kps [N,k,2], proc [N,3], offsets [T+1] -> dict(bbox int32 [T,4], cams_crop float32 [N,3] (rows of an EMPTY
    range untouched: NaN-filled here and masked by `written`), cams64 [N,3], status int32 [T], trap bool [N], written bool [N])"""
    cams, kps, proc = (np.asarray(a, np.float64) for a in (cams, kps, proc))
    T = len(offsets) - 1
    N = int(offsets[-1])
    bbox, status = np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
    cams64, trap, written = np.full((N, 3), np.nan), np.zeros(N, bool), np.zeros(N, bool)
    for t in range(T):
        a, b = int(offsets[t]), int(offsets[t + 1])
        if b <= a:
            status[t] = EMPTY
            continue
        written[a:b] = True
        ext = frame_extremes(kps[a:b], proc[a:b], proc_size, img_h, img_w, margin)
        e = np.array([ext[:, 0].min(), ext[:, 1].max(), ext[:, 2].min(), ext[:, 3].max()]) if np.isfinite(ext).all() else np.full(4, np.nan)
        finite = np.isfinite(cams[a:b]).all() and np.isfinite(kps[a:b]).all() and np.isfinite(proc[a:b]).all() and np.isfinite(e).all()
        if not finite or not ((e > -2147483649.) & (e < 2147483648.)).all():
            status[t] = NOT_FINITE
            continue
        bbox[t] = np.trunc(e).astype(np.int64)
        cams64[a:b], trap[a:b] = crop_cameras(cams[a:b], proc[a:b], proc_size, bbox[t])
        S = max(int(bbox[t, 1]) - int(bbox[t, 0]), int(bbox[t, 3]) - int(bbox[t, 2]))
        status[t] = (DEGENERATE if S <= 0 else 0) | (BEYOND_START if trap[a:b].any() else 0)
    with np.errstate(all="ignore"):
        cams32 = cams64.astype(np.float32)
    return {"bbox": bbox, "cams_crop": cams32, "cams64": cams64, "status": status, "trap": trap, "written": written}


def clip_size(bbox, max_img_size=300):
    """(h', w', S'): the window of a box after visualize_mesh_og's optional down-scale (resize_img's floor) and its longer side"""
    h, w = int(bbox[1]) - int(bbox[0]), int(bbox[3]) - int(bbox[2])
    if max(h, w) > max_img_size:
        s = max_img_size / float(max(h, w))
        h, w = int(np.floor(h * s)), int(np.floor(w * s))
    return h, w, max(h, w)
