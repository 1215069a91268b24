"""NumPy spec of the scene view (include/hmmr_hip.h: hmmr_render_scene), in float64, on top of tests/render_oracle.py.

Per instance (track t present in frame f, row f - start_t) the camera is moved to the original image as csrc/image_geom.h
does, then `O.project`, `O.rasterize` and `O.shade` say what that person alone would draw.  The persons of a frame are
ordered by a key, descending (ties: lower track index; non-finite keys last): the given priority, else the camera scale
after the move.  A subpixel belongs to the FIRST person in that order whose own rasterisation covers it; it is ambiguous
if ANY person of the frame flags it.  `O.composite` / `O.resize_frame` finish the frame.

The seeded cases of tests/test_gpu_scene.py are built here (`case`), so that tests/test_scene_oracle.py can hold them to
the ambiguity cap without a GPU.  Their keys are bit-identical or differ by more than 1e-3, relatively.
"""
from __future__ import annotations

import functools

import numpy as np

import render_oracle as O


def frame_camera(cam, geom):
    """(camera [s, tx, ty] float32 the projection uses, its scale in float64): csrc/image_geom.h frame_camera."""
    cam = np.asarray(cam, np.float32).reshape(-1)[:3]
    if geom is None:
        return cam.copy(), float(cam[0])
    undo, sx, sy, proc, size = np.asarray(geom, np.float32).astype(np.float64)
    c = cam.astype(np.float64)
    crop_s = proc * c[0] * 0.5
    half = (2.0 / c[0]) * 0.5
    crop_tx, crop_ty = c[1] + half, c[2] + half
    orig_s = crop_s * undo
    orig_tx, orig_ty = crop_tx + (sx - proc) / crop_s, crop_ty + (sy - proc) / crop_s
    k = 2.0 / size
    new = np.array([orig_s * k, orig_tx - 1.0 / (k * orig_s), orig_ty - 1.0 / (k * orig_s)])
    return new.astype(np.float32), float(new[0])


def depth_at(proj_verts, faces, S, index):
    """z' at the centre of every subpixel on its face `index` [2S,2S] (nan where index < 0)."""
    q, zp, area2, _ = O._faces_geometry(proj_verts, faces)
    S2 = 2 * S
    rr, cc = np.nonzero(index >= 0)
    ids = index[rr, cc]
    _, z = O._eval(q[ids], zp[ids], area2[ids], S, (2 * cc + 1 - S2) / S2, (2 * rr + 1 - S2) / S2)
    out = np.full(index.shape, np.nan)
    out[rr, cc] = z
    return out


def _order(keys):
    """[(track, key)] -> tracks, key descending, ties to the lower track, non-finite keys last"""
    return [t for t, k in sorted(keys, key=lambda tk: ((0, -tk[1]) if np.isfinite(tk[1]) else (1, 0.0), tk[0]))]


def render_frame(tracks, f, faces, S, bg_color=(1, 1, 1), frame=None, out_hw=None):
    """Frame f of the scene.  tracks: dicts(verts [m,V,3], cams [m,3], range (start, end), geom [m,5] or None, priority [m]
    or None, color rgb).  -> dict(rgb, alpha, index, owner, ambiguous, pixel_ambiguous, order, solo {track: (index, z')})"""
    S2 = 2 * S
    keys, solo = [], {}
    amb = np.zeros((S2, S2), bool)
    for t, trk in enumerate(tracks):
        start, end = trk["range"]
        if not start <= f < end:
            continue
        r = f - start
        cam, scale = frame_camera(trk["cams"][r], None if trk.get("geom") is None else trk["geom"][r])
        keys.append((t, float(np.float32(trk["priority"][r])) if trk.get("priority") is not None else scale))
        p = O.project(trk["verts"][r], cam)
        idx, a = O.rasterize(p, faces, S)
        amb |= a
        solo[t] = (idx, p, O.shade(p, faces, trk["color"]))
    order = _order(keys)
    index = np.full((S2, S2), -1, np.int64)
    owner = np.full((S2, S2), -1, np.int64)
    comb = np.full((S2, S2), -1, np.int64)           # index into the concatenated colour table
    table = []
    for n, t in enumerate(order):
        idx, _, cols = solo[t]
        take = (owner < 0) & (idx >= 0)
        index[take], owner[take], comb[take] = idx[take], t, idx[take] + n * len(faces)
        table.append(cols)
    table = np.concatenate(table) if table else np.zeros((1, 3))
    bg = O.resize_frame(frame, *(out_hw or (S, S))) if frame is not None else None
    rgb, alpha = O.composite(comb, table, S, bg_color, bg, 'frame' if frame is not None else None, out_hw)
    return {"rgb": rgb, "alpha": alpha, "index": index, "owner": owner, "ambiguous": amb,
            "pixel_ambiguous": O.pixel_ambiguity(amb, S, out_hw), "order": order,
            "solo": {t: (v[0], v[1]) for t, v in solo.items()}}


def render(tracks, faces, S, n_frames, bg_color=(1, 1, 1), frames=None, out_hw=None):
    return [render_frame(tracks, f, faces, S, bg_color, None if frames is None else frames[f], out_hw) for f in range(n_frames)]


# --------------------------------------------------------------------------------------------------- the seeded cases
COLORS = [O.COLORS[c] for c in ('blue', 'pink', 'mint', 'orange')]
RANGES3 = ((0, 4), (1, 6), (3, 5))


def ellipsoid(n_lon, n_rings):
    from human_dynamics_amd.util.render.mesh import latlong_sphere
    v, f = latlong_sphere(n_lon, n_rings)
    return (v * np.array([0.3, 0.55, 0.25], np.float32)).astype(np.float32), f


def out_geometry(frame_hw, max_img):
    """(h', w', S) of video.orig_output_size, restated"""
    h, w = frame_hw
    if max(h, w) > max_img:
        s = max_img / float(max(h, w))
        h, w = int(np.floor(h * s)), int(np.floor(w * s))
    return h, w, max(h, w)


def make_track(rng, v, rng_frames, frame_hw, max_img, centre, cam_s, crop_scale, z_shift, color, drift=1.0):
    """A person as process_image + the network would hand it over: per-frame vertices (they differ per row), crop cameras,
    and the process_image dicts that put the 224 crop's centre at `centre` (x, y; resized-frame pixels, drifting)."""
    from human_dynamics_amd.util.render.handoff import orig_image_geometry
    start, end = rng_frames
    m = end - start
    h, w, _ = out_geometry(frame_hw, max_img)
    scale_orig = h / float(frame_hw[0]) if max(frame_hw) > max_img else 1.0
    verts = np.stack([v * (1 + 0.04 * drift * r) + np.array([0.01 * drift * r, -0.015 * drift * r, z_shift], np.float32)
                      for r in range(m)]).astype(np.float32)
    cams = np.stack([[cam_s * (1 + 0.003 * r), 0.02 * rng.uniform(-1, 1), 0.02 * rng.uniform(-1, 1)] for r in range(m)]).astype(np.float32)
    params = []
    for r in range(m):
        cx, cy = centre[0] + 1.5 * drift * r, centre[1] - 1.0 * drift * r
        params.append({"start_pt": np.array([int(round(cx / scale_orig * crop_scale)) + 112, int(round(cy / scale_orig * crop_scale)) + 112]),
                       "scale": crop_scale, "im_shape": [224, 224]})
    geom = np.stack([orig_image_geometry(p, frame_hw, max_img) for p in params])
    return {"verts": verts, "cams": cams, "range": (start, end), "geom": geom, "priority": None, "color": color,
            "params": params}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(tracks, faces, S, n_frames, frames uint8 [F,H,W,3], out_hw, max_img)"""
    seed = {"three48": 1, "three80": 2, "pair80": 3, "edges48": 4, "slab16": 5, "video80": 6}[name]
    rng = np.random.default_rng(seed)
    drift = 1.0
    if name == "slab16":
        frame_hw, max_img, drift = (40, 64), 16, 0.05    # -> 10 x 16 in the smallest raster, 70 frames: three slabs of 32
        v, faces = ellipsoid(4, 1)                       # 8 faces
    elif name in ("three48", "edges48"):
        frame_hw, max_img = (60, 96), 48                 # -> 30 x 48 in a 48 raster: one full tile + one partial per side
        v, faces = ellipsoid(25, 14)                     # 700 faces: two full LDS batches and a part
    else:
        frame_hw, max_img = (120, 160), 80               # -> 60 x 80 in an 80 raster: three tiles per side
        v, faces = ellipsoid(12, 10)                     # 240 faces
    h, w, S = out_geometry(frame_hw, max_img)
    # crop scales chosen so that the camera scales (the default keys) are about 1.0, 0.8, 0.62: far more than 1e-3 apart;
    # the LARGEST person gets the FARTHEST local z: layering must beat depth
    k = 224.0 * (h / float(frame_hw[0])) / S
    spec = [(0.45, 0.50, 0.90, 0.9 * k / 1.00, +0.6), (0.58, 0.45, 0.85, 0.85 * k / 0.80, -0.5), (0.50, 0.58, 0.80, 0.8 * k / 0.62, 0.0)]
    if name in ("three48", "three80"):
        n_frames, ranges = 6, RANGES3
    elif name == "pair80":
        n_frames, ranges = 2, ((0, 2), (0, 2))
    elif name == "edges48":
        n_frames, ranges = 5, ((1, 3), (2, 4))           # frames 0 and 4 are empty
    elif name == "slab16":
        n_frames, ranges = 70, ((0, 70), (10, 65))
    else:
        n_frames, ranges = 7, ((0, 5), (2, 7))           # two tracks of 5 frames
    tracks = [make_track(rng, v, ranges[t], frame_hw, max_img, (spec[t][0] * w, spec[t][1] * h), spec[t][2], spec[t][3],
                         spec[t][4], COLORS[t], drift) for t in range(len(ranges))]
    frames = rng.integers(0, 256, (n_frames,) + frame_hw + (3,), dtype=np.uint8)
    return {"tracks": tracks, "faces": faces, "S": S, "n_frames": n_frames, "frames": frames, "out_hw": (h, w), "max_img": max_img}


@functools.lru_cache(maxsize=None)
def reference(name, mode="frame", reverse=False):
    """The oracle's frames of a case (computed once per session).  mode 'color': no frame background; reverse: explicit
    priorities that turn the default order round."""
    c = case(name)
    tracks = c["tracks"]
    if reverse:
        tracks = [dict(t, priority=np.full(t["range"][1] - t["range"][0], float(i), np.float32)) for i, t in enumerate(tracks)]
    return render(tracks, c["faces"], c["S"], c["n_frames"], frames=c["frames"] if mode == "frame" else None, out_hw=c["out_hw"])


ORACLE_CASES = [("three48", "frame", False), ("three80", "frame", False), ("three80", "color", False),
                ("pair80", "frame", False), ("pair80", "frame", True), ("edges48", "frame", False)]
