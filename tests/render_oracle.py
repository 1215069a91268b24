"""NumPy brute-force rasteriser: the spec of csrc/render.hip (include/hmmr_hip.h: hmmr_render_mesh), in float64.

What the reference's VisRenderer (src/util/render/nmr_renderer.py) asks of neural_renderer: camera_mode='look_at',
perspective=False, viewing angle 30 deg (eye at z = -2.7320508 looking at the origin, so z' = z + 2.7320508), near/far
0.1 / 100, fill_back with back-face culling (every face drawn once, shaded with its viewer-facing normal), and
anti-aliasing by a 2x2 mean over a 2S x 2S grid of subpixels.

* subpixel (c, r) has centre u = (2c+1-2S)/2S, v = (2r+1-2S)/2S and is covered by a face whose unflipped projected
  triangle q = (p.x, -p.y) contains (u, v), edges included;
* depth z'_p = 1 / sum(w_i / z'_i) with screen-space barycentrics w_i, drawn only in [0.1, 100]; the nearest wins, ties
  go to the lower face index; faces with a non-finite vertex or zero area draw nothing;
* colour = tex (I_amb c_amb + I_dir c_dir max(0, n . d)), n = normalize(cross(p0-p1, p2-p1)) (|n| floored at 1e-5)
  turned so that n_z <= 0;
* pixel = mean of its four subpixels (background colour where uncovered), rend = clip(., 0, 1) 255 in fp32,
  alpha = covered / 4, out = trunc(bg (1 - alpha) + rend alpha) (trunc(rend) without a background image).

Every subpixel also gets an ambiguity flag: its centre lies within `tol_edge` subpixels of an edge of a face that could
decide it, two candidate depths are within `tol_depth` (relative), or its depth is that close to near / far.  There an
fp32 implementation may legitimately differ from this float64 one; everywhere else it must agree.
"""
from __future__ import annotations

import numpy as np

EYE_Z = np.float32(2.7320508075688772)           # 1 / tan(30 deg) + 1
NEAR, FAR = 0.1, 100.0
TOL_EDGE = 1e-3                                  # subpixels (fp32 edge tests err by ~1e-4 at S = 720)
TOL_DEPTH = 1e-5                                 # relative

COLORS = {
    'blue': [0.65098039, 0.74117647, 0.85882353],
    'pink': [.9, .7, .7],
    'mint': [166 / 255., 229 / 255., 204 / 255.],
    'mint2': [202 / 255., 229 / 255., 223 / 255.],
    'green': [153 / 255., 216 / 255., 201 / 255.],
    'green2': [171 / 255., 221 / 255., 164 / 255.],
    'red': [251 / 255., 128 / 255., 114 / 255.],
    'orange': [253 / 255., 174 / 255., 97 / 255.],
    'yellow': [250 / 255., 230 / 255., 154 / 255.],
}


def project(verts, cam):
    """VisRenderer.__call__'s projection in fp32: [s (x + tx), -s (y + ty), z]."""
    v = np.asarray(verts, np.float32)
    c = np.asarray(cam, np.float32).reshape(3)
    out = np.empty_like(v)
    out[:, 0] = c[0] * (v[:, 0] + c[1])
    out[:, 1] = -(c[0] * (v[:, 1] + c[2]))
    out[:, 2] = v[:, 2]
    return out


def rodrigues(deg, axis='y'):
    """cv2.Rodrigues(deg2rad(deg) * axis) in float64 (cos 90 deg is 6.1e-17, not 0)."""
    k = {'y': [0, 1., 0], 'x': [1., 0, 0]}.get(axis, [0, 0, 1.])
    r = np.deg2rad(deg) * np.asarray(k, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def rotate(verts, R):
    """VisRenderer.rotated: about the fp32 centroid, R rounded to fp32."""
    v = np.asarray(verts, np.float32)
    c = v.mean(0, dtype=np.float32)
    return ((v - c) @ np.asarray(R, np.float32).T + c).astype(np.float32)


def shade(proj_verts, faces, color=COLORS['blue'], face_colors=None, light_dir=(1, .5, -1), int_dir=0.3, int_amb=0.7,
          col_dir=(1, 1, 1), col_amb=(1, 1, 1)):
    p = np.asarray(proj_verts, np.float64)[np.asarray(faces)]
    n = np.cross(p[:, 0] - p[:, 1], p[:, 2] - p[:, 1])
    n[n[:, 2] > 0] *= -1
    n = n / np.maximum(np.linalg.norm(n, axis=1), 1e-5)[:, None]
    cos = np.maximum(0.0, n @ np.asarray(light_dir, np.float64))
    tex = np.asarray(face_colors, np.float64) if face_colors is not None else np.tile(np.asarray(color, np.float64), (len(p), 1))
    light = int_amb * np.asarray(col_amb, np.float64)[None] + int_dir * np.asarray(col_dir, np.float64)[None] * cos[:, None]
    return tex * light


def _faces_geometry(proj_verts, faces):
    p = np.asarray(proj_verts, np.float32)[np.asarray(faces)]            # [F,3,3]
    q = np.stack([p[..., 0], -p[..., 1]], -1).astype(np.float64)        # unflipped camera
    zp = (p[..., 2] + EYE_Z).astype(np.float64)                         # fp32 shift, as NMR's look_at
    area2 = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(p).all(axis=(1, 2)) & np.isfinite(area2) & (area2 != 0)
    return q, zp, area2, valid


def _eval(q, zp, area2, S, u, v):
    """q [F,3,2] against points (u, v) [...]: signed distance to the nearest edge in subpixels (> 0 inside) and z'_p."""
    w, dist = [], []
    sg = np.sign(area2)
    for i in range(3):
        a, b = q[..., (i + 1) % 3, :], q[..., (i + 2) % 3, :]
        e = (a[..., 0] - u) * (b[..., 1] - v) - (a[..., 1] - v) * (b[..., 0] - u)
        w.append(e / area2)
        ln = np.hypot(b[..., 0] - a[..., 0], b[..., 1] - a[..., 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            dist.append(np.where(ln > 0, sg * e / ln * S, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = 1.0 / (w[0] / zp[..., 0] + w[1] / zp[..., 1] + w[2] / zp[..., 2])
    return np.minimum(np.minimum(dist[0], dist[1]), dist[2]), z


class _Acc:
    def __init__(self, shape):
        self.idx = np.full(shape, -1, np.int64)
        self.z1 = np.full(shape, np.inf)            # depth of the winner
        self.z2 = np.full(shape, np.inf)            # next depth among certain coverers
        self.zamb = np.full(shape, np.inf)          # nearest depth among faces whose edge passes within tol
        self.amb = np.zeros(shape, bool)

    def update(self, sel, fid, dmin, z, tol_edge, tol_depth):
        with np.errstate(invalid="ignore"):
            inr = (z >= NEAR) & (z <= FAR)
            near_lim = np.isfinite(z) & ((np.abs(z - NEAR) <= tol_depth * NEAR) | (np.abs(z - FAR) <= tol_depth * FAR))
        cand = dmin > -tol_edge
        self.amb[sel] |= cand & near_lim
        edge = cand & (dmin < tol_edge) & (inr | near_lim)
        zz = np.where(edge, z, np.inf)
        self.zamb[sel] = np.minimum(self.zamb[sel], zz)
        cov = (dmin >= 0) & inr
        z1, z2, idx = self.z1[sel], self.z2[sel], self.idx[sel]
        zc = np.where(cov, z, np.inf)
        win = zc < z1
        z2n = np.where(win, z1, np.minimum(z2, zc))
        self.z1[sel] = np.where(win, zc, z1)
        self.z2[sel] = z2n
        self.idx[sel] = np.where(win, fid, idx)

    def finish(self, tol_depth):
        amb = self.amb | (np.isfinite(self.zamb) & (self.zamb <= self.z1 * (1 + tol_depth)))
        with np.errstate(invalid="ignore"):
            amb |= np.isfinite(self.z2) & (self.z2 - self.z1 <= tol_depth * self.z1)
        return self.idx, amb


def rasterize(proj_verts, faces, S, tol_edge=TOL_EDGE, tol_depth=TOL_DEPTH):
    """Whole 2S x 2S grid: (face index [2S,2S] int64, -1 uncovered; ambiguity mask [2S,2S])."""
    q, zp, area2, valid = _faces_geometry(proj_verts, faces)
    S2 = 2 * S
    acc = _Acc((S2, S2))
    for f in np.nonzero(valid)[0]:
        lo, hi = q[f].min(0), q[f].max(0)
        c0, c1 = int(np.floor(lo[0] * S + S - 0.5)) - 1, int(np.ceil(hi[0] * S + S - 0.5)) + 1
        r0, r1 = int(np.floor(lo[1] * S + S - 0.5)) - 1, int(np.ceil(hi[1] * S + S - 0.5)) + 1
        c0, r0, c1, r1 = max(c0, 0), max(r0, 0), min(c1, S2 - 1), min(r1, S2 - 1)
        if c0 > c1 or r0 > r1:
            continue
        cc, rr = np.arange(c0, c1 + 1), np.arange(r0, r1 + 1)
        u = ((2 * cc + 1 - S2) / S2)[None, :]
        v = ((2 * rr + 1 - S2) / S2)[:, None]
        dmin, z = _eval(q[f], zp[f], area2[f], S, u, v)
        sel = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        acc.update(sel, f, dmin, z, tol_edge, tol_depth)
    return acc.finish(tol_depth)


def rasterize_points(proj_verts, faces, S, rows, cols, tol_edge=TOL_EDGE, tol_depth=TOL_DEPTH, chunk=256):
    """Only the subpixels (rows[k], cols[k]): for scenes whose faces span the image (the synthetic SMPL's soup)."""
    q, zp, area2, valid = _faces_geometry(proj_verts, faces)
    S2 = 2 * S
    u = (2 * np.asarray(cols) + 1 - S2) / S2
    v = (2 * np.asarray(rows) + 1 - S2) / S2
    acc = _Acc(u.shape)
    ids = np.nonzero(valid)[0]
    for s in range(0, len(ids), chunk):
        fs = ids[s:s + chunk]
        dmin, z = _eval(q[fs][:, None], zp[fs][:, None], area2[fs][:, None], S, u[None], v[None])
        for k, f in enumerate(fs):                 # in index order: ties keep the lower index
            acc.update(slice(None), f, dmin[k], z[k], tol_edge, tol_depth)
    return acc.finish(tol_depth)


def resize_frame(frame_u8, out_h, out_w):
    """visualize_img_orig's image: ((frame / 255) - 0.5) * 2, cv2.resize INTER_LINEAR to (out_h, out_w) with the taps of
    csrc/image_geom.h (float32 coordinates and weights, float64 sums), then ((img + 1) / 2) 255, float64."""
    fr = ((np.asarray(frame_u8, np.float64) / 255.) - 0.5) * 2
    H, W = fr.shape[:2]

    def taps(n_dst, n_src):
        d = np.arange(n_dst)
        f = (((d + 0.5) * (n_src / n_dst)) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = (f - s.astype(np.float32)).astype(np.float32)
        lo, hi = s < 0, s >= n_src - 1
        f[lo | hi] = 0
        s[lo] = 0
        s[hi] = n_src - 1
        return s, np.minimum(s + 1, n_src - 1), (np.float32(1) - f).astype(np.float64), f.astype(np.float64)
    x0, x1, a0, a1 = taps(out_w, W)
    y0, y1, b0, b1 = taps(out_h, H)
    r0 = fr[y0][:, x0] * a0[None, :, None] + fr[y0][:, x1] * a1[None, :, None]
    r1 = fr[y1][:, x0] * a0[None, :, None] + fr[y1][:, x1] * a1[None, :, None]
    img = r0 * b0[:, None, None] + r1 * b1[:, None, None]
    return ((img + 1) * 0.5) * 255.


def pool(index, colors, S, bg_color=(1, 1, 1)):
    """NMR's anti-aliased images before any clipping: (rgb float32 [S,S,3], alpha float32 [S,S])."""
    colors = np.asarray(colors, np.float32)
    sub = np.where(index[..., None] >= 0, colors[np.maximum(index, 0)], np.asarray(bg_color, np.float32)[None, None])
    sub = sub.astype(np.float32).reshape(S, 2, S, 2, 3)
    pooled = ((sub[:, 0, :, 0] + sub[:, 0, :, 1]) + (sub[:, 1, :, 0] + sub[:, 1, :, 1])) * np.float32(0.25)
    alpha = ((index >= 0).reshape(S, 2, S, 2).sum(axis=(1, 3)) * 0.25).astype(np.float32)
    return pooled, alpha


def composite(index, colors, S, bg_color=(1, 1, 1), bg=None, bg_kind=None, out_hw=None):
    """Subpixel face map [2S,2S] + per-face colours -> (rgb uint8 [h,w,3], alpha float32 [h,w]).
    bg_kind None: no image; 'float': bg = float32 image already in [0, 255] terms (fp32 composite); 'frame': float64
    image of resize_frame (float64 composite, as visualize_img_orig's float64 image)."""
    pooled, alpha = pool(index, colors, S, bg_color)
    rend = (np.clip(pooled, 0, 1) * np.float32(255.0)).astype(np.float32)
    h, w = out_hw if out_hw is not None else (S, S)
    rend, alpha = rend[:h, :w], alpha[:h, :w]
    a3 = alpha[..., None]
    if bg_kind is None:
        out = rend
    elif bg_kind == 'float':
        out = np.asarray(bg, np.float32)[:h, :w] * (np.float32(1) - a3) + rend * a3
    else:
        out = np.asarray(bg, np.float64)[:h, :w] * (np.float32(1) - a3).astype(np.float64) + (rend * a3).astype(np.float64)
    return out.astype(np.uint8), alpha


def pixel_ambiguity(amb_sub, S, out_hw=None):
    """A pixel is ambiguous if any of its four subpixels is."""
    a = amb_sub.reshape(S, 2, S, 2).any(axis=(1, 3))
    h, w = out_hw if out_hw is not None else (S, S)
    return a[:h, :w]


def render(proj_verts, faces, S, color=COLORS['blue'], face_colors=None, bg_color=(1, 1, 1), bg=None, bg_kind=None,
           out_hw=None, light=None):
    """The whole spec for one frame: dict(rgb, alpha, index [2S,2S], ambiguous [2S,2S], pixel_ambiguous [h,w])."""
    idx, amb = rasterize(proj_verts, faces, S)
    cols = shade(proj_verts, faces, color, face_colors, **(light or {}))
    rgb, alpha = composite(idx, cols, S, bg_color, bg, bg_kind, out_hw)
    return {"rgb": rgb, "alpha": alpha, "index": idx, "ambiguous": amb, "pixel_ambiguous": pixel_ambiguity(amb, S, out_hw)}
