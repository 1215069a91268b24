"""NumPy restatement of csrc/collage.hip: the skeleton's draw list, the three primitives and the 2x2 collage.

The draw list restates src/util/render/render_utils.py:38-234 (pinned to the executed reference by
tests/golden/reference_collage.npz); the primitives are the integer rules of include/hmmr_hip.h -- a specification, not a
measurement of OpenCV; the collage restates src/evaluation/run_video.py:178-197 with oracle.preprocess_oracle's resize.

A draw list is an int64 array [m, 9]: kind (1 disc, 2 ring, 3 line), x0, y0, x1, y1, radius or thickness, r, g, b.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.preprocess_oracle import cv2_resize_linear  # noqa: E402

DISC, RING, LINE = 1, 2, 3
COORD_MIN, COORD_MAX = -32768, 32767

COLORS = {'pink': [197, 27, 125], 'light_pink': [233, 163, 201], 'light_green': [161, 215, 106], 'green': [77, 146, 33],
          'red': [215, 48, 39], 'light_red': [252, 146, 114], 'light_orange': [252, 141, 89], 'orange': [200, 90, 39],
          'purple': [118, 42, 131], 'light_purple': [175, 141, 195], 'light_blue': [145, 191, 219], 'blue': [69, 117, 180],
          'gray': [130, 130, 130], 'white': [255, 255, 255]}
JCOLORS = ['light_pink'] * 3 + ['pink'] * 3 + ['light_blue'] * 3 + ['blue'] * 3 + ['purple', 'purple', 'red', 'green', 'green',
           'white', 'white', 'orange', 'light_orange', 'orange', 'light_orange', 'pink', 'light_pink']
ECOLORS = dict([(c, 'light_pink') for c in (0, 1, 2)] + [(c, 'pink') for c in (3, 4, 5)] + [(c, 'light_blue') for c in (6, 7, 8)] +
               [(c, 'blue') for c in (9, 10, 11)] + [(12, 'purple'), (14, 'purple'), (17, 'light_green'), (18, 'light_green'),
                (19, 'orange'), (20, 'light_orange'), (21, 'orange'), (22, 'light_orange'), (23, 'green'), (24, 'gray')])
PARENTS = {19: [1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16],
           25: [24, 2, 8, 9, 3, 23, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16, 23, 24, 19, 20, 4, 1]}


def crop_from_bytes(u8):
    """a crop in [-1, 1] from byte values (the fixture stores the bytes of its crops)"""
    return (u8 / np.float32(127.5) - np.float32(1)).astype(np.float32)


def radius_rule(h, w):
    return max(4, int(np.mean([h, w]) * 0.01))


def pixel_joints(kp, kp_add=0.0, kp_mul=1.0):
    """[K,2] float32 -> (int64 [K,2], finite [K]): (kp + add) * mul in float32, half to even, clamped as the kernel does"""
    v = (np.asarray(kp, np.float32) + np.float32(kp_add)) * np.float32(kp_mul)
    ok = ~np.isnan(v).any(1)
    with np.errstate(invalid="ignore"):
        r = np.clip(np.round(np.where(np.isnan(v), np.float32(0), v)), COORD_MIN, COORD_MAX).astype(np.int64)
    return r, ok


def draw_list(joints, radius, draw_edges=True, vis=None):
    """joints: int [K,2] (K = 19 or 25), vis: [K] or None -> the draw list in painter's order"""
    joints = np.asarray(joints)
    nk = len(joints)
    parents = PARENTS[nk]
    seen = np.ones(nk, bool) if vis is None else np.asarray(vis) != 0
    out = []
    for child in range(nk):
        if not seen[child]:
            continue
        x, y = (int(v) for v in joints[child])
        if not draw_edges:
            out.append([RING, x, y, x, y, radius - 1] + COLORS[JCOLORS[child]])
            continue
        out.append([DISC, x, y, x, y, radius] + COLORS['white'])
        out.append([DISC, x, y, x, y, radius - 1] + COLORS[JCOLORS[child]])
        pa = parents[child]
        if pa >= 0 and seen[pa]:
            px, py = (int(v) for v in joints[pa])
            out.append([DISC, px, py, px, py, radius - 1] + COLORS[JCOLORS[pa]])
            out.append([LINE, x, y, px, py, radius - 2] + COLORS[ECOLORS[child]])
    return np.array(out, np.int64).reshape(-1, 9)


def disc_mask(h, w, cx, cy, r):
    if r < 0:
        return np.zeros((h, w), bool)
    dy, dx = np.mgrid[0:h, 0:w].astype(np.int64)
    dx, dy = dx - cx, dy - cy
    return dx * dx + dy * dy <= r * r + r


def line_mask(h, w, x0, y0, x1, y1, t):
    """4 dist^2(q, segment) <= t^2 as the kernel evaluates it: the clamped ends by distance to the end point, the middle
    by the cross product (|a L - (a.d) d|^2 = L (a x d)^2); equal to the header's formula in exact integers"""
    ay, ax = np.mgrid[0:h, 0:w].astype(np.int64)
    ax, ay = ax - x0, ay - y0
    dx, dy = int(x1 - x0), int(y1 - y0)
    L = dx * dx + dy * dy
    s = ax * dx + ay * dy
    cr = ax * dy - ay * dx
    near = np.abs(cr) < (1 << 27)
    mid = near & (4 * np.where(near, cr, 0) ** 2 <= t * t * L)
    return np.where(s <= 0, 4 * (ax * ax + ay * ay) <= t * t,
                    np.where(s >= L, 4 * ((ax - dx) ** 2 + (ay - dy) ** 2) <= t * t, mid))


def prim_mask(h, w, prim):
    kind, x0, y0, x1, y1, r = (int(v) for v in prim[:6])
    if kind == DISC:
        return disc_mask(h, w, x0, y0, r)
    if kind == RING:
        return disc_mask(h, w, x0, y0, r) & ~disc_mask(h, w, x0, y0, r - 1)
    return line_mask(h, w, x0, y0, x1, y1, r)


def rasterise(img_u8, prims):
    """-> (image, covered [h,w]): the primitives painted in order over a copy of the uint8 image"""
    out = np.array(img_u8, np.uint8)
    h, w = out.shape[:2]
    covered = np.zeros((h, w), bool)
    for p in prims:
        m = prim_mask(h, w, p)
        out[m] = p[6:9]
        covered |= m
    return out, covered


def draw_skeleton(input_image, joints, draw_edges=True, vis=None, radius=None):
    """render_utils.draw_skeleton -> (image in the reference's dtype conventions, draw list, covered mask)"""
    if radius is None:
        radius = radius_rule(*input_image.shape[:2])
    image = np.array(input_image)
    is_float = image.dtype in (np.float32, np.float64)
    if is_float:
        max_val = image.max()
        image = (image * 255).astype(np.uint8) if max_val <= 2. else image.astype(np.uint8)
    joints = np.asarray(joints)
    if joints.shape[0] != 2:
        joints = joints.T
    j = np.clip(np.round(joints), COORD_MIN, COORD_MAX).astype(np.int64).T
    prims = draw_list(j, int(radius), draw_edges, vis)
    image, covered = rasterise(image, prims)
    if is_float:
        image = image.astype(np.float32) / 255. if max_val <= 1. else image.astype(np.float32)
    return image, prims, covered


def collage_width(S, h, w):
    return S + max(w * S // h, S)


def compose(rend_crop, skel_crop, render_og, rot_og):
    """uint8 panels [S,S,3], [S,S,3], [h,w,3], [h,w,3] -> the uint8 collage frame, through the reference's floats"""
    S = rend_crop.shape[0]
    rend_f = rend_crop / 255
    skel_f = skel_crop.astype(np.float32) / 255             # draw_skeleton hands back float32
    h, w, _ = render_og.shape
    w2 = w * S // h
    og = cv2_resize_linear(render_og / 255, (w2, S))
    rot = cv2_resize_linear(rot_og / 255, (S, S))
    padding = np.ones((S, abs(w2 - S), 3))
    if w2 > S:
        rot = np.hstack((rot, padding))
    else:
        og = np.hstack((og, padding))
    frame = np.hstack((np.vstack((rend_f, skel_f)), np.vstack((og, rot))))
    return (frame * 255).astype(np.uint8)                   # plt.imsave's float-to-bytes


def resize_footprint(mask, h2, w2):
    """every pixel of the (w2, h2) resize whose taps touch a masked input pixel"""
    from oracle.preprocess_oracle import _taps
    x0, x1, _, _ = _taps(mask.shape[1], w2)
    y0, y1, _, _ = _taps(mask.shape[0], h2)
    cols = mask[:, x0] | mask[:, x1]
    return cols[y0] | cols[y1]
