"""ctypes front of the rasteriser (csrc/render.hip, include/hmmr_hip.h: hmmr_render_mesh).

`render_mesh` renders n frames of one mesh topology in one call (slabs of RENDER_MAX_FRAMES for longer inputs) and
returns device tensors; `MeshFaces` holds a face set, checked once against the vertex count, with its device copy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ... import _lib as L

COLORS = {                                   # src/util/render/nmr_renderer.py
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


def rodrigues(deg, axis='y'):
    """cv2.Rodrigues(np.deg2rad(deg) * axis)[0] (VisRenderer.rotated) in float64: cos 90 deg stays 6.1e-17."""
    k = {'y': [0, 1., 0], 'x': [1., 0, 0]}.get(axis, [0, 0, 1.])
    r = np.deg2rad(deg) * np.asarray(k, np.float64)
    th = float(np.linalg.norm(r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


class MeshFaces(object):
    """A face set [F,3]: validated once (range, count) and kept on each device it is used on."""

    def __init__(self, faces):
        f = np.asarray(faces)
        if f.ndim == 3 and f.shape[0] == 1:
            f = f[0]
        if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
            raise ValueError("faces must be an integer array [F, 3], got %s %s" % (f.dtype, f.shape))
        if not 1 <= len(f) <= L.RENDER_MAX_FACES:
            raise ValueError("%d faces: the rasteriser takes 1 .. %d" % (len(f), L.RENDER_MAX_FACES))
        if f.min() < 0:
            raise ValueError("negative face index")
        self.np = f.astype(np.int32)
        self.max_index = int(f.max())
        self._dev = {}

    def __len__(self):
        return len(self.np)

    def device(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = torch.as_tensor(self.np, device=dev).contiguous()
        return self._dev[key]


def _rows(t, n):
    t2 = t.reshape(n, -1) if t.dim() != 2 else t
    if t2.dtype != torch.float32 or t2.stride(1) != 1:
        t2 = t2.float().contiguous()
    return t2


def _ld(t2):
    """row stride in floats; a single row may carry any stride (numpy's [None] gives 0), the row length is what counts"""
    return t2.stride(0) if t2.shape[0] > 1 else t2.shape[1]


def _f3(x):
    return (C.c_float * 3)(*[float(v) for v in np.asarray(x, np.float64).reshape(3)])


def render_mesh(verts, cams, faces, size, geom=None, rot=None, color=COLORS['blue'], face_colors=None,
                bg_color=(1., 1., 1.), light_dir=(1, .5, -1), int_dir=0.3, int_amb=0.7, col_dir=(1, 1, 1),
                col_amb=(1, 1, 1), bg_mode=L.RENDER_BG_COLOR, bg_image=None, bg_add=0.0, bg_mul=1.0, out_hw=None,
                want_alpha=False, want_index=False, stream=None):
    """verts [n,V,3] (or [n, >= 3V] rows, e.g. the verts field of packed records) and cams [n, >= 3] on the device ->
    dict(rgb uint8 [n,h,w,3], alpha float32 [n,h,w] or None, index int32 [n,2S,2S] or None), on the device.

    geom [n,5]: move the cameras to the original image first (handoff.orig_image_geometry rows); rot [3,3]: rotate about
    the centroid (VisRenderer.rotated); bg_mode / bg_image: L.RENDER_BG_FLOAT (float [n,S,S,3], value (img + bg_add) *
    bg_mul) or L.RENDER_BG_FRAME (uint8 [n,H,W,3] original frames, resized to out_hw); out_hw: the top-left of the S x S
    raster to keep (remove_pads)."""
    lib = L.load()
    if not isinstance(faces, MeshFaces):
        faces = MeshFaces(faces)
    dev = verts.device
    if dev.type != "cuda":
        raise L.HmmrError("render_mesh needs device tensors (the HIP library has no CPU path)")
    n = verts.shape[0]
    v2 = _rows(verts, n)
    nv = v2.shape[1] // 3 if verts.dim() == 2 else verts.shape[1]
    if faces.max_index >= nv:
        raise ValueError("face index %d >= %d vertices" % (faces.max_index, nv))
    c2 = _rows(cams, n)
    size = int(size)
    h, w = (size, size) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    fdev = faces.device(dev)
    fc = None
    if face_colors is not None:
        fc = torch.as_tensor(np.asarray(face_colors, np.float32) if not torch.is_tensor(face_colors) else face_colors,
                             device=dev).float().contiguous()
        if fc.numel() not in (len(faces) * 3, n * len(faces) * 3):
            raise ValueError("face_colors must be [F,3] or [n,F,3]")
    g = None
    if geom is not None:
        g = torch.as_tensor(np.asarray(geom, np.float64).reshape(n, 5), dtype=torch.float32).to(dev)
    img = None
    if bg_mode == L.RENDER_BG_FLOAT:
        img = torch.as_tensor(bg_image, device=dev).float().contiguous()
        if tuple(img.shape) != (n, size, size, 3):
            raise ValueError("a float background must be [n, S, S, 3] = %s, got %s" % ((n, size, size, 3), tuple(img.shape)))
    elif bg_mode == L.RENDER_BG_FRAME:
        img = torch.as_tensor(bg_image, device=dev)
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[0] != n or img.shape[3] != 3:
            raise ValueError("a frame background must be uint8 [n, H, W, 3]")
        img = img.contiguous()
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    alpha = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_alpha else None
    index = torch.empty((n, 2 * size, 2 * size), dtype=torch.int32, device=dev) if want_index else None
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    step = L.RENDER_MAX_FRAMES
    ws = torch.empty(int(lib.hmmr_render_workspace_bytes(min(n, step), nv, len(faces))), dtype=torch.uint8, device=dev)
    for a in range(0, n, step):
        m = min(step, n - a)
        d = L.RenderDesc()
        d.verts, d.ld_verts = v2[a].data_ptr(), _ld(v2)
        d.cams, d.ld_cam = c2[a].data_ptr(), _ld(c2)
        d.geom = g[a].data_ptr() if g is not None else None
        d.faces = fdev.data_ptr()
        if fc is not None:
            per_frame = fc.numel() != len(faces) * 3
            d.face_colors = fc.data_ptr() + (a * len(faces) * 3 * 4 if per_frame else 0)
            d.ld_face_colors = len(faces) * 3 if per_frame else 0
        d.n, d.nv, d.nf, d.size = m, nv, len(faces), size
        if rot is not None:
            d.rotate = 1
            d.rot = (C.c_float * 9)(*[float(x) for x in np.asarray(rot, np.float32).reshape(9)])
        d.color, d.bg_color, d.light_dir = _f3(color), _f3(bg_color), _f3(light_dir)
        d.light_int_ambient, d.light_int_directional = float(int_amb), float(int_dir)
        d.light_color_ambient, d.light_color_directional = _f3(col_amb), _f3(col_dir)
        d.bg_mode = int(bg_mode)
        if img is not None:
            d.bg_image = img[a].data_ptr()
        d.bg_add, d.bg_mul = float(bg_add), float(bg_mul)
        if bg_mode == L.RENDER_BG_FRAME:
            d.frame_h, d.frame_w = int(img.shape[1]), int(img.shape[2])
        d.out_h, d.out_w = h, w
        d.rgb = rgb[a].data_ptr()
        d.alpha = alpha[a].data_ptr() if alpha is not None else None
        d.face_index = index[a].data_ptr() if index is not None else None
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
        L.check(lib.hmmr_render_mesh(C.byref(d), st), "hmmr_render_mesh")
    return {"rgb": rgb, "alpha": alpha, "index": index}
