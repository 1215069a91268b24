"""ctypes front of the rasteriser (csrc/render.hip, include/hmmr_hip.h: hmmr_render_mesh).

`render_mesh` renders n frames of one mesh topology in one call (slabs of RENDER_MAX_FRAMES for longer inputs) and
returns device tensors; `MeshFaces` holds a face set, checked once against the vertex count, with its device copy.
`render_scene` (hmmr_render_scene) renders all person tracks of a video into each frame, layered by a per-frame key.
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


SCENE_COLORS = ('blue', 'pink', 'mint', 'orange', 'yellow', 'green', 'red', 'mint2', 'green2')   # the default cycle, by track


def scene_color(i, colors=None):
    """rgb of track i: colors[i] (a COLORS name or an rgb triple) where given, else SCENE_COLORS cycled in that order."""
    c = colors[i] if colors is not None else SCENE_COLORS[i % len(SCENE_COLORS)]
    return COLORS[c] if isinstance(c, str) else [float(v) for v in np.asarray(c, np.float64).reshape(3)]


def render_scene(tracks, faces, size, n_frames, colors=None, bg_color=(1., 1., 1.), light_dir=(1, .5, -1), int_dir=0.3,
                 int_amb=0.7, col_dir=(1, 1, 1), col_amb=(1, 1, 1), bg_mode=L.RENDER_BG_COLOR, bg_image=None, out_hw=None,
                 want_alpha=False, want_index=False, want_owner=False, stream=None):
    """All persons of every frame in one raster (include/hmmr_hip.h: hmmr_render_scene), 1 .. 16 tracks of one topology.

    tracks: per track a dict(verts [m,V,3] or [m, >= 3V] rows, cams [m, >= 3], range=(start, end) with m = end - start,
    geom=None or [m,5], priority=None or [m] float keys) of device tensors read in place; row f - start is the person in
    frame f.  A frame's persons are layered by priority (else by the camera scale the projection uses), descending, ties
    to the lower track index; the first one covering a subpixel owns it.  colors: see `scene_color`.
    bg_mode: L.RENDER_BG_COLOR or L.RENDER_BG_FRAME (bg_image uint8 [n_frames,H,W,3], resized to out_hw).
    -> dict(rgb uint8 [F,h,w,3], alpha float32 [F,h,w] or None, index / owner int32 [F,2S,2S] or None), on the device."""
    lib = L.load()
    if not isinstance(faces, MeshFaces):
        faces = MeshFaces(faces)
    n_frames, size = int(n_frames), int(size)
    if not 1 <= len(tracks) <= L.SCENE_MAX_TRACKS:
        raise ValueError("%d tracks: the scene view takes 1 .. %d" % (len(tracks), L.SCENE_MAX_TRACKS))
    if not 1 <= n_frames <= L.RENDER_MAX_FRAMES:
        raise ValueError("%d frames: one call takes 1 .. %d (render longer videos in chunks)" % (n_frames, L.RENDER_MAX_FRAMES))
    dev = tracks[0]["verts"].device
    if dev.type != "cuda":
        raise L.HmmrError("render_scene needs device tensors (the HIP library has no CPU path)")
    arr = (L.SceneTrack * len(tracks))()
    keep, nv = [], None
    for i, trk in enumerate(tracks):
        start, end = (int(x) for x in trk["range"])
        m = end - start
        verts = trk["verts"]
        if m < 1 or verts.shape[0] != m or trk["cams"].shape[0] != m:
            raise ValueError("track %d: range (%d, %d) for %d verts rows and %d cams rows"
                             % (i, start, end, verts.shape[0], trk["cams"].shape[0]))
        v2, c2 = _rows(verts, m), _rows(trk["cams"], m)
        nvi = v2.shape[1] // 3 if verts.dim() == 2 else verts.shape[1]
        if nv is not None and nvi != nv:
            raise ValueError("track %d has %d vertices, track 0 has %d: one topology per scene" % (i, nvi, nv))
        nv = nvi
        t = arr[i]
        t.verts, t.ld_verts, t.cams, t.ld_cam = v2.data_ptr(), _ld(v2), c2.data_ptr(), _ld(c2)
        keep += [v2, c2]
        if trk.get("geom") is not None:
            g = torch.as_tensor(np.asarray(trk["geom"], np.float64).reshape(m, 5), dtype=torch.float32).to(dev)
            t.geom = g.data_ptr()
            keep.append(g)
        if trk.get("priority") is not None:
            p = trk["priority"]
            p = (p if torch.is_tensor(p) else torch.as_tensor(np.asarray(p, np.float32))).to(dev).float().contiguous()
            if p.numel() != m:
                raise ValueError("track %d: %d priority keys for %d rows" % (i, p.numel(), m))
            t.priority = p.data_ptr()
            keep.append(p)
        t.start, t.end = start, end
        t.color = _f3(scene_color(i, colors))
    if faces.max_index >= nv:
        raise ValueError("face index %d >= %d vertices" % (faces.max_index, nv))
    h, w = (size, size) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    fdev = faces.device(dev)
    img = None
    if bg_mode == L.RENDER_BG_FRAME:
        img = torch.as_tensor(bg_image, device=dev)
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[0] != n_frames or img.shape[3] != 3:
            raise ValueError("a frame background must be uint8 [n_frames, H, W, 3]")
        img = img.contiguous()
    rgb = torch.empty((n_frames, h, w, 3), dtype=torch.uint8, device=dev)
    alpha = torch.empty((n_frames, h, w), dtype=torch.float32, device=dev) if want_alpha else None
    index = torch.empty((n_frames, 2 * size, 2 * size), dtype=torch.int32, device=dev) if want_index else None
    owner = torch.empty((n_frames, 2 * size, 2 * size), dtype=torch.int32, device=dev) if want_owner else None
    ws = torch.empty(int(lib.hmmr_render_scene_workspace_bytes(n_frames, len(tracks), nv, len(faces))), dtype=torch.uint8, device=dev)
    d = L.SceneDesc()
    d.tracks, d.n_tracks, d.faces = arr, len(tracks), fdev.data_ptr()
    d.nv, d.nf, d.n_frames, d.size, d.out_h, d.out_w = nv, len(faces), n_frames, size, h, w
    d.bg_color, d.light_dir = _f3(bg_color), _f3(light_dir)
    d.light_int_ambient, d.light_int_directional = float(int_amb), float(int_dir)
    d.light_color_ambient, d.light_color_directional = _f3(col_amb), _f3(col_dir)
    d.bg_mode = int(bg_mode)
    if img is not None:
        d.bg_image, d.frame_h, d.frame_w = img.data_ptr(), int(img.shape[1]), int(img.shape[2])
    d.rgb = rgb.data_ptr()
    d.alpha = alpha.data_ptr() if alpha is not None else None
    d.face_index = index.data_ptr() if index is not None else None
    d.owner = owner.data_ptr() if owner is not None else None
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.hmmr_render_scene(C.byref(d), st), "hmmr_render_scene")
    return {"rgb": rgb, "alpha": alpha, "index": index, "owner": owner}
