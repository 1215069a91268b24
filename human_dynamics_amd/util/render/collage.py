"""ctypes front of csrc/collage.hip (include/hmmr_hip.h: hmmr_draw_skeleton, hmmr_compose_collage): the 2D skeleton panel of
src/util/render/render_utils.py:38-234 and the 2x2 collage of src/evaluation/run_video.py:178-197.

The draw list (which discs, rings and lines, in which order, at which integers, in which colours) is the reference's, pinned
by executing it.  The pixels of each primitive follow the integer rules of the header, not OpenCV's scan conversion:
agreement with cv2.circle / cv2.line at primitive boundaries has not been measured.  `draw_text` is not provided.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ... import _lib as L
from .raster import _ld, _rows

COORD_MIN, COORD_MAX = -32768, 32767


def _stream(dev, stream):
    return stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream


def skeleton_panels(kps, bg, nk=None, kp_add=0.0, kp_mul=1.0, vis=None, draw_edges=True, radius=None, bg_add=0.0, bg_mul=1.0,
                    out=None, stream=None):
    """The batched device form.  kps: float32 [n,nk,2], or [n, >= 2 nk] rows read in place (the kps field of packed records;
    then give nk); joint = rint((kp + kp_add) * kp_mul).  bg: float32 [n,h,w,3], drawn over trunc((bg + bg_add) * bg_mul), or
    uint8 [n,h,w,3] (out=bg draws in place).  vis: [n,nk], 0 = invisible.  -> uint8 [n,h,w,3] on the device."""
    lib = L.load()
    dev = bg.device
    if dev.type != "cuda" or kps.device != dev:
        raise L.HmmrError("skeleton_panels needs device tensors (the HIP library has no CPU path)")
    n, h, w = int(bg.shape[0]), int(bg.shape[1]), int(bg.shape[2])
    if bg.dim() != 4 or bg.shape[3] != 3 or bg.dtype not in (torch.float32, torch.uint8):
        raise ValueError("the background must be float32 or uint8 [n, h, w, 3]")
    if kps.dim() == 3:
        nk = int(kps.shape[1]) if nk is None else nk
    if nk is None:
        raise ValueError("rows of keypoints need nk")
    k2 = _rows(kps, n)
    if k2.shape[0] != n:
        raise ValueError("%d rows of keypoints for %d images" % (k2.shape[0], n))
    bg = bg.contiguous()
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 [n, h, w, 3]")
    v = None
    if vis is not None:
        v = (torch.as_tensor(np.asarray(vis) if not torch.is_tensor(vis) else vis, device=dev) != 0).to(torch.uint8).reshape(n, nk)
        v = v.contiguous()
    if radius is not None and int(radius) <= 0:
        raise ValueError("radius %s: a positive integer, or None for the reference's rule" % (radius,))
    st = _stream(dev, stream)
    step = L.RENDER_MAX_FRAMES
    for a in range(0, n, step):
        d = L.SkeletonDesc()
        d.kps, d.ld_kps = k2[a].data_ptr(), _ld(k2)
        d.vis = v[a].data_ptr() if v is not None else None
        d.n, d.nk, d.h, d.w = min(step, n - a), int(nk), h, w
        d.kp_add, d.kp_mul = float(kp_add), float(kp_mul)
        d.draw_edges, d.radius = int(bool(draw_edges)), 0 if radius is None else int(radius)
        if bg.dtype == torch.float32:
            d.bg_float, d.bg_add, d.bg_mul = bg[a].data_ptr(), float(bg_add), float(bg_mul)
        else:
            d.bg_u8 = bg[a].data_ptr()
        d.out = out[a].data_ptr()
        L.check(lib.hmmr_draw_skeleton(C.byref(d), st), "hmmr_draw_skeleton")
    return out


def _pixel_joints(joints, device):
    """np.round(joints).astype(int) of draw_skeleton, as float32 rows [1, 2 K] the kernel reads back exactly.  The rounding
    stays in the caller's dtype (a float64 joint is not rounded through float32); the clamp is the kernel's."""
    j = joints.detach().cpu().numpy() if torch.is_tensor(joints) else np.asarray(joints)
    if j.shape[0] != 2:
        j = j.T
    with np.errstate(invalid="ignore"):
        r = np.clip(np.round(j.astype(np.float64) if j.dtype != np.float32 else j), COORD_MIN, COORD_MAX).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(r.T).reshape(1, -1)).to(device), r.shape[1]


def draw_skeleton(input_image, joints, draw_edges=True, vis=None, radius=None, on_device=False, device=None):
    """draw_skeleton of the reference for one image [h,w,3]: joints 2 x K or K x 2 in pixels (K = 19 or 25), vis [K].
    A uint8 image comes back as uint8.  A float image is read as [0, 1] when its maximum is <= 2 and as [0, 255] above, is
    truncated to bytes, and comes back as float32: divided by 255 when the maximum was <= 1, as byte values otherwise.
    A numpy image gives a numpy image; on_device=True (or a device tensor) gives a device tensor.
    An unknown joint count raises L.HmmrError where the reference enters a debugger."""
    is_t = torch.is_tensor(input_image)
    if device is None:
        device = input_image.device if is_t and input_image.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    img = input_image if is_t else torch.from_numpy(np.ascontiguousarray(input_image))
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("draw_skeleton: one image [h, w, 3] (skeleton_panels takes batches)")
    is_float = img.dtype in (torch.float32, torch.float64)
    if not is_float and img.dtype != torch.uint8:
        raise ValueError("draw_skeleton: uint8, float32 or float64 images")
    mul, max_val = 1.0, None
    if is_float:
        max_val = float(img.max())
        if max_val <= 2.0:                                   # "should be 1 but sometimes it's slightly above 1"
            mul = 255.0
        if img.dtype == torch.float64:                       # the product in the image's own precision, then the kernel truncates
            img = (img * mul).clamp(0, 255).floor().float()
            mul = 1.0
    kp, nk = _pixel_joints(joints, device)
    out = skeleton_panels(kp, img.to(device)[None], nk=nk, vis=None if vis is None else np.asarray(vis).reshape(1, -1),
                          draw_edges=draw_edges, radius=None if radius is None else int(radius), bg_mul=mul)[0]
    if is_float:
        out = out.float() / 255. if max_val <= 1.0 else out.float()
    return out if (on_device or (is_t and input_image.device.type == "cuda")) else out.cpu().numpy()


def collage_width(size, h, w):
    """columns of the collage of S x S crops and h x w original panels: S + max(w S // h, S)"""
    W = int(L.load().hmmr_collage_width(int(size), int(h), int(w)))
    if W <= 0:
        raise ValueError("no collage for S = %d and %d x %d panels (sizes out of range, or w S // h < 1)" % (size, h, w))
    return W


def compose_collage(rend_crop, skel_crop, render_og, rot_og, out=None, stream=None):
    """uint8 device panels rend_crop, skel_crop [n,S,S,3] and render_og, rot_og [n,h,w,3] -> the collage frames
    uint8 [n, 2 S, S + max(w S // h, S), 3] of render_preds, on the device."""
    lib = L.load()
    dev = rend_crop.device
    if dev.type != "cuda":
        raise L.HmmrError("compose_collage needs device tensors (the HIP library has no CPU path)")
    n, S = int(rend_crop.shape[0]), int(rend_crop.shape[1])
    h, w = int(render_og.shape[1]), int(render_og.shape[2])
    for name, t, shp in (("rend_crop", rend_crop, (n, S, S, 3)), ("skel_crop", skel_crop, (n, S, S, 3)),
                         ("render_og", render_og, (n, h, w, 3)), ("rot_og", rot_og, (n, h, w, 3))):
        if t.dtype != torch.uint8 or tuple(t.shape) != shp or t.device != dev:
            raise ValueError("%s must be uint8 %s on %s, got %s %s" % (name, shp, dev, t.dtype, tuple(t.shape)))
    W = collage_width(S, h, w)
    panels = [t.contiguous() for t in (rend_crop, skel_crop, render_og, rot_og)]
    if out is None:
        out = torch.empty((n, 2 * S, W, 3), dtype=torch.uint8, device=dev)
    st = _stream(dev, stream)
    step = L.RENDER_MAX_FRAMES
    for a in range(0, n, step):
        d = L.CollageDesc()
        d.rend_crop, d.skel_crop, d.render_og, d.rot_og = (p[a].data_ptr() for p in panels)
        d.n, d.S, d.h, d.w = min(step, n - a), S, h, w
        d.out = out[a].data_ptr()
        L.check(lib.hmmr_compose_collage(C.byref(d), st), "hmmr_compose_collage")
    return out


__all__ = ["skeleton_panels", "draw_skeleton", "collage_width", "compose_collage"]
