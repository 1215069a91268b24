"""VisRenderer: a drop-in for the reference's class of the same name (src/util/render/nmr_renderer.py:43-240) on the
project's own rasteriser (csrc/render.hip) instead of neural_renderer, which does not exist for ROCm.

The reference's `visualize_img`, `visualize_img_orig` and `render_preds` run unchanged on top of it for their mesh
panels (they set `.renderer.image_size` and call `__call__` / `rotated`).  The module-level `visualize_img` and
`visualize_img_orig` below are the reference's functions of those names (:265-419) without cv2: the skeleton comes from
util/render/collage.draw_skeleton, whose draw list is the reference's and whose primitives follow the integer rules of
include/hmmr_hip.h -- agreement with OpenCV's circles and lines at primitive boundaries has not been measured -- and
`draw_text` (cv2.putText) is not provided: they take `no_text=True` only.  `compute_video_bbox` and `visualize_mesh_og`
(:519-634, :422-488) are the reference's person-centred view: the box of a person over the whole video, the cameras relative to it
(one hmmr_video_bbox launch) and the mesh, optionally turned, in a square of the box's size.  Inputs may be numpy arrays or device tensors; results
are what the reference returns (uint8 numpy: [S,S,3], [B,S,S,3], RGBA [S,S,4], or the silhouette), or the same data as
device tensors with `on_device=True`.  Only t_size = 1 textures (one colour per face) are supported.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import _lib as L
from ...tf_smpl.batch_smpl import _SmplUnpickler
from .collage import draw_skeleton
from .handoff import orig_image_geometry
from .person_view import clip_size, proc_rows, video_bbox
from .raster import COLORS, MeshFaces, render_mesh, rodrigues

colors = COLORS


def load_faces(face_path):
    """Faces [F,3] int32 from a .npy (the reference's smpl_faces.npy) or from an SMPL .pkl's `f` (read without
    chumpy, as batch_smpl.load_smpl_constants reads the model)."""
    if str(face_path).endswith(".pkl"):
        with open(face_path, "rb") as fh:
            dd = _SmplUnpickler(fh, encoding="latin1").load()
        f = dd["f"]
        f = getattr(f, "r", f)
    else:
        f = np.load(face_path)
    return np.asarray(f).astype(np.int32)


class _RendererState(object):
    """The attributes of nr.Renderer that VisRenderer and visualize_img_orig read or set."""

    def __init__(self, image_size):
        self.image_size = image_size
        self.light_direction = [0, 1, 0]
        self.light_intensity_directional = 0.5
        self.light_intensity_ambient = 0.5
        self.light_color_ambient = [1, 1, 1]
        self.light_color_directional = [1, 1, 1]
        self.background_color = [0, 0, 0]
        self.camera_mode, self.perspective, self.viewing_angle = 'look_at', False, 30
        self.near, self.far, self.anti_aliasing, self.fill_back = 0.1, 100, True, True


def _dims(x):
    return x.dim() if isinstance(x, torch.Tensor) else np.ndim(x)


class VisRenderer(object):
    """Renders meshes with the same orthographic projection as HMR (no perspective); faces F x 3 or 1 x F x 3."""

    def __init__(self, img_size=256, face_path='src/tf_smpl/smpl_faces.npy', t_size=1, device="cuda", on_device=False,
                 faces=None):
        if t_size != 1:
            raise NotImplementedError("VisRenderer: textures with t_size > 1 are not supported (one colour per face)")
        self.renderer = _RendererState(img_size)
        self.set_light_dir([1, .5, -1], int_dir=0.3, int_amb=0.7)
        self.set_bgcolor([1, 1, 1.])
        self.img_size = img_size
        self.faces_np = np.asarray(faces if faces is not None else load_faces(face_path)).astype(np.int32)
        if self.faces_np.ndim == 3:
            self.faces_np = self.faces_np[0]
        self._faces = MeshFaces(self.faces_np)
        self.device = torch.device(device)
        self.on_device = on_device
        self.default_cam = np.array([[0.9, 0, 0]], np.float32)

    def _tensor(self, x):
        if isinstance(x, torch.Tensor):
            return x.to(self.device, torch.float32)
        return torch.as_tensor(np.asarray(x, np.float32), device=self.device)

    def _render(self, verts, cam, texture, rend_mask, alpha, img, color_name, rot):
        num_batch = 1
        if _dims(verts) == 3 and verts.shape[0] != 1:
            num_batch = verts.shape[0]
            if cam is not None:
                assert _dims(cam) == 2 and cam.shape[0] == num_batch
            if img is not None:
                assert img.ndim == 4 and img.shape[0] == num_batch
        v = self._tensor(verts)
        if v.dim() == 2:
            v = v.unsqueeze(0)
        n = v.shape[0]
        c = self._tensor(self.default_cam if cam is None else cam).reshape(-1, 3)
        if c.shape[0] == 1 and n > 1:
            c = c.expand(n, 3).contiguous()
        face_colors = None
        if texture is not None:
            t = self._tensor(texture)
            if t.dim() == 5:
                t = t.unsqueeze(0)
            face_colors = t.reshape(t.shape[0], t.shape[1], -1, 3)[:, :, 0, :]      # t_size = 1: one colour per face
            if face_colors.shape[0] == 1:
                face_colors = face_colors[0]
        r = self.renderer
        S = int(r.image_size)
        kw = dict(color=colors[color_name], face_colors=face_colors, bg_color=r.background_color,
                  light_dir=r.light_direction, int_dir=r.light_intensity_directional,
                  int_amb=r.light_intensity_ambient, col_dir=r.light_color_directional, col_amb=r.light_color_ambient,
                  rot=rot)
        if img is not None and not rend_mask:
            im = self._tensor(img).reshape(n, S, S, 3)
            out = render_mesh(v, c, self._faces, S, bg_mode=L.RENDER_BG_FLOAT, bg_image=im, **kw)["rgb"]
            if num_batch == 1:
                out = out[0]
            return out if self.on_device else out.cpu().numpy()
        res = render_mesh(v, c, self._faces, S, want_alpha=rend_mask or alpha, **kw)
        if rend_mask:                          # render_silhouettes, repeated to 3 channels as the reference does
            sil = (torch.clamp(res["alpha"], 0, 1) * 255.0).to(torch.uint8)        # [n,S,S]
            out = sil.permute(1, 2, 0).repeat(1, 1, 3).unsqueeze(0)                # [1,S,S,3n]
            if num_batch == 1:
                out = out[0]
        elif alpha:
            a = (res["alpha"] * 255).to(torch.uint8)
            out = torch.cat([res["rgb"], a.unsqueeze(-1)], -1)
            if num_batch == 1:
                out = out[0]
        else:
            out = res["rgb"][0] if num_batch == 1 else res["rgb"]
        return out if self.on_device else out.cpu().numpy()

    def __call__(self, verts, cam=None, texture=None, rend_mask=False, alpha=False, img=None, color_name='blue'):
        """verts [V,3] or [B,V,3], cam [3] or [B,3] ([s, tx, ty], HMR's), img [S,S,3] / [B,S,S,3] in [0, 255]:
        uint8 [S,S,3] (or [B,S,S,3]); RGBA [S,S,4] with alpha; the silhouette with rend_mask."""
        return self._render(verts, cam, texture, rend_mask, alpha, img, color_name, None)

    def rotated(self, verts, deg, axis='y', cam=None, texture=None, rend_mask=False, alpha=False, color_name='blue'):
        """The mesh rotated by `deg` about `axis` through its centroid, then rendered as __call__ does (no image)."""
        v = verts if _dims(verts) == 3 else verts[None]
        return self._render(v, cam, texture, rend_mask, alpha, None, color_name, rodrigues(deg, axis))

    def make_alpha(self, rend, mask):
        rend = rend.astype(np.uint8)
        alpha = (mask * 255).astype(np.uint8)
        return np.dstack((rend, alpha))

    def set_light_dir(self, direction, int_dir=0.8, int_amb=0.8):
        self.renderer.light_direction = direction
        self.renderer.light_intensity_directional = int_dir
        self.renderer.light_intensity_ambient = int_amb

    def set_bgcolor(self, color):
        self.renderer.background_color = color


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def make_square(img):
    """Pads the shorter side with zeros at its end (the rasteriser draws squares): (img, pad_vals)."""
    img_size = np.max(img.shape[:2])
    pad_vals = img_size - np.array(img.shape[:2])
    return np.pad(img, ((0, pad_vals[0]), (0, pad_vals[1]), (0, 0)), mode='constant'), pad_vals


def remove_pads(img, pad_vals):
    """Undoes make_square."""
    if pad_vals[0] != 0:
        img = img[:-pad_vals[0], :]
    if pad_vals[1] != 0:
        img = img[:, :-pad_vals[1]]
    return img


def _resize_linear(img, h, w):
    """cv2.resize(img, (w, h)) of a float image as csrc/image_geom.h's taps have it: pixel centres aligned in float32,
    float32 weights, float64 sums, the horizontal pass first (resize_img of src/util/common.py)."""
    def taps(src, dst):
        f = ((np.arange(dst) + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = f - s.astype(np.float32)
        edge = (s < 0) | (s >= src - 1)
        s = np.clip(s, 0, src - 1)
        f[edge] = 0
        return s, np.minimum(s + 1, src - 1), (np.float32(1) - f).astype(np.float64), f.astype(np.float64)
    x0, x1, a0, a1 = taps(img.shape[1], w)
    y0, y1, b0, b1 = taps(img.shape[0], h)
    img = np.asarray(img, np.float64)
    rows = img[:, x0] * a0[None, :, None] + img[:, x1] * a1[None, :, None]
    return rows[y0] * b0[:, None, None] + rows[y1] * b1[:, None, None]


def _no_text(text, no_text):
    if not no_text or text:
        raise NotImplementedError("draw_text (cv2.putText, a Hershey font) is not provided: call with no_text=True and no text")


def visualize_img(img, cam, kp_pred, vert, renderer, kp_gt=None, text={}, rotated_view=False, mesh_color='blue',
                  pad_vals=None, no_text=False):
    """img [S,S,3] in [-1, 1], keypoints in normalised coordinates -> (skel_img / 255, rend_img / 255[, rot_img / 255]):
    the predicted skeleton (and kp_gt's visible joints as rings) over the image, the mesh over the image, the mesh turned
    by 90 degrees.  pad_vals: what make_square added, removed again from every panel."""
    _no_text(text, no_text)
    img = _host(img)
    img_size = img.shape[0]
    input_img = ((img + 1) * 0.5) * 255.
    rend_img = _host(renderer(vert, cam=cam, img=input_img, color_name=mesh_color))
    kp_pred = _host(kp_pred)
    skel_img = draw_skeleton(input_img, ((kp_pred + 1) * 0.5) * img_size)
    if kp_gt is not None:
        kp_gt = _host(kp_gt)
        skel_img = draw_skeleton(skel_img, ((kp_gt[:, :2] + 1) * 0.5) * img_size, draw_edges=False,
                                 vis=kp_gt[:, 2].astype(bool))
    panels = [skel_img, rend_img]
    if rotated_view:
        panels.append(_host(renderer.rotated(vert, 90, cam=cam, alpha=False, color_name=mesh_color)))
    if pad_vals is not None:
        panels = [remove_pads(p, pad_vals) for p in panels]
    return tuple(p / 255 for p in panels)


def visualize_img_orig(cam, kp_pred, vert, renderer, start_pt, scale, proc_img_shape, im_path=None, img=None,
                       rotated_view=False, mesh_color='blue', max_img_size=300, no_text=False, bbox=None, crop_cam=None):
    """visualize_img in the space of the original image: img in [-1, 1] (or im_path, read with PIL), down-scaled to
    max_img_size, squared, with the camera and the keypoints moved from the crop (start_pt, scale, proc_img_shape are
    process_image's) to it."""
    _no_text(None, no_text)
    if img is None:
        from PIL import Image
        img = ((np.asarray(Image.open(im_path).convert("RGB")) / 255.) - 0.5) * 2
    img = _host(img)
    undo_scale = 1. / np.array(scale)
    if np.max(img.shape[:2]) > max_img_size:
        scale_orig = max_img_size / float(np.max(img.shape[:2]))
        new_hw = np.floor(np.array(img.shape[:2]) * scale_orig).astype(int)
        img = _resize_linear(img, new_hw[0], new_hw[1])
        undo_scale = undo_scale * scale_orig
    if bbox is not None:
        assert crop_cam is not None
        img = img[bbox[0]:bbox[1], bbox[2]:bbox[3]]
        start_pt = np.array([0, 0])
    img, pad_vals = make_square(img)
    img_size = np.max(img.shape[:2])
    renderer.renderer.image_size = img_size
    proc = proc_img_shape[0]
    pred_joint_orig = (((_host(kp_pred) + 1) * 0.5) * proc + start_pt - proc) * undo_scale
    kp_orig = 2 * (pred_joint_orig / img_size) - 1
    if bbox is not None:
        use_cam = crop_cam
    else:
        cam = _host(cam)
        cam_crop = np.hstack([proc * cam[0] * 0.5, cam[1:] + (2. / cam[0]) * 0.5])
        cam_orig = np.hstack([cam_crop[0] * undo_scale, cam_crop[1:] + (start_pt - proc) / cam_crop[0]])
        k = 2. / img_size
        use_cam = np.hstack([cam_orig[0] * k, cam_orig[1:] - (1 / (k * cam_orig[0]))]).astype(np.float32)
    return visualize_img(img=img, cam=use_cam, kp_pred=kp_orig, vert=vert, renderer=renderer, rotated_view=rotated_view,
                         mesh_color=mesh_color, pad_vals=pad_vals, no_text=no_text)


def _image_hw(im_path):
    from PIL import Image
    with Image.open(im_path) as im:
        return im.size[1], im.size[0]


def compute_video_bbox(cams, kps, proc_infos, margin=10, img_shape=None, status=False, device=None):
    """The reference's function of this name (:519-634) in one hmmr_video_bbox launch: the box [ymin, ymax, xmin, xmax] that
    holds the person of cams [N,3] / kps [N,K,2] (host arrays, device tensors, or lists of N per-frame arrays or tensors as the
    reference takes them; crop coordinates in [-1, 1]) over the whole video, and the N cameras relative to it.  proc_infos: process_image's dicts (scale, start_pt, im_shape).
    img_shape=(h, w) stands for the reference's imread(proc_infos[0]['im_path']); without it that file's size is read with PIL.
    -> (bbox int array [4], list of N float32 cameras [3]); with status=True also the HMMR_BBOX_* word (_lib.BBOX_*): where the
    reference prints 'crop is more than start pt..?' and stops in a debugger, BEYOND_START is set and the results are those it
    computes when continued."""
    if img_shape is None:
        img_shape = _image_hw(proc_infos[0]['im_path'])
    if device is None:
        first = [x if torch.is_tensor(x) or not len(x) else x[0] for x in (cams, kps)]
        device = next((x.device for x in first if torch.is_tensor(x) and x.device.type == "cuda"),
                      torch.device("cuda", torch.cuda.current_device()))

    def up(x):                                         # an array, a tensor, or the reference's list of per-frame arrays / tensors
        if not torch.is_tensor(x):
            x = torch.stack(list(x)) if len(x) and torch.is_tensor(x[0]) else torch.as_tensor(np.asarray(x, np.float32))
        return x.to(device, torch.float32)

    c, k = up(cams), up(kps)
    n = c.shape[0]
    c, k = c.reshape(n, -1).contiguous(), k.reshape(n, -1, k.shape[-1])[:, :, :2].reshape(n, -1).contiguous()
    proc = torch.as_tensor(proc_rows(proc_infos), device=device)
    bbox, crop, st = video_bbox(c, k, k.shape[1] // 2, proc, [0, n], img_shape, margin, proc_size=float(proc_infos[0]['im_shape'][0]))
    bbox_h = bbox[0].cpu().numpy().astype(int)
    new_cams = list(crop.cpu().numpy())
    return (bbox_h, new_cams, int(st[0])) if status else (bbox_h, new_cams)


def visualize_mesh_og(cam, vert, renderer, start_pt, scale, proc_img_shape, im_path=None, img=None, deg=0, mesh_color='blue',
                      max_img_size=300, pad=50, crop_cam=None, bbox=None):
    """The reference's function of this name (:422-488): the mesh, turned by `deg` about y, in the space of the original image
    (bbox None: the camera moves from the crop to the image as in visualize_img_orig) or of the video-level box
    (bbox, crop_cam: compute_video_bbox's).  The image (img [H,W,...], or im_path, whose size is read with PIL) only decides the
    size, as in the reference: the window of the box or the whole image, down-scaled to max_img_size and squared.  Sets
    renderer.renderer.image_size and returns renderer.rotated(...)."""
    hw = tuple(img.shape[:2]) if img is not None else _image_hw(im_path)
    if bbox is not None:
        assert crop_cam is not None
        rows, cols = range(hw[0])[int(bbox[0]):int(bbox[1])], range(hw[1])[int(bbox[2]):int(bbox[3])]      # img[ymin:ymax, xmin:xmax], clipped as a slice is
        renderer.renderer.image_size = clip_size([0, len(rows), 0, len(cols)], max_img_size)[2]
        return renderer.rotated(vert, deg, cam=crop_cam, color_name=mesh_color)
    undo_scale, sx, sy, proc, img_size = orig_image_geometry({"scale": scale, "start_pt": start_pt, "im_shape": proc_img_shape}, hw, max_img_size)
    renderer.renderer.image_size = int(img_size)
    cam = np.asarray(_host(cam), np.float64)
    cam_crop = np.hstack([proc * cam[0] * 0.5, cam[1:] + (2. / cam[0]) * 0.5])
    cam_orig = np.hstack([cam_crop[0] * undo_scale, cam_crop[1:] + (np.array([sx, sy]) - proc) / cam_crop[0]])
    k = 2. / int(img_size)
    new_cam = np.hstack([cam_orig[0] * k, cam_orig[1:] - (1 / (k * cam_orig[0]))]).astype(np.float32)
    return renderer.rotated(vert, deg, cam=new_cam, color_name=mesh_color)


__all__ = ["VisRenderer", "colors", "load_faces", "visualize_img", "visualize_img_orig", "make_square", "remove_pads",
           "compute_video_bbox", "visualize_mesh_og"]
