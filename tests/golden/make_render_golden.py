"""Golden vectors for the rasteriser's glue, produced by EXECUTING the reference's own source
(src/util/render/nmr_renderer.py: VisRenderer.__call__, rotated, visualize_img, visualize_img_orig) with stand-ins for
what cannot be installed here:

  neural_renderer   Renderer.render / render_silhouettes call tests/render_oracle.py (the spec of csrc/render.hip)
  Tensor.cuda       identity (no CUDA device)
  cv2               Rodrigues and resize restated in NumPy (resize with the taps of csrc/image_geom.h); draw_skeleton's
                    drawing is not needed (only the mesh panels are recorded)
  skimage.io        unused

so the fixture pins what the reference does AROUND NMR: texture x default texture, the y flip, the uint8 casts, alpha /
RGBA / silhouettes, the centroid rotation, make_square and remove_pads.  Every recorded image comes with the oracle's
pixel ambiguity mask (any of the four subpixels ambiguous).

    python tests/golden/make_render_golden.py      -> tests/golden/reference_render.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference"

import render_oracle as O  # noqa: E402
from human_dynamics_amd.util.render.mesh import latlong_sphere  # noqa: E402

_last_amb = []


class _Renderer(object):
    """neural_renderer.Renderer as VisRenderer configures it, on the NumPy oracle"""

    def __init__(self, image_size, camera_mode='look_at', perspective=False):
        assert camera_mode == 'look_at' and perspective is False
        self.image_size = image_size
        self.light_direction = [0, 1, 0]
        self.light_intensity_directional = 0.5
        self.light_intensity_ambient = 0.5
        self.light_color_ambient = [1, 1, 1]
        self.light_color_directional = [1, 1, 1]
        self.background_color = [0, 0, 0]

    def _raster(self, vertices, faces):
        S = int(self.image_size)
        out = []
        for b in range(vertices.shape[0]):
            idx, amb = O.rasterize(vertices[b].numpy(), faces[b].numpy(), S)
            out.append((idx, amb))
        _last_amb.append(np.stack([O.pixel_ambiguity(a, S) for _, a in out]))
        return out

    def render(self, vertices, faces, textures):
        S = int(self.image_size)
        imgs = []
        for b, (idx, _) in enumerate(self._raster(vertices, faces)):
            tex = textures[b].numpy().reshape(textures.shape[1], -1, 3)[:, 0, :]
            cols = O.shade(vertices[b].numpy(), faces[b].numpy(), face_colors=tex, light_dir=self.light_direction,
                           int_dir=self.light_intensity_directional, int_amb=self.light_intensity_ambient,
                           col_dir=self.light_color_directional, col_amb=self.light_color_ambient)
            pooled, _ = O.pool(idx, cols, S, self.background_color)
            imgs.append(pooled.transpose(2, 0, 1))
        return torch.from_numpy(np.stack(imgs))

    def render_silhouettes(self, vertices, faces):
        S = int(self.image_size)
        return torch.from_numpy(np.stack([O.pool(idx, np.zeros((faces.shape[1], 3)), S)[1]
                                          for idx, _ in self._raster(vertices, faces)]))


def _cv2():
    cv2 = types.ModuleType("cv2")
    cv2.Rodrigues = lambda r: (O.rodrigues(np.rad2deg(np.linalg.norm(r)), 'y' if abs(r[1]) > 0 else ('x' if abs(r[0]) > 0 else 'z')), None)

    def resize(img, dsize):
        # visualize_img_orig resizes the float64 frame in [-1, 1]; resize_frame takes uint8 and returns [0, 255] terms
        raise AssertionError("replaced per call")
    cv2.resize = resize
    return cv2


def main():
    if not hasattr(np, "int"):
        np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self
    nr = types.ModuleType("neural_renderer"); nr.Renderer = _Renderer
    skio = types.ModuleType("skimage.io"); skio.imread = lambda p: None
    sk = types.ModuleType("skimage"); sk.io = skio
    cv2 = _cv2()
    for n, m in (("neural_renderer", nr), ("skimage", sk), ("skimage.io", skio), ("cv2", cv2)):
        sys.modules.setdefault(n, m)
    sys.path.insert(0, REF)
    try:
        from src.util.render import nmr_renderer as R
    finally:
        sys.path.remove(REF)
    R.draw_skeleton = lambda img, joints, **kw: img
    R.draw_text = lambda img, text: img

    v0, faces = latlong_sphere(30, 32)                      # 1 922 vertices, 1 920 faces
    rng = np.random.default_rng(3)
    fpath = os.path.join(HERE, "_faces_tmp.npy")
    np.save(fpath, faces)
    out = {"faces": faces.astype(np.int32)}

    def mesh(seed):
        r = np.random.default_rng(seed)
        v = v0 * np.array([0.35, 0.7, 0.3], np.float32) * (1 + 0.1 * np.sin(3 * v0[:, 1:2] + r.uniform(0, 6)))
        return v.astype(np.float32)

    def pattern(shape, seed):
        """a smooth uint8 image (compresses well; random pixels would not)"""
        yy, xx, cc = np.meshgrid(*[np.arange(n) for n in shape[-3:]], indexing="ij")
        a, b = 1 + seed % 5, 2 + seed % 3
        return np.broadcast_to(((a * xx + b * yy + 60 * cc + 8 * np.sin(xx / 7.0)) % 256).astype(np.uint8), shape).copy()

    def cam():
        return np.array([rng.uniform(0.8, 1.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)], np.float32)
    try:
        # ---- VisRenderer.__call__ / rotated: [kind, S, batch, rend_mask, alpha, img, rotate]
        cases = [(32, 1, 0, 0, 0, 0), (64, 1, 0, 1, 0, 0), (48, 1, 1, 0, 0, 0), (96, 1, 0, 0, 1, 0), (64, 3, 0, 0, 0, 0),
                 (80, 2, 0, 0, 1, 0), (128, 1, 0, 0, 0, 1), (224, 1, 0, 0, 1, 0)]
        for k, (S, batch, rend_mask, alpha, has_img, rot) in enumerate(cases):
            r = R.VisRenderer(img_size=S, face_path=fpath)
            verts = np.stack([mesh(10 * k + b) for b in range(batch)]) if batch > 1 else mesh(10 * k)
            c = np.stack([cam() for _ in range(batch)]) if batch > 1 else cam()
            img = pattern(((batch,) if batch > 1 else ()) + (S, S, 3), k).astype(np.float32) + np.float32(0.25) if has_img else None
            del _last_amb[:]
            if rot:
                got = r.rotated(torch.from_numpy(verts), 90, cam=c, rend_mask=bool(rend_mask), alpha=bool(alpha))
            else:
                got = r(verts, cam=c, rend_mask=bool(rend_mask), alpha=bool(alpha), img=img)
            amb = np.logical_or.reduce(_last_amb)               # [B,S,S] over the render and the silhouette passes
            key = "case_%d" % k
            out[key] = np.asarray(got)
            out[key + "_spec"] = np.array([0, S, batch, rend_mask, alpha, has_img, rot])
            out[key + "_verts"], out[key + "_cam"] = verts, c
            if has_img:
                out[key + "_img"] = img
            out[key + "_amb"] = amb[0] if batch == 1 else amb
        # ---- visualize_img_orig (the mesh half: rend_img and the rotated view) and visualize_img on the crop
        shapes = [((60, 80), 720), ((90, 50), 720), ((400, 300), 224), ((240, 320), 160)]
        params, hw = [], []
        for k, ((h, w), max_img) in enumerate(shapes):
            frame = pattern((h, w, 3), 7 + k)
            c = cam()
            verts = mesh(100 + k)
            start_pt = np.array([w / 2 + rng.uniform(-10, 10), h / 2 + rng.uniform(-10, 10)])
            scale = 224.0 / max(h, w) * rng.uniform(0.8, 1.2)
            h2, w2 = (int(np.floor(h * max_img / max(h, w))), int(np.floor(w * max_img / max(h, w)))) if max(h, w) > max_img else (h, w)

            def resize(img, dsize, _frame=frame):
                assert dsize == (w2, h2)
                return (O.resize_frame(_frame, h2, w2) / 255. - 0.5) * 2      # [-1, 1] float64, as cv2 on the float frame
            cv2.resize = resize
            del _last_amb[:]
            r = R.VisRenderer(img_size=224, face_path=fpath)
            _, rend, rot = R.visualize_img_orig(cam=c, kp_pred=np.zeros((25, 2), np.float32), vert=verts, renderer=r,
                                                start_pt=start_pt, scale=scale, proc_img_shape=[224, 224],
                                                img=((frame / 255.) - 0.5) * 2, max_img_size=max_img, no_text=True,
                                                rotated_view=True)
            key = "orig_%d" % k
            out[key + "_frame"], out[key + "_cam"], out[key + "_verts"] = frame, c, verts
            out[key + "_params"] = np.array([start_pt[0], start_pt[1], scale, max_img])
            out[key + "_rend"] = np.round(rend * 255).astype(np.uint8)
            out[key + "_rot"] = np.round(rot * 255).astype(np.uint8)
            out[key + "_amb"] = _last_amb[0][0][:h2, :w2] | _last_amb[1][0][:h2, :w2]
            out[key + "_amb_rot"] = _last_amb[2][0][:h2, :w2]
            params.append([h, w, max_img]); hw.append([h2, w2])
            # the crop panel (render_preds' visualize_img on the 224x224 crop)
            crop = (pattern((224, 224, 3), k) / np.float32(127.5) - np.float32(1)).astype(np.float32)
            del _last_amb[:]
            rc = R.VisRenderer(img_size=224, face_path=fpath)
            _, rend_crop = R.visualize_img(img=crop, cam=c, kp_pred=np.zeros((25, 2), np.float32), vert=verts, renderer=rc,
                                           no_text=True)
            out[key + "_crop"] = crop
            out[key + "_rend_crop"] = np.round(rend_crop * 255).astype(np.uint8)
            out[key + "_amb_crop"] = _last_amb[0][0] | _last_amb[1][0]
        out["orig_params"] = np.array(params)
        out["orig_out_hw"] = np.array(hw)
    finally:
        os.remove(fpath)
    path = os.path.join(HERE, "reference_render.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
