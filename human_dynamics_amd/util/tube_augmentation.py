"""Mirror of src/util/tube_augmentation.py: `TubePreprocessor` and `TubePreprocessorDriver`, the augmentor every tfrecord
writer of the reference puts in front of `FeatureExtractor.compute_all_phis`.

A bounded random walk of translation, scale (and rotation) over the tube, then per frame: bilinear resize, edge pad,
img_size crop, optional rotation, whole-tube flip, [0,1] -> [-1,1]; keypoints, SMPL pose and 3-D joints follow.  The
labels and the integers are computed on the host in float32 (util/data_utils.py); the pixels are ONE launch of
hmmr_tube_augment (csrc/tube.hip) on the whole tube and stay on the device.

Two agreements with the reference are unmeasured and cannot be measured without TensorFlow: the resize / rotate rules the
kernel follows are restated from the published TF 1.8 kernels (include/hmmr_hip.h), and the random draws are NumPy's, not
TensorFlow's stream.  `walks=` / `flip=` replace the draws, so that a recorded augmentation can be replayed exactly.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from . import data_utils

F = np.float32


def tube_augment(images, geom, flip, rot, img_size, device="cuda:0", out=None):
    """hmmr_tube_augment on a tube: images [n,H,W,3] float32 in [0,1] or uint8 (host array or device tensor), geom [n,4]
    int32 {newH, newW, x0, y0}, flip [n] bool, rot [n,6] float32 or None -> [n,img_size,img_size,3] float32 device tensor."""
    lib = L.load()
    if isinstance(images, torch.Tensor):
        im = images.to(device).contiguous()
    else:
        images = np.asarray(images)
        if images.dtype != np.uint8:
            images = images.astype(np.float32, copy=False)
        im = torch.from_numpy(np.ascontiguousarray(images)).to(device)
    if im.dtype not in (torch.uint8, torch.float32) or im.dim() != 4 or im.shape[3] != 3:
        raise ValueError("images: [n,H,W,3] float32 in [0,1] or uint8")
    n, h, w = (int(v) for v in im.shape[:3])
    geom = np.ascontiguousarray(geom, np.int32).reshape(-1, 4)
    flip = np.ascontiguousarray(np.broadcast_to(np.asarray(flip, bool).reshape(-1), (n,)), np.uint8)
    if len(geom) != n or (geom[:, :2] < 1).any():
        raise ValueError("geom: one {newH, newW, x0, y0} row per frame with a positive scaled size")
    g = torch.from_numpy(geom).to(device)
    fl = torch.from_numpy(flip).to(device)
    r = None
    if rot is not None:
        rot = np.ascontiguousarray(rot, np.float32).reshape(-1, 6)
        if len(rot) != n:
            raise ValueError("rot: one row of 6 per frame")
        r = torch.from_numpy(rot).to(device)
    S = int(img_size)
    if out is None:
        out = torch.empty((n, S, S, 3), dtype=torch.float32, device=device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, S, S, 3) and out.is_contiguous()
    if n:
        L.check(lib.hmmr_tube_augment(im.data_ptr(), int(im.dtype == torch.uint8), n, h, w, g.data_ptr(), fl.data_ptr(), L.ptr(r), S,
                                      out.data_ptr(), torch.cuda.current_stream(device).cuda_stream), "hmmr_tube_augment")
    return out


class TubePreprocessor(object):
    def __init__(self, img_size=224, trans_max=20, delta_trans_max=3, scale_max=0.3, delta_scale_max=0.05, rotate_max=0,
                 delta_rotate_max=0):
        self.output_size = img_size
        self.trans_max, self.scale_max, self.rotate_max = trans_max, scale_max, rotate_max
        self.delta_trans_max, self.delta_scale_max, self.delta_rotate_max = delta_trans_max, delta_scale_max, delta_rotate_max
        self.image_normalizing_fn = data_utils.rescale_image

    def draw_walks(self, T, rng=None):
        """(trans_walk [T,2] int32, scale_walk [T,1], rotate_walk [T,1]) as __call__ draws them (tube_augmentation.py:60-85)"""
        rng = np.random.default_rng() if rng is None else rng
        trans = data_utils.bounded_random_walk(-self.trans_max, self.trans_max + 1, -self.delta_trans_max, self.delta_trans_max + 1,
                                               T, np.int32, 2, rng)
        scale = data_utils.bounded_random_walk(-self.scale_max, self.scale_max, -self.delta_scale_max, self.delta_scale_max, T, F, 1, rng)
        rotate = data_utils.bounded_random_walk(-self.rotate_max, self.rotate_max, -self.delta_rotate_max, self.delta_rotate_max,
                                                T, F, 1, rng)
        return trans, scale, rotate

    def host_side(self, image_sizes, labels, centers, poses, gt3ds, walks, flip):
        """Everything but the pixels, for the whole tube: the dict of labels / poses / gt3ds / centers (as the reference returns
        them) and the kernel's operands geom [T,4], rot [T,6] or None.  Raises ValueError for a frame whose crop tf.slice
        would refuse, or whose scaled size has a zero."""
        S = self.output_size
        trans, scale, rotate = walks
        labels = np.asarray(labels, F)
        T = len(labels)
        trans = np.asarray(trans, np.int32).reshape(T, 2)
        scale, rotate = np.asarray(scale, F).reshape(T), np.asarray(rotate, F).reshape(T)
        vis, kp = labels[:, 2, :], labels[:, :2, :]
        center = data_utils.jitter_center(centers, trans)
        new_size, _, kp, center = data_utils.jitter_scale(image_sizes, kp, center, scale)
        margin = int(S / 2)
        margin_safe = margin + self.trans_max + 50
        start = center.astype(np.int64) + margin_safe - margin                  # crop origin in the padded image, (x, y)
        limit = new_size[:, ::-1].astype(np.int64) + 2 * margin_safe
        bad = (new_size < 1).any(1) | (start < 0).any(1) | (start + S > limit).any(1)
        if bad.any():
            t = int(np.argmax(bad))
            raise ValueError("frame %d: a %dx%d crop at (%d, %d) leaves the padded %dx%d scaled image (h x w; pad %d)"
                             % (t, S, S, start[t, 0] - margin_safe, start[t, 1] - margin_safe, new_size[t, 0], new_size[t, 1], margin_safe))
        startf = start.astype(F)
        x_crop = (kp[:, 0, :] + F(margin_safe)) - startf[:, 0:1]
        y_crop = (kp[:, 1, :] + F(margin_safe)) - startf[:, 1:2]
        crop_kp = np.stack([x_crop, y_crop, vis], 1)
        poses, gt3ds = np.asarray(poses, F), np.asarray(gt3ds, F)
        rot = None
        if self.rotate_max != 0:
            rot = data_utils.rotate_transforms(rotate, S)
            kp_rot, gt3ds, poses = data_utils.rotate_labels(crop_kp[:, :2], S, gt3ds, poses, rotate)
            crop_kp = np.concatenate([kp_rot, crop_kp[:, 2:]], 1)
        if flip:
            crop_kp, poses, gt3ds = data_utils.flip_labels(crop_kp, S, poses, gt3ds)
        final_vis = (crop_kp[:, 2, :] > 0).astype(F)
        final = np.stack([F(2.0) * (crop_kp[:, 0, :] / F(S)) - F(1.0), F(2.0) * (crop_kp[:, 1, :] / F(S)) - F(1.0), final_vis], 1)
        final = final_vis[:, None, :] * final
        geom = np.concatenate([new_size, (start - margin_safe).astype(np.int32)], 1).astype(np.int32)
        ret = {"labels": final.astype(F), "poses": poses.astype(F), "gt3ds": gt3ds.astype(F), "centers": center.reshape(T, 2, 1)}
        return ret, geom, rot

    def __call__(self, images, image_sizes, labels, centers, poses, gt3ds, return_walk=False, rng=None, walks=None, flip=None,
                 device="cuda:0"):
        """images [T,H,W,3] float32 in [0,1] or uint8, host or device; image_sizes [T,2]; labels [T,3,25]; centers [T,2];
        poses [T,72]; gt3ds [T,14,3].  walks = (trans [T,2] int, scale [T,1], rotate [T,1]) and flip (bool) replace the random
        draws.  Returns the reference's dict with `images` [T,S,S,3] float32 as a DEVICE tensor, the rest host arrays."""
        T = len(images)
        rng = np.random.default_rng() if rng is None else rng
        if flip is None:
            flip = bool(rng.random(dtype=np.float32) < 0.5)
        if walks is None:
            walks = self.draw_walks(T, rng)
        ret, geom, rot = self.host_side(image_sizes, labels, centers, poses, gt3ds, walks, bool(flip))
        ret["images"] = tube_augment(images, geom, np.full(T, bool(flip)), rot, self.output_size, device)
        if return_walk:
            ret.update({"trans_walk": np.asarray(walks[0], np.int32).reshape(T, 2), "scale_walk": np.asarray(walks[1], F).reshape(T, 1),
                        "rot_walk": np.asarray(walks[2], F).reshape(T, 1)})
        return ret


class TubePreprocessorDriver(object):
    """The reference's Session wrapper; `sess` is accepted and ignored (there is no graph here)."""

    def __init__(self, img_size=224, trans_max=20, delta_trans_max=3, scale_max=0.3, delta_scale_max=0.05, rotate_max=0,
                 delta_rotate_max=0, sess=None, device="cuda:0"):
        self.preprocessor = TubePreprocessor(img_size, trans_max, delta_trans_max, scale_max, delta_scale_max, rotate_max,
                                             delta_rotate_max)
        self.sess = sess
        self.device = device

    def run_device(self, images, image_sizes, labels, centers, poses, gt3ds, **kw):
        """__call__ with the crops left on the device (what FeatureExtractor.compute_all_phis_augmented consumes)"""
        if np.shape(labels)[-1] == 3:
            labels = np.transpose(labels, [0, 2, 1])
        kw.setdefault("device", self.device)
        return self.preprocessor(images, image_sizes, labels, centers, poses, gt3ds, return_walk=True, **kw)

    def __call__(self, images, image_sizes, labels, centers, poses, gt3ds, **kw):
        """Returns host arrays under the reference's keys: images, labels, poses, gt3ds, centers, trans_walk, scale_walk,
        rot_walk.  Keyword arguments (rng=, walks=, flip=) go to the preprocessor."""
        ret = self.run_device(images, image_sizes, labels, centers, poses, gt3ds, **kw)
        ret["images"] = ret["images"].cpu().numpy()
        return ret
