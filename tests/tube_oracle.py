"""Float32 NumPy oracle of TubePreprocessor.preprocess_image (src/util/tube_augmentation.py:114-186) for one frame: pixels
and labels.  TEST INFRASTRUCTURE ONLY; the product's host mirror is human_dynamics_amd/util/{data_utils,tube_augmentation}.py
and its pixels come from csrc/tube.hip.

`tf_resize_bilinear` and `tf_rotate_bilinear` restate the two TensorFlow 1.8 kernels the reference calls through
tf.image.resize_images and tf.contrib.image.rotate (resize_bilinear_op.cc; contrib/image/kernels/image_ops.h) by the rules
written next to hmmr_tube_augment in include/hmmr_hip.h.  They are restatements: no TensorFlow binary was run against them.
Every operation is one float32 NumPy ufunc, so the kernel (compiled without contraction) performs the same IEEE operations
in the same order and must agree bit for bit.

The rest of this file follows the reference's own code line by line (jitter_center, jitter_scale, pad_image_edge, the
slice, rotate_img, flip_image, reflect_pose, reflect_joints3d, rescale_image, batch_rodrigues, batch_rot2aa) and is pinned
to it by tests/golden/reference_tube.npz, which tests/golden/make_tube_golden.py produces by executing that code.
"""
import numpy as np

F = np.float32

FLIP_KP = np.array([5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 16, 15, 18, 17, 20, 19, 22, 21, 24, 23])
FLIP_POSE = np.array([0, 1, 2, 6, 7, 8, 3, 4, 5, 9, 10, 11, 15, 16, 17, 12, 13, 14, 18, 19, 20, 24, 25, 26, 21, 22, 23, 27, 28, 29, 33,
                      34, 35, 30, 31, 32, 36, 37, 38, 42, 43, 44, 39, 40, 41, 45, 46, 47, 51, 52, 53, 48, 49, 50, 57, 58, 59, 54, 55,
                      56, 63, 64, 65, 60, 61, 62, 69, 70, 71, 66, 67, 68])
FLIP_J3D = np.array([5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13])


def _axis_taps(src, dst):
    """lo, hi, lerp of every destination index of a src -> dst resize (align_corners=False, no half-pixel offset)"""
    scale = F(src) / F(dst)
    pos = np.arange(dst, dtype=np.int64).astype(F) * scale
    lo = pos.astype(np.int64)
    hi = np.minimum(lo + 1, src - 1)
    return lo, hi, pos - lo.astype(F)


def tf_resize_bilinear(image, new_h, new_w):
    """image [H,W,C] float32 -> [new_h,new_w,C] float32: tf.image.resize_images(image, [new_h, new_w]) of TF 1.8"""
    image = np.asarray(image)
    assert image.dtype == np.float32 and new_h > 0 and new_w > 0
    ylo, yhi, yl = _axis_taps(image.shape[0], new_h)
    xlo, xhi, xl = _axis_taps(image.shape[1], new_w)
    xl = xl[None, :, None]
    yl = yl[:, None, None]
    tl, tr = image[ylo][:, xlo], image[ylo][:, xhi]
    bl, br = image[yhi][:, xlo], image[yhi][:, xhi]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    out = top + (bot - top) * yl
    assert out.dtype == np.float32
    return out


def rotate_transform(theta, size):
    """[cos, -sin, xoff, sin, cos, yoff] float32: angles_to_projective_transforms of a size x size image (TF 1.8)"""
    theta = F(theta)
    c, s = np.cos(theta), np.sin(theta)
    m = F(size - 1)
    xoff = (m - (c * m - s * m)) / F(2)
    yoff = (m - (s * m + c * m)) / F(2)
    return np.array([c, -s, xoff, s, c, yoff], F)


def tf_rotate_bilinear(image, transform):
    """image [S,S,C] float32, transform [6] float32 (output -> input) -> the rotated image, zeros outside"""
    image = np.asarray(image)
    assert image.dtype == np.float32 and image.shape[0] == image.shape[1]
    S = image.shape[0]
    a = np.asarray(transform, F)
    x = np.arange(S).astype(F)[None, :]
    y = np.arange(S).astype(F)[:, None]
    fx = a[0] * x + a[1] * y + a[2]
    fy = a[3] * x + a[4] * y + a[5]
    xf, yf = np.floor(fx), np.floor(fy)
    xc, yc = xf + F(1), yf + F(1)

    def read(ty, tx):
        ok = (ty >= 0) & (ty < S) & (tx >= 0) & (tx < S)
        iy = np.where(ok, ty, 0).astype(np.int64)
        ix = np.where(ok, tx, 0).astype(np.int64)
        return np.where(ok[..., None], image[iy, ix], F(0))

    wx0, wx1 = (xc - fx)[..., None], (fx - xf)[..., None]
    row_f = wx0 * read(yf, xf) + wx1 * read(yf, xc)
    row_c = wx0 * read(yc, xf) + wx1 * read(yc, xc)
    out = (yc - fy)[..., None] * row_f + (fy - yf)[..., None] * row_c
    assert out.dtype == np.float32
    return out


def scale_geometry(image_size, center, trans, scale):
    """The integers of jitter_center + jitter_scale for one frame: (new_size [2] = (h, w), actual_factor [2] float32,
    scaled centre [2] = (x, y) int32)."""
    center = np.asarray(center, np.int32).reshape(2) + np.asarray(trans, np.int32).reshape(2)
    factor = np.power(F(2), F(scale))
    size = np.asarray(image_size, np.int32).astype(F)
    new_size = (size * factor).astype(np.int32)
    actual = new_size.astype(F) / size
    cx = F(center[0]) * actual[1]
    cy = F(center[1]) * actual[0]
    return new_size, actual, np.array([cx, cy], F).astype(np.int32)


def crop_origin(new_size, center, S, trans_max):
    """(x0, y0) of the crop in scaled-image coordinates and whether tf.slice would accept it"""
    margin = int(S / 2)
    safe = margin + trans_max + 50
    start = center.astype(np.int64) + safe - margin            # in the padded image
    ok = bool(np.all(new_size > 0) and start[0] >= 0 and start[1] >= 0
              and start[0] + S <= new_size[1] + 2 * safe and start[1] + S <= new_size[0] + 2 * safe)
    return int(center[0]) - margin, int(center[1]) - margin, ok


def crop_from_scaled(scaled, x0, y0, S):
    """edge pad + slice: crop pixel (x, y) is the scaled image at the clamped (x0 + x, y0 + y)"""
    ys = np.clip(np.arange(S) + y0, 0, scaled.shape[0] - 1)
    xs = np.clip(np.arange(S) + x0, 0, scaled.shape[1] - 1)
    return scaled[ys][:, xs]


def pixels(image, new_h, new_w, x0, y0, S, flip=False, transform=None):
    """One frame of hmmr_tube_augment: image [H,W,3] float32 in [0,1] -> [S,S,3] float32 in [-1,1]"""
    crop = crop_from_scaled(tf_resize_bilinear(image, new_h, new_w), x0, y0, S)
    if transform is not None:
        crop = tf_rotate_bilinear(crop, transform)
    if flip:
        crop = crop[:, ::-1]
    return (crop - F(0.5)) * F(2.0)


def u8_to_float(images):
    """what the writers feed for a uint8 frame: float32(image / 255.)"""
    return (np.asarray(images, np.uint8).astype(np.float64) / 255.0).astype(F)


def batch_rodrigues(theta):
    """src/tf_smpl/batch_lbs.py:42-60 for one axis-angle vector, float32"""
    theta = np.asarray(theta, F).reshape(3)
    angle = np.sqrt(np.sum((theta + F(1e-8)) * (theta + F(1e-8))))
    r = theta / angle
    c, s = np.cos(angle), np.sin(angle)
    skew = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]], F)
    return (c * np.eye(3, dtype=F) + (F(1) - c) * np.outer(r, r) + s * skew).astype(F)


def batch_rot2aa(R):
    """src/tf_smpl/batch_lbs.py:63-105 for one matrix, float32"""
    R = np.asarray(R, F)
    c = np.clip(F(0.5) * (np.trace(R) - F(1)), F(-1), F(1))
    theta = np.arccos(c)
    m = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], F)
    denom = np.sqrt(np.sum(m * m))
    with np.errstate(invalid="ignore", divide="ignore"):
        axis = m if abs(theta) < 0.00001 else m / denom
    return (theta * axis).astype(F)


def reflect_pose(pose):
    sign = np.tile(np.array([1, -1, -1], F), 24)
    return np.asarray(pose, F)[FLIP_POSE] * sign


def reflect_joints3d(joints):
    j = np.asarray(joints, F)[FLIP_J3D] * np.array([-1, 1, 1], F)
    return j - np.mean(j, axis=0)


def frame(image, image_size, label, center, pose, gt3d, trans, scale, rotate, flip, S, trans_max, rotate_max):
    """preprocess_image for one frame.  label [3,25]; returns (crop [S,S,3], label [3,25], pose [72], gt3d [14,3],
    centre [2] int32) or raises ValueError where tf.slice would."""
    label = np.asarray(label, F)
    pose, gt3d = np.asarray(pose, F), np.asarray(gt3d, F)
    new_size, actual, c = scale_geometry(image_size, center, trans, scale)
    x0, y0, ok = crop_origin(new_size, c, S, trans_max)
    if not ok:
        raise ValueError("the crop leaves the padded image")
    margin = int(S / 2)
    safe = margin + trans_max + 50
    kx = label[0] * actual[1] + F(safe) - F(c[0] + safe - margin)
    ky = label[1] * actual[0] + F(safe) - F(c[1] + safe - margin)
    vis = label[2]
    transform = None
    if rotate_max != 0:
        theta = F(rotate)
        transform = rotate_transform(theta, S)
        cs, sn = np.cos(theta), np.sin(theta)
        R = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]], F)
        mid = F(S) * F(0.5)
        k0 = np.stack([kx - mid, ky - mid])                       # [2,N]
        kr = (k0.T @ R[:2, :2]).T + mid
        kx, ky = kr[0], kr[1]
        mean = np.mean(gt3d)
        gt3d = (gt3d - mean) @ R + mean
        pose = np.concatenate([batch_rot2aa(R.T @ batch_rodrigues(pose[:3])), pose[3:]]).astype(F)
    if flip:
        kx = F(S) - kx - F(1)
        kx, ky, vis = kx[FLIP_KP], ky[FLIP_KP], vis[FLIP_KP]
        pose, gt3d = reflect_pose(pose), reflect_joints3d(gt3d)
    fvis = (vis > 0).astype(F)
    out_label = fvis * np.stack([F(2.0) * (kx / F(S)) - F(1.0), F(2.0) * (ky / F(S)) - F(1.0), fvis])
    crop = pixels(np.asarray(image, F), int(new_size[0]), int(new_size[1]), x0, y0, S, flip, transform)
    return crop, out_label.astype(F), pose.astype(F), gt3d.astype(F), c
