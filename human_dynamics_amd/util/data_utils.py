"""Mirror of the augmentation half of src/util/data_utils.py: the label side and the geometry of the tube augmentor in
NumPy float32, over all frames of a tube at once.  The pixels are csrc/tube.hip's (util/tube_augmentation.py launches it).

Float32 on purpose: the reference runs in TensorFlow float32 and its truncations to int32 (the scaled size, the scaled
centre) decide which pixels a crop holds, so the integers are computed with the same float32 operations in the same order.
Pinned to the reference's own code by tests/golden/reference_tube.npz (tests/test_tube_oracle.py).  What cannot be pinned:
TensorFlow's random stream -- the walks below take NumPy draws, or the caller's -- and TF's `pow` / `cos` / `sin`, for
which NumPy's float32 routines stand in.
"""
from __future__ import annotations

import numpy as np

F = np.float32

# flip_image's 25-joint gather (data_utils.py:616-628): every joint takes its left / right partner -- the 12 limb joints
# mirrored, neck, head and nose kept, then the eye, ear, big-toe, small-toe and last left / right pairs swapped
KP_SWAP_INDS = np.array([5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 16, 15, 18, 17, 20, 19, 22, 21, 24, 23])
J3D_SWAP_INDS = np.array([5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13])


def _pose_swap_inds():
    """reflect_pose's gather, built the way its docstring says (data_utils.py:646-662)"""
    right, left = [11, 8, 5, 2, 14, 17, 19, 21, 23], [10, 7, 4, 1, 13, 16, 18, 20, 22]
    joint = np.arange(24)
    joint[right], joint[left] = left, right
    return (joint[:, None] * 3 + np.arange(3)).reshape(-1)


POSE_SWAP_INDS = _pose_swap_inds()
POSE_SIGN_FLIP = np.tile(np.array([1, -1, -1], F), 24)


def rescale_image(image):
    """[0, 1] -> [-1, 1] (data_utils.py:370-378)"""
    return (np.asarray(image, F) - F(0.5)) * F(2.0)


def walk_from_draws(minval, maxval, start, steps, dtype=np.float32):
    """The reflected walk of bounded_random_walk from its two uniform draws: start [1,dim] in [minval, maxval) and
    steps [T,dim] in [delta_min, delta_max), as tf.random_uniform returned them (data_utils.py:821-835)."""
    dtype = np.dtype(dtype)
    start, steps = np.asarray(start, dtype), np.asarray(steps, dtype)
    lo, size, period = dtype.type(minval), dtype.type(maxval - minval), dtype.type(2 * (maxval - minval))   # Python arithmetic first
    walk = np.cumsum(steps, axis=0, dtype=dtype)
    return (np.abs((walk + start - lo + size) % period - size) + lo).astype(dtype)


def _uniform(rng, shape, minval, maxval, dtype):
    if np.dtype(dtype).kind == "i":
        return rng.integers(int(minval), int(maxval), size=shape).astype(dtype)
    return rng.random(size=shape, dtype=np.float32) * F(maxval - minval) + F(minval)      # tf.random_uniform's own scaling


def bounded_random_walk(minval, maxval, delta_min, delta_max, T, dtype=np.float32, dim=1, rng=None):
    """[T,dim] random walk that stays inside [minval, maxval) with steps in [delta_min, delta_max) (data_utils.py:787-835).
    The draws are NumPy's (rng: a numpy Generator; None = a fresh one), not TensorFlow's.

    One departure from the reference, for integer walks only: its reflection formula (walk_from_draws) returns maxval ITSELF
    when the unreflected position is a multiple of 2 * size, although every caller passes maxval as an exclusive bound
    ("trans_max + 1  # Upper-bound is exclusive", tube_augmentation.py:62) -- the reference's translation walk reaches
    trans_max + 1 (reference_tube.npz records one such frame).  A walk drawn here keeps the bound its callers state: that one
    lattice point is folded onto maxval - 1, which lengthens no step.  walk_from_draws stays the reference's formula, so that
    a recorded walk is replayed as the reference computed it."""
    if maxval <= minval:
        return np.ones((T, dim), F) * F(minval)
    rng = np.random.default_rng() if rng is None else rng
    if minval == delta_min and maxval == delta_max:            # "the old data augmentation": independent draws per frame
        return _uniform(rng, (T, dim), minval, maxval, dtype)
    start = _uniform(rng, (1, dim), minval, maxval, dtype)
    steps = _uniform(rng, (T, dim), delta_min, delta_max, dtype)
    walk = walk_from_draws(minval, maxval, start, steps, dtype)
    if np.dtype(dtype).kind == "i":
        walk = np.minimum(walk, np.dtype(dtype).type(maxval - 1))
    return walk


def jitter_center(center, rand_trans):
    """centres [T,2] int32 (x, y) + the translation walk (data_utils.py:512-521)"""
    return np.asarray(center, np.int32).reshape(-1, 2) + np.asarray(rand_trans, np.int32).reshape(-1, 2)


def jitter_scale(image_size, keypoints, center, scale_factor):
    """The integers and labels of jitter_scale (data_utils.py:524-548) for T frames: image_size [T,2] (h, w), keypoints
    [T,2,N], center [T,2] (x, y) int32, scale_factor [T] (the exponent).  Returns new_size [T,2] int32 (h, w), actual_factor
    [T,2] float32, the scaled keypoints [T,2,N] and the scaled centre [T,2] truncated to int32."""
    size = np.asarray(image_size, np.int32).reshape(-1, 2).astype(F)
    factor = np.power(F(2), np.asarray(scale_factor, F).reshape(-1, 1))
    new_size = (size * factor).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        actual = new_size.astype(F) / size
    kp = np.asarray(keypoints, F)
    x = kp[:, 0, :] * actual[:, 1:2]
    y = kp[:, 1, :] * actual[:, 0:1]
    c = np.asarray(center, np.int32).reshape(-1, 2).astype(F)
    with np.errstate(invalid="ignore"):
        new_center = np.stack([c[:, 0] * actual[:, 1], c[:, 1] * actual[:, 0]], 1).astype(np.int32)
    return new_size, actual, np.stack([x, y], 1), new_center


def batch_rodrigues(theta):
    """[N,3] axis-angle -> [N,3,3] (src/tf_smpl/batch_lbs.py:42-60), float32"""
    theta = np.asarray(theta, F).reshape(-1, 3)
    t = theta + F(1e-8)
    angle = np.sqrt(np.sum(t * t, axis=1))[:, None]
    r = theta / angle
    c, s = np.cos(angle)[:, :, None], np.sin(angle)[:, :, None]
    outer = r[:, :, None] * r[:, None, :]
    skew = np.zeros((len(r), 3, 3), F)
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 0] = -r[:, 2], r[:, 1], r[:, 2]
    skew[:, 1, 2], skew[:, 2, 0], skew[:, 2, 1] = -r[:, 0], -r[:, 1], r[:, 0]
    return c * np.eye(3, dtype=F) + (F(1) - c) * outer + s * skew


def batch_rot2aa(Rs):
    """[N,3,3] -> [N,3] axis-angle (src/tf_smpl/batch_lbs.py:63-105): below 1e-5 rad the un-normalised axis is kept"""
    Rs = np.asarray(Rs, F)
    cos = np.clip(F(0.5) * (np.trace(Rs, axis1=1, axis2=2) - F(1)), F(-1), F(1))
    theta = np.arccos(cos)
    m = np.stack([Rs[:, 2, 1] - Rs[:, 1, 2], Rs[:, 0, 2] - Rs[:, 2, 0], Rs[:, 1, 0] - Rs[:, 0, 1]], 1)
    denom = np.sqrt(np.sum(m * m, axis=1))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        axis = np.where((np.abs(theta) < 0.00001)[:, None], m, m / denom)
    return theta[:, None] * axis


def rotate_transforms(theta, image_size):
    """[T,6] float32 rows [cos, -sin, xoff, sin, cos, yoff]: the output -> input transforms tf.contrib.image.rotate builds for
    a square image (angles_to_projective_transforms), as hmmr_tube_augment reads them"""
    theta = np.asarray(theta, F).reshape(-1)
    c, s = np.cos(theta), np.sin(theta)
    m = F(image_size - 1)
    xoff = (m - (c * m - s * m)) / F(2)
    yoff = (m - (s * m + c * m)) / F(2)
    return np.stack([c, -s, xoff, s, c, yoff], 1).astype(F)


def rotate_labels(keypoints, image_size, gt3d, pose, theta):
    """The label part of rotate_img (data_utils.py:702-762) for T frames: keypoints [T,2,N] in crop pixels rotate about
    image_size * 0.5, gt3d [T,14,3] about its SCALAR mean, the root pose becomes rot2aa(R^T rodrigues(pose[:3])) -- the
    reference's conventions as they are.  theta [T]."""
    theta = np.asarray(theta, F).reshape(-1)
    c, s = np.cos(theta), np.sin(theta)
    R = np.zeros((len(theta), 3, 3), F)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = c, -s, s, c, 1
    mid = F(image_size) * F(0.5)
    kp0 = np.asarray(keypoints, F) - mid
    kp_rot = np.swapaxes(np.matmul(np.swapaxes(kp0, 1, 2), R[:, :2, :2]), 1, 2) + mid
    gt3d, pose = np.asarray(gt3d, F), np.asarray(pose, F)
    mean = np.mean(gt3d, axis=(1, 2), keepdims=True)
    gt3d_rot = np.matmul(gt3d - mean, R) + mean
    R0_new = np.matmul(np.swapaxes(R, 1, 2), batch_rodrigues(pose[:, :3]))
    pose_rot = np.concatenate([batch_rot2aa(R0_new), pose[:, 3:]], 1)
    return kp_rot.astype(F), gt3d_rot.astype(F), pose_rot.astype(F)


def reflect_pose(pose):
    """[..., 72]: swap left and right joints, negate the y and z components (data_utils.py:639-684)"""
    return np.asarray(pose, F)[..., POSE_SWAP_INDS] * POSE_SIGN_FLIP


def reflect_joints3d(joints):
    """[..., 14, 3]: swap left and right, negate x, subtract the mean joint (data_utils.py:687-699)"""
    j = np.asarray(joints, F)[..., J3D_SWAP_INDS, :] * np.array([-1, 1, 1], F)
    return j - np.mean(j, axis=-2, keepdims=True)


def flip_labels(kp, image_size, pose=None, gt3d=None):
    """The label part of flip_image (data_utils.py:601-636): kp [T,3,N] in crop pixels, new_x = image_size - x - 1, then the
    left / right gather (N = 25)."""
    kp = np.asarray(kp, F)
    new_kp = np.concatenate([(F(image_size) - kp[:, 0:1, :]) - F(1), kp[:, 1:, :]], 1)[:, :, KP_SWAP_INDS]
    if pose is None:
        return new_kp
    return new_kp, reflect_pose(pose), reflect_joints3d(gt3d)
