"""Float64 restatement of the evaluation this project adds on the device: the keypoint metrics of
src/evaluation/eval_util.py (compute_error_kp, compute_opt_cam_with_vis), the rotation maps it takes from OpenCV, and
compute_errors_batched / test_sequence_const of src/evaluation/eval.py.  Written from the formulas; the 3D metrics come from
oracle/metrics_oracle.py.  tests/golden/make_eval_golden.py executes the reference's own functions on the same inputs and
tests/test_eval_oracle.py holds this file to them at 1e-12, so the GPU tests and tools may use either.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import metrics_oracle as MO          # noqa: E402


# ---- rotations -----------------------------------------------------------------------------------------------------------------
def rodrigues64(w):
    """Axis-angle [..., 3] -> rotation matrices [..., 3, 3]: R = I + sin(t) K + (1 - cos(t)) K^2, K = skew(w / t); the exact map
    (no epsilon), with the series limit at t = 0."""
    w = np.asarray(w, np.float64)
    flat = w.reshape(-1, 3)
    out = np.empty((len(flat), 3, 3))
    for i, v in enumerate(flat):
        t = np.linalg.norm(v)
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        if t < 1e-12:
            out[i] = np.eye(3) + K
        else:
            K = K / t
            out[i] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K.dot(K)
    return out.reshape(w.shape[:-1] + (3, 3))


def log_map64(R):
    """Rotation matrices [..., 3, 3] -> axis-angle [..., 3] with |w| <= pi: the angle from atan2(|antisymmetric part|, (trace - 1) / 2);
    the axis from the antisymmetric part up to a quarter turn and from the symmetric part (R + R^T) / 2 = c I + (1 - c) n n^T beyond."""
    R = np.asarray(R, np.float64)
    flat = R.reshape(-1, 3, 3)
    out = np.empty((len(flat), 3))
    for i, M in enumerate(flat):
        v = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2.0
        s, c = np.linalg.norm(v), (np.trace(M) - 1.0) / 2.0
        angle = np.arctan2(s, c)
        if c >= 0:
            out[i] = v * (angle / s if s > 1e-8 else 1.0)
            continue
        m = int(np.argmax(np.diag(M)))
        ax = np.zeros(3)
        ax[m] = np.sqrt(max((M[m, m] - c) / (1.0 - c), 0.0))
        if ax[m] > 0:
            for a in range(3):
                if a != m:
                    ax[a] = (M[m, a] + M[a, m]) / 2.0 / ((1.0 - c) * ax[m])
        else:
            ax[m] = 1.0
        ax /= np.linalg.norm(ax)
        out[i] = (-1.0 if ax.dot(v) < 0 else 1.0) * angle * ax
    return out.reshape(R.shape[:-2] + (3,))


class Cv2(object):
    """Stand-in for the one OpenCV function eval_util.py calls: Rodrigues in both directions, float64."""

    @staticmethod
    def Rodrigues(x):
        x = np.asarray(x, np.float64)
        if x.shape == (3, 3):
            return log_map64(x).reshape(3, 1), None
        return rodrigues64(x.reshape(3)), None


# ---- keypoints -------------------------------------------------------------------------------------------------------------------
def to_image_space32(kps_pred, img_size):
    """(x + 1) * 0.5 * img_size in float32, the arithmetic of eval.py:131 on the network's float32 output."""
    x = np.asarray(kps_pred, np.float32)
    return (x + np.float32(1)) * np.float32(0.5) * np.float32(img_size)


def opt_cam(got, want, vis):
    """[scale, tx, ty] of compute_opt_cam_with_vis and the aligned points."""
    got, want, vis = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(vis).astype(bool)
    nv = vis.sum()
    mu1 = (got * vis[:, None]).sum(0) / nv
    mu2 = (want * vis[:, None]).sum(0) / nv
    x, y = (got - mu1) * vis[:, None], (want - mu2) * vis[:, None]
    scale = np.trace(np.linalg.inv(x.T.dot(x) + 1e-6 * np.identity(2)).dot(x.T.dot(y))) / 2.0
    trans = mu2 / scale - mu1
    return scale * (got + trans), np.hstack((scale, trans))


def compute_error_kp(kps_gt, kps_pred, alpha=0.05, min_visible=6, with_cam=False):
    """Per frame: mean visible-keypoint distance, the same after the optimal camera, share of aligned distances below alpha; NaN
    where fewer than min_visible keypoints (or none) are visible.  kps_pred in pixels."""
    e, epa, pck, cams = [], [], [], []
    for gt, pred in zip(np.asarray(kps_gt, np.float64), np.asarray(kps_pred, np.float64)):
        vis = gt[:, 2] != 0
        if vis.sum() == 0 or vis.sum() < min_visible:
            e.append(np.nan), epa.append(np.nan), pck.append(np.nan), cams.append(np.full(3, np.nan))
            continue
        aligned, cam = opt_cam(pred, gt[:, :2], vis)
        d = np.linalg.norm(gt[vis, :2] - aligned[vis], axis=1)
        e.append(np.mean(np.linalg.norm(gt[vis, :2] - pred[vis], axis=1)))
        epa.append(np.mean(d)), pck.append(np.mean(d < alpha)), cams.append(cam)
    return (e, epa, pck, np.array(cams)) if with_cam else (e, epa, pck)


def aligned_distances(kps_gt, kps_pred):
    """Every visible keypoint's distance after the alignment, all frames with a visible keypoint (the PCK margin check)."""
    out = []
    for gt, pred in zip(np.asarray(kps_gt, np.float64), np.asarray(kps_pred, np.float64)):
        vis = gt[:, 2] != 0
        if vis.sum():
            out.append(np.linalg.norm(gt[vis, :2] - opt_cam(pred, gt[:, :2], vis)[0][vis], axis=1))
    return np.concatenate(out)


# ---- eval.py -----------------------------------------------------------------------------------------------------------------------
def compute_errors_batched(kps_gt, kps_pred, joints_gt=None, joints_pred=None, poses_gt=None, poses_pred=None, shape_gt=None,
                           shapes_pred=None, img_size=224, has_3d=False, min_visible=6, compute_mesh=False, smpl=None):
    """The dictionary of eval.py:114-193.  smpl(poses [N,72], shapes [N,10]) -> vertices [N,V,3]."""
    f64 = lambda a: np.asarray(a, np.float64)
    e, epa, pck = compute_error_kp(kps_gt, to_image_space32(kps_pred, img_size), 0.05 * img_size, min_visible)
    out = {"accel": MO.compute_accel(f64(joints_pred)), "kp": e, "kp_pa": epa, "kp_pck": pck}
    if not has_3d:
        return out
    vis = np.sum(f64(kps_gt)[:, :14, 2], axis=1) > min_visible
    gt3 = f64(joints_gt).reshape(len(joints_gt), -1, 3)
    mesh_posed = mesh_tpose = -1
    if compute_mesh:
        n = len(poses_gt)
        shapes_gt = np.tile(f64(shape_gt), (n, 1))
        aa = log_map64(f64(poses_pred)).reshape(n, 72)
        zero = np.zeros((n, 72))
        mesh_tpose = MO.compute_error_verts(smpl(zero, shapes_gt)[vis], smpl(zero, f64(shapes_pred))[vis])
        mesh_posed = MO.compute_error_verts(smpl(f64(poses_gt), shapes_gt)[vis], smpl(aa, f64(shapes_pred))[vis])
    j, jpa = MO.compute_error_3d(gt3, f64(joints_pred), vis)
    out.update({"accel_error": MO.compute_error_accel(gt3, f64(joints_pred), vis), "mesh_posed": mesh_posed,
                "mesh_tpose": mesh_tpose, "pose": -1, "joints": j, "joints_pa": jpa, "shape": -1})
    return out


def score_old_way(preds, data, smpl, img_size=224, min_visible=6, compute_mesh=True):
    """What a user did before the device path: the downloaded dictionary scored on the host (tools/eval_bench.py)."""
    return compute_errors_batched(data["kps"], preds["kps"], data["gt3ds"], preds["joints"][:, :14], data["poses"], preds["poses"],
                                  data["shape"], preds["shapes"], img_size, True, min_visible, compute_mesh, smpl)


# ---- stub tubes for the accumulation tests (no device, no model) -------------------------------------------------------------------
STUB_DATASETS = {"3dpw": (("a.tfrecord", 2), ("b.tfrecord", 1)), "penn_action": (("c.tfrecord", 3),)}     # tubes per tfrecord


def stub_errors(seed, has_3d):
    """A tube's error dictionary with the shapes, NaN entries and -1 placeholders compute_errors_batched returns."""
    rng = np.random.default_rng(seed)
    n = 6 + seed % 3
    kp = rng.uniform(1, 9, n)
    kp[seed % n] = np.nan
    out = {"accel": rng.uniform(0, 1, n - 2), "kp": list(kp), "kp_pa": list(kp * 0.5), "kp_pck": list(rng.uniform(0, 1, n))}
    if has_3d:
        out.update({"accel_error": rng.uniform(0, 1, n - 3), "mesh_posed": rng.uniform(0, 1, n - 1), "mesh_tpose": -1, "pose": -1,
                    "joints": list(rng.uniform(0, 1, n - 1)), "joints_pa": list(rng.uniform(0, 1, n - 1)), "shape": -1})
    return out


def stub_tubes(tf_dir="tf"):
    """{dataset: [(tf_path, p_id, seed)]} in the order main() visits them."""
    out, seed = {}, 0
    for dataset, paths in STUB_DATASETS.items():
        out[dataset] = []
        for name, tubes in paths:
            for p_id in range(tubes):
                out[dataset].append((os.path.join(tf_dir, dataset, "test", name), p_id, seed))
                seed += 1
    return out
