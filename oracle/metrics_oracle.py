"""ORACLE (test infrastructure only -- never imported by the product path).

NumPy float64 restatement of the error metrics of the reference's src/evaluation/eval_util.py, written from the
formulas:
  * `align_by_pelvis`        joints minus the midpoint of the two hips (LSP ids 3 and 2)
  * `similarity_transform`   the orthogonal Procrustes problem: K = X1 X2^T = U S V^T (np.linalg.svd of K itself),
                             R = V diag(1, 1, sign det(U V^T)) U^T, scale = tr(R K) / |X1|^2, t = mu2 - scale R mu1
  * `compute_error_3d`       MPJPE after pelvis alignment and after Procrustes, per (visible) frame
  * `compute_accel`, `accel_error_all`, `compute_error_accel`   second differences, before / after the visibility filter
  * `compute_error_verts`    mean vertex distance per frame
PARITY: PINNED -- tests/test_metrics_oracle.py checks every array of tests/golden/reference_metrics.npz to 1e-12 and
of tests/golden/reference_metrics_edges.npz (the degenerate families below, recorded from the reference's own functions
by tests/golden/make_metrics_edges_golden.py) to 1e-9.

The second half builds the test inputs that the recipe and the GPU tests share: `family(name, n, k, seed)` returns the
float32 (gt, pred) of one degenerate Procrustes family, `well_conditioned` is the filter that drops the frames whose
PA-MPJPE is itself unstable under one float32 ulp of input noise (a near-tie between the rotation and the reflection).
"""
import numpy as np

LEFT_HIP, RIGHT_HIP = 3, 2


def align_by_pelvis(joints, left_id=LEFT_HIP, right_id=RIGHT_HIP):
    joints = np.asarray(joints, np.float64)
    pelvis = (joints[left_id] + joints[right_id]) / 2.0
    return joints - pelvis[None]


def similarity_transform(s1, s2):
    """s1, s2 [k,3] -> s1 after the similarity transform (scale, rotation, translation) that brings it closest to s2."""
    s1, s2 = np.asarray(s1, np.float64).T, np.asarray(s2, np.float64).T          # 3 x k
    mu1, mu2 = s1.mean(axis=1, keepdims=True), s2.mean(axis=1, keepdims=True)
    x1, x2 = s1 - mu1, s2 - mu2
    var1 = np.sum(x1 ** 2)
    K = x1 @ x2.T
    U, _, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ V.T))
    R = V @ Z @ U.T
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.trace(R @ K) / var1
        t = mu2 - scale * (R @ mu1)
        out = scale * (R @ s1) + t
    return out.T


def frame_errors(gt, pred, left_id=LEFT_HIP, right_id=RIGHT_HIP):
    """One frame [k,3] x 2 -> (MPJPE after pelvis alignment, MPJPE after Procrustes)."""
    g, p = align_by_pelvis(gt, left_id, right_id), align_by_pelvis(pred, left_id, right_id)
    e = np.mean(np.sqrt(np.sum((g - p) ** 2, axis=1)))
    pa = np.mean(np.sqrt(np.sum((g - similarity_transform(p, g)) ** 2, axis=1)))
    return e, pa


def compute_error_3d(gt3ds, preds, vis=None, left_id=LEFT_HIP, right_id=RIGHT_HIP):
    assert len(gt3ds) == len(preds)
    errors, errors_pa = [], []
    for i in range(len(preds)):
        if vis is None or vis[i]:
            e, pa = frame_errors(np.asarray(gt3ds[i]).reshape(-1, 3), preds[i], left_id, right_id)
            errors.append(e)
            errors_pa.append(pa)
    return np.array(errors, np.float64), np.array(errors_pa, np.float64)


def _second_difference(x):
    x = np.asarray(x, np.float64)
    return x[:-2] - 2.0 * x[1:-1] + x[2:]


def compute_accel(joints):
    """[n,k,3] -> [n-2]: mean over the joints of |X[i-1] - 2 X[i] + X[i+1]|."""
    return np.mean(np.linalg.norm(_second_difference(joints), axis=2), axis=1)


def accel_error_all(joints_gt, joints_pred):
    """[n-2] acceleration errors of every interior frame, BEFORE the visibility filter."""
    return np.mean(np.linalg.norm(_second_difference(joints_pred) - _second_difference(joints_gt), axis=2), axis=1)


def accel_visibility(vis, n):
    """Interior frame i (stencil i, i+1, i+2) stays when none of its three frames is invisible."""
    if vis is None:
        return np.ones(max(n - 2, 0), bool)
    invis = np.logical_not(np.asarray(vis).astype(bool))
    return np.array([not invis[i:i + 3].any() for i in range(max(n - 2, 0))], bool)


def compute_error_accel(joints_gt, joints_pred, vis=None):
    return accel_error_all(joints_gt, joints_pred)[accel_visibility(vis, len(joints_pred))]


def compute_error_verts(verts_gt, verts_pred):
    d = np.asarray(verts_gt, np.float64) - np.asarray(verts_pred, np.float64)
    return np.mean(np.sqrt(np.sum(d ** 2, axis=2)), axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the degenerate Procrustes families (float32 inputs at metre scale: gt ~ N(0, 0.3), pred = gt + N(0, 0.05))

FAMILIES = ("planar_pred_axis", "planar_pred_rot", "planar_gt_axis", "planar_gt_rot", "planar_both_axis",
            "planar_both_rot", "thick_1e-2", "thick_1e-4", "thick_1e-7", "collinear_pred", "identical", "mirror",
            "scale_1e-3", "scale_1e3", "offset_1000", "equal_sv")
NONFINITE_FAMILIES = ("coincident_pred",)          # var1 == 0: the reference divides 0 by 0


def random_rotations(rng, n):
    q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    return q * np.sign(np.linalg.det(q))[:, None, None]


def family(name, n, k=14, seed=0):
    """(gt, pred) float32 [n,k,3] of one family; what a family fixes holds exactly in the float32 values wherever the
    construction allows it (z == 0 planes, pred == gt, powers of ten applied before the rounding)."""
    rng = np.random.default_rng([seed, (FAMILIES + NONFINITE_FAMILIES).index(name)])
    gt = rng.normal(size=(n, k, 3)) * 0.3
    pred = gt + rng.normal(size=(n, k, 3)) * 0.05
    R = random_rotations(rng, n)
    rot = lambda x: np.einsum("nab,nkb->nka", R, x)
    if name.startswith("planar_"):
        which, how = name.split("_")[1:]
        if which in ("pred", "both"):
            pred[..., 2] = 0.0
        if which in ("gt", "both"):
            gt[..., 2] = 0.0
        if how == "rot":                                       # the same rotation for both: the plane is shared
            gt, pred = rot(gt), rot(pred)
    elif name.startswith("thick_"):
        pred[..., 2] = rng.normal(size=(n, k)) * float(name.split("_")[1])
        gt, pred = rot(gt), rot(pred)
    elif name == "collinear_pred":
        d = rng.normal(size=(n, 1, 3))
        pred = rng.normal(size=(n, k, 1)) * 0.3 * d / np.linalg.norm(d, axis=2, keepdims=True) + rng.normal(size=(n, 1, 3)) * 0.1
    elif name == "identical":
        pred = gt.copy()
    elif name == "mirror":
        pred = pred * np.array([-1.0, 1.0, 1.0])
    elif name.startswith("scale_"):
        pred = pred * float(name.split("_")[1])
    elif name == "offset_1000":
        gt, pred = gt + 1000.0, pred + 1000.0
    elif name == "equal_sv":
        # gt symmetric under a 90-degree turn about z: orbits of four points, the rest on the axis -> X2 X2^T = diag(a, a, b)
        turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        for j in range(k):
            if j % 4 and j < 4 * (k // 4):
                gt[:, j] = gt[:, j - 1] @ turn.T
            elif j >= 4 * (k // 4):
                gt[:, j, :2] = 0.0
        noise = rng.normal(size=(n, k, 3)) * 0.05
        noise[::2] = 0.0                                       # even frames: exactly equal, odd frames: nearly equal
        pred = 0.8 * rot(gt) + rot(noise) + 0.1
    elif name == "coincident_pred":
        pred = np.broadcast_to(rng.normal(size=(n, 1, 3)) * 0.3, (n, k, 3)).copy()
    else:
        raise KeyError(name)
    return gt.astype(np.float32), pred.astype(np.float32)


def well_conditioned(gt, pred, seed=0, bound=1e-7, offset=0.0):
    """[n] bool: the oracle's PA-MPJPE of the frame moves by less than `bound` when every input coordinate is moved by
    one float32 ulp, for three random sign patterns.  A frame that fails sits on a near-tie between the rotation and the
    reflection solution: no arithmetic can be held to 1e-6 there.
    offset: a translation common to every coordinate that the pelvis alignment removes; the ulp is then that of the
    coordinate without it (at 1000 m one float32 ulp is 6e-5 m, which moves every well-posed error by more than the bound
    and would say nothing about the tie)."""
    gt, pred = np.asarray(gt, np.float32), np.asarray(pred, np.float32)
    rng = np.random.default_rng([seed, 77])
    base = compute_error_3d(gt, pred)[1]
    keep = np.isfinite(base)
    for _ in range(3):
        moved = []
        for x in (gt, pred):
            ulp = np.spacing(np.abs(x.astype(np.float64) - offset).astype(np.float32)).astype(np.float64)
            moved.append(x.astype(np.float64) + np.where(rng.random(x.shape) < 0.5, ulp, -ulp))
        with np.errstate(invalid="ignore"):
            keep &= np.abs(compute_error_3d(moved[0], moved[1])[1] - base) < bound
    return keep
