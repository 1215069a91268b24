"""Mirror of the error metrics of src/evaluation/eval_util.py, evaluated on the device
(csrc/eval_metrics.hip) so predictions can be scored where the SMPL stage left them.

Same function names, arguments and return values as the reference (lists / arrays of per-frame
errors); inputs may be NumPy arrays or device tensors.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib as L

LEFT_HIP, RIGHT_HIP = 3, 2            # LSP order, eval_util.py:166-167


def _dev(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device, torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _joint_metrics(gt, pred, device, want_err=True, want_accel=True):
    lib = L.load()
    pred = _dev(pred, device)
    n, k = pred.shape[0], pred.shape[1]
    gt = _dev(gt, device) if gt is not None else None
    mp = torch.empty(n, device=device) if (want_err and gt is not None) else None
    pa = torch.empty(n, device=device) if (want_err and gt is not None) else None
    ac = torch.empty(max(n - 2, 0), device=device) if want_accel else None
    ae = torch.empty(max(n - 2, 0), device=device) if (want_accel and gt is not None) else None
    L.check(lib.hmmr_eval_joints(L.ptr(gt), pred.data_ptr(), n, k, LEFT_HIP, RIGHT_HIP, L.ptr(mp), L.ptr(pa),
                                 L.ptr(ac), L.ptr(ae), _stream(device)), "hmmr_eval_joints")
    return mp, pa, ac, ae


def compute_accel(joints, device="cuda:0"):
    """Acceleration of 3D joints (Nx25x3) -> (N-2) (eval_util.py:14-27)."""
    return _joint_metrics(None, joints, device, want_err=False)[2].cpu().numpy()


def compute_error_3d(gt3ds, preds, vis=None, device="cuda:0"):
    """MPJPE after pelvis alignment and after Procrustes, per visible frame (eval_util.py:30-60)."""
    assert len(gt3ds) == len(preds)
    mp, pa, _, _ = _joint_metrics(np.asarray(gt3ds).reshape(len(gt3ds), -1, 3) if not isinstance(gt3ds, torch.Tensor)
                                  else gt3ds, preds, device, want_accel=False)
    mp, pa = mp.cpu().numpy(), pa.cpu().numpy()
    keep = np.ones(len(mp), bool) if vis is None else np.asarray(vis).astype(bool)
    return list(mp[keep]), list(pa[keep])


def compute_error_accel(joints_gt, joints_pred, vis=None, device="cuda:0"):
    """Acceleration error per interior frame, dropping every frame whose 3-frame stencil touches an
    invisible frame (eval_util.py:63-94)."""
    ae = _joint_metrics(joints_gt, joints_pred, device, want_err=False)[3].cpu().numpy()
    if vis is None:
        new_vis = np.ones(len(ae), dtype=bool)
    else:
        invis = np.logical_not(np.asarray(vis).astype(bool))
        new_invis = np.logical_or(invis, np.logical_or(np.roll(invis, -1), np.roll(invis, -2)))[:-2]
        new_vis = np.logical_not(new_invis)
    return ae[new_vis]


def compute_error_verts(verts_gt, verts_pred, device="cuda:0"):
    """Mean per-vertex distance per frame (eval_util.py:140-155)."""
    lib = L.load()
    g, p = _dev(verts_gt, device), _dev(verts_pred, device)
    assert g.shape == p.shape
    n, nv = g.shape[0], g.shape[1]
    out = torch.empty(n, device=device)
    L.check(lib.hmmr_eval_verts(g.data_ptr(), nv * 3, p.data_ptr(), nv * 3, n, nv, out.data_ptr(), _stream(device)),
            "hmmr_eval_verts")
    return out.cpu().numpy()


# ---- keypoint metrics (csrc/eval_metrics.hip: hmmr_eval_kps) --------------------------------------------------------------------
def _rows(x, device, inner):
    """x [n, ..., *inner] as an fp32 device tensor whose rows can be read in place: a device view whose trailing dimensions are
    packed (a field of the packed per-frame record, or the first k joints of one) is used as it is, anything else is copied.
    Returns (tensor, row stride in floats)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2):
        x = _dev(x, device)
    want, ok = 1, x.dim() >= 2
    for d in range(x.dim() - 1, 0, -1):
        ok = ok and (x.shape[d] == 1 or x.stride(d) == want)
        want *= x.shape[d]
    if not ok or (x.shape[0] > 1 and x.stride(0) < want):
        x = x.contiguous()
    assert tuple(x.shape[-len(inner):]) == tuple(inner), (tuple(x.shape), inner)
    return x, (x.stride(0) if x.shape[0] > 1 else want)


def kp_metrics_device(kps_gt, kps_pred, alpha, min_visible, img_size=0, want_cam=False, device="cuda:0"):
    """Per-frame device tensors (err_kp, err_kp_pa, pck, cam or None) of hmmr_eval_kps: kps_gt [n,k,3], kps_pred [n,k,2] read in
    place when they are device views.  img_size > 0 maps the prediction from [-1, 1] to pixels in the kernel."""
    lib = L.load()
    gt, ld_gt = _rows(kps_gt, device, (3,))
    pred, ld_pred = _rows(kps_pred, device, (2,))
    assert gt.dim() == 3 and pred.dim() == 3 and gt.shape[:2] == pred.shape[:2], (tuple(gt.shape), tuple(pred.shape))
    n, k = pred.shape[0], pred.shape[1]
    e, epa, pck = (torch.empty(n, device=device) for _ in range(3))
    cam = torch.empty((n, 3), device=device) if want_cam else None
    if n:
        L.check(lib.hmmr_eval_kps(gt.data_ptr(), ld_gt, pred.data_ptr(), ld_pred, n, k, float(alpha), int(min_visible),
                                  float(img_size), e.data_ptr(), epa.data_ptr(), pck.data_ptr(), L.ptr(cam), _stream(device)),
                "hmmr_eval_kps")
    return e, epa, pck, cam


def _float_list(t):
    return list(t.cpu().numpy().astype(np.float64))


def compute_error_kp(kps_gt, kps_pred, alpha=0.05, min_visible=6, device="cuda:0"):
    """Keypoint error in pixels, the error after the optimal-camera alignment and the share of correct keypoints, per frame
    (eval_util.py:97-137): kps_gt (Nxkx3), kps_pred (Nxkx2) -> errors_kp, errors_kp_pa, errors_kp_pck, lists with NaN for the
    frames that show fewer than min_visible keypoints."""
    assert len(kps_gt) == len(kps_pred)
    e, epa, pck, _ = kp_metrics_device(kps_gt, kps_pred, alpha, min_visible, device=device)
    return _float_list(e), _float_list(epa), _float_list(pck)


def compute_opt_cam_with_vis(got, want, vis, device="cuda:0"):
    """The optimal camera [scale, tx, ty] that maps the 2D keypoints `got` (kx2) onto `want` (kx2) over the keypoints with
    vis set (eval_util.py:235-260) -> (scale * (got + trans), cam).  The camera is the kernel's (float32); the aligned points
    are formed from it on the host."""
    got_np = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want_t = want.detach().cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.asarray(want, np.float32))
    vis_t = torch.as_tensor(np.asarray(vis.detach().cpu() if isinstance(vis, torch.Tensor) else vis).astype(bool))
    gt = torch.cat([want_t.to(torch.float32).reshape(-1, 2), vis_t.to(torch.float32).reshape(-1, 1)], dim=1)[None]
    cam = kp_metrics_device(gt, torch.as_tensor(got_np, dtype=torch.float32)[None], 0.0, 0, want_cam=True, device=device)[3]
    cam = cam[0].cpu().numpy().astype(np.float64)
    return cam[0] * (got_np.astype(np.float64) + cam[1:]), cam


# ---- rotations (hmmr_rotmat_to_axis_angle / hmmr_axis_angle_to_rotmat) -----------------------------------------------------------
def rotmat_to_aa_device(rot, device="cuda:0"):
    """rot [n, per, 3, 3] (read in place when it is a device view, e.g. preds['poses'] inside the packed record) ->
    axis-angle vectors [n, per * 3] on the device."""
    lib = L.load()
    r, ld = _rows(rot, device, (3, 3))
    assert r.dim() == 4, tuple(r.shape)
    n, per = r.shape[0], r.shape[1]
    out = torch.empty((n, per * 3), device=device)
    if n and per:
        L.check(lib.hmmr_rotmat_to_axis_angle(r.data_ptr(), ld, n, per, out.data_ptr(), per * 3, _stream(device)),
                "hmmr_rotmat_to_axis_angle")
    return out


def aa_to_rotmat_device(aa, device="cuda:0"):
    """aa [n, per * 3] -> rotation matrices [n, per, 3, 3] on the device (the Rodrigues of the SMPL pose kernel)."""
    lib = L.load()
    a = _dev(aa, device)
    a = a.reshape(a.shape[0], -1)
    n, per = a.shape[0], a.shape[1] // 3
    assert a.shape[1] == per * 3
    out = torch.empty((n, per, 3, 3), device=device)
    if n and per:
        L.check(lib.hmmr_axis_angle_to_rotmat(a.data_ptr(), per * 3, n, per, out.data_ptr(), per * 9, _stream(device)),
                "hmmr_axis_angle_to_rotmat")
    return out


def axis_angle_to_rot_mat(poses_aa, device="cuda:0"):
    """poses_aa (72) -> rot_matrices (24x3x3) (eval_util.py:318-329)."""
    a = poses_aa if isinstance(poses_aa, torch.Tensor) else np.asarray(poses_aa, np.float32)
    return aa_to_rotmat_device(a.reshape(1, -1), device)[0].cpu().numpy()


def rot_mat_to_axis_angle(rot_matrices, device="cuda:0"):
    """rot_matrices (24x3x3) -> poses_aa (72) (eval_util.py:332-343): |w| <= pi per joint and Rodrigues(w) = R."""
    r = rot_matrices if isinstance(rot_matrices, torch.Tensor) else np.asarray(rot_matrices, np.float32)
    return rotmat_to_aa_device(r.reshape((1, -1, 3, 3)), device)[0].cpu().numpy()


# ---- single-frame host utilities (NumPy in the reference too; the batched device forms are compute_error_3d's kernel) --------------
def align_by_pelvis(joints, get_pelvis=False):
    """Joints (14x3, LSP order) with the midpoint of the hips at the origin (eval_util.py:158-174)."""
    joints = np.asarray(joints)
    pelvis = (joints[LEFT_HIP, :] + joints[RIGHT_HIP, :]) / 2.
    aligned = joints - pelvis[None]
    return (aligned, pelvis) if get_pelvis else aligned


def compute_similarity_transform(S1, S2):
    """S1 after the similarity transform (scale, rotation, translation) that brings it closest to S2: the orthogonal Procrustes
    problem (eval_util.py:177-232).  Points as columns (3xN or 2xN) or as rows."""
    S1, S2 = np.asarray(S1), np.asarray(S2)
    rows = S1.shape[0] not in (2, 3)
    if rows:
        S1, S2 = S1.T, S2.T
    assert S2.shape[1] == S1.shape[1]
    mu1, mu2 = S1.mean(axis=1, keepdims=True), S2.mean(axis=1, keepdims=True)
    X1, X2 = S1 - mu1, S2 - mu2
    K = X1.dot(X2.T)
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(U.shape[0])
    Z[-1, -1] *= np.sign(np.linalg.det(U.dot(Vh)))           # a proper rotation
    R = Vh.T.dot(Z.dot(U.T))
    scale = np.trace(R.dot(K)) / np.sum(X1 ** 2)
    out = scale * R.dot(S1) + (mu2 - scale * R.dot(mu1))
    return out.T if rows else out


# ---- accumulation of error dictionaries (eval_util.py:263-313) ------------------------------------------------------------------------
def concat_dict_entries(dictionary):
    """Every value (a list of lists) becomes one array."""
    for k in dictionary:
        dictionary[k] = np.concatenate(dictionary[k])


def extend_dict_entries(accumulator, appender):
    """Extends the lists in accumulator with the values of appender (a scalar is appended)."""
    for k, v in appender.items():
        dst = accumulator.setdefault(k, [])
        if hasattr(v, "__iter__"):
            dst.extend(v)
        else:
            dst.append(v)


def mean_of_dict_values(dictionary):
    """Every value (a list of lists) becomes the mean of the means of its lists, NaN entries left out, rounded to 5 places."""
    for k, v in dictionary.items():
        dictionary[k] = float(round(np.nanmean([np.nanmean(values) for values in v]), 5))


def update_dict_entries(accumulator, appender):
    """Appends each value of appender to the list under the same key in accumulator."""
    for k, v in appender.items():
        accumulator.setdefault(k, []).append(v)
