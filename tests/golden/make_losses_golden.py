"""Golden vectors for the trainer's losses, produced by EXECUTING the reference's own source (the reference tree is not part of this
repository, so the outputs are committed as a fixture):

  reference_losses.npz   (results only; the fp32 inputs are tests/loss_cases.py: golden_inputs(), seeded)  src/ops.py (compute_loss_e_kp, compute_loss_e_kp_optcam, compute_loss_e_3d, compute_loss_mse,
                         compute_loss_e_smooth, compute_loss_shape, align_by_pelvis, compute_deltas_batched), src/tf_smpl/projection.py
                         (batch_orth_proj_optcam, procrustes2d_vis, batch_orth_proj_idrot) and src/tf_smpl/batch_lbs.py
                         (batch_rodrigues), unmodified, on the NumPy TensorFlow stand-in in float64 (oracle.tf_shim.install()).
                         The frame slices of compute_losses_deltas (src/trainer_sequence_fc.py:867-884: s_gt, e_gt, s_pr, e_pr) are
                         restated in `slices` below, because the trainer class itself needs a TF session, data loaders and a
                         config; the functions it calls on those slices are the reference's.

The elementary ops the stand-in lacks (reduce_sum, square, trace, matrix_inverse, clip_by_value, abs, the `**` operator) are added to
the installed module from this script with their documented TF semantics.  ONE piece is NOT the reference's code and NOT
TensorFlow's binary: `tf.losses.absolute_difference` and `tf.losses.mean_squared_error` are restated here from the published
TF 1.x tensorflow/python/ops/losses/losses_impl.py -- the weights broadcast against the losses, `_num_present` (the count of the
broadcast weight's non-zero elements), `_safe_div` (0 where the denominator is not positive) and the default reduction
SUM_BY_NONZERO_WEIGHTS.  Their agreement with a TensorFlow binary is UNMEASURED: no TensorFlow 1.x was at hand.

    python tests/golden/make_losses_golden.py <reference tree>        (or HMMR_REFERENCE_TREE)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HMMR_REFERENCE_TREE", "")
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import loss_cases as LC  # noqa: E402  (the fixture's seeded inputs live with the test that reads it)

B, T, K, DELTAS = LC.GOLDEN_B, LC.GOLDEN_T, LC.GOLDEN_K, LC.GOLDEN_DELTAS
PER_DELTA = ("e_kp", "e_kp_optcam", "e_joints", "e_smpl_pose", "e_smpl_shape")       # the columns of `per_delta`


def extend_shim(tf):
    T_, _a = tf.Tensor, tf._a

    def _axis(axis):
        return None if axis is None else tuple(int(a) for a in np.atleast_1d(_a(axis)))

    def reduce_sum(x, axis=None, keepdims=None, name=None, keep_dims=None):
        return T_(np.sum(_a(x), axis=_axis(axis), keepdims=bool(keepdims or keep_dims)))

    # ---- tensorflow/python/ops/losses/losses_impl.py (TF 1.x), restated
    def _safe_div(numerator, denominator):
        den = np.asarray(denominator)
        return np.where(den > 0, np.divide(numerator, np.where(den == 0, np.ones_like(den), den)), np.zeros_like(numerator))

    def _num_present(losses, weights):
        present = np.where(weights == 0.0, np.zeros_like(weights), np.ones_like(weights))
        return np.sum(np.broadcast_to(present, np.broadcast(present, losses).shape))

    def compute_weighted_loss(losses, weights=1.0):                 # reduction = Reduction.SUM_BY_NONZERO_WEIGHTS, the default
        losses = np.asarray(_a(losses), tf.DTYPE)
        weights = np.asarray(_a(weights), tf.DTYPE)
        assert weights.ndim == 0 or weights.ndim == losses.ndim, "weights must be a scalar or of the losses' rank"
        weighted = losses * weights
        return T_(_safe_div(np.sum(weighted), _num_present(losses, weights)))

    def absolute_difference(labels, predictions, weights=1.0, scope=None):
        return compute_weighted_loss(np.abs(np.subtract(_a(predictions), _a(labels))), weights)

    def mean_squared_error(labels, predictions, weights=1.0, scope=None):
        d = np.subtract(_a(predictions), _a(labels))
        return compute_weighted_loss(d * d, weights)

    ops = dict(
        reduce_sum=reduce_sum,
        square=lambda x, name=None: T_(np.square(_a(x))),
        abs=lambda x, name=None: T_(np.abs(_a(x))),
        trace=lambda x, name=None: T_(np.trace(_a(x), axis1=-2, axis2=-1)),
        matrix_inverse=lambda x, adjoint=False, name=None: T_(np.linalg.inv(_a(x))),
        # tf.clip_by_value = minimum(maximum(x, lo), hi)
        clip_by_value=lambda x, lo, hi, name=None: T_(np.minimum(np.maximum(_a(x), np.asarray(lo, _a(x).dtype)), np.asarray(hi, _a(x).dtype))),
        losses=types.SimpleNamespace(absolute_difference=absolute_difference, mean_squared_error=mean_squared_error,
                                     compute_weighted_loss=compute_weighted_loss),
    )
    for k, v in ops.items():
        assert not hasattr(tf, k), k
        setattr(tf, k, v)
    # tf.TensorShape: equality with a shape, a list or a tuple, and a slice that is a TensorShape again (compute_deltas_batched)
    TS = tf.TensorShape
    saved = {k: TS.__dict__.get(k) for k in ("__eq__", "__getitem__", "__hash__")}
    item = TS.__getitem__
    TS.__eq__ = lambda self, o: self.as_list() == (o.as_list() if isinstance(o, TS) else [int(_a(d)) for d in o])
    TS.__hash__ = lambda self: hash(tuple(self.as_list()))
    TS.__getitem__ = lambda self, i: TS(self.as_list()[i]) if isinstance(i, slice) else item(self, i)
    had_pow = hasattr(T_, "__pow__")
    if not had_pow:
        T_.__pow__ = lambda self, o: T_(np.power(self.a, _a(o)))
    return list(ops), had_pow, saved


def slices(delta_t):
    """compute_losses_deltas :867-884 -> (s_gt, e_gt, s_pr, e_pr, seq_length)"""
    if delta_t == 0:
        return None, None, None, None, T
    if delta_t < 0:
        return None, delta_t, abs(delta_t), None, T - abs(delta_t)
    return delta_t, None, None, -delta_t, T - delta_t


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        raise SystemExit("usage: make_losses_golden.py <reference tree> (a checkout of akanazawa/human_dynamics)")
    from oracle import tf_shim
    added = tf_shim.install(np.float64)
    names, had_pow, saved = extend_shim(tf_shim)
    sys.path.insert(0, REF)
    try:
        from src import ops as R
        from src.tf_smpl.batch_lbs import batch_rodrigues
    finally:
        sys.path.remove(REF)
    Tn, _a = tf_shim.Tensor, tf_shim._a
    val = lambda x: np.asarray(_a(x), np.float64)
    inp = LC.golden_inputs()
    out = {}
    w = {k: Tn(v.astype(np.float64)) for k, v in inp.items()}
    sh = lambda x, *s: Tn(val(x).reshape(s))
    kps_gt, kps_pred = sh(w["kps_gt"], B, T, K, 3), sh(w["kps_pred"], B, T, K, 2)
    joints_gt, joints_pred = sh(w["joints_gt"], B, T, 14, 3), sh(w["joints_pred"], B, T, K, 3)
    rs_gt = sh(batch_rodrigues(sh(w["poses_gt"], -1, 3)), B, T, 24, 3, 3)
    rs_pred = sh(batch_rodrigues(sh(w["poses_pred"], -1, 3)), B, T, 24, 3, 3)
    shapes_gt = Tn(np.tile(val(w["shapes_gt"])[:, None], (1, T, 1)))             # OmegasGt.get_shapes
    betas = sh(w["beta_pred"], B, T, 10)

    for dt in DELTAS:
        s_gt, e_gt, s_pr, e_pr, L = slices(dt)
        p = "d%+d_" % dt
        out[p + "e_kp"] = val(R.compute_loss_e_kp(kps_gt[:, s_gt:e_gt], kps_pred[:, s_pr:e_pr]))
        loss, cam = R.compute_loss_e_kp_optcam(kp_gt=kps_gt[:, s_gt:e_gt], kp_pred=kps_pred[:, s_pr:e_pr])
        out[p + "e_kp_optcam"], out[p + "best_cam"] = val(loss), val(cam)
        rep = lambda h: Tn(np.repeat(val(h), L, 0))                               # tf_repeat(tensor, seq_length, 0)
        pose, shape, joints = R.compute_loss_e_3d(
            poses_gt=rs_gt[:, s_gt:e_gt], poses_pred=rs_pred[:, s_pr:e_pr], shapes_gt=shapes_gt[:, s_gt:e_gt], shapes_pred=betas[:, s_pr:e_pr],
            joints_gt=joints_gt[:, s_gt:e_gt], joints_pred=joints_pred[:, s_pr:e_pr, :14], batch_size=B * L,
            has_gt3d_smpl=rep(w["has_gt3d_smpl"]), has_gt3d_joints=rep(w["has_gt3d_joints"]))
        out[p + "e_smpl_pose"], out[p + "e_smpl_shape"], out[p + "e_joints"] = val(pose), val(shape), val(joints)
    out["e_const"] = val(R.compute_loss_e_smooth(betas[:, :-1], betas[:, 1:]))
    out["e_shape"] = val(R.compute_loss_shape(sh(betas, -1, 10)))
    out["aligned"] = val(R.align_by_pelvis(sh(joints_pred[:, :, :14], -1, 14, 3)))[:2]          # (rows 0, 1: the file stays small)
    out["deltas_rot"] = val(R.compute_deltas_batched(rs_gt[:, :-1], rs_gt[:, 1:]))[1, T - 2, ::8]       # (the last pair, joints 0, 8, 16)
    # all-zero weights: the safe division
    zero = Tn(np.zeros(B * T))
    pose0, shape0, joints0 = R.compute_loss_e_3d(rs_gt, rs_pred, shapes_gt, betas, joints_gt, joints_pred[:, :, :14], B * T, zero, zero)
    out["zero_weights"] = np.array([val(pose0), val(shape0), val(joints0)])
    novis = val(kps_gt).copy()
    novis[..., 2] = 0.0
    out["e_kp_novis"] = val(R.compute_loss_e_kp(Tn(novis), kps_pred))
    assert any(k.endswith("best_cam") for k in out)
    scales = np.concatenate([out[k][..., 0].ravel() for k in out if k.endswith("best_cam")])
    assert (scales == 0.7).any() and (scales == 10.0).any() and ((scales > 0.7) & (scales < 10.0)).any(), scales
    # few arrays, results only: the inputs come from loss_cases.golden_inputs() again where the fixture is read
    cams = np.full((len(DELTAS), B, T, 3), np.nan)
    for i, dt in enumerate(DELTAS):
        cams[i, :, :T - abs(dt)] = out["d%+d_best_cam" % dt]                     # the slice's frames first, NaN behind them
    packed = dict(
        deltas=np.array(DELTAS, np.int32),
        per_delta=np.array([[float(out["d%+d_%s" % (dt, k)]) for k in PER_DELTA] for dt in DELTAS]),
        best_cam=cams,
        scalars=np.array([float(out["e_const"]), float(out["e_shape"]), float(out["e_kp_novis"])] + [float(v) for v in out["zero_weights"]]),
        aligned=out["aligned"], deltas_rot=out["deltas_rot"],
        inputs_sum=np.array([np.abs(v.astype(np.float64)).sum() for _, v in sorted(inp.items())]))        # (the seeded inputs, checked where they are rebuilt)
    path = os.path.join(HERE, "reference_losses.npz")
    np.savez_compressed(path, **packed)
    print(path, os.path.getsize(path), sorted(packed))
    for k in names:
        delattr(tf_shim, k)
    if not had_pow:
        del tf_shim.Tensor.__pow__
    for k, v in saved.items():
        if v is None:
            delattr(tf_shim.TensorShape, k)
        else:
            setattr(tf_shim.TensorShape, k, v)
    tf_shim.uninstall(added)


if __name__ == "__main__":
    main()
