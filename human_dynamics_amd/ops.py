"""Mirror of the loss functions of src/ops.py for device tensors: the reference's names and argument meaning, every loss one launch
set of the loss stage (HmmrEngine.seq_losses -> hmmr_seq_losses, csrc/losses.hip) with ONE flag set, under torch.autograd: the
forward computes the loss and its unit-weight cotangents together, the backward scales them by the upstream gradient, so
`loss.backward()` reaches tf_smpl.autograd.smpl_apply (hmmr_smpl_bwd) and whatever produced its inputs.

The reference's functions take no engine; here the last keyword of each is `engine` (as tf_smpl.batch_lbs.batch_rodrigues has it),
and `set_engine` names the one used when it is left out.  Ground truth carries no gradient.  TensorFlow's reduction rule
(tf.losses.*, SUM_BY_NONZERO_WEIGHTS with its safe division) is restated in include/hmmr_hip.h, "Trainer losses".

compute_loss_e_fake / compute_loss_d_fake / compute_loss_d_real take the discriminator's output (discriminators.PoseDiscriminator,
disc_autograd.disc_pose_apply) and are plain tensor arithmetic on 24 values per row; the closed loop of a step, losses and both
gradients in one call, is HmmrEngine.pose_prior (hmmr_pose_prior).

mean_squared_error is tf.losses.mean_squared_error as the trainer uses it for e_hallucinate (HmmrEngine.strip_mse -> hmmr_strip_mse).

Not here: call_hmr_ief / hmr_ief (the IEF lives in HmmrEngine.ief)."""
from __future__ import annotations

import torch

from . import _lib as L

_ENGINE = [None]


def set_engine(engine):
    """the engine the functions below use when called without `engine=`"""
    _ENGINE[0] = engine


def _eng(engine):
    engine = engine if engine is not None else _ENGINE[0]
    if engine is None:
        raise L.HmmrError("human_dynamics_amd.ops: no engine (pass engine=, or call ops.set_engine first): the losses run on the device")
    return engine


_PRED = ("kps_pred", "joints_pred", "rs_pred", "beta_pred")
_GRAD = ("d_kps", "d_joints", "d_rs", "d_beta")


class _SeqLoss(torch.autograd.Function):
    """one call of the loss stage with unit weights: (engine, B, T, K, flags, delta_t, gt, slots, want_cam, *the four predictions or
    None) -> (losses[slots], best_cam or an empty tensor).  The cotangent of loss slot s reaches only the predictions `_REACH[s]`
    names, so two slots of one call (e_smpl_pose, e_smpl_shape) are scaled separately."""
    _REACH = {0: ("d_kps",), 1: ("d_joints",), 2: ("d_rs",), 3: ("d_beta",), 4: ("d_beta",), 5: ("d_beta",)}

    @staticmethod
    def forward(ctx, engine, B, T, K, flags, delta_t, gt, slots, want_cam, *preds):
        kw = {k: (p.detach() if p is not None else None) for k, p in zip(_PRED, preds)}
        need = [i for i, p in enumerate(preds) if p is not None and ctx.needs_input_grad[9 + i]]
        out = engine.seq_losses(B, T, flags, gt, weights=(1.0,) * 5, delta_t=delta_t, want_grads=[_GRAD[i] for i in need],
                                want_best_cam=want_cam, K=K, **kw)
        ctx.slots, ctx.need, ctx.shapes = tuple(slots), need, [None if p is None else p.shape for p in preds]
        ctx.save_for_backward(*[out[_GRAD[i]] for i in need])
        cam = out["best_cam"] if want_cam else torch.empty(0, device=engine.device)
        ctx.mark_non_differentiable(cam)
        return out["losses"][list(slots)], cam

    @staticmethod
    def backward(ctx, g, _g_cam):
        grads = [None] * 4
        for i, saved in zip(ctx.need, ctx.saved_tensors):
            scale = sum(g[j] for j, s in enumerate(ctx.slots) if _GRAD[i] in _SeqLoss._REACH[s])
            grads[i] = (saved * scale).reshape(ctx.shapes[i])
        return (None,) * 9 + tuple(grads)


def _f32(engine, x):
    return x.to(engine.device, torch.float32) if isinstance(x, torch.Tensor) else engine.to_device(x)


def compute_loss_e_kp(kp_gt, kp_pred, name=None, engine=None):
    """L_KP = sum_i v_i ||x_i - x^_i||_1 / (2 #{v != 0}) (src/ops.py: compute_loss_e_kp).  kp_gt [N,K,3] or [B,T,K,3], kp_pred the
    same with a last dimension of 2."""
    engine = _eng(engine)
    kp_gt, kp_pred = _f32(engine, kp_gt), _f32(engine, kp_pred)
    K = kp_gt.shape[-2]
    kp_pred = kp_pred.reshape(-1, K, 2)
    return _SeqLoss.apply(engine, kp_pred.shape[0], 1, K, L.LOSS_KP, 0, {"kps": kp_gt.detach()}, (0,), False, kp_pred, None, None, None)[0][0]


def compute_loss_e_kp_optcam(kp_gt, kp_pred, name=None, engine=None):
    """The keypoint loss under the optimal scale and translation of every frame, which carry no gradient (src/ops.py:
    compute_loss_e_kp_optcam; projection.batch_orth_proj_optcam, procrustes2d_vis).  kp_gt [B,T,K,3], kp_pred [B,T,K,2] ->
    (loss, best_cam [B,T,3]).  A frame without a visible keypoint makes the loss non-finite, as in the reference."""
    engine = _eng(engine)
    kp_gt, kp_pred = _f32(engine, kp_gt), _f32(engine, kp_pred)
    B, T, K = kp_gt.shape[0], kp_gt.shape[1], kp_gt.shape[2]
    loss, cam = _SeqLoss.apply(engine, B, T, K, L.LOSS_KP_OPTCAM, 0, {"kps": kp_gt.detach()}, (0,), True, kp_pred.reshape(B * T, K, 2),
                               None, None, None)
    return loss[0], cam.reshape(B, T, 3)


def align_by_pelvis(joints):
    """joints [N,14,3] in LSP order minus the midpoint of the hips 3 and 2 (src/ops.py: align_by_pelvis).  Plain tensor arithmetic
    on the tensor's device; the 3-D loss below aligns inside its kernel."""
    if joints.dim() != 3:
        joints = joints.reshape(-1, 14, 3)
    pelvis = (joints[:, 3, :] + joints[:, 2, :]) / 2.
    return joints - pelvis.unsqueeze(1)


def _has(engine, has, rows):
    return _f32(engine, has).detach().reshape(rows)


def compute_loss_e_3d(poses_gt, poses_pred, shapes_gt, shapes_pred, joints_gt, joints_pred, batch_size, has_gt3d_smpl, has_gt3d_joints,
                      engine=None):
    """(loss_e_pose, loss_e_shape, loss_e_joints) of src/ops.py: compute_loss_e_3d: rotations [.., 24,3,3], shapes [.., 10] and
    joints [B,T,14,3] of `batch_size` rows each, has_gt3d_* one weight per row.  The joints are aligned by the pelvis inside the
    kernel.  Two calls of the loss stage: SMPL (pose and shape) and JOINTS."""
    engine = _eng(engine)
    n = int(batch_size)
    rs_gt, rs = _f32(engine, poses_gt).reshape(n, 24, 3, 3), _f32(engine, poses_pred).reshape(n, 24, 3, 3)
    sh_gt, sh = _f32(engine, shapes_gt).reshape(n, 10), _f32(engine, shapes_pred).reshape(n, 10)
    j_gt, j = _f32(engine, joints_gt), _f32(engine, joints_pred)
    assert j_gt.dim() == 4
    j_gt, j = j_gt.reshape(n, 14, 3), j.reshape(n, 14, 3)
    # every row is a sequence of one frame: the row weights of the reference are per row
    gt = {"rs": rs_gt.detach(), "shapes": sh_gt.detach(), "has_gt3d_smpl": _has(engine, has_gt3d_smpl, n)}
    smpl = _SeqLoss.apply(engine, n, 1, 14, L.LOSS_SMPL, 0, gt, (2, 3), False, None, None, rs, sh)[0]
    gt = {"joints": j_gt.detach(), "has_gt3d_joints": _has(engine, has_gt3d_joints, n)}
    joints = _SeqLoss.apply(engine, n, 1, 14, L.LOSS_JOINTS, 0, gt, (1,), False, None, j, None, None)[0]
    return smpl[0], smpl[1], joints[0]


def compute_loss_mse(params_gt, params_pred, has_gt3d, engine=None):
    """0.5 x tf.losses.mean_squared_error with one weight per row (src/ops.py: compute_loss_mse) for rows of up to 216 values -- the
    reference calls it with 216 (rotations), 10 (shape) and 42 (joints it has aligned itself).  Nothing is aligned here.  The rows run
    as the 216-wide rotation term of the loss stage, padded with zeros on both sides (a zero difference adds nothing to the sum); for a
    narrower row the stage's normaliser 216 is turned into the row's width by one fp32 factor 216 / D on the loss."""
    engine = _eng(engine)
    gt_, pr = _f32(engine, params_gt), _f32(engine, params_pred)
    n = gt_.shape[0]
    gt_, pr = gt_.reshape(n, -1), pr.reshape(n, -1)
    D = gt_.shape[1]
    if not 1 <= D <= 216 or pr.shape[1] != D:
        raise ValueError("compute_loss_mse: rows of %d and %d values; the loss stage takes equal rows of 1 .. 216" % (D, pr.shape[1]))
    pad = lambda x: torch.nn.functional.pad(x, (0, 216 - D)).reshape(n, 24, 3, 3)
    zeros = torch.zeros((n, 10), dtype=torch.float32, device=engine.device)       # (the shape half of the SMPL term: nothing to compare)
    gt = {"rs": pad(gt_.detach()), "shapes": zeros, "has_gt3d_smpl": _has(engine, has_gt3d, n)}
    loss = _SeqLoss.apply(engine, n, 1, 14, L.LOSS_SMPL, 0, gt, (2,), False, None, None, pad(pr), zeros)[0][0]
    return loss if D == 216 else loss * (216.0 / D)


def compute_loss_e_smooth(joints_prev, joints_curr, engine=None):
    """0.5 x the mean squared difference of two tensors of one shape (src/ops.py: compute_loss_e_smooth, which the trainer applies to
    betas[:, :-1] and betas[:, 1:]).  A mean over all elements does not depend on their shape: the elements run in rows of ten, every
    (prev, curr) row pair as a sequence of two frames of the CONST term; a count that is no multiple of ten is padded with zeros and
    the loss scaled by padded / actual count in fp32."""
    engine = _eng(engine)
    a, b = _f32(engine, joints_prev), _f32(engine, joints_curr)
    if a.shape != b.shape or a.numel() == 0:
        raise ValueError("compute_loss_e_smooth: two non-empty tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    count = a.numel()
    n = (count + 9) // 10
    rows = lambda x: torch.nn.functional.pad(x.reshape(-1), (0, 10 * n - count)).reshape(n, 10)
    pairs = torch.stack((rows(a), rows(b)), dim=1)                                # [n, 2, 10]
    loss = _SeqLoss.apply(engine, n, 2, 14, L.LOSS_CONST, 0, {}, (4,), False, None, None, None, pairs.reshape(2 * n, 10))[0][0]
    return loss if 10 * n == count else loss * (10.0 * n / count)


def compute_loss_shape(shapes, engine=None):
    """mean(shapes^2) (src/ops.py: compute_loss_shape) of a [..., 10] tensor"""
    engine = _eng(engine)
    s = _f32(engine, shapes).reshape(-1, 10)
    return _SeqLoss.apply(engine, s.shape[0], 1, 14, L.LOSS_SHAPE_PRIOR, 0, {}, (5,), False, None, None, None, s)[0][0]


class _StripMse(torch.autograd.Function):
    """(engine, labels, predictions) -> the mean squared difference; the forward call already holds both unit-weight cotangents"""

    @staticmethod
    def forward(ctx, engine, a, b):
        need = ctx.needs_input_grad
        loss, d_a, d_b = engine.strip_mse(a.detach(), b.detach(), 1.0, want_d_a=bool(need[1]), want_d_b=bool(need[2]))
        ctx.has = (d_a is not None, d_b is not None)
        ctx.save_for_backward(*[d for d in (d_a, d_b) if d is not None])
        return loss

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        d_a = saved.pop(0) * g if ctx.has[0] else None
        d_b = saved.pop(0) * g if ctx.has[1] else None
        return None, d_a, d_b


def mean_squared_error(labels, predictions, engine=None):
    """tf.losses.mean_squared_error(labels, predictions) with the default weight: mean((labels - predictions)^2) over all elements of
    two tensors of one shape [..., cols] (the trainer's e_hallucinate on two [B, T, 2048] movie strips; hmmr_strip_mse).  Unlike the
    losses above it is differentiable in BOTH arguments: the reference puts no stop-gradient on the movie strip."""
    engine = _eng(engine)
    a, b = _f32(engine, labels), _f32(engine, predictions)
    if a.shape != b.shape or a.numel() == 0:
        raise ValueError("mean_squared_error: two non-empty tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    return _StripMse.apply(engine, a, b)


def compute_loss_e_fake(out_fake):
    """mean over the rows of sum_24 (out - 1)^2 (src/ops.py: compute_loss_e_fake); out_fake [N,24]"""
    return ((out_fake - 1) ** 2).sum(dim=1).mean()


def compute_loss_d_fake(out_fake):
    """mean over the rows of sum_24 out^2 (src/ops.py: compute_loss_d_fake)"""
    return (out_fake ** 2).sum(dim=1).mean()


def compute_loss_d_real(out_real):
    """mean over the rows of sum_24 (out - 1)^2 (src/ops.py: compute_loss_d_real)"""
    return ((out_real - 1) ** 2).sum(dim=1).mean()


def compute_deltas_batched(poses_prev, poses_curr):
    """R_prev R_curr^T of [B,T,24,3,3] rotations (src/ops.py: compute_deltas_batched); plain tensor arithmetic"""
    assert poses_prev.shape == poses_curr.shape
    assert len(poses_prev.shape) == 5
    assert tuple(poses_prev.shape[2:]) == (24, 3, 3)
    return torch.matmul(poses_prev, poses_curr.transpose(-1, -2))
