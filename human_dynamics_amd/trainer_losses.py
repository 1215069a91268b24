"""The encoder losses of the sequence trainer on precomputed phis (src/trainer_sequence_fc.py: compute_losses_batched :791-846,
compute_losses_deltas :848-953, the shape prior e_shape of compute_losses_prior :1018) for device tensors, each container ONE call
of the closed loop omega -> losses, d_omega (HmmrEngine.omega_loss_grad -> hmmr_omega_loss_grad: hmmr_smpl_fwd, hmmr_seq_losses,
hmmr_smpl_bwd).  The results are the reference's dictionary keys -- e_kp, e_joints, e_smpl, e_const, e_shape, with the
future / past / present suffixes -- as device scalars that are differentiable in the raw omegas.

compute_losses_prior (:989-1020) is the pose discriminator's closed loop (HmmrEngine.pose_prior -> hmmr_pose_prior,
csrc/disc_pose.hip): e_pose, d_pose and e_shape.

e_hallucinate is ops.mean_squared_error; the optimiser is optim.TFAdam and the step that composes all of this
trainer_sequence_fc.HMRSequenceTrainer.  Out of scope (README): the tfrecord and mocap loaders."""
from __future__ import annotations

import torch

from . import _lib as L

LOSS_KEYS = ("e_kp", "e_joints", "e_smpl", "e_const", "e_shape")
DEFAULT_WEIGHTS = {k: 1.0 for k in LOSS_KEYS}


def _weight_list(loss_weights, suffix=""):
    w = dict(DEFAULT_WEIGHTS)
    for k in LOSS_KEYS:
        for key in (k, k + suffix):
            if loss_weights and key in loss_weights:
                w[k] = float(loss_weights[key])
    return [w[k] for k in LOSS_KEYS]


class _OmegaLoss(torch.autograd.Function):
    """omega [N,85] in, the loss vector [8] out (order _lib.LOSS_NAMES; [6] = total = sum w_i L_i).  The forward call already holds
    d total / d omega.  A backward that asks for the total alone scales it; one that asks for single losses (which needs the upstream
    vector on the host: one synchronisation) runs the loop again with the weights that upstream vector amounts to."""

    @staticmethod
    def forward(ctx, engine, B, T, flags, gt, weights, delta_t, use_optcam, want_cam, omega):
        om = omega.detach()
        losses, d_omega, status, cam = engine.omega_loss_grad(om, B, T, flags, gt, weights=weights, delta_t=delta_t, use_optcam=use_optcam,
                                                              want_best_cam=want_cam)
        ctx.args = (engine, B, T, flags, gt, list(weights), delta_t, use_optcam)
        ctx.save_for_backward(om, d_omega)
        cam = cam if cam is not None else torch.empty(0, device=engine.device)
        ctx.mark_non_differentiable(status, cam)
        return losses, status, cam

    @staticmethod
    def backward(ctx, g, _gs, _gc):
        om, d_omega = ctx.saved_tensors
        engine, B, T, flags, gt, w, delta_t, use_optcam = ctx.args
        gl = [float(v) for v in g.tolist()]
        if not any(gl[:6]):
            return (None,) * 9 + ((d_omega * g[6]).reshape(om.shape),)
        if gl[2] != gl[3]:
            raise L.HmmrError("e_smpl_pose and e_smpl_shape share one weight in hmmr_seq_losses: their upstream gradients must be equal "
                              "(got %g and %g); take e_smpl = pose + shape, or ops.compute_loss_e_3d" % (gl[2], gl[3]))
        eff = [gl[0] + gl[6] * w[0], gl[1] + gl[6] * w[1], gl[2] + gl[6] * w[2], gl[4] + gl[6] * w[3], gl[5] + gl[6] * w[4]]
        d2 = engine.omega_loss_grad(om, B, T, flags, gt, weights=eff, delta_t=delta_t, use_optcam=use_optcam)[1]
        return (None,) * 9 + (d2.reshape(om.shape),)


def omega_losses(engine, omega, B, T, flags, gt, weights, delta_t=0, use_optcam=False, want_best_cam=False):
    """(losses [8], status [1], best_cam [N,3] or None) of one container; losses is differentiable in omega"""
    om = omega if isinstance(omega, torch.Tensor) else engine.to_device(omega)
    om = om.to(engine.device, torch.float32).reshape(-1, 85)
    losses, status, cam = _OmegaLoss.apply(engine, int(B), int(T), int(flags), gt, list(weights), int(delta_t), bool(use_optcam),
                                           bool(want_best_cam), om)
    return losses, status, (cam if want_best_cam else None)


def _gt_dict(gt, has_gt3d_smpl, has_gt3d_joints, use_3d_label):
    d = {"kps": gt.get_kps()}
    if use_3d_label:
        d.update(joints=gt.get_joints(), rs=gt.get_poses_rot(), shapes=gt.shapes, has_gt3d_smpl=has_gt3d_smpl, has_gt3d_joints=has_gt3d_joints)
    return d


def compute_losses_batched(engine, omegas_raw, gt, has_gt3d_smpl=None, has_gt3d_joints=None, use_3d_label=True, loss_weights=None,
                           with_shape_prior=True, use_optcam=False):
    """compute_losses_batched of the trainer for the present container: omegas_raw [B,T,85] (the IEF's output), gt an
    omega.OmegasGt, has_gt3d_* [B].  -> {e_kp, e_joints, e_smpl, e_const, e_shape, total, status; e_smpl_pose, e_smpl_shape as values}: device
    scalars of ONE call; `total` = sum of loss_weights[key] x loss (weights default to 1) is the one to call .backward() on (no
    synchronisation; a single entry's .backward() costs one and a second run).  e_shape is the shape prior of compute_losses_prior
    on this container's shapes (with_shape_prior).  use_optcam: the forward runs with cams [1, 0, 0]."""
    B, T = omegas_raw.shape[0], omegas_raw.shape[1]
    flags = L.LOSS_KP | L.LOSS_CONST | (L.LOSS_SHAPE_PRIOR if with_shape_prior else 0)
    if use_3d_label:
        flags |= L.LOSS_JOINTS | L.LOSS_SMPL
    losses, status, _ = omega_losses(engine, omegas_raw, B, T, flags, _gt_dict(gt, has_gt3d_smpl, has_gt3d_joints, use_3d_label),
                                     _weight_list(loss_weights), 0, use_optcam)
    out = {"e_kp": losses[0], "e_const": losses[4], "total": losses[6], "status": status}
    if use_3d_label:
        # (the two halves share one weight in the loss stage: they are reported as values, e_smpl is the differentiable entry)
        out.update(e_joints=losses[1], e_smpl=losses[2] + losses[3], e_smpl_pose=losses[2].detach(), e_smpl_shape=losses[3].detach())
    if with_shape_prior:
        out["e_shape"] = losses[5]
    return out


def compute_losses_deltas(engine, omegas_dict, gt, suffix_future="_dt_future", suffix_past="_dt_past", suffix_present="_dt",
                          has_gt3d_smpl=None, has_gt3d_joints=None, use_3d_label=True, loss_weights=None, use_optcam=True):
    """compute_losses_deltas of the trainer: omegas_dict {delta_t: raw omegas [B,T,85]}, one closed-loop call per container.
    delta_t = 0 takes the plain keypoint loss, every other one the optimal camera on its frame slice (pred [0, T - dt) against gt
    [dt, T) for the future, pred [|dt|, T) against gt [0, T - |dt|) for the past).  -> {'e_kp' + suffix, 'e_joints' + suffix,
    'e_smpl' + suffix for the three suffixes that occur (summed over their containers, as the reference's `+=`), 'total' (the
    weighted sum over all containers; loss_weights may carry suffixed keys), 'best_cam': {delta_t: [B,T,3], NaN outside the slice},
    'status': {delta_t: word}}."""
    out, cams, stat, total = {}, {}, {}, None
    gtd = _gt_dict(gt, has_gt3d_smpl, has_gt3d_joints, use_3d_label)
    for delta_t, raw in omegas_dict.items():
        delta_t = int(delta_t)
        B, T = raw.shape[0], raw.shape[1]
        suffix = suffix_present if delta_t == 0 else (suffix_future if delta_t > 0 else suffix_past)
        flags = (L.LOSS_KP if delta_t == 0 else L.LOSS_KP_OPTCAM) | ((L.LOSS_JOINTS | L.LOSS_SMPL) if use_3d_label else 0)
        losses, status, cam = omega_losses(engine, raw, B, T, flags, gtd, _weight_list(loss_weights, suffix), delta_t,
                                           use_optcam and delta_t != 0, want_best_cam=delta_t != 0)
        terms = {"e_kp": losses[0]}
        if use_3d_label:
            terms.update(e_joints=losses[1], e_smpl=losses[2] + losses[3])
        for k, v in terms.items():
            out[k + suffix] = v if k + suffix not in out else out[k + suffix] + v
        total = losses[6] if total is None else total + losses[6]
        stat[delta_t] = status
        if cam is not None:
            cams[delta_t] = cam.reshape(B, T, 3)
    out.update(total=total, best_cam=cams, status=stat)
    return out


class _PosePrior(torch.autograd.Function):
    """(engine, real rows, fake rows, the bank's tensors...) -> (e_pose, d_pose), two outputs.  The forward call already holds both
    gradients of unit weight: d e_pose / d fake and d d_pose / d bank.  e_pose does not reach the bank and d_pose does not reach the
    poses: the reference's e_opt and d_opt differentiate with respect to the encoder's and the discriminator's variables only -- an
    output whose cotangent is absent passes nothing on (not even zeros)."""

    @staticmethod
    def forward(ctx, engine, real, fake, *bank_tensors):
        from .disc_bank import NAMES
        need = ctx.needs_input_grad
        want_w = [n for i, n in enumerate(NAMES) if need[3 + i]]
        losses, d_rs, g = engine.pose_prior(real, fake.detach(), 1.0, 1.0, want_d_rs=bool(need[2]), want_weights=want_w)
        ctx.shape, ctx.names, ctx.has_rs = fake.shape, want_w, d_rs is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*([d_rs] if d_rs is not None else []), *[g[n] for n in want_w])
        return losses[0], losses[1] + losses[2]

    @staticmethod
    def backward(ctx, g_e, g_d):
        from .disc_bank import NAMES
        saved = list(ctx.saved_tensors)
        d_rs = saved.pop(0) if ctx.has_rs else None
        d_fake = (d_rs * g_e).reshape(ctx.shape) if (d_rs is not None and g_e is not None) else None
        by_name = dict(zip(ctx.names, saved)) if g_d is not None else {}
        return (None, None, d_fake) + tuple((by_name[n] * g_d) if n in by_name else None for n in NAMES)


def compute_losses_prior(engine, poses_real, pred_poses_all, pred_shapes_all, bank_tensors=None):
    """compute_losses_prior of the trainer (src/trainer_sequence_fc.py:989-1020): poses_real [n_real, 216] (or [n_real,24,3,3]; or
    [n_real, 207], the global rotation already dropped) mocap rotations, pred_poses_all a list of predicted Rs [.., 24,3,3] (or one tensor), pred_shapes_all the same of shapes [.., 10].
    -> {e_pose, d_pose, e_shape}: device scalars of ONE call of the closed loop plus the shape prior.  e_pose is differentiable in
    the predicted Rs (through tf_smpl.autograd.smpl_apply, .backward() reaches omega), d_pose in the bank's tensors that require a
    gradient (.grad lands on engine.disc_pose_bank().tensors()); e_pose does not reach the bank and d_pose does not reach the poses,
    as the reference's two var_lists have it.  The counts of real and fake rows need not be equal: each mean runs over its own rows."""
    from . import ops
    def cat(x, w):
        """a lone tensor (or a list of one) passes through as a view: the C call reads the predicted Rs where smpl_apply left them"""
        x = list(x) if isinstance(x, (list, tuple)) else [x]
        return x[0].reshape(-1, w) if len(x) == 1 else torch.cat([t.reshape(-1, w) for t in x], 0)
    fake = cat(pred_poses_all, 216)
    real = poses_real if isinstance(poses_real, torch.Tensor) else engine.to_device(poses_real)
    real = real.reshape(real.shape[0], -1)                  # (rows of 216 values, or of the 207 behind the global rotation)
    tensors = engine.disc_pose_bank().tensors() if bank_tensors is None else list(bank_tensors)
    e_pose, d_pose = _PosePrior.apply(engine, real, fake, *tensors)
    return {"e_pose": e_pose, "d_pose": d_pose, "e_shape": ops.compute_loss_shape(cat(pred_shapes_all, 10), engine=engine)}
