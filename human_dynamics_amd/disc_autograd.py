"""The pose discriminator under torch.autograd: the forward is HmmrEngine.disc_pose (hmmr_disc_pose_fwd), the backward
HmmrEngine.disc_pose_backward (hmmr_disc_pose_bwd, csrc/disc_pose.hip), both on the engine's trainable fp32 bank
(disc_bank.PoseDiscBank).  The derivative is that of the exact fp32 function (include/hmmr_hip.h, "Pose discriminator"); only the
forward's inputs are kept for it."""
from __future__ import annotations

import torch

from .disc_bank import NAMES


def _rows(engine, x):
    """pose rows as an fp32 device tensor [n, 207 or 216] that shares x's memory where it can (so Rs of smpl_apply is used in place)"""
    if x is None:
        return None
    x = x.to(engine.device, torch.float32) if isinstance(x, torch.Tensor) else engine.to_device(x)
    per = x[0].numel() if x.shape[0] else (216 if x.dim() > 1 and x.shape[1] == 24 else 207)
    if per not in (207, 216):
        raise ValueError("pose rows: 207 (joints 1..23) or 216 (all 24 rotations) values per row, got %s" % (tuple(x.shape),))
    return x.reshape(x.shape[0], per)


class _DiscPoseFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, poses_a, poses_b, *bank_tensors):
        a = poses_a.detach() if poses_a is not None else None
        b = poses_b.detach() if poses_b is not None else None
        out = engine.disc_pose(a, b)
        ctx.engine, ctx.has = engine, (a is not None, b is not None)
        ctx.set_materialize_grads(False)             # a cotangent autograd reports absent stays None: nothing is launched for it
        ctx.save_for_backward(*[t for t in (a, b) if t is not None])
        return out

    @staticmethod
    def backward(ctx, d_out):
        n_bank = len(ctx.needs_input_grad) - 3
        none = (None,) * (3 + n_bank)
        if d_out is None:
            return none
        saved = list(ctx.saved_tensors)
        a = saved.pop(0) if ctx.has[0] else None
        b = saved.pop(0) if ctx.has[1] else None
        need = ctx.needs_input_grad
        want_w = [n for i, n in enumerate(NAMES) if need[3 + i]]
        want_a = bool(ctx.has[0] and need[1] and a.shape[0]), bool(ctx.has[1] and need[2] and b.shape[0])
        if not (want_a[0] or want_a[1] or want_w):
            return none
        d_a, d_b, g = ctx.engine.disc_pose_backward(a, b, d_out.contiguous(), want_poses_a=want_a[0], want_poses_b=want_a[1], want_weights=want_w,
                                                    full_a=a is not None and a.shape[1] == 216, full_b=b is not None and b.shape[1] == 216)
        zero = lambda t, want: torch.zeros_like(t) if (t is not None and want and t.shape[0] == 0) else None
        d_a = d_a if d_a is not None else zero(a, ctx.has[0] and need[1])
        d_b = d_b if d_b is not None else zero(b, ctx.has[1] and need[2])
        return (None, d_a, d_b) + tuple(g[n] for n in NAMES)


def disc_pose_apply(engine, poses_a, poses_b=None, bank_tensors=None):
    """Two segments of pose rows ([n,23,1,9], [n,207], or all 24 rotations [n,24,3,3] / [n,216], whose global rotation is dropped) ->
    out [n_a + n_b, 24], differentiable in the poses and in the tensors of engine.disc_pose_bank() -- they are inputs of the autograd
    node, so `.grad` lands on them (set `requires_grad_()` on the ones to train; bank_tensors defaults to
    engine.disc_pose_bank().tensors()).  Through Rs of tf_smpl.autograd.smpl_apply the gradient reaches theta."""
    bank = engine.disc_pose_bank()
    tensors = bank.tensors() if bank_tensors is None else list(bank_tensors)
    views = bank.tensors()
    if len(tensors) != len(views) or any(t.data_ptr() != v.data_ptr() for t, v in zip(tensors, views)):
        raise ValueError("disc_pose_apply: bank_tensors must be the bank's own tensors (engine.disc_pose_bank().tensors()), in their order")
    return _DiscPoseFunction.apply(engine, _rows(engine, poses_a), _rows(engine, poses_b), *tensors)
