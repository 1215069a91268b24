"""SMPL under torch.autograd: the forward is HmmrEngine.smpl (hmmr_smpl_fwd, its default blend form, unchanged), the backward
HmmrEngine.smpl_backward (hmmr_smpl_bwd, csrc/smpl_grad.hip).  The derivative is that of the exact fp32 function (include/hmmr_hip.h,
"SMPL backward"); nothing but the forward's inputs and its `joints` is kept for it."""
from __future__ import annotations

import torch


class _SmplFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, theta, beta, cams):
        theta, beta = theta.detach(), beta.detach()
        cams = cams.detach() if cams is not None else None
        verts, joints, kps, rs = engine.smpl(theta, beta, cams, want_rs=True)
        ctx.engine, ctx.has_cams = engine, cams is not None
        ctx.set_materialize_grads(False)             # an output the loss does not use arrives as None and reaches the kernel as NULL
        ctx.save_for_backward(theta, beta, joints, *([cams] if cams is not None else []))
        if kps is None:
            return verts, joints, rs
        return verts, joints, kps, rs

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        theta, beta, joints = saved[:3]
        cams = saved[3] if ctx.has_cams else None
        if ctx.has_cams:
            d_verts, d_joints, d_kps, d_rs = grads
        else:
            (d_verts, d_joints, d_rs), d_kps = grads, None
        want_cams = ctx.has_cams and ctx.needs_input_grad[3]
        if all(g is None for g in (d_verts, d_joints, d_kps, d_rs)):
            return None, None, None, None
        d_theta, d_beta, d_cams = ctx.engine.smpl_backward(theta, beta, cams, joints, d_verts=d_verts, d_joints=d_joints, d_kps=d_kps,
                                                           d_rs=d_rs, want_cams=want_cams)
        return (None, d_theta.reshape(theta.shape) if ctx.needs_input_grad[1] else None,
                d_beta.reshape(beta.shape) if ctx.needs_input_grad[2] else None, d_cams)


def smpl_apply(engine, theta, beta, cams=None):
    """theta [m,72], beta [m,10], cams [m,3] or None (fp32 tensors on the engine's device) -> (verts [m,V,3], joints [m,K,3],
    kps [m,K,2] or None, Rs [m,24,3,3]), differentiable in theta, beta and cams.  An output whose gradient autograd reports as
    absent reaches hmmr_smpl_bwd as NULL."""
    def prep(x, width):                      # (a tensor stays in the graph; a row-major view with unit inner stride stays in place)
        x = x.to(engine.device, torch.float32) if isinstance(x, torch.Tensor) else engine.to_device(x)
        return x.reshape(-1, width)
    theta, beta = prep(theta, 72), prep(beta, 10)
    if cams is not None:
        cams = prep(cams, 3)
        return _SmplFunction.apply(engine, theta, beta, cams)
    verts, joints, rs = _SmplFunction.apply(engine, theta, beta, None)
    return verts, joints, None, rs
