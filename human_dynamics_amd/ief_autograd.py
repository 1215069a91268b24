"""The IEF regressors under torch.autograd: the forward is HmmrEngine.ief_train (hmmr_ief_fwd_train), the backward
HmmrEngine.ief_backward (hmmr_ief_bwd, csrc/ief_grad.hip), both on the engine's trainable fp32 bank (ief_bank.IefBank).  The
derivative is that of the exact fp32 function (include/hmmr_hip.h, "IEF backward"); only the forward's inputs are kept for it."""
from __future__ import annotations

import torch

from .ief_bank import NAMES


class _IefFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, strips, omega_start, keep, keep_prob, use_delta_from_pred, *bank_tensors):
        strips = strips.detach()
        omega_start = omega_start.detach() if omega_start is not None else None
        omegas = engine.ief_train(strips, omega_start, keep, keep_prob, use_delta_from_pred)
        ctx.engine, ctx.keep_prob, ctx.from_pred = engine, keep_prob, use_delta_from_pred
        ctx.has_start, ctx.has_keep = omega_start is not None, keep is not None
        ctx.set_materialize_grads(False)             # a cotangent autograd reports absent stays None: nothing is launched for it
        ctx.save_for_backward(strips, *([omega_start] if omega_start is not None else []), *([keep] if keep is not None else []))
        return omegas

    @staticmethod
    def backward(ctx, d_omegas):
        n_bank = len(ctx.needs_input_grad) - 6
        if d_omegas is None:
            return (None,) * (6 + n_bank)
        saved = list(ctx.saved_tensors)
        strips = saved.pop(0)
        omega_start = saved.pop(0) if ctx.has_start else None
        keep = saved.pop(0) if ctx.has_keep else None
        need = ctx.needs_input_grad
        want_w = [[n for i, n in enumerate(NAMES) if need[6 + 7 * r + i]] for r in range(n_bank // 7)]
        want_strips, want_start = need[1], ctx.has_start and need[2]
        if not (want_strips or want_start or any(want_w)):
            return (None,) * (6 + n_bank)
        d_strips, d_start, grads = ctx.engine.ief_backward(strips, d_omegas, omega_start, keep, ctx.keep_prob, ctx.from_pred,
                                                           want_strips=want_strips, want_start=want_start, want_weights=want_w)
        return (None, d_strips, d_start, None, None, None) + tuple(g[n] for g in grads for n in NAMES)


def ief_apply(engine, strips, omega_start=None, keep=None, keep_prob=None, use_delta_from_pred=True, bank_tensors=None):
    """strips [m,2048], omega_start [m,85] or None (fp32 tensors on the engine's device) -> omegas [R,m,85], differentiable in strips,
    omega_start and the parameter tensors of engine.ief_bank() -- they are inputs of the autograd node, so `.grad` lands on them
    (set `requires_grad_()` on the ones to train; bank_tensors defaults to engine.ief_bank().tensors()).  keep / keep_prob: the dropout
    mask of HmmrEngine.ief_train.  A cotangent that autograd reports absent reaches hmmr_ief_bwd as NULL."""
    bank = engine.ief_bank()
    tensors = bank.tensors() if bank_tensors is None else list(bank_tensors)
    views = bank.tensors()
    if len(tensors) != len(views) or any(t.data_ptr() != v.data_ptr() for t, v in zip(tensors, views)):
        raise ValueError("ief_apply: bank_tensors must be the bank's own tensors (engine.ief_bank().tensors()), in their order")
    prep = lambda x, width: (x.to(engine.device, torch.float32) if isinstance(x, torch.Tensor) else engine.to_device(x)).reshape(-1, width)
    strips = prep(strips, 2048)
    if omega_start is not None:
        omega_start = prep(omega_start, 85)
        if omega_start.shape[0] == 1:
            omega_start = omega_start.expand(strips.shape[0], 85)
    if keep is not None:
        keep = (keep if isinstance(keep, torch.Tensor) else torch.tensor(keep)).to(engine.device, torch.uint8).contiguous()
    return _IefFunction.apply(engine, strips, omega_start, keep, keep_prob, bool(use_delta_from_pred), *tensors)
