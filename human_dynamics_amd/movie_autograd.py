"""f_movie under torch.autograd: the temporal encoder (forward HmmrEngine.temporal_train, backward HmmrEngine.temporal_backward) and the
hallucinator (hallucinate_train / hallucinate_backward), both on the engine's trainable fp32 bank (movie_bank.MovieBank; csrc/movie_grad.hip).
The derivative is that of the exact fp32 function (include/hmmr_hip.h, "f_movie / hallucinator backward"); only the forward's input is
kept for it."""
from __future__ import annotations

import torch

from .movie_bank import BLOCK_NAMES, HAL_NAMES


class _TemporalFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, phi, *bank_tensors):
        phi = phi.detach()
        strips = engine.temporal_train(phi)
        ctx.engine = engine
        ctx.set_materialize_grads(False)             # a cotangent autograd reports absent stays None: nothing is launched for it
        ctx.save_for_backward(phi)
        return strips

    @staticmethod
    def backward(ctx, d_strips):
        need = ctx.needs_input_grad
        n_bank = len(need) - 2
        nothing = (None,) * (2 + n_bank)
        if d_strips is None:
            return nothing
        nb = len(BLOCK_NAMES)
        want_w = [[n for i, n in enumerate(BLOCK_NAMES) if need[2 + nb * k + i]] for k in range(n_bank // nb)]
        if not (need[1] or any(want_w)):
            return nothing
        (phi,) = ctx.saved_tensors
        d_phi, grads = ctx.engine.temporal_backward(phi, d_strips.contiguous(), want_phi=need[1], want_weights=want_w)
        return (None, d_phi) + tuple(g[n] for g in grads for n in BLOCK_NAMES)


class _HallucinatorFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, phi, *bank_tensors):
        phi = phi.detach()
        out = engine.hallucinate_train(phi)
        ctx.engine = engine
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(phi)
        return out

    @staticmethod
    def backward(ctx, d_out):
        need = ctx.needs_input_grad
        nothing = (None,) * len(need)
        if d_out is None:
            return nothing
        want_w = [n for i, n in enumerate(HAL_NAMES) if need[2 + i]]
        if not (need[1] or want_w):
            return nothing
        (phi,) = ctx.saved_tensors
        d_phi, g = ctx.engine.hallucinate_backward(phi, d_out.contiguous(), want_phi=need[1], want_weights=want_w)
        return (None, d_phi) + tuple(g[n] for n in HAL_NAMES)


def _own(tensors, views, who, what):
    tensors = views if tensors is None else list(tensors)
    if len(tensors) != len(views) or any(t.data_ptr() != v.data_ptr() for t, v in zip(tensors, views)):
        raise ValueError("%s: bank_tensors must be the bank's own tensors (engine.movie_bank().%s()), in their order" % (who, what))
    return tensors


def _prep(engine, phi):
    return phi.to(engine.device, torch.float32) if isinstance(phi, torch.Tensor) else engine.to_device(phi)


def temporal_apply(engine, phi, bank_tensors=None):
    """phi [b,t,2048] (an fp32 tensor on the engine's device) -> movie strips [b,t,2048], differentiable in phi and the temporal tensors of
    engine.movie_bank() -- they are inputs of the autograd node, so `.grad` lands on them (set `requires_grad_()` on the ones to train;
    bank_tensors defaults to engine.movie_bank().temporal_tensors()).  A cotangent that autograd reports absent queues nothing."""
    tensors = _own(bank_tensors, engine.movie_bank().temporal_tensors(), "temporal_apply", "temporal_tensors")
    phi = _prep(engine, phi)
    if phi.dim() != 3 or phi.shape[2] != 2048:
        raise ValueError("temporal_apply: phi is [b, t, 2048], got %s" % (tuple(phi.shape),))
    return _TemporalFunction.apply(engine, phi.contiguous(), *tensors)


def hallucinate_apply(engine, phi, bank_tensors=None):
    """phi [..., 2048] -> hallucinated movie strips of the same shape, differentiable in phi and the hallucinator's tensors of
    engine.movie_bank() (bank_tensors defaults to engine.movie_bank().hallucinator_tensors())."""
    bank = engine._hal_bank()
    tensors = _own(bank_tensors, bank.hallucinator_tensors(), "hallucinate_apply", "hallucinator_tensors")
    phi = _prep(engine, phi)
    if phi.shape[-1] != 2048:
        raise ValueError("hallucinate_apply: phi is [..., 2048], got %s" % (tuple(phi.shape),))
    return _HallucinatorFunction.apply(engine, phi.contiguous(), *tensors)
