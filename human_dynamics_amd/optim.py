"""tf.train.AdamOptimizer for tensors on the device (HmmrEngine.adam_step -> hmmr_adam_step, csrc/adam.hip): the reference's optimiser
(src/trainer_sequence_fc.py: self.optimizer), one fused launch set per step over every tensor that has a gradient.

This is TF 1.x's Adam, not torch.optim.Adam (include/hmmr_hip.h, "TF Adam"): epsilon is added to sqrt(v) before the bias correction
is folded into the step size, and the beta powers are float32 values multiplied by beta once per step, after the update
(AdamOptimizer._finish).  The tensors are usually the views of a bank (movie_bank, ief_bank, disc_bank): the update is in place, so
the next forward on the bank reads it, and the moments have the bank's layouts, so a bank's `to_checkpoint(tensors=...)` converts
them as it converts gradients."""
from __future__ import annotations

import numpy as np
import torch


class TFAdam(object):
    """tensors: the fp32 device tensors to train (contiguous; `requires_grad_()` is the caller's).  `m` and `v` are zeros in their
    shapes; `beta1_power` / `beta2_power` are np.float32 values, beta before the first step."""

    def __init__(self, engine, tensors, lr, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.engine = engine
        self.tensors = list(tensors)
        self.lr, self.beta1, self.beta2, self.epsilon = float(lr), float(beta1), float(beta2), float(epsilon)
        self.m = [torch.zeros_like(t, memory_format=torch.contiguous_format).detach() for t in self.tensors]
        self.v = [torch.zeros_like(t, memory_format=torch.contiguous_format).detach() for t in self.tensors]
        self.beta1_power, self.beta2_power = np.float32(self.beta1), np.float32(self.beta2)
        self.steps = 0

    def step(self):
        """one ApplyAdam over every tensor whose `.grad` is set (None: the tensor and its moments keep their bytes), then the beta
        powers advance -- also when no tensor had a gradient, as TF's _finish runs with every apply_gradients"""
        segs = [(t.detach(), (t.grad.detach().contiguous() if t.grad is not None else None), m, v) for t, m, v in zip(self.tensors, self.m, self.v)]
        self.engine.adam_step(segs, self.lr, self.beta1, self.beta2, self.epsilon, self.beta1_power, self.beta2_power)
        self.beta1_power = np.float32(self.beta1_power * np.float32(self.beta1))
        self.beta2_power = np.float32(self.beta2_power * np.float32(self.beta2))
        self.steps += 1

    def zero_grad(self):
        for t in self.tensors:
            t.grad = None

    @staticmethod
    def slot_names(variable):
        """TF's names of a variable's two Adam slots: (<variable>/Adam, <variable>/Adam_1) = (m, v)"""
        return variable + "/Adam", variable + "/Adam_1"

    def state_dict(self, to_checkpoint=None):
        """{<variable>/Adam: m, <variable>/Adam_1: v, beta1_power, beta2_power} as float32 arrays.  to_checkpoint: a function from the
        list of tensors (the moments, in the order of `tensors`) to {checkpoint name: array} -- for a bank,
        lambda ts: bank.to_checkpoint(tensors=<ts in the shape `like` returns>); None names the tensors by their index."""
        conv = to_checkpoint if to_checkpoint is not None else (lambda ts: {"var_%d" % i: t.detach().cpu().numpy().copy() for i, t in enumerate(ts)})
        out = {"beta1_power": np.float32(self.beta1_power), "beta2_power": np.float32(self.beta2_power)}
        for slot, ts in ((0, self.m), (1, self.v)):
            for name, a in conv(ts).items():
                out[self.slot_names(name)[slot]] = np.asarray(a, np.float32)
        return out

    def load_state_dict(self, state, from_checkpoint=None):
        """the inverse of `state_dict`.  from_checkpoint: a function ({checkpoint name: array}, the list of tensors to fill); None
        reads the index names."""
        def fill(ckpt, ts):
            with torch.no_grad():
                for i, t in enumerate(ts):
                    t.copy_(torch.from_numpy(np.ascontiguousarray(ckpt["var_%d" % i], dtype=np.float32)).to(t.device).reshape(t.shape))
        put = from_checkpoint if from_checkpoint is not None else fill
        for suffix, ts in (("/Adam", self.m), ("/Adam_1", self.v)):
            put({k[:-len(suffix)]: v for k, v in state.items() if k.endswith(suffix)}, ts)
        self.beta1_power, self.beta2_power = np.float32(state["beta1_power"]), np.float32(state["beta2_power"])
        return self
