"""The trainable pose-discriminator bank: the HMMR_F32 pack of PoseDiscriminator (include/hmmr_hip.h, "Pose discriminator") whose
twelve tensors VIEW the packed memory -- an in-place update of a tensor is what the next hmmr_disc_pose_* call reads, and an optimiser
step on the bank is elementwise: no repack between steps.  The gradients hmmr_disc_pose_bwd / hmmr_pose_prior return have the same
layouts, and `to_checkpoint` / `load_checkpoint` convert either between them and the checkpoint's names and shapes."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import packing

# the twelve tensors in the order of hmmr_disc_pose_grads_t: name, (layer of hmmr_disc_pose_weights_t, its field), shape
LAYERS = (("conv1", ("conv1", "w"), (32, 16)), ("bc1", ("conv1", "shift"), (32,)), ("conv2", ("conv2", "w"), (32, 32)),
          ("bc2", ("conv2", "shift"), (32,)), ("heads", ("heads", "w"), (32, 32)), ("bj", ("heads", "shift"), (32,)),
          ("fc1", ("fc1", "w"), (1024, 1024)), ("b1", ("fc1", "shift"), (1024,)), ("fc2", ("fc2", "w"), (1024, 1024)),
          ("b2", ("fc2", "shift"), (1024,)), ("fc_out", ("fc_out", "w"), (128, 1024)), ("bo", ("fc_out", "shift"), (128,)))
NAMES = tuple(n for n, _, _ in LAYERS)
assert NAMES == L.DISC_POSE_GRAD_NAMES
NUM_JOINTS, FLAT = 23, 736
SCOPE = "D_pose"


def checkpoint_shapes():
    """{checkpoint name: shape} of the 58 variables of the D_pose scope"""
    s = {SCOPE + "/D_conv1/weights": (1, 1, 9, 32), SCOPE + "/D_conv1/biases": (32,), SCOPE + "/D_conv2/weights": (1, 1, 32, 32),
         SCOPE + "/D_conv2/biases": (32,), SCOPE + "/D_alljoints_fc1/weights": (FLAT, 1024), SCOPE + "/D_alljoints_fc1/biases": (1024,),
         SCOPE + "/D_alljoints_fc2/weights": (1024, 1024), SCOPE + "/D_alljoints_fc2/biases": (1024,),
         SCOPE + "/D_alljoints_out/weights": (1024, 1), SCOPE + "/D_alljoints_out/biases": (1,)}
    for j in range(NUM_JOINTS):
        s[SCOPE + "/pose_out_j%d/weights" % j] = (32, 1)
        s[SCOPE + "/pose_out_j%d/biases" % j] = (1,)
    return s


def to_checkpoint(p):
    """{name: tensor in the bank's layouts} -> {checkpoint name: float32 array}: weights, or a set of gradients"""
    a = {n: p[n].detach().cpu().numpy() for n in NAMES}
    out = {SCOPE + "/D_conv1/weights": np.ascontiguousarray(a["conv1"][:, :9].T).reshape(1, 1, 9, 32), SCOPE + "/D_conv1/biases": a["bc1"].copy(),
           SCOPE + "/D_conv2/weights": np.ascontiguousarray(a["conv2"].T).reshape(1, 1, 32, 32), SCOPE + "/D_conv2/biases": a["bc2"].copy(),
           SCOPE + "/D_alljoints_fc1/weights": np.ascontiguousarray(a["fc1"][:, :FLAT].T), SCOPE + "/D_alljoints_fc1/biases": a["b1"].copy(),
           SCOPE + "/D_alljoints_fc2/weights": np.ascontiguousarray(a["fc2"].T), SCOPE + "/D_alljoints_fc2/biases": a["b2"].copy(),
           SCOPE + "/D_alljoints_out/weights": a["fc_out"][0].reshape(1024, 1).copy(), SCOPE + "/D_alljoints_out/biases": a["bo"][:1].copy()}
    for j in range(NUM_JOINTS):
        out[SCOPE + "/pose_out_j%d/weights" % j] = a["heads"][j].reshape(32, 1).copy()
        out[SCOPE + "/pose_out_j%d/biases" % j] = a["bj"][j:j + 1].copy()
    return out


class PoseDiscBank(object):
    """weights: dict of checkpoint-named arrays (D_pose/*).  `dw` is the packed hmmr_disc_pose_weights_t, `params` the
    {name: tensor view} of its twelve tensors (NAMES)."""

    def __init__(self, weights, device):
        self.store = packing.DeviceStore(device)
        self.dw = packing.pack_disc_pose(weights, self.store)
        blob = self.store.tensors[-1]                              # the packer's one blob: every pointer of `dw` lies in it
        base, nbytes = blob.data_ptr(), blob.numel()

        def view(ptr, shape):
            n = int(np.prod(shape)) * 4
            off = int(ptr) - base
            if not (0 <= off and off + n <= nbytes and off % 4 == 0):
                raise L.HmmrError("PoseDiscBank: a packed layer lies outside the bank's blob")
            return blob[off:off + n].view(torch.float32).view(*shape)

        self.blob = blob
        self.params = {name: view(getattr(getattr(self.dw, lay), field), shape) for name, (lay, field), shape in LAYERS}

    @property
    def device(self):
        return self.blob.device

    def tensors(self):
        """the twelve tensor views in the order of NAMES"""
        return [self.params[n] for n in NAMES]

    def like(self, fill=None):
        """a set of new tensors in the bank's layouts (zeros, or uninitialised with fill=None): what the backward writes"""
        make = torch.empty if fill is None else torch.zeros
        return {n: make(self.params[n].shape, dtype=torch.float32, device=self.device) for n in NAMES}

    def to_checkpoint(self, tensors=None):
        """{checkpoint name: float32 array} of the bank in the checkpoint's shapes ([1,1,9,32], [32,1] per joint, [736,1024], ...) or,
        with `tensors` ({name: tensor} in the bank's layouts: a set of gradients), the same conversion of those"""
        return to_checkpoint(self.params if tensors is None else tensors)

    def load_checkpoint(self, ckpt):
        """write checkpoint-named arrays into the bank in place (the padding stays zero); names the bank does not hold are refused"""
        shapes = checkpoint_shapes()
        unknown = sorted(set(ckpt) - set(shapes))
        if unknown:
            raise KeyError("PoseDiscBank.load_checkpoint: not a variable of this bank: %s" % ", ".join(unknown))
        p = self.params

        def put(dst, name):
            a = np.asarray(ckpt[name], np.float32)
            if a.shape != shapes[name]:
                raise ValueError("%s has shape %s, the bank holds %s" % (name, a.shape, shapes[name]))
            return dst, a

        with torch.no_grad():
            for name in ckpt:
                tail = name[len(SCOPE) + 1:]
                scope, kind = tail.rsplit("/", 1)
                if scope.startswith("pose_out_j"):
                    j = int(scope[len("pose_out_j"):])
                    dst, a = put(p["heads"][j] if kind == "weights" else p["bj"][j:j + 1], name)
                    a = a.reshape(-1)
                elif kind == "biases":
                    key, n = {"D_conv1": ("bc1", 32), "D_conv2": ("bc2", 32), "D_alljoints_fc1": ("b1", 1024), "D_alljoints_fc2": ("b2", 1024),
                              "D_alljoints_out": ("bo", 1)}[scope]
                    dst, a = put(p[key][:n], name)
                else:
                    dst = {"D_conv1": p["conv1"][:, :9], "D_conv2": p["conv2"], "D_alljoints_fc1": p["fc1"][:, :FLAT], "D_alljoints_fc2": p["fc2"],
                           "D_alljoints_out": p["fc_out"][:1]}[scope]
                    dst, a = put(dst, name)
                    a = a.reshape(-1, a.shape[-1]).T
                dst.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dst.device))
        return self
