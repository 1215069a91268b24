"""The trainable IEF bank: an HMMR_F32 pack of the regressors (include/hmmr_hip.h, "IEF backward") whose layers are torch tensors that
VIEW the packed device memory -- an in-place update of a tensor is what the next hmmr_ief_fwd_train / hmmr_ief_bwd call reads, and an
optimiser step on the bank is elementwise: no repack between steps.  The gradients hmmr_ief_bwd returns have the same layouts, and
`to_checkpoint` / `load_checkpoint` convert either between them and the checkpoint's names and shapes."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import assets, packing

# the seven tensors of a regressor, in the order of hmmr_ief_reg_grads_t: name, (hmmr_ief_regressor_t layer, its field), shape
LAYERS = (("fc1_phi", ("fc1_phi", "w"), (1024, 2048)), ("fc1_theta", ("fc1_theta", "w"), (1024, 128)), ("fc2", ("fc2", "w"), (1024, 1024)),
          ("fc3", ("fc3", "w"), (128, 1024)), ("b1", ("fc1_phi", "shift"), (1024,)), ("b2", ("fc2", "shift"), (1024,)), ("b3", ("fc3", "shift"), (128,)))
NAMES = tuple(n for n, _, _ in LAYERS)


class IefBank(object):
    """weights: dict of checkpoint-named arrays (single_view_ief*/3D_module/*, mean_param); delta_keys: the delta regressors' offsets.
    `iw` is the packed hmmr_ief_weights_t, `keys` the regressors' delta_t in the packed order ([0] + sorted deltas), `params[r]` the
    {name: tensor view} of regressor r."""

    def __init__(self, weights, delta_keys, device, num_stages=3):
        self.store = packing.DeviceStore(device)
        w = {k: v for k, v in weights.items() if k.startswith("single_view_ief") or k == "mean_param"}
        self.iw, self.keys = packing.pack_ief(w, L.HMMR_F32, self.store, list(delta_keys), num_stages=num_stages)
        blob = self.store.tensors[-1]                              # the packer's one blob: every pointer of `iw` lies in it
        base, nbytes = blob.data_ptr(), blob.numel()

        def view(ptr, shape):
            n = int(np.prod(shape)) * 4
            off = int(ptr) - base
            if not (0 <= off and off + n <= nbytes and off % 4 == 0):
                raise L.HmmrError("IefBank: a packed layer lies outside the bank's blob")
            return blob[off:off + n].view(torch.float32).view(*shape)

        self.scopes = assets.ief_scopes([k for k in self.keys if k != 0])
        self.nd = [int(self.iw.reg[r].nd) for r in range(len(self.keys))]
        self.params = [{name: view(getattr(getattr(self.iw.reg[r], lay), field), shape) for name, (lay, field), shape in LAYERS}
                       for r in range(len(self.keys))]
        self.mean_theta = view(self.iw.mean_theta, (85,))

    @property
    def num_regressors(self):
        return len(self.keys)

    def tensors(self):
        """the 7 R tensor views in one fixed order: regressor after regressor, each in the order of NAMES"""
        return [p[n] for p in self.params for n in NAMES]

    def like(self, fill=None):
        """a set of new tensors in the bank's layouts (zeros, or uninitialised with fill=None): what hmmr_ief_bwd writes"""
        make = torch.empty if fill is None else torch.zeros
        return [{n: make(p[n].shape, dtype=torch.float32, device=p[n].device) for n in NAMES} for p in self.params]

    def to_checkpoint(self, tensors=None):
        """{checkpoint name: float32 array} of the bank -- fc1/weights [2048 + nd, 1024], fc1/biases, fc2/weights [1024, 1024],
        fc2/biases, fc3/weights [1024, nd], fc3/biases [nd] per scope, and mean_param -- or, with `tensors` (a list of {name: tensor}
        in the bank's layouts, one per regressor: a set of gradients), the same conversion of those (without mean_param)"""
        out = {}
        for r, key in enumerate(self.keys):
            p, nd = (self.params if tensors is None else tensors)[r], self.nd[r]
            a = {n: p[n].detach().cpu().numpy() for n in NAMES}
            s = self.scopes[key][0] + "/3D_module"
            out[s + "/fc1/weights"] = np.ascontiguousarray(np.concatenate([a["fc1_phi"].T, a["fc1_theta"][:, :nd].T], axis=0))
            out[s + "/fc1/biases"] = a["b1"].copy()
            out[s + "/fc2/weights"] = np.ascontiguousarray(a["fc2"].T)
            out[s + "/fc2/biases"] = a["b2"].copy()
            out[s + "/fc3/weights"] = np.ascontiguousarray(a["fc3"][:nd].T)
            out[s + "/fc3/biases"] = a["b3"][:nd].copy()
        if tensors is None:
            out["mean_param"] = self.mean_theta.detach().cpu().numpy().reshape(1, 85).copy()
        return out

    def load_checkpoint(self, ckpt):
        """write checkpoint-named arrays into the bank in place (the padding stays zero); names the bank does not hold are refused"""
        known = set(self.to_checkpoint())
        unknown = sorted(set(ckpt) - known)
        if unknown:
            raise KeyError("IefBank.load_checkpoint: not a variable of this bank: %s" % ", ".join(unknown))
        put = lambda dst, a: dst.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dst.device))
        with torch.no_grad():
            for r, key in enumerate(self.keys):
                p, nd = self.params[r], self.nd[r]
                s = self.scopes[key][0] + "/3D_module"
                if s + "/fc1/weights" in ckpt:
                    W1 = np.asarray(ckpt[s + "/fc1/weights"], np.float32)
                    if W1.shape != (2048 + nd, 1024):
                        raise ValueError("%s/fc1/weights has shape %s, the bank holds (%d, 1024)" % (s, W1.shape, 2048 + nd))
                    put(p["fc1_phi"], W1[:2048].T)
                    put(p["fc1_theta"][:, :nd], W1[2048:].T)
                if s + "/fc2/weights" in ckpt:
                    put(p["fc2"], np.asarray(ckpt[s + "/fc2/weights"], np.float32).reshape(1024, 1024).T)
                if s + "/fc3/weights" in ckpt:
                    put(p["fc3"][:nd], np.asarray(ckpt[s + "/fc3/weights"], np.float32).reshape(1024, nd).T)
                for b, layer, n in (("b1", "fc1", 1024), ("b2", "fc2", 1024), ("b3", "fc3", nd)):
                    if s + "/%s/biases" % layer in ckpt:
                        put(p[b][:n], np.asarray(ckpt[s + "/%s/biases" % layer], np.float32).reshape(n))
            if "mean_param" in ckpt:
                put(self.mean_theta, np.asarray(ckpt["mean_param"], np.float32).reshape(85))
        return self
