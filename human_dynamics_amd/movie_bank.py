"""The trainable f_movie bank: an HMMR_F32 pack of the temporal encoder's blocks and, when the checkpoint has one, of the hallucinator
(include/hmmr_hip.h, "f_movie / hallucinator backward") whose layers are torch tensors that VIEW the packed device memory -- an in-place
update of a tensor is what the next hmmr_temporal_fwd / hmmr_temporal_bwd (hmmr_hallucinator_fwd / _bwd) call on the bank reads, and an
optimiser step on the bank is elementwise: no repack between steps.  The gradients the backward entry points return have the same
layouts, and `to_checkpoint` / `load_checkpoint` convert either between them and the checkpoint's names and shapes (conv weights
[3, 1, 2048, 2048] HWIO, fc weights [in, out])."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import assets, packing

C_ = 2048
# the eight tensors of a block in the order of hmmr_temporal_block_grads_t: name, path into hmmr_temporal_block_t, shape
BLOCK_LAYERS = (("gn1_gamma", ("gn1_gamma",), (C_,)), ("gn1_beta", ("gn1_beta",), (C_,)), ("conv1", ("conv1", "w"), (C_, 3 * C_)),
                ("b1", ("conv1", "shift"), (C_,)), ("gn2_gamma", ("gn2_gamma",), (C_,)), ("gn2_beta", ("gn2_beta",), (C_,)),
                ("conv2", ("conv2", "w"), (C_, 3 * C_)), ("b2", ("conv2", "shift"), (C_,)))
# the six of the hallucinator in the order of hmmr_hallucinator_bwd_desc_t
HAL_LAYERS = (("fc1", ("fc1", "w"), (C_, C_)), ("fc2", ("fc2", "w"), (C_, C_)), ("fc3", ("fc3", "w"), (C_, C_)),
              ("b1", ("fc1", "shift"), (C_,)), ("b2", ("fc2", "shift"), (C_,)), ("b3", ("fc3", "shift"), (C_,)))
BLOCK_NAMES = tuple(n for n, _, _ in BLOCK_LAYERS)
HAL_NAMES = tuple(n for n, _, _ in HAL_LAYERS)
assert BLOCK_NAMES == L.TEMPORAL_GRAD_NAMES and HAL_NAMES == L.HALLUCINATOR_GRAD_NAMES


def conv_to_hwio(bank_rows):
    """[2048][tap * 2048 + ci] (packing.pack_conv_weight's rows) -> [3, 1, ci, co]"""
    a = np.asarray(bank_rows)
    return np.ascontiguousarray(a.reshape(C_, 3, C_).transpose(1, 2, 0)[:, None])


def conv_from_hwio(w_hwio):
    a = np.asarray(w_hwio, np.float32)
    if a.shape != (3, 1, C_, C_):
        raise ValueError("a temporal conv weight has shape (3, 1, 2048, 2048), got %s" % (a.shape,))
    return np.ascontiguousarray(a.reshape(3 * C_, C_).T)


class MovieBank(object):
    """weights: dict of checkpoint-named arrays (AZ_FC_block*, fc2_res/*).  `tw` is the packed hmmr_temporal_weights_t, `hw` the
    hmmr_hallucinator_weights_t or None, `blocks[i]` the {name: tensor view} of temporal block i, `hal` that of the hallucinator."""

    def __init__(self, weights, device, num_conv_layers=3):
        self.store = packing.DeviceStore(device)
        w = {k: v for k, v in weights.items() if k.startswith(("AZ_FC_block", "fc2_res/"))}
        self.num_blocks = int(num_conv_layers)
        self.tw = packing.pack_temporal(w, L.HMMR_F32, self.store, self.num_blocks)
        self.blocks = [self._views(self.store.tensors[-1], self.tw.block[i], BLOCK_LAYERS) for i in range(self.num_blocks)]
        self.hw = packing.pack_hallucinator(w, L.HMMR_F32, self.store)
        self.hal = self._views(self.store.tensors[-1], self.hw, HAL_LAYERS) if self.hw is not None else None

    @staticmethod
    def _views(blob, struct, layers):
        base, nbytes = blob.data_ptr(), blob.numel()            # the packer's one blob: every pointer of the struct lies in it

        def view(path, shape):
            p = struct
            for f in path:
                p = getattr(p, f)
            n, off = int(np.prod(shape)) * 4, int(p) - base
            if not (0 <= off and off + n <= nbytes and off % 4 == 0):
                raise L.HmmrError("MovieBank: a packed layer lies outside the bank's blob")
            return blob[off:off + n].view(torch.float32).view(*shape)

        return {name: view(path, shape) for name, path, shape in layers}

    def temporal_tensors(self):
        """the 8 num_blocks tensor views in one fixed order: block after block, each in the order of BLOCK_NAMES"""
        return [p[n] for p in self.blocks for n in BLOCK_NAMES]

    def hallucinator_tensors(self):
        return [self.hal[n] for n in HAL_NAMES] if self.hal is not None else []

    def tensors(self):
        """every tensor view: the temporal blocks', then the hallucinator's six"""
        return self.temporal_tensors() + self.hallucinator_tensors()

    def like(self, fill=None):
        """a set of new tensors in the bank's layouts (zeros, or uninitialised with fill=None): ([{name: tensor}] per block, {name: tensor}
        of the hallucinator or None) -- what hmmr_temporal_bwd / hmmr_hallucinator_bwd write"""
        make = torch.empty if fill is None else torch.zeros
        new = lambda p: {n: make(v.shape, dtype=torch.float32, device=v.device) for n, v in p.items()}
        return [new(p) for p in self.blocks], (new(self.hal) if self.hal is not None else None)

    def to_checkpoint(self, tensors=None):
        """{checkpoint name: float32 array} of the bank -- <gn>/gamma, <gn>/beta, <conv>/weights [3, 1, 2048, 2048], <conv>/biases per
        block, fc2_res/fc*/weights [in, out] and biases -- or, with `tensors` (the pair `like` returns: a set of gradients; the
        hallucinator's part may be None), the same conversion of those"""
        blocks, hal = (self.blocks, self.hal) if tensors is None else tensors
        a = lambda t: t.detach().cpu().numpy()
        out = {}
        for i, p in enumerate(blocks):
            gn1, c1, gn2, c2 = assets.temporal_scopes(i)
            for gn, k in ((gn1, "gn1"), (gn2, "gn2")):
                out[gn + "/gamma"], out[gn + "/beta"] = a(p[k + "_gamma"]).copy(), a(p[k + "_beta"]).copy()
            for cv, k, bk in ((c1, "conv1", "b1"), (c2, "conv2", "b2")):
                out[cv + "/weights"], out[cv + "/biases"] = conv_to_hwio(a(p[k])), a(p[bk]).copy()
        if hal is not None:
            for k in ("fc1", "fc2", "fc3"):
                out["fc2_res/%s/weights" % k] = np.ascontiguousarray(a(hal[k]).T)
                out["fc2_res/%s/biases" % k] = a(hal["b" + k[2]]).copy()
        return out

    def load_checkpoint(self, ckpt):
        """write checkpoint-named arrays into the bank in place; names the bank does not hold are refused"""
        known = set(self.to_checkpoint_names())
        unknown = sorted(set(ckpt) - known)
        if unknown:
            raise KeyError("MovieBank.load_checkpoint: not a variable of this bank: %s" % ", ".join(unknown))

        def put(dst, arr):
            arr = np.array(arr, dtype=np.float32, order="C")          # (a copy: torch.from_numpy wants a writable array)
            if arr.shape != tuple(dst.shape):
                raise ValueError("a variable of shape %s does not fit the bank's %s" % (arr.shape, tuple(dst.shape)))
            dst.copy_(torch.from_numpy(arr).to(dst.device))

        with torch.no_grad():
            for i, p in enumerate(self.blocks):
                gn1, c1, gn2, c2 = assets.temporal_scopes(i)
                for name, dst, conv in ((gn1 + "/gamma", p["gn1_gamma"], 0), (gn1 + "/beta", p["gn1_beta"], 0), (c1 + "/weights", p["conv1"], 1),
                                        (c1 + "/biases", p["b1"], 0), (gn2 + "/gamma", p["gn2_gamma"], 0), (gn2 + "/beta", p["gn2_beta"], 0),
                                        (c2 + "/weights", p["conv2"], 1), (c2 + "/biases", p["b2"], 0)):
                    if name in ckpt:
                        put(dst, conv_from_hwio(ckpt[name]) if conv else np.asarray(ckpt[name], np.float32).reshape(-1))
            if self.hal is not None:
                for k in ("fc1", "fc2", "fc3"):
                    if "fc2_res/%s/weights" % k in ckpt:
                        put(self.hal[k], np.asarray(ckpt["fc2_res/%s/weights" % k], np.float32).reshape(C_, C_).T)
                    if "fc2_res/%s/biases" % k in ckpt:
                        put(self.hal["b" + k[2]], np.asarray(ckpt["fc2_res/%s/biases" % k], np.float32).reshape(-1))
        return self

    def to_checkpoint_names(self):
        """the checkpoint names of the bank's variables (no copy of the bank is made)"""
        names = []
        for i in range(self.num_blocks):
            gn1, c1, gn2, c2 = assets.temporal_scopes(i)
            names += [gn1 + "/gamma", gn1 + "/beta", c1 + "/weights", c1 + "/biases", gn2 + "/gamma", gn2 + "/beta", c2 + "/weights", c2 + "/biases"]
        if self.hal is not None:
            names += ["fc2_res/%s/%s" % (k, v) for k in ("fc1", "fc2", "fc3") for v in ("weights", "biases")]
        return names
