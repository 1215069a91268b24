"""Mirror of src/datasets/resnet_extractor.py: ResNet-only feature extraction
(BASELINE config 2).  ``FeatureExtractor(model_path, img_size=224, batch_size=64)``
with ``compute_phis(images[B,H,W,3]) -> [B,2048]`` and
``compute_all_phis(all_images[T,H,W,3]) -> [T,2048]`` (zero-padded tail batch,
resnet_extractor.py:74-98).  Both also take crops that already lie on the device, and
``compute_all_phis_augmented`` puts the tube augmentor (util/tube_augmentation.py) in front of them as the
reference's tfrecord writers do."""
from __future__ import annotations

import numpy as np
import torch

from ..engine import DEFAULT_DTYPE, HmmrEngine
from ..evaluation.tester import load_weights


class FeatureExtractor(object):
    def __init__(self, model_path, img_size=224, batch_size=64, sess=None, weights=None,
                 dtype=DEFAULT_DTYPE, device="cuda:0"):
        if img_size != 224:
            raise ValueError("the ResNet stage is built for 224x224 crops")
        self.model_path = model_path
        self.img_size = img_size
        self.batch_size = batch_size
        if weights is None:
            weights = load_weights(model_path)
        self.engine = HmmrEngine(weights, None, dtype=dtype, device=device)

    def compute_phis(self, images, to_numpy=True):
        """images (BxHxWx3), a host array or a CUDA float32 tensor (used where it lies) -> phis (Bx2048): a float32 ndarray,
        or with to_numpy=False the device tensor (on the current stream, not synchronised)."""
        if isinstance(images, torch.Tensor):
            if not (images.is_cuda and images.dtype == torch.float32):
                raise ValueError("a tensor batch must be CUDA float32 [B,%d,%d,3]" % (self.img_size, self.img_size))
            images = images.contiguous()
        else:
            images = np.asarray(images, np.float32)
        phi = self.engine.resnet(images)
        if not to_numpy:
            return phi
        torch.cuda.synchronize(self.engine.device)
        return phi.cpu().numpy()

    def compute_all_phis(self, all_images, to_numpy=True):
        """all_images (TxHxWx3), a host array or a CUDA float32 tensor -> phis (Tx2048).  A device tensor is batched, and its
        last batch padded with zero frames, on the device: no host copy of the crops."""
        all_phis = []
        T = len(all_images)
        on_device = isinstance(all_images, torch.Tensor)
        for i in range(0, T, self.batch_size):
            if on_device:
                images = all_images[i:i + self.batch_size]
            else:
                images = np.asarray(all_images[i:i + self.batch_size], np.float32)
            if len(images) < self.batch_size:          # pad the last batch with zeros
                leftover = self.batch_size - len(images)
                if on_device:
                    images = torch.cat((images, images.new_zeros((leftover, self.img_size, self.img_size, 3))))
                else:
                    pad = np.zeros((leftover, self.img_size, self.img_size, 3), np.float32)
                    images = np.vstack((images, pad))
            all_phis.append(self.compute_phis(images, to_numpy=to_numpy))
        if to_numpy:
            return np.vstack(all_phis)[:T]
        return torch.cat(all_phis)[:T]

    def compute_all_phis_augmented(self, augmentor, images, image_sizes, labels, centers, poses, gt3ds, keep_images=True, **kw):
        """The writers' call site (upenn_to_tfrecords_video.py:194-211) in one step: `augmentor` (a
        util.tube_augmentation.TubePreprocessorDriver built with img_size=224) augments the tube on the device and its crops
        go straight into the ResNet.  Returns the driver's dict plus `phis` (Tx2048 ndarray); `images` are downloaded only
        with keep_images=True (the reference's dict has them), otherwise the key holds the device tensor.
        Keyword arguments (rng=, walks=, flip=) go to the augmentor."""
        ret = augmentor.run_device(images, image_sizes, labels, centers, poses, gt3ds, device=self.engine.device, **kw)
        ret["phis"] = self.compute_all_phis(ret["images"])
        if keep_images:
            ret["images"] = ret["images"].cpu().numpy()
        return ret
