"""Mirror of src/discriminators.py for device tensors: PoseDiscriminator on the engine's trainable bank (disc_bank.PoseDiscBank,
csrc/disc_pose.hip) under torch.autograd.

Three differences from the reference, on purpose (include/hmmr_hip.h, "Pose discriminator"):
 - `weight_decay` is kept in the signature and has no effect.  The reference hands it to slim.l2_regularizer, which fills the
   REGULARIZATION_LOSSES collection; its trainer's gather_losses never reads that collection, so d_loss carries no decay term.  None
   is built here.
 - the output is always [N, 24]: the reference's tf.squeeze drops the batch axis of a single row and its concat then fails.
 - the variables are the twelve tensors of the packed bank, not 58 TensorFlow variables; PoseDiscBank.to_checkpoint converts."""
from __future__ import annotations

from . import ops
from .disc_autograd import disc_pose_apply


class PoseDiscriminator(object):
    def __init__(self, weight_decay=None, engine=None):
        self.wd = weight_decay          # (no effect: see the module's text)
        self.engine = engine
        self.reuse = False

    def _eng(self):
        return ops._eng(self.engine)

    def get_output(self, poses, poses_b=None):
        """poses [N,23,1,9] (or [N,207]; or all 24 rotations [N,24,3,3] / [N,216], whose global rotation is dropped in place) ->
        predictions [N,24]: one per joint, then the one over all joints.  poses_b: a second segment of rows behind the first, so
        real and fake rows need no concatenation."""
        self.reuse = True
        return disc_pose_apply(self._eng(), poses, poses_b)

    def get_vars(self):
        """the twelve tensors of the bank, in the order of disc_bank.NAMES"""
        return self._eng().disc_pose_bank().tensors()
