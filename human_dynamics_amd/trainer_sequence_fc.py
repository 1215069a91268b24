"""The sequence trainer on precomputed phis (src/trainer_sequence_fc.py: HMRSequenceTrainer) for device tensors: one training step is
composed in Python from the autograd functions of the package -- models.az_fc2_groupnorm_train, fc2_res_train, batch_pred_omega_train,
trainer_losses.compute_losses_*, ops.mean_squared_error -- and applied by optim.TFAdam (hmmr_adam_step), the reference's
tf.train.AdamOptimizer.

Wiring (build_model :551-633).  movie_strip = az_fc2_groupnorm(phi); the regressors run from the tiled mean_param (the IEF bank's
`mean_theta`, trainable as in the reference) with use_delta_from_pred = True; compute_losses_batched on the present container (without
the shape prior, which compute_losses_prior owns), compute_losses_deltas with the `_dt*` suffixes when predict_delta is set.  With
do_hallucinate: pred_movie_strip = fc2_res(phi), the regressors on it (config.use_delta_from_pred), compute_losses_deltas with the
`_hal*` suffixes (the present one alone unless do_hallucinate_preds), and e_hallucinate = mean_squared_error(movie_strip,
pred_movie_strip), which reaches both the temporal encoder and the hallucinator.  compute_losses_prior runs over the concatenated Rs
and shapes of ALL containers, in the reference's order (hallucinated, present, deltas); tf_smpl.autograd.smpl_apply supplies the Rs.

Optimisers (setup_optimizers :744-766).  e_loss / d_loss are the sums of loss_weights[key] x loss over the keys that start with e / d;
e_opt is a TFAdam(e_lr) over the temporal blocks, the hallucinator (with do_hallucinate), the regressors and mean_param; d_opt a
TFAdam(d_lr) over the discriminator's bank when d_lw_pose > 0.  e_pose does not reach the discriminator and d_pose does not reach the
encoder (trainer_losses._PosePrior), as the two var_lists have it.

Update order.  TensorFlow leaves the order of the two apply ops of one session.run undefined.  This trainer's rule: BOTH gradients
come from ONE forward on the parameters as they were before the step; then both updates are applied (encoder first; the two touch
disjoint tensors, so their order changes nothing).  `iteration` is the reference's global_step: it advances once per minimize, so by
2 per step with the discriminator on.

Not built: summaries and visualisation, the tfrecord and mocap loaders (ground truth and real poses are arguments of train_step), a
fused C step, use_hmr_only, image input (precomputed_phi=False) and a trainable ResNet (freeze_phi=False): the last three are refused."""
from __future__ import annotations

import torch

from . import models, ops
from . import trainer_losses as TL
from .optim import TFAdam
from .tf_smpl.autograd import smpl_apply


def loss_weights(config):
    """the reference's loss_weights table (:280-310)"""
    g = lambda k, d: float(getattr(config, k, d))
    kp, joints, smpl = g("e_lw_kp", 60), g("e_lw_joints", 60), g("e_lw_smpl", 60)
    w = {"d_pose": g("d_lw_pose", 1), "e_const": g("e_lw_const", 1), "e_joints": joints, "e_kp": kp, "e_pose": g("e_lw_pose", 1),
         "e_shape": g("e_lw_shape", 1), "e_smpl": smpl, "e_hallucinate": g("e_lw_hallucinate", 1)}
    for suffix in ("_static", "_dt_future", "_dt_past", "_hal", "_hal_future", "_hal_past"):
        w.update({"e_kp" + suffix: kp, "e_joints" + suffix: joints, "e_smpl" + suffix: smpl})
    return w


def loss_keys(predict_delta=True, do_hallucinate=False, do_hallucinate_preds=False):
    """the keys of the reference's self.losses for a configuration (:236-277)"""
    keys = ["d_pose", "e_const", "e_joints", "e_kp", "e_pose", "e_shape", "e_smpl"]
    three = lambda s: ["e_joints" + s, "e_kp" + s, "e_smpl" + s]
    if predict_delta:
        keys += three("_dt_future") + three("_dt_past")
    if do_hallucinate:
        keys += ["e_hallucinate"] + three("_hal")
        if do_hallucinate_preds:
            keys += three("_hal_future") + three("_hal_past")
    return keys


class HMRSequenceTrainer(object):
    """config: duck-typed flags (batch_size, sequence_length or T, num_conv_layers, delta_t_values, predict_delta, do_hallucinate,
    do_hallucinate_preds, use_3d_label, use_delta_from_pred, e_lr, d_lr, e_lw_*, d_lw_pose, num_kps); engine: an HmmrEngine whose
    checkpoint holds the temporal blocks, the regressors with mean_param, D_pose/* and, with do_hallucinate, fc2_res/*."""

    def __init__(self, config, engine, generator=None):
        g = lambda k, d: getattr(config, k, d)
        if g("use_hmr_only", False):
            raise NotImplementedError("HMRSequenceTrainer: use_hmr_only (the static HMR branch) is not built")
        if not g("precomputed_phi", True):
            raise NotImplementedError("HMRSequenceTrainer: precomputed_phi=False (images through the ResNet) is not built: pass phis")
        if not g("freeze_phi", True):
            raise NotImplementedError("HMRSequenceTrainer: freeze_phi=False (a trainable ResNet) is not built")
        self.config, self.engine, self.generator = config, engine, generator
        self.batch_size = int(config.batch_size)
        self.sequence_length = int(g("sequence_length", g("T", 20)))
        self.num_conv_layers = int(g("num_conv_layers", engine.num_conv_layers))
        self.predict_delta = bool(g("predict_delta", True))
        self.do_hallucinate = bool(g("do_hallucinate", False))
        self.do_hallucinate_preds = bool(g("do_hallucinate_preds", False))
        self.use_3d_label = bool(g("use_3d_label", True))
        self.use_delta_from_pred = bool(g("use_delta_from_pred", True))
        self.delta_t_values = [int(d) for d in g("delta_t_values", engine.delta_keys)]
        self.e_lr, self.d_lr = float(g("e_lr", 1e-5)), float(g("d_lr", 1e-4))
        self.loss_weights = loss_weights(config)
        self.use_disc_pose = self.loss_weights["d_pose"] > 0.
        self.keys = loss_keys(self.predict_delta, self.do_hallucinate, self.do_hallucinate_preds)
        movie, ief = engine.movie_bank(), engine.ief_bank()
        self.mean_param = ief.mean_theta
        self.E_var = movie.temporal_tensors() + (engine._hal_bank().hallucinator_tensors() if self.do_hallucinate else []) + ief.tensors() + [self.mean_param]
        self.D_var = engine.disc_pose_bank().tensors()
        for t in self.E_var + (self.D_var if self.use_disc_pose else []):
            t.requires_grad_(True)
        self.e_opt = TFAdam(engine, self.E_var, self.e_lr)
        self.d_opt = TFAdam(engine, self.D_var, self.d_lr) if self.use_disc_pose else None
        self.iteration = 0
        self.last_keep = None

    # -- the forward: every loss of the reference's dictionary, e_loss and d_loss ---------------------------------------------------
    def _regress(self, strips, use_delta_from_pred, keep):
        B, T = self.batch_size, self.sequence_length
        return models.batch_pred_omega_train(strips, B, True, 85, self.mean_param.reshape(1, 85), T, "single_view_ief", self.engine,
                                             predict_delta_keys=[k for k in self.engine.reg_keys if k != 0], use_delta_from_pred=use_delta_from_pred,
                                             use_optcam=self.engine.use_optcam, keep=keep, generator=self.generator, return_keep=True)

    def compute_losses(self, phis, gt, poses_real, has_gt3d_smpl=None, has_gt3d_joints=None, keep=None):
        """-> ({key: device scalar} over loss_keys, e_loss, d_loss); `self.last_keep` holds the dropout masks drawn (or given): the
        present regressors' and, with do_hallucinate, the hallucinated ones' -- pass it back as `keep` to replay the step"""
        eng, B, T = self.engine, self.batch_size, self.sequence_length
        phis = phis.to(eng.device, torch.float32) if isinstance(phis, torch.Tensor) else eng.to_device(phis)
        phis = phis.reshape(B, T, 2048)
        ones = torch.ones(B, dtype=torch.float32, device=eng.device)
        has_smpl = ones if has_gt3d_smpl is None else eng.to_device(has_gt3d_smpl).reshape(B)
        has_joints = ones if has_gt3d_joints is None else eng.to_device(has_gt3d_joints).reshape(B)
        keep = (None, None) if keep is None else tuple(keep)
        kw = dict(has_gt3d_smpl=has_smpl, has_gt3d_joints=has_joints, use_3d_label=self.use_3d_label, loss_weights=self.loss_weights)
        zero = torch.zeros((), dtype=torch.float32, device=eng.device)
        losses = {k: zero for k in self.keys}
        containers, e_loss = [], zero

        movie_strip = models.az_fc2_groupnorm_train(True, phis, self.num_conv_layers, eng)
        omega_pred, deltas_pred, keep_pred = self._regress(movie_strip, True, keep[0])
        keep_hal = None
        if self.do_hallucinate:
            pred_movie_strip = models.fc2_res_train(phis, eng)
            omega_hal, deltas_hal, keep_hal = self._regress(pred_movie_strip, self.use_delta_from_pred, keep[1])
            hal = {0: omega_hal}
            if self.do_hallucinate_preds:
                hal.update({dt: deltas_hal[dt] for dt in self.delta_t_values})
            out = TL.compute_losses_deltas(eng, hal, gt, "_hal_future", "_hal_past", "_hal", **kw)
            losses.update({k: v for k, v in out.items() if k in losses})
            e_loss = e_loss + out["total"]
            containers += list(hal.values())
        self.last_keep = (keep_pred, keep_hal)

        out = TL.compute_losses_batched(eng, omega_pred, gt, with_shape_prior=False, **kw)
        losses.update({k: v for k, v in out.items() if k in losses})
        e_loss = e_loss + out["total"]
        containers.append(omega_pred)
        if self.do_hallucinate:
            losses["e_hallucinate"] = ops.mean_squared_error(movie_strip, pred_movie_strip, engine=eng)
            e_loss = e_loss + self.loss_weights["e_hallucinate"] * losses["e_hallucinate"]
        if self.predict_delta:
            dts = {dt: deltas_pred[dt] for dt in self.delta_t_values}
            out = TL.compute_losses_deltas(eng, dts, gt, "_dt_future", "_dt_past", "_dt", **kw)
            losses.update({k: v for k, v in out.items() if k in losses})
            e_loss = e_loss + out["total"]
            containers += list(dts.values())

        rs = [smpl_apply(eng, om[..., 3:75], om[..., 75:85])[3] for om in containers]
        prior = TL.compute_losses_prior(eng, poses_real, rs, [om[..., 75:85] for om in containers], bank_tensors=self.D_var)
        losses.update(prior)
        e_loss = e_loss + self.loss_weights["e_pose"] * prior["e_pose"] + self.loss_weights["e_shape"] * prior["e_shape"]
        d_loss = self.loss_weights["d_pose"] * prior["d_pose"]
        return losses, e_loss, d_loss

    # -- one step -----------------------------------------------------------------------------------------------------------------
    def backward(self, e_loss, d_loss):
        """both gradients from the one forward: e_loss reaches E_var only and d_loss D_var only, so one backward pass of their sum
        leaves exactly d e_loss / d E_var and d d_loss / d D_var on the tensors' .grad"""
        self.e_opt.zero_grad()
        if self.d_opt is not None:
            self.d_opt.zero_grad()
        (e_loss + d_loss if self.d_opt is not None else e_loss).backward()

    def train_step(self, phis, gt, poses_real, has_gt3d_smpl=None, has_gt3d_joints=None, keep=None):
        """phis [B,T,2048], gt an omega.OmegasGt, poses_real [n,216] (or [n,24,3,3]) mocap rotations -> {the reference's loss keys,
        e_loss, d_loss, iteration}: device scalars of the forward BEFORE the update.  This function adds no synchronisation."""
        losses, e_loss, d_loss = self.compute_losses(phis, gt, poses_real, has_gt3d_smpl, has_gt3d_joints, keep)
        self.backward(e_loss, d_loss)
        self.e_opt.step()
        self.iteration += 1
        if self.d_opt is not None:
            self.d_opt.step()
            self.iteration += 1
        out = {k: v.detach() for k, v in losses.items()}
        out.update(e_loss=e_loss.detach(), d_loss=d_loss.detach(), iteration=torch.full((), self.iteration, dtype=torch.int64, device=self.engine.device))
        return out

    def train(self, batches):
        """a loop over an iterable of dicts (phis, gt, poses_real and optionally has_gt3d_smpl, has_gt3d_joints, keep) -> the list of
        train_step's results"""
        return [self.train_step(**b) for b in batches]
