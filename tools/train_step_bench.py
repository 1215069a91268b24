"""One training step of the sequence trainer at the reference's default (B, T) = (8, 20) on the default engine's weights (recorded
once, not gated): HMRSequenceTrainer.train_step split into its forward + backward (compute_losses, backward) and the two optimiser
calls (e_opt over the encoder set, d_opt over the discriminator).  Every figure is the median of 9 samples between two device events
after warm-up; the parts are timed in runs of their own, so they need not add up to the whole step exactly.
    python tools/train_step_bench.py"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from human_dynamics_amd import assets, disc_bank
from human_dynamics_amd.engine import HmmrEngine
from human_dynamics_amd.omega import OmegasGt
from human_dynamics_amd.trainer_sequence_fc import HMRSequenceTrainer

B, T, K, SAMPLES, WARMUP = 8, 20, 25, 9, 2


class Config(object):
    batch_size, sequence_length, num_conv_layers, delta_t_values, num_kps = B, T, 3, [-5, 5], K
    do_hallucinate, d_lw_pose = True, 1.0


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench needs a HIP device")
    rng = np.random.default_rng(1)
    w = assets.make_synthetic_weights(0, with_hallucinator=True)
    w = {k: v for k, v in w.items() if not k.startswith("resnet_v2_50")}
    for name, shape in sorted(disc_bank.checkpoint_shapes().items()):
        fan_in = int(np.prod(shape[:-1])) if name.endswith("weights") else 100
        w[name] = (rng.normal(size=shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    eng = HmmrEngine(w, assets.make_synthetic_smpl(2), device="cuda:0")
    f = lambda x: np.ascontiguousarray(x, np.float32)
    vis = (rng.random((B, T, K)) < 0.7).astype(np.float64)
    vis[:, :, :3] = 1.0
    gt = OmegasGt(Config(), f(0.3 * rng.standard_normal((B, T, 72))), f(rng.standard_normal((B, 10))), f(0.5 * rng.standard_normal((B, T, 14, 3))),
                  f(np.concatenate([0.5 * rng.standard_normal((B, T, K, 2)), vis[..., None]], -1)), batch_size=B, engine=eng)
    args = dict(phis=torch.from_numpy(f(rng.standard_normal((B, T, 2048)))).cuda(), gt=gt,
                poses_real=torch.from_numpy(f(0.5 * rng.standard_normal((4 * B * T, 216)))).cuda())
    tr = HMRSequenceTrainer(Config(), eng)
    n_e, n_d = sum(t.numel() for t in tr.E_var), sum(t.numel() for t in tr.D_var)
    print("train_step_bench: %s; (B, T) = (%d, %d), do_hallucinate and the discriminator on; e_opt over %.1f M values, d_opt over %.2f M"
          % (torch.cuda.get_device_name(0), B, T, n_e / 1e6, n_d / 1e6))

    def fwd_bwd():
        losses, e_loss, d_loss = tr.compute_losses(**args)
        tr.backward(e_loss, d_loss)
    line = lambda name, r: print("train_step_bench: %-44s %8.3f ms (median of %d; min %.3f, max %.3f)" % ((name, r[0], SAMPLES) + r[1:]))
    line("train_step, whole", median_ms(lambda: tr.train_step(**args)))
    line("forward + backward (compute_losses, backward)", median_ms(fwd_bwd))
    line("e_opt.step (hmmr_adam_step, encoder set)", median_ms(tr.e_opt.step))
    line("d_opt.step (hmmr_adam_step, discriminator)", median_ms(tr.d_opt.step))
    print("train_step_bench: the four figures are not taken on one parameter state: the optimiser calls are timed by repeating step() on the last "
          "gradients, which moves the banks and advances the beta powers between the measurements (the time of a step does not depend on the values)")
    print("train_step_bench: the forward + backward includes one host synchronisation per loss container (trainer_losses._OmegaLoss reads its "
          "upstream vector); unmeasured: any counter, any shape but this one")


if __name__ == "__main__":
    main()
