"""Trainer loss step timing (recorded once, not gated): hmmr_omega_loss_grad -- omega [B T, 85] -> losses, d_omega in one C call --
beside the route a user has without it IN THE SAME RUN: the same losses as torch ops on smpl_apply's outputs plus .backward()
(hmmr_smpl_fwd and hmmr_smpl_bwd under torch.autograd, the losses and their gradients as eager torch kernels).  Also the loss stage
alone (hmmr_seq_losses, forward and cotangents) beside its torch-op equivalent (forward + autograd.grad on given predictions).
B = 8 x T = 20 (the trainer's default) and m = 256 rows (B = 16 x T = 16), the 6890-vertex model, device in, device out; every
figure is the median of 9 samples of 10 back-to-back calls between two device events, after warm-up.
    python tools/loss_step_bench.py"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from human_dynamics_amd import _lib as L, assets
from human_dynamics_amd.engine import HmmrEngine
from human_dynamics_amd.tf_smpl.autograd import smpl_apply

CALLS, SAMPLES, WARMUP = 10, 9, 5
FLAGS = L.LOSS_KP | L.LOSS_JOINTS | L.LOSS_SMPL | L.LOSS_CONST | L.LOSS_SHAPE_PRIOR
WEIGHTS = (60.0, 60.0, 60.0, 1.0, 1.0)


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(SAMPLES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / CALLS * 1e3)
    return statistics.median(out), min(out), max(out)


def torch_losses(kps, joints, rs, beta, gt, B, T, w=WEIGHTS):
    """the present container's losses (compute_losses_batched + the shape prior) as eager torch ops -> total"""
    vis = gt["kps"][:, :, 2:3]
    e_kp = (vis * (gt["kps"][:, :, :2] - kps).abs()).sum() / (2 * (vis != 0).sum()).clamp(min=1)
    align = lambda j: j - ((j[:, 3] + j[:, 2]) / 2.).unsqueeze(1)

    def mse(a, b, has):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        return 0.5 * (has[:, None] * (a - b) ** 2).sum() / ((has != 0).sum() * a.shape[1]).clamp(min=1)
    hj, hs = gt["has_gt3d_joints"].repeat_interleave(T), gt["has_gt3d_smpl"].repeat_interleave(T)
    e_joints = mse(align(gt["joints"]), align(joints[:, :14]), hj)
    e_smpl = mse(gt["rs"], rs, hs) + mse(gt["shapes"].repeat_interleave(T, 0), beta, hs)
    b3 = beta.reshape(B, T, 10)
    e_const = 0.5 * ((b3[:, :-1] - b3[:, 1:]) ** 2).mean()
    e_shape = (beta ** 2).mean()
    return w[0] * e_kp + w[1] * e_joints + w[2] * e_smpl + w[3] * e_const + w[4] * e_shape


def main():
    if not torch.cuda.is_available():
        raise SystemExit("loss_step_bench needs a HIP device")
    eng = HmmrEngine(None, assets.make_synthetic_smpl(2), device="cuda:0")
    V, K = eng.num_verts, eng.num_kps
    print("loss_step_bench: %d vertices, %d keypoints, %s" % (V, K, torch.cuda.get_device_name(0)))
    report = lambda name, r: print("loss_step_bench: %-58s %8.1f us per call (median of %d; min %.1f, max %.1f)" % ((name,) + (r[0], SAMPLES) + r[1:]))
    for B, T in ((8, 20), (16, 16)):
        N = B * T
        rng = np.random.default_rng(N)
        dev = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda()
        omega = torch.cat([1.0 + 0.1 * dev(N, 1), 0.1 * dev(N, 2), 0.4 * dev(N, 72), dev(N, 10)], 1).contiguous()
        gt = {"kps": torch.cat([dev(N, K, 2), (dev(N, K, 1) > -0.5).float()], 2).contiguous(), "joints": 0.3 * dev(N, 14, 3),
              "rs": eng.smpl(0.4 * dev(N, 72), dev(N, 10), None)[3], "shapes": dev(B, 10), "has_gt3d_smpl": (dev(B) > -0.5).float(),
              "has_gt3d_joints": (dev(B) > -0.5).float()}
        print("loss_step_bench: B %d x T %d = %d rows" % (B, T, N))
        fused = median_us(lambda: eng.omega_loss_grad(omega, B, T, FLAGS, gt, weights=WEIGHTS))
        report("hmmr_omega_loss_grad (one C call)", fused)

        def eager():
            om = omega.detach().requires_grad_(True)
            verts, joints, kps, rs = smpl_apply(eng, om[:, 3:75], om[:, 75:85], om[:, 0:3])
            torch_losses(kps, joints, rs, om[:, 75:85], gt, B, T).backward()
            return om.grad
        plain = median_us(eager)
        report("smpl_apply + torch-op losses + .backward()", plain)
        a, b = eng.omega_loss_grad(omega, B, T, FLAGS, gt, weights=WEIGHTS)[1], eager()
        print("loss_step_bench: the two routes' d_omega differ by at most %.3e (largest |d_omega| %.3e)" % (float((a - b).abs().max()), float(a.abs().max())))
        verts, joints, kps, rs = eng.smpl(omega[:, 3:75], omega[:, 75:85], omega[:, 0:3])
        beta = omega[:, 75:85]
        stage = median_us(lambda: eng.seq_losses(B, T, FLAGS, gt, kps_pred=kps, joints_pred=joints, rs_pred=rs, beta_pred=beta, weights=WEIGHTS))
        report("hmmr_seq_losses alone (losses + four cotangents)", stage)

        def eager_stage():
            p = [x.detach().requires_grad_(True) for x in (kps, joints, rs, beta.contiguous())]
            return torch.autograd.grad(torch_losses(p[0], p[1], p[2], p[3], gt, B, T), p)
        plain_stage = median_us(eager_stage)
        report("torch-op losses + autograd.grad alone", plain_stage)
        print("loss_step_bench: one call / torch route = %.2f (whole step), %.2f (loss stage alone)" % (fused[0] / plain[0], stage[0] / plain_stage[0]))


if __name__ == "__main__":
    main()
