"""Pose discriminator timing (recorded once, not gated): hmmr_pose_prior (losses, d_rs_fake and the twelve gradients), hmmr_disc_pose_fwd,
the separate-calls route (hmmr_disc_pose_fwd + two hmmr_disc_pose_bwd calls with the step's two cotangents) at n_real = n_fake = 160
and 640, beside the route a user has without them IN THE SAME RUN: the same step as eager torch ops on the bank's fp32 tensors plus two
.backward() calls.  Device in, device out; every figure is the median of 9 samples of 10 back-to-back calls between two device events,
after warm-up.  The launch count of a call is MEASURED: the device kernels torch.profiler records for one call after warm-up (for the
separate-calls route that includes the few torch kernels that build the cotangents); the count read off csrc/disc_pose.hip (a split-K
hmmr_conv_gemm is two launches) is printed beside it.  Where the profiler records no device kernel the line says so and shows the
code's count alone.
    python tools/disc_bench.py"""
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from human_dynamics_amd import disc_bank
from human_dynamics_amd.engine import HmmrEngine

CALLS, SAMPLES, WARMUP = 10, 9, 5
PEAK_TF = 157.3           # fp32 MFMA, MI355X
CODE_LAUNCHES = {"fwd": 7, "bwd_all": 18, "prior": 23, "separate": 7 + (7 + 4) + (7 + 11)}      # read off csrc/disc_pose.hip


def count_kernels(fn):
    """device kernels of ONE call of fn, by torch.profiler (memory copies and memsets are not counted); None if it records none"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset"))]
    except Exception as e:          # (a build of torch without a device tracer)
        print("disc_bench: torch.profiler failed (%s): launch counts not measured" % e)
        return None
    return len(names) or None


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


def weights(seed=3):
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in sorted(disc_bank.checkpoint_shapes().items()):
        fan_in = int(np.prod(shape[:-1])) if name.endswith("weights") else 100
        w[name] = (rng.normal(size=shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    return w


def torch_out(p, x):
    """the function of include/hmmr_hip.h, "Pose discriminator", as eager torch ops on the bank's tensors; x [n,23,9]"""
    n = x.shape[0]
    h1 = torch.relu(F.linear(x, p["conv1"][:, :9], p["bc1"]))
    h2 = torch.relu(F.linear(h1, p["conv2"], p["bc2"]))
    heads = (h2 * p["heads"][:23]).sum(2) + p["bj"][:23]
    h3 = torch.relu(F.linear(h2.reshape(n, 736), p["fc1"][:, :736], p["b1"]))
    h4 = torch.relu(F.linear(h3, p["fc2"], p["b2"]))
    return torch.cat([heads, F.linear(h4, p["fc_out"][:1], p["bo"][:1])], 1)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("disc_bench needs a HIP device")
    eng = HmmrEngine(weights(), None, device="cuda:0")
    bank = eng.disc_pose_bank()
    print("disc_bench: %s, library %s" % (torch.cuda.get_device_name(0), eng.lib._name))

    def report(name, r, k, fn):
        measured = count_kernels(fn)
        n_l = measured or CODE_LAUNCHES[k]
        print("disc_bench: %-66s %8.1f us per call (median of %d; min %.1f, max %.1f; %s, %d read off the code; %.1f us each)"
              % ((name,) + (r[0], SAMPLES) + r[1:] + ("%d launches measured" % measured if measured else "launches NOT measured", CODE_LAUNCHES[k], r[0] / n_l)))
    rng = np.random.default_rng(5)

    def rots(n):
        """[n,24,3,3] rotations near the identity, orthonormalised"""
        a = np.eye(3) + 0.3 * rng.normal(size=(n, 24, 3, 3))
        return torch.from_numpy(np.linalg.qr(a)[0].astype(np.float32)).cuda()
    for n in (160, 640):
        real, fake = rots(n), rots(n)
        print("disc_bench: n_real = n_fake = %d rows" % n)
        f_prior = lambda: eng.pose_prior(real, fake)
        prior = median_us(f_prior)
        report("hmmr_pose_prior: losses, d_rs_fake, twelve gradients", prior, "prior", f_prior)
        f_fwd = lambda: eng.disc_pose(real, fake)
        fwd = median_us(f_fwd)
        report("hmmr_disc_pose_fwd", fwd, "fwd", f_fwd)
        cot = torch.randn(2 * n, 24, device="cuda")
        f_bwd = lambda: eng.disc_pose_backward(real, fake, cot)
        report("hmmr_disc_pose_bwd, every output (recomputes the forward)", median_us(f_bwd), "bwd_all", f_bwd)

        def separate():
            out = eng.disc_pose(real, fake)
            ce = torch.cat([torch.zeros_like(out[:n]), (2.0 / n) * (out[n:] - 1)])
            cd = torch.cat([(2.0 / n) * (out[:n] - 1), (2.0 / n) * out[n:]])
            d_b = eng.disc_pose_backward(real, fake, ce, want_poses_a=False, want_weights=False, full_b=True)[1]
            g = eng.disc_pose_backward(real, fake, cd, want_poses_a=False, want_poses_b=False)[2]
            return d_b, g
        sep = median_us(separate)
        report("separate calls: fwd + bwd (d_poses_b) + bwd (gradients), cotangents in torch", sep, "separate", separate)
        tensors = bank.tensors()

        def eager():
            for t in tensors:
                t.grad = None
            x = fake.detach().requires_grad_(True)
            out = torch_out(bank.params, torch.cat([real, x])[:, 1:].reshape(2 * n, 23, 9))
            e = ((out[n:] - 1) ** 2).sum(1).mean()
            d = ((out[:n] - 1) ** 2).sum(1).mean() + (out[n:] ** 2).sum(1).mean()
            gx, = torch.autograd.grad(e, x, retain_graph=True)
            d.backward()
            return gx
        try:
            for t in tensors:
                t.requires_grad_()
            plain = median_us(eager)
            print("disc_bench: %-66s %8.1f us per call (median of %d; min %.1f, max %.1f)" % (("torch ops (F.linear) forward + two backward passes", plain[0], SAMPLES) + plain[1:]))
            a, b = eng.pose_prior(real, fake)[1], eager()
            print("disc_bench: the two routes' d_rs_fake differ by at most %.3e (largest |d_rs_fake| %.3e)" % (float((a - b).abs().max()), float(a.abs().max())))
        finally:
            for t in tensors:
                t.grad = None
                t.requires_grad_(False)
        rows = 2 * n
        f = 2.0 * rows * (23 * (9 * 32 + 32 * 32 + 32) + 736 * 1024 + 1024 * 1024 + 1024)
        total = f + 2.0 * n * (736 * 1024 + 1024 * 1024) + 2 * f          # forward, the encoder's data gradient on the fake rows, the discriminator's data + weight gradients
        print("disc_bench: %.2f GFLOP per step of unpadded products; hmmr_pose_prior %.1f TF = %.1f %% of the %.1f TF fp32 MFMA peak; pose_prior / torch route = %.2f, "
              "pose_prior / separate calls = %.2f" % (total / 1e9, total / prior[0] / 1e6, 100 * total / prior[0] / 1e6 / PEAK_TF, PEAK_TF, prior[0] / plain[0],
                                                      prior[0] / sep[0]))


if __name__ == "__main__":
    main()
