"""IEF backward timing (recorded once, not gated): hmmr_ief_fwd_train and hmmr_ief_bwd (every output) at m = 160 and 256 rows with R = 3
regressors and three stages, a random 0.5 keep mask, beside the route a user has without them IN THE SAME RUN: the same function as eager
torch ops on the bank's fp32 tensors (F.linear, relu, the mask) plus torch.autograd.  Also hmmr_ief_fwd on the default engine -- the
inference path, to be compared with a run of the parent commit's library (HMMR_LIB_PATH=<its libhmmr_hip.so> python tools/ief_grad_bench.py
--inference-only).  Device in, device out; every figure is the median of 9 samples of 10 back-to-back calls between two device events,
after warm-up.  --trace N: N backward calls at m = 160 and nothing else, for a kernel trace.
    python tools/ief_grad_bench.py"""
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from human_dynamics_amd import assets
from human_dynamics_amd.engine import HmmrEngine

CALLS, SAMPLES, WARMUP = 10, 9, 5
PEAK_TF = 157.3           # fp32 MFMA, MI355X


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


def flops(m, nds, stages):
    """(forward, data gradients, weight gradients) in FLOP: 2 x multiply-adds of the unpadded products"""
    third = sum(2.0 * m * (2048 * 1024 + stages * 1024 * (nd + 1024 + nd)) for nd in nds)
    return third, third, third


def torch_forward(bank, strips, start, keep, scale, stages=3):
    """the function of include/hmmr_hip.h, "IEF backward", as eager torch ops on the bank's tensors (72-wide deltas from the prediction)"""
    def regress(p, theta, kp, nd):
        pre = F.linear(strips, p["fc1_phi"], p["b1"])
        for s in range(stages):
            h1 = torch.relu(pre + F.linear(theta, p["fc1_theta"][:, :nd])) * kp[s, 0] * scale
            h2 = torch.relu(F.linear(h1, p["fc2"], p["b2"])) * kp[s, 1] * scale
            theta = theta + F.linear(h2, p["fc3"][:nd], p["b3"][:nd])
        return theta
    om0 = regress(bank.params[0], start, keep[0], 85)
    out = [om0]
    for r in range(1, bank.num_regressors):
        d = regress(bank.params[r], om0[:, 3:75], keep[r], 72)
        out.append(torch.cat([torch.ones_like(d[:, :1]), torch.zeros_like(d[:, :2]), d, om0[:, 75:]], 1))
    return torch.stack(out)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ief_grad_bench needs a HIP device")
    w = {k: v for k, v in assets.make_synthetic_weights(0).items() if k.startswith("single_view_ief") or k == "mean_param"}
    eng = HmmrEngine(w, None, device="cuda:0")
    print("ief_grad_bench: %s, library %s" % (torch.cuda.get_device_name(0), eng.lib._name))
    report = lambda name, r: print("ief_grad_bench: %-62s %8.1f us per call (median of %d; min %.1f, max %.1f)" % ((name,) + (r[0], SAMPLES) + r[1:]))
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    dev = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda()
    if "--inference-only" in sys.argv:
        for m in (160, 256):
            strips = dev(m, 2048)
            report("hmmr_ief_fwd, default engine (f16x3), m = %d" % m, median_us(lambda: eng.ief(strips)))
        return
    bank = eng.ief_bank()
    R, S = bank.num_regressors, bank.iw.num_stages
    if "--trace" in sys.argv:
        m, n = 160, int(sys.argv[sys.argv.index("--trace") + 1])
        strips, d_om = dev(m, 2048), dev(R, m, 85)
        keep = (torch.rand((R, S, 2, m, 1024), device="cuda") < 0.5).to(torch.uint8)
        for _ in range(n):
            eng.ief_backward(strips, d_om, keep=keep, keep_prob=0.5, want_start=True)
        torch.cuda.synchronize()
        return
    for m in (160, 256):
        strips, d_om = dev(m, 2048), dev(R, m, 85)
        start = bank.mean_theta.reshape(1, 85).expand(m, 85).contiguous()
        keep = (torch.rand((R, S, 2, m, 1024), device="cuda") < 0.5).to(torch.uint8)
        keepf = keep.float()
        print("ief_grad_bench: m = %d rows, R = %d, %d stages" % (m, R, S))
        fwd = median_us(lambda: eng.ief_train(strips, keep=keep, keep_prob=0.5))
        report("hmmr_ief_fwd_train", fwd)
        bwd = median_us(lambda: eng.ief_backward(strips, d_om, keep=keep, keep_prob=0.5, want_start=True))
        report("hmmr_ief_bwd, every output (recomputes the forward)", bwd)
        only = median_us(lambda: eng.ief_backward(strips, d_om, keep=keep, keep_prob=0.5, want_start=False, want_weights=False))
        report("hmmr_ief_bwd, d_strips alone", only)
        tensors = bank.tensors()

        def eager():
            for t in tensors:
                t.grad = None
            x = strips.detach().requires_grad_(True)
            torch_forward(bank, x, start, keepf, 2.0, S).backward(d_om)
            return x.grad
        try:
            for t in tensors:
                t.requires_grad_()
            plain = median_us(eager)
            report("torch ops (F.linear) forward + .backward()", plain)
            a, b = eng.ief_backward(strips, d_om, keep=keep, keep_prob=0.5, want_weights=False)[0], eager()
            print("ief_grad_bench: the two routes' d_strips differ by at most %.3e (largest |d_strips| %.3e; a pre-activation that rounds to the other side of zero "
                  "in one of them shows as a difference of 1e-3 .. 1e-2)" % (float((a - b).abs().max()), float(a.abs().max())))
        finally:
            for t in tensors:
                t.grad = None
                t.requires_grad_(False)
        f, dg, wg = flops(m, bank.nd, S)
        print("ief_grad_bench: %.2f GFLOP forward, %.2f data gradients, %.2f weight gradients; hmmr_ief_fwd_train %.1f TF, hmmr_ief_bwd %.1f TF = %.1f %% of the "
              "%.1f TF fp32 MFMA peak; one call / torch route = %.2f" % (f / 1e9, dg / 1e9, wg / 1e9, f / fwd[0] / 1e6, (f + dg + wg) / bwd[0] / 1e6,
                                                                         100 * (f + dg + wg) / bwd[0] / 1e6 / PEAK_TF, PEAK_TF, (fwd[0] + bwd[0]) / plain[0]))
        report("hmmr_ief_fwd, default engine (f16x3)", median_us(lambda: eng.ief(strips)))


if __name__ == "__main__":
    main()
