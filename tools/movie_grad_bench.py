"""f_movie / hallucinator backward timing (recorded once, not gated): hmmr_temporal_bwd (every output, and d_phi alone), hmmr_hallucinator_bwd
and the fp32 forwards on the trainable bank at (b, t) = (8, 20) and (8, 32) -- 160 and 256 rows -- beside the route a user has without
them IN THE SAME RUN: the same functions as eager torch ops on the bank's fp32 tensors (F.group_norm, the three taps laid side by side in
front of one F.linear on the bank's own rows, relu) plus torch.autograd.  Also hmmr_temporal_fwd and hmmr_ief_fwd on the default engine --
the inference path, to be compared with a run of the parent commit's library in a process of its own
(HMMR_LIB_PATH=<its libhmmr_hip.so> python tools/movie_grad_bench.py --inference-only --tag "parent commit").  Device in, device out; every
figure is the median of 9 samples of 10 back-to-back calls between two device events, after warm-up.  --log PATH: the file the lines are
appended to (default profiles/movie_grad_bench.log).
    python tools/movie_grad_bench.py"""
import ctypes
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from human_dynamics_amd import _lib, assets

CALLS, SAMPLES, WARMUP = 10, 9, 5
PEAK_TF = 157.3           # fp32 MFMA, MI355X
SHAPES = ((8, 20), (8, 32))
C = 2048
_LOG = None


def say(text):
    line = "movie_grad_bench: " + text
    print(line, flush=True)
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(line + "\n")


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


def report(name, r, tag=""):
    say("%s%-66s %8.1f us per call (median of %d; min %.1f, max %.1f)" % (("[%s] " % tag) if tag else "", name, r[0], SAMPLES, r[1], r[2]))


def torch_temporal(bank, phi):
    """az_fc2_groupnorm as eager torch ops on the bank's tensors: the bank's conv rows [co][tap * 2048 + ci] are F.linear's weight for the
    three shifted copies of the input laid side by side"""
    def gn_relu(x, gamma, beta):
        return torch.relu(F.group_norm(x.transpose(1, 2), 32, gamma, beta, 1e-6).transpose(1, 2))

    def conv(h, w, bias):
        hp = F.pad(h, (0, 0, 1, 1))
        return F.linear(torch.cat([hp[:, :-2], hp[:, 1:-1], hp[:, 2:]], dim=2), w, bias)

    net = phi
    for p in bank.blocks:
        h = conv(gn_relu(net, p["gn1_gamma"], p["gn1_beta"]), p["conv1"], p["b1"])
        net = conv(gn_relu(h, p["gn2_gamma"], p["gn2_beta"]), p["conv2"], p["b2"]) + net
    return net


def torch_hal(bank, phi):
    p = bank.hal
    h = torch.relu(F.linear(phi, p["fc1"], p["b1"]))
    h = torch.relu(F.linear(h, p["fc2"], p["b2"]))
    return F.linear(h, p["fc3"], p["b3"]) + phi


def drop_missing_entry_points():
    """a library of an earlier commit lacks the entry points added since; the inference path calls none of them"""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in _lib.SIGNATURES if not hasattr(lib, n)]
    for n in missing:
        del _lib.SIGNATURES[n]
    return missing


def main():
    global _LOG
    if not torch.cuda.is_available():
        raise SystemExit("movie_grad_bench needs a HIP device")
    argv = sys.argv
    _LOG = argv[argv.index("--log") + 1] if "--log" in argv else "profiles/movie_grad_bench.log"
    tag = argv[argv.index("--tag") + 1] if "--tag" in argv else ""
    inference = "--inference-only" in argv
    missing = drop_missing_entry_points() if inference else []
    from human_dynamics_amd.engine import HmmrEngine
    w = {k: v for k, v in assets.make_synthetic_weights(0, with_hallucinator=True).items()
         if k.startswith(("AZ_FC_block", "fc2_res/", "single_view_ief")) or k == "mean_param"}
    eng = HmmrEngine(w, None, device="cuda:0")
    say("%s%s, library %s%s" % (("[%s] " % tag) if tag else "", torch.cuda.get_device_name(0), eng.lib._name,
                                (" (without %s)" % ", ".join(missing)) if missing else ""))
    rng = np.random.default_rng(5)
    dev = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda()
    if inference:
        for b, t in SHAPES:
            phi = dev(b, t, C)
            report("hmmr_temporal_fwd, default engine (f16x3), (b, t) = (%d, %d)" % (b, t), median_us(lambda: eng.temporal(phi)), tag)
            strips = dev(b * t, C)
            report("hmmr_ief_fwd, default engine (f16x3), m = %d" % (b * t), median_us(lambda: eng.ief(strips)), tag)
        return
    bank = eng.movie_bank()
    nblk = bank.num_blocks
    for b, t in SHAPES:
        m = b * t
        phi, cot = dev(b, t, C), dev(b, t, C)
        say("(b, t) = (%d, %d): %d rows, %d temporal blocks" % (b, t, m, nblk))
        fwd = median_us(lambda: eng.temporal_train(phi))
        report("hmmr_temporal_fwd on the fp32 bank", fwd)
        bwd = median_us(lambda: eng.temporal_backward(phi, cot))
        report("hmmr_temporal_bwd, every output (recomputes the forward)", bwd)
        only = median_us(lambda: eng.temporal_backward(phi, cot, want_weights=False))
        report("hmmr_temporal_bwd, d_phi alone", only)
        hf = median_us(lambda: eng.hallucinate_train(phi))
        report("hmmr_hallucinator_fwd on the fp32 bank", hf)
        hb = median_us(lambda: eng.hallucinate_backward(phi, cot))
        report("hmmr_hallucinator_bwd, every output (recomputes two layers)", hb)
        tensors = bank.tensors()

        def eager(fn):
            def run():
                for x in tensors:
                    x.grad = None
                x = phi.detach().requires_grad_(True)
                fn(bank, x).backward(cot)
                return x.grad
            return run
        try:
            for x in tensors:
                x.requires_grad_()
            pt = median_us(eager(torch_temporal))
            report("temporal encoder, torch ops forward + .backward()", pt)
            ph = median_us(eager(torch_hal))
            report("hallucinator, torch ops forward + .backward()", ph)
            for name, mine, theirs in (("temporal", eng.temporal_backward(phi, cot, want_weights=False)[0], eager(torch_temporal)()),
                                       ("hallucinator", eng.hallucinate_backward(phi, cot, want_weights=False)[0], eager(torch_hal)())):
                say("%s: the two routes' d_phi differ by at most %.3e (largest |d_phi| %.3e; a pre-activation that rounds to the other side of "
                    "zero in one of them shows as a larger difference)" % (name, float((mine - theirs).abs().max()), float(mine.abs().max())))
        finally:
            for x in tensors:
                x.grad = None
                x.requires_grad_(False)
        conv = 2.0 * m * 3 * C * C                      # one convolution's multiply-adds x 2
        tf_, td, tw = 2 * nblk * conv, 2 * nblk * conv, 2 * nblk * conv
        recomputed = tf_ - conv                         # the backward recomputes the forward without the last conv2
        say("temporal: %.2f GFLOP forward, %.2f data gradients, %.2f weight gradients; hmmr_temporal_fwd %.1f TF, hmmr_temporal_bwd (%.2f GFLOP "
            "with its recomputed forward) %.1f TF = %.1f %% of the %.1f TF fp32 MFMA peak; forward + backward / torch route = %.2f"
            % (tf_ / 1e9, td / 1e9, tw / 1e9, tf_ / fwd[0] / 1e6, (recomputed + td + tw) / 1e9, (recomputed + td + tw) / bwd[0] / 1e6,
               100 * (recomputed + td + tw) / bwd[0] / 1e6 / PEAK_TF, PEAK_TF, (fwd[0] + bwd[0]) / pt[0]))
        fc = 2.0 * m * C * C
        say("hallucinator: %.2f GFLOP forward, %.2f data gradients, %.2f weight gradients; hmmr_hallucinator_bwd (%.2f GFLOP with its two "
            "recomputed layers) %.1f TF = %.1f %% of the peak; forward + backward / torch route = %.2f"
            % (3 * fc / 1e9, 3 * fc / 1e9, 3 * fc / 1e9, 8 * fc / 1e9, 8 * fc / hb[0] / 1e6, 100 * 8 * fc / hb[0] / 1e6 / PEAK_TF, (hf[0] + hb[0]) / ph[0]))
        strips = dev(m, C)
        report("hmmr_temporal_fwd, default engine (f16x3)", median_us(lambda: eng.temporal(phi)))
        report("hmmr_ief_fwd, default engine (f16x3)", median_us(lambda: eng.ief(strips)))


if __name__ == "__main__":
    main()
