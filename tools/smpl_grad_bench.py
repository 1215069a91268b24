"""SMPL backward timing (recorded once, not gated): hmmr_smpl_bwd with all four cotangents and with joints, kps and Rs only (the
trainer's case) beside hmmr_smpl_fwd in the same run.  m = 256 instances of the 6890-vertex model, device in, device out; every
figure is the median of 9 samples of 10 back-to-back calls between two device events, after warm-up.
    python tools/smpl_grad_bench.py [--forward-only]        (--forward-only: no new symbol is touched -- what runs at an older commit)"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from human_dynamics_amd import assets
from human_dynamics_amd.engine import HmmrEngine

M, CALLS, SAMPLES, WARMUP = 256, 10, 9, 5


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("smpl_grad_bench needs a HIP device")
    eng = HmmrEngine(None, assets.make_synthetic_smpl(2), device="cuda:0")
    V, K = eng.num_verts, eng.num_kps
    rng = np.random.default_rng(0)
    dev = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda()
    theta, beta, cams = dev(M, 72) * 0.5, dev(M, 10), dev(M, 3)
    print("smpl_grad_bench: m %d, %d vertices, %d keypoints, %s" % (M, V, K, torch.cuda.get_device_name(0)))
    report = lambda name, r: print("smpl_grad_bench: %-46s %8.1f us per call (median of %d; min %.1f, max %.1f)" % ((name,) + (r[0], SAMPLES) + r[1:]))
    fwd = median_us(lambda: eng.smpl(theta, beta, cams))
    report("hmmr_smpl_fwd (default blend form)", fwd)
    if "--forward-only" in sys.argv:
        return
    joints = eng.smpl(theta, beta, cams)[1]
    dv, dj, dk, dr = dev(M, V, 3), dev(M, K, 3), dev(M, K, 2), dev(M, 24, 3, 3)
    full = median_us(lambda: eng.smpl_backward(theta, beta, cams, joints, d_verts=dv, d_joints=dj, d_kps=dk, d_rs=dr))
    report("hmmr_smpl_bwd, all four cotangents", full)
    train = median_us(lambda: eng.smpl_backward(theta, beta, cams, joints, d_joints=dj, d_kps=dk, d_rs=dr))
    report("hmmr_smpl_bwd, joints + kps + Rs (no d_verts)", train)
    print("smpl_grad_bench: backward / forward = %.2f (all four), %.2f (joints + kps + Rs)" % (full[0] / fwd[0], train[0] / fwd[0]))


if __name__ == "__main__":
    main()
