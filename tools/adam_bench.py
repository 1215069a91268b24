"""TF Adam timing (recorded once, not gated): one hmmr_adam_step over the default engine's encoder set -- three temporal blocks, the
hallucinator, three regressors and mean_param, about 94 M fp32 values -- beside torch.optim.Adam(foreach=True) on the same tensors IN
THE SAME RUN and beside the derived floor, 28 bytes per value at the measured float4-copy ceiling of 6.29 TB/s.  Every figure is the
median of 9 samples of 5 back-to-back steps between two device events, after warm-up.  It also prints how many bytes of the set take
the 4-byte path (a segment whose p, g, m or v is not 16-byte aligned).
    python tools/adam_bench.py"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from human_dynamics_amd import assets
from human_dynamics_amd.engine import HmmrEngine
from human_dynamics_amd.optim import TFAdam

CALLS, SAMPLES, WARMUP = 5, 9, 3
COPY_TBS = 6.29


def median_ms(fn):
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
        out.append(e0.elapsed_time(e1) / CALLS)
    return statistics.median(out), min(out), max(out)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench needs a HIP device")
    w = assets.make_synthetic_weights(0, with_hallucinator=True)
    w = {k: v for k, v in w.items() if not k.startswith("resnet_v2_50")}
    eng = HmmrEngine(w, None, device="cuda:0")
    movie, ief = eng.movie_bank(), eng.ief_bank()
    tensors = movie.tensors() + ief.tensors() + [ief.mean_theta]
    n = sum(t.numel() for t in tensors)
    print("adam_bench: %s; %d tensors, %d values (%.1f M), %.3f GB moved per step at 28 B per value"
          % (torch.cuda.get_device_name(0), len(tensors), n, n / 1e6, 28 * n / 1e9))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for t in tensors:
        t.requires_grad_()
        t.grad = torch.randn(t.shape, device="cuda", generator=gen) * 1e-2
    opt = TFAdam(eng, tensors, lr=1e-5)
    slow = sum(t.numel() for t, m, v in zip(tensors, opt.m, opt.v) if (t.data_ptr() | t.grad.data_ptr() | m.data_ptr() | v.data_ptr()) & 15)
    print("adam_bench: %d values (%d bytes of parameters, %.4f %% of the set) take the 4-byte path" % (slow, 4 * slow, 100.0 * slow / n))
    floor = 28 * n / (COPY_TBS * 1e12) * 1e3
    ours = median_ms(opt.step)
    print("adam_bench: hmmr_adam_step (TFAdam.step)            %7.3f ms per step (median of %d; min %.3f, max %.3f) = %.2f TB/s; derived floor %.3f ms "
          "at %.2f TB/s; measured / floor = %.2f" % (ours[0], SAMPLES, ours[1], ours[2], 28 * n / ours[0] / 1e9, floor, COPY_TBS, ours[0] / floor))
    topt = torch.optim.Adam(tensors, lr=1e-5, foreach=True)
    ref = median_ms(topt.step)
    print("adam_bench: torch.optim.Adam(foreach=True).step      %7.3f ms per step (median of %d; min %.3f, max %.3f); hmmr_adam_step / torch = %.2f"
          % (ref[0], SAMPLES, ref[1], ref[2], ours[0] / ref[0]))
    print("adam_bench: unmeasured: any counter, any set but this one, agreement with a TensorFlow binary")


if __name__ == "__main__":
    main()
