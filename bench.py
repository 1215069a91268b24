"""Headline benchmark: frames/sec/GPU of HMMR's inference hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--frames 256] [--dtype f16x3] [--video-frames V]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: set up, the initialisation call, W warm-up steps, K timed steps, the
outputs of the last timed step when `--dump-outputs DIR` is given, and the result line (`value`, `ms_per_step`, ...).
Every other leg described below -- `modes`, the end-to-end error against the oracle, `stress`, `roofline`,
`by_config`, `fps_sustained_2s` / `power`, the PCIe-inclusive rates, `cpu_baseline`, `smpl_verts_max_abs_err` and, with
N > 1, the gather / scaling-efficiency measurements -- runs only with `--full` (their `--no-*` switches still apply
there); in a plain line their fields are null or absent.

`--dump-outputs DIR` writes what the last timed step computed -- the per-frame arrays a caller of the path receives
(`cams`, `joints`, `kps`, `poses`, `shapes`, `verts`, `omegas` and their `_delta` forms) -- as DIR/<name>.npy in
float32.  When all frames together exceed 64 MB, every array holds the same fixed, seeded sample of frames (ascending;
listed in the line's `dump_outputs.frames`).  The inputs (seeded weights and video) are the same from run to run.

Workload (BASELINE.json configs[3], the configuration the metric
"frames/sec/GPU (ResNet+temporal+SMPL, 224x224)" is quoted on): each GPU takes a
256-frame shard of a synthetic video through the `predict_all_images` contract
(B=8, T=20 -> 32 windows): ResNet-v2-50 on every frame of the shard + its halo +
the zero padding image, f_movie on the windows, 3 IEF regressors and 3 SMPL
forwards (present, -5, +5) on every kept frame, 6890-vertex meshes included.
A "step" is one such pass; a "frame" is one OUTPUT frame.  ResNet features are
de-duplicated (each frame encoded once; the reference's literal schedule
encodes it T/g = 2.5 times) -- stated in `config`.  Inputs are resident in HBM
before the timed region and outputs stay in HBM; the PCIe-inclusive rate
(host ndarray in, host dict out, the reference's call surface) is reported
separately as `pcie_inclusive_fps`.

`value` is the mode that meets the reference tolerance (vertices / joints within
1e-4 of the fp32 TF graph): `--dtype auto` (the drop-in default), which probes the
weights on the device (human_dynamics_amd/precision.py) and for the synthetic
seed-0 weights settles on f16x3 -- split-fp16 operands (hi/lo pairs, three fp16
MFMAs per product, fp32 accumulate; filters scaled per output channel).  `stress` in the same line repeats the
end-to-end error for more weight seeds and two hard-conditioned sets.  On one GPU the same line also
carries `modes`: fps and the END-TO-END vertex / joint error against the float64
oracle for every operand mode timed (f16x3, bf16, f32), so the throughput of the
cheaper, out-of-tolerance bf16 mode is visible next to it but never the headline.

With N > 1 ranks: default = weak scaling (every rank its own 256-frame shard; one
RCCL all-gather per step inside the timed region, overlapped with the next
step's compute); `--video-frames V` = strong scaling of ONE V-frame video
(BASELINE configs[4]: V = 4096): rank r encodes V/N output frames + halo.
`all_gather_ms` is the isolated cost of one gather of the step's records.

One JSON line on stdout (rank 0).  `roofline` is for the dominant kernel family
(the ResNet's MFMA launches), timed per launch with HIP events inside
libhmmr_hip.so on the launch stream; `cpu_baseline` times the CPU oracle (a
PyTorch-CPU restatement of the reference graph -- TF 1.8 cannot run here) on a
bounded sample on the host cores.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RESNET_FLOPS_PER_FRAME = 6.9604e9        # 3.4802 GMAC, 53 convs
PEAK_BF16 = 2.5e15                       # dense MFMA peak, MI355X_MICROARCH.md
PEAK_F32 = 157.3e12
# f16x3 issues three fp16 MFMAs (same rate as bf16: 2.5 PF dense) per algorithmic multiply-add: its MFMA ceiling in algorithmic FLOP/s
PEAKS = {"bf16": PEAK_BF16, "f16x3": PEAK_BF16 / 3.0, "f32": PEAK_F32}
ERR_WINDOW_START = 96                    # output frames [96, 104) are checked end to end against the oracle (every weight set of `stress`)
# the headline's own check: four windows spread over the step's output frames -- the first (its leading frames are the reference's zero
# padding images), two in the middle, and the last (trailing padding)
ERR_WINDOW_STARTS = (0, 96, 176, 248)
DUMP_BYTES = 64 * 10 ** 6                # --dump-outputs: at most this much in all
DUMP_SEED = 0                            # ... and the seed of the frame sample beyond it


class Cfg(object):
    def __init__(self, **kw):
        self.load_path = "synthetic:0"
        self.batch_size = 8
        self.sequence_length = 20
        self.pred_mode = "pred"
        self.num_conv_layers = 3
        self.delta_t_values = ["-5", "5"]
        self.smpl_model_path = "synthetic:2"
        self.num_kps = 25
        self.__dict__.update(kw)


def usable_cores(cap=32):
    """Threads worth starting: the cgroup CPU quota of the container (cpu.max) when there is one -- the GPU boxes show
    256 cores but grant 16 CPUs' worth of time, and oversubscribing a quota stalls the process -- else the affinity
    mask, capped (PyTorch-CPU convolutions stop scaling past a few dozen threads)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, cap))


def conv_slot_mask():
    """Which HMMR_RESNET_PROF_SLOTS are conv_gemm launches (csrc/resnet.hip launch order)."""
    from human_dynamics_amd import assets
    kinds = ["misc", "conv", "misc"]
    for scope, c_in, base, depth, stride, has_sc in assets.resnet_units():
        kinds += (["conv"] if has_sc else []) + ["conv"] * 3
    kinds.append("misc")
    return np.array([k == "conv" for k in kinds])


def cpu_baseline(windows=16):
    """The CPU oracle on a bounded sample: `windows` 20-frame windows through the
    reference-literal predict() (ResNet on all 20 frames, 8 kept per window), on
    `cores` threads = what the container may actually use (usable_cores)."""
    from human_dynamics_amd import assets
    from oracle import hmmr_oracle as O
    cores = usable_cores()
    torch.set_num_threads(cores)
    w = assets.make_synthetic_weights(0)
    s = assets.make_synthetic_smpl(2)
    frames = assets.make_synthetic_frames(20 * windows, seed=11).reshape(windows, 20, 224, 224, 3)
    t = O.OracleTester(w, s, batch_size=windows, dtype=torch.float32)
    t.features(frames[0, :2])           # warm the thread pools / allocator
    t0 = time.perf_counter()
    t.predict(frames)
    dt = time.perf_counter() - t0
    return {"value": round(8 * windows / dt, 3), "unit": "frames/sec", "cores": cores, "kind": "port",
            "frames_through_resnet_per_sec": round(20 * windows / dt, 3),
            "host_cores": os.cpu_count(),
            "sample": "%d windows x 20 frames through the fp32 PyTorch-CPU oracle (restatement of the "
                      "reference graph; TF 1.8 unavailable), reference-literal schedule: 8 output frames "
                      "kept per 20-frame window, %.1f s, on %d threads = the CPU quota this process may use "
                      "(sched_getaffinity / cgroup cpu.max), NOT the %d cores the host shows" % (windows, dt, cores, os.cpu_count())}


def oracle_window(span_host, f0, n_total, weights, smpl, starts=(ERR_WINDOW_START,)):
    """float64 oracle on the reference's padded windows that keep output frames [s, s + 8) of the bench video for every s in
    `starts` (tester.py:281-295); the kept frames of all windows, concatenated in the order of `starts`."""
    from oracle import hmmr_oracle as O
    torch.set_num_threads(usable_cores())
    win = np.zeros((len(starts), 20, 224, 224, 3), np.float32)
    for i, s0 in enumerate(starts):
        for j in range(20):
            f = s0 - 6 + j
            if 0 <= f < n_total:
                win[i, j] = span_host[f - f0]
    ref = O.OracleTester(weights, smpl, batch_size=len(starts), dtype=torch.float64).predict(win)
    return {k: np.concatenate([ref[k][i, 6:14] for i in range(len(starts))]) for k in ("verts", "joints", "omegas")}


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n, argv, script=None):
    """Re-run this script (or `script`: the CPU test's stand-in) under torch.distributed.run with one process per GPU -- what
    the driver's N > 1 command does; returns the launcher's exit code.  Rendezvous on 127.0.0.1: the container hostname
    may not resolve."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), script or os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def resolve_workload(args, world):
    """(strong, frames in the job) of a run on `world` ranks: N = 1 and --weak: a --frames shard per rank (BASELINE configs[3],
    weak scaling); N > 1 by default: ONE 4096-frame video sharded over the ranks (BASELINE configs[4], strong scaling);
    --video-frames picks the video length explicitly."""
    if world > 1 and args.video_frames == 0 and not args.weak:
        args.video_frames = 4096
    strong = args.video_frames > 0
    return strong, (args.video_frames if strong else args.frames * world)


def multi_gpu_fields(tester, n_total, span, world, rank, device, reps=3, pipeline=False, step_streams=True):
    """What the N > 1 line says about the ONE collective of the path (run on every rank; works on any backend -- the CPU tests drive it
    with gloo and a stand-in Tester):
      rccl_ranks        dist.get_world_size(), read after an actual all-gather has completed on this group;
      all_gather_ms     {records, theta}: the isolated cost of one gather of a step's payload (max over ranks, mean of `reps`);
      all_gather_bytes  {records, theta}: bytes every rank ends up holding;
      single_video_ms   {records, theta}: ONE step of the whole video -- local pass, gather and (theta) the SMPL evaluation of all
                        frames -- launch to completion with NOTHING overlapped across steps: what one video costs, the
                        north_star's 'reassemble the output sequence' (max over ranks, best of `reps`);
      gather_by_measurement   the mode with the smaller single_video_ms."""
    from human_dynamics_amd import dist as hd

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    plan = hd.ShardPlan(n_total, tester.batch_size, tester.sequence_length, tester.fov, world, rank)
    _, rec_len = tester.record_layout()
    n_reg = 1 + len(tester.delta_t_values)
    out = {"all_gather_ms": {}, "all_gather_bytes": {}, "single_video_ms": {}}
    for mode, width in (("records", rec_len), ("theta", 85 * n_reg)):
        loc = torch.zeros((plan.out_per_rank, width), dtype=torch.float32, device=device)
        full = torch.empty((world * plan.out_per_rank, width), dtype=torch.float32, device=device)
        for _ in range(2):
            dist.all_gather_into_tensor(full, loc)
        sync()
        dist.barrier()
        t1 = time.perf_counter()
        for _ in range(reps):
            dist.all_gather_into_tensor(full, loc)
        sync()
        out["all_gather_ms"][mode] = round(max_over_ranks((time.perf_counter() - t1) / reps * 1e3), 3)
        out["all_gather_bytes"][mode] = int(full.numel() * 4)
        del loc, full
    out["rccl_ranks"] = dist.get_world_size()               # (after the gathers above have completed on this group)
    for mode in ("records", "theta"):
        p = hd.ShardedPredictor(tester, n_total, rank, world, overlap_gather=False, pipeline=pipeline, gather_mode=mode,
                                step_streams=step_streams)
        p.run(span)
        p.finish()
        best = None
        for _ in range(reps):
            sync()
            dist.barrier()
            t1 = time.perf_counter()
            res = p.run(span)
            p.finish()
            sync()
            ms = max_over_ranks((time.perf_counter() - t1) * 1e3)
            best = ms if best is None else min(best, ms)
        assert res.shape[0] == n_total
        out["single_video_ms"][mode] = round(best, 3)
        del p, res
    sv = out["single_video_ms"]
    out["gather_by_measurement"] = "theta" if sv["theta"] < sv["records"] else "records"
    return out


def run_mode(dtype, args, world, rank, device, weights, smpl, span, n_total, steps, warmup, sustain_s=0.0, tester=None,
             on_timed=None):
    """Time `steps` passes of the hot path in operand mode `dtype`.  Returns the timing dict, the
    tester / predictor (for the roofline leg) and the last output tensor.  `on_timed(out, tester)` is called with the
    output of the last timed step right after the timed region (before the sustained leg re-uses its buffer)."""
    from human_dynamics_amd import dist as hd
    from human_dynamics_amd.evaluation.tester import Tester
    if tester is None:
        tester = Tester(Cfg(), weights=weights, smpl=smpl, dtype=dtype, device=str(device))  # "auto": precision.choose_engine
    eng = tester.engine
    pipeline = not (args.no_pipeline or args.graph or args.serial)
    if args.serial or args.graph:
        eng.resnet_streams = 1
    predictor = hd.ShardedPredictor(tester, n_total, rank, world, use_graph=args.graph,
                                     overlap_gather=not args.serial_gather, pipeline=pipeline,
                                     gather_mode=args.gather, step_streams=not args.no_step_streams)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    try:
        # initialisation, not a step: the first call sizes the workspaces and tunes the per-layer conv tiles
        # for this batch size (engine._tune_resnet, ~65 ms) -- kept out of the timed region even with --warmup 0
        out = predictor.run(span)
        predictor.finish()
        for _ in range(warmup):
            out = predictor.run(span)
        predictor.finish()
    except Exception as e:          # never lose the whole measurement to the overlap machinery
        if not pipeline:
            raise
        print("bench.py: pipelined mode failed (%r); falling back to one stream" % (e,), file=sys.stderr)
        pipeline = False
        eng.resnet_streams = 1
        predictor = hd.ShardedPredictor(tester, n_total, rank, world, overlap_gather=False, pipeline=False,
                                         gather_mode=args.gather)
        for _ in range(max(warmup, 1)):
            out = predictor.run(span)
        predictor.finish()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = predictor.run(span)
    predictor.finish()                       # outstanding (overlapped) all-gathers complete inside the timed region
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert out.shape[0] == n_total and bool(torch.isfinite(out[:, :1000]).all())
    if on_timed is not None:
        on_timed(out, tester)
    timing = {"fps": n_total * steps / elapsed, "ms_per_step": elapsed / steps * 1e3, "steps": steps,
              "pipeline": pipeline, "resnet_streams": eng.resnet_streams,
              "step_streams": getattr(predictor, "step_streams", None) is not None}
    if sustain_s > 0:
        # the same steps for at least `sustain_s` seconds of GPU time (the K-step region above is ~0.1 s: too short to say what the box
        # does once its power management has settled): a step count from the measurement above, one timed region, same brackets
        n2 = int(sustain_s * 1.05 / (elapsed / steps)) + 1
        smi = SmiSampler(device.index or 0) if (rank == 0 and not args.no_power) else None
        barrier()
        if smi is not None:
            smi.start()
        t0 = time.perf_counter()
        for _ in range(n2):
            out = predictor.run(span)
        predictor.finish()
        barrier()
        el2 = time.perf_counter() - t0
        power = smi.stop() if smi is not None else None
        if isinstance(power, dict) and power.get("joules"):
            power["joules_per_output_frame"] = round(power["joules"] / (n_total / world * n2), 4)       # this rank's socket, this rank's frames
        timing["power"] = power
        if world > 1:
            t = torch.tensor([el2], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el2 = float(t.item())
        timing.update(sustained_fps=n_total * n2 / el2, sustained_steps=n2, sustained_seconds=el2)
    return timing, tester, predictor, out


def rows_of(out, starts):
    """the output frames [s, s + 8) of every s in `starts`, in that order"""
    return torch.cat([out[s0:s0 + 8] for s0 in starts])


def e2e_errors(out, tester, ref, sliced=False, starts=(ERR_WINDOW_START,)):
    from human_dynamics_amd import dist as hd
    layout, _ = hd.record_layout(len(tester.delta_t_values))
    rec = hd.unpack_outputs(out if sliced else rows_of(out, starts), layout)
    return {"e2e_%s_max_abs_err" % k: float(np.abs(rec[k].cpu().numpy() - ref[k]).max()) for k in ("verts", "joints", "omegas")}


def dump_outputs(out, tester, path, budget=DUMP_BYTES, seed=DUMP_SEED):
    """Write the packed records `out` [n_frames, rec_len] of one step as the per-frame arrays a caller of the path receives,
    path/<name>.npy in float32.  Beyond `budget` bytes every array keeps the same fixed, seeded sample of frames (ascending).
    -> what the line says about it."""
    from human_dynamics_amd import dist as hd
    layout, rec_len = hd.record_layout(len(tester.delta_t_values))
    n = out.shape[0]
    per_frame = rec_len * 4 + 2 * len(layout)          # (the .npy headers, ~128 B per file, budgeted as 2 B per frame and file)
    rows = None
    if n * per_frame > budget:
        rows = np.sort(np.random.default_rng(seed).choice(n, budget // per_frame, replace=False))
        out = out[torch.as_tensor(rows, device=out.device)]
    host = out.float().cpu().numpy()
    os.makedirs(path, exist_ok=True)
    written = 0
    for k, v in hd.unpack_outputs(host, layout).items():
        v = np.ascontiguousarray(v, dtype=np.float32)
        np.save(os.path.join(path, k + ".npy"), v)
        written += v.nbytes
    return {"dir": path, "arrays": sorted(k for k, _, _, _ in layout), "dtype": "float32", "bytes": written,
            "frames_total": n, "frames": None if rows is None else [int(r) for r in rows],
            "sample": None if rows is None else "%d of %d frames, numpy default_rng(%d).choice, ascending" % (len(rows), n, seed)}


def stress_leg(span, span_host, plan, n_total, smpl, device):
    """The end-to-end error of the DEFAULT operand selection (dtype="auto") for more weight sets than the headline's:
    two more seeds of the ordinary generator and the two hard-conditioned sets of oracle/hard_weights.py.  Per set: the
    mode the probe settled on, the error against the float64 oracle on the window that keeps output frames
    [ERR_WINDOW_START, +8), and the distance from the exact-fp32 operand mode over ALL output frames of the step."""
    from human_dynamics_amd import assets, dist as hd
    from human_dynamics_amd.evaluation.tester import Tester
    from oracle import hard_weights as H
    out = []
    plain3 = assets.make_synthetic_weights(3)
    hard = H.make_hard_weights(3)
    sets = [("seed 1", assets.make_synthetic_weights(1)), ("seed 2", assets.make_synthetic_weights(2))]
    hb = dict(hard)
    fx = dict(plain3)
    for k in plain3:
        if k.endswith("fc3/weights"):
            hb[k], fx[k] = plain3[k], hard[k]
    sets += [("hard BN / GN conditioning (oracle/hard_weights.py), seed 3", hb), ("fc3 at 10 x small_xavier, seed 3", fx)]
    del plain3, hard
    for name, w in sets:
        ref = oracle_window(span_host, plan.f0, n_total, w, smpl)
        recs = {}
        for dt in ("f32", None):
            t = Tester(Cfg(), weights=w, smpl=smpl, dtype=dt, device=str(device))
            p = hd.ShardedPredictor(t, n_total, 0, 1)
            recs[dt] = p.run(span).clone()
            torch.cuda.synchronize(device)
            if dt is None:
                e = e2e_errors(recs[dt], t, ref)
                layout, _ = hd.record_layout(len(t.delta_t_values))
                a, b = hd.unpack_outputs(recs[None], layout), hd.unpack_outputs(recs["f32"], layout)
                d = {k: float((a[k] - b[k]).abs().max()) for k in ("verts", "joints", "verts_delta", "joints_delta")}
                e32 = e2e_errors(recs["f32"], t, ref)
                out.append({"weights": name, "operands": t.precision["operands"],
                            "probe": [{k: (round(v, 8) if isinstance(v, float) else v) for k, v in r.items()} for r in t.precision["rungs"]],
                            "e2e_verts_max_abs_err": e["e2e_verts_max_abs_err"], "e2e_joints_max_abs_err": e["e2e_joints_max_abs_err"],
                            "max_abs_diff_from_f32_operands_all_%d_frames" % n_total: d,
                            "f32_operands_e2e_verts_max_abs_err": e32["e2e_verts_max_abs_err"],
                            "within_tolerance": bool(max(e["e2e_verts_max_abs_err"], e["e2e_joints_max_abs_err"]) <= 1e-4 and
                                                     max(d.values()) + e32["e2e_verts_max_abs_err"] <= 1e-4)})
            del t, p
            torch.cuda.empty_cache()
    return out


class SmiSampler:
    """Socket power and the XCDs' shader clocks while a region runs, read by a host thread from the driver's metrics table (amdsmi): nothing runs on
    the GPU for it.  stop() -> means over the samples taken between start() and stop(), the energy the socket drew (the driver's accumulator),
    the power cap; None when amdsmi is not importable, {"error": ...} when it fails."""

    def __init__(self, device_index=0, period_s=0.01):
        self.idx, self.period = device_index, period_s
        self.samples, self.run, self.th, self.smi, self.h = [], False, None, None, None
        try:
            import amdsmi
            amdsmi.amdsmi_init()
            self.smi = amdsmi
            hs = amdsmi.amdsmi_get_processor_handles()
            self.h = hs[device_index] if device_index < len(hs) else hs[0]
            try:
                # amdsmi lists every GPU of the node in ITS order; HIP's device numbering follows *_VISIBLE_DEVICES: match by PCI address
                pr = torch.cuda.get_device_properties(device_index)
                want = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
                for h in hs:
                    if amdsmi.amdsmi_get_gpu_device_bdf(h).lower().startswith(want):
                        self.h = h
                        break
            except Exception:
                pass
        except Exception:
            self.smi = None

    def _poll(self):
        while self.run:
            try:
                m = self.smi.amdsmi_get_gpu_metrics_info(self.h)
                clk = [c for c in (m.get("current_gfxclks") or []) if isinstance(c, (int, float)) and 0 < c < 10000]
                pw = m.get("current_socket_power")
                pw = pw if isinstance(pw, (int, float)) else m.get("average_socket_power")
                self.samples.append((clk, pw if isinstance(pw, (int, float)) else None, m.get("temperature_hotspot")))
            except Exception:
                pass
            time.sleep(self.period)

    def _energy(self):
        try:
            e = self.smi.amdsmi_get_energy_count(self.h)
            return float(e["energy_accumulator"]) * float(e["counter_resolution"]) * 1e-6       # J
        except Exception:
            return None

    def start(self):
        if self.smi is None:
            return
        import threading
        self.samples, self.run = [], True
        self.e0 = self._energy()
        self.th = threading.Thread(target=self._poll, daemon=True)
        self.th.start()

    def stop(self):
        if self.smi is None:
            return None
        e1 = self._energy()
        self.run = False
        self.th.join()
        try:
            clk = np.array([np.mean(c) for c, _, _ in self.samples if c])
            clk_lo = np.array([np.min(c) for c, _, _ in self.samples if c])
            pw = np.array([p for _, p, _ in self.samples if p is not None], dtype=np.float64)
            hot = [t for _, _, t in self.samples if isinstance(t, (int, float))]
            cap = None
            try:
                cap = self.smi.amdsmi_get_power_cap_info(self.h)["power_cap"] / 1e6
            except Exception:
                pass
            return {"socket_w_mean": round(float(pw.mean()), 0) if len(pw) else None, "socket_w_max": round(float(pw.max()), 0) if len(pw) else None,
                    "power_cap_w": cap,
                    "gfxclk_mhz_mean": round(float(clk.mean()), 0) if len(clk) else None,
                    "gfxclk_mhz_min_xcd": round(float(clk_lo.min()), 0) if len(clk_lo) else None,
                    "gfxclk_mhz_max": round(float(clk.max()), 0) if len(clk) else None, "gfxclk_nominal_mhz": 2400,
                    "hotspot_c_max": max(hot) if hot else None, "samples": len(self.samples),
                    "joules": round(e1 - self.e0, 2) if (e1 is not None and self.e0 is not None) else None,
                    "source": "amdsmi gpu_metrics (the driver's table: clocks per XCD as the firmware averages them, socket power), polled every %d ms by a host thread" % int(self.period * 1e3)}
        except Exception as e:
            return {"error": repr(e)}


class ClockSampler:
    """The shader clock beside a measured region (csrc/probe.hip hmmr_clock_probe): one wave on its own stream stores (s_memtime, s_memrealtime)
    pairs every ~5 us until stop() -- shader ticks against the constant reference counter = the clock the part ran at under THAT load."""

    def __init__(self, eng, n=16384):
        self.eng, self.n = eng, n
        self.buf = torch.zeros((n, 2), dtype=torch.int64, device=eng.device)
        self.flag = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        self.one = torch.ones((1,), dtype=torch.int32, device=eng.device)
        self.s_probe, self.s_stop = torch.cuda.Stream(device=eng.device), torch.cuda.Stream(device=eng.device)

    def start(self):
        from human_dynamics_amd import _lib as L
        self.buf.zero_(); self.flag.zero_()
        torch.cuda.synchronize(self.eng.device)
        L.check(self.eng.lib.hmmr_clock_probe(self.buf.data_ptr(), self.n, 1, self.flag.data_ptr(), self.s_probe.cuda_stream), "hmmr_clock_probe")

    def stop(self):
        """-> {"mhz_mean", "mhz_min", "mhz_max" (over ~50 us windows), "samples", "ref_khz"} or None when too few samples landed."""
        torch.cuda.current_stream(self.eng.device).synchronize()    # the measured work (enqueued, not necessarily done) ends first
        with torch.cuda.stream(self.s_stop):
            self.flag.copy_(self.one, non_blocking=True)
        torch.cuda.synchronize(self.eng.device)
        b = self.buf.cpu().numpy()
        b = b[b[:, 1] > 0]
        if len(b) < 12:
            return None
        try:
            ref_khz = int(torch.cuda.get_device_properties(self.eng.device).wall_clock_rate) if hasattr(torch.cuda.get_device_properties(self.eng.device), "wall_clock_rate") else 100000
        except Exception:
            ref_khz = 100000
        b = b[1:]                                                   # (the first sample precedes the region's first launch)
        w = b[::10]
        win = (w[1:, 0] - w[:-1, 0]) / np.maximum(w[1:, 1] - w[:-1, 1], 1) * ref_khz / 1e3
        win = win[(win > 50) & (win < 3000)]                        # (a window that spans a counter glitch reads tens of GHz: dropped)
        if len(win) < 3:
            return None
        return {"mhz_mean": round(float(win.mean()), 0), "mhz_median": round(float(np.median(win)), 0), "mhz_min": round(float(win.min()), 0), "mhz_max": round(float(win.max()), 0),
                "samples": int(len(b)), "ref_khz": ref_khz}


def roofline_leg(tester, plan, span, dtype, frames, power=True):
    """Per-launch timing of the ResNet's MFMA launches, one stream, HIP events inside the library."""
    eng = tester.engine
    device = eng.device
    n_enc = plan.f1 - plan.f0 + 1
    # (a) whole ResNet pass, HIP events on the launch stream, no per-launch instrumentation;
    # (b) one instrumented pass (an event after every launch) only to apportion the pass between
    #     the MFMA launches and the bandwidth kernels around them.
    # Both on ONE stream (no concurrent half-batches): a per-kernel figure, comparable with rocprofv3's
    # per-kernel durations of `bench.py --serial`.
    streams_used = eng.resnet_streams
    eng.resnet_streams = 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        eng.resnet(span, n_zero=1)
    e0.record()
    for _ in range(5):
        eng.resnet(span, n_zero=1)
    e1.record()
    torch.cuda.synchronize(device)
    pass_ms = e0.elapsed_time(e1) / 5
    # the clock the part runs these passes at: ~0.6 s of the same one-stream passes while a host thread reads the driver's metrics table
    # (a separate run: the timing above is undisturbed, and nothing extra runs on the GPU)
    clock_pass = None
    try:
        if not power:
            raise RuntimeError("--no-power")
        smi = SmiSampler(device.index or 0)
        n_p = max(10, int(0.6 / (pass_ms * 1e-3)))
        smi.start()
        for _ in range(n_p):
            eng.resnet(span, n_zero=1)
        torch.cuda.synchronize(device)
        clock_pass = smi.stop()
        if isinstance(clock_pass, dict) and clock_pass.get("gfxclk_mhz_mean"):
            clock_pass["mhz_mean"] = clock_pass["gfxclk_mhz_mean"]
            clock_pass["passes"] = n_p
    except Exception as e:                                # a reporting aid: never fail the bench over it
        clock_pass = {"error": repr(e)}
    sampler = ClockSampler(eng)                           # (for the MFMA-rate probes below: one wave beside kernels that leave room for it)
    eng.resnet(span, prof=True, n_zero=1)
    _, prof = eng.resnet(span, prof=True, n_zero=1)
    eng.resnet_streams = streams_used
    mask = conv_slot_mask()
    fused_stem = dtype in ("bf16", "f16x3")      # slot 0 = the fused stem kernel (an MFMA launch); else slot 1 = the stem GEMM
    if fused_stem:
        mask[0], mask[1] = True, False
    conv_share = float(prof[:len(mask)][mask].sum()) / float(prof[:len(mask)].sum())
    conv_ms = pass_ms * conv_share
    # launches: 53 convolutions minus what the fused units / column-split GEMMs / the fused stem absorb
    skipped = {0: 0, 1: 1, 2: 2, 3: 3, 4: 1}       # launches a fused unit saves, by hmmr_resnet_unit_t.fuse_tail
    n_tails = sum(int(eng.rw.unit[i].fuse_tail > 0) for i in range(16))
    n_conv = 53 - sum(skipped[int(eng.rw.unit[i].fuse_tail)] + int(bool(eng.rw.unit[i].sc_c1.w)) + int(bool(eng.rw.unit[i].c3sc.w)) for i in range(16))
    if dtype in ("bf16", "f16x3") and os.environ.get("HMMR_STEM_C1", "1") != "0":
        n_conv -= 1                                   # block1/unit_1's conv1 runs inside the fused stem launch
    flops_per_launch = RESNET_FLOPS_PER_FRAME * n_enc / n_conv
    avg_launch_s = conv_ms * 1e-3 / n_conv
    achieved = flops_per_launch / avg_launch_s
    peak = PEAKS[dtype]
    mfma_per_product = 3 if dtype == "f16x3" else 1
    # HBM traffic per launch comes from separate rocprofv3 --pmc passes of this same command
    # (FETCH_SIZE x2, WRITE_SIZE x1, KiB; tools/pmc_summary.py) committed under profiles/
    traffic, traffic_src, mfma_util, traffic_commit, families = None, None, None, None, None
    here = os.path.dirname(os.path.abspath(__file__))
    for pm in sorted(glob.glob(os.path.join(here, "profiles", "r*_pmc_summary.json")), reverse=True):
        js = json.load(open(pm))
        if js.get("dtype", "bf16") == dtype and frames == 256:
            rc = js.get("resnet_conv_gemm", {})
            traffic, mfma_util = rc.get("hbm_bytes_per_launch"), rc.get("mfma_util")
            traffic_src = "profiles/" + os.path.basename(pm)
            traffic_commit = js.get("commit")            # stamped by tools/collect_profiles.py: the kernels the counters saw
            families = {k: v.get("mfma_util") for k, v in js.get("families", {}).items()} or None
            break
    # what the matrix pipes of THIS box sustain when they do nothing else (csrc/probe.hip): one wave per SIMD on every CU issuing
    # v_mfma_f32_32x32x16_f16 back to back for ~0.3 ms, best of five launches -- the chip clocks well below 2.4 GHz under that load
    sustained = None
    if dtype in ("f16x3", "bf16"):
        try:
            from human_dynamics_amd import _lib as L
            cus = torch.cuda.get_device_properties(device).multi_processor_count
            n8 = 2500                                     # 20 000 MFMAs per wave: ~0.35 ms

            def mfma_rate(n8_):
                best = None
                for _ in range(6):
                    p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    p0.record()
                    L.check(eng.lib.hmmr_mfma_rate_probe(cus, n8_, None, torch.cuda.current_stream(device).cuda_stream), "hmmr_mfma_rate_probe")
                    p1.record()
                    torch.cuda.synchronize(device)
                    ms_ = p0.elapsed_time(p1)
                    best = ms_ if best is None else min(best, ms_)
                clock = None
                try:
                    if not power:
                        raise RuntimeError("--no-power")
                    sampler.start()
                    for _ in range(12):
                        L.check(eng.lib.hmmr_mfma_rate_probe(cus, n8_, None, torch.cuda.current_stream(device).cuda_stream), "hmmr_mfma_rate_probe")
                    clock = sampler.stop()
                except Exception as e:
                    clock = {"error": repr(e)}
                return cus * 4 * 8 * abs(n8_) * 32768.0 / (best * 1e-3), clock

            rate, clock_mfma = mfma_rate(n8)
            # the same stream on operands that change from MFMA to MFMA (n8 < 0): what the cap allows when the multipliers toggle as on real tensors
            rate_t, clock_t = mfma_rate(-n8)
            sustained = {"tflops": round(rate / 1e12, 1), "instruction": "v_mfma_f32_32x32x16_f16, one wave per SIMD, nothing else issued",
                         "frac_of_nominal": round(rate / PEAK_BF16, 4),
                         "ceiling_for_this_mode": round(rate / mfma_per_product / 1e12, 1),
                         "frac_of_sustained": round(achieved * mfma_per_product / rate, 4),
                         "shader_clock": clock_mfma,
                         "changing_operands": {"tflops": round(rate_t / 1e12, 1), "frac_of_nominal": round(rate_t / PEAK_BF16, 4),
                                               "ceiling_for_this_mode": round(rate_t / mfma_per_product / 1e12, 1),
                                               "frac_of_sustained": round(achieved * mfma_per_product / rate_t, 4), "shader_clock": clock_t,
                                               "instruction": "the same stream, four hashed fp16 fragment pairs taken in turn"},
                         "note": "measured on this box in this run: the power cap, not the 2.4 GHz nominal clock, sets what a dense "
                                 "fp16 MFMA stream reaches; `frac` above stays against the nominal peak"}
        except Exception as e:                            # the probe is a reporting aid: never fail the bench over it
            sustained = {"error": repr(e)}
    clock_adj = None
    if isinstance(clock_pass, dict) and clock_pass.get("mhz_mean"):
        # the same `achieved` against the peak AT THE CLOCK THE PASS RAN AT (nominal peak x measured clock / 2400 MHz): how busy the matrix
        # pipes are in cycles, which is what the PMC figure (mfma_util_pmc) counts; `frac` stays against the nominal peak
        clock_adj = round(achieved / (peak * clock_pass["mhz_mean"] / 2400.0), 4)
    return {"bound": "mfma",
            "mfma_sustained": sustained,
            "shader_clock_during_pass": clock_pass, "frac_at_measured_clock": clock_adj,
            "kernel": "conv_gemm_kernel%s (ResNet-v2-50, %s operands: %d MFMA launches/pass, %d of them fused bottleneck units)"
                      % ({"bf16": " / bottleneck_tail_kernel / stem_fused_kernel", "f16x3": " / conv3x3_stream_kernel / conv1x1_stream_kernel / unit_pair_kernel / b1_unit_kernel / stem_fused_split_kernel"}.get(dtype, ""), dtype, n_conv, n_tails),
            "achieved": round(achieved / 1e12, 2), "peak": round(peak / 1e12, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4),
            # the other reading of the same measurement: algorithmic FLOP/s against the RAW dense bf16 / fp16 MFMA peak (2.5 PF),
            # i.e. what fraction of the machine's headline rate the arithmetic of the reference graph proceeds at
            "frac_of_16bit_dense_peak": round(achieved / PEAK_BF16, 4),
            "mfma_instruction_flops": round(achieved * mfma_per_product / 1e12, 2),
            "peak_note": {"bf16": "dense bf16 MFMA", "f32": "fp32 MFMA",
                          "f16x3": "dense fp16 MFMA (2.5 PF, = bf16) / 3 (three fp16 MFMAs per algorithmic multiply-add)"}[dtype],
            "traffic": traffic, "traffic_unit": "B/launch",
            "traffic_source": traffic_src, "traffic_commit": traffic_commit, "mfma_util_pmc": mfma_util,
            # the counter figures are READ from the committed summary of separate rocprofv3 --pmc passes (the guide's procedure: counters
            # in their own runs), taken at `traffic_commit`; nothing in THIS run measures them
            "traffic_measured_in_this_run": False,
            "mfma_util_pmc_by_family": families,
            "avg_launch_us": round(avg_launch_s * 1e6, 2),
            "flops_per_launch": flops_per_launch,
            "measured": "one stream, no co-running kernels (the timed steps overlap streams)",
            "resnet_pass_ms": round(pass_ms, 3), "conv_ms": round(conv_ms, 3), "frames_encoded": n_enc}


def by_config_leg(tester, weights, device, dtype, headline_frac):
    """The hot path at the OTHER sizes the reference and BASELINE.json name (outside the headline's timed region; everything resident
    in HBM, HIP events on the launch stream, tile tuning and workspaces warmed before each figure):
      configs[1]  batch = 64 frames, ResNet only (FeatureExtractor's fixed batch: src/datasets/resnet_extractor.py:14,74-98) -- the
                  ResNet pass on one stream and as the engine runs it, and the host surface compute_phis (ndarray in, ndarray out);
      predict     the reference's default call: Tester.predict on B = 8 windows of T = 20 frames (src/config.py:43-44,
                  tester.py:229-258), literal schedule: 160 frames through ResNet, f_movie, IEF and 3 x SMPL, all 160 frames returned;
      configs[2]  64 windows x 20 frames = 1280 frames through ResNet + f_movie + IEF (no SMPL);
      window      ONE 20-frame window through Tester.predict_device, launch to completion (latency, not throughput).
    `roofline.frac` of an entry = ResNet FLOPs of its frames / its ResNet pass time (one stream) / the mode's MFMA peak, the headline's
    definition; `frac_vs_headline` relates it to the 257-frame pass of the headline."""
    from human_dynamics_amd.datasets.resnet_extractor import FeatureExtractor
    eng = tester.engine
    peak = PEAKS[dtype]
    gen = torch.Generator(device=device)
    gen.manual_seed(4321)

    def frames(n):
        return torch.rand((n, 224, 224, 3), generator=gen, device=device) * 2 - 1

    def ev_ms(fn, reps, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(device)
        return e0.elapsed_time(e1) / reps

    def resnet_figures(x, reps):
        n = x.shape[0]
        streams = eng.resnet_streams
        eng.resnet_streams = 1
        one = ev_ms(lambda: eng.resnet(x), reps)
        eng.resnet_streams = streams
        asrun = ev_ms(lambda: eng.resnet(x), reps) if len(eng.resnet_cuts(n)) > 2 else one
        tf = RESNET_FLOPS_PER_FRAME * n / (one * 1e-3)
        return one, asrun, {"bound": "mfma", "achieved": round(tf / 1e12, 2), "peak": round(peak / 1e12, 1), "unit": "TFLOP/s",
                            "frac": round(tf / peak, 4), "frac_vs_headline": round(tf / peak / headline_frac, 3) if headline_frac else None}

    out = {}
    # ---- configs[1]
    x64 = frames(64)
    one, asrun, roof = resnet_figures(x64, 30)
    fx = FeatureExtractor("synthetic:0", weights=weights, dtype=dtype, device=str(device))
    x64h = x64.cpu().numpy()
    fx.compute_phis(x64h)
    t0 = time.perf_counter()
    for _ in range(5):
        fx.compute_phis(x64h)
    host_ms = (time.perf_counter() - t0) / 5 * 1e3
    del fx
    out["configs[1]: batch 64, ResNet only"] = {
        "frames": 64, "ms": round(one, 4), "fps": round(64 / (one * 1e-3), 1), "roofline": roof,
        "host_surface": {"call": "FeatureExtractor.compute_phis(ndarray[64,224,224,3]) -> ndarray[64,2048]", "ms": round(host_ms, 3),
                         "fps": round(64 / (host_ms * 1e-3), 1)}}
    # ---- the reference's default predict: B = 8, T = 20
    cfg = Cfg(batch_size=8)
    x160 = frames(160)
    one, asrun, roof = resnet_figures(x160, 20)
    img = x160.reshape(8, 20, 224, 224, 3)
    ms = ev_ms(lambda: tester.predict_device(img), 20)
    out["Tester.predict default: B=8, T=20 (160 frames, literal schedule, all frames returned)"] = {
        "frames": 160, "ms": round(ms, 4), "fps": round(160 / (ms * 1e-3), 1), "resnet_ms_one_stream": round(one, 4),
        "resnet_ms_as_run": round(asrun, 4), "roofline": roof}
    # ---- one window: latency
    w1 = img[:1].contiguous()
    def one_window():
        tester.predict_device(w1)
        torch.cuda.synchronize(device)
    for _ in range(3):
        one_window()
    lat = []
    for _ in range(20):
        t0 = time.perf_counter()
        one_window()
        lat.append((time.perf_counter() - t0) * 1e3)
    one20, _, roof20 = resnet_figures(w1.reshape(20, 224, 224, 3), 30)
    out["one 20-frame window, Tester.predict_device, launch to completion"] = {
        "frames": 20, "ms": round(float(np.median(lat)), 4), "ms_min": round(float(min(lat)), 4),
        "fps": round(20 / (float(np.median(lat)) * 1e-3), 1), "resnet_ms_one_stream": round(one20, 4), "roofline": roof20}
    del x160, img, w1
    # ---- configs[2]: 64 windows x 20 frames, ResNet + f_movie + IEF
    x = frames(1280)
    def cfg2():
        phi = tester.features(x)
        strips = tester._movie_strips(phi.reshape(64, 20, -1))
        return eng.ief(strips.reshape(1280, -1))
    ms = ev_ms(cfg2, 6, warm=2)
    streams = eng.resnet_streams
    eng.resnet_streams = 1
    one = ev_ms(lambda: tester.features(x), 6, warm=1)
    eng.resnet_streams = streams
    tf = RESNET_FLOPS_PER_FRAME * 1280 / (one * 1e-3)
    out["configs[2]: 64 windows x 20 frames (1280), ResNet + f_movie + IEF"] = {
        "frames": 1280, "ms": round(ms, 4), "fps": round(1280 / (ms * 1e-3), 1), "resnet_ms_one_stream": round(one, 4),
        "resnet_passes": "%d frames per pass (Tester.MAX_DEVICE_FRAMES)" % tester.MAX_DEVICE_FRAMES,
        "roofline": {"bound": "mfma", "achieved": round(tf / 1e12, 2), "peak": round(peak / 1e12, 1), "unit": "TFLOP/s",
                     "frac": round(tf / peak, 4), "frac_vs_headline": round(tf / peak / headline_frac, 3) if headline_frac else None}}
    del x
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=256, help="output frames per GPU per step (weak scaling)")
    ap.add_argument("--video-frames", type=int, default=0,
                    help="strong scaling: ONE video of this many frames sharded over the ranks (BASELINE configs[4]: 4096)")
    ap.add_argument("--dtype", default="auto", choices=["auto", "f16x3", "bf16", "f32"],
                    help="operand mode of the headline `value`; auto = the drop-in default (probed on the device against the "
                         "exact-fp32 mode, precision.py): f16x3 for well-conditioned weights")
    ap.add_argument("--no-stress", action="store_true", help="skip the tolerance stress leg (more weight seeds, hard conditioning)")
    ap.add_argument("--only-main", action="store_true", help="skip the other operand modes (`modes`)")
    ap.add_argument("--gather", default="auto", choices=["auto", "records", "theta"],
                    help="N > 1: all-gather the packed per-frame records (253 KB/frame) or only the 3 x 85 omegas "
                         "(1 KB/frame) and evaluate SMPL for the whole video on every rank.  auto: weak scaling -> records "
                         "(hidden under the next step); one video (--video-frames, the N > 1 default) -> theta.  Both modes are "
                         "measured after the timed region (`single_video_ms_by_gather`, `gather_by_measurement`)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline (other operand modes, end-to-end error and stress checks, roofline, "
                         "by_config, sustained leg and power, PCIe-inclusive rates, CPU baseline; N > 1: gather and scaling "
                         "measurements).  Off: set up, warm up, time the steps, dump outputs, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32; at most 64 MB in all, a fixed "
                         "seeded sample of frames beyond that)")
    ap.add_argument("--sustain", type=float, default=None,
                    help="seconds of a second, longer timed leg of the same steps (`fps_sustained_2s`; 0 = skip; "
                         "default 2 with --full, 0 without)")
    ap.add_argument("--no-by-config", action="store_true", help="skip the `by_config` legs (the other BASELINE sizes)")
    ap.add_argument("--no-power", action="store_true",
                    help="skip the power / clock sampling (SmiSampler's ~0.6 s of extra ResNet passes, the clock-probe wave): for runs under a profiler, "
                         "whose per-pass averages should be taken over the steps' own passes")
    ap.add_argument("--by-config-only", action="store_true", help="run ONLY the `by_config` legs and print them as one JSON line (what a --full run "
                                                                  "starts as a child process; --dtype: the operand mode, not auto)")
    ap.add_argument("--no-pcie", action="store_true", help="skip the PCIe-inclusive leg (used for PMC passes)")
    ap.add_argument("--serial-gather", action="store_true",
                    help="N > 1: wait for each all-gather instead of overlapping it with the next step")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="run the per-window tail on the ResNet's stream instead of a second stream "
                         "(default: tail of step k overlaps the ResNet of step k+1)")
    ap.add_argument("--no-step-streams", action="store_true",
                    help="pipelined mode: keep every step's ResNet on the caller's stream as two concurrent half-batch "
                         "sequences instead of alternating whole-batch passes of consecutive steps on two streams")
    ap.add_argument("--serial", action="store_true",
                    help="one HIP stream for everything (no tail pipeline, no concurrent ResNet half-batches): the "
                         "configuration the per-kernel rocprofv3 summaries under profiles/ are taken in, so that "
                         "kernel durations are not inflated by co-running kernels")
    ap.add_argument("--graph", action="store_true",
                    help="replay the local pass as one hipGraph per step (measured equal to eager launches: "
                         "the step is GPU-bound, the host keeps 150 launches ahead)")
    ap.add_argument("--weak", action="store_true",
                    help="N > 1: weak scaling (every rank its own --frames shard) instead of the default, BASELINE configs[4]: "
                         "ONE 4096-frame video sharded over the ranks")
    args = ap.parse_args()

    if args.by_config_only:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (no HIP device visible)")
        from human_dynamics_amd import assets
        from human_dynamics_amd.evaluation.tester import Tester
        device = torch.device("cuda", 0)
        torch.cuda.set_device(device)
        weights, smpl = assets.make_synthetic_weights(0), assets.make_synthetic_smpl(2)
        dt = "f16x3" if args.dtype == "auto" else args.dtype
        t = Tester(Cfg(), weights=weights, smpl=smpl, dtype=dt, device=str(device))
        print(json.dumps(by_config_leg(t, weights, device, dt, None)), flush=True)
        return
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` on its own: become the launcher (one rank per GPU over RCCL, the contract's command)
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    strong, n_total = resolve_workload(args, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible)")
    # (test hook, tests/test_gpu_sizes.py: HMMR_BENCH_BACKEND=gloo with HMMR_BENCH_ONE_DEVICE=1 runs the N > 1 code path with every rank on
    #  cuda:0 of a one-GPU box -- RCCL refuses two ranks on one device; the driver's command never sets them)
    one_dev = os.environ.get("HMMR_BENCH_ONE_DEVICE") == "1"
    backend = os.environ.get("HMMR_BENCH_BACKEND", "nccl")
    device = torch.device("cuda", 0 if one_dev else local_rank)
    torch.cuda.set_device(device)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from human_dynamics_amd import assets, dist as hd

    weights = assets.make_synthetic_weights(0)
    smpl = assets.make_synthetic_smpl(2)
    plan = hd.ShardPlan(n_total, 8, 20, 13, world, rank)
    # synthetic video, resident in HBM: this rank's span of real frames (shard + halo)
    gen = torch.Generator(device=device)
    gen.manual_seed(1234 + rank)
    span = torch.rand((plan.f1 - plan.f0, 224, 224, 3), generator=gen, device=device) * 2 - 1

    # N > 1, `--gather auto`: ONE video is what `--video-frames` measures, and for one video the records gather (253 KB per frame) is
    # exposed while the omegas gather (1 KB per frame + SMPL for all frames on every rank) is not -> theta for a strong-scaling run, records
    # (hidden under the next step) for weak scaling.  Both modes are MEASURED further down (multi_gpu_fields: `single_video_ms`,
    # `gather_by_measurement`), after the headline: HIP streams share a few hardware queues in creation order, and predictors created in
    # front of the headline's would slow it (profiles/r06n).
    gather_requested = args.gather
    if args.gather == "auto":
        args.gather = "theta" if (world > 1 and strong) else "records"
    full = args.full                                       # every leg beyond the headline; a plain run times the steps and stops
    if args.sustain is None:
        args.sustain = 2.0 if full else 0.0
    dumped = {}

    def keep_outputs(out_, tester_):
        if rank == 0:
            dumped.update(dump_outputs(out_, tester_, args.dump_outputs))
    timing, tester, predictor, out = run_mode(args.dtype, args, world, rank, device, weights, smpl, span, n_total,
                                              args.steps, args.warmup, sustain_s=args.sustain,
                                              on_timed=keep_outputs if args.dump_outputs else None)
    mg = None
    if world > 1 and full:
        mg = multi_gpu_fields(tester, n_total, span, world, rank, device, pipeline=False)
    value, ms_per_step = timing["fps"], timing["ms_per_step"]
    from human_dynamics_amd import precision
    from human_dynamics_amd.engine import DTYPE_NAMES
    requested = args.dtype
    args.dtype = DTYPE_NAMES[tester.engine.dtype]         # the ResNet's operand mode (what "auto" resolved to)
    operands_desc = precision.describe(tester.engine)

    # isolated cost of the one collective of a step (outside the timed region): multi_gpu_fields above, the mode the steps ran with
    all_gather_ms = mg["all_gather_ms"][args.gather] if mg else None
    gather_bytes = mg["all_gather_bytes"][args.gather] if mg else None

    # the same per-rank shard as a 1-GPU job (no collective), every rank at once: value / (world x this) = the scaling efficiency
    # of this run (the driver computes its own from the per-N lines)
    scaling_eff, shard_fps, rccl_ranks = None, None, None
    if world > 1 and full:
        rccl_ranks = mg["rccl_ranks"]
        n_loc = plan.o1 - plan.o0
        solo = hd.ShardedPredictor(tester, n_loc, 0, 1, pipeline=not (args.no_pipeline or args.graph or args.serial),
                                   step_streams=not args.no_step_streams)
        span1 = span[plan.o0 - plan.f0:plan.o0 - plan.f0 + n_loc] if span.shape[0] >= n_loc else span
        for _ in range(2):
            solo.run(span1)
        solo.finish()
        torch.cuda.synchronize(device)
        dist.barrier()
        t1 = time.perf_counter()
        for _ in range(max(2, args.steps // 2)):
            solo.run(span1)
        solo.finish()
        torch.cuda.synchronize(device)
        ts = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=device)
        dist.all_reduce(ts, op=dist.ReduceOp.MAX)
        shard_fps = n_loc * max(2, args.steps // 2) / float(ts.item())
        scaling_eff = round(value / (world * shard_fps), 4)
        del solo

    result = None
    if rank == 0:
        roofline = None
        if full:
            roofline = roofline_leg(tester, plan, span, args.dtype, args.frames if not strong else -1, power=not args.no_power)
            # the overlapped reading of the same FLOPs: the timed steps run the ResNet passes of consecutive steps on two streams
            roofline["achieved_overlapped"] = round(RESNET_FLOPS_PER_FRAME * (plan.f1 - plan.f0 + 1) / (ms_per_step * 1e-3) / 1e12, 2)
            roofline["frac_overlapped"] = round(roofline["achieved_overlapped"] / roofline["peak"], 4)
            roofline["achieved_overlapped_note"] = ("ResNet FLOPs of one step / ms_per_step (the step also carries the f_movie / IEF / "
                                                    "SMPL tail on a second stream): the figure `value` corresponds to")
        single = world == 1
        # the other BASELINE / reference sizes in a PROCESS OF THEIR OWN (`bench.py --by-config-only`): HIP streams share a few hardware
        # queues in creation order, and whichever of the two -- the headline's predictor (two step streams, tail stream) or these legs
        # (side streams of the two-part ResNet pass) -- comes second in one process reads 20-25 % slow (profiles/r06a, r06m, r06n)
        by_config = None
        if single and full and not args.no_by_config:
            import subprocess
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--by-config-only", "--dtype", args.dtype],
                                   capture_output=True, text=True, timeout=600)
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                by_config = json.loads(lines[-1]) if (r.returncode == 0 and lines) else {"error": (r.stderr or "no output")[-400:]}
            except Exception as e:                            # a reporting leg: never lose the headline over it
                by_config = {"error": repr(e)}
        if by_config and "error" not in by_config:
            for ent in by_config.values():                    # relate every size to the headline's 257-frame pass
                if isinstance(ent.get("roofline"), dict) and roofline["frac"]:
                    ent["roofline"]["frac_vs_headline"] = round(ent["roofline"]["frac"] / roofline["frac"], 3)
        # ---- the other operand modes, same workload, same steps (extras: never the headline).  Timed BEFORE any host-side
        # work of this script (oracle, PCIe legs): under the container's CPU quota the oracle's thread pool slows the launch
        # thread down afterwards, and the 190-launch bf16 step is the first thing to become host-bound.
        others, modes = {}, {}
        all_frames_diff = None
        err_starts = tuple(s0 for s0 in ERR_WINDOW_STARTS if s0 + 8 <= n_total) or (0,)
        if single and full and not args.only_main:
            for other in [m for m in ("f16x3", "bf16", "f32") if m != args.dtype]:
                tm, t_o, pred_o, out_o = run_mode(other, args, world, rank, device, weights, smpl, span, n_total,
                                                  args.steps, args.warmup)
                modes[other] = dict(fps=round(tm["fps"], 1), ms_per_step=round(tm["ms_per_step"], 3))
                others[other] = (t_o, rows_of(out_o, err_starts).clone())
                if other == "f32" or args.dtype == "f32":
                    # every output frame of the step, headline mode against exact-fp32 operands: with the f32 mode's own
                    # distance from the float64 oracle (in `modes`) this bounds the error of ALL frames, not of 8
                    layout_, _ = hd.record_layout(len(tester.delta_t_values))
                    a_, b_ = hd.unpack_outputs(out, layout_), hd.unpack_outputs(out_o, layout_)
                    all_frames_diff = {k: float((a_[k] - b_[k]).abs().max()) for k in ("verts", "joints", "verts_delta", "joints_delta")}
                    del a_, b_
                del pred_o, out_o
                torch.cuda.empty_cache()
        span_host = span.cpu().numpy() if (single and full) else None
        ref = None
        if single and full and not args.no_cpu_baseline and n_total >= ERR_WINDOW_START + 14:
            ref = oracle_window(span_host, plan.f0, n_total, weights, smpl, err_starts)
            modes[args.dtype] = dict(fps=round(value, 1), ms_per_step=round(ms_per_step, 3), **e2e_errors(out, tester, ref, starts=err_starts))
            for other, (t_o, rows) in others.items():
                modes[other].update(e2e_errors(rows, t_o, ref, sliced=True))
        elif modes:
            modes[args.dtype] = dict(fps=round(value, 1), ms_per_step=round(ms_per_step, 3))

        # ---- PCIe-inclusive rate (host frames in, host dict out: the reference's call surface), 1 GPU only, untimed extra
        def pcie_rate(t, video=None):
            """host float32 frames in -> host dict out, through Tester.predict_all_images (the reference's call surface);
            one warm-up call of the same size (pinned output buffers, staging buffers), then the best of two calls."""
            video = span_host if video is None else video
            def once(**kw):
                t1 = time.perf_counter()
                res = t.predict_all_images(video, **kw)
                dt = time.perf_counter() - t1
                del res
                return dt
            once()
            r = round(len(video) / min(once(), once()), 1)
            r2 = round(len(video) / min(once(want=("joints", "omegas", "cams")), once(want=("joints", "omegas", "cams"))), 1)
            return r, r2
        def pcie_rate_sustained(t, video, n_videos=8):
            """the sustained form of the same surface: n_videos tracks of len(video) frames handed over together
            (Tester.predict_videos: how demo_video.py:172 is driven, one call per person track) -- track k+1 uploads under track
            k's ResNet, track k's tail and download under track k+1's.  Different frames per track (rolled copies)."""
            vids = [np.ascontiguousarray(np.roll(video, 7 * i, axis=0)) for i in range(n_videos)]
            def once():
                t1 = time.perf_counter()
                res = t.predict_videos(vids)
                dt = time.perf_counter() - t1
                del res
                return dt
            once()
            return round(n_videos * len(video) / min(once(), once()), 1)
        pcie_fps = pcie_nov = pcie_sustained = pcie_u8_sustained = None
        pcie_long = pcie_u8 = pcie_u8_long = None
        pcie_other = {}
        if single and full and not args.no_pcie:
            pcie_fps, pcie_nov = pcie_rate(tester)
            if len(span_host) >= 256:            # a 4-chunk video: the streamed steady state (copies under the kernels)
                pcie_long = pcie_rate(tester, np.concatenate([span_host[:256]] * 4))[0]
                pcie_sustained = pcie_rate_sustained(tester, span_host[:256])
            if "bf16" in others:
                pcie_other["bf16"] = pcie_rate(others["bf16"][0])[0]
            # the same frames as uint8 crops (what a video decoder hands over; normalised on the device: 4x less H2D)
            u8 = np.clip(np.rint((span_host + 1.0) * 127.5), 0, 255).astype(np.uint8)
            pcie_u8 = pcie_rate(tester, u8)[0]
            pcie_u8_long = pcie_rate(tester, np.concatenate([u8[:256]] * 4))[0] if len(u8) >= 256 else None
            pcie_u8_sustained = pcie_rate_sustained(tester, u8[:256]) if len(u8) >= 256 else None
        tol = 1e-4
        result = {
            "metric": "frames/sec/GPU (ResNet+temporal+SMPL, 224x224); SMPL verts max-abs-err",
            "value": round(value, 1), "unit": "frames/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": args.dtype if operands_desc == args.dtype else operands_desc, "dtype_requested": requested,
            "precision_probe": tester.precision, "data": "synthetic",
            "config": {"workload": ("BASELINE configs[4]: one %d-frame video sharded over %d GPU(s), full pipeline incl. "
                                    "SMPL LBS (6890 verts), predict_all_images contract B=8 T=20" % (n_total, world))
                       if strong else
                       ("BASELINE configs[3]: %d-frame video shard per GPU, full pipeline incl. "
                        "SMPL LBS (6890 verts), predict_all_images contract B=8 T=20" % args.frames),
                       "frames_per_gpu_per_step": plan.o1 - plan.o0, "windows_per_gpu": plan.w1 - plan.w0,
                       "resnet_frames_encoded_per_gpu": plan.f1 - plan.f0 + 1,
                       "resnet_schedule": "de-duplicated (1x per frame + halo; reference-literal is 2.5x)",
                       "operands": {"f16x3": "split fp16 (hi/lo pairs, 3 fp16 MFMAs per product, fp32 accumulate, filters scaled by a power of two per output channel; "
                                              "tensors 4 B/element): inside the 1e-4 tolerance",
                                    "bf16": "bf16 operands and activations, fp32 accumulate: OUTSIDE the 1e-4 tolerance",
                                    "f32": "exact fp32 MFMA"}[args.dtype],
                       "smpl_calls_per_frame": 3, "launch": ("hipGraph replay of the local pass" if args.graph else
                                  "eager; the ResNet passes of consecutive steps alternate between two streams (one whole-batch "
                                  "launch sequence each, two steps in flight); the f_movie/IEF/SMPL tail of step k runs on its "
                                  "own stream under the ResNets of steps k+1, k+2" if timing.get("step_streams") else
                                  "eager; ResNet as %d concurrent half-batch launch sequences%s" % (
                                      timing["resnet_streams"], "; the f_movie/IEF/SMPL tail of step k runs on its own "
                                      "stream under the ResNet of step k+1" if timing["pipeline"] else "")
                                  if (timing["pipeline"] or timing["resnet_streams"] > 1) else "eager, one stream"),
                       "weights": "synthetic (seed 0), random-init, reference shapes",
                       "parallelism": ("window-sharded x%d, one RCCL all-gather of the %s per step%s" % (
                           world, "packed records" if args.gather == "records" else "omegas (SMPL re-evaluated on every rank)",
                           "" if args.serial_gather else ", overlapped with the compute of the next step"))
                       if world > 1 else "single GPU"},
            "saturated": bool(tester.engine.run_flags() & 1),      # hmmr_run_flags: a split store clamped a value to the fp16 range
            "per_gpu_fps": round(value / world, 1),
            # the same steps over >= 2 s of GPU time (K steps are ~0.1 s): what the box sustains once its clocks have settled
            "fps_sustained_2s": round(timing["sustained_fps"], 1) if "sustained_fps" in timing else None,
            "sustained_leg": ({"steps": timing["sustained_steps"], "seconds": round(timing["sustained_seconds"], 3)}
                              if "sustained_fps" in timing else None),
            # rank 0's socket over that sustained leg (amdsmi, a host thread): the path runs AT the 1 400 W cap, and the cap -- not the 2.4 GHz
            # nominal clock -- sets the clock the matrix pipes get
            "power": timing.get("power"),
            "frames_total": n_total,
            "all_gather_ms": all_gather_ms, "all_gather_bytes": gather_bytes, "rccl_ranks": rccl_ranks,
            "gather": args.gather if world > 1 else None, "gather_requested": gather_requested if world > 1 else None,
            "gather_by_measurement": (mg["gather_by_measurement"] if mg else None),
            # N > 1: both gather modes measured in this run -- one whole step with nothing overlapped across steps, and the bare gather
            "single_video_ms": (mg["single_video_ms"][args.gather] if mg else None),
            "single_video_ms_by_gather": (mg["single_video_ms"] if mg else None),
            "all_gather_ms_by_gather": (mg["all_gather_ms"] if mg else None),
            "all_gather_bytes_by_gather": (mg["all_gather_bytes"] if mg else None),
            # N > 1: value / (N x the fps of one rank's shard run as a 1-GPU job, all ranks at once, same run); the driver
            # computes its own from the per-N lines (tools/scale_table.py does the same)
            "scaling_efficiency": scaling_eff,
            "single_gpu_fps_same_shard": round(shard_fps, 1) if shard_fps else None,
            "roofline": roofline,
            "by_config": by_config,
            "init_untimed": {"conv_tile_tuning_ms_by_batch": {str(n_): ms_ for n_, ms_ in tester.engine.tune_log},
                             "note": "one pass per candidate tile and batch size on the first call, before the warm-up steps"},
            "pcie_inclusive_fps": pcie_fps, "pcie_inclusive_fps_without_verts": pcie_nov,
            "pcie_inclusive_fps_1024_frame_video": pcie_long,
            "pcie_inclusive_fps_sustained": pcie_sustained, "pcie_inclusive_fps_sustained_uint8_input": pcie_u8_sustained,
            "pcie_inclusive_fps_uint8_input": pcie_u8, "pcie_inclusive_fps_uint8_input_1024_frame_video": pcie_u8_long,
        }
        if args.dump_outputs:
            result["dump_outputs"] = dumped
        if modes:
            result["modes"] = modes
            result["tolerance"] = tol
            for m, d in modes.items():
                result[{"f16x3": "f16x3_fps", "bf16": "bf16_fps", "f32": "fp32_fps"}[m]] = d["fps"]
            if "e2e_verts_max_abs_err" in modes.get(args.dtype, {}):
                result["e2e_verts_max_abs_err"] = modes[args.dtype]["e2e_verts_max_abs_err"]
                result["e2e_joints_max_abs_err"] = modes[args.dtype]["e2e_joints_max_abs_err"]
                result["value_meets_tolerance"] = bool(max(result["e2e_verts_max_abs_err"], result["e2e_joints_max_abs_err"]) <= tol)
            if all_frames_diff is not None:
                result["max_abs_diff_from_f32_operands_all_%d_frames" % n_total] = all_frames_diff
        if pcie_other:
            result["pcie_inclusive_fps_bf16"] = pcie_other.get("bf16")
        if single and ref is not None and not args.no_stress and not args.only_main:
            result["stress"] = stress_leg(span, span_host, plan, n_total, smpl, device)
        if full and not args.no_cpu_baseline and single:
            result["cpu_baseline"] = cpu_baseline()
            # second half of the metric: SMPL-stage vertex error vs the float64 oracle on device-regressed theta
            # (the SMPL stage is fp32 in every operand mode)
            from oracle import hmmr_oracle as O
            strips = torch.randn((16, 2048), generator=torch.Generator(device=device).manual_seed(7), device=device)
            om = tester.engine.ief(strips)[0].contiguous()
            v, _, _, _ = tester.engine.smpl(om[:, 3:75], om[:, 75:85], om[:, :3])
            omh = om.cpu().numpy()
            rv, _, _ = O.smpl_forward(omh[:, 75:], omh[:, 3:75], smpl, torch.float64)
            result["smpl_verts_max_abs_err"] = float(np.abs(v.cpu().numpy() - rv.numpy()).max())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
