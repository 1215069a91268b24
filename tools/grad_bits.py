"""One sha256 per output tensor of the three backward entry points, to compare two builds of the library byte for byte:

    python tools/grad_bits.py > new.txt;  HMMR_LIB_PATH=<another libhmmr_hip.so> python tools/grad_bits.py > parent.txt;  diff parent.txt new.txt

hmmr_ief_fwd_train / hmmr_ief_bwd with every output on every case of tests/ief_grad_cases.py (its shapes, wirings and inputs with the mask
as drawn), grouped and with hmmr_debug_t.ief_no_group; hmmr_temporal_fwd / hmmr_temporal_bwd and hmmr_hallucinator_fwd /
hmmr_hallucinator_bwd with every output on every case of tests/movie_grad_cases.py (the checkpoint's own weights: equal bytes need no
prepared ones); and the shapes of tools/ief_grad_bench.py and tools/movie_grad_bench.py, m = 160 and 256, (8, 20) and (8, 32).  The sums
of these kernels have fixed orders, so two builds of one function print the same listing.  Only lines that start with "grad_bits " count."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ief_grad_cases as IC          # noqa: E402
import movie_grad_cases as MC        # noqa: E402
import tail_cases as TC              # noqa: E402
from human_dynamics_amd import _lib, engine as E, packing      # noqa: E402


def show(tag, name, x):
    if x is not None:
        a = np.ascontiguousarray(x.cpu().numpy())
        print("grad_bits %-46s %-16s %-18s %s" % (tag, name, "x".join(map(str, a.shape)), hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


_IEF = {}


def ief_engine(R, width, stages):
    deltas = tuple(sorted(IC.DELTAS_OF[R]))
    key = (deltas, width, stages)
    if key not in _IEF:
        _IEF.clear()                  # one bank at a time
        scopes = tuple(TC.delta_scope(d) + "/" for d in deltas) + ("single_view_ief/", "mean_param")
        w = {k: v for k, v in TC.ief_weights(width).items() if k.startswith(scopes)}
        eng = E.HmmrEngine(w, None, dtype="f32", device="cuda:0", delta_t_values=deltas)
        if stages != 3:
            eng.iw, eng.reg_keys = packing.pack_ief(w, eng.ief_dtype, eng.store, deltas, num_stages=stages)
        _IEF[key] = eng
    return _IEF[key]


def ief(tag, eng, inp, start, from_pred):
    mask = dict(keep=inp["keep0"], keep_prob=1.0 / inp["scale"])
    show(tag, "omegas", eng.ief_train(inp["strips"], start, use_delta_from_pred=from_pred, **mask))
    d_strips, d_start, grads = eng.ief_backward(inp["strips"], inp["d_omegas"], start, use_delta_from_pred=from_pred, want_start=True, **mask)
    show(tag, "d_strips", d_strips)
    show(tag, "d_omega_start", d_start)
    for r, g in enumerate(grads):
        for n in IC.NAMES:
            show(tag, "r%d/%s" % (r, n), g[n])


def movie_engine(blocks):
    held = {v for i in range(blocks) for v in MC.block_vars(i).values()}
    w = {k: v for k, v in TC.weights().items() if k in held or (blocks == 3 and k.startswith("fc2_res/"))}
    return E.HmmrEngine(w, None, dtype="f32", device="cuda:0", num_conv_layers=blocks)


def temporal(tag, eng, phi, cot):
    show(tag, "strips", eng.temporal_train(phi))
    d_phi, grads = eng.temporal_backward(phi, cot)
    show(tag, "d_phi", d_phi)
    for i, g in enumerate(grads):
        for n in MC.BLOCK_NAMES:
            show(tag, "b%d/%s" % (i, n), g[n])


def hallucinator(tag, eng, phi, cot):
    show(tag, "out", eng.hallucinate_train(phi))
    d_phi, g = eng.hallucinate_backward(phi, cot)
    show(tag, "d_phi", d_phi)
    for n in MC.HAL_NAMES:
        show(tag, n, g[n])


def main():
    if not torch.cuda.is_available():
        raise SystemExit("grad_bits needs a HIP device")
    print("grad_bits: %s, library %s" % (torch.cuda.get_device_name(0), _lib.LIB_PATH))
    bench = IC.Case("bench_m256_R3", 256, 3, 3, 72, True, "rows", "half", 14)
    for case in sorted(IC.CASES + (bench,), key=lambda c: (c.R, c.width, c.stages)):
        eng, inp = ief_engine(case.R, case.width, case.stages), IC.inputs(case)
        start = inp["start"] if case.start == "rows" else None
        ief("ief " + case.name, eng, inp, start, case.from_pred)
        E.set_debug(ief_no_group=1)
        try:
            ief("ief " + case.name + " no_group", eng, inp, start, case.from_pred)
        finally:
            E.set_debug()
    _IEF.clear()
    rng = np.random.default_rng(5)
    draw = lambda *shape: rng.normal(size=shape).astype(np.float32)
    for blocks in (1, 2, 3):
        eng = movie_engine(blocks)
        for case in MC.TEMPORAL_CASES:
            if case.blocks == blocks:
                temporal("temporal " + case.name, eng, MC.phi_of(case), MC.cotangent_of(case))
        if blocks == 3:
            for case in MC.HAL_CASES:
                hallucinator("hallucinator " + case.name, eng, MC.phi_of(case), MC.cotangent_of(case))
            for b, t in ((8, 20), (8, 32)):
                phi, cot = draw(b, t, MC.C), draw(b, t, MC.C)
                temporal("temporal bench b%d_t%d" % (b, t), eng, phi, cot)
                hallucinator("hallucinator bench m%d" % (b * t), eng, phi.reshape(b * t, MC.C), cot.reshape(b * t, MC.C))
        del eng


if __name__ == "__main__":
    main()
