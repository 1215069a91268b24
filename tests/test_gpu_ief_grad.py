"""The IEF regressors under training on the device (csrc/ief_grad.hip: hmmr_ief_fwd_train, hmmr_ief_bwd) and their Python routes
(HmmrEngine.ief_train / ief_backward, ief_autograd.ief_apply, models.batch_pred_omega_train) against torch.autograd in float64.

The omegas and every gradient are compared SEPARATELY with the float64 autograd of the restated oracle (tests/ief_grad_cases.py, pinned to
tail_cases.compose_ief by tests/test_ief_grad_cases.py).  The bound is not a chosen number: E32 = |autograd in float32 - autograd in float64|
over the case's group is the error of the same computation in fp32, and a kernel may be FACTOR = 4 times that away.  Every compared case
carries a keep mask whose ambiguous units (pre-activations within rounding distance of zero) are cleared, so kernel and oracle agree on the
sign of every unit that counts; the keep == NULL path is pinned bit for bit to the all-ones mask and compared on a case without any
ambiguous unit.  With `-s` every case prints its error, E32 and their ratio, and the module prints the largest ratio per quantity at the
end (profiles/ief_grad_sweep.log is one such run).  Every call in this file is a valid call; the refusals are in tests/test_ief_grad_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import ief_grad_cases as IC
import tail_cases as TC
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
GUARD = 0x7FC12345            # a quiet NaN with a payload: the bit pattern of every float no kernel may touch
_STATS = {}
_ENGINES = {}
_RESULTS = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _engine(device, R=3, width=72, stages=3):
    deltas = tuple(sorted(IC.DELTAS_OF[R]))
    key = (device, deltas, width, stages)
    if key not in _ENGINES:
        from human_dynamics_amd import packing
        from human_dynamics_amd.engine import HmmrEngine
        all_w = TC.ief_weights(width)
        scopes = tuple(TC.delta_scope(d) + "/" for d in deltas) + ("single_view_ief/", "mean_param")
        w = {k: v for k, v in all_w.items() if k.startswith(scopes)}
        eng = HmmrEngine(w, None, dtype="f32", device=device, delta_t_values=deltas)
        if stages != 3:
            eng.iw, eng.reg_keys = packing.pack_ief(w, eng.ief_dtype, eng.store, deltas, num_stages=stages)
        bank = eng.ief_bank()
        assert (bank.iw.dtype, bank.iw.num_regressors, bank.iw.num_stages) == (L.HMMR_F32, R, stages)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k, (r, tag) in sorted(_STATS.items()):
        print("ief_grad summary: largest err / E32 of %-20s: %5.2f (%s)" % (k, r, tag))
    _ENGINES.clear()
    _RESULTS.clear()


def _note(key, tag, err, bound):
    e = bound / IC.FACTOR
    ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
    print("ief_grad %-44s %-20s err %.3e  E32 %.3e  ratio %5.2f" % (tag, key, err, e, ratio))
    if ratio > _STATS.get(key, (-1.0, ""))[0]:
        _STATS[key] = (ratio, tag)


def _check(tag, got, ref, bnd):
    for k, err in IC.errors(got, ref).items():
        assert all(np.isfinite(a).all() for a in IC.quantities(got)[k]), (tag, k)
        _note(k, tag, err, bnd[k])
        assert err <= bnd[k], (tag, k, err, bnd[k])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _same_result(a, b):
    qa, qb = IC.quantities(a), IC.quantities(b)
    return sorted(qa) == sorted(qb) and all(_same_bits(x, y) for k in qa for x, y in zip(qa[k], qb[k]))


def _run(eng, case, pc, keep="mask", **kw):
    """engine.ief_train + engine.ief_backward on a case -> dict(omegas, d_strips, d_omega_start, grads) of float32 numpy"""
    mask = dict(keep=pc["keep"], keep_prob=1.0 / pc["scale"]) if keep == "mask" else {}
    start = pc["start"] if case.start == "rows" else None
    om = eng.ief_train(pc["strips"], start, use_delta_from_pred=case.from_pred, **mask)
    d_strips, d_start, grads = eng.ief_backward(pc["strips"], pc["d_omegas"], start, use_delta_from_pred=case.from_pred, want_start=True, **dict(mask, **kw))
    n = lambda x: None if x is None else x.cpu().numpy()
    return dict(omegas=n(om), d_strips=n(d_strips), d_omega_start=n(d_start), grads=[{k: n(v) for k, v in g.items()} for g in grads])


def _result(device, case):
    """the case's full result, computed once per module"""
    if case.name not in _RESULTS:
        _RESULTS[case.name] = _run(_engine(device, case.R, case.width, case.stages), case, IC.prepared(case))
    return _RESULTS[case.name]


# ---------------------------------------------------------------------------------------------------------------- a. against the oracle
@pytest.mark.parametrize("case", IC.CASES, ids=lambda c: c.name)
def test_case_matches_float64_autograd(case, gpu_device):
    """omegas and every gradient within FACTOR x E32; the copied / constant columns of the omegas exactly; padded rows and columns of the
    weight gradients exact zeros; a second call gives the same bytes"""
    pc, ref = IC.prepared(case), IC.reference(case)
    got = _result(gpu_device, case)
    _check(case.name, got, ref, IC.bounds(case))
    src = got["omegas"][0] if case.from_pred else pc["start"]
    for r in range(1, case.R):
        assert _same_bits(got["omegas"][r][:, 75:], np.ascontiguousarray(src[:, 75:]))
        if case.width == 72:
            assert (got["omegas"][r][:, 0] == 1.0).all() and not got["omegas"][r][:, 1:3].any()
    for r, g in enumerate(got["grads"]):
        nd = 85 if r == 0 else case.width
        for a in (g["fc1_theta"][:, nd:], g["fc3"][nd:], g["b3"][nd:]):
            assert not a.view(np.int32).any(), (case.name, r)                       # (+0.0, bit for bit)
    again = _run(_engine(gpu_device, case.R, case.width, case.stages), case, pc)
    assert _same_result(got, again), case.name


@pytest.mark.parametrize("name", ["m33_R3", "m7_R8", "m33_R3_w75_from_start_stage1_mean_ones"])
def test_ungrouped_launches_give_the_same_bytes(name, gpu_device):
    from human_dynamics_amd import engine as E
    case = IC.BY_NAME[name]
    got = _result(gpu_device, case)
    E.set_debug(ief_no_group=1)
    try:
        alone = _run(_engine(gpu_device, case.R, case.width, case.stages), case, IC.prepared(case))
    finally:
        E.set_debug()
    assert _same_result(got, alone)


def test_a_row_does_not_depend_on_the_other_rows(gpu_device):
    """rows 0..6 of the m = 33 call equal the m = 7 call on those rows, bit for bit: omegas, d_strips, d_omega_start"""
    big, small = _result(gpu_device, IC.BY_NAME["m33_R3"]), _result(gpu_device, IC.BY_NAME["m7_R3"])
    assert _same_bits(np.ascontiguousarray(big["omegas"][:, :7]), small["omegas"])
    assert _same_bits(np.ascontiguousarray(big["d_strips"][:7]), small["d_strips"])
    assert _same_bits(np.ascontiguousarray(big["d_omega_start"][:7]), small["d_omega_start"])


# ---------------------------------------------------------------------------------------------------------------- b. the keep == NULL path
def test_null_keep_is_the_all_ones_mask_bit_for_bit(gpu_device):
    case = IC.BY_NAME["m33_R3_ones"]
    inp = IC.inputs(case)
    pc = dict(IC.prepared(case), keep=inp["keep0"])                    # all ones, nothing cleared, keep_scale 1
    assert pc["keep"].all() and pc["scale"] == 1.0
    eng = _engine(gpu_device, case.R, case.width, case.stages)
    assert _same_result(_run(eng, case, pc), _run(eng, case, pc, keep=None))
    # ... and hmmr_ief_fwd_from on the same fp32 arithmetic: the inference path of an f32 engine
    assert _same_bits(eng.ief_train(pc["strips"], pc["start"]).cpu().numpy(), eng.ief(pc["strips"], pc["start"]).cpu().numpy())


def test_null_keep_matches_float64_autograd(gpu_device):
    case, tried, _ = IC.null_case()
    assert tried <= IC.MAX_NULL_SEEDS
    got = _run(_engine(gpu_device, case.R, case.width, case.stages), case, IC.null_inputs(), keep=None)
    _check("null_keep", got, IC.null_reference(), IC.null_bounds())


# ---------------------------------------------------------------------------------------------------------------- c. outputs and guards
OUTPUTS = ["d_strips", "d_omega_start"] + [(r, n) for r in range(3) for n in IC.NAMES]
SHAPES = dict(d_strips=2048, d_omega_start=85, fc1_phi=1024 * 2048, fc1_theta=1024 * 128, fc2=1024 * 1024, fc3=128 * 1024, b1=1024, b2=1024, b3=128)


def _guarded(eng, case, pc, wanted):
    """hmmr_ief_bwd through ctypes: every wanted output between guard words, the workspace at exactly its reported size in front of a guard
    tail, everything filled with the guard pattern first -> ({output: float32 array}, every guard intact?)"""
    dev, lib, m = eng.device, eng.lib, case.m
    bank = eng.ief_bank()
    t = lambda a, dt=torch.float32: torch.tensor(np.asarray(a)).to(dev, dt)
    strips, start, d_om, keep = t(pc["strips"]), t(pc["start"]), t(pc["d_omegas"]), t(pc["keep"], torch.uint8)
    numel = lambda o: SHAPES[o] * m if isinstance(o, str) else SHAPES[o[1]]
    bufs = {o: torch.full((numel(o) + 64,), GUARD, dtype=torch.int32, device=dev) for o in wanted}
    nbytes = lib.hmmr_ief_bwd_workspace_bytes(m, case.R, case.stages)
    ws = torch.full(((nbytes + (1 << 16)) // 4,), GUARD, dtype=torch.int32, device=dev)
    d = L.IefBwdDesc()
    d.strips, d.omega_start, d.keep, d.keep_scale, d.m, d.d_omegas = strips.data_ptr(), start.data_ptr(), keep.data_ptr(), pc["scale"], m, d_om.data_ptr()
    for o in wanted:
        p = bufs[o].data_ptr() + 32 * 4
        if isinstance(o, str):
            setattr(d, o, p)
        else:
            setattr(d.reg[o[0]], "d_" + o[1], p)
    iw = L.IefWeights.from_buffer_copy(bank.iw)
    iw.delta_from_start = int(not case.from_pred)
    L.check(lib.hmmr_ief_bwd(C.byref(iw), C.byref(d), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream), "hmmr_ief_bwd")
    torch.cuda.synchronize(dev)
    intact = bool((ws[nbytes // 4:].cpu().numpy() == GUARD).all())
    out = {}
    for o in wanted:
        host = bufs[o].cpu().numpy()
        intact = intact and bool((host[:32] == GUARD).all() and (host[-32:] == GUARD).all())
        out[o] = host[32:-32].view(np.float32)
    return out, intact


def _full_of(res, o):
    return (res[o] if isinstance(o, str) else res["grads"][o[0]][o[1]]).reshape(-1)


@pytest.mark.parametrize("name,wanted", [("m33_R3", OUTPUTS), ("m33_R3", ["d_strips"]), ("m33_R3", ["d_omega_start"]), ("m33_R3", [(0, "fc2")]),
                                         ("m33_R3", [(2, "b3"), (1, "fc1_phi")]), ("m33_R3", [(1, "fc3"), "d_strips"]),
                                         ("m33_R3", [(r, n) for r in (0, 2) for n in ("fc1_theta", "b1", "b2")]),
                                         ("m33_R3_from_start", [(1, "fc2")]), ("m33_R3_from_start", [(0, "fc3"), (0, "b1")]),
                                         ("m33_R3_from_start", ["d_omega_start"])],
                         ids=["all", "d_strips", "d_omega_start", "present_fc2", "two_deltas", "fc3_and_strips", "small_ones",
                              "from_start_delta_alone", "from_start_present_alone", "from_start_d_omega_start"])
def test_skipped_outputs_and_guards(name, wanted, gpu_device):
    """every output sits between guard words and the workspace ends at its reported size: nothing beside them changes; a call that asks
    for some outputs gives the bytes of the full call's -- also where whole regressors are left out (delta_from_start: a delta's weights
    need no other regressor, the present one's need no delta)"""
    case = IC.BY_NAME[name]
    full = _result(gpu_device, case)
    got, intact = _guarded(_engine(gpu_device, case.R, case.width, case.stages), case, IC.prepared(case), wanted)
    assert intact
    for o in wanted:
        assert not (got[o].view(np.int32) == GUARD).any(), o                        # written in full
        assert _same_bits(got[o], np.ascontiguousarray(_full_of(full, o))), o


# ---------------------------------------------------------------------------------------------------------------- d. the Python route
def test_autograd_route_gives_the_bytes_of_ief_backward(gpu_device):
    from human_dynamics_amd.ief_autograd import ief_apply
    case = IC.BY_NAME["m33_R3"]
    pc, full = IC.prepared(case), _result(gpu_device, case)
    eng = _engine(gpu_device, case.R, case.width, case.stages)
    tensors = eng.ief_bank().tensors()
    strips = torch.from_numpy(pc["strips"]).to(gpu_device).requires_grad_()
    start = torch.from_numpy(pc["start"]).to(gpu_device).requires_grad_()
    try:
        for t in tensors:
            t.requires_grad_()
        om = ief_apply(eng, strips, start, keep=pc["keep"], keep_prob=1.0 / pc["scale"], use_delta_from_pred=case.from_pred)
        assert _same_bits(om.detach().cpu().numpy(), full["omegas"])
        om.backward(torch.from_numpy(pc["d_omegas"]).to(gpu_device))
        assert _same_bits(strips.grad.cpu().numpy(), full["d_strips"]) and _same_bits(start.grad.cpu().numpy(), full["d_omega_start"])
        for r in range(case.R):
            for i, n in enumerate(IC.NAMES):
                assert _same_bits(tensors[7 * r + i].grad.cpu().numpy(), full["grads"][r][n]), (r, n)
        # a leaf that does not require a gradient gets none, and the others keep their bytes
        for t in tensors:
            t.grad = None
        tensors[2].requires_grad_(False)
        strips2 = torch.from_numpy(pc["strips"]).to(gpu_device)
        ief_apply(eng, strips2, start.detach(), keep=pc["keep"], keep_prob=1.0 / pc["scale"]).backward(torch.from_numpy(pc["d_omegas"]).to(gpu_device))
        assert tensors[2].grad is None and _same_bits(tensors[3].grad.cpu().numpy(), full["grads"][0]["fc3"])
    finally:
        for t in tensors:
            t.grad = None
            t.requires_grad_(False)


def test_batch_pred_omega_train_draws_and_replays(gpu_device):
    from human_dynamics_amd import models
    eng = _engine(gpu_device, 3, 72, 3)
    B, T = 2, 5
    x = torch.from_numpy(TC.strips_input(B * T, 31)).to(gpu_device).reshape(B, T, 2048)
    args = (x, B, True, 85, None, T, "single_view_ief", eng)
    kw = dict(predict_delta_keys=(-5, 5), use_delta_from_pred=True, use_optcam=True)
    g = torch.Generator(device=gpu_device).manual_seed(7)
    om, deltas, keep = models.batch_pred_omega_train(*args, generator=g, return_keep=True, **kw)
    assert om.shape == (B, T, 85) and sorted(deltas) == [-5, 5] and keep.shape == (3, 3, 2, B * T, 1024) and keep.dtype == torch.uint8
    assert 0.45 < float(keep.float().mean()) < 0.55
    om2, deltas2 = models.batch_pred_omega_train(*args, keep=keep, **kw)                       # a given mask replays the step
    assert _same_bits(om.cpu().numpy(), om2.cpu().numpy()) and all(_same_bits(deltas[k].cpu().numpy(), deltas2[k].cpu().numpy()) for k in deltas)
    ev, _ = models.batch_pred_omega_train(x, B, False, 85, None, T, "single_view_ief", eng, **kw)          # is_training=False: the inference function
    assert _same_bits(ev.reshape(B * T, 85).cpu().numpy(), eng.ief(x.reshape(B * T, 2048))[0].cpu().numpy())
    assert not _same_bits(ev.cpu().numpy(), om.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- e. the chain to the losses
class _Config(object):
    batch_size, num_kps = 2, 25


def _chain_engine(device):
    key = (device, "chain")
    if key not in _ENGINES:
        import loss_cases as LC
        from human_dynamics_amd.engine import HmmrEngine
        scopes = tuple(TC.delta_scope(d) + "/" for d in (-5, 5)) + ("single_view_ief/", "mean_param")
        w = {k: v for k, v in TC.ief_weights(72).items() if k.startswith(scopes)}
        _ENGINES[key] = HmmrEngine(w, LC.G._model(IC.CHAIN_NV), dtype="f32", device=device, delta_t_values=(-5, 5))       # all fp32: the exact function
    return _ENGINES[key]


def _chain_total(eng, c, strips, tensors):
    """strips, bank -> ief_apply -> trainer_losses.compute_losses_batched (the present container) -> the total, a device scalar"""
    import loss_cases as LC
    from human_dynamics_amd import trainer_losses as TL
    from human_dynamics_amd.ief_autograd import ief_apply
    from human_dynamics_amd.omega import OmegasGt
    B, T = c.B, c.T
    gt = OmegasGt(_Config(), np.zeros((B, T, 72), np.float32), c.shapes_gt, c.joints_gt.reshape(B, T, 14, 3), c.kps_gt.reshape(B, T, -1, 3),
                  batch_size=B, engine=eng)
    gt.poses_rot = torch.from_numpy(c.rs_gt).to(eng.device).reshape(B, T, 24, 3, 3)
    om = ief_apply(eng, strips, None, keep=c.keep, keep_prob=1.0 / c.scale, bank_tensors=tensors)
    lw = dict(zip(("e_kp", "e_joints", "e_smpl", "e_const", "e_shape"), LC.WEIGHTS))
    out = TL.compute_losses_batched(eng, om[0].reshape(B, T, 85), gt, torch.from_numpy(c.has_smpl), torch.from_numpy(c.has_joints), loss_weights=lw)
    assert int(out["status"]) == 0
    return out["total"]


@pytest.mark.parametrize("B,T", IC.CHAIN_BT)
def test_chain_to_the_losses_matches_float64_autograd(B, T, gpu_device):
    """loss.backward() through compute_losses_batched and ief_apply puts gradients on the bank's tensors and on the strips: each within
    FACTOR x E32 of the composed oracle's float64 autograd; the delta regressors, which the present container's loss does not read, get
    exact zeros"""
    c = IC.chain_case(B, T)
    eng = _chain_engine(gpu_device)
    tensors = eng.ief_bank().tensors()
    strips = torch.from_numpy(c.strips).to(gpu_device).requires_grad_()
    try:
        for t in tensors:
            t.requires_grad_()
        total = _chain_total(eng, c, strips, tensors)
        total.backward()
        got = dict(total=total.detach().cpu().numpy().reshape(1), d_strips=strips.grad.cpu().numpy(),
                   grads=[{n: tensors[7 * r + i].grad.cpu().numpy() for i, n in enumerate(IC.NAMES)} for r in range(3)])
    finally:
        for t in tensors:
            t.grad = None
            t.requires_grad_(False)
    ref, bnd = c.result(), IC.chain_bounds(c)
    for k, err in IC.chain_errors(got, ref).items():
        _note("chain " + k, c.name, err, bnd[k])
        assert err <= bnd[k], (c.name, k, err, bnd[k])
    assert all(not g[n].view(np.int32).any() for g in got["grads"][1:] for n in IC.NAMES)


def test_twelve_descent_steps_follow_the_float64_run(gpu_device):
    """plain gradient descent on the bank's tensors in place (fixed mask, fixed step): the next call sees the update, and the loss follows
    the float64 run's within FACTOR x the float32 run's deviation, measured on the host (ief_grad_cases.descent_reference)"""
    c = IC.chain_case(*IC.DESCENT_BT)
    d64, bound = IC.descent_reference()
    eng = _chain_engine(gpu_device)
    bank = eng.ief_bank()
    tensors = bank.tensors()
    before = bank.to_checkpoint()
    strips = torch.from_numpy(c.strips).to(gpu_device)
    got = []
    try:
        for t in tensors:
            t.requires_grad_()
        for _ in range(IC.DESCENT_STEPS + 1):
            total = _chain_total(eng, c, strips, tensors)
            got.append(float(total.detach()))
            total.backward()
            with torch.no_grad():
                for t in tensors:
                    t -= IC.DESCENT_LR * t.grad
                    t.grad = None
    finally:
        for t in tensors:
            t.grad = None
            t.requires_grad_(False)
        bank.load_checkpoint(before)
    for i, (g, r, b) in enumerate(zip(got, d64, bound)):
        print("ief_grad descent step %2d: device %.7f  float64 %.7f  deviation %.2e  allowed %.2e" % (i, g, r, abs(g - r), b))
    assert all(abs(g - r) <= b for g, r, b in zip(got, d64, bound)), (got, d64, bound)
    assert all(np.array_equal(v, bank.to_checkpoint()[k]) for k, v in before.items())          # the bank is as it was found
