"""The trainer's loss stage (csrc/losses.hip: hmmr_seq_losses), the closed loop omega -> losses, d_omega (hmmr_omega_loss_grad) and
their Python routes (ops.py, trainer_losses.py) against torch.autograd in float64.

Every loss vector and every cotangent is compared SEPARATELY with the float64 autograd of the restated oracle (tests/loss_cases.py,
pinned to the reference's own functions by tests/test_loss_cases.py).  The bound is not a chosen number: E32 = |autograd in float32
- autograd in float64| over the case's group (the cases of one (B, T)) is the error of the same computation in fp32, and a kernel may
be FACTOR = 4 times that away.  tests/test_loss_cases.py asserts that every term alone is at least 1000 bounds large, so a dropped
term cannot pass.  The closed loop is compared on an all-fp32 engine: its forward is then the exact fp32 function that hmmr_smpl_bwd
differentiates (the default engine's split-fp16 blend carries its own documented 2e-6 allowance on joints and kps, which is not a
property of this stage); the default engine is checked byte for byte against the three separate calls.  With `-s` every case prints
its error, E32 and their ratio, and the module prints the largest ratio per quantity at the end (profiles/losses_sweep.log is one
such run).  Every call in this file is a valid call; the refusals are in tests/test_loss_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_cases as LC
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
GUARD = 0x7FC12345            # a quiet NaN with a payload: the bit pattern of every float no kernel may touch
_STATS = {}
_ENGINES = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _engine(device, nv=130, exact=False):
    key = (device, nv, exact)
    if key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        _ENGINES[key] = HmmrEngine(None, LC.G._model(nv), device=device, **({"dtype": "f32"} if exact else {}))
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k, (r, tag) in sorted(_STATS.items()):
        print("losses summary: largest err / E32 of %-16s: %5.2f (%s)" % (k, r, tag))
    _ENGINES.clear()


def _note(kind, key, tag, err, bound):
    e = bound / LC.FACTOR
    ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
    print("losses %-5s %-52s %-9s err %.3e  E32 %.3e  ratio %5.2f" % (kind, tag, key, err, e, ratio))
    k = "%s %s" % (kind, key)
    if ratio > _STATS.get(k, (-1.0, ""))[0]:
        _STATS[k] = (ratio, tag)


def _check(kind, tag, got, ref, bnd, keys):
    for k in keys:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (tag, k)
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        _note(kind, k, tag, err, bnd[k])
        assert err <= bnd[k], (tag, k, err, bnd[k])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _np(x):
    return None if x is None else x.cpu().numpy()


def _stage(eng, case, flags=None, gt=None, **kw):
    """engine.seq_losses on a stage case -> {losses [7], d_kps, d_joints, d_rs, d_beta, best_cam, status} as numpy"""
    flags = case.flags if flags is None else flags
    out = eng.seq_losses(case.B, case.T, flags, case.gt() if gt is None else gt, kps_pred=case.kps_pred, joints_pred=case.joints_pred,
                         rs_pred=case.rs_pred, beta_pred=case.beta_pred, weights=case.weights, delta_t=case.delta_t, K=case.K,
                         want_best_cam=bool(flags & LC.KP_OPTCAM), **kw)
    r = {k: _np(v) for k, v in out.items()}
    assert r["losses"][7] == 0.0
    r["losses"], r["status"] = r["losses"][:7], int(r["status"][0])
    return r


def _cam_bound(cases):
    e = 0.0
    for c in cases:
        if c.flags & LC.KP_OPTCAM:
            e = max(e, float(np.nanmax(np.abs(c.result(torch.float32)["best_cam"] - c.result()["best_cam"]))))
    return LC.FACTOR * e


# ---------------------------------------------------------------------------------------------------------------- the stage
@pytest.mark.parametrize("bt", LC.BT_LIST)
def test_stage_against_float64(bt, gpu_device):
    """everything together for every delta_t (0, +-1, +-5, T - 1) and K = 14 / 25 (19 once), each term alone, vis and has_gt3d as
    weights other than 0 / 1, frames and whole batches without a visible keypoint, all-zero has_gt3d, planted zero residuals"""
    eng = _engine(gpu_device)
    cases = LC.stage_group(*bt)
    bnd = LC.bounds(cases, LC.STAGE_KEYS)
    cam_bnd = _cam_bound(cases)
    for case in cases:
        got, ref = _stage(eng, case), case.result()
        _check("stage", case.name, got, ref, bnd, LC.STAGE_KEYS)
        assert got["status"] == 0, case.name
        reached = set(k for f, ks in LC.FLAG_REACH.items() if case.flags & f for k in ks)
        for k in LC.STAGE_GRADS:
            if k not in reached:
                assert not got[k].view(np.int32).any(), (case.name, k)            # zeros written, exactly
        pi, _ = LC.slice_rows(case.B, case.T, case.delta_t)
        outside = np.setdiff1d(np.arange(case.B * case.T), pi)
        for k in ("d_kps", "d_joints", "d_rs"):                                   # rows outside the slice: zero from the sliced terms
            assert not got[k][outside].view(np.int32).any(), (case.name, k)
        assert not got["d_joints"][:, 14:].view(np.int32).any(), case.name
        for (n, k, e) in case.planted:
            assert got["d_kps"][n, k, e] == 0.0, (case.name, n, k, e)             # sign(0) = 0
        if case.vis == "none":
            assert got["losses"][0] == 0.0 and not got["d_kps"].any(), case.name        # (a product with vis = 0: +-0)
        if case.has == "zeros":
            assert not got["losses"][1:4].any() and not got["d_joints"].any() and not got["d_rs"].any(), case.name
        if case.flags & LC.KP_OPTCAM:
            cam, want = got["best_cam"], ref["best_cam"]
            assert np.array_equal(np.isnan(cam), np.isnan(want)), case.name       # rows outside the slice are left as they were
            err = float(np.nanmax(np.abs(cam - want)))
            _note("stage", "best_cam", case.name, err, cam_bnd)
            assert err <= cam_bnd, (case.name, err, cam_bnd)
        else:
            assert got["best_cam"] is None


def test_keypoint_counts_beside_the_model_s(gpu_device):
    """the stage alone runs on any keypoint count: 13 (below the 14 joints of the 3-D term, which is then not asked for) and 70"""
    eng = _engine(gpu_device)
    cases = [LC.StageCase(3, 3, 13, 0, LC.KP | LC.SMPL | LC.CONST | LC.SHAPE_PRIOR, seed=920), LC.StageCase(3, 3, 13, 1, LC.KP_OPTCAM, seed=921),
             LC.StageCase(2, 3, 70, -1, LC.KP_OPTCAM | LC.SMPL, seed=922), LC.StageCase(2, 3, 70, 0, LC.ALL | LC.KP, seed=923)]
    bnd = LC.bounds(cases, LC.STAGE_KEYS)
    for case in cases:
        got = _stage(eng, case)
        _check("stage", case.name, got, case.result(), bnd, LC.STAGE_KEYS)
        assert got["status"] == 0 and got["d_kps"].shape == (case.B * case.T, case.K, 2)


def test_frame_without_a_visible_keypoint_under_the_optimal_camera(gpu_device):
    """the reference divides 0 by 0 there: the oracle's loss is not finite, the device's is not either, and says why"""
    eng = _engine(gpu_device)
    case = LC.StageCase(3, 3, 25, 1, LC.ALL | LC.KP_OPTCAM, seed=900)
    pi, gi = LC.slice_rows(3, 3, 1)
    gt = case.gt()
    gt["kps"] = gt["kps"].copy()
    gt["kps"][gi[2], :, 2] = 0.0
    with np.errstate(all="ignore"):
        want = LC.losses(case.pred(torch.float64), {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in gt.items()}, 3, 3, case.flags,
                         case.weights, 1)
    assert not np.isfinite(float(want["e_kp"])) and not np.isfinite(float(want["total"]))
    got = _stage(eng, case, gt=gt)
    assert got["status"] == L.LOSS_NO_VISIBLE | L.LOSS_NOT_FINITE
    assert not np.isfinite(got["losses"][0]) and not np.isfinite(got["losses"][6]) and np.isfinite(got["losses"][1:6]).all()
    others = np.delete(pi, 2)
    assert np.isfinite(got["best_cam"][others]).all() and not np.isfinite(got["best_cam"][pi[2]]).any()
    assert np.isfinite(got["d_kps"][others]).all() and np.isfinite(got["d_joints"]).all() and np.isfinite(got["d_beta"]).all()
    # the same frame outside the slice is never read
    gt["kps"][gi[2], :, 2] = case.kps_gt[gi[2], :, 2]
    outside = np.setdiff1d(np.arange(9), gi)[0]
    gt["kps"][outside] = np.nan
    again = _stage(eng, case, gt=gt)
    clean = _stage(eng, case)
    assert again["status"] == 0 and all(_same_bits(again[k], clean[k]) for k in LC.STAGE_KEYS)
    with pytest.raises(L.HmmrError):
        gt["kps"][gi[2], :, 2] = 0.0
        _stage(eng, case, gt=gt, check=True)


def _raw_call(eng, case, null=(), device=None):
    """hmmr_seq_losses through ctypes with every output between guard rows, the workspace at exactly its reported size in front of a
    guard tail, everything filled with the guard pattern first -> ({name: the output's own rows as float32}, every guard intact?)"""
    lib, dev = L.load(), eng.device
    N, K = case.B * case.T, case.K
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    keep = {k: up(v) for k, v in dict(case.gt(), kps_pred=case.kps_pred, joints_pred=case.joints_pred, rs_pred=case.rs_pred,
                                       beta_pred=case.beta_pred).items()}
    d = L.SeqLossDesc()
    d.B, d.T, d.K, d.delta_t, d.flags = case.B, case.T, K, case.delta_t, case.flags
    d.weights = (C.c_float * 6)(*(list(case.weights) + [0.0]))
    for k in ("kps_pred", "joints_pred", "rs_pred", "beta_pred", "has_gt3d_smpl", "has_gt3d_joints"):
        setattr(d, k, keep[k].data_ptr())
    d.kps_gt, d.joints_gt, d.rs_gt, d.shapes_gt, d.ld_beta = keep["kps"].data_ptr(), keep["joints"].data_ptr(), keep["rs"].data_ptr(), keep["shapes"].data_ptr(), 10
    widths = {"losses": (1, 8), "d_kps": (N, K * 2), "d_joints": (N, K * 3), "d_rs": (N, 216), "d_beta": (N, 10), "best_cam": (N, 3), "status": (1, 1)}
    bufs = {k: torch.full((r + 2, w), GUARD, dtype=torch.int32, device=dev) for k, (r, w) in widths.items()}
    for k in widths:
        setattr(d, k, None if k in null else bufs[k][1:].data_ptr())
    nbytes = lib.hmmr_seq_losses_workspace_bytes(case.B, case.T)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full(((nbytes + (1 << 16)) // 4,), GUARD, dtype=torch.int32, device=dev)
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    L.check(lib.hmmr_seq_losses(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "hmmr_seq_losses")
    torch.cuda.synchronize()
    intact = bool((ws[nbytes // 4:].cpu().numpy() == GUARD).all())
    out = {}
    for k, full in bufs.items():
        host = full.cpu().numpy()
        intact = intact and bool((host[0] == GUARD).all() and (host[-1] == GUARD).all())
        out[k] = host[1:-1]
    return out, intact


@pytest.mark.parametrize("B,T,dt", [(1, 1, 0), (3, 3, -1), (8, 20, 5)])
def test_null_outputs_and_guards(B, T, dt, gpu_device):
    """every output sits between guard rows: nothing beside it changes; a NULL gradient output is not written and changes no other
    output's bytes; best_cam rows outside the slice keep the guard pattern"""
    eng = _engine(gpu_device)
    case = LC.StageCase(B, T, 25, dt, LC.ALL | LC.KP_OPTCAM, seed=910)
    full, intact = _raw_call(eng, case)
    assert intact
    pi, _ = LC.slice_rows(B, T, dt)
    outside = np.setdiff1d(np.arange(B * T), pi)
    assert (full["best_cam"][outside] == GUARD).all() and not (full["best_cam"][pi] == GUARD).any()
    for k in LC.STAGE_GRADS + ("losses", "status"):
        assert not (full[k] == GUARD).any(), k                                    # written in full
    want = _stage(eng, case)                                                      # the engine's own call: the same bits
    for k in LC.STAGE_GRADS:
        assert _same_bits(full[k].view(np.float32).reshape(want[k].shape), want[k]), k
    assert _same_bits(full["losses"].view(np.float32)[0, :7], want["losses"])
    for null in (("d_kps",), ("d_joints",), ("d_rs",), ("d_beta",), ("best_cam", "status"), LC.STAGE_GRADS):
        part, intact = _raw_call(eng, case, null=null)
        assert intact, null
        for k in full:
            if k in null:
                assert (part[k] == GUARD).all(), (null, k)                        # untouched
            else:
                assert np.array_equal(part[k], full[k]), (null, k)


def test_same_call_twice_gives_the_same_bytes(gpu_device):
    eng = _engine(gpu_device)
    case = LC.stage_group(7, 9)[2]
    other = LC.stage_group(5, 13)[0]
    a = _stage(eng, case)
    b = _stage(eng, case)
    _stage(eng, other)                                                            # another call in between leaves nothing behind in the workspace
    c = _stage(eng, case)
    for k in LC.STAGE_KEYS + ("best_cam",):
        if a[k] is not None:
            assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), k


# ---------------------------------------------------------------------------------------------------------------- the closed loop
def _loop(eng, case, flags=None, weights=None):
    losses, d_omega, status, cam = eng.omega_loss_grad(case.omega, case.B, case.T, case.flags if flags is None else flags, case.gt(),
                                                       weights=weights or case.weights, delta_t=case.delta_t, use_optcam=case.use_optcam,
                                                       want_best_cam=bool(case.flags & LC.KP_OPTCAM))
    g = _np(d_omega)
    r = {"losses": _np(losses)[:7], "d_omega": g, "status": int(_np(status)[0]), "best_cam": _np(cam)}
    r.update({k: np.ascontiguousarray(g[:, s]) for k, s in LC.OMEGA_PARTS.items()})
    return r


def _three_calls(eng, case):
    """hmmr_smpl_fwd, hmmr_seq_losses, hmmr_smpl_bwd as three engine calls + the one addition -> (losses [8], d_omega [N,85])"""
    om = torch.from_numpy(case.omega).to(eng.device)
    N = om.shape[0]
    theta, beta = om[:, 3:75], om[:, 75:85]
    cams = torch.tensor([1.0, 0.0, 0.0], device=eng.device).repeat(N, 1) if case.use_optcam else om[:, 0:3]
    verts, joints, kps, rs = eng.smpl(theta, beta, cams)
    out = eng.seq_losses(case.B, case.T, case.flags, case.gt(), kps_pred=kps, joints_pred=joints, rs_pred=rs, beta_pred=beta,
                         weights=case.weights, delta_t=case.delta_t)
    d_theta, d_beta, d_cams = eng.smpl_backward(theta, beta, cams, joints, d_joints=out["d_joints"], d_kps=out["d_kps"], d_rs=out["d_rs"],
                                                want_cams=not case.use_optcam)
    d_cams = torch.zeros((N, 3), device=eng.device) if case.use_optcam else d_cams
    return out["losses"], torch.cat([d_cams, d_theta, d_beta + out["d_beta"]], 1)


@pytest.mark.parametrize("exact", (False, True))
@pytest.mark.parametrize("bt", ((1, 1), (3, 3), (8, 20)))
def test_closed_loop_equals_the_three_calls_byte_for_byte(bt, exact, gpu_device):
    for case in LC.loop_group(*bt):
        eng = _engine(gpu_device, case.nv, exact)
        got = eng.omega_loss_grad(case.omega, case.B, case.T, case.flags, case.gt(), weights=case.weights, delta_t=case.delta_t,
                                  use_optcam=case.use_optcam)
        losses, d_omega = _three_calls(eng, case)
        assert _same_bits(_np(got[0]), _np(losses)) and _same_bits(_np(got[1]), _np(d_omega)), case.name
        again = eng.omega_loss_grad(case.omega, case.B, case.T, case.flags, case.gt(), weights=case.weights, delta_t=case.delta_t,
                                    use_optcam=case.use_optcam)
        assert _same_bits(_np(got[0]), _np(again[0])) and _same_bits(_np(got[1]), _np(again[1])), case.name      # the same call twice
        if case.use_optcam:
            assert not _np(got[1])[:, :3].view(np.int32).any(), case.name


@pytest.mark.parametrize("bt", LC.BT_LIST)
def test_closed_loop_against_float64(bt, gpu_device):
    """d_omega and the losses of the present container (plain keypoint loss, the omega's own camera) and of a delta container (optimal
    camera, cams [1, 0, 0]) on the 50- and 130-vertex models, on the all-fp32 engine"""
    cases = LC.loop_group(*bt)
    bnd = LC.bounds(cases, LC.LOOP_KEYS)
    cam_bnd = _cam_bound(cases)
    for case in cases:
        eng = _engine(gpu_device, case.nv, exact=True)
        got, ref = _loop(eng, case), case.result()
        _check("loop", case.name, got, ref, bnd, LC.LOOP_KEYS)
        assert got["status"] == 0
        if case.flags & LC.KP_OPTCAM:
            assert np.array_equal(np.isnan(got["best_cam"]), np.isnan(ref["best_cam"]))
            err = float(np.nanmax(np.abs(got["best_cam"] - ref["best_cam"])))
            _note("loop", "best_cam", case.name, err, cam_bnd)
            assert err <= cam_bnd
        # the default engine (split-fp16 blend in the forward): measured, not asserted -- its allowance belongs to the forward
        dflt = _loop(_engine(gpu_device, case.nv, exact=False), case)
        for k in LC.LOOP_KEYS:
            _note("split", k, case.name, float(np.abs(dflt[k].astype(np.float64) - ref[k]).max()), bnd[k])


# ---------------------------------------------------------------------------------------------------------------- autograd routes
class _Config(object):
    batch_size, num_kps = 3, 25


def _omegas_gt(eng, case):
    from human_dynamics_amd.omega import OmegasGt
    B, T = case.B, case.T
    gt = OmegasGt(_Config(), np.zeros((B, T, 72), np.float32), case.shapes_gt, case.joints_gt.reshape(B, T, 14, 3),
                  case.kps_gt.reshape(B, T, -1, 3), batch_size=B, engine=eng)
    assert tuple(gt.get_shapes().shape) == (B, T, 10) and torch.equal(gt.get_shapes()[:, 1], gt.shapes)
    eye = torch.eye(3, device=eng.device).expand(B, T, 24, 3, 3)
    assert torch.allclose(gt.get_poses_rot(), eye, atol=1e-6) and tuple(gt.get_deltas_rot().shape) == (B, T - 1, 24, 3, 3)
    gt.poses_rot = torch.from_numpy(case.rs_gt).to(eng.device).reshape(B, T, 24, 3, 3)           # the case's own rotations
    return gt


def test_backward_through_trainer_losses(gpu_device):
    """loss.backward() through trainer_losses.compute_losses_batched gives hmmr_omega_loss_grad's d_omega, bit for bit; a single entry's
    backward (one more run with that entry's weight) gives that term's float64 gradient within the bound"""
    from human_dynamics_amd import trainer_losses as TL
    cases = LC.loop_group(3, 3)
    case = cases[0]
    assert (case.nv, case.delta_t, case.use_optcam) == (130, 0, False)
    eng = _engine(gpu_device, 130, exact=True)
    bnd = LC.bounds(cases, LC.LOOP_KEYS)
    direct = _loop(eng, case)
    gt = _omegas_gt(eng, case)
    names = ("e_kp", "e_joints", "e_smpl", "e_const", "e_shape")
    lw = dict(zip(names, case.weights))
    om = torch.from_numpy(case.omega).to(gpu_device).reshape(3, 3, 85).requires_grad_(True)
    out = TL.compute_losses_batched(eng, om, gt, torch.from_numpy(case.has_smpl), torch.from_numpy(case.has_joints), loss_weights=lw)
    assert sorted(k for k in out if k.startswith("e_")) == sorted(names + ("e_smpl_pose", "e_smpl_shape"))
    assert _same_bits(_np(out["total"].detach()).reshape(1), direct["losses"][6:7]) and int(out["status"]) == 0
    assert float(out["e_smpl"].detach()) == pytest.approx(float(direct["losses"][2] + direct["losses"][3]), rel=1e-6)
    out["total"].backward()
    assert om.grad.shape == (3, 3, 85) and _same_bits(_np(om.grad).reshape(9, 85), direct["d_omega"])
    # one entry alone: e_kp and e_smpl (= pose + shape, one shared weight)
    for key, flag in (("e_kp", LC.KP), ("e_smpl", LC.SMPL)):
        om2 = om.detach().clone().requires_grad_(True)
        TL.compute_losses_batched(eng, om2, gt, torch.from_numpy(case.has_smpl), torch.from_numpy(case.has_joints), loss_weights=lw)[key].backward()
        ref = case.result(flags=flag, weights=(1.0,) * 5)
        got = _np(om2.grad).reshape(9, 85)
        _check("entry", "%s d %s" % (case.name, key), {k: np.ascontiguousarray(got[:, s]) for k, s in LC.OMEGA_PARTS.items()}, ref, bnd, tuple(LC.OMEGA_PARTS))
    # the delta containers: the reference's keys, one call per container
    dcase = cases[2]
    assert dcase.use_optcam and dcase.delta_t != 0
    omd = torch.from_numpy(dcase.omega).to(gpu_device).reshape(3, 3, 85).requires_grad_(True)
    gtd = _omegas_gt(eng, dcase)
    d = TL.compute_losses_deltas(eng, {dcase.delta_t: omd}, gtd, has_gt3d_smpl=torch.from_numpy(dcase.has_smpl),
                                 has_gt3d_joints=torch.from_numpy(dcase.has_joints), loss_weights=lw)
    suffix = "_dt_future" if dcase.delta_t > 0 else "_dt_past"
    assert sorted(k for k in d if k.startswith("e_")) == sorted(k + suffix for k in ("e_kp", "e_joints", "e_smpl"))
    want = case_result = dcase.result(flags=LC.KP_OPTCAM | LC.JOINTS | LC.SMPL)
    d["total"].backward()
    got = _np(omd.grad).reshape(9, 85)
    dbnd = LC.bounds(cases, LC.LOOP_KEYS)
    _check("delta", dcase.name, {k: np.ascontiguousarray(got[:, s]) for k, s in LC.OMEGA_PARTS.items()}, want, dbnd, tuple(LC.OMEGA_PARTS))
    assert abs(float(d["e_kp" + suffix].detach()) - case_result["losses"][0]) <= dbnd["losses"]
    assert np.array_equal(np.isnan(_np(d["best_cam"][dcase.delta_t]).reshape(9, 3)), np.isnan(want["best_cam"]))


def test_ops_reach_smpl_apply(gpu_device):
    """the reference's functions on smpl_apply's outputs: the losses are the oracle's, and loss.backward() arrives at omega with the
    float64 gradient within the bound (another grouping of the same sums than the closed loop)"""
    from human_dynamics_amd import ops
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    cases = LC.loop_group(3, 3)
    case = cases[0]
    eng = _engine(gpu_device, 130, exact=True)
    bnd = LC.bounds(cases, LC.LOOP_KEYS)
    B, T, N = case.B, case.T, case.B * case.T
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    om = dev(case.omega).requires_grad_(True)
    verts, joints, kps, rs = smpl_apply(eng, om[:, 3:75], om[:, 75:85], om[:, 0:3])
    beta = om[:, 75:85]
    ops.set_engine(eng)
    try:
        e_kp = ops.compute_loss_e_kp(dev(case.kps_gt), kps)
        rep = lambda h: dev(h).repeat_interleave(T)
        shapes_gt = dev(case.shapes_gt).repeat_interleave(T, 0)
        e_pose, e_shape, e_joints = ops.compute_loss_e_3d(dev(case.rs_gt), rs, shapes_gt, beta, dev(case.joints_gt).reshape(B, T, 14, 3),
                                                          joints.reshape(B, T, -1, 3)[:, :, :14], N, rep(case.has_smpl), rep(case.has_joints))
        b3 = beta.reshape(B, T, 10)
        e_const = ops.compute_loss_e_smooth(b3[:, :-1], b3[:, 1:])
        e_prior = ops.compute_loss_shape(beta)
        mse = ops.compute_loss_mse(dev(case.rs_gt).reshape(N, 216), rs.reshape(N, 216), rep(case.has_smpl))
        opt, cam = ops.compute_loss_e_kp_optcam(dev(case.kps_gt).reshape(B, T, -1, 3), kps.reshape(B, T, -1, 2))
    finally:
        ops.set_engine(None)
    ref = case.result()
    got = np.array([float(v.detach()) for v in (e_kp, e_joints, e_pose, e_shape, e_const, e_prior)])
    for i, k in enumerate(LC.LOSS_NAMES[:6]):
        assert abs(got[i] - ref["losses"][i]) <= bnd["losses"], (k, got[i], ref["losses"][i])
    assert float(mse.detach()) == float(e_pose.detach()) and tuple(cam.shape) == (B, T, 3) and np.isfinite(float(opt.detach()))
    w = case.weights
    (w[0] * e_kp + w[1] * e_joints + w[2] * (e_pose + e_shape) + w[3] * e_const + w[4] * e_prior).backward()
    g = _np(om.grad)
    _check("ops", case.name, {k: np.ascontiguousarray(g[:, s]) for k, s in LC.OMEGA_PARTS.items()}, ref, bnd, tuple(LC.OMEGA_PARTS))


def test_ops_mse_and_smoothness_on_other_widths(gpu_device):
    """compute_loss_mse aligns nothing and takes any row width up to 216 (42 unaligned joints, 10, 216, 7); compute_loss_e_smooth any
    shape (a count that is no multiple of ten).  Against float64 torch on the same fp32 inputs; the tolerance is a few fp32 roundings of
    the result (the stage rounds its fp64 loss once, the width factor once more: 1e-6 relative), gradients likewise per element of
    the largest"""
    from human_dynamics_amd import ops
    eng = _engine(gpu_device)
    rng = np.random.Generator(np.random.PCG64(4711))
    n = 9
    has = np.array([1.0, 0.0, 0.5, 1.0, 2.0, 1.0, 0.0, 1.0, 1.0], np.float32)
    for D in (42, 10, 216, 7):
        a, b = rng.normal(0, 0.3, (n, D)).astype(np.float32), rng.normal(0, 0.3, (n, D)).astype(np.float32)
        x = torch.from_numpy(b).to(gpu_device).requires_grad_(True)
        got = ops.compute_loss_mse(torch.from_numpy(a).to(gpu_device), x, torch.from_numpy(has).to(gpu_device), engine=eng)
        got.backward()
        x64 = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
        want = LC._mse(torch.from_numpy(a.astype(np.float64)), x64, torch.from_numpy(has.astype(np.float64)))
        want.backward()
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-6 * float(want.detach()), (D, float(got.detach()), float(want.detach()))
        assert float((x.grad.cpu().double() - x64.grad).abs().max()) <= 1e-6 * float(x64.grad.abs().max()), D
    for shape in ((3, 2, 14, 3), (9, 10), (1, 7)):
        a, b = rng.normal(0, 0.3, shape).astype(np.float32), rng.normal(0, 0.3, shape).astype(np.float32)
        x = torch.from_numpy(a).to(gpu_device).requires_grad_(True)
        got = ops.compute_loss_e_smooth(x, torch.from_numpy(b).to(gpu_device), engine=eng)
        got.backward()
        x64 = torch.from_numpy(a.astype(np.float64)).requires_grad_(True)
        want = 0.5 * ((x64 - torch.from_numpy(b.astype(np.float64))) ** 2).mean()
        want.backward()
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-6 * float(want.detach()), shape
        assert x.grad.shape == x.shape and float((x.grad.cpu().double() - x64.grad).abs().max()) <= 1e-6 * float(x64.grad.abs().max()), shape


# ---------------------------------------------------------------------------------------------------------------- descent
def test_gradient_descent_on_omega_follows_the_float64_run(gpu_device):
    """twelve plain gradient-descent steps on omega under the present container's total loss, step size chosen on the host
    (test_loss_cases.py: the float64 run falls at every step and ends below half its start).  The device run falls at every step and
    ends within 1e-3 relative of the float64 run: gradient errors at the bound are orders below the gradients, so a larger gap is a
    wrong term, not rounding."""
    case, want = LC.descent_case(), LC.descent_reference()
    eng = _engine(gpu_device, case.nv, exact=True)
    om = torch.from_numpy(case.omega).to(gpu_device)
    gt = {k: torch.from_numpy(v).to(gpu_device) for k, v in case.gt().items()}
    losses = []
    for _ in range(LC.DESCENT_STEPS + 1):
        l, g, status, _cam = eng.omega_loss_grad(om, case.B, case.T, case.flags, gt, weights=case.weights)
        losses.append(float(l[6]))
        om = om - LC.DESCENT_LR * g
    print("losses descent: device  %s" % " ".join("%.5g" % v for v in losses))
    print("losses descent: float64 %s" % " ".join("%.5g" % v for v in want))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs(losses[-1] - want[-1]) <= 1e-3 * want[-1], (losses[-1], want[-1])
