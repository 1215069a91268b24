"""Host checks of the trainer-loss tests' own foundations (no GPU): the restated oracle of tests/loss_cases.py equals the reference's
own functions executed (tests/golden/reference_losses.npz), the input conditions and the dominance of every term hold, every
refusal of hmmr_seq_losses / hmmr_omega_loss_grad is a -1 with a message in front of any launch, and human_dynamics_amd.ops carries
the reference's names and signatures."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
from human_dynamics_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_losses.npz")


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _golden():
    """the fixture's results under their names + the seeded inputs they were computed from (loss_cases.golden_inputs)"""
    f = np.load(GOLDEN)
    inp = LC.golden_inputs()
    sums = np.array([np.abs(v.astype(np.float64)).sum() for _, v in sorted(inp.items())])
    assert np.array_equal(sums, f["inputs_sum"]), "golden_inputs() no longer yields the inputs the fixture was made from"
    B, T, K = LC.GOLDEN_B, LC.GOLDEN_T, LC.GOLDEN_K
    assert tuple(f["deltas"]) == LC.GOLDEN_DELTAS
    z = {"deltas": f["deltas"], "aligned": f["aligned"], "deltas_rot": f["deltas_rot"], "e_const": f["scalars"][0], "e_shape": f["scalars"][1], "e_kp_novis": f["scalars"][2],
         "zero_weights": f["scalars"][3:6]}
    for i, dt in enumerate(LC.GOLDEN_DELTAS):
        for j, k in enumerate(("e_kp", "e_kp_optcam", "e_joints", "e_smpl_pose", "e_smpl_shape")):
            z["d%+d_%s" % (dt, k)] = f["per_delta"][i, j]
        z["d%+d_best_cam" % dt] = f["best_cam"][i, :, :T - abs(dt)]
    t = lambda k: torch.from_numpy(inp[k].astype(np.float64))
    rod = lambda k: LC.G.O.batch_rodrigues(t(k).reshape(-1, 3)).reshape(B * T, 24, 3, 3)
    pred = {"kps": t("kps_pred"), "joints": t("joints_pred"), "rs": rod("poses_pred"), "beta": t("beta_pred")}
    gt = {"kps": t("kps_gt"), "joints": t("joints_gt"), "rs": rod("poses_gt"), "shapes": t("shapes_gt"), "has_gt3d_smpl": t("has_gt3d_smpl"),
          "has_gt3d_joints": t("has_gt3d_joints")}
    return z, B, T, K, pred, gt


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.abs(a - b).max() <= 1e-11 * max(1.0, float(np.abs(b).max())), (what, a, b)


def test_oracle_equals_the_reference_s_own_functions():
    z, B, T, K, pred, gt = _golden()
    unit = (1.0,) * 5
    kinds = set()
    for dt in [int(d) for d in z["deltas"]]:
        p = "d%+d_" % dt
        pi, _ = LC.slice_rows(B, T, dt)
        plain = LC.losses(pred, gt, B, T, LC.KP | LC.JOINTS | LC.SMPL, unit, dt)
        for k in ("e_kp", "e_joints", "e_smpl_pose", "e_smpl_shape"):
            _close(plain[k], z[p + k], p + k)
        opt = LC.losses(pred, gt, B, T, LC.KP_OPTCAM, unit, dt)
        _close(opt["e_kp"], z[p + "e_kp_optcam"], p + "e_kp_optcam")
        _close(opt["best_cam"].numpy().reshape(B, -1, 3), z[p + "best_cam"], p + "best_cam")
        raw = opt["scale_raw"].numpy()
        kinds |= {"low"} if (raw < 0.7).any() else set()
        kinds |= {"high"} if (raw > 10).any() else set()
        kinds |= {"inside"} if ((raw > 0.7) & (raw < 10)).any() else set()
    assert kinds == {"low", "high", "inside"}
    both = LC.losses(pred, gt, B, T, LC.CONST | LC.SHAPE_PRIOR, unit, 0)
    _close(both["e_const"], z["e_const"], "e_const")
    _close(both["e_shape"], z["e_shape"], "e_shape")
    _close(LC.align_by_pelvis(pred["joints"][:, :14])[:2], z["aligned"], "align_by_pelvis")
    from human_dynamics_amd import ops
    rs = gt["rs"].reshape(B, T, 24, 3, 3)
    _close(ops.compute_deltas_batched(rs[:, :-1], rs[:, 1:])[1, T - 2, ::8], z["deltas_rot"], "compute_deltas_batched")
    # weights: a non-0/1 row weight and a zero one are in the fixture; all zero -> the safe division
    zero = dict(gt, has_gt3d_smpl=gt["has_gt3d_smpl"] * 0, has_gt3d_joints=gt["has_gt3d_joints"] * 0)
    o = LC.losses(pred, zero, B, T, LC.JOINTS | LC.SMPL, unit, 0)
    _close([o["e_smpl_pose"], o["e_smpl_shape"], o["e_joints"]], z["zero_weights"], "zero weights")
    assert not z["zero_weights"].any()
    novis = dict(gt, kps=gt["kps"] * torch.tensor([1.0, 1.0, 0.0], dtype=torch.float64))
    _close(LC.losses(pred, novis, B, T, LC.KP, unit, 0)["e_kp"], z["e_kp_novis"], "no visible keypoint")
    assert float(z["e_kp_novis"]) == 0.0
    # total = sum w_i L_i
    w = LC.WEIGHTS
    o = LC.losses(pred, gt, B, T, LC.ALL | LC.KP, w, 0)
    want = (w[0] * z["d+0_e_kp"] + w[1] * z["d+0_e_joints"] + w[2] * (z["d+0_e_smpl_pose"] + z["d+0_e_smpl_shape"]) + w[3] * z["e_const"]
            + w[4] * z["e_shape"])
    _close(o["total"], want, "total")


def test_slices_are_the_trainer_s():
    """pred [0, T - dt) against gt [dt, T) for the future, pred [|dt|, T) against gt [0, T - |dt|) for the past"""
    assert [a.tolist() for a in LC.slice_rows(2, 4, 0)] == [list(range(8))] * 2
    assert [a.tolist() for a in LC.slice_rows(2, 4, 1)] == [[0, 1, 2, 4, 5, 6], [1, 2, 3, 5, 6, 7]]
    assert [a.tolist() for a in LC.slice_rows(2, 4, -3)] == [[3, 7], [0, 4]]
    assert LC.deltas_for(1) == (0,) and LC.deltas_for(2) == (0, 1, -1) and LC.deltas_for(6) == (0, 1, -1, 5, -5)
    assert LC.deltas_for(9) == (0, 1, -1, 5, -5, 8, -8) and LC.deltas_for(20)[-2:] == (19, -19)


# ---------------------------------------------------------------------------------------------------------------- conditions, dominance
@pytest.mark.parametrize("bt", LC.BT_LIST)
def test_input_conditions_and_dominance(bt):
    """the builders assert the residual and scale conditions themselves (check_conditions); here: the clip families, the planted
    zeros, and that every term ALONE moves each cotangent it reaches by at least DOMINANCE bounds, so a dropped term cannot pass"""
    for group, keys, reach in ((LC.stage_group(*bt), LC.STAGE_KEYS, LC.FLAG_REACH),
                               (LC.loop_group(*bt), LC.LOOP_KEYS, LC.LOOP_REACH)):
        bnd = LC.bounds(group, keys)
        if bt[0] * bt[1] >= 4:
            assert LC.clip_kinds(group) == {"low", "high", "inside"}, (bt, LC.clip_kinds(group))
        for c in group:
            LC.check_conditions(c, c.result())
            if getattr(c, "planted", None):
                for (n, k, e) in c.planted:
                    assert c.result()["d_kps"][n, k, e] == 0.0                    # sign(0) = 0
        full = [c for c in group if c.flags & LC.ALL == LC.ALL and getattr(c, "vis", "binary") == "binary" and getattr(c, "has", "mixed") == "mixed"]
        assert full
        for c in full[:2]:
            for flag, outs in reach.items():
                if not c.flags & flag or (flag == LC.CONST and c.T == 1):
                    continue
                if flag in (LC.JOINTS, LC.SMPL) and not (c.has_smpl.any() and c.has_joints.any()):
                    continue
                alone = c.result(flags=flag)
                for k in outs:
                    assert np.abs(alone[k]).max() >= LC.DOMINANCE * bnd[k], (c.name, flag, k, float(np.abs(alone[k]).max()), bnd[k])


def test_descent_reference_falls():
    ref = LC.descent_reference()
    assert len(ref) == LC.DESCENT_STEPS + 1 and all(b < a for a, b in zip(ref, ref[1:])), ref
    assert ref[-1] < 0.5 * ref[0], ref


# ---------------------------------------------------------------------------------------------------------------- refusals
P = [0x10000 * (i + 1) for i in range(24)]
BIG = 1 << 40


def _desc(**kw):
    d = L.SeqLossDesc()
    d.B, d.T, d.K, d.delta_t, d.flags = 3, 4, 25, 0, LC.ALL | LC.KP
    d.weights = (C.c_float * 6)(*([1.0] * 6))
    names = ("kps_pred", "joints_pred", "rs_pred", "beta_pred", "kps_gt", "joints_gt", "rs_gt", "shapes_gt", "has_gt3d_smpl", "has_gt3d_joints",
             "losses", "d_kps", "d_joints", "d_rs", "d_beta", "best_cam", "status", "ws")
    for i, n in enumerate(names):
        setattr(d, n, P[i])
    d.ld_beta, d.ws_bytes = 10, BIG
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(lib, rc, *words):
    msg = lib.hmmr_last_error()
    assert rc == -1 and msg, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)
    with pytest.raises(L.HmmrError):
        L.check(rc, "losses")


def test_seq_losses_refuses_before_anything_is_queued():
    """every refusal of include/hmmr_hip.h with dummy (never dereferenced) pointers and no device: a call that got past its checks would
    have to launch, and a failed launch is -2"""
    lib = L.load()
    call = lambda **kw: lib.hmmr_seq_losses(C.byref(_desc(**kw)), None)
    _refused(lib, lib.hmmr_seq_losses(None, None), b"hmmr_seq_losses", b"null descriptor")
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-2), dict(K=0), dict(K=-1)):
        _refused(lib, call(**kw), b"hmmr_seq_losses", b"must be positive")
    _refused(lib, call(B=1 << 13, T=(1 << 11) + 1), b"rows exceed 2^24")
    _refused(lib, call(K=13), b"JOINTS needs K >= 14")
    _refused(lib, call(flags=LC.KP | LC.KP_OPTCAM), b"KP and KP_OPTCAM are both set")
    _refused(lib, call(flags=64), b"unknown flag bits")
    for dt in (4, -4, 5, -100):
        _refused(lib, call(delta_t=dt), b"|delta_t|=%d must be below T=4" % abs(dt))
    operands = {LC.KP: ("kps_pred", "kps_gt"), LC.KP_OPTCAM: ("kps_pred", "kps_gt"), LC.JOINTS: ("joints_pred", "joints_gt", "has_gt3d_joints"),
                LC.SMPL: ("rs_pred", "rs_gt", "beta_pred", "shapes_gt", "has_gt3d_smpl"), LC.CONST: ("beta_pred",), LC.SHAPE_PRIOR: ("beta_pred",)}
    for flag, names in operands.items():
        for n in names:
            _refused(lib, call(flags=flag, **{n: None}), b"hmmr_seq_losses", b"is NULL", n.encode() if n != "beta_pred" or flag == LC.SMPL else b"beta_pred")
    _refused(lib, call(losses=None), b"losses is NULL")
    _refused(lib, call(ld_beta=9), b"ld_beta=9")
    need = lib.hmmr_seq_losses_workspace_bytes(3, 4)
    assert need > 0 and lib.hmmr_seq_losses_workspace_bytes(0, 4) == 0 and lib.hmmr_seq_losses_workspace_bytes(3, -1) == 0
    assert lib.hmmr_seq_losses_workspace_bytes(8, 20) > need
    _refused(lib, call(ws_bytes=need - 1), b"workspace too small")
    _refused(lib, call(ws=None), b"workspace too small")


def test_omega_loss_grad_refuses_before_anything_is_queued():
    lib = L.load()
    sc = L.SmplConsts()
    sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = 170, 25, 4, 256
    for name, _ in L.SmplConsts._fields_[4:]:
        setattr(sc, name, 0x100000)
    gc = L.SmplGradConsts()
    gc.num_verts, gc.num_kps, gc.vk_ptr, gc.vk_idx, gc.vk_val = 170, 25, 0x200000, 0x300000, 0x400000

    def call(sc_=sc, gc_=gc, omega=P[20], losses=P[21], d_omega=P[22], ws=P[23], ws_bytes=BIG, desc=True, **kw):
        d = _desc(**kw)
        return lib.hmmr_omega_loss_grad(C.byref(sc_) if sc_ is not None else None, C.byref(gc_) if gc_ is not None else None,
                                        C.byref(d) if desc else None, omega, 0, losses, d_omega, ws, ws_bytes, None)
    for kw in (dict(sc_=None), dict(gc_=None), dict(omega=None), dict(losses=None), dict(d_omega=None)):
        _refused(lib, call(**kw), b"hmmr_omega_loss_grad", b"null argument")
    _refused(lib, call(desc=False), b"hmmr_omega_loss_grad", b"null descriptor")
    _refused(lib, call(T=0), b"must be positive")
    _refused(lib, call(delta_t=-4), b"must be below T=4")
    _refused(lib, call(flags=LC.KP | LC.KP_OPTCAM), b"both set")
    _refused(lib, call(K=14), b"K=14 is not the model's keypoint count 25")
    # what hmmr_smpl_fwd / hmmr_smpl_bwd would refuse only after the launches in front of them
    def model(**kw):
        m = L.SmplConsts.from_buffer_copy(sc)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    for bad in (0, -1, 25):
        _refused(lib, call(sc_=model(lbs_nnz=bad)), b"hmmr_omega_loss_grad", b"lbs_nnz=%d out of range" % bad)
    for vpad in (0, 128, 170, 257, 320):
        _refused(lib, call(sc_=model(vpad=vpad)), b"hmmr_omega_loss_grad", b"vpad=%d" % vpad)
    _refused(lib, call(sc_=model(dirs=0x100004)), b"16-byte aligned")
    for field, v in (("num_verts", 171), ("num_kps", 14)):
        other = L.SmplGradConsts.from_buffer_copy(gc)
        setattr(other, field, v)
        _refused(lib, call(gc_=other), b"hmmr_omega_loss_grad", b"belong to another model")
    _refused(lib, call(kps_gt=None), b"kps_gt is NULL")
    _refused(lib, call(has_gt3d_smpl=None), b"has_gt3d_smpl is NULL")
    need = lib.hmmr_omega_loss_grad_workspace_bytes(C.byref(sc), 3, 4)
    assert need >= 12 * 170 * 3 * 4 + lib.hmmr_smpl_workspace_bytes(12) + lib.hmmr_smpl_bwd_workspace_bytes(C.byref(sc), 12) + lib.hmmr_seq_losses_workspace_bytes(3, 4)
    assert lib.hmmr_omega_loss_grad_workspace_bytes(None, 3, 4) == 0 and lib.hmmr_omega_loss_grad_workspace_bytes(C.byref(sc), 0, 4) == 0
    _refused(lib, call(ws_bytes=need - 1), b"workspace too small")
    _refused(lib, call(ws=None), b"workspace too small")


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_ops_carry_the_reference_s_names_and_signatures():
    from human_dynamics_amd import ops
    want = {"compute_loss_e_kp_optcam": ["kp_gt", "kp_pred", "name"], "compute_loss_e_kp": ["kp_gt", "kp_pred", "name"],
            "compute_loss_e_3d": ["poses_gt", "poses_pred", "shapes_gt", "shapes_pred", "joints_gt", "joints_pred", "batch_size", "has_gt3d_smpl",
                                  "has_gt3d_joints"],
            "compute_loss_mse": ["params_gt", "params_pred", "has_gt3d"], "compute_loss_e_smooth": ["joints_prev", "joints_curr"],
            "compute_loss_shape": ["shapes"], "align_by_pelvis": ["joints"], "compute_deltas_batched": ["poses_prev", "poses_curr"]}
    for name, params in want.items():
        got = list(inspect.signature(getattr(ops, name)).parameters)
        assert got[:len(params)] == params and got[len(params):] in ([], ["engine"]), (name, got)
    # the two that are plain tensor arithmetic run anywhere
    j = torch.arange(2 * 14 * 3, dtype=torch.float64).reshape(2, 14, 3) ** 0.5
    assert torch.equal(ops.align_by_pelvis(j), LC.align_by_pelvis(j))
    R = torch.randn(2, 3, 24, 3, 3, dtype=torch.float64)
    assert torch.allclose(ops.compute_deltas_batched(R[:, :-1], R[:, 1:]), R[:, :-1] @ R[:, 1:].transpose(-1, -2))
    with pytest.raises(L.HmmrError):
        ops.set_engine(None)
        ops.compute_loss_shape(torch.zeros(3, 10))                                # no engine: an error, not a quiet torch fall-back


def test_trainer_loss_surface():
    from human_dynamics_amd import trainer_losses as TL, omega
    assert list(inspect.signature(TL.compute_losses_batched).parameters)[:3] == ["engine", "omegas_raw", "gt"]
    assert list(inspect.signature(TL.compute_losses_deltas).parameters)[:3] == ["engine", "omegas_dict", "gt"]
    assert list(inspect.signature(omega.OmegasGt.__init__).parameters)[1:6] == ["config", "poses_aa", "shapes", "joints", "kps"]
    assert TL._weight_list({"e_kp": 60.0, "e_smpl_dt_future": 2.0}, "_dt_future") == [60.0, 1.0, 2.0, 1.0, 1.0]
    assert L.SeqLossDesc.weights.size == 24 and L.LOSS_NAMES[6] == "total"
