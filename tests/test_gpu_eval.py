"""The device evaluation path (csrc/eval_metrics.hip, evaluation/eval_util.py, evaluation/eval.py) against
tests/golden/reference_eval.npz, which the reference's own eval_util.py / eval.py produced (tests/golden/make_eval_golden.py).
Every figure is printed before it is asserted."""
import contextlib
import io
import os

import numpy as np
import pytest

import eval_oracle as EO
from conftest import GOLDEN, Config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_eval.npz")))


@pytest.fixture(scope="module")
def engine(weights, smpl_consts, gpu_device):
    from human_dynamics_amd.engine import HmmrEngine
    return HmmrEngine(weights, smpl_consts, dtype="f32", device=gpu_device)


def _tube(ref, name):
    return {k[len(name) + 1:]: v for k, v in ref.items() if k.startswith(name + "/") and k.count("/") == 1}


def _sub(ref, prefix):
    return {k[len(prefix):]: v for k, v in ref.items() if k.startswith(prefix)}


def _rel(name, got, want, tol=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name          # NaN exactly where the reference has NaN
    ok = ~np.isnan(want)
    excess = np.abs(got - want)[ok] - tol * np.abs(want)[ok]
    worst = np.max(np.abs(got - want)[ok] / np.maximum(np.abs(want)[ok], 1e-300), initial=0.0)
    print("%-28s max |got - ref| / |ref| = %.3e over %d values" % (name, worst, ok.sum()))
    assert (excess <= 0).all(), (name, worst)


def _abs(name, got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print("%-28s max |got - ref| = %.3e over %d values" % (name, err, got.size))
    assert err <= tol, (name, err)
    return err


def _check_errors(name, got, want, k):
    """One error dictionary against the fixture's: kp entries relative, pck as a count, 3D entries 1e-6, meshes 2e-5 m."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    worst_mesh = 0.0
    for key in sorted(want):
        label = "%s/%s" % (name, key)
        if key in ("kp", "kp_pa"):
            _rel(label, got[key], want[key])
        elif key == "kp_pck":
            assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), label
            ok = ~np.isnan(want[key])
            assert (np.abs(np.asarray(got[key]) - want[key])[ok] < 0.5 / k).all(), label
        elif key in ("pose", "shape") or np.ndim(want[key]) == 0:
            assert got[key] == -1 and want[key] == -1, label                      # the literal placeholders
        elif key.startswith("mesh"):
            worst_mesh = max(worst_mesh, _abs(label, got[key], want[key], 2e-5))
        else:
            _abs(label, got[key], want[key], 1e-6)
    return worst_mesh


@pytest.mark.parametrize("name,k", [("k25", 25), ("k19", 19)])
def test_keypoint_metrics_and_camera(ref, gpu_device, name, k):
    import ctypes as C
    import torch
    from human_dynamics_amd import _lib
    from human_dynamics_amd.evaluation import eval_util as E
    t = _tube(ref, name)
    img, mv = int(ref["img_size"]), int(ref["min_visible"])
    px = EO.to_image_space32(t["kps_pred"], img)
    flags = C.c_uint(0)
    assert _lib.load().hmmr_run_flags(C.byref(flags), 1) == 0                     # clear what earlier tests left
    e, epa, pck = E.compute_error_kp(t["kps_gt"], px, alpha=0.05 * img, min_visible=mv, device=gpu_device)
    assert isinstance(e, list) and len(e) == len(t["kp"])
    _rel(name + "/kp", e, t["kp"]), _rel(name + "/kp_pa", epa, t["kp_pa"])
    assert np.array_equal(np.isnan(pck), np.isnan(t["kp_pck"]))
    ok = ~np.isnan(t["kp_pck"])
    assert (np.abs(np.array(pck) - t["kp_pck"])[ok] < 0.5 / k).all()
    # the fused map from [-1, 1] gives the same bits as the float32 map done outside, and the camera of every frame
    f = E.kp_metrics_device(t["kps_gt"], t["kps_pred"], 0.05 * img, mv, img_size=img, want_cam=True, device=gpu_device)
    g = E.kp_metrics_device(t["kps_gt"], px, 0.05 * img, mv, img_size=0, want_cam=True, device=gpu_device)
    for a, b in zip(f, g):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    _rel(name + "/cam", f[3].cpu().numpy(), t["cam"])
    # NaN is a result here, not an error
    torch.cuda.synchronize()
    assert _lib.load().hmmr_run_flags(C.byref(flags), 0) == 0 and not (flags.value & _lib.FLAG_NAN)
    # the single-frame function of the reference
    vis = t["kps_gt"][20, :, 2] != 0
    new_got, cam = E.compute_opt_cam_with_vis(px[20], t["kps_gt"][20, :, :2], vis, device=gpu_device)
    _rel(name + "/cam[20]", cam, t["cam"][20])
    assert np.abs(new_got - EO.opt_cam(px[20], t["kps_gt"][20, :, :2], vis)[0]).max() < 1e-4


def test_strided_joints_equal_the_contiguous_call(ref, gpu_device):
    import torch
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.evaluation import eval as ev, eval_util as E
    t = _tube(ref, "k25")
    pred = torch.as_tensor(t["joints_pred"], device=gpu_device)                    # [n,25,3]
    gt = torch.as_tensor(t["gt3ds"], device=gpu_device)
    view = pred[:, :14]
    assert not view.is_contiguous()
    got = ev._joint_metrics_ld(gt, view, gpu_device, want_err=True)
    assert E._rows(view, gpu_device, (3,))[0].data_ptr() == pred.data_ptr()      # read in place
    want = E._joint_metrics(gt, view.contiguous(), gpu_device)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def _rotation_cases():
    rng = np.random.default_rng(7)
    axes = rng.normal(size=(64, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    axes = np.concatenate([axes, np.eye(3), -np.eye(3)])
    angles = np.concatenate([[0.0, 1e-8, np.pi - 1e-6, np.pi, 1e-4, np.pi / 2, np.pi - 1e-3], np.linspace(0, np.pi, 33)])
    w = (angles[:, None, None] * axes[None]).reshape(-1, 3)
    w = np.concatenate([w, w[:-len(w) % 24]])                                   # whole frames of 24 joints: no case is dropped
    return EO.rodrigues64(w).astype(np.float32), w


def test_rotation_log_and_exp_maps(gpu_device):
    from oracle import hmmr_oracle as O
    import torch
    from human_dynamics_amd.evaluation import eval_util as E
    R32, w_true = _rotation_cases()
    assert len(R32) % 24 == 0
    R32 = R32.reshape(-1, 24, 3, 3)
    got = np.concatenate([E.rot_mat_to_axis_angle(r, device=gpu_device).reshape(24, 3) for r in R32[:2]])
    all_w = E.rotmat_to_aa_device(R32, gpu_device).cpu().numpy().reshape(-1, 3)
    assert np.array_equal(got, all_w[:48])
    err = np.abs(EO.rodrigues64(all_w) - R32.reshape(-1, 3, 3).astype(np.float64)).reshape(len(all_w), -1).max(1)
    norm = np.linalg.norm(all_w.astype(np.float64), axis=1)
    print("log map: max |Rodrigues64(w) - R| = %.3e over %d rotations, max |w| / pi - 1 = %.3e" % (err.max(), len(err), norm.max() / np.pi - 1))
    assert err.max() <= 1.2e-6 and norm.max() <= np.pi * (1 + 2.0 ** -23)
    # a strided input: the poses of a packed record
    rec = torch.zeros((R32.shape[0], 300), device=gpu_device)
    rec[:, 40:40 + 216] = torch.as_tensor(R32.reshape(-1, 216), device=gpu_device)
    view = rec[:, 40:40 + 216].reshape(-1, 24, 3, 3)
    assert np.array_equal(E.rotmat_to_aa_device(view, gpu_device).cpu().numpy().reshape(-1, 3), all_w)
    # the exp map is the SMPL kernel's Rodrigues: batch_rodrigues of the oracle
    aa = np.random.default_rng(3).normal(0, 0.8, (5, 72)).astype(np.float32)
    back = np.stack([E.axis_angle_to_rot_mat(a, device=gpu_device) for a in aa])
    want = O.batch_rodrigues(torch.as_tensor(aa.reshape(-1, 3), dtype=torch.float64)).numpy().reshape(5, 24, 3, 3)
    _abs("axis_angle_to_rot_mat", back, want, 1e-6)


def _data(t):
    return {"images": np.zeros((len(t["kps_gt"]), 224, 1, 1), np.uint8), "kps": t["kps_gt"], "gt3ds": t["gt3ds"], "poses": t["poses_gt"],
            "shape": t["shape_gt"]}


def _preds(t):
    return {"kps": t["kps_pred"], "joints": t["joints_pred"], "poses": t["poses_pred"], "shapes": t["shapes_pred"]}


def test_compute_errors_batched_and_the_sequence_drivers(ref, engine, tmp_path):
    from human_dynamics_amd.evaluation import eval as ev
    mv, dt = int(ref["min_visible"]), int(ref["delta_t"])
    quiet = contextlib.redirect_stdout(io.StringIO())
    worst = 0.0
    for name, k, mesh in (("k25", 25, True), ("k19", 19, False)):
        t = _tube(ref, name)
        got = ev.compute_errors_batched(t["kps_gt"], t["kps_pred"], t["gt3ds"], t["joints_pred"][:, :14], t["poses_gt"], t["poses_pred"],
                                        t["shape_gt"], t["shapes_pred"], img_size=224, has_3d=True, min_visible=mv, compute_mesh=mesh,
                                        engine=engine)
        worst = max(worst, _check_errors(name + "/batched", got, _sub(ref, name + "/batched/"), k))
        with quiet:
            seq = ev.test_sequence(_data(t), _preds(t), str(tmp_path / (name + "a.pkl")), has_3d=True, min_visible=mv, compute_mesh=mesh,
                                   engine=engine)
            seq2 = ev.test_sequence(_data(t), _preds(t), str(tmp_path / (name + "b.pkl")), has_3d=False, min_visible=mv)
        worst = max(worst, _check_errors(name + "/sequence", seq, _sub(ref, name + "/sequence/"), k))
        _check_errors(name + "/sequence_2d", seq2, _sub(ref, name + "/sequence_2d/"), k)
    t = _tube(ref, "k25")
    hal = {"kps_hal": t["kps_hal"], "joints_hal": t["joints_hal"], "poses_hal": np.stack([t["poses_pred"]] * 3, 1),
           "shapes_hal": np.stack([t["shapes_pred"]] * 3, 1), "cams": np.zeros((64, 3), np.float32)}
    with quiet:
        got = ev.test_sequence(_data(t), hal, str(tmp_path / "hal.pkl"), pred_mode="hal", has_3d=True, min_visible=mv, compute_mesh=True,
                               engine=engine)
        const = ev.test_sequence_const(_data(t), hal, str(tmp_path / "const.pkl"), has_3d=True, min_visible=mv, delta_t=dt, engine=engine)
    worst = max(worst, _check_errors("k25/sequence_hal", got, _sub(ref, "k25/sequence_hal/"), 25))
    assert list(const) == ["past", "past_const", "present", "future", "future_const"]
    for part, errors in const.items():
        _check_errors("k25/const/" + part, errors, _sub(ref, "k25/const/%s/" % part), 25)
    print("mesh entries: max |got - ref| = %.3e m" % worst)


def _tester(gpu_device, weights, smpl_consts):
    from human_dynamics_amd.evaluation.tester import Tester
    return Tester(Config(batch_size=1), weights=weights, smpl=smpl_consts, dtype="f32", device=gpu_device)


def _window_records(tester, golden_window):
    import torch
    return tester.predict_records(torch.as_tensor(golden_window["strips"], device=tester.engine.device))


def _window_truth(n, seed=11):
    rng = np.random.default_rng(seed)
    kps = np.concatenate([rng.uniform(40, 180, (n, 25, 2)), (rng.uniform(size=(n, 25, 1)) < 0.8)], axis=2).astype(np.float32)
    kps[0, :, 2] = 0
    kps[1, 3:, 2] = 0
    return {"kps": kps, "gt3ds": rng.normal(0, 0.3, (n, 14, 3)).astype(np.float32), "poses": rng.normal(0, 0.3, (n, 72)).astype(np.float32),
            "shape": rng.normal(0, 1, 10).astype(np.float32)}


def _same(a, b):
    assert sorted(set(a) - {"_device"}) == sorted(set(b) - {"_device"})       # '_device' is the keep_device extra, not a result
    for k in a:
        if k != "_device":
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_score_records_equals_the_unpacked_dictionary(gpu_device, weights, smpl_consts, golden_window):
    import torch
    from human_dynamics_amd.dist import unpack_outputs
    from human_dynamics_amd.evaluation import eval as ev
    tester = _tester(gpu_device, weights, smpl_consts)
    rec = _window_records(tester, golden_window)
    layout, _ = tester.record_layout()
    n = rec.shape[0]
    data = _window_truth(n)
    got = ev.score_records(rec, layout, data, has_3d=True, min_visible=6, compute_mesh=True, engine=tester.engine, keep_device=True)
    host = {k: v.cpu().numpy() for k, v in unpack_outputs(rec, layout).items()}
    want = ev.compute_errors_batched(data["kps"], host["kps"], data["gt3ds"], host["joints"][:, :14], data["poses"], host["poses"],
                                     data["shape"], host["shapes"], has_3d=True, min_visible=6, compute_mesh=True, engine=tester.engine)
    _same(got, want)                                                             # bit for bit
    assert np.isnan(got["kp"][0]) and np.isfinite(got["kp"][2:]).all() and len(got["mesh_posed"]) < n
    # the mesh errors were read from device buffers of n floats: no mesh, and no record, came to the host
    vis = np.sum(data["kps"][:, :14, 2], axis=1) > 6
    for key in ("mesh_posed", "mesh_tpose"):
        buf = got["_device"][key]
        assert isinstance(buf, torch.Tensor) and buf.is_cuda and tuple(buf.shape) == (n,) and buf.dtype == torch.float32
        assert np.array_equal(buf.cpu().numpy().astype(np.float64)[vis], got[key])
    # against the float64 restatement on the downloaded dictionary (the old way), with the oracle's SMPL
    from oracle import hmmr_oracle as O
    old = EO.score_old_way(host, data, lambda p, s: O.smpl_forward(s, p, smpl_consts)[0].numpy(), min_visible=6)
    got.pop("_device")
    _check_errors("records", got, {k: np.asarray(v, np.float64) for k, v in old.items()}, 25)


def test_scoring_beside_the_resnet_is_bit_identical(gpu_device, weights, smpl_consts, golden_window):
    """The condition under which the packed-fp32 fault of DESIGN 4.6 showed: the scoring kernels on a side stream while ResNet
    kernels occupy another.  One repetition."""
    import torch
    from human_dynamics_amd.evaluation import eval as ev
    tester = _tester(gpu_device, weights, smpl_consts)
    rec = _window_records(tester, golden_window)
    layout, _ = tester.record_layout()
    data = _window_truth(rec.shape[0])
    score = lambda: ev.score_records(rec, layout, data, has_3d=True, min_visible=6, compute_mesh=True, engine=tester.engine)
    quiet = score()
    torch.cuda.synchronize()
    from human_dynamics_amd import assets
    frames = torch.as_tensor(assets.make_synthetic_frames(120, seed=5), device=gpu_device)             # 120 frames of ResNet
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    tester.engine.resnet(frames, ws_key="busy")
    with torch.cuda.stream(side):
        busy = score()
    torch.cuda.synchronize()
    _same(quiet, busy)
