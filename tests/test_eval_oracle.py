"""The evaluation drivers without a device: the float64 restatement (tests/eval_oracle.py) against the fixture the reference's own
code produced (tests/golden/make_eval_golden.py), the accumulation and caching of evaluation/eval.py with stub metric values, and
the argument checks of the new entry points."""
import contextlib
import io
import json
import os
import pickle
import types

import numpy as np
import pytest

import eval_oracle as EO
from conftest import GOLDEN


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_eval.npz")))


def _tube(ref, name):
    return {k[len(name) + 1:]: v for k, v in ref.items() if k.startswith(name + "/") and k.count("/") == 1}


def _close(got, want, tol=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if got.size:
        assert np.nanmax(np.abs(got - want), initial=0.0) <= tol, np.nanmax(np.abs(got - want))


@pytest.mark.parametrize("name", ["k25", "k19"])
def test_restated_keypoint_metrics_match_the_reference(ref, name):
    t = _tube(ref, name)
    img, mv = int(ref["img_size"]), int(ref["min_visible"])
    px = EO.to_image_space32(t["kps_pred"], img)
    e, epa, pck, cam = EO.compute_error_kp(t["kps_gt"], px, 0.05 * img, mv, with_cam=True)
    _close(e, t["kp"]), _close(epa, t["kp_pa"]), _close(pck, t["kp_pck"]), _close(cam, t["cam"])
    # the cases the fixture must hold: NaN frames, the boundary counts, odd visibility values, the equal frame
    nvis = (t["kps_gt"][:, :, 2] != 0).sum(1)
    assert nvis[0] == 0 and list(nvis[1:4]) == [mv - 1, mv, mv + 1] and np.isnan(t["kp"][[0, 1]]).all() and np.isfinite(t["kp"][[2, 3]]).all()
    assert t["kps_gt"][4, :14, 2].sum() == mv and t["kps_gt"][5, :14, 2].sum() == mv + 1
    assert set(np.unique(t["kps_gt"][6, :, 2])) - {0.0, 1.0}
    assert t["kp"][7] == 0.0 and 0.0 < t["kp_pa"][7] < 1e-6
    assert len(t["kp"]) >= 64 and np.abs(t["kps_pred"]).max() <= 1.0


@pytest.mark.parametrize("name,mesh", [("k25", True), ("k19", False)])
def test_restated_compute_errors_batched_matches_the_reference(ref, smpl_consts, name, mesh):
    from oracle import hmmr_oracle as O
    t = _tube(ref, name)
    smpl = lambda poses, shapes: O.smpl_forward(shapes, poses, smpl_consts)[0].numpy()
    got = EO.compute_errors_batched(t["kps_gt"], t["kps_pred"], t["gt3ds"], t["joints_pred"][:, :14], t["poses_gt"], t["poses_pred"],
                                    t["shape_gt"], t["shapes_pred"], int(ref["img_size"]), True, int(ref["min_visible"]), mesh, smpl)
    want = {k.split("/")[-1]: v for k, v in ref.items() if k.startswith(name + "/batched/")}
    assert sorted(got) == sorted(want) == sorted(["accel", "kp", "kp_pa", "kp_pck", "accel_error", "mesh_posed", "mesh_tpose", "pose",
                                                   "joints", "joints_pa", "shape"])
    for k in want:
        _close(got[k], want[k])
    assert got["pose"] == -1 and got["shape"] == -1 and (mesh or (got["mesh_posed"] == -1 and got["mesh_tpose"] == -1))
    # test_sequence is compute_errors_batched on the tube's own keys
    for k, v in want.items():
        _close(ref[name + "/sequence/" + k], v, 0.0)


def test_single_frame_utilities_match_the_reference(ref):
    """align_by_pelvis and compute_similarity_transform (host NumPy in the reference too) on frame 12 of the k25 tube."""
    from human_dynamics_amd.evaluation import eval_util as E
    j_gt, j_pred = ref["k25/gt3ds"][12].astype(np.float64), ref["k25/joints_pred"][12, :14].astype(np.float64)
    aligned, pelvis = E.align_by_pelvis(j_pred, get_pelvis=True)
    _close(aligned, ref["single/aligned"]), _close(pelvis, ref["single/pelvis"]), _close(E.align_by_pelvis(j_pred), ref["single/aligned"])
    _close(E.compute_similarity_transform(j_pred, j_gt), ref["single/procrustes_rows"])              # points as rows: transposed
    _close(E.compute_similarity_transform(j_pred.T.copy(), j_gt.T.copy()), ref["single/procrustes_cols"])
    assert ref["single/procrustes_rows"].shape == (14, 3) and ref["single/procrustes_cols"].shape == (3, 14)


def test_rotation_maps_invert_each_other():
    """A check of the oracle itself (the stand-in cv2.Rodrigues of the fixture maker and the yardstick of the device log map):
    it does not touch the package."""
    rng = np.random.default_rng(0)
    axes = rng.normal(size=(40, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    for angle in (0.0, 1e-8, 1e-3, 1.0, np.pi / 2, 2.0, np.pi - 1e-6, np.pi):
        w = EO.log_map64(EO.rodrigues64(axes * angle))
        assert np.abs(EO.rodrigues64(w) - EO.rodrigues64(axes * angle)).max() < 1e-9
        assert np.linalg.norm(w, axis=1).max() <= np.pi * (1 + 1e-15)


# ---- eval.py without a device: stub metric values --------------------------------------------------------------------------------
class _StubModel(object):
    engine = None

    def predict_all_images(self, frames):
        n = len(frames)
        out = {"kps": np.zeros((n, 25, 2), np.float32), "joints": np.zeros((n, 25, 3), np.float32),
               "poses": np.zeros((n, 24, 3, 3), np.float32), "shapes": np.zeros((n, 10), np.float32), "verts": np.zeros((n, 4, 3), np.float32)}
        out.update({k + "_hal": np.stack([v] * 3, 1) for k, v in list(out.items())})
        return out


def _stub_data(seed):
    return {"images": np.full((12, 224, 2, 3), seed % 200, np.uint8), "kps": np.full((12, 25, 3), float(seed)), "gt3ds": np.zeros((12, 14, 3)),
            "poses": np.zeros((12, 72)), "shape": np.zeros(10)}


@pytest.mark.parametrize("mode", ["pred", "const"])
def test_evaluate_accumulates_like_main(ref, tmp_path, monkeypatch, mode):
    from human_dynamics_amd.evaluation import eval as ev
    keys = list(ev.CONST_KEYS)
    calls = []

    def fake_errors(kps_gt, **kw):                       # the tube's seed travels in its ground truth
        seed = int(np.asarray(kps_gt).flat[0])
        calls.append((seed, kw["has_3d"], kw.get("compute_mesh", False), kw["min_visible"]))
        i = (len([c for c in calls if c[0] == seed]) - 1) if mode == "const" else 0
        order = ["present", "past", "past_const", "future", "future_const"]      # the order test_sequence_const computes them in
        return EO.stub_errors(100 * keys.index(order[i]) + seed if mode == "const" else seed, kw["has_3d"])

    monkeypatch.setattr(ev, "compute_errors_batched", fake_errors)
    cfg = types.SimpleNamespace(load_path="models/stub.ckpt-1", pred_mode=mode, pred_dir=str(tmp_path / "cache"), min_visible=6,
                                split="test", delta_t=int(ref["delta_t"]))
    datasets = {d: [(p, i, _stub_data(seed)) for p, i, seed in tubes] for d, tubes in EO.stub_tubes(str(tmp_path / "tf")).items()}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = ev.evaluate(_StubModel(), cfg, datasets)
    want = json.loads(str(ref["accumulated_" + mode]))
    assert got == want
    if mode == "const":
        assert sorted(got) == sorted(keys) and all(sorted(v) == sorted(EO.STUB_DATASETS) for v in got.values())
    else:
        assert out.getvalue().endswith(str(ref["summary_pred"]))
        # the mesh errors only on the 3DPW test split; 3D metrics only on the 3D datasets; one call per tube
        assert [c[1:3] for c in calls] == [(True, True)] * 3 + [(False, False)] * 3
        # both caches were written: a second run recomputes nothing
        calls.clear()
        with contextlib.redirect_stdout(io.StringIO()):
            assert ev.evaluate(_StubModel(), cfg, datasets) == want
        assert calls == []
    path = ev.get_result_path_name(split="test", load_path=cfg.load_path, pred_mode=mode, datasets=list(datasets), pred_dir=cfg.pred_dir)
    assert json.load(open(path)) == want


def test_accumulators_match_the_reference(ref):
    from human_dynamics_amd.evaluation import eval_util as E
    s = EO.stub_errors(3, True)
    cat = {"a": [s["accel"], s["mesh_posed"]], "b": [np.array(s["kp"])]}
    E.concat_dict_entries(cat)
    _close(cat["a"], ref["concat/a"], 0.0), _close(cat["b"], ref["concat/b"], 0.0)
    acc = {}
    E.extend_dict_entries(acc, {"x": [1.0, 2.0], "y": -1})
    E.extend_dict_entries(acc, {"x": np.array([3.0]), "y": -1})
    assert acc == {"x": [1.0, 2.0, 3.0], "y": [-1, -1]}
    upd = {}
    E.update_dict_entries(upd, acc)
    E.update_dict_entries(upd, {"x": [np.nan, 5.0]})
    assert len(upd["x"]) == 2 and upd["y"] == [[-1, -1]]
    E.mean_of_dict_values(upd)
    assert upd == {"x": 3.5, "y": -1.0}


def test_sequence_cache_and_hal_keys(tmp_path, monkeypatch):
    from human_dynamics_amd.evaluation import eval as ev
    seen = {}

    def fake_errors(**kw):
        seen.update(kw)
        return {"kp": [1.0, np.nan], "accel": np.array([0.5])}

    monkeypatch.setattr(ev, "compute_errors_batched", fake_errors)
    data = _stub_data(1)
    preds = {"kps": np.zeros((4, 25, 2)), "joints": np.zeros((4, 25, 3)), "poses": np.zeros((4, 24, 3, 3)), "shapes": np.zeros((4, 10))}
    hal = {k + "_hal": np.stack([v + 1, v + 2, v + 3], 1) for k, v in preds.items()}
    hal["cams"] = np.zeros((4, 3))                       # no '_hal' in the key: dropped
    path = str(tmp_path / "eval.pkl")
    with contextlib.redirect_stdout(io.StringIO()):
        got = ev.test_sequence(data, hal, path, pred_mode="hal", has_3d=True, min_visible=4, compute_mesh=True)
    assert (seen["kps_pred"] == 2).all() and seen["kps_pred"].shape == (4, 25, 2)          # the centre container
    assert seen["joints_pred"].shape == (4, 14, 3) and (seen["poses_pred"] == 2).all() and seen["shapes_pred"].shape == (4, 10)
    assert seen["img_size"] == 224 and seen["min_visible"] == 4 and seen["has_3d"] and seen["compute_mesh"]
    assert pickle.load(open(path, "rb"))["kp"][0] == 1.0
    seen.clear()
    with contextlib.redirect_stdout(io.StringIO()):
        again = ev.test_sequence(data, None, path, pred_mode="pred")          # the cache answers, whatever the predictions are
    assert not seen and again["kp"][0] == got["kp"][0] and np.isnan(again["kp"][1])
    # test_sequence_const: five slices of the three containers, shifted by delta_t
    got_calls = []
    monkeypatch.setattr(ev, "compute_errors_batched", lambda **kw: got_calls.append(kw) or {"kp": [float(len(got_calls))]})
    data8 = {"images": np.zeros((8, 224, 1, 1), np.uint8), "kps": np.arange(8.0)[:, None, None] * np.ones((8, 25, 3)),
             "gt3ds": np.zeros((8, 14, 3)), "poses": np.zeros((8, 72)), "shape": np.zeros(10)}
    hal8 = {"kps_hal": np.arange(8.0)[:, None, None, None] + 10 * np.arange(3.0)[None, :, None, None] + np.zeros((8, 3, 25, 2)),
            "joints_hal": np.zeros((8, 3, 25, 3)), "poses_hal": np.zeros((8, 3, 24, 3, 3))}
    with contextlib.redirect_stdout(io.StringIO()):
        out = ev.test_sequence_const(data8, hal8, str(tmp_path / "const.pkl"), has_3d=True, delta_t=3)
    assert list(out) == ["past", "past_const", "present", "future", "future_const"]
    by_name = dict(zip(["present", "past", "past_const", "future", "future_const"], got_calls))
    first = lambda kw: (kw["kps_gt"][0, 0, 0], kw["kps_pred"][0, 0, 0], len(kw["kps_gt"]), kw["joints_pred"].shape[1:])
    assert first(by_name["present"]) == (0.0, 0.0, 8, (14, 3))
    assert first(by_name["past"]) == (0.0, 3.0, 5, (14, 3)) and first(by_name["past_const"]) == (0.0, 13.0, 5, (14, 3))
    assert first(by_name["future"]) == (3.0, 20.0, 5, (14, 3)) and first(by_name["future_const"]) == (3.0, 10.0, 5, (14, 3))
    assert sorted(pickle.load(open(str(tmp_path / "const.pkl"), "rb"))) == sorted(out)


def test_new_entry_points_refuse_bad_arguments():
    """Dummy, never dereferenced pointers: refusal happens before anything is launched, no device is needed."""
    from human_dynamics_amd import _lib
    lib = _lib.load()
    P = [0x1000 * (i + 1) for i in range(8)]

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc != 0 and msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        with pytest.raises(_lib.HmmrError):
            _lib.check(rc, "evaluation")

    def call(fn, names, defaults, kw):
        args = dict(defaults)
        args.update(kw)
        return fn(*[args[a] for a in names.split()])

    kps = lambda **kw: call(lib.hmmr_eval_kps, "gt ldg pred ldp n k alpha mv img e epa pck cam st",
                            dict(gt=P[0], ldg=75, pred=P[1], ldp=50, n=4, k=25, alpha=11.2, mv=6, img=224.0, e=P[2], epa=P[3], pck=P[4],
                                 cam=None, st=None), kw)
    refused(kps(k=33, ldg=99, ldp=66), b"hmmr_eval_kps", b"k <= 32")
    refused(kps(n=0), b"hmmr_eval_kps")
    refused(kps(ldg=74), b"hmmr_eval_kps", b"row strides")
    refused(kps(ldp=49), b"row strides")
    refused(kps(gt=None), b"hmmr_eval_kps", b"without kps_gt")
    refused(kps(pred=None), b"without kps_gt / kps_pred")
    refused(kps(e=None, epa=None, pck=None), b"no output")
    refused(kps(alpha=float("nan")), b"alpha")

    jl = lambda **kw: call(lib.hmmr_eval_joints_ld, "gt ldg pred ldp n k l r mp pa ac ae st",
                           dict(gt=P[0], ldg=42, pred=P[1], ldp=75, n=4, k=14, l=3, r=2, mp=P[2], pa=P[3], ac=None, ae=None, st=None), kw)
    refused(jl(k=33, ldg=99, ldp=99), b"hmmr_eval_joints_ld", b"k <= 32")
    refused(jl(n=0), b"hmmr_eval_joints_ld")
    refused(jl(ldp=41), b"hmmr_eval_joints_ld", b"row strides")
    refused(jl(ldg=41), b"row strides")
    refused(jl(gt=None), b"needs gt")
    refused(jl(l=14), b"hip ids")

    for fn, name, (a, b) in ((lib.hmmr_rotmat_to_axis_angle, b"hmmr_rotmat_to_axis_angle", (216, 72)),
                             (lib.hmmr_axis_angle_to_rotmat, b"hmmr_axis_angle_to_rotmat", (72, 216))):
        f = lambda **kw: call(fn, "src lds n per dst ldd st", dict(src=P[0], lds=a, n=4, per=24, dst=P[1], ldd=b, st=None), kw)
        refused(f(n=0), name)
        refused(f(per=0), name)
        refused(f(lds=a - 1), name, b"row strides")
        refused(f(ldd=b - 1), name, b"row strides")
        refused(f(src=None), name, b"requested without")
        refused(f(dst=None), name, b"no output")
