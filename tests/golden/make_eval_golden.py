"""Golden vectors for the device evaluation path (human_dynamics_amd/evaluation/eval.py, eval_util.py), produced by EXECUTING the
reference's own code:

  reference_eval.npz   two tubes of 64 frames (k = 25 with 3D ground truth and meshes, k = 19), their inputs and
      * compute_error_kp and compute_opt_cam_with_vis of src/evaluation/eval_util.py, imported with a stand-in cv2;
      * compute_errors_batched, test_sequence ('pred' and 'hal') and test_sequence_const of src/evaluation/eval.py: the module
        needs TensorFlow and absl, so the three functions are lifted out of its source with `ast` and executed in a namespace
        that holds the executed eval_util functions and a compute_gpu_smpl made of oracle.hmmr_oracle.smpl_forward in float64
        on assets.make_synthetic_smpl(2);
      * the accumulators and print_summary on the stub tubes of tests/eval_oracle.py, in the order of main()'s loops.
    cv2.Rodrigues is the float64 log map of tests/eval_oracle.py; np.float = float is set in this process only (NumPy dropped
    the alias compute_opt_cam_with_vis uses).

Arithmetic: the device contract is float64 arithmetic on float32 inputs, so the reference's functions get float64 copies of the
float32 inputs (as make_metrics_edges_golden.py does).  The one exception is the reference's own float32 step: kps_pred stays
float32 into compute_errors_batched, whose `(kps_pred + 1) * 0.5 * img_size` is then three float32 operations; the float32 result
is widened before compute_error_kp (otherwise NumPy would sum the prediction's column means in float32).

The frame where the prediction equals the ground truth is a small figure in the image corner: its aligned error is the
regulariser's residue, 1e-6 / sum(x^2) of the figure's extent, and only for a small figure near the origin does that stand seven
digits above float64 rounding of the pixel coordinates.

No visible keypoint's aligned distance may lie within 1e-3 px of alpha, so that PCK is a count rounding cannot flip.  The maker
checks this for every slice that is scored and, where a seed's tubes miss it, goes on to the next seed (up to 64 of them) rather
than stopping: the stored fixture satisfies the property, and 'seed' in the file is the seed that did.
Only inputs and results are stored (poses and shapes, no meshes).

    python tests/golden/make_eval_golden.py [reference tree]
"""
import ast
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_oracle as EO                                   # noqa: E402
from human_dynamics_amd import assets                      # noqa: E402
from oracle import hmmr_oracle as O                        # noqa: E402

N, MIN_VISIBLE, IMG, DELTA_T, SEED = 64, 6, 224, 5, 31
LIFTED = ("compute_errors_batched", "test_sequence", "test_sequence_const", "print_summary")


def reference_functions():
    np.float = float                                       # this process only
    cv2 = types.ModuleType("cv2")
    cv2.Rodrigues = EO.Cv2.Rodrigues
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    try:
        from src.evaluation import eval_util
    finally:
        sys.path.remove(REF)
    smpl = assets.make_synthetic_smpl(2)

    def compute_gpu_smpl(poses, shapes, get_joints=False):
        verts, joints, _ = O.smpl_forward(np.asarray(shapes, np.float64), np.asarray(poses, np.float64), smpl)
        return (verts.numpy(), joints.numpy()) if get_joints else verts.numpy()

    def compute_error_kp(kps_gt, kps_pred, **kw):          # the float32 image-space prediction, widened (see the docstring)
        return eval_util.compute_error_kp(kps_gt=np.asarray(kps_gt, np.float64), kps_pred=np.asarray(kps_pred, np.float64), **kw)

    ns = {k: getattr(eval_util, k) for k in dir(eval_util) if not k.startswith("_")}
    ns.update(compute_gpu_smpl=compute_gpu_smpl, compute_error_kp=compute_error_kp, np=np, os=os, time=__import__("time").time,
              pickle=__import__("pickle"), config=types.SimpleNamespace(delta_t=DELTA_T))
    tree = ast.parse(open(os.path.join(REF, "src", "evaluation", "eval.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in LIFTED]
    assert sorted(n.name for n in body) == sorted(LIFTED)
    exec(compile(ast.Module(body=body, type_ignores=[]), "eval.py", "exec"), ns)
    return eval_util, ns, compute_gpu_smpl


def make_tube(rng, k, corner_frame=True):
    """float32 inputs of one tube with the visibility cases the kernels must honour."""
    gt_px = rng.uniform(30, 194, (N, 1, 2)) + rng.normal(0, 22, (N, k, 2))
    noise = rng.normal(0, 1, (N, k, 2)) * rng.choice([1.5, 4.0, 9.0], (N, 1, 1))
    vis = (rng.uniform(size=(N, k)) < 0.8).astype(np.float32)
    vis[:, :9] = 1.0                                                  # ordinary frames: at least 9 visible, all inside the first 14
    def only(f, cols):
        vis[f] = 0.0
        vis[f, list(cols)] = 1.0
    only(0, ())                                                       # no visible keypoint
    only(1, range(2, 2 + MIN_VISIBLE - 1))                            # min_visible - 1
    only(2, range(k - MIN_VISIBLE, k))                                # exactly min_visible, the last ones (k = 19: one of the 14)
    only(3, range(3, 3 + MIN_VISIBLE + 1))                            # min_visible + 1
    only(4, list(range(MIN_VISIBLE)) + [15, 16])                      # 14-joint sum == min_visible: the frame is not visible in 3D
    only(5, list(range(MIN_VISIBLE + 1)) + [17])                      # 14-joint sum == min_visible + 1
    vis[6, :8] = [0.5, 2.0, 0.25, 3.0, 1.0, 0.5, 0.5, 0.25]           # visibility values other than 0 and 1 (sum 8)
    vis[6, 8:] = 0.0
    vis[9] = vis[10] = 0.0                                            # two adjacent invisible frames: the acceleration stencil
    vis[9, :3] = vis[10, :3] = 1.0
    pred = ((gt_px + noise) / (0.5 * IMG) - 1).clip(-1, 1).astype(np.float32)
    if corner_frame:                                                  # frame 7: the prediction IS the ground truth
        pred[7] = (rng.uniform(1, 15, (k, 2)) / (0.5 * IMG) - 1).astype(np.float32)
    gt = np.concatenate([gt_px, vis[..., None]], axis=2).astype(np.float32)
    gt[7, :, :2] = EO.to_image_space32(pred[7], IMG)
    vis[7] = gt[7, :, 2] = 1.0
    assert np.abs(pred).max() <= 1
    out = {"kps_gt": gt, "kps_pred": pred}
    # 3D: ground-truth joints, predicted joints (k of them, the first 14 are scored), poses, shapes
    j_gt = rng.normal(0, 0.3, (N, 14, 3)).cumsum(0) * 0.05 + rng.normal(0, 0.3, (1, 14, 3))
    j_pred = np.concatenate([j_gt + rng.normal(0, 0.03, j_gt.shape), rng.normal(0, 0.3, (N, k - 14, 3))], axis=1)
    poses_gt = rng.normal(0, 0.35, (N, 72))
    poses_gt[11, 3:6] = [np.pi - 1e-4, 0, 0]                          # a joint half a turn about: the log map's far end
    poses_pred = EO.rodrigues64((poses_gt + rng.normal(0, 0.05, (N, 72))).reshape(N, 24, 3))
    out.update(gt3ds=j_gt.astype(np.float32), joints_pred=j_pred.astype(np.float32), poses_gt=poses_gt.astype(np.float32),
               poses_pred=poses_pred.astype(np.float32), shape_gt=rng.normal(0, 1, 10).astype(np.float32),
               shapes_pred=rng.normal(0, 1, (N, 10)).astype(np.float32))
    return out


def hal_preds(t, rng):
    """The '_hal' containers [N, 3, ...]: kps and joints differ per container (stored), poses and shapes are the tube's (rebuilt)."""
    kps = np.stack([(t["kps_pred"] + rng.normal(0, s, t["kps_pred"].shape)).clip(-1, 1) for s in (0.02, 0.0, 0.03)], 1)
    joints = np.stack([t["joints_pred"] + rng.normal(0, s, t["joints_pred"].shape) for s in (0.02, 0.0, 0.04)], 1)
    return kps.astype(np.float32), joints.astype(np.float32)


def hal_dict(t, kps_hal, joints_hal):
    return {"kps_hal": kps_hal, "joints_hal": joints_hal, "poses_hal": np.stack([t["poses_pred"]] * 3, 1),
            "shapes_hal": np.stack([t["shapes_pred"]] * 3, 1), "cams": np.zeros((N, 3), np.float32)}


def data_dict(t, f64=True):
    c = (lambda a: np.asarray(a, np.float64)) if f64 else (lambda a: a)
    return {"images": np.zeros((N, IMG, 1, 1), np.uint8), "kps": c(t["kps_gt"]), "gt3ds": c(t["gt3ds"]), "poses": c(t["poses_gt"]),
            "shape": c(t["shape_gt"])}


def preds_dict(t):
    """float64 copies of everything but kps (float32: the reference's own float32 step)."""
    return {"kps": t["kps_pred"], "joints": t["joints_pred"].astype(np.float64), "poses": t["poses_pred"].astype(np.float64),
            "shapes": t["shapes_pred"].astype(np.float64)}


def flat(prefix, errors, out):
    for k, v in errors.items():
        if isinstance(v, dict):
            flat(prefix + k + "/", v, out)
        else:
            out[prefix + k] = np.asarray(v, np.float64)


class TooCloseToAlpha(Exception):
    pass


def margin(d, alpha):
    if not np.abs(d - alpha).min() > 1e-3:
        raise TooCloseToAlpha(np.abs(d - alpha).min())


def build(eval_util, ns, seed):
    rng = np.random.default_rng(seed)
    out = {"min_visible": np.array(MIN_VISIBLE), "img_size": np.array(IMG), "delta_t": np.array(DELTA_T)}
    quiet = contextlib.redirect_stdout(io.StringIO())
    for name, k, mesh in (("k25", 25, True), ("k19", 19, False)):
        t = make_tube(rng, k)
        for key, v in t.items():
            out[name + "/" + key] = v
        px = EO.to_image_space32(t["kps_pred"], IMG).astype(np.float64)
        gt64 = t["kps_gt"].astype(np.float64)
        alpha = 0.05 * IMG
        d = EO.aligned_distances(gt64, px)
        margin(d, alpha)
        e, epa, pck = eval_util.compute_error_kp(gt64, px, alpha=alpha, min_visible=MIN_VISIBLE)
        out[name + "/kp"], out[name + "/kp_pa"], out[name + "/kp_pck"] = np.array(e), np.array(epa), np.array(pck)
        assert np.array_equal(np.isnan(e), (gt64[:, :, 2] != 0).sum(1) < MIN_VISIBLE) and np.isnan(e).sum() == 4
        cams = np.full((N, 3), np.nan)
        for f in range(N):
            vis = gt64[f, :, 2].astype(bool)
            if vis.any() and vis.sum() >= MIN_VISIBLE:
                cams[f] = eval_util.compute_opt_cam_with_vis(got=px[f], want=gt64[f, :, :2], vis=vis)[1]
        out[name + "/cam"] = cams
        print("%s: equal frame kp %.3e kp_pa %.3e" % (name, e[7], epa[7]))
        with tempfile.TemporaryDirectory() as tmp, quiet:
            data, preds = data_dict(t), preds_dict(t)
            flat(name + "/batched/", ns["compute_errors_batched"](
                kps_gt=data["kps"], kps_pred=preds["kps"], joints_gt=data["gt3ds"], joints_pred=preds["joints"][:, :14],
                poses_gt=data["poses"], poses_pred=preds["poses"], shape_gt=data["shape"], shapes_pred=preds["shapes"],
                img_size=IMG, has_3d=True, min_visible=MIN_VISIBLE, compute_mesh=mesh), out)
            flat(name + "/sequence/", ns["test_sequence"](data, preds, os.path.join(tmp, "a.pkl"), "pred", True, MIN_VISIBLE, mesh), out)
            flat(name + "/sequence_2d/", ns["test_sequence"](data, preds, os.path.join(tmp, "b.pkl"), "pred", False, MIN_VISIBLE, False), out)
            if mesh:
                kps_hal, joints_hal = hal_preds(t, rng)
                out[name + "/kps_hal"], out[name + "/joints_hal"] = kps_hal, joints_hal
                hal = hal_dict(t, kps_hal, joints_hal)
                hal = {kk: (v if kk == "kps_hal" else v.astype(np.float64)) for kk, v in hal.items()}
                px_hal = EO.to_image_space32(kps_hal, IMG).astype(np.float64)
                for c in range(3):
                    for g, p in ((slice(None), slice(None)), (slice(None, -DELTA_T), slice(DELTA_T, None)),
                                 (slice(DELTA_T, None), slice(None, -DELTA_T))):
                        dd = EO.aligned_distances(gt64[g], px_hal[p, c])
                        margin(dd, alpha)
                flat(name + "/sequence_hal/", ns["test_sequence"](data, hal, os.path.join(tmp, "c.pkl"), "hal", True, MIN_VISIBLE, True), out)
                flat(name + "/const/", ns["test_sequence_const"](data, hal, os.path.join(tmp, "d.pkl"), True, MIN_VISIBLE), out)
                # the cache: a second call returns what the file holds, whatever the predictions are
                again = ns["test_sequence"](data, None, os.path.join(tmp, "a.pkl"), "pred", True, MIN_VISIBLE, mesh)
                assert np.array_equal(again["kp"], out[name + "/sequence/kp"], equal_nan=True)
    # ---- the single-frame utilities on frame 12 of the k25 tube: points as rows (the transposed path) and as columns
    j_gt, j_pred = out["k25/gt3ds"][12].astype(np.float64), out["k25/joints_pred"][12, :14].astype(np.float64)
    out["single/aligned"], out["single/pelvis"] = eval_util.align_by_pelvis(j_pred, get_pelvis=True)
    assert np.array_equal(eval_util.align_by_pelvis(j_pred), out["single/aligned"])
    out["single/procrustes_rows"] = eval_util.compute_similarity_transform(j_pred, j_gt)
    out["single/procrustes_cols"] = eval_util.compute_similarity_transform(j_pred.T.copy(), j_gt.T.copy())
    # ---- the accumulation of main() on stub tubes, with the reference's accumulators and print_summary
    for mode in ("pred", "const"):
        keys = ("past", "past_const", "present", "future", "future_const")
        nest = (lambda: {k: {} for k in keys}) if mode == "const" else dict
        results = nest()
        for dataset, tubes in EO.stub_tubes().items():
            dataset_result, by_path = nest(), {}
            for tf_path, p_id, seed in tubes:
                path_result = by_path.setdefault(tf_path, nest())
                has_3d = dataset in ("3dpw", "h36m")
                if mode == "const":
                    for i, k in enumerate(keys):
                        eval_util.extend_dict_entries(path_result[k], EO.stub_errors(100 * i + seed, has_3d))
                else:
                    eval_util.extend_dict_entries(path_result, EO.stub_errors(seed, has_3d))
            for path_result in by_path.values():
                if mode == "const":
                    for k in keys:
                        eval_util.update_dict_entries(dataset_result[k], path_result[k])
                else:
                    eval_util.update_dict_entries(dataset_result, path_result)
            if mode == "const":
                for k, result in dataset_result.items():
                    eval_util.mean_of_dict_values(result)
                    results[k][dataset] = result
            else:
                eval_util.mean_of_dict_values(dataset_result)
                results[dataset] = dataset_result
        out["accumulated_" + mode] = np.array(json.dumps(results, sort_keys=True))
        if mode == "pred":
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ns["print_summary"](results)
            out["summary_pred"] = np.array(buf.getvalue())
    s = EO.stub_errors(3, True)
    cat = {"a": [s["accel"], s["mesh_posed"]], "b": [np.array(s["kp"])]}
    eval_util.concat_dict_entries(cat)
    out["concat/a"], out["concat/b"] = cat["a"], cat["b"]
    return out


def main():
    eval_util, ns, _ = reference_functions()
    for seed in range(SEED, SEED + 64):          # the first seed whose tubes keep every aligned distance 1e-3 px away from alpha
        try:
            out = build(eval_util, ns, seed)
            break
        except TooCloseToAlpha as e:
            print("seed %d: an aligned distance lies %.2e px from alpha, next seed" % (seed, e.args[0]))
    out["seed"] = np.array(seed)
    path = os.path.join(HERE, "reference_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
