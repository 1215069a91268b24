"""Golden vectors for the evaluation metrics on degenerate inputs, produced by EXECUTING the reference's own
src/evaluation/eval_util.py (pure NumPy; cv2 is only imported there, a stand-in module satisfies the import):

  reference_metrics_edges.npz   for every family of oracle/metrics_oracle.py (planar / near-planar / collinear /
                                identical / mirrored / scaled / offset / equal singular values): the float32 inputs and
                                the reference's compute_error_3d, compute_accel, compute_error_accel (with and without a
                                visibility mask) and compute_similarity_transform of frame 0; for the families where the
                                reference divides 0 by 0, the inputs and the fact that its result is not finite.

Only inputs and outputs are stored.  The reference tree is not on the GPU box; the tests read the fixture.

    python tests/golden/make_metrics_edges_golden.py
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from oracle import metrics_oracle as MO          # noqa: E402  (only the input generators are used here)

N_FRAMES, K, SEED = 24, 14, 20


def main():
    added = "cv2" not in sys.modules
    if added:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, REF)
    try:
        from src.evaluation import eval_util
    finally:
        sys.path.remove(REF)
        if added:
            del sys.modules["cv2"]
    vis = np.ones(N_FRAMES, bool)
    vis[[0, 9, 10, N_FRAMES - 1]] = False                     # both ends and two adjacent frames in the middle
    out = {"vis": vis.astype(np.float64), "families": np.array(MO.FAMILIES), "nonfinite": np.array(MO.NONFINITE_FAMILIES)}
    for name in MO.FAMILIES:
        gt32, pred32 = MO.family(name, N_FRAMES, K, SEED)
        gt, pred = gt32.astype(np.float64), pred32.astype(np.float64)
        e, epa = eval_util.compute_error_3d(gt, pred)
        assert np.isfinite(e).all() and np.isfinite(epa).all(), name
        out[name + "/gt"], out[name + "/pred"] = gt32, pred32
        out[name + "/mpjpe"], out[name + "/pa_mpjpe"] = np.array(e), np.array(epa)
        out[name + "/accel"] = eval_util.compute_accel(pred)
        out[name + "/accel_err_all"] = eval_util.compute_error_accel(gt, pred)
        out[name + "/accel_err"] = eval_util.compute_error_accel(gt, pred, vis)
        out[name + "/pa_aligned0"] = eval_util.compute_similarity_transform(eval_util.align_by_pelvis(pred[0]),
                                                                            eval_util.align_by_pelvis(gt[0]))
    for name in MO.NONFINITE_FAMILIES:
        gt32, pred32 = MO.family(name, N_FRAMES, K, SEED)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                e, epa = eval_util.compute_error_3d(gt32.astype(np.float64), pred32.astype(np.float64))
                finite = np.isfinite(np.array(epa))
            except Exception:                                  # a refusal counts as "no finite answer" as well
                e, finite = None, np.zeros(N_FRAMES, bool)
        assert not finite.any(), name
        out[name + "/gt"], out[name + "/pred"] = gt32, pred32
        out[name + "/pa_is_finite"] = finite
        if e is not None:
            out[name + "/mpjpe"] = np.array(e)                 # the pelvis-aligned error itself is well defined
    path = os.path.join(HERE, "reference_metrics_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
