"""oracle/metrics_oracle.py (NumPy float64, SVD of K itself) pinned to the reference's own eval_util.py: the generic
fixture tests/golden/reference_metrics.npz to 1e-12 and the degenerate Procrustes families of
tests/golden/reference_metrics_edges.npz (tests/golden/make_metrics_edges_golden.py) to 1e-9.  No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import metrics_oracle as MO


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_metrics.npz")))


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(os.path.join(GOLDEN, "reference_metrics_edges.npz")))


def test_oracle_reproduces_every_array_of_the_generic_fixture(ref):
    vis = ref["vis"].astype(bool)
    e, epa = MO.compute_error_3d(ref["gt"], ref["pred"], vis)
    got = {"mpjpe": e, "pa_mpjpe": epa, "accel": MO.compute_accel(ref["pred"]),
           "accel_err": MO.compute_error_accel(ref["gt"], ref["pred"], vis),
           "verts_err": MO.compute_error_verts(ref["verts_gt"], ref["verts_pred"]),
           "pa_aligned0": MO.similarity_transform(MO.align_by_pelvis(ref["pred"][0]), MO.align_by_pelvis(ref["gt"][0]))}
    assert sorted(got) == sorted(set(ref) - {"gt", "pred", "vis", "verts_gt", "verts_pred"})     # nothing left unpinned
    for k, v in got.items():
        assert v.shape == ref[k].shape, k
        err = np.abs(v - ref[k]).max()
        print("metrics oracle vs reference, %-12s max abs err %.2e" % (k, err))
        assert err < 1e-12, k
    # before the visibility filter: the filtered rows are a subset of the unfiltered ones, at the stencil's positions
    allrows = MO.accel_error_all(ref["gt"], ref["pred"])
    keep = MO.accel_visibility(vis, len(vis))
    assert allrows.shape == (len(vis) - 2,) and np.array_equal(allrows[keep], got["accel_err"])
    assert [bool(k) for k in keep] == [bool(vis[i] and vis[i + 1] and vis[i + 2]) for i in range(len(vis) - 2)]


@pytest.mark.parametrize("name", MO.FAMILIES)
def test_oracle_matches_reference_on_degenerate_family(edges, name):
    assert list(edges["families"]) == list(MO.FAMILIES)
    gt, pred = edges[name + "/gt"], edges[name + "/pred"]
    assert gt.dtype == np.float32 and len(gt) >= 24
    g2, p2 = MO.family(name, len(gt), gt.shape[1], 20)                # the recorded inputs are the generator's
    assert np.array_equal(g2, gt) and np.array_equal(p2, pred)
    vis = edges["vis"].astype(bool)
    e, epa = MO.compute_error_3d(gt, pred)
    got = {"mpjpe": e, "pa_mpjpe": epa, "accel": MO.compute_accel(pred), "accel_err_all": MO.accel_error_all(gt, pred),
           "accel_err": MO.compute_error_accel(gt, pred, vis),
           "pa_aligned0": MO.similarity_transform(MO.align_by_pelvis(pred[0]), MO.align_by_pelvis(gt[0]))}
    for k, v in got.items():
        r = edges[name + "/" + k]
        assert v.shape == r.shape, k
        scale = max(1.0, float(np.abs(r).max()))          # scale_1e3: errors of hundreds of metres, float64 relative
        err = np.abs(v - r).max() / scale
        print("metrics oracle vs reference, %-18s %-13s max err %.2e" % (name, k, err))
        assert err < 1e-9, (name, k)


@pytest.mark.parametrize("name", MO.NONFINITE_FAMILIES)
def test_oracle_is_not_finite_where_the_reference_is_not(edges, name):
    assert not edges[name + "/pa_is_finite"].any()
    with np.errstate(all="ignore"):
        e, epa = MO.compute_error_3d(edges[name + "/gt"], edges[name + "/pred"])
    assert not np.isfinite(epa).any()
    assert np.abs(e - edges[name + "/mpjpe"]).max() < 1e-9


@pytest.mark.parametrize("name", MO.FAMILIES)
def test_conditioning_filter_keeps_95_percent_of_every_family(name):
    """The seeds of the GPU sweep (tests/test_gpu_periphery.py: 256 frames, seed 1) and of the fixture (seed 20), for
    the oracle alone: the near-tie filter may drop at most 5 % of a family."""
    for n, seed in ((256, 1), (24, 20)):
        gt, pred = MO.family(name, n, 14, seed)
        keep = MO.well_conditioned(gt, pred, seed, offset=1000.0 if name == "offset_1000" else 0.0)
        print("%-18s seed %2d: %d of %d frames dropped" % (name, seed, int((~keep).sum()), n))
        assert (~keep).sum() <= 0.05 * n


def test_conditioning_filter_drops_a_rotation_reflection_tie():
    """A frame whose two smallest singular values tie under a reflection has two equally good alignments; the filter
    must see it (otherwise it filters nothing)."""
    rng = np.random.default_rng(0)
    gt = rng.normal(size=(1, 14, 3)) * 0.3
    turn = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    for j in range(12):
        if j % 4:
            gt[0, j] = gt[0, j - 1] @ turn.T                # symmetric about x: X2 X2^T = diag(a, b, b)
    gt[0, 12:, 1:] = 0.0
    pred = gt * np.array([1.0, 1.0, -1.0]) + rng.normal(size=gt.shape) * 1e-6     # mirrored across the tied plane
    assert not MO.well_conditioned(gt.astype(np.float32), pred.astype(np.float32))[0]
    g, p = MO.family("identical", 4)
    assert MO.well_conditioned(g, p).all()
