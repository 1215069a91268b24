"""The tube augmentor without a device: the float32 oracle (tests/tube_oracle.py) and the host mirror
(human_dynamics_amd/util/{data_utils,tube_augmentation}.py) against tests/golden/reference_tube.npz, which
tests/golden/make_tube_golden.py produced by executing the reference's own tube_augmentation.py / data_utils.py.

Tolerances: pixels, centres and walks exactly (the pixels of the fixture ARE the oracle's two restated TF kernels around the
reference's own pad / slice / flip / rescale; integers and walks are integer or replayed float32 arithmetic).  Labels, poses
and gt3ds within 1e-6: at most ~10 float32 roundings (6e-8 each) on normalised values of order 1, where the two sides may
differ by the accumulation order of a 2- or 3-term matrix product.
"""
import ctypes as C
import os

import numpy as np
import pytest

import tube_oracle as O
from human_dynamics_amd import _lib
from human_dynamics_amd.util import data_utils as D
from human_dynamics_amd.util.tube_augmentation import TubePreprocessor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tube.npz")
TOL = 1e-6


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def _pre(fx, case):
    S, tmax, dtmax, smax, dsmax = fx["ctor"]
    rmax = float(fx["c%d_rotate_max" % case])
    return TubePreprocessor(int(S), int(tmax), int(dtmax), float(smax), float(dsmax), rmax, float(fx["delta_rotate_max"]) if rmax else 0)


def _walks(fx, case):
    p = "c%d_" % case
    return fx[p + "trans_walk"], fx[p + "scale_walk"], fx[p + "rot_walk"]


@pytest.mark.parametrize("case", range(4))
def test_oracle_equals_the_reference_fixture(fx, case):
    p = "c%d_" % case
    pre = _pre(fx, case)
    trans, scale, rot = _walks(fx, case)
    assert bool(fx[p + "flip"]) == (case >= 2) and (pre.rotate_max != 0) == (case % 2 == 1)
    for t in range(len(fx["images"])):
        crop, label, pose, gt3d, c = O.frame(fx["images"][t], fx["image_sizes"][t], fx["labels"][t], fx["centers"][t], fx["poses"][t],
                                             fx["gt3ds"][t], trans[t], scale[t, 0], rot[t, 0], bool(fx[p + "flip"]), pre.output_size,
                                             pre.trans_max, pre.rotate_max)
        assert crop.dtype == np.float32 and np.array_equal(crop, fx[p + "images"][t]), (case, t)
        assert np.array_equal(c, fx[p + "centers"][t].reshape(2))
        assert np.abs(label - fx[p + "labels"][t]).max() <= TOL
        assert np.abs(pose - fx[p + "poses"][t]).max() <= TOL
        assert np.abs(gt3d - fx[p + "gt3ds"][t]).max() <= TOL
    assert np.abs(fx[p + "images"]).max() <= 1.0


@pytest.mark.parametrize("case", range(4))
def test_mirror_host_side_equals_the_reference_fixture(fx, case):
    p = "c%d_" % case
    pre = _pre(fx, case)
    ret, geom, rot = pre.host_side(fx["image_sizes"], fx["labels"], fx["centers"], fx["poses"], fx["gt3ds"], _walks(fx, case),
                                   bool(fx[p + "flip"]))
    assert ret["centers"].dtype == np.int32 and np.array_equal(ret["centers"], fx[p + "centers"])
    for k in ("labels", "poses", "gt3ds"):
        assert ret[k].dtype == np.float32 and ret[k].shape == fx[p + k].shape
        assert np.abs(ret[k] - fx[p + k]).max() <= TOL, k
    assert (rot is not None) == (pre.rotate_max != 0)
    # the kernel's operands reproduce the fixture's pixels through the oracle: geometry integers and rotation rows are right
    for t in range(len(geom)):
        crop = O.pixels(fx["images"][t], geom[t, 0], geom[t, 1], geom[t, 2], geom[t, 3], pre.output_size, bool(fx[p + "flip"]),
                        None if rot is None else rot[t])
        assert np.array_equal(crop, fx[p + "images"][t]), (case, t)


@pytest.mark.parametrize("case", range(4))
def test_walks_from_the_recorded_draws(fx, case):
    """draws, in the reference's order: flip, trans start, trans steps, scale start, scale steps[, rotate start, rotate steps]"""
    p = "c%d_" % case
    pre = _pre(fx, case)
    d = [fx[p + "draw%d" % i] for i in range(int(fx[p + "n_draws"]))]
    assert len(d) == (7 if pre.rotate_max else 5) and bool(d[0] < 0.5) == bool(fx[p + "flip"])
    trans = D.walk_from_draws(-pre.trans_max, pre.trans_max + 1, d[1], d[2], np.int32)
    assert trans.dtype == np.int32 and np.array_equal(trans, fx[p + "trans_walk"])
    assert np.array_equal(D.walk_from_draws(-pre.scale_max, pre.scale_max, d[3], d[4]), fx[p + "scale_walk"])
    if pre.rotate_max:
        assert np.array_equal(D.walk_from_draws(-pre.rotate_max, pre.rotate_max, d[5], d[6]), fx[p + "rot_walk"])
    else:
        assert np.array_equal(fx[p + "rot_walk"], np.zeros((6, 1), np.float32))
        assert np.array_equal(D.bounded_random_walk(-0, 0, -0, 0, 6), fx[p + "rot_walk"])


def test_seeded_walks_stay_inside_their_bounds():
    rng = np.random.default_rng(5)
    for tmax, dmax in ((20, 3), (6, 2), (2, 1), (3, 7)):
        w = D.bounded_random_walk(-tmax, tmax + 1, -dmax, dmax + 1, 400, np.int32, 2, rng)
        assert w.dtype == np.int32 and w.shape == (400, 2) and w.min() >= -tmax and w.max() <= tmax          # [minval, maxval)
        assert np.abs(np.diff(w, axis=0)).max() <= dmax                          # a reflection never lengthens a step
    for vmax, dmax in ((0.3, 0.05), (0.4, 0.1), (0.05, 0.3)):
        w = D.bounded_random_walk(-vmax, vmax, -dmax, dmax, 400, np.float32, 1, rng)
        assert w.dtype == np.float32 and w.shape == (400, 1)
        assert w.min() >= np.float32(-vmax) and w.max() <= np.float32(vmax)
    # maxval <= minval: the constant branch; minval == delta_min and maxval == delta_max: independent draws ("old augmentation")
    assert np.array_equal(D.bounded_random_walk(2, 2, -1, 1, 5, dim=3), np.full((5, 3), 2, np.float32))
    old = D.bounded_random_walk(-0.3, 0.3, -0.3, 0.3, 300, np.float32, 1, rng)
    assert old.min() >= -0.3 and old.max() < 0.3 and np.abs(np.diff(old[:, 0])).max() > 0.3
    pre = TubePreprocessor(32, 6, 2, 0.3, 0.05, 0.4, 0.1)
    a, b = pre.draw_walks(9, np.random.default_rng(1)), pre.draw_walks(9, np.random.default_rng(1))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and [x.shape for x in a] == [(9, 2), (9, 1), (9, 1)]


def test_integer_trans_walk_stays_inside_trans_max():
    """The translation walk is drawn with maxval = trans_max + 1 "exclusive" (tube_augmentation.py:60-68) and stays inside
    [-trans_max, trans_max], although the reference's reflection formula alone returns maxval at multiples of its period
    (with the seed below, before the fold of bounded_random_walk: trans_max 20 -> [-20, 21], 6 -> [-6, 7], 2 -> [-2, 3],
    3 -> [-3, 4] in 400 steps each).  walk_from_draws is that formula untouched: fed the draws of a walk that touches the
    bound it returns maxval, as the reference does in the fixture's case 3."""
    rng = np.random.default_rng(5)
    seen = []
    for tmax, dmax in ((20, 3), (6, 2), (2, 1), (3, 7)):
        w = D.bounded_random_walk(-tmax, tmax + 1, -dmax, dmax + 1, 400, np.int32, 2, rng)
        seen.append((tmax, int(w.min()), int(w.max())))
        print("trans_max %d: walk in [%d, %d]" % seen[-1])
    assert all(lo >= -tmax and hi <= tmax for tmax, lo, hi in seen), seen
    assert all(lo == -tmax and hi == tmax for tmax, lo, hi in seen), seen              # 400 steps reach both ends
    # the formula alone, bounds -6 .. 7: from 1 by steps of +3 the unreflected positions 4, 7, 10 give 4, 7 (= maxval), 4
    raw = D.walk_from_draws(-6, 7, np.array([[1]], np.int32), np.array([[3], [3], [3]], np.int32), np.int32)
    assert raw.ravel().tolist() == [4, 7, 4]


def test_geometry_integers_sweep_against_the_oracle():
    """sizes 8..700, scale exponents -3..1, centres from outside one edge to outside the other: the mirror's integers are the
    oracle's, and it refuses exactly the crops tf.slice would refuse"""
    rng = np.random.default_rng(77)
    refused = accepted = 0
    for S, tmax in ((32, 6), (224, 20), (7, 0)):
        pre = TubePreprocessor(S, tmax, 2, 0.3, 0.05)
        T = 150
        sizes = rng.integers(8, 701, (T, 2)).astype(np.int32)
        scale = rng.uniform(-3, 1, T).astype(np.float32)
        scale[:4] = (-3, 1, 0, -0.5)
        u = rng.uniform(-0.6, 1.6, (T, 2))
        u[:8] = ((-0.6, 0.5), (1.6, 0.5), (0.5, -0.6), (0.5, 1.6), (0, 0), (1, 1), (-0.6, -0.6), (1.6, 1.6))
        centers = (u * sizes[:, ::-1]).astype(np.int32)                           # (x, y) against (w, h)
        trans = rng.integers(-tmax, tmax + 1, (T, 2)).astype(np.int32)
        labels = rng.uniform(0, 700, (T, 3, 25)).astype(np.float32)
        for t in range(T):
            new_size, actual, c = O.scale_geometry(sizes[t], centers[t], trans[t], scale[t])
            x0, y0, ok = O.crop_origin(new_size, c, S, tmax)
            args = (sizes[t:t + 1], labels[t:t + 1], centers[t:t + 1], np.zeros((1, 72), np.float32), np.zeros((1, 14, 3), np.float32),
                    (trans[t:t + 1], scale[t:t + 1], np.zeros(1, np.float32)), False)
            if not ok:
                with pytest.raises(ValueError, match="frame 0"):
                    pre.host_side(*args)
                refused += 1
                continue
            ret, geom, rot = pre.host_side(*args)
            assert rot is None and geom.dtype == np.int32 and geom[0].tolist() == [new_size[0], new_size[1], x0, y0], (S, t)
            assert np.array_equal(ret["centers"].reshape(2), c)
            accepted += 1
    assert refused >= 20 and accepted >= 200, (refused, accepted)
    # the frame is named: the third of four frames is the bad one
    pre = TubePreprocessor(32, 6, 2, 0.3, 0.05)
    sizes = np.full((4, 2), 64, np.int32)
    centers = np.array([[32, 32], [32, 32], [400, 32], [32, 32]], np.int32)
    with pytest.raises(ValueError, match="frame 2"):
        pre.host_side(sizes, np.zeros((4, 3, 25), np.float32), centers, np.zeros((4, 72)), np.zeros((4, 14, 3)),
                      (np.zeros((4, 2), np.int32), np.zeros(4), np.zeros(4)), False)
    with pytest.raises(ValueError, match="frame 1"):                              # a scaled size of zero
        pre.host_side(np.array([[64, 64], [64, 1]], np.int32), np.zeros((2, 3, 25), np.float32), centers[:2], np.zeros((2, 72)),
                      np.zeros((2, 14, 3)), (np.zeros((2, 2), np.int32), np.full(2, -0.3), np.zeros(2)), False)


def test_reflections():
    rng = np.random.default_rng(3)
    pose = rng.normal(size=(5, 72)).astype(np.float32)
    assert np.array_equal(D.reflect_pose(D.reflect_pose(pose)), pose)
    assert np.array_equal(D.reflect_pose(pose[0]), O.reflect_pose(pose[0]))
    assert np.array_equal(D.POSE_SWAP_INDS, O.FLIP_POSE) and np.array_equal(D.KP_SWAP_INDS, O.FLIP_KP)
    assert np.array_equal(D.KP_SWAP_INDS[D.KP_SWAP_INDS], np.arange(25))
    j = rng.normal(size=(14, 3)).astype(np.float32)
    assert np.abs(D.reflect_joints3d(j) - O.reflect_joints3d(j)).max() <= TOL
    kp = rng.uniform(0, 32, (2, 3, 25)).astype(np.float32)
    back = D.flip_labels(D.flip_labels(kp, 32), 32)
    assert np.abs(back - kp).max() <= 4e-6                                         # two roundings of S - x - 1 at |x| <= 32
    assert np.array_equal(D.rescale_image(np.array([0, 0.5, 1], np.float32)), np.array([-1, 0, 1], np.float32))


def test_resize_and_rotate_restatements_on_known_cases():
    """identity resize, an exact 2x up-sampling row, rotation by 0 and by pi/2 of a one-hot image"""
    rng = np.random.default_rng(4)
    img = rng.random((5, 7, 3), dtype=np.float32)
    assert np.array_equal(O.tf_resize_bilinear(img, 5, 7), img)
    up = O.tf_resize_bilinear(img, 10, 14)
    assert np.array_equal(up[::2, ::2], img)                                       # in = i * 0.5: even outputs are source pixels
    assert np.allclose(up[0, 1], (img[0, 0] + img[0, 1]) / 2) and np.array_equal(up[:, -1], up[:, -2])   # no half-pixel offset; edge repeats
    sq = rng.random((9, 9, 3), dtype=np.float32)
    assert np.array_equal(O.tf_rotate_bilinear(sq, O.rotate_transform(0.0, 9)), sq)
    hot = np.zeros((9, 9, 3), np.float32)
    hot[2, 6] = 1
    r = O.tf_rotate_bilinear(hot, O.rotate_transform(np.pi / 2, 9))
    assert np.abs(r[2, 2] - 1).max() < 1e-5 and r.sum() < 3 + 1e-4                 # (x, y) = (6, 2) turns to (2, 2): counter-clockwise on screen


def test_tube_augment_refuses_bad_arguments():
    """dummy, never dereferenced pointers: validation runs before any launch, so no device is needed"""
    lib = _lib.load()
    assert "hmmr_tube_augment" in _lib.SIGNATURES
    P = [0x1000 * (i + 1) for i in range(5)]
    base = dict(images=P[0], u8=0, n=2, h=40, w=52, geom=P[1], flip=P[2], rot=None, S=32, out=P[3], st=None)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return lib.hmmr_tube_augment(*[a[k] for k in "images u8 n h w geom flip rot S out st".split()])
    for bad in (dict(images=None), dict(geom=None), dict(flip=None), dict(out=None), dict(n=0), dict(h=0), dict(w=-1), dict(S=0),
                dict(n=-3, rot=P[4]), dict(u8=1, S=-1)):
        rc = call(**bad)
        msg = lib.hmmr_last_error()
        assert rc == -1 and b"hmmr_tube_augment" in msg, (bad, rc, msg)
        with pytest.raises(_lib.HmmrError):
            _lib.check(rc, "hmmr_tube_augment")
    assert lib.hmmr_abi_version() == 19
