"""hmmr_tube_augment (csrc/tube.hip), TubePreprocessorDriver and the device route of FeatureExtractor on the GPU.

Pixels are compared with np.array_equal: the kernel (compiled without contraction) and the float32 NumPy oracle
(tests/tube_oracle.py) perform the same IEEE float32 operations in the same order, so a difference is a bug, not noise.
Labels, poses and gt3ds within 1e-6 (tests/test_tube_oracle.py says why).  No input here is refused by the host checks and
none leaves the frame: the kernel clamps every tap, and crop origins "beyond the image" are the edge pad's normal case.
"""
import os

import numpy as np
import pytest
import torch

import tube_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
TOL = 1e-6


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reference_tube.npz")))


def _driver(fx, case, device):
    from human_dynamics_amd.util.tube_augmentation import TubePreprocessorDriver
    S, tmax, dtmax, smax, dsmax = fx["ctor"]
    rmax = float(fx["c%d_rotate_max" % case])
    return TubePreprocessorDriver(int(S), int(tmax), int(dtmax), float(smax), float(dsmax), rmax, float(fx["delta_rotate_max"]) if rmax else 0,
                                  device=device)


@pytest.mark.parametrize("case", range(4))
def test_driver_reproduces_the_reference_fixture(fx, case, gpu_device):
    """(a) flip off / on x rotate_max 0 / 0.4, the recorded walks replayed; labels enter as [T,25,3] and are transposed"""
    p = "c%d_" % case
    drv = _driver(fx, case, gpu_device)
    ret = drv(fx["images"], fx["image_sizes"], np.transpose(fx["labels"], [0, 2, 1]), fx["centers"], fx["poses"], fx["gt3ds"],
              walks=(fx[p + "trans_walk"], fx[p + "scale_walk"], fx[p + "rot_walk"]), flip=bool(fx[p + "flip"]))
    assert sorted(ret) == ["centers", "gt3ds", "images", "labels", "poses", "rot_walk", "scale_walk", "trans_walk"]
    assert isinstance(ret["images"], np.ndarray) and ret["images"].dtype == np.float32
    diff = ret["images"] != fx[p + "images"]
    print("tube: case %d, %d of %d pixels differ from the fixture" % (case, int(diff.sum()), diff.size))
    assert np.array_equal(ret["images"], fx[p + "images"])
    for k in ("centers", "trans_walk", "scale_walk", "rot_walk"):
        assert np.array_equal(ret[k], fx[p + k]), k
    for k in ("labels", "poses", "gt3ds"):
        assert np.abs(ret[k] - fx[p + k]).max() <= TOL, k


ANGLES = (0.0, 0.3, -0.3, float(np.pi / 2))


def _sweep_cases():
    """~100 geometries, each launched twice (uint8 and float32 frames): explicit edge cases first, then seeded ones"""
    rng = np.random.default_rng(31)
    cases = []

    def add(S, n, H, W, geom, flip, angles):
        geom = np.broadcast_to(np.asarray(geom, np.int32), (n, 4)).copy()
        cases.append(dict(S=S, n=n, H=H, W=W, geom=geom, flip=np.broadcast_to(np.asarray(flip, bool), (n,)).copy(),
                          angles=None if angles is None else np.broadcast_to(np.asarray(angles, np.float32), (n,)).copy()))
    for S in (7, 8, 32):
        for ang in (None,) + ANGLES:
            add(S, 1, 9, 13, (5, 6, -1, -2), False, ang)                 # the scaled image smaller than S in both axes (S = 7: 5 x 6)
            add(S, 5, 70, 8, (1, 11, -3, 0), True, ang)                  # newH == 1; flip (odd S with S = 7)
            add(S, 1, 8, 70, (16, 140, -S - 2, 20), True, ang)            # origin negative in x, beyond the image in y
            add(S, 5, 33, 21, (66, 42, 40, -S - 1), False, ang)           # beyond the image in x, negative in y
    while len(cases) < 100:
        S, n = int(rng.choice((7, 8, 32))), int(rng.choice((1, 5)))
        H, W = (int(v) for v in rng.integers(8, 71, 2))
        if H == W:
            W = W + 1 if W < 70 else W - 1
        geom = np.stack([rng.integers(1, 2 * H + 1, n), rng.integers(1, 2 * W + 1, n), np.zeros(n, np.int64), np.zeros(n, np.int64)], 1)
        geom[:, 2] = rng.integers(-S - 3, geom[:, 1] + 4)
        geom[:, 3] = rng.integers(-S - 3, geom[:, 0] + 4)
        kind = len(cases) % 3
        angles = None if kind == 0 else (rng.choice(ANGLES, n) if kind == 1 else rng.uniform(-0.4, 0.4, n))
        add(S, n, H, W, geom, rng.integers(0, 2, n).astype(bool), angles)
    return cases


def test_kernel_sweep_against_the_oracle(gpu_device):
    """(b) ~200 launches: S in {7, 8, 32}, H != W in 8..70 (odd sizes among them), n in {1, 5}, the edge cases of _sweep_cases,
    rotation by 0, +-0.3, pi/2 and seeded angles, per-frame flips; uint8 and float32 frames of the same tube agree with each
    other and with the oracle bit for bit"""
    from human_dynamics_amd.util import data_utils as D
    from human_dynamics_amd.util.tube_augmentation import tube_augment
    rng = np.random.default_rng(32)
    cases = _sweep_cases()
    assert {c["S"] for c in cases} == {7, 8, 32} and {c["n"] for c in cases} == {1, 5}
    assert any(c["H"] % 2 and c["W"] % 2 == 0 for c in cases) and all(c["H"] != c["W"] for c in cases)
    launches = wrong = 0
    for i, c in enumerate(cases):
        S, n = c["S"], c["n"]
        u8 = rng.integers(0, 256, (n, c["H"], c["W"], 3), dtype=np.uint8)
        f32 = O.u8_to_float(u8)
        rot = None if c["angles"] is None else D.rotate_transforms(c["angles"], S)
        if rot is not None:
            assert np.array_equal(rot, np.stack([O.rotate_transform(a, S) for a in c["angles"]]))
        want = np.stack([O.pixels(f32[t], c["geom"][t, 0], c["geom"][t, 1], c["geom"][t, 2], c["geom"][t, 3], S, bool(c["flip"][t]),
                                  None if rot is None else rot[t]) for t in range(n)])
        got_f = tube_augment(f32, c["geom"], c["flip"], rot, S, gpu_device).cpu().numpy()
        got_u = tube_augment(torch.from_numpy(u8).to(gpu_device), c["geom"], c["flip"], rot, S, gpu_device).cpu().numpy()
        launches += 2
        bad = int((got_f != want).sum()), int((got_u != want).sum())
        if bad != (0, 0):
            wrong += 1
            print("tube: sweep case %d (S=%d n=%d %dx%d geom0=%s rot=%s): %d / %d of %d values differ (float / uint8 frames)"
                  % (i, S, n, c["H"], c["W"], c["geom"][0].tolist(), None if rot is None else c["angles"].tolist(), bad[0], bad[1], want.size))
    print("tube: %d launches, %d geometries with a difference" % (launches, wrong))
    assert launches >= 200 and wrong == 0


@pytest.fixture(scope="module")
def extractor(weights, gpu_device):
    from human_dynamics_amd.datasets.resnet_extractor import FeatureExtractor
    return FeatureExtractor("synthetic:0", batch_size=4, weights=weights, dtype="f32", device=gpu_device)


def test_compute_all_phis_on_a_device_tensor(extractor, gpu_device):
    """(c) 5 frames in batches of 4: the crops as a CUDA tensor give the bits of the same crops as a host array"""
    from human_dynamics_amd import assets
    frames = assets.make_synthetic_frames(5, seed=1)
    host = extractor.compute_all_phis(frames)
    dev = torch.from_numpy(np.ascontiguousarray(frames, np.float32)).to(gpu_device)
    got = extractor.compute_all_phis(dev)
    assert isinstance(got, np.ndarray) and got.shape == host.shape == (5, 2048) and np.isfinite(host).all()
    assert np.array_equal(got, host)
    t = extractor.compute_all_phis(dev, to_numpy=False)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), host)
    assert np.array_equal(extractor.compute_phis(dev[:4]), host[:4])
    with pytest.raises(ValueError):
        extractor.compute_phis(dev.double())


def test_compute_all_phis_augmented(extractor, gpu_device):
    """(d) the writers' call site: the phis are those of the driver's own crops, the labels the driver's"""
    from human_dynamics_amd.util.tube_augmentation import TubePreprocessorDriver
    rng = np.random.default_rng(8)
    T, H, W = 5, 120, 90
    images = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    image_sizes = np.tile(np.array([[H, W]], np.int32), (T, 1))
    labels = np.stack([rng.uniform(0, W, (T, 25)), rng.uniform(0, H, (T, 25)), rng.integers(0, 2, (T, 25))], 2).astype(np.float32)
    centers = np.tile(np.array([[W // 2, H // 2]], np.int32), (T, 1))
    poses = rng.normal(0, 0.3, (T, 72)).astype(np.float32)
    gt3ds = rng.normal(0, 0.3, (T, 14, 3)).astype(np.float32)
    drv = TubePreprocessorDriver(rotate_max=0.2, delta_rotate_max=0.05, device=gpu_device)
    walks = drv.preprocessor.draw_walks(T, np.random.default_rng(9))
    args = (images, image_sizes, labels, centers, poses, gt3ds)
    plain = drv(*args, walks=walks, flip=True)
    assert plain["images"].shape == (T, 224, 224, 3) and np.abs(plain["images"]).max() <= 1.0 + 1e-6
    aug = extractor.compute_all_phis_augmented(drv, *args, walks=walks, flip=True)
    assert sorted(aug) == sorted(list(plain) + ["phis"])
    for k in plain:
        assert np.array_equal(aug[k], plain[k]), k
    assert aug["phis"].shape == (T, 2048) and np.array_equal(aug["phis"], extractor.compute_all_phis(plain["images"]))
    on_dev = extractor.compute_all_phis_augmented(drv, *args, walks=walks, flip=True, keep_images=False)
    assert on_dev["images"].is_cuda and np.array_equal(on_dev["phis"], aug["phis"])
    # one frame of the 224 route against the oracle (the uint8 table, rotation and flip at the extractor's size)
    _, geom, rot = drv.preprocessor.host_side(image_sizes, np.transpose(labels, [0, 2, 1]), centers, poses, gt3ds, walks, True)
    want = O.pixels(O.u8_to_float(images[2]), geom[2, 0], geom[2, 1], geom[2, 2], geom[2, 3], 224, True, rot[2])
    assert np.array_equal(plain["images"][2], want)
