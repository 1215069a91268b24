"""The crop before the path against the reference's own process_image, executed from
the reference tree (tests/golden/make_reference_golden.py, part 6; cv2.resize itself is restated)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import preprocess_oracle as PO


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_crops.npz")))


def test_oracle_crop_equals_reference_process_image(ref):
    for fr, crop, p in zip(ref["frames"], ref["crops"], ref["params"]):
        out = PO.process_image(fr, p[:3])
        assert np.abs(out["image"] - crop).max() < 1e-6
        assert list(out["center"]) == [int(p[3]), int(p[4])] and list(out["start_pt"]) == [int(p[5]), int(p[6])]


def test_crop_geometry_matches_reference_integers(ref):
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    for fr, p in zip(ref["frames"], ref["params"]):
        g = crop_geometry(fr.shape[0], fr.shape[1], p[:3])
        assert list(g["center"]) == [int(p[3]), int(p[4])] and list(g["start_pt"]) == [int(p[5]), int(p[6])]
    with pytest.raises(ValueError):
        crop_geometry(96, 128, [64.0, 40.0, 0.001])


def test_resize_known_answers():
    img = np.arange(12, dtype=np.float64).reshape(3, 4, 1)
    assert np.array_equal(PO.cv2_resize_linear(img, (4, 3)), img)               # identity size
    up = PO.cv2_resize_linear(img, (8, 3))[..., 0]                              # 2x in x: centres at 0.25-steps
    assert np.allclose(up[0], [0, 0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.0])


@pytest.mark.gpu
def test_hip_crop_equals_reference_process_image(ref, gpu_device):
    from human_dynamics_amd.evaluation.run_video import process_images
    out, infos = process_images(ref["frames"], ref["params"][:, :3], device=gpu_device)
    got = out.cpu().numpy()
    assert got.shape == ref["crops"].shape and got.dtype == np.float32
    err = np.abs(got - ref["crops"]).max()
    print("HIP crop vs reference process_image: max abs err %.2e" % err)
    assert err < 1e-6
    for info, p in zip(infos, ref["params"]):
        assert list(info["center"]) == [int(p[3]), int(p[4])] and list(info["start_pt"]) == [int(p[5]), int(p[6])]


def _agree(h, w, bbox):
    """crop_geometry against the oracle's integers: same centre, same crop origin, same verdict on the full crop."""
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    o = PO.crop_integers((h, w), bbox)
    full = o["im_shape"] == [224, 224] and int(o["new_size"].min()) >= 1
    try:
        g = crop_geometry(h, w, bbox)
    except ValueError:
        return (not full), False
    ok = (full and list(g["center"]) == list(o["center"]) and list(g["start_pt"]) == list(o["start_pt"])
          and [g["hs"], g["ws"]] == list(o["new_size"]) and [g["u0"], g["v0"]] == [int(o["start_pt"][0]) - 224, int(o["start_pt"][1]) - 224])
    return ok, True


def test_crop_geometry_sweep_against_the_oracle():
    """Seeded sweep: frames 8..2160 x 8..3840 (odd sizes included), scales 0.05..4, bbox centres from 20 px outside the
    frame on one side to 20 px outside on the other.  The integers come from the oracle's geometry part (the part of
    process_image that needs no pixels); on the small frames process_image itself is run on a 1-channel dummy, which also
    pins that geometry part to it."""
    rng = np.random.default_rng(8)
    sizes = [(8, 8), (9, 13), (2160, 3840), (2159, 3839), (1080, 1920), (720, 1280), (101, 203), (8, 3840), (2160, 8)]
    sizes += [(int(rng.integers(8, 2161)), int(rng.integers(8, 3841))) for _ in range(600)]
    sizes += [(int(rng.integers(8, 120)), int(rng.integers(8, 120))) for _ in range(200)]
    bad, accepted, with_pixels = [], 0, 0
    for h, w in sizes:
        for scale in (0.05, 4.0, 1.0, float(rng.uniform(0.05, 0.6)), float(np.exp(rng.uniform(np.log(0.05), np.log(4.0))))):
            fx, fy = rng.choice([0.0, 1.0, float(rng.random()), float(rng.random())], 2)
            bbox = [-20.0 + fx * (w + 40.0), -20.0 + fy * (h + 40.0), scale]
            ok, acc = _agree(h, w, bbox)
            accepted += acc
            if not ok:
                bad.append((h, w, bbox))
            if h * w * max(scale, 1.0) ** 2 <= 120 * 120 * 4 and acc:
                out = PO.process_image(np.zeros((h, w, 1), np.uint8), bbox)
                o = PO.crop_integers((h, w), bbox)
                assert list(out["center"]) == list(o["center"]) and list(out["start_pt"]) == list(o["start_pt"])
                assert out["im_shape"] == o["im_shape"] == [224, 224]
                with_pixels += 1
    print("crop geometry sweep: %d cases, %d accepted, %d also through process_image, %d disagreements"
          % (5 * len(sizes), accepted, with_pixels, len(bad)))
    assert not bad, bad[:5]
    assert accepted > 0.9 * 5 * len(sizes) and with_pixels >= 300      # the sweep compares integers, it does not just agree on refusals


def test_windowed_oracle_is_bit_identical_to_process_image():
    """process_image_window (what the GPU sweep uses on 1080p frames scaled up) is process_image, bit for bit: scales below,
    at and above 1, windows inside the image and hanging over every edge, a scaled image of one row."""
    rng = np.random.default_rng(12)
    n = 0
    for h, w in ((96, 128), (101, 203), (37, 301)):
        fr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for scale in (0.03, 0.3, 0.97, 1.0, 1.7, 3.9):
            for cx, cy in ((w / 2, h / 2), (0, 0), (w, h), (-15, h + 15), (w + 15, -15)):
                a, b = PO.process_image(fr, [cx, cy, scale]), PO.process_image_window(fr, [cx, cy, scale])
                assert np.array_equal(a["image"], b["image"]) and list(a["start_pt"]) == list(b["start_pt"])
                n += 1
    assert n == 90
