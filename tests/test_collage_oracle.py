"""tests/collage_oracle.py (the NumPy restatement of csrc/collage.hip) against the executed reference
(tests/golden/reference_collage.npz), and the host surface of the feature: symbols, refusals, signatures, render_preds'
files.  No GPU.  The fixture's primitives are painted by the header's integer rules, not by OpenCV."""
import inspect
import os

import numpy as np
import pytest

import collage_oracle as CO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_collage.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _a_case(g, name):
    h, w, nk, edges, radius = (int(v) for v in g[name + "_spec"])
    vis = g[name + "_vis"] if name + "_vis" in g.files else None
    return dict(img=g[name + "_img"], joints=g[name + "_joints"], vis=vis, draw_edges=bool(edges),
                radius=None if radius < 0 else radius, out=g[name + "_out"], prims=g[name + "_list"])


def test_draw_list_and_skeleton_images_equal_the_executed_reference(gold):
    for name in gold["a_cases"]:
        c = _a_case(gold, str(name))
        img, prims, _ = CO.draw_skeleton(c["img"], c["joints"], c["draw_edges"], c["vis"], c["radius"])
        assert np.array_equal(prims, c["prims"]), name                      # integer for integer
        assert img.dtype == c["out"].dtype and np.array_equal(img, c["out"]), name
    assert CO.radius_rule(600, 400) == 5 and CO.radius_rule(224, 224) == 4 and CO.radius_rule(17, 23) == 4


def test_the_fixture_covers_the_listed_cases(gold):
    specs = {str(n): tuple(int(v) for v in gold[str(n) + "_spec"]) for n in gold["a_cases"]}
    assert {(s[0], s[1]) for s in specs.values()} == {(32, 32), (17, 23), (224, 224), (600, 400)}
    assert {s[2] for s in specs.values()} == {19, 25}
    assert any(s[3] == 0 for s in specs.values()) and any(s[4] > 0 for s in specs.values())
    kinds = set()
    for n in specs:
        img = gold[n + "_img"]
        kinds.add("u8" if img.dtype == np.uint8 else ("f1" if img.max() <= 1 else "f2" if img.max() <= 2 else "f255"))
    assert kinds == {"u8", "f1", "f2", "f255"}
    j = gold["a00_joints"]
    assert (np.abs(j - np.floor(j)) == 0.5).any()                            # half-way joints: 10.5 -> 10, 11.5 -> 12
    assert [int(v) for v in gold["a00_list"][0, 1:3]] == [10, 12]
    assert (gold["a04_list"][:, 0] == CO.LINE).any() and any(p[0] == CO.LINE and p[1] == p[3] and p[2] == p[4] for p in gold["a04_list"])
    j = gold["a01_joints"]
    assert (j[:, 0] < 0).any() and (j[:, 0] > 23).any() and (j[:, 1] < 0).any() and (j[:, 1] > 17).any()
    assert float(gold["ambiguous_share"].max()) < 0.02


def test_visualize_img_skeletons_equal_the_executed_reference(gold):
    for key in ("b0", "b1"):
        crop = CO.crop_from_bytes(gold[key + "_crop_u8"])
        input_img = ((crop + 1) * 0.5) * 255.
        skel, prims, _ = CO.draw_skeleton(input_img, ((gold[key + "_kps"] + 1) * 0.5) * 224)
        if key + "_kp_gt" in gold.files:
            gt = gold[key + "_kp_gt"]
            skel, p2, _ = CO.draw_skeleton(skel, ((gt[:, :2] + 1) * 0.5) * 224, draw_edges=False, vis=gt[:, 2].astype(bool))
            prims = np.concatenate([prims, p2])
        assert np.array_equal(prims, gold[key + "_list"])
        assert np.array_equal(skel.astype(np.uint8), gold[key + "_skel"])


def test_collage_frames_equal_the_executed_reference_given_its_panels(gold):
    for k in range(5):
        key = "c%d" % k
        S, h, w, _ = (int(v) for v in gold[key + "_spec"])
        right = gold[key + "_collage_right"]
        assert right.shape[1:] == (2 * S, max(w * S // h, S), 3)
        for i in range(3):
            frame = CO.compose(gold[key + "_rend_crop"][i], gold[key + "_skel_crop"][i], gold[key + "_render_og"][i],
                               gold[key + "_rot_og"][i])
            assert frame.shape == (2 * S, CO.collage_width(S, h, w), 3)
            assert np.array_equal(frame[:, S:], right[i]), (key, i)
            assert np.array_equal(frame[:S, :S], gold[key + "_rend_crop"][i]) and np.array_equal(frame[S:, :S], gold[key + "_skel_crop"][i])
        assert np.array_equal(gold[key + "_full"], gold[key + "_render_og"])      # the full-size frames are the panel's bytes


def test_bytes_survive_the_references_floats():
    """trunc((v / 255) * 255) == v with the division in float64 (mesh panels) and in float32 (the skeleton panel): the
    kernel copies the left column of the collage on the strength of this"""
    v = np.arange(256)
    assert np.array_equal(((v / 255) * 255).astype(np.uint8), v)
    assert np.array_equal(((v.astype(np.float32) / 255).astype(np.float64) * 255).astype(np.uint8), v)


def test_line_rule_equals_the_headers_formula_in_exact_integers():
    """the kernel's three-branch form against 4 |a L - s d|^2 <= t^2 L^2 in Python's integers"""
    rng = np.random.default_rng(0)
    for _ in range(40):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-40, 60, 4))
        t = int(rng.integers(1, 9))
        got = CO.line_mask(24, 24, x0, y0, x1, y1, t)
        dx, dy = x1 - x0, y1 - y0
        L = dx * dx + dy * dy
        for y in range(24):
            for x in range(24):
                ax, ay = x - x0, y - y0
                s = min(max(ax * dx + ay * dy, 0), L)
                want = 4 * (ax * ax + ay * ay) <= t * t if L == 0 else \
                    4 * ((ax * L - s * dx) ** 2 + (ay * L - s * dy) ** 2) <= t * t * L * L
                assert bool(got[y, x]) == want
    far = CO.line_mask(16, 16, -32768, 3, 32767, 9, 3)                       # the clamped extremes stay exact
    assert far.any() and not far.all()


# ------------------------------------------------------------------------------------------------ the built library
def _lib():
    from human_dynamics_amd import _lib as L, build
    build.build(verbose=False)
    return L, L.load()


def test_new_symbols_are_exported_and_the_abi_number_stays():
    L, lib = _lib()
    for name in ("hmmr_draw_skeleton", "hmmr_compose_collage", "hmmr_collage_width", "hmmr_skeleton_radius"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.hmmr_abi_version() == 19


def test_collage_width_and_radius_helpers():
    _, lib = _lib()
    assert lib.hmmr_collage_width(224, 405, 720) == 224 + 398             # a 720 x 1280 frame after its down-scale
    assert lib.hmmr_collage_width(224, 720, 405) == 448 and lib.hmmr_collage_width(224, 300, 300) == 448
    for S, h, w in ((16, 12, 20), (16, 20, 12), (16, 16, 16), (16, 9, 31), (224, 96, 128)):
        assert lib.hmmr_collage_width(S, h, w) == CO.collage_width(S, h, w)
    assert lib.hmmr_collage_width(16, 1000, 20) == 0                        # w' = 0
    assert lib.hmmr_collage_width(8, 20, 20) == 0 and lib.hmmr_collage_width(2048, 20, 20) == 0
    assert lib.hmmr_collage_width(224, 0, 20) == 0 and lib.hmmr_collage_width(224, 20, -1) == 0
    for h, w in ((600, 400), (224, 224), (17, 23), (1024, 1024), (901, 900)):
        assert lib.hmmr_skeleton_radius(h, w) == CO.radius_rule(h, w)
    assert lib.hmmr_skeleton_radius(0, 5) == 0


def test_argument_refusals_need_no_gpu():
    """dummy, never dereferenced pointers: validation runs before any launch"""
    import ctypes as C
    L, lib = _lib()

    def skeleton(**kw):
        d = L.SkeletonDesc()
        d.kps, d.ld_kps, d.n, d.nk, d.h, d.w, d.draw_edges, d.bg_u8, d.out = 0x1000, 50, 2, 25, 32, 32, 1, 0x2000, 0x3000
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hmmr_draw_skeleton(C.byref(d), None)

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg)
        with pytest.raises(L.HmmrError):
            L.check(rc, "collage")

    refused(skeleton(nk=14), b"hmmr_draw_skeleton", b"nk = 14")
    refused(skeleton(radius=2), b"radius 2 < 3")
    refused(skeleton(radius=-1), b"radius")
    refused(skeleton(radius=L.SKELETON_MAX_RADIUS + 1), b"radius")
    refused(skeleton(kps=None), b"NULL operand")
    refused(skeleton(out=None), b"NULL operand")
    refused(skeleton(bg_u8=None), b"bg_float or bg_u8")
    refused(skeleton(bg_float=0x4000), b"bg_float or bg_u8")
    refused(skeleton(ld_kps=49), b"row stride")
    refused(skeleton(n=0), b"n = 0")
    refused(skeleton(h=15), b"image 15 x 32")
    refused(skeleton(w=1025), b"image 32 x 1025")
    refused(skeleton(draw_edges=2), b"draw_edges")
    refused(lib.hmmr_draw_skeleton(None, None), b"NULL descriptor")

    def collage(**kw):
        d = L.CollageDesc()
        d.rend_crop, d.skel_crop, d.render_og, d.rot_og, d.out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
        d.n, d.S, d.h, d.w = 2, 16, 12, 20
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.hmmr_compose_collage(C.byref(d), None)

    refused(collage(h=1000, w=20), b"hmmr_compose_collage", b"resized width")
    for name in ("rend_crop", "skel_crop", "render_og", "rot_og", "out"):
        refused(collage(**{name: None}), b"NULL operand")
    refused(collage(n=0), b"n = 0")
    refused(collage(S=8), b"S = 8")
    refused(lib.hmmr_compose_collage(None, None), b"NULL descriptor")


def test_python_signatures_follow_the_reference():
    from human_dynamics_amd.evaluation.run_video import render_preds
    from human_dynamics_amd.util.render import collage, nmr_renderer, video

    def names(fn):
        return list(inspect.signature(fn).parameters)
    assert names(render_preds)[:7] == ["output_path", "config", "preds", "images", "images_orig", "trim_length", "img_size"]
    assert inspect.signature(render_preds).parameters["img_size"].default == 224
    assert {"frames", "faces"} <= set(names(render_preds))
    assert names(nmr_renderer.visualize_img) == ["img", "cam", "kp_pred", "vert", "renderer", "kp_gt", "text", "rotated_view",
                                                 "mesh_color", "pad_vals", "no_text"]
    assert names(nmr_renderer.visualize_img_orig) == ["cam", "kp_pred", "vert", "renderer", "start_pt", "scale", "proc_img_shape",
                                                      "im_path", "img", "rotated_view", "mesh_color", "max_img_size", "no_text",
                                                      "bbox", "crop_cam"]
    assert inspect.signature(nmr_renderer.visualize_img_orig).parameters["max_img_size"].default == 300
    assert names(collage.draw_skeleton)[:5] == ["input_image", "joints", "draw_edges", "vis", "radius"]
    assert "on_device" in names(collage.draw_skeleton)
    assert inspect.signature(video.render_views).parameters["views"].default == ('orig', 'rotated', 'crop')
    with pytest.raises(NotImplementedError, match="draw_text"):
        nmr_renderer.visualize_img(np.zeros((16, 16, 3), np.float32), np.zeros(3), np.zeros((25, 2)), None, None)
    with pytest.raises(NotImplementedError, match="draw_text"):
        nmr_renderer.visualize_img(None, None, None, None, None, text={"a": 1}, no_text=True)


def test_make_square_and_remove_pads_round_trip():
    from human_dynamics_amd.util.render.nmr_renderer import make_square, remove_pads
    img = np.arange(9 * 31 * 3, dtype=np.float64).reshape(9, 31, 3)
    sq, pads = make_square(img)
    assert sq.shape == (31, 31, 3) and list(pads) == [22, 0] and not sq[9:].any()
    assert np.array_equal(remove_pads(sq, pads), img)
    sq, pads = make_square(img.transpose(1, 0, 2))
    assert sq.shape == (31, 31, 3) and list(pads) == [0, 22] and np.array_equal(remove_pads(sq, pads), img.transpose(1, 0, 2))


class _Config(object):
    mesh_color = 'blue'


def test_render_preds_files_and_early_return(gold, tmp_path, monkeypatch):
    """file naming, directory creation, trimming, chunking and the "video exists" return, with the device call replaced by
    the oracle's compose over the recorded panels"""
    import torch
    from PIL import Image
    from human_dynamics_amd.evaluation import run_video
    from human_dynamics_amd.util.render import video
    key, trim = "c1", 1
    S, h, w, _ = (int(v) for v in gold[key + "_spec"])
    n = 3 + 2 * trim
    calls = []

    def fake_render_views(records, layout, frames, params, faces, crops=None, views=None, max_img_size=720, mesh_color='blue',
                          device=None):
        assert views == ('collage',) and max_img_size == 720 and mesh_color == 'blue'
        idx = [int(k[0, 0]) for k in records["kps"]]                      # the frame numbers hidden in the keypoints
        calls.append(idx)
        assert tuple(np.asarray(crops).shape) == (len(idx), S, S, 3) and tuple(np.asarray(frames).shape) == (len(idx), h, w, 3)
        col = np.stack([CO.compose(gold[key + "_rend_crop"][i], gold[key + "_skel_crop"][i], gold[key + "_render_og"][i],
                                   gold[key + "_rot_og"][i]) for i in idx])
        return {"orig": torch.from_numpy(gold[key + "_render_og"][idx]), "collage": torch.from_numpy(col)}
    monkeypatch.setattr(video, "render_views", fake_render_views)
    monkeypatch.setattr(run_video.shutil, "which", lambda name: None)
    kps = np.zeros((n, 25, 2), np.float32)
    kps[:, 0, 0] = np.arange(n) - trim
    preds = {"kps": kps, "cams": np.zeros((n, 3), np.float32), "verts": np.zeros((n, 4, 3), np.float32)}
    images = [np.zeros((S, S, 3), np.float32)] * n
    images_orig = [{"im_path": "unused", "start_pt": np.array([0, 0]), "scale": 1.0, "im_shape": [S, S]}] * n
    out = str(tmp_path / "person0")
    res = run_video.render_preds(out, _Config(), preds, images, images_orig, trim, img_size=S, chunk=2,
                                 frames=np.zeros((n, h, w, 3), np.uint8), faces=np.array([[0, 1, 2]]), device="cpu")
    assert calls == [[0, 1], [2]]
    assert res["n_frames"] == 3 and res["videos"] is None and "ffmpeg" in res["note"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(out + "_crop")) == ["frame%06d.png" % i for i in range(3)]
    for i in range(3):
        full = np.asarray(Image.open(os.path.join(out, "frame%06d.png" % i)))
        crop = np.asarray(Image.open(os.path.join(out + "_crop", "frame%06d.png" % i)))
        assert np.array_equal(full, gold[key + "_full"][i])
        assert np.array_equal(crop[:, S:], gold[key + "_collage_right"][i])
    # the reference's early return
    open(out + ".mp4", "wb").close()
    calls[:] = []
    assert run_video.render_preds(out, _Config(), preds, images, images_orig, trim, img_size=S, frames=np.zeros((n, h, w, 3), np.uint8),
                                  faces=np.array([[0, 1, 2]]), device="cpu") is None
    assert calls == []
    assert run_video._ffmpeg_command("a.mp4", "dir")[:2] == ["ffmpeg", "-y"] and "dir/frame%06d.png" in run_video._ffmpeg_command("a.mp4", "dir")
