"""csrc/collage.hip on the device against the executed reference (tests/golden/reference_collage.npz) and the NumPy
restatement (tests/collage_oracle.py, pinned to that fixture by tests/test_collage_oracle.py).

Skeleton rule: a pixel covered by any primitive equals the reference to the byte; an uncovered pixel is equal over a uint8
background and within 1 LSB over a float one (the tolerance HMMR_RENDER_BG_FLOAT has).  Mesh rule (tests/test_gpu_render.py):
within 1 LSB outside the oracle's ambiguity mask; in the two resized quadrants of the collage the mask is dilated by the
resize footprint and the bound is 2 (a second truncation).  The primitives' pixels are the header's integer rules: nothing
here measures OpenCV.

Mutations of csrc/collage.hip and the test that catches each:
  `<=` -> `<` in the disc rule .................. test_draw_skeleton_against_the_executed_reference
  draw order reversed ........................... test_draw_skeleton_against_the_executed_reference
  parent-invisible treated as child-invisible ... test_draw_skeleton_against_the_executed_reference (a07), test_batched_rows_...
  rintf -> floorf(x + 0.5) ...................... test_batched_rows_strides_nan_and_clamp (kps at .5), ..._executed_reference (a00)
  padding on the wrong panel .................... test_compose_collage_against_the_recorded_panels (c0, c3: w' > S; c1: w' < S)
  w' computed as h S / w ........................ test_compose_collage_against_the_recorded_panels (shape)
  rot_og resized with its aspect kept ........... test_compose_collage_against_the_recorded_panels (c0, c1, c3)
  rounding instead of truncation at the end ..... test_compose_collage_against_the_recorded_panels (0 differing bytes)
"""
import os

import numpy as np
import pytest

import collage_oracle as CO

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_collage.npz")
MAX_EXCLUDED = 0.02


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _skeleton_check(got, want, covered, float_bg, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d[covered].max(initial=0) == 0, (what, "covered pixels differ", int((d[covered] > 0).sum()))
    assert d[~covered].max(initial=0) <= (1 if float_bg else 0), (what, "background differs", int(d[~covered].max()))


def test_draw_skeleton_against_the_executed_reference(gold, gpu_device):
    from human_dynamics_amd.util.render import collage
    for name in (str(n) for n in gold["a_cases"]):
        h, w, nk, edges, radius = (int(v) for v in gold[name + "_spec"])
        img, joints, want = gold[name + "_img"], gold[name + "_joints"], gold[name + "_out"]
        vis = gold[name + "_vis"] if name + "_vis" in gold.files else None
        kw = dict(draw_edges=bool(edges), vis=vis, radius=None if radius < 0 else radius)
        got = collage.draw_skeleton(img, joints, device=gpu_device, **kw)
        _, _, covered = CO.draw_skeleton(img, joints, **kw)
        assert covered.any(), name
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype, (name, got.dtype, want.dtype)
        scale = 255.0 if (img.dtype != np.uint8 and img.max() <= 1) else 1.0       # back to byte values
        _skeleton_check(np.round(got * scale), np.round(want * scale), covered, img.dtype != np.uint8, name)
        if name == "a00":                                                           # 2 x K joints and a device result
            dev = collage.draw_skeleton(img, joints.T, on_device=True, device=gpu_device, **kw)
            assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


def test_batched_rows_strides_nan_and_clamp(gpu_device):
    """n = 3 frames whose joints sit in rows of 64 floats (> 2 nk), the fused (kp + 1) * (S / 2) with half-way values, a NaN
    joint, a joint far beyond the clamp, vis; 17 x 23 (no multiple of the 64 x 16 tile); in place equals out of place"""
    import torch
    from human_dynamics_amd.util.render import collage
    rng = np.random.default_rng(5)
    for (h, w), nk in (((32, 32), 25), ((17, 23), 19), ((40, 150), 25)):
        n, S = 3, h
        rows = rng.uniform(-1.1, 1.1, (n, 64)).astype(np.float32)
        rows[0, 0:4] = [10.5 / (S / 2) - 1, 11.5 / (S / 2) - 1, 12.5 / (S / 2) - 1, 7.5 / (S / 2) - 1]      # 10.5, 11.5, 12.5, 7.5 when S/2 is a power of two
        rows[1, 4] = np.nan                                                          # joint 2: nothing drawn, its edges go
        rows[2, 6:8] = [1e9, -1e9]                                                   # joint 3: clamped to 32767, -32768
        vis = np.ones((n, nk), np.uint8)
        vis[1, 8], vis[2, 0] = 0, 0                                                  # a parent and a leaf
        crops = rng.uniform(-1, 1, (n, h, w, 3)).astype(np.float32)
        bytes_bg = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        want_f, want_u, cov = [], [], []
        for i in range(n):
            j, ok = CO.pixel_joints(rows[i, :2 * nk].reshape(nk, 2), 1.0, 0.5 * S)
            prims = CO.draw_list(j, CO.radius_rule(h, w), True, vis[i] * ok)
            bg = (((crops[i] + np.float32(1)) * np.float32(127.5))).astype(np.uint8)
            a, c = CO.rasterise(bg, prims)
            want_f.append(a); cov.append(c); want_u.append(CO.rasterise(bytes_bg[i], prims)[0])
        k_dev, v_dev = torch.as_tensor(rows, device=gpu_device), torch.as_tensor(vis, device=gpu_device)
        got_f = collage.skeleton_panels(k_dev, torch.as_tensor(crops, device=gpu_device), nk=nk, kp_add=1.0, kp_mul=0.5 * S, vis=v_dev,
                                        bg_add=1.0, bg_mul=127.5).cpu().numpy()
        b_dev = torch.as_tensor(bytes_bg, device=gpu_device)
        got_u = collage.skeleton_panels(k_dev, b_dev, nk=nk, kp_add=1.0, kp_mul=0.5 * S, vis=v_dev)
        in_place = b_dev.clone()
        assert collage.skeleton_panels(k_dev, in_place, nk=nk, kp_add=1.0, kp_mul=0.5 * S, vis=v_dev, out=in_place) is in_place
        assert torch.equal(in_place, got_u)
        for i in range(n):
            _skeleton_check(got_f[i], want_f[i], cov[i], True, ((h, w), i, "float"))
            _skeleton_check(got_u.cpu().numpy()[i], want_u[i], cov[i], False, ((h, w), i, "uint8"))
        assert cov[0].any() and cov[1].any() and cov[2].any()
    with pytest.raises(Exception, match="nk = 14"):
        collage.skeleton_panels(k_dev, b_dev, nk=14)


def test_compose_collage_against_the_recorded_panels(gold, gpu_device):
    import torch
    from human_dynamics_amd.util.render import collage
    differing = {}
    for k in range(5):
        key = "c%d" % k
        S, h, w, _ = (int(v) for v in gold[key + "_spec"])
        panels = [torch.as_tensor(gold[key + p], device=gpu_device) for p in ("_rend_crop", "_skel_crop", "_render_og", "_rot_og")]
        got = collage.compose_collage(*panels).cpu().numpy()
        w2 = w * S // h
        assert got.shape == (3, 2 * S, S + max(w2, S), 3) and got.dtype == np.uint8
        want = np.concatenate([np.concatenate([gold[key + "_rend_crop"], gold[key + "_skel_crop"]], 1), gold[key + "_collage_right"]], 2)
        if w2 > S:                                           # the padding side, exactly: ones to the right of the narrower panel
            assert (got[:, S:, 2 * S:] == 255).all() and not (want[:, :S, 2 * S:] == 255).all()
        elif w2 < S:
            assert (got[:, :S, S + w2:] == 255).all()
        d = np.abs(got.astype(int) - want.astype(int))
        assert d.max() <= 1, (key, d.max())
        differing[key] = int((d > 0).sum())
    print("compose_collage: differing bytes per case:", differing)
    assert sum(differing.values()) == 0, differing           # the arithmetic is the oracle's fp64, operation for operation


def _collage_case(gold, key, gpu_device):
    S, h, w, trim = (int(v) for v in gold[key + "_spec"])
    lo = trim
    sl = slice(lo, lo + 3)
    preds = {"cams": gold[key + "_cams"][sl], "kps": gold[key + "_kps"][sl],
             "verts": np.broadcast_to(gold[key + "_verts"], (3,) + gold[key + "_verts"].shape).copy()}
    params = [{"start_pt": np.array([int(p[0]), int(p[1])]), "scale": float(p[2]), "im_shape": [S, S]} for p in gold[key + "_params"][sl]]
    crops = CO.crop_from_bytes(gold[key + "_images_u8"][sl])
    return S, h, w, trim, preds, params, crops, gold[key + "_frames"][sl]


def _mesh_check(got, want, amb, bound, what):
    d = np.abs(got.astype(int) - want.astype(int)).max(-1)
    assert d[~amb].max(initial=0) <= bound, (what, int(d[~amb].max()), int((d[~amb] > bound).sum()))


@pytest.mark.parametrize("key", ["c0", "c1", "c2", "c3", "c4"])
def test_render_views_collage_end_to_end(key, gold, gpu_device):
    import torch
    from human_dynamics_amd.util.render import video
    S, h, w, trim, preds, params, crops, frames = _collage_case(gold, key, gpu_device)
    out = video.render_views(preds, None, frames, params, gold["faces"], crops=crops, views=('collage',), device=torch.device(gpu_device))
    assert set(out) == {"orig", "rotated", "crop", "skel", "collage"} and out["collage"].is_cuda
    got = out["collage"].cpu().numpy()
    w2 = w * S // h
    assert got.shape == (3, 2 * S, S + max(w2, S), 3)
    excluded = 0
    for i in range(3):
        # the skeleton quadrant
        j, ok = CO.pixel_joints(preds["kps"][i], 1.0, 0.5 * S)
        covered = CO.rasterise(np.zeros((S, S, 3), np.uint8), CO.draw_list(j, CO.radius_rule(S, S), True, ok))[1]
        _skeleton_check(got[i, S:, :S], gold[key + "_skel_crop"][i], covered, True, (key, i, "skel"))
        assert np.array_equal(got[i, S:, :S], out["skel"][i].cpu().numpy())
        # the three mesh quadrants
        a_crop = gold[key + "_amb_crop"][i]
        a_og = CO.resize_footprint(gold[key + "_amb_og"][i], S, w2)
        a_rot = CO.resize_footprint(gold[key + "_amb_rot"][i], S, S)
        want_right = gold[key + "_collage_right"][i]
        _mesh_check(got[i, :S, :S], gold[key + "_rend_crop"][i], a_crop, 1, (key, i, "crop"))
        _mesh_check(got[i, :S, S:S + w2], want_right[:S, :w2], a_og, 2, (key, i, "orig"))
        _mesh_check(got[i, S:, S:2 * S], want_right[S:, :S], a_rot, 2, (key, i, "rotated"))
        assert np.array_equal(got[i, :S, S + w2:], want_right[:S, w2:]) and np.array_equal(got[i, S:, 2 * S:], want_right[S:, S:])
        _mesh_check(out["orig"][i].cpu().numpy(), gold[key + "_full"][i], gold[key + "_amb_og"][i], 1, (key, i, "full"))
        excluded += int(a_crop.sum()) + int(a_og.sum()) + int(a_rot.sum())
    share = excluded / float(got[..., 0].size)
    print("%s: %.3f %% of the collage excluded as ambiguous" % (key, 100 * share))
    assert share < MAX_EXCLUDED, share
    # today's callers get today's dict
    plain = video.render_views(preds, None, frames, params, gold["faces"], crops=crops, device=torch.device(gpu_device))
    assert set(plain) == {"orig", "rotated", "crop"} and all(torch.equal(plain[v], out[v]) for v in plain)


def test_visualize_img_against_the_executed_reference(gold, gpu_device):
    from human_dynamics_amd.util.render.nmr_renderer import VisRenderer, visualize_img
    for key in ("b0", "b1"):
        crop = CO.crop_from_bytes(gold[key + "_crop_u8"])
        kp_gt = gold[key + "_kp_gt"] if key + "_kp_gt" in gold.files else None
        r = VisRenderer(224, faces=gold["faces"], device=gpu_device)
        skel, rend = visualize_img(img=crop, cam=gold[key + "_cam"], kp_pred=gold[key + "_kps"], vert=gold["b_verts"], renderer=r,
                                   kp_gt=kp_gt, no_text=True)
        assert skel.shape == rend.shape == (224, 224, 3) and skel.max() <= 1 and rend.max() <= 1
        covered = np.zeros((224, 224), bool)
        for p in gold[key + "_list"]:
            covered |= CO.prim_mask(224, 224, p)
        _skeleton_check(np.round(skel * 255), gold[key + "_skel"], covered, True, key)
        _mesh_check(np.round(rend * 255), gold[key + "_rend"], gold[key + "_amb"], 1, key)


def test_visualize_img_orig_and_render_preds_against_the_executed_reference(gold, gpu_device, tmp_path):
    from PIL import Image
    from human_dynamics_amd.evaluation.run_video import render_preds
    from human_dynamics_amd.util.render.nmr_renderer import VisRenderer, visualize_img_orig
    key = "c3"                                               # 9 x 31 frames: make_square pads 22 rows, w' > S
    S, h, w, trim, preds, params, crops, frames = _collage_case(gold, key, gpu_device)
    r = VisRenderer(S, faces=gold["faces"], device=gpu_device)
    skel, rend, rot = visualize_img_orig(cam=preds["cams"][0], kp_pred=preds["kps"][0], vert=preds["verts"][0], renderer=r,
                                         start_pt=params[0]["start_pt"], scale=params[0]["scale"], proc_img_shape=[S, S],
                                         img=((frames[0] / 255.) - 0.5) * 2, max_img_size=720, no_text=True, rotated_view=True)
    assert skel.shape == rend.shape == rot.shape == (h, w, 3) and r.renderer.image_size == max(h, w)
    _mesh_check(np.round(rend * 255), gold[key + "_render_og"][0], gold[key + "_amb_og"][0], 1, "render_og")
    _mesh_check(np.round(rot * 255), gold[key + "_rot_og"][0], gold[key + "_amb_rot"][0], 1, "rot_og")

    class Config(object):
        mesh_color = 'blue'
    n = 3 + 2 * trim                                         # the trimmed frames are there and must not be rendered
    pad = lambda a: np.concatenate([a[:1]] * trim + [a] + [a[-1:]] * trim) if trim else a
    full = {k: pad(v) for k, v in preds.items()}
    out = str(tmp_path / "track")
    res = render_preds(out, Config(), full, list(pad(crops)), [params[0]] * trim + params + [params[-1]] * trim, trim, img_size=S,
                       frames=pad(frames), faces=gold["faces"], chunk=2, device=gpu_device)
    assert res["n_frames"] == 3 and len(os.listdir(out)) == len(os.listdir(out + "_crop")) == 3 and n == 5
    for i in range(3):
        got = np.asarray(Image.open(os.path.join(out + "_crop", "frame%06d.png" % i)))
        assert got.shape == (2 * S, S + max(w * S // h, S), 3)
        _mesh_check(np.asarray(Image.open(os.path.join(out, "frame%06d.png" % i))), gold[key + "_full"][i], gold[key + "_amb_og"][i],
                    1, "full frame")
        _mesh_check(got[:S, :S], gold[key + "_rend_crop"][i], gold[key + "_amb_crop"][i], 1, "rend_crop")
