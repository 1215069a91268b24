"""hmmr_render_mesh (csrc/render.hip) against the NumPy spec (tests/render_oracle.py) and the reference's VisRenderer glue
(tests/golden/reference_render.npz).  Agreement criterion everywhere: the face-index map equals the oracle's on every
non-ambiguous subpixel; where all four subpixels of a pixel are non-ambiguous, alpha is exact and RGB within 1 LSB."""
import os

import numpy as np
import pytest

import render_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mods():
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.util.render import raster, video, mesh
    return L, raster, video, mesh


def _check(got, ref, max_amb=None):
    idx, rgb, alpha = got
    amb = ref["ambiguous"]
    assert np.array_equal(idx[~amb], ref["index"][~amb]), "face index differs on %d subpixels" % (idx[~amb] != ref["index"][~amb]).sum()
    pa = ref["pixel_ambiguous"]
    d = np.abs(rgb.astype(np.int32) - ref["rgb"].astype(np.int32))
    assert d[~pa].max(initial=0) <= 1, d[~pa].max()
    if alpha is not None:
        assert np.array_equal(alpha[~pa], ref["alpha"][~pa])
    if max_amb is not None:
        assert amb.mean() < max_amb, amb.mean()


def _render1(verts, cam, faces, S, gpu_device, **kw):
    import torch
    L, raster, _, _ = _mods()
    v = torch.as_tensor(np.asarray(verts, np.float32)[None], device=gpu_device)
    c = torch.as_tensor(np.asarray(cam, np.float32).reshape(1, 3), device=gpu_device)
    r = raster.render_mesh(v, c, faces, S, want_alpha=True, want_index=True, **kw)
    return r["index"][0].cpu().numpy(), r["rgb"][0].cpu().numpy(), r["alpha"][0].cpu().numpy()


# ------------------------------------------------------------------------------------------------ hand-built scenes
def _scene(name):
    """vertices in the unflipped camera (cam = [1, 0, 0]: q = (x, y), z' = z + 2.732) and faces"""
    t = lambda pts, z=0.0: [[x, y, z] for x, y in pts]
    if name == "one":
        return t([(-0.6, -0.5), (0.7, -0.2), (0.1, 0.8)]), [[0, 1, 2]]
    if name == "overlap":
        return t([(-0.8, -0.8), (0.8, -0.8), (0.0, 0.8)], 0.5) + t([(-0.7, -0.6), (0.9, -0.5), (0.1, 0.9)], -0.4), [[0, 1, 2], [3, 4, 5]]
    if name == "windings":
        v = t([(-0.9, -0.9), (0.0, -0.9), (-0.45, 0.2)]) + t([(0.1, -0.2), (0.9, -0.3), (0.5, 0.9)])
        v[2][2], v[5][2] = 0.4, -0.3
        return v, [[0, 1, 2], [5, 4, 3]]
    if name == "near":
        return [[-0.9, 0.9, 0.05 - 2.7320508], [0.9, 0.9, 2.0 - 2.7320508], [0.9, -0.9, 2.0 - 2.7320508],
                [-0.9, -0.9, 0.05 - 2.7320508]], [[0, 1, 2], [0, 2, 3]]
    if name == "offscreen":
        return t([(1.2, 1.2), (1.9, 1.3), (1.5, 1.9)]) + t([(-1.5, -0.3), (0.3, -1.4), (0.2, 0.4)]), [[0, 1, 2], [3, 4, 5]]
    if name == "tiny":
        return t([(0.0101, 0.0102), (0.0112, 0.0103), (0.0104, 0.0114)]) + t([(-0.5, -0.5), (-0.3, -0.5), (-0.4, -0.3)]), [[0, 1, 2], [3, 4, 5]]
    if name == "nan":
        v = t([(-0.6, -0.5), (0.7, -0.2), (0.1, 0.8)]) + t([(-0.9, 0.1), (0.2, 0.9), (-0.5, 0.9)])
        v[4][0] = float("nan")
        return v, [[0, 1, 2], [3, 4, 5], [0, 0, 1]]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one", "overlap", "windings", "near", "offscreen", "tiny", "nan"])
def test_hand_built_scenes(name, gpu_device):
    v, f = _scene(name)
    v, f = np.asarray(v, np.float32), np.asarray(f, np.int32)
    cam = np.array([1, 0, 0], np.float32)
    S = 32
    got = _render1(v, cam, f, S, gpu_device)
    ref = O.render(O.project(v, cam), f, S)
    _check(got, ref)
    if name != "offscreen" and name != "nan":
        assert (got[0] >= 0).sum() > 0
    if name == "nan":
        assert not (got[0] == 1).any() and not (got[0] == 2).any()


# ------------------------------------------------------------------------------------------------ the closed mesh
@pytest.mark.parametrize("S", [224, 300, 720])
def test_closed_smpl_sized_mesh_in_all_background_modes(S, gpu_device):
    import torch
    L, raster, _, mesh = _mods()
    rng = np.random.default_rng(S)
    v, f = mesh.deformed_sphere(seed=S)
    cam = np.array([rng.uniform(0.7, 1.1), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)], np.float32)
    p = O.project(v, cam)
    idx, amb = O.rasterize(p, f, S)
    cols = O.shade(p, f)
    base = {"index": idx, "ambiguous": amb}
    assert amb.mean() < 1e-3, amb.mean()
    assert (idx >= 0).mean() > 0.1
    # (1) background colour
    rgb, alpha = O.composite(idx, cols, S)
    _check(_render1(v, cam, f, S, gpu_device), dict(base, rgb=rgb, alpha=alpha, pixel_ambiguous=O.pixel_ambiguity(amb, S)))
    # (2) a float crop in [-1, 1] (visualize_img)
    crop = rng.uniform(-1, 1, (S, S, 3)).astype(np.float32)
    bgf = ((crop + np.float32(1)) * np.float32(0.5)) * np.float32(255)
    rgb, alpha = O.composite(idx, cols, S, bg=bgf, bg_kind='float')
    got = _render1(v, cam, f, S, gpu_device, bg_mode=L.RENDER_BG_FLOAT, bg_image=torch.as_tensor(crop[None], device=gpu_device),
                   bg_add=1.0, bg_mul=127.5)
    _check(got, dict(base, rgb=rgb, alpha=alpha, pixel_ambiguous=O.pixel_ambiguity(amb, S)))
    # (3) an original uint8 frame, larger than the raster: resized, then the top-left out_h x out_w kept (remove_pads)
    out_hw = (int(S * 0.6), S)
    frame = rng.integers(0, 256, (int(out_hw[0] * 1.7), int(S * 1.7), 3), dtype=np.uint8)
    bg = O.resize_frame(frame, *out_hw)
    rgb, alpha = O.composite(idx, cols, S, bg=bg, bg_kind='frame', out_hw=out_hw)
    got = _render1(v, cam, f, S, gpu_device, bg_mode=L.RENDER_BG_FRAME, bg_image=torch.as_tensor(frame[None], device=gpu_device),
                   out_hw=out_hw)
    _check(got, dict(base, rgb=rgb, alpha=alpha, pixel_ambiguous=O.pixel_ambiguity(amb, S, out_hw)))


def test_rotated_view_and_orig_geometry_match_the_spec(gpu_device):
    """The rotation about the centroid and the camera change to the original image (the handoff's device code)."""
    import torch
    L, raster, video, mesh = _mods()
    from human_dynamics_amd.util.render.handoff import orig_image_geometry
    from oracle import handoff_oracle as HO
    v, f = mesh.deformed_sphere(seed=3)
    cam = np.array([0.9, 0.05, -0.1], np.float32)
    params = {"start_pt": np.array([310, 250]), "scale": 0.8, "im_shape": [224, 224]}
    h, w, S = video.orig_output_size((480, 640), 300)
    geom = orig_image_geometry(params, (480, 640), 300)
    new_cam, _, _ = HO.orig_camera(cam, np.zeros((1, 2), np.float32), params["start_pt"], 1.0 / geom[0], 224, (h, w), 10 ** 6)
    R = raster.rodrigues(90, 'y')
    vr = O.rotate(v, R)
    p = O.project(vr, new_cam)
    ref = O.render(p, f, S, out_hw=(h, w))
    vt = torch.as_tensor(v[None], device=gpu_device)
    ct = torch.as_tensor(cam[None], device=gpu_device)
    r = raster.render_mesh(vt, ct, f, S, geom=geom[None], rot=R, out_hw=(h, w), want_alpha=True, want_index=True)
    _check((r["index"][0].cpu().numpy(), r["rgb"][0].cpu().numpy(), r["alpha"][0].cpu().numpy()), ref, max_amb=1e-3)


# ------------------------------------------------------------------------------------------------ the synthetic SMPL's soup
def test_triangle_soup_from_tester_records(weights, smpl_consts, gpu_device):
    import torch
    from conftest import Config
    from human_dynamics_amd import assets, dist as hd
    from human_dynamics_amd.evaluation.tester import Tester
    L, raster, video, mesh = _mods()
    _, faces = mesh.latlong_sphere()
    t = Tester(Config(batch_size=2), weights=weights, smpl=smpl_consts, dtype="f32", device=gpu_device)
    n = 24
    frames = torch.from_numpy(assets.make_synthetic_frames(n, seed=7)).to(gpu_device)
    sp = hd.ShardedPredictor(t, n, 0, 1)
    rec = sp.run(frames)
    views = video.render_views(rec, sp.layout, np.zeros((n, 8, 8, 3), np.uint8), None, faces, crops=frames,
                               views=('crop',))["crop"].cpu().numpy()
    un = hd.unpack_outputs(rec, sp.layout)
    cams, verts = un["cams"].cpu().numpy(), un["verts"].cpu().numpy()
    S = 224
    idx_all = raster.render_mesh(torch.as_tensor(verts, device=gpu_device), torch.as_tensor(cams, device=gpu_device),
                                 faces, S, want_index=True)["index"].cpu().numpy()
    rng = np.random.default_rng(0)
    for i in (0, n - 1):
        p = O.project(verts[i], cams[i])
        px = rng.integers(0, S, (300, 2))
        rows = (2 * px[:, :1] + np.array([[0, 0, 1, 1]])).reshape(-1)
        cols = (2 * px[:, 1:] + np.array([[0, 1, 0, 1]])).reshape(-1)
        idx, amb = O.rasterize_points(p, faces, S, rows, cols)
        ok = ~amb
        assert np.array_equal(idx_all[i][rows, cols][ok], idx[ok])
        assert (idx >= 0).mean() > 0.1                      # faces spanning much of the image
        cols_f = O.shade(p, faces).astype(np.float32)
        sub = np.where(idx[:, None] >= 0, cols_f[np.maximum(idx, 0)], np.float32(1)).reshape(-1, 4, 3)
        pooled = ((sub[:, 0] + sub[:, 1]) + (sub[:, 2] + sub[:, 3])) * np.float32(0.25)
        a = ((idx >= 0).reshape(-1, 4).sum(1) * 0.25).astype(np.float32)[:, None]
        bg = ((frames[i].cpu().numpy()[px[:, 0], px[:, 1]] + np.float32(1)) * np.float32(0.5)) * np.float32(255)
        exp = (bg * (np.float32(1) - a) + (np.clip(pooled, 0, 1) * np.float32(255)) * a).astype(np.uint8)
        pok = ~amb.reshape(-1, 4).any(1)
        d = np.abs(views[i][px[:, 0], px[:, 1]].astype(int) - exp.astype(int))
        assert d[pok].max(initial=0) <= 1


# ------------------------------------------------------------------------------------------------ reproducibility, sizes
def test_bit_identical_runs_batch_equals_alone_and_4096_frames(gpu_device):
    import torch
    L, raster, _, mesh = _mods()
    v, f = mesh.deformed_sphere(seed=1)
    n = 300
    rng = np.random.default_rng(5)
    verts = torch.as_tensor(v[None] + rng.normal(0, 0.02, (n, 1, 3)).astype(np.float32), device=gpu_device)
    cams = torch.as_tensor(np.stack([rng.uniform(0.6, 1.2, n), rng.uniform(-.3, .3, n), rng.uniform(-.3, .3, n)], 1)
                           .astype(np.float32), device=gpu_device)
    a = raster.render_mesh(verts, cams, f, 96, want_alpha=True, want_index=True)
    b = raster.render_mesh(verts, cams, f, 96, want_alpha=True, want_index=True)
    for k in ("rgb", "alpha", "index"):
        assert torch.equal(a[k], b[k])
    for i in (0, 77, 299):
        one = raster.render_mesh(verts[i:i + 1], cams[i:i + 1], f, 96, want_alpha=True, want_index=True)
        for k in ("rgb", "alpha", "index"):
            assert torch.equal(one[k][0], a[k][i])
    big = 4096
    vb = verts[torch.arange(big, device=gpu_device) % n]
    cb = cams[torch.arange(big, device=gpu_device) % n]
    r = raster.render_mesh(vb, cb, f, 64, want_index=True)
    torch.cuda.synchronize()
    ref = raster.render_mesh(verts, cams, f, 64, want_index=True)
    assert torch.equal(r["rgb"][n + 5], ref["rgb"][5]) and torch.equal(r["rgb"][big - 1], ref["rgb"][(big - 1) % n])
    assert (r["index"] >= 0).any(dim=(1, 2)).all()


# ------------------------------------------------------------------------------------------------ the reference's glue
def test_vis_renderer_against_the_reference_fixture(gpu_device):
    from human_dynamics_amd.util.render.nmr_renderer import VisRenderer
    g = np.load(os.path.join(GOLD, "reference_render.npz"))
    faces = g["faces"]
    n_amb = 0
    import re
    for key in [k for k in g.files if re.fullmatch(r"case_\d+", k)]:
        spec = g[key + "_spec"]            # [kind, S, batch, rend_mask, alpha, img, rotate]
        kind, S, batch, rend_mask, alpha, has_img, rot = (int(x) for x in spec)
        r = VisRenderer(S, faces=faces, device=gpu_device)
        kw = dict(cam=g[key + "_cam"], rend_mask=bool(rend_mask), alpha=bool(alpha))
        if rot:
            got = r.rotated(g[key + "_verts"], 90, **kw)
        else:
            got = r(g[key + "_verts"], img=g[key + "_img"] if has_img else None, **kw)
        want = g[key]
        amb = g[key + "_amb"]                 # pixels the oracle flagged (any subpixel), broadcast over channels
        assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape)
        d = np.abs(got.astype(int) - want.astype(int))
        mask = np.broadcast_to(amb.reshape(amb.shape + (1,) * (d.ndim - amb.ndim)), d.shape) if amb.shape != d.shape else amb
        assert d[~mask].max(initial=0) <= 1, key
        n_amb += int(mask.sum())


def test_render_views_against_the_reference_fixture(gpu_device):
    """render_preds' three mesh panels (visualize_img_orig's rend_img and rotated view, visualize_img on the crop), one
    frame per call here, against the reference's own glue around the spec."""
    import torch
    _, _, video, _ = _mods()
    g = np.load(os.path.join(GOLD, "reference_render.npz"))
    faces = g["faces"]
    for k in range(len(g["orig_params"])):
        b = "orig_%d" % k
        sx, sy, scale, max_img = g[b + "_params"]
        preds = {"cams": g[b + "_cam"][None], "verts": g[b + "_verts"][None]}
        params = [{"start_pt": np.array([sx, sy]), "scale": scale, "im_shape": [224, 224]}]
        out = video.render_views(preds, None, g[b + "_frame"][None], params, faces, crops=g[b + "_crop"][None],
                                 max_img_size=int(max_img), device=torch.device(gpu_device))
        for view, key, amb in (("orig", "_rend", "_amb"), ("rotated", "_rot", "_amb_rot"), ("crop", "_rend_crop", "_amb_crop")):
            got, want, a = out[view][0].cpu().numpy(), g[b + key], g[b + amb]
            assert got.shape == want.shape, (b, view, got.shape, want.shape)
            d = np.abs(got.astype(int) - want.astype(int))
            assert d[~a].max(initial=0) <= 1, (b, view, d[~a].max())
