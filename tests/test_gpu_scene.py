"""hmmr_render_scene (csrc/render.hip) against hmmr_render_mesh, bit for bit, and against the NumPy spec (tests/scene_oracle.py).
Agreement with the spec, as for the mesh renderer: `owner` and `face_index` equal the oracle's on every non-ambiguous
subpixel; where all four subpixels of a pixel are non-ambiguous, alpha is exact and RGB within 1 LSB.  The cases are
seeded in scene_oracle.case; tests/test_scene_oracle.py holds them under 1 % ambiguous subpixels without a GPU.

Observed on an MI355X (pytest -s prints the figures): see DESIGN.md 4.7.

Which test catches which mutation of the kernel:
  order ascending instead of descending ......... test_three_overlapping_tracks (owner), test_order_default_priority_and_ties
  f <= end instead of f < end .................... test_range_edges (track 0 absent at its end; frame 4 empty)
  no owner lock (nearer local z of a farther
  person wins) ................................... test_three_overlapping_tracks (the owner is the farther in z'), test_order_...
  the colour of the wrong track .................. test_three_overlapping_tracks (rgb), test_one_track_equals_render_mesh (rgb)
  row f instead of f - start ..................... test_range_edges, test_three_overlapping_tracks (rows differ per frame)
  a tie going to the higher track index .......... test_order_default_priority_and_ties (identical twins: owner 0)
"""
import os

import numpy as np
import pytest

import scene_oracle as SO

pytestmark = pytest.mark.gpu


def _mods():
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.util.render import raster, video
    return L, raster, video


def _upload(tracks, dev):
    import torch
    return [{"verts": torch.as_tensor(t["verts"], device=dev), "cams": torch.as_tensor(t["cams"], device=dev), "range": t["range"],
             "geom": t["geom"], "priority": t.get("priority")} for t in tracks]


def _scene(c, dev, tracks=None, n_frames=None, frames=None, mode="frame"):
    """one hmmr_render_scene call on a case (or on other tracks / frames of its geometry) -> host arrays"""
    import torch
    L, raster, _ = _mods()
    tracks = c["tracks"] if tracks is None else tracks
    n = c["n_frames"] if n_frames is None else n_frames
    frames = c["frames"][:n] if frames is None else frames
    kw = dict(bg_mode=L.RENDER_BG_FRAME, bg_image=torch.as_tensor(frames, device=dev)) if mode == "frame" else {}
    r = raster.render_scene(_upload(tracks, dev), c["faces"], c["S"], n, colors=[t["color"] for t in tracks], out_hw=c["out_hw"],
                            want_alpha=True, want_index=True, want_owner=True, **kw)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.fixture(scope="module")
def rendered(gpu_device):
    """the cases' GPU frames, rendered once per (case, mode, reverse)"""
    cache = {}

    def get(name, mode="frame", reverse=False):
        if (name, mode, reverse) not in cache:
            c = SO.case(name)
            tracks = c["tracks"]
            if reverse:
                tracks = [dict(t, priority=np.full(t["range"][1] - t["range"][0], float(i), np.float32)) for i, t in enumerate(tracks)]
            cache[(name, mode, reverse)] = _scene(c, gpu_device, tracks=tracks, mode=mode)
        return cache[(name, mode, reverse)]
    return get


def _check(got, ref, label):
    """the criterion of the module docstring over all frames; prints the worst RGB difference and the ambiguous share"""
    worst, amb_share = 0, 0.0
    for f, r in enumerate(ref):
        amb, pa = r["ambiguous"], r["pixel_ambiguous"]
        d = np.abs(got["rgb"][f].astype(np.int32) - r["rgb"].astype(np.int32))
        worst, amb_share = max(worst, int(d[~pa].max(initial=0))), max(amb_share, float(amb.mean()))
    print("%s: worst rgb difference %d LSB off ambiguous pixels, ambiguous subpixels at most %.4f %% of a raster"
          % (label, worst, 100 * amb_share))
    for f, r in enumerate(ref):
        amb, pa = r["ambiguous"], r["pixel_ambiguous"]
        assert np.array_equal(got["owner"][f][~amb], r["owner"][~amb]), (label, f, (got["owner"][f][~amb] != r["owner"][~amb]).sum())
        assert np.array_equal(got["index"][f][~amb], r["index"][~amb]), (label, f)
        assert np.array_equal(got["alpha"][f][~pa], r["alpha"][~pa]), (label, f)
        d = np.abs(got["rgb"][f].astype(np.int32) - r["rgb"].astype(np.int32))
        assert d[~pa].max(initial=0) <= 1, (label, f, d[~pa].max())
        assert amb.mean() < 0.01


# ---------------------------------------------------------------------------------------------------------- 1. T = 1
@pytest.mark.parametrize("name", ["three48", "three80"])
def test_one_track_equals_render_mesh(name, gpu_device):
    import torch
    L, raster, _ = _mods()
    c = SO.case(name)
    for t in c["tracks"]:
        m = t["range"][1] - t["range"][0]
        got = _scene(c, gpu_device, tracks=[dict(t, range=(0, m))], n_frames=m)
        ref = raster.render_mesh(torch.as_tensor(t["verts"], device=gpu_device), torch.as_tensor(t["cams"], device=gpu_device),
                                 c["faces"], c["S"], geom=t["geom"], color=t["color"], bg_mode=L.RENDER_BG_FRAME,
                                 bg_image=torch.as_tensor(c["frames"][:m], device=gpu_device), out_hw=c["out_hw"],
                                 want_alpha=True, want_index=True)
        assert (ref["index"] >= 0).any()
        for k in ("rgb", "alpha", "index"):
            assert np.array_equal(got[k], ref[k].cpu().numpy()), (name, k)
        assert np.array_equal(got["owner"], np.where(got["index"] >= 0, 0, -1))


# ------------------------------------------------------------------------------------------ 2. three overlapping tracks
@pytest.mark.parametrize("name", ["three48", "three80"])
def test_three_overlapping_tracks(name, rendered):
    c, ref, got = SO.case(name), SO.reference(name), rendered(name)
    assert [t["range"] for t in c["tracks"]] == [(0, 4), (1, 6), (3, 5)] and c["n_frames"] == 6
    _check(got, ref, name)
    # layering beats local depth: where the GPU says track 0 owns a subpixel that track 1 covers too, 0 is the FARTHER in z'
    r = ref[3]
    (i0, p0), (i1, p1) = r["solo"][0], r["solo"][1]
    both = (i0 >= 0) & (i1 >= 0) & ~r["ambiguous"] & (got["owner"][3] == 0)
    z0, z1 = SO.depth_at(p0, c["faces"], c["S"], i0), SO.depth_at(p1, c["faces"], c["S"], i1)
    assert both.sum() > 100 and (z0[both] > z1[both]).all()


# --------------------------------------------------------------------------------------------------------- 3. the order
def test_order_default_priority_and_ties(rendered, gpu_device):
    c = SO.case("pair80")
    ref, got = SO.reference("pair80"), rendered("pair80")
    assert ref[0]["order"] == [0, 1]                                      # the default key: the larger camera scale in front
    _check(got, ref, "pair80 default")
    rev_ref, rev = SO.reference("pair80", "frame", True), rendered("pair80", "frame", True)
    assert rev_ref[0]["order"] == [1, 0]
    _check(rev, rev_ref, "pair80 priority")
    r = ref[0]
    both = (r["solo"][0][0] >= 0) & (r["solo"][1][0] >= 0) & ~r["ambiguous"]
    assert both.sum() > 100 and (got["owner"][0][both] == 0).all() and (rev["owner"][0][both] == 1).all()
    # identical twins (rows and keys bit-identical; another colour): the lower track index owns everything both cover
    t0 = c["tracks"][0]
    twins = _scene(c, gpu_device, tracks=[t0, dict(t0, color=SO.COLORS[1])])
    alone = _scene(c, gpu_device, tracks=[t0])
    assert (twins["owner"] == 0).any() and not (twins["owner"] == 1).any()
    for k in ("rgb", "alpha", "index", "owner"):
        assert np.array_equal(twins[k], alone[k]), k
    # ... also with explicit equal keys, and a non-finite key sorts last although nan > x is false either way
    eq = np.zeros(2, np.float32)
    twins = _scene(c, gpu_device, tracks=[dict(t0, priority=eq), dict(t0, color=SO.COLORS[1], priority=eq)])
    assert np.array_equal(twins["owner"], alone["owner"]) and np.array_equal(twins["rgb"], alone["rgb"])
    nan = _scene(c, gpu_device, tracks=[dict(c["tracks"][0], priority=np.full(2, np.nan, np.float32)),
                                        dict(c["tracks"][1], priority=np.full(2, -1e30, np.float32))])
    assert np.array_equal(nan["owner"], rev["owner"]) and np.array_equal(nan["rgb"], rev["rgb"])


# ---------------------------------------------------------------------------------------------------- 4. the range edges
def test_range_edges(rendered):
    import render_oracle as O
    c, ref, got = SO.case("edges48"), SO.reference("edges48"), rendered("edges48")
    assert [t["range"] for t in c["tracks"]] == [(1, 3), (2, 4)]
    _check(got, ref, "edges48")                                           # rows f - start: the tracks' rows differ per frame
    own = got["owner"]
    assert (own[1] == 0).any() and (own[2] == 0).any() and not (own[3] == 0).any()      # drawn at start and end - 1, absent at end
    assert not (own[1] == 1).any() and (own[2] == 1).any() and (own[3] == 1).any()
    for f in (0, 4):                                                      # nobody: the resized frame, byte for byte
        assert (own[f] == -1).all() and (got["index"][f] == -1).all() and (got["alpha"][f] == 0).all()
        assert np.array_equal(got["rgb"][f], O.resize_frame(c["frames"][f], *c["out_hw"]).astype(np.uint8))
        assert np.array_equal(got["rgb"][f], ref[f]["rgb"])


# -------------------------------------------------------------------------------------------------- 5. reproducibility
def _frame_alone(c, f, dev):
    """frame f as a 1-frame call on the tracks present, ranges shifted to (0, 1); the owners mapped back to the case's tracks"""
    ids = [i for i, t in enumerate(c["tracks"]) if t["range"][0] <= f < t["range"][1]]
    tracks = []
    for i in ids:
        t, r = c["tracks"][i], f - c["tracks"][i]["range"][0]
        tracks.append(dict(t, verts=t["verts"][r:r + 1], cams=t["cams"][r:r + 1], geom=t["geom"][r:r + 1], range=(0, 1)))
    one = _scene(c, dev, tracks=tracks, n_frames=1, frames=c["frames"][f:f + 1])
    one["owner"] = np.where(one["owner"] >= 0, np.asarray(ids)[np.maximum(one["owner"], 0)], -1)
    return one


def test_same_bytes_twice_and_a_frame_alone(rendered, gpu_device):
    c, a = SO.case("three48"), rendered("three48")
    b = _scene(c, gpu_device)
    for k in ("rgb", "alpha", "index", "owner"):
        assert np.array_equal(a[k], b[k]), k
    for f in range(c["n_frames"]):
        one = _frame_alone(c, f, gpu_device)
        for k in ("rgb", "alpha", "index", "owner"):
            assert np.array_equal(one[k][0], a[k][f]), (f, k)


def test_seventy_frames_equal_seventy_single_frame_calls(gpu_device):
    c = SO.case("slab16")                                                 # two tracks: slabs of 32 frames, so 70 frames are three
    assert c["n_frames"] == 70 and len(c["tracks"]) == 2 and len(c["faces"]) == 8 and c["S"] == 16
    a = _scene(c, gpu_device)
    assert all((a["owner"][f] == 0).any() for f in range(70)) and all((a["owner"][f] == 1).any() for f in (10, 31, 32, 63, 64))
    assert not (a["owner"][:10] == 1).any() and not (a["owner"][65:] == 1).any()
    for f in range(70):
        one = _frame_alone(c, f, gpu_device)
        for k in ("rgb", "alpha", "index", "owner"):
            assert np.array_equal(one[k][0], a[k][f]), (f, k)


# ------------------------------------------------------------------------------------------------- 6. background colour
def test_background_colour_mode(rendered):
    _check(rendered("three80", "color"), SO.reference("three80", "color"), "three80 colour")


# ------------------------------------------------------------------------------------------------ 7. the python drivers
def test_video_render_scene_and_render_tracks(gpu_device, tmp_path, monkeypatch):
    import torch
    from PIL import Image
    from human_dynamics_amd.evaluation import run_video
    L, raster, video = _mods()
    c = SO.case("video80")
    h, w, S = video.orig_output_size(c["frames"].shape[1:3], c["max_img"])
    assert (h, w) == c["out_hw"] and S == c["S"]
    # as predict_all_images / process_tracks return them: a dict of host arrays, no layout, the range, the images_orig dicts
    tracks = [({"cams": t["cams"], "verts": t["verts"]}, None, t["range"], t["params"]) for t in c["tracks"]]
    dev = torch.device(gpu_device)
    out = video.render_scene(tracks, c["frames"], c["faces"], max_img_size=c["max_img"], device=dev)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (7, h, w, 3) and out.device.type == "cuda"
    direct = raster.render_scene(_upload(c["tracks"], gpu_device), c["faces"], S, 7, bg_mode=L.RENDER_BG_FRAME,
                                 bg_image=torch.as_tensor(c["frames"], device=gpu_device), out_hw=(h, w))["rgb"]   # default colours
    assert torch.equal(out, direct)
    named = video.render_scene(tracks, c["frames"], c["faces"], max_img_size=c["max_img"], colors=['pink', (0.2, 0.9, 0.3)], device=dev)
    assert not torch.equal(named, out)
    # render_tracks: chunks of 3 cut both tracks; trim 1 -> frames 1 .. 5 as frame000000 .. frame000004
    monkeypatch.setenv("PATH", str(tmp_path / "nothing-here"))
    res = run_video.render_tracks(str(tmp_path / "scene"), tracks, c["frames"], faces=c["faces"], trim_length=1, chunk=3,
                                  max_img_size=c["max_img"], device=dev)
    assert res["n_frames"] == 5 and res["video"] is None and "no ffmpeg" in res["note"]
    assert sorted(os.listdir(tmp_path / "scene")) == ["frame%06d.png" % i for i in range(5)]
    host = out.cpu().numpy()
    for i in range(5):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "scene" / ("frame%06d.png" % i))), host[i + 1]), i
