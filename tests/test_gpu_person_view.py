"""The person-centred view on the device: hmmr_video_bbox (csrc/person_view.hip) against the reference-executed fixture
(tests/golden/reference_video_bbox.npz) and the float64 restatement (tests/person_view_oracle.py), the two drop-ins of
util/render/nmr_renderer.py, and the whole-video drivers util/render/video.render_person_clips and
evaluation/run_video.render_person_clips.  Run with -s for the largest observed differences
(profiles/person_view_gpu_tests.log is one such run)."""
import os
import warnings

import numpy as np
import pytest

import person_view_oracle as PV
import render_oracle as RO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_video_bbox.npz")))


def camera_bound(want):
    """2^-23 |ref| + 1e-12: one fp32 rounding of the result plus the fp64 error of the cancelling o12 - S / (2 o0) terms (order 1e3)"""
    return 2.0 ** -23 * np.abs(want.astype(np.float64)) + 1e-12


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _call(dev, cams, kps, proc, offsets, hw, margin):
    """one hmmr_video_bbox call on host arrays cams [N,3], kps [N,k,2], proc [N,3] -> host (bbox, cams_crop, status)"""
    import torch
    from human_dynamics_amd.util.render import person_view
    n, k = kps.shape[0], kps.shape[1]
    bbox, crop, st = person_view.video_bbox(torch.as_tensor(np.ascontiguousarray(cams, np.float32), device=dev).reshape(n, 3),
                                            torch.as_tensor(np.ascontiguousarray(kps, np.float32), device=dev).reshape(n, 2 * k), k,
                                            torch.as_tensor(np.ascontiguousarray(proc, np.float64), device=dev).reshape(n, 3), offsets, hw, margin)
    return bbox.cpu().numpy(), crop.cpu().numpy(), st.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the fixture
def test_kernel_equals_the_reference_fixture(ref, gpu_device):
    off = ref["offsets"]
    worst_abs, worst_rel, differing = 0.0, 0.0, 0
    for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
        h, w, margin = (int(x) for x in ref["meta"][t])
        bbox, crop, st = _call(gpu_device, ref["cams"][a:b], ref["kps"][a:b], ref["proc"][a:b], [0, b - a], (h, w), margin)
        assert np.array_equal(bbox[0], ref["bbox"][t]), (t, bbox, ref["bbox"][t])
        assert st[0] == (PV.BEYOND_START if ref["trap"][a:b].any() else 0), (t, st)
        want = ref["cams_crop"][a:b]
        err = np.abs(crop.astype(np.float64) - want)
        worst_abs, worst_rel = max(worst_abs, float(err.max())), max(worst_rel, float((err / camera_bound(want)).max()))
        differing += int((_bits(crop) != _bits(want)).sum())
        assert (err <= camera_bound(want)).all(), (t, float(err.max()))
    print("\nkernel vs reference fixture (9 tracks, %d cameras): boxes and status equal; largest camera difference %.3e (%.3f of the bound "
          "2^-23 |ref| + 1e-12); %d of %d values differ in any bit" % (off[-1], worst_abs, worst_rel, differing, 3 * off[-1]))


# ------------------------------------------------------------------------------------------------ the ragged call
LENGTHS = (1, 0, 255, 256, 257, 600)
# (track, frame that holds the smallest ymin / xmin, frame that holds the largest ymax / xmax): first frame, last frame, the last lane
# of a pass (frames 255 and 511: the workgroup has 256 lanes)
PLANTED = ((2, 0, 254), (3, 255, 0), (4, 256, 255), (5, 511, 599))
LD = 90


def _ragged_case(k, seed=0):
    """records-like rows [N, 90]: the camera in columns 0..2, the keypoints from column 3; the tracks of LENGTHS, then good / NaN /
    good tracks of 5 frames"""
    rng = np.random.default_rng(seed + k)
    lengths = list(LENGTHS) + [5, 5, 5]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    n = int(offsets[-1])
    rows = rng.normal(size=(n, LD)).astype(np.float32)                  # whatever else a record holds
    rows[:, 0] = rng.uniform(0.5, 1.2, n)
    rows[:, 1:3] = rng.uniform(-0.3, 0.3, (n, 2))
    rows[:, 3:3 + 2 * k] = rng.uniform(-0.5, 0.5, (n, 2 * k))          # within 56 pixels of the centre at these scales
    scale = rng.uniform(1.0, 1.4, n)
    centre = np.array([640., 360.]) + np.clip(rng.normal(0, 5, (n, 2)), -15, 15)
    for trk, lo, hi in PLANTED:                                         # 220 pixels away: beyond what keypoints and jitter can make up, within the frame
        centre[offsets[trk] + lo] -= 220
        centre[offsets[trk] + hi] += 220
    proc = np.concatenate([scale[:, None], np.round(centre * scale[:, None]) + 112], 1)
    nan_track = len(LENGTHS) + 1
    rows[offsets[nan_track] + 2, 3 + 2 * k - 1] = np.nan                # the last keypoint value of one frame of the middle track
    return rows, proc, offsets, nan_track


def _ragged_run(dev, rows, proc, offsets, k, hw=(720, 1280), margin=10):
    import torch
    from human_dynamics_amd.util.render import person_view
    buf = torch.as_tensor(rows, device=dev)
    bbox, crop, st = person_view.video_bbox(buf[:, 0:3], buf[:, 3:3 + 2 * k], k, torch.as_tensor(proc, device=dev), offsets, hw, margin)
    return bbox.cpu().numpy(), crop.cpu().numpy(), st.cpu().numpy()


def _oracle(rows, proc, offsets, k, hw=(720, 1280), margin=10):
    n = rows.shape[0]
    return PV.video_bbox(rows[:, 0:3], rows[:, 3:3 + 2 * k].reshape(n, k, 2), proc, 224., offsets, hw[0], hw[1], margin)


@pytest.mark.parametrize("k", [1, 19, 25])
def test_ragged_call_equals_the_oracle_and_every_track_its_own_call(k, gpu_device):
    import torch
    from human_dynamics_amd.util.render import person_view
    rows, proc, offsets, nan_track = _ragged_case(k)
    want = _oracle(rows, proc, offsets, k)
    bbox, crop, st = _ragged_run(gpu_device, rows, proc, offsets, k)
    assert np.array_equal(bbox, want["bbox"]) and np.array_equal(st, want["status"]), (bbox, want["bbox"], st, want["status"])
    # the planted frames decide the box: the extreme sits where it was put
    n = rows.shape[0]
    ext = PV.frame_extremes(np.nan_to_num(rows[:, 3:3 + 2 * k]).reshape(n, k, 2), proc, 224., 720, 1280, 10)
    for trk, lo, hi in PLANTED:
        a, b = offsets[trk], offsets[trk + 1]
        assert ext[a:b, 0].argmin() == lo == ext[a:b, 2].argmin() and ext[a:b, 1].argmax() == hi == ext[a:b, 3].argmax(), trk
    assert st[1] == PV.EMPTY and not bbox[1].any()
    assert st[nan_track] == PV.NOT_FINITE and not bbox[nan_track].any()
    assert np.isnan(crop[offsets[nan_track]:offsets[nan_track + 1]]).all()
    assert st[nan_track - 1] in (0, PV.BEYOND_START) and st[nan_track + 1] in (0, PV.BEYOND_START)
    good = want["written"] & ~np.isnan(want["cams_crop"]).any(1)
    err = np.abs(crop[good].astype(np.float64) - want["cams_crop"][good])
    assert (err <= camera_bound(want["cams_crop"][good])).all(), float(err.max())
    print("\nragged call, k = %d: boxes and status equal the oracle; largest camera difference %.3e (%.3f of the bound); %d of %d values "
          "differ in any bit" % (k, float(err.max()), float((err / camera_bound(want["cams_crop"][good])).max()),
                                 int((_bits(crop[good]) != _bits(want["cams_crop"][good])).sum()), 3 * int(good.sum())))
    # two runs are identical; every track equals its own single-track call (on its rows of the same buffer) bit for bit
    bbox2, crop2, st2 = _ragged_run(gpu_device, rows, proc, offsets, k)
    assert np.array_equal(bbox, bbox2) and np.array_equal(st, st2) and np.array_equal(_bits(crop), _bits(crop2))
    buf, dproc = torch.as_tensor(rows, device=gpu_device), torch.as_tensor(proc, device=gpu_device)
    for t in range(len(offsets) - 1):
        a, b = int(offsets[t]), int(offsets[t + 1])
        b1, c1, s1 = person_view.video_bbox(buf[a:b, 0:3], buf[a:b, 3:3 + 2 * k], k, dproc[a:b], [0, b - a], (720, 1280), 10)
        assert np.array_equal(b1.cpu().numpy()[0], bbox[t]) and int(s1[0]) == st[t], t
        assert np.array_equal(_bits(c1.cpu().numpy()), _bits(crop[a:b])), t


def test_sixty_five_tracks_cross_the_chunk_of_sixty_four(gpu_device):
    k = 25
    rng = np.random.default_rng(65)
    n = 65 * 3
    offsets = (3 * np.arange(66)).astype(np.int32)
    rows = rng.normal(size=(n, LD)).astype(np.float32)
    rows[:, 0] = rng.uniform(0.5, 1.2, n)
    rows[:, 3:3 + 2 * k] = rng.uniform(-0.8, 0.8, (n, 2 * k))
    scale = rng.uniform(0.5, 2.0, n)
    centre = np.repeat(rng.uniform([100, 100], [1180, 620], (65, 2)), 3, 0) + rng.normal(0, 5, (n, 2))      # every person somewhere else
    proc = np.concatenate([scale[:, None], np.round(centre * scale[:, None]) + 112], 1)
    want = _oracle(rows, proc, offsets, k)
    bbox, crop, st = _ragged_run(gpu_device, rows, proc, offsets, k)
    assert np.array_equal(bbox, want["bbox"]) and np.array_equal(st, want["status"])
    assert len(set(map(tuple, bbox))) == 65                             # (a track that read its neighbour's rows would repeat a box)
    err = np.abs(crop.astype(np.float64) - want["cams_crop"])
    assert (err <= camera_bound(want["cams_crop"])).all(), float(err.max())


# ------------------------------------------------------------------------------------------------ the two drop-ins
def _small_mesh():
    from human_dynamics_amd.util.render import mesh
    v, f = mesh.deformed_sphere(seed=2, n_lon=14, n_rings=12)
    assert v.shape == (170, 3)
    return v, f


def test_compute_video_bbox_equals_the_fixture(ref, gpu_device):
    import torch
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.util.render.nmr_renderer import compute_video_bbox
    off = ref["offsets"]
    for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
        h, w, margin = (int(x) for x in ref["meta"][t])
        infos = [{"scale": float(p[0]), "start_pt": p[1:3].astype(int), "im_shape": [224, 224]} for p in ref["proc"][a:b]]
        cams, kps = ref["cams"][a:b], ref["kps"][a:b]
        if t % 3 == 1:                                                  # host arrays, device tensors, and the reference's per-frame lists alike
            cams, kps = torch.as_tensor(cams, device=gpu_device), torch.as_tensor(kps, device=gpu_device)
        elif t % 3 == 2:
            cams, kps = list(torch.as_tensor(cams, device=gpu_device)), list(torch.as_tensor(kps, device=gpu_device))
        elif t == 3:
            cams, kps = list(cams), list(kps)
        bbox, new_cams, status = compute_video_bbox(cams, kps, infos, margin=margin, img_shape=(h, w), status=True)
        assert np.array_equal(bbox, ref["bbox"][t]) and bbox.shape == (4,) and bbox.dtype.kind == "i"
        assert isinstance(new_cams, list) and len(new_cams) == b - a and new_cams[0].dtype == np.float32 and new_cams[0].shape == (3,)
        err = np.abs(np.stack(new_cams).astype(np.float64) - ref["cams_crop"][a:b])
        assert (err <= camera_bound(ref["cams_crop"][a:b])).all()
        assert status == (L.BBOX_BEYOND_START if ref["trap"][a:b].any() else 0)
        two = compute_video_bbox(cams, kps, infos, margin=margin, img_shape=(h, w))
        assert len(two) == 2 and np.array_equal(two[0], bbox)


def test_visualize_mesh_og_equals_rotated_with_the_recorded_camera(ref, gpu_device):
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.util.render.nmr_renderer import VisRenderer, visualize_mesh_og
    v, f = _small_mesh()
    renderer = VisRenderer(img_size=224, faces=f, device=gpu_device)
    seen, drawn = set(), 0
    for m, cam in zip(ref["og_meta"], ref["og_cam"]):
        case, row, h, w, max_img, deg, boxed, size = (int(x) for x in m)
        if size > L.RENDER_MAX_SIZE:                                     # (1080 and 1280: recorded, beyond the rasteriser; the CPU test checks them)
            continue
        seen.add((boxed, max(h, w) > max_img if not boxed else size == max_img, deg))
        renderer.renderer.image_size = 1
        got = visualize_mesh_og(ref["cams"][row], v, renderer, ref["proc"][row, 1:3].astype(int), float(ref["proc"][row, 0]), [224, 224],
                                img=np.zeros((h, w, 3)), deg=deg, max_img_size=max_img, crop_cam=ref["cams_crop"][row] if boxed else None,
                                bbox=ref["bbox"][case] if boxed else None)
        assert renderer.renderer.image_size == size
        want = renderer.rotated(v, deg, cam=cam)
        assert got.shape == (size, size, 3) and got.dtype == np.uint8 and np.array_equal(got, want), m
        drawn += int((got != 255).any())
    assert seen == {(b, r, d) for b in (0, 1) for r in (False, True) for d in (0, 90)}      # both branches, resized or not, both angles
    assert drawn >= 8


# ------------------------------------------------------------------------------------------------ the clips
@pytest.fixture(scope="module")
def clip_case(gpu_device):
    import torch
    v, f = _small_mesh()
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (4, 96, 128, 3), dtype=np.uint8)
    tracks, host = [], []
    for (start, end), centre, scale in (((0, 3), (64., 48.), 2.5), ((2, 4), (44., 50.), 3.0), ((2, 2), (0., 0.), 1.0)):
        n = end - start
        verts = (v[None] + rng.normal(0, 0.01, (n, 1, 3))).astype(np.float32)
        cams = np.stack([rng.uniform(0.85, 0.95, n), rng.uniform(-.05, .05, n), rng.uniform(-.05, .05, n)], 1).astype(np.float32)
        # 25 "joints": the four vertices that bound the mesh in x and y, and 21 others -- so the box must hold the whole mesh
        ends = [int(fn(v[:, a])) for a in (0, 1) for fn in (np.argmin, np.argmax)]
        pick = np.concatenate([np.unique(ends), rng.choice(np.setdiff1d(np.arange(170), ends), 25 - len(np.unique(ends)), replace=False)])
        kps = (cams[:, None, :1] * (verts[:, pick, :2] + cams[:, None, 1:])).astype(np.float32)        # the projection the model's kps are
        sc = scale * rng.uniform(0.98, 1.02, n)
        c = np.asarray(centre)[None] + rng.normal(0, 1.0, (n, 2))
        params = [{"scale": float(sc[i]), "start_pt": (np.round(c[i] * sc[i]) + 112).astype(int), "im_shape": [224, 224]} for i in range(n)]
        rec = {"cams": torch.as_tensor(cams, device=gpu_device), "kps": torch.as_tensor(kps, device=gpu_device),
               "verts": torch.as_tensor(verts, device=gpu_device)}
        tracks.append((rec, None, (start, end), params))
        proc = np.array([[p["scale"], p["start_pt"][0], p["start_pt"][1]] for p in params], np.float64).reshape(n, 3)
        host.append({"cams": cams, "kps": kps, "verts": verts, "proc": proc})
    return {"tracks": tracks, "host": host, "frames": frames, "faces": f}


def _oracle_track(hst, hw, margin):
    n = len(hst["cams"])
    return PV.video_bbox(hst["cams"], hst["kps"], hst["proc"], 224., [0, n], hw[0], hw[1], margin)


def test_person_clips_on_white_equal_render_mesh_with_the_oracle_cameras(clip_case, gpu_device):
    import torch
    from human_dynamics_amd.util.render import raster, video
    c = clip_case
    with pytest.warns(UserWarning, match="track 2"):
        out = video.render_person_clips(c["tracks"], c["frames"], c["faces"], degs=(0, 90), margin=10, background=False)
    assert len(out) == 3 and out[2]["views"] == {} and out[2]["status"] == PV.EMPTY and not np.any(out[2]["bbox"])
    for t in (0, 1):
        want = _oracle_track(c["host"][t], (96, 128), 10)
        assert np.array_equal(out[t]["bbox"], want["bbox"][0]) and out[t]["status"] == want["status"][0]
        h, w, S = PV.clip_size(want["bbox"][0], 300)
        assert out[t]["size"] == (h, w, S) and S >= 16
        for deg in (0, 90):
            ref_img = raster.render_mesh(c["tracks"][t][0]["verts"], torch.as_tensor(want["cams_crop"], device=gpu_device), c["faces"], S,
                                         rot=raster.rodrigues(deg, 'y'), color=raster.scene_color(t), out_hw=(h, w))["rgb"]
            got = out[t]["views"][deg]
            assert got.dtype == torch.uint8 and tuple(got.shape) == (len(c["host"][t]["cams"]), h, w, 3)
            assert torch.equal(got, ref_img), (t, deg)
            assert bool((got != 255).any())                              # the person is in the view
        # the whole mesh is inside the window at 0 degrees: no drawn pixel on the border of the clip
        g0 = out[t]["views"][0].cpu().numpy()
        border = np.concatenate([g0[:, 0].reshape(-1), g0[:, -1].reshape(-1), g0[:, :, 0].reshape(-1), g0[:, :, -1].reshape(-1)])
        assert (border == 255).all()


@pytest.mark.parametrize("max_img_size", [300, 48])
def test_person_clips_over_the_frames_window(clip_case, max_img_size, gpu_device):
    """background=True: the deg == 0 view lies over the frames' window (down-scaled to 48 pixels in the second case); where the mesh
    covers nothing the pixel is the resize oracle's.  The other view stays white."""
    import torch
    from human_dynamics_amd.util.render import raster, video
    c = clip_case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = video.render_person_clips(c["tracks"], torch.as_tensor(c["frames"], device=gpu_device), c["faces"], degs=(0, 90), margin=10,
                                        max_img_size=max_img_size, background=True)
        white = video.render_person_clips(c["tracks"], c["frames"], c["faces"], degs=(0, 90), margin=10, max_img_size=max_img_size,
                                          background=False)
    assert out[2]["views"] == {}
    for t in (0, 1):
        start, end = c["tracks"][t][2]
        y0, y1, x0, x1 = (int(x) for x in out[t]["bbox"])
        h, w, S = out[t]["size"]
        assert (h, w, S) == PV.clip_size(out[t]["bbox"], max_img_size) and S <= max_img_size
        assert torch.equal(out[t]["views"][90], white[t]["views"][90])
        _, crops, _ = video.video_bboxes(c["tracks"], (96, 128), 10)
        alpha = raster.render_mesh(c["tracks"][t][0]["verts"], crops[t], c["faces"], S, rot=raster.rodrigues(0, 'y'), out_hw=(h, w),
                                   want_alpha=True)["alpha"].cpu().numpy()
        got = out[t]["views"][0].cpu().numpy()
        for i, f in enumerate(range(start, end)):
            bg = RO.resize_frame(c["frames"][f, y0:y1, x0:x1], h, w).astype(np.uint8)
            clear = alpha[i] == 0
            assert clear.mean() > 0.3 and (~clear).mean() > 0.05
            assert np.array_equal(got[i][clear], bg[clear]), (t, f, int(np.abs(got[i][clear].astype(int) - bg[clear]).max()))
            assert np.array_equal(got[i][alpha[i] == 1], white[t]["views"][0].cpu().numpy()[i][alpha[i] == 1])


def test_run_video_writes_one_folder_per_person(clip_case, gpu_device, tmp_path, monkeypatch):
    from PIL import Image
    from human_dynamics_amd.evaluation import run_video
    from human_dynamics_amd.util.render import video
    c = clip_case
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = video.render_person_clips(c["tracks"], c["frames"], c["faces"], degs=(0, 90, 270))
    monkeypatch.setenv("PATH", str(tmp_path / "nothing-here"))
    with pytest.warns(UserWarning, match="track 2"):
        res = run_video.render_person_clips(str(tmp_path / "clips"), c["tracks"], c["frames"], faces=c["faces"], chunk=2, degs=(0, 90, 270))
    late = [c["tracks"][0], (c["tracks"][1][0], None, (3, 5), c["tracks"][1][3])]
    with pytest.raises(ValueError, match="track 1: range \\(3, 5\\) outside the 4 frames"):
        run_video.render_person_clips(str(tmp_path / "late"), late, c["frames"], faces=c["faces"])
    assert len(res) == 3 and res[2]["frames"] is None and res[2]["n_frames"] == 0 and "EMPTY" in res[2]["note"]
    assert sorted(os.listdir(tmp_path / "clips")) == ["track00", "track01"]
    for t in (0, 1):
        n = len(c["host"][t]["cams"])
        assert res[t]["n_frames"] == n and res[t]["video"] is None and "no ffmpeg" in res[t]["note"]
        assert res[t]["bbox"] == [int(x) for x in want[t]["bbox"]] and res[t]["size"] == want[t]["size"]
        folder = tmp_path / "clips" / ("track%02d" % t)
        assert sorted(os.listdir(folder)) == ["frame%06d.png" % i for i in range(n)]
        side = np.concatenate([want[t]["views"][d].cpu().numpy() for d in (0, 90, 270)], axis=2)
        for i in range(n):
            assert np.array_equal(np.asarray(Image.open(folder / ("frame%06d.png" % i))), side[i]), (t, i)


def test_video_bboxes_reads_packed_records_in_place(clip_case, gpu_device):
    """tracks that are views of ONE record buffer (what Tester.predict_tracks(records=True) returns) give what the dicts give"""
    import torch
    from human_dynamics_amd.dist import record_layout
    from human_dynamics_amd.util.render import video
    c = clip_case
    fields = (("cams", (3,)), ("joints", (25, 3)), ("kps", (25, 2)), ("poses", (24, 3, 3)), ("shapes", (10,)), ("verts", (170, 3)), ("omegas", (85,)))
    layout, rec_len = record_layout(2, fields)
    get = {k: (off, size) for k, _, off, size in layout}
    n = sum(len(h["cams"]) for h in c["host"])
    rec = torch.randn((n, rec_len), device=gpu_device)
    views, a = [], 0
    for (d, _, rng_, params), h in zip(c["tracks"], c["host"]):
        b = a + len(h["cams"])
        for key in ("cams", "kps", "verts"):
            o, size = get[key]
            rec[a:b, o:o + size] = d[key].flatten(1)
        views.append((rec[a:b], layout, rng_, params))
        a = b
    assert video._records_in_place(views) is not None
    b1, c1, s1 = video.video_bboxes(views, (96, 128), 10)
    b2, c2, s2 = video.video_bboxes(c["tracks"], (96, 128), 10)
    assert np.array_equal(b1, b2) and np.array_equal(s1, s2) and b1.shape == (3, 4) and s1.shape == (3,)
    for x, y in zip(c1, c2):
        assert x.device.type == "cuda" and np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    # separate buffers: the rows are laid end to end first, the answers are the same
    apart = [(v[0].clone(), v[1], v[2], v[3]) for v in views]
    assert video._records_in_place(apart) is None
    b3, c3, s3 = video.video_bboxes(apart, (96, 128), 10)
    assert np.array_equal(b1, b3) and np.array_equal(s1, s3)
    for x, y in zip(c1, c3):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ every status bit on the device
def _status_case():
    """seven tracks of 3 frames, k = 2, one call (720x1280, margin 0): good | S = 0 | S < 0 | an extreme above int32 | one below
    | scale = 0 behind finite inputs | good"""
    rng = np.random.default_rng(7)
    T, n_t, k = 7, 3, 2
    n = T * n_t
    cams = np.stack([rng.uniform(0.5, 1.2, n), rng.uniform(-.3, .3, n), rng.uniform(-.3, .3, n)], 1).astype(np.float32)
    kps = rng.uniform(-0.5, 0.5, (n, k, 2)).astype(np.float32)
    scale = rng.uniform(0.8, 1.2, n)
    centre = np.array([640., 360.]) + rng.normal(0, 5, (n, 2))
    proc = np.concatenate([scale[:, None], np.round(centre * scale[:, None]) + 112], 1)
    kps[3:6] = 0.25                                                      # a point person that does not move, inside the frame: S = 0
    proc[3:6] = proc[3]
    kps[6:9] = 0.                                                        # a point person above and left of the frame: xmax, ymax < 0 = xmin, ymin
    proc[6:9, 1:] = 0.
    proc[9:12, 1] = 1e13                                                 # xmin beyond int32 (xmax is clamped to w - 1)
    proc[12:15, 2] = -1e13                                               # ymax below int32 (ymin is clamped to 0)
    proc[16, 0] = 0.                                                     # 1 / 0 behind finite inputs
    return cams, kps, proc, (n_t * np.arange(T + 1)).astype(np.int32)


def _same_values(a, b):
    return np.array_equal(a, b, equal_nan=True)                          # (a NaN's sign and payload are nobody's contract)


def test_every_status_bit_on_the_device_equals_the_oracle(gpu_device):
    cams, kps, proc, offsets = _status_case()
    want = PV.video_bbox(cams, kps, proc, 224., offsets, 720, 1280, 0)
    assert list(want["status"]) == [0, PV.DEGENERATE, PV.DEGENERATE, PV.NOT_FINITE, PV.NOT_FINITE, PV.NOT_FINITE, 0], want["status"]
    S = np.maximum(want["bbox"][:, 1] - want["bbox"][:, 0], want["bbox"][:, 3] - want["bbox"][:, 2])
    assert S[1] == 0 and S[2] < 0
    bbox, crop, st = _call(gpu_device, cams, kps, proc, offsets, (720, 1280), 0)
    assert np.array_equal(bbox, want["bbox"]) and np.array_equal(st, want["status"]), (bbox, st)
    assert _same_values(crop, want["cams_crop"])
    assert np.isinf(crop[3:6]).any() and np.isnan(crop[9:18]).all() and np.isfinite(crop[:3]).all() and np.isfinite(crop[18:]).all()
    # a side that no int32 holds: with a margin of -2.1e9 the clamps leave xmin = 2.1e9 and xmax = -2.1e9, both int32, their difference not
    want = PV.video_bbox(cams[:3], kps[:3], proc[:3], 224., [0, 3], 720, 1280, -2.1e9)
    side = int(want["bbox"][0, 3]) - int(want["bbox"][0, 2])
    assert want["status"][0] & PV.DEGENERATE and side < -2 ** 31 and np.isfinite(want["cams_crop"]).all()
    bbox, crop, st = _call(gpu_device, cams[:3], kps[:3], proc[:3], [0, 3], (720, 1280), -2.1e9)
    assert np.array_equal(bbox, want["bbox"]) and np.array_equal(st, want["status"]) and np.array_equal(_bits(crop), _bits(want["cams_crop"]))
