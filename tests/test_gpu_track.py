"""The track front end on the device (csrc/track.hip, util/smooth_bbox.py, run_video.process_tracks) against the reference's own
results (tests/golden/reference_tracks.npz) and, for the seeded cases the fixture does not carry, the NumPy restatement that is
pinned to it (tests/track_oracle.py; the fixture's maker checked every seeded case against the reference as well).

Bound: |got - ref| <= 1e-12 max(1, |ref|).  A 25-term float64 sum with weights summing to 1 carries at most about
25 * 2^-53 ~ 3e-15 relative error, so the bound leaves roughly 300x margin; ranges, leading zeros, geometry and crops are exact.
No row is dropped: the maker asserts that no floor / round argument of any recorded or seeded row lies within 1e-6 of its
decision boundary."""
import ctypes as C
import os

import numpy as np
import pytest

import track_oracle as TO
from conftest import GOLDEN, Config

pytestmark = pytest.mark.gpu
VIS = TO.VIS_THRESH


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "reference_tracks.npz")))


@pytest.fixture(scope="module")
def cases():
    return TO.seeded_cases()


@pytest.fixture(scope="module")
def oracle(cases):
    """name -> [(raw, smooth [end, 3], start, end) per track], computed once"""
    out = {}
    for name, (h, w, tracks) in cases.items():
        rows = []
        for trk in tracks:
            raw, start, end = TO.get_all_bbox_params(trk, VIS)
            smooth = TO.get_smooth_bbox_params(trk, VIS)[0] if start >= 0 else np.zeros((0, 3))
            rows.append((raw, smooth, start, end))
        out[name] = rows
    return out


def _recorded(ref, name):
    n = len(ref[name + "/offsets"]) - 1
    return [(ref["%s/%d/raw" % (name, t)], ref["%s/%d/smooth" % (name, t)], int(ref["%s/%d/range" % (name, t)][0]),
             int(ref["%s/%d/range" % (name, t)][1])) for t in range(n)]


def _close(what, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size:
        err = float((np.abs(got - want) / np.maximum(1, np.abs(want))).max())
        print("%s: max |got - ref| / max(1, |ref|) = %.3e" % (what, err))
        assert err <= 1e-12, (what, err)


def _run(tracks, **kw):
    from human_dynamics_amd.util import smooth_bbox
    return smooth_bbox.smooth_tracks(tracks, vis_thresh=VIS, want_raw=True, **kw)


def _check(name, got, want):
    assert len(got) == len(want)
    for t, ((smooth, start, end, raw), (w_raw, w_smooth, w_start, w_end)) in enumerate(zip(got, want)):
        assert (start, end) == (w_start, w_end), (name, t, start, end, w_start, w_end)           # exact
        assert smooth.shape == (max(end, 0), 3) and not smooth[:max(start, 0)].any(), (name, t)  # leading rows exactly zero
        _close("%s[%d] raw" % (name, t), raw, w_raw)
        _close("%s[%d] smooth" % (name, t), smooth, w_smooth)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[1:3] == y[1:3] and np.array_equal(x[0], y[0]) and np.array_equal(x[3], y[3])


def test_track_lengths(gpu_device, cases, oracle):
    """1 .. 26 rows (shorter than, equal to and longer than the median and the Gaussian), 257, and T-1, T, T+1, 2T+1 for the
    scan's step T; fewer than six rows smooth to exact zeros"""
    tracks = cases["lengths"][2]
    assert [len(t) for t in tracks] == [1, 2, 5, 6, 10, 11, 12, 13, 24, 25, 26, 257, 255, 256, 257, 513]
    got = _run(tracks)
    _check("lengths", got, oracle["lengths"])
    for (smooth, start, end, raw), trk in zip(got, tracks):
        assert (start, end) == (0, len(trk)) and (len(trk) >= 6 or not smooth.any()) and (len(trk) < 6 or smooth.all())


@pytest.mark.parametrize("name", ["gaps", "tile_edges", "k1"])
def test_gaps_against_the_oracle(gpu_device, cases, oracle, name):
    """leading, trailing, interior gaps of 1, 2, 15 and 13 rows across a scan step, a gap of two whole steps, present but
    invisible frames, frames less than half a pixel tall (k = 25); k = 1 is never valid"""
    got = _run(cases[name][2])
    _check(name, got, oracle[name])
    if name == "gaps":
        assert got[0][1:3] == (3, 505)
    if name == "k1":
        assert got[0][1:3] == (-1, 0) and got[0][0].shape == (0, 3) and got[0][3].shape == (0, 3)


@pytest.mark.parametrize("name", ["k25", "mixed", "bad_rows", "short"])
def test_recorded_tracks_against_the_reference(gpu_device, ref, name):
    from human_dynamics_amd.evaluation.tracks import unpack_tracks
    tracks = unpack_tracks(ref[name + "/kps"], ref[name + "/present"], ref[name + "/offsets"])
    _check(name, _run(tracks), _recorded(ref, name))


def test_a_score_equal_to_the_threshold_is_not_visible(gpu_device):
    from human_dynamics_amd.util import smooth_bbox as sb
    kp = np.array([[10., 20., 0.1], [50., 80., 0.1], [30., 40., 0.05]])
    assert sb.kp_to_bbox_param(kp, 0.1) is None and sb.kp_to_bbox_param(None, 0.1) is None
    up = kp.copy()
    up[:2, 2] = np.nextafter(0.1, 1)
    _close("box", sb.kp_to_bbox_param(up, 0.1), TO.kp_to_bbox_param(up, 0.1))
    _close("box", sb.kp_to_bbox_param(up, 0.1), [30., 50., 150. / np.sqrt(40. * 40. + 60. * 60.)])
    one = up.copy()
    one[1, 2] = 0.1                                     # a single visible keypoint: zero height, no box
    assert sb.kp_to_bbox_param(one, 0.1) is None
    with pytest.raises(ValueError):
        sb.get_smooth_bbox_params([None, None, kp], vis_thresh=0.1)             # nothing valid: the reference raises too
    raw, start, end = sb.get_all_bbox_params([None, None, kp], vis_thresh=0.1)
    assert raw.shape == (0, 3) and (start, end) == (-1, 0)
    smooth, start, end = sb.get_smooth_bbox_params([None, up, None, up, None], vis_thresh=0.1, kernel_size=1, sigma=0.1)
    assert (start, end) == (1, 4) and smooth.shape == (4, 3) and not smooth[0].any() and np.array_equal(smooth[1], smooth[2])


def test_several_tracks_in_one_call_equal_each_alone(gpu_device, cases, oracle):
    """lengths {1, 13, 257, 6} with a track without a valid frame in the middle: no halo reads a neighbour"""
    tracks = cases["mixed"][2]
    assert [len(t) for t in tracks] == [1, 13, 9, 257, 6]
    together = _run(tracks)
    assert together[2][1:3] == (-1, 0) and together[2][0].shape == (0, 3)
    _same(together, [_run([trk])[0] for trk in tracks])
    _same(together[::-1], _run(tracks[::-1]))
    _check("mixed", together, oracle["mixed"])


def test_smooth_bbox_params_alone(gpu_device, ref):
    from human_dynamics_amd.util import smooth_bbox as sb
    for key in sorted(k[:-3] for k in ref if k.startswith("filters/") and k.endswith("/in")):
        n, ks, sigma = key.split("/")[1].split("_")
        _close(key, sb.smooth_bbox_params(ref[key + "/in"], int(ks), float(sigma)), ref[key + "/out"])
    assert not sb.smooth_bbox_params(ref["filters/5_11_3/in"], 11, 3).any()


def _device_geometry(boxes_per_track, h, w, device):
    """hmmr_track_crop_geom on given smoothed boxes ([end, 3] per track, rows [start, end) are cropped)"""
    import torch
    from human_dynamics_amd import _lib as L
    lib = L.load()
    offsets = np.zeros(len(boxes_per_track) + 1, np.int32)
    offsets[1:] = np.cumsum([len(b[0]) for b in boxes_per_track])
    n = int(offsets[-1])
    box = torch.from_numpy(np.concatenate([b[0] for b in boxes_per_track]).reshape(n, 3)).to(device)
    rng = torch.tensor([[b[1], b[2]] for b in boxes_per_track], dtype=torch.int32).to(device)
    geom = torch.full((n, 4), -7, dtype=torch.int32, device=device)
    info = torch.full((n, 5), -7., dtype=torch.float64, device=device)
    status = torch.full((n,), -7, dtype=torch.int32, device=device)
    L.check(lib.hmmr_track_crop_geom(box.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_int32)), rng.data_ptr(), len(boxes_per_track),
                                     h, w, geom.data_ptr(), info.data_ptr(), status.data_ptr(), None), "hmmr_track_crop_geom")
    torch.cuda.synchronize()
    return offsets, geom.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("name", ["k25", "mixed", "bad_rows", "short"])
def test_geometry_equals_crop_geometry_on_the_reference_boxes(gpu_device, ref, name):
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    h, w = (int(v) for v in ref[name + "/hw"])
    rec = [r for r in _recorded(ref, name) if r[2] >= 0]
    offsets, geom, info, status = _device_geometry([(r[1], r[2], r[3]) for r in rec], h, w, gpu_device)
    n_bad = 0
    for t, (_, smooth, start, end) in enumerate(rec):
        o = offsets[t]
        assert (geom[o:o + start] == [h, w, 0, 0]).all() and not status[o:o + start].any() and not info[o:o + start].any()
        for i in range(start, end):
            try:
                g = crop_geometry(h, w, smooth[i])
            except ValueError:
                n_bad += 1
                assert status[o + i] != 0 and geom[o + i].tolist() == [h, w, 0, 0] and not info[o + i].any(), (t, i)
                assert status[o + i] == TO.crop_geometry(h, w, smooth[i])[0]
                continue
            assert status[o + i] == 0, (t, i, status[o + i])
            assert geom[o + i].tolist() == [g["hs"], g["ws"], g["u0"], g["v0"]], (t, i)
            assert info[o + i].tolist() == [g["start_pt"][0], g["start_pt"][1], g["center"][0], g["center"][1], g["scale"]], (t, i)
    assert (n_bad > 0) == (name != "k25")               # short tracks smooth to zeros; bad_rows leaves the frame


def _frames(n, h, w, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("name,keep", [("k25", (0,)), ("bad_rows", (0, 2)), ("mixed", (1, 3, 4))])
def test_process_tracks_crops_equal_process_images_on_the_reference_boxes(gpu_device, ref, name, keep):
    import torch
    from human_dynamics_amd.evaluation.run_video import process_images, process_tracks
    from human_dynamics_amd.evaluation.tracks import unpack_tracks
    h, w = (int(v) for v in ref[name + "/hw"])
    tracks = unpack_tracks(ref[name + "/kps"], ref[name + "/present"], ref[name + "/offsets"])
    rec = _recorded(ref, name)
    frames = torch.from_numpy(_frames(max(len(t) for t in tracks), h, w)).to(gpu_device)
    got = process_tracks(frames, [tracks[t] for t in keep], vis_thresh=VIS)
    assert len(got) == len(keep)
    for (crops, (start, end), infos), t in zip(got, keep):
        _, smooth, w_start, w_end = rec[t]
        assert (start, end) == (w_start, w_end) and crops.is_cuda and tuple(crops.shape) == (end - start, 224, 224, 3)
        want, want_infos = process_images(frames[start:end], smooth[start:end], device=gpu_device)
        assert torch.equal(crops, want), (name, t)                                            # bit for bit
        assert len(infos) == len(want_infos) == end - start
        for a, b in zip(infos, want_infos):
            assert sorted(a) == sorted(b) == ["center", "im_shape", "scale", "start_pt"] and a["im_shape"] == b["im_shape"]
            assert np.array_equal(a["center"], b["center"]) and np.array_equal(a["start_pt"], b["start_pt"])
            assert abs(a["scale"] - b["scale"]) <= 1e-12 * max(1, abs(b["scale"]))
    # a host array is uploaded once and gives the same crops
    again = process_tracks(frames.cpu().numpy(), [tracks[keep[0]]], vis_thresh=VIS)
    assert torch.equal(again[0][0], got[0][0]) and again[0][1] == got[0][1]


def test_bad_rows_are_reported_not_faulted(gpu_device, ref):
    """one track's keypoints leave the frame: status != 0 on exactly the rows where crop_geometry raises, ValueError from
    process_tracks naming the track and the first bad frame; the neighbours in the same call and hmmr_run_flags are untouched"""
    import torch
    from human_dynamics_amd import _lib as L
    from human_dynamics_amd.evaluation.run_video import crop_geometry, process_tracks
    from human_dynamics_amd.evaluation.tracks import pack_tracks, unpack_tracks
    from human_dynamics_amd.util import smooth_bbox as sb
    lib = L.load()
    flags = C.c_uint(0)
    L.check(lib.hmmr_run_flags(C.byref(flags), 1), "hmmr_run_flags")
    name = "bad_rows"
    h, w = (int(v) for v in ref[name + "/hw"])
    tracks = unpack_tracks(ref[name + "/kps"], ref[name + "/present"], ref[name + "/offsets"])
    rec = _recorded(ref, name)
    kps, present, offsets = pack_tracks(tracks)
    smooth, rng, _ = sb.track_boxes(torch.from_numpy(kps).to(gpu_device), torch.from_numpy(present).to(gpu_device), offsets, VIS)
    n = len(kps)
    geom = torch.empty((n, 4), dtype=torch.int32, device=gpu_device)
    status = torch.empty(n, dtype=torch.int32, device=gpu_device)
    L.check(lib.hmmr_track_crop_geom(smooth.data_ptr(), offsets.ctypes.data_as(C.POINTER(C.c_int32)), rng.data_ptr(), 3, h, w, geom.data_ptr(),
                                     None, status.data_ptr(), None), "hmmr_track_crop_geom")
    torch.cuda.synchronize()
    status, geom = status.cpu().numpy(), geom.cpu().numpy()

    def raises(b):
        try:
            crop_geometry(h, w, b)
        except ValueError:
            return True
        return False
    want_bad = [np.array([raises(b) for b in r[1]]) for r in rec]
    assert not want_bad[0].any() and not want_bad[2].any() and 0 < want_bad[1].sum() < len(want_bad[1])
    for t in range(3):
        got_bad = status[offsets[t]:offsets[t + 1]] != 0
        assert np.array_equal(got_bad, want_bad[t]), t
        assert (geom[offsets[t]:offsets[t + 1]][got_bad] == [h, w, 0, 0]).all()
    frames = torch.from_numpy(_frames(40, h, w)).to(gpu_device)
    first = int(np.flatnonzero(want_bad[1])[0])
    with pytest.raises(ValueError, match=r"track 1: the smoothed box of frame %d " % first):
        process_tracks(frames, tracks, vis_thresh=VIS)
    with pytest.raises(ValueError, match="track 1: no frame has a bounding box"):
        process_tracks(frames, [tracks[0], [None] * 5], vis_thresh=VIS)
    alone = process_tracks(frames, [tracks[0], tracks[2]], vis_thresh=VIS)
    _same(_run(tracks)[::2], _run([tracks[0], tracks[2]]))
    assert alone[0][1] == tuple(rec[0][2:]) and alone[1][1] == tuple(rec[2][2:])
    L.check(lib.hmmr_run_flags(C.byref(flags), 0), "hmmr_run_flags")
    assert flags.value == 0


def test_two_runs_give_the_same_bits_also_beside_the_resnet(gpu_device, weights, smpl_consts, cases):
    """the pattern of test_gpu_eval.py: the track kernels on a side stream while ResNet kernels occupy another.  One repetition."""
    import torch
    from human_dynamics_amd import assets
    from human_dynamics_amd.evaluation.run_video import process_tracks
    from human_dynamics_amd.evaluation.tester import Tester
    h, w, tracks = cases["mixed"]
    tracks = [tracks[1], tracks[3], tracks[4]]
    frames = torch.from_numpy(_frames(257, h, w)).to(gpu_device)
    run = lambda: (_run(tracks), process_tracks(frames, tracks, vis_thresh=VIS))
    quiet, again = run(), run()
    torch.cuda.synchronize()
    tester = Tester(Config(batch_size=1), weights=weights, smpl=smpl_consts, dtype="f32", device=gpu_device)
    crops = torch.as_tensor(assets.make_synthetic_frames(120, seed=5), device=gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    tester.engine.resnet(crops, ws_key="busy")
    with torch.cuda.stream(side):
        busy = run()
    torch.cuda.synchronize()
    for other in (again, busy):
        _same(quiet[0], other[0])
        for a, b in zip(quiet[1], other[1]):
            assert torch.equal(a[0], b[0]) and a[1] == b[1]
            assert all(x["scale"] == y["scale"] and np.array_equal(x["start_pt"], y["start_pt"]) for x, y in zip(a[2], b[2]))
