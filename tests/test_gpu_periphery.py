"""The kernels AROUND the path -- crop (csrc/preprocess.hip), evaluation metrics (csrc/eval_metrics.hip), rasteriser
hand-off (csrc/handoff.hip) and the FK mirror (csrc/smpl.hip) -- against their float64 oracles, at the sizes, strides and
degenerate inputs where such kernels go wrong: second blocks and strided trips, slab boundaries, NULL outputs, row
strides with NaN in the gaps, pad edges, and Procrustes problems of rank two and one.

Every case prints its measured maximum error ("periphery: ..." lines; one full run is kept in profiles/).  The guard
rows are written by the test and read back on the host; nothing here reads or writes outside its own allocations.

Tolerances: the project's 1e-6 (metre scale) for the metrics and the crop, rtol = atol = 2e-6 for the hand-off cameras,
2e-6 for FK -- those of the existing tests.  One refinement, from the output format alone: a metric is returned as
float32, so where its VALUE exceeds 8 m (MPJPE of a prediction scaled by 1000) one float32 ulp of the value is the bound.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, Config
from oracle import handoff_oracle as HO
from oracle import metrics_oracle as MO
from oracle import preprocess_oracle as PO

pytestmark = pytest.mark.gpu
S = 224
NAN = float("nan")


def _lib():
    from human_dynamics_amd import _lib as L
    return L, L.load()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _say(what, err):
    print("periphery: %-78s max err %.2e" % (what, err))


# ===================================================================================================== crop
SIZES = [(96, 128), (101, 203), (224, 224), (360, 640), (720, 1280), (1080, 1920)]
SCALES = {"down": (0.2, 0.6), "about1": (0.97, 1.03), "one": (1.0, 1.0), "up": (1.5, 4.0)}


def _centres(h, w):
    """the frame centre, the four corners, 15 px outside each corner -> (cx, cy, pads_x, pads_y); pads: -1 low side, +1 high"""
    out = [(w / 2.0, h / 2.0, 0, 0)]
    for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
        for d in (0.0, 15.0):
            out.append(((w + d) if sx > 0 else -d, (h + d) if sy > 0 else -d, sx, sy))
    return out


def _frames(rng, n, h, w):
    """n different frames for the cost of one draw: a noisy gradient, rolled and inverted per frame"""
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    base[: h // 2, : w // 2] //= 2
    return np.stack([np.roll(base, (7 * i, 13 * i, i), (0, 1, 2)) ^ np.uint8(37 * i % 256) for i in range(n)])


def _oracle_crop(frame, bbox):
    big = frame.shape[0] * frame.shape[1] * max(float(bbox[2]), 1.0) ** 2 > 2.5e6
    return (PO.process_image_window if big else PO.process_image)(frame, bbox)          # bit-identical (test_preprocess.py)


def _check_crops(frames, bboxes, dev, per_call):
    from human_dynamics_amd.evaluation.run_video import process_images
    worst = 0.0
    for i0 in range(0, len(frames), per_call):
        out, infos = process_images(frames[i0:i0 + per_call], bboxes[i0:i0 + per_call], device=dev)
        got = out.cpu().numpy()
        for j, info in enumerate(infos):
            ref = _oracle_crop(frames[i0 + j], bboxes[i0 + j])
            assert list(info["center"]) == list(ref["center"]) and list(info["start_pt"]) == list(ref["start_pt"])
            assert np.isfinite(got[j]).all()
            worst = max(worst, float(np.abs(got[j] - ref["image"]).max()))
    return worst


@pytest.mark.parametrize("family", list(SCALES))
@pytest.mark.parametrize("h,w", SIZES)
def test_crop_sizes_scales_and_pad_edges(gpu_device, h, w, family):
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    rng = np.random.default_rng([h, w, list(SCALES).index(family)])
    cs = _centres(h, w)
    lo, hi = SCALES[family]
    bboxes = np.array([[cx, cy, rng.uniform(lo, hi)] for cx, cy, _, _ in cs])
    for (cx, cy, px, py), bb in zip(cs, bboxes):          # precondition: a corner case really has padding on two sides
        g = crop_geometry(h, w, bb)
        if px:
            assert (g["u0"] < 0) if px < 0 else (g["u0"] + S - 1 > g["ws"] - 1), (bb, g)
            assert (g["v0"] < 0) if py < 0 else (g["v0"] + S - 1 > g["hs"] - 1), (bb, g)
    frames = _frames(rng, len(cs), h, w)
    err = _check_crops(frames, bboxes, gpu_device, 2 if h >= 720 else len(cs))
    _say("crop %4dx%-4d scale %-6s (%.2f..%.2f), centre + 4 corners + 4 outside" % (h, w, family, bboxes[:, 2].min(), bboxes[:, 2].max()), err)
    assert err < 1e-6


@pytest.mark.parametrize("h,w,scale,hs", [(96, 128, 0.015, 1), (96, 128, 0.025, 2), (101, 203, 0.012, 1), (101, 203, 0.0285, 2),
                                          (1080, 1920, 0.00095, 1)])
def test_crop_of_a_scaled_image_one_or_two_pixels_high(gpu_device, h, w, scale, hs):
    """floor(h * scale) is 1 or 2: every tap of `taps` is in the `s >= src - 1` clamp or next to it, the whole crop is padding."""
    assert int(np.floor(h * scale)) == hs
    rng = np.random.default_rng([h, hs])
    cs = _centres(h, w)[:3] + _centres(h, w)[-1:]
    frames = _frames(rng, len(cs), h, w)
    bboxes = np.array([[cx, cy, scale] for cx, cy, _, _ in cs])
    err = _check_crops(frames, bboxes, gpu_device, 2)
    _say("crop %4dx%-4d scaled to %d row(s)" % (h, w, hs), err)
    assert err < 1e-6


def test_crop_257_frames_each_with_its_own_content_and_bbox(gpu_device):
    from human_dynamics_amd.evaluation.run_video import process_images
    rng = np.random.default_rng(257)
    n, h, w = 257, 96, 128
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    bboxes = np.stack([rng.uniform(-15, w + 15, n), rng.uniform(-15, h + 15, n), rng.uniform(0.3, 3.2, n)], 1)
    out, infos = process_images(frames, bboxes, device=gpu_device)
    got = out.cpu().numpy()
    worst = 0.0
    for i in range(n):
        ref = PO.process_image(frames[i], bboxes[i])
        assert list(infos[i]["start_pt"]) == list(ref["start_pt"])
        worst = max(worst, float(np.abs(got[i] - ref["image"]).max()))
        alone, _ = process_images(frames[i:i + 1], bboxes[i:i + 1], device=gpu_device)
        assert np.array_equal(alone[0].cpu().numpy(), got[i]), i                  # frame i alone: the same bits
    _say("crop 257 frames of 96x128, own content and bbox each; alone == in batch", worst)
    assert worst < 1e-6


def _raw_crop(frames_u8, geom, dev):
    """hmmr_crop_frames itself, `out` followed by one guard row of NaN"""
    L, lib = _lib()
    n, h, w = frames_u8.shape[:3]
    fr = torch.from_numpy(np.ascontiguousarray(frames_u8)).to(dev)
    g = torch.tensor(geom, dtype=torch.int32).reshape(n, 4).to(dev)
    buf = torch.full((n * S * S * 3 + S * 3,), NAN, dtype=torch.float32, device=dev)
    L.check(lib.hmmr_crop_frames(fr.data_ptr(), g.data_ptr(), n, h, w, buf.data_ptr(), _stream(dev)), "hmmr_crop_frames")
    host = buf.cpu().numpy()
    assert np.isnan(host[n * S * S * 3:]).all(), "the guard row after `out` was written"
    return host[:n * S * S * 3].reshape(n, S, S, 3)


def test_crop_identity_geometry_is_the_bitwise_uint8_conversion(gpu_device):
    """{224, 224, 0, 0} on a 224x224 frame: out == float32(((b / 255.) - 0.5) * 2) bit for bit (evaluation/streaming.py
    converts its uint8 input this way), for all 256 byte values, 5 frames."""
    rng = np.random.default_rng(224)
    frames = (np.arange(5 * S * S * 3) % 256).astype(np.uint8)
    rng.shuffle(frames)
    frames = frames.reshape(5, S, S, 3)
    assert len(np.unique(frames)) == 256
    got = _raw_crop(frames, [[S, S, 0, 0]] * 5, gpu_device)
    want = np.float32(((frames / 255.) - 0.5) * 2)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    _say("crop identity geometry, all 256 byte values, bit-equal, guard row intact", float(np.abs(got - want).max()))


def test_crop_raw_entry_with_guard_row(gpu_device):
    from human_dynamics_amd.evaluation.run_video import crop_geometry
    rng = np.random.default_rng(31)
    h, w = 101, 203
    frames = rng.integers(0, 256, (7, h, w, 3), dtype=np.uint8)
    bboxes = [[w + 15.0, h + 15.0, 0.45], [-15.0, -15.0, 0.3], [w / 2, h / 2, 1.0], [w, 0.0, 2.5], [0.0, h, 0.02],
              [50.0, 50.0, 0.97], [w - 1.0, h - 1.0, 3.7]]
    gs = [crop_geometry(h, w, b) for b in bboxes]
    got = _raw_crop(frames, [[g["hs"], g["ws"], g["u0"], g["v0"]] for g in gs], gpu_device)
    err = max(float(np.abs(got[i] - PO.process_image(frames[i], bboxes[i])["image"]).max()) for i in range(7))
    _say("crop raw C entry, 7 frames of 101x203, guard row intact", err)
    assert err < 1e-6


# ===================================================================================================== metrics
def _tol(ref):
    """1e-6, or one float32 ulp of the value where that is larger (values above 8 m): the result is a float32"""
    return np.maximum(1e-6, np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))


def _raw_joints(gt, pred, left, right, dev, want=("mp", "pa", "ac", "ae")):
    L, lib = _lib()
    n, k = pred.shape[:2]
    g = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).to(dev) if gt is not None else None
    p = torch.from_numpy(np.ascontiguousarray(pred, np.float32)).to(dev)
    out = {"mp": torch.full((n + 1,), NAN, device=dev), "pa": torch.full((n + 1,), NAN, device=dev),
           "ac": torch.full((max(n - 2, 0) + 1,), NAN, device=dev), "ae": torch.full((max(n - 2, 0) + 1,), NAN, device=dev)}
    L.check(lib.hmmr_eval_joints(L.ptr(g), p.data_ptr(), n, k, left, right, *[out[o].data_ptr() if o in want else None
                                                                             for o in ("mp", "pa", "ac", "ae")], _stream(dev)),
            "hmmr_eval_joints")
    res = {}
    for o, t in out.items():
        host = t.cpu().numpy()
        assert np.isnan(host[-1]), "guard element after %s was written" % o
        if o in want:
            res[o] = host[:-1]
        else:
            assert np.isnan(host).all(), "%s was not requested but was written" % o
    return res


def _vis(n):
    v = np.ones(n, bool)
    if n >= 12:
        v[[0, n - 1, n // 2, n // 2 + 1]] = False        # both ends, two adjacent frames in the middle
    return v


@pytest.mark.parametrize("k", [2, 14, 25, 32])
@pytest.mark.parametrize("n", [1, 2, 3, 12, 63, 64, 65, 4096])
def test_joint_metrics_over_frame_and_joint_counts(gpu_device, n, k):
    from human_dynamics_amd.evaluation import eval_util as E
    rng = np.random.default_rng([n, k])
    gt = (rng.normal(size=(n, k, 3)) * 0.3).astype(np.float32)
    pred = (gt + rng.normal(size=(n, k, 3)) * 0.05).astype(np.float32)
    left, right = (3, 2) if k > 3 else (1, 0)
    vis = _vis(n)
    ref_e, ref_pa = MO.compute_error_3d(gt, pred, None, left, right)
    ref_ac, ref_ae_all, ref_ae = MO.compute_accel(pred), MO.accel_error_all(gt, pred), MO.compute_error_accel(gt, pred, vis)
    raw = _raw_joints(gt, pred, left, right, gpu_device)
    errs = {"mpjpe": np.abs(raw["mp"] - ref_e).max(), "pa_mpjpe": np.abs(raw["pa"] - ref_pa).max()}
    assert raw["ac"].shape == ref_ac.shape == (max(n - 2, 0),)
    if n > 2:
        errs["accel"], errs["accel_err_all"] = np.abs(raw["ac"] - ref_ac).max(), np.abs(raw["ae"] - ref_ae_all).max()
    if k > 3:                                               # the mirror of eval_util.py (LSP hips 3 and 2)
        e, epa = E.compute_error_3d(gt, pred, vis, device=gpu_device)
        assert len(e) == len(epa) == int(vis.sum())
        errs["E.mpjpe"], errs["E.pa_mpjpe"] = np.abs(np.array(e) - ref_e[vis]).max(), np.abs(np.array(epa) - ref_pa[vis]).max()
        ac, ae = E.compute_accel(pred, device=gpu_device), E.compute_error_accel(gt, pred, vis, device=gpu_device)
        assert ac.shape == ref_ac.shape and ae.shape == ref_ae.shape
        if n <= 2:
            assert ac.size == 0 and ae.size == 0            # empty, and no failure
        else:
            errs["E.accel"] = np.abs(ac - ref_ac).max()
            if ae.size:
                errs["E.accel_err"] = np.abs(ae - ref_ae).max()
    _say("joints n=%-4d k=%-2d %s" % (n, k, " ".join("%s %.1e" % kv for kv in sorted(errs.items()))), max(errs.values()))
    assert max(errs.values()) < 1e-6, errs
    # accel alone (gt NULL, no error outputs) writes nothing else
    only = _raw_joints(None, pred, left, right, gpu_device, want=("ac",))
    assert np.array_equal(only["ac"], raw["ac"])


@pytest.fixture(scope="module")
def edges():
    return dict(np.load(os.path.join(GOLDEN, "reference_metrics_edges.npz")))


@pytest.mark.parametrize("name", MO.FAMILIES)
def test_procrustes_degenerate_family(gpu_device, edges, name):
    """The recorded fixture (the reference's own numbers) and 256 seeded frames against the oracle, at 1e-6, after the
    near-tie filter (at most 5 % of a family dropped)."""
    from human_dynamics_amd.evaluation import eval_util as E
    offset = 1000.0 if name == "offset_1000" else 0.0
    worst = {}
    for label, (gt, pred), seed, ref in (("recorded", (edges[name + "/gt"], edges[name + "/pred"]), 20,
                                          (edges[name + "/mpjpe"], edges[name + "/pa_mpjpe"])),
                                         ("seeded", MO.family(name, 256, 14, 1), 1, None)):
        if ref is None:
            ref = MO.compute_error_3d(gt, pred)
        keep = MO.well_conditioned(gt, pred, seed, offset=offset)
        assert (~keep).sum() <= 0.05 * len(gt), "%d of %d frames dropped" % ((~keep).sum(), len(gt))
        e, epa = (np.array(x, np.float64) for x in E.compute_error_3d(gt, pred, device=gpu_device))
        assert np.isfinite(e).all() and np.isfinite(epa).all(), (name, label)
        d_e, d_pa = np.abs(e - ref[0]), np.abs(epa - ref[1])
        worst[label] = (float(d_e.max()), float(d_pa[keep].max()), int((~keep).sum()))
        _say("procrustes %-17s %-8s %3d frames, %d dropped, mpjpe %.1e pa(all) %.1e" % (name, label, len(gt), (~keep).sum(),
                                                                                       d_e.max(), d_pa.max()), d_pa[keep].max())
        assert (d_e <= _tol(ref[0])).all(), (name, label, float(d_e.max()))
        assert (d_pa[keep] < 1e-6).all(), (name, label, float(d_pa[keep].max()))
        if name == "identical":
            assert epa.max() < 1e-6 and e.max() < 1e-6
        # the acceleration metrics on the same inputs (recorded: the reference's arrays)
        if label == "recorded":
            vis = edges["vis"].astype(bool)
            ac = E.compute_accel(pred, device=gpu_device)
            ae = E.compute_error_accel(gt, pred, vis, device=gpu_device)
            r_ac, r_ae = edges[name + "/accel"], edges[name + "/accel_err"]
            assert ae.shape == r_ae.shape
            assert (np.abs(ac - r_ac) <= _tol(r_ac)).all() and (np.abs(ae - r_ae) <= _tol(r_ae)).all()


@pytest.mark.parametrize("name", MO.NONFINITE_FAMILIES)
def test_procrustes_is_not_finite_where_the_reference_is_not(gpu_device, edges, name):
    from human_dynamics_amd.evaluation import eval_util as E
    assert not edges[name + "/pa_is_finite"].any()
    e, epa = E.compute_error_3d(edges[name + "/gt"], edges[name + "/pred"], device=gpu_device)
    assert not np.isfinite(np.array(epa)).any()
    assert np.abs(np.array(e) - edges[name + "/mpjpe"]).max() < 1e-6


def _raw_verts(gt, pred, ld_gt, ld_pred, dev):
    """rows of gt / pred placed at strides ld_gt / ld_pred, NaN in the gaps; err followed by a guard element"""
    L, lib = _lib()
    n, nv = gt.shape[:2]
    bufs = []
    for x, ld in ((gt, ld_gt), (pred, ld_pred)):
        b = np.full((n, ld), np.nan, np.float32)
        b[:, :3 * nv] = x.reshape(n, -1)
        bufs.append(torch.from_numpy(b).to(dev))
    err = torch.full((n + 1,), NAN, device=dev)
    L.check(lib.hmmr_eval_verts(bufs[0].data_ptr(), ld_gt, bufs[1].data_ptr(), ld_pred, n, nv, err.data_ptr(), _stream(dev)),
            "hmmr_eval_verts")
    host = err.cpu().numpy()
    assert np.isnan(host[-1])
    return host[:-1]


@pytest.mark.parametrize("n", [1, 12, 257])
@pytest.mark.parametrize("nv", [1, 50, 255, 256, 257, 6890])
def test_vertex_error_over_sizes_and_row_strides(gpu_device, nv, n):
    from human_dynamics_amd.evaluation import eval_util as E
    rng = np.random.default_rng([nv, n])
    gt = rng.normal(size=(n, nv, 3)).astype(np.float32)
    pred = (gt + rng.normal(size=(n, nv, 3)) * 0.1).astype(np.float32)
    pred[:, -1] += np.float32(3.0)                          # the last vertex counts: a trip cut short is seen
    ref = MO.compute_error_verts(gt, pred)
    a = np.abs(E.compute_error_verts(gt, pred, device=gpu_device) - ref).max()
    b = np.abs(_raw_verts(gt, pred, 3 * nv + 5, 3 * nv + 11, gpu_device) - ref).max()
    c = np.abs(_raw_verts(gt, pred, 3 * nv, 3 * nv + 1, gpu_device) - ref).max()
    _say("verts nv=%-4d n=%-3d dense %.1e, ld +5/+11 with NaN gaps %.1e, ld +0/+1 %.1e" % (nv, n, a, b, c), max(a, b, c))
    assert max(a, b, c) < 1e-6


def test_vertex_error_reads_pred_inside_the_packed_records(weights, smpl_consts, gpu_device):
    """pred = the `verts` field of the records of Tester.predict_records, in place (ld = rec_len)."""
    from human_dynamics_amd import assets, dist as hd
    from human_dynamics_amd.evaluation.tester import Tester
    L, lib = _lib()
    t = Tester(Config(batch_size=2), weights=weights, smpl=smpl_consts, dtype="f32", device=gpu_device)
    frames = torch.from_numpy(assets.make_synthetic_frames(24, seed=4)).to(gpu_device)
    sp = hd.ShardedPredictor(t, 24, 0, 1)
    rec = sp.run(frames)                                    # [24, rec_len], written by predict_records
    off = {k: (o, sz, shp) for k, shp, o, sz in sp.layout}
    o, sz, shp = off["verts"]
    nv = int(shp[0])
    assert rec.is_contiguous() and rec.stride(0) > 3 * nv and sz == 3 * nv
    verts = hd.unpack_outputs(rec, sp.layout)["verts"].cpu().numpy()
    rng = np.random.default_rng(9)
    gt = (verts + rng.normal(size=verts.shape) * 0.02).astype(np.float32)
    g = torch.from_numpy(gt).to(gpu_device)
    err = torch.full((25,), NAN, device=gpu_device)
    L.check(lib.hmmr_eval_verts(g.data_ptr(), 3 * nv, rec.data_ptr() + 4 * o, rec.stride(0), 24, nv, err.data_ptr(),
                                _stream(gpu_device)), "hmmr_eval_verts")
    host = err.cpu().numpy()
    d = np.abs(host[:24] - MO.compute_error_verts(gt, verts)).max()
    _say("verts from the packed records in place, nv=%d ld=%d" % (nv, rec.stride(0)), d)
    assert np.isnan(host[24]) and d < 1e-6


# ===================================================================================================== hand-off
def _raw_handoff(cams, verts, kps, geom, dev, ld_cam=None, ld_verts=None, ld_kps=None, want_cam=True, want_kp=True):
    """hmmr_render_handoff itself: inputs at the given row strides with NaN in the gaps, outputs pre-filled with NaN and
    followed by a guard row each.  Returns the outputs that were asked for."""
    L, lib = _lib()
    n, nv = verts.shape[:2]
    nk = kps.shape[1] if kps is not None else 0

    def rows(x, ld):
        x = np.asarray(x, np.float32).reshape(n, -1)
        b = np.full((n, ld or x.shape[1]), np.nan, np.float32)
        b[:, :x.shape[1]] = x
        return torch.from_numpy(b).to(dev)
    c, v = rows(cams, ld_cam), rows(verts, ld_verts)
    k = rows(kps, ld_kps) if kps is not None else None
    g = torch.from_numpy(np.asarray(geom, np.float32).reshape(n, 5)).to(dev) if geom is not None else None
    cam_o = torch.full((n + 1, 3), NAN, device=dev)
    proj_o = torch.full((n + 1, nv, 3), NAN, device=dev)
    kp_o = torch.full((n + 1, max(nk, 1), 2), NAN, device=dev)
    ask_kp = want_kp and k is not None
    L.check(lib.hmmr_render_handoff(c.data_ptr(), c.stride(0), v.data_ptr(), v.stride(0), L.ptr(k), k.stride(0) if k is not None else 0,
                                    L.ptr(g), n, nv, nk, cam_o.data_ptr() if want_cam else None, proj_o.data_ptr(),
                                    kp_o.data_ptr() if ask_kp else None, _stream(dev)), "hmmr_render_handoff")
    out = {}
    for name, t, asked in (("cams", cam_o, want_cam), ("proj_verts", proj_o, True), ("kps", kp_o, ask_kp)):
        host = t.cpu().numpy()
        assert np.isnan(host[n]).all(), "the guard row after %s was written" % name
        if asked:
            assert not np.isnan(host[:n]).any(), "%s was not written completely" % name
            out[name] = host[:n]
        else:
            assert np.isnan(host).all(), "%s was not requested but was written" % name
    return out


def _geom_rows(rng, n, extreme=False):
    """{undo_scale, start_x, start_y, proc_size, img_size}, float32-exact so the device and the oracle read the same numbers"""
    if extreme:
        undo = np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))
        size = np.exp(rng.uniform(np.log(64), np.log(4096), n)).round()
        start = rng.integers(0, 4001, (n, 2))
    else:
        undo, size, start = rng.uniform(0.4, 2.0, n), rng.integers(200, 720, n), rng.integers(100, 400, (n, 2))
    return np.stack([undo, start[:, 0], start[:, 1], np.full(n, 224.0), size], 1).astype(np.float32).astype(np.float64)


def _oracle_handoff(cams, kps, geom):
    """new_cam / kp_orig [n,...] float64 from handoff_oracle.orig_camera, one frame at a time (geom None: unchanged)"""
    cams = np.asarray(cams, np.float32)[:, :3]
    if geom is None:
        return cams.astype(np.float64), None if kps is None else np.asarray(kps, np.float64)
    nc, nkp = [], []
    for i in range(len(cams)):
        kp = kps[i] if kps is not None else np.zeros((1, 2))
        cam, kpo, _ = HO.orig_camera(cams[i], kp, geom[i, 1:3], 1.0 / geom[i, 0], geom[i, 3], (int(geom[i, 4]), int(geom[i, 4])), 10 ** 7)
        nc.append(cam)
        nkp.append(kpo)
    return np.array(nc), (np.array(nkp) if kps is not None else None)


def _compare_handoff(out, cams, verts, kps, geom, what, cam_from_full_call=None):
    rc, rk = _oracle_handoff(cams, kps, geom)
    errs = {}
    cam_dev = out.get("cams")
    if cam_dev is not None:
        if geom is None:
            assert np.array_equal(cam_dev, np.asarray(cams, np.float32)[:, :3])
        assert np.allclose(cam_dev, rc, rtol=2e-6, atol=2e-6), what
        errs["cam(rel)"] = float((np.abs(cam_dev - rc) / (np.abs(rc) + 1.0)).max())
    else:
        cam_dev = cam_from_full_call                        # new_cam == NULL: the camera of a call that returned it
    if "kps" in out:
        if geom is None:
            assert np.array_equal(out["kps"], np.asarray(kps, np.float32))
        assert np.allclose(out["kps"], rk, rtol=2e-6, atol=2e-6), what
        errs["kp(rel)"] = float((np.abs(out["kps"] - rk) / (np.abs(rk) + 1.0)).max())
    want = HO.project(np.asarray(verts, np.float32), cam_dev)
    assert np.array_equal(out["proj_verts"], want), what     # fp32 mul(add) without contraction: bit-equal
    _say("handoff %s: proj_verts bit-equal; %s" % (what, " ".join("%s %.1e" % kv for kv in sorted(errs.items()))),
         max(errs.values()) if errs else 0.0)


def _handoff_inputs(rng, n, nv, nk, extreme=False):
    s = np.exp(rng.uniform(np.log(0.05), np.log(5.0), n)) if extreme else rng.uniform(0.5, 1.5, n)
    cams = np.concatenate([s[:, None], rng.normal(size=(n, 2)) * 0.2], 1).astype(np.float32)
    verts = rng.normal(size=(n, nv, 3)).astype(np.float32)
    kps = rng.uniform(-1, 1, (n, nk, 2)).astype(np.float32) if nk else None
    return cams, verts, kps


def test_handoff_across_the_slab_boundary(gpu_device):
    """n = 32768 + 5: the launch loop's second slab (f0 = 32768) holds frames 32768..32772"""
    rng = np.random.default_rng(32768)
    n = 32768 + 5
    cams, verts, kps = _handoff_inputs(rng, n, 3, 1)
    geom = _geom_rows(rng, n)
    out = _raw_handoff(cams, verts, kps, geom, gpu_device)
    rc, rk = _oracle_handoff(cams, kps, geom)
    for f in (0, 32767, 32768, n - 1):
        assert np.allclose(out["cams"][f], rc[f], rtol=2e-6, atol=2e-6), f
        assert np.allclose(out["kps"][f], rk[f], rtol=2e-6, atol=2e-6), f
        assert np.array_equal(out["proj_verts"][f], HO.project(verts[f:f + 1], out["cams"][f:f + 1])[0]), f
    _compare_handoff(out, cams, verts, kps, geom, "n=32773 nv=3 nk=1, every frame its own camera and geometry")
    via = __import__("human_dynamics_amd.util.render.handoff", fromlist=["x"]).rasteriser_inputs(
        torch.from_numpy(cams).to(gpu_device), torch.from_numpy(verts).to(gpu_device), torch.from_numpy(kps).to(gpu_device), geom)
    assert np.array_equal(via["proj_verts"].cpu().numpy(), out["proj_verts"]) and np.array_equal(via["cams"].cpu().numpy(), out["cams"])


@pytest.mark.parametrize("with_geom", [True, False])
def test_handoff_production_mesh_from_strided_rows(gpu_device, with_geom):
    rng = np.random.default_rng(6890)
    n, nv, nk = 3, 6890, 25
    cams, verts, kps = _handoff_inputs(rng, n, nv, nk)
    geom = _geom_rows(rng, n) if with_geom else None
    out = _raw_handoff(cams, verts, kps, geom, gpu_device, ld_cam=85, ld_verts=3 * nv + 7, ld_kps=2 * nk + 3)
    _compare_handoff(out, cams, verts, kps, geom, "nv=6890 nk=25 ld 85 / 3nv+7 / 2nk+3, NaN gaps, geom=%s" % with_geom)


@pytest.mark.parametrize("with_geom", [True, False])
@pytest.mark.parametrize("case", ["no_new_cam", "no_kps", "no_kp_orig", "nv1_nk25", "nv1_nk25_no_new_cam"])
def test_handoff_null_outputs_and_keypoint_sized_grid(gpu_device, case, with_geom):
    rng = np.random.default_rng([len(case), with_geom])
    n = 70
    nv, nk = (1, 25) if case.startswith("nv1") else (300, 0 if case == "no_kps" else 25)
    cams, verts, kps = _handoff_inputs(rng, n, nv, nk)
    geom = _geom_rows(rng, n) if with_geom else None
    out = _raw_handoff(cams, verts, kps, geom, gpu_device, want_cam="no_new_cam" not in case, want_kp=case != "no_kp_orig")
    assert ("cams" in out) == ("no_new_cam" not in case) and ("kps" in out) == (case not in ("no_kps", "no_kp_orig"))
    full = _raw_handoff(cams, verts, kps, geom, gpu_device) if "cams" not in out else out
    assert np.array_equal(full["proj_verts"], out["proj_verts"])
    _compare_handoff(out, cams, verts, kps, geom, "%s nv=%d nk=%d geom=%s" % (case, nv, nk, with_geom), full["cams"])


@pytest.mark.parametrize("with_geom", [True, False])
def test_handoff_geometry_extremes(gpu_device, with_geom):
    """undo_scale 0.1..10, img_size 64..4096, start points 0..4000, camera scale 0.05..5"""
    rng = np.random.default_rng(4000)
    n = 1024
    cams, verts, kps = _handoff_inputs(rng, n, 5, 3, extreme=True)
    geom = _geom_rows(rng, n, extreme=True) if with_geom else None
    out = _raw_handoff(cams, verts, kps, geom, gpu_device)
    _compare_handoff(out, cams, verts, kps, geom, "extremes n=1024 geom=%s" % with_geom)


# ===================================================================================================== FK mirror
def _rotations(rng, m):
    """[m,24,3,3] float64 Rodrigues rotations; a third of the angles within 1e-3 of 0, a third within 1e-3 of pi"""
    axis = rng.normal(size=(m, 24, 3))
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    kind = rng.integers(0, 3, (m, 24))
    ang = np.where(kind == 0, rng.uniform(-1e-3, 1e-3, (m, 24)),
                   np.where(kind == 1, np.pi + rng.uniform(-1e-3, 1e-3, (m, 24)), rng.uniform(-np.pi, np.pi, (m, 24))))
    Kx = np.zeros((m, 24, 3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
    s, c = np.sin(ang)[..., None, None], np.cos(ang)[..., None, None]
    return np.eye(3) + s * Kx + (1 - c) * (Kx @ Kx)


@pytest.mark.parametrize("rotate_base", [False, True])
@pytest.mark.parametrize("m", [1, 7, 64, 65, 1000])
def test_fk_mirror_over_batch_sizes(smpl_consts, gpu_device, m, rotate_base):
    from human_dynamics_amd.tf_smpl.batch_lbs import batch_global_rigid_transformation as fk
    from oracle import hmmr_oracle as O
    rng = np.random.default_rng([m, rotate_base])
    Rs = _rotations(rng, m).astype(np.float32)
    Js = (rng.normal(size=(m, 24, 3)) * 0.3).astype(np.float32)
    parents = [int(p) for p in smpl_consts["parents"]]
    ref_j, ref_A = O.batch_global_rigid_transformation(torch.tensor(Rs, dtype=torch.float64), torch.tensor(Js, dtype=torch.float64),
                                                       parents, rotate_base=rotate_base)
    new_j, A = fk(Rs, Js, smpl_consts["parents"], rotate_base=rotate_base)
    new_j, A = new_j.cpu().numpy(), A.cpu().numpy()
    assert new_j.shape == (m, 24, 3) and A.shape == (m, 24, 4, 4)
    ej, eA = np.abs(new_j - ref_j.numpy()).max(), np.abs(A - ref_A.numpy()).max()
    for i in sorted({0, m // 2, m - 1, min(63, m - 1), min(64, m - 1)}):          # row i alone: the same bits
        j1, A1 = fk(Rs[i:i + 1], Js[i:i + 1], smpl_consts["parents"], rotate_base=rotate_base)
        assert np.array_equal(j1.cpu().numpy()[0], new_j[i]) and np.array_equal(A1.cpu().numpy()[0], A[i]), i
    _say("fk m=%-4d rotate_base=%d angles near 0 and pi: joints %.1e A %.1e; rows alone == in batch" % (m, rotate_base, ej, eA), max(ej, eA))
    assert ej < 2e-6 and eA < 2e-6
