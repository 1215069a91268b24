"""Every tracked person through one C call (include/hmmr_hip.h: hmmr_predict_tracks, Tester.predict_tracks): the two ragged copies alone
(csrc/windows.hip) against the NumPy rule of tests/tracks_rule.py and against the one-video copies run on every track's slice, the call
against the per-track route byte for byte -- one pass and several, both f_movie forms -- its refusals, and the Python layer up to the
scene view.

The one-video copies are the ragged kernels launched with a one-track table, so the comparison with them on every track's slice
(test_gather_follows_the_ragged_rule) checks the table the one-video entry builds, not a second implementation.  Each form keeps a pin
of its own: the one-video form tests/golden/reference_windows.npz (tests/test_gpu_video_call.py), the ragged form tests/tracks_rule.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN, Config
from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets
from tracks_rule import G, LENGTHS, MARGIN, T, offsets, ragged_rule

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
CUTS = [(0, 1), (1, 10), (10, 10), (10, 24)]                     # tracks of 1, 9, 0 and 14 frames cut from the 24 seed-7 frames


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _p(off):
    return off.ctypes.data_as(C.POINTER(C.c_int32))


def _phi(n, c, dev):
    """phi[r][j] = 4096 r + j (exact in fp32 for r < 4096, j < 2048), phi_zero[j] = -1 - j: every element names its row and column"""
    import torch
    j = torch.arange(c, dtype=torch.float32, device=dev)
    return (4096.0 * torch.arange(n, dtype=torch.float32, device=dev)[:, None] + j[None, :]).contiguous(), (-1.0 - j).contiguous()


def _ranges(off):
    """(w0, nw): the whole numbering; a start inside a track; a start on a track boundary; a range spanning an empty track; and, with
    more than 64 tracks, ranges across and on every boundary of the argument table's chunks"""
    lengths = np.diff(off)
    base = np.concatenate([[0], np.cumsum(-(-lengths // G))])
    total = int(base[-1])
    out = [(0, total)]
    multi = [k for k in range(len(lengths)) if lengths[k] > G]
    out.append((int(base[multi[0]]) + 1, min(3, total - int(base[multi[0]]) - 1)))                      # starts at a track's second window
    out.append((int(base[multi[-1]]), int(base[multi[-1] + 1] - base[multi[-1]])))                      # exactly one track
    empty = [k for k in range(1, len(lengths) - 1) if lengths[k] == 0 and lengths[k - 1] and lengths[k + 1]]
    out.append((int(base[empty[0]]) - 1, 2))                                                            # the windows on either side of an empty track
    for edge in range(64, len(lengths), 64):
        b = int(base[edge])
        out += [(b - 3, min(7, total - b + 3)), (b, min(4, total - b)), (b - 2, 2)]
    assert all(w0 >= 0 and nw >= 1 and w0 + nw <= total for w0, nw in out), out
    return out


# ------------------------------------------------------------------------- gather
def _gather(lib, phi, zero, off, w0, nw, dev):
    import torch
    c = phi.shape[1]
    out = torch.full((nw + 1, T, c), SENTINEL, dtype=torch.float32, device=dev)           # one window of sentinel behind the last
    L.check(lib.hmmr_gather_windows_tracks(phi.data_ptr(), zero.data_ptr(), _p(off), len(off) - 1, w0, nw, T, MARGIN, G, c, out.data_ptr(),
                                           _stream(dev)), "hmmr_gather_windows_tracks")
    torch.cuda.synchronize(dev)
    assert bool((out[nw] == SENTINEL).all())
    return out[:nw].cpu().numpy()


@pytest.mark.parametrize("c", [2048, 8])
@pytest.mark.parametrize("name", ["mixed", "many"])
def test_gather_follows_the_ragged_rule(gpu_device, name, c):
    import torch
    lib = L.load()
    off = offsets(LENGTHS[name])
    fed, owner, _ = ragged_rule(off)
    phi, zero = _phi(int(off[-1]), c, gpu_device)
    col = np.arange(c, dtype=np.float64)
    want = np.where(fed[..., None] >= 0, 4096.0 * fed[..., None] + col, -1.0 - col).astype(np.float32)
    full = _gather(lib, phi, zero, off, 0, len(owner), gpu_device)
    assert np.array_equal(full, want)
    # no slot of a track holds a row of a neighbour, and every track's windows are what the one-video copy gives for its slice alone
    row = np.floor(full[..., 0].astype(np.float64) / 4096.0)
    first = 0
    for k in range(len(off) - 1):
        n_k = int(off[k + 1] - off[k])
        nw = -(-n_k // G)
        mine = full[first:first + nw]
        r = row[first:first + nw]
        assert ((mine[..., 0] < 0) | ((r >= off[k]) & (r < off[k + 1]))).all(), k
        if nw:
            alone = torch.full((nw, T, c), SENTINEL, dtype=torch.float32, device=gpu_device)
            L.check(lib.hmmr_gather_windows(phi[int(off[k]):].data_ptr(), n_k, zero.data_ptr(), 0, nw, T, MARGIN, G, c, alone.data_ptr(),
                                            _stream(gpu_device)), "hmmr_gather_windows")
            assert np.array_equal(alone.cpu().numpy(), mine), k
        first += nw
    assert first == len(owner)
    for w0, nw in _ranges(off)[1:]:
        assert np.array_equal(_gather(lib, phi, zero, off, w0, nw, gpu_device), want[w0:w0 + nw]), (w0, nw)


# ------------------------------------------------------------------------- keep
def _keep(lib, strips, off, w0, nw, out, dev):
    """windows [w0, w0 + nw) of strips [n_windows][T][c] -> their rows of out; returns (o0, keep)"""
    o0, keep = C.c_int(-1), C.c_int(-1)
    L.check(lib.hmmr_tracks_window_rows(_p(off), len(off) - 1, G, w0, nw, C.byref(o0), C.byref(keep)), "hmmr_tracks_window_rows")
    L.check(lib.hmmr_keep_rows_tracks(strips[w0:].data_ptr(), _p(off), len(off) - 1, w0, nw, T, MARGIN, G, strips.shape[2], out[o0.value:].data_ptr(),
                                      out.shape[1], _stream(dev)), "hmmr_keep_rows_tracks")
    return o0.value, keep.value


@pytest.mark.parametrize("c", [2048, 8])
@pytest.mark.parametrize("name", ["mixed", "many"])
def test_keep_writes_every_track_s_centre_rows_and_nothing_else(gpu_device, name, c):
    import torch
    lib = L.load()
    off = offsets(LENGTHS[name])
    _, owner, kept = ragged_rule(off)
    n, nw = int(off[-1]), len(owner)
    strips, _ = _phi(nw * T, c, gpu_device)                                               # slot (w, t) holds 4096 (20 w + t) + j
    strips = strips.reshape(nw, T, c)
    ld = c + 12
    out = torch.full((n + 1, ld), SENTINEL, dtype=torch.float32, device=gpu_device)
    assert _keep(lib, strips, off, 0, nw, out, gpu_device) == (0, n)
    torch.cuda.synchronize(gpu_device)
    got = out.cpu().numpy()
    src = np.full(n, -1, np.int64)
    for w in range(nw):
        for slot, r in kept[w]:
            src[r] = w * T + slot
    assert (src >= 0).all()
    want = (4096.0 * src[:, None] + np.arange(c)[None, :]).astype(np.float32)
    assert np.array_equal(got[:n, :c], want)
    assert (got[:n, c:] == SENTINEL).all() and (got[n:] == SENTINEL).all()
    # two tail passes write what one does; the first leaves the second's rows alone
    for w0 in sorted({nw // 2} | {w for w, _ in _ranges(off)[1:]}):
        if not 0 < w0 < nw:
            continue
        two = torch.full_like(out, SENTINEL)
        o0, keep = _keep(lib, strips, off, 0, w0, two, gpu_device)
        torch.cuda.synchronize(gpu_device)
        assert o0 == 0 and bool((two[keep:] == SENTINEL).all())
        o1, keep1 = _keep(lib, strips, off, w0, nw - w0, two, gpu_device)
        torch.cuda.synchronize(gpu_device)
        assert o1 == keep and keep + keep1 == n and np.array_equal(two.cpu().numpy(), got), w0
    # a range in the middle writes its own rows only
    for w0, cnt in _ranges(off)[1:]:
        part = torch.full_like(out, SENTINEL)
        o0, keep = _keep(lib, strips, off, w0, cnt, part, gpu_device)
        torch.cuda.synchronize(gpu_device)
        p = part.cpu().numpy()
        assert np.array_equal(p[o0:o0 + keep], got[o0:o0 + keep]) and (p[:o0] == SENTINEL).all() and (p[o0 + keep:] == SENTINEL).all(), (w0, cnt)


# ------------------------------------------------------------------------- the whole call
@pytest.fixture(scope="module")
def testers(weights, smpl_consts, gpu_device):
    """Tester per operand mode, built on first use and shared by the tests of this module"""
    from human_dynamics_amd.evaluation.tester import Tester
    made = {}

    def get(dt):
        if dt not in made:
            made[dt] = Tester(Config(batch_size=2), weights=weights, smpl=smpl_consts, dtype=dt, device=gpu_device)
        return made[dt]
    return get


@pytest.fixture(scope="module")
def frames24():
    return assets.make_synthetic_frames(24, seed=7)


@pytest.fixture(scope="module")
def reference(testers, frames24, gpu_device):
    """Tester.predict_all_images (stream=False) on every non-empty track of CUTS alone, computed once per (mode, track) and left unchanged"""
    import torch
    made = {}

    def get(dt, k):
        if (dt, k) not in made:
            a, b = CUTS[k]
            made[(dt, k)] = testers(dt).predict_all_images(torch.from_numpy(frames24[a:b]).to(gpu_device), stream=False)
        return made[(dt, k)]
    return get


def _same_bytes(got, want):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, float(np.abs(got[k] - want[k]).max()))


def _same_tracks(got, want_of):
    """got: predict_tracks' list for CUTS; the empty track has every key of the others, with no row"""
    assert len(got) == len(CUTS)
    for k, (a, b) in enumerate(CUTS):
        if b > a:
            _same_bytes(got[k], want_of(k))
        else:
            assert sorted(got[k]) == sorted(want_of(0)) and all(v.shape == (0,) + want_of(0)[key].shape[1:] for key, v in got[k].items())


@pytest.mark.parametrize("dt", ["f32", "f16x3"])
def test_tracks_call_equals_the_per_track_route_bit_for_bit(testers, reference, frames24, gpu_device, dt):
    import torch
    t = testers(dt)
    want_of = lambda k: reference(dt, k)
    assert want_of(3)["verts"].shape == (14, 6890, 3) and want_of(1)["omegas_delta"].shape == (9, 2, 85) and float(np.abs(want_of(3)["verts"]).max()) > 0.1
    tracks = [torch.from_numpy(frames24[a:b]).to(gpu_device) for a, b in CUTS]
    _same_tracks(t.predict_tracks(tracks), want_of)
    # several ResNet passes (the 1-frame and the 9-frame track share the first) and several tail passes (windows of two tracks in one): the same bytes
    _same_tracks(t.predict_tracks(tracks, max_frames=8, max_windows=2), want_of)
    assert t.precision["saturated"] is False


def _layout_args(t, lib):
    eng = t.engine
    layout, rec_len = t.record_layout()
    R = eng.iw.num_regressors
    offs, ld = (C.c_int32 * (R * 7))(), C.c_int64(0)
    L.check(lib.hmmr_record_layout(eng.num_kps, eng.num_verts, R, offs, C.byref(ld)), "hmmr_record_layout")
    assert ld.value == rec_len
    return layout, rec_len, offs


def test_one_track_gives_the_one_video_call_s_record_buffer(testers, frames24, gpu_device):
    import torch
    t, lib = testers("f32"), L.load()
    N = 9
    frames = torch.from_numpy(frames24[:N]).to(gpu_device)
    layout, rec_len, offs = _layout_args(t, lib)
    model = t.native_model()
    off = offsets([N])
    for mf, mw in ((1024, 128), (8, 1)):
        nbytes = lib.hmmr_predict_tracks_workspace_bytes(C.byref(model), _p(off), 1, mf, mw)
        assert nbytes == lib.hmmr_predict_video_workspace_bytes(C.byref(model), N, mf, mw) > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
        one = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
        many = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
        L.check(lib.hmmr_predict_video(C.byref(model), frames.data_ptr(), N, one.data_ptr(), rec_len, offs, mf, mw, ws.data_ptr(), nbytes,
                                       _stream(gpu_device)), "hmmr_predict_video")
        L.check(lib.hmmr_predict_tracks(C.byref(model), frames.data_ptr(), _p(off), 1, many.data_ptr(), rec_len, offs, mf, mw, ws.data_ptr(), nbytes,
                                        _stream(gpu_device)), "hmmr_predict_tracks")
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(one.view(torch.int32), many.view(torch.int32)) and not bool((many == SENTINEL).any())
    # no track, or only empty ones: 0, and nothing is written
    for lengths in ([], [0, 0]):
        off0 = offsets(lengths)
        assert lib.hmmr_predict_tracks(C.byref(model), None, _p(off0), len(lengths), None, rec_len, offs, 1024, 128, None, 0, _stream(gpu_device)) == 0


def test_the_two_public_entries_agree(testers, reference, frames24, gpu_device):
    """a video is the one-track case: for the 9 frames of CUTS[1], several ResNet and tail passes, hmmr_predict_video and hmmr_predict_tracks
    with {0, 9} ask for the same workspace and write the same bytes, those of the per-track route"""
    import torch
    from human_dynamics_amd.dist import unpack_outputs
    t, lib = testers("f32"), L.load()
    a, b = CUTS[1]
    N, mf, mw = b - a, 8, 1
    assert N == 9
    frames = torch.from_numpy(frames24[a:b]).to(gpu_device)
    layout, rec_len, offs = _layout_args(t, lib)
    model = t.native_model()
    off = offsets([N])
    nbytes = lib.hmmr_predict_video_workspace_bytes(C.byref(model), N, mf, mw)
    assert nbytes == lib.hmmr_predict_tracks_workspace_bytes(C.byref(model), _p(off), 1, mf, mw) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)
    one = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
    many = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
    L.check(lib.hmmr_predict_video(C.byref(model), frames.data_ptr(), N, one.data_ptr(), rec_len, offs, mf, mw, ws.data_ptr(), nbytes,
                                   _stream(gpu_device)), "hmmr_predict_video")
    L.check(lib.hmmr_predict_tracks(C.byref(model), frames.data_ptr(), _p(off), 1, many.data_ptr(), rec_len, offs, mf, mw, ws.data_ptr(), nbytes,
                                    _stream(gpu_device)), "hmmr_predict_tracks")
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(one.view(torch.int32), many.view(torch.int32))
    for rec in (one, many):
        _same_bytes({k: v.cpu().numpy() for k, v in unpack_outputs(rec, layout).items()}, reference("f32", 1))


def test_tracks_call_in_hal_mode_equals_the_per_track_route(smpl_consts, gpu_device):
    import torch
    from human_dynamics_amd.evaluation.tester import Tester
    w = assets.make_synthetic_weights(0, with_hallucinator=True)
    t = Tester(Config(batch_size=2, pred_mode="hal"), weights=w, smpl=smpl_consts, dtype="f32", device=gpu_device)
    m = t.native_model()
    assert not m.temporal and bool(m.hallucinator)
    frames = torch.from_numpy(assets.make_synthetic_frames(9, seed=21)).to(gpu_device)
    tracks = [frames[:4], frames[4:]]
    want = [t.predict_all_images(trk, stream=False) for trk in tracks]
    for kw in (dict(), dict(max_frames=8, max_windows=1)):
        got = t.predict_tracks(tracks, **kw)
        assert len(got) == 2
        _same_bytes(got[0], want[0])
        _same_bytes(got[1], want[1])


def test_refused_tracks_calls_queue_nothing(testers, reference, frames24, gpu_device):
    import torch
    t = testers("f32")
    lib = L.load()
    tracks = [(a, b) for a, b in CUTS]
    off = offsets([b - a for a, b in tracks])
    N = int(off[-1])
    frames = torch.from_numpy(frames24[:N]).to(gpu_device)
    layout, rec_len, offs = _layout_args(t, lib)
    rec = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
    model = t.native_model()
    nbytes = lib.hmmr_predict_tracks_workspace_bytes(C.byref(model), _p(off), len(tracks), 1024, 128)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)

    def call(model=model, off=off, ws_bytes=nbytes, ld_rec=rec_len, images=None):
        return lib.hmmr_predict_tracks(C.byref(model), images or frames.data_ptr(), _p(off), len(off) - 1, rec.data_ptr(), ld_rec, offs, 1024, 128,
                                       ws.data_ptr(), ws_bytes, _stream(gpu_device))

    def refused(rc, word):
        torch.cuda.synchronize(gpu_device)
        assert rc == -1 and word in lib.hmmr_last_error(), (rc, lib.hmmr_last_error())
        assert bool((rec == SENTINEL).all())

    refused(call(off=np.array([0, 1, 10, 9, 24], np.int32)), b"must not decrease")
    refused(call(off=np.array([4, 4, 10, 10, 24], np.int32)), b"track_offsets[0]=4")
    refused(call(ws_bytes=nbytes - 1), b"workspace too small")
    refused(call(ld_rec=rec_len - 1), b"does not fit")
    refused(call(images=frames.data_ptr() + 4), b"images must be 16-byte aligned")        # -1 from the call's own checks, not -2 from its first pass
    both = t.native_model()
    both.hallucinator = C.pointer(L.HallucinatorWeights())
    refused(call(model=both), b"exactly one")
    neither = t.native_model()
    neither.temporal = None
    refused(call(model=neither), b"exactly one")
    # the same arguments, accepted: the sentinel is gone and every track's rows are the Tester's for that track alone
    assert call() == 0
    torch.cuda.synchronize(gpu_device)
    from human_dynamics_amd.dist import unpack_outputs
    for k, (a, b) in enumerate(tracks):
        if b > a:
            _same_bytes({key: v.cpu().numpy() for key, v in unpack_outputs(rec[a:b], layout).items()}, reference("f32", k))


# ------------------------------------------------------------------------- the Python layer
def test_predict_tracks_python_layer(testers, reference, frames24, gpu_device):
    import torch
    from human_dynamics_amd.dist import unpack_outputs
    t = testers("f32")
    want_of = lambda k: reference("f32", k)
    dev_tracks = [torch.from_numpy(frames24[a:b]).to(gpu_device) for a, b in CUTS]
    _same_tracks(t.predict_tracks([frames24[a:b] for a, b in CUTS]), want_of)                 # host arrays
    _same_tracks(t.predict_videos(dev_tracks, batched=True), want_of)                         # device tensors through predict_videos
    some = t.predict_tracks(dev_tracks, want=("joints", "omegas"))
    assert [sorted(d) for d in some] == [["joints", "omegas"]] * 4 and np.array_equal(some[3]["joints"], want_of(3)["joints"])
    views, layout = t.predict_tracks(dev_tracks, records=True)
    assert layout == t.record_layout()[0] and [tuple(v.shape) for v in views] == [(b - a, t.record_layout()[1]) for a, b in CUTS]
    assert all(v.is_cuda for v in views) and views[1].data_ptr() == views[0].data_ptr() + 4 * t.record_layout()[1]      # views of ONE buffer
    _same_tracks([{k: v.cpu().numpy() for k, v in unpack_outputs(view, layout).items()} for view in views], want_of)
    with pytest.raises(ValueError, match="uint8"):
        t.predict_tracks([np.zeros((2, 224, 224, 3), np.uint8)])
    assert t.predict_tracks([]) == []


def _track_records(t, crops):
    """the per-track route down to Tester.predict_records: features, the padded windows of Tester.predict_windows_device, f_movie, the
    kept rows, IEF and SMPL for ONE track"""
    import torch
    from human_dynamics_amd.evaluation.tester import window_plan
    N, B = len(crops), t.batch_size
    phi = t.features(crops, n_zero=1)
    margin, g, count, num_fill = window_plan(N, B, t.sequence_length, t.fov)
    padded = torch.cat([phi[N:].expand(margin, -1), phi[:N], phi[N:].expand(num_fill, -1)], dim=0)
    idx = torch.arange(count * B, device=phi.device)[:, None] * g + torch.arange(t.sequence_length, device=phi.device)[None, :]
    return t.predict_strips_records(padded[idx], N)


def test_crops_to_scene_chain_equals_the_per_track_chain(testers, gpu_device):
    """process_tracks -> predict_tracks(records=True) -> render_scene against the same chain through per-track predict_records: two
    recorded tracks of 13 and 6 frames over 13 small frames, a synthetic triangle list over the synthetic body's vertices"""
    import os
    import torch
    from human_dynamics_amd.evaluation.run_video import process_tracks
    from human_dynamics_amd.evaluation.tracks import unpack_tracks
    from human_dynamics_amd.util.render import video
    ref = np.load(os.path.join(GOLDEN, "reference_tracks.npz"))
    h, w = (int(v) for v in ref["mixed/hw"])
    kps = unpack_tracks(ref["mixed/kps"], ref["mixed/present"], ref["mixed/offsets"])
    kps = [kps[1], kps[4]]
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (13, h, w, 3), dtype=np.uint8)).to(gpu_device)
    per_track = process_tracks(frames, kps, vis_thresh=0.1)
    assert [r for _, r, _ in per_track] == [(0, 13), (0, 6)]
    faces = np.stack([np.arange(0, 6880, 20), np.arange(5, 6885, 20), np.arange(9, 6889, 20)], axis=1).astype(np.int32)
    t = testers("f32")
    views, layout = t.predict_tracks([crops for crops, _, _ in per_track], records=True)
    alone = [_track_records(t, crops) for crops, _, _ in per_track]
    for a, b in zip(views, alone):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    scene = lambda recs: video.render_scene([(r, layout, rng, infos) for r, (_, rng, infos) in zip(recs, per_track)], frames, faces, max_img_size=96,
                                            device=torch.device(gpu_device))
    got, want = scene(views), scene(alone)
    assert got.dtype == torch.uint8 and got.shape[0] == 13 and torch.equal(got, want)
