"""A whole video through one C call (include/hmmr_hip.h: hmmr_predict_video, Tester.predict_all_images_native): the two copies of the
sliding-window scheme alone (csrc/windows.hip) against the reference's recorded windows, the call against Tester.predict_all_images bit
for bit -- one pass and several, both f_movie forms -- and against the golden video, its refusals, and the Python-free program
tests/c_abi/predict_video.c."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import Config
from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 8), (24, 2), (64, 8), (65, 8), (100, 3), (256, 8)]      # (N, B) of tests/golden/reference_windows.npz
T, MARGIN, G = 20, 6, 8
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def windows():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_windows.npz")))


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


# ------------------------------------------------------------------------- gather
def _phi(n, c, dev):
    """phi[r][j] = 4096 r + j (exact in fp32 for r <= 256, j < 2048), phi_zero[j] = -1 - j: every element names its row and column"""
    import torch
    j = torch.arange(c, dtype=torch.float32, device=dev)
    return (4096.0 * torch.arange(n, dtype=torch.float32, device=dev)[:, None] + j[None, :]).contiguous(), (-1.0 - j).contiguous()


def _gather(lib, phi, zero, w0, nw, dev):
    import torch
    n, c = phi.shape
    out = torch.full((nw + 1, T, c), SENTINEL, dtype=torch.float32, device=dev)           # one window of sentinel behind the last
    L.check(lib.hmmr_gather_windows(phi.data_ptr(), n, zero.data_ptr(), w0, nw, T, MARGIN, G, c, out.data_ptr(), _stream(dev)), "hmmr_gather_windows")
    torch.cuda.synchronize(dev)
    assert bool((out[nw] == SENTINEL).all())
    return out[:nw].cpu().numpy()


@pytest.mark.parametrize("c", [2048, 8])
@pytest.mark.parametrize("N,B", CASES)
def test_gather_feeds_what_the_reference_fed(gpu_device, windows, N, B, c):
    lib = L.load()
    phi, zero = _phi(N, c, gpu_device)
    fed = windows["fed_n%d_b%d" % (N, B)]                                                # frame numbers from 1; -1 = the zero image
    assert fed.shape[0] == {1: 8, 24: 4, 64: 8, 65: 16, 100: 15, 256: 32}[N] >= -(-N // G)
    # every window the reference ran, count * batch_size of them: those past ceil(N / G) keep no frame, but the early slots of the first
    # one still hold real frames -- the one-video gather takes any window range, not only the numbering of its single track
    got = _gather(lib, phi, zero, 0, fed.shape[0], gpu_device)
    col = np.arange(c, dtype=np.float64)
    want = np.where(fed[..., None] > 0, 4096.0 * (fed[..., None] - 1) + col, -1.0 - col).astype(np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("c", [2048, 8])
def test_gather_of_a_window_range_equals_the_rows_of_the_full_gather(gpu_device, c):
    lib = L.load()
    phi, zero = _phi(100, c, gpu_device)
    full = _gather(lib, phi, zero, 0, 13, gpu_device)
    part = _gather(lib, phi, zero, 5, 3, gpu_device)
    assert np.array_equal(part, full[5:8]) and float(part.max()) > 4096.0 * 40


# ------------------------------------------------------------------------- keep
def _keep(lib, strips, w0, nw, n_total, out, row0, dev):
    c = strips.shape[2]
    L.check(lib.hmmr_keep_rows(strips[w0:].data_ptr(), w0, nw, T, MARGIN, G, c, n_total, out[row0:].data_ptr(), out.shape[1], _stream(dev)),
            "hmmr_keep_rows")


@pytest.mark.parametrize("c", [2048, 8])
@pytest.mark.parametrize("N", [1, 8, 9, 24, 65])
def test_keep_writes_the_centre_rows_and_nothing_else(gpu_device, N, c):
    import torch
    lib = L.load()
    nw = -(-N // G)
    strips, _ = _phi(nw * T, c, gpu_device)                                               # slot (w, t) holds 4096 (20 w + t) + j
    strips = strips.reshape(nw, T, c)
    ld = c + 12
    out = torch.full((nw * G + 1, ld), SENTINEL, dtype=torch.float32, device=gpu_device)
    _keep(lib, strips, 0, nw, N, out, 0, gpu_device)
    torch.cuda.synchronize(gpu_device)
    got = out.cpu().numpy()
    f = np.arange(N)
    want = (4096.0 * ((f // G) * T + MARGIN + f % G)[:, None] + np.arange(c)[None, :]).astype(np.float32)
    assert np.array_equal(got[:N, :c], want)
    assert (got[:N, c:] == SENTINEL).all() and (got[N:] == SENTINEL).all()
    if nw > 1:      # the same frames as two tail passes: the second one's windows start at w0 > 0 and land at row w0 g
        w0 = nw // 2
        two = torch.full_like(out, SENTINEL)
        _keep(lib, strips, 0, w0, N, two, 0, gpu_device)
        torch.cuda.synchronize(gpu_device)
        assert bool((two[w0 * G:] == SENTINEL).all())
        _keep(lib, strips, w0, nw - w0, N, two, w0 * G, gpu_device)
        torch.cuda.synchronize(gpu_device)
        assert np.array_equal(two.cpu().numpy(), got)
    if N == 9:      # two windows more than hold a kept frame: the copy clips at n_total and writes rows 0 .. 8 only ...
        more = torch.full_like(out, SENTINEL)
        L.check(lib.hmmr_keep_rows(strips.data_ptr(), 0, 4, T, MARGIN, G, c, N, more.data_ptr(), ld, _stream(gpu_device)), "hmmr_keep_rows")
        torch.cuda.synchronize(gpu_device)
        assert np.array_equal(more.cpu().numpy(), got)
        # ... and windows that hold none are no error: 0, and nothing is written
        assert lib.hmmr_keep_rows(strips.data_ptr(), 2, 2, T, MARGIN, G, c, N, more[2 * G:].data_ptr(), ld, _stream(gpu_device)) == 0
        torch.cuda.synchronize(gpu_device)
        assert np.array_equal(more.cpu().numpy(), got)


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
    """Tester.predict_all_images on the first N of the seed-7 frames, computed once per (mode, N) and left unchanged"""
    import torch
    made = {}

    def get(dt, N):
        if (dt, N) not in made:
            dev_frames = torch.from_numpy(frames24[:N]).to(gpu_device)
            made[(dt, N)] = testers(dt).predict_all_images(dev_frames, stream=False)
        return made[(dt, N)]
    return get


def _same_bytes(got, want):
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, float(np.abs(got[k] - want[k]).max()))


@pytest.mark.parametrize("N", [1, 9, 24])
@pytest.mark.parametrize("dt", ["f32", "f16x3"])
def test_native_call_equals_predict_all_images_bit_for_bit(testers, reference, frames24, gpu_device, dt, N):
    import torch
    t, want = testers(dt), reference(dt, N)
    assert want["verts"].shape == (N, 6890, 3) and want["omegas_delta"].shape == (N, 2, 85) and float(np.abs(want["verts"]).max()) > 0.1
    dev_frames = torch.from_numpy(frames24[:N]).to(gpu_device)
    _same_bytes(t.predict_all_images_native(dev_frames), want)
    # several ResNet passes and several tail passes (at N = 24 the zero image rides on a full last pass of 8 frames): the same bytes
    _same_bytes(t.predict_all_images_native(dev_frames, max_frames=8, max_windows=2), want)
    assert t.precision["saturated"] is False


def test_native_call_f32_matches_the_golden_video(testers, frames24, golden_video):
    """the independent pin: keys and tolerance of test_predict_all_images_fp32_matches_golden_video"""
    res = testers("f32").predict_all_images_native(frames24)
    assert res["verts"].shape == (24, 6890, 3) and res["omegas_delta"].shape == (24, 2, 85)
    for k, g in golden_video.items():
        if k in ("phi", "strips", "omegas_all"):
            continue
        got = res[k[:-4]][..., ::16, :] if k.endswith("_sub") else res[k]
        assert got.shape == g.shape, (k, got.shape, g.shape)
        assert float(np.abs(got - g).max()) < 1e-4, k


def test_native_call_in_hal_mode_equals_the_tester(smpl_consts, gpu_device):
    import torch
    from human_dynamics_amd.evaluation.tester import Tester
    w = assets.make_synthetic_weights(0, with_hallucinator=True)
    t = Tester(Config(batch_size=2, pred_mode="hal"), weights=w, smpl=smpl_consts, dtype="f32", device=gpu_device)
    m = t.native_model()
    assert not m.temporal and bool(m.hallucinator)
    frames = torch.from_numpy(assets.make_synthetic_frames(9, seed=21)).to(gpu_device)
    want = t.predict_all_images(frames, stream=False)
    _same_bytes(t.predict_all_images_native(frames), want)
    _same_bytes(t.predict_all_images_native(frames, max_frames=8, max_windows=1), want)
    # and the hallucinator is what ran: the temporal encoder of the same weights gives other numbers
    t_pred = Tester(Config(batch_size=2), weights=w, smpl=smpl_consts, dtype="f32", device=gpu_device)
    assert float(np.abs(t_pred.predict_all_images_native(frames)["omegas"] - want["omegas"]).max()) > 1e-3


def test_refused_calls_queue_nothing(testers, frames24, gpu_device):
    import torch
    t = testers("f32")
    eng, lib = t.engine, L.load()
    N = 9
    frames = torch.from_numpy(frames24[:N]).to(gpu_device)
    layout, rec_len = t.record_layout()
    R = eng.iw.num_regressors
    offs, ld = (C.c_int32 * (R * 7))(), C.c_int64(0)
    L.check(lib.hmmr_record_layout(eng.num_kps, eng.num_verts, R, offs, C.byref(ld)), "hmmr_record_layout")
    assert ld.value == rec_len
    rec = torch.full((N, rec_len), SENTINEL, dtype=torch.float32, device=gpu_device)
    model = t.native_model()
    nbytes = lib.hmmr_predict_video_workspace_bytes(C.byref(model), N, 1024, 128)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu_device)

    def call(model=model, ws_bytes=nbytes, ld_rec=rec_len, images=None):
        return lib.hmmr_predict_video(C.byref(model), images or frames.data_ptr(), N, rec.data_ptr(), ld_rec, offs, 1024, 128, ws.data_ptr(), ws_bytes,
                                      _stream(gpu_device))

    def refused(rc, word):
        torch.cuda.synchronize(gpu_device)
        assert rc == -1 and word in lib.hmmr_last_error(), (rc, lib.hmmr_last_error())
        assert bool((rec == SENTINEL).all())

    refused(call(ws_bytes=nbytes - 1), b"workspace too small")
    both = t.native_model()
    both.hallucinator = C.pointer(L.HallucinatorWeights())
    refused(call(model=both), b"exactly one")
    neither = t.native_model()
    neither.temporal = None
    refused(call(model=neither), b"exactly one")
    refused(call(ld_rec=rec_len - 1), b"does not fit")
    even = t.native_model()
    even.fov = 12
    refused(call(model=even), b"odd")
    refused(call(images=frames.data_ptr() + 4), b"images must be 16-byte aligned")      # -1 from the call's own checks, not -2 from its first pass
    # the same arguments, accepted: the sentinel is gone and the records are the Tester's
    assert call() == 0
    torch.cuda.synchronize(gpu_device)
    from human_dynamics_amd.dist import unpack_outputs
    want = t.predict_all_images(frames, stream=False)
    _same_bytes({k: v.cpu().numpy() for k, v in unpack_outputs(rec, layout).items()}, want)


# ------------------------------------------------------------------------- the Python-free program
@pytest.fixture(scope="module")
def c_program(weights, smpl_consts, tmp_path_factory):
    """tests/c_abi/predict_video.c compiled once, and one dump of every checkpoint variable and the SMPL source arrays"""
    d = tmp_path_factory.mktemp("predict_video")
    exe, pkg = str(d / "predict_video"), os.path.join(ROOT, "human_dynamics_amd")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-x", "hip", os.path.join(ROOT, "tests", "c_abi", "predict_video.c"),
                        "-I", os.path.join(ROOT, "include"), "-L", pkg, "-lhmmr_hip", "-Wl,-rpath," + pkg, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    dump = {k: v for k, v in weights.items() if np.asarray(v).dtype.kind == "f"}
    for k, name in (("v_template", "v_template"), ("shapedirs", "shapedirs"), ("posedirs", "posedirs"), ("J_regressor", "J_regressor"),
                    ("lbs_weights", "lbs_weights"), ("cocoplus_regressor", "kp_regressor"), ("parents", "parents")):
        dump["smpl/" + name] = np.asarray(smpl_consts[k], np.float32)
    with open(str(d / "vars.bin"), "wb") as f:
        f.write(struct.pack("<i", len(dump)))
        for k in sorted(dump):
            a = np.ascontiguousarray(dump[k], np.float32)
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", a.size))
            a.tofile(f)
    frames = assets.make_synthetic_frames(21, seed=17)
    frames.astype(np.float32).tofile(str(d / "frames.bin"))
    return exe, d, frames


@pytest.mark.parametrize("dt", ["f32", "f16x3"])
def test_c_program_runs_a_video_without_python(testers, c_program, gpu_device, dt):
    import torch
    exe, d, frames = c_program
    n, out = len(frames), str(d / ("records_%s.bin" % dt))
    code = {"f32": L.HMMR_F32, "f16x3": L.HMMR_F16X3}[dt]
    r = subprocess.run([exe, str(d / "vars.bin"), str(d / "frames.bin"), str(n), str(code), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "run flags 0" in r.stdout
    t = testers(dt)
    layout, rec_len = t.record_layout()
    rec = np.fromfile(out, np.float32).reshape(n, rec_len)
    want = t.predict_all_images(torch.from_numpy(frames).to(gpu_device), stream=False)
    _same_bytes({k: np.ascontiguousarray(rec[:, off:off + size]).reshape((n,) + shp) for k, shp, off, size in layout}, want)
