"""No stage writes past what its *_workspace_bytes query reports (csrc/workspace.h: the query and the carve are one layout).  Every
entry point that carves a caller-owned workspace runs twice through the C ABI: in exactly `need` bytes with 4096 guard bytes of a
pattern behind them, inside the test's own allocation, and in a roomy workspace of 4 x need.  The guard must be untouched and the two
runs' outputs must hold the same bytes.  The engine's own workspaces only grow, so no other test would see a carve that ran a few KB
past the reported size -- the whole-video call would: it packs the stages' workspaces back to back at exactly those sizes."""
import ctypes as C

import numpy as np
import pytest

from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 4096, 0xA5
MODES = ["f32", "bf16", "f16x3"]


@pytest.fixture(scope="module")
def engines(smpl_consts, gpu_device):
    """one engine per operand mode over one weight set that holds both f_movie forms, built on first use"""
    from human_dynamics_amd.engine import HmmrEngine
    w = assets.make_synthetic_weights(0, with_hallucinator=True)
    made = {}

    def get(dt):
        if dt not in made:
            made[dt] = HmmrEngine(w, smpl_consts, dtype=dt, device=gpu_device)
        return made[dt]
    return get


def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def _rand(shape, seed, dev, lo=-1.0, hi=1.0, dtype=None):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(shape, generator=g, dtype=dtype or torch.float32) * (hi - lo) + lo
    return x.to(dev).contiguous()


def exact_and_roomy(dev, need, run, outs):
    """run(ws_ptr, ws_bytes) queues the stage on the current stream and returns its status; outs: the tensors it writes.  Both runs start
    from the same bytes everywhere: the outputs zeroed, the workspaces filled with the pattern (a stage may read its scratch before
    writing it, and the bytes it would then see must not differ between the runs)."""
    import torch
    assert need > 0
    got = []
    for nbytes, ws_bytes in ((need + GUARD, need), (4 * need, 4 * need)):
        ws = torch.full((nbytes,), PATTERN, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
        for o in outs:
            o.view(torch.uint8).zero_()
        rc = run(ws.data_ptr(), ws_bytes)
        torch.cuda.synchronize(dev)
        assert rc == 0, L.load().hmmr_last_error()
        if ws_bytes == need:
            touched = int((ws[need:] != PATTERN).sum())
            assert touched == 0, "%d of the %d guard bytes behind a workspace of %d bytes were written" % (touched, GUARD, need)
            assert bool((ws[:need] != PATTERN).any()), "the stage never wrote its workspace"
        got.append([o.view(torch.uint8).reshape(-1).cpu().numpy().copy() for o in outs])
        del ws
    for k, (a, b) in enumerate(zip(*got)):
        assert a.any(), "output %d was never written" % k
        assert np.array_equal(a, b), "output %d differs between the exact and the roomy workspace in %d bytes" % (k, int((a != b).sum()))


# ------------------------------------------------------------------------- f_movie, IEF, SMPL
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("dt", MODES)
def test_temporal_stays_inside_its_workspace(engines, gpu_device, dt, b):
    import torch
    eng, lib = engines(dt), L.load()
    phi = _rand((b, 20, 2048), 3, gpu_device)
    out = torch.empty_like(phi)
    need = lib.hmmr_temporal_workspace_bytes(b, 20, eng.temporal_dtype)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_temporal_fwd(C.byref(eng.tw), phi.data_ptr(), b, 20, out.data_ptr(), ws, nb,
                                                                           _stream(gpu_device)), [out])


@pytest.mark.parametrize("dt", MODES)
def test_hallucinator_stays_inside_its_workspace(engines, gpu_device, dt):
    import torch
    eng, lib = engines(dt), L.load()
    phi = _rand((3, 2048), 4, gpu_device)
    out = torch.empty_like(phi)
    need = lib.hmmr_hallucinator_workspace_bytes(3, eng.temporal_dtype)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_hallucinator_fwd(C.byref(eng.hw), phi.data_ptr(), 3, out.data_ptr(), ws, nb,
                                                                               _stream(gpu_device)), [out])


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("dt", MODES)
def test_ief_stays_inside_its_workspace(engines, gpu_device, dt, R):
    import torch
    eng, lib = engines(dt), L.load()
    iw = L.IefWeights.from_buffer_copy(eng.iw)                   # (a copy of the host struct: R = 1 runs regressor 0 alone)
    assert eng.iw.num_regressors == 3
    iw.num_regressors = R
    strips = _rand((3, 2048), 5, gpu_device)
    om = torch.empty((R, 3, 85), dtype=torch.float32, device=gpu_device)
    need = lib.hmmr_ief_workspace_bytes(3, R, eng.ief_dtype)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_ief_fwd(C.byref(iw), strips.data_ptr(), 3, om.data_ptr(), ws, nb,
                                                                      _stream(gpu_device)), [om])


@pytest.mark.parametrize("m", [5, 33])
def test_smpl_stays_inside_its_workspace(engines, gpu_device, m):
    import torch
    eng, lib = engines("f16x3"), L.load()
    theta, beta, cams = _rand((m, 72), 6, gpu_device, -0.4, 0.4), _rand((m, 10), 7, gpu_device), _rand((m, 3), 8, gpu_device, 0.5, 1.0)
    V, K = eng.num_verts, eng.num_kps
    verts, joints = torch.empty((m, V, 3), device=gpu_device), torch.empty((m, K, 3), device=gpu_device)
    kps, rs = torch.empty((m, K, 2), device=gpu_device), torch.empty((m, 24, 3, 3), device=gpu_device)
    need = lib.hmmr_smpl_workspace_bytes(m)
    assert lib.hmmr_smpl_workspace_bytes(5) < lib.hmmr_smpl_workspace_bytes(33)          # one group of 32 instances, and two
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_smpl_fwd(C.byref(eng.sc), theta.data_ptr(), 72, beta.data_ptr(), 10, cams.data_ptr(), 3,
                                                                       m, verts.data_ptr(), joints.data_ptr(), kps.data_ptr(), rs.data_ptr(), ws, nb,
                                                                       _stream(gpu_device)), [verts, joints, kps, rs])


# ------------------------------------------------------------------------- the rasteriser
NV, NF, SIZE = 10, 8, 16


def _mesh(n, seed, dev):
    """n poses of a 10-vertex, 8-face fan around the image centre, with cameras that keep it in view"""
    import torch
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, NV - 1, endpoint=False)
    base = np.concatenate([[[0, 0, 0.1]], np.stack([0.6 * np.cos(ang), 0.6 * np.sin(ang), 0 * ang], 1)]).astype(np.float32)
    verts = base[None] + rng.uniform(-0.05, 0.05, (n, NV, 3)).astype(np.float32)
    cams = np.concatenate([rng.uniform(0.7, 1.0, (n, 1)), rng.uniform(-0.1, 0.1, (n, 2))], 1).astype(np.float32)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % (NV - 1)] for i in range(NF)], np.int32)
    return torch.from_numpy(verts).to(dev), torch.from_numpy(cams).to(dev), torch.from_numpy(faces).to(dev)


def _f3(*v):
    return (C.c_float * 3)(*v)


def _lights(d):
    d.bg_color, d.light_dir = _f3(1, 1, 1), _f3(1, .5, -1)
    d.light_int_ambient, d.light_int_directional = 0.7, 0.3
    d.light_color_ambient, d.light_color_directional = _f3(1, 1, 1), _f3(1, 1, 1)
    d.bg_mode, d.size, d.out_h, d.out_w, d.nv, d.nf = L.RENDER_BG_COLOR, SIZE, SIZE, SIZE, NV, NF


@pytest.mark.parametrize("n", [1, 65])
def test_render_mesh_stays_inside_its_workspace(gpu_device, n):
    import torch
    lib = L.load()
    verts, cams, faces = _mesh(n, 11, gpu_device)
    rgb = torch.empty((n, SIZE, SIZE, 3), dtype=torch.uint8, device=gpu_device)
    alpha = torch.empty((n, SIZE, SIZE), dtype=torch.float32, device=gpu_device)
    index = torch.empty((n, 2 * SIZE, 2 * SIZE), dtype=torch.int32, device=gpu_device)
    need = lib.hmmr_render_workspace_bytes(n, NV, NF)
    assert need == lib.hmmr_render_workspace_bytes(min(n, 64), NV, NF)                  # (at n = 65 the second slab is one frame)

    def run(ws, nb):
        d = L.RenderDesc()
        _lights(d)
        d.verts, d.ld_verts, d.cams, d.ld_cam, d.faces, d.n = verts.data_ptr(), 3 * NV, cams.data_ptr(), 3, faces.data_ptr(), n
        d.color, d.bg_mul = _f3(0.65, 0.74, 0.86), 1.0
        d.rgb, d.alpha, d.face_index, d.ws, d.ws_bytes = rgb.data_ptr(), alpha.data_ptr(), index.data_ptr(), ws, nb
        return lib.hmmr_render_mesh(C.byref(d), _stream(gpu_device))
    exact_and_roomy(gpu_device, need, run, [rgb, alpha, index])
    assert int((index >= 0).sum()) > 0 and int(index.max()) < NF                         # faces were drawn


def test_render_scene_stays_inside_its_workspace(gpu_device):
    import torch
    lib = L.load()
    n_frames, n_tracks = 23, 3                                   # slabs of 64 // 3 = 21 frames: the second slab holds two
    meshes = [_mesh(n_frames, 20 + k, gpu_device) for k in range(n_tracks)]
    rgb = torch.empty((n_frames, SIZE, SIZE, 3), dtype=torch.uint8, device=gpu_device)
    owner = torch.empty((n_frames, 2 * SIZE, 2 * SIZE), dtype=torch.int32, device=gpu_device)
    need = lib.hmmr_render_scene_workspace_bytes(n_frames, n_tracks, NV, NF)
    assert need == lib.hmmr_render_scene_workspace_bytes(21, n_tracks, NV, NF) > lib.hmmr_render_scene_workspace_bytes(20, n_tracks, NV, NF)

    def run(ws, nb):
        tracks = (L.SceneTrack * n_tracks)()
        for k, (verts, cams, _) in enumerate(meshes):
            t = tracks[k]
            t.verts, t.ld_verts, t.cams, t.ld_cam, t.start, t.end = verts.data_ptr(), 3 * NV, cams.data_ptr(), 3, 0, n_frames
            t.color = _f3(0.3 * k, 0.5, 0.9 - 0.3 * k)
        d = L.SceneDesc()
        _lights(d)
        d.tracks, d.n_tracks, d.faces, d.n_frames = tracks, n_tracks, meshes[0][2].data_ptr(), n_frames
        d.rgb, d.owner, d.ws, d.ws_bytes = rgb.data_ptr(), owner.data_ptr(), ws, nb
        return lib.hmmr_render_scene(C.byref(d), _stream(gpu_device))
    exact_and_roomy(gpu_device, need, run, [rgb, owner])
    assert int((owner[22] >= 0).sum()) > 0                                               # the last frame of the second slab was drawn


# ------------------------------------------------------------------------- the track front end
def test_track_front_end_stays_inside_its_workspace(gpu_device):
    import torch
    lib = L.load()
    K, off = 25, (C.c_int32 * 3)(0, 7, 7)                        # two tracks of 7 and 0 rows
    kps = _rand((7, K, 3), 31, gpu_device, 10.0, 200.0, dtype=torch.float64)
    kps[..., 2] = 1.0                                            # all visible
    present = torch.ones(7, dtype=torch.uint8, device=gpu_device)
    gauss = (C.c_double * 3)(0.5, 0.2, 0.05)
    raw, smooth = torch.empty((7, 3), dtype=torch.float64, device=gpu_device), torch.empty((7, 3), dtype=torch.float64, device=gpu_device)
    rng = torch.empty((2, 2), dtype=torch.int32, device=gpu_device)
    need = lib.hmmr_track_workspace_bytes(7, 2)
    assert need == 80 * 7
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_track_bbox(kps.data_ptr(), present.data_ptr(), off, 2, K, 0.1, 5, gauss, 2, raw.data_ptr(),
                                                                         smooth.data_ptr(), rng.data_ptr(), ws, nb, _stream(gpu_device)), [raw, smooth, rng])
    assert rng.cpu().tolist()[0] == [0, 7]
    params = raw.clone()
    out = torch.empty_like(params)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_track_smooth(params.data_ptr(), off, 2, 5, gauss, 2, out.data_ptr(), ws, nb,
                                                                           _stream(gpu_device)), [out])


# ------------------------------------------------------------------------- the ResNet and the whole-video call
def test_resnet_stays_inside_its_workspace(engines, gpu_device):
    import torch
    eng, lib = engines("f16x3"), L.load()
    images = torch.from_numpy(assets.make_synthetic_frames(1, seed=9)).to(gpu_device)
    phi = torch.empty((1, 2048), dtype=torch.float32, device=gpu_device)
    need = lib.hmmr_resnet50_workspace_bytes(1, eng.dtype)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_resnet50_fwd(C.byref(eng.rw), images.data_ptr(), 1, 0, phi.data_ptr(), ws, nb,
                                                                           _stream(gpu_device), None), [phi])


@pytest.mark.parametrize("form", ["pred", "hal"])
def test_predict_video_stays_inside_its_workspace(engines, gpu_device, form):
    """n = 9 with passes of 4 frames and 1 window: three ResNet passes, then two tail passes through the same region"""
    import torch
    eng, lib = engines("f16x3"), L.load()
    model = L.Model()
    model.resnet, model.ief, model.smpl = C.pointer(eng.rw), C.pointer(eng.iw), C.pointer(eng.sc)
    if form == "pred":
        model.temporal = C.pointer(eng.tw)
    else:
        model.hallucinator = C.pointer(eng.hw)
    model.sequence_length, model.fov = 20, 13
    n, mf, mw = 9, 4, 1
    plan = L.VideoPlan()
    assert lib.hmmr_video_plan(n, 20, 13, mf, mw, C.byref(plan)) == 0 and (plan.resnet_passes, plan.tail_passes) == (3, 2)
    R = eng.iw.num_regressors
    offs, ld = (C.c_int32 * (R * 7))(), C.c_int64(0)
    L.check(lib.hmmr_record_layout(eng.num_kps, eng.num_verts, R, offs, C.byref(ld)), "hmmr_record_layout")
    images = torch.from_numpy(assets.make_synthetic_frames(n, seed=7)).to(gpu_device)
    rec = torch.empty((n, ld.value), dtype=torch.float32, device=gpu_device)
    need = lib.hmmr_predict_video_workspace_bytes(C.byref(model), n, mf, mw)
    exact_and_roomy(gpu_device, need, lambda ws, nb: lib.hmmr_predict_video(C.byref(model), images.data_ptr(), n, rec.data_ptr(), ld.value, offs, mf, mw,
                                                                            ws, nb, _stream(gpu_device)), [rec])
