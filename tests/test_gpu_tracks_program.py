"""The Python-free program for several tracks (tests/c_abi/predict_tracks.c: predict_video.c with an offsets argument) against the
per-track route of the Python mirror, byte for byte."""
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
OFFSETS = [0, 4, 4, 13, 21]                                      # tracks of 4, 0, 9 and 8 frames


@pytest.fixture(scope="module")
def c_program(weights, smpl_consts, tmp_path_factory):
    """the program compiled once, and one dump of every checkpoint variable and the SMPL source arrays (the format of predict_video.c)"""
    d = tmp_path_factory.mktemp("predict_tracks")
    exe, pkg = str(d / "predict_tracks"), os.path.join(ROOT, "human_dynamics_amd")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-x", "hip", os.path.join(ROOT, "tests", "c_abi", "predict_tracks.c"),
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
    frames = assets.make_synthetic_frames(OFFSETS[-1], seed=17)
    frames.astype(np.float32).tofile(str(d / "frames.bin"))
    return exe, d, frames


@pytest.mark.parametrize("dt", ["f16x3"])                        # (the f32 route of the call: tests/test_gpu_tracks_call.py)
def test_c_program_runs_every_track_without_python(c_program, weights, smpl_consts, gpu_device, dt):
    import torch
    from human_dynamics_amd.evaluation.tester import Tester
    exe, d, frames = c_program
    n, out = len(frames), str(d / ("records_%s.bin" % dt))
    code = {"f32": L.HMMR_F32, "f16x3": L.HMMR_F16X3}[dt]
    r = subprocess.run([exe, str(d / "vars.bin"), str(d / "frames.bin"), ",".join(str(o) for o in OFFSETS), str(code), out], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "4 tracks, 21 frames, 4 windows" in r.stdout and "run flags 0" in r.stdout
    t = Tester(Config(batch_size=2), weights=weights, smpl=smpl_consts, dtype=dt, device=gpu_device)
    layout, rec_len = t.record_layout()
    rec = np.fromfile(out, np.float32).reshape(n, rec_len)
    for a, b in zip(OFFSETS, OFFSETS[1:]):
        if b == a:
            continue
        want = t.predict_all_images(torch.from_numpy(frames[a:b]).to(gpu_device), stream=False)
        got = {k: np.ascontiguousarray(rec[a:b, off:off + size]).reshape((b - a,) + shp) for k, shp, off, size in layout}
        assert sorted(got) == sorted(want)
        for k in sorted(want):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (k, float(np.abs(got[k] - want[k]).max()))
