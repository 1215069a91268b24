"""hmmr_video_bbox refuses what its kernel could not honour before anything is launched: dummy, never dereferenced device
pointers and no device (the pattern of test_abi.py::test_periphery_argument_validation_reports_errors).  `offsets` is host
memory and is read."""
import ctypes as C

import pytest

from human_dynamics_amd import _lib


def test_video_bbox_refusals():
    lib = _lib.load()
    P = [0x1000 * (i + 1) for i in range(8)]

    def call(**kw):
        a = dict(cams=P[0], ldc=90, kps=P[1], ldk=90, k=25, proc=P[2], size=224.0, off=[0, 7, 7, 20], h=720, w=1280, margin=10.0,
                 bbox=P[3], crop=P[4], status=P[5])
        a.update(kw)
        off = a["off"]
        arr = (C.c_int32 * len(off))(*off) if off is not None else None
        n_tracks = a.get("n_tracks", len(off) - 1 if off is not None else 1)
        return lib.hmmr_video_bbox(a["cams"], a["ldc"], a["kps"], a["ldk"], a["k"], a["proc"], a["size"], arr, n_tracks, a["h"], a["w"],
                                   a["margin"], a["bbox"], a["crop"], a["status"], None)

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc == -1 and msg and b"hmmr_video_bbox" in msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        with pytest.raises(_lib.HmmrError):
            _lib.check(rc, "hmmr_video_bbox")

    for name in ("cams", "kps", "proc", "off", "bbox", "crop", "status"):
        refused(call(**{name: None}), b"null argument")
    for k in (0, -1, _lib.TRACK_MAX_KPS + 1):
        refused(call(k=k, ldk=4096), b"1 <= k <= 64")
    refused(call(ldk=49), b"row strides")
    refused(call(k=1, ldk=1), b"row strides")
    refused(call(ldc=2), b"row strides")
    refused(call(ldc=0), b"row strides")
    for n_tracks in (0, -1):
        refused(call(n_tracks=n_tracks), b"at least one track")
    refused(call(off=[0, 7, 6, 20]), b"not monotone")
    refused(call(off=[-1, 7]), b"negative")
    refused(call(off=[0, _lib.TRACK_MAX_ROWS + 1]), b"rows")
    refused(call(h=0), b"img_h >= 1")
    refused(call(w=0), b"img_w >= 1")
    refused(call(h=-5, w=-5), b"img_h >= 1")
    for size in (0.0, -224.0, float("nan"), float("inf")):
        refused(call(size=size), b"proc_size")
    for margin in (float("nan"), float("inf"), float("-inf")):
        refused(call(margin=margin), b"margin")


def test_visualize_mesh_og_hands_rotated_what_the_reference_does():
    """the camera, angle and image_size that reach renderer.rotated equal the fixture's records of the reference, bit for bit, in both
    branches, with the image below and above max_img_size (a recorder stands where the renderer would: no device)"""
    import os

    import numpy as np

    from conftest import GOLDEN
    from human_dynamics_amd.util.render.nmr_renderer import visualize_mesh_og
    from human_dynamics_amd.util.render.person_view import clip_size

    class Recorder(object):
        class _State(object):
            image_size = 0

        def __init__(self):
            self.renderer, self.seen = self._State(), None

        def rotated(self, verts, deg, cam=None, color_name='blue'):
            self.seen = (np.array(cam), deg, self.renderer.image_size, color_name)
            return "rendered"

    ref = dict(np.load(os.path.join(GOLDEN, "reference_video_bbox.npz")))
    assert len(ref["og_meta"]) == 24 and set(ref["og_meta"][:, 5]) == {0, 90} and set(ref["og_meta"][:, 6]) == {0, 1}
    for m, cam in zip(ref["og_meta"], ref["og_cam"]):
        case, row, h, w, max_img, deg, boxed, size = (int(x) for x in m)
        rec = Recorder()
        out = visualize_mesh_og(ref["cams"][row], np.zeros((4, 3), np.float32), rec, ref["proc"][row, 1:3].astype(int), float(ref["proc"][row, 0]),
                                [224, 224], img=np.zeros((h, w, 3)), deg=deg, mesh_color='pink', max_img_size=max_img,
                                crop_cam=ref["cams_crop"][row] if boxed else None, bbox=ref["bbox"][case] if boxed else None)
        got_cam, got_deg, got_size, color = rec.seen
        assert out == "rendered" and got_deg == deg and got_size == size and color == 'pink', m
        assert got_cam.dtype == np.float32 and np.array_equal(got_cam.view(np.int32), cam.view(np.int32)), m
    assert clip_size([133, 571, 241, 967]) == (180, 300, 300)          # a 438 x 726 window at max_img_size 300
