"""Golden vectors for the person-centred view, produced by EXECUTING the reference's own two functions (the reference tree is
not part of this repository, so the outputs are committed as a fixture):

  reference_video_bbox.npz   src/util/render/nmr_renderer.py `compute_video_bbox` (:519-634) on nine tracks, and
                             `visualize_mesh_og` (:422-488) in both branches, with stand-ins for what cannot be installed:
                             neural_renderer, skimage.io (imread returns zeros of the case's frame size), cv2.resize (only its
                             output SHAPE matters), and an `ipdb` whose set_trace records the frame index and returns, so that
                             the reference runs on past its 'crop is more than start pt..?' breakpoint (:613-615) and what it
                             computes there is pinned.  `renderer.rotated` is replaced by a recorder of its arguments.

Inputs are drawn as float32 (what the device holds); the reference gets float64 copies, so that NumPy's scalar promotion
rules cannot change a result.  The maker asserts what the tests rely on (conditions on the inputs, not tolerances) and draws
again until they hold: every extreme, before `astype(np.int)` truncates it, is a clamp value or lies at least 1e-6 from an
integer (read from a second run of the reference in which np.int is float64), and the box's longer side is at least 16.

    python tests/golden/make_video_bbox_golden.py <path of the reference tree>      (or HMMR_REFERENCE=<path>)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HMMR_REFERENCE", "")
PROC = 224
K = 25

# (frame h, w), frames, margin, scale range, the person's centre in the frame as fractions (x, y), drift in pixels over the track
CASES = [
    ((240, 320), 1, 0, (1.6, 2.5), (0.50, 0.50), 0),          # a small person in the middle: no clamp, no trap (scale > 1)
    ((240, 320), 7, 10, (0.9, 1.2), (0.08, 0.50), 6),         # at the left edge: xmin clamps to 0
    ((240, 320), 40, 25, (0.9, 1.3), (0.60, 0.12), 20),       # at the top: ymin clamps to 0
    ((720, 1280), 1, 25, (0.4, 0.5), (0.75, 0.60), 0),        # far from the origin at a small scale: the trap
    ((720, 1280), 7, 10, (0.44, 0.47), (0.55, 0.55), 40),     # at the trap's threshold: some of the seven frames meet it
    ((720, 1280), 40, 0, (0.5, 0.7), (0.93, 0.55), 60),       # at the right edge: xmax clamps to w - 1
    ((1080, 810), 1, 10, (0.4, 0.45), (0.50, 0.88), 0),       # at the bottom: ymax clamps to h - 1
    ((1080, 810), 7, 0, (1.2, 2.0), (0.20, 0.15), 10),        # near the origin, enlarged: no trap
    ((1080, 810), 40, 25, (0.6, 1.0), (0.55, 0.45), 80),      # a walk through the middle
]


def load_reference():
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit("give the path of the reference tree (the directory that holds src/)")
    if not hasattr(np, "int"):
        np.int = int
    state = {"frame_hw": (0, 0), "trap": []}
    nr = types.ModuleType("neural_renderer")
    skio = types.ModuleType("skimage.io")
    skio.imread = lambda p: np.zeros(state["frame_hw"] + (3,), np.uint8)
    sk = types.ModuleType("skimage"); sk.io = skio
    cv2 = types.ModuleType("cv2")
    cv2.resize = lambda img, dsize: np.zeros((dsize[1], dsize[0]) + img.shape[2:], img.dtype)
    ipdb = types.ModuleType("ipdb")
    ipdb.set_trace = lambda: state["trap"].append(int(sys._getframe(1).f_locals["i"]))
    for n, m in (("neural_renderer", nr), ("skimage", sk), ("skimage.io", skio), ("cv2", cv2), ("ipdb", ipdb)):
        sys.modules[n] = m
    sys.path.insert(0, REF)
    try:
        from src.util.render import nmr_renderer as R
    finally:
        sys.path.remove(REF)
    return R, state


def draw_track(rng, hw, n, scales, centre, drift):
    h, w = hw
    cams = np.stack([rng.uniform(0.5, 1.2, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1).astype(np.float32)
    kps = rng.uniform(-0.85, 0.85, (n, K, 2)).astype(np.float32)
    base = rng.uniform(*scales)
    scale = np.clip(base * rng.uniform(0.97, 1.03, n), 0.4, 2.5)
    step = np.linspace(0, 1, n) if n > 1 else np.zeros(1)
    c = np.stack([centre[0] * w + drift * step, centre[1] * h + 0.3 * drift * step], 1) + rng.normal(0, 1.5, (n, 2))
    start = np.round(c * scale[:, None]) + PROC - PROC // 2           # process_image: the crop's origin in the padded, scaled image
    return cams, kps, np.concatenate([scale[:, None], start], 1).astype(np.float64)


def run_reference(R, state, hw, cams, kps, proc, margin):
    state["frame_hw"] = hw
    infos = [{"im_path": "frame.png", "im_shape": [PROC, PROC], "scale": float(p[0]), "start_pt": p[1:3].astype(np.int64)} for p in proc]
    c64, k64 = [c.astype(np.float64) for c in cams], [k.astype(np.float64) for k in kps]
    _stdout, sys.stdout = sys.stdout, open(os.devnull, "w")             # ('crop is more than start pt..?' per trapped frame)
    keep = np.int
    try:
        np.int = np.float64                                             # the extremes before truncation, from the reference itself
        raw, _ = R.compute_video_bbox(c64, k64, infos, margin=margin)
        np.int = keep
        state["trap"] = []
        bbox, new = R.compute_video_bbox(c64, k64, infos, margin=margin)
    finally:
        np.int = keep
        sys.stdout.close()
        sys.stdout = _stdout
    new = np.stack(new)
    assert new.dtype == np.float32 and bbox.dtype.kind == "i"
    return np.asarray(raw, np.float64), bbox, new, sorted(state["trap"])


def acceptable(raw, bbox, hw):
    clamps = ({0.}, {float(hw[0] - 1)}, {0.}, {float(hw[1] - 1)})
    for v, cl in zip(raw, clamps):
        if v not in cl and abs(v - np.rint(v)) < 1e-6:
            return False
    return max(bbox[1] - bbox[0], bbox[3] - bbox[2]) >= 16


class Recorder(object):
    """stands where a VisRenderer would: keeps what reaches `rotated`"""

    class _State(object):
        image_size = 0

    def __init__(self):
        self.renderer, self.seen = self._State(), None

    def rotated(self, verts, deg, cam=None, color_name='blue'):
        self.seen = (np.array(cam), deg, int(self.renderer.image_size))


def main():
    R, state = load_reference()
    rng = np.random.default_rng(23)
    out, offsets, clamp_hits, trapped, free = {}, [0], np.zeros(4, bool), 0, 0
    cams_all, kps_all, proc_all, crop_all, trap_all, bboxes, raws, meta = [], [], [], [], [], [], [], []
    for hw, n, margin, scales, centre, drift in CASES:
        for _ in range(100):
            cams, kps, proc = draw_track(rng, hw, n, scales, centre, drift)
            raw, bbox, new, trap = run_reference(R, state, hw, cams, kps, proc, margin)
            if acceptable(raw, bbox, hw):
                break
        else:
            raise AssertionError("no acceptable draw for %s" % ((hw, n, margin),))
        clamp_hits |= np.array([raw[0] == 0, raw[1] == hw[0] - 1, raw[2] == 0, raw[3] == hw[1] - 1])
        trapped += bool(trap)
        free += not trap
        t = np.zeros(n, bool)
        t[trap] = True
        cams_all.append(cams); kps_all.append(kps); proc_all.append(proc); crop_all.append(new); trap_all.append(t)
        bboxes.append(bbox); raws.append(raw); meta.append([hw[0], hw[1], margin])
        offsets.append(offsets[-1] + n)
        print("%4dx%-4d n=%2d margin=%2d  bbox %s  S=%d  trap frames %d" % (hw[0], hw[1], n, margin, bbox, max(bbox[1] - bbox[0], bbox[3] - bbox[2]),
                                                                            len(trap)))
    assert clamp_hits.all(), "every clamp must bind in some case: %s" % clamp_hits
    assert trapped >= 2 and free >= 2, (trapped, free)
    out.update(cams=np.concatenate(cams_all), kps=np.concatenate(kps_all), proc=np.concatenate(proc_all), offsets=np.array(offsets, np.int32),
               meta=np.array(meta, np.int32), bbox=np.stack(bboxes).astype(np.int32), bbox_raw=np.stack(raws),
               cams_crop=np.concatenate(crop_all), trap=np.concatenate(trap_all))

    # ---- visualize_mesh_og: what reaches renderer.rotated, in both branches, below and above max_img_size, at 0 and 90 degrees
    vert = np.zeros((4, 3), np.float32)
    og = []
    for case in (1, 4, 8):                                              # boxes of 240x320, 720x1280 and 1080x810 tracks
        a = offsets[case]
        hw = tuple(int(x) for x in meta[case][:2])
        bbox = bboxes[case]
        for max_img in (300, 2000):                                      # the window (or frame) is above / below it
            for deg in (0, 90):
                for boxed in (False, True):
                    rec = Recorder()
                    cam = cams_all[case][0]
                    scale, start = float(proc_all[case][0, 0]), proc_all[case][0, 1:3].astype(np.int64)
                    R.visualize_mesh_og(cam.astype(np.float64), vert, rec, start, scale, [PROC, PROC], img=np.zeros(hw + (3,)), deg=deg,
                                        max_img_size=max_img, crop_cam=crop_all[case][0] if boxed else None, bbox=bbox if boxed else None)
                    got_cam, got_deg, size = rec.seen
                    assert got_cam.dtype == np.float32
                    og.append(([case, a, hw[0], hw[1], max_img, deg, int(boxed), size], got_cam))
    sizes = sorted(set((r[0][6], r[0][7]) for r in og))
    print("visualize_mesh_og (boxed, image_size):", sizes)
    out.update(og_meta=np.array([r[0] for r in og], np.int32), og_cam=np.stack([r[1] for r in og]))
    path = os.path.join(HERE, "reference_video_bbox.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
