"""float64 NumPy restatement of the track front end (csrc/track.hip, human_dynamics_amd/util/smooth_bbox.py), without SciPy:
the per-frame box, the extent of a track with np.linspace over its gaps, the zero-padded median, the reflect-boundary Gaussian
and the crop integers.  tests/test_track_oracle.py pins it to tests/golden/reference_tracks.npz, which holds what the reference's
own smooth_bbox.py returned with the real SciPy; it then serves the seeded cases the fixture does not carry (`seeded_cases`).

The seeded cases live here because the fixture's maker checks them too: no floor / round argument of the crop geometry of any
recorded or seeded row lies within 1e-6 of its decision boundary (`rounding_margin`), so no test has to drop a row.
"""
import numpy as np

IMG = 224
TILE = 256          # the gap scan's step (include/hmmr_hip.h: HMMR_TRACK_TILE)


# ---- smooth_bbox.py
def kp_to_bbox_param(kp, vis_thresh):
    if kp is None:
        return None
    kp = np.asarray(kp, np.float64)
    vis = kp[:, 2] > vis_thresh
    if not vis.any():
        return None
    lo, hi = kp[vis, :2].min(axis=0), kp[vis, :2].max(axis=0)
    d = hi - lo
    height = np.sqrt(d[0] * d[0] + d[1] * d[1])
    if height < 0.5:
        return None
    return np.array([(lo[0] + hi[0]) / 2., (lo[1] + hi[1]) / 2., 150. / height])


def get_all_bbox_params(kps, vis_thresh=2):
    boxes = [kp_to_bbox_param(kp, vis_thresh) for kp in kps]
    valid = [i for i, b in enumerate(boxes) if b is not None]
    if not valid:
        return np.zeros((0, 3)), -1, 0
    start, end = valid[0], valid[-1] + 1
    rows = np.zeros((end - start, 3))
    for p, q in zip(valid[:-1], valid[1:]):
        step = (boxes[q] - boxes[p]) / float(q - p)
        for i in range(p + 1, q):
            rows[i - start] = float(i - p) * step + boxes[p]          # np.linspace: arange * step + start
    for i in valid:
        rows[i - start] = boxes[i]
    return rows, start, end


def gaussian_weights(sigma, truncate=4.0):
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return w / w.sum(), radius


def medfilt_zero(x, kernel_size):
    x = np.asarray(x, np.float64)
    half = kernel_size // 2
    padded = np.concatenate([np.zeros(half), x, np.zeros(half)])
    return np.array([np.sort(padded[i:i + kernel_size])[half] for i in range(len(x))]).reshape(len(x))


def reflect_index(j, n):
    m = np.mod(j, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def gaussian_reflect(x, sigma):
    x = np.asarray(x, np.float64)
    n = len(x)
    if n == 0:
        return x.copy()
    w, r = gaussian_weights(sigma)
    i = np.arange(n)
    out = x * w[r]
    for j in range(-r, 0):                                         # correlate1d's symmetric branch, in its order
        out = out + (x[reflect_index(i + j, n)] + x[reflect_index(i - j, n)]) * w[r + j]
    return out


def smooth_bbox_params(bbox_params, kernel_size=11, sigma=8):
    p = np.asarray(bbox_params, np.float64).reshape(-1, 3)
    return np.stack([gaussian_reflect(medfilt_zero(p[:, a], kernel_size), sigma) for a in range(3)], axis=1)


def get_smooth_bbox_params(kps, vis_thresh=2, kernel_size=11, sigma=3):
    rows, start, end = get_all_bbox_params(kps, vis_thresh)
    if start < 0:
        raise ValueError("no frame of the track has a box")
    return np.vstack([np.zeros((start, 3)), smooth_bbox_params(rows, kernel_size, sigma)]), start, end


# ---- the crop integers (evaluation/run_video.crop_geometry) with the status word of hmmr_track_crop_geom
EMPTY, BEFORE_ORIGIN, CLIPPED, NOT_FINITE = 1, 2, 4, 8


def crop_geometry(h, w, bbox):
    """(status, geom [4], info [5]) of one row; a bad row has the identity geometry and a zero info."""
    cx, cy, scale = (float(v) for v in bbox)
    fh, fw = np.floor(h * scale), np.floor(w * scale)
    bad = lambda st: (st, np.array([h, w, 0, 0], np.int32), np.zeros(5))
    if not (abs(fh) < 1e9 and abs(fw) < 1e9):
        return bad(NOT_FINITE)
    if fh < 1 or fw < 1:
        return bad(EMPTY)
    rx, ry = np.round(cx * (fh / float(h))), np.round(cy * (fw / float(w)))
    if not (abs(rx) < 1e9 and abs(ry) < 1e9):
        return bad(NOT_FINITE)
    csx, csy = int(rx) + IMG, int(ry) + IMG
    sx, sy = csx - IMG // 2, csy - IMG // 2
    st = (BEFORE_ORIGIN if sx < 0 or sy < 0 else 0) | (CLIPPED if csx + IMG // 2 > fw + 2 * IMG or csy + IMG // 2 > fh + 2 * IMG else 0)
    if st:
        return bad(st)
    return 0, np.array([fh, fw, sx - IMG, sy - IMG], np.int32), np.array([sx, sy, csx - sx, csy - sy, scale], np.float64)


def rounding_margin(h, w, bbox):
    """Distance of the nearest floor / round argument of crop_geometry from its decision boundary.  A box of exact zeros (what a
    track of fewer than six rows smooths to: a median of mostly padding) is exempt: its products are exactly zero in any
    summation order."""
    cx, cy, scale = (float(v) for v in bbox)
    if cx == 0. and cy == 0. and scale == 0.:
        return np.inf
    to_int = lambda v: abs(v - np.round(v))
    to_half = lambda v: abs((v - 0.5) - np.round(v - 0.5))
    fh, fw = np.floor(h * scale), np.floor(w * scale)
    return min(to_int(h * scale), to_int(w * scale), to_half(cx * (fh / float(h))), to_half(cy * (fw / float(w))))


# ---- seeded synthetic tracks
def make_track(rng, n, k, h, w, holes=(), invisible=(), tiny=(), vis_thresh=0.1, centre=None):
    """n frames of a person wandering inside an h x w frame: k keypoints (x, y, score) on a binary grid, so that a fixture
    holding them compresses.  holes: frames that are None; invisible: present, every score <= vis_thresh; tiny: present
    and visible but less than half a pixel tall."""
    t = np.arange(n)
    size = min(h, w) * (0.30 + 0.08 * np.sin(t / 9. + rng.uniform(0, 6)))
    c = np.array([w, h]) * 0.5 if centre is None else np.asarray(centre, np.float64)
    cx = c[0] + w * 0.15 * np.sin(t / 17. + rng.uniform(0, 6)) + rng.normal(0, 1.5, n)
    cy = c[1] + h * 0.10 * np.cos(t / 23. + rng.uniform(0, 6)) + rng.normal(0, 1.5, n)
    out = []
    for i in range(n):
        if i in holes:
            out.append(None)
            continue
        kp = np.empty((k, 3))
        kp[:, 0] = cx[i] + rng.uniform(-0.25, 0.25, k) * size[i]
        kp[:, 1] = cy[i] + rng.uniform(-0.5, 0.5, k) * size[i]
        kp[:, 2] = rng.uniform(0.15, 1.0, k)
        kp[rng.uniform(size=k) < 0.2, 2] = rng.uniform(0.0, 0.09)        # some keypoints below the threshold
        kp[:, :2] = np.round(kp[:, :2] * 16.) / 16.                      # sixteenths of a pixel, scores in 256ths
        kp[:, 2] = np.round(kp[:, 2] * 256.) / 256.
        if i in invisible:
            kp[:, 2] = np.minimum(kp[:, 2], vis_thresh) * rng.choice([1.0, 0.5], k)
            kp[0, 2] = vis_thresh                                        # equal to the threshold: not visible
        elif i in tiny:
            kp[:, :2] = kp[0, :2] + rng.integers(0, 4, (k, 2)) / 16.
            kp[:, 2] = 0.875
        elif k > 1:
            kp[:2, 2] = 0.875                                            # an ordinary frame has at least two visible keypoints
        out.append(kp)
    return out


VIS_THRESH = 0.1
LENGTHS = (1, 2, 5, 6, 10, 11, 12, 13, 24, 25, 26, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def seeded_cases():
    """name -> (h, w, [track, ...]): the cases the GPU tests run against this oracle.  Deterministic."""
    rng = np.random.default_rng(20240607)
    cases = {}
    cases["lengths"] = (96, 128, [make_track(rng, n, 17, 96, 128) for n in LENGTHS])
    n = 2 * TILE + 1
    gaps = set(range(0, 3)) | {40} | {60, 61} | set(range(100, 115)) | set(range(TILE - 6, TILE + 7)) | set(range(n - 8, n))
    cases["gaps"] = (270, 480, [make_track(rng, n, 25, 270, 480, holes=gaps, invisible={130, 131, 200}, tiny={150, 300})])
    cases["tile_edges"] = (96, 128, [make_track(rng, TILE + 1, 17, 96, 128, holes={TILE - 1}),            # p in tile 0, q in tile 1
                                     make_track(rng, 2 * TILE, 17, 96, 128, holes=set(range(1, 2 * TILE - 1))),   # a gap over two whole tiles
                                     make_track(rng, TILE + 2, 17, 96, 128, holes={TILE})])
    cases["k25"] = (270, 480, [make_track(rng, 48, 25, 270, 480, holes={0, 1, 10, 20, 21, 46, 47}, invisible={5, 45}, tiny={30})])
    cases["k1"] = (96, 128, [make_track(rng, 12, 1, 96, 128)])                                             # one keypoint: never valid
    cases["mixed"] = (270, 480, [make_track(rng, 1, 17, 270, 480), make_track(rng, 13, 17, 270, 480, holes={4}),
                                 make_track(rng, 9, 17, 270, 480, holes=set(range(9))),                   # no valid frame, in the middle
                                 make_track(rng, 257, 17, 270, 480, holes={0, 100, 256}, invisible={7}), make_track(rng, 6, 17, 270, 480)])
    far = make_track(rng, 40, 17, 96, 128, centre=(128 + 400, 96 + 300))                                  # far outside the frame
    for i in range(20, 40):                                                                               # ... and back inside
        far[i] = make_track(rng, 1, 17, 96, 128)[0]
    cases["bad_rows"] = (96, 128, [make_track(rng, 30, 17, 96, 128, holes={3}), far, make_track(rng, 26, 17, 96, 128)])
    return cases


def case_margin(h, w, tracks, vis_thresh=VIS_THRESH):
    """the smallest rounding_margin over every smoothed row of the case"""
    worst = np.inf
    for trk in tracks:
        rows, start, end = get_all_bbox_params(trk, vis_thresh)
        if start < 0:
            continue
        sm = smooth_bbox_params(rows, 11, 3)
        worst = min([worst] + [rounding_margin(h, w, b) for b in sm])
    return worst
