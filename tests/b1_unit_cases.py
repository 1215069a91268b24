"""Grids, seeded operands, the float64 reference and the float32 emulation of the whole-unit kernel of block 1 (csrc/b1_unit.hip:
conv2 3x3 + conv3 + add + the next unit's preact + conv1 in one launch; tests/test_b1_unit_cases.py on the host,
tests/test_gpu_b1_unit_kernel.py and tests/test_gpu_b1_unit.py on the device).  No GPU is needed by anything in here.

Both references take the operands AS STORED: activations as packing.to_split rounds them (_split_round: fp16 hi + fp16 lo, clamped to the
fp16 range), filters as the packers round them (_split_round_w: every output channel scaled by its power of two, split, unscaled).

    reference()     float64: h2 = relu(bn2(conv2(h1))), trunk = conv3({h2 [, xp]}) + bias [+ res]
    reference_h1()  float64: h1' = [relu](bn1(conv1(relu(pre(trunk))))) of a GIVEN trunk -- the device tests pass the trunk the kernel stored,
                    so the error of h1' is that of the second half of the chain alone (as _float64 of tests/test_gpu_unit_pair.py)
    emulate()       float32 arithmetic with the kernel's rounding points: h2, the trunk, the pre-activation and h1' are split-rounded

The bound of every comparison with float64 is TOL max(1, max |ref|), TOL = 2e-5: that of every split kernel's test."""
import functools
import zlib

import numpy as np

from test_gpu_f16x3 import _split_round, _split_round_w

TOL = 2e-5
SPLIT_MAX = 65504.0
FORMS = ("identity", "folded")              # the shortcut as a tensor (RES) / folded into conv3's K (KC3B = 4)

# (n, H, W): what each grid exercises is said in tests/test_gpu_b1_unit_kernel.py
GRIDS = ((1, 1, 1), (129, 1, 1), (5, 1, 56), (3, 56, 1), (7, 3, 5), (1, 3, 11), (1, 4, 8), (4, 8, 4), (2, 16, 40), (2, 40, 16),
         (1, 56, 55), (1, 55, 56), (1, 8, 8), (5, 24, 24), (3, 56, 56))
TILE_GRID = (8, 16)                         # one 128-pixel tile per image
TILE_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17)
KNOWN_GRIDS = ((3, 5, 7), (1, 56, 56), (2, 9, 4))          # the last: H > W
FLAG_GRID = (6, 5, 7)
NAN_GRIDS = ((6, 5, 7), (2, 56, 56))
NAN_CHANNEL = 5


def grid_id(g):
    return "%dx%dx%d" % g


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def filters(form):
    """one filter set per form, scaled as _unit_inputs of tests/test_gpu_b1_unit.py scales them; nobody writes to it"""
    rng, f32 = _rng("b1 unit filters/" + form), np.float32
    f = {"w2": (rng.normal(size=(3, 3, 64, 64)) * 0.06).astype(f32),
         "bn2": (rng.uniform(0.5, 1.5, 64).astype(f32), (rng.normal(size=64) * 0.3).astype(f32)),
         "w3": (rng.normal(size=(1, 1, 64, 256)) * 0.12).astype(f32), "b3": (rng.normal(size=256) * 0.2).astype(f32),
         "pre": (rng.uniform(0.5, 1.5, 256).astype(f32), (rng.normal(size=256) * 0.3).astype(f32)),
         "w1": (rng.normal(size=(1, 1, 256, 64)) * 0.06).astype(f32),
         "bn1": (rng.uniform(0.5, 1.5, 64).astype(f32), (rng.normal(size=64) * 0.3).astype(f32))}
    if form == "folded":
        f["wsc"] = (rng.normal(size=(1, 1, 64, 256)) * 0.12).astype(f32)
        f["bsc"] = (rng.normal(size=256) * 0.2).astype(f32)
    return f


@functools.lru_cache(maxsize=None)
def operands(grid, form, name=""):
    """a ReLU'd normal h1 [n,h,w,64] (x 2) and xp [n,h,w,64], a normal res [n,h,w,256] (x 1.5): float32; nobody writes to them"""
    n, h, w = grid
    rng, f32 = _rng("b1 unit operands/%s/%s/%s" % (grid_id(grid), form, name)), np.float32
    d = {"h1": np.maximum(rng.normal(size=(n, h, w, 64)), 0).astype(f32) * 2.0}
    if form == "folded":
        d["xp"] = np.maximum(rng.normal(size=(n, h, w, 64)), 0).astype(f32)
    else:
        d["res"] = (rng.normal(size=(n, h, w, 256)) * 1.5).astype(f32)
    return d


def with_filters(f, **kw):
    g = dict(f)
    g.update(kw)
    return g


# ---- the saturation cases (FLAG_GRID): each pushes ONE stored tensor of the chain beyond the fp16 range in some elements, fewer than half
def saturating_trunk(form):
    """(filters, operands): the shortcut x 3e4 (kept inside the fp16 range itself) and h1 x 3e3 -- the sum leaves the range"""
    d = operands(FLAG_GRID, form)
    big = {"h1": d["h1"] * np.float32(3e3)}
    for k in ("xp", "res"):
        if k in d:
            big[k] = np.clip(d[k] * np.float32(3e4), -6e4, 6e4).astype(np.float32)
    return filters(form), big


def saturating_h1(form, lower=False):
    """(filters, operands, relu1): bn1's scale x 3e4 on a normal trunk (the upper clamp); lower: relu1 = 0, scale x 1e3 and shift - 6.4e4"""
    f = filters(form)
    s, b = f["bn1"]
    bn1 = (s * np.float32(1e3), b - np.float32(6.4e4)) if lower else (s * np.float32(3e4), b)
    return with_filters(f, bn1=bn1), operands(FLAG_GRID, form), not lower


def saturating_h2(form):
    """(filters, operands): bn2's scale x 2e4"""
    f = filters(form)
    return with_filters(f, bn2=(f["bn2"][0] * np.float32(2e4), f["bn2"][1])), operands(FLAG_GRID, form)


def beyond_range(x):
    """(elements beyond the fp16 range, elements)"""
    return int((np.abs(x) > SPLIT_MAX).sum()), x.size


# ---- the NaN cases
def poisoned_pixels(grid):
    """pixel 0 and pixel M - 1 (the two the patch clamp re-reads for rows outside the tensor) and the top right corner of the middle image"""
    n, h, w = grid
    return (0, n * h * w - 1, (n // 2) * h * w + w - 1)


def poisoned(grid, form):
    d = dict(operands(grid, form))
    d["h1"] = d["h1"].copy()
    d["h1"].reshape(-1, 64)[list(poisoned_pixels(grid)), NAN_CHANNEL] = np.nan
    return d


def poisoned_neighbourhood(grid):
    """bool [M]: the pixels whose in-image 3 x 3 neighbourhood holds a poisoned pixel"""
    n, h, w = grid
    mask = np.zeros((n, h, w), bool)
    for p in poisoned_pixels(grid):
        i, y, x = p // (h * w), (p % (h * w)) // w, p % w
        mask[i, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    return mask.reshape(-1)


# ---- exact known answers: one-hot conv2 taps, power-of-two selections behind them
KNOWN_SCALES = (1.0, 2.0, 0.5, 0.25)        # trunk channel c selects h2 channel c % 64 times KNOWN_SCALES[c // 64]


@functools.lru_cache(maxsize=None)
def known_filters(ky, kx, form):
    """w2 = the identity of the 64 channels at tap (ky, kx) and zero elsewhere; bn2, pre and bn1 = (1, 0); no bias; w3 selects channel
    c % 64 with a power of two; wsc selects xp's channel c % 64; w1 selects trunk channel j"""
    f32, eye = np.float32, np.eye(64, dtype=np.float32)
    w2 = np.zeros((3, 3, 64, 64), f32)
    w2[ky, kx] = eye
    one = lambda c: (np.ones(c, f32), np.zeros(c, f32))
    f = {"w2": w2, "bn2": one(64), "w3": np.concatenate([eye * f32(s) for s in KNOWN_SCALES], axis=1)[None, None], "b3": None, "pre": one(256),
         "w1": np.concatenate([eye, np.zeros((192, 64), f32)], axis=0)[None, None], "bn1": one(64)}
    if form == "folded":
        f["wsc"], f["bsc"] = np.concatenate([eye] * 4, axis=1)[None, None], None
    return f


@functools.lru_cache(maxsize=None)
def known_operands(grid, form):
    """small integers: h1 = 1 + (64 pixel + channel) mod 16381 (a prime: two pixels of a tensor never agree in a channel), xp = (64 pixel +
    channel) mod 1021, res = (256 pixel + channel) mod 2041 - 1020"""
    n, h, w = grid
    m = n * h * w
    px = np.arange(m, dtype=np.int64)[:, None]
    d = {"h1": (1 + (64 * px + np.arange(64)) % 16381).astype(np.float32).reshape(n, h, w, 64)}
    if form == "folded":
        d["xp"] = ((64 * px + np.arange(64)) % 1021).astype(np.float32).reshape(n, h, w, 64)
    else:
        d["res"] = ((256 * px + np.arange(256)) % 2041 - 1020).astype(np.float32).reshape(n, h, w, 256)
    return d


def known_expected(grid, form, ky, kx):
    """(trunk [n,h,w,256], h1' [n,h,w,64]) float64 by INDEXING, no arithmetic but the selections' powers of two and the shortcut's sum:
    trunk[y, x, c] = s(c) h1[y + ky - 1, x + kx - 1, c % 64] (0 outside the image) + shortcut; h1' = relu(trunk[..., :64])"""
    n, h, w = grid
    d = known_operands(grid, form)
    x = np.pad(d["h1"].astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))[:, ky:ky + h, kx:kx + w, :]
    trunk = np.concatenate([x * s for s in KNOWN_SCALES], axis=-1)
    trunk = trunk + (np.tile(d["xp"].astype(np.float64), 4) if form == "folded" else d["res"].astype(np.float64))
    return trunk, np.maximum(trunk[..., :64], 0)


# ---- what hmmr_b1_unit_split refuses: (name, the form it is built from, fields to set on a good descriptor, words of the message).  A field
# value PTR stands for some non-null pointer (never dereferenced: every check runs in front of the launch), a callable takes the good value
PTR = "some non-null pointer"
_NEEDS, _SHAPE = "needs h1, the unit's filter stream", "whole images at most 56 pixels wide"
REFUSALS = (
    ("h2 beside h1", "identity", {"h2": PTR}, _NEEDS),
    ("no out", "identity", {"out": None}, _NEEDS),
    ("no out_h1", "folded", {"out_h1": None}, _NEEDS),
    ("no pre_scale", "identity", {"pre_scale": None}, _NEEDS),
    ("no pre_shift", "folded", {"pre_shift": None}, _NEEDS),
    ("no scale1", "folded", {"scale1": None}, _NEEDS),
    ("no shift1", "identity", {"shift1": None}, _NEEDS),
    ("no scale2", "identity", {"scale2": None}, _NEEDS),
    ("no shift2", "folded", {"shift2": None}, _NEEDS),
    ("out_pre set", "identity", {"out_pre": PTR}, _NEEDS),
    ("res_strided", "identity", {"res_strided": 1}, _NEEDS),
    ("conv2_stride 2", "folded", {"conv2_stride": 2}, _NEEDS),
    ("m 0", "identity", {"m": 0}, _NEEDS),
    ("c_mid 128", "identity", {"c_mid": 128}, _SHAPE),
    ("depth 512", "folded", {"depth": 512}, _SHAPE),
    ("n2 128", "identity", {"n2": 128}, _SHAPE),
    ("win 57", "identity", {"win": 57}, _SHAPE),
    ("win 0", "folded", {"win": 0}, _SHAPE),
    ("hin 0", "identity", {"hin": 0}, _SHAPE),
    ("m not whole images", "folded", {"m": lambda m: m - 1}, _SHAPE),
    ("res and xp", "identity", {"xp": PTR, "c_xp": 64}, "either a shortcut tensor"),
    ("neither res nor xp", "identity", {"res": None}, "null argument"),
    ("neither xp nor res", "folded", {"xp": None}, "null argument"),
    ("c_xp 32", "folded", {"c_xp": 32}, "a folded shortcut has 64 input channels"),
    ("ldr 255", "identity", {"ldr": 255}, "residual row stride < depth"),
)


def apply_refusal(t, fields, ptr):
    """set `fields` on the descriptor t (PTR -> ptr)"""
    for k, v in fields.items():
        setattr(t, k, ptr if v is PTR else v(getattr(t, k)) if callable(v) else v)


# ---------------------------------------------------------------------------------------------------------------- references
def stored(f, d):
    """operands and filters as the device holds them, float64"""
    s = {k: _split_round(v) for k, v in d.items()}
    w3 = f["w3"] if "wsc" not in f else np.concatenate([f["w3"], f["wsc"]], axis=2)          # one row_pow2 per row of [W3 | Wsc]
    s["w2"], s["w3"], s["w1"] = _split_round_w(f["w2"]), _split_round_w(w3)[0, 0], _split_round_w(f["w1"])[0, 0]
    b = [np.asarray(f[k], np.float64) for k in ("b3", "bsc") if f.get(k) is not None]
    s["bias"] = np.float32(sum(b)).astype(np.float64) if b else None                         # (the wrapper sums in float64, stores float32)
    return s


def _conv3x3(x, w):
    n, h, w_, _ = x.shape
    xp_ = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return sum(xp_[:, ky:ky + h, kx:kx + w_, :] @ w[ky, kx] for ky in range(3) for kx in range(3))


def reference(f, d, bias=True):
    """float64 (h2 [M,64], trunk [M,256]); bias = False: without shift3"""
    s = stored(f, d)
    h2 = np.maximum(_conv3x3(s["h1"], s["w2"]) * f["bn2"][0].astype(np.float64) + f["bn2"][1].astype(np.float64), 0).reshape(-1, 64)
    k = h2 if "xp" not in s else np.concatenate([h2, s["xp"].reshape(-1, 64)], axis=1)
    trunk = k @ s["w3"]
    if bias and s["bias"] is not None:
        trunk = trunk + s["bias"]
    if "res" in s:
        trunk = trunk + s["res"].reshape(-1, 256)
    return h2, trunk


def reference_h1(f, trunk, relu1=True):
    """float64 h1' [M,64] of a trunk [M,256] as stored; the pre-activation stays unrounded"""
    w1 = _split_round_w(f["w1"])[0, 0]
    pre = np.maximum(np.asarray(trunk, np.float64) * f["pre"][0].astype(np.float64) + f["pre"][1].astype(np.float64), 0)
    h = pre @ w1 * f["bn1"][0].astype(np.float64) + f["bn1"][1].astype(np.float64)
    return np.maximum(h, 0) if relu1 else h


def emulate(f, d, relu1=True, bias=True):
    """(trunk [M,256], h1' [M,64]) as float64 values of a float32 chain with the kernel's rounding points: float32 products and sums of
    the stored operands, one float32 rounding of acc * scale + shift, and h2, the trunk, the pre-activation and h1' clamped and split"""
    s, f32, f64 = stored(f, d), np.float32, np.float64
    fma = lambda a, sc, sh: (a.astype(f64) * np.asarray(sc, f64) + np.asarray(sh, f64)).astype(f32)
    rnd = lambda v, lo: _split_round(np.clip(v, lo, SPLIT_MAX)).astype(f32)                   # (22 bits: exact in float32)
    h2 = rnd(fma(_conv3x3(s["h1"].astype(f32), s["w2"].astype(f32)), f["bn2"][0], f["bn2"][1]), 0.0).reshape(-1, 64)
    k = h2 if "xp" not in s else np.concatenate([h2, s["xp"].astype(f32).reshape(-1, 64)], axis=1)
    t = fma(k @ s["w3"].astype(f32), 1.0, s["bias"] if bias and s["bias"] is not None else 0.0)
    if "res" in s:
        t = t + s["res"].astype(f32).reshape(-1, 256)
    trunk = rnd(t, -SPLIT_MAX)
    pre = rnd(fma(trunk, f["pre"][0], f["pre"][1]), 0.0)
    h = fma(pre @ s["w1"].astype(f32), f["bn1"][0], f["bn1"][1])
    return trunk.astype(f64), rnd(h, 0.0 if relu1 else -SPLIT_MAX).astype(f64)


def errors(trunk, h1, f, d, relu1=True, bias=True):
    """((max |err|, max |ref|) of the trunk, ... of h1') of stored outputs [M,256] / [M,64] (float64 values) against the float64 reference"""
    ref_t = reference(f, d, bias)[1]
    ref_h = reference_h1(f, trunk, relu1)
    return (float(np.abs(trunk - ref_t).max()), float(np.abs(ref_t).max())), (float(np.abs(h1 - ref_h).max()), float(np.abs(ref_h).max()))


def inside(e):
    """the bound of every split kernel's test"""
    return e[0] < TOL * max(1.0, e[1])
