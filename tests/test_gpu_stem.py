"""The ResNet stem ALONE (engine.stem / engine.StemCall -> hmmr_resnet50_stem: the launches hmmr_resnet50_fwd starts with), in its three
modes (fp32, bf16, f16x3) and on both routes (csrc/stem.hip's fused kernels; stem_repack* + hmmr_conv_gemm + maxpool_bn_relu_kernel of
csrc/resnet.hip), looked at where it can go wrong: every element of `pooled` [n + n_zero, 56, 56, 64] (7x7/2 conv + bias -> 3x3/2 TF-SAME
max pool -> preact BN + ReLU of block1/unit_1) and of `h1` (that unit's conv1 + BN + ReLU, where the fused kernel computes it).

    a  an exact known answer: one-hot filters on integer images, equal to a pure index computation, no tolerance
    b  float64 on the operands as stored, element by element, inside a forward error bound carried beside the reference
    c  the two routes, and the stem's conv1 against its own launch, bit for bit on the tensors; the launch counters
    d  batch behaviour: position, the zero tail, NULL images, sentinel / guard rows / NaN guard, determinism
    e  run flags of the split mode: one bad pixel
    f  a refused call queues nothing (the refusals themselves: tests/test_abi.py, no GPU)

The geometry is fixed (224 x 224), so the small cases are batch sizes: (n, n_zero) = (1, 0), (3, 0), (2, 1), (0, 2).

THE ERROR BOUND OF b.  Reference: conv (stride 2, pad 3) + bias, the -inf-padded pool, the folded BN (as oracle._fold_bn32) + ReLU, conv1 +
BN + ReLU, in float64 on the image and the filters AS THE MODE STORES THEM (oracle.quantize; filters with weight=True).  With u = 2^-24,
S = sum |x| |w| over a pixel's taps, P = 1 (fp32, bf16) or 3 (f16x3: three partial products per product), r the relative rounding of a
store: the unit roundoff 2^-p of a format with p significand bits, round to nearest -- 2^-24 fp32, 2^-22 for the fp16 pair, 2^-8 for bf16
(8 bits: a value at the bottom of its binade is moved by up to half a unit in the last place, 2^-8 of it; 0.06708835 -> 0.06689453 is
a correct rounding and 2.9e-3 of the value):

  conv + bias   A = 224 P u (S + |b|)                  fp32 accumulation.  The kernels add 7 taps x 32 = 224 products per pixel, of which 147
                                                       are not zero (their partial sums are <= S + |b| in magnitude, each addition rounds
                                                       once, rounding the 147 fp32 products of fp32 mode costs u S in all), and the bias: at
                                                       most 148 P + 1 <= 224 P roundings.
                  + 2^-22 S   (f16x3)                  the lo x lo partial product that is never formed
                E_c = A + r (|c| + A) [+ 2^-25]        one store of the computed value.  f16x3: hi = fp16(v) leaves |v - hi| <= 2^-11 |v|, lo =
                                                       fp16(v - hi) leaves 2^-11 of that -- or, where lo is an fp16 subnormal, half its spacing
                                                       of 2^-24: the absolute floor the header documents for split tensors
  pool          E_m = max of E_c over the window       |max a_i - max b_i| <= max |a_i - b_i|, over the window positions that exist
  BN + ReLU     v = |s m + t| + |s| E_m                one fma (u v), then one store (r v (1 + u) [+ 2^-25]; none in fp32, where the fma's
                E_p = |s| E_m + u v + r v (1 + u)      result is what is stored); ReLU does not increase a difference
  conv1         E_a = sum |w1| E_p + (64 P u [+ 2^-22]) sum |w1| (|p| + E_p)       the operand is the pooled tensor the kernel STORED
  BN + ReLU     as above with (s1, t1) -> E_h
Every element must lie inside its own bound: no factor, no excluded share.  Largest error / bound ratios measured on an MI355X are in
profiles/stem_alone.log (listed in profiles/README.md).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from human_dynamics_amd import _lib as L
from human_dynamics_amd import assets
from oracle import hmmr_oracle as O

gpu = pytest.mark.gpu

MODES = {"f32": (L.HMMR_F32, None), "bf16": (L.HMMR_BF16, "bf16"), "f16x3": (L.HMMR_F16X3, "f16x3")}
THREE, FUSED = 1, 2                                   # hmmr_debug_t.stem_route
ROUTES = {"three_kernel": THREE, "fused": FUSED}
BATCHES = [(1, 0), (3, 0), (2, 1), (0, 2)]
ZERO = 3                                              # index of the all-zero image in a reference of [3 images + the zero image]
U1 = "resnet_v2_50/block1/unit_1/bottleneck_v2"
ONE_HOT = ("onehot0", "onehot1", "onehot2")
F64 = torch.float64
_wsets, _frames_of, _packed, _ref64, _exact = {}, {}, {}, {}, {}


# ------------------------------------------------------------------------------------------------------------------ inputs
def _exact_bn(scale, shift):
    """BN variables whose fold (packing.fold_bn / oracle._fold_bn32) is EXACTLY (scale, shift): mean 0, var = fp32(1 - 1e-5)"""
    var = np.full(len(scale), np.float32(1.0 - 1e-5), np.float32)
    return {"/gamma": np.asarray(scale, np.float32), "/beta": np.asarray(shift, np.float32), "/moving_mean": np.zeros(len(scale), np.float32),
            "/moving_variance": var}


def _taps(s):
    """one-hot set s: output channel o looks at tap (64 s + o) mod 147 = (ky, kx, c); the three sets cover all 147 taps"""
    return np.stack(np.unravel_index((64 * s + np.arange(64)) % 147, (7, 7, 3)), axis=1)


def _weight_set(name, base):
    """the session's synthetic weights with the stem filter and bias, block1/unit_1's preact BN, its conv1 and conv1's BN replaced"""
    if name in _wsets:
        return _wsets[name]
    w = dict(base)
    rng = np.random.Generator(np.random.PCG64([77, sorted(("plain", "wide") + ONE_HOT).index(name)]))
    if name in ONE_HOT:
        taps = _taps(ONE_HOT.index(name))
        f = np.zeros((7, 7, 3, 64), np.float32)
        f[taps[:, 0], taps[:, 1], taps[:, 2], np.arange(64)] = 1.0
        w["resnet_v2_50/conv1/weights"] = f
        w["resnet_v2_50/conv1/biases"] = rng.integers(-32, 33, 64).astype(np.float32)
        pre = _exact_bn(np.array([1, -1, 2, 0], np.float32)[(np.arange(64) + ONE_HOT.index(name)) % 4], rng.integers(-32, 33, 64))
        w[U1 + "/conv1/weights"] = np.eye(64, dtype=np.float32)[None, None]
        bn1 = _exact_bn(np.ones(64), np.zeros(64))
    else:
        f = np.array(base["resnet_v2_50/conv1/weights"], np.float32)
        if name == "wide":                                   # rows from 2^-12 to 2^4: the f16x3 pack-time row scale runs from 2^25 to 2^9
            top = np.exp2(np.linspace(-12.0, 4.0, 64))[rng.permutation(64)]
            f = (f * (top / np.abs(f).reshape(-1, 64).max(axis=0))).astype(np.float32)
        w["resnet_v2_50/conv1/weights"] = f
        b = np.array(base["resnet_v2_50/conv1/biases"], np.float32)
        b[rng.permutation(64)[:16]] = -10.0                  # a quarter of the channels: every conv value of such a channel is negative
        w["resnet_v2_50/conv1/biases"] = b
        pre = {k: np.array(base[U1 + "/preact" + k], np.float32) for k in ("/gamma", "/beta", "/moving_mean", "/moving_variance")}
        order = rng.permutation(64)
        pre["/gamma"][order[:12]] *= -1.0                    # negative scales ...
        pre["/gamma"][order[12:20]] = 0.0                    # ... and exact zeros
        bn1 = {k: np.array(base[U1 + "/conv1/BatchNorm" + k], np.float32) for k in ("/gamma", "/beta", "/moving_mean", "/moving_variance")}
    for k, v in pre.items():
        w[U1 + "/preact" + k] = v
    for k, v in bn1.items():
        w[U1 + "/conv1/BatchNorm" + k] = v
    _wsets[name] = w
    return w


def _frames(name):
    """three images [3,224,224,3] fp32: noise; +-5 stripes on the top rows and left columns; stripes on the bottom rows and right columns.
    The one-hot sets get integers in [-64, 64] with the same stripes (+-64)."""
    kind = "int" if name in ONE_HOT else "float"
    if kind not in _frames_of:
        if kind == "int":
            f = np.random.Generator(np.random.PCG64(5)).integers(-64, 65, (3, 224, 224, 3)).astype(np.float32)
            amp = 64.0
        else:
            f = assets.make_synthetic_frames(3, seed=11)
            amp = 5.0
        sign = np.where(np.arange(224) % 2 == 0, amp, -amp).astype(np.float32)
        f[1, :7] = sign[:7, None, None]
        f[1, :, :7] = sign[None, :7, None]
        f[2, -9:] = -sign[-9:, None, None]
        f[2, :, -9:] = -sign[None, -9:, None]
        _frames_of[kind] = f
    return _frames_of[kind]


def _four(name):
    """the reference's images: the three frames + the zero image"""
    return np.concatenate([_frames(name), np.zeros((1, 224, 224, 3), np.float32)])


def _ref_index(batch, order=(0, 1, 2)):
    """rows of a [3 images + zero image] reference that a batch (n, n_zero) of the frames `order[:n]` produces"""
    return list(order[:batch[0]]) + [ZERO] * batch[1]


# ------------------------------------------------------------------------------------------------------------------ references
def index_answer(images, taps, bias, pscale, pshift):
    """a's answer, no convolution: conv[cy, cx, o] = img[2 cy + ky - 3, 2 cx + kx - 3, c] (0 outside the image) + bias[o]; pooled = relu(scale *
    max over the window rows 2 py .. 2 py + 2, columns alike, THAT EXIST (<= 111) + shift).  float64 arrays of integers."""
    m = images.shape[0]
    pad = np.zeros((m, 230, 230, 3), np.float64)
    pad[:, 3:227, 3:227] = images
    ext = np.full((m, 113, 113, 64), -np.inf)
    for o, (ky, kx, c) in enumerate(taps):
        ext[:, :112, :112, o] = pad[:, ky:ky + 223:2, kx:kx + 223:2, c] + float(bias[o])
    pool = np.full((m, 56, 56, 64), -np.inf)
    for dy in range(3):
        for dx in range(3):
            pool = np.maximum(pool, ext[:, dy:dy + 111:2, dx:dx + 111:2])
    return np.maximum(pool * np.asarray(pscale, np.float64) + np.asarray(pshift, np.float64), 0.0)


def _exact_answer(name):
    if name not in _exact:
        w = _wsets[name]
        ps, pt = O._fold_bn32(w, U1 + "/preact")
        _exact[name] = index_answer(_four(name), _taps(ONE_HOT.index(name)), w["resnet_v2_50/conv1/biases"], ps, pt)
    return _exact[name]


U = 2.0 ** -24
PARTS = {"f32": 1, "bf16": 1, "f16x3": 3}
LOLO = {"f32": 0.0, "bf16": 0.0, "f16x3": 2.0 ** -22}
STORE = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16x3": 2.0 ** -22}       # unit roundoff: 24, 8 and 11 + 11 significand bits
FLOOR = {"f32": 0.0, "bf16": 0.0, "f16x3": 2.0 ** -25}


def float64_stem(images, w, mode, bounds=True):
    """{conv1, pooled, h1 [, E_pooled, E_h1]} as NHWC float64 arrays: the module docstring's reference and bound"""
    em = MODES[mode][1]
    col = lambda a: torch.as_tensor(np.asarray(a, np.float64)).view(1, -1, 1, 1)
    x = O.quantize(torch.as_tensor(np.asarray(images), dtype=F64), em).permute(0, 3, 1, 2).contiguous()
    wq = O.quantize(torch.as_tensor(np.asarray(w["resnet_v2_50/conv1/weights"]), dtype=F64), em, weight=True)
    bias = np.asarray(w["resnet_v2_50/conv1/biases"], np.float64)
    conv = O._conv(x, wq, F64, stride=2, pad=3, bias=bias)
    pool = lambda t: F.max_pool2d(F.pad(t, (0, 1, 0, 1), value=float("-inf")), 3, stride=2)
    ps, pt = (col(v) for v in O._fold_bn32(w, U1 + "/preact"))
    z = pool(conv) * ps + pt
    pooled = torch.relu(z)
    w1 = O.quantize(torch.as_tensor(np.asarray(w[U1 + "/conv1/weights"]), dtype=F64), em, weight=True)[0, 0]        # [in][out]
    s1, t1 = (col(v) for v in O._fold_bn32(w, U1 + "/conv1/BatchNorm"))
    mix = lambda t, m: torch.einsum("nchw,co->nohw", t, m)
    z1 = mix(pooled, w1) * s1 + t1
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()
    out = {"conv1": nhwc(conv), "pooled": nhwc(pooled), "h1": nhwc(torch.relu(z1))}
    if bounds:
        P, r, lolo, floor = PARTS[mode], STORE[mode], LOLO[mode], FLOOR[mode]
        r2 = 0.0 if mode == "f32" else r                                    # after an fma: fp32 stores the fma's own result
        S = O._conv(x.abs(), wq.abs(), F64, stride=2, pad=3)
        A = 224 * P * U * (S + col(np.abs(bias))) + lolo * S
        Ec = A + r * (conv.abs() + A) + floor
        Em = pool(Ec)
        v = z.abs() + ps.abs() * Em
        Ep = ps.abs() * Em + U * v + r2 * v * (1 + U) + floor
        Ea = mix(Ep, w1.abs()) + (64 * P * U + lolo) * mix(pooled + Ep, w1.abs())
        v1 = z1.abs() + s1.abs() * Ea
        out["E_pooled"], out["E_h1"] = nhwc(Ep), nhwc(s1.abs() * Ea + U * v1 + r2 * v1 * (1 + U) + floor)
    return out


def _reference(name, mode):
    if (name, mode) not in _ref64:
        _ref64[(name, mode)] = float64_stem(_four(name), _wsets[name], mode)
    return _ref64[(name, mode)]


# ------------------------------------------------------------------------------------------------------------------ CPU: the references themselves
def test_float64_stem_reference_equals_the_reference_project_at_conv1(weights):
    """float64_stem's conv1 stage on the fixture frames against tests/golden/reference_resnet.npz (the reference project's encoder executed
    on slim's transcription), with the sampling of test_reference_golden.py: the stage b's reference shares with nothing in this package."""
    from test_reference_golden import _resnet_frames, _sample
    import os
    g = dict(np.load(os.path.join(GOLDEN, "reference_resnet.npz")))
    got = float64_stem(_resnet_frames(), weights, "f32", bounds=False)
    want = g["ep:resnet_v2_50/conv1"]
    assert _sample(got["conv1"]).shape == want.shape
    assert np.abs(_sample(got["conv1"]) - want).max() < 1e-11
    # ... and its later stages are the oracle's (whose every unit output is pinned to the same file)
    _, ep = O.resnet_v2_50(_resnet_frames(), weights, F64, return_endpoints=True)
    ps, pt = O._fold_bn32(weights, U1 + "/preact")
    pre = np.maximum(ep["pool1"].permute(0, 2, 3, 1).numpy() * ps.astype(np.float64) + pt.astype(np.float64), 0)
    assert np.abs(got["pooled"] - pre).max() < 1e-12


def test_index_answer_equals_the_float64_reference_on_one_hot_filters(weights):
    """a's index computation and b's convolution are two statements of the same stem: on a one-hot set they agree exactly (every value is a
    small integer), including 'rows past 111 do not exist' -- checked here on pixels where a zero there would win."""
    w = _weight_set("onehot2", weights)
    imgs = _four("onehot2")[[2, ZERO]]
    ps, pt = O._fold_bn32(w, U1 + "/preact")
    assert set(np.unique(ps)) == {-1.0, 0.0, 1.0, 2.0} and np.array_equal(pt, np.round(pt))          # the fold is exact
    a = index_answer(imgs, _taps(2), w["resnet_v2_50/conv1/biases"], ps, pt)
    b = float64_stem(imgs, w, "f32", bounds=False)
    assert np.array_equal(a, b["pooled"]) and np.array_equal(a, b["h1"])       # conv1 = identity, pooled >= 0
    # had the pool read zeros past row / column 111, these elements would differ
    zeros = index_answer_with_zero_border(imgs, _taps(2), w["resnet_v2_50/conv1/biases"], ps, pt)
    differ = (zeros != a)
    assert differ[:, 55].any() and differ[:, :, 55].any() and not differ[:, :55, :55].any()
    assert sorted(set(map(tuple, np.concatenate([_taps(s) for s in range(3)])))) == [(ky, kx, c) for ky in range(7) for kx in range(7) for c in range(3)]


def index_answer_with_zero_border(images, taps, bias, pscale, pshift):
    """index_answer with the WRONG pool rule (row / column 112 of the conv map = 0): only to show that the inputs tell the two apart"""
    right = index_answer(images, taps, bias, pscale, pshift)
    m = images.shape[0]
    pad = np.zeros((m, 230, 230, 3), np.float64)
    pad[:, 3:227, 3:227] = images
    ext = np.zeros((m, 113, 113, 64))
    for o, (ky, kx, c) in enumerate(taps):
        ext[:, :112, :112, o] = pad[:, ky:ky + 223:2, kx:kx + 223:2, c] + float(bias[o])
    pool = np.full((m, 56, 56, 64), -np.inf)
    for dy in range(3):
        for dx in range(3):
            pool = np.maximum(pool, ext[:, dy:dy + 111:2, dx:dx + 111:2])
    wrong = np.maximum(pool * np.asarray(pscale, np.float64) + np.asarray(pshift, np.float64), 0.0)
    assert wrong.shape == right.shape
    return wrong


def test_error_bound_is_positive_and_of_the_formats_size(weights):
    """the bound of b on the striped image: nowhere zero where the reference is not, and of the size its leading terms give -- 224 P u
    (1.3e-5 P) and r of sum |x||w|, which the cancellation of a convolution leaves several times |c|; conv1 sums 64 such bounds.  Half the
    elements above 0.1 have a bound below: pooled 3e-4 (fp32), 1e-3 (f16x3), 2e-2 (bf16: two stores at 2^-8 of |c|, not of c) of their value,
    h1 ten times that.  A wrong tap,
    origin or pool rule moves an element by a good part of its value."""
    for name in ("plain", "wide"):
        w = _weight_set(name, weights)
        for mode, size in (("f32", 3e-4), ("f16x3", 1e-3), ("bf16", 2e-2)):
            r = float64_stem(_frames(name)[1:2], w, mode)
            for t, k in (("pooled", 1.0), ("h1", 10.0)):
                E, ref = r["E_" + t], r[t]
                assert (E[ref != 0] > 0).all() and np.isfinite(E).all()
                assert np.median(E[ref > 0.1] / ref[ref > 0.1]) < k * size, (name, mode, t)


# ------------------------------------------------------------------------------------------------------------------ GPU plumbing
def _flags():
    """read and clear hmmr_run_flags"""
    fl = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(fl), 1), "hmmr_run_flags")
    return fl.value


def _pack(name, mode, base, dev):
    from human_dynamics_amd import engine as E
    if (name, mode) not in _packed:
        _packed[(name, mode)] = E.pack_stem(_weight_set(name, base), mode, dev)
    return _packed[(name, mode)]


class Run(object):
    """one stem call: .pooled / .h1 as raw storage rows with their guard rows, .written, .flags, .counts"""


def _run(name, mode, route, base, dev, images=None, n_zero=0, no_conv1=0):
    from human_dynamics_amd import engine as E
    _flags()
    L.stem_launch_counts(clear=True)
    c = E.StemCall(images, None, mode, n_zero=n_zero, route=route, no_conv1=no_conv1, device=dev, packed=_pack(name, mode, base, dev))
    c.run()
    torch.cuda.synchronize()
    r = Run()
    r.call, r.pooled, r.h1, r.written, r.rows, r.nt = c, c.pooled, c.h1, c.h1_written, c.rows, c.n + c.n_zero
    r.flags, r.counts = _flags(), L.stem_launch_counts(clear=True)
    # the launch counters prove which kernels ran, and h1_written is what the schedule says
    is_fused = route == FUSED or (route == 0 and mode != "f32")              # 0: the product default
    want_h1 = is_fused and mode != "f32" and not no_conv1
    if is_fused:
        assert r.counts == dict(fused=int(not want_h1), fused_conv1=int(want_h1), repack=0, gemm=0, pool=0), r.counts
    else:
        assert r.counts == dict(fused=0, fused_conv1=0, repack=1, gemm=1, pool=1), r.counts
    assert r.written == want_h1
    _guards(r, "%s %s route %d" % (name, mode, route))
    return r


def _sentinel(t):
    from human_dynamics_amd import engine as E
    return t.contiguous().view(torch.uint8) == E.STEM_SENTINEL_BYTE


def _guards(r, what):
    """guard rows untouched; every element of a written output written (an element = its bytes: none still all-sentinel); an unwritten h1
    intact"""
    from human_dynamics_amd import engine as E
    for nm, t, written in (("pooled", r.pooled, True), ("h1", r.h1, r.written)):
        assert t.shape[0] == r.rows + E.STEM_GUARD_ROWS
        assert bool(_sentinel(t[r.rows:]).all()), "%s %s: a store past row %d" % (what, nm, r.rows)
        left = _sentinel(t[:r.rows]).reshape(r.rows, 64, -1).all(dim=2)
        if written:
            assert not bool(left.any()), "%s %s: %d elements never written, first (row, channel) %s" % (
                what, nm, int(left.sum()), left.nonzero()[:4].tolist())
        else:
            assert bool(left.all()), "%s %s: written although the schedule leaves conv1 to its own launch" % (what, nm)


def _values(t, mode, rows):
    """storage rows -> float64 [images, 56, 56, 64] on the host"""
    from human_dynamics_amd import packing
    v = packing.from_split(t[:rows]) if mode == "f16x3" else t[:rows].float()
    return v.double().cpu().numpy().reshape(-1, 56, 56, 64)


def _where(mask, limit=6):
    return [tuple(int(i) for i in ix) for ix in np.argwhere(mask)[:limit]]


# ------------------------------------------------------------------------------------------------------------------ a
@gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("mode", list(MODES))
def test_stem_exact_known_answer(mode, route, weights, gpu_device):
    """One-hot filters (three sets: all 147 taps), integer pixels in [-64, 64], integer bias and preact shift in [-32, 32], preact scales in
    {1, -1, 2, 0}, conv1 = identity: every intermediate (|.| <= 224) is exact in bf16, in an fp16 pair and in fp32, so pooled EQUALS the index
    computation and h1 = relu(pooled) = pooled.  A difference is named: (image, pooled row, pooled column, channel) and the channel's tap."""
    for name in ONE_HOT:
        _weight_set(name, weights)
        want_all = _exact_answer(name)
        assert np.abs(want_all).max() <= 224 and (want_all[:, 55] > 0).any()
        taps = _taps(ONE_HOT.index(name))
        for batch in (BATCHES if name == ONE_HOT[0] else [(3, 0), (2, 1)]):
            r = _run(name, mode, ROUTES[route], weights, gpu_device, images=_frames(name)[:batch[0]], n_zero=batch[1])
            assert r.flags == 0
            want = want_all[_ref_index(batch)]
            for nm, t in (("pooled", r.pooled),) + ((("h1", r.h1),) if r.written else ()):
                got = _values(t, mode, r.rows)
                bad = got != want
                if bad.any():
                    first = _where(bad)
                    raise AssertionError("%s %s %s batch %s: %s differs at %d elements; (image, row, column, channel) [tap ky kx c] got / want: %s" % (
                        name, mode, route, batch, nm, int(bad.sum()),
                        "; ".join("%s %s %g / %g" % (ix, taps[ix[3]].tolist(), got[ix], want[ix]) for ix in first)))


# ------------------------------------------------------------------------------------------------------------------ b
@gpu
@pytest.mark.parametrize("name", ["plain", "wide"])
@pytest.mark.parametrize("mode", list(MODES))
def test_stem_against_float64_within_its_error_bound(mode, name, weights, gpu_device):
    """Every element of pooled and h1, on both routes and for every batch shape, inside ITS OWN bound (module docstring).  Measured on an
    MI355X (profiles/stem_alone.log), largest error / bound, weight sets plain / wide: fp32 pooled 0.167 / 0.167; bf16 pooled 0.936 / 0.947, h1 0.250 /
    0.428; f16x3 pooled 0.405 / 0.896, h1 0.0014 / 0.0022 (the same on both routes)."""
    _weight_set(name, weights)
    ref = _reference(name, mode)
    assert np.abs(ref["pooled"]).max() > 1 and np.abs(ref["h1"]).max() > 1
    worst = {}
    for route in ROUTES:
        for batch in BATCHES:
            r = _run(name, mode, ROUTES[route], weights, gpu_device, images=_frames(name)[:batch[0]], n_zero=batch[1])
            assert r.flags == 0
            rows = _ref_index(batch)
            for nm, t in (("pooled", r.pooled),) + ((("h1", r.h1),) if r.written else ()):
                got, want, E = _values(t, mode, r.rows), ref[nm][rows], ref["E_" + nm][rows]
                err = np.abs(got - want)
                ratio = np.where(E > 0, err / np.where(E > 0, E, 1.0), np.where(err > 0, np.inf, 0.0))
                worst[(route, nm)] = max(worst.get((route, nm), 0.0), float(ratio.max()))
                ix = np.unravel_index(np.argmax(ratio), ratio.shape)
                print("%-5s %-5s %-12s batch %s %-6s err/bound max %.3f at %s (err %.3e, bound %.3e, ref %.4g); max |err| %.3e, max |ref| %.3g" % (
                    mode, name, route, batch, nm, ratio.max(), tuple(int(i) for i in ix), err[ix], E[ix], want[ix], err.max(), np.abs(want).max()))
                bad = err > E
                assert not bad.any(), "%s %s %s batch %s: %s outside its bound at %d elements, first (image, row, column, channel) %s: got %r, float64 %r, bound %.3e" % (
                    mode, name, route, batch, nm, int(bad.sum()), _where(bad), got[bad][:3], want[bad][:3], E[bad][0])
    print("%s %s: largest err/bound %s" % (mode, name, {"%s/%s" % k: round(v, 4) for k, v in sorted(worst.items())}))


# ------------------------------------------------------------------------------------------------------------------ c
@gpu
@pytest.mark.parametrize("name", ["plain", "wide"])
@pytest.mark.parametrize("mode", list(MODES))
def test_stem_routes_and_conv1_launch_bit_for_bit(mode, name, weights, gpu_device):
    """pooled: fused == three-kernel.  h1 (bf16, f16x3): the fused kernel's conv1 == one hmmr_conv_gemm launch on the pooled tensor as stored.
    stem_no_conv1 = 1 leaves h1 unwritten (the sentinel intact) and pooled unchanged.  _run's counter assertions prove which kernels ran."""
    from human_dynamics_amd import engine as E
    from human_dynamics_amd import packing
    w = _weight_set(name, weights)
    imgs = _frames(name)[:2]
    three = _run(name, mode, THREE, weights, gpu_device, images=imgs, n_zero=1)
    fused = _run(name, mode, FUSED, weights, gpu_device, images=imgs, n_zero=1)
    plain = _run(name, mode, FUSED, weights, gpu_device, images=imgs, n_zero=1, no_conv1=1)
    default = _run(name, mode, 0, weights, gpu_device, images=imgs, n_zero=1) if mode != "f32" else None
    assert not three.written and not plain.written and three.flags == fused.flags == plain.flags == 0
    for other, what in ((fused, "fused"), (plain, "fused, stem_no_conv1")) + (((default, "default route"),) if default else ()):
        if not torch.equal(other.pooled, three.pooled):
            a, b = _values(other.pooled, mode, three.rows), _values(three.pooled, mode, three.rows)
            raise AssertionError("%s %s: pooled of the %s stem differs from the three-kernel route at (image, row, column, channel) %s, max |d| %.3e" % (
                mode, name, what, _where(a != b), np.abs(a - b).max()))
    if mode == "f32":
        return
    assert fused.written and default.written and torch.equal(default.h1, fused.h1)
    s1, t1 = packing.fold_bn(w, U1 + "/conv1/BatchNorm")
    dt = MODES[mode][0]
    x = fused.pooled[:fused.rows].reshape(3, 56, 56, 64)
    launch, _ = E.conv_gemm(x, np.asarray(w[U1 + "/conv1/weights"], np.float32), scale=s1, shift=t1, relu=True, raw=True, in_dtype=dt, out_dtype=dt,
                            device=gpu_device)
    assert _flags() == 0
    got = fused.h1[:fused.rows].reshape(3, 56, 56, 64)
    if not torch.equal(got, launch):
        a, b = _values(fused.h1, mode, fused.rows), _values(launch.reshape(-1, 64), mode, fused.rows)
        raise AssertionError("%s %s: h1 of the fused stem differs from the conv1 launch at (image, row, column, channel) %s, max |d| %.3e" % (
            mode, name, _where(a != b), np.abs(a - b).max()))


@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_full_pass_issues_the_stem_launches_of_the_entry(mode, weights, gpu_device):
    """hmmr_resnet50_fwd and hmmr_resnet50_stem issue ONE function: a full pass of the shipped configuration counts the launches the entry
    counts under the same switches (default: the three kernels in fp32, the fused kernel with conv1 inside else), and with the stem's conv1
    switched off phi keeps its bits (the launch the plan then adds computes the same h1)."""
    from human_dynamics_amd import engine as E
    eng = E.HmmrEngine(weights, None, dtype=mode, device=gpu_device, autotune=False)
    frames = assets.make_synthetic_frames(2, seed=7)
    out = {}
    try:
        for label, kw in (("default", {}), ("fused", dict(stem_route=2)), ("fused_no_conv1", dict(stem_route=2, stem_no_conv1=1)), ("three", dict(stem_route=1))):
            E.set_debug(**kw)
            L.stem_launch_counts(clear=True)
            out[label] = eng.resnet(frames, n_zero=1, parts=1).clone()
            torch.cuda.synchronize()
            got = L.stem_launch_counts(clear=True)
            c1 = mode != "f32" and label in ("default", "fused")
            three = label == "three" or (label == "default" and mode == "f32")
            assert got == dict(fused=int(not three and not c1), fused_conv1=int(c1), repack=int(three), gemm=int(three), pool=int(three)), (label, got)
    finally:
        E.set_debug()
    for label, phi in out.items():
        assert torch.equal(phi, out["three"]), label
    assert float(out["three"].abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------------------------ d
@gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("mode", list(MODES))
def test_stem_batch_behaviour(mode, route, weights, gpu_device):
    """An image's bits depend neither on n nor on its position (three images, permuted; alone; in front of a zero tail); a zero-tail image
    equals an explicit zero image; (0, 2) runs with images = NULL; no sentinel is left in a written output and the guard rows keep theirs
    (_run); the NaN rows behind the n real images are never read (finite outputs, flags 0); two runs give equal bits."""
    rt = ROUTES[route]
    f = _frames("plain")
    run = lambda imgs, nz=0: _run("plain", mode, rt, weights, gpu_device, images=imgs, n_zero=nz)
    per = lambda r, t, i: t[i * 3136:(i + 1) * 3136]
    a = run(f)
    outs = lambda r: (("pooled", r.pooled),) + ((("h1", r.h1),) if r.written else ())
    for nm, t in outs(a):
        assert np.isfinite(_values(t, mode, a.rows)).all(), nm
    assert a.flags == 0
    again = run(f)
    assert torch.equal(again.pooled, a.pooled) and torch.equal(again.h1, a.h1) and again.flags == 0
    order = [2, 0, 1]
    b = run(f[order])
    for (nm, ta), (_, tb) in zip(outs(a), outs(b)):
        for pos, src in enumerate(order):
            assert torch.equal(per(b, tb, pos), per(a, ta, src)), "%s: image %d at position %d differs from itself at position %d" % (nm, src, pos, src)
    one = run(f[:1])
    two_z = run(f[:2], 1)
    z_explicit = run(np.concatenate([f[:1], np.zeros_like(f[:1]), f[1:2]]))
    zz = run(f[:0], 2)
    assert zz.call.args["images"] is None and zz.flags == two_z.flags == one.flags == z_explicit.flags == 0
    for k, (nm, ta) in enumerate(outs(a)):
        get = lambda r: outs(r)[k][1]
        assert torch.equal(per(one, get(one), 0), per(a, ta, 0)), nm + ": image 0 alone"
        assert torch.equal(get(two_z)[:2 * 3136], ta[:2 * 3136]), nm + ": images 0, 1 in front of a zero tail"
        zero = per(z_explicit, get(z_explicit), 1)
        assert torch.equal(per(two_z, get(two_z), 2), zero), nm + ": the zero tail differs from an explicit zero image"
        assert torch.equal(per(zz, get(zz), 0), zero) and torch.equal(per(zz, get(zz), 1), zero), nm + ": (0, 2) with images = NULL"
        assert torch.equal(per(z_explicit, get(z_explicit), 2), per(a, ta, 1)), nm + ": image 1 behind a zero image"
        assert float(_values(zero, mode, 3136).max()) > 0                          # (bias and shifts alone: not a tensor of zeros)


# ------------------------------------------------------------------------------------------------------------------ e
@gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_stem_run_flags_f16x3(route, weights, gpu_device):
    """One bad pixel (NaN, +inf, 7e4: beyond the fp16 range) at (0, 0), at (223, 223) and on an interior tile seam (row 95 / column 128: the last
    input row of one 8 x 8 pooled tile's centre, the first column of the next), in the first and in the last real image of (3, 1): the
    saturation flag rises on either route (with the NaN flag for the NaN), the other images keep their bits; clean input and the zero tail
    raise nothing."""
    rt = ROUTES[route]
    f = _frames("plain")
    clean = _run("plain", "f16x3", rt, weights, gpu_device, images=f, n_zero=1)
    assert clean.flags == 0
    assert _run("plain", "f16x3", rt, weights, gpu_device, images=f[:0], n_zero=2).flags == 0
    outs = lambda r: [r.pooled] + ([r.h1] if r.written else [])
    for img in (0, 2):
        for (y, x) in ((0, 0), (223, 223), (95, 128)):
            for val in (float("nan"), float("inf"), 7e4):
                bad = f.copy()
                bad[img, y, x, 1] = val
                r = _run("plain", "f16x3", rt, weights, gpu_device, images=bad, n_zero=1)
                what = "pixel %r at image %d (%d, %d)" % (val, img, y, x)
                assert r.flags & L.FLAG_SATURATED, (what, r.flags)
                assert bool(r.flags & L.FLAG_NAN) == (val != val), (what, r.flags)
                for t, tc in zip(outs(r), outs(clean)):
                    for other in range(4):
                        if other != img:
                            assert torch.equal(t[other * 3136:(other + 1) * 3136], tc[other * 3136:(other + 1) * 3136]), "%s reached image %d" % (what, other)
                    assert not torch.equal(t[img * 3136:(img + 1) * 3136], tc[img * 3136:(img + 1) * 3136]), what + " changed nothing"
    after = _run("plain", "f16x3", rt, weights, gpu_device, images=f, n_zero=1)
    assert after.flags == 0 and torch.equal(after.pooled, clean.pooled) and torch.equal(after.h1, clean.h1)


# ------------------------------------------------------------------------------------------------------------------ f
@gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_refused_stem_call_queues_nothing(mode, weights, gpu_device):
    """each refusal of tests/test_abi.py::test_stem_entry_refuses_before_anything_is_queued on live buffers: an error, both outputs still the
    sentinel in every byte, no launch counted"""
    from human_dynamics_amd import engine as E
    f = _frames("plain")[:2]
    rw, store = _pack("plain", mode, weights, gpu_device)

    def refused(match, route=FUSED, table=None, **edit):
        c = E.StemCall(f, None, mode, n_zero=1, route=route, device=gpu_device, packed=(table if table is not None else rw, store))
        for k, v in edit.items():
            c.args[k] = v(c) if callable(v) else v
        L.stem_launch_counts(clear=True)
        with pytest.raises(L.HmmrError, match=match):
            c.run()
        torch.cuda.synchronize()
        assert bool(_sentinel(c.pooled).all()) and bool(_sentinel(c.h1).all()), match
        assert sum(L.stem_launch_counts(clear=True).values()) == 0
        assert c.h1_written is None

    for route in (THREE, FUSED):
        refused("16-byte aligned", route, images=lambda c: c.images.data_ptr() + 4)
        refused("null argument", route, images=None)
        refused("null argument", route, pooled=None)
        refused("at least one image", route, n=-1)
        refused("at least one image", route, n_zero=-3)
        refused("at least one image", route, n=0, n_zero=0)
    refused("workspace too small", THREE, ws_bytes=lambda c: 4096)
    bad = L.ResnetWeights.from_buffer_copy(rw)
    bad.dtype = 7
    refused("bad dtype", table=bad)
    if mode != "f16x3":
        scaled = L.ResnetWeights.from_buffer_copy(rw)
        scaled.stem.scale = scaled.unit[0].pre_scale          # a live vector of 64 floats: the three-kernel route would apply it
        refused("stem.scale", FUSED, table=scaled)
    # the same arguments unedited run
    c = E.StemCall(f, None, mode, n_zero=1, route=FUSED, device=gpu_device, packed=(rw, store))
    c.run()
    torch.cuda.synchronize()
    assert not bool(_sentinel(c.pooled[:c.rows]).reshape(c.rows, 64, -1).all(dim=2).any())


@gpu
def test_stem_without_conv1_filters_says_h1_is_not_written(weights, gpu_device):
    """a bf16 table whose block1/unit_1 has no conv1 filters: the fused kernel computes no conv1, and the entry says so -- h1_written 0,
    the counter of the plain fused launch, h1 still the sentinel (_run checks all three), pooled unchanged"""
    from human_dynamics_amd import engine as E
    rw, store = _pack("plain", "bf16", weights, gpu_device)
    bare = L.ResnetWeights.from_buffer_copy(rw)
    bare.unit[0].conv1.w = None
    f = _frames("plain")[:1]
    want = _run("plain", "bf16", FUSED, weights, gpu_device, images=f, no_conv1=1)
    L.stem_launch_counts(clear=True)
    c = E.StemCall(f, None, "bf16", route=FUSED, device=gpu_device, packed=(bare, store))
    c.run()
    torch.cuda.synchronize()
    assert c.h1_written is False and bool(_sentinel(c.h1).all())
    assert L.stem_launch_counts(clear=True) == dict(fused=1, fused_conv1=0, repack=0, gemm=0, pool=0)
    assert torch.equal(c.pooled, want.pooled) and _flags() == 0
