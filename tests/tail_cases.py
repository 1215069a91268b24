"""Weights, inputs, the float64 references and the error bounds of the f_movie / IEF tail sweep (tests/test_tail_cases.py on the host,
tests/test_gpu_tail.py on the device): csrc/temporal.hip (GroupNorm + ReLU, the temporal encoder, the hallucinator) and csrc/ief.hip.
No GPU is needed by anything in here.

The references are oracle.hmmr_oracle's own functions -- group_norm_time, az_fc2_groupnorm, hmr_ief -- in float64 with the rounding
points of the operand mode (`emulate`); the hallucinator's emulated form is written here (O.fc2_res has none), the present and delta
regressors are composed here as O.call_hmr_ief composes them (it does not pass num_stage through).

The bound comes from the reference, not from the kernels: E32 = |reference in float32 - reference in float64|, both with the same
`emulate`, over a family's inputs is the error of the same computation in the kernels' working precision, and a kernel may be FACTOR
times that away from the float64 reference.  In bf16 the maximum of E32 is made by single values that cross a bf16 rounding boundary,
so maximum and rms are two bounds.

The family's inputs: the temporal encoder takes three seeds of 2 windows x 7 frames and one window of 20.  The row-wise stages
(hallucinator, IEF) take three seeds of 86 rows: 258 rows, as many as the largest case of the sweep.  That is needed in bf16: there a
row is either right to 1e-7 or, where one stored value of its hidden layers crossed a rounding boundary, wrong by 1e-4 .. 1e-3 through
the layers behind it (about one hallucinator row in sixty) -- the maximum over a call is the maximum over its rows, so a family of
fewer rows than a case understates it (measured on the CPU: the hallucinator's E32 is 5.5e-5 over 62 rows and 9.5e-4 over 64 others)."""
import functools

import numpy as np
import torch

from human_dynamics_amd import assets
from oracle import hmmr_oracle as O

MODES = ("f32", "bf16", "f16x3")
EMULATE = {"f32": None, "bf16": "bf16", "f16x3": "f16x3"}
# |kernel - float64 reference| <= FACTOR x E32.  It starts at 4 (tests/smpl_cases.py); a measured legitimate ratio above 4 raises it to the
# smallest power of two that leaves 1.5 x over the largest ratio, 16 at the most -- profiles/tail_sweep.log holds the measured ratios.
FACTOR = 4.0
# what the suite asserted for these stages before the sweep (test_temporal_f32_matches_oracle, test_ief_f32_matches_oracle,
# test_temporal_and_ief_split_match_oracle), against the un-emulated float64 reference: no case of the sweep may exceed it
LEGACY = {("temporal", "f32"): 1e-4, ("temporal", "f16x3"): 2e-4, ("ief", "f32"): 2e-5, ("ief", "f16x3"): 5e-5}
SEED = 11
PACKED_BLOCKS = 3                                                # temporal blocks in the checkpoint
MAX_BLOCKS = 4                                                   # block 3 of a 4-block run takes block 0's variables again
DELTAS7 = (-15, -10, -5, 5, 10, 15, 20)                          # 1 + 7 = HMMR_MAX_REGRESSORS
REGRESSOR_SETS = ((), (5,), (-5, 5), (-10, -5, 5, 10), DELTAS7)      # R = 1, 2, 3, 5, 8
FAMILY_INPUTS = ((2, 7, 1), (2, 7, 2), (2, 7, 3), (1, 20, 4))    # (b, t, seed) of the windows the temporal encoder's E32 is taken over
FAMILY_ROWS = ((86, 1), (86, 2), (86, 3))                        # (rows, seed) of the inputs the hallucinator's and the IEF's are taken over


# ---------------------------------------------------------------------------------------------------------------- weights
def _is_tail(name):
    return name.startswith(("AZ_FC_block", "fc2_res/", "single_view_ief")) or name == "mean_param"


@functools.lru_cache(maxsize=None)
def weights():
    """3 temporal blocks (a run of n blocks uses the first n), the hallucinator, the present regressor and seven 72-wide delta regressors
    (a regressor set uses the scopes it names): assets.make_synthetic_weights filtered to the tail's variables; nobody writes to them"""
    w = assets.make_synthetic_weights(SEED, num_conv_layers=PACKED_BLOCKS, delta_t_values=DELTAS7, with_hallucinator=True)
    return {k: v for k, v in w.items() if _is_tail(k)}


@functools.lru_cache(maxsize=None)
def weights75():
    """the IEF variables alone with 75-wide delta regressors (use_optcam off)"""
    return assets.make_synthetic_ief_weights(SEED, DELTAS7, 75)


def temporal_weights(blocks):
    """the temporal variables of a run of `blocks` blocks: block i >= 3 has the variables of block i - 3 (packing one more 100 MB
    block per operand mode would only cost time: what a fourth block adds is the second use of the trunk buffer net[0])"""
    w = {k: v for k, v in weights().items() if k.startswith("AZ_FC_block")}
    for i in range(PACKED_BLOCKS, blocks):
        for old, new in zip(assets.temporal_scopes(i - PACKED_BLOCKS), assets.temporal_scopes(i)):
            w.update({new + k[len(old):]: v for k, v in weights().items() if k.startswith(old + "/")})
    return w


def ief_weights(width):
    return {72: weights, 75: weights75}[width]()


def delta_scope(dt):
    return assets.ief_scopes((dt,))[dt][0]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def phi_input(b, t, seed, scale=1.0):
    """[b, t, 2048] float32 features, every row different"""
    return (_rng(1, seed, b, t).standard_normal((b, t, 2048)) * scale).astype(np.float32)


def strips_input(m, seed):
    """[m, 2048] float32 movie strips"""
    return _rng(2, seed, m).standard_normal((m, 2048)).astype(np.float32)


def omega_rows(m, seed):
    """[m, 85] float32 starting omegas around the mean theta, every row different"""
    mean = np.asarray(weights()["mean_param"], np.float32).reshape(1, 85)
    return (mean + _rng(3, seed, m).standard_normal((m, 85)) * 0.1).astype(np.float32)


GN_FAMILIES = ("standard", "offset", "constant", "negative")
GN_CONSTANTS = (1.5, -2.25, 3.0, 0.0)                            # dyadic: any sum of up to 2^20 of them, and its mean, is exact in float32


def gn_input(family, b, t, c, groups, seed):
    """x [b, t, c], gamma [c], beta [c] (float32) of one input family:
      standard   N(0, 1), gamma in (0.5, 1.5), beta N(0, 0.1);
      offset     mean 100, deviation 0.01: the cancellation of the mean, and a variance of 1e-4 next to eps = 1e-6;
      constant   every second (window, group) holds one dyadic constant: variance 0, the output is relu(beta) in the output format;
      negative   beta = -10: everything is negative after the affine, the output is exactly 0."""
    rng = _rng(4, seed, b, t, c, groups, GN_FAMILIES.index(family))
    x = rng.standard_normal((b, t, c))
    gamma = rng.uniform(0.5, 1.5, c)
    beta = rng.standard_normal(c) * 0.1
    if family == "offset":
        x = 100.0 + 0.01 * x
    elif family == "constant":
        xg = x.reshape(b, t, groups, c // groups)
        for i in range(b):
            for g in range((i + 1) % 2, groups, 2):
                xg[i, :, g, :] = GN_CONSTANTS[(i + g) % len(GN_CONSTANTS)]
        x = xg.reshape(b, t, c)
    elif family == "negative":
        beta = beta - 10.0
    return x.astype(np.float32), gamma.astype(np.float32), beta.astype(np.float32)


def gn_constant_mask(b, t, c, groups):
    """[b, t, c] bool: the elements of the constant (window, group)s of gn_input('constant', ...)"""
    m = np.zeros((b, t, groups, c // groups), bool)
    for i in range(b):
        m[i, :, (i + 1) % 2::2, :] = True
    return m.reshape(b, t, c)


# ---------------------------------------------------------------------------------------------------------------- references
def _np64(t):
    a = t.to(torch.float64).numpy()
    a.setflags(write=False)
    return a


def ref_groupnorm_relu(x, gamma, beta, groups, dtype=torch.float64):
    """relu(O.group_norm_time) as float64 numpy (the values of a float32 run, widened)"""
    return _np64(torch.relu(O.group_norm_time(O._t(x, dtype), O._t(gamma, dtype), O._t(beta, dtype), groups)))


def ref_temporal(phi, blocks, mode, dtype=torch.float64):
    return _np64(O.az_fc2_groupnorm(phi, temporal_weights(blocks), blocks, dtype, EMULATE[mode]))


def ref_hallucinator(phi, w, dtype=torch.float64, emulate=None):
    """O.fc2_res with the rounding points of hmmr_hallucinator_fwd: phi cast to the operand type, h1 and h2 stored in it, the filters
    quantised as filter banks; the last layer leaves in fp32 and adds the fp32 phi"""
    q = lambda t: O.quantize(t, emulate)
    qw = lambda name: O.quantize(O._t(w["fc2_res/%s/weights" % name], dtype), emulate, weight=True)
    b = lambda name: O._t(w["fc2_res/%s/biases" % name], dtype)
    phi = O._t(phi, dtype)
    h = q(torch.relu(q(phi) @ qw("fc1") + b("fc1")))
    h = q(torch.relu(h @ qw("fc2") + b("fc2")))
    return h @ qw("fc3") + b("fc3") + phi


def ref_hallucinate(phi, mode, dtype=torch.float64):
    return _np64(ref_hallucinator(phi, weights(), dtype, EMULATE[mode]))


def compose_ief(strips, omega_start, w, deltas, num_stage=3, dtype=torch.float64, emulate=None, use_optcam=True, use_delta_from_pred=True):
    """O.call_hmr_ief (models.py:299-377) line for line, with num_stage passed on to O.hmr_ief -> (present [m, 85], {dt: delta [m, 85]})"""
    phi = O._t(strips, dtype)
    omega_start = O._t(omega_start, dtype)
    theta_here = O.hmr_ief(phi, omega_start, w, "single_view_ief", num_stage, dtype, emulate)
    nd = 72 if use_optcam else 3 + 72
    out = {}
    for dt in deltas:
        start_full = theta_here if use_delta_from_pred else omega_start
        beta = start_full[:, -10:]
        start = start_full[:, 3:3 + nd] if use_optcam else start_full[:, :nd]
        d = O.hmr_ief(phi, start, w, delta_scope(dt), num_stage, dtype, emulate)
        n = d.shape[0]
        if use_optcam:
            out[dt] = torch.cat([torch.ones(n, 1, dtype=dtype), torch.zeros(n, 2, dtype=dtype), d, beta], dim=1)
        else:
            out[dt] = torch.cat([d[:, :75], beta], dim=1)
    return theta_here, out


def start_rows(omega_start, m, w):
    """what the IEF starts from as [m, 85]: None = the mean theta in every row, one row = that row in every row, or m rows"""
    if omega_start is None:
        omega_start = np.asarray(w["mean_param"], np.float32)
    s = np.asarray(omega_start, np.float32).reshape(-1, 85)
    return np.array(np.broadcast_to(s, (m, 85))) if s.shape[0] == 1 else s           # (a copy: a broadcast view is read-only)


def ref_ief(strips, deltas, mode, stages=3, width=72, from_pred=True, omega_start=None, dtype=torch.float64):
    """[R, m, 85] float64 numpy in the engine's order: the present regressor, then the deltas sorted"""
    w = ief_weights(width)
    here, d = compose_ief(strips, start_rows(omega_start, strips.shape[0], w), w, sorted(deltas), stages, dtype, EMULATE[mode],
                          use_optcam=width == 72, use_delta_from_pred=from_pred)
    return _np64(torch.stack([here] + [d[k] for k in sorted(deltas)]))


# ---------------------------------------------------------------------------------------------------------------- E32 and the bounds
def _err(a32, a64):
    d = np.abs(a32 - a64)
    return float(d.max()), float(np.sqrt(np.mean(d * d)))


def _worst(pairs):
    return max(p[0] for p in pairs), max(p[1] for p in pairs)


def _family_windows():
    """the family's inputs as whole calls: windows of one length side by side (every window is a problem of its own)"""
    by_t = {}
    for b, t, s in FAMILY_INPUTS:
        by_t.setdefault(t, []).append(phi_input(b, t, s))
    return [np.concatenate(v) for _, v in sorted(by_t.items())]


@functools.lru_cache(maxsize=None)
def e32_temporal(mode, blocks):
    """(max, rms) of |float32 - float64| of the temporal reference over the family's inputs"""
    return _worst([_err(ref_temporal(phi, blocks, mode, torch.float32), ref_temporal(phi, blocks, mode)) for phi in _family_windows()])


@functools.lru_cache(maxsize=None)
def e32_hallucinator(mode):
    phi = np.concatenate([phi_input(1, m, s)[0] for m, s in FAMILY_ROWS])
    return _err(ref_hallucinate(phi, mode, torch.float32), ref_hallucinate(phi, mode))


@functools.lru_cache(maxsize=None)
def e32_ief(mode, stages=3, width=72, from_pred=True):
    """{'present': (max, rms), 'delta': (max, rms)}: the delta entry is the worst of all seven delta regressors; columns 3..74 of a
    72-wide delta and 0..74 of a 75-wide one (the others are copies and constants, asserted exactly).  The family's inputs run as one
    call: every row is a problem of its own."""
    lo = 3 if width == 72 else 0
    x = np.concatenate([strips_input(m, s) for m, s in FAMILY_ROWS])
    start = np.concatenate([omega_rows(m, s) for m, s in FAMILY_ROWS])
    r32 = ref_ief(x, DELTAS7, mode, stages, width, from_pred, start, torch.float32)
    r64 = ref_ief(x, DELTAS7, mode, stages, width, from_pred, start)
    return {"present": _err(r32[0], r64[0]), "delta": _worst([_err(r32[r][:, lo:75], r64[r][:, lo:75]) for r in range(1, r64.shape[0])])}


@functools.lru_cache(maxsize=None)
def e32_groupnorm(family, c, groups):
    """the maximum over three seeds at (b, t) = (3, 7) and one at (1, 20)"""
    out = []
    for b, t, s in ((3, 7, 1), (3, 7, 2), (3, 7, 3), (1, 20, 4)):
        x, g, be = gn_input(family, b, t, c, groups, s)
        out.append(_err(ref_groupnorm_relu(x, g, be, groups, torch.float32), ref_groupnorm_relu(x, g, be, groups)))
    return _worst(out)


def half_unit(ref, fmt):
    """half a unit in the last place of the output format at |ref| (elementwise, float64): f32, bf16 (8 significant bits), or the split
    pair (hi = fp16(x), lo = fp16(x - hi): 22 significant bits, and 2^-25 where lo is an fp16 subnormal)"""
    a = np.abs(np.asarray(ref, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    if fmt == "f32":
        return np.where(a > 0, np.exp2(e - 24), 0.0)
    if fmt == "bf16":
        return np.where(a > 0, np.exp2(e - 8), 0.0)
    if fmt == "f16x3":
        return np.where(a > 0, np.maximum(np.exp2(e - 22), 2.0 ** -25), 0.0)
    raise KeyError(fmt)


def bound(e32, mode, factor=None):
    """(bound on the maximum, bound on the rms or None): FACTOR x E32; the rms is a bound of its own in bf16 only"""
    f = FACTOR if factor is None else factor
    assert 1.0 <= f <= 16.0
    return f * e32[0], (f * e32[1] if mode == "bf16" else None)


# ---------------------------------------------------------------------------------------------------------------- the IEF workspace
def ief_theta_sets(m, regressors, mode):
    """Where hmmr_ief_fwd keeps the theta state (csrc/ief.hip, ief_layout; every buffer starts on a multiple of 256 bytes): the byte
    offset of th[0] in the workspace, the bytes of one problem's set, the number of sets, the whole workspace.  Set 0 serves a regressor
    that runs alone; sets 1 .. are written only by a grouped launch of the delta regressors."""
    r256 = lambda x: (x + 255) // 256 * 256
    e = 2 if mode == "bf16" else 4
    g = max(regressors - 1, 1)
    pre_s, th_s = r256(m * 1024 * e), r256(m * 128 * 4)
    th0 = r256(m * 2048 * e) + 3 * r256(g * pre_s)
    total = th0 + 2 * r256(g * th_s) + r256(g * 4 * m * 1024 * 4)
    return th0, th_s, g, total
