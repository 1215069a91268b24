"""The f_movie / IEF tail alone (csrc/temporal.hip: hmmr_groupnorm_relu, hmmr_temporal_fwd, hmmr_hallucinator_fwd; csrc/ief.hip:
hmmr_ief_fwd_from with its init and finalize kernels) against the float64 oracle: window lengths and row counts around every tile edge,
one-row calls, 1 to 4 temporal blocks, 1 to 4 IEF stages, 1 to 8 regressors of both delta widths, the three operand modes.

Every case compares each output SEPARATELY (the present regressor and every delta regressor of the IEF) with the float64 reference that
rounds where the operand mode rounds (tests/tail_cases.py).  The bound is not a chosen number: E32 = |reference in float32 - reference
in float64| over the case's family is the error of the same computation in the kernels' working precision, and a kernel may be
T.FACTOR times that; in bf16, where single values that cross a rounding boundary make the maximum, the rms has a bound of its own.
Independently no f32 / f16x3 case may exceed what the suite asserted for its stage before (T.LEGACY).  With `-s` every case prints its
error, E32, their ratio and a CRC of the output's bytes (two builds that give the same bits print the same lines), and the module
prints the largest ratio per stage, output and mode at the end (profiles/tail_sweep.log is one such run).

The bitwise promises of the code -- a window, a row do not depend on what shares the launch; grouped delta regressors give the bits of
one launch each; a grow-only workspace leaves nothing behind -- are asserted bit for bit.  Every call in this file is a valid call; the
refusals are in tests/test_abi.py."""
import copy
import functools
import time
import zlib

import numpy as np
import pytest
import torch

import tail_cases as T
from human_dynamics_amd import _lib as L
from human_dynamics_amd import packing

pytestmark = pytest.mark.gpu
MODES = T.MODES
DT = {"f32": L.HMMR_F32, "bf16": L.HMMR_BF16, "f16x3": L.HMMR_F16X3}
GUARD = 0xA5                  # every byte of a row no kernel may touch
_STATS = {"ratio": {}, "tests": 0, "t0": None}
_ENGINES = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _subset(prefixes):
    return {k: v for k, v in T.weights().items() if k.startswith(prefixes)}


def _movie_engine(device, mode, blocks):
    """the temporal encoder of `blocks` blocks, or (blocks = 0) the hallucinator.  The three packed blocks exist once per mode: a run of
    fewer is the same table with a lower count, a run of four takes block 0's entry again as block 3 (T.temporal_weights)."""
    key = ("movie", device, mode, blocks)
    if key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        if blocks in (0, T.PACKED_BLOCKS):
            w = _subset(("fc2_res/",)) if blocks == 0 else _subset(("AZ_FC_block",))
            eng = HmmrEngine(w, None, dtype=mode, device=device, num_conv_layers=T.PACKED_BLOCKS)
        else:
            base = _movie_engine(device, mode, T.PACKED_BLOCKS)
            eng = copy.copy(base)                                          # the same store and workspaces, a table of its own
            eng.tw = L.TemporalWeights.from_buffer_copy(base.tw)
            eng.tw.num_blocks = blocks
            for i in range(T.PACKED_BLOCKS, blocks):
                eng.tw.block[i] = base.tw.block[i - T.PACKED_BLOCKS]
        assert (eng.hw is not None) == (blocks == 0) and (eng.tw is None or eng.tw.num_blocks == blocks) and eng.iw is None
        _ENGINES[key] = eng
    return _ENGINES[key]


def _ief_engine(device, mode, deltas=(-5, 5), width=72, stages=3, fresh=False):
    key = ("ief", device, mode, tuple(deltas), width, stages)
    if fresh or key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        all_w = T.ief_weights(width)
        scopes = tuple(T.delta_scope(d) + "/" for d in deltas) + ("single_view_ief/", "mean_param")
        w = {k: v for k, v in all_w.items() if k.startswith(scopes)}
        eng = HmmrEngine(w, None, dtype=mode, device=device, delta_t_values=deltas)
        if stages != 3:
            eng.iw, eng.reg_keys = packing.pack_ief(w, eng.ief_dtype, eng.store, deltas, num_stages=stages)
        optcam = width == 72 or not deltas                                 # (the delta regressors' width decides; none: the default)
        assert (eng.iw.num_regressors, eng.iw.num_stages, eng.iw.no_optcam) == (1 + len(deltas), stages, int(not optcam))
        assert eng.reg_keys == [0] + sorted(deltas) and eng.use_optcam == optcam
        if fresh:
            return eng
        _ENGINES[key] = eng
    return _ENGINES[key]


def _flags(clear=True):
    import ctypes as C
    torch.cuda.synchronize()
    v = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(v), int(clear)), "hmmr_run_flags")
    return int(v.value)


@pytest.fixture(autouse=True)
def _clean_flags(gpu_device):
    """every test starts with clear run flags and must leave them clear"""
    _flags()
    _STATS["tests"] += 1
    yield
    assert _flags() == 0


@pytest.fixture(scope="module", autouse=True)
def _summary():
    _STATS["t0"] = time.time()
    yield
    from human_dynamics_amd.engine import set_debug
    set_debug()
    print("\ntail-sweep summary: %d tests, %.1f s wall (references included), FACTOR %g" % (_STATS["tests"], time.time() - _STATS["t0"], T.FACTOR))
    for (stage, out, mode, what), (r, tag) in sorted(_STATS["ratio"].items()):
        print("tail-sweep summary: largest err / E32 of %-12s %-8s %-5s %-3s: %6.2f (%s)" % (stage, out, mode, what, r, tag))
    _ENGINES.clear()


# ---------------------------------------------------------------------------------------------------------------- helpers
def _guarded(rows, row_shape, dtype, device):
    """[rows + 1, ...] with every byte GUARD, for a call that writes the first `rows`"""
    full = torch.empty((rows + 1,) + tuple(row_shape), dtype=dtype, device=device)
    full.view(torch.uint8).fill_(GUARD)
    return full


def _guard_kept(full, rows):
    return bool((full[rows:].contiguous().view(torch.uint8) == GUARD).all())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ratio(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float("inf"))


def _note(stage, out, mode, what, ratio, tag):
    if ratio > _STATS["ratio"].get((stage, out, mode, what), (-1.0, ""))[0]:
        _STATS["ratio"][(stage, out, mode, what)] = (ratio, tag)


def _check(stage, out, tag, mode, got, ref, e32, plain=None, allowance=None):
    """|got - ref| against FACTOR x E32 (+ an elementwise allowance): the maximum in every mode, the rms too in bf16; and against the
    stage's legacy bound, measured from the un-emulated float64 reference `plain`"""
    assert got.shape == ref.shape and np.isfinite(got).all(), (stage, out, tag, mode)
    d = np.abs(got.astype(np.float64) - ref)
    if allowance is not None:
        d = np.maximum(d - allowance, 0.0)
    err, rms = float(d.max()), float(np.sqrt(np.mean(d * d)))
    bmax, brms = T.bound(e32, mode)
    rmax, rrms = _ratio(err, e32[0]), _ratio(rms, e32[1])
    print("tail-sweep %-12s %-8s %-34s %-5s err %.3e  E32 %.3e  ratio %5.2f | rms %.3e  E32 %.3e  ratio %5.2f | crc %08x" %
          (stage, out, tag, mode, err, e32[0], rmax, rms, e32[1], rrms, zlib.crc32(np.ascontiguousarray(got).tobytes())))
    _note(stage, out, mode, "max", rmax, tag)
    assert err <= bmax, (stage, out, tag, mode, err, bmax)
    if brms is not None:
        _note(stage, out, mode, "rms", rrms, tag)
        assert rms <= brms, (stage, out, tag, mode, rms, brms)
    legacy = T.LEGACY.get((stage if stage in ("temporal", "ief") else None, mode))
    if legacy is not None:
        worst = float(np.abs(got.astype(np.float64) - (ref if plain is None else plain)).max())
        assert worst < legacy, (stage, out, tag, mode, worst, legacy)


# ---------------------------------------------------------------------------------------------------------------- a. GroupNorm + ReLU
GN_SHAPES = ((2048, 32), (256, 32), (512, 4))
GN_B, GN_T = (1, 3), (1, 2, 7, 20, 21, 33)


@functools.lru_cache(maxsize=None)
def _gn_case(family, b, t, c, groups):
    x, gamma, beta = T.gn_input(family, b, t, c, groups, 100 * b + t)
    return x, gamma, beta, T.ref_groupnorm_relu(x, gamma, beta, groups)


def _round_to(fmt, a):
    """float32 values as the output format stores them"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    if fmt == "bf16":
        return t.to(torch.bfloat16).float().numpy()
    if fmt == "f16x3":
        return packing.from_split(packing.to_split(t)).numpy()
    return t.numpy()


@pytest.mark.parametrize("fmt", MODES)
@pytest.mark.parametrize("c,groups", GN_SHAPES, ids=["c%d-g%d" % s for s in GN_SHAPES])
def test_groupnorm_relu(c, groups, fmt, gpu_device):
    """one workgroup of 256 threads per (window, group): t = 1 gives it 64 values (8 where a group has 8 channels), t = 7 a ragged 448;
    8 channels per group is the least the entry takes.  Output in fp32, bf16 and the split pair."""
    eng = _movie_engine(gpu_device, "f32", T.PACKED_BLOCKS)
    for b in GN_B:
        for t in GN_T:
            for fam in T.GN_FAMILIES:
                x, gamma, beta, ref = _gn_case(fam, b, t, c, groups)
                full = _guarded(b, (t, c), packing.empty_act((0,), DT[fmt], "cpu").dtype, gpu_device)
                out = eng.groupnorm_relu(x, gamma, beta, groups, DT[fmt], out=full)
                got = packing.act_to_f32(out, DT[fmt]).cpu().numpy()
                assert _guard_kept(full, b), (c, groups, fmt, b, t, fam)
                tag = "%s b%d t%d c%d g%d" % (fam, b, t, c, groups)
                if fam == "negative":
                    assert not _bits(got).any(), tag                     # exactly +0
                    continue
                _check("groupnorm", fmt, tag, "f32", got, ref, T.e32_groupnorm(fam, c, groups), allowance=T.half_unit(ref, fmt))
                if fam == "constant":                                    # variance 0, x - mean = 0: relu(beta) as the format stores it
                    mask = T.gn_constant_mask(b, t, c, groups)
                    want = np.broadcast_to(_round_to(fmt, np.maximum(beta, 0)), got.shape)
                    assert np.array_equal(got[mask], want[mask]), tag


# ---------------------------------------------------------------------------------------------------------------- b. the temporal encoder
TEMPORAL_SHAPES = ((1, 1), (1, 2), (2, 3), (3, 7), (1, 20), (2, 20), (3, 21), (5, 13), (7, 19), (13, 20))      # ... 65, 133, 260 rows
BLOCK_SHAPES = ((1, 2), (3, 7), (5, 13))


@functools.lru_cache(maxsize=None)
def _temporal_ref(b, t, blocks, mode):
    return T.ref_temporal(T.phi_input(b, t, 10 * b + t), blocks, mode)


def _temporal_case(device, mode, b, t, blocks):
    eng = _movie_engine(device, mode, blocks)
    full = _guarded(b, (t, 2048), torch.float32, device)
    got = eng.temporal(T.phi_input(b, t, 10 * b + t), out=full).cpu().numpy()
    assert _guard_kept(full, b), (mode, b, t, blocks)
    _check("temporal", "strips", "b%d t%d blocks %d" % (b, t, blocks), mode, got, _temporal_ref(b, t, blocks, mode),
           T.e32_temporal(mode, blocks), plain=_temporal_ref(b, t, blocks, "f32"))
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,t", TEMPORAL_SHAPES, ids=["b%d-t%d" % s for s in TEMPORAL_SHAPES])
def test_temporal_shapes(b, t, mode, gpu_device):
    """window lengths from 1 (every tap but the middle one reads padding) to 21, row counts b t from 1 across the 64, 128 and 256 row
    tiles; 3 blocks"""
    _temporal_case(gpu_device, mode, b, t, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("blocks", (1, 2, 4))
def test_temporal_block_counts(blocks, mode, gpu_device):
    """1 block writes the strips straight from phi, 2 use net[0] once; 4 come back to net[0] (block 2 overwrites what block 0 left there
    while block 1's output in net[1] is the residual).  3 blocks at three shapes and more: test_temporal_shapes."""
    for b, t in (BLOCK_SHAPES if blocks < 4 else BLOCK_SHAPES[1:2]):
        _temporal_case(gpu_device, mode, b, t, blocks)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,t", ((3, 7), (5, 13)))
def test_a_window_does_not_depend_on_what_shares_the_launch(b, t, mode, gpu_device):
    """csrc/temporal.hip: the slice count is fixed per layer and mode, so a window's bits are those of the window run alone -- which
    also rules out any row leaking across a window edge"""
    eng = _movie_engine(gpu_device, mode, 3)
    phi = T.phi_input(b, t, 10 * b + t)
    whole = eng.temporal(phi).cpu().numpy()
    for i in range(b):
        alone = eng.temporal(phi[i:i + 1]).cpu().numpy()
        assert _same_bits(whole[i:i + 1], alone), (mode, b, t, i)
    assert not _same_bits(whole[0], whole[1])


@pytest.mark.parametrize("mode", MODES)
def test_temporal_leaves_nothing_behind_in_its_workspace(mode, gpu_device):
    """a call after a larger call on inputs of magnitude 1e3 gives the bits of an engine that never saw it"""
    from human_dynamics_amd.engine import HmmrEngine
    small = [T.phi_input(b, t, 10 * b + t) for b, t in ((3, 7), (1, 2), (2, 20))]
    fresh = HmmrEngine(_subset(("AZ_FC_block",)), None, dtype=mode, device=gpu_device, num_conv_layers=3)
    want = [fresh.temporal(p).cpu().numpy() for p in small]
    eng = _movie_engine(gpu_device, mode, 3)
    for p, w in zip(small, want):
        big = eng.temporal(T.phi_input(13, 21, 5, scale=1e3))
        assert bool(torch.isfinite(big).all())
        assert _same_bits(eng.temporal(p).cpu().numpy(), w), (mode, p.shape)


# ---------------------------------------------------------------------------------------------------------------- c. the hallucinator
HAL_M = (1, 3, 63, 64, 65, 129, 257)


@functools.lru_cache(maxsize=None)
def _hal_ref(m, mode):
    return T.ref_hallucinate(T.phi_input(1, m, 7)[0], mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", HAL_M)
def test_hallucinator_rows(m, mode, gpu_device):
    eng = _movie_engine(gpu_device, mode, 0)
    phi = T.phi_input(1, m, 7)[0]
    full = _guarded(m, (2048,), torch.float32, gpu_device)
    got = eng.hallucinate(phi, out=full).cpu().numpy()
    assert _guard_kept(full, m), (mode, m)
    _check("hallucinator", "strips", "m%d" % m, mode, got, _hal_ref(m, mode), T.e32_hallucinator(mode))
    for i in sorted({0, m // 2, m - 1, min(m - 1, 63), min(m - 1, 64)}):       # a row is the row run alone, bit for bit
        alone = eng.hallucinate(phi[i:i + 1]).cpu().numpy()
        assert _same_bits(got[i:i + 1], alone), (mode, m, i)


# ---------------------------------------------------------------------------------------------------------------- d. the IEF
IEF_M = (1, 2, 20, 63, 64, 65, 129, 257)


def _start(kind, m, seed):
    return {"none": None, "row": T.omega_rows(1, seed), "rows": T.omega_rows(m, seed)}[kind]


@functools.lru_cache(maxsize=None)
def _ief_ref(m, deltas, mode, stages, width, from_pred, start_kind):
    seed = 1000 + m
    return T.ref_ief(T.strips_input(m, seed), deltas, mode, stages, width, from_pred, _start(start_kind, m, seed))


def _ief_run(eng, m, from_pred, start_kind):
    seed = 1000 + m
    R = eng.iw.num_regressors
    full = _guarded(R * m, (85,), torch.float32, eng.device)
    out = eng.ief(T.strips_input(m, seed), _start(start_kind, m, seed), use_delta_from_pred=from_pred, out=full.view(-1))
    assert _guard_kept(full, R * m), (m, R)
    return out.cpu().numpy()


def _ief_case(device, mode, m, deltas=(-5, 5), stages=3, width=72, from_pred=True, start_kind="none", rows_alone=()):
    """one call: the present and every delta regressor against float64, one by one; the constant and copied columns exactly"""
    eng = _ief_engine(device, mode, deltas, width, stages)
    got = _ief_run(eng, m, from_pred, start_kind)
    ref = _ief_ref(m, tuple(deltas), mode, stages, width, from_pred, start_kind)
    plain = _ief_ref(m, tuple(deltas), "f32", stages, width, from_pred, start_kind)
    e = T.e32_ief(mode, stages, width, from_pred)
    tag = "m%d R%d st%d w%d %s %s" % (m, 1 + len(deltas), stages, width, "pred" if from_pred else "start", start_kind)
    assert got.shape == ref.shape == (1 + len(deltas), m, 85)
    _check("ief", "present", tag, mode, got[0], ref[0], e["present"], plain=plain[0])
    lo = 3 if width == 72 else 0
    src = got[0] if from_pred else T.start_rows(_start(start_kind, m, 1000 + m), m, T.ief_weights(width))
    for r, dt in enumerate(sorted(deltas), 1):
        _check("ief", "delta", tag + " dt%+d" % dt, mode, got[r][:, lo:75], ref[r][:, lo:75], e["delta"], plain=plain[r][:, lo:75])
        if width == 72:
            assert _same_bits(got[r][:, :3], np.tile(np.float32([1, 0, 0]), (m, 1))), (tag, dt)
        assert _same_bits(got[r][:, 75:], np.ascontiguousarray(src[:, 75:], np.float32)), (tag, dt)     # beta: a copy of its source row
    for i in rows_alone:                                                   # a row is the row run alone, bit for bit
        seed = 1000 + m
        st = _start(start_kind, m, seed)
        alone = eng.ief(T.strips_input(m, seed)[i:i + 1], st if st is None or st.shape[0] == 1 else st[i:i + 1],
                        use_delta_from_pred=from_pred).cpu().numpy()
        assert _same_bits(got[:, i:i + 1], alone), (tag, i)
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", IEF_M)
def test_ief_row_counts(m, mode, gpu_device):
    """3 stages, 3 regressors; one row, and rows across the 64, 128 and 256 row tiles"""
    _ief_case(gpu_device, mode, m, rows_alone=sorted({0, m // 2, m - 1, min(m - 1, 63), min(m - 1, 64)}))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stages", (1, 2, 3, 4))
def test_ief_stage_counts(stages, mode, gpu_device):
    """the parity of the stage count decides which theta buffer ief_finalize_kernel reads"""
    for m in (20, 65):
        _ief_case(gpu_device, mode, m, stages=stages)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("start_kind", ("none", "row", "rows"))
def test_ief_starting_points(start_kind, mode, gpu_device):
    """omega_start: the mean theta (one broadcast row inside the kernels), one row, a row per frame; deltas from the prediction and from
    the start; both delta widths"""
    for width in (72, 75):
        for from_pred in (True, False):
            _ief_case(gpu_device, mode, 20, width=width, from_pred=from_pred, start_kind=start_kind, rows_alone=(0, 19))


def _ief_workspace(eng, m):
    """the engine's IEF workspace for m rows, every byte GUARD"""
    n = eng.lib.hmmr_ief_workspace_bytes(m, eng.iw.num_regressors, eng.ief_dtype)
    ws = eng._ws["ief"].get(n)
    ws.fill_(GUARD)
    return ws


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", (72, 75))
@pytest.mark.parametrize("deltas", T.REGRESSOR_SETS, ids=["R%d" % (1 + len(s)) for s in T.REGRESSOR_SETS])
def test_ief_regressor_sets(deltas, width, mode, gpu_device):
    """R = 1, 2, 3, 5, 8 (HMMR_MAX_REGRESSORS).  From 3 delta regressors on `strides_of` in hmmr_ief_fwd_from decides whether they run
    as grouped launches; a silent `false` would pass every comparison.  hmmr_launch_counts_t counts the fused-unit kernel families only,
    none of which the IEF launches, so the test reads what a grouped launch alone does: problem z > 0 keeps its theta state in set z of
    the workspace, a regressor that runs alone always in set 0."""
    from human_dynamics_amd.engine import set_debug
    m, R = 65, 1 + len(deltas)
    eng = _ief_engine(gpu_device, mode, deltas, width)
    th0, th_s, g, total = T.ief_theta_sets(m, R, mode)
    for from_pred in (True, False):
        ws = _ief_workspace(eng, m)
        assert ws.numel() >= total
        got = _ief_case(gpu_device, mode, m, deltas=deltas, width=width, from_pred=from_pred, start_kind="rows")
        sets = ws[th0:th0 + g * th_s].cpu().numpy().reshape(g, th_s)[:, :m * 512]
        assert (sets[0] != GUARD).any()
        if R < 3:
            continue
        assert all((sets[z] != GUARD).any() for z in range(1, g)), "the delta regressors did not run grouped"
        try:                                                               # ... and one launch each gives the same bits
            set_debug(ief_no_group=1)
            ws = _ief_workspace(eng, m)
            alone = _ief_run(eng, m, from_pred, "rows")
            sets = ws[th0:th0 + g * th_s].cpu().numpy().reshape(g, th_s)[:, :m * 512]
        finally:
            set_debug()
        assert (sets[0] != GUARD).any() and (sets[1:] == GUARD).all()      # the control: ungrouped, sets 1 .. stay untouched
        assert _same_bits(got, alone), (deltas, width, mode, from_pred)
        assert all(not _same_bits(got[1], got[r]) for r in range(2, R))


@pytest.mark.parametrize("mode", MODES)
def test_ief_leaves_nothing_behind_in_its_workspace(mode, gpu_device):
    """a call after a larger call on strips of magnitude 1e3 gives the bits of an engine that never saw it"""
    fresh = _ief_engine(gpu_device, mode, fresh=True)
    want = {m: _ief_run(fresh, m, True, "none") for m in (1, 20, 65)}
    eng = _ief_engine(gpu_device, mode)
    for m, w in want.items():
        big = eng.ief(T.strips_input(257, 3) * np.float32(1e3))
        assert bool(torch.isfinite(big).all())
        assert _same_bits(_ief_run(eng, m, True, "none"), w), (mode, m)
