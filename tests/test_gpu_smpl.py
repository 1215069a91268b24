"""The SMPL stage alone (csrc/smpl.hip: smpl_pose_kernel, the three vertex kernels, smpl_joints_kernel) against the float64 oracle:
ragged instance counts, vertex counts around every tile edge, skinning widths, keypoint regressors with empty and long columns,
strided inputs, record mode, the multi-tile loop of the split-fp16 form, stale scratch and the run flags.

Every case compares verts, joints, kps and Rs SEPARATELY with oracle.smpl_forward in float64.  The bound is not a chosen number:
E32 = |oracle in float32 - oracle in float64| over the case's family (tests/smpl_cases.py) is the error of the same computation in the
kernels' working precision, and a kernel may be FACTOR = 4 times that (another summation order, FMA, the joint regressor folded on the
host, device sinf / cosf, the wave reduction); the split-fp16 blend (form 0) gets the 2e-6 the project documents for it on top.
Independently no `standard` case may exceed the 2e-5 the suite asserted before.  With `-s` every case prints its error, E32 and their
ratio, and the module prints the largest ratio per output and form at the end (profiles/smpl_sweep.log is one such run).

Forms (hmmr_debug_t.smpl_blend_mfma): 0 = split-fp16 MFMA blend (the default), 1 = exact-fp32 MFMA blend, 2 = packed-FMA vector blend.
Every call in this file is a valid call; the refusals are in tests/test_abi.py."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import smpl_cases as S
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
FORMS = (0, 1, 2)
FAMILIES = ("standard", "wide")
M_LIST = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 36, 37, 63, 64, 65)
NV_LIST = (1, 31, 32, 33, 100, 127, 128, 129, 255, 256, 257, 300)
GUARD = 0x7FC12345            # a quiet NaN with a payload: the bit pattern of every float no kernel may touch
_STATS = {"ratio": {}, "tests": 0, "t0": None}


# ---------------------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def _model(nv, nk=25, nnz=4, short=True, empty=False, long=False):
    return S.model(nv, nk=nk, nnz=nnz, seed=nv + 100 * nk + 10000 * nnz, short_rows=short, empty_col=empty, long_cols=long)


_ENGINES = {}


def _engine(device, nv, joint_type="cocoplus", **kw):
    key = (device, nv, joint_type, tuple(sorted(kw.items())))
    if key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        eng = HmmrEngine(None, _model(nv, **kw), device=device, joint_type=joint_type)
        assert eng.sc.dirs_split and eng.sc.vpad == (nv + 255) // 256 * 256                # form 0 is the split kernel
        _ENGINES[key] = eng
    return _ENGINES[key]


def _flags(clear=True):
    torch.cuda.synchronize()
    v = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(v), int(clear)), "hmmr_run_flags")
    return int(v.value)


@pytest.fixture(autouse=True)
def _clean_flags(gpu_device):
    """every test starts with clear run flags and must leave them clear (the flag tests read-and-clear what they raise)"""
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
    print("\nsmpl-sweep summary: %d tests, %.1f s wall (references included)" % (_STATS["tests"], time.time() - _STATS["t0"]))
    for (k, form), (r, tag) in sorted(_STATS["ratio"].items()):
        print("smpl-sweep summary: largest err / E32 of %-6s form %d: %5.2f (%s)" % (k, form, r, tag))
    _ENGINES.clear()


@functools.lru_cache(maxsize=None)
def _family(name):
    """the cases whose float32-against-float64 error makes one bound"""
    group, fam = name.split("/")
    if group == "a":        # instance counts on the 170-vertex model
        return tuple(S.Case(_model(170), *S.inputs(m, 1000 + m, fam), family=fam, name="nv170 m%d" % m) for m in M_LIST)
    if group == "b":        # vertex counts; the few-vertex models are pooled with their neighbours
        return tuple(S.Case(_model(nv), *S.inputs(m, 2000 + nv, fam), family=fam, name="nv%d m%d" % (nv, m)) for nv in NV_LIST for m in (5, 33))
    if group == "c":        # skinning widths and keypoint regressors
        return tuple(S.Case(_model(nv, **kw), *S.inputs(33, 3000 + i, fam), family=fam, joint_type=jt, name=tag)
                     for i, (tag, nv, jt, kw) in enumerate(C_CASES))
    if group == "g":        # record mode
        return tuple(_record_case(R, n) for R in (1, 3, 8) for n in (1, 21, 33))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _bounds(name):
    return S.bounds(_family(name))


# ---------------------------------------------------------------------------------------------------------------- helpers
def _run_dev(eng, form, theta, beta, cams, want_rs=True):
    from human_dynamics_amd.engine import set_debug
    try:
        set_debug(smpl_blend_mfma=form)
        out = eng.smpl(theta, beta, cams, want_rs=want_rs)
    finally:
        set_debug()
    return dict(zip(S.OUTPUTS, out))


def _np(out):
    return {k: (None if v is None else v.reshape(v.shape[0], -1, v.shape[-1] if k != "Rs" else 9).cpu().numpy()) for k, v in out.items()}


def _run(eng, form, case, want_rs=True):
    return _np(_run_dev(eng, form, case.theta, case.beta, case.cams, want_rs))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check(tag, form, got, ref, bnd, standard):
    """verts, joints, kps, Rs one by one against float64, inside the family's bound"""
    for k in S.OUTPUTS:
        if got[k] is None or ref[k] is None:
            continue
        want = ref[k].reshape(got[k].shape)
        assert np.isfinite(got[k]).all(), (tag, form, k)
        err = float(np.abs(got[k].astype(np.float64) - want).max())
        e = bnd[1][k] / S.FACTOR
        ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("smpl-sweep %-28s form %d %-6s err %.3e  E32 %.3e  ratio %5.2f  bound %.3e" % (tag, form, k, err, e, ratio, bnd[form][k]))
        if ratio > _STATS["ratio"].get((k, form), (-1.0, ""))[0]:
            _STATS["ratio"][(k, form)] = (ratio, tag)
        assert err <= bnd[form][k], (tag, form, k, err, bnd[form][k])
        if standard:
            assert err < S.LEGACY_BOUND, (tag, form, k, err)


def _guarded_rows(rows, ld, device):
    """[rows + 2, ld] floats that all hold the GUARD pattern, and the view of its inner rows that a call writes into"""
    full = torch.full((rows + 2, ld), GUARD, dtype=torch.int32, device=device).view(torch.float32)
    return full, full[1:rows + 1]


def _untouched(full, field_mask):
    """every float outside the fields -- the row in front, the row behind, the gaps -- still holds the GUARD bits"""
    got = full.view(torch.int32).cpu().numpy()
    keep = np.ones(got.shape, bool)
    keep[1:-1, field_mask] = False
    return bool((got[keep] == GUARD).all())


def _strided_call(eng, form, case, V, K):
    """hmmr_smpl_fwd_strided into rows with guard floats in front of, between and behind the fields, at odd float offsets"""
    from human_dynamics_amd.engine import set_debug
    off, o = {}, 5
    for k, n, gap in (("verts", 3 * V, 3), ("joints", 3 * K, 7), ("kps", 2 * K, 1), ("Rs", 216, 4)):
        off[k] = (o, n)
        o += n + gap
    ld = o | 1                                               # an odd row length: a field's alignment changes from row to row
    full, rows = _guarded_rows(case.m, ld, eng.device)
    dev = [eng.to_device(x) for x in (case.theta, case.beta, case.cams)]
    try:
        set_debug(smpl_blend_mfma=form)
        eng.smpl_into(dev[0], dev[1], dev[2], rows, off["verts"][0], off["joints"][0], off["kps"][0], off["Rs"][0])
    finally:
        set_debug()
    mask = np.zeros(ld, bool)
    for a, n in off.values():
        mask[a:a + n] = True
    host = rows.cpu().numpy()
    width = {"verts": 3, "joints": 3, "kps": 2, "Rs": 9}
    return {k: host[:, a:a + n].reshape(case.m, -1, width[k]) for k, (a, n) in off.items()}, _untouched(full, mask)


# ---------------------------------------------------------------------------------------------------------------- a. instance counts
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", M_LIST)
def test_instance_counts(m, form, gpu_device):
    """the blockings of 8 (pose kernel), 16 in fours (vector form) and 32 in half-wave fours (MFMA forms) around every edge, on a
    170-vertex model: a whole wave + a ragged wave in the second tile + two waves of padding, short skinning rows"""
    eng = _engine(gpu_device, 170)
    for fam in FAMILIES:
        case = _family("a/" + fam)[M_LIST.index(m)]
        got = _run(eng, form, case)
        _check("a %s %s" % (case.name, fam), form, got, case.ref(), _bounds("a/" + fam), fam == "standard")
        into, untouched = _strided_call(eng, form, case, 170, 25)
        assert untouched, (m, form, fam)
        for k in S.OUTPUTS:                                  # the strided entry point runs the same kernels: the same bits
            assert _same_bits(got[k], into[k]), (m, form, fam, k)


# ---------------------------------------------------------------------------------------------------------------- b. vertex counts
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nv", NV_LIST)
def test_vertex_counts(nv, form, gpu_device):
    """nv below one wave, at and around the 32 / 128 / 256 edges; nv % 256 in 1..128 leaves the split form a tile that is all padding
    (its `v0 >= nv` skip and the nv - 1 clamp of the weight rows)"""
    eng = _engine(gpu_device, nv)
    for fam in FAMILIES:
        for case in _family("b/" + fam):
            if case.model is not _model(nv):
                continue
            got = _run(eng, form, case)
            _check("b %s %s" % (case.name, fam), form, got, case.ref(), _bounds("b/" + fam), fam == "standard")
            into, untouched = _strided_call(eng, form, case, nv, 25)
            assert untouched, (nv, form, fam, case.m)
            assert all(_same_bits(got[k], into[k]) for k in S.OUTPUTS), (nv, form, fam, case.m)


def test_full_size_model_on_the_sweep_recipe(gpu_device):
    """6890 vertices (one ragged wave of 10 lanes) with the heavy pose-blend basis: every one of the 218 basis rows counts"""
    eng = _engine(gpu_device, 6890)
    case = S.Case(_model(6890), *S.inputs(37, 6890), name="nv6890 m37")
    bnd = S.bounds([case])
    outs = {}
    for form in FORMS:
        outs[form] = _run(eng, form, case)
        _check("b " + case.name, form, outs[form], case.ref(), bnd, True)
    assert _same_bits(outs[0]["Rs"], outs[1]["Rs"]) and _same_bits(outs[0]["Rs"], outs[2]["Rs"])


# ---------------------------------------------------------------------------------------------------------------- c. widths, regressors
C_CASES = (
    ("nnz1 nk25", 100, "cocoplus", dict(nnz=1, nk=25, short=False)),
    ("nnz4s nk1", 100, "cocoplus", dict(nnz=4, nk=1)),
    ("nnz24s nk14", 100, "cocoplus", dict(nnz=24, nk=14)),
    ("nnz24s nk25 lsp", 100, "lsp", dict(nnz=24, nk=25)),
    ("nnz4s empty+long", 300, "cocoplus", dict(nnz=4, nk=25, empty=True, long=True)),
)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("idx", range(len(C_CASES)), ids=[c[0].replace(" ", "-") for c in C_CASES])
def test_skinning_widths_and_keypoint_regressors(idx, form, gpu_device):
    tag, nv, jt, kw = C_CASES[idx]
    eng = _engine(gpu_device, nv, joint_type=jt, **kw)
    nk = 14 if jt == "lsp" else kw["nk"]
    assert (eng.sc.lbs_nnz, eng.sc.num_kps) == (kw["nnz"], nk)
    for fam in FAMILIES:
        case = _family("c/" + fam)[idx]
        got = _run(eng, form, case)
        assert got["joints"].shape == (33, nk, 3) and got["kps"].shape == (33, nk, 2)
        _check("c %s %s" % (tag, fam), form, got, case.ref(), _bounds("c/" + fam), fam == "standard")
        if kw.get("empty"):
            # a keypoint without a vertex: the joint is exactly 0 and the keypoint exactly s * t (one float32 product)
            s, t = case.cams[:, 0:1], case.cams[:, 1:3]
            assert not _bits(got["joints"][:, 12]).any()
            assert _same_bits(got["kps"][:, 12], (s * (np.float32(0) + t)).astype(np.float32))
        # kps not requested, Rs not requested: the same verts and joints
        bare = _np(_run_dev(eng, form, case.theta, case.beta, None, want_rs=False))
        assert bare["kps"] is None and bare["Rs"] is None
        assert _same_bits(bare["verts"], got["verts"]) and _same_bits(bare["joints"], got["joints"])


# ---------------------------------------------------------------------------------------------------------------- d. strided inputs
@pytest.mark.parametrize("form", FORMS)
def test_strided_inputs_equal_contiguous_copies(form, gpu_device):
    """theta, beta and cams as column views of one [m, 85] tensor (row stride 85, the omega layout) against contiguous copies"""
    eng = _engine(gpu_device, 170)
    th, be, ca = S.inputs(37, 41)
    om = torch.from_numpy(np.concatenate([ca, th, be], 1)).to(gpu_device)
    views = (om[:, 3:75], om[:, 75:85], om[:, 0:3])
    assert all(v.stride(0) == 85 and not v.is_contiguous() for v in views)
    a = _np(_run_dev(eng, form, *views))
    b = _np(_run_dev(eng, form, *[v.contiguous() for v in views]))
    c = _np(_run_dev(eng, form, th, be, ca))
    for k in S.OUTPUTS:
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), (form, k)


# ---------------------------------------------------------------------------------------------------------------- e. position independence
@pytest.mark.parametrize("form", FORMS)
def test_an_instance_does_not_depend_on_its_position(form, gpu_device):
    eng = _engine(gpu_device, 170)
    x = [a[5:6] for a in S.inputs(8, 51)]                    # the probe row
    alone = _run(eng, form, S.Case(_model(170), *x))
    for m, pos in ((37, 36), (70, 40), (70, 0), (33, 31), (33, 32)):
        batch = [a.copy() for a in S.inputs(m, 52 + m)]
        for a, row in zip(batch, x):
            a[pos] = row[0]
        got = _run(eng, form, S.Case(_model(170), *batch))
        for k in S.OUTPUTS:
            assert _same_bits(got[k][pos:pos + 1], alone[k]), (form, m, pos, k)
    # a batch against the same rows run as two halves
    th, be, ca = S.inputs(70, 53)
    whole = _run(eng, form, S.Case(_model(170), th, be, ca))
    for lo, hi in ((0, 35), (35, 70)):
        part = _run(eng, form, S.Case(_model(170), th[lo:hi], be[lo:hi], ca[lo:hi]))
        for k in S.OUTPUTS:
            assert _same_bits(whole[k][lo:hi], part[k]), (form, lo, k)


# ---------------------------------------------------------------------------------------------------------------- f. the multi-tile loop
@pytest.mark.parametrize("nv,m,want_vpw,want_groups", [
    (300, 65, 1, [1, 1, 1, 1]),
    (6890, 289, 2, [2] * 27),                                # vpw divides the 54 tiles
    (1100, 3265, 3, [3, 3, 3, 1]),                           # 10 tiles in groups of 3: the last group is clipped (t1 = vtiles) ...
    (1200, 3265, 3, [3, 3, 3, 1]),                           # ... there an all-padding tile, here one with 48 vertices
], ids=["vpw1", "vpw2-divides", "vpw3-clipped", "vpw3-clipped-live"])
def test_split_form_walks_several_tiles_per_workgroup(nv, m, want_vpw, want_groups, gpu_device):
    """smpl_verts_split_kernel keeps its 32 instances' records in LDS and walks vpw vertex tiles; vpw > 1 needs more than 512
    workgroups.  The case must give the vpw it is meant to give (a change of the launch rule fails here, it does not empty the test);
    every instance is compared bit for bit with the same rows in calls of at most 256 instances, where vpw = 1 (the kernel's comment
    promises the same bits), and every 32nd instance and the last two 32-blocks with float64."""
    vpw, tiles = S.split_vpw(nv, m)
    assert vpw == want_vpw and [min(vpw, tiles - t) for t in range(0, tiles, vpw)] == want_groups
    assert S.split_vpw(nv, 256)[0] == 1
    eng = _engine(gpu_device, nv)
    th, be, ca = [torch.from_numpy(a).to(gpu_device) for a in S.inputs(m, 6000 + nv)]
    whole = _run_dev(eng, 0, th, be, ca)
    for a in range(0, m, 256):
        b = min(m, a + 256)
        part = _run_dev(eng, 0, th[a:b], be[a:b], ca[a:b])
        for k in S.OUTPUTS:
            assert torch.equal(whole[k][a:b].view(torch.int32), part[k].view(torch.int32)), (nv, m, a, k)
    idx = np.array(sorted(set(range(0, m, 32)) | set(range(max(0, (m - 1) // 32 * 32 - 32), m))))
    case = S.Case(_model(nv), th.cpu().numpy()[idx], be.cpu().numpy()[idx], ca.cpu().numpy()[idx], name="nv%d m%d vpw%d" % (nv, m, vpw))
    pick = torch.from_numpy(idx).to(gpu_device)
    _check("f " + case.name, 0, _np({k: v[pick] for k, v in whole.items()}), case.ref(), S.bounds([case]), True)


# ---------------------------------------------------------------------------------------------------------------- g. record mode
REC_FIELDS = ("cams", "joints", "kps", "poses", "shapes", "verts", "omegas")       # the order of hmmr_smpl_fwd_records' offsets
REC_NV, REC_NK = 70, 25                                      # two whole waves (the 16-byte store route) and a ragged one


def _record_case(R, n):
    """container r, frame i = instance r n + i; every container projects with container 0's camera of the same frame"""
    th, be, ca = S.inputs(R * n, 7000 + 10 * R + n)
    c = S.Case(_model(REC_NV), th, be, np.tile(ca[:n], (R, 1)), name="R%d n%d" % (R, n))
    c.omegas = np.concatenate([ca, th, be], 1).reshape(R, n, 85)
    return c


def _record_layout(R):
    """field offsets chosen to hurt: a different field order per container, gaps of 1..3 floats between all fields (so the offsets
    run through every residue mod 4), a gap at the row start and at the row end"""
    size = dict(cams=3, joints=3 * REC_NK, kps=2 * REC_NK, poses=216, shapes=10, verts=3 * REC_NV, omegas=85)
    o, offs = 3, []
    for r in range(R):
        order = REC_FIELDS[r % 7:] + REC_FIELDS[:r % 7]
        order = order[::-1] if r % 2 else order
        row = {}
        for j, f in enumerate(order):
            row[f] = o
            o += size[f] + 1 + (r + 2 * j) % 3
        offs.append(row)
    return offs, size, (o + 2) | 1                        # an odd row length: a field's alignment changes from frame to frame


@pytest.mark.parametrize("form", (0, 2))
@pytest.mark.parametrize("n", (1, 21, 33))
@pytest.mark.parametrize("R", (1, 3, 8))
def test_record_mode_against_float64(R, n, form, gpu_device):
    from human_dynamics_amd.engine import set_debug
    eng = _engine(gpu_device, REC_NV)
    case = [c for c in _family("g/standard") if c.name == "R%d n%d" % (R, n)][0]
    offs, size, ld = _record_layout(R)
    assert ld % 2 == 1 and offs[0]["verts"] % 2 == 1                                   # 16-byte stores at odd float offsets
    full, rows = _guarded_rows(n, ld, gpu_device)
    om = torch.from_numpy(case.omegas).to(gpu_device)
    try:
        set_debug(smpl_blend_mfma=form)
        eng.smpl_records(om, rows, [[o[f] for f in REC_FIELDS] for o in offs])
    finally:
        set_debug()
    mask = np.zeros(ld, bool)
    for o in offs:
        for f in REC_FIELDS:
            assert not mask[o[f]:o[f] + size[f]].any()                                  # the layout's fields do not overlap
            mask[o[f]:o[f] + size[f]] = True
    assert _untouched(full, mask), (R, n, form)
    host = rows.cpu().numpy()
    field = lambda f, w: np.concatenate([host[:, o[f]:o[f] + size[f]].reshape(n, -1, w) for o in offs])      # [R n, ., w]
    got = {"verts": field("verts", 3), "joints": field("joints", 3), "kps": field("kps", 2), "Rs": field("poses", 9)}
    _check("g %s" % case.name, form, got, case.ref(), _bounds("g/standard"), True)
    flat = case.omegas.reshape(R * n, 85)
    assert _same_bits(field("omegas", 85)[:, 0], flat)
    assert _same_bits(field("shapes", 10)[:, 0], flat[:, 75:85])
    assert _same_bits(field("cams", 3)[:, 0], np.tile(case.omegas[0, :, :3], (R, 1)))   # container 0's camera in every container
    # ... and the same bits as the plain call on the same instances (theta, beta of the container, camera of container 0)
    plain = _run(eng, form, case)
    for k in S.OUTPUTS:
        assert _same_bits(got[k], plain[k]), (R, n, form, k)


# ---------------------------------------------------------------------------------------------------------------- h. stale scratch
@pytest.mark.parametrize("form", FORMS)
def test_a_bad_call_leaves_nothing_behind_in_the_workspace(form, gpu_device):
    """The vertex kernels read feature rows up to m rounded up to 32 (16 in the vector form) out of a grow-only workspace.  After a
    saturating call and a NaN call of 64 instances, calls of 33 and 17 instances raise no flag and give the bits of an engine that
    never saw the bad calls."""
    from human_dynamics_amd.engine import HmmrEngine
    good = {m: S.Case(_model(170), *S.inputs(m, 8000 + m)) for m in (33, 17)}
    fresh = HmmrEngine(None, _model(170), device=gpu_device)
    want = {m: _run(fresh, form, c) for m, c in good.items()}
    assert _flags() == 0
    eng = HmmrEngine(None, _model(170), device=gpu_device)
    th, _, ca = S.inputs(64, 8064)
    for bad in (300.0, float("nan")):
        out = _run(eng, form, S.Case(_model(170), th, np.full((64, 10), bad, np.float32), ca))
        fl = _flags()
        if form == 0:
            assert fl == (L.FLAG_SATURATED if bad == bad else L.FLAG_SATURATED | L.FLAG_NAN), (bad, fl)
        else:                                                # the fp32 forms clamp nothing and have no flag: a NaN stays a NaN
            assert fl == 0 and (bad == bad or np.isnan(out["verts"]).all())
        for m in (33, 17):
            got = _run(eng, form, good[m])
            assert _flags() == 0, (form, bad, m)
            for k in S.OUTPUTS:
                assert _same_bits(got[k], want[m][k]), (form, bad, m, k)


# ---------------------------------------------------------------------------------------------------------------- i. run flags
def test_split_form_flags_the_fp16_range_of_its_features(gpu_device):
    """features are scaled by 2^8 before they are split: |beta| = 255 (65280) is inside the fp16 range, 256 (65536 > 65504) is not"""
    eng = _engine(gpu_device, 170)
    th, be, ca = S.inputs(37, 91)
    sign = np.where(np.arange(10) % 2 == 0, 1.0, -1.0).astype(np.float32)
    edge = S.Case(_model(170), th, np.tile(255.0 * sign, (37, 1)).astype(np.float32) * np.where(np.arange(37) % 2, -1, 1)[:, None].astype(np.float32),
                  ca, name="beta +-255")
    got = _run(eng, 0, edge)
    assert _flags() == 0
    _check("i " + edge.name, 0, got, edge.ref(), S.bounds([edge]), False)
    clean = _run(eng, 0, S.Case(_model(170), th, be, ca))
    assert _flags() == 0
    for pos in (0, 31, 32, 36):                               # a live instance raises the flag wherever it sits
        for val in (256.0, -256.0):
            b = be.copy()
            b[pos, 3] = val
            out = _run(eng, 0, S.Case(_model(170), th, b, ca))
            assert _flags() == L.FLAG_SATURATED, (pos, val)
            others = np.arange(37) != pos
            for k in S.OUTPUTS:                              # ... and touches nobody else
                assert _same_bits(out[k][others], clean[k][others]), (pos, val, k)


@pytest.mark.parametrize("what", ("theta", "beta"))
def test_split_form_reports_a_nan_as_a_nan(what, gpu_device):
    """include/hmmr_hip.h: HMMR_FLAG_NAN together with HMMR_FLAG_SATURATED when the value a split store clamped was a NaN.  The first run
    of this test read HMMR_FLAG_SATURATED alone for a NaN in theta and in beta alike: smpl_verts_split_kernel tested its features with
    split_overflows() only.  It now tracks the NaN beside it (no output bit moved)."""
    eng = _engine(gpu_device, 170)
    th, be, ca = S.inputs(37, 92)
    clean = _run(eng, 0, S.Case(_model(170), th, be, ca))
    for pos in (0, 33, 36):
        t, b = th.copy(), be.copy()
        if what == "theta":
            t[pos, 7] = np.nan
        else:
            b[pos, 9] = np.nan
        out = _run(eng, 0, S.Case(_model(170), t, b, ca))
        assert _flags() == (L.FLAG_NAN | L.FLAG_SATURATED), (what, pos)
        others = np.arange(37) != pos
        for k in S.OUTPUTS:
            assert _same_bits(out[k][others], clean[k][others]), (what, pos, k)


@pytest.mark.parametrize("form", (1, 2))
def test_fp32_forms_pass_a_nan_through_and_raise_nothing(form, gpu_device):
    eng = _engine(gpu_device, 170)
    th, be, ca = S.inputs(37, 93)
    clean = _run(eng, form, S.Case(_model(170), th, be, ca))
    for what in ("theta", "beta"):
        for pos in (0, 33):
            t, b = th.copy(), be.copy()
            if what == "theta":
                t[pos, 7] = np.nan
            else:
                b[pos, 9] = np.nan
            out = _run(eng, form, S.Case(_model(170), t, b, ca))
            assert _flags() == 0, (form, what, pos)
            assert np.isnan(out["verts"][pos]).all() and np.isnan(out["joints"][pos]).all() and np.isnan(out["kps"][pos]).all()
            others = np.arange(37) != pos
            for k in S.OUTPUTS:
                assert _same_bits(out[k][others], clean[k][others]), (form, what, pos, k)
