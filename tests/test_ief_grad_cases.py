"""The IEF backward's cases on the host (tests/ief_grad_cases.py): the oracle is pinned to tail_cases.compose_ief, every case's mask meets the
conditions on its cleared units, a dropped term of the backward cannot pass the bound, hmmr_ief_fwd_train / hmmr_ief_bwd refuse bad calls
with -1 and a message in front of any launch, the workspace is the stated layout, and the bank converts to the checkpoint's shapes and back."""
import ctypes as C

import numpy as np
import pytest
import torch

from human_dynamics_amd import _lib
import ief_grad_cases as IC
import tail_cases as TC


@pytest.mark.parametrize("width,from_pred,stages,R", [(72, True, 3, 3), (75, True, 3, 3), (72, False, 3, 3), (75, False, 1, 3), (72, True, 1, 8), (72, True, 3, 1)])
def test_oracle_without_mask_is_the_composed_reference(width, from_pred, stages, R):
    m = 9
    keys = (0,) + tuple(sorted(IC.DELTAS_OF[R]))
    strips, start = TC.strips_input(m, 21), TC.omega_rows(m, 21)
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    with torch.no_grad():
        got = IC.forward(IC.params(width, keys, torch.float64, False), t(strips), t(start), None, 1.0, stages, width, from_pred).numpy()
    ref = TC.ref_ief(strips, keys[1:], "f32", stages, width, from_pred, start)
    assert got.shape == ref.shape == (R, m, 85)
    assert float(np.abs(got - ref).max()) <= 1e-12
    # ... and an all-ones mask with keep_scale 1 is the same function
    with torch.no_grad():
        ones = IC.forward(IC.params(width, keys, torch.float64, False), t(strips), t(start), torch.ones(R, stages, 2, m, 1024, dtype=torch.float64), 1.0,
                          stages, width, from_pred).numpy()
    assert np.array_equal(ones, got)


def test_the_cases_cover_every_axis_at_m33_R3():
    at = [c for c in IC.CASES if (c.m, c.R) == (33, 3)]
    assert {c.stages for c in at} == {1, 3} and {c.width for c in at} == {72, 75} and {c.from_pred for c in at} == {True, False}
    assert {c.start for c in at} == {"rows", None} and {c.keep for c in at} == {"half", "ones"}
    assert {c.m for c in IC.CASES} == {1, 7, 33, 86, 160} and {c.R for c in IC.CASES} == {1, 2, 3, 8}
    assert sum(c.m == 160 for c in IC.CASES) == 1 and [c.m for c in IC.CASES if c.R == 8] == [7]
    assert len({c.name for c in IC.CASES}) == len(IC.CASES)


@pytest.mark.parametrize("case", IC.CASES, ids=lambda c: c.name)
def test_cleared_units_are_few_and_the_iteration_ends(case):
    pc = IC.prepared(case)
    print("%s: tau %.3e, %d of %d units cleared (%.2e) in %d round(s)" % (case.name, pc["tau"], pc["cleared"], pc["units"], pc["cleared"] / pc["units"], pc["rounds"]))
    assert pc["cleared"] <= IC.MAX_CLEARED * pc["units"]
    assert pc["rounds"] <= IC.MAX_ROUNDS
    inp = IC.inputs(case)
    assert not ((pc["keep"] != 0) & (inp["keep0"] == 0)).any()                     # only cleared, never set
    a = IC._pre(case, inp, pc["keep"], torch.float64).reshape(pc["keep"].shape)
    assert not ((np.abs(a) <= pc["tau"]) & (pc["keep"] != 0)).any()                # no unmasked unit is ambiguous
    # float32 and float64 agree on the sign of every unit that counts
    a32 = IC._pre(case, inp, pc["keep"], torch.float32).reshape(pc["keep"].shape)
    assert np.array_equal((a32 > 0) & (pc["keep"] != 0), (a > 0) & (pc["keep"] != 0))


def test_m7_is_the_head_of_m33():
    a, b = IC.prepared(IC.BY_NAME["m7_R3"]), IC.prepared(IC.BY_NAME["m33_R3"])
    assert np.array_equal(a["strips"], b["strips"][:7]) and np.array_equal(a["start"], b["start"][:7])
    assert np.array_equal(a["d_omegas"], b["d_omegas"][:, :7]) and np.array_equal(a["keep"], b["keep"][:, :, :, :7])


def test_null_keep_case_has_no_ambiguous_unit():
    case, tried, tau = IC.null_case()
    print("null_keep: seed %d after %d tried, tau %.3e" % (case.seed, tried, tau))
    assert tried <= IC.MAX_NULL_SEEDS and (case.m, case.R) == (5, 1)
    b = IC.null_bounds()
    assert all(v > 0 for k, v in b.items() if not k.startswith("delta/")) and not any(k.startswith("delta/") for k in b)


def test_bounds_are_positive_and_small():
    for group in sorted({IC.group_of(c) for c in IC.CASES}, key=str):
        e = IC.e32(group)
        ref = {}
        for c in IC.cases_of(group):
            for k, v in IC.quantities(IC.reference(c)).items():
                ref[k] = max(ref.get(k, 0.0), max(float(np.abs(a).max()) for a in v))
        for k in sorted(e):
            print("%-40s %-22s E32 %.3e  max |ref| %.3e" % (group, k, e[k], ref[k]))
            assert 0.0 < e[k] < 1e-3 * ref[k], (group, k, e[k], ref[k])


@pytest.mark.parametrize("cot", ["present", "delta_pose", "delta_beta"])
def test_each_cotangent_alone_reaches_its_outputs_by_a_thousand_bounds(cot):
    """a dropped term cannot pass: with one cotangent alone -- the present d_omega, one delta's pose columns, one delta's beta columns -- every
    output it reaches holds a gradient at least 1000 bounds large"""
    case = IC.BY_NAME["m33_R3"]
    pc, bound = IC.prepared(case), IC.bounds(case)
    d = np.zeros_like(pc["d_omegas"])
    if cot == "present":
        d[0] = pc["d_omegas"][0]
    elif cot == "delta_pose":
        d[2, :, 3:75] = pc["d_omegas"][2, :, 3:75]
    else:
        d[1, :, 75:] = pc["d_omegas"][1, :, 75:]
    res = IC.quantities(IC.autograd(case, pc, pc["keep"], torch.float64, d_omegas=d))
    reached = ["d_strips", "d_omega_start"] + ["present/" + n for n in IC.NAMES]
    if cot == "delta_pose":
        for n in IC.NAMES:                                   # the delta regressor that got the cotangent (index 1 of the delta list); the other one gets nothing
            g = res["delta/" + n]
            assert float(np.abs(g[1]).max()) >= 1000 * bound["delta/" + n], (n, float(np.abs(g[1]).max()), bound["delta/" + n])
            assert not g[0].any()
    else:
        assert not any(g.any() for n in IC.NAMES for g in res["delta/" + n])
    for k in reached:
        big = max(float(np.abs(a).max()) for a in res[k])
        print("%-12s %-20s max |g| %.3e = %.0f bounds" % (cot, k, big, big / bound[k]))
        assert big >= 1000 * bound[k], (cot, k, big, bound[k])


@pytest.mark.parametrize("B,T", IC.CHAIN_BT)
def test_chain_case_meets_its_conditions(B, T):
    """the chain to the losses: few cleared units, loss_cases' residual condition (asserted by the builder), no gradient into the delta
    regressors (the present container's loss does not read them), positive bounds"""
    c = IC.chain_case(B, T)
    print("%s: tau %.3e, %d of %d units cleared in %d round(s)" % (c.name, c.tau, c.cleared, c.keep.size, c.rounds))
    assert c.cleared <= IC.MAX_CLEARED * c.keep.size and c.rounds <= IC.MAX_ROUNDS
    r = c.result()
    assert all(not g[n].any() for g in r["grads"][1:] for n in IC.NAMES)
    b = IC.chain_bounds(c)
    for k, v in IC.chain_quantities(r).items():
        print("%s %-20s bound %.3e  max |ref| %.3e" % (c.name, k, b[k], float(np.abs(v[0]).max())))
        assert 0.0 < b[k] < 1e-3 * float(np.abs(v[0]).max())


def test_descent_reference_falls_at_every_step():
    d64, bound = IC.descent_reference()
    print("descent float64:", " ".join("%.4f" % x for x in d64))
    print("descent bound:  ", " ".join("%.1e" % x for x in bound))
    assert len(d64) == IC.DESCENT_STEPS + 1 == len(bound)
    assert all(b < a for a, b in zip(d64, d64[1:])) and d64[-1] < 0.5 * d64[0]
    assert all(0.0 < b < 1e-5 * x for b, x in zip(bound, d64))


# ---------------------------------------------------------------------------------------------------------------- the C entry points, no device
P = [0x10000 * (i + 1) for i in range(12)]
BIG = 1 << 40


def _bank(dt=_lib.HMMR_F32, R=3, S=3, nd=(85, 72, 72, 72, 72, 72, 72, 72), no_optcam=0, scale=False):
    """a syntactically valid bank with dummy (never dereferenced) pointers"""
    iw = _lib.IefWeights()
    iw.dtype, iw.num_regressors, iw.num_stages, iw.no_optcam, iw.mean_theta = dt, R, S, no_optcam, P[3]
    for r in range(_lib.MAX_REGRESSORS):
        g = iw.reg[r]
        g.nd = nd[r]
        for lay in ("fc1_phi", "fc1_theta", "fc2", "fc3"):
            getattr(g, lay).w = P[4]
            if lay != "fc1_theta":
                getattr(g, lay).shift = P[5]
        if scale:
            g.fc2.scale = P[6]
    return iw


def _refused(lib, rc, *words):
    msg = lib.hmmr_last_error()
    assert rc == -1 and msg, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_fwd_train_refuses_before_anything_is_queued():
    lib = _lib.load()

    def call(iw=None, w=True, strips=P[0], start=None, keep=None, scale=1.0, m=5, omegas=P[1], ws=P[2], ws_bytes=BIG):
        iw = _bank() if iw is None else iw
        return lib.hmmr_ief_fwd_train(C.byref(iw) if w else None, strips, start, keep, scale, m, omegas, ws, ws_bytes, None)

    who = b"hmmr_ief_fwd_train"
    _refused(lib, call(w=False), who, b"null argument")
    for missing in ("strips", "omegas", "ws"):
        _refused(lib, call(**{missing: None}), who, b"null argument")
    for m in (0, -1):
        _refused(lib, call(m=m), who, b"m must be positive")
    for dt in (_lib.HMMR_BF16, _lib.HMMR_F16X3, 3, -1):
        _refused(lib, call(_bank(dt)), who, b"HMMR_F32")
    _refused(lib, call(_bank(scale=True)), who, b"scaled layer")
    for R in (0, -1, _lib.MAX_REGRESSORS + 1):
        _refused(lib, call(_bank(R=R)), who, b"bad num_regressors")
    _refused(lib, call(_bank(S=0)), who, b"bad num_stages")
    _refused(lib, call(_bank(nd=(85,) + (75,) * 7)), who, b"regressor 1 has nd=75 (expected 72)")
    _refused(lib, call(_bank(nd=(72,) * 8)), who, b"regressor 0 has nd=72 (expected 85)")
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        _refused(lib, call(keep=P[7], scale=bad), who, b"keep_scale")
    need = lib.hmmr_ief_bwd_workspace_bytes(5, 3, 3)
    _refused(lib, call(ws_bytes=need - 1), who, b"workspace too small")


def test_bwd_refuses_before_anything_is_queued():
    lib = _lib.load()

    def call(iw=None, w=True, desc=True, ws=P[2], ws_bytes=BIG, outputs=("d_strips",), **kw):
        iw = _bank() if iw is None else iw
        d = _lib.IefBwdDesc()
        d.strips, d.omega_start, d.keep, d.keep_scale, d.m, d.d_omegas = P[0], None, None, 1.0, 5, P[1]
        for k, v in kw.items():
            setattr(d, k, v)
        for o in outputs:
            if o in ("d_strips", "d_omega_start"):
                setattr(d, o, P[8])
            else:
                r, name = o
                setattr(d.reg[r], name, P[9])
        return lib.hmmr_ief_bwd(C.byref(iw) if w else None, C.byref(d) if desc else None, ws, ws_bytes, None)

    who = b"hmmr_ief_bwd"
    _refused(lib, call(desc=False), who, b"null descriptor")
    _refused(lib, call(w=False), who, b"null argument")
    for missing in ("strips", "d_omegas"):
        _refused(lib, call(**{missing: None}), who, b"null argument")
    _refused(lib, call(ws=None), who, b"null argument")
    for m in (0, -7):
        _refused(lib, call(m=m), who, b"m must be positive")
    for dt in (_lib.HMMR_BF16, _lib.HMMR_F16X3):
        _refused(lib, call(_bank(dt)), who, b"HMMR_F32")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(lib, call(keep=P[7], keep_scale=bad), who, b"keep_scale")
    _refused(lib, call(outputs=()), who, b"no output is requested")
    _refused(lib, call(outputs=((5, "d_fc2"),)), who, b"no output is requested")          # regressor 5 of 3 does not exist
    for outputs in (("d_strips",), ("d_omega_start",), ((2, "d_b3"),)):
        _refused(lib, call(outputs=outputs, ws_bytes=lib.hmmr_ief_bwd_workspace_bytes(5, 3, 3) - 1), who, b"workspace too small")


def test_bwd_workspace_is_the_stated_layout():
    lib = _lib.load()
    for m, R, S in ((1, 1, 1), (5, 3, 3), (7, 8, 3), (33, 2, 1), (160, 3, 3), (256, 3, 3)):
        assert lib.hmmr_ief_bwd_workspace_bytes(m, R, S) == IC.bwd_workspace_bytes(m, R, S), (m, R, S)
    for m, R, S in ((0, 3, 3), (-1, 3, 3), (5, 0, 3), (5, _lib.MAX_REGRESSORS + 1, 3), (5, 3, 0)):
        assert lib.hmmr_ief_bwd_workspace_bytes(m, R, S) == 0


def test_bank_converts_to_the_checkpoint_and_back():
    from human_dynamics_amd.ief_bank import NAMES, IefBank
    assert NAMES == IC.NAMES
    for width, deltas in ((72, (-5, 5)), (75, (5,))):
        src = TC.ief_weights(width)
        want = {k: np.asarray(v, np.float32) for k, v in src.items()
                if k == "mean_param" or any(k.startswith(IC.scope_of(d) + "/") for d in (0,) + deltas)}
        bank = IefBank(src, deltas, "cpu")
        got = bank.to_checkpoint()
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k].reshape(got[k].shape)), k
        # another checkpoint goes in and comes out unchanged; the padding stays zero; the tensors are views of the packed memory
        rng = np.random.default_rng(3)
        x = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in got.items()}
        back = bank.load_checkpoint(x).to_checkpoint()
        assert all(np.array_equal(back[k], x[k]) for k in x)
        for r, p in enumerate(bank.params):
            nd = bank.nd[r]
            assert not p["fc1_theta"][:, nd:].any() and not p["fc3"][nd:].any() and not p["b3"][nd:].any()
        blob = bank.store.tensors[-1]
        lo, hi = blob.data_ptr(), blob.data_ptr() + blob.numel()
        assert all(lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= hi for t in bank.tensors())
        assert bank.params[0]["fc2"].data_ptr() == bank.iw.reg[0].fc2.w and bank.params[1]["b3"].data_ptr() == bank.iw.reg[1].fc3.shift
        # a set of gradients converts the same way
        g = bank.like(fill=0)
        g[1]["fc3"][:bank.nd[1]] = 1.0
        ck = bank.to_checkpoint(g)
        assert "mean_param" not in ck and ck[IC.scope_of(deltas[0]) + "/3D_module/fc3/weights"].shape == (1024, bank.nd[1])
        assert ck[IC.scope_of(deltas[0]) + "/3D_module/fc3/weights"].all() and not ck["single_view_ief/3D_module/fc3/weights"].any()
        with pytest.raises(KeyError):
            bank.load_checkpoint({"AZ_FC_block/nope": np.zeros(3, np.float32)})
