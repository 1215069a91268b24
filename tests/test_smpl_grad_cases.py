"""The helper of the SMPL backward tests (tests/smpl_grad_cases.py) and the host side of the new entry points: the restated forward
is the oracle's bit for bit, every single cotangent's gradient towers over the bound, the descent problem of the device test
descends in float64, the workspace query, every refusal of hmmr_smpl_bwd and the by-vertex regressor of hmmr_pack_smpl_grad.
No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import smpl_cases as S
import smpl_grad_cases as G
from human_dynamics_amd import _lib as L
from human_dynamics_amd import packing
from oracle import hmmr_oracle as O


def _all_cases():
    return [c for fam in G.FAMILIES for cases in G.sweep(fam).values() for c in cases] + [G.full_size_case()]


def test_restated_forward_is_the_oracle_bit_for_bit():
    seen = set()
    for c in _all_cases():
        key = (c.nv, tuple(sorted(c.model_kw.items())), c.joint_type, c.family, c.m)
        if key in seen:
            continue
        seen.add(key)
        mdl = c.model if c.joint_type != "lsp" else dict(c.model, cocoplus_regressor=np.ascontiguousarray(c.model["cocoplus_regressor"][:, :14]))
        v, j, r = O.smpl_forward(c.beta, c.theta, mdl, torch.float64)
        k = O.batch_orth_proj_idrot(j, torch.from_numpy(c.cams).to(torch.float64))
        with torch.no_grad():
            got = G.forward(c.model, *[torch.from_numpy(a).to(torch.float64) for a in (c.theta, c.beta, c.cams)], joint_type=c.joint_type)
        for name, want in (("verts", v), ("joints", j), ("kps", k), ("Rs", r)):
            assert torch.equal(got[name], want), (c.name, name)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_every_single_cotangent_towers_over_the_bound(family):
    """for each cotangent alone and each gradient it reaches, max |g64| >= 1000 x FACTOR x E32 of that gradient -- in every case of every
    group, not only in the group's largest: a dropped term cannot hide inside the bound.  Gradients are finite on the rows with
    theta = 0, a half turn and 1e-7."""
    groups = dict(G.sweep(family))
    if family == "standard":
        groups["full"] = (G.full_size_case(),)
    for name, cases in groups.items():
        e = G.e32(cases)
        for k in G.GRADS:
            assert 0.0 < e[k] < 1e-4, (name, k, e[k])                                  # float32 noise, not a broken reference
        for c in cases:
            for k in G.GRADS:
                assert np.isfinite(c.grads()[k]).all() and np.isfinite(c.grads(torch.float32)[k]).all(), (c.name, k)
                for o in G.OUTPUTS:
                    big = float(np.abs(c.grads(only=o)[k]).max())
                    if o in G.REACH[k]:
                        assert big >= G.DOMINANCE * G.FACTOR * e[k], (c.name, k, o, big, e[k])
                    else:
                        assert big == 0.0, (c.name, k, o)
    assert 1.0 <= G.FACTOR <= 8.0


def test_descent_problem_descends_in_float64():
    losses = G.descent_reference()
    assert len(losses) == G.DESCENT_STEPS + 1
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < 0.5 * losses[0], losses


def _host_consts(nv=130, nk=25, nnz=4):
    sc, gc = L.SmplConsts(), L.SmplGradConsts()
    sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = nv, nk, nnz, (nv + 255) // 256 * 256
    sc.dirs = 0x10000
    gc.num_verts, gc.num_kps = nv, nk
    return sc, gc


def test_workspace_query_needs_no_gpu():
    lib = L.load()
    sc, _ = _host_consts(6890)
    q = lambda m: lib.hmmr_smpl_bwd_workspace_bytes(C.byref(sc), m)
    assert q(0) == 0 and q(-3) == 0 and lib.hmmr_smpl_bwd_workspace_bytes(None, 4) == 0
    sizes = [q(m) for m in range(1, 70)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # one {d_feat, d_A} partial per (128-vertex tile, instance) beside the forward's scratch
    assert q(256) >= 54 * 256 * (218 + 288) * 4 + lib.hmmr_smpl_workspace_bytes(256)
    small, _ = _host_consts(50)
    assert 0 < lib.hmmr_smpl_bwd_workspace_bytes(C.byref(small), 8) < q(8)


def test_backward_refuses_what_it_cannot_honour():
    """dummy, never dereferenced device pointers; no device is needed: every refusal happens before a launch"""
    lib = L.load()
    sc, gc = _host_consts()
    P = [0x1000 * (i + 1) for i in range(16)]
    m = 5
    need = lib.hmmr_smpl_bwd_workspace_bytes(C.byref(sc), m)
    names = "c g theta ldt beta ldb cams ldc joints m dv dj dk dr dth dbe dca ws wsb st"
    good = dict(c=C.byref(sc), g=C.byref(gc), theta=P[0], ldt=72, beta=P[1], ldb=10, cams=P[2], ldc=3, joints=P[3], m=m, dv=P[4], dj=P[5], dk=P[6],
                dr=P[7], dth=P[8], dbe=P[9], dca=P[10], ws=P[11], wsb=need, st=None)

    def refused(*words, **kw):
        args = dict(good)
        args.update(kw)
        rc = lib.hmmr_smpl_bwd(*[args[a] for a in names.split()])
        msg = lib.hmmr_last_error()
        assert rc != 0 and msg and b"hmmr_smpl_bwd" in msg, (kw, rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        with pytest.raises(L.HmmrError):
            L.check(rc, "hmmr_smpl_bwd")

    for k in ("c", "g", "theta", "beta", "dth", "dbe", "ws"):
        refused(b"null", **{k: None})
    refused(b"positive", m=0)
    refused(b"positive", m=-1)
    refused(b"no upstream gradient", dv=None, dj=None, dk=None, dr=None)
    refused(b"d_kps", cams=None, dca=None)
    refused(b"d_kps", joints=None)
    refused(b"d_cams", cams=None, dk=None)
    refused(b"workspace too small", wsb=need - 1)
    refused(b"workspace too small", wsb=0)
    for nnz in (0, 25, -1):
        bad, _ = _host_consts(nnz=nnz)
        refused(b"lbs_nnz", c=C.byref(bad))
    other, _ = _host_consts(nv=131)
    refused(b"another model", c=C.byref(other), wsb=1 << 30)


def _ints(ptr, n):
    return np.frombuffer(bytes((C.c_ubyte * (4 * n)).from_address(ptr)), np.int32).copy()


def _floats(ptr, n):
    return np.frombuffer(bytes((C.c_ubyte * (4 * n)).from_address(ptr)), np.float32).copy()


@pytest.mark.parametrize("joint_type", ("cocoplus", "lsp"))
@pytest.mark.parametrize("nv,kw", [(1, {}), (50, {}), (130, {}), (300, dict(empty_col=True, long_cols=True)), (700, {})],
                         ids=["nv1", "nv50", "nv130", "nv300-empty-long", "nv700"])
def test_grad_packer_reproduces_the_regressor_by_vertex(nv, kw, joint_type):
    mdl = S.model(nv, nk=25, nnz=4, seed=nv, short_rows=True, **kw)
    store = packing.DeviceStore("cpu")
    gc = packing.pack_smpl_grad(mdl, store, joint_type)
    kreg = mdl["cocoplus_regressor"][:, :14] if joint_type == "lsp" else mdl["cocoplus_regressor"]
    nk = kreg.shape[1]
    assert (gc.num_verts, gc.num_kps) == (nv, nk)
    ptr = _ints(gc.vk_ptr, nv + 1)
    assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] == int((kreg != 0).sum())
    idx, val = _ints(gc.vk_idx, max(1, ptr[-1])), _floats(gc.vk_val, max(1, ptr[-1]))
    dense = np.zeros_like(kreg)
    for v in range(nv):
        ks = idx[ptr[v]:ptr[v + 1]]
        assert (np.diff(ks) > 0).all() and (ks >= 0).all() and (ks < nk).all()          # ascending keypoint ids, each once
        dense[v, ks] = val[ptr[v]:ptr[v + 1]]
    assert np.array_equal(dense.view(np.int32), np.ascontiguousarray(kreg).view(np.int32))      # exactly
    if kw:
        per_col = (dense != 0).sum(0)
        if joint_type == "cocoplus":
            assert per_col[12] == 0 and per_col[0] == 100 and per_col[24] == 150
        else:
            assert per_col[7] == 48 and per_col[0] == 100
    # the forward's constants are untouched by the new packer: the same header as before for the same model
    sc = packing.pack_smpl(mdl, packing.DeviceStore("cpu"), joint_type)
    assert (sc.num_verts, sc.num_kps) == (gc.num_verts, gc.num_kps)


def test_grad_packer_refuses_an_incomplete_source():
    lib = L.load()
    src = L.SmplSource()
    src.num_verts, src.num_kps = 10, 25
    assert lib.hmmr_pack_smpl_grad_bytes(C.byref(src), 0) == 0 and b"hmmr_pack_smpl_grad_bytes" in lib.hmmr_last_error()
    gc = L.SmplGradConsts()
    assert lib.hmmr_pack_smpl_grad(None, 0, None, 0, None, C.byref(gc)) != 0 and b"hmmr_pack_smpl_grad" in lib.hmmr_last_error()
