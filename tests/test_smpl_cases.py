"""The helper of the SMPL stage sweep (tests/smpl_cases.py) on the host: the models have the properties the device tests rely on,
both packers take every one of them, the chunked reference is the unchunked one, and the sweep's bound is never looser than the
2e-5 the suite already asserts.  No GPU."""
import numpy as np
import pytest
import torch

import smpl_cases as S
from human_dynamics_amd import _lib as L
from human_dynamics_amd import packing

SWEEP_NV = (1, 31, 32, 33, 100, 127, 128, 129, 170, 255, 256, 257, 300, 1100, 1200)


def _ints(ptr, n):
    import ctypes as C
    return np.frombuffer(bytes((C.c_ubyte * (4 * n)).from_address(ptr)), np.int32)


def test_builder_delivers_the_promised_properties():
    m = S.model(300, nk=25, nnz=4, seed=1, short_rows=True, empty_col=True, long_cols=True)
    assert m["v_template"].shape == (300, 3) and m["shapedirs"].shape == (10, 900) and m["posedirs"].shape == (207, 900)
    assert m["J_regressor"].shape == (300, 24) and m["cocoplus_regressor"].shape == (300, 25) and m["lbs_weights"].shape == (300, 24)
    # magnitudes: the pose-blend basis is as heavy as the shape basis
    for k, sigma in (("v_template", 0.3), ("shapedirs", 0.01), ("posedirs", 0.01)):
        assert 0.9 * sigma < m[k].std() < 1.1 * sigma, k
    per_col = (m["cocoplus_regressor"] != 0).sum(0)
    assert per_col[12] == 0 and per_col[0] == 100 and per_col[24] == 150              # empty, two trips, three trips of the 64-lane loop
    assert sorted(set(per_col)) == [0, 48, 100, 150]
    live = per_col > 0
    assert np.allclose(m["cocoplus_regressor"].sum(0)[live], 1.0, atol=1e-6) and np.allclose(m["J_regressor"].sum(0), 1.0, atol=1e-6)
    per_row = (m["lbs_weights"] != 0).sum(1)
    assert sorted(set(per_row)) == [1, 2, 3, 4] and per_row[0] == 4                    # every length; vertex 0 has the full width
    assert np.allclose(m["lbs_weights"].sum(1), 1.0, atol=1e-6)
    dense = S.model(100, nnz=24, seed=1, short_rows=True)
    assert sorted(set((dense["lbs_weights"] != 0).sum(1))) == list(range(1, 25))
    full = S.model(33, nnz=4, seed=1)
    assert set((full["lbs_weights"] != 0).sum(1)) == {4}
    assert set((S.model(1, seed=1)["cocoplus_regressor"] != 0).sum(0)) == {1}         # one vertex: every regressor column is that vertex
    # a different seed or size is a different model; the same arguments the same one
    assert not np.array_equal(S.model(33, seed=1)["v_template"], S.model(33, seed=2)["v_template"])
    assert np.array_equal(S.model(33, seed=1)["posedirs"], S.model(33, seed=1)["posedirs"])


def test_inputs_deliver_the_promised_rows():
    th, be, ca = S.inputs(37, 3, "standard")
    assert th.dtype == be.dtype == ca.dtype == np.float32 and th.shape == (37, 72) and be.shape == (37, 10) and ca.shape == (37, 3)
    assert not th[0, 3:6].any() and tuple(th[1, 6:9]) == (np.float32(np.pi), 0.0, 0.0) and (th[2, 9:12] == np.float32(1e-7)).all()
    assert 0.5 <= ca[:, 0].min() and ca[:, 0].max() <= 1.5
    assert len({r.tobytes() for r in th}) == 37 and len({r.tobytes() for r in be}) == 37 and len({r.tobytes() for r in ca}) == 37
    assert 0.55 < th[3:].std() < 0.65 and 0.9 < be.std() < 1.1
    th, be, ca = S.inputs(64, 3, "wide")
    assert np.linalg.norm(th.reshape(-1, 3), axis=1).max() > 2 * np.pi                 # angles beyond a full turn
    assert 2.7 < th.std() < 3.3 and 4.5 < be.std() < 5.5 and (ca[:, 0] < 0).any() and (ca[:, 0] > 0).any()
    assert np.abs(be).max() * 256 < 65504                                               # no input of the sweep saturates by itself
    for m in (1, 2, 3):                                                                 # the special rows exist only where m allows
        assert S.inputs(m, 0)[0].shape == (m, 72)


@pytest.mark.parametrize("nv", SWEEP_NV)
def test_python_packer_accepts_every_model_of_the_sweep(nv):
    mdl = S.model(nv, nk=25, nnz=4, seed=nv, short_rows=True, empty_col=True, long_cols=nv > 64)
    store = packing.DeviceStore("cpu")
    sc = packing.pack_smpl(mdl, store, impl="py")
    vpad = (nv + 255) // 256 * 256
    assert (sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad) == (nv, 25, 4, vpad) and sc.dirs_split
    kptr = _ints(sc.kreg_ptr, 26)
    assert kptr[12] == kptr[13] and (np.diff(kptr) >= 0).all()                          # the empty column is an empty CSR range
    if nv > 128:
        assert kptr[1] - kptr[0] == 100 and kptr[25] - kptr[24] == min(nv, 150)
    idx = _ints(sc.lbs_idx, nv * 4).reshape(nv, 4)
    assert idx.min() >= 0 and idx.max() < 24
    if nv > 1:
        assert tuple(idx[1, 3:]) == (0,)                                                # a short row is padded with joint 0 (weight 0)
    # the C packer, the one the engine uses, gives the same header for the same model
    sc_c = packing.pack_smpl(mdl, packing.DeviceStore("cpu"), impl="c")
    assert (sc_c.num_verts, sc_c.num_kps, sc_c.lbs_nnz, sc_c.vpad) == (nv, 25, 4, vpad) and sc_c.dirs_split


def test_packers_take_the_other_widths_and_keypoint_counts():
    for nnz, nk, jt, want_nk in ((1, 1, "cocoplus", 1), (24, 14, "cocoplus", 14), (24, 25, "lsp", 14)):
        mdl = S.model(100, nk=nk, nnz=nnz, seed=7, short_rows=nnz > 1)
        for impl in ("py", "c"):
            sc = packing.pack_smpl(mdl, packing.DeviceStore("cpu"), jt, impl=impl)
            assert (sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad) == (100, want_nk, nnz, 256), (nnz, nk, jt, impl)


def test_chunked_reference_equals_the_unchunked_one():
    mdl = S.model(33, seed=5, short_rows=True)
    th, be, ca = S.inputs(7, 5)
    whole = S.reference(mdl, th, be, ca, torch.float64, chunk=7)
    whole32 = S.reference(mdl, th, be, ca, torch.float32, chunk=7)
    for chunk in (1, 3, 4):
        part = S.reference(mdl, th, be, ca, torch.float64, chunk=chunk)
        part32 = S.reference(mdl, th, be, ca, torch.float32, chunk=chunk)
        for k in S.OUTPUTS:
            assert whole[k].shape[0] == 7 and np.array_equal(whole[k], part[k]), (chunk, k)      # the reference: bit for bit
            # the float32 run is the yardstick's noise, not the reference: BLAS sums a one-row product in another order than a
            # several-row one, which moves it by float32 rounding and no more
            assert np.abs(whole32[k] - part32[k]).max() < 1e-6, (chunk, k)
    assert S.reference(mdl, th, be, None)["kps"] is None
    lsp = S.reference(mdl, th, be, ca, joint_type="lsp")
    assert lsp["joints"].shape == (7, 14, 3) and np.array_equal(lsp["joints"], whole["joints"][:, :14])
    # the [N, nv, 4, 4] float64 intermediate of one chunk stays at or below 128 MB
    for nv in (1, 300, 1100, 6890):
        assert S.chunk_rows(nv) >= 1 and S.chunk_rows(nv) * nv * 128 <= 128 << 20


def test_new_bound_is_inside_the_existing_one():
    """4 x E32 + 2e-6 for the `standard` family stays below the 2e-5 that test_smpl_stage_matches_oracle asserts: on the sweep's
    small model, on a 300-vertex one and -- the sizes the issue measured -- on the 6890-vertex one"""
    for nv, m in ((170, 37), (300, 33), (6890, 8)):
        mdl = S.model(nv, seed=nv, short_rows=True)
        th, be, ca = S.inputs(m, nv)
        case = S.Case(mdl, th, be, ca)
        e = S.e32([case])
        b = S.bounds([case])
        print("nv=%d m=%d E32 %s" % (nv, m, {k: "%.2e" % v for k, v in e.items()}))
        for k in S.OUTPUTS:
            assert 0.0 < e[k] < 2e-6, (nv, k, e[k])                                     # float32 noise, not a broken reference
            assert b[1][k] == b[2][k] == S.FACTOR * e[k] and b[0][k] >= b[1][k]
            assert b[0][k] < S.LEGACY_BOUND, (nv, k, b[0][k])
        assert b[0]["verts"] == b[1]["verts"] + 2e-6 and b[0]["Rs"] == b[1]["Rs"]
        assert b[0]["kps"] <= b[1]["kps"] + 2e-6 * 1.5
    assert S.FACTOR <= 8.0
    with pytest.raises(AssertionError):
        S.bounds([case], factor=8.5)


def test_vpw_follows_the_launch_rule():
    assert S.split_vpw(300, 65) == (1, 4)
    assert S.split_vpw(6890, 288) == (1, 54) and S.split_vpw(6890, 289) == (2, 54)
    assert S.split_vpw(1100, 3265) == (3, 10) and S.split_vpw(6890, 897) == (4, 54)
    assert S.split_vpw(1, 1 << 20) == (2, 2)                                            # clamped to the tile count
    assert L.load().hmmr_smpl_workspace_bytes(3265) >= 3296 * (224 + 288) * 4
