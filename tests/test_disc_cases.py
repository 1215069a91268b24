"""The host side of the pose discriminator (no GPU): the oracle of tests/disc_cases.py against the reference's own code, the redraw
condition of its cases, hmmr_pack_disc_pose's layout element by element, the bank's checkpoint round trip, and every refusal of
hmmr_disc_pose_fwd / hmmr_disc_pose_bwd / hmmr_pose_prior (include/hmmr_hip.h, "Pose discriminator") with dummy, never dereferenced
pointers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import disc_cases as D
from human_dynamics_amd import _lib as L
from human_dynamics_amd import build, disc_bank

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return L.load()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_is_the_reference_s_function():
    """forward and the three losses of the oracle equal what src/discriminators.py and src/ops.py give on the same seeded weights
    and 4 + 4 rows (tests/golden/make_disc_golden.py), to 1e-12"""
    gold = np.load(os.path.join(HERE, "golden", "reference_disc_pose.npz"))
    real, fake = D.fixture_rows()
    w = D.weights()
    sums = [np.abs(real.astype(np.float64)).sum() + 3.0 * len(real), np.abs(fake.astype(np.float64)).sum() + 3.0 * len(fake),
            sum(np.abs(v.astype(np.float64)).sum() for v in w.values())]
    assert np.allclose(gold["inputs_sum"], sums, rtol=1e-13, atol=0), "the fixture was made from other seeded inputs"
    P = D.params(torch.float64, False)
    x = torch.tensor(np.concatenate([real, fake]).astype(np.float64))
    with torch.no_grad():
        out = D.forward(P, x)
        ls = D.losses(out[:len(real)], out[len(real):])
    assert out.shape == (8, 24) and np.abs(out.numpy() - gold["out"]).max() <= 1e-12
    assert np.abs(np.array([float(v) for v in ls]) - gold["losses"]).max() <= 1e-12 * np.abs(gold["losses"]).max()
    assert abs(float(ls[1] + ls[2]) - float(gold["d_pose"])) <= 1e-12 * abs(float(gold["d_pose"]))


def test_ops_losses_are_the_oracle_s():
    from human_dynamics_amd import ops
    rng = np.random.Generator(np.random.PCG64(5))
    a, b = torch.tensor(rng.standard_normal((5, 24))), torch.tensor(rng.standard_normal((3, 24)))
    e, dr, df = D.losses(a, b)
    assert float(ops.compute_loss_e_fake(b)) == pytest.approx(float(e), rel=1e-14)
    assert float(ops.compute_loss_d_real(a)) == pytest.approx(float(dr), rel=1e-14)
    assert float(ops.compute_loss_d_fake(b)) == pytest.approx(float(df), rel=1e-14)


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_redraw_cap_holds(case):
    """at most max(2, n / 4) redraws per case, within 4 rounds; no row is left ambiguous"""
    total, rounds = D.redraws(case)
    n = case.n_a + case.n_b
    assert total <= D.max_redraws(n) and rounds <= D.MAX_ROUNDS, (case.name, total, rounds)
    assert not D.ambiguous(np.concatenate(D.rows(case))).any()
    if case.name == "7_0":
        assert np.array_equal(D.rows(case)[0], D.rows(D.BY_NAME["33_0"])[0][:7])


def test_bounds_come_from_the_yardstick():
    e = D.e32()
    assert sorted(e) == sorted(D.QUANTITIES) and all(0 < v < 1e-3 for v in e.values()), e


# ---------------------------------------------------------------------------------------------------------------- the packer
def _marked():
    """checkpoint-named arrays whose every element says where it came from: tensor index * 2^20 + flat index (exact in float32)"""
    out = {}
    for t, (name, shape) in enumerate(sorted(disc_bank.checkpoint_shapes().items())):
        n = int(np.prod(shape))
        out[name] = ((t + 1) * float(1 << 20) + np.arange(n, dtype=np.float64)).reshape(shape).astype(np.float32)
    return out


def test_pack_gives_the_stated_layout_element_by_element(lib):
    """an index marker per tensor, padding zero (include/hmmr_hip.h: conv1 [32][16], conv2 [32][32], heads [32][32], fc1 [1024][1024]
    with K = 736 padded, fc2 [1024][1024], fc_out [128][1024]; every bias padded to a multiple of 128)"""
    w = _marked()
    bank = disc_bank.PoseDiscBank(w, "cpu")
    p = {k: v.numpy() for k, v in bank.params.items()}
    g = lambda k: w["D_pose/" + k]
    want = {k: np.zeros(v.shape, np.float32) for k, v in p.items()}
    want["conv1"][:, :9] = g("D_conv1/weights").reshape(9, 32).T
    want["conv2"][:] = g("D_conv2/weights").reshape(32, 32).T
    for j in range(23):
        want["heads"][j] = g("pose_out_j%d/weights" % j).reshape(32)
        want["bj"][j] = g("pose_out_j%d/biases" % j)[0]
    want["fc1"][:, :736] = g("D_alljoints_fc1/weights").T
    want["fc2"][:] = g("D_alljoints_fc2/weights").T
    want["fc_out"][0] = g("D_alljoints_out/weights").reshape(1024)
    want["bc1"][:], want["bc2"][:], want["b1"][:], want["b2"][:] = g("D_conv1/biases"), g("D_conv2/biases"), g("D_alljoints_fc1/biases"), g("D_alljoints_fc2/biases")
    want["bo"][0] = g("D_alljoints_out/biases")[0]
    for k in disc_bank.NAMES:
        assert np.array_equal(p[k], want[k]), k
    # the bias vectors are padded with zeros to 128 floats, and no two tensors overlap
    base = bank.blob.data_ptr()
    spans = []
    for name, (lay, field), shape in disc_bank.LAYERS:
        off = int(getattr(getattr(bank.dw, lay), field)) - base
        n = int(np.prod(shape)) if len(shape) == 2 else max(128, shape[0])
        tail = bank.blob[off:off + 4 * n].view(torch.float32).numpy()
        assert off % 256 == 0 and not tail[int(np.prod(shape)):].any(), name
        spans.append((off, off + 4 * n))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= bank.blob.numel()
    assert bank.dw.dtype == L.HMMR_F32 and all(not getattr(bank.dw, lay).scale for lay in L.DISC_POSE_LAYERS)


def test_pack_refuses_other_dtypes_and_missing_variables(lib):
    from human_dynamics_amd import packing
    w = D.weights()
    for dt in (L.HMMR_BF16, L.HMMR_F16X3):
        with pytest.raises(ValueError, match="HMMR_F32 only"):
            packing.pack_disc_pose(w, packing.DeviceStore("cpu"), dtype=dt)
    less = {k: v for k, v in w.items() if "pose_out_j22" not in k}
    with pytest.raises(ValueError, match="pose_out_j22"):
        packing.pack_disc_pose(less, packing.DeviceStore("cpu"))
    bad = dict(w)
    bad["D_pose/D_alljoints_fc1/weights"] = np.zeros((735, 1024), np.float32)
    with pytest.raises(ValueError, match="D_alljoints_fc1"):
        packing.pack_disc_pose(bad, packing.DeviceStore("cpu"))


def test_checkpoint_round_trip(lib):
    """to_checkpoint(load_checkpoint(x)) == x in the checkpoint's names and shapes, for weights and for a set of gradients; the
    padding stays zero; unknown names and wrong shapes are refused"""
    bank = disc_bank.PoseDiscBank(D.weights(), "cpu")
    x = _marked()
    bank.load_checkpoint(x)
    back = bank.to_checkpoint()
    assert sorted(back) == sorted(x) and all(back[k].shape == x[k].shape and np.array_equal(back[k], x[k]) for k in x)
    assert {k: v.shape for k, v in back.items()} == disc_bank.checkpoint_shapes()
    p = bank.params
    assert not p["conv1"][:, 9:].any() and not p["heads"][23:].any() and not p["fc1"][:, 736:].any() and not p["fc_out"][1:].any()
    assert not p["bj"][23:].any() and not p["bo"][1:].any()
    like = bank.like(fill=0)
    assert [tuple(like[n].shape) for n in disc_bank.NAMES] == [tuple(t.shape) for t in bank.tensors()]
    grads = {n: torch.arange(t.numel(), dtype=torch.float32).reshape(t.shape) for n, t in bank.params.items()}
    as_ckpt = bank.to_checkpoint(grads)
    other = disc_bank.PoseDiscBank(D.weights(), "cpu").load_checkpoint(as_ckpt)
    again = other.to_checkpoint()
    assert all(np.array_equal(again[k], as_ckpt[k]) for k in as_ckpt)
    with pytest.raises(KeyError):
        bank.load_checkpoint({"D_pose/nothing/weights": np.zeros(3, np.float32)})
    with pytest.raises(ValueError):
        bank.load_checkpoint({"D_pose/D_conv1/weights": np.zeros((9, 32), np.float32)})


# ---------------------------------------------------------------------------------------------------------------- refusals
def _bank(dtype=L.HMMR_F32):
    dw = L.DiscPoseWeights()
    dw.dtype = dtype
    for i, lay in enumerate(L.DISC_POSE_LAYERS):
        getattr(dw, lay).w, getattr(dw, lay).shift = 0x10000 * (i + 1), 0x10000 * (i + 1) + 0x8000
    return dw


def _rows(n, ld=207, ptr=0x200000):
    r = L.Rows()
    r.ptr, r.ld, r.n = ptr, ld, n
    return r


WS, OUT = 0x400000, 0x800000


def test_workspace_query(lib):
    assert lib.hmmr_disc_pose_workspace_bytes(0) == 0 and lib.hmmr_disc_pose_workspace_bytes(-3) == 0
    a, b = lib.hmmr_disc_pose_workspace_bytes(1), lib.hmmr_disc_pose_workspace_bytes(320)
    assert 0 < a < b and b >= 320 * 6 * 1024 * 4


def test_forward_refuses_before_anything_is_queued(lib):
    """dummy pointers: a call that got past its checks would fault"""
    big = 1 << 40
    err = lambda: lib.hmmr_last_error().decode()
    fwd = lambda dw, a, b, out=OUT, ws=WS, nb=big: lib.hmmr_disc_pose_fwd(C.byref(dw) if dw else None, C.byref(a) if a else None,
                                                                          C.byref(b) if b else None, out, ws, nb, None)
    dw = _bank()
    assert fwd(None, _rows(2), None) == -1 and "null argument" in err()
    assert fwd(dw, None, None) == -1 and "null argument" in err()
    assert fwd(dw, _rows(2), None, ws=None) == -1 and "null argument" in err()
    assert fwd(dw, _rows(2), None, out=None) == -1 and "null argument (out)" in err()
    assert fwd(dw, _rows(0), _rows(0)) == -1 and "n_a + n_b" in err()
    assert fwd(dw, _rows(-1), _rows(3)) == -1 and "negative" in err()
    assert fwd(dw, _rows(2, ptr=None), None) == -1 and "rows of a segment" in err()
    assert fwd(dw, _rows(2, ld=206), None) == -1 and "below 207" in err()
    assert fwd(dw, _rows(2), _rows(1, ld=100)) == -1 and "below 207" in err()
    for dt in (L.HMMR_BF16, L.HMMR_F16X3):
        assert fwd(_bank(dt), _rows(2), None) == -1 and "HMMR_F32" in err()
    scaled = _bank()
    scaled.fc2.scale = 0x9000
    assert fwd(scaled, _rows(2), None) == -1 and "scaled layer" in err()
    holed = _bank()
    holed.heads.shift = None
    assert fwd(holed, _rows(2), None) == -1 and "a layer of the bank" in err()
    need = lib.hmmr_disc_pose_workspace_bytes(5)
    assert fwd(dw, _rows(2), _rows(3), nb=need - 1) == -1 and "workspace too small" in err()


def test_backward_and_prior_refuse_before_anything_is_queued(lib):
    big = 1 << 40
    err = lambda: lib.hmmr_last_error().decode()
    dw = _bank()

    def desc(a=None, b=None, d_out=OUT, da=OUT, db=None, ld_a=207, ld_b=207, grad=None):
        d = L.DiscPoseBwdDesc()
        d.rows_a, d.rows_b = a if a is not None else _rows(2), b if b is not None else _rows(0)
        d.d_out, d.d_poses_a, d.ld_a, d.d_poses_b, d.ld_b = d_out, da, ld_a, db, ld_b
        if grad:
            setattr(d.grads, "d_" + grad, OUT)
        return d
    bwd = lambda d, w=dw, ws=WS, nb=big: lib.hmmr_disc_pose_bwd(C.byref(w), C.byref(d) if d else None, ws, nb, None)
    assert bwd(None) == -1 and "null descriptor" in err()
    assert bwd(desc(d_out=None)) == -1 and "d_out" in err()
    assert bwd(desc(da=None)) == -1 and "no output" in err()
    assert bwd(desc(a=_rows(0), b=_rows(2), da=OUT, db=None)) == -1 and "no output" in err()       # (d_poses of an empty segment is no output)
    assert bwd(desc(ld_a=206)) == -1 and "d_poses below 207" in err()
    assert bwd(desc(a=_rows(2, ld=10))) == -1 and "below 207" in err()
    assert bwd(desc(a=_rows(0))) == -1 and "n_a + n_b" in err()
    assert bwd(desc(a=_rows(-2))) == -1 and "negative" in err()
    assert bwd(desc(), w=_bank(L.HMMR_BF16)) == -1 and "HMMR_F32" in err()
    assert bwd(desc(), ws=None) == -1 and "null argument" in err()
    assert bwd(desc(da=None, grad="fc1"), nb=lib.hmmr_disc_pose_workspace_bytes(2) - 1) == -1 and "workspace too small" in err()

    def prior(real=None, fake=None, losses=None, d_rs=None, grad=None, w_e=1.0):
        d = L.PosePriorDesc()
        d.real, d.fake = real if real is not None else _rows(2), fake if fake is not None else _rows(2)
        d.w_e, d.w_d, d.losses, d.d_rs_fake = w_e, 1.0, losses, d_rs
        if grad:
            setattr(d.grads, "d_" + grad, OUT)
        return d
    run = lambda d, w=dw, ws=WS, nb=big: lib.hmmr_pose_prior(C.byref(w), C.byref(d) if d else None, ws, nb, None)
    assert run(None) == -1 and "null descriptor" in err()
    assert run(prior()) == -1 and "no output" in err()
    assert run(prior(fake=_rows(0), losses=OUT)) == -1 and "fake segment" in err()
    assert run(prior(fake=_rows(0), d_rs=OUT)) == -1 and "fake segment" in err()
    assert run(prior(real=_rows(0), fake=_rows(0), grad="b1")) == -1 and "n_a + n_b" in err()
    assert run(prior(fake=_rows(-1), grad="b1")) == -1 and "negative" in err()
    assert run(prior(real=_rows(2, ld=200), losses=OUT)) == -1 and "below 207" in err()
    assert run(prior(losses=OUT), w=_bank(L.HMMR_F16X3)) == -1 and "HMMR_F32" in err()
    assert run(prior(losses=OUT), ws=None) == -1 and "null argument" in err()
    assert run(prior(losses=OUT), nb=16) == -1 and "workspace too small" in err()
    assert run(prior(losses=OUT, w_e=float("nan"))) == -1 and "finite" in err()


def test_engine_and_mirror_modules_import_without_a_gpu():
    from human_dynamics_amd import disc_autograd, discriminators, trainer_losses      # noqa: F401
    d = discriminators.PoseDiscriminator(1e-4)
    assert d.wd == 1e-4 and hasattr(d, "get_output") and hasattr(d, "get_vars")
    assert callable(trainer_losses.compute_losses_prior)
