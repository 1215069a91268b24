"""The pose discriminator on the device (csrc/disc_pose.hip: hmmr_disc_pose_fwd, hmmr_disc_pose_bwd, hmmr_pose_prior) and its Python
routes (HmmrEngine.disc_pose / disc_pose_backward / pose_prior, discriminators.PoseDiscriminator.get_output = disc_autograd.disc_pose_apply,
trainer_losses.compute_losses_prior)
against torch.autograd in float64.

out, d_poses, each of the twelve gradients and each loss are compared SEPARATELY with the float64 autograd of the restated oracle
(tests/disc_cases.py, pinned to the reference's code by tests/test_disc_cases.py).  The bound is not a chosen number:
E32 = |autograd in float32 - autograd in float64| over all cases is the error of the same computation in fp32, and a kernel may be
FACTOR = 4 times that away.  Rows with a pre-activation within rounding distance of zero are redrawn (disc_cases.py).  With `-s` every
case prints its error, E32 and their ratio, and the module prints the largest ratio per quantity at the end.  Every call in this file
is a valid call; the refusals are in tests/test_disc_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import disc_cases as D
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
GUARD = D.GUARD
_STATS = {}
_ENGINES = {}
_RESULTS = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _engine(device, smpl=None):
    key = (device, smpl is not None)
    if key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        eng = HmmrEngine(dict(D.weights()), smpl, dtype="f32", device=device)
        assert eng.disc_pose_bank().dw.dtype == L.HMMR_F32
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k, (r, tag) in sorted(_STATS.items()):
        print("disc_pose summary: largest err / E32 of %-10s: %5.2f (%s)" % (k, r, tag))
    _ENGINES.clear()
    _RESULTS.clear()


def _note(key, tag, err, e):
    ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
    print("disc_pose %-10s %-10s err %.3e  E32 %.3e  ratio %5.2f" % (tag, key, err, e, ratio))
    if ratio > _STATS.get(key, (-1.0, ""))[0]:
        _STATS[key] = (ratio, tag)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _guarded(eng, shape):
    return torch.full(shape, GUARD, dtype=torch.int32, device=eng.device).view(torch.float32)


def _seg(eng, x, ld):
    """rows x [n,207] on the device at row stride ld (gaps = the guard pattern) -> (buffer, hmmr_rows_t)"""
    r = L.Rows()
    if not x.shape[0]:
        return None, r
    buf = torch.from_numpy(D.strided(x, ld)).to(eng.device)
    r.ptr, r.ld, r.n = buf.data_ptr(), ld, x.shape[0]
    return buf, r


def _call(eng, xa, xb, cot, ld_a=207, ld_b=207, want_a=True, want_b=True, names=D.NAMES, ld_out=None):
    """hmmr_disc_pose_fwd + hmmr_disc_pose_bwd through ctypes on guarded buffers -> dict of float32 numpy (out, d_a / d_b as the raw
    strided buffers, the gradients)"""
    bank, lib = eng.disc_pose_bank(), eng.lib
    ka, ra = _seg(eng, xa, ld_a)
    kb, rb = _seg(eng, xb, ld_b)
    n = ra.n + rb.n
    ws, nbytes = eng._disc_ws(n)
    out = _guarded(eng, (n + 1, 24))
    L.check(lib.hmmr_disc_pose_fwd(C.byref(bank.dw), C.byref(ra), C.byref(rb), out.data_ptr(), ws.data_ptr(), nbytes, eng._stream()), "fwd")
    ld_out = ld_out or (ld_a, ld_b)
    d = L.DiscPoseBwdDesc()
    d.rows_a, d.rows_b = ra, rb
    dc = torch.from_numpy(np.ascontiguousarray(cot, np.float32)).to(eng.device)
    d.d_out = dc.data_ptr()
    da = _guarded(eng, (ra.n * ld_out[0] + 8,)) if want_a and ra.n else None
    db = _guarded(eng, (rb.n * ld_out[1] + 8,)) if want_b and rb.n else None
    d.d_poses_a, d.ld_a, d.d_poses_b, d.ld_b = L.ptr(da), ld_out[0], L.ptr(db), ld_out[1]
    pad = {k: (_guarded(eng, (bank.params[k].numel() + 8,)) if k in names else None) for k in D.NAMES}      # 8 guard floats behind each
    for k in D.NAMES:
        setattr(d.grads, "d_" + k, L.ptr(pad[k]))
    L.check(lib.hmmr_disc_pose_bwd(C.byref(bank.dw), C.byref(d), ws.data_ptr(), nbytes, eng._stream()), "bwd")
    torch.cuda.synchronize()
    n_ = lambda t: None if t is None else t.cpu().numpy()
    res = dict(out=n_(out), d_a=n_(da), d_b=n_(db), ld=ld_out, n=(ra.n, rb.n), inputs=(n_(ka), n_(kb)))
    for k in D.NAMES:
        res[k] = n_(pad[k])
    return res


def _unpack(res):
    """the checked view of a _call result: guards verified, {out [n,24], d_poses [n,207] (None when not asked), gradients}"""
    guard = np.int32(GUARD)
    n_a, n_b = res["n"]
    n = n_a + n_b
    assert (_bits(res["out"][n:]) == guard).all(), "out: written behind row n"
    out = dict(out=res["out"][:n])
    parts = []
    for key, cnt, ld in (("d_a", n_a, res["ld"][0]), ("d_b", n_b, res["ld"][1])):
        buf = res[key]
        if buf is None:
            parts.append(None)
            continue
        body = buf[:cnt * ld].reshape(cnt, ld)
        assert (_bits(body[:, 207:]) == guard).all() and (_bits(buf[cnt * ld:]) == guard).all(), key + ": written outside a row's 207 values"
        assert np.isfinite(body[:, :207]).all(), key
        parts.append(body[:, :207])
    have = [p for p in parts if p is not None]
    out["d_poses"] = np.concatenate(have) if len(have) == (n_a > 0) + (n_b > 0) and have else None
    out["d_a"], out["d_b"] = parts
    for k in D.NAMES:
        if res[k] is not None:
            assert (_bits(res[k][-8:]) == guard).all(), k + ": written behind its extent"
            out[k] = res[k][:-8]
    return out


def _result(device, case):
    if case.name not in _RESULTS:
        xa, xb = D.rows(case)
        _RESULTS[case.name] = _unpack(_call(_engine(device), xa, xb, D.cotangent(case), case.ld_a, case.ld_b))
    return _RESULTS[case.name]


def _prior(eng, real, fake, w_e=1.0, w_d=1.0, **kw):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(eng.device).reshape(-1, 207) if x.shape[0] else None
    losses, d_rs, g = eng.pose_prior(t(real), t(fake), w_e, w_d, **kw)
    torch.cuda.synchronize()
    n_ = lambda v: None if v is None else v.cpu().numpy()
    return n_(losses), n_(d_rs), {k: n_(v) for k, v in g.items()}


# ---------------------------------------------------------------------------------------------------------------- a. against the oracle
@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_case_matches_float64_autograd(case, gpu_device):
    """out, d_poses, the twelve gradients and the three losses within FACTOR x E32; padding of the gradients exact zeros; nothing
    outside the stated extents is written (ld = 216 / 221: the gaps stay)"""
    ref, e32 = D.reference(case), D.e32()
    got = _result(gpu_device, case)
    eng = _engine(gpu_device)
    real, fake = D.loss_segments(case)
    losses = _prior(eng, real.reshape(-1, 207), fake.reshape(-1, 207), want_d_rs=False, want_weights=False)[0]
    got = dict(got, **dict(zip(D.LOSSES, losses)))
    for q in D.QUANTITIES:
        bank_shape = ref[q].shape
        err = float(np.abs(np.asarray(got[q], np.float64).reshape(bank_shape) - ref[q]).max())
        _note(q, case.name, err, e32[q])
        assert np.isfinite(got[q]).all() and err <= D.FACTOR * e32[q], (case.name, q, err, e32[q])
    z = lambda a: not _bits(a).any()
    assert z(got["conv1"].reshape(32, 16)[:, 9:]) and z(got["heads"].reshape(32, 32)[23:]) and z(got["bj"][23:])
    assert z(got["fc1"].reshape(1024, 1024)[:, 736:]) and z(got["fc_out"].reshape(128, 1024)[1:]) and z(got["bo"][1:])


# ---------------------------------------------------------------------------------------------------------------- b. rows stand alone
def test_a_row_does_not_depend_on_the_other_rows(gpu_device):
    """(7,0) equals rows 0..6 of (33,0) in out and d_poses, bit for bit (their cotangents: rows 0..6 of the larger case's)"""
    big_case, small_case = D.BY_NAME["33_0"], D.BY_NAME["7_0"]
    big = _result(gpu_device, big_case)
    xa, xb = D.rows(small_case)
    small = _unpack(_call(_engine(gpu_device), xa, xb, D.cotangent(big_case)[:7], small_case.ld_a, small_case.ld_b))
    assert _same_bits(np.ascontiguousarray(big["out"][:7]), small["out"])
    assert _same_bits(np.ascontiguousarray(big["d_poses"][:7]), small["d_poses"])


def test_the_split_into_segments_changes_no_byte(gpu_device):
    """the 64 rows of (31,33) as 31 + 33, 1 + 63 and 64 + 0: the same bytes everywhere"""
    case = D.BY_NAME["31_33"]
    base = _result(gpu_device, case)
    x = np.concatenate(D.rows(case))
    for cut, lds in ((1, (207, 216)), (64, (221, 207))):
        got = _unpack(_call(_engine(gpu_device), x[:cut], x[cut:], D.cotangent(case), *lds))
        for q in ("out", "d_poses") + D.NAMES:
            assert _same_bits(np.ascontiguousarray(got[q]), np.ascontiguousarray(base[q])), (cut, q)


# ---------------------------------------------------------------------------------------------------------------- c. the closed loop
@pytest.mark.parametrize("name,w_e,w_d", [("2_2", 1.0, 1.0), ("31_33", 0.75, 1.5)])
def test_pose_prior_is_forward_plus_two_backward_calls(name, w_e, w_d, gpu_device):
    """losses, d_rs_fake and the twelve gradients of hmmr_pose_prior equal, bit for bit, what hmmr_disc_pose_fwd and two
    hmmr_disc_pose_bwd calls with the stated cotangents give; two runs give equal bytes; a NULL output changes no other output; in
    d_rs_fake the first nine values of a row are zeros and the other 207 are written"""
    case = D.BY_NAME[name]
    eng = _engine(gpu_device)
    real, fake = [r.reshape(-1, 207) for r in D.rows(case)]
    n_r, n_f = real.shape[0], fake.shape[0]
    losses, d_rs, g = _prior(eng, real, fake, w_e, w_d)
    again = _prior(eng, real, fake, w_e, w_d)
    assert _same_bits(losses, again[0]) and _same_bits(d_rs, again[1]) and all(_same_bits(g[k], again[2][k]) for k in D.NAMES)
    out = eng.disc_pose(torch.from_numpy(real).to(eng.device), torch.from_numpy(fake).to(eng.device)).cpu().numpy()
    s_e, s_f, s_r = np.float32(2.0 * w_e / n_f), np.float32(2.0 * w_d / n_f), np.float32(2.0 * w_d / n_r)
    one = np.float32(1.0)
    cot_e = np.concatenate([np.zeros((n_r, 24), np.float32), s_e * (out[n_r:] - one)])
    cot_d = np.concatenate([s_r * (out[:n_r] - one), s_f * out[n_r:]])
    sep_e = _unpack(_call(eng, real, fake, cot_e, want_a=False, names=()))
    sep_d = _unpack(_call(eng, real, fake, cot_d, want_a=False, want_b=False))
    d_rs = d_rs.reshape(n_f, 216)
    assert not _bits(d_rs[:, :9]).any()
    assert _same_bits(np.ascontiguousarray(d_rs[:, 9:]), np.ascontiguousarray(sep_e["d_b"]))
    for k in D.NAMES:
        assert _same_bits(g[k].reshape(-1), sep_d[k]), k
    # the losses: a row's 24 terms in column order, the rows in row order, all in double, divided by the count and rounded once -- from
    # the device's own out, so the bits are equal
    def mean_of(rows, shift):
        total = 0.0
        for r in rows:
            row = 0.0
            for v in r:
                d = float(np.float32(v - np.float32(shift))) if shift else float(v)
                row += d * d
            total += row
        return np.float32(total / len(rows))
    want = np.array([mean_of(out[n_r:], 1.0), mean_of(out[:n_r], 1.0), mean_of(out[n_r:], 0.0)], np.float32)
    assert _same_bits(losses, want), (losses, want)
    # through ctypes on guarded buffers: nothing is written behind losses[3] or behind the n_fake rows of d_rs_fake
    ka, ra = _seg(eng, real, 207)
    kb, rb = _seg(eng, fake, 216)
    d = L.PosePriorDesc()
    d.real, d.fake, d.w_e, d.w_d = ra, rb, w_e, w_d
    gl, gr = _guarded(eng, (8,)), _guarded(eng, (n_f * 216 + 8,))
    d.losses, d.d_rs_fake = gl.data_ptr(), gr.data_ptr()
    ws, nbytes = eng._disc_ws(n_r + n_f)
    L.check(eng.lib.hmmr_pose_prior(C.byref(eng.disc_pose_bank().dw), C.byref(d), ws.data_ptr(), nbytes, eng._stream()), "prior")
    torch.cuda.synchronize()
    gl, gr = gl.cpu().numpy(), gr.cpu().numpy()
    assert _same_bits(gl[:3], losses) and (_bits(gl[3:]) == np.int32(GUARD)).all()
    assert _same_bits(gr[:n_f * 216].reshape(n_f, 216), d_rs) and (_bits(gr[n_f * 216:]) == np.int32(GUARD)).all()
    # NULL outputs change no other output's bytes
    only_l = _prior(eng, real, fake, w_e, w_d, want_d_rs=False, want_weights=False)
    only_r = _prior(eng, real, fake, w_e, w_d, want_losses=False, want_weights=False)
    only_w = _prior(eng, real, fake, w_e, w_d, want_losses=False, want_d_rs=False, want_weights=("fc1", "bj"))
    assert _same_bits(only_l[0], losses) and only_l[1] is None
    assert _same_bits(only_r[1].reshape(n_f, 216), d_rs) and only_r[0] is None
    assert _same_bits(only_w[2]["fc1"], g["fc1"]) and _same_bits(only_w[2]["bj"], g["bj"]) and only_w[2]["fc2"] is None


def test_null_outputs_of_the_backward_change_no_other_output(gpu_device):
    case = D.BY_NAME["31_33"]
    base = _result(gpu_device, case)
    xa, xb = D.rows(case)
    eng = _engine(gpu_device)
    got = _unpack(_call(eng, xa, xb, D.cotangent(case), case.ld_a, case.ld_b, want_a=False, names=("conv1", "b2", "fc_out")))
    assert got["d_a"] is None and _same_bits(got["d_b"], base["d_b"])
    for k in ("conv1", "b2", "fc_out"):
        assert _same_bits(got[k], base[k]), k
    got = _unpack(_call(eng, xa, xb, D.cotangent(case), case.ld_a, case.ld_b, want_b=False, names=()))
    assert _same_bits(got["d_a"], base["d_a"])
    got = _unpack(_call(eng, xa, xb, D.cotangent(case), case.ld_a, case.ld_b, want_a=False, want_b=False, names=("heads",)))
    assert _same_bits(got["heads"], base["heads"])


# ---------------------------------------------------------------------------------------------------------------- d. sensitivity
def test_single_column_cotangents_reach_what_they_must(gpu_device):
    """a cotangent in column 23 alone: d_wj == 0 exactly, and d_F1, d_F2, d_fo, d_poses more than 1000 bounds large; in column j alone:
    d_wj non-zero in row j only, d_poses non-zero in joint j only -- a dropped term cannot pass"""
    case = D.BY_NAME["2_2"]
    eng, bnd = _engine(gpu_device), D.bounds()
    xa, xb = D.rows(case)
    cot = np.zeros((4, 24), np.float32)
    cot[:, 23] = 1.0
    got = _unpack(_call(eng, xa, xb, cot))
    assert not _bits(got["heads"]).any() and not _bits(got["bj"]).any()
    for q in ("fc1", "fc2", "fc_out", "d_poses"):
        assert np.abs(got[q]).max() > 1000 * bnd[q], (q, np.abs(got[q]).max(), bnd[q])
    for j in (0, 11, 22):
        cot = np.zeros((4, 24), np.float32)
        cot[:, j] = 1.0
        got = _unpack(_call(eng, xa, xb, cot))
        heads, dp = got["heads"].reshape(32, 32), got["d_poses"].reshape(4, 23, 9)
        other = [i for i in range(32) if i != j]
        assert heads[j].any() and not _bits(heads[other]).any()
        assert dp[:, j].any() and not _bits(dp[:, [i for i in range(23) if i != j]]).any()
        assert not _bits(got["fc1"]).any() and not _bits(got["fc_out"]).any()


# ---------------------------------------------------------------------------------------------------------------- e. the chain
def _chain_problem(n):
    import smpl_grad_cases as SG
    from oracle import hmmr_oracle as O

    def row(kind, i):
        """theta [72] (kind 0) or a mocap row [207] (kind 1) whose discriminator input has no pre-activation near a kink: the draw
        is repeated with the next seed until it has none (disc_cases.py, "ReLU kinks")"""
        for r in range(64):
            if kind:
                x = D.draw_row(90, i, r)
                v = x.reshape(207)
            else:
                v = (0.4 * np.random.Generator(np.random.PCG64([31, i, r])).standard_normal(72)).astype(np.float32)
                x = O.batch_rodrigues(torch.tensor(v.astype(np.float64)).reshape(-1, 3)).reshape(24, 9)[1:].numpy()
            if not D.ambiguous(x[None])[0]:
                return v
        raise AssertionError("no unambiguous draw")
    theta = np.stack([row(0, i) for i in range(n)])
    real = np.stack([row(1, i) for i in range(n)])
    beta = np.random.Generator(np.random.PCG64([32, n])).standard_normal((n, 10)).astype(np.float32)
    return SG._model(130), theta, beta, real


def _chain_oracle(theta, real, dtype):
    """e_pose of the fake rows Rs(theta)[:, 1:] and its gradient in theta, by autograd in `dtype` -> (e_pose, d_pose, d_theta)"""
    from oracle import hmmr_oracle as O
    P = D.params(dtype, False)
    th = torch.tensor(theta.astype(np.float64), dtype=dtype).requires_grad_(True)
    rs = O.batch_rodrigues(th.reshape(-1, 3)).reshape(-1, 24, 9)
    e, dr, df = D.losses(D.forward(P, torch.tensor(real.astype(np.float64), dtype=dtype).reshape(-1, 23, 9)), D.forward(P, rs[:, 1:]))
    g, = torch.autograd.grad(e, th)
    return float(e.detach()), float((dr + df).detach()), g.to(torch.float64).numpy()


@pytest.mark.parametrize("n", [2, 20])
def test_compute_losses_prior_reaches_theta_through_smpl_apply(n, gpu_device):
    """compute_losses_prior on smpl_apply's Rs with .backward(): d_theta within 4 x E32 of float64, E32 of the composed function
    theta -> Rodrigues -> discriminator -> e_pose; d_pose's gradient lands on the bank and not on theta"""
    from human_dynamics_amd import trainer_losses
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    mdl, theta, beta, real = _chain_problem(n)
    eng = _engine(gpu_device, mdl)
    e64, d64, g64 = _chain_oracle(theta, real, torch.float64)
    e32, d32, g32 = _chain_oracle(theta, real, torch.float32)
    th = torch.from_numpy(theta).to(eng.device).requires_grad_(True)
    be = torch.from_numpy(beta).to(eng.device)
    rs = smpl_apply(eng, th, be)[3]
    bank = eng.disc_pose_bank()
    for t in bank.tensors():
        t.requires_grad_(True)
        t.grad = None
    try:
        out = trainer_losses.compute_losses_prior(eng, real, [rs], [be])
        assert sorted(out) == ["d_pose", "e_pose", "e_shape"]
        out["e_pose"].backward(retain_graph=True)
        assert all(t.grad is None for t in bank.tensors())            # e_pose does not reach the bank
        got = th.grad.cpu().numpy().astype(np.float64)
        th.grad = None
        out["d_pose"].backward()
        assert th.grad is None and all(t.grad is not None for t in bank.tensors())      # d_pose does not reach the poses
    finally:
        for t in bank.tensors():
            t.requires_grad_(False)
            t.grad = None
    for key, err, e in (("chain d_theta", np.abs(got - g64).max(), np.abs(g32 - g64).max()),
                        ("chain e_pose", abs(float(out["e_pose"].detach()) - e64), abs(e32 - e64)), ("chain d_pose", abs(float(out["d_pose"].detach()) - d64), abs(d32 - d64))):
        _note(key, "n%d" % n, err, e)
    assert np.abs(got - g64).max() <= D.FACTOR * np.abs(g32 - g64).max()


# ---------------------------------------------------------------------------------------------------------------- e2. the autograd routes
def _apply_oracle(theta, xb, cot, dtype):
    """sum(out * cot) for rows Rs(theta)[:, 1:] | xb -> (d_theta, d_xb) by autograd in `dtype`"""
    from oracle import hmmr_oracle as O
    P = D.params(dtype, False)
    th = torch.tensor(theta.astype(np.float64), dtype=dtype).requires_grad_(True)
    b = torch.tensor(xb.astype(np.float64), dtype=dtype).reshape(-1, 23, 9).requires_grad_(True)
    rs = O.batch_rodrigues(th.reshape(-1, 3)).reshape(-1, 24, 9)
    out = D.forward(P, torch.cat([rs[:, 1:], b]))
    g = torch.autograd.grad((out * torch.tensor(cot.astype(np.float64), dtype=dtype)).sum(), [th, b])
    return [t.to(torch.float64).numpy() for t in g]


@pytest.mark.parametrize("order", ["rs_first", "rs_second"])
def test_autograd_routes_give_the_direct_calls_gradients(order, gpu_device):
    """PoseDiscriminator.get_output / disc_autograd.disc_pose_apply on smpl_apply's Rs [n,24,3,3] (used in place: Rs + 9, ld 216)
    and a second [m,207] segment, .backward() with a random cotangent: out, the gradient on Rs (nine zeros, then 207 values: the
    full_a / full_b form of HmmrEngine.disc_pose_backward), on the 207-wide rows and the twelve .grads on the bank's tensors equal
    the ctypes route's bytes; d_theta is within 4 x E32 (of the composed function) of float64.  Both segment orders."""
    from human_dynamics_amd.discriminators import PoseDiscriminator
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    n, case = 5, D.BY_NAME["2_2"]
    mdl, theta, beta, _ = _chain_problem(n)
    xb = np.concatenate(D.rows(case)).reshape(-1, 207)[:3]
    m = xb.shape[0]
    cot = np.random.Generator(np.random.PCG64([41, n])).standard_normal((n + m, 24)).astype(np.float32)
    eng = _engine(gpu_device, mdl)
    bank = eng.disc_pose_bank()
    th = torch.from_numpy(theta).to(eng.device).requires_grad_(True)
    be = torch.from_numpy(beta).to(eng.device)
    b = torch.from_numpy(xb).to(eng.device).requires_grad_(True)
    for t in bank.tensors():
        t.requires_grad_(True)
        t.grad = None
    try:
        rs = smpl_apply(eng, th, be)[3]
        rs.retain_grad()
        disc = PoseDiscriminator(1e-4, engine=eng)
        assert [t.data_ptr() for t in disc.get_vars()] == [t.data_ptr() for t in bank.tensors()]
        first = order == "rs_first"
        out = disc.get_output(rs, b) if first else disc.get_output(b, rs)
        assert tuple(out.shape) == (n + m, 24)
        c = cot if first else np.concatenate([cot[n:], cot[:n]])                    # (cot rows follow theta | xb; the call's rows follow its segments)
        (out * torch.from_numpy(c).to(eng.device)).sum().backward()
        torch.cuda.synchronize()
        got_w = {k: t.grad.cpu().numpy() for k, t in zip(D.NAMES, bank.tensors())}
        d_rs, d_b, d_th = rs.grad.cpu().numpy().reshape(n, 216), b.grad.cpu().numpy(), th.grad.cpu().numpy().astype(np.float64)
    finally:
        for t in bank.tensors():
            t.requires_grad_(False)
            t.grad = None
    xa = rs.detach().cpu().numpy().reshape(n, 216)[:, 9:]
    direct = _unpack(_call(eng, xa, xb, cot, 216, 207) if first else _call(eng, xb, xa, c, 207, 216))
    assert _same_bits(out.detach().cpu().numpy(), direct["out"])
    assert not _bits(d_rs[:, :9]).any()
    assert _same_bits(np.ascontiguousarray(d_rs[:, 9:]), np.ascontiguousarray(direct["d_a" if first else "d_b"]))
    assert _same_bits(d_b, np.ascontiguousarray(direct["d_b" if first else "d_a"]))
    for k in D.NAMES:
        assert _same_bits(got_w[k].reshape(-1), direct[k]), k
    (g64, gb64), (g32, gb32) = _apply_oracle(theta, xb, cot, torch.float64), _apply_oracle(theta, xb, cot, torch.float32)
    for key, err, e in (("apply d_theta", np.abs(d_th - g64).max(), np.abs(g32 - g64).max()),
                        ("apply d_rows", np.abs(d_b.reshape(-1, 23, 9) - gb64).max(), np.abs(gb32 - gb64).max())):
        _note(key, order, err, e)
        assert err <= D.FACTOR * e, (key, err, e)


def test_autograd_route_with_an_empty_or_absent_segment(gpu_device):
    """disc_pose_apply with poses_b None, with an empty [0,207] second segment and with an empty first one: the rows' out and
    gradient are the two-segment call's bytes, an empty segment gets an empty gradient"""
    from human_dynamics_amd.disc_autograd import disc_pose_apply
    eng = _engine(gpu_device)
    case = D.BY_NAME["2_2"]
    x = np.concatenate(D.rows(case)).reshape(-1, 207)
    cot = D.cotangent(case)
    direct = _unpack(_call(eng, x[:2], x[2:], cot, names=()))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    for kind in ("none", "empty_b", "empty_a"):
        rows = dev(x).requires_grad_(True)
        empty = torch.zeros((0, 207), device=eng.device).requires_grad_(True)
        out = disc_pose_apply(eng, rows) if kind == "none" else (disc_pose_apply(eng, rows, empty) if kind == "empty_b" else disc_pose_apply(eng, empty, rows))
        (out * dev(cot)).sum().backward()
        assert _same_bits(out.detach().cpu().numpy(), direct["out"]), kind
        assert _same_bits(rows.grad.cpu().numpy(), direct["d_poses"]), kind
        assert kind == "none" or (empty.grad is not None and tuple(empty.grad.shape) == (0, 207)), kind


# ---------------------------------------------------------------------------------------------------------------- f. descent
DESCENT_STEPS, DESCENT_N, LR_D, LR_E = 12, 4, 1e-4, 1e-3


def _descent_oracle(theta, real, dtype):
    """twelve alternating plain gradient-descent steps in `dtype`: even steps move the bank along -d d_pose, odd steps theta along
    -d e_pose -> [(e_pose, d_pose) at the start of every step], the final theta"""
    from oracle import hmmr_oracle as O
    P = D.params(dtype, True)
    th = torch.tensor(theta.astype(np.float64), dtype=dtype).requires_grad_(True)
    x_real = torch.tensor(real.astype(np.float64), dtype=dtype).reshape(-1, 23, 9)
    trace = []
    for k in range(DESCENT_STEPS):
        rs = O.batch_rodrigues(th.reshape(-1, 3)).reshape(-1, 24, 9)
        e, dr, df = D.losses(D.forward(P, x_real), D.forward(P, rs[:, 1:]))
        trace.append((float(e.detach()), float((dr + df).detach())))
        grads = torch.autograd.grad(dr + df, list(P.values())) if k % 2 == 0 else torch.autograd.grad(e, th)
        with torch.no_grad():
            if k % 2 == 0:
                for p, g in zip(P.values(), grads):
                    p -= LR_D * g
            else:
                th -= LR_E * grads[0]
    return np.array(trace), th.detach().to(torch.float64).numpy()


def test_alternating_descent_follows_the_float64_run(gpu_device):
    """Twelve alternating gradient-descent steps (the bank on d_pose, theta on e_pose, through compute_losses_prior and smpl_apply)
    against the same steps of the oracle in float64.  The bound is the composed function's own float32 error: at step k the device's
    e_pose and d_pose may each be 4 x E32_k away from the float64 run's, E32_k = the largest |float32 run - float64 run| of THAT loss
    over steps 0..k (an error made at one step stays in the parameters of every later one, so the yardstick's error is taken
    cumulatively, as tests/ief_grad_cases.py does); the final theta likewise, by its own largest float32 error."""
    from human_dynamics_amd import trainer_losses
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    mdl, theta, beta, real = _chain_problem(DESCENT_N)
    t64, th64 = _descent_oracle(theta, real, torch.float64)
    t32, th32 = _descent_oracle(theta, real, torch.float32)
    eng = _engine(gpu_device, mdl)
    bank = eng.disc_pose_bank()
    th = torch.from_numpy(theta).to(eng.device)
    be = torch.from_numpy(beta).to(eng.device)
    real_d = torch.from_numpy(real).to(eng.device)
    trace = []
    try:
        for k in range(DESCENT_STEPS):
            thk = th.clone().requires_grad_(True)
            for t in bank.tensors():
                t.requires_grad_(k % 2 == 0)
                t.grad = None
            out = trainer_losses.compute_losses_prior(eng, real_d, [smpl_apply(eng, thk, be)[3]], [be])
            trace.append((float(out["e_pose"].detach()), float(out["d_pose"].detach())))
            if k % 2 == 0:
                out["d_pose"].backward()
                with torch.no_grad():
                    for t in bank.tensors():
                        g = t.grad
                        t.requires_grad_(False)
                        t -= LR_D * g
            else:
                out["e_pose"].backward()
                th = th - LR_E * thk.grad
    finally:
        for t in bank.tensors():
            t.requires_grad_(False)
            t.grad = None
        bank.load_checkpoint(D.weights())                  # the module's other tests read the seeded bank
    trace = np.array(trace)
    e32 = np.maximum.accumulate(np.abs(t32 - t64), axis=0)       # [step, loss]: per loss, cumulative over the steps
    err = np.abs(trace - t64)
    for k in range(DESCENT_STEPS):
        digits = -np.log10(max(err[k].max(), 1e-300) / np.abs(t64[k]).max())
        print("disc_pose descent step %2d: e_pose %.7f d_pose %.7f (float64 %.7f %.7f)  err %.2e %.2e  E32 %.2e %.2e  digits %.1f"
              % (k, trace[k, 0], trace[k, 1], t64[k, 0], t64[k, 1], err[k, 0], err[k, 1], e32[k, 0], e32[k, 1], digits))
        _note("descent e_pose", "step%d" % k, err[k, 0], e32[k, 0])
        _note("descent d_pose", "step%d" % k, err[k, 1], e32[k, 1])
    assert (t64[2:, 1] < t64[:-2, 1]).any()                   # (the float64 run moves at all)
    assert (err <= D.FACTOR * e32).all(), (err, e32)
    e_th = np.abs(th32 - th64).max()
    err_th = np.abs(th.cpu().numpy().astype(np.float64) - th64).max()
    _note("descent th", "final", err_th, e_th)
    assert err_th <= D.FACTOR * e_th, (err_th, e_th)
