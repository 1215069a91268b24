"""The SMPL backward (csrc/smpl_grad.hip: hmmr_smpl_bwd) and its autograd route against torch.autograd in float64.

Every gradient is compared SEPARATELY with g64 = autograd of the restated oracle in float64 (tests/smpl_grad_cases.py).  The bound
is not a chosen number: E32 = |autograd in float32 - g64| over the case's group is the error of the same derivative in the kernels'
working precision, and a kernel may be FACTOR = 4 times that away.  tests/test_smpl_grad_cases.py asserts that every single
cotangent's gradient is at least 1000 bounds large, so a dropped term cannot pass.  With `-s` every case prints its error, E32
and their ratio, and the module prints the largest ratio per gradient and input family at the end (profiles/smpl_grad_sweep.log
is one such run).  Every call in this file is a valid call; the refusals are in tests/test_smpl_grad_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import smpl_grad_cases as G
from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
GUARD = 0x7FC12345            # a quiet NaN with a payload: the bit pattern of every float no kernel may touch
_STATS = {}
_ENGINES = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _engine(device, case):
    key = (device, case.nv, case.joint_type, tuple(sorted(case.model_kw.items())))
    if key not in _ENGINES:
        from human_dynamics_amd.engine import HmmrEngine
        _ENGINES[key] = HmmrEngine(None, case.model, device=device, joint_type=case.joint_type)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for (k, fam), (r, tag) in sorted(_STATS.items()):
        print("smpl-grad summary: largest err / E32 of %-7s %-8s: %5.2f (%s)" % (k, fam, r, tag))
    _ENGINES.clear()


def _dev(eng, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrays]


def _backward(eng, case, only=None, want_cams=True, inputs=None):
    """forward (for joints), then hmmr_smpl_bwd with all four cotangents or one of them -> {d_theta, d_beta, d_cams} numpy"""
    th, be, ca = inputs if inputs is not None else _dev(eng, case.theta, case.beta, case.cams)
    joints = eng.smpl(th, be, ca)[1]
    cot = {k: (_dev(eng, case.cot[k])[0] if only in (None, k) else None) for k in G.OUTPUTS}
    out = eng.smpl_backward(th, be, ca, joints, d_verts=cot["verts"], d_joints=cot["joints"], d_kps=cot["kps"], d_rs=cot["Rs"],
                            want_cams=want_cams)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in zip(G.GRADS, out)}


def _check(tag, family, got, ref, bnd):
    for k in G.GRADS:
        if got[k] is None:
            continue
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), (tag, k)
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        e = bnd[k] / G.FACTOR
        ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
        print("smpl-grad %-44s %-7s err %.3e  E32 %.3e  ratio %5.2f  |g64| %.3e" % (tag, k, err, e, ratio, float(np.abs(ref[k]).max())))
        if ratio > _STATS.get((k, family), (-1.0, ""))[0]:
            _STATS[(k, family)] = (ratio, tag)
        assert err <= bnd[k], (tag, k, err, bnd[k])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("group", ("nv50", "nv130", "nv700", "nv300"))
@pytest.mark.parametrize("family", G.FAMILIES)
def test_backward_against_float64(family, group, gpu_device):
    """all four cotangents together: vertex counts below one tile, one tile + two vertices and several tiles, crossed with instance
    counts around the blocks of 8; short skinning rows, widths 1, 4 and 24, the lsp keypoints, a regressor with an empty and two long
    columns"""
    cases = G.sweep(family)[group]
    bnd = G.bounds(cases)
    for case in cases:
        got = _backward(_engine(gpu_device, case), case)
        assert got["d_theta"].shape == (case.m, 72) and got["d_beta"].shape == (case.m, 10) and got["d_cams"].shape == (case.m, 3)
        _check(case.name, family, got, case.grads(), bnd)


def test_backward_full_size_model(gpu_device):
    """6890 vertices: 54 tiles, the last one with 106 vertices; the partial sum has 54 terms"""
    case = G.full_size_case()
    _check(case.name, "full", _backward(_engine(gpu_device, case), case), case.grads(), G.bounds([case]))


# ---------------------------------------------------------------------------------------------------------------- NULL cotangents
@pytest.mark.parametrize("only", G.OUTPUTS)
def test_each_cotangent_alone(only, gpu_device):
    """the other three are NULL: never read, treated as zero"""
    case = G.sweep("standard")["nv130"][1]
    assert (case.nv, case.m) == (130, 5)
    bnd = G.bounds(G.sweep("standard")["nv130"])
    eng = _engine(gpu_device, case)
    got = _backward(eng, case, only=only)
    _check("%s only %s" % (case.name, only), "standard", got, case.grads(only=only), bnd)
    for k in G.GRADS:
        if only not in G.REACH[k]:
            assert not got[k].any(), (only, k)                      # exactly zero, not small
    if only == "kps":                                                # d_cams not requested: the same pose and shape gradients
        bare = _backward(eng, case, only="kps", want_cams=False)
        assert bare["d_cams"] is None and _same_bits(bare["d_theta"], got["d_theta"]) and _same_bits(bare["d_beta"], got["d_beta"])


def test_camera_gradient_without_keypoint_cotangent_is_zero(gpu_device):
    case = G.sweep("standard")["nv130"][1]
    eng = _engine(gpu_device, case)
    th, be, ca = _dev(eng, case.theta, case.beta, case.cams)
    dv = _dev(eng, case.cot["verts"])[0]
    d_theta, d_beta, d_cams = eng.smpl_backward(th, be, ca, None, d_verts=dv)        # (joints are needed with d_kps only)
    assert d_cams.shape == (5, 3) and not d_cams.cpu().numpy().view(np.int32).any()
    ref = case.grads(only="verts")
    bnd = G.bounds(G.sweep("standard")["nv130"])
    assert np.abs(d_theta.cpu().numpy() - ref["d_theta"]).max() <= bnd["d_theta"]
    assert np.abs(d_beta.cpu().numpy() - ref["d_beta"]).max() <= bnd["d_beta"]
    # without cams at all: no camera gradient, the same bits
    t2, b2, c2 = eng.smpl_backward(th, be, None, None, d_verts=dv)
    assert c2 is None and torch.equal(t2.view(torch.int32), d_theta.view(torch.int32)) and torch.equal(b2.view(torch.int32), d_beta.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- strides, determinism
def test_strided_inputs_equal_contiguous_copies(gpu_device):
    """theta, beta and cams in place as columns 3..74, 75..84 and 0..2 of one [m, 85] omega tensor (ld = 85)"""
    case = G.sweep("standard")["nv130"][2]
    assert case.m == 17
    eng = _engine(gpu_device, case)
    om = torch.from_numpy(np.concatenate([case.cams, case.theta, case.beta], 1)).to(gpu_device)
    views = (om[:, 3:75], om[:, 75:85], om[:, 0:3])
    assert all(v.stride(0) == 85 and not v.is_contiguous() for v in views)
    a = _backward(eng, case, inputs=views)
    b = _backward(eng, case, inputs=[v.contiguous() for v in views])
    c = _backward(eng, case)
    for k in G.GRADS:
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), k


@pytest.mark.parametrize("nv", (130, 700))
def test_two_calls_give_the_same_bytes(nv, gpu_device):
    case = G.sweep("wide")["nv%d" % nv][3]
    eng = _engine(gpu_device, case)
    a = _backward(eng, case)
    b = _backward(eng, case)
    other = G.sweep("standard")["nv%d" % nv][2]
    _backward(eng, other)                                            # another call in between leaves nothing behind in the workspace
    c = _backward(eng, case)
    for k in G.GRADS:
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), (nv, k)


# ---------------------------------------------------------------------------------------------------------------- overruns
@pytest.mark.parametrize("nv,m", [(50, 1), (130, 5), (700, 33)])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(nv, m, gpu_device):
    """the outputs sit between guard rows, the workspace has exactly the reported size in front of a guard tail, and everything is
    filled with a NaN pattern first: no output element stays NaN, no guard float changes"""
    case = [c for c in G.sweep("standard")["nv%d" % nv] if c.m == m and not c.model_kw and c.joint_type == "cocoplus"][0]
    eng = _engine(gpu_device, case)
    lib = L.load()
    th, be, ca = _dev(eng, case.theta, case.beta, case.cams)
    joints = eng.smpl(th, be, ca)[1]
    cot = {k: _dev(eng, case.cot[k])[0] for k in G.OUTPUTS}
    eng.smpl_backward(th, be, ca, joints, d_kps=cot["kps"])           # (packs the grad constants)
    nbytes = lib.hmmr_smpl_bwd_workspace_bytes(C.byref(eng.sc), m)
    assert nbytes > 0 and nbytes % 4 == 0
    tail = 1 << 16
    ws = torch.full(((nbytes + tail) // 4,), GUARD, dtype=torch.int32, device=gpu_device)
    outs = {k: torch.full((m + 2, w), GUARD, dtype=torch.int32, device=gpu_device) for k, w in (("d_theta", 72), ("d_beta", 10), ("d_cams", 3))}
    L.check(lib.hmmr_smpl_bwd(C.byref(eng.sc), C.byref(eng._gc), th.data_ptr(), 72, be.data_ptr(), 10, ca.data_ptr(), 3, joints.data_ptr(), m,
                              cot["verts"].data_ptr(), cot["joints"].data_ptr(), cot["kps"].data_ptr(), cot["Rs"].data_ptr(),
                              outs["d_theta"][1:].data_ptr(), outs["d_beta"][1:].data_ptr(), outs["d_cams"][1:].data_ptr(),
                              ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "hmmr_smpl_bwd")
    torch.cuda.synchronize()
    assert (ws[nbytes // 4:].cpu().numpy() == GUARD).all()
    got = {}
    for k, full in outs.items():
        host = full.cpu().numpy()
        assert (host[0] == GUARD).all() and (host[-1] == GUARD).all(), k
        got[k] = host[1:-1].view(np.float32)
        assert np.isfinite(got[k]).all(), k
    want = _backward(eng, case)                                      # the engine's own call: the same bits
    for k in G.GRADS:
        assert _same_bits(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------- autograd
def _loss(outs, cot, keys=G.OUTPUTS):
    return sum((outs[k] * cot[k]).sum() for k in keys if outs.get(k) is not None)


def test_smpl_apply_gives_the_direct_call_s_gradients(gpu_device):
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    case = G.sweep("standard")["nv130"][1]
    eng = _engine(gpu_device, case)
    direct = _backward(eng, case)
    x = [t.requires_grad_(True) for t in _dev(eng, case.theta, case.beta, case.cams)]
    outs = dict(zip(G.OUTPUTS, smpl_apply(eng, x[0], x[1], x[2])))
    plain = eng.smpl(x[0].detach(), x[1].detach(), x[2].detach())
    for k, p in zip(G.OUTPUTS, plain):                               # the forward is engine.smpl, bit for bit
        assert outs[k].requires_grad and torch.equal(outs[k].detach().view(torch.int32), p.view(torch.int32)), k
    cot = {k: _dev(eng, case.cot[k])[0] for k in G.OUTPUTS}
    _loss(outs, cot).backward()
    for k, t in zip(G.GRADS, x):
        assert _same_bits(t.grad.cpu().numpy(), direct[k]), k
    # a loss on two outputs only: the others reach the kernel as NULL -- the bits of the direct call with those two
    y = [t.detach().clone().requires_grad_(True) for t in x]
    outs = dict(zip(G.OUTPUTS, smpl_apply(eng, *y)))
    _loss(outs, cot, ("joints", "Rs")).backward()
    j = eng.smpl(*[t.detach() for t in y])[1]
    want = eng.smpl_backward(y[0].detach(), y[1].detach(), y[2].detach(), j, d_joints=cot["joints"], d_rs=cot["Rs"])
    assert torch.equal(y[0].grad.view(torch.int32), want[0].view(torch.int32)) and torch.equal(y[1].grad.view(torch.int32), want[1].view(torch.int32))
    assert y[2].grad is None or not y[2].grad.any()
    # cams that do not require grad: no camera gradient is asked for
    z = [x[0].detach().clone().requires_grad_(True), x[1].detach().clone().requires_grad_(True), x[2].detach()]
    outs = dict(zip(G.OUTPUTS, smpl_apply(eng, *z)))
    _loss(outs, cot).backward()
    assert _same_bits(z[0].grad.cpu().numpy(), direct["d_theta"]) and _same_bits(z[1].grad.cpu().numpy(), direct["d_beta"]) and z[2].grad is None
    # no cams: no kps
    v, jn, k, r = smpl_apply(eng, z[0], z[1])
    assert k is None and v.requires_grad and jn.requires_grad and r.requires_grad


def test_smpl_call_differentiates_only_when_asked(gpu_device):
    from human_dynamics_amd.tf_smpl.batch_smpl import SMPL
    case = G.sweep("standard")["nv130"][1]
    eng = _engine(gpu_device, case)
    smpl = SMPL(case.model, engine=eng)
    th, be, _ = _dev(eng, case.theta, case.beta, None)
    plain = eng.smpl(th, be, None)
    # without requires_grad, and under no_grad with it: the present path, the same bytes, nothing to differentiate
    for beta, theta, ctx in ((be, th, torch.enable_grad()), (be.clone().requires_grad_(True), th.clone().requires_grad_(True), torch.no_grad())):
        with ctx:
            verts, joints, rs = smpl(beta, theta, get_skin=True)
            only_joints = smpl(beta, theta)
        for got, want in ((verts, plain[0]), (joints, plain[1]), (rs, plain[3]), (only_joints, plain[1])):
            assert not got.requires_grad and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # numpy inputs still work
    assert torch.equal(smpl(case.beta, case.theta).view(torch.int32), plain[1].view(torch.int32))
    # with requires_grad: .grad equals the direct call (no cams: verts, joints and Rs cotangents)
    beta, theta = be.clone().requires_grad_(True), th.clone().requires_grad_(True)
    verts, joints, rs = smpl(beta, theta, get_skin=True)
    assert verts.requires_grad and torch.equal(verts.detach().view(torch.int32), plain[0].view(torch.int32))
    cot = {k: _dev(eng, case.cot[k])[0] for k in G.OUTPUTS}
    ((verts * cot["verts"]).sum() + (joints * cot["joints"]).sum() + (rs * cot["Rs"]).sum()).backward()
    want = eng.smpl_backward(th, be, None, None, d_verts=cot["verts"], d_joints=cot["joints"], d_rs=cot["Rs"])
    assert torch.equal(theta.grad.view(torch.int32), want[0].view(torch.int32)) and torch.equal(beta.grad.view(torch.int32), want[1].view(torch.int32))
    # theta as [N, 24, 3], joints only
    t3 = th.reshape(-1, 24, 3).clone().requires_grad_(True)
    (smpl(be, t3) * cot["joints"]).sum().backward()
    want = eng.smpl_backward(th, be, None, None, d_joints=cot["joints"])
    assert t3.grad.shape == (5, 24, 3) and torch.equal(t3.grad.reshape(-1, 72).view(torch.int32), want[0].view(torch.int32))


def test_projection_in_torch_is_the_second_route_to_the_camera(gpu_device):
    """joints -> projection.batch_orth_proj_idrot -> loss against the fused kps output: both inside the bound of the float64 gradient"""
    from human_dynamics_amd.tf_smpl import projection
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    case = G.sweep("standard")["nv130"][1]
    eng = _engine(gpu_device, case)
    bnd = G.bounds(G.sweep("standard")["nv130"])
    ref = case.grads(only="kps")
    ck = _dev(eng, case.cot["kps"])[0]
    routes = {}
    for route in ("fused", "torch"):
        x = [t.requires_grad_(True) for t in _dev(eng, case.theta, case.beta, case.cams)]
        verts, joints, kps, rs = smpl_apply(eng, *x)
        if route == "torch":
            kps = projection.batch_orth_proj_idrot(joints, x[2])
        (kps * ck).sum().backward()
        routes[route] = {k: t.grad.cpu().numpy() for k, t in zip(G.GRADS, x)}
        _check("%s kps by %s" % (case.name, route), "standard", routes[route], ref, bnd)
    for k in G.GRADS:
        assert np.abs(routes["fused"][k].astype(np.float64) - routes["torch"][k]).max() <= 2 * bnd[k], k


# ---------------------------------------------------------------------------------------------------------------- descent
def test_gradient_descent_on_keypoints_follows_the_float64_run(gpu_device):
    """minimise sum ||kps - target||^2 over (theta, beta, cams) by plain gradient descent from a perturbed start, step size and count
    chosen on the host (test_smpl_grad_cases.py: the float64 run falls at every step and ends below half its start).  The device run
    falls at every step and ends within 1e-3 relative of the float64 run: gradient errors at the bound are four or more orders below
    the gradients, so a larger gap is a wrong term, not rounding."""
    from human_dynamics_amd.engine import HmmrEngine
    from human_dynamics_amd.tf_smpl.autograd import smpl_apply
    mdl, start, target = G.descent_problem()
    want = G.descent_reference()
    eng = HmmrEngine(None, mdl, device=gpu_device)
    x = [torch.from_numpy(a).to(gpu_device) for a in start]
    tgt = torch.from_numpy(target).to(gpu_device)
    losses = []
    for _ in range(G.DESCENT_STEPS + 1):
        xs = [a.clone().requires_grad_(True) for a in x]
        loss = ((smpl_apply(eng, *xs)[2] - tgt) ** 2).sum()
        losses.append(float(loss.detach()))
        loss.backward()
        x = [a - G.DESCENT_LR * b.grad for a, b in zip(x, xs)]
    print("smpl-grad descent: device %s" % " ".join("%.5g" % v for v in losses))
    print("smpl-grad descent: float64 %s" % " ".join("%.5g" % v for v in want))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs(losses[-1] - want[-1]) <= 1e-3 * want[-1], (losses[-1], want[-1])
