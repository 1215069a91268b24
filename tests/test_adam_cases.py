"""The oracle of tests/test_gpu_adam.py checked on the host (tests/adam_cases.py), every refusal of hmmr_adam_step and hmmr_strip_mse --
each returned with its message before anything is queued: dummy, never dereferenced pointers, no device --, and the names optim.TFAdam
gives its state."""
import ctypes as C

import numpy as np
import pytest

import adam_cases as A
from human_dynamics_amd import _lib as L


def _grads(n, steps, kind="mixed"):
    return [A.gradients(kind, n, k) for k in range(steps)]


def test_oracle_matches_the_float64_closed_form_over_12_steps():
    """p, m and v of the float32 restatement stay within a few float32 units of the float64 closed form.  Per step p moves by at most
    ~lr and each of the ~8 roundings on its way is half a unit of a value no larger than |p| or lr: the bound is 12 steps x 4 units of
    max(|p|, lr); m and v are sums of 12 terms of one sign pattern each, 16 units of their own size."""
    n = 4097
    p0, gs = A.values(n, 1), _grads(n, 12)
    r32, r64 = A.run32(p0, gs), A.closed64(p0, gs)
    for k in (0, 1, 2, 11):
        (p, m, v), (p6, m6, v6) = r32[k], r64[k]
        scale = np.maximum(np.abs(p6), A.LR)
        assert float((np.abs(p - p6) / np.spacing(scale.astype(np.float32))).max()) <= 4 * (k + 1)
        # m mixes both signs (cancellation): measured against the largest gradient magnitude that entered it
        gmax = np.max(np.abs(np.stack(gs[:k + 1])), axis=0)
        assert float((np.abs(m - m6) / np.spacing(np.maximum(gmax * (1 - A.BETA1), 1e-30).astype(np.float32))).max()) <= 16
        assert float(A.ulps32(v, np.maximum(v6, 1e-30)).max()) <= 16


def test_tf_form_is_not_torch_optim_adam():
    """with |g| << eps the two forms differ by the factor sqrt(1 - beta2^t): TF's first step is lr * g * sqrt(1 - b2) / eps-ish, torch's
    lr * g / eps.  The oracle follows the TF closed form and is far from torch's; where |g| >> eps both give lr * sign(g)."""
    g = np.full(8, 1e-10, np.float32)
    p0 = np.zeros(8, np.float32)
    tf32, tf64, th64 = A.run32(p0, [g], eps=1e-8)[0][0], A.closed64(p0, [g], eps=1e-8)[0][0], A.torch_form64(p0, [g], eps=1e-8)[0]
    # TF: alpha m / (sqrt(v) + eps) = lr sqrt(.001) / .1 * 1e-11 / (sqrt(1e-23) + 1e-8);  torch: lr * 1e-10 / (1e-10 + 1e-8)
    assert np.allclose(tf32, tf64, rtol=1e-5, atol=0)
    assert np.all(np.abs(tf64 - th64) > 0.5 * np.abs(th64))
    assert np.all(np.abs(tf32 - th64) > 0.5 * np.abs(th64))
    big = np.full(8, 3.0, np.float32)
    a, b = A.closed64(p0, [big])[0][0], A.torch_form64(p0, [big])[0]
    assert np.allclose(a, -A.LR, rtol=1e-6) and np.allclose(b, -A.LR, rtol=1e-6)
    # torch.optim.Adam itself is the form restated above
    import torch
    t = torch.zeros(8, dtype=torch.float64, requires_grad=True)
    f = lambda x: float(np.float32(x))
    opt = torch.optim.Adam([t], lr=f(A.LR), betas=(f(A.BETA1), f(A.BETA2)), eps=f(1e-8))
    t.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    assert np.allclose(t.detach().numpy(), th64, rtol=1e-9, atol=0)


def test_beta_powers_are_float32_products():
    for beta in (A.BETA1, A.BETA2, 0.5):
        p = np.float32(beta)
        for k in range(13):
            got = A.powers(beta, k)
            assert got.dtype == np.float32 and got == p
            p = np.float32(p * np.float32(beta))
    # ... which is not the float32 rounding of beta ** k
    assert any(A.powers(A.BETA1, k) != np.float32(A.BETA1 ** (k + 1)) for k in range(1, 40))


def test_zero_gradients_move_nothing_in_the_oracle():
    p0 = A.values(65, 3)
    for p, m, v in A.run32(p0, _grads(65, 3, "zeros")):
        assert p.tobytes() == p0.tobytes() and not m.any() and not v.any()


def test_oracle_intermediates_stay_normal():
    """the GPU cases assert nothing about denormals: every value the oracle produces for them is a normal float32 or an exact zero"""
    tiny = np.finfo(np.float32).tiny
    for kind in ("mixed", "some_zeros"):
        for p, m, v in A.run32(A.values(4097, 5), _grads(4097, 12, kind)):
            for x in (p, m, v):
                assert np.all((x == 0) | (np.abs(x) >= tiny))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refused(lib, rc, who, words):
    msg = lib.hmmr_last_error()
    assert rc == -1 and msg and who.encode() in msg and words.encode() in msg, (rc, msg, words)
    with pytest.raises(L.HmmrError):
        L.check(rc, who)


@pytest.mark.parametrize("name,change,words", A.ADAM_REFUSALS, ids=[r[0] for r in A.ADAM_REFUSALS])
def test_adam_step_refuses_before_anything_is_queued(name, change, words):
    lib = L.load()
    kw = dict(p=0x1000, g=0x4000, m=0x8000, v=0xC000, n=5, n_segs=3, segs=True, h=True, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
              beta1_power=0.9, beta2_power=0.999)
    kw.update(change)
    segs = (L.AdamSeg * 3)()
    segs[0].p, segs[0].g, segs[0].m, segs[0].v, segs[0].n = 0x100000, 0x200000, 0x300000, 0x400000, 9
    segs[1].p, segs[1].g, segs[1].m, segs[1].v, segs[1].n = kw["p"], kw["g"], kw["m"], kw["v"], kw["n"]       # the segment under test
    segs[2].n = 0
    h = L.AdamHyper(*[kw[k] for k in ("lr", "beta1", "beta2", "eps", "beta1_power", "beta2_power")])
    rc = lib.hmmr_adam_step(segs if kw["segs"] else None, kw["n_segs"], C.byref(h) if kw["h"] else None, None)
    _refused(lib, rc, "hmmr_adam_step", words)


def test_adam_step_with_nothing_to_do_queues_nothing():
    """no segment, only skipped segments (n = 0, or no gradient): 0 without a launch -- there is no device here to launch on"""
    lib = L.load()
    h = L.AdamHyper(1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999)
    assert lib.hmmr_adam_step(None, 0, C.byref(h), None) == 0
    segs = (L.AdamSeg * 2)()
    segs[0].p, segs[0].m, segs[0].v, segs[0].n = 0x1000, 0x2000, 0x3000, 7          # g NULL
    assert lib.hmmr_adam_step(segs, 2, C.byref(h), None) == 0


@pytest.mark.parametrize("name,change,words", A.MSE_REFUSALS, ids=[r[0] for r in A.MSE_REFUSALS])
def test_strip_mse_refuses_before_anything_is_queued(name, change, words):
    lib = L.load()
    kw = dict(a=0x1000, lda=7, b=0x2000, ldb=7, rows=3, cols=7, weight=1.0, loss=0x3000, d_a=0x4000, ld_da=7, d_b=0x5000, ld_db=7, ws=0x6000,
              ws_bytes=256)
    kw.update(change)
    rc = lib.hmmr_strip_mse(*[kw[k] for k in "a lda b ldb rows cols weight loss d_a ld_da d_b ld_db ws ws_bytes".split()], None)
    _refused(lib, rc, "hmmr_strip_mse", words)


def test_strip_mse_workspace_query():
    lib = L.load()
    assert lib.hmmr_strip_mse_workspace_bytes(0) == 0 and lib.hmmr_strip_mse_workspace_bytes(-3) == 0
    assert lib.hmmr_strip_mse_workspace_bytes(1) == 256 and lib.hmmr_strip_mse_workspace_bytes(32) == 256
    assert lib.hmmr_strip_mse_workspace_bytes(33) == 512 and lib.hmmr_strip_mse_workspace_bytes(40) >= 40 * 8


# ---------------------------------------------------------------------------------------------------------------- optim.TFAdam
class _NoEngine(object):
    def adam_step(self, *a, **k):
        raise AssertionError("no step is made here")


def test_tfadam_state_dict_names_and_beta_powers():
    import torch
    from human_dynamics_amd.optim import TFAdam
    ts = [torch.zeros(3, 4), torch.zeros(5)]
    opt = TFAdam(_NoEngine(), ts, lr=1e-3)
    assert opt.beta1_power == np.float32(0.9) and opt.beta2_power == np.float32(0.999)
    assert type(opt.beta1_power) is np.float32 and type(opt.beta2_power) is np.float32
    assert [tuple(m.shape) for m in opt.m] == [(3, 4), (5,)] and not any(bool(x.any()) for x in opt.m + opt.v)
    assert TFAdam.slot_names("AZ_FC_block1/conv1/weights") == ("AZ_FC_block1/conv1/weights/Adam", "AZ_FC_block1/conv1/weights/Adam_1")
    names = {0: "scope/fc1/weights", 1: "scope/fc1/biases"}
    conv = lambda tensors: {names[i]: t.numpy() + (1 if tensors is opt.v else 0) for i, t in enumerate(tensors)}
    sd = opt.state_dict(conv)
    assert sorted(sd) == sorted(["beta1_power", "beta2_power", "scope/fc1/weights/Adam", "scope/fc1/weights/Adam_1", "scope/fc1/biases/Adam",
                                 "scope/fc1/biases/Adam_1"])
    assert not sd["scope/fc1/weights/Adam"].any() and (sd["scope/fc1/weights/Adam_1"] == 1).all()       # Adam = m, Adam_1 = v
    # the round trip through the index names
    opt.v[1].fill_(2.0)
    opt.beta1_power = A.powers(0.9, 3)
    other = TFAdam(_NoEngine(), [torch.zeros(3, 4), torch.zeros(5)], lr=1e-3).load_state_dict(opt.state_dict())
    assert other.beta1_power == A.powers(0.9, 3) and bool((other.v[1] == 2).all()) and not bool(other.m[0].any())
    ts[0].grad = torch.ones(3, 4)
    opt.zero_grad()
    assert ts[0].grad is None
