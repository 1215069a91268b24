"""The derivative of f_movie's temporal encoder and of the hallucinator on the device (csrc/movie_grad.hip: hmmr_temporal_bwd,
hmmr_hallucinator_bwd) and their Python routes (HmmrEngine.temporal_train / temporal_backward / hallucinate_train / hallucinate_backward,
movie_autograd.temporal_apply / hallucinate_apply) against torch.autograd in float64.

The strips and every gradient are compared SEPARATELY with the float64 autograd of the restated oracle (tests/movie_grad_cases.py, pinned to
oracle.hmmr_oracle by tests/test_movie_grad_cases.py).  The bound is not a chosen number: E32 = |autograd in float32 - autograd in float64|
over the case's group is the error of the same computation in fp32, and a kernel may be FACTOR times that away.  Every compared case runs
on weights prepared for it (GroupNorm betas / fc biases nudged so that no pre-activation lies within rounding distance of zero), written
into the bank's views.  With `-s` every case prints its error, E32 and their ratio, and the module prints the largest ratio per quantity at
the end (profiles/movie_grad_sweep.log is one such run).  Every call in this file is a valid call; the refusals are in
tests/test_movie_grad_cases.py."""
import numpy as np
import pytest
import torch

import movie_grad_cases as MC
import tail_cases as TC

pytestmark = pytest.mark.gpu
_STATS = {}
_ENGINES = {}
_RESULTS = {}


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _engine(device, blocks):
    """an all-fp32 engine of `blocks` temporal blocks; the three-block one holds the hallucinator, the one-block one the regressors"""
    key = (device, blocks)
    if key not in _ENGINES:
        from human_dynamics_amd import _lib as L
        from human_dynamics_amd.engine import HmmrEngine
        held = {v for i in range(blocks) for v in MC.block_vars(i).values()}
        ief = tuple(TC.delta_scope(d) + "/" for d in (-5, 5)) + ("single_view_ief/", "mean_param")
        w = {k: v for k, v in TC.weights().items() if k in held or (blocks == 3 and k.startswith("fc2_res/")) or (blocks == 1 and k.startswith(ief))}
        eng = HmmrEngine(w, None, dtype="f32", device=device, num_conv_layers=blocks, delta_t_values=(-5, 5))
        bank = eng.movie_bank()
        assert (bank.tw.dtype, bank.tw.num_blocks, bank.hw is not None) == (L.HMMR_F32, blocks, blocks == 3)
        _ENGINES[key] = eng
    return _ENGINES[key]


def _load(eng, prepared=None):
    """the checkpoint's GroupNorm betas and fc biases, then the prepared ones of a case, into the bank's views"""
    bank = eng.movie_bank()
    names = [v for i in range(bank.num_blocks) for k, v in MC.block_vars(i).items() if k.endswith("_beta")]
    if bank.hal is not None:
        names += [MC.HAL_VARS[k] for k in ("b1", "b2", "b3")]
    ck = {n: TC.weights()[n] for n in names}
    ck.update(prepared or {})
    bank.load_checkpoint(ck)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k, (r, tag) in sorted(_STATS.items()):
        print("movie_grad summary: largest err / E32 of %-24s: %5.2f (%s)" % (k, r, tag))
    _ENGINES.clear()
    _RESULTS.clear()


def _note(key, tag, err, bound):
    e = bound / MC.FACTOR
    ratio = err / e if e > 0 else (0.0 if err == 0 else float("inf"))
    print("movie_grad %-14s %-24s err %.3e  E32 %.3e  ratio %5.2f" % (tag, key, err, e, ratio))
    if ratio > _STATS.get(key, (-1.0, ""))[0]:
        _STATS[key] = (ratio, tag)


def _check(tag, got, ref, bnd, prefix=""):
    for k, err in MC.errors(got, ref).items():
        assert np.isfinite(got[k]).all(), (tag, k)
        _note(prefix + k, tag, err, bnd[k])
        assert err <= bnd[k], (tag, k, err, bnd[k])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _same_result(a, b):
    return sorted(a) == sorted(b) and all(_same_bits(a[k], b[k]) for k in a)


def _n(x):
    return None if x is None else x.cpu().numpy()


def _run_temporal(eng, phi, cot, **kw):
    """engine.temporal_train + engine.temporal_backward -> {quantity: float32 array} named as movie_grad_cases names them"""
    strips = eng.temporal_train(phi)
    d_phi, grads = eng.temporal_backward(phi, cot, **kw)
    q = {"strips": _n(strips), "d_phi": _n(d_phi)}
    for i, g in enumerate(grads):
        q.update({"b%d/%s" % (i, n): _n(v) for n, v in g.items()})
    return {k: v for k, v in q.items() if v is not None}


def _run_hal(eng, phi, cot, **kw):
    out = eng.hallucinate_train(phi)
    d_phi, g = eng.hallucinate_backward(phi, cot, **kw)
    q = {"out": _n(out), "d_phi": _n(d_phi)}
    q.update({n: _n(v) for n, v in g.items()})
    return {k: v for k, v in q.items() if v is not None}


def _result(device, case):
    """the case's full result on its prepared weights, computed once per module for the cases other tests read again"""
    if case.name not in _RESULTS:
        if isinstance(case, MC.TCase):
            eng = _engine(device, case.blocks)
            _load(eng, MC.prepared(case)[0])
            _RESULTS[case.name] = _run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case))
        else:
            eng = _engine(device, 3)
            _load(eng, MC.prepared(case)[0])
            _RESULTS[case.name] = _run_hal(eng, MC.phi_of(case), MC.cotangent_of(case))
    return _RESULTS[case.name]


# ---------------------------------------------------------------------------------------------------------------- a. against the oracle
@pytest.mark.parametrize("case", MC.TEMPORAL_CASES, ids=lambda c: c.name)
def test_temporal_case_matches_float64_autograd(case, gpu_device):
    """the strips and every gradient within FACTOR x E32; a second call gives the same bytes"""
    eng = _engine(gpu_device, case.blocks)
    _load(eng, MC.prepared(case)[0])
    got = _run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case))
    if case.name in ("b2_t7_n3", "b5_t7_n1", "b2_t7_n1"):
        _RESULTS[case.name] = got
    _check(case.name, got, MC.reference(case), MC.bounds(case))
    assert _same_result(got, _run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case))), case.name


@pytest.mark.parametrize("case", MC.HAL_CASES, ids=lambda c: c.name)
def test_hallucinator_case_matches_float64_autograd(case, gpu_device):
    eng = _engine(gpu_device, 3)
    _load(eng, MC.prepared(case)[0])
    got = _run_hal(eng, MC.phi_of(case), MC.cotangent_of(case))
    if case.name == "m14":
        _RESULTS[case.name] = got
    _check(case.name, got, MC.reference(case), MC.bounds(case), "hal/")
    assert _same_result(got, _run_hal(eng, MC.phi_of(case), MC.cotangent_of(case))), case.name


def test_train_forwards_are_the_inference_forwards_of_an_fp32_engine(gpu_device):
    """on the checkpoint's own weights, bank and inference pack hold the same numbers: the same launches, the same bytes"""
    eng = _engine(gpu_device, 3)
    _load(eng)
    phi = TC.phi_input(3, 20, 5)
    assert _same_bits(_n(eng.temporal_train(phi)), _n(eng.temporal(phi)))
    assert _same_bits(_n(eng.hallucinate_train(phi)), _n(eng.hallucinate(phi)))
    eng1 = _engine(gpu_device, 1)
    _load(eng1)
    assert _same_bits(_n(eng1.temporal_train(phi[:1, :1])), _n(eng1.temporal(phi[:1, :1])))


# ---------------------------------------------------------------------------------------------------------------- b. outputs
ALL3 = [list(MC.BLOCK_NAMES)] * 3
TEMPORAL_SUBSETS = {
    "d_phi": (True, False),
    "weights": (False, True),
    "top_conv2": (False, [[], [], ["conv2"]]),                         # the chain stops inside the last block: one weight gradient, no data gradient
    "top_b2": (False, [[], [], ["b2"]]),
    "top_gn2": (False, [[], [], ["gn2_gamma"]]),
    "mid_gn1_beta": (False, [[], ["gn1_beta"], ["b1"]]),
    "low_b1_and_d_phi": (True, [["b1"], [], []]),
    "low_conv1": (False, [["conv1"], [], []]),
    "one_of_each": (False, [["gn1_gamma", "b2"], ["conv2", "gn2_beta"], ["conv1", "gn1_beta"]]),
}


@pytest.mark.parametrize("name", sorted(TEMPORAL_SUBSETS))
def test_temporal_subsets_give_the_bytes_of_the_full_call(name, gpu_device):
    case = MC.T_BY_NAME["b2_t7_n3"]
    full = _result(gpu_device, case)
    eng = _engine(gpu_device, 3)
    _load(eng, MC.prepared(case)[0])
    want_phi, want_w = TEMPORAL_SUBSETS[name]
    got = _run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case), want_phi=want_phi, want_weights=want_w)
    wanted = {"strips"} | ({"d_phi"} if want_phi else set())
    wanted |= {"b%d/%s" % (i, n) for i in range(3) for n in (MC.BLOCK_NAMES if want_w is True else (want_w[i] if want_w else ()))}
    assert set(got) == wanted
    for k in got:
        assert _same_bits(got[k], full[k]), (name, k)


@pytest.mark.parametrize("want_phi,names", [(True, ()), (False, ("b3",)), (False, ("fc3",)), (False, ("b2",)), (False, ("fc2", "b3")), (False, ("fc1",)),
                                            (False, ("b1", "fc3")), (True, ("fc2",)), (False, MC.HAL_NAMES)],
                         ids=["d_phi", "b3", "fc3", "b2", "fc2_b3", "fc1", "b1_fc3", "d_phi_fc2", "weights"])
def test_hallucinator_subsets_give_the_bytes_of_the_full_call(want_phi, names, gpu_device):
    case = MC.H_BY_NAME["m14"]
    full = _result(gpu_device, case)
    eng = _engine(gpu_device, 3)
    _load(eng, MC.prepared(case)[0])
    got = _run_hal(eng, MC.phi_of(case), MC.cotangent_of(case), want_phi=want_phi, want_weights=list(names))
    assert set(got) == {"out"} | ({"d_phi"} if want_phi else set()) | set(names)
    for k in got:
        assert _same_bits(got[k], full[k]), k


# ---------------------------------------------------------------------------------------------------------------- c. windows and rows
def test_a_window_does_not_depend_on_the_other_windows(gpu_device):
    """window 2 of the (5, 7) call: its d_phi (and its strips) equal, bit for bit, those of the window run alone; a d_strips that is
    non-zero in window 0 only leaves d_phi of every other window exactly 0.0"""
    case = MC.T_BY_NAME["b5_t7_n1"]
    full = _result(gpu_device, case)
    eng = _engine(gpu_device, 1)
    _load(eng, MC.prepared(case)[0])
    phi, cot = MC.phi_of(case), MC.cotangent_of(case)
    alone = _run_temporal(eng, phi[2:3], cot[2:3], want_weights=False)
    assert _same_bits(alone["d_phi"], full["d_phi"][2:3]) and _same_bits(alone["strips"], full["strips"][2:3])
    only0 = np.zeros_like(cot)
    only0[0] = cot[0]
    got = _run_temporal(eng, phi, only0, want_weights=False)
    assert np.abs(got["d_phi"][0]).max() > 0.1 and (got["d_phi"][1:] == 0.0).all()
    assert _same_bits(got["d_phi"][0], _run_temporal(eng, phi[:1], cot[:1], want_weights=False)["d_phi"][0])


def test_a_hallucinator_row_does_not_depend_on_the_other_rows(gpu_device):
    case = MC.H_BY_NAME["m14"]
    full = _result(gpu_device, case)
    eng = _engine(gpu_device, 3)
    _load(eng, MC.prepared(case)[0])
    phi, cot = MC.phi_of(case), MC.cotangent_of(case)
    alone = _run_hal(eng, phi[5:6], cot[5:6], want_weights=False)
    assert _same_bits(alone["d_phi"], full["d_phi"][5:6]) and _same_bits(alone["out"], full["out"][5:6])


# ---------------------------------------------------------------------------------------------------------------- d. the bank's views
def test_an_in_place_update_is_what_the_next_calls_read(gpu_device):
    """the last block's conv2 doubled in place (no pre-activation moves): the next forward is the float64 function of the doubled weights,
    and everything below conv2 in the next backward is exactly twice what it was"""
    case = MC.T_BY_NAME["b2_t7_n1"]
    before = _result(gpu_device, case)
    eng = _engine(gpu_device, 1)
    prepared = MC.prepared(case)[0]
    _load(eng, prepared)
    conv2 = eng.movie_bank().blocks[0]["conv2"]
    name = MC.block_vars(0)["conv2"]
    try:
        with torch.no_grad():
            conv2 *= 2.0
        got = _run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case))
    finally:
        with torch.no_grad():
            conv2 *= 0.5
    assert not _same_bits(got["strips"], before["strips"])
    ref = MC.temporal_autograd(case, torch.float64, betas=dict(prepared, **{name: 2.0 * np.asarray(TC.weights()[name], np.float64)}))
    bnd = MC.bounds(case)
    for k in ("strips", "b0/b1", "b0/conv1", "b0/gn1_gamma", "d_phi"):
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        assert err <= 2.0 * bnd[k], (k, err, bnd[k])                                   # (every term below conv2 is doubled, and so is its error)
    for k in ("b0/b1", "b0/conv1", "b0/gn2_gamma", "b0/gn2_beta", "b0/gn1_gamma", "b0/gn1_beta"):
        assert _same_bits(got[k], 2.0 * before[k]), k
    assert _same_bits(got["b0/conv2"], before["b0/conv2"]) and _same_bits(got["b0/b2"], before["b0/b2"])
    assert _same_result(_run_temporal(eng, MC.phi_of(case), MC.cotangent_of(case)), before)              # ... and the bank is as it was found


# ---------------------------------------------------------------------------------------------------------------- e. autograd
def _grads_on(tensors):
    class _Scope(object):
        def __enter__(self):
            for t in tensors:
                t.requires_grad_()

        def __exit__(self, *exc):
            for t in tensors:
                t.grad = None
                t.requires_grad_(False)
    return _Scope()


def test_autograd_through_f_movie_and_the_regressors_gives_the_bytes_of_the_two_backwards(gpu_device):
    """temporal_apply -> ief_apply -> sum(omegas * fixed), .backward(): on both banks and on phi, byte for byte what engine.ief_backward
    followed by engine.temporal_backward gives"""
    from human_dynamics_amd.ief_autograd import ief_apply
    from human_dynamics_amd.ief_bank import NAMES as IEF_NAMES
    from human_dynamics_amd.movie_autograd import temporal_apply
    case = MC.T_BY_NAME["b2_t7_n1"]
    eng = _engine(gpu_device, 1)
    _load(eng, MC.prepared(case)[0])
    b, t = case.b, case.t
    phi_np = MC.phi_of(case)
    fixed = torch.from_numpy(MC._rng(9, b, t).standard_normal((3, b * t, 85)).astype(np.float32)).to(gpu_device)
    # by hand
    strips = eng.temporal_train(phi_np)
    d_strips, _, ief_grads = eng.ief_backward(strips.reshape(b * t, 2048), fixed)
    d_phi, t_grads = eng.temporal_backward(phi_np, d_strips.reshape(b, t, 2048))
    # by autograd
    tt, it = eng.movie_bank().temporal_tensors(), eng.ief_bank().tensors()
    phi = torch.from_numpy(phi_np).to(gpu_device).requires_grad_()
    with _grads_on(tt + it):
        om = ief_apply(eng, temporal_apply(eng, phi).reshape(b * t, 2048))
        (om * fixed).sum().backward()
        assert _same_bits(_n(phi.grad), _n(d_phi))
        for i, n in enumerate(MC.BLOCK_NAMES):
            assert _same_bits(_n(tt[i].grad), _n(t_grads[0][n])), n
        for r in range(3):
            for i, n in enumerate(IEF_NAMES):
                assert _same_bits(_n(it[7 * r + i].grad), _n(ief_grads[r][n])), (r, n)
        # a leaf that does not require a gradient gets none, and an absent cotangent queues nothing
        for x in tt + it:
            x.grad = None
        tt[2].requires_grad_(False)
        strips2 = temporal_apply(eng, torch.from_numpy(phi_np).to(gpu_device))
        strips2.sum().backward()
        assert tt[2].grad is None and tt[3].grad is not None


def test_e_hallucinate_reaches_both_modules(gpu_device):
    """mse(hallucinate_apply(phi), temporal_apply(phi)) (src/trainer_sequence_fc.py:839-846, no stop-gradient) on the (2, 7, 3) case:
    the loss, d_phi and every gradient of both modules within FACTOR x E32 of the composed function's float64 autograd"""
    from human_dynamics_amd.movie_autograd import hallucinate_apply, temporal_apply
    eng = _engine(gpu_device, 3)
    betas, biases = MC.hal_chain_prepared()
    _load(eng, dict(betas, **biases))
    bank = eng.movie_bank()
    tt, ht = bank.temporal_tensors(), bank.hallucinator_tensors()
    phi = torch.from_numpy(MC.hal_chain_phi()).to(gpu_device).requires_grad_()
    with _grads_on(tt + ht):
        loss = torch.mean((hallucinate_apply(eng, phi) - temporal_apply(eng, phi)) ** 2)
        loss.backward()
        got = {"loss": _n(loss.detach()).reshape(1), "d_phi": _n(phi.grad)}
        got.update({"t/b%d/%s" % (i, n): _n(tt[8 * i + j].grad) for i in range(3) for j, n in enumerate(MC.BLOCK_NAMES)})
        got.update({"h/" + n: _n(ht[j].grad) for j, n in enumerate(MC.HAL_NAMES)})
    ref, bnd = MC.hal_chain_reference()
    _check("e_hallucinate", got, ref, bnd, "chain ")


def test_twelve_descent_steps_follow_the_float64_run(gpu_device):
    """plain gradient descent on the one-block bank's tensors in place (fixed step): the next call sees the update, and the loss follows
    the float64 run's within FACTOR x the float32 run's deviation, measured on the host (movie_grad_cases.descent_reference)"""
    from human_dynamics_amd.movie_autograd import temporal_apply
    case = MC.DESCENT_CASE
    d64, bound = MC.descent_reference()
    eng = _engine(gpu_device, 1)
    _load(eng, MC.prepared(case)[0])
    bank = eng.movie_bank()
    tensors = bank.temporal_tensors()
    before = [x.clone() for x in tensors]
    phi = torch.from_numpy(MC.phi_of(case)).to(gpu_device)
    target = torch.from_numpy(MC.descent_target()).to(gpu_device)
    got = []
    try:
        with _grads_on(tensors):
            for _ in range(MC.DESCENT_STEPS + 1):
                loss = torch.mean((temporal_apply(eng, phi, tensors) - target) ** 2)
                got.append(float(loss.detach()))
                loss.backward()
                with torch.no_grad():
                    for x in tensors:
                        x -= MC.DESCENT_LR * x.grad
                        x.grad = None
    finally:
        with torch.no_grad():
            for x, v in zip(tensors, before):
                x.copy_(v)
    for i, (g, r, bd) in enumerate(zip(got, d64, bound)):
        print("movie_grad descent step %2d: device %.7f  float64 %.7f  deviation %.2e  allowed %.2e" % (i, g, r, abs(g - r), bd))
    assert all(abs(g - r) <= bd for g, r, bd in zip(got, d64, bound)), (got, d64, bound)
