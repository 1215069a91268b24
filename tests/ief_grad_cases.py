"""Cases, the torch oracle and the error bounds of the IEF backward (tests/test_ief_grad_cases.py on the host, tests/test_gpu_ief_grad.py on
the device): hmmr_ief_fwd_train / hmmr_ief_bwd of csrc/ief_grad.hip.  No GPU is needed by anything in here.

The oracle restates the function of include/hmmr_hip.h ("IEF backward") in torch with the weights as leaf tensors (oracle.hmmr_oracle.hmr_ief
converts them through NumPy, where autograd cannot follow); weights and inputs are tests/tail_cases.py's, and with no mask its forward is
pinned to tail_cases.compose_ief in float64 (test_ief_grad_cases.py), the composition that is itself pinned to the reference.

The bound is the project's rule: E32 = |autograd in float32 - autograd in float64| over the cases of one group, per output quantity (omegas,
d_strips, d_omega_start, each of the seven weight gradients per regressor kind, present / delta); a kernel may be FACTOR times that away from
the float64 result.

ReLU kinks.  A pre-activation within rounding distance of zero takes one sign in float32 and the other in float64, and its whole gradient path
then differs by a full-size term: a property of the function, not an error of a kernel.  So every case that is compared with the oracle carries
a keep mask (all ones with keep_scale 1, or a random 0.5 mask with keep_scale 2) in which every AMBIGUOUS unit is cleared: |a_float64| <= tau,
tau = 16 x the float32-against-float64 error of the pre-activations over the case's group; cleared again until no unmasked unit is ambiguous
(clearing a unit moves the later pre-activations).  Kernel and oracle then agree on every unit that counts, whatever sign the kernel computes
for the cleared ones.  test_ief_grad_cases.py asserts for every case that at most 1e-4 of the units are cleared, within 4 rounds.  The
keep == NULL path is compared on one tiny case whose seed is searched until no unit at all is ambiguous."""
import collections
import functools

import numpy as np
import torch

import tail_cases as TC

FACTOR = 4.0              # tests/tail_cases.py's rule: 4, or the smallest power of two that leaves 1.5 x over the largest measured, understood ratio (16 at most)
TAU_FACTOR = 16.0
MAX_CLEARED = 1e-4        # of a case's units
MAX_ROUNDS = 4
NAMES = ("fc1_phi", "fc1_theta", "fc2", "fc3", "b1", "b2", "b3")            # the bank's tensors, in the order of hmmr_ief_reg_grads_t
DELTAS_OF = {1: (), 2: (5,), 3: (-5, 5), 8: TC.DELTAS7}

Case = collections.namedtuple("Case", "name m R stages width from_pred start keep seed")


def _case(name, m, R, stages=3, width=72, from_pred=True, start="rows", keep="half", seed=1):
    return Case(name, m, R, stages, width, from_pred, start, keep, seed)


# every value of every axis with m = 33, R = 3; the other m and R once each; no cross product
CASES = (
    _case("m33_R3", 33, 3, seed=1),
    _case("m33_R3_stage1", 33, 3, stages=1, seed=2),
    _case("m33_R3_w75", 33, 3, width=75, seed=3),
    _case("m33_R3_from_start", 33, 3, from_pred=False, seed=4),
    _case("m33_R3_mean_start", 33, 3, start=None, seed=5),
    _case("m33_R3_ones", 33, 3, keep="ones", seed=6),
    _case("m33_R3_w75_from_start_stage1_mean_ones", 33, 3, stages=1, width=75, from_pred=False, start=None, keep="ones", seed=7),
    _case("m33_R1", 33, 1, seed=8),
    _case("m33_R2", 33, 2, seed=9),
    _case("m1_R3", 1, 3, seed=10),
    _case("m7_R3", 7, 3, seed=1),              # the rows 0..6 of m33_R3 (same seed: tail_cases' inputs are drawn per (seed, m), so they are cut from it)
    _case("m7_R8", 7, 8, seed=11),
    _case("m86_R3", 86, 3, seed=12),
    _case("m160_R3", 160, 3, seed=13),
)
BY_NAME = {c.name: c for c in CASES}


def group_of(case):
    """the cases whose E32 and tau are taken together: one function (stages, width, wiring, kind of mask), any m, R, seed and start"""
    return (case.stages, case.width, case.from_pred, case.keep)


def cases_of(group):
    return tuple(c for c in CASES if group_of(c) == group)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def keys_of(case):
    return (0,) + tuple(sorted(DELTAS_OF[case.R]))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """strips [m, 2048], start [m, 85] (the mean theta in every row for start None), d_omegas [R, m, 85] float32, the mask as drawn
    keep0 uint8 [R, S, 2, m, 1024] and keep_scale.  m7_R3 is rows 0..6 of m33_R3 in every input (row independence)."""
    if case.name == "m7_R3":
        big = inputs(BY_NAME["m33_R3"])
        return dict(strips=big["strips"][:7].copy(), start=big["start"][:7].copy(), d_omegas=big["d_omegas"][:, :7].copy(),
                    keep0=big["keep0"][:, :, :, :7].copy(), scale=big["scale"])
    w = TC.ief_weights(case.width)
    strips = TC.strips_input(case.m, case.seed)
    start = TC.omega_rows(case.m, case.seed) if case.start == "rows" else TC.start_rows(None, case.m, w)
    d_omegas = _rng(5, case.seed, case.m, case.R).standard_normal((case.R, case.m, 85)).astype(np.float32)
    shape = (case.R, case.stages, 2, case.m, 1024)
    if case.keep == "half":
        keep0 = (_rng(6, case.seed, case.m, case.R).random(shape) < 0.5).astype(np.uint8)
    else:
        keep0 = np.ones(shape, np.uint8)
    return dict(strips=strips, start=np.asarray(start, np.float32), d_omegas=d_omegas, keep0=keep0, scale=2.0 if case.keep == "half" else 1.0)


def scope_of(key):
    return "single_view_ief" if key == 0 else TC.delta_scope(key)


def params(width, keys, dtype, requires_grad=True, source=None):
    """[{W1 [2048 + nd, 1024], b1, W2, b2, W3 [1024, nd], b3}] per regressor: leaf tensors in the checkpoint's shapes"""
    w = TC.ief_weights(width) if source is None else source
    out = []
    for k in keys:
        p = scope_of(k) + "/3D_module/"
        leaf = lambda name: torch.tensor(np.asarray(w[p + name], np.float64), dtype=dtype).requires_grad_(requires_grad)
        out.append(dict(W1=leaf("fc1/weights"), b1=leaf("fc1/biases"), W2=leaf("fc2/weights"), b2=leaf("fc2/biases"),
                        W3=leaf("fc3/weights"), b3=leaf("fc3/biases")))
    return out


# ---------------------------------------------------------------------------------------------------------------- the oracle
def forward(P, strips, start, keep, scale, stages, width, from_pred, pre=None):
    """The function of include/hmmr_hip.h, "IEF backward": P = params(), strips [m, 2048], start [m, 85] (tensors of P's dtype), keep a
    {0, 1} tensor [R, S, 2, m, 1024] of that dtype or None -> omegas [R, m, 85].  pre: a list that receives every pre-activation
    (a1, a2 per stage, regressor after regressor)."""
    def regress(p, theta, kp):
        for s in range(stages):
            a1 = strips @ p["W1"][:2048] + p["b1"] + theta @ p["W1"][2048:]
            h1 = torch.relu(a1) if kp is None else torch.relu(a1) * kp[s, 0] * scale
            a2 = h1 @ p["W2"] + p["b2"]
            h2 = torch.relu(a2) if kp is None else torch.relu(a2) * kp[s, 1] * scale
            theta = theta + h2 @ p["W3"] + p["b3"]
            if pre is not None:
                pre.extend([a1.detach(), a2.detach()])
        return theta
    kp = lambda r: None if keep is None else keep[r]
    omega0 = regress(P[0], start, kp(0))
    out = [omega0]
    for r in range(1, len(P)):
        src = omega0 if from_pred else start                      # no stop-gradient (src/models.py:343-361)
        d = regress(P[r], src[:, 3:75] if width == 72 else src[:, :75], kp(r))
        n = d.shape[0]
        if width == 72:
            out.append(torch.cat([torch.ones(n, 1, dtype=d.dtype), torch.zeros(n, 2, dtype=d.dtype), d, src[:, 75:]], dim=1))
        else:
            out.append(torch.cat([d, src[:, 75:]], dim=1))
    return torch.stack(out)


def _pre(case, inp, keep, dtype):
    """every pre-activation of the case under the mask `keep` (uint8 or None), as one float64 array [R S 2, m, 1024]"""
    pre = []
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    with torch.no_grad():
        forward(params(case.width, keys_of(case), dtype, False), t(inp["strips"]), t(inp["start"]), None if keep is None else t(keep),
                inp["scale"], case.stages, case.width, case.from_pred, pre)
    return torch.stack(pre).to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def tau_of(group):
    """TAU_FACTOR x the largest |float32 - float64| of a pre-activation over the group's cases, under the masks as drawn"""
    worst = 0.0
    for c in cases_of(group):
        inp = inputs(c)
        worst = max(worst, float(np.abs(_pre(c, inp, inp["keep0"], torch.float32) - _pre(c, inp, inp["keep0"], torch.float64)).max()))
    return TAU_FACTOR * worst


def clear_ambiguous(case, inp, tau):
    """-> (keep with every ambiguous unit cleared, units cleared, rounds).  A round clears the unmasked units with |a_float64| <= tau;
    the last round finds none."""
    keep = inp["keep0"].copy()
    shape = keep.shape
    rounds = 0
    while True:
        a = _pre(case, inp, keep, torch.float64).reshape(shape)        # (regressor, stage, layer) is the order the oracle emits them in
        amb = (np.abs(a) <= tau) & (keep != 0)
        if not amb.any():
            break
        keep[amb] = 0
        rounds += 1
        if rounds > 16:
            raise RuntimeError("clear_ambiguous does not end")
    return keep, int((keep != inp["keep0"]).sum()), rounds


@functools.lru_cache(maxsize=None)
def prepared(case):
    """the case's inputs with the final mask: dict(strips, start, d_omegas, keep, scale, cleared, rounds, units, tau)"""
    inp = inputs(case)
    tau = tau_of(group_of(case))
    keep, cleared, rounds = clear_ambiguous(case, inp, tau)
    keep.setflags(write=False)
    return dict(strips=inp["strips"], start=inp["start"], d_omegas=inp["d_omegas"], keep=keep, scale=inp["scale"], cleared=cleared,
                rounds=rounds, units=int(keep.size), tau=tau)


def bank_layout(g, nd):
    """gradients in the checkpoint's shapes {W1, b1, W2, b2, W3, b3} -> the bank's {fc1_phi [1024, 2048], fc1_theta [1024, 128], fc2,
    fc3 [128, 1024], b1, b2, b3 [128]} (float64 numpy, zero padded)"""
    pad = lambda a, shape: np.pad(a, [(0, s - n) for s, n in zip(shape, a.shape)])
    return dict(fc1_phi=np.ascontiguousarray(g["W1"][:2048].T), fc1_theta=pad(g["W1"][2048:].T, (1024, 128)), fc2=np.ascontiguousarray(g["W2"].T),
                fc3=pad(g["W3"].T, (128, 1024)), b1=g["b1"], b2=g["b2"], b3=pad(g["b3"], (128,)))


def autograd(case, inp, keep, dtype, d_omegas=None, source=None):
    """omegas and every gradient of sum(omegas * d_omegas) by torch.autograd in `dtype`, as float64 numpy:
    dict(omegas [R, m, 85], d_strips, d_omega_start, grads = [bank_layout per regressor])"""
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype).requires_grad_(g)
    P = params(case.width, keys_of(case), dtype, True, source)
    strips, start = t(inp["strips"], True), t(inp["start"], True)
    om = forward(P, strips, start, None if keep is None else t(keep), inp["scale"], case.stages, case.width, case.from_pred)
    (om * t(inp["d_omegas"] if d_omegas is None else d_omegas)).sum().backward()
    n64 = lambda x: (torch.zeros_like(x) if x.grad is None else x.grad).to(torch.float64).numpy()
    nds = [85] + [case.width] * (case.R - 1)
    return dict(omegas=om.detach().to(torch.float64).numpy(), d_strips=n64(strips), d_omega_start=n64(start),
                grads=[bank_layout({k: n64(v) for k, v in p.items()}, nd) for p, nd in zip(P, nds)])


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64):
    """autograd() of the prepared case; computed once, nobody writes to it"""
    pc = prepared(case)
    out = autograd(case, pc, pc["keep"], dtype)
    for a in [out["omegas"], out["d_strips"], out["d_omega_start"]] + [g[n] for g in out["grads"] for n in NAMES]:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- E32 and the bound
def quantities(res):
    """{quantity: [arrays]}: omegas, d_strips, d_omega_start, present/<name>, delta/<name> (one array per delta regressor)"""
    q = {"omegas": [res["omegas"]], "d_strips": [res["d_strips"]], "d_omega_start": [res["d_omega_start"]]}
    for n in NAMES:
        q["present/" + n] = [res["grads"][0][n]]
        if len(res["grads"]) > 1:
            q["delta/" + n] = [g[n] for g in res["grads"][1:]]
    return q


def errors(got, ref):
    """{quantity: max |got - ref|} over the quantities of `ref`"""
    qg, qr = quantities(got), quantities(ref)
    return {k: max(float(np.abs(np.asarray(a, np.float64) - b).max()) for a, b in zip(qg[k], qr[k])) for k in qr}


@functools.lru_cache(maxsize=None)
def e32(group):
    """{quantity: the largest |autograd in float32 - autograd in float64| over the group's cases}"""
    out = {}
    for c in cases_of(group):
        for k, v in errors(reference(c, torch.float32), reference(c)).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def bounds(case):
    return {k: FACTOR * v for k, v in e32(group_of(case)).items()}


# ---------------------------------------------------------------------------------------------------------------- the keep == NULL case
NULL_CASE_SHAPE = dict(m=5, R=1, stages=3, width=72, from_pred=True, start="rows", keep="ones")
MAX_NULL_SEEDS = 64


@functools.lru_cache(maxsize=None)
def null_case():
    """-> (case, seeds tried, tau): m = 5, R = 1 without a mask, the first seed (100, 101, ...) at which NO unit is ambiguous, tau =
    TAU_FACTOR x the float32-against-float64 error of that seed's own pre-activations"""
    for tried in range(1, MAX_NULL_SEEDS + 1):
        c = Case(name="null_keep", seed=99 + tried, **NULL_CASE_SHAPE)
        inp = _null_inputs(c)
        a64 = _pre(c, inp, None, torch.float64)
        tau = TAU_FACTOR * float(np.abs(_pre(c, inp, None, torch.float32) - a64).max())
        if not (np.abs(a64) <= tau).any():
            return c, tried, tau
    raise RuntimeError("no seed without an ambiguous unit among %d" % MAX_NULL_SEEDS)


def _null_inputs(c):
    return dict(strips=TC.strips_input(c.m, c.seed), start=TC.omega_rows(c.m, c.seed),
                d_omegas=_rng(5, c.seed, c.m, c.R).standard_normal((c.R, c.m, 85)).astype(np.float32), scale=1.0)


@functools.lru_cache(maxsize=None)
def null_reference(dtype=torch.float64):
    c = null_case()[0]
    return autograd(c, _null_inputs(c), None, dtype)


def null_inputs():
    return _null_inputs(null_case()[0])


def null_bounds():
    return {k: FACTOR * v for k, v in errors(null_reference(torch.float32), null_reference()).items()}


# ---------------------------------------------------------------------------------------------------------------- the workspace
def bwd_workspace_bytes(m, R, S):
    """hmmr_ief_bwd_workspace_bytes as csrc/ief_grad.hip states it (ief_grad_layout; every buffer starts on a multiple of 256 bytes): one
    set per regressor -- pre, h1 and h2 of every stage, theta_0 .. theta_S, d_a1 and d_a2 of every stage, d_theta_0 .. d_theta_S, the
    stage sum of d_a1 -- then the split-K planes of the recomputed forward (one set of 4 per grouped problem), the recomputed omegas, the
    present regressor's cotangent and the deltas' contributions to d_omega_start"""
    r256 = lambda x: (x + 255) // 256 * 256
    wide, narrow = m * 1024 * 4, m * 128 * 4
    one_set = r256(wide) + 2 * r256(S * wide) + r256((S + 1) * narrow) + 2 * r256(S * wide) + r256((S + 1) * narrow) + r256(wide)
    return r256(R * one_set) + r256(max(R - 1, 1) * 4 * m * 1024 * 4) + r256(R * m * 85 * 4) + 2 * r256(m * 85 * 4)


# ---------------------------------------------------------------------------------------------------------------- the chain to the losses
# strips, bank -> the regressors -> trainer_losses.compute_losses_batched (the present container) -> backward, on the 130-vertex model:
# this oracle composed with tests/loss_cases.py's (smpl_grad_cases.forward + losses).  E32 is that of the composed function, per (B, T).
CHAIN_BT = ((2, 5), (8, 20))
CHAIN_NV = 130
DESCENT_BT, DESCENT_STEPS, DESCENT_LR = (2, 5), 12, 2e-5      # chosen on the host: test_ief_grad_cases.py asserts that the float64 run falls at every step


def _loss_cases():
    import loss_cases as LC
    return LC


class ChainCase(object):
    """R = 3 (the engine's default deltas), 72-wide, three stages, the mean theta as the start, a random 0.5 mask with its ambiguous units
    cleared (tau from this case's own pre-activations).  The ground truth is made as loss_cases.LoopCase makes it -- the float64 forward
    of a perturbed omega -- around the omega the float64 oracle predicts, with loss_cases' condition on the keypoint residuals."""

    def __init__(self, B, T, seed):
        LC = _loss_cases()
        self.B, self.T, self.delta_t, self.flags, self.use_optcam, self.weights = B, T, 0, LC.ALL | LC.KP, False, LC.WEIGHTS
        self.name = "chain B%d T%d" % (B, T)
        self.ief = Case(self.name, B * T, 3, 3, 72, True, None, "half", seed)
        inp = inputs(self.ief)
        tau = TAU_FACTOR * float(np.abs(_pre(self.ief, inp, inp["keep0"], torch.float32) - _pre(self.ief, inp, inp["keep0"], torch.float64)).max())
        keep, self.cleared, self.rounds = clear_ambiguous(self.ief, inp, tau)
        self.strips, self.start, self.keep, self.scale, self.tau = inp["strips"], inp["start"], keep, inp["scale"], tau
        t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
        with torch.no_grad():
            om = forward(params(72, keys_of(self.ief), torch.float64, False), t64(self.strips), t64(self.start), t64(keep), self.scale, 3, 72, True)[0].numpy()
        self.omega = np.ascontiguousarray(om, np.float32)
        self.model = LC.G._model(CHAIN_NV)
        self.K = self.model["cocoplus_regressor"].shape[1]
        N = B * T
        f = lambda x: np.ascontiguousarray(x, np.float32)
        rng = _rng(7, seed, B, T)
        ca, th, be = om[:, :3], om[:, 3:75], om[:, 75:]
        th2, be2, ca2 = th + 0.1 * rng.standard_normal(th.shape), be + 0.3 * rng.standard_normal(be.shape), ca + 0.05 * rng.standard_normal(ca.shape)
        with torch.no_grad():
            o = LC.G.forward(self.model, t64(th2), t64(be2), t64(ca2))
        v = (rng.random((N, self.K)) < 0.7).astype(np.float64)
        v[:, 0] = v[:, 1] = 1.0
        self.kps_gt = f(np.concatenate([o["kps"].numpy(), v[:, :, None]], 2))
        self.joints_gt, self.rs_gt = f(o["joints"].numpy()[:, :14]), f(o["Rs"].numpy())
        self.shapes_gt = f(be2.reshape(B, T, 10)[:, 0])
        h = (np.arange(B) % 3 != 1).astype(np.float64)
        self.has_smpl, self.has_joints = f(h), f(h[::-1])
        self._kp64, self._r = None, {}
        LC.enforce_min_residual(self)
        LC.check_conditions(self, None)

    def gt(self, dtype):
        g = {"kps": self.kps_gt, "joints": self.joints_gt, "rs": self.rs_gt, "shapes": self.shapes_gt, "has_gt3d_smpl": self.has_smpl,
             "has_gt3d_joints": self.has_joints}
        return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in g.items()}

    def smpl(self, om):
        o = _loss_cases().G.forward(self.model, om[:, 3:75], om[:, 75:85], om[:, :3])
        return {"kps": o["kps"], "joints": o["joints"], "rs": o["Rs"], "beta": om[:, 75:85]}

    def kps_pred_f64(self):
        if self._kp64 is None:
            with torch.no_grad():
                self._kp64 = self.smpl(torch.from_numpy(self.omega.astype(np.float64)))["kps"].numpy()
        return self._kp64

    def total(self, P, strips, dtype):
        """the composed function: the present container's weighted total loss, a scalar tensor"""
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
        om = forward(P, strips, t(self.start), t(self.keep), self.scale, 3, 72, True)
        return _loss_cases().losses(self.smpl(om[0]), self.gt(dtype), self.B, self.T, self.flags, self.weights, 0)["total"]

    def result(self, dtype=torch.float64):
        """dict(total [1], d_strips, grads = [bank_layout per regressor]) of float64 numpy by autograd in `dtype`"""
        if dtype not in self._r:
            P = params(72, keys_of(self.ief), dtype)
            strips = torch.tensor(np.asarray(self.strips, np.float64), dtype=dtype).requires_grad_(True)
            tot = self.total(P, strips, dtype)
            tot.backward()
            n64 = lambda x: (torch.zeros_like(x) if x.grad is None else x.grad).to(torch.float64).numpy()
            self._r[dtype] = dict(total=np.array([float(tot.detach())]), d_strips=n64(strips),
                                  grads=[bank_layout({k: n64(v) for k, v in p.items()}, nd) for p, nd in zip(P, (85, 72, 72))])
        return self._r[dtype]

    def descent(self, dtype, steps=DESCENT_STEPS, lr=DESCENT_LR):
        """plain gradient descent on every tensor of the bank, fixed mask, fixed step -> [total before step 0, ..., after the last]"""
        P = params(72, keys_of(self.ief), dtype)
        strips = torch.tensor(np.asarray(self.strips, np.float64), dtype=dtype)
        out = []
        for _ in range(steps + 1):
            tot = self.total(P, strips, dtype)
            out.append(float(tot.detach()))
            leaves = [v for p in P for v in p.values()]
            grads = torch.autograd.grad(tot, leaves, allow_unused=True)
            with torch.no_grad():
                for v, g in zip(leaves, grads):
                    if g is not None:
                        v -= lr * g
        return out


@functools.lru_cache(maxsize=None)
def chain_case(B, T):
    return ChainCase(B, T, seed=40 + B)


def chain_quantities(res):
    q = {"total": [res["total"]], "d_strips": [res["d_strips"]]}
    for n in NAMES:
        q["present/" + n] = [res["grads"][0][n]]
    return q


def chain_errors(got, ref):
    qg, qr = chain_quantities(got), chain_quantities(ref)
    return {k: float(np.abs(np.asarray(qg[k][0], np.float64) - qr[k][0]).max()) for k in qr}


def chain_bounds(case):
    """FACTOR x E32 of the composed function.  `total` is ONE float32 number, and the |float32 - float64| of one number can be any
    fraction of its rounding step by chance (1.4e-8 at (8, 20), an eighth of a step): its E32 is floored at half a unit in the last
    place of a float32 of that size, the closest a float32 result can be promised to lie."""
    e = chain_errors(case.result(torch.float32), case.result())
    e["total"] = max(e["total"], float(TC.half_unit(case.result()["total"], "f32").max()))
    return {k: FACTOR * v for k, v in e.items()}


@functools.lru_cache(maxsize=None)
def descent_reference():
    """-> (the float64 run's totals [steps + 1], the bound per step): FACTOR x the deviation of the same steps run in float32 on the host,
    as the largest deviation up to that step (the deviation of a run accumulates; one step's own |float32 - float64| can be any fraction
    of the loss's rounding step by chance), floored like chain_bounds' total"""
    c = chain_case(*DESCENT_BT)
    d64, d32 = c.descent(torch.float64), c.descent(torch.float32)
    dev = np.maximum.accumulate(np.abs(np.array(d32) - np.array(d64)))
    dev = np.maximum(dev, TC.half_unit(np.array(d64), "f32"))
    return d64, [FACTOR * float(v) for v in dev]
