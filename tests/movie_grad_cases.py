"""Cases, the torch oracle and the error bounds of the f_movie / hallucinator backward (tests/test_movie_grad_cases.py on the host,
tests/test_gpu_movie_grad.py on the device): hmmr_temporal_bwd / hmmr_hallucinator_bwd of csrc/movie_grad.hip.  No GPU is needed by
anything in here.

The oracle restates az_fc2_groupnorm and fc2_res in torch with the weights as LEAF tensors (oracle.hmmr_oracle converts them through
NumPy, where autograd cannot follow), out of the oracle's own group_norm_time and temporal_conv3; its forward is pinned to
oracle.hmmr_oracle.az_fc2_groupnorm / fc2_res in float64 to 1e-12 (test_movie_grad_cases.py).  Weights and inputs are tests/tail_cases.py's.

The bound is the project's rule: E32 = |autograd in float32 - autograd in float64| over the cases of one group (the temporal cases of one
block count; the hallucinator's cases), per output quantity (strips, d_phi, every gradient of every block); a kernel may be FACTOR times
that away from the float64 result.

ReLU kinks.  A pre-activation within rounding distance of zero takes one sign in float32 and the other in float64, and in a backward that
flips a whole term: a property of the function, not an error of a kernel.  These modules have no dropout mask to clear such units
through (tests/ief_grad_cases.py), so every case prepares its own weights: the layers in forward order, in float64; tau = TAU_FACTOR x
the float32-against-float64 error of that layer's pre-activations; every channel that holds a unit with |a| <= tau gets its GroupNorm
beta (the hallucinator: its fc bias) nudged by the smallest amount that puts all of the channel's units at least 4 tau from zero; at most
MAX_ROUNDS rounds per layer, at most MAX_NUDGED channels of a layer's 2048 (a condition of the case, asserted on the host).  The prepared
weights are what the oracle and the device both get (written into the bank's views)."""
import collections
import functools

import numpy as np
import torch

import tail_cases as TC
from human_dynamics_amd import assets
from oracle import hmmr_oracle as O

FACTOR = 4.0              # tests/tail_cases.py's rule: 4, or the smallest power of two that leaves 1.5 x over the largest measured, understood ratio (16 at most)
TAU_FACTOR = 16.0
CLEAR = 4.0               # a nudged channel's units lie at least CLEAR x tau from zero
MAX_NUDGED = 40           # channels of a layer's 2048 (2 %)
MAX_ROUNDS = 4
C = 2048
BLOCK_NAMES = ("gn1_gamma", "gn1_beta", "conv1", "b1", "gn2_gamma", "gn2_beta", "conv2", "b2")      # the order of hmmr_temporal_block_grads_t
HAL_NAMES = ("fc1", "fc2", "fc3", "b1", "b2", "b3")                                                # ... of hmmr_hallucinator_bwd_desc_t

TCase = collections.namedtuple("TCase", "name b t blocks seed")
HCase = collections.namedtuple("HCase", "name m seed rows")         # rows: "own", or the name of the temporal case whose rows it reads

# (b, t, blocks): (1, 1) both neighbours outside the window; (5, 7) 35 rows, window seams inside a 32-row tile; (1, 33) a window longer
# than a tile; (4, 17) 68 rows, the weight gradient's four contraction slices hold 32, 32, 4 and 0 rows
TEMPORAL_CASES = tuple(TCase("b%d_t%d_n%d" % (b, t, n), b, t, n, 1) for b, t, n in
                       ((1, 1, 1), (1, 2, 1), (1, 3, 1), (2, 7, 1), (2, 7, 3), (5, 7, 1), (1, 33, 1), (4, 17, 2), (3, 20, 3)))
HAL_CASES = tuple(HCase("m%d" % m, m, 1, "own") for m in (1, 14, 33, 68))
T_BY_NAME = {c.name: c for c in TEMPORAL_CASES}
H_BY_NAME = {c.name: c for c in HAL_CASES}
MAX_ROWS = 70


def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def rows_of(case):
    return case.b * case.t if isinstance(case, TCase) else case.m


def group_of(case):
    return ("temporal", case.blocks) if isinstance(case, TCase) else ("hal",)


def cases_of(group):
    return tuple(c for c in TEMPORAL_CASES + HAL_CASES if group_of(c) == group)


# ---------------------------------------------------------------------------------------------------------------- weights and inputs
def block_vars(i):
    """{name of BLOCK_NAMES: checkpoint name} of temporal block i"""
    gn1, c1, gn2, c2 = assets.temporal_scopes(i)
    return dict(gn1_gamma=gn1 + "/gamma", gn1_beta=gn1 + "/beta", conv1=c1 + "/weights", b1=c1 + "/biases",
                gn2_gamma=gn2 + "/gamma", gn2_beta=gn2 + "/beta", conv2=c2 + "/weights", b2=c2 + "/biases")


HAL_VARS = dict(fc1="fc2_res/fc1/weights", fc2="fc2_res/fc2/weights", fc3="fc2_res/fc3/weights",
                b1="fc2_res/fc1/biases", b2="fc2_res/fc2/biases", b3="fc2_res/fc3/biases")


@functools.lru_cache(maxsize=None)
def _base(name, dtype):
    """one checkpoint variable of tail_cases.weights() as a tensor of `dtype`, made once (the conv weights are 100 MB each in float64):
    leaves share its storage, nobody writes to it"""
    return torch.tensor(np.asarray(TC.weights()[name], np.float64), dtype=dtype)


def temporal_params(blocks, dtype, betas=None, requires_grad=True):
    """[{name: leaf tensor in the checkpoint's shape}] per block; betas: {checkpoint name: float32 array} of the prepared GN betas"""
    out = []
    for i in range(blocks):
        p = {}
        for n, v in block_vars(i).items():
            t = torch.tensor(np.asarray(betas[v], np.float64), dtype=dtype) if betas and v in betas else _base(v, dtype)
            p[n] = t.detach().requires_grad_(requires_grad)
        out.append(p)
    return out


def hal_params(dtype, biases=None, requires_grad=True):
    p = {}
    for n, v in HAL_VARS.items():
        t = torch.tensor(np.asarray(biases[v], np.float64), dtype=dtype) if biases and v in biases else _base(v, dtype)
        p[n] = t.detach().requires_grad_(requires_grad)
    return p


def phi_of(case):
    """the case's input: [b, t, 2048] (temporal) or [m, 2048] (hallucinator) float32"""
    if isinstance(case, TCase):
        return TC.phi_input(case.b, case.t, case.seed)
    if case.rows != "own":
        return np.ascontiguousarray(phi_of(T_BY_NAME[case.rows]).reshape(case.m, C))
    return np.ascontiguousarray(TC.phi_input(1, case.m, case.seed)[0])


def cotangent_of(case):
    shape = (case.b, case.t, C) if isinstance(case, TCase) else (case.m, C)
    return _rng(8, case.seed, *shape).standard_normal(shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the oracle
def temporal_forward(P, phi):
    """az_fc2_groupnorm (src/models.py:121-228) on leaf weights: P = temporal_params(), phi [b, t, 2048] of P's dtype"""
    net = phi
    for p in P:
        h = torch.relu(O.group_norm_time(net, p["gn1_gamma"], p["gn1_beta"]))
        h = O.temporal_conv3(h, p["conv1"], p["b1"])
        h = torch.relu(O.group_norm_time(h, p["gn2_gamma"], p["gn2_beta"]))
        h = O.temporal_conv3(h, p["conv2"], p["b2"])
        net = h + net
    return net


def hal_forward(p, phi):
    """fc2_res (src/models.py:270-296) on leaf weights: phi [m, 2048]"""
    h = torch.relu(phi @ p["fc1"] + p["b1"])
    h = torch.relu(h @ p["fc2"] + p["b2"])
    return h @ p["fc3"] + p["b3"] + phi


# ---------------------------------------------------------------------------------------------------------------- prepared weights
def _nudge(a, tau):
    """a [units of one channel] float64 -> the shift of smallest size after which every unit lies at least CLEAR x tau (and a little)
    from zero: the point nearest to 0 outside the union of the intervals (-a_r - w, -a_r + w)"""
    w = CLEAR * tau * 1.125
    lo, hi = np.sort(-a - w), np.sort(-a + w)           # (one width: sorted starts and ends pair up)
    best = None
    cur_lo, cur_hi = lo[0], hi[0]
    merged = []
    for l, h in zip(lo[1:], hi[1:]):
        if l <= cur_hi:
            cur_hi = max(cur_hi, h)
        else:
            merged.append((cur_lo, cur_hi))
            cur_lo, cur_hi = l, h
    merged.append((cur_lo, cur_hi))
    for l, h in merged:
        if l < 0.0 < h:
            best = l if -l <= h else h
    return 0.0 if best is None else float(best)


def _prepare_layer(pre, bias32, name, log):
    """pre(bias, dtype) -> the layer's pre-activations [rows, 2048] as a float64 array, computed in `dtype`.  Nudges bias32 (float32
    [2048], in place) until no unit of the float64 pre-activations lies within tau of zero."""
    a64 = pre(bias32, torch.float64)
    tau = TAU_FACTOR * float(np.abs(pre(bias32, torch.float32) - a64).max())
    nudged = set()
    rounds = 0
    while True:
        amb = np.nonzero((np.abs(a64) <= tau).any(axis=0))[0]
        if not len(amb):
            break
        rounds += 1
        if rounds > MAX_ROUNDS:
            break
        for c in amb:
            bias32[c] = np.float32(np.float64(bias32[c]) + _nudge(a64[:, c], tau))
            nudged.add(int(c))
        a64 = pre(bias32, torch.float64)
    log.append(dict(layer=name, tau=tau, nudged=len(nudged), rounds=rounds, left=int((np.abs(a64) <= tau).sum()),
                    closest=float(np.abs(a64[:, sorted(nudged)]).min()) if nudged else None))
    return a64


@functools.lru_cache(maxsize=None)
def prepared(case):
    """-> (weights: {checkpoint name: float32 array} of the nudged GN betas / fc biases, log: one dict per layer with tau, the channels
    nudged, the rounds taken, the ambiguous units left (0) and the distance from zero of the closest unit of a nudged channel)"""
    t = lambda a, dt: torch.tensor(np.asarray(a, np.float64), dtype=dt)
    n64 = lambda x: x.detach().to(torch.float64).numpy()
    src, out, log = TC.weights(), {}, []
    with torch.no_grad():
        if isinstance(case, HCase):
            x = {dt: t(phi_of(case), dt) for dt in (torch.float32, torch.float64)}
            for k in ("1", "2"):
                name = "fc2_res/fc%s/biases" % k
                bias = np.array(src[name], np.float32)
                W = "fc2_res/fc%s/weights" % k
                pre = lambda bv, dt, W=W: n64(x[dt] @ _base(W, dt) + t(bv, dt))
                _prepare_layer(pre, bias, name, log)
                out[name] = bias
                x = {dt: torch.relu(x[dt] @ _base(W, dt) + t(bias, dt)) for dt in x}
        else:
            x = {dt: t(phi_of(case), dt) for dt in (torch.float32, torch.float64)}
            for i in range(case.blocks):
                v = block_vars(i)
                cur = x
                for k in ("1", "2"):
                    name = v["gn%s_beta" % k]
                    beta = np.array(src[name], np.float32)
                    gamma = v["gn%s_gamma" % k]
                    pre = lambda bv, dt, cur=cur, gamma=gamma: n64(O.group_norm_time(cur[dt], _base(gamma, dt), t(bv, dt))).reshape(-1, C)
                    _prepare_layer(pre, beta, name, log)
                    out[name] = beta
                    conv, bias = v["conv%s" % k], v["b%s" % k]
                    cur = {dt: O.temporal_conv3(torch.relu(O.group_norm_time(cur[dt], _base(gamma, dt), t(beta, dt))), _base(conv, dt), _base(bias, dt))
                           for dt in cur}
                x = {dt: cur[dt] + x[dt] for dt in x}
    for a in out.values():
        a.setflags(write=False)
    return out, log


# ---------------------------------------------------------------------------------------------------------------- references
def conv_bank(g_hwio):
    """a conv weight (gradient) [3, 1, ci, co] -> the bank's rows [co][tap * 2048 + ci]"""
    return np.ascontiguousarray(np.asarray(g_hwio).reshape(3 * C, C).T)


def _n64(x):
    return (torch.zeros_like(x) if x.grad is None else x.grad).to(torch.float64).numpy()


def temporal_autograd(case, dtype, cot=None, betas=None):
    """{quantity: float64 array}: strips, d_phi and b<i>/<name> in the bank's layouts, by torch.autograd in `dtype` of
    sum(strips * cotangent) on the case's prepared weights"""
    betas = prepared(case)[0] if betas is None else betas
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype).requires_grad_(g)
    P = temporal_params(case.blocks, dtype, betas)
    phi = t(phi_of(case), True)
    strips = temporal_forward(P, phi)
    (strips * t(cotangent_of(case) if cot is None else cot)).sum().backward()
    q = {"strips": strips.detach().to(torch.float64).numpy(), "d_phi": _n64(phi)}
    for i, p in enumerate(P):
        for n in BLOCK_NAMES:
            q["b%d/%s" % (i, n)] = conv_bank(_n64(p[n])) if n.startswith("conv") else _n64(p[n])
    return q


def hal_autograd(case, dtype, cot=None, biases=None):
    """{quantity: float64 array}: out, d_phi and the six gradients in the bank's layouts ([out][in])"""
    biases = prepared(case)[0] if biases is None else biases
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype).requires_grad_(g)
    p = hal_params(dtype, biases)
    phi = t(phi_of(case), True)
    out = hal_forward(p, phi)
    (out * t(cotangent_of(case) if cot is None else cot)).sum().backward()
    q = {"out": out.detach().to(torch.float64).numpy(), "d_phi": _n64(phi)}
    for n in HAL_NAMES:
        q[n] = np.ascontiguousarray(_n64(p[n]).T) if n.startswith("fc") else _n64(p[n])
    return q


def autograd(case, dtype, cot=None):
    return (temporal_autograd if isinstance(case, TCase) else hal_autograd)(case, dtype, cot)


@functools.lru_cache(maxsize=1)
def reference(case):
    """the float64 autograd of the case.  One case is kept at a time: a three-block reference holds 600 MB of weight gradients."""
    return autograd(case, torch.float64)


def errors(got, ref):
    """{quantity: max |got - ref|} over the quantities of `ref`"""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(ref[k].shape) - ref[k]).max()) for k in ref}


@functools.lru_cache(maxsize=None)
def e32(group):
    """{quantity: the largest |autograd in float32 - autograd in float64| over the group's cases} -- only the numbers are kept"""
    out = {}
    for c in cases_of(group):
        r64 = autograd(c, torch.float64)
        for k, v in errors(autograd(c, torch.float32), r64).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def bounds(case):
    return {k: FACTOR * v for k, v in e32(group_of(case)).items()}


# ---------------------------------------------------------------------------------------------------------------- the workspaces
def _r256(x):
    return (x + 255) // 256 * 256


def temporal_bwd_workspace_bytes(b, t, blocks):
    """hmmr_temporal_bwd_workspace_bytes as csrc/movie_grad.hip states it (temporal_grad_layout; every buffer starts on a multiple of 256
    bytes): per block its input (not block 0's: that is phi), h1, c1, h2; the cotangent's two trunk buffers, d_h, d_c1; the per-window
    d_gamma and d_beta partial sums in double; the 4 split-K planes of the recomputed forward"""
    rows = _r256(b * t * C * 4)
    return (4 * blocks - 1) * rows + 4 * rows + 2 * _r256(b * C * 8) + _r256(4 * b * t * C * 4)


def hal_bwd_workspace_bytes(m):
    """hmmr_hallucinator_bwd_workspace_bytes (hal_grad_layout): h1, h2, d_a2, d_a1, the 4 split-K planes"""
    return 4 * _r256(m * C * 4) + _r256(4 * m * C * 4)


# ---------------------------------------------------------------------------------------------------------------- e_hallucinate
# mse(fc2_res(phi), az_fc2_groupnorm(phi)) (src/trainer_sequence_fc.py:839-846: no stop-gradient, the loss reaches both modules) on the
# (2, 7, 3) case, the hallucinator prepared on the same 14 rows.
HAL_CHAIN_T = T_BY_NAME["b2_t7_n3"]
HAL_CHAIN_H = HCase("chain_m14", 14, 1, "b2_t7_n3")


def hal_chain_phi():
    return phi_of(HAL_CHAIN_T)                         # [2, 7, 2048]; the hallucinator sees its 14 rows


def hal_chain_prepared():
    """(GN betas of the temporal case, fc biases of the hallucinator prepared on the same rows)"""
    return prepared(HAL_CHAIN_T)[0], prepared(HAL_CHAIN_H)[0]


def hal_chain_autograd(dtype):
    """{quantity: float64 array} of the composed function: loss [1], d_phi, t/b<i>/<name>, h/<name>"""
    betas, biases = hal_chain_prepared()
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=dtype).requires_grad_(g)
    P, H = temporal_params(3, dtype, betas), hal_params(dtype, biases)
    phi = t(hal_chain_phi(), True)
    loss = torch.mean((hal_forward(H, phi.reshape(14, C)).reshape(2, 7, C) - temporal_forward(P, phi)) ** 2)
    loss.backward()
    q = {"loss": np.array([float(loss.detach())]), "d_phi": _n64(phi)}
    for i, p in enumerate(P):
        for n in BLOCK_NAMES:
            q["t/b%d/%s" % (i, n)] = conv_bank(_n64(p[n])) if n.startswith("conv") else _n64(p[n])
    for n in HAL_NAMES:
        q["h/" + n] = np.ascontiguousarray(_n64(H[n]).T) if n.startswith("fc") else _n64(H[n])
    return q


@functools.lru_cache(maxsize=None)
def hal_chain_reference():
    """-> (the float64 result, {quantity: FACTOR x E32 of the composed function}); the loss is ONE float32 number, whose E32 is floored
    at half a unit in the last place (tests/ief_grad_cases.py, chain_bounds)"""
    r64 = hal_chain_autograd(torch.float64)
    e = errors(hal_chain_autograd(torch.float32), r64)
    e["loss"] = max(e["loss"], float(TC.half_unit(r64["loss"], "f32").max()))
    return r64, {k: FACTOR * v for k, v in e.items()}


# ---------------------------------------------------------------------------------------------------------------- the descent
# Plain gradient descent on every tensor of a one-block bank at (2, 7): loss = mean((az_fc2_groupnorm(phi) - target)^2), fixed step.
DESCENT_CASE, DESCENT_STEPS, DESCENT_LR = T_BY_NAME["b2_t7_n1"], 12, 0.1      # chosen on the host: test_movie_grad_cases.py asserts that the float64 run falls at every step


def descent_target():
    return TC.phi_input(2, 7, 9)


def descent(dtype, steps=DESCENT_STEPS, lr=DESCENT_LR):
    """-> [loss before step 0, ..., after the last] of the host run in `dtype`, from the case's prepared weights"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    P = temporal_params(1, dtype, prepared(DESCENT_CASE)[0])
    P = [{n: v.detach().clone().requires_grad_() for n, v in p.items()} for p in P]          # (the cached base tensors are never written)
    phi, target = t(phi_of(DESCENT_CASE)), t(descent_target())
    out = []
    for _ in range(steps + 1):
        loss = torch.mean((temporal_forward(P, phi) - target) ** 2)
        out.append(float(loss.detach()))
        leaves = [v for p in P for v in p.values()]
        grads = torch.autograd.grad(loss, leaves)
        with torch.no_grad():
            for v, g in zip(leaves, grads):
                v -= lr * g
    return out


@functools.lru_cache(maxsize=None)
def descent_reference():
    """-> (the float64 run's losses [steps + 1], the allowed deviation per step): FACTOR x the deviation of the same steps run in float32
    on the host, as the largest deviation up to that step, floored at half a unit in the last place of the loss (ief_grad_cases.py)"""
    d64, d32 = descent(torch.float64), descent(torch.float32)
    dev = np.maximum.accumulate(np.abs(np.array(d32) - np.array(d64)))
    dev = np.maximum(dev, TC.half_unit(np.array(d64), "f32"))
    return d64, [FACTOR * float(v) for v in dev]
