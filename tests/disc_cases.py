"""Cases, the torch oracle and the error bounds of the pose discriminator (tests/test_disc_cases.py on the host,
tests/test_gpu_disc_pose.py on the device): hmmr_disc_pose_fwd / hmmr_disc_pose_bwd / hmmr_pose_prior of csrc/disc_pose.hip.  No GPU
is needed by anything in here.

The oracle restates the function of include/hmmr_hip.h ("Pose discriminator") in torch with the weights as leaf tensors, differentiated
by autograd in float64; tests/test_disc_cases.py pins its forward and losses to the reference's own code (the fixture
tests/golden/reference_disc_pose.npz).  Weights are He-scaled normals with 0.1-sigma biases, rows are Rodrigues of 0.4-sigma
axis-angles, rounded to float32.

The bound is the project's rule: E32 = |autograd in float32 - autograd in float64| over all cases, per quantity (out, d_poses, each
of the twelve gradients, each loss); a kernel may be FACTOR = 4 times that away from the float64 result.

ReLU kinks.  A pre-activation within rounding distance of zero takes one sign in float32 and the other in float64, and its gradient
path then differs by a full-size term: a property of the function, not an error of a kernel.  A row with any pre-activation within
tau = 16 x the layer's float32-against-float64 error (over the first draw of every row of every case) is AMBIGUOUS.  The function is
row-wise, so an ambiguous row is REDRAWN -- a new seed for that row alone -- until none is left; a row's draws depend on its stream
and index only, so (7,0) stays rows 0..6 of (33,0).  Condition (test_disc_cases.py): at most max(2, n / 4) redraws per case, within
4 rounds."""
import collections
import functools

import numpy as np
import torch

from oracle import hmmr_oracle as O

FACTOR = 4.0
TAU_FACTOR = 16.0
MAX_ROUNDS = 4
GUARD = 0x7FC12345
NAMES = ("conv1", "bc1", "conv2", "bc2", "heads", "bj", "fc1", "b1", "fc2", "b2", "fc_out", "bo")      # hmmr_disc_pose_grads_t
LOSSES = ("e_pose", "d_real", "d_fake")
LAYERS = ("a1", "a2", "a3", "a4")

Case = collections.namedtuple("Case", "name n_a n_b stream first ld_a ld_b")


def _case(n_a, n_b, stream, first=0, ld_a=207, ld_b=216):
    return Case("%d_%d" % (n_a, n_b), n_a, n_b, stream, first, ld_a, ld_b)


# (7,0) is rows 0..6 of (33,0): the same stream.  Row strides: 207, 216 (the Rs + 9 form) and 221 once.
CASES = (_case(1, 0, 1), _case(0, 1, 2), _case(2, 2, 3), _case(7, 0, 4), _case(33, 0, 4, ld_a=216), _case(31, 33, 5, ld_a=216, ld_b=221),
         _case(64, 64, 6), _case(65, 0, 7), _case(160, 160, 8))
BY_NAME = {c.name: c for c in CASES}
FIXTURE_ROWS = (4, 4)        # the fixture's real + fake rows: stream 0


def max_redraws(n):
    return max(2, n // 4)


# ---------------------------------------------------------------------------------------------------------------- weights
def _rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


@functools.lru_cache(maxsize=None)
def weights():
    """{checkpoint name: float32 array} of the D_pose scope: He-scaled normals, 0.1-sigma biases"""
    rng = _rng(2024, 11)
    w = {}

    def layer(scope, shape, fan_in):
        w["D_pose/%s/weights" % scope] = (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        w["D_pose/%s/biases" % scope] = (0.1 * rng.standard_normal(shape[-1])).astype(np.float32)
    layer("D_conv1", (1, 1, 9, 32), 9)
    layer("D_conv2", (1, 1, 32, 32), 32)
    for j in range(23):
        layer("pose_out_j%d" % j, (32, 1), 32)
    layer("D_alljoints_fc1", (736, 1024), 736)
    layer("D_alljoints_fc2", (1024, 1024), 1024)
    layer("D_alljoints_out", (1024, 1), 1024)
    return w


def params(dtype, requires_grad=True, source=None):
    """the oracle's leaf tensors: C1 [9,32], bc1, C2 [32,32], bc2, wj [23,32], bj [23], F1 [736,1024], b1, F2, b2, fo [1024], bo [1]"""
    w = weights() if source is None else source
    g = lambda k: np.asarray(w["D_pose/" + k], np.float64)
    raw = dict(C1=g("D_conv1/weights").reshape(9, 32), bc1=g("D_conv1/biases"), C2=g("D_conv2/weights").reshape(32, 32), bc2=g("D_conv2/biases"),
               wj=np.stack([g("pose_out_j%d/weights" % j).reshape(32) for j in range(23)]),
               bj=np.stack([g("pose_out_j%d/biases" % j).reshape(()) for j in range(23)]),
               F1=g("D_alljoints_fc1/weights"), b1=g("D_alljoints_fc1/biases"), F2=g("D_alljoints_fc2/weights"), b2=g("D_alljoints_fc2/biases"),
               fo=g("D_alljoints_out/weights").reshape(1024), bo=g("D_alljoints_out/biases").reshape(1))
    return {k: torch.tensor(v, dtype=dtype).requires_grad_(requires_grad) for k, v in raw.items()}


def bank_layout(g):
    """the oracle's gradients {C1, ...} (arrays) -> {name: array} in the bank's layouts, padding zero"""
    z = lambda *s: np.zeros(s, np.float64)
    out = {n: None for n in NAMES}
    out["conv1"] = z(32, 16); out["conv1"][:, :9] = g["C1"].T
    out["bc1"], out["conv2"], out["bc2"] = g["bc1"].copy(), g["C2"].T.copy(), g["bc2"].copy()
    out["heads"] = z(32, 32); out["heads"][:23] = g["wj"]
    out["bj"] = z(32); out["bj"][:23] = g["bj"]
    out["fc1"] = z(1024, 1024); out["fc1"][:, :736] = g["F1"].T
    out["b1"], out["fc2"], out["b2"] = g["b1"].copy(), g["F2"].T.copy(), g["b2"].copy()
    out["fc_out"] = z(128, 1024); out["fc_out"][0] = g["fo"]
    out["bo"] = z(128); out["bo"][0] = g["bo"][0]
    return out


# ---------------------------------------------------------------------------------------------------------------- the oracle
def forward(P, x, pre=None):
    """The function of include/hmmr_hip.h, "Pose discriminator": x [n,23,9] of P's dtype -> out [n,24].  pre: a dict that receives the
    four pre-activations"""
    n = x.shape[0]
    a1 = x @ P["C1"] + P["bc1"]
    h1 = torch.relu(a1)
    a2 = h1 @ P["C2"] + P["bc2"]
    h2 = torch.relu(a2)
    heads = (h2 * P["wj"]).sum(dim=2) + P["bj"]
    a3 = h2.reshape(n, 736) @ P["F1"] + P["b1"]
    h3 = torch.relu(a3)
    a4 = h3 @ P["F2"] + P["b2"]
    h4 = torch.relu(a4)
    last = h4 @ P["fo"].reshape(1024, 1) + P["bo"]
    if pre is not None:
        pre.update(a1=a1.detach().reshape(n, -1), a2=a2.detach().reshape(n, -1), a3=a3.detach(), a4=a4.detach())
    return torch.cat([heads, last], dim=1)


def losses(out_real, out_fake):
    """(e_pose, d_real, d_fake) of src/ops.py:127-136; the loss of an empty segment is 0"""
    zero = out_real.sum() * 0 + out_fake.sum() * 0
    e = ((out_fake - 1) ** 2).sum(dim=1).mean() if out_fake.shape[0] else zero
    dr = ((out_real - 1) ** 2).sum(dim=1).mean() if out_real.shape[0] else zero
    df = (out_fake ** 2).sum(dim=1).mean() if out_fake.shape[0] else zero
    return e, dr, df


# ---------------------------------------------------------------------------------------------------------------- rows
def draw_row(stream, index, round_):
    """x [23,9] float32: Rodrigues of 0.4-sigma axis-angles"""
    aa = 0.4 * _rng(7, stream, index, round_).standard_normal((23, 3))
    return O.batch_rodrigues(torch.tensor(aa, dtype=torch.float64)).reshape(23, 9).numpy().astype(np.float32)


def _streams():
    """{stream: rows drawn from it}: the largest first + n_a + n_b of the cases that share it (and the fixture's stream 0)"""
    need = {0: sum(FIXTURE_ROWS)}
    for c in CASES:
        need[c.stream] = max(need.get(c.stream, 0), c.first + c.n_a + c.n_b)
    return need


def _pre(x64):
    """the four pre-activations of rows x [n,23,9] in float32 and float64"""
    out = []
    for dt in (torch.float32, torch.float64):
        pre = {}
        with torch.no_grad():
            forward(params(dt, False), torch.tensor(x64, dtype=dt), pre)
        out.append({k: v.to(torch.float64).numpy() for k, v in pre.items()})
    return out


@functools.lru_cache(maxsize=None)
def drawn():
    """every stream's rows after the redraws: {stream: (x [n,23,9] float32, redraw count per row [n], rounds used)}, and tau per layer"""
    need = _streams()
    keys = [(s, i) for s in sorted(need) for i in range(need[s])]
    rounds = {k: 0 for k in keys}
    x = {k: draw_row(k[0], k[1], 0) for k in keys}
    p32, p64 = _pre(np.stack([x[k] for k in keys]).astype(np.float64))
    tau = {l: TAU_FACTOR * float(np.abs(p32[l] - p64[l]).max()) for l in LAYERS}
    amb = lambda p: np.any([np.abs(p[l]).min(axis=1) <= tau[l] for l in LAYERS], axis=0)
    bad = [k for k, a in zip(keys, amb(p64)) if a]
    used = 0
    while bad and used < MAX_ROUNDS + 4:
        used += 1
        for k in bad:
            rounds[k] += 1
            x[k] = draw_row(k[0], k[1], rounds[k])
        p64 = _pre(np.stack([x[k] for k in bad]).astype(np.float64))[1]
        bad = [k for k, a in zip(bad, amb(p64)) if a]
    assert not bad, "rows stay ambiguous after %d rounds: %r" % (used, bad)
    out = {s: (np.stack([x[(s, i)] for i in range(need[s])]), np.array([rounds[(s, i)] for i in range(need[s])])) for s in need}
    return out, tau


def ambiguous(x):
    """per row of x [n,23,9]: whether any float64 pre-activation lies within tau of zero"""
    tau = drawn()[1]
    p64 = _pre(np.asarray(x, np.float64).reshape(-1, 23, 9))[1]
    return np.any([np.abs(p64[l]).min(axis=1) <= tau[l] for l in LAYERS], axis=0)


def redraws(case):
    """(redraws of the case's rows in all, the largest count of one row = the rounds it took)"""
    r = drawn()[0][case.stream][1][case.first:case.first + case.n_a + case.n_b]
    return int(r.sum()), int(r.max())


def rows(case):
    """(x_a [n_a,23,9], x_b [n_b,23,9]) float32"""
    x = drawn()[0][case.stream][0][case.first:case.first + case.n_a + case.n_b]
    return x[:case.n_a], x[case.n_a:]


def fixture_rows():
    x = drawn()[0][0][0]
    return x[:FIXTURE_ROWS[0]], x[FIXTURE_ROWS[0]:]


def cotangent(case):
    """d_out [n,24] float32, standard normal"""
    return _rng(9, case.stream, case.n_a, case.n_b).standard_normal((case.n_a + case.n_b, 24)).astype(np.float32)


def loss_segments(case):
    """the (real, fake) rows the case's three losses are taken on: its own segments, or for a case without rows_b nothing | rows_a
    (hmmr_pose_prior refuses an empty fake segment when the losses are wanted)"""
    a, b = rows(case)
    return (a, b) if case.n_b else (b, a)


# ---------------------------------------------------------------------------------------------------------------- references
def compute(case, dtype):
    """{out, d_poses, the twelve gradients (bank layouts), the three losses} of the oracle in `dtype`, as float64 arrays"""
    a, b = rows(case)
    P = params(dtype)
    x = torch.tensor(np.concatenate([a, b]).astype(np.float64), dtype=dtype).requires_grad_(True)
    out = forward(P, x)
    names = list(P)
    g = torch.autograd.grad((out * torch.tensor(cotangent(case).astype(np.float64), dtype=dtype)).sum(), [x] + [P[k] for k in names])
    n64 = lambda t: t.detach().to(torch.float64).numpy()
    res = dict(out=n64(out), d_poses=n64(g[0]).reshape(-1, 207))
    res.update(bank_layout({k: n64(v) for k, v in zip(names, g[1:])}))
    real, fake = loss_segments(case)
    with torch.no_grad():
        P0 = params(dtype, False)
        t = lambda r: torch.tensor(r.astype(np.float64), dtype=dtype).reshape(-1, 23, 9)
        ls = losses(forward(P0, t(real)), forward(P0, t(fake)))
    res.update({k: np.array(float(v)) for k, v in zip(LOSSES, ls)})
    return res


QUANTITIES = ("out", "d_poses") + NAMES + LOSSES


@functools.lru_cache(maxsize=None)
def reference(case):
    return compute(case, torch.float64)


@functools.lru_cache(maxsize=None)
def e32():
    """{quantity: max |float32 autograd - float64 autograd| over all cases}"""
    e = {q: 0.0 for q in QUANTITIES}
    for c in CASES:
        r32, r64 = compute(c, torch.float32), reference(c)
        for q in QUANTITIES:
            e[q] = max(e[q], float(np.abs(r32[q] - r64[q]).max()))
    return e


def bounds():
    return {q: FACTOR * v for q, v in e32().items()}


def strided(x, ld, lead=0, fill=None):
    """rows x [n,207] laid out at row stride ld behind `lead` floats: (the float32 buffer [n * ld + lead], the offset of row 0).  The
    gaps hold the guard pattern"""
    n = x.shape[0]
    buf = np.full(n * ld + lead, GUARD if fill is None else fill, np.uint32).view(np.float32)
    if n:
        v = buf[lead:].reshape(n, ld)
        v[:, :207] = x.reshape(n, 207)
    return buf
