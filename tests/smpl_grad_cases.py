"""Cases, the float64 reference gradient and the error bound of the SMPL backward (tests/test_smpl_grad_cases.py on the host,
tests/test_gpu_smpl_grad.py on the device).  No GPU is needed by anything in here.

oracle.hmmr_oracle.smpl_forward detaches its inputs (they pass through NumPy), so `forward` restates its ten lines with tensors in,
from the same torch pieces (batch_rodrigues, batch_global_rigid_transformation, batch_orth_proj_idrot).  The loss is
L = sum_X <X, G_X> over X in {verts, joints, kps, Rs} with fixed, seeded, standard-normal cotangents G_X; torch.autograd gives
d_theta, d_beta and d_cams in float64 (the reference) and in float32 (the yardstick's noise).  The bound is smpl_cases' scheme:
E32 = max |g32 - g64| over a family of cases, and a kernel may be FACTOR times that away from g64."""
import functools

import numpy as np
import torch

import smpl_cases as S
from oracle import hmmr_oracle as O

OUTPUTS = S.OUTPUTS
GRADS = ("d_theta", "d_beta", "d_cams")
# which gradient a cotangent reaches: the camera only through kps, the shape through everything but Rs, the pose through all four
REACH = {"d_theta": ("verts", "joints", "kps", "Rs"), "d_beta": ("verts", "joints", "kps"), "d_cams": ("kps",)}
FACTOR = S.FACTOR              # may be raised to a ratio measured on the MI355X, never beyond 8 (smpl_cases.py)
DOMINANCE = 1000.0             # a single cotangent's gradient is at least this many bounds large: a dropped term cannot hide
FAMILIES = ("standard", "wide")


def forward(mdl, theta, beta, cams=None, joint_type="cocoplus"):
    """oracle.smpl_forward (+ batch_orth_proj_idrot) with tensors in: theta [N,72], beta [N,10], cams [N,3] or None, all of one
    dtype -> {verts, joints, kps (None without cams), Rs}"""
    dtype = theta.dtype
    t = lambda k: torch.as_tensor(np.asarray(mdl[k])).to(dtype)
    N = beta.shape[0]
    v_template, shapedirs, posedirs = t("v_template"), t("shapedirs"), t("posedirs")
    J_regressor, weights, kreg = t("J_regressor"), t("lbs_weights"), t("cocoplus_regressor")
    if joint_type == "lsp":
        kreg = kreg[:, :14].contiguous()                                                # batch_smpl.py:81-82
    parents = [int(p) for p in np.asarray(mdl["parents"])]
    nv = v_template.shape[0]
    v_shaped = (beta @ shapedirs).reshape(N, nv, 3) + v_template
    J = torch.stack([v_shaped[:, :, c] @ J_regressor for c in range(3)], dim=2)
    Rs = O.batch_rodrigues(theta.reshape(-1, 3)).reshape(N, 24, 3, 3)
    pose_feature = (Rs[:, 1:] - torch.eye(3, dtype=dtype)).reshape(N, 207)
    v_posed = (pose_feature @ posedirs).reshape(N, nv, 3) + v_shaped
    _, A = O.batch_global_rigid_transformation(Rs, J, parents)
    T = (weights @ A.reshape(N, 24, 16)).reshape(N, nv, 4, 4)
    v_homo = torch.cat([v_posed, torch.ones(N, nv, 1, dtype=dtype)], dim=2)
    verts = (T @ v_homo.unsqueeze(-1))[:, :, :3, 0]
    joints = torch.stack([verts[:, :, c] @ kreg for c in range(3)], dim=2)
    kps = O.batch_orth_proj_idrot(joints, cams) if cams is not None else None
    return {"verts": verts, "joints": joints, "kps": kps, "Rs": Rs}


def cotangents(m, nv, nk, seed):
    """{output: float32 standard-normal array of the output's shape}"""
    rng = np.random.Generator(np.random.PCG64([seed, m, nv, nk, 77]))
    shapes = {"verts": (m, nv, 3), "joints": (m, nk, 3), "kps": (m, nk, 2), "Rs": (m, 24, 3, 3)}
    return {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in OUTPUTS}


def gradients(mdl, theta, beta, cams, cot, dtype=torch.float64, joint_type="cocoplus"):
    """d L / d (theta, beta, cams) for L = sum_X <X, cot[X]> over the outputs present in `cot` -> float64 numpy arrays (the values
    of a float32 run, widened); an input no given cotangent reaches gets zeros"""
    x = [torch.as_tensor(np.asarray(a)).to(dtype).requires_grad_(True) for a in (theta, beta, cams)]
    out = forward(mdl, x[0], x[1], x[2], joint_type)
    loss = sum((out[k] * torch.as_tensor(cot[k]).to(dtype)).sum() for k in OUTPUTS if cot.get(k) is not None)
    g = torch.autograd.grad(loss, x, allow_unused=True)
    return {n: (torch.zeros_like(xi) if gi is None else gi).to(torch.float64).numpy() for n, xi, gi in zip(GRADS, x, g)}


class GradCase(object):
    """one model + one set of inputs + its cotangents; every reference is computed once, on first use, and never written to"""

    def __init__(self, nv, m, family="standard", joint_type="cocoplus", seed=0, **model_kw):
        self.nv, self.m, self.family, self.joint_type = nv, m, family, joint_type
        self.model_kw = dict(model_kw)
        self.model = _model(nv, **model_kw)
        self.nk = 14 if joint_type == "lsp" else self.model["cocoplus_regressor"].shape[1]
        self.theta, self.beta, self.cams = S.inputs(m, 9000 + seed, family)
        self.cot = cotangents(m, nv, self.nk, 9100 + seed)
        self.name = "nv%d m%d %s%s%s" % (nv, m, family, " lsp" if joint_type == "lsp" else "",
                                         "".join(" %s=%s" % kv for kv in sorted(model_kw.items())))
        self._g = {}

    def grads(self, dtype=torch.float64, only=None):
        """all four cotangents together (only=None), or one of them alone"""
        key = (dtype, only)
        if key not in self._g:
            cot = self.cot if only is None else {only: self.cot[only]}
            g = gradients(self.model, self.theta, self.beta, self.cams, cot, dtype, self.joint_type)
            for a in g.values():
                a.setflags(write=False)
            self._g[key] = g
        return self._g[key]


@functools.lru_cache(maxsize=None)
def _model_cached(nv, nk, nnz, short, empty, long):
    return S.model(nv, nk=nk, nnz=nnz, seed=nv + 100 * nk + 10000 * nnz + 7, short_rows=short, empty_col=empty, long_cols=long)


def _model(nv, nk=25, nnz=4, short=True, empty=False, long=False):
    return _model_cached(nv, nk, nnz, short, empty, long)


NV_LIST = (50, 130, 700)             # below one 128-vertex tile, one tile + two vertices, several tiles (a partial sum of six terms)
M_LIST = (1, 5, 17, 33)              # one instance, below / across / several blocks of 8 with a ragged last one


@functools.lru_cache(maxsize=None)
def sweep(family):
    """the device sweep of one input family, as {group: (cases)}: a group shares a vertex count, hence the size of its sums, and
    makes one bound"""
    groups = {}
    for nv in NV_LIST:
        groups["nv%d" % nv] = [GradCase(nv, m, family, seed=nv + m) for m in M_LIST]
    groups["nv130"] += [GradCase(130, 5, family, seed=1, nnz=1, short=False),
                        GradCase(130, 5, family, seed=24, nnz=24),
                        GradCase(130, 5, family, "lsp", seed=14)]
    groups["nv300"] = [GradCase(300, 9, family, seed=300, empty=True, long=True)]
    return {k: tuple(v) for k, v in groups.items()}


@functools.lru_cache(maxsize=None)
def full_size_case():
    return GradCase(6890, 3, "standard", seed=6890)


def e32(cases):
    """E32(X): the largest |autograd in float32 - autograd in float64| of gradient X over the cases"""
    out = {k: 0.0 for k in GRADS}
    for c in cases:
        g32, g64 = c.grads(torch.float32), c.grads(torch.float64)
        for k in GRADS:
            out[k] = max(out[k], float(np.abs(g32[k] - g64[k]).max()))
    return out


def bounds(cases, factor=FACTOR):
    assert 1.0 <= factor <= 8.0
    return {k: factor * v for k, v in e32(cases).items()}


# ---- the descent of tests/test_gpu_smpl_grad.py: sum ||kps - target||^2 over (theta, beta, cams), plain gradient descent.  Step
# size and count are chosen on the host (test_smpl_grad_cases.py asserts that the float64 run falls at every step and ends below
# half its start).
DESCENT_NV, DESCENT_M, DESCENT_STEPS, DESCENT_LR = 700, 5, 12, 0.02


def descent_problem():
    """(model, start (theta, beta, cams), target kps): the target is the projection of one set of inputs, the start a perturbation"""
    mdl = _model(DESCENT_NV)
    th, be, ca = S.inputs(DESCENT_M, 4242)
    with torch.no_grad():
        target = forward(mdl, *[torch.from_numpy(a).to(torch.float64) for a in (th, be, ca)])["kps"].numpy()
    rng = np.random.Generator(np.random.PCG64(4243))
    start = (th + 0.1 * rng.standard_normal(th.shape).astype(np.float32), be + 0.3 * rng.standard_normal(be.shape).astype(np.float32),
             ca + 0.05 * rng.standard_normal(ca.shape).astype(np.float32))
    return mdl, start, target.astype(np.float32)


def descent_reference():
    """the float64 run -> [loss before step 0, ..., loss after the last step]"""
    mdl, start, target = descent_problem()
    x = [torch.from_numpy(a).to(torch.float64) for a in start]
    tgt = torch.from_numpy(target).to(torch.float64)
    losses = []
    for _ in range(DESCENT_STEPS + 1):
        xs = [a.clone().requires_grad_(True) for a in x]
        loss = ((forward(mdl, *xs)["kps"] - tgt) ** 2).sum()
        losses.append(float(loss.detach()))
        g = torch.autograd.grad(loss, xs)
        x = [a - DESCENT_LR * gi for a, gi in zip(x, g)]
    return losses
