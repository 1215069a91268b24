"""Models, inputs, the float64 reference and the error bound of the SMPL stage sweep (tests/test_smpl_cases.py on the host,
tests/test_gpu_smpl.py on the device).  No GPU is needed by anything in here.

The body models follow the src/tf_smpl layout of assets.make_synthetic_smpl for ANY vertex count, with a pose-blend basis as heavy
as the shape basis (sigma 0.01, not 0.001): every one of the 218 basis rows moves a vertex by a visible amount, so a lost K step
is far outside any bound.  The bound itself comes from the reference, not from the kernels: E32 = |oracle in float32 - oracle in
float64| over a family of cases is the error of the same computation in the kernels' working precision."""
import numpy as np
import torch

from human_dynamics_amd import assets
from oracle import hmmr_oracle as O

OUTPUTS = ("verts", "joints", "kps", "Rs")
# |kernel - float64| <= FACTOR x E32: the 218-term sum in another order and with FMA, the joint regressor folded to fp32 on the
# host, device sinf / cosf, the wave reduction of the keypoint sum.  (May be raised with a measured ratio, never beyond 8.)
FACTOR = 4.0
# the split-fp16 blend (form 0) against the fp32 forms: the allowance the project documents (csrc/smpl.hip)
SPLIT_ALLOWANCE = 2e-6
# what the suite asserted before this sweep (test_smpl_stage_matches_oracle): no `standard` case may exceed it
LEGACY_BOUND = 2e-5


def _columns_sum1(rng, rows, counts):
    """[rows, len(counts)] non-negative matrix, counts[k] non-zeros in column k (0 allowed), every non-empty column sums to 1"""
    m = np.zeros((rows, len(counts)), np.float32)
    for k, c in enumerate(counts):
        if c == 0:
            continue
        idx = rng.choice(rows, size=c, replace=False)
        v = rng.uniform(0.05, 1.0, c)
        m[idx, k] = (v / v.sum()).astype(np.float32)
    return m


def kp_columns(nv, nk, empty_col=False, long_cols=False):
    """non-zeros per keypoint column: 48 like the synthetic model (all of them below 48 vertices); one empty column; one column
    beyond one trip of the keypoint kernel's 64-lane loop and one beyond two, where nv allows"""
    counts = [min(48, nv)] * nk
    if long_cols:
        assert nk >= 3 and nv > 64
        counts[0] = min(nv, 100)
        if nv > 128:
            counts[nk - 1] = min(nv, 150)
    if empty_col:
        counts[nk // 2] = 0
    return counts


def model(nv, nk=25, nnz=4, seed=0, short_rows=False, empty_col=False, long_cols=False):
    """A body model of nv vertices and nk keypoints in the tf_smpl layout.  short_rows: vertex v has nnz - v % nnz skinning
    weights (vertex 0 keeps the full width, so the packed ELL width is nnz whatever nv is); otherwise every vertex has nnz."""
    rng = np.random.Generator(np.random.PCG64([seed, nv, nk, nnz]))
    s = {}
    s["v_template"] = (rng.standard_normal((nv, 3)) * 0.3).astype(np.float32)
    s["shapedirs"] = (rng.standard_normal((10, nv * 3)) * 0.01).astype(np.float32)
    s["posedirs"] = (rng.standard_normal((207, nv * 3)) * 0.01).astype(np.float32)
    s["J_regressor"] = _columns_sum1(rng, nv, [min(32, nv)] * 24)
    s["cocoplus_regressor"] = _columns_sum1(rng, nv, kp_columns(nv, nk, empty_col, long_cols))
    w = np.zeros((nv, 24), np.float32)
    for v in range(nv):
        c = nnz - (v % nnz if short_rows else 0)
        idx = rng.choice(24, size=c, replace=False)
        x = rng.uniform(0.05, 1.0, c)
        w[v, idx] = (x / x.sum()).astype(np.float32)
    s["lbs_weights"] = w
    s["parents"] = assets.SMPL_PARENTS.copy()
    return s


def inputs(m, seed, family="standard"):
    """theta [m,72], beta [m,10], cams [m,3] (float32), every row different"""
    rng = np.random.Generator(np.random.PCG64([seed, m, {"standard": 0, "wide": 1}[family]]))
    if family == "standard":
        theta = (rng.standard_normal((m, 72)) * 0.6).astype(np.float32)
        theta[0, 3:6] = 0.0                              # the 1e-8 epsilon of batch_rodrigues alone
        if m > 1:
            theta[1, 6:9] = (np.pi, 0.0, 0.0)            # a half turn: sin ~ 0, 1 - cos = 2
        if m > 2:
            theta[2, 9:12] = 1e-7                        # an angle next to the epsilon
        beta = rng.standard_normal((m, 10)).astype(np.float32)
        s = rng.uniform(0.5, 1.5, (m, 1))
    else:
        theta = (rng.standard_normal((m, 72)) * 3.0).astype(np.float32)      # angles beyond 2 pi
        beta = (rng.standard_normal((m, 10)) * 5.0).astype(np.float32)
        s = rng.uniform(0.5, 1.5, (m, 1)) * np.where(np.arange(m) % 3 == 1, -1.0, 1.0)[:, None]
    cams = np.concatenate([s, rng.standard_normal((m, 2)) * 0.2], 1).astype(np.float32)
    return theta, beta, cams


def chunk_rows(nv):
    """instances per reference chunk: the float64 [N, nv, 4, 4] intermediate stays at or below 128 MB"""
    return max(1, (1 << 20) // nv)


def reference(mdl, theta, beta, cams, dtype=torch.float64, chunk=None, joint_type="cocoplus"):
    """oracle.smpl_forward + batch_orth_proj_idrot in chunks of instances -> {verts, joints, kps (None without cams), Rs} as
    float64 numpy arrays (the values of a float32 run, widened)"""
    if joint_type == "lsp":
        mdl = dict(mdl, cocoplus_regressor=np.ascontiguousarray(mdl["cocoplus_regressor"][:, :14]))       # batch_smpl.py:81-82
    m = theta.shape[0]
    step = chunk or chunk_rows(mdl["v_template"].shape[0])
    parts = {k: [] for k in OUTPUTS}
    for a in range(0, m, step):
        b = min(m, a + step)
        v, j, r = O.smpl_forward(beta[a:b], theta[a:b], mdl, dtype)
        parts["verts"].append(v)
        parts["joints"].append(j)
        parts["Rs"].append(r)
        if cams is not None:
            parts["kps"].append(O.batch_orth_proj_idrot(j, torch.as_tensor(np.asarray(cams[a:b])).to(dtype)))
    return {k: (torch.cat(p).to(torch.float64).numpy() if p else None) for k, p in parts.items()}


class Case(object):
    """one model + one set of inputs; the two references are computed once, on first use, and never written to"""

    def __init__(self, mdl, theta, beta, cams, family="standard", joint_type="cocoplus", name=""):
        self.model, self.theta, self.beta, self.cams = mdl, theta, beta, cams
        self.family, self.joint_type, self.name = family, joint_type, name
        self._ref = {}

    @property
    def m(self):
        return self.theta.shape[0]

    def ref(self, dtype=torch.float64):
        if dtype not in self._ref:
            r = reference(self.model, self.theta, self.beta, self.cams, dtype, joint_type=self.joint_type)
            for a in r.values():
                if a is not None:
                    a.setflags(write=False)
            self._ref[dtype] = r
        return self._ref[dtype]


def e32(family_cases):
    """E32(X, F): the largest |oracle_float32 - oracle_float64| of output X over the family's cases"""
    out = {k: 0.0 for k in OUTPUTS}
    for c in family_cases:
        r32, r64 = c.ref(torch.float32), c.ref(torch.float64)
        for k in OUTPUTS:
            if r64[k] is not None:
                out[k] = max(out[k], float(np.abs(r32[k] - r64[k]).max()))
    return out


def bounds(family_cases, factor=FACTOR):
    """{form: {output: bound}} for a family of cases.  Forms 1 and 2 (fp32 blends): factor x E32.  Form 0 (split-fp16 blend): + 2e-6 on
    verts and joints, + 2e-6 x max |s| on kps (the camera scale multiplies the joints).  Rs do not depend on the form."""
    assert 1.0 <= factor <= 8.0
    e = e32(family_cases)
    smax = max([float(np.abs(c.cams[:, 0]).max()) for c in family_cases if c.cams is not None] or [1.0])
    base = {k: factor * e[k] for k in OUTPUTS}
    split = dict(base)
    split["verts"] += SPLIT_ALLOWANCE
    split["joints"] += SPLIT_ALLOWANCE
    split["kps"] += SPLIT_ALLOWANCE * smax
    return {0: split, 1: base, 2: dict(base)}


def split_vpw(nv, m):
    """vertex tiles per workgroup of the split-fp16 form, from its launch rule (csrc/smpl.hip, smpl_launch): as many as it takes for
    (vpad / 128) x ceil(m / 32) workgroups to be at most 512 -> (vpw, tiles)"""
    vpad = (nv + 255) // 256 * 256
    vt = vpad // 128
    vpw = (vt * ((m + 31) // 32) + 511) // 512
    return max(1, min(vt, vpw)), vt
