"""Cases, the float64 reference and the error bound of the trainer's loss stage and of the closed loop omega -> losses, d_omega
(tests/test_loss_cases.py on the host, tests/test_gpu_losses.py on the device).  No GPU is needed by anything in here.

`losses` restates src/ops.py (compute_loss_e_kp, compute_loss_e_kp_optcam, compute_loss_e_3d / compute_loss_mse / align_by_pelvis,
compute_loss_e_smooth, compute_loss_shape), src/tf_smpl/projection.py (procrustes2d_vis, batch_orth_proj_optcam) and the frame
slices of compute_losses_deltas (src/trainer_sequence_fc.py:867-884) with tensors in, in any dtype; tests/test_loss_cases.py pins
it to tests/golden/reference_losses.npz, the reference's own functions executed.  The closed loop puts smpl_grad_cases.forward in
front of it.  Gradients come from torch.autograd in float64 (the reference) and in float32 (the yardstick's noise).

The bound is the project's scheme (smpl_cases.py), not a new number: E32 = max |g32 - g64| over the case's GROUP -- the cases of
one (B, T), which share their normalisers' size -- and a kernel may be FACTOR = 4 (never beyond 8) times that away from g64; the
same for the loss values.  A cotangent that is an exact product of inputs (vis sign / P) is compared the same way, with the E32 of
its own group.

Input conditions (asserted by the builders: conditions on the inputs, not measurements of the kernels):
  - every |pred - gt| on a keypoint with vis != 0 is >= 1e-4 in float64, so the signs of a float32 and a float64 evaluation agree;
    the exceptions are planted exact zeros, and those exist only where kps_pred is an INPUT (stage cases without the optimal camera);
  - the unclipped optimal scale lies at least 1e-3 away from 0.7 and from 10 in float64, in every frame of every case;
  - the optimal-camera cases hold unclipped, clipped-low (a mirrored prediction) and clipped-high frames."""
import functools

import numpy as np
import torch

import smpl_cases as S
import smpl_grad_cases as G

KP, KP_OPTCAM, JOINTS, SMPL, CONST, SHAPE_PRIOR = 1, 2, 4, 8, 16, 32
ALL = JOINTS | SMPL | CONST | SHAPE_PRIOR            # + KP or KP_OPTCAM
LOSS_NAMES = ("e_kp", "e_joints", "e_smpl_pose", "e_smpl_shape", "e_const", "e_shape", "total")
# which losses a flag produces, and which cotangent it reaches
FLAG_LOSSES = {KP: ("e_kp",), KP_OPTCAM: ("e_kp",), JOINTS: ("e_joints",), SMPL: ("e_smpl_pose", "e_smpl_shape"), CONST: ("e_const",),
               SHAPE_PRIOR: ("e_shape",)}
FLAG_REACH = {KP: ("d_kps",), KP_OPTCAM: ("d_kps",), JOINTS: ("d_joints",), SMPL: ("d_rs", "d_beta"), CONST: ("d_beta",),
              SHAPE_PRIOR: ("d_beta",)}
# ... and the part of d_omega a term alone is large in (the keypoint and joint terms reach beta too, but weakly: a dropped term shows in
# the pose, and for the plain keypoint loss in the camera)
LOOP_REACH = {KP: ("d_cams", "d_theta"), KP_OPTCAM: ("d_theta",), JOINTS: ("d_theta",), SMPL: ("d_theta", "d_beta"), CONST: ("d_beta",),
              SHAPE_PRIOR: ("d_beta",)}
STAGE_GRADS = ("d_kps", "d_joints", "d_rs", "d_beta")
OMEGA_PARTS = {"d_cams": slice(0, 3), "d_theta": slice(3, 75), "d_beta": slice(75, 85)}
FACTOR = S.FACTOR
DOMINANCE = G.DOMINANCE
# e_kp, e_joints, e_smpl, e_const, e_shape: all different, so a swapped weight shows; the 3-D terms, whose normalisers are the larger
# ones, carry the larger weights, so that every term alone stays DOMINANCE bounds large in the closed loop (test_loss_cases.py)
WEIGHTS = (1.0, 20.0, 5.0, 3.0, 0.25)
MIN_RESIDUAL, SCALE_MARGIN = 1e-4, 1e-3
BT_LIST = ((1, 1), (1, 2), (3, 3), (1, 9), (7, 9), (8, 8), (5, 13), (8, 20))     # N around 1, a wave and 64; the trainer's default


def deltas_for(T):
    """0, +-1, +-5 where they fit, and the delta that leaves ONE frame (T = |delta_t| + 1)"""
    d = [0] + [s * a for a in (1, 5) for s in (1, -1) if a < T]
    if T > 1 and (T - 1) not in (1, 5):
        d += [T - 1, -(T - 1)]
    return tuple(d)


def slice_rows(B, T, delta_t):
    """(pred rows, gt rows) of the slice, sequence-major (compute_losses_deltas :867-884)"""
    a = abs(delta_t)
    assert a < T
    t = np.arange(T - a)
    ps, gs = (a if delta_t < 0 else 0), (a if delta_t > 0 else 0)
    base = (np.arange(B) * T)[:, None]
    return (base + t + ps).ravel(), (base + t + gs).ravel()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def optimal_camera(x, xg):
    """procrustes2d_vis: x [n,K,2], xg [n,K,3] -> (best_cam [n,3], the scale before the clip); the 2x2 inverse in closed form"""
    vis = (xg[:, :, 2] > 0).to(x.dtype).unsqueeze(2)
    nv = vis.sum(1, keepdim=True)
    mu1, mu2 = (vis * x).sum(1, keepdim=True) / nv, (vis * xg[:, :, :2]).sum(1, keepdim=True) / nv
    xmu, y = vis * (x - mu1), vis * (xg[:, :, :2] - mu2)
    A = xmu.transpose(1, 2) @ xmu + 1e-6 * torch.eye(2, dtype=x.dtype)
    Bm = xmu.transpose(1, 2) @ y
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    Ainv = torch.stack([torch.stack([A[:, 1, 1], -A[:, 0, 1]], 1), torch.stack([-A[:, 1, 0], A[:, 0, 0]], 1)], 1) / det[:, None, None]
    raw = torch.diagonal(Ainv @ Bm, dim1=1, dim2=2).sum(1) / 2.
    scale = torch.clamp(raw, 0.7, 10.)
    trans = mu2[:, 0] / scale[:, None] - mu1[:, 0]
    return torch.cat([scale[:, None], trans], 1), raw


def align_by_pelvis(j):
    return j - ((j[:, 3] + j[:, 2]) / 2.).unsqueeze(1)


def _mse(a, b, w):
    """0.5 x tf.losses.mean_squared_error(weights = w [rows, 1]): SUM_BY_NONZERO_WEIGHTS with the safe division"""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    present = int((w != 0).sum()) * a.shape[1]
    s = (w[:, None] * (a - b) ** 2).sum()
    return 0.5 * s / present if present > 0 else s * 0.


def losses(pred, gt, B, T, flags, weights=WEIGHTS, delta_t=0):
    """pred {kps [N,K,2], joints [N,K,3], rs [N,24,3,3], beta [N,10]}, gt {kps [N,K,3], joints [N,14,3], rs, shapes [B,10],
    has_gt3d_smpl [B], has_gt3d_joints [B]} (tensors of one dtype; what no flag needs may be missing) -> {LOSS_NAMES: scalars,
    best_cam [rows of the slice, 3] or None, scale_raw}"""
    ref = next(v for v in pred.values() if v is not None)
    zero = ref.sum() * 0.
    out = {k: zero for k in LOSS_NAMES}
    out["best_cam"] = out["scale_raw"] = None
    pi, gi = slice_rows(B, T, delta_t)
    L = T - abs(delta_t)
    if flags & (KP | KP_OPTCAM):
        x, xg = pred["kps"][pi], gt["kps"][gi]
        if flags & KP_OPTCAM:
            cam, out["scale_raw"] = optimal_camera(x.detach(), xg)
            out["best_cam"] = cam = cam.detach()                                  # tf.stop_gradient
            x = cam[:, None, 0:1] * (x + cam[:, None, 1:3])                       # batch_orth_proj_idrot
        vis = xg[:, :, 2:3]
        s = (vis * (xg[:, :, :2] - x).abs()).sum()
        present = 2 * int((vis != 0).sum())
        out["e_kp"] = s / present if present > 0 else s * 0.
    if flags & JOINTS:
        w = gt["has_gt3d_joints"].repeat_interleave(L)
        out["e_joints"] = _mse(align_by_pelvis(gt["joints"][gi]), align_by_pelvis(pred["joints"][pi][:, :14]), w)
    if flags & SMPL:
        w = gt["has_gt3d_smpl"].repeat_interleave(L)
        out["e_smpl_pose"] = _mse(gt["rs"][gi], pred["rs"][pi], w)
        out["e_smpl_shape"] = _mse(gt["shapes"].repeat_interleave(T, 0)[gi], pred["beta"][pi], w)
    if flags & CONST and T > 1:
        b = pred["beta"].reshape(B, T, 10)
        out["e_const"] = 0.5 * ((b[:, :-1] - b[:, 1:]) ** 2).mean()
    if flags & SHAPE_PRIOR:
        out["e_shape"] = (pred["beta"] ** 2).mean()
    w = weights
    out["total"] = (w[0] * out["e_kp"] + w[1] * out["e_joints"] + w[2] * (out["e_smpl_pose"] + out["e_smpl_shape"]) + w[3] * out["e_const"]
                    + w[4] * out["e_shape"])
    return out


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _result(out, grads, N, pi):
    r = {"losses": np.array([float(out[k].detach().to(torch.float64)) for k in LOSS_NAMES]), "best_cam": None, "scale_raw": None}
    if out["best_cam"] is not None:
        cam = np.full((N, 3), np.nan)
        cam[pi] = out["best_cam"].to(torch.float64).numpy()
        r["best_cam"], r["scale_raw"] = cam, out["scale_raw"].to(torch.float64).numpy()
    r.update(grads)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


# ---------------------------------------------------------------------------------------------------------------- the fixture's inputs
GOLDEN_B, GOLDEN_T, GOLDEN_K = 2, 4, 14
GOLDEN_DELTAS = (0, 1, -1, 3, -3)


def golden_inputs():
    """the fp32 inputs of tests/golden/reference_losses.npz, from a seed: the generator (tests/golden/make_losses_golden.py) and the test
    that reads the fixture both call this, so the fixture stores results only.  The optimal scale of the frames is spread over the
    unclipped range, below 0.7 (a mirrored prediction) and above 10 (a prediction a twentieth of the size)"""
    B, T, K = GOLDEN_B, GOLDEN_T, GOLDEN_K
    rng = np.random.Generator(np.random.PCG64(20261))
    N = B * T
    kps_gt = np.concatenate([rng.uniform(-1, 1, (N, K, 2)), (rng.random((N, K, 1)) < 0.7).astype(np.float64)], 2)
    kps_gt[0, :3, 2] = (0.5, 2.0, -1.0)                  # vis values other than 0 / 1: a weight as given; z <= 0 is invisible to the camera
    kps_gt[3, 1:, 2] = 0.0                               # one visible keypoint: a singular 2x2 problem that only the 1e-6 I holds up
    kps_gt[3, 0, 2] = 1.0
    scale = np.array([0.9, 1.3, -1.0, 1.0, 0.05, 0.8, 1.0, 0.04])[:, None, None]
    kps_pred = (kps_gt[:, :, :2] + rng.normal(0, 0.05, (N, K, 2))) * scale + rng.normal(0, 0.2, (N, 1, 2))
    out = dict(
        kps_gt=kps_gt, kps_pred=kps_pred,
        joints_gt=rng.normal(0, 0.3, (N, 14, 3)), joints_pred=rng.normal(0, 0.3, (N, K, 3)),
        poses_gt=rng.normal(0, 0.4, (N, 72)), poses_pred=rng.normal(0, 0.4, (N, 72)),
        shapes_gt=rng.normal(0, 1, (B, 10)), beta_pred=rng.normal(0, 1, (N, 10)),
        has_gt3d_smpl=np.array([1.0, 0.0]), has_gt3d_joints=np.array([0.5, 1.0]),
    )
    return {k: v.astype(np.float32) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------- stage cases
class StageCase(object):
    """the loss stage alone: predictions and ground truth are seeded fp32 inputs.  vis: 'binary', 'weights' (values 0, 0.5, 2, and -1:
    a weight that the optimal camera does not see), 'some_frames_invisible', 'none'; has: 'ones', 'zeros', 'mixed', 'weights';
    plant: exact-zero residuals on visible keypoints (without the optimal camera only)"""

    def __init__(self, B, T, K, delta_t, flags, vis="binary", has="mixed", plant=False, seed=0, weights=WEIGHTS):
        self.B, self.T, self.K, self.delta_t, self.flags, self.weights = B, T, K, delta_t, flags, tuple(weights)
        self.vis, self.has, self.plant = vis, has, plant
        self.name = "B%d T%d K%d dt%+d flags%02x %s %s%s" % (B, T, K, delta_t, flags, vis, has, " planted" if plant else "")
        N = B * T
        rng = np.random.Generator(np.random.PCG64([seed, B, T, K, delta_t + 100, flags]))
        xy = rng.uniform(-1, 1, (N, K, 2))
        v = (rng.random((N, K)) < 0.7).astype(np.float64)
        v[:, 0] = v[:, 1] = 1.0                                                   # every frame keeps two visible keypoints ...
        if vis == "weights":
            v = v * rng.choice([0.5, 1.0, 2.0], (N, K))
            if not flags & KP_OPTCAM:
                v[:, 2] = -1.0
        elif vis == "some_frames_invisible":
            assert not flags & KP_OPTCAM
            v[::2] = 0.0                                                          # ... but for these: P shrinks
        elif vis == "none":
            assert not flags & KP_OPTCAM
            v[:] = 0.0
        pi, gi = slice_rows(B, T, delta_t)
        # the prediction of slice row r is its gt frame under a per-frame similarity + noise: scales inside, below and above the clip
        a = np.resize(np.array([1.25, -1.0, 0.05, 0.5, 1.0]), len(pi))
        kp = rng.normal(0, 0.3, (N, K, 2))
        kp[pi] = (xy[gi] + rng.normal(0, 0.05, (len(pi), K, 2))) * a[:, None, None] + rng.normal(0, 0.2, (len(pi), 1, 2))
        self.planted = []
        f = lambda x: np.ascontiguousarray(x, np.float32)
        self.kps_gt, self.kps_pred = f(np.concatenate([xy, v[:, :, None]], 2)), f(kp)
        if plant:
            assert not flags & KP_OPTCAM
            for r in range(0, len(pi), 2):
                self.kps_pred[pi[r], 0, r % 2] = self.kps_gt[gi[r], 0, r % 2]
                self.planted.append((pi[r], 0, r % 2))
        self.joints_gt, self.joints_pred = f(rng.normal(0, 0.3, (N, 14, 3))), f(rng.normal(0, 0.3, (N, K, 3)))
        rod = lambda th: G.O.batch_rodrigues(torch.from_numpy(th.reshape(-1, 3))).reshape(N, 24, 3, 3).numpy()
        self.rs_gt, self.rs_pred = f(rod(rng.normal(0, 0.4, (N, 72)))), f(rod(rng.normal(0, 0.4, (N, 72))))
        self.shapes_gt, self.beta_pred = f(rng.normal(0, 1, (B, 10))), f(rng.normal(0, 1, (N, 10)))
        h = {"ones": np.ones(B), "zeros": np.zeros(B), "mixed": (np.arange(B) % 3 != 1).astype(np.float64),
             "weights": np.resize(np.array([0.5, 2.0, 0.0, 1.0]), B)}[has]
        self.has_smpl, self.has_joints = f(h), f(h[::-1])
        self._r = {}
        enforce_min_residual(self)
        check_conditions(self, self.result())

    def kps_pred_f64(self):
        return self.kps_pred

    def pred(self, dtype, grad=False):
        p = {"kps": self.kps_pred, "joints": self.joints_pred, "rs": self.rs_pred, "beta": self.beta_pred}
        return {k: _t(v, dtype).requires_grad_(grad) for k, v in p.items()}

    def gt(self, dtype=None):
        g = {"kps": self.kps_gt, "joints": self.joints_gt, "rs": self.rs_gt, "shapes": self.shapes_gt, "has_gt3d_smpl": self.has_smpl,
             "has_gt3d_joints": self.has_joints}
        return g if dtype is None else {k: _t(v, dtype) for k, v in g.items()}

    def result(self, dtype=torch.float64, flags=None):
        """{losses [7], d_kps, d_joints, d_rs, d_beta (of total), best_cam [N,3] with NaN outside the slice} as float64 arrays"""
        flags = self.flags if flags is None else flags
        key = (dtype, flags)
        if key not in self._r:
            p = self.pred(dtype, grad=True)
            out = losses(p, self.gt(dtype), self.B, self.T, flags, self.weights, self.delta_t)
            names = ("kps", "joints", "rs", "beta")
            g = torch.autograd.grad(out["total"], [p[k] for k in names], allow_unused=True) if out["total"].requires_grad else [None] * 4
            grads = {"d_" + k: (torch.zeros_like(p[k]) if gi is None else gi).to(torch.float64).numpy() for k, gi in zip(names, g)}
            self._r[key] = _result(out, grads, self.B * self.T, slice_rows(self.B, self.T, self.delta_t)[0])
        return self._r[key]


def check_conditions(case, r64):
    """the input conditions of the module docstring, for a stage case or a loop case (r64: its float64 result with `residual`)"""
    pi, gi = slice_rows(case.B, case.T, case.delta_t)
    if case.flags & (KP | KP_OPTCAM):
        res = np.abs(residuals(case))
        vis = np.asarray(case.kps_gt, np.float64)[gi][:, :, 2] != 0
        planted = np.zeros(res.shape, bool)
        row_of = {int(p): i for i, p in enumerate(pi)}
        for (n, k, c) in getattr(case, "planted", ()):
            planted[row_of[int(n)], k, c] = True
            assert res[row_of[int(n)], k, c] == 0.0
        ok = (res >= MIN_RESIDUAL) | planted | ~vis[:, :, None]
        assert ok.all(), (case.name, float(res[~ok].min()))
    if case.flags & KP_OPTCAM:
        raw = r64["scale_raw"]
        assert np.isfinite(raw).all() and (np.abs(raw - 0.7) >= SCALE_MARGIN).all() and (np.abs(raw - 10.0) >= SCALE_MARGIN).all(), (case.name, raw)


def residuals(case):
    """pred - gt of the slice's keypoints in float64, under the optimal camera where the case uses it -> [rows, K, 2]"""
    pi, gi = slice_rows(case.B, case.T, case.delta_t)
    x = torch.from_numpy(np.asarray(case.kps_pred_f64(), np.float64))[pi]
    xg = torch.from_numpy(np.asarray(case.kps_gt, np.float64))[gi]
    if case.flags & KP_OPTCAM:
        cam, _ = optimal_camera(x, xg)
        x = cam[:, None, 0:1] * (x + cam[:, None, 1:3])
    return (x - xg[:, :, :2]).numpy()


def enforce_min_residual(case, target=6e-4, rounds=10):
    """the first input condition, made to hold: a visible keypoint whose residual is below `target` has its GROUND TRUTH moved away
    from the prediction by `target` (a planted zero stays).  Under the optimal camera the move shifts the camera of its frame a
    little, hence the rounds; the builders assert the condition itself afterwards (check_conditions)."""
    if not case.flags & (KP | KP_OPTCAM):
        return
    pi, gi = slice_rows(case.B, case.T, case.delta_t)
    planted = np.zeros((len(pi), case.K, 2), bool)
    row_of = {int(p): i for i, p in enumerate(pi)}
    for (n, k, c) in getattr(case, "planted", ()):
        planted[row_of[int(n)], k, c] = True
    for _ in range(rounds):
        res = residuals(case)
        vis = (np.asarray(case.kps_gt, np.float64)[gi][:, :, 2] != 0)[:, :, None]
        bad = (np.abs(res) < target) & vis & ~planted
        if not bad.any():
            return
        xy = case.kps_gt[gi][:, :, :2].astype(np.float64)
        xy = np.where(bad, xy - np.where(res >= 0, 1.0, -1.0) * target, xy)
        case.kps_gt[gi, :, :2] = xy.astype(np.float32)


def clip_kinds(cases):
    """{'low', 'high', 'inside'} that occur among the optimal-camera frames of the cases"""
    kinds = set()
    for c in cases:
        if c.flags & KP_OPTCAM:
            raw = c.result()["scale_raw"]
            kinds |= {"low"} if (raw < 0.7).any() else set()
            kinds |= {"high"} if (raw > 10.0).any() else set()
            kinds |= {"inside"} if ((raw > 0.7) & (raw < 10.0)).any() else set()
    return kinds


@functools.lru_cache(maxsize=None)
def stage_group(B, T):
    """the loss-stage cases of one (B, T): everything together for every delta_t and both keypoint counts (the plain keypoint loss for
    delta_t = 0, the optimal camera elsewhere, as the trainer; + each the other way round once), each term alone, and the input
    variants"""
    cases = []
    ds = deltas_for(T)
    for d in ds:
        for K in (14, 25):
            cases.append(StageCase(B, T, K, d, ALL | (KP if d == 0 else KP_OPTCAM), seed=len(cases)))
    cases.append(StageCase(B, T, 25, 0, ALL | KP_OPTCAM, seed=len(cases)))
    cases.append(StageCase(B, T, 19, ds[-1], ALL | KP, plant=True, seed=len(cases)))
    for d in sorted(set((0, ds[-1]))):
        for flag in (KP, KP_OPTCAM, JOINTS, SMPL, CONST, SHAPE_PRIOR):
            cases.append(StageCase(B, T, 25, d, flag, seed=len(cases)))
    cases.append(StageCase(B, T, 25, 0, ALL | KP, vis="weights", has="weights", seed=len(cases)))
    cases.append(StageCase(B, T, 14, ds[-1], ALL | KP_OPTCAM, vis="weights", has="ones", seed=len(cases)))
    cases.append(StageCase(B, T, 25, 0, ALL | KP, vis="some_frames_invisible", has="zeros", plant=True, seed=len(cases)))
    cases.append(StageCase(B, T, 14, 0, ALL | KP, vis="none", has="mixed", seed=len(cases)))
    return tuple(cases)


def e32(cases, keys):
    """E32 per key over the cases: the largest |float32 autograd - float64 autograd|; 'losses' is one number over the loss vector"""
    out = {k: 0.0 for k in keys}
    for c in cases:
        r32, r64 = c.result(torch.float32), c.result(torch.float64)
        for k in keys:
            out[k] = max(out[k], float(np.abs(r32[k] - r64[k]).max()))
    return out


def bounds(cases, keys, factor=FACTOR):
    assert 1.0 <= factor <= 8.0
    return {k: factor * v for k, v in e32(cases, keys).items()}


STAGE_KEYS = STAGE_GRADS + ("losses",)


# ---------------------------------------------------------------------------------------------------------------- loop cases
class LoopCase(object):
    """the closed loop on a small synthetic body model: omega [N,85] fp32 -> forward -> losses -> d_omega.  The ground truth is the
    float64 forward of a perturbed omega (+ the per-frame similarity of the optimal-camera families), so every term has a residual"""

    def __init__(self, nv, B, T, delta_t, flags, use_optcam, seed=0, weights=WEIGHTS, has="mixed"):
        self.nv, self.B, self.T, self.delta_t, self.flags, self.use_optcam, self.weights = nv, B, T, delta_t, flags, bool(use_optcam), tuple(weights)
        self.model = G._model(nv)
        self.K = self.model["cocoplus_regressor"].shape[1]
        self.name = "nv%d B%d T%d dt%+d flags%02x%s" % (nv, B, T, delta_t, flags, " optcam" if use_optcam else "")
        N = B * T
        f = lambda x: np.ascontiguousarray(x, np.float32)
        pi, gi = slice_rows(B, T, delta_t)
        rng = np.random.Generator(np.random.PCG64([seed, nv, B, T, delta_t + 100, flags]))
        th, be, ca = S.inputs(N, 7000 + 31 * seed)
        self.omega = f(np.concatenate([ca, th, be], 1))
        # the ground truth of PRED row r is the forward of that row's perturbed omega; it is stored at the row's GT index
        th2 = th + 0.1 * rng.standard_normal(th.shape)
        be2 = be + 0.3 * rng.standard_normal(be.shape)
        ca2 = ca + 0.05 * rng.standard_normal(ca.shape)
        t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64))
        with torch.no_grad():
            o = G.forward(self.model, t64(th2), t64(be2), t64(np.tile([1.0, 0, 0], (N, 1))) if use_optcam else t64(ca2))
        kp = o["kps"].numpy()
        if flags & KP_OPTCAM:
            a = np.resize(np.array([1.25, -1.0, 20.0, 0.5]), N)
            kp = kp * a[:, None, None] + rng.normal(0, 0.2, (N, 1, 2))
        v = (rng.random((N, self.K)) < 0.7).astype(np.float64)
        v[:, 0] = v[:, 1] = 1.0
        gt = {"kps": np.concatenate([kp, v[:, :, None]], 2), "joints": o["joints"].numpy()[:, :14], "rs": o["Rs"].numpy()}
        self.kps_gt, self.joints_gt, self.rs_gt = [f(np.zeros_like(gt[k])) for k in ("kps", "joints", "rs")]
        for dst, k in ((self.kps_gt, "kps"), (self.joints_gt, "joints"), (self.rs_gt, "rs")):
            dst[:] = rng.normal(0, 0.3, dst.shape)                            # (gt rows outside the slice: never read)
            dst[gi] = gt[k][pi]
        self.kps_gt[:, :, 2] = 0.0
        self.kps_gt[gi, :, 2] = v[pi]
        self.shapes_gt = f(be2.reshape(B, T, 10)[:, 0])
        h = {"ones": np.ones(B), "mixed": (np.arange(B) % 3 != 1).astype(np.float64)}[has]
        self.has_smpl, self.has_joints = f(h), f(h[::-1])
        self._r, self._kp64 = {}, None
        enforce_min_residual(self)
        check_conditions(self, self.result())

    def gt(self, dtype=None):
        g = {"kps": self.kps_gt, "joints": self.joints_gt, "rs": self.rs_gt, "shapes": self.shapes_gt, "has_gt3d_smpl": self.has_smpl,
             "has_gt3d_joints": self.has_joints}
        return g if dtype is None else {k: _t(v, dtype) for k, v in g.items()}

    def forward(self, om):
        N = om.shape[0]
        cams = torch.tensor([1.0, 0.0, 0.0], dtype=om.dtype).repeat(N, 1) if self.use_optcam else om[:, :3]
        o = G.forward(self.model, om[:, 3:75], om[:, 75:85], cams)
        return {"kps": o["kps"], "joints": o["joints"], "rs": o["Rs"], "beta": om[:, 75:85]}

    def kps_pred_f64(self):
        if self._kp64 is None:
            with torch.no_grad():
                self._kp64 = self.forward(torch.from_numpy(self.omega.astype(np.float64)))["kps"].numpy()
        return self._kp64

    def result(self, dtype=torch.float64, flags=None, weights=None):
        """{losses [7], d_omega [N,85] and its parts d_cams, d_theta, d_beta, best_cam} as float64 arrays"""
        flags = self.flags if flags is None else flags
        key = (dtype, flags, weights)
        if key not in self._r:
            om = _t(self.omega, dtype).requires_grad_(True)
            out = losses(self.forward(om), self.gt(dtype), self.B, self.T, flags, weights or self.weights, self.delta_t)
            g = torch.autograd.grad(out["total"], om)[0].to(torch.float64).numpy()
            grads = {"d_omega": g}
            grads.update({k: np.ascontiguousarray(g[:, s]) for k, s in OMEGA_PARTS.items()})
            self._r[key] = _result(out, grads, self.B * self.T, slice_rows(self.B, self.T, self.delta_t)[0])
        return self._r[key]


LOOP_KEYS = tuple(OMEGA_PARTS) + ("losses",)


@functools.lru_cache(maxsize=None)
def loop_group(B, T):
    """the closed-loop cases of one (B, T): the present container (plain keypoint loss, the omega's own camera) and a delta container
    (optimal camera, cams [1, 0, 0]) on the 130-vertex model, the present one on the 50-vertex model as well"""
    ds = deltas_for(T)
    cases = [LoopCase(130, B, T, 0, ALL | KP, False, seed=1), LoopCase(50, B, T, 0, ALL | KP, False, seed=2),
             LoopCase(130, B, T, ds[-1], ALL | KP_OPTCAM, True, seed=3)]
    if len(ds) > 1:
        cases.append(LoopCase(50, B, T, ds[1], ALL | KP_OPTCAM, False, seed=4))          # the optimal camera on the omega's own projection
    return tuple(cases)


# ---- the descent of tests/test_gpu_losses.py: total loss of the present container over omega, plain gradient descent.  Step size and
# count are chosen on the host (test_loss_cases.py asserts that the float64 run falls at every step and ends below half its start).
DESCENT_STEPS, DESCENT_LR = 12, 1.0


@functools.lru_cache(maxsize=None)
def descent_case():
    return LoopCase(130, 2, 3, 0, ALL | KP, False, seed=77, weights=(0.2, 1.0, 1.0, 1.0, 0.01), has="ones")


@functools.lru_cache(maxsize=None)
def descent_reference():
    """the float64 run -> [total before step 0, ..., total after the last step]"""
    c = descent_case()
    om = torch.from_numpy(c.omega.astype(np.float64))
    gt = c.gt(torch.float64)
    out = []
    for _ in range(DESCENT_STEPS + 1):
        x = om.clone().requires_grad_(True)
        tot = losses(c.forward(x), gt, c.B, c.T, c.flags, c.weights, 0)["total"]
        out.append(float(tot.detach()))
        om = om - DESCENT_LR * torch.autograd.grad(tot, x)[0]
    return out
