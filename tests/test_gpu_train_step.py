"""HMRSequenceTrainer.train_step on the device (human_dynamics_amd/trainer_sequence_fc.py) on the smallest problem that has every wiring
(tests/train_step_cases.py), the hallucinator and the discriminator each on and off:
  wiring   after the trainer's backward every bank tensor's .grad equals, byte for byte, the gradient of the same autograd functions
           called by hand (e_loss and d_loss differentiated SEPARATELY by hand: d_pose must not reach the encoder, e_pose not the
           discriminator), and the returned keys are the reference's for the configuration;
  update   the parameters after one train_step are the bytes of the float32 NumPy Adam oracle applied to those gradients; `iteration`
           advances by 1 or 2; with the discriminator off its bank keeps every byte;
  padding  after 3 steps every padded region of the three banks is exactly 0 and the banks survive the checkpoint round trip;
  replay   a step with the recorded dropout masks reproduces its bytes;
  descent  e_loss over 6 steps follows the whole step restated on the host in torch float64 from the existing case modules' functions
           plus a float64 TF Adam (train_step_cases.Restated, which shares nothing with the trainer), within 4 x E32, E32 being the
           largest deviation of the same restatement run in float32.  With `-s` every step prints its deviation, E32 and their ratio
           (profiles/train_step_sweep.log is one such run).
The banks are restored after every test."""
import numpy as np
import pytest
import torch

import adam_cases as A
import train_step_cases as S

pytestmark = pytest.mark.gpu
_STATE = {}


def _setup(device):
    if device not in _STATE:
        from human_dynamics_amd.engine import HmmrEngine
        from human_dynamics_amd.omega import OmegasGt
        eng = HmmrEngine(S.weights(), S.smpl_model(), dtype="f32", device=device, num_conv_layers=S.BLOCKS, delta_t_values=S.DELTAS)
        b = S.batch()
        gt = OmegasGt(S.Config(False, False), b["poses_aa"], b["shapes"], b["joints"], b["kps"], batch_size=S.B, engine=eng)
        gt.poses_rot = torch.from_numpy(S.rs_gt(b)).to(device).reshape(S.B, S.T, 24, 3, 3)        # the array the host restatement reads
        banks = (eng.movie_bank(), eng.ief_bank(), eng.disc_pose_bank())
        _STATE[device] = (eng, b, gt, banks, [bk.to_checkpoint() for bk in banks])
    return _STATE[device]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    _STATE.clear()


def _restore(state):
    eng, b, gt, banks, before = state
    for bk, ck in zip(banks, before):
        bk.load_checkpoint(ck)
    for t in banks[0].tensors() + banks[1].tensors() + [banks[1].mean_theta] + banks[2].tensors():
        t.grad = None


def _trainer(state, hal, disc, seed=0, lr=None):
    from human_dynamics_amd.trainer_sequence_fc import HMRSequenceTrainer
    eng = state[0]
    for t in eng.disc_pose_bank().tensors():
        t.requires_grad_(False)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(seed)
    cfg = S.Config(hal, disc)
    if lr is not None:
        cfg.e_lr = cfg.d_lr = lr
    return HMRSequenceTrainer(cfg, eng, generator=gen)


def _args(state, keep=None):
    eng, b, gt = state[:3]
    return dict(phis=b["phis"], gt=gt, poses_real=b["poses_real"], has_gt3d_smpl=b["has_gt3d_smpl"], has_gt3d_joints=b["has_gt3d_joints"], keep=keep)


def _bytes(ts):
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.tobytes() == b.tobytes())


def _hand_gradients(state, tr, keep):
    """e_loss and d_loss of the hand-written step, each differentiated on its own"""
    eng, b, gt = state[:3]
    e_loss, d_loss, losses = S.hand_losses(eng, tr.config, gt, b, keep)
    ge = torch.autograd.grad(e_loss, tr.E_var, retain_graph=True, allow_unused=True)
    gd = torch.autograd.grad(d_loss, tr.D_var, allow_unused=True) if tr.use_disc_pose else [None] * len(tr.D_var)
    return _bytes(ge), _bytes(gd), e_loss.detach(), d_loss.detach(), losses


@pytest.mark.parametrize("hal,disc", S.CONFIGS)
def test_wiring_and_one_update(hal, disc, gpu_device):
    state = _setup(gpu_device)
    eng = state[0]
    try:
        tr = _trainer(state, hal, disc)
        # -- wiring: the trainer's forward + backward against the hand-written step, same dropout masks
        losses, e_loss, d_loss = tr.compute_losses(**_args(state))
        keep = tr.last_keep
        assert (keep[1] is not None) == hal
        tr.backward(e_loss, d_loss)
        got_e, got_d = _bytes([t.grad for t in tr.E_var]), _bytes([t.grad for t in tr.D_var])
        tr.e_opt.zero_grad()
        for t in tr.D_var:
            t.grad = None
        ge, gd, e_hand, d_hand, l_hand = _hand_gradients(state, tr, keep)
        assert set(losses) == S.reference_keys(hal)
        assert float(e_loss.detach()) == float(e_hand) and float(d_loss.detach()) == float(d_hand)
        for k in S.reference_keys(hal):
            assert float(losses[k].detach()) == float(l_hand[k].detach()), k
        assert sum(g is not None for g in ge) >= len(ge) - 1 and all(np.isfinite(g).all() for g in ge if g is not None)
        for i, (a, w) in enumerate(zip(got_e, ge)):
            assert _same(a, w), "E_var[%d]: the trainer's gradient is not the hand-written step's" % i
        for i, (a, w) in enumerate(zip(got_d, gd)):
            assert _same(a, w), "D_var[%d]" % i
        assert all(g is None for g in got_d) == (not disc)
        # the hallucinator's tensors are trained only with do_hallucinate, and e_hallucinate reaches the temporal encoder too
        assert len(tr.E_var) == 8 * S.BLOCKS + (6 if hal else 0) + 7 * 3 + 1

        # -- update: one train_step from the restored banks with the same masks = the NumPy oracle on those gradients
        _restore(state)
        p_e, p_d = _bytes(tr.E_var), _bytes(tr.D_var)
        tr = _trainer(state, hal, disc)
        out = tr.train_step(**_args(state, keep))
        assert set(out) == S.reference_keys(hal) | {"e_loss", "d_loss", "iteration"}
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in out.values())
        assert int(out["iteration"]) == tr.iteration == (2 if disc else 1)
        assert float(out["e_loss"]) == float(e_hand) and float(out["d_loss"]) == float(d_hand)
        moved = 0
        for i, (t, p0, g) in enumerate(zip(tr.E_var, p_e, ge)):
            want = p0.reshape(-1) if g is None else S.adam_first_step(p0, g, S.E_LR)
            got = t.detach().cpu().numpy().reshape(-1)
            assert got.tobytes() == want.tobytes(), "E_var[%d] after the step: %d values differ from the oracle" % (i, int((got != want).sum()))
            moved += int((got != p0.reshape(-1)).sum())
        assert moved > 1000000                                    # the step is not a no-op
        for i, (t, p0, g) in enumerate(zip(tr.D_var, p_d, gd)):
            want = p0.reshape(-1) if g is None else S.adam_first_step(p0, g, S.D_LR)          # the discriminator off: every byte kept
            assert t.detach().cpu().numpy().reshape(-1).tobytes() == want.tobytes(), "D_var[%d]" % i
        assert tr.e_opt.beta1_power == A.powers(A.BETA1, 1) and tr.e_opt.beta2_power == A.powers(A.BETA2, 1)
    finally:
        _restore(state)


def test_padding_stays_zero_and_banks_round_trip(gpu_device):
    from human_dynamics_amd.disc_bank import PoseDiscBank
    from human_dynamics_amd.ief_bank import IefBank
    from human_dynamics_amd.movie_bank import MovieBank
    state = _setup(gpu_device)
    eng, _, _, (movie, ief, disc), _ = state
    try:
        tr = _trainer(state, True, True)
        its = [int(tr.train_step(**_args(state))["iteration"]) for _ in range(3)]
        assert its == [2, 4, 6]
        zero = lambda x: not x.detach().cpu().numpy().view(np.int32).any()
        p = disc.params
        assert zero(p["fc1"][:, 736:]) and zero(p["conv1"][:, 9:]) and zero(p["heads"][23:]) and zero(p["bj"][23:]) and zero(p["fc_out"][1:]) and zero(p["bo"][1:])
        for r, nd in enumerate(ief.nd):
            q = ief.params[r]
            assert nd in (85, 72) and zero(q["fc1_theta"][:, nd:]) and zero(q["fc3"][nd:]) and zero(q["b3"][nd:]), r
        # the live parts did move
        assert not zero(p["fc1"][:, :736] - torch.from_numpy(state[4][2]["D_pose/D_alljoints_fc1/weights"].T.copy()).to(eng.device))
        same = lambda a, b: all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))
        assert same(PoseDiscBank(disc.to_checkpoint(), eng.device).tensors(), disc.tensors())
        fresh = IefBank(ief.to_checkpoint(), [k for k in ief.keys if k != 0], eng.device, num_stages=ief.iw.num_stages)
        assert same(fresh.tensors() + [fresh.mean_theta], ief.tensors() + [ief.mean_theta])
        assert same(MovieBank(movie.to_checkpoint(), eng.device, num_conv_layers=S.BLOCKS).tensors(), movie.tensors())
        # the optimiser's moments have the banks' layouts: named as TF names its slots
        like = lambda ts: {n: t for n, t in zip(disc.params, ts)}
        sd = tr.d_opt.state_dict(lambda ts: disc.to_checkpoint(tensors=like(ts)))
        assert "D_pose/D_alljoints_fc1/weights/Adam" in sd and "D_pose/D_alljoints_fc1/weights/Adam_1" in sd
        assert sd["D_pose/D_alljoints_fc1/weights/Adam_1"].shape == (736, 1024) and sd["D_pose/D_alljoints_fc1/weights/Adam_1"].min() >= 0
        assert sd["beta1_power"] == A.powers(A.BETA1, 3)
    finally:
        _restore(state)


def test_a_step_with_its_recorded_masks_reproduces_its_bytes(gpu_device):
    state = _setup(gpu_device)
    try:
        tr = _trainer(state, True, True, seed=3)
        out1 = tr.train_step(**_args(state))
        keep = tr.last_keep
        after1 = _bytes(tr.E_var + tr.D_var)
        _restore(state)
        tr = _trainer(state, True, True, seed=4)                  # another stream of draws: the masks come from `keep`
        out2 = tr.train_step(**_args(state, keep))
        assert all(torch.equal(a, b) for a, b in zip(tr.last_keep, keep))
        for a, b in zip(after1, _bytes(tr.E_var + tr.D_var)):
            assert a.tobytes() == b.tobytes()
        for k in out1:
            assert torch.equal(out1[k], out2[k]), k
        # ... and other masks give another step
        _restore(state)
        tr = _trainer(state, True, True, seed=4)
        out3 = tr.train_step(**_args(state))
        assert not torch.equal(out3["e_loss"], out1["e_loss"])
    finally:
        _restore(state)


@pytest.mark.parametrize("hal,disc", ((True, True), (False, False)))
def test_six_steps_follow_the_float64_restatement(hal, disc, gpu_device):
    """everything on, and everything off: the device's e_loss before each of 6 steps against the float64 run of the restated step"""
    d64, bound, dev32 = S.descent_reference(hal, disc)
    assert all(b < a for a, b in zip(d64, d64[1:])) and d64[-1] < 0.9 * d64[0], d64          # the test rate makes e_loss fall visibly
    state = _setup(gpu_device)
    keep = S.descent_keep()
    try:
        tr = _trainer(state, hal, disc, lr=S.DESCENT_LR)
        got = [tr.train_step(**_args(state, (keep[0], keep[1] if hal else None)))["e_loss"] for _ in range(S.DESCENT_STEPS)]
        got = [float(v) for v in got]
    finally:
        _restore(state)
    worst = 0.0
    for i, (g, r, b, e) in enumerate(zip(got, d64, bound, dev32)):
        ratio = abs(g - r) / (b / 4.0)
        worst = max(worst, ratio)
        print("train_step descent hal=%d disc=%d step %d: device e_loss %.6f  float64 %.6f  deviation %.2e  E32 %.2e (float32 run's deviation %.2e)  ratio %.2f"
              % (hal, disc, i, g, r, abs(g - r), b / 4.0, e, ratio))
    print("train_step descent hal=%d disc=%d: largest deviation / E32 = %.2f (bound 4)" % (hal, disc, worst))
    for i, (g, r, b) in enumerate(zip(got, d64, bound)):
        assert abs(g - r) <= b, (i, g, r, b)


def test_unbuilt_configurations_are_refused(gpu_device):
    from human_dynamics_amd.trainer_sequence_fc import HMRSequenceTrainer
    state = _setup(gpu_device)
    for field, value in (("use_hmr_only", True), ("precomputed_phi", False), ("freeze_phi", False)):
        cfg = S.Config(False, True)
        setattr(cfg, field, value)
        with pytest.raises(NotImplementedError, match=field):
            HMRSequenceTrainer(cfg, state[0])
