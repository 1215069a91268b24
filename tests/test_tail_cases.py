"""The helper of the f_movie / IEF tail sweep (tests/tail_cases.py) on the host: the composed IEF reference is O.call_hmr_ief, the float64
references reproduce the golden window, the emulated hallucinator without emulation is O.fc2_res, the input families have the properties
the device tests rely on, every family's E32 is float32 noise (finite, non-zero) and FACTOR x E32 is inside the bounds the suite asserted
before.  No GPU."""
import numpy as np
import pytest
import torch

import tail_cases as T
from human_dynamics_amd import assets
from oracle import hmmr_oracle as O


def test_weights_are_the_tail_of_the_synthetic_checkpoint():
    w = T.weights()
    assert not any(k.startswith("resnet_v2_50") for k in w) and "mean_param" in w and "fc2_res/fc3/weights" in w
    w4 = T.temporal_weights(T.MAX_BLOCKS)
    for i in range(T.MAX_BLOCKS):
        assert all(s + "/weights" in w4 or s + "/gamma" in w4 for s in assets.temporal_scopes(i))
        assert all((s + "/weights" in w or s + "/gamma" in w) == (i < T.PACKED_BLOCKS) for s in assets.temporal_scopes(i))
    b0, b3 = assets.temporal_scopes(0), assets.temporal_scopes(3)
    assert all(w4[b3[j] + "/" + v] is w[b0[j] + "/" + v] for j, v in ((0, "gamma"), (1, "weights"), (2, "beta"), (3, "biases")))
    assert len(w4) == len(T.temporal_weights(3)) * 4 // 3 and not any(k.startswith("fc2_res") for k in w4)
    for dt in T.DELTAS7:
        assert w[T.delta_scope(dt) + "/3D_module/fc1/weights"].shape == (2048 + 72, 1024)
        assert T.weights75()[T.delta_scope(dt) + "/3D_module/fc3/weights"].shape == (1024, 75)
    assert len(T.DELTAS7) + 1 == 8 and [len(s) + 1 for s in T.REGRESSOR_SETS] == [1, 2, 3, 5, 8]
    assert all(set(s) <= set(T.DELTAS7) and tuple(sorted(s)) == s for s in T.REGRESSOR_SETS)


@pytest.mark.parametrize("width,from_pred", [(72, True), (72, False), (75, True), (75, False)])
def test_composed_ief_reference_equals_call_hmr_ief_at_three_stages(width, from_pred):
    w = T.ief_weights(width)
    x, start = T.strips_input(5, 1), T.omega_rows(5, 1)
    for emulate in (None, "f16x3"):
        here, deltas = O.call_hmr_ief(O._t(x, torch.float64), O._t(start, torch.float64), w, (-5, 5), torch.float64, emulate,
                                      use_optcam=width == 72, use_delta_from_pred=from_pred)
        mine, md = T.compose_ief(x, start, w, (-5, 5), 3, torch.float64, emulate, use_optcam=width == 72, use_delta_from_pred=from_pred)
        assert float((here - mine).abs().max()) <= 1e-12
        for dt in (-5, 5):
            assert deltas[dt].shape == md[dt].shape == (5, 85) and float((deltas[dt] - md[dt]).abs().max()) <= 1e-12
    # the stage count is really passed on, and ref_ief orders the regressors as the engine does
    two = T.compose_ief(x, start, w, (5,), 2, use_optcam=width == 72, use_delta_from_pred=from_pred)[0]
    assert float((two - mine).abs().max()) > 1e-4
    r = T.ref_ief(x, (5, -5), "f16x3", 3, width, from_pred, start)
    assert r.shape == (3, 5, 85) and np.abs(r[0] - mine.numpy()).max() <= 1e-12
    assert np.abs(r[1] - md[-5].numpy()).max() <= 1e-12 and np.abs(r[2] - md[5].numpy()).max() <= 1e-12


def test_float64_references_reproduce_the_golden_window(weights, golden_window):
    """the conftest checkpoint (seed 0, 3 blocks, deltas -5 and 5) through the same oracle calls the sweep makes"""
    phi = golden_window["phi"].reshape(1, 20, 2048)
    strips = O.az_fc2_groupnorm(phi, weights, 3, torch.float64, None).numpy()[0]
    assert np.abs(strips - golden_window["strips"]).max() < 1e-5          # (the golden file is float32)
    mean = T.start_rows(None, 20, weights)
    here, d = T.compose_ief(golden_window["strips"], mean, weights, (-5, 5))
    got = torch.stack([here, d[-5], d[5]]).numpy()
    assert np.abs(got - golden_window["omegas_all"]).max() < 1e-6


def test_emulated_hallucinator_without_emulation_is_fc2_res():
    w = T.weights()
    phi = T.phi_input(1, 5, 3)[0]
    for dtype in (torch.float64, torch.float32):
        assert torch.equal(T.ref_hallucinator(phi, w, dtype, None), O.fc2_res(phi, w, dtype))
    a, b = T.ref_hallucinate(phi, "bf16"), T.ref_hallucinate(phi, "f32")
    assert 1e-4 < np.abs(a - b).max() < 0.1                               # the emulation rounds something, and only a little


def test_groupnorm_families_deliver_the_promised_inputs():
    for c, groups in ((2048, 32), (256, 32), (512, 4)):
        x, g, be = T.gn_input("offset", 3, 7, c, groups, 1)
        assert abs(x.mean() - 100) < 0.01 and 0.008 < x.std() < 0.012
        x, g, be = T.gn_input("negative", 3, 7, c, groups, 1)
        assert not T.ref_groupnorm_relu(x, g, be, groups).any()
        x, g, be = T.gn_input("constant", 3, 7, c, groups, 1)
        mask = T.gn_constant_mask(3, 7, c, groups)
        xg = x.reshape(3, 7, groups, c // groups)
        const = np.ptp(xg, axis=(1, 3)) == 0
        assert const.sum() == 3 * groups // 2 and mask.sum() == const.sum() * 7 * (c // groups)
        assert np.array_equal(np.broadcast_to(const[:, None, :, None], xg.shape).reshape(x.shape), mask)
        ref = T.ref_groupnorm_relu(x, g, be, groups)
        want = np.broadcast_to(np.maximum(be.astype(np.float64), 0), x.shape)
        assert np.abs(ref - want)[mask].max() < 1e-9 and ref[~mask].max() > 1
    assert (T.gn_input("standard", 1, 1, 256, 32, 2)[1] > 0.49).all()
    h = T.half_unit(np.array([0.0, 1.0, 1.5, 3.0, 1e-3]), "bf16")
    assert h[0] == 0 and h[1] == h[2] == 2.0 ** -8 and h[3] == 2.0 ** -7
    assert T.half_unit(np.array([1.0]), "f32")[0] == 2.0 ** -24 and T.half_unit(np.array([1.0, 1e-4]), "f16x3").tolist() == [2.0 ** -22, 2.0 ** -25]


def _noise(e, lo, hi):
    assert np.isfinite(e[0]) and np.isfinite(e[1]) and lo < e[1] <= e[0] < hi, (e, lo, hi)


@pytest.mark.parametrize("mode", T.MODES)
def test_every_family_has_a_finite_nonzero_e32_inside_the_legacy_bound(mode):
    """E32 is float32 noise (bf16: the noise that tips single operands over a rounding boundary), not a broken reference, and FACTOR x
    E32 stays inside what the suite asserted before"""
    hi = 2.0 ** -7 if mode == "bf16" else 5e-6                            # bf16: within one unit in the last place of a value in [1, 2)
    for blocks in range(1, T.MAX_BLOCKS + 1):
        e = T.e32_temporal(mode, blocks)
        print("E32 temporal %-5s blocks %d  max %.3e rms %.3e" % (mode, blocks, e[0], e[1]))
        _noise(e, 1e-9, hi)
        if (("temporal", mode) in T.LEGACY) and blocks <= 3:
            assert T.bound(e, mode)[0] < T.LEGACY[("temporal", mode)]
    e = T.e32_hallucinator(mode)
    print("E32 hallucinator %-5s  max %.3e rms %.3e" % (mode, e[0], e[1]))
    _noise(e, 1e-9, hi)
    for stages, width, from_pred in [(s, 72, True) for s in (1, 2, 3, 4)] + [(3, 72, False), (3, 75, True), (3, 75, False)]:
        e = T.e32_ief(mode, stages, width, from_pred)
        for k in ("present", "delta"):
            print("E32 ief %-5s stages %d width %d from_pred %d %-7s max %.3e rms %.3e" % (mode, stages, width, from_pred, k, e[k][0], e[k][1]))
            _noise(e[k], 1e-10, hi)
            if ("ief", mode) in T.LEGACY and stages <= 3:
                assert T.bound(e[k], mode)[0] < T.LEGACY[("ief", mode)]
    assert T.bound((1.0, 0.5), "bf16") == (T.FACTOR, T.FACTOR / 2) and T.bound((1.0, 0.5), "f32") == (T.FACTOR, None)
    assert 4.0 <= T.FACTOR <= 16.0
    with pytest.raises(AssertionError):
        T.bound((1.0, 0.5), "f32", factor=16.5)


def test_groupnorm_e32_is_finite_and_nonzero():
    for fam in ("standard", "offset", "constant"):
        for c, groups in ((2048, 32), (256, 32), (512, 4)):
            e = T.e32_groupnorm(fam, c, groups)
            print("E32 groupnorm %-8s c %4d groups %2d  max %.3e rms %.3e" % (fam, c, groups, e[0], e[1]))
            assert np.isfinite(e[0]) and 0 < e[0] < (1e-2 if fam != "standard" else 5e-6)
    assert T.e32_groupnorm("negative", 256, 32) == (0.0, 0.0)              # exactly 0 in both precisions: asserted exactly on the device


def test_restated_ief_workspace_is_the_library_s():
    from human_dynamics_amd import _lib as L
    lib = L.load()
    for mode, dt in (("f32", L.HMMR_F32), ("bf16", L.HMMR_BF16), ("f16x3", L.HMMR_F16X3)):
        for m in (1, 20, 65, 257):
            for R in range(1, 9):
                th0, th_s, g, total = T.ief_theta_sets(m, R, mode)
                assert total == lib.hmmr_ief_workspace_bytes(m, R, dt), (mode, m, R)
                assert g == max(R - 1, 1) and th_s >= m * 512 and th0 % 256 == 0
