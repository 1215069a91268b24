"""The f_movie / hallucinator backward's cases on the host (tests/movie_grad_cases.py): the oracle is pinned to oracle.hmmr_oracle, every
case's prepared weights meet the cap on nudged channels, a dropped term of the backward cannot pass the bound, hmmr_temporal_bwd /
hmmr_hallucinator_bwd refuse bad calls with -1 and a message in front of any launch, the workspaces are the stated layouts, the header,
the ctypes table and the structs agree, and the bank converts to the checkpoint's shapes and back."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from human_dynamics_amd import _lib
import movie_grad_cases as MC
import tail_cases as TC
from oracle import hmmr_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmmr_hip.h")


# ---------------------------------------------------------------------------------------------------------------- the oracle and the cases
@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_temporal_oracle_is_the_reference_function(blocks):
    phi = TC.phi_input(2, 7, 21)
    with torch.no_grad():
        got = MC.temporal_forward(MC.temporal_params(blocks, torch.float64, None, False), torch.tensor(np.asarray(phi, np.float64))).numpy()
    ref = O.az_fc2_groupnorm(phi, TC.temporal_weights(blocks), blocks, torch.float64).numpy()
    assert got.shape == ref.shape == (2, 7, 2048)
    assert float(np.abs(got - ref).max()) <= 1e-12


def test_hallucinator_oracle_is_the_reference_function():
    phi = TC.phi_input(1, 9, 21)[0]
    with torch.no_grad():
        got = MC.hal_forward(MC.hal_params(torch.float64, None, False), torch.tensor(np.asarray(phi, np.float64))).numpy()
    ref = O.fc2_res(phi, TC.weights(), torch.float64).numpy()
    assert float(np.abs(got - ref).max()) <= 1e-12


def test_the_cases_are_the_stated_ones():
    assert [(c.b, c.t, c.blocks) for c in MC.TEMPORAL_CASES] == [(1, 1, 1), (1, 2, 1), (1, 3, 1), (2, 7, 1), (2, 7, 3), (5, 7, 1), (1, 33, 1),
                                                                 (4, 17, 2), (3, 20, 3)]
    assert [c.m for c in MC.HAL_CASES] == [1, 14, 33, 68]
    assert max(MC.rows_of(c) for c in MC.TEMPORAL_CASES + MC.HAL_CASES) <= MC.MAX_ROWS
    # (4, 17): the weight gradient's four contraction slices
    K = 4 * 17
    ks = ((K + 3) // 4 + 15) // 16 * 16
    assert [max(0, min(K, (w + 1) * ks) - w * ks) for w in range(4)] == [32, 32, 4, 0]


@pytest.mark.parametrize("case", MC.TEMPORAL_CASES + MC.HAL_CASES + (MC.HAL_CHAIN_H,), ids=lambda c: c.name)
def test_few_channels_are_nudged_and_none_is_left_ambiguous(case):
    weights, log = MC.prepared(case)
    assert len(log) == (2 * case.blocks if isinstance(case, MC.TCase) else 2) == len(weights)
    for l in log:
        print("%s %-40s tau %.3e  %2d channel(s) nudged in %d round(s)" % (case.name, l["layer"], l["tau"], l["nudged"], l["rounds"]))
        assert l["nudged"] <= MC.MAX_NUDGED and l["rounds"] <= MC.MAX_ROUNDS and l["left"] == 0
        assert 0.0 < l["tau"] < 1e-3
        assert l["closest"] is None or l["closest"] >= MC.CLEAR * l["tau"]
    src = TC.weights()
    for name, a in weights.items():
        assert a.dtype == np.float32 and a.shape == (2048,)
        assert int((a != np.asarray(src[name], np.float32)).sum()) <= MC.MAX_NUDGED


@pytest.mark.parametrize("group", [("temporal", 1), ("temporal", 2), ("temporal", 3), ("hal",)], ids=str)
def test_every_reference_is_a_thousand_bounds_large(group):
    """a dropped term cannot pass: under a cotangent on the strips (the hallucinator's output) every quantity of the group's largest case
    holds values at least 1000 bounds large, and every bound is positive"""
    case = max(MC.cases_of(group), key=MC.rows_of)
    bound, ref = MC.bounds(case), MC.reference(case)
    assert sorted(bound) == sorted(ref)
    for k in sorted(ref):
        big = float(np.abs(ref[k]).max())
        print("%-14s %-16s bound %.3e  max |ref| %.3e = %.0f bounds" % (group, k, bound[k], big, big / bound[k]))
        assert 0.0 < bound[k] and big >= 1000 * bound[k], (group, k, big, bound[k])


def test_descent_reference_falls_at_every_step():
    d64, bound = MC.descent_reference()
    print("descent float64:", " ".join("%.4f" % x for x in d64))
    print("descent bound:  ", " ".join("%.1e" % x for x in bound))
    assert len(d64) == MC.DESCENT_STEPS + 1 == len(bound)
    assert all(b < a for a, b in zip(d64, d64[1:])) and d64[-1] < 0.75 * d64[0]
    assert all(0.0 < b < 1e-5 * x for b, x in zip(bound, d64))


def test_e_hallucinate_chain_has_positive_bounds():
    ref, bound = MC.hal_chain_reference()
    assert sorted(ref) == sorted(bound) and len(ref) == 2 + 3 * 8 + 6
    for k in sorted(ref):
        big = float(np.abs(ref[k]).max())
        print("e_hallucinate %-16s bound %.3e  max |ref| %.3e" % (k, bound[k], big))
        assert 0.0 < bound[k] < 1e-2 * big, (k, bound[k], big)


# ---------------------------------------------------------------------------------------------------------------- the C entry points, no device
P = [0x10000 * (i + 1) for i in range(12)]
BIG = 1 << 40


def _temporal_bank(dt=_lib.HMMR_F32, blocks=3, scale=False, missing=None):
    """a syntactically valid bank with dummy (never dereferenced) pointers"""
    tw = _lib.TemporalWeights()
    tw.dtype, tw.num_blocks = dt, blocks
    for i in range(_lib.MAX_TEMPORAL_BLOCKS):
        b = tw.block[i]
        b.gn1_gamma, b.gn1_beta, b.gn2_gamma, b.gn2_beta = P[3], P[3], P[3], P[3]
        for lay in (b.conv1, b.conv2):
            lay.w, lay.shift = P[4], P[5]
    if scale:
        tw.block[1].conv2.scale = P[6]
    if missing:
        setattr(tw.block[0], missing, None)
    return tw


def _hal_bank(dt=_lib.HMMR_F32, scale=False):
    hw = _lib.HallucinatorWeights()
    hw.dtype = dt
    for lay in (hw.fc1, hw.fc2, hw.fc3):
        lay.w, lay.shift = P[4], P[5]
    if scale:
        hw.fc2.scale = P[6]
    return hw


def _refused(lib, rc, *words):
    msg = lib.hmmr_last_error()
    assert rc == -1 and msg, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_temporal_bwd_refuses_before_anything_is_queued():
    lib = _lib.load()

    def call(tw=None, w=True, desc=True, ws=P[2], ws_bytes=BIG, outputs=("d_phi",), **kw):
        tw = _temporal_bank() if tw is None else tw
        d = _lib.TemporalBwdDesc()
        d.phi, d.b, d.t, d.d_strips = P[0], 2, 7, P[1]
        for k, v in kw.items():
            setattr(d, k, v)
        for o in outputs:
            if o == "d_phi":
                d.d_phi = P[8]
            else:
                setattr(d.block[o[0]], o[1], P[9])
        return lib.hmmr_temporal_bwd(C.byref(tw) if w else None, C.byref(d) if desc else None, ws, ws_bytes, None)

    who = b"hmmr_temporal_bwd"
    _refused(lib, call(desc=False), who, b"null descriptor")
    _refused(lib, call(w=False), who, b"null argument")
    for missing in ("phi", "d_strips"):
        _refused(lib, call(**{missing: None}), who, b"null argument")
    _refused(lib, call(ws=None), who, b"null argument")
    for bad in (dict(b=0), dict(b=-1), dict(t=0), dict(t=-3)):
        _refused(lib, call(**bad), who, b"must be positive")
    for dt in (_lib.HMMR_BF16, _lib.HMMR_F16X3, 3, -1):
        _refused(lib, call(_temporal_bank(dt)), who, b"HMMR_F32")
    _refused(lib, call(_temporal_bank(scale=True)), who, b"block 1", b"not an HMMR_F32 bank")
    _refused(lib, call(_temporal_bank(missing="gn2_beta")), who, b"block 0", b"not an HMMR_F32 bank")
    for blocks in (0, -1, _lib.MAX_TEMPORAL_BLOCKS + 1):
        _refused(lib, call(_temporal_bank(blocks=blocks)), who, b"bad num_blocks")
    _refused(lib, call(outputs=()), who, b"no output is requested")
    _refused(lib, call(outputs=((5, "d_conv2"),)), who, b"no output is requested")          # block 5 of 3 does not exist
    need = lib.hmmr_temporal_bwd_workspace_bytes(2, 7, 3)
    for outputs in (("d_phi",), ((2, "d_b2"),), ((0, "d_gn1_gamma"), "d_phi")):
        _refused(lib, call(outputs=outputs, ws_bytes=need - 1), who, b"workspace too small")


def test_hallucinator_bwd_refuses_before_anything_is_queued():
    lib = _lib.load()

    def call(hw=None, w=True, desc=True, ws=P[2], ws_bytes=BIG, outputs=("d_phi",), **kw):
        hw = _hal_bank() if hw is None else hw
        d = _lib.HallucinatorBwdDesc()
        d.phi, d.m, d.d_out = P[0], 5, P[1]
        for k, v in kw.items():
            setattr(d, k, v)
        for o in outputs:
            setattr(d, o, P[8])
        return lib.hmmr_hallucinator_bwd(C.byref(hw) if w else None, C.byref(d) if desc else None, ws, ws_bytes, None)

    who = b"hmmr_hallucinator_bwd"
    _refused(lib, call(desc=False), who, b"null descriptor")
    _refused(lib, call(w=False), who, b"null argument")
    for missing in ("phi", "d_out"):
        _refused(lib, call(**{missing: None}), who, b"null argument")
    _refused(lib, call(ws=None), who, b"null argument")
    for m in (0, -7):
        _refused(lib, call(m=m), who, b"m must be positive")
    for dt in (_lib.HMMR_BF16, _lib.HMMR_F16X3, 3):
        _refused(lib, call(_hal_bank(dt)), who, b"HMMR_F32")
    _refused(lib, call(_hal_bank(scale=True)), who, b"not an HMMR_F32 bank")
    _refused(lib, call(outputs=()), who, b"no output is requested")
    need = lib.hmmr_hallucinator_bwd_workspace_bytes(5)
    for outputs in (("d_phi",), ("d_b3",), ("d_fc1", "d_b2")):
        _refused(lib, call(outputs=outputs, ws_bytes=need - 1), who, b"workspace too small")


def test_workspaces_are_the_stated_layouts():
    lib = _lib.load()
    for b, t, n in ((1, 1, 1), (2, 7, 1), (2, 7, 3), (5, 7, 2), (1, 33, 1), (3, 20, 3), (8, 20, 3), (3, 5, _lib.MAX_TEMPORAL_BLOCKS)):
        assert lib.hmmr_temporal_bwd_workspace_bytes(b, t, n) == MC.temporal_bwd_workspace_bytes(b, t, n), (b, t, n)
    for b, t, n in ((0, 7, 3), (-1, 7, 3), (2, 0, 3), (2, -1, 3), (2, 7, 0), (2, 7, _lib.MAX_TEMPORAL_BLOCKS + 1)):
        assert lib.hmmr_temporal_bwd_workspace_bytes(b, t, n) == 0
    for m in (1, 14, 33, 68, 256):
        assert lib.hmmr_hallucinator_bwd_workspace_bytes(m) == MC.hal_bwd_workspace_bytes(m), m
    assert lib.hmmr_hallucinator_bwd_workspace_bytes(0) == 0 and lib.hmmr_hallucinator_bwd_workspace_bytes(-3) == 0


def _header_struct(name):
    """the field names of `typedef struct { ... } name;` in the header, in order (comments removed, arrays kept as names)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", part.strip().split()[-1].lstrip("*")) for part in decl.split(",")]
    return fields


def test_header_table_and_structs_agree():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in ("hmmr_temporal_bwd_workspace_bytes", "hmmr_temporal_bwd", "hmmr_hallucinator_bwd_workspace_bytes", "hmmr_hallucinator_bwd"):
        assert re.search(r"\b%s\s*\(" % fn, src) and fn in _lib.SIGNATURES, fn
        assert hasattr(_lib.load(), fn)
    names = lambda s: [f[0] for f in s._fields_]
    assert _header_struct("hmmr_temporal_block_grads_t") == names(_lib.TemporalBlockGrads) == ["d_" + n for n in MC.BLOCK_NAMES]
    assert _header_struct("hmmr_temporal_bwd_desc_t") == names(_lib.TemporalBwdDesc)
    assert _header_struct("hmmr_hallucinator_bwd_desc_t") == names(_lib.HallucinatorBwdDesc)
    assert names(_lib.HallucinatorBwdDesc)[4:] == ["d_" + n for n in MC.HAL_NAMES]
    # the sizes of the C structs on an LP64 target: pointers of 8 bytes, an int pair (or an int and its padding) in front of a pointer
    assert C.sizeof(_lib.TemporalBlockGrads) == 8 * 8
    assert C.sizeof(_lib.TemporalBwdDesc) == 8 + 4 + 4 + 8 + 8 + _lib.MAX_TEMPORAL_BLOCKS * 64
    assert C.sizeof(_lib.HallucinatorBwdDesc) == 8 + 8 + 8 + 8 + 6 * 8
    assert _lib.load().hmmr_abi_version() == 19 == _lib.ABI_VERSION


# ---------------------------------------------------------------------------------------------------------------- the bank, on the host
def test_bank_converts_to_the_checkpoint_and_back():
    from human_dynamics_amd import packing
    from human_dynamics_amd.movie_bank import BLOCK_NAMES, HAL_NAMES, MovieBank
    assert BLOCK_NAMES == MC.BLOCK_NAMES and HAL_NAMES == MC.HAL_NAMES
    src = TC.weights()
    blocks = 2
    held = {v for i in range(blocks) for v in MC.block_vars(i).values()}
    want = {k: np.asarray(v, np.float32) for k, v in src.items() if k.startswith("fc2_res/") or k in held}
    bank = MovieBank(src, "cpu", num_conv_layers=blocks)
    assert bank.tw.dtype == _lib.HMMR_F32 and bank.tw.num_blocks == blocks and bank.hw is not None and bank.hw.dtype == _lib.HMMR_F32
    got = bank.to_checkpoint()
    assert sorted(got) == sorted(want) == sorted(bank.to_checkpoint_names())
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    # the views are the packed rows: packing.pack_conv_weight's [co][tap * 2048 + ci], fc weights transposed
    v = MC.block_vars(1)
    assert np.array_equal(bank.blocks[1]["conv2"].numpy(), packing.pack_conv_weight(src[v["conv2"]]))
    assert np.array_equal(bank.hal["fc3"].numpy(), np.asarray(src["fc2_res/fc3/weights"]).T)
    assert len(bank.tensors()) == 8 * blocks + 6 and len(bank.temporal_tensors()) == 8 * blocks
    for blob, tensors in ((bank.store.tensors[0], bank.temporal_tensors()), (bank.store.tensors[-1], bank.hallucinator_tensors())):
        lo, hi = blob.data_ptr(), blob.data_ptr() + blob.numel()
        assert all(lo <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= hi for t in tensors)
    assert bank.blocks[0]["conv1"].data_ptr() == bank.tw.block[0].conv1.w and bank.blocks[1]["b2"].data_ptr() == bank.tw.block[1].conv2.shift
    assert bank.blocks[1]["gn2_beta"].data_ptr() == bank.tw.block[1].gn2_beta and bank.hal["b2"].data_ptr() == bank.hw.fc2.shift
    # another checkpoint goes in and comes out unchanged
    rng = np.random.default_rng(3)
    x = {k: rng.standard_normal(a.shape).astype(np.float32) for k, a in got.items()}
    back = bank.load_checkpoint(x).to_checkpoint()
    assert all(np.array_equal(back[k], x[k]) for k in x)
    # a set of gradients converts the same way
    gb, gh = bank.like(fill=0)
    gb[1]["conv1"][5, 2 * 2048 + 7] = 1.0                # co 5, tap 2, ci 7
    gh["fc2"][3, 9] = 2.0                                # out 3, in 9
    ck = bank.to_checkpoint((gb, gh))
    assert sorted(ck) == sorted(want)
    w1 = ck[v["conv1"]]
    assert w1.shape == (3, 1, 2048, 2048) and w1[2, 0, 7, 5] == 1.0 and np.count_nonzero(w1) == 1
    assert ck["fc2_res/fc2/weights"][9, 3] == 2.0 and np.count_nonzero(ck["fc2_res/fc2/weights"]) == 1
    assert "fc2_res/fc1/weights" not in bank.to_checkpoint((gb, None))
    with pytest.raises(KeyError):
        bank.load_checkpoint({"single_view_ief/3D_module/fc1/weights": np.zeros(3, np.float32)})
    with pytest.raises(KeyError):
        bank.load_checkpoint({MC.block_vars(2)["b1"]: np.zeros(2048, np.float32)})                # block 2 of a two-block bank
