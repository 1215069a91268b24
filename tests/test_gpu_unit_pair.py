"""csrc/unit_pair.hip ALONE (engine.unit_pair -> hmmr_bottleneck_tail with a pair_stream), all five forms of hmmr_unit_pair_split:

    b3     256 -> 1024 -> 256 with a shortcut tensor          b3_ws / b2_ws   the same with hmmr_debug_t.pair_form = 2 (wave-specialised)
    b2     128 ->  512 -> 128 with a shortcut tensor          b2f             b2 with the shortcut folded into conv3's K (c_xp = 256)

against (1) the two hmmr_conv_gemm launches it replaces on the same operands, bit for bit, and (2) a float64 product of the operands as
stored.  Every input carries trailing rows of NaN halves and every output starts as a sentinel word with trailing guard rows: a read or
a store past row M shows (hmmr_run_flags / the sentinel).  The library's unit_pair launch counter proves which kernel ran.

    a  ragged row counts (one row, one valid row in a wave, on / off the 32- and 128-row boundaries), one tile per workgroup
    b  float64
    c  persistent workgroups of the block-2 forms: 1, 2, 3, CUs + 1, 2 CUs, 2 CUs + 1 tiles, forced on / off / the default switch
    d  descriptor values the ResNet never passes: a shortcut row stride > depth, relu1 = 0, shift3 = NULL
    e  run flags (saturation of the trunk and of h1', a NaN operand) and the independence of rows
    f  what the entry refuses
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from human_dynamics_amd import _lib as L
from test_gpu_f16x3 import _split_round_w

pytestmark = pytest.mark.gpu

SHAPES = {"b3": (256, 1024, 256, 0), "b2": (128, 512, 128, 0), "b2f": (128, 512, 128, 256)}      # c_mid, depth, n2, c_xp
FORMS = {"b3": ("b3", 0), "b2": ("b2", 0), "b2f": ("b2f", 0), "b3_ws": ("b3", 2), "b2_ws": ("b2", 2)}   # shape, hmmr_debug_t.pair_form
ALL = list(FORMS)
GUARD = 3
NEVER = 2 ** 31 - 1
_filters, _cases = {}, {}


def _gen(name):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(name.encode()))


def _filter_set(shape, dev):
    """W / sqrt(K), scales in [0.5, 1.5] -- and the filter stream, packed ONCE per shape (host work)"""
    if shape not in _filters:
        from human_dynamics_amd import packing
        cm, depth, n2, cxp = SHAPES[shape]
        g = _gen("filters/" + shape)
        rnd = lambda *s: torch.randn(*s, generator=g)
        K3 = cm + cxp
        f = {"W3": (rnd(depth, K3) / K3 ** 0.5).numpy(), "W1": (rnd(n2, depth) / depth ** 0.5).numpy(), "b3": rnd(depth).numpy(),
             "pre": ((torch.rand(depth, generator=g) + 0.5).numpy(), (rnd(depth) * 0.3).numpy()),
             "bn1": ((torch.rand(n2, generator=g) + 0.5).numpy(), (rnd(n2) * 0.3).numpy())}
        f["stream"] = packing.pack_pair_stream(f["W3"], f["W1"]).to(dev)
        _filters[shape] = f
    return _filters[shape]


def _rows(shape, m, name):
    """ReLU'd normal h2 / xp, normal res: float32 host tensors"""
    cm, depth, n2, cxp = SHAPES[shape]
    g = _gen("%s/%d/%s" % (shape, m, name))
    rnd = lambda *s: torch.randn(*s, generator=g)
    return {"h2": rnd(m, cm).clamp_(min=0), "xp": rnd(m, cxp).clamp_(min=0) if cxp else None, "res": None if cxp else rnd(m, depth)}


def _flags():
    """read and clear hmmr_run_flags"""
    fl = C.c_uint(0)
    L.check(L.load().hmmr_run_flags(C.byref(fl), 1), "hmmr_run_flags")
    return fl.value


def _launch(shape, rows, dev, two_launches=False, relu1=True, bias=True, res_ld=0, bn1=None, stream=None):
    from human_dynamics_amd import engine as E
    from human_dynamics_amd import packing
    f = _filter_set(shape, dev)
    cm = SHAPES[shape][0]
    up = lambda x: None if x is None else (x if x.is_cuda else packing.to_split(x.to(dev)))
    return E.unit_pair(up(rows["h2"]), f["W3"][:, :cm], f["b3"] if bias else None, f["pre"], f["W1"], bn1 or f["bn1"], res=up(rows["res"]),
                       shortcut=None if rows["xp"] is None else (up(rows["xp"]), f["W3"][:, cm:]), relu1=relu1, res_ld=res_ld,
                       guard_rows=GUARD, stream=None if two_launches else (stream if stream is not None else f["stream"]),
                       two_launches=two_launches, device=dev)


def _pair(form, rows, dev, two_tile_min=0, **kw):
    """the unit pair in `form` under the given debug switches; the launch counter proves which kernel ran; the flags it raised"""
    from human_dynamics_amd import engine as E
    shape, pair_form = FORMS[form]
    try:
        E.set_debug(pair_form=pair_form, pair_two_tile_min=two_tile_min)
        _flags()
        L.launch_counts(clear=True)
        trunk, h1 = _launch(shape, rows, dev, **kw)
        assert L.launch_counts(clear=True)["unit_pair"] == 1
    finally:
        E.set_debug()
    return trunk, h1, _flags()


def _two(shape, rows, dev, **kw):
    """the two hmmr_conv_gemm launches the pair replaces, on the same operands"""
    _flags()
    L.launch_counts(clear=True)
    trunk, h1 = _launch(shape, rows, dev, two_launches=True, **kw)
    assert L.launch_counts(clear=True)["unit_pair"] == 0
    return trunk, h1, _flags()


def _case(shape, m, dev, name="", **kw):
    """operands (uploaded once) and their two-launch reference, shared by the forms of a shape and left unchanged"""
    key = (shape, m, name, tuple(sorted((k, v) for k, v in kw.items() if k != "bn1")))
    if key not in _cases:
        from human_dynamics_amd import packing
        rows = {k: None if v is None else packing.to_split(v.to(dev)) for k, v in _rows(shape, m, name).items()}
        _cases[key] = (rows, _two(shape, rows, dev, **kw))
    return _cases[key]


def _same(got, want, m, what):
    """outputs equal bit for bit, guard rows (still the sentinel in both) included"""
    from human_dynamics_amd import engine as E
    from human_dynamics_amd import packing
    for name, a, b in (("trunk", got[0], want[0]), ("h1'", got[1], want[1])):
        assert a.shape == b.shape and a.shape[0] == m + GUARD
        assert bool((a[m:] == E.PAIR_SENTINEL).all()) and bool((b[m:] == E.PAIR_SENTINEL).all()), "%s %s: a store past row %d" % (what, name, m)
        if not torch.equal(a, b):
            bad = torch.unique((a != b).nonzero()[:, 0])
            raise AssertionError("%s %s: %d rows differ (first %s), max |diff| %.3e" % (
                what, name, bad.numel(), bad[:8].tolist(), float((packing.from_split(a[:m]) - packing.from_split(b[:m])).abs().max())))


def _float64(shape, rows, got, m, relu1, what):
    """trunk = h2 @ W3^T [+ xp @ Wsc^T] + b3 [+ res] on the rows as stored and the filters as the packer rounds them; h1' from the trunk
    the kernel STORED (the chain rounds the trunk and the pre-activation to 22 bits; the reference leaves the pre-activation unrounded).
    Bound: 2e-5 max(1, max |ref|), that of every split kernel's test."""
    from human_dynamics_amd import packing
    f = _filters[shape]
    cm = SHAPES[shape][0]
    st = lambda t: packing.from_split(t[:m]).double().cpu().numpy()
    W3 = _split_round_w(f["W3"].T[None, None])[0, 0].astype(np.float64)             # [K3][depth]
    W1 = _split_round_w(f["W1"].T[None, None])[0, 0].astype(np.float64)             # [depth][n2]
    ref_t = st(rows["h2"]) @ W3[:cm] + f["b3"].astype(np.float64)
    ref_t += st(rows["xp"]) @ W3[cm:] if rows["xp"] is not None else st(rows["res"])
    trunk, h1 = st(got[0]), st(got[1])
    pre = np.maximum(trunk * f["pre"][0].astype(np.float64) + f["pre"][1].astype(np.float64), 0)
    ref_h = pre @ W1 * f["bn1"][0].astype(np.float64) + f["bn1"][1].astype(np.float64)
    if relu1:
        ref_h = np.maximum(ref_h, 0)
    assert np.abs(ref_t).max() > 0.1 and np.abs(ref_h).max() > 0.1
    et, eh = np.abs(trunk - ref_t).max(), np.abs(h1 - ref_h).max()
    print("%s: trunk max |err| %.3e (max |ref| %.3e)   h1' max |err| %.3e (max |ref| %.3e)" % (what, et, np.abs(ref_t).max(), eh, np.abs(ref_h).max()))
    assert et < 2e-5 * max(1.0, np.abs(ref_t).max()), (what, "trunk", et)
    assert eh < 2e-5 * max(1.0, np.abs(ref_h).max()), (what, "h1'", eh)
    return ref_h


# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("m", [1, 31, 32, 33, 127, 128, 129, 255, 300])
@pytest.mark.parametrize("form", ALL)
def test_unit_pair_ragged_rows_equal_the_two_launches(form, m, gpu_device):
    """One tile per workgroup (the default switches).  m = 1: one tile of one row; 33 / 129: a wave with a single valid row; 32 / 128: on the
    wave's / the tile's boundary; the rest odd.  Rows beyond M read row 0 (the NaN guard rows never reach a maximum: flags 0) and store
    to the dump page (the guard rows keep the sentinel)."""
    shape = FORMS[form][0]
    rows, want = _case(shape, m, gpu_device)
    assert want[2] == 0
    got = _pair(form, rows, gpu_device)
    _same(got, want, m, "%s m=%d" % (form, m))
    assert got[2] == 0, got[2]
    again = _pair(form, rows, gpu_device)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and again[2] == 0


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("form", ALL)
def test_unit_pair_against_float64(form, gpu_device):
    """M = 300.  Measured on an MI355X (profiles/unit_pair_sweep.log): trunk max |err| 1.5e-6 (b3), 1.3e-6 (b2), 1.4e-6 (b2f) with max |ref|
    5-8; h1' 3.4e-6, 3.0e-6, 2.6e-6 with max |ref| 4-6; the wave-specialised forms give their one-wave forms' bits.  Bound: 1.0-1.6e-4."""
    shape = FORMS[form][0]
    rows, want = _case(shape, 300, gpu_device)
    got = _pair(form, rows, gpu_device)
    _same(got, want, 300, form)
    _float64(shape, rows, got, 300, True, form)


# ------------------------------------------------------------------------------------------------------------------ c
def _tiles_to_rows(case, cus):
    return {"1": 100, "2": 200, "3": 300, "cus+1": 128 * cus + 5, "2cus": 256 * cus, "2cus+1": 256 * cus + 1}[case]


@pytest.mark.parametrize("case", ["1", "2", "3", "cus+1", "2cus", "2cus+1"])
@pytest.mark.parametrize("form", ["b2", "b2f"])
def test_unit_pair_persistent_tiles(form, case, gpu_device):
    """pair_two_tile_min = 1: 1 tile; 2 tiles = one workgroup, two tiles; 3 = the last workgroup has one; CUs + 1 = every workgroup but
    one breaks out of its second round; 2 CUs = two full tiles each; 2 CUs + 1 = three tiles per workgroup, one row in the third round.
    Forced persistent, forced off and the two launches: the same bits (the large cases are checked against the two launches only).
    The launch counter proves that the pair kernel ran; grid and tiles per workgroup are NOT observed: they follow from
    pair_two_tile_min and the tile count as launch_pair (csrc/unit_pair.hip) computes them."""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    m = _tiles_to_rows(case, cus)
    shape = FORMS[form][0]
    from human_dynamics_amd import packing
    rows = {k: None if v is None else packing.to_split(v.to(gpu_device)) for k, v in _rows(shape, m, "tiles").items()}
    want = _two(shape, rows, gpu_device)
    assert want[2] == 0
    for label, two_min in (("persistent", 1), ("one tile per workgroup", NEVER)):
        got = _pair(form, rows, gpu_device, two_tile_min=two_min)
        _same(got, want, m, "%s %s tiles, %s" % (form, case, label))
        assert got[2] == 0, (label, got[2])


@pytest.mark.parametrize("form", ["b2", "b2f"])
def test_unit_pair_three_tiles_per_workgroup_at_the_default_switch(form, gpu_device):
    """2 CUs + 1 tiles with the default switches: the tpw = 3 geometry production takes from 513 tiles on"""
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    if 2 * cus + 1 < 512:
        pytest.skip("%d CUs: 2 CUs + 1 tiles stay below the default switch of 512 tiles" % cus)
    m = 256 * cus + 1
    shape = FORMS[form][0]
    from human_dynamics_amd import packing
    rows = {k: None if v is None else packing.to_split(v.to(gpu_device)) for k, v in _rows(shape, m, "tiles").items()}
    want = _two(shape, rows, gpu_device)
    got = _pair(form, rows, gpu_device)
    _same(got, want, m, "%s default switches" % form)
    assert got[2] == 0 and want[2] == 0


# ------------------------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("form", ["b3", "b2", "b3_ws", "b2_ws"])
def test_unit_pair_shortcut_row_stride_above_depth(form, gpu_device):
    """ldr = depth + 32: the shortcut is a view into a wider buffer whose other columns are NaN"""
    shape = FORMS[form][0]
    rows, want = _case(shape, 200, gpu_device)
    got = _pair(form, rows, gpu_device, res_ld=SHAPES[shape][1] + 32)
    _same(got, want, 200, form)
    assert got[2] == 0, got[2]


@pytest.mark.parametrize("form", ALL)
def test_unit_pair_without_relu1(form, gpu_device):
    """relu1 = 0: h1' is clamped at -65504 instead of 0"""
    shape = FORMS[form][0]
    rows, want = _case(shape, 200, gpu_device, relu1=False)
    got = _pair(form, rows, gpu_device, relu1=False)
    _same(got, want, 200, form)
    assert got[2] == 0, got[2]
    ref_h = _float64(shape, rows, got, 200, False, form + " relu1=0")
    from human_dynamics_amd import packing
    assert ref_h.min() < -0.1 and float(packing.from_split(got[1][:200]).min()) < -0.1


@pytest.mark.parametrize("form", ALL)
def test_unit_pair_without_bias3(form, gpu_device):
    """shift3 = NULL: the kernel's c_b3 = 0 branch"""
    shape = FORMS[form][0]
    rows, want = _case(shape, 200, gpu_device, bias=False)
    got = _pair(form, rows, gpu_device, bias=False)
    _same(got, want, 200, form)
    assert got[2] == 0, got[2]
    _, with_bias = _case(shape, 200, gpu_device)
    assert not torch.equal(with_bias[0], want[0])


# ------------------------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("form", ["b2", "b3_ws", "b2f"])
def test_unit_pair_run_flags_and_row_independence(form, gpu_device):
    from human_dynamics_amd import packing
    shape = FORMS[form][0]
    dev, m = gpu_device, 200
    f = _filter_set(shape, dev)
    rows, want = _case(shape, m, dev)
    clean = _pair(form, rows, dev)
    assert clean[2] == 0 and want[2] == 0
    _same(clean, want, m, form)
    val = lambda t: packing.from_split(t[:m])
    # the trunk saturates: conv3's operands x 3e4 (kept inside the fp16 range themselves): a trunk value is ~N(0, 2e4), 65504 is 3 sigma
    host = _rows(shape, m, "")
    big = dict(host, h2=(host["h2"] * 3e4).clamp_(max=6e4), xp=None if host["xp"] is None else (host["xp"] * 3e4).clamp_(max=6e4))
    big = {k: None if v is None else packing.to_split(v.to(dev)) for k, v in big.items()}
    w_big, g_big = _two(shape, big, dev), _pair(form, big, dev)
    assert g_big[2] == L.FLAG_SATURATED and w_big[2] == L.FLAG_SATURATED, (g_big[2], w_big[2])
    assert float(val(g_big[0]).abs().max()) == 65504.0
    _same(g_big, w_big, m, form + " saturated trunk")
    # h1' saturates: scale1 = 1e6 on a normal trunk
    bn1 = (np.full_like(f["bn1"][0], 1e6), f["bn1"][1])
    w_s1, g_s1 = _two(shape, rows, dev, bn1=bn1), _pair(form, rows, dev, bn1=bn1)
    assert g_s1[2] == L.FLAG_SATURATED and w_s1[2] == L.FLAG_SATURATED, (g_s1[2], w_s1[2])
    assert float(val(g_s1[1]).abs().max()) == 65504.0 and float(val(g_s1[0]).abs().max()) < 100
    _same(g_s1, w_s1, m, form + " saturated h1'")
    assert torch.equal(g_s1[0], clean[0])
    # one NaN in row 37 of conv3's operand: the flag says so, and no other row notices
    key = "xp" if shape == "b2f" else "h2"
    bad = dict(host)
    bad[key] = host[key].clone()
    bad[key][37, 5] = float("nan")
    bad = {k: None if v is None else packing.to_split(v.to(dev)) for k, v in bad.items()}
    w_nan, g_nan = _two(shape, bad, dev), _pair(form, bad, dev)
    assert g_nan[2] == (L.FLAG_NAN | L.FLAG_SATURATED) and w_nan[2] == (L.FLAG_NAN | L.FLAG_SATURATED), (g_nan[2], w_nan[2])
    others = [r for r in range(m + GUARD) if r != 37]
    for k in range(2):
        assert torch.equal(g_nan[k][others], clean[k][others]), "the NaN of row 37 reached another row of output %d" % k
        r37 = val(g_nan[k])[37]
        assert bool(torch.isfinite(r37).all()) and float(r37.abs().max()) <= 65504.0
        assert torch.equal(g_nan[k][37], w_nan[k][37]), "row 37 of output %d differs from the two launches'" % k
    # (every _pair / _two call above read AND cleared the flags) a clean run after all that raises nothing and gives the clean bits
    again = _pair(form, rows, dev)
    assert again[2] == 0 and torch.equal(again[0], clean[0]) and torch.equal(again[1], clean[1])


# ------------------------------------------------------------------------------------------------------------------ f
def test_unit_pair_refuses_what_it_is_not_built_for(gpu_device):
    from human_dynamics_amd import engine as E
    from human_dynamics_amd import packing
    dev, m = gpu_device, 200
    f = _filter_set("b2", dev)
    host = _rows("b2", m, "")
    xp = _rows("b2f", m, "")["xp"]
    mk = lambda **kw: E.UnitPairCall(host["h2"], f["W3"], f["b3"], f["pre"], f["W1"], f["bn1"], res=host["res"], stream=f["stream"], device=dev, **kw)

    def refused(call, match):
        with pytest.raises(L.HmmrError, match=match):
            call.run()
        torch.cuda.synchronize()

    c = mk()
    c.descs[0].m = 0
    refused(c, "needs h2")
    c = mk()
    xps = packing.to_split(xp.to(dev))
    c.descs[0].xp, c.descs[0].c_xp = xps.data_ptr(), 256
    refused(c, "either a shortcut tensor")
    c = mk()
    c.descs[0].res = None
    refused(c, "null argument")
    c = mk()
    c.descs[0].ldr = 512 - 8
    refused(c, "residual row stride < depth")
    c = mk()
    c.descs[0].out_h1 = None
    refused(c, "needs h2")
    g = _gen("refusals")
    rnd = lambda *s: torch.randn(*s, generator=g)
    small = E.UnitPairCall(rnd(m, 64), rnd(256, 64).numpy(), f["b3"][:256], (f["pre"][0][:256], f["pre"][1][:256]), rnd(64, 256).numpy(),
                           (f["bn1"][0][:64], f["bn1"][1][:64]), res=rnd(m, 256), device=dev)
    refused(small, "supported shapes")
    narrow = E.UnitPairCall(host["h2"], f["W3"], f["b3"], f["pre"], f["W1"], f["bn1"], shortcut=(xp[:, :128].contiguous(), rnd(512, 128).numpy()),
                            device=dev)
    refused(narrow, "supported shapes")
    # pair_form = 2 has no folded form: the folded one-wave kernel runs, with the same bits
    rows, want = _case("b2f", m, dev)
    try:
        E.set_debug(pair_form=2)
        L.launch_counts(clear=True)
        got = _launch("b2f", rows, dev)
        assert L.launch_counts(clear=True)["unit_pair"] == 1
    finally:
        E.set_debug()
    _same(got, want, m, "b2f under pair_form = 2")
    assert _flags() == 0
