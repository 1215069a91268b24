"""The C-ABI library builds for gfx950, loads, and exports every symbol
include/hmmr_hip.h declares (no compute calls: there is no GPU here)."""
import os
import re

import pytest

from human_dynamics_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "hmmr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hmmr_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_every_declared_symbol():
    build.build(verbose=False)
    lib = _lib.load()
    names = _declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), "libhmmr_hip.so does not export %s" % n
    assert sorted(_lib.SIGNATURES) == names        # the ctypes table covers the header one to one
    assert lib.hmmr_abi_version() == _lib.ABI_VERSION == 19


def test_workspace_queries_need_no_gpu():
    lib = _lib.load()
    assert lib.hmmr_resnet50_workspace_bytes(0, _lib.HMMR_BF16) == 0
    b16 = lib.hmmr_resnet50_workspace_bytes(64, _lib.HMMR_BF16)
    f32 = lib.hmmr_resnet50_workspace_bytes(64, _lib.HMMR_F32)
    assert 0 < b16 < f32 <= 2 * b16 + 4096
    assert lib.hmmr_smpl_workspace_bytes(256) >= 256 * (224 + 288) * 4
    assert lib.hmmr_temporal_workspace_bytes(8, 20, _lib.HMMR_F32) >= 4 * 160 * 2048 * 4
    assert lib.hmmr_ief_workspace_bytes(160, 3, _lib.HMMR_F32) > 0
    # split (f16x3) tensors are 4 bytes per element, like fp32
    assert lib.hmmr_resnet50_workspace_bytes(64, _lib.HMMR_F16X3) == f32


def test_debug_switches_round_trip():
    import ctypes as C
    lib = _lib.load()
    d = _lib.Debug()
    lib.hmmr_get_debug(C.byref(d))
    assert (d.stem_route, d.stem_no_conv1) == (0, 0)          # product defaults
    d.stem_route, d.stem_no_conv1 = 1, 1
    lib.hmmr_set_debug(C.byref(d))
    e = _lib.Debug()
    lib.hmmr_get_debug(C.byref(e))
    assert (e.stem_route, e.stem_no_conv1) == (1, 1)
    lib.hmmr_set_debug(None)
    lib.hmmr_get_debug(C.byref(e))
    assert (e.stem_route, e.stem_no_conv1) == (0, 0)


def test_argument_validation_reports_errors():
    lib = _lib.load()
    d = _lib.ConvDesc()
    rc = lib.hmmr_conv_gemm(d, None)
    assert rc != 0 and b"null operand" in lib.hmmr_last_error()
    with pytest.raises(_lib.HmmrError):
        _lib.check(rc, "hmmr_conv_gemm")


def test_periphery_argument_validation_reports_errors():
    """The entry points around the path (crop, hand-off, metrics) refuse what their kernels could not honour before
    anything is launched -- dummy, never dereferenced pointers; no device is needed -- and leave a message."""
    lib = _lib.load()
    P = [0x1000 * (i + 1) for i in range(8)]

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc != 0 and msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        with pytest.raises(_lib.HmmrError):
            _lib.check(rc, "periphery")

    def call(fn, names, defaults, kw):
        args = dict(defaults)
        args.update(kw)
        return fn(*[args[a] for a in names.split()])

    joints = lambda **kw: call(lib.hmmr_eval_joints, "gt pred n k l r mp pa ac ae st",
                               dict(gt=P[0], pred=P[1], n=4, k=14, l=3, r=2, mp=P[2], pa=P[3], ac=None, ae=None, st=None), kw)
    refused(joints(k=33), b"hmmr_eval_joints", b"k <= 32")                   # one past the per-lane array
    refused(joints(k=0), b"hmmr_eval_joints")
    refused(joints(n=0), b"hmmr_eval_joints")
    for l, r in ((14, 2), (3, 14), (-1, 2), (3, -1)):
        refused(joints(l=l, r=r), b"hmmr_eval_joints", b"hip ids")
    refused(joints(k=2), b"hip ids")                                         # the LSP hips (3, 2) do not exist with 2 joints
    refused(joints(pa=None), b"hmmr_eval_joints", b"both outputs")
    refused(joints(mp=None), b"both outputs")
    refused(joints(gt=None), b"needs gt")
    refused(joints(pred=None), b"hmmr_eval_joints")

    handoff = lambda **kw: call(lib.hmmr_render_handoff, "cams ldc verts ldv kps ldk geom n nv nk cam proj kp st",
                                dict(cams=P[0], ldc=3, verts=P[1], ldv=3 * 50, kps=P[2], ldk=50, geom=None, n=2, nv=50, nk=25,
                                     cam=P[3], proj=P[4], kp=P[5], st=None), kw)
    refused(handoff(ldv=3 * 50 - 1), b"hmmr_render_handoff", b"row strides")
    refused(handoff(ldc=2), b"row strides")
    refused(handoff(ldk=49), b"row strides")
    refused(handoff(kps=None), b"hmmr_render_handoff", b"kp_orig requested without kps")
    refused(handoff(n=0), b"hmmr_render_handoff")
    refused(handoff(nv=0), b"hmmr_render_handoff")
    refused(handoff(nk=-1), b"hmmr_render_handoff")
    refused(handoff(proj=None), b"hmmr_render_handoff")

    crop = lambda **kw: call(lib.hmmr_crop_frames, "fr geom n h w out st",
                             dict(fr=P[0], geom=P[1], n=1, h=96, w=128, out=P[2], st=None), kw)
    refused(crop(n=0), b"hmmr_crop_frames")
    refused(crop(h=0), b"hmmr_crop_frames")
    refused(crop(geom=None), b"hmmr_crop_frames")
    refused(crop(out=None), b"hmmr_crop_frames")

    verts = lambda **kw: call(lib.hmmr_eval_verts, "gt ldg pred ldp n nv err st",
                              dict(gt=P[0], ldg=150, pred=P[1], ldp=150, n=2, nv=50, err=P[2], st=None), kw)
    refused(verts(nv=0), b"hmmr_eval_verts")
    refused(verts(n=0), b"hmmr_eval_verts")
    refused(verts(err=None), b"hmmr_eval_verts")


def _dense_1x1(m=256, cin=64, cout=256, dtype=_lib.HMMR_F16X3):
    """a syntactically valid 1x1 descriptor with dummy (never dereferenced) pointers: validation runs before any launch"""
    d = _lib.ConvDesc()
    d.in_, d.w, d.out = 0x1000, 0x2000, 0x3000
    d.in_dtype = d.out_dtype = dtype
    d.n_img, d.hin, d.win, d.cin = 1, m, 1, cin
    d.in_img_stride, d.in_row_stride, d.in_px_stride = m * cin, cin, cin
    d.kh = d.kw = d.sy = d.sx = 1
    d.ho, d.wo, d.cout, d.ldo = m, 1, cout, cout
    return d


def test_conv_desc_validation_of_the_round_2_fields():
    """hmmr_conv_desc_t.in2 (a second operand source appended along K) and the 128x256 tile are refused with a message
    where the kernel could not honour them -- before anything is launched, so this runs without a GPU."""
    lib = _lib.load()
    d = _dense_1x1()
    d.in2, d.cin2 = 0x4000, 48                       # not a multiple of the 128-byte K step (32 split elements)
    assert lib.hmmr_conv_gemm(d, None) != 0 and b"multiple of 32" in lib.hmmr_last_error()
    d = _dense_1x1()
    d.in2, d.cin2, d.sy, d.sx, d.ho = 0x4000, 64, 2, 2, 128       # strided: the two sources would not share a pixel grid
    assert lib.hmmr_conv_gemm(d, None) != 0 and b"second operand source" in lib.hmmr_last_error()
    d = _dense_1x1()
    d.in2, d.cin2 = 0x4000, 64
    d.pro_scale = d.pro_shift = 0x5000               # the fused pre-activation takes the register route: no second source there
    assert lib.hmmr_conv_gemm(d, None) != 0
    d = _dense_1x1(cout=128)
    d.tile = 8
    assert lib.hmmr_conv_gemm(d, None) != 0 and b"tile 8" in lib.hmmr_last_error()
    t = _lib.TailDesc()
    t.dtype, t.h2, t.w3, t.res, t.m, t.c_mid, t.depth, t.n2 = _lib.HMMR_F16X3, 0x1000, 0x2000, 0x3000, 64, 256, 1024, 256
    t.w1 = t.out = t.out_h1 = t.pre_scale = t.pre_shift = t.scale1 = t.shift1 = 0x4000
    t.ldr = 1024
    assert lib.hmmr_bottleneck_tail(t, None) != 0 and b"supported shapes" in lib.hmmr_last_error()


def test_b1_unit_entry_refuses_with_its_messages():
    """hmmr_bottleneck_tail with unit_stream set (csrc/b1_unit.hip): every check of hmmr_b1_unit_split, each with its message, on dummy
    pointers -- the checks run in front of the launch.  That a refused call queues nothing: tests/test_gpu_b1_unit_kernel.py."""
    import b1_unit_cases as B
    lib = _lib.load()

    def good(form):
        t = _lib.TailDesc()
        t.dtype, t.m, t.c_mid, t.depth, t.n2 = _lib.HMMR_F16X3, 6 * 5 * 7, 64, 256, 64
        t.h1, t.hin, t.win, t.ho, t.wo, t.unit_stream = 0x1000, 5, 7, 5, 7, 0x2000
        t.scale2 = t.shift2 = t.scale3 = t.shift3 = t.pre_scale = t.pre_shift = t.scale1 = t.shift1 = 0x3000
        t.out, t.out_h1, t.relu1 = 0x4000, 0x5000, 1
        if form == "folded":
            t.xp, t.c_xp = 0x6000, 64
        else:
            t.res, t.ldr = 0x6000, 256
        return t

    assert len(B.REFUSALS) >= 21 and len({r[0] for r in B.REFUSALS}) == len(B.REFUSALS)
    for name, form, fields, words in B.REFUSALS:
        t = good(form)
        B.apply_refusal(t, fields, 0x7000)
        rc, msg = lib.hmmr_bottleneck_tail(t, None), lib.hmmr_last_error()
        assert rc != 0 and words.encode() in msg, (name, rc, msg)
        assert b"hmmr_bottleneck_tail" in msg
        with pytest.raises(_lib.HmmrError, match=words):
            _lib.check(rc, name)


def test_fragment_major_packing_layout():
    """packing.pack_frag_major: [n][K] -> [n / 32][K / 16][64 lanes][hi, lo][8]; lane = 32 * (k half) + row, i.e. the 16 bytes a
    lane feeds v_mfma_f32_32x32x16_f16 as its A operand (csrc/bottleneck_split.hip reads them straight from L2); fp16 halves
    of the rows scaled by packing.row_pow2."""
    import numpy as np
    import torch
    from human_dynamics_amd import packing
    rng = np.random.default_rng(0)
    w = rng.normal(size=(64, 48)).astype(np.float32)
    f = packing.pack_frag_major(w)
    assert tuple(f.shape) == (2, 3, 64, 2, 8) and f.dtype == torch.float16
    k = packing.row_pow2(w)
    ws = torch.from_numpy(packing.scale_rows(w, k))
    assert float(ws.abs().max()) < 2.0 ** 14 and float(ws.abs().max(dim=1).values.min()) >= 2.0 ** 13
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    for rb, kc, lane in ((0, 0, 0), (1, 2, 63), (0, 1, 37), (1, 0, 31)):
        row, half = rb * 32 + lane % 32, lane // 32
        k0 = kc * 16 + 8 * half
        assert torch.equal(f[rb, kc, lane, 0], hi[row, k0:k0 + 8]) and torch.equal(f[rb, kc, lane, 1], lo[row, k0:k0 + 8])
    back = (f[:, :, :, 0].float() + f[:, :, :, 1].float()).reshape(2, 3, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(64, 48)
    unscaled = back.double() / torch.from_numpy(np.exp2(k.astype(np.float64)))[:, None]
    assert float(((unscaled - torch.from_numpy(w).double()).abs() / torch.from_numpy(w).double().abs()).max()) < 2.0 ** -20


def test_engine_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from human_dynamics_amd.engine import HmmrEngine
    with pytest.raises(_lib.HmmrError):
        HmmrEngine(None, None)


def test_integration_doc_stub_matches_the_struct():
    """INTEGRATION.md shows a ctypes stub of hmmr_smpl_consts_t for a maintainer to paste: its fields are the
    library's, in order (the doc had drifted once, when `vpad` was added)."""
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "INTEGRATION.md")).read()
    block = txt[txt.index("class SmplConsts(C.Structure)"):]
    block = block[:block.index("def smpl_forward")]
    doc_fields = re.findall(r"\('(\w+)',\s*C\.(\w+)\)", block)
    lib_fields = [(n, "c_int" if t is C.c_int else "c_void_p") for n, t in _lib.SmplConsts._fields_]
    assert doc_fields == lib_fields


def _stem_table(dtype, conv1_frag=True):
    """a table whose stem and block1/unit_1 hold dummy (never dereferenced) pointers: every check runs before anything is queued"""
    rw = _lib.ResnetWeights()
    rw.dtype = dtype
    rw.stem.w, rw.stem.shift = 0x1000, 0x2000
    if dtype == _lib.HMMR_F16X3:
        rw.stem.scale = 0x3000                       # the pack-time row scale of the split filters
    u = rw.unit[0]
    u.pre_scale, u.pre_shift = 0x4000, 0x5000
    u.conv1.w, u.conv1.scale, u.conv1.shift = 0x6000, 0x7000, 0x8000
    if dtype == _lib.HMMR_F16X3 and conv1_frag:
        u.conv1_frag = 0x9000
    u.c_in, u.base, u.depth, u.stride = 64, 64, 256, 1
    rw.unit[15].depth = 2048
    return rw


class _stem_switches(object):
    """hmmr_debug_t.stem_route / stem_no_conv1 for the block; every switch is put back as it was found"""

    def __init__(self, lib, route, no_conv1=0):
        self.lib, self.route, self.no_conv1 = lib, route, no_conv1

    def __enter__(self):
        import ctypes as C
        self.old, d = _lib.Debug(), _lib.Debug()
        self.lib.hmmr_get_debug(C.byref(self.old))
        self.lib.hmmr_get_debug(C.byref(d))
        d.stem_route, d.stem_no_conv1 = self.route, self.no_conv1
        self.lib.hmmr_set_debug(C.byref(d))

    def __exit__(self, *exc):
        import ctypes as C
        self.lib.hmmr_set_debug(C.byref(self.old))
        return False


def test_stem_entry_refuses_before_anything_is_queued():
    """hmmr_resnet50_stem: every refusal of include/hmmr_hip.h, with dummy pointers and no device -- a call that got past its checks would
    have to launch.  hmmr_resnet50_fwd refuses a misaligned image pointer and a scaled bf16 / fp32 fused stem as well."""
    import ctypes as C
    lib = _lib.load()
    IMG, OUT, H1, WS = 0x10000, 0x20000, 0x30000, 0x40000
    BIG = 1 << 40

    def stem(rw, images=IMG, n=2, n_zero=1, pooled=OUT, h1=H1, ws=WS, ws_bytes=BIG, route=0, no_conv1=0):
        flag = C.c_int(7)
        with _stem_switches(lib, route, no_conv1):
            rc = lib.hmmr_resnet50_stem(C.byref(rw) if rw is not None else None, images, n, n_zero, pooled, h1, C.byref(flag), ws, ws_bytes, None)
        return rc, flag.value, lib.hmmr_last_error()

    def refused(res, *words):
        rc, flag, msg = res
        assert rc == -1 and flag == 0 and b"hmmr_resnet50_stem" in msg, res
        for w in words:
            assert w in msg, (w, msg)

    for dt in (_lib.HMMR_F32, _lib.HMMR_BF16, _lib.HMMR_F16X3):
        rw = _stem_table(dt)
        for route in (1, 2):
            refused(stem(None, route=route), b"null argument")
            refused(stem(rw, pooled=None, route=route), b"null argument")
            refused(stem(rw, images=None, route=route), b"null argument")            # n = 2 images, no pointer
            refused(stem(rw, n=-1, route=route), b"at least one image")
            refused(stem(rw, n_zero=-1, route=route), b"at least one image")
            refused(stem(rw, n=0, n_zero=0, route=route), b"at least one image")
            refused(stem(rw, n=0, n_zero=0, images=None, route=route), b"at least one image")
            for off in (4, 8, 12, 1):
                refused(stem(rw, images=IMG + off, route=route), b"16-byte aligned")
        # the three-kernel route needs the re-packed image and the conv map; the fused one no workspace at all
        with _stem_switches(lib, 1):
            need = lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), 3)
        with _stem_switches(lib, 2):
            assert lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), 3) == 0
        e = 2 if dt == _lib.HMMR_BF16 else 4
        assert need >= 3 * (230 * 232 * 4 + 112 * 112 * 64) * e and need < lib.hmmr_resnet50_workspace_bytes(3, dt)
        assert lib.hmmr_resnet50_stem_workspace_bytes(C.byref(rw), 0) == 0 and lib.hmmr_resnet50_stem_workspace_bytes(None, 3) == 0
        refused(stem(rw, ws_bytes=need - 1, route=1), b"workspace too small")
        refused(stem(rw, ws=None, route=1), b"workspace too small")
        for part in ("w", "shift"):
            bad = _stem_table(dt)
            setattr(bad.stem, part, None)
            refused(stem(bad, route=1), b"null argument")
            refused(stem(bad, route=2), b"null argument")
        bad = _stem_table(dt)
        bad.unit[0].pre_shift = None
        refused(stem(bad, route=2), b"null argument")
    for bad_dt in (3, -1, 17):
        refused(stem(_stem_table(bad_dt)), b"bad dtype")
    # a scaled bf16 / fp32 stem on the fused route (default route for bf16, forced for fp32); the three-kernel route would apply it
    for dt, routes, word in ((_lib.HMMR_BF16, (0, 2), b"bf16"), (_lib.HMMR_F32, (2,), b"fp32")):
        rw = _stem_table(dt)
        rw.stem.scale = 0x3000
        for route in routes:
            refused(stem(rw, route=route), b"stem.scale", word)

    # hmmr_resnet50_fwd: the same two refusals, before its first launch
    def fwd(rw, images=IMG, route=0):
        with _stem_switches(lib, route):
            return lib.hmmr_resnet50_fwd(C.byref(rw), images, 2, 1, OUT, WS, BIG, None, None), lib.hmmr_last_error()

    for dt in (_lib.HMMR_F32, _lib.HMMR_BF16, _lib.HMMR_F16X3):
        for route in (0, 1, 2):
            rc, msg = fwd(_stem_table(dt), images=IMG + 4, route=route)
            assert rc == -1 and b"hmmr_resnet50_fwd" in msg and b"16-byte aligned" in msg, (rc, msg)
    rw = _stem_table(_lib.HMMR_BF16)
    rw.stem.scale = 0x3000
    rc, msg = fwd(rw)
    assert rc == -1 and b"hmmr_resnet50_fwd" in msg and b"stem.scale" in msg, (rc, msg)
    rc, msg = fwd(_stem_table(5))
    assert rc == -1 and b"bad dtype" in msg, (rc, msg)


def test_smpl_entries_refuse_before_anything_is_queued():
    """hmmr_smpl_fwd / _strided / _records: every refusal of csrc/smpl.hip's launcher, with dummy (never dereferenced) pointers and no
    device -- the valid calls are what tests/test_gpu_smpl.py sweeps."""
    import ctypes as C
    lib = _lib.load()
    P = [0x10000 * (i + 1) for i in range(8)]
    BIG = 1 << 40

    def consts(**kw):
        sc = _lib.SmplConsts()
        sc.num_verts, sc.num_kps, sc.lbs_nnz, sc.vpad = 170, 25, 4, 256
        for name, _ in _lib.SmplConsts._fields_[4:]:
            setattr(sc, name, 0x100000)
        for k, v in kw.items():
            setattr(sc, k, v)
        return sc

    def fwd(sc=None, theta=P[0], beta=P[1], cams=P[2], m=5, verts=P[3], joints=P[4], kps=P[5], rs=P[6], ws=P[7], ws_bytes=BIG, strided=False):
        sc = consts() if sc is None else sc
        head = (C.byref(sc) if sc else None, theta, 72, beta, 10, cams, 3, m, verts, joints, kps, rs)
        if strided:
            return lib.hmmr_smpl_fwd_strided(*head, 1000, ws, ws_bytes, None)
        return lib.hmmr_smpl_fwd(*head, ws, ws_bytes, None)

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc != 0 and msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for strided in (False, True):
        refused(fwd(m=0, strided=strided), b"hmmr_smpl_fwd", b"m must be positive")
        refused(fwd(m=-3, strided=strided), b"m must be positive")
        for bad in (0, -1, 25):
            refused(fwd(consts(lbs_nnz=bad), strided=strided), b"lbs_nnz=%d out of range" % bad)
        refused(fwd(consts(lbs_nnz=24), cams=None, strided=strided), b"kps requested without cams")      # (24 itself is a valid width)
        refused(fwd(cams=None, strided=strided), b"kps requested without cams")
        for vpad in (0, 128, 170, 250, 257, 320):            # below the vertex count rounded up to 128, or no multiple of 128
            refused(fwd(consts(vpad=vpad), strided=strided), b"vpad=%d" % vpad, b"num_verts=170")
        need = lib.hmmr_smpl_workspace_bytes(5)
        assert need == lib.hmmr_smpl_workspace_bytes(32) > 0 and lib.hmmr_smpl_workspace_bytes(33) == lib.hmmr_smpl_workspace_bytes(64) > need
        assert lib.hmmr_smpl_workspace_bytes(0) == 0 and lib.hmmr_smpl_workspace_bytes(-1) == 0
        refused(fwd(ws_bytes=need - 1, strided=strided), b"workspace too small")
        for missing in ("theta", "beta", "verts", "joints", "ws"):
            refused(fwd(strided=strided, **{missing: None}), b"null argument")
    refused(lib.hmmr_smpl_fwd(None, P[0], 72, P[1], 10, P[2], 3, 5, P[3], P[4], P[5], P[6], P[7], BIG, None), b"null argument")

    def records(sc=None, om=P[0], R=3, n=21, rec=P[1], ld=2000, offs=None, ws=P[7]):
        sc = consts() if sc is None else sc
        offs = [90 * i for i in range(7 * max(R, 1))] if offs is None else offs
        arr = (C.c_int32 * len(offs))(*offs)
        return lib.hmmr_smpl_fwd_records(C.byref(sc), om, R, n, rec, ld, arr, ws, BIG, None)

    refused(records(R=0), b"hmmr_smpl_fwd_records", b"bad container count")
    refused(records(R=9, ld=1 << 20), b"bad container count")
    refused(records(n=0), b"bad container count")
    refused(records(om=None), b"null argument")
    refused(records(rec=None), b"null argument")
    for bad in (-1, 2000, 2001):
        offs = [90 * i for i in range(21)]
        offs[9] = bad
        refused(records(offs=offs), b"field offset outside the record")
    refused(records(sc=consts(vpad=320)), b"vpad=320")
    refused(records(sc=consts(lbs_nnz=25)), b"lbs_nnz=25")


def test_tail_entries_refuse_before_anything_is_queued():
    """hmmr_groupnorm_relu, hmmr_temporal_fwd, hmmr_hallucinator_fwd, hmmr_ief_fwd_from: every refusal, with dummy (never dereferenced)
    pointers and no device -- each is a -1 with a message, the status of a check in front of the first launch (a call that got past
    its checks would have to launch; a failed launch is -2).  The valid calls are what tests/test_gpu_tail.py sweeps."""
    import ctypes as C
    lib = _lib.load()
    P = [0x10000 * (i + 1) for i in range(8)]
    BIG = 1 << 40
    DTYPES = (_lib.HMMR_F32, _lib.HMMR_BF16, _lib.HMMR_F16X3)

    def refused(rc, *words):
        msg = lib.hmmr_last_error()
        assert rc == -1 and msg, (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    def gn(x=P[0], gamma=P[1], beta=P[2], b=2, t=7, c=2048, groups=32, out=P[3], dt=_lib.HMMR_F32):
        return lib.hmmr_groupnorm_relu(x, gamma, beta, b, t, c, groups, out, dt, None)

    for missing in ("x", "gamma", "beta", "out"):
        refused(gn(**{missing: None}), b"hmmr_groupnorm_relu", b"null argument")
    for kw in (dict(b=0), dict(b=-1), dict(t=0), dict(t=-2), dict(groups=0), dict(groups=-4)):
        refused(gn(**kw), b"hmmr_groupnorm_relu", b"bad shape")
    for c, groups in ((2048, 31), (128, 32), (2048, 512), (2052, 513), (96, 8), (100, 10)):      # no whole groups, or 4 / 12 / 10 channels each
        refused(gn(c=c, groups=groups), b"multiple of 8")
    for dt in (3, -1):
        refused(gn(dt=dt), b"bad dtype")

    def temporal(dt=_lib.HMMR_F32, blocks=3, w=True, phi=P[0], b=2, t=7, strips=P[1], ws=P[2], ws_bytes=BIG):
        tw = _lib.TemporalWeights()
        tw.dtype, tw.num_blocks = dt, blocks
        return lib.hmmr_temporal_fwd(C.byref(tw) if w else None, phi, b, t, strips, ws, ws_bytes, None)

    def hal(dt=_lib.HMMR_F32, w=True, phi=P[0], m=5, out=P[1], ws=P[2], ws_bytes=BIG):
        hw = _lib.HallucinatorWeights()
        hw.dtype = dt
        return lib.hmmr_hallucinator_fwd(C.byref(hw) if w else None, phi, m, out, ws, ws_bytes, None)

    def ief(dt=_lib.HMMR_F32, R=3, nd=(85, 72, 72, 72, 72, 72, 72, 72), no_optcam=0, w=True, strips=P[0], start=None, m=5, omegas=P[1],
            ws=P[2], ws_bytes=BIG):
        iw = _lib.IefWeights()
        iw.dtype, iw.num_regressors, iw.num_stages, iw.no_optcam, iw.mean_theta = dt, R, 3, no_optcam, P[3]
        for r in range(_lib.MAX_REGRESSORS):
            iw.reg[r].nd = nd[r]
        return lib.hmmr_ief_fwd_from(C.byref(iw) if w else None, strips, start, m, omegas, ws, ws_bytes, None)

    for dt in DTYPES:
        refused(temporal(dt, w=False), b"hmmr_temporal_fwd", b"null argument")
        for missing in ("phi", "strips", "ws"):
            refused(temporal(dt, **{missing: None}), b"hmmr_temporal_fwd", b"null argument")
        for kw in (dict(b=0), dict(b=-1), dict(t=0), dict(t=-1)):
            refused(temporal(dt, **kw), b"hmmr_temporal_fwd", b"bad shape")
        for blocks in (0, -1, _lib.MAX_TEMPORAL_BLOCKS + 1):
            refused(temporal(dt, blocks=blocks), b"bad num_blocks")
        refused(temporal(dt, ws_bytes=lib.hmmr_temporal_workspace_bytes(2, 7, dt) - 1), b"workspace too small")

        refused(hal(dt, w=False), b"hmmr_hallucinator_fwd", b"null argument")
        for missing in ("phi", "out", "ws"):
            refused(hal(dt, **{missing: None}), b"hmmr_hallucinator_fwd", b"null argument")
        for m in (0, -1):
            refused(hal(dt, m=m), b"m must be positive")
        refused(hal(dt, ws_bytes=lib.hmmr_hallucinator_workspace_bytes(5, dt) - 1), b"workspace too small")

        refused(ief(dt, w=False), b"hmmr_ief_fwd", b"null argument")
        for missing in ("strips", "omegas", "ws"):
            refused(ief(dt, **{missing: None}), b"hmmr_ief_fwd", b"null argument")
        for m in (0, -1):
            refused(ief(dt, m=m), b"m must be positive")
        for R in (0, -1, _lib.MAX_REGRESSORS + 1):
            refused(ief(dt, R=R), b"bad num_regressors")
        for nd0 in (72, 75, 0, 86):
            refused(ief(dt, nd=(nd0,) + (72,) * 7), b"regressor 0 must predict 85-D omega")
        # a delta width that contradicts no_optcam: 75-wide regressors in a use_optcam struct and the reverse, one odd one among eight
        refused(ief(dt, nd=(85,) + (75,) * 7), b"regressor 1 has nd=75 (expected 72)")
        refused(ief(dt, nd=(85,) + (72,) * 7, no_optcam=1), b"regressor 1 has nd=72 (expected 75)")
        refused(ief(dt, R=8, nd=(85,) + (72,) * 6 + (75,)), b"regressor 7 has nd=75 (expected 72)")
        refused(ief(dt, R=2, nd=(85, 85) + (72,) * 6), b"regressor 1 has nd=85")
        refused(ief(dt, ws_bytes=lib.hmmr_ief_workspace_bytes(5, 3, dt) - 1), b"workspace too small")
        refused(ief(dt, start=P[4], ws_bytes=lib.hmmr_ief_workspace_bytes(5, 3, dt) - 1), b"workspace too small")
