"""Device engine: owns the packed weights, the HBM workspaces and the four
stage calls of libhmmr_hip.so.  Everything above it (models.py, omega.py,
evaluation/tester.py) mirrors the reference's Python interface and only
shuffles tensors.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import time

import numpy as np
import torch

from . import _lib as L
from . import assets, devflags, packing

DTYPES = {"f32": L.HMMR_F32, "fp32": L.HMMR_F32, "float32": L.HMMR_F32,
          "bf16": L.HMMR_BF16, "bfloat16": L.HMMR_BF16,
          "f16x3": L.HMMR_F16X3, "split": L.HMMR_F16X3}
DTYPE_NAMES = {L.HMMR_F32: "f32", L.HMMR_BF16: "bf16", L.HMMR_F16X3: "f16x3"}
# The explicit fast mode: split-fp16 operands (hi/lo pairs, three fp16 MFMAs per product, fp32 accumulate) --
# the fastest mode whose end-to-end vertices / joints stay within the reference tolerance of 1e-4.
# 'bf16' is the opt-in throughput mode (vertex error ~7e-3), 'f32' the exact-fp32 MFMA mode.
DEFAULT_DTYPE = "f16x3"
TILE_TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tile_tables.json")


def set_debug(stem_route=0, stem_no_conv1=0, gemm_probe=0, smpl_blend_mfma=0, ief_no_group=0, pair_min_pixels=0, pair_two_tile_min=0, pair_form=0, keep_dead_rows=0):
    """Development switches of libhmmr_hip.so (hmmr_debug_t; process-wide, zeros = product defaults).
    pair_min_pixels: the unit-pair switch of hmmr_resnet50_fwd (0 = 12000 pixels, 1 = always the pair kernel, 2**31 - 1 = never);
    pair_two_tile_min: tiles from which a block-2 unit pair runs two tiles per workgroup (0 = 512, 1 = always, 2**31 - 1 = never);
    pair_form: 0 = the one-wave-per-SIMD unit pair of round 4 (the default), 2 = the wave-specialised form of round 6 (two waves per SIMD; same bits);
    keep_dead_rows: 1 = the fused-unit launches store every trunk row, also those only a stride-2 shortcut would skip (hmmr_tail_desc_t.trunk_keep_stride)."""
    d = L.Debug()
    d.stem_route, d.stem_no_conv1, d.gemm_probe = int(stem_route), int(stem_no_conv1), int(gemm_probe)
    d.smpl_blend_mfma, d.ief_no_group, d.pair_min_pixels = int(smpl_blend_mfma), int(ief_no_group), int(pair_min_pixels)
    d.pair_two_tile_min, d.pair_form, d.keep_dead_rows = int(pair_two_tile_min), int(pair_form), int(keep_dead_rows)
    L.load().hmmr_set_debug(C.byref(d))


def _debug_from_env():
    """devflags STEM / STEM_C1 / GEMM_PROBE (tools/ A/B scripts) -> hmmr_set_debug; the library itself never reads the
    environment."""
    e = devflags.get("STEM")
    c1 = devflags.get("STEM_C1")
    probe = int(devflags.get("GEMM_PROBE") or 0)
    if e or c1 == "0" or probe or _debug_from_env.was_set:
        set_debug(stem_route={"u": 1, "f": 2}.get(e[:1], 0), stem_no_conv1=int(c1 == "0"), gemm_probe=probe)
        _debug_from_env.was_set = bool(e or c1 == "0" or probe)


_debug_from_env.was_set = False


def _dt(d):
    if isinstance(d, str):
        if d == "bf16x3":              # rounds 1-2 called the split mode by its (then bf16) halves
            import warnings
            warnings.warn("dtype 'bf16x3' is now 'f16x3' (split operands with fp16 halves since round 3)", DeprecationWarning, stacklevel=3)
            d = "f16x3"
        if d not in DTYPES:
            raise ValueError("unknown operand mode %r: use one of %s" % (d, ", ".join(sorted(set(DTYPES)))))
        return DTYPES[d]
    return int(d)


def _packer_choices(fold_sc=None, fuse_tail=None, patch_3x3=None, unit_pair=None, b1_stream=None, b1_unit=None, stem_conv1=True,
                    stream_1x1=None):
    """HmmrEngine's constructor arguments -> the keyword arguments of packing.pack_resnet.  An argument left at None takes the
    development switch of devflags.py that names it; the switches without an argument always apply."""
    def _flag_choice(name):
        """a switch's value: "0" -> False, "1" -> True, any other word as it stands"""
        v = devflags.get(name)
        return {"0": False, "1": True}.get(v, v)

    def pick(arg, flag):
        return flag if arg is None else arg
    fsc, fold = _flag_choice("FUSE_SC"), _flag_choice("FOLD_SC")
    return dict(fuse_preact_blocks=tuple(b for b in devflags.get("FUSE_PREACT").split(",") if b),
                fuse_tail=pick(fuse_tail, _flag_choice("FUSE_TAIL")),
                fuse_sc=fsc if isinstance(fsc, bool) else "all",
                fuse_preact_first=_flag_choice("PREACT_FIRST") is not False,
                fold_sc=pick(fold_sc, fold if isinstance(fold, bool) else None),          # (None: the packer's default per operand mode)
                patch_3x3=pick(patch_3x3, int(devflags.get("PATCH_3X3"))),
                unit_pair=pick(unit_pair, _flag_choice("UNIT_PAIR")),
                b1_stream=pick(b1_stream, _flag_choice("B1_STREAM") is True),
                b1_unit=pick(b1_unit, _flag_choice("B1_UNIT") is True),
                stem_conv1=stem_conv1,
                stream_1x1=pick(stream_1x1, _flag_choice("STREAM_1X1") is True))


class _Workspace(object):
    """Grow-only HBM scratch buffer."""

    def __init__(self, device):
        self.device, self.buf = device, None

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self.buf


class HmmrEngine(object):
    """weights: dict of checkpoint-named arrays (assets.py); smpl: dict in the
    src/tf_smpl layout.  dtype: GEMM operand mode of ResNet / temporal / IEF: 'f16x3' (default: split-fp16 hi/lo
    operands, three fp16 MFMAs per product -- the mode inside the reference tolerance), 'bf16' or 'f32'; SMPL is
    always fp32 at its boundaries (its blend-shape product runs on split-fp16 MFMAs)."""

    def __init__(self, weights, smpl, dtype=DEFAULT_DTYPE, device="cuda:0", num_conv_layers=3,
                 delta_t_values=(-5, 5), joint_type="cocoplus", resnet_chunk=0,
                 temporal_dtype=None, ief_dtype=None, autotune=True, fold_sc=None, fuse_tail=None, patch_3x3=None,
                 unit_pair=None, b1_stream=None, b1_unit=None, stem_conv1=True, stream_1x1=None):
        self.lib = L.load()
        _debug_from_env()
        if not torch.cuda.is_available():
            raise L.HmmrError("HmmrEngine needs a HIP device (torch.cuda.is_available() is False)")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.dtype = _dt(dtype)
        self.temporal_dtype = self.dtype if temporal_dtype is None else _dt(temporal_dtype)
        self.ief_dtype = self.dtype if ief_dtype is None else _dt(ief_dtype)
        self.resnet_chunk = int(devflags.get("RESNET_CHUNK") or resnet_chunk)
        self.store = packing.DeviceStore(self.device)
        self.num_conv_layers = num_conv_layers
        self.delta_keys = sorted(int(d) for d in delta_t_values)
        # every stage is packed only when its variables exist: a ResNet-only checkpoint (hmr_noS5.ckpt-642561, what
        # FeatureExtractor is given: src/datasets/resnet_extractor.py:31-40) has no AZ_FC_* / single_view_ief* names
        w = weights if weights is not None else {}
        # (round 6) a NaN / inf variable is refused here, by name: the clamp of a split store would turn what it produces into finite
        # numbers, and a pre-activation constant is not behind any of the kernels' range checks (hmmr_run_flags: HMMR_FLAG_NAN)
        for name, v in w.items():
            a_ = np.asarray(v)
            if a_.dtype.kind == "f" and not np.isfinite(a_).all():
                raise ValueError("variable %r holds %d non-finite value(s)" % (name, int((~np.isfinite(a_)).sum())))
        choices = _packer_choices(fold_sc=fold_sc, fuse_tail=fuse_tail, patch_3x3=patch_3x3, unit_pair=unit_pair, b1_stream=b1_stream,
                                  b1_unit=b1_unit, stem_conv1=stem_conv1, stream_1x1=stream_1x1)
        self.rw = packing.pack_resnet(w, self.dtype, self.store, **choices) if "resnet_v2_50/conv1/weights" in w else None
        self.tw = (packing.pack_temporal(w, self.temporal_dtype, self.store, num_conv_layers)
                   if assets.temporal_scopes(0)[1] + "/weights" in w else None)
        self.hw = packing.pack_hallucinator(w, self.temporal_dtype, self.store)
        if "single_view_ief/3D_module/fc1/weights" in w and "mean_param" in w:
            self.iw, self.reg_keys = packing.pack_ief(w, self.ief_dtype, self.store, self.delta_keys)
        else:
            self.iw, self.reg_keys = None, [0]
        # the trainable fp32 bank of the regressors: packed on first use (ief_bank) from these arrays, whatever ief_dtype is
        self._ief_source = {k: v for k, v in w.items() if k.startswith("single_view_ief") or k == "mean_param"} if self.iw is not None else None
        self._ief_bank = None
        # ... and that of f_movie (the temporal blocks and the hallucinator): movie_bank, the same way
        self._movie_source = {k: v for k, v in w.items() if k.startswith(("AZ_FC_block", "fc2_res/"))} if self.tw is not None else None
        self._movie_bank = None
        # ... and the pose discriminator's (disc_pose_bank): the checkpoint's D_pose/* variables, when it has them
        self._disc_source = {k: v for k, v in w.items() if k.startswith("D_pose/")}
        self._disc_pose_bank = None
        # an all-fp32 engine is the exact-arithmetic reference (the probe's last rung, the saturation fallback): its SMPL blend product
        # stays on fp32 operands too, so nothing in it can clamp
        all_f32 = (self.dtype, self.temporal_dtype, self.ief_dtype) == (L.HMMR_F32,) * 3
        self.sc = packing.pack_smpl(smpl, self.store, joint_type, split=not all_f32) if smpl is not None else None
        self._smpl_source, self.joint_type, self._gc = smpl, joint_type, None     # the backward's constants: packed on first use (smpl_backward)
        self.num_kps = self.sc.num_kps if self.sc is not None else assets.NUM_KPS
        self.num_verts = self.sc.num_verts if self.sc is not None else assets.NUM_VERTS
        self._ws = {k: _Workspace(self.device) for k in ("resnet", "temporal", "ief", "smpl", "hal")}   # + "resnet<i>" per side stream
        # per-layer conv tiles of the ResNet.  Shipped tables (tile_tables.json: measured on an MI355X for the batch sizes
        # the BASELINE configurations produce, per operand mode) make the first call cost nothing; a batch size with no
        # shipped table within 30 % is tuned on first use (_tune_resnet), autotune="force" tunes every size and ignores
        # the shipped tables, autotune=False never tunes.  The tile never changes a result bit.
        at = devflags.get("AUTOTUNE")
        self.autotune = False if (not autotune or at == "0") else ("force" if (autotune == "force" or at == "force") else True)
        self._tiles, self._shipped = {}, set()
        self.tune_log = []       # [(frames, ms)] of every tuning pass run by this engine: never silent
        # optional on-disk copy of the tuned tables (devflags TILE_CACHE): profiling runs load it so that no tuning
        # pass ends up inside the rocprofv3 trace; tools/make_tile_tables.py writes the shipped file through it
        self._tile_cache = devflags.get("TILE_CACHE")
        sources = []
        if self.autotune != "force" and devflags.get("TILE_TABLE") != "0" and os.path.exists(TILE_TABLES):
            sources.append((TILE_TABLES, True))
        if self._tile_cache and os.path.exists(self._tile_cache):
            sources.append((self._tile_cache, False))
        for path, shipped in sources:
            import json
            for key, tab in json.load(open(path)).items():
                if key.startswith("_"):
                    continue
                dt, nt = key.split(":")
                if int(dt) == self.dtype:
                    self._tiles[int(nt)] = {(int(k.split(":")[0]), k.split(":")[1]): int(v) for k, v in tab.items()}
                    if shipped:
                        self._shipped.add(int(nt))
        # concurrent half-batches (see resnet()); env: dev A/B switch
        self.resnet_streams = int(devflags.get("RESNET_STREAMS"))
        self._side_streams = []

    # -- helpers ---------------------------------------------------------------
    @staticmethod
    def _need(packed, names):
        if packed is None:
            raise L.HmmrError("the loaded weights have no %s variables: this stage was not packed" % names)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # flags that a scoped reader (flag_scope: Tester's saturation guard, the operand-mode probe) found raised BEFORE its own work and
    # took out of the device word so that it would not mistake them for its own: run_flags() keeps reporting them, per device
    _carried_flags = {}

    def run_flags(self, clear=False):
        """Sticky run flags of this engine's device (hmmr_run_flags; _lib.FLAG_SATURATED: a split store clamped a value to the
        fp16 range since the last clear).  Synchronises with the device."""
        key = (self.device.type, self.device.index)
        v = self._device_flags(clear) | HmmrEngine._carried_flags.get(key, 0)
        if clear:
            HmmrEngine._carried_flags.pop(key, None)
        return v

    def _device_flags(self, clear):
        torch.cuda.synchronize(self.device)
        with torch.cuda.device(self.device):
            v = C.c_uint(0)
            L.check(self.lib.hmmr_run_flags(C.byref(v), int(bool(clear))), "hmmr_run_flags")
        return int(v.value)

    def flag_scope(self):
        """Context manager around a piece of work whose OWN flags are wanted: on entry whatever the (device-wide, sticky) word already
        holds is moved aside -- it stays visible to run_flags() -- and `.flags` after the block holds what was raised inside it (the word
        is left clear).  The flags are per device, not per engine: earlier work of any engine (the operand-mode probe's rejected rungs,
        raw engine calls, another Tester) must neither demote this caller nor be erased by it."""
        return _FlagScope(self)

    def to_device(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):
            return a.to(self.device, dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device).to(dtype).contiguous()

    # -- ResNet launch tuning ----------------------------------------------------
    _TUNE_TILES = tuple(int(t) for t in devflags.get("TUNE_TILES").split(","))   # hmmr_conv_desc_t.tile candidates (8-wave 128x128 / 128x64, 4-wave 64x64 / 128x128 / 128x64, 8-wave ping-pong 256x128 / 128x256)
    _TUNE_MIN_FRAMES = 32
    # two contiguous parts on concurrent streams from this many frames on (tools/resnet_parts_small.py, profiles/r06t_resnet_parts_*.log, f16x3: one stream /
    # two parts 3.35 / 3.44 ms at 128 frames, 4.01 / 4.17 at 160 -- the reference's default Tester.predict, B = 8 x T = 20 -- 5.21 / 4.80 at 192, 6.47 / 6.19 at 257)
    _SPLIT_MIN_FRAMES = 176

    def _resnet_layers(self):
        """[(profile slot, unit index, layer name)] in launch order (csrc/resnet.hip)."""
        out, slot = [], 3
        for u in range(L.RESNET_UNITS):
            names = (["shortcut"] if self.rw.unit[u].shortcut.w else []) + ["conv1", "conv2", "conv3"]
            for nm in names:
                out.append((slot, u, nm))
                slot += 1
        return out

    def _layer_of(self, u, nm):
        """the hmmr_layer_t whose .tile the launch of (unit, layer name) reads (csrc/resnet.hip)"""
        U = self.rw.unit[u]
        if nm == "conv3" and U.c3sc.w:
            return U.c3sc
        return getattr(U, nm)

    @staticmethod
    def _tile_for(lay, cand, cout, dtype=None, nm="conv2"):
        """hmmr_layer_t.tile for candidate `cand` (a tuner candidate or a tile number) on a layer with `cout` output columns, launched
        under the name `nm`: 0 (the library's choice) where nothing of the layer's kernel family fits.  The rule and the candidate maps are
        the tile list's (csrc/conv_tiles.h: hmmr_conv_tile_for)."""
        return L.load().hmmr_conv_tile_for(lay.k_order, int(nm != "conv2"), int(nm == "conv3"), cout, -1 if dtype is None else dtype, cand)

    def _layer_cout(self, u, nm):
        U = self.rw.unit[u]
        if nm == "shortcut" and U.sc_c1.w:          # shortcut + conv1 as one column-split GEMM: depth + base columns
            return U.depth + U.base
        return U.base if nm in ("conv1", "conv2") else U.depth

    def _set_tiles(self, table):
        for (u, nm), t in table.items():
            self._layer_of(u, nm).tile = self._tile_for(self._layer_of(u, nm), int(t), self._layer_cout(u, nm), self.dtype, nm)

    def _needs_tuning(self, nt):
        """A tuning pass is due for batch size nt: tuning is on, the size is worth it, it has no table of its own and (unless
        forced) no shipped or tuned table within 30 % of it; at most 8 passes per engine."""
        if not self.autotune or nt < self._TUNE_MIN_FRAMES or nt in self._tiles or torch.cuda.is_current_stream_capturing():
            return False
        if len(self.tune_log) >= 8:
            return False
        if self.autotune == "force":
            return True
        return not any(max(k, nt) <= 1.3 * min(k, nt) for k in self._tiles)

    def _tune_resnet(self, images, n, n_zero, ws_key="resnet", reps=3):
        """Pick hmmr_layer_t.tile for every ResNet conv at this batch size: `reps` instrumented passes per
        candidate tile (the first is a warm-up; every layer timed in place, behind its real producer), fastest wins per layer.
        The tile never changes a result bit (each output element is one fixed-order K reduction), it
        only moves the balance between tile-count quantisation, occupancy and operand reuse, which
        flips between layers as the batch grows.  ~90 ms once per batch size."""
        layers = self._resnet_layers()
        t_start = time.perf_counter()
        nt = n + n_zero
        nbytes = self.lib.hmmr_resnet50_workspace_bytes(nt, self.dtype)
        ws = self._ws.setdefault(ws_key, _Workspace(self.device)).get(nbytes)     # the workspace of the pass being tuned
        phi = torch.empty((nt, 2048), dtype=torch.float32, device=self.device)
        src = images.data_ptr() if n else None
        best = {}
        for cand in (0,) + self._TUNE_TILES:
            for slot, u, nm in layers:
                lay = self._layer_of(u, nm)
                lay.tile = self._tile_for(lay, cand, self._layer_cout(u, nm), self.dtype, nm)
            t = None
            for rep in range(reps):
                pm = (C.c_float * L.RESNET_PROF_SLOTS)()
                L.check(self.lib.hmmr_resnet50_fwd(C.byref(self.rw), src, n, n_zero, phi.data_ptr(), ws.data_ptr(),
                                                   nbytes, self._stream(), pm), "hmmr_resnet50_fwd")
                cur = np.frombuffer(pm, dtype=np.float32).copy()
                t = cur if (t is None or rep == 0) else np.minimum(t, cur)      # rep 0 is the warm-up
            for slot, u, nm in layers:
                tile = self._layer_of(u, nm).tile
                if (u, nm) not in best or t[slot] < best[(u, nm)][0] * 0.98:    # 2 % hysteresis towards the heuristic
                    best[(u, nm)] = (float(t[slot]), tile)
        table = {k: v[1] for k, v in best.items()}
        self.tune_log.append((nt, round((time.perf_counter() - t_start) * 1e3, 1)))     # (frames, ms): never silent
        if self._tile_cache:
            import json
            old = json.load(open(self._tile_cache)) if os.path.exists(self._tile_cache) else {}
            old["%d:%d" % (self.dtype, nt)] = {"%d:%s" % k: v for k, v in table.items()}
            json.dump(old, open(self._tile_cache, "w"))
        return table

    # -- stages ----------------------------------------------------------------
    def _resnet_pass(self, images, n, n_zero, phi, ws_key, prof=False, tune=True):
        """One hmmr_resnet50_fwd launch sequence on the current stream: images[:n] (+ n_zero zero
        images) -> phi[:n + n_zero]."""
        nt = n + n_zero
        table = None
        if tune and nt >= self._TUNE_MIN_FRAMES:
            if self._needs_tuning(nt):
                self._tiles[nt] = self._tune_resnet(images, n, n_zero, ws_key)
            if self._tiles:                                  # an untuned size borrows the nearest tuned one
                table = self._tiles[min(self._tiles, key=lambda k: abs(k - nt))]
        if table is not None:
            self._set_tiles(table)
        elif self._tiles:
            self._set_tiles({k: 0 for k in next(iter(self._tiles.values()))})
        nbytes = self.lib.hmmr_resnet50_workspace_bytes(nt, self.dtype)
        ws = self._ws.setdefault(ws_key, _Workspace(self.device)).get(nbytes)
        pm = (C.c_float * L.RESNET_PROF_SLOTS)() if prof else None
        L.check(self.lib.hmmr_resnet50_fwd(C.byref(self.rw), images.data_ptr() if n else None, n, n_zero,
                                           phi.data_ptr(), ws.data_ptr(), nbytes, self._stream(), pm),
                "hmmr_resnet50_fwd")
        return np.frombuffer(pm, dtype=np.float32).astype(np.float64) if prof else None

    def resnet_cuts(self, n, parts=None):
        """Frame boundaries of the contiguous parts `resnet()` runs n frames as ([0, n]: one part).  A caller that
        feeds the parts itself (evaluation/streaming.py: part i starts when ITS upload has landed) runs part i as
        `resnet(images[a:b], parts=1, ws_key="resnet%d" % i)` on `side_stream(i)`."""
        parts = self.resnet_streams if parts is None else int(parts)
        if parts < 2 or n < self._SPLIT_MIN_FRAMES or self.resnet_chunk > 0:
            return [0, n]
        return [(i * n) // parts for i in range(parts + 1)]

    def resnet(self, images, prof=False, n_zero=0, out=None, ws_key="resnet", parts=None):
        """images [n,224,224,3] fp32 (device) -> phi [n + n_zero,2048] fp32; the last
        n_zero rows are the features of all-zero images (the padding frames of
        predict_all_images), encoded in the same pass.  encoder_resnet, src/models.py:50-77.

        Large batches run as `resnet_streams` (default 2) contiguous parts on concurrent HIP streams:
        every layer launch ends in a partial round of workgroups (tile-count quantisation, worst in
        blocks 3-4 where a 256-frame batch is only 1.5-3 rounds), and a second, independent launch
        sequence fills those tails.  Per-frame independent => bit-identical; measured -4 %.
        parts: overrides `resnet_streams` for this call (1 = one launch sequence on the current stream, whose
        workspace is `ws_key`: a caller that keeps several passes in flight gives each its own)."""
        self._need(self.rw, "resnet_v2_50/*")
        images = self.to_device(images)
        n = images.shape[0]
        assert n == 0 or tuple(images.shape[1:]) == (224, 224, 3), images.shape
        nt = n + n_zero
        if out is not None:                                  # caller-owned feature rows (a slice of a longer video's phi)
            assert out.is_cuda and out.dtype == torch.float32 and out.shape == (nt, 2048) and out.is_contiguous()
        phi = out if out is not None else torch.empty((nt, 2048), dtype=torch.float32, device=self.device)
        if self.resnet_chunk > 0:                            # dev switch: sequential chunks, heuristic tiles
            chunk, i = self.resnet_chunk, 0
            prof_tot = np.zeros(L.RESNET_PROF_SLOTS, np.float64) if prof else None
            while i < nt:
                c_real = max(0, min(chunk, n - i))
                c_zero = min(chunk - c_real, nt - i - c_real) if i + c_real >= n else 0
                pm = self._resnet_pass(images[i:i + c_real], c_real, c_zero, phi[i:i + c_real + c_zero], "resnet",
                                       prof, tune=False)
                if prof:
                    prof_tot += pm
                i += c_real + c_zero
            return (phi, prof_tot) if prof else phi
        parts = self.resnet_streams if parts is None else int(parts)
        if prof or parts < 2 or n < self._SPLIT_MIN_FRAMES or torch.cuda.is_current_stream_capturing():
            pm = self._resnet_pass(images, n, n_zero, phi, ws_key, prof)
            return (phi, pm) if prof else phi
        cur = torch.cuda.current_stream(self.device)
        self.side_stream(parts - 1)
        cuts = [(i * n) // parts for i in range(parts + 1)]
        if self.autotune:                                    # tune every part size before anything overlaps
            for i in range(parts):
                ni, nz = cuts[i + 1] - cuts[i], (n_zero if i == parts - 1 else 0)
                if self._needs_tuning(ni + nz):
                    self._tiles[ni + nz] = self._tune_resnet(images[cuts[i]:cuts[i + 1]], ni, nz, "resnet%d" % i)
        for i in range(parts):
            side = self._side_streams[i]
            side.wait_stream(cur)                            # the frames are ready on the caller's stream
            with torch.cuda.stream(side):
                nz = n_zero if i == parts - 1 else 0
                self._resnet_pass(images[cuts[i]:cuts[i + 1]], cuts[i + 1] - cuts[i], nz,
                                  phi[cuts[i]:cuts[i + 1] + nz], "resnet%d" % i)
        for i in range(parts):
            cur.wait_stream(self._side_streams[i])
        return phi

    def side_stream(self, i):
        """The i-th of the high-priority streams the ResNet parts run on (created on first use)."""
        while len(self._side_streams) <= i:
            self._side_streams.append(torch.cuda.Stream(device=self.device, priority=int(devflags.get("RESNET_PRIORITY"))))
        return self._side_streams[i]

    def _out(self, out, shape, dtype=torch.float32):
        """the output of a stage call: a fresh tensor, or the caller's (contiguous, on this device, at least `shape` along axis 0:
        its first rows are written and returned)"""
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        assert out.is_cuda and out.device == self.device and out.dtype == dtype and out.is_contiguous(), "out: a contiguous device tensor"
        assert out.dim() == len(shape) and out.shape[0] >= shape[0] and tuple(out.shape[1:]) == tuple(shape[1:]), (tuple(out.shape), shape)
        return out[:shape[0]]

    def temporal(self, phi, out=None):
        """phi [b,t,2048] fp32 -> movie strips [b,t,2048] (into the first b windows of `out`, if given).  az_fc2_groupnorm,
        src/models.py:121-141."""
        self._need(self.tw, "AZ_FC_block*")
        phi = self.to_device(phi)
        b, t, c = phi.shape
        assert c == 2048
        out = self._out(out, (b, t, c))
        nbytes = self.lib.hmmr_temporal_workspace_bytes(b, t, self.temporal_dtype)
        ws = self._ws["temporal"].get(nbytes)
        L.check(self.lib.hmmr_temporal_fwd(C.byref(self.tw), phi.data_ptr(), b, t, out.data_ptr(),
                                           ws.data_ptr(), nbytes, self._stream()), "hmmr_temporal_fwd")
        return out

    def hallucinate(self, phi, out=None):
        """phi [..., 2048] -> hallucinated movie strips, same shape (out: [>= rows, 2048], its first rows are written).  fc2_res,
        src/models.py:270-296."""
        if self.hw is None:
            raise L.HmmrError("the loaded weights have no fc2_res/* variables (pred_mode 'hal')")
        phi = self.to_device(phi)
        flat = phi.reshape(-1, 2048)
        m = flat.shape[0]
        out = self._out(out, (m, 2048))
        nbytes = self.lib.hmmr_hallucinator_workspace_bytes(m, self.temporal_dtype)
        ws = self._ws["hal"].get(nbytes)
        L.check(self.lib.hmmr_hallucinator_fwd(C.byref(self.hw), flat.data_ptr(), m, out.data_ptr(),
                                               ws.data_ptr(), nbytes, self._stream()), "hmmr_hallucinator_fwd")
        return out.reshape(phi.shape)

    def ief(self, strips, omega_start=None, use_delta_from_pred=True, out=None):
        """strips [m,2048] -> omegas [R,m,85]; R = 1 + len(delta_t_values), deltas in sorted order.
        batch_pred_omega / call_hmr_ief, src/models.py:233-267, 299-377.  omega_start: [m,85] starting point of the IEF
        (`omega_mean`; None = the checkpoint's mean theta in every row, tester.py:181).  use_optcam is a property of the
        packed delta regressors (72- or 75-wide, `self.use_optcam`).  out: a flat fp32 tensor of at least R * m * 85 floats; its
        head is written and returned as [R,m,85]."""
        self._need(self.iw, "single_view_ief*/3D_module/* and mean_param")
        strips = self.to_device(strips)
        m = strips.shape[0]
        R = self.iw.num_regressors
        out = self._out(out, (R * m * 85,)).view(R, m, 85)
        nbytes = self.lib.hmmr_ief_workspace_bytes(m, R, self.ief_dtype)
        ws = self._ws["ief"].get(nbytes)
        start = None
        if omega_start is not None:
            start = self.to_device(omega_start).reshape(-1, 85)
            if start.shape[0] == 1:
                start = start.expand(m, 85).contiguous()
            assert start.shape == (m, 85), start.shape
        iw = L.IefWeights.from_buffer_copy(self.iw)          # a per-call copy of the (host) struct: the shared one is never toggled
        iw.delta_from_start = int(not use_delta_from_pred)
        L.check(self.lib.hmmr_ief_fwd_from(C.byref(iw), strips.data_ptr(), L.ptr(start), m, out.data_ptr(),
                                           ws.data_ptr(), nbytes, self._stream()), "hmmr_ief_fwd_from")
        return out

    @property
    def use_optcam(self):
        """True when the packed delta regressors predict 72 values and get the fixed camera [1, 0, 0] (models.py:333-371)."""
        return self.iw is None or not self.iw.no_optcam

    # -- the regressors under training (csrc/ief_grad.hip) ------------------------
    def ief_bank(self):
        """The trainable IEF bank (ief_bank.IefBank): an HMMR_F32 pack of the engine's regressors whose layers are tensor views of
        the packed memory, whatever `ief_dtype` the engine runs.  Packed on the first call: an inference-only process never pays
        for it.  The inference path (`ief`) keeps its own pack and does not see updates of the bank."""
        self._need(self.iw, "single_view_ief*/3D_module/* and mean_param")
        if self._ief_bank is None:
            from .ief_bank import IefBank
            self._ief_bank = IefBank(self._ief_source, [k for k in self.reg_keys if k != 0], self.device, num_stages=self.iw.num_stages)
        return self._ief_bank

    def _ief_train_args(self, strips, omega_start, keep, keep_prob, use_delta_from_pred):
        bank = self.ief_bank()
        strips = self.to_device(strips).reshape(-1, 2048)
        m, R, S = strips.shape[0], bank.iw.num_regressors, bank.iw.num_stages
        start = None
        if omega_start is not None:
            start = self.to_device(omega_start).reshape(-1, 85)
            if start.shape[0] == 1:
                start = start.expand(m, 85).contiguous()
            if start.shape != (m, 85):
                raise ValueError("omega_start: expected [%d, 85], got %s" % (m, tuple(start.shape)))
        scale = 1.0
        if keep is not None:
            keep = (keep if isinstance(keep, torch.Tensor) else torch.tensor(np.asarray(keep))).to(self.device, torch.uint8).contiguous()
            if tuple(keep.shape) != (R, S, 2, m, 1024):
                raise ValueError("keep: expected a uint8 mask of shape %s, got %s" % ((R, S, 2, m, 1024), tuple(keep.shape)))
            if keep_prob is None or not (0.0 < float(keep_prob) <= 1.0):
                raise ValueError("keep is given: keep_prob must lie in (0, 1], got %r" % (keep_prob,))
            scale = 1.0 / float(keep_prob)
        iw = L.IefWeights.from_buffer_copy(bank.iw)          # a per-call copy of the (host) struct: the shared one is never toggled
        iw.delta_from_start = int(not use_delta_from_pred)
        nbytes = self.lib.hmmr_ief_bwd_workspace_bytes(m, R, S)
        ws = self._ws.setdefault("ief_grad", _Workspace(self.device)).get(nbytes)
        return bank, iw, strips, start, keep, scale, m, R, ws, nbytes

    def ief_train(self, strips, omega_start=None, keep=None, keep_prob=None, use_delta_from_pred=True):
        """The training form of `ief` on the fp32 bank (hmmr_ief_fwd_train): strips [m,2048] -> omegas [R,m,85].  keep: uint8
        [R, num_stages, 2, m, 1024] of zeros and ones (the dropout behind fc1 and fc2 of every stage, src/models.py:103-105) with
        keep_prob, the probability it was drawn with (the kept units are scaled by 1 / keep_prob); None = no dropout."""
        bank, iw, strips, start, keep, scale, m, R, ws, nbytes = self._ief_train_args(strips, omega_start, keep, keep_prob, use_delta_from_pred)
        out = torch.empty((R, m, 85), dtype=torch.float32, device=self.device)
        L.check(self.lib.hmmr_ief_fwd_train(C.byref(iw), strips.data_ptr(), L.ptr(start), L.ptr(keep), scale, m, out.data_ptr(),
                                            ws.data_ptr(), nbytes, self._stream()), "hmmr_ief_fwd_train")
        return out

    def ief_backward(self, strips, d_omegas, omega_start=None, keep=None, keep_prob=None, use_delta_from_pred=True,
                     want_strips=True, want_start=None, want_weights=True):
        """The derivative of `ief_train` (hmmr_ief_bwd): the forward's inputs as it took them and d_omegas [R,m,85] ->
        (d_strips [m,2048] or None, d_omega_start [m,85] or None, [{name: gradient}] per regressor in the bank's layouts).
        want_weights: True, False, or per regressor a collection of the names wanted (ief_bank.NAMES); what is not wanted is None and
        its launches are not queued.  want_start defaults to `omega_start is not None`.  Nothing is kept from a forward call."""
        from .ief_bank import NAMES
        bank, iw, strips, start, keep, scale, m, R, ws, nbytes = self._ief_train_args(strips, omega_start, keep, keep_prob, use_delta_from_pred)
        d_omegas = self.to_device(d_omegas).reshape(R, m, 85).contiguous()
        want_start = (start is not None) if want_start is None else bool(want_start)
        d = L.IefBwdDesc()
        d.strips, d.omega_start, d.keep, d.keep_scale, d.m, d.d_omegas = strips.data_ptr(), L.ptr(start), L.ptr(keep), scale, m, d_omegas.data_ptr()
        d_strips = torch.empty((m, 2048), dtype=torch.float32, device=self.device) if want_strips else None
        d_start = torch.empty((m, 85), dtype=torch.float32, device=self.device) if want_start else None
        d.d_strips, d.d_omega_start = L.ptr(d_strips), L.ptr(d_start)
        grads = []
        for r in range(R):
            names = NAMES if want_weights is True else (() if not want_weights else tuple(want_weights[r] or ()))
            g = {n: (torch.empty(bank.params[r][n].shape, dtype=torch.float32, device=self.device) if n in names else None) for n in NAMES}
            for n in NAMES:
                setattr(d.reg[r], "d_" + n, L.ptr(g[n]))
            grads.append(g)
        L.check(self.lib.hmmr_ief_bwd(C.byref(iw), C.byref(d), ws.data_ptr(), nbytes, self._stream()), "hmmr_ief_bwd")
        return d_strips, d_start, grads

    # -- f_movie under training (csrc/movie_grad.hip) ------------------------------
    def movie_bank(self):
        """The trainable f_movie bank (movie_bank.MovieBank): an HMMR_F32 pack of the engine's temporal blocks and, when the checkpoint
        has one, of the hallucinator, whose layers are tensor views of the packed memory, whatever `temporal_dtype` the engine runs.
        Packed on the first call: an inference-only process never pays for it.  The inference path (`temporal`, `hallucinate`) keeps
        its own pack and does not see updates of the bank."""
        self._need(self.tw, "AZ_FC_block*")
        if self._movie_bank is None:
            from .movie_bank import MovieBank
            self._movie_bank = MovieBank(self._movie_source, self.device, num_conv_layers=self.num_conv_layers)
        return self._movie_bank

    def _hal_bank(self):
        bank = self.movie_bank()
        if bank.hw is None:
            raise L.HmmrError("the loaded weights have no fc2_res/* variables (pred_mode 'hal')")
        return bank

    def _movie_ws(self, nbytes):
        return self._ws.setdefault("movie_grad", _Workspace(self.device)).get(nbytes)

    def temporal_train(self, phi):
        """`temporal` on the fp32 bank (hmmr_temporal_fwd; the encoder has no dropout, src/models.py:121-228): phi [b,t,2048] ->
        movie strips [b,t,2048]"""
        bank = self.movie_bank()
        phi = self.to_device(phi)
        b, t, c = phi.shape
        assert c == 2048
        out = torch.empty((b, t, c), dtype=torch.float32, device=self.device)
        nbytes = self.lib.hmmr_temporal_workspace_bytes(b, t, L.HMMR_F32)
        ws = self._movie_ws(nbytes)
        L.check(self.lib.hmmr_temporal_fwd(C.byref(bank.tw), phi.data_ptr(), b, t, out.data_ptr(), ws.data_ptr(), nbytes, self._stream()),
                "hmmr_temporal_fwd")
        return out

    def hallucinate_train(self, phi):
        """`hallucinate` on the fp32 bank (hmmr_hallucinator_fwd): phi [..., 2048] -> hallucinated movie strips, same shape"""
        bank = self._hal_bank()
        phi = self.to_device(phi)
        flat = phi.reshape(-1, 2048)
        m = flat.shape[0]
        out = torch.empty((m, 2048), dtype=torch.float32, device=self.device)
        nbytes = self.lib.hmmr_hallucinator_workspace_bytes(m, L.HMMR_F32)
        ws = self._movie_ws(nbytes)
        L.check(self.lib.hmmr_hallucinator_fwd(C.byref(bank.hw), flat.data_ptr(), m, out.data_ptr(), ws.data_ptr(), nbytes, self._stream()),
                "hmmr_hallucinator_fwd")
        return out.reshape(phi.shape)

    def temporal_backward(self, phi, d_strips, want_phi=True, want_weights=True):
        """The derivative of `temporal_train` (hmmr_temporal_bwd): phi [b,t,2048] as the forward took it and d_strips [b,t,2048] ->
        (d_phi [b,t,2048] or None, [{name: gradient}] per block in the bank's layouts).  want_weights: True, False, or per block a
        collection of the names wanted (movie_bank.BLOCK_NAMES); what is not wanted is None and its launches are not queued.
        Nothing is kept from a forward call."""
        from .movie_bank import BLOCK_NAMES
        bank = self.movie_bank()
        phi = self.to_device(phi)
        b, t, c = phi.shape
        assert c == 2048
        d_strips = self.to_device(d_strips).reshape(b, t, c)
        d = L.TemporalBwdDesc()
        d.phi, d.b, d.t, d.d_strips = phi.data_ptr(), b, t, d_strips.data_ptr()
        d_phi = torch.empty((b, t, c), dtype=torch.float32, device=self.device) if want_phi else None
        d.d_phi = L.ptr(d_phi)
        grads = []
        for i in range(bank.num_blocks):
            names = BLOCK_NAMES if want_weights is True else (() if not want_weights else tuple(want_weights[i] or ()))
            g = {n: (torch.empty(bank.blocks[i][n].shape, dtype=torch.float32, device=self.device) if n in names else None) for n in BLOCK_NAMES}
            for n in BLOCK_NAMES:
                setattr(d.block[i], "d_" + n, L.ptr(g[n]))
            grads.append(g)
        nbytes = self.lib.hmmr_temporal_bwd_workspace_bytes(b, t, bank.num_blocks)
        ws = self._movie_ws(nbytes)
        L.check(self.lib.hmmr_temporal_bwd(C.byref(bank.tw), C.byref(d), ws.data_ptr(), nbytes, self._stream()), "hmmr_temporal_bwd")
        return d_phi, grads

    def hallucinate_backward(self, phi, d_out, want_phi=True, want_weights=True):
        """The derivative of `hallucinate_train` (hmmr_hallucinator_bwd): phi [..., 2048] and d_out of the same shape ->
        (d_phi of that shape or None, {name: gradient} in the bank's layouts).  want_weights: True, False or a collection of the names
        wanted (movie_bank.HAL_NAMES)."""
        from .movie_bank import HAL_NAMES
        bank = self._hal_bank()
        phi = self.to_device(phi)
        flat = phi.reshape(-1, 2048)
        m = flat.shape[0]
        d_out = self.to_device(d_out).reshape(m, 2048)
        names = HAL_NAMES if want_weights is True else (() if not want_weights else tuple(want_weights))
        d = L.HallucinatorBwdDesc()
        d.phi, d.m, d.d_out = flat.data_ptr(), m, d_out.data_ptr()
        d_phi = torch.empty((m, 2048), dtype=torch.float32, device=self.device) if want_phi else None
        d.d_phi = L.ptr(d_phi)
        g = {n: (torch.empty(bank.hal[n].shape, dtype=torch.float32, device=self.device) if n in names else None) for n in HAL_NAMES}
        for n in HAL_NAMES:
            setattr(d, "d_" + n, L.ptr(g[n]))
        nbytes = self.lib.hmmr_hallucinator_bwd_workspace_bytes(m)
        ws = self._movie_ws(nbytes)
        L.check(self.lib.hmmr_hallucinator_bwd(C.byref(bank.hw), C.byref(d), ws.data_ptr(), nbytes, self._stream()), "hmmr_hallucinator_bwd")
        return (d_phi.reshape(phi.shape) if d_phi is not None else None), g

    # -- the pose discriminator (csrc/disc_pose.hip) -------------------------------
    def disc_pose_bank(self, weights=None):
        """The trainable pose-discriminator bank (disc_bank.PoseDiscBank): an HMMR_F32 pack whose twelve tensors are views of the
        packed memory.  weights: a dict of checkpoint-named arrays (D_pose/*) that (re)places the bank; None = the bank there is, packed
        on the first call from the engine's checkpoint -- an inference-only process never pays for it."""
        if weights is not None or self._disc_pose_bank is None:
            from .disc_bank import PoseDiscBank
            src = weights if weights is not None else self._disc_source
            if not src:
                raise L.HmmrError("the loaded weights have no D_pose/* variables: pass them to disc_pose_bank(weights)")
            self._disc_pose_bank = PoseDiscBank(src, self.device)
        return self._disc_pose_bank

    def _pose_rows(self, x, what):
        """a segment of pose rows as (tensor kept alive, hmmr_rows_t): fp32 device rows of 207 values at any row stride >= 207 with
        a unit inner stride are used in place -- [n,207], [n,23,9], [n,23,1,9], [n,23,3,3], or [n,24,...] / [n,216] from which the
        global rotation is dropped as a view (Rs + 9, ld = 216)"""
        r = L.Rows()
        if x is None:
            return None, r
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
            x = self.to_device(x)
        n = x.shape[0]
        if n == 0:
            return None, r
        per = x[0].numel()
        if per not in (207, 216):
            raise ValueError("%s: rows of 207 (joints 1..23) or 216 (all 24 rotations) values, got %s" % (what, tuple(x.shape)))
        inner = x[0]
        if not inner.is_contiguous() or (n > 1 and x.stride(0) < per):
            x = x.contiguous()
        flat = x.as_strided((n, per), (x.stride(0) if n > 1 else per, 1), x.storage_offset())
        if per == 216:
            flat = flat[:, 9:]
        r.ptr, r.ld, r.n = flat.data_ptr(), flat.stride(0), n
        return flat, r

    def _disc_ws(self, n):
        nbytes = self.lib.hmmr_disc_pose_workspace_bytes(n)
        return self._ws.setdefault("disc_pose", _Workspace(self.device)).get(nbytes), nbytes

    def _disc_grads(self, bank, want_weights, g):
        from .disc_bank import NAMES
        names = NAMES if want_weights is True else (() if not want_weights else tuple(want_weights))
        out = {n: (torch.empty(bank.params[n].shape, dtype=torch.float32, device=self.device) if n in names else None) for n in NAMES}
        for n in NAMES:
            setattr(g, "d_" + n, L.ptr(out[n]))
        return out

    def disc_pose(self, poses_a, poses_b=None):
        """PoseDiscriminator.get_output on the bank (hmmr_disc_pose_fwd): two segments of pose rows (see _pose_rows; either may be
        None or empty) -> out [n_a + n_b, 24], the rows of poses_a first.  Nothing is concatenated or copied."""
        bank = self.disc_pose_bank()
        ka, ra = self._pose_rows(poses_a, "poses_a")
        kb, rb = self._pose_rows(poses_b, "poses_b")
        n = ra.n + rb.n
        out = torch.empty((n, 24), dtype=torch.float32, device=self.device)
        ws, nbytes = self._disc_ws(n)
        L.check(self.lib.hmmr_disc_pose_fwd(C.byref(bank.dw), C.byref(ra), C.byref(rb), out.data_ptr(), ws.data_ptr(), nbytes, self._stream()),
                "hmmr_disc_pose_fwd")
        return out

    def disc_pose_backward(self, poses_a, poses_b, d_out, want_poses_a=True, want_poses_b=True, want_weights=True, full_a=False, full_b=False):
        """The derivative of `disc_pose` (hmmr_disc_pose_bwd): the forward's inputs and d_out [n_a + n_b, 24] -> (d_poses_a [n_a,207]
        or None, d_poses_b [n_b,207] or None, {name: gradient} in the bank's layouts).  want_weights: True, False or a collection of
        the names wanted (disc_bank.NAMES); what is not wanted is None and its launches are not queued.  full_a / full_b: the
        segment's gradient as [n,216] rows whose first nine values (the global rotation) are zeros."""
        bank = self.disc_pose_bank()
        ka, ra = self._pose_rows(poses_a, "poses_a")
        kb, rb = self._pose_rows(poses_b, "poses_b")
        n = ra.n + rb.n
        d_out = self.to_device(d_out).reshape(n, 24)
        d = L.DiscPoseBwdDesc()
        d.rows_a, d.rows_b, d.d_out = ra, rb, d_out.data_ptr()
        def grad_rows(want, r, full):
            if not (want and r.n):
                return None, None, 207
            if full:                                         # [n,216] rows: zeros for the global rotation, the 207 values behind them
                g = torch.zeros((r.n, 216), dtype=torch.float32, device=self.device)
                return g, g.data_ptr() + 36, 216
            g = torch.empty((r.n, 207), dtype=torch.float32, device=self.device)
            return g, g.data_ptr(), 207
        d_a, d.d_poses_a, d.ld_a = grad_rows(want_poses_a, ra, full_a)
        d_b, d.d_poses_b, d.ld_b = grad_rows(want_poses_b, rb, full_b)
        grads = self._disc_grads(bank, want_weights, d.grads)
        ws, nbytes = self._disc_ws(n)
        L.check(self.lib.hmmr_disc_pose_bwd(C.byref(bank.dw), C.byref(d), ws.data_ptr(), nbytes, self._stream()), "hmmr_disc_pose_bwd")
        return d_a, d_b, grads

    def pose_prior(self, real, fake, w_e=1.0, w_d=1.0, want_losses=True, want_d_rs=True, want_weights=True):
        """The closed loop of one step on one recomputed forward (hmmr_pose_prior): mocap rows `real`, predicted rows `fake` ->
        (losses [3] = e_pose, d_real, d_fake, d_rs_fake [n_fake,24,3,3] = w_e d e_pose / d Rs with a zero global rotation -- what
        `smpl_backward` takes as d_rs --, {name: gradient of w_d d_pose} in the bank's layouts).  Each is None when not wanted."""
        bank = self.disc_pose_bank()
        ka, ra = self._pose_rows(real, "real")
        kb, rb = self._pose_rows(fake, "fake")
        d = L.PosePriorDesc()
        d.real, d.fake, d.w_e, d.w_d = ra, rb, float(w_e), float(w_d)
        losses = torch.empty((3,), dtype=torch.float32, device=self.device) if want_losses else None
        d_rs = torch.empty((rb.n, 24, 3, 3), dtype=torch.float32, device=self.device) if want_d_rs else None
        d.losses, d.d_rs_fake = L.ptr(losses), L.ptr(d_rs)
        grads = self._disc_grads(bank, want_weights, d.grads)
        ws, nbytes = self._disc_ws(ra.n + rb.n)
        L.check(self.lib.hmmr_pose_prior(C.byref(bank.dw), C.byref(d), ws.data_ptr(), nbytes, self._stream()), "hmmr_pose_prior")
        return losses, d_rs, grads

    def smpl(self, theta, beta, cams=None, want_rs=True):
        """theta [m,72], beta [m,10], cams [m,3] or None (row-major views with a
        unit inner stride are used in place).  Returns verts [m,V,3], joints
        [m,K,3], kps [m,K,2] or None, Rs [m,24,3,3] or None.
        SMPL.__call__, src/tf_smpl/batch_smpl.py:89-162."""
        def prep(x, width):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32
                    and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == width):
                x = self.to_device(x).reshape(-1, width)
            return x
        theta, beta = prep(theta, 72), prep(beta, 10)
        m = theta.shape[0]
        cams = prep(cams, 3) if cams is not None else None
        V, K = self.num_verts, self.num_kps
        verts = torch.empty((m, V, 3), dtype=torch.float32, device=self.device)
        joints = torch.empty((m, K, 3), dtype=torch.float32, device=self.device)
        kps = torch.empty((m, K, 2), dtype=torch.float32, device=self.device) if cams is not None else None
        rs = torch.empty((m, 24, 3, 3), dtype=torch.float32, device=self.device) if want_rs else None
        nbytes = self.lib.hmmr_smpl_workspace_bytes(m)
        ws = self._ws["smpl"].get(nbytes)
        L.check(self.lib.hmmr_smpl_fwd(C.byref(self.sc), theta.data_ptr(), theta.stride(0),
                                       beta.data_ptr(), beta.stride(0),
                                       L.ptr(cams), cams.stride(0) if cams is not None else 0, m,
                                       verts.data_ptr(), joints.data_ptr(), L.ptr(kps), L.ptr(rs),
                                       ws.data_ptr(), nbytes, self._stream()), "hmmr_smpl_fwd")
        return verts, joints, kps, rs

    def smpl_backward(self, theta, beta, cams=None, joints=None, d_verts=None, d_joints=None, d_kps=None, d_rs=None, want_cams=None):
        """The derivative of `smpl` (hmmr_smpl_bwd, csrc/smpl_grad.hip): theta [m,72], beta [m,10], cams [m,3] or None as the forward
        took them (fp32 device tensors; row-major views with a unit inner stride are used in place), joints [m,K,3] = the forward's
        output (needed with d_kps), and the gradients of a loss with respect to verts [m,V,3], joints [m,K,3], kps [m,K,2] and
        Rs [m,24,3,3] -- any of them None (= zero), at least one given.  Returns d_theta [m,72], d_beta [m,10] and d_cams [m,3]
        (None without cams, or with want_cams=False).  The function differentiated is the exact fp32 forward."""
        def prep(x, width):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32
                    and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == width):
                x = self.to_device(x).reshape(-1, width)
            return x
        theta, beta = prep(theta, 72), prep(beta, 10)
        m = theta.shape[0]
        cams = prep(cams, 3) if cams is not None else None
        V, K = self.num_verts, self.num_kps

        def dense(x, shape):
            if x is None:
                return None
            x = self.to_device(x)
            if tuple(x.shape) != (m,) + shape:
                raise ValueError("expected a gradient of shape %s, got %s" % ((m,) + shape, tuple(x.shape)))
            return x
        joints, d_verts, d_joints = dense(joints, (K, 3)), dense(d_verts, (V, 3)), dense(d_joints, (K, 3))
        d_kps, d_rs = dense(d_kps, (K, 2)), dense(d_rs, (24, 3, 3))
        if self._gc is None:                                 # packed on the first backward call: an inference-only process never pays for it
            self._gc = packing.pack_smpl_grad(self._smpl_source, self.store, self.joint_type)
        want_cams = (cams is not None) if want_cams is None else (bool(want_cams) and cams is not None)
        d_theta = torch.empty((m, 72), dtype=torch.float32, device=self.device)
        d_beta = torch.empty((m, 10), dtype=torch.float32, device=self.device)
        d_cams = torch.empty((m, 3), dtype=torch.float32, device=self.device) if want_cams else None
        nbytes = self.lib.hmmr_smpl_bwd_workspace_bytes(C.byref(self.sc), m)
        ws = self._ws.setdefault("smpl_bwd", _Workspace(self.device)).get(nbytes)
        L.check(self.lib.hmmr_smpl_bwd(C.byref(self.sc), C.byref(self._gc), theta.data_ptr(), theta.stride(0), beta.data_ptr(), beta.stride(0),
                                       L.ptr(cams), cams.stride(0) if cams is not None else 0, L.ptr(joints), m,
                                       L.ptr(d_verts), L.ptr(d_joints), L.ptr(d_kps), L.ptr(d_rs),
                                       d_theta.data_ptr(), d_beta.data_ptr(), L.ptr(d_cams),
                                       ws.data_ptr(), nbytes, self._stream()), "hmmr_smpl_bwd")
        return d_theta, d_beta, d_cams

    # -- the trainer's losses (csrc/losses.hip) -----------------------------------
    def _loss_desc(self, B, T, K, flags, weights, delta_t, gt):
        """hmmr_seq_loss_desc_t with shape, selection and ground truth filled in; `gt`: {kps, joints, rs, shapes, has_gt3d_smpl,
        has_gt3d_joints} of fp32 device tensors (missing = NULL).  Returns (desc, the tensors it points to)."""
        d = L.SeqLossDesc()
        d.B, d.T, d.K, d.delta_t, d.flags = int(B), int(T), int(K), int(delta_t), int(flags)
        w = list(weights) if weights is not None else [1.0] * 5
        if len(w) not in (5, 6):
            raise ValueError("weights: (e_kp, e_joints, e_smpl, e_const, e_shape), got %d values" % len(w))
        d.weights = (C.c_float * 6)(*([float(v) for v in w] + [0.0] * (6 - len(w))))
        N = d.B * d.T
        shapes = {"kps": (N, d.K, 3), "joints": (N, 14, 3), "rs": (N, 24, 3, 3), "shapes": (d.B, 10), "has_gt3d_smpl": (d.B,),
                  "has_gt3d_joints": (d.B,)}
        keep = {}
        for k, shp in shapes.items():
            x = (gt or {}).get(k)
            if x is None:
                continue
            x = self.to_device(x).reshape(shp)
            keep[k] = x
            setattr(d, {"kps": "kps_gt", "joints": "joints_gt", "rs": "rs_gt", "shapes": "shapes_gt"}.get(k, k), x.data_ptr())
        return d, keep

    def seq_losses(self, B, T, flags, gt, kps_pred=None, joints_pred=None, rs_pred=None, beta_pred=None, weights=None, delta_t=0,
                   want_grads=True, want_best_cam=False, check=False, K=None):
        """The trainer's loss stage (hmmr_seq_losses): predictions as `smpl` returns them for N = B T sequence-major rows (kps_pred
        [N,K,2], joints_pred [N,K,3], rs_pred [N,24,3,3], beta_pred [N,10] -- a view with a row stride is used in place), `gt` a dict of
        kps [N,K,3], joints [N,14,3], rs [N,24,3,3], shapes [B,10], has_gt3d_smpl [B], has_gt3d_joints [B]; `flags` a mask of
        _lib.LOSS_*, `weights` = (e_kp, e_joints, e_smpl, e_const, e_shape).  Returns {losses [8] (order _lib.LOSS_NAMES), d_kps,
        d_joints, d_rs, d_beta (want_grads: the gradients of total = sum w_i L_i; a bool, or the set of names wanted), best_cam
        [N,3] (want_best_cam; rows outside an optcam slice are NaN), status (a device int32 word)}.  check=True reads the status back
        (synchronises) and raises on a frame without a visible keypoint under KP_OPTCAM."""
        N, K = int(B) * int(T), int(self.num_kps if K is None else K)          # (K: the loss stage alone runs on any keypoint count)
        d, keep = self._loss_desc(B, T, K, flags, weights, delta_t, gt)

        def dense(x, shape):
            if x is None:
                return None
            x = self.to_device(x)
            if tuple(x.shape) != shape:
                raise ValueError("expected a prediction of shape %s, got %s" % (shape, tuple(x.shape)))
            return x
        kps_pred, joints_pred, rs_pred = dense(kps_pred, (N, K, 2)), dense(joints_pred, (N, K, 3)), dense(rs_pred, (N, 24, 3, 3))
        if beta_pred is not None:
            if not (isinstance(beta_pred, torch.Tensor) and beta_pred.is_cuda and beta_pred.dtype == torch.float32 and beta_pred.dim() == 2
                    and beta_pred.stride(1) == 1 and beta_pred.shape[1] == 10):
                beta_pred = self.to_device(beta_pred).reshape(-1, 10)
            if beta_pred.shape[0] != N:
                raise ValueError("expected %d rows of beta, got %d" % (N, beta_pred.shape[0]))
            d.beta_pred, d.ld_beta = beta_pred.data_ptr(), beta_pred.stride(0)
        d.kps_pred, d.joints_pred, d.rs_pred = L.ptr(kps_pred), L.ptr(joints_pred), L.ptr(rs_pred)
        names = ("d_kps", "d_joints", "d_rs", "d_beta")
        wanted = set(names if want_grads is True else (() if not want_grads else want_grads))
        out = {"losses": torch.empty(8, dtype=torch.float32, device=self.device),
               "status": torch.zeros(1, dtype=torch.int32, device=self.device)}
        for k, shp in zip(names, ((N, K, 2), (N, K, 3), (N, 24, 3, 3), (N, 10))):
            out[k] = torch.empty(shp, dtype=torch.float32, device=self.device) if k in wanted else None
            setattr(d, k, L.ptr(out[k]))
        out["best_cam"] = torch.full((N, 3), float("nan"), dtype=torch.float32, device=self.device) if want_best_cam else None
        d.losses, d.status, d.best_cam = out["losses"].data_ptr(), out["status"].data_ptr(), L.ptr(out["best_cam"])
        nbytes = self.lib.hmmr_seq_losses_workspace_bytes(d.B, d.T)
        ws = self._ws.setdefault("losses", _Workspace(self.device)).get(nbytes)
        d.ws, d.ws_bytes = ws.data_ptr(), nbytes
        L.check(self.lib.hmmr_seq_losses(C.byref(d), self._stream()), "hmmr_seq_losses")
        if check and int(out["status"].item()) & L.LOSS_NO_VISIBLE:
            raise L.HmmrError("hmmr_seq_losses: a frame of the slice has no visible keypoint under KP_OPTCAM (the loss is not finite)")
        return out

    def omega_loss_grad(self, omega, B, T, flags, gt, weights=None, delta_t=0, use_optcam=False, want_best_cam=False):
        """The closed loop (hmmr_omega_loss_grad): omega [B T, 85] (or [B, T, 85]) fp32 -> (losses [8], d_omega of omega's shape, status
        [1] int32, best_cam [N,3] or None): hmmr_smpl_fwd, hmmr_seq_losses and hmmr_smpl_bwd on one stream out of one workspace."""
        shape = tuple(omega.shape) if isinstance(omega, torch.Tensor) else None
        om = self.to_device(omega).reshape(-1, 85)
        N = int(B) * int(T)
        if om.shape[0] != N:
            raise ValueError("expected %d rows of omega, got %d" % (N, om.shape[0]))
        d, keep = self._loss_desc(B, T, self.num_kps, flags, weights, delta_t, gt)
        if self._gc is None:
            self._gc = packing.pack_smpl_grad(self._smpl_source, self.store, self.joint_type)
        losses = torch.empty(8, dtype=torch.float32, device=self.device)
        d_omega = torch.empty((N, 85), dtype=torch.float32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        best_cam = torch.full((N, 3), float("nan"), dtype=torch.float32, device=self.device) if want_best_cam else None
        d.status, d.best_cam = status.data_ptr(), L.ptr(best_cam)
        nbytes = self.lib.hmmr_omega_loss_grad_workspace_bytes(C.byref(self.sc), d.B, d.T)
        ws = self._ws.setdefault("omega_loss", _Workspace(self.device)).get(nbytes)
        L.check(self.lib.hmmr_omega_loss_grad(C.byref(self.sc), C.byref(self._gc), C.byref(d), om.data_ptr(), int(bool(use_optcam)),
                                              losses.data_ptr(), d_omega.data_ptr(), ws.data_ptr(), nbytes, self._stream()),
                "hmmr_omega_loss_grad")
        return losses, (d_omega.reshape(shape) if shape is not None else d_omega), status, best_cam

    def strip_mse(self, a, b, weight=1.0, want_loss=True, want_d_a=True, want_d_b=True):
        """tf.losses.mean_squared_error of two [..., cols] fp32 device tensors of one shape (hmmr_strip_mse; the trainer's e_hallucinate):
        -> (loss, a device scalar; d_a = weight 2 (a - b) / N and d_b = -d_a in the inputs' shape).  Each is None when not wanted.
        2-D views with a unit inner stride are read in place."""
        def rows(x):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
                x = self.to_device(x)
            if not (x.dim() == 2 and x.stride(1) == 1 and (x.shape[0] == 1 or x.stride(0) >= x.shape[1])):
                x = x.contiguous().reshape(-1, x.shape[-1])
            return x
        shape = tuple(a.shape)
        if tuple(b.shape) != shape or len(shape) == 0:
            raise ValueError("strip_mse: two tensors of one shape [..., cols], got %s and %s" % (shape, tuple(b.shape)))
        a, b = rows(a), rows(b)
        n, c = a.shape
        ld = lambda x: x.stride(0) if n > 1 else c
        loss = torch.empty((), dtype=torch.float32, device=self.device) if want_loss else None
        d_a = torch.empty((n, c), dtype=torch.float32, device=self.device) if want_d_a else None
        d_b = torch.empty((n, c), dtype=torch.float32, device=self.device) if want_d_b else None
        nbytes = self.lib.hmmr_strip_mse_workspace_bytes(n)
        ws = self._ws.setdefault("strip_mse", _Workspace(self.device)).get(nbytes)
        L.check(self.lib.hmmr_strip_mse(a.data_ptr(), ld(a), b.data_ptr(), ld(b), n, c, float(weight), L.ptr(loss), L.ptr(d_a), c, L.ptr(d_b), c,
                                        ws.data_ptr(), nbytes, self._stream()), "hmmr_strip_mse")
        return loss, (d_a.reshape(shape) if d_a is not None else None), (d_b.reshape(shape) if d_b is not None else None)

    def adam_step(self, segments, lr, beta1, beta2, epsilon, beta1_power, beta2_power):
        """One tf.train.AdamOptimizer step over `segments` in ONE call (hmmr_adam_step, csrc/adam.hip): an iterable of (p, g, m, v)
        contiguous fp32 device tensors of equal element counts, updated in place; g None = a variable without a gradient, which keeps
        its bytes.  The beta powers are the caller's float32 products of the step (optim.TFAdam owns them)."""
        segs = list(segments)
        table = (L.AdamSeg * max(len(segs), 1))()
        for i, (p, g, m, v) in enumerate(segs):
            for t in (p, m, v) + ((g,) if g is not None else ()):
                if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()):
                    raise ValueError("adam_step: segment %d needs contiguous fp32 device tensors of one element count" % i)
            table[i].p, table[i].g, table[i].m, table[i].v, table[i].n = p.data_ptr(), L.ptr(g), m.data_ptr(), v.data_ptr(), p.numel()
        h = L.AdamHyper(float(lr), float(beta1), float(beta2), float(epsilon), float(beta1_power), float(beta2_power))
        L.check(self.lib.hmmr_adam_step(table, len(segs), C.byref(h), self._stream()), "hmmr_adam_step")

    def smpl_into(self, theta, beta, cams, rec, off_verts, off_joints, off_kps, off_rs):
        """SMPL forward that writes instance i's verts/joints/kps/Rs straight into row i of
        the packed record tensor `rec` [m, rec_len] at the given float offsets
        (hmmr_smpl_fwd_strided).  theta/beta/cams: fp32 device views with unit inner stride."""
        m = theta.shape[0]
        assert rec.dtype == torch.float32 and rec.stride(1) == 1 and rec.shape[0] >= m
        for x, wdt in ((theta, 72), (beta, 10), (cams, 3)):
            assert x.is_cuda and x.dtype == torch.float32 and x.stride(1) == 1 and x.shape == (m, wdt)
        nbytes = self.lib.hmmr_smpl_workspace_bytes(m)
        ws = self._ws["smpl"].get(nbytes)
        base = rec.data_ptr()
        L.check(self.lib.hmmr_smpl_fwd_strided(
            C.byref(self.sc), theta.data_ptr(), theta.stride(0), beta.data_ptr(), beta.stride(0),
            cams.data_ptr(), cams.stride(0), m, base + 4 * off_verts, base + 4 * off_joints,
            base + 4 * off_kps, base + 4 * off_rs, rec.stride(0), ws.data_ptr(), nbytes, self._stream()),
            "hmmr_smpl_fwd_strided")

    def smpl_records(self, om, rec, field_offsets):
        """All containers in one launch set (hmmr_smpl_fwd_records): om [R,n,85] contiguous fp32 (present first), rec
        [>= n, rec_len] fp32 with unit inner stride, field_offsets [R][7] = float offsets of (cams, joints, kps, poses,
        shapes, verts, omegas) of each container inside a record."""
        R, n = om.shape[0], om.shape[1]
        assert om.is_cuda and om.dtype == torch.float32 and om.is_contiguous() and om.shape[2] == 85
        assert rec.dtype == torch.float32 and rec.stride(1) == 1 and rec.shape[0] >= n
        offs = (C.c_int32 * (R * 7))(*[int(o) for row in field_offsets for o in row])
        nbytes = self.lib.hmmr_smpl_workspace_bytes(R * n)
        ws = self._ws["smpl"].get(nbytes)
        L.check(self.lib.hmmr_smpl_fwd_records(C.byref(self.sc), om.data_ptr(), R, n, rec.data_ptr(), rec.stride(0), offs,
                                               ws.data_ptr(), nbytes, self._stream()), "hmmr_smpl_fwd_records")

    def groupnorm_relu(self, x, gamma, beta, groups=32, out_dtype=L.HMMR_F32, out=None):
        """x [b,t,c] fp32 -> relu(group_norm) [b,t,c] in the storage type of `out_dtype` (packing.act_to_f32 reads it); out: a tensor of
        that storage type with at least b windows, its first b are written"""
        x = self.to_device(x)
        b, t, c = x.shape
        g, be = self.to_device(gamma), self.to_device(beta)
        out = self._out(out, (b, t, c), packing.empty_act((0,), out_dtype, "cpu").dtype)
        L.check(self.lib.hmmr_groupnorm_relu(x.data_ptr(), g.data_ptr(), be.data_ptr(), b, t, c, groups,
                                             out.data_ptr(), out_dtype, self._stream()), "hmmr_groupnorm_relu")
        return out


class _FlagScope(object):
    """See HmmrEngine.flag_scope.  The flag word is per DEVICE: two scopes on one device that overlapped would read (and clear) each
    other's flags -- scope A's entry would move what B's in-flight call raised to 'carried', and B's exit would then read 0 and return
    clamped results without falling back.  So scopes of one device are serialised: a per-device re-entrant lock is held from entry
    to exit (two Testers on one device in two threads run their guarded calls one after the other; different devices do not wait for
    each other)."""
    _locks = {}
    _locks_guard = threading.Lock()

    def __init__(self, engine):
        self.engine, self.flags = engine, 0
        key = (engine.device.type, engine.device.index)
        with _FlagScope._locks_guard:
            self._lock = _FlagScope._locks.setdefault(key, threading.RLock())

    def __enter__(self):
        self._lock.acquire()
        try:
            e = self.engine
            stale = e._device_flags(True)
            if stale:
                key = (e.device.type, e.device.index)
                HmmrEngine._carried_flags[key] = HmmrEngine._carried_flags.get(key, 0) | stale
        except BaseException:
            self._lock.release()
            raise
        return self

    def __exit__(self, *exc):
        try:
            self.flags = self.engine._device_flags(True)
        finally:
            self._lock.release()
        return False


def conv_gemm(x, w_hwio, stride=1, pad=0, scale=None, shift=None, res=None, relu=False,
              scale2=None, shift2=None, in_dtype=L.HMMR_F32, out_dtype=L.HMMR_F32, tile=0,
              device="cuda:0", res_stride=1, split_k=0, pro=None, raw=False, second=None, k_order=0, n_split=0, relu_b=False):
    """Test/utility entry: run one NHWC convolution through hmmr_conv_gemm.
    x [n,h,w,cin] (numpy/torch), w_hwio [kh,kw,cin,cout].  Returns (out, out2) as float32 arrays, or with
    raw=True the device tensors in their storage type; x may itself be such a device tensor.  n_split > 0: the column split
    (hmmr_conv_desc_t.out_b) -- returns (out [.., n_split], out_b [.., cout - n_split]) with ReLU flags relu / relu_b."""
    lib = L.load()
    dev = torch.device(device)
    store = packing.DeviceStore(dev)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        xt = x.contiguous()
    else:
        xt = store.put(np.asarray(x, np.float32), packing.TORCH_DT[in_dtype])
    n, h, w_, cin = xt.shape
    kh, kw, _, cout = w_hwio.shape
    py, px = (pad, pad) if isinstance(pad, int) else pad
    ho = (h + 2 * py - kh) // stride + 1
    wo = (w_ + 2 * px - kw) // stride + 1
    x2 = None
    if second is not None:          # (x2 [n,h,w,cin2], w2 [1,1,cin2,cout]): a second 1x1 source appended along K (hmmr_conv_desc_t.in2)
        x2 = store.put(np.asarray(second[0], np.float32), packing.TORCH_DT[in_dtype])
        w_hwio = np.concatenate([np.asarray(w_hwio, np.float32), np.asarray(second[1], np.float32)], axis=2)
    wp = packing.pack_conv_weight(np.asarray(w_hwio, np.float32), k_order if k_order != 2 else 0, chunk=64 if in_dtype == L.HMMR_BF16 else 32)
    if k_order == 2 and in_dtype == L.HMMR_BF16:        # the filter stream of csrc/conv3x3_stream.hip, bf16 form
        scale = np.ones(cout, np.float32) if scale is None else scale
        shift = np.zeros(cout, np.float32) if shift is None else shift
        wt = store.put_tensor(packing.pack_conv3x3_stream(np.asarray(w_hwio, np.float32), bf16=True))
    elif k_order == 2:                                  # ... split form (as packing._layer_stream3x3)
        k = packing.row_pow2(wp[:cout])
        sc = np.ones(cout, np.float64) if scale is None else np.asarray(scale, np.float64)
        scale = (sc * np.exp2(-k.astype(np.float64))).astype(np.float32)
        shift = np.zeros(cout, np.float32) if shift is None else shift
        wt = store.put_tensor(packing.pack_conv3x3_stream(np.asarray(w_hwio, np.float32), k))      # (a 1x1 filter: pack_conv1x1_stream, the same layout)
    elif packing.TORCH_DT[in_dtype] is packing.SPLIT:   # as packing._layer: rows scaled by a power of two, undone by `scale`
        k = packing.row_pow2(wp)
        wp = packing.scale_rows(wp, k)
        sc = np.ones(wp.shape[0], np.float64)
        if scale is not None:
            sc[:len(scale)] = np.asarray(scale, np.float64)
        scale = (sc * np.exp2(-k.astype(np.float64))).astype(np.float32)
    if k_order != 2:
        wt = store.put(wp, packing.TORCH_DT[in_dtype])
    ldo = (cout + 7) // 8 * 8
    out = packing.empty_act((n, ho, wo, ldo), out_dtype, dev, zero=True)
    d = L.ConvDesc()
    d.in_, d.w, d.out = xt.data_ptr(), wt.data_ptr(), out.data_ptr()
    if x2 is not None:
        d.in2, d.cin2 = x2.data_ptr(), x2.shape[-1]
    d.scale = store.vec(scale).data_ptr() if scale is not None else None
    d.shift = store.vec(shift).data_ptr() if shift is not None else None
    out2 = None
    if scale2 is not None:
        out2 = torch.zeros_like(out)
        d.out2, d.scale2, d.shift2 = out2.data_ptr(), store.vec(scale2).data_ptr(), store.vec(shift2).data_ptr()
    if res is not None:
        rt = store.put(np.asarray(res, np.float32), packing.TORCH_DT[out_dtype])
        d.res = rt.data_ptr()
        if res_stride == 1:
            assert tuple(rt.shape) == (n, ho, wo, cout) and cout % 8 == 0
            d.ldr = cout
        else:
            d.res_strided = 1
            d.res_img_stride = rt.shape[1] * rt.shape[2] * cout
            d.res_row_stride = res_stride * rt.shape[2] * cout
            d.res_px_stride = res_stride * cout
    d.in_dtype, d.out_dtype = in_dtype, out_dtype
    d.n_img, d.hin, d.win, d.cin = n, h, w_, cin
    d.in_img_stride, d.in_row_stride, d.in_px_stride = h * w_ * cin, w_ * cin, cin
    d.kh, d.kw, d.sy, d.sx, d.py, d.px = kh, kw, stride, stride, py, px
    d.ho, d.wo, d.cout, d.ldo = ho, wo, cout, ldo
    d.relu, d.tile, d.k_order = int(relu), tile, k_order
    out_b = None
    if n_split:
        out_b = packing.empty_act((n, ho, wo, cout - n_split), out_dtype, dev, zero=True)
        d.out_b, d.ldo_b, d.n_split, d.relu_b = out_b.data_ptr(), cout - n_split, n_split, int(relu_b)
    if pro is not None:
        d.pro_scale, d.pro_shift = store.put(pro[0]).data_ptr(), store.put(pro[1]).data_ptr()
    if split_k > 1:
        nb = lib.hmmr_conv_splitk_workspace_bytes(n * ho * wo, cout, split_k)
        skws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
        d.split_k, d.ws, d.ws_bytes = split_k, skws.data_ptr(), nb
    L.check(lib.hmmr_conv_gemm(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "hmmr_conv_gemm")
    torch.cuda.synchronize(dev)
    if raw:
        return out, (out_b if n_split else out2)
    if n_split:
        return (packing.act_to_f32(out, out_dtype)[..., :n_split].cpu().numpy(), packing.act_to_f32(out_b, out_dtype).cpu().numpy())
    o = packing.act_to_f32(out, out_dtype)[..., :cout].cpu().numpy()
    o2 = packing.act_to_f32(out2, out_dtype)[..., :cout].cpu().numpy() if out2 is not None else None
    return o, o2


def bottleneck_tail(h2, w3_hwio, bias3, res, pre, w1_hwio, bn1, res_stride=1, device="cuda:0", conv2=None, shortcut=None):
    """Test/utility entry for hmmr_bottleneck_tail (bf16): h2 [n,h,w,64], w3 [1,1,64,256], res
    [n,h*s,w*s,256] (s = res_stride), pre = (scale, shift) [256], w1 [1,1,256,64], bn1 = (scale, shift) [64].
    With conv2 = (w2 [3,3,64,64], scale2, shift2) the first argument is h1 and the 3x3 conv runs inside the launch.
    Returns (trunk [n,h,w,256], h1 [n,h,w,64]) as float32 arrays of the bf16 results."""
    lib = L.load()
    dev = torch.device(device)
    store = packing.DeviceStore(dev)
    bf = torch.bfloat16
    x = store.put(np.asarray(h2, np.float32), bf)
    n, h, w_, cm = x.shape
    depth, n2 = w3_hwio.shape[3], w1_hwio.shape[3]
    w3 = store.put(packing.pack_conv_weight(np.asarray(w3_hwio, np.float32)), bf)
    w1 = store.put(packing.pack_conv_weight(np.asarray(w1_hwio, np.float32)), bf)
    rt = store.put(np.asarray(res, np.float32), bf) if res is not None else None
    out = torch.zeros((n, h, w_, depth), dtype=bf, device=dev)
    h1 = torch.zeros((n, h, w_, n2), dtype=bf, device=dev)
    d = L.TailDesc()
    d.dtype, d.m, d.c_mid, d.depth = L.HMMR_BF16, n * h * w_, cm, depth
    d.ho, d.wo = h, w_
    if conv2 is None:
        d.h2 = x.data_ptr()
    else:                                  # h2 argument is h1; conv2 = (w2_hwio [3,3,64,64], scale2, shift2)
        w2 = store.put(packing.pack_conv_weight(np.asarray(conv2[0], np.float32)), bf)
        d.h1, d.hin, d.win, d.w2 = x.data_ptr(), h, w_, w2.data_ptr()
        d.scale2, d.shift2 = store.vec(conv2[1]).data_ptr(), store.vec(conv2[2]).data_ptr()
    d.w3, d.shift3 = w3.data_ptr(), store.vec(bias3).data_ptr()
    if shortcut is not None:               # (xp [n,h,w,64], wsc [1,1,64,256], bias): the shortcut conv runs in the launch
        xp = store.put(np.asarray(shortcut[0], np.float32), bf)
        wsc = store.put(packing.pack_conv_weight(np.asarray(shortcut[1], np.float32)), bf)
        d.xp, d.wsc, d.shift_sc = xp.data_ptr(), wsc.data_ptr(), store.vec(shortcut[2]).data_ptr()
    else:
        d.res = rt.data_ptr()
    if shortcut is not None:
        pass
    elif res_stride == 1:
        d.ldr = depth
    else:
        d.res_strided, d.ho, d.wo = 1, h, w_
        d.res_img_stride = rt.shape[1] * rt.shape[2] * depth
        d.res_row_stride, d.res_px_stride = res_stride * rt.shape[2] * depth, res_stride * depth
    d.out, d.out_h1 = out.data_ptr(), h1.data_ptr()
    d.pre_scale, d.pre_shift = store.vec(pre[0]).data_ptr(), store.vec(pre[1]).data_ptr()
    d.w1, d.scale1, d.shift1, d.relu1, d.n2 = w1.data_ptr(), store.vec(bn1[0]).data_ptr(), store.vec(bn1[1]).data_ptr(), 1, n2
    L.check(lib.hmmr_bottleneck_tail(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "hmmr_bottleneck_tail")
    torch.cuda.synchronize(dev)
    return out.float().cpu().numpy(), h1.float().cpu().numpy()


def bottleneck_tail_single(h1, conv2, stride, w3_hwio, bias3, res, pre, want_raw=True, want_pre=True, device="cuda:0"):
    """Test/utility entry for the single-phase hmmr_bottleneck_tail (a block's stride-2 last unit):
    h1 [n,h,w,cm], conv2 = (w2 [3,3,cm,cm], scale2, shift2) with `stride`, w3 [1,1,cm,depth], res [n,h,w,depth]
    (sub-sampled by `stride` as the identity shortcut), pre = (scale, shift).  Returns (trunk, preact) float32."""
    lib = L.load()
    dev = torch.device(device)
    store = packing.DeviceStore(dev)
    bf = torch.bfloat16
    x = store.put(np.asarray(h1, np.float32), bf)
    n, h, w_, cm = x.shape
    ho, wo = (h + stride - 1) // stride, (w_ + stride - 1) // stride
    depth = w3_hwio.shape[3]
    w2 = store.put(packing.pack_conv_weight(np.asarray(conv2[0], np.float32)), bf)
    w3 = store.put(packing.pack_conv_weight(np.asarray(w3_hwio, np.float32)), bf)
    rt = store.put(np.asarray(res, np.float32), bf)
    out = torch.zeros((n, ho, wo, depth), dtype=bf, device=dev)
    outp = torch.zeros((n, ho, wo, depth), dtype=bf, device=dev)
    d = L.TailDesc()
    d.dtype, d.m, d.c_mid, d.depth = L.HMMR_BF16, n * ho * wo, cm, depth
    d.h1, d.hin, d.win, d.ho, d.wo, d.conv2_stride = x.data_ptr(), h, w_, ho, wo, stride
    d.w2, d.scale2, d.shift2 = w2.data_ptr(), store.vec(conv2[1]).data_ptr(), store.vec(conv2[2]).data_ptr()
    d.w3, d.shift3 = w3.data_ptr(), store.vec(bias3).data_ptr()
    d.res = rt.data_ptr()
    if stride == 1:
        d.ldr = depth
    else:
        d.res_strided = 1
        d.res_img_stride = rt.shape[1] * rt.shape[2] * depth
        d.res_row_stride, d.res_px_stride = stride * rt.shape[2] * depth, stride * depth
    if want_raw:
        d.out = out.data_ptr()
    if want_pre:
        d.out_pre, d.pre_scale, d.pre_shift = outp.data_ptr(), store.vec(pre[0]).data_ptr(), store.vec(pre[1]).data_ptr()
    L.check(lib.hmmr_bottleneck_tail(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "hmmr_bottleneck_tail")
    torch.cuda.synchronize(dev)
    return (out.float().cpu().numpy() if want_raw else None), (outp.float().cpu().numpy() if want_pre else None)


def b1_unit(h1, conv2, w3_hwio, bias3, pre, w1_hwio, bn1, res=None, shortcut=None, device="cuda:0"):
    """Test/utility entry for the whole-unit kernel of block 1 (hmmr_tail_desc_t.unit_stream, csrc/b1_unit.hip; f16x3):
    h1 [n,h,w,64] (a split device tensor or a float array), conv2 = (w2 [3,3,64,64], scale2, shift2), w3 [1,1,64,256], bias3 [256],
    pre = (scale, shift) [256], w1 [1,1,256,64], bn1 = (scale, shift) [64]; either res [n,h,w,256] (a float array: the identity
    shortcut) or shortcut = (xp [n,h,w,64], wsc [1,1,64,256], bias [256]) folded into conv3.  Returns the split device tensors
    (trunk [n,h,w,256], h1' [n,h,w,64])."""
    c = B1UnitCall(h1, conv2, w3_hwio, bias3, pre, w1_hwio, bn1, res=res, shortcut=shortcut, device=device)
    c.run()
    torch.cuda.synchronize(c.dev)
    n, h, w_ = c.grid
    return c.trunk.view(n, h, w_, 256), c.h1.view(n, h, w_, 64)


PAIR_NAN_WORD = 0x7e007e00          # two fp16 NaNs: what the guard rows / columns of a UnitPairCall's / B1UnitCall's inputs hold
PAIR_SENTINEL = 0x5a5a5a5a          # ... and what its outputs hold before the launch, valid rows included


def pack_b1_unit(conv2, w3_hwio, w1_hwio, shortcut=None):
    """The filter stream of a B1UnitCall (host work: packing.pack_b1_unit_stream of conv2 = (w2 [3,3,64,64], ...), w3 [1,1,64,256] with
    the folded shortcut's wsc = shortcut[1] appended along K, and w1 [1,1,256,64]) as a host tensor."""
    w2 = np.asarray(conv2[0], np.float32)
    w3 = np.asarray(w3_hwio, np.float32)[0, 0]                                   # [K][256]
    if shortcut is not None:
        w3 = np.concatenate([w3, np.asarray(shortcut[1], np.float32)[0, 0]], axis=0)
    k2 = packing.row_pow2(packing.pack_conv_weight(w2)[:64])
    return packing.pack_b1_unit_stream(w2, k2, w3.T, np.asarray(w1_hwio, np.float32)[0, 0].T)


class B1UnitCall(object):
    """Test/utility entry for the whole-unit kernel of block 1 (hmmr_tail_desc_t.unit_stream, csrc/b1_unit.hip; f16x3) ALONE, and for the
    three hmmr_conv_gemm launches it replaces on the same device operands: conv2 with k_order = 2 (csrc/conv3x3_stream.hip, tiles 19 /
    20), conv3 with the shortcut as `res` or as the second K source `in2`, and the fused-preact conv1.
    h1 [n,h,w,64] (a split device tensor or a float array), conv2 = (w2 [3,3,64,64], scale2, shift2), w3 [1,1,64,256], bias3 [256] or None,
    pre = (scale, shift) [256], w1 [1,1,256,64], bn1 = (scale, shift) [64]; either res [n,h,w,256] (the identity shortcut) or
    shortcut = (xp [n,h,w,64], wsc [1,1,64,256], bias [256] or None) folded into conv3.  With neither bias, shift3 = NULL.
      relu1: ReLU on h1' (else only the clamp to the fp16 range);
      res_ld > 256: the kernel reads the shortcut out of rows of res_ld elements whose extra columns hold PAIR_NAN_WORD (the three
        launches always get it contiguous);
      guard_rows: h1, xp and res are followed by that many rows of NaN halves, trunk and h1' by that many rows of PAIR_SENTINEL -- the
        valid rows of the outputs start as PAIR_SENTINEL too, not as zeros;
      stream: the device tensor of pack_b1_unit(...) if the caller has packed it already (host work);
      three_launches: build the three hmmr_conv_gemm launches instead of the unit kernel (.h2 is their intermediate);
      keep_stride: hmmr_tail_desc_t.trunk_keep_stride of the unit kernel (> 1: only the trunk rows [:, ::s, ::s] are stored).
    .descs are the descriptors run() launches (a test may edit them), .trunk [M + guard_rows, 256] / .h1 [M + guard_rows, 64] the split
    outputs as rows of pixels, .grid = (n, h, w)."""

    def __init__(self, h1, conv2, w3_hwio, bias3, pre, w1_hwio, bn1, res=None, shortcut=None, relu1=True, res_ld=0, guard_rows=0,
                 stream=None, three_launches=False, keep_stride=0, device="cuda:0"):
        self.lib = L.load()
        dev = self.dev = torch.device(device)
        store = self.store = packing.DeviceStore(dev)
        X3 = L.HMMR_F16X3

        def act(x):
            if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32:
                return x.contiguous()
            return packing.to_split(torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev))

        def guarded(x, ld=0):                                                    # [n,h,w,c] -> rows of pixels (+ NaN rows / columns)
            x = x.reshape(-1, x.shape[-1])
            m_, c = x.shape
            if not guard_rows and ld <= c:
                return x
            buf = torch.full((m_ + guard_rows, max(ld, c)), PAIR_NAN_WORD, dtype=torch.int32, device=dev)
            buf[:m_, :c] = x
            return buf

        x = act(h1)
        n, h, w_, cm = x.shape
        m = n * h * w_
        self.grid, self.m, self.guard_rows = (n, h, w_), m, guard_rows
        x = guarded(x)
        w2 = np.asarray(conv2[0], np.float32)
        k2 = packing.row_pow2(packing.pack_conv_weight(w2)[:64])
        w3 = np.asarray(w3_hwio, np.float32)[0, 0]                               # [K][256]
        w1 = np.asarray(w1_hwio, np.float32)[0, 0]                               # [256][64]
        b3 = None if bias3 is None else np.asarray(bias3, np.float64)
        xp = rt = None
        if shortcut is not None:
            assert res is None
            xp = act(shortcut[0])
            assert tuple(xp.shape) == (n, h, w_, 64), xp.shape
            xp = guarded(xp)
            w3 = np.concatenate([w3, np.asarray(shortcut[1], np.float32)[0, 0]], axis=0)
            if shortcut[2] is not None:
                b3 = np.asarray(shortcut[2], np.float64) + (0.0 if b3 is None else b3)
        else:
            rt = act(res)
            assert tuple(rt.shape) == (n, h, w_, 256), rt.shape
            rt = guarded(rt, 0 if three_launches else res_ld)
        self.inputs = (x, xp, rt)
        k3, k1 = packing.row_pow2(w3.T), packing.row_pow2(w1.T)
        sc2 = store.vec((np.asarray(conv2[1], np.float64) * np.exp2(-k2.astype(np.float64))).astype(np.float32))
        sc3 = store.vec(np.exp2(-k3.astype(np.float64)).astype(np.float32))
        sc1 = store.vec((np.asarray(bn1[0], np.float64) * np.exp2(-k1.astype(np.float64))).astype(np.float32))
        b2, b1 = store.vec(conv2[2]), store.vec(bn1[1])
        b3 = store.vec(b3.astype(np.float32)) if b3 is not None else None
        ps, pb = store.vec(pre[0]), store.vec(pre[1])
        self.trunk = torch.full((m + guard_rows, 256), PAIR_SENTINEL, dtype=torch.int32, device=dev)
        self.h1 = torch.full((m + guard_rows, 64), PAIR_SENTINEL, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if three_launches:
            self.h2 = torch.full((m + guard_rows, 64), PAIR_SENTINEL, dtype=torch.int32, device=dev)
            w2s = store.put_tensor(packing.pack_conv3x3_stream(w2, k2))
            w3p = store.put(packing.scale_rows(w3.T, k3), packing.SPLIT)         # [256][K3] rows, K-contiguous (what hmmr_conv_gemm reads)
            w1p = store.put(packing.scale_rows(w1.T, k1), packing.SPLIT)

            def desc(in_, w, scale, shift, out, cin, cout, k):
                d = L.ConvDesc()
                d.in_, d.w, d.scale, d.shift, d.out = in_.data_ptr(), w.data_ptr(), scale.data_ptr(), ptr(shift), out.data_ptr()
                d.in_dtype = d.out_dtype = X3
                d.n_img, d.hin, d.win, d.cin = n, h, w_, cin
                d.in_img_stride, d.in_row_stride, d.in_px_stride = h * w_ * cin, w_ * cin, cin
                d.kh = d.kw = k
                d.sy = d.sx = 1
                d.py = d.px = k // 2
                d.ho, d.wo, d.cout, d.ldo = h, w_, cout, cout
                return d

            c2 = desc(x, w2s, sc2, b2, self.h2, 64, 64, 3)
            c2.relu, c2.k_order = 1, 2
            c3 = desc(self.h2, w3p, sc3, b3, self.trunk, 64, 256, 1)
            if xp is not None:
                c3.in2, c3.cin2 = xp.data_ptr(), 64
            else:
                c3.res, c3.ldr = rt.data_ptr(), 256
            c1 = desc(self.trunk, w1p, sc1, b1, self.h1, 256, 64, 1)
            c1.relu, c1.pro_scale, c1.pro_shift = int(bool(relu1)), ps.data_ptr(), pb.data_ptr()
            self.descs, self._call, self._what = [c2, c3, c1], self.lib.hmmr_conv_gemm, "hmmr_conv_gemm (one of the unit's three launches)"
        else:
            if stream is None:
                stream = packing.pack_b1_unit_stream(w2, k2, w3.T, w1.T)
            self.stream = stream.to(dev)
            assert self.stream.numel() * 2 == self.lib.hmmr_b1_unit_stream_bytes(0 if xp is None else 64)
            d = L.TailDesc()
            d.dtype, d.m, d.c_mid, d.depth, d.n2 = X3, m, cm, 256, 64
            d.h1, d.hin, d.win, d.ho, d.wo = x.data_ptr(), h, w_, h, w_
            d.unit_stream = self.stream.data_ptr()
            d.scale2, d.shift2, d.scale3, d.shift3 = sc2.data_ptr(), b2.data_ptr(), sc3.data_ptr(), ptr(b3)
            if xp is not None:
                d.xp, d.c_xp = xp.data_ptr(), 64
            else:
                d.res, d.ldr = rt.data_ptr(), rt.shape[1]
            d.pre_scale, d.pre_shift = ps.data_ptr(), pb.data_ptr()
            d.scale1, d.shift1, d.relu1 = sc1.data_ptr(), b1.data_ptr(), int(bool(relu1))
            d.out, d.out_h1, d.trunk_keep_stride = self.trunk.data_ptr(), self.h1.data_ptr(), int(keep_stride)
            self.descs, self._call, self._what = [d], self.lib.hmmr_bottleneck_tail, "hmmr_bottleneck_tail (block-1 unit)"

    def run(self):
        """launch on the current stream (no synchronisation: tools time this)"""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        for d in self.descs:
            L.check(self._call(C.byref(d), st), self._what)


class UnitPairCall(object):
    """Test/utility entry for the register-resident unit pair (hmmr_tail_desc_t.pair_stream, csrc/unit_pair.hip; f16x3) ALONE, and for
    the two hmmr_conv_gemm launches it replaces (conv3 + shortcut -> trunk; fused-preact conv1 -> h1'; tile 5) on the same operands.
    Rows are pixels: h2 [M, c_mid]; either res [M, depth] (the shortcut tensor) or shortcut = (xp [M, c_xp], wsc_rows [depth][c_xp])
    folded into conv3's K; W3 [depth][c_mid] and W1 [n2][depth] as filter ROWS; bias3 [depth] or None; pre = (scale, shift) [depth];
    bn1 = (scale, shift) [n2]; relu1: ReLU on h1' (else only the clamp to the fp16 range).  Activations are float arrays / tensors or
    split device tensors.
      res_ld > depth: the pair reads the shortcut out of a buffer with rows of res_ld elements whose extra columns are NaN (the two
        launches always get it contiguous);
      guard_rows: every input is followed by that many rows of NaN halves, every output by that many rows of PAIR_SENTINEL -- and the
        valid rows of the outputs start as PAIR_SENTINEL too, not as zeros;
      stream: the device tensor of packing.pack_pair_stream([W3 | wsc_rows], W1) if the caller has packed it already (host work);
      two_launches: build the two hmmr_conv_gemm launches instead of the pair;
      grid = (h, w), keep_stride: the rows are whole h x w images and hmmr_tail_desc_t.trunk_keep_stride of the pair (> 1: only the
        trunk rows [:, ::s, ::s] are stored).
    .descs are the descriptors run() launches (a test may edit them), .trunk / .h1 the split outputs, guard rows included."""

    def __init__(self, h2, W3, bias3, pre, W1, bn1, res=None, shortcut=None, relu1=True, res_ld=0, guard_rows=0, stream=None,
                 two_launches=False, grid=None, keep_stride=0, device="cuda:0"):
        self.lib = L.load()
        dev = self.dev = torch.device(device)
        store = self.store = packing.DeviceStore(dev)
        X3 = L.HMMR_F16X3

        def rows(x):
            if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32:
                return x.contiguous()
            return packing.to_split(torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev))

        def guarded(x, ld=0):
            m_, c = x.shape
            if not guard_rows and ld <= c:
                return x
            buf = torch.full((m_ + guard_rows, max(ld, c)), PAIR_NAN_WORD, dtype=torch.int32, device=dev)
            buf[:m_, :c] = x
            return buf

        W3 = np.asarray(W3, np.float32)
        W1 = np.asarray(W1, np.float32)
        h2 = guarded(rows(h2))
        m, cm = h2.shape[0] - guard_rows, h2.shape[1]
        depth, n2 = W3.shape[0], W1.shape[0]
        assert W3.shape == (depth, cm) and W1.shape == (n2, depth), (W3.shape, W1.shape)
        xp = rt = None
        c_xp = 0
        if shortcut is not None:
            xp = guarded(rows(shortcut[0]))
            c_xp = xp.shape[1]
            W3 = np.concatenate([W3, np.asarray(shortcut[1], np.float32)], axis=1)
            assert xp.shape[0] == m + guard_rows and W3.shape == (depth, cm + c_xp)
        if res is not None:
            rt = rows(res)
            assert tuple(rt.shape) == (m, depth)
            rt = guarded(rt, 0 if two_launches else res_ld)
        self.m, self.guard_rows = m, guard_rows
        self.inputs = (h2, xp, rt)
        k3, k1 = packing.row_pow2(W3), packing.row_pow2(W1)
        sc3 = store.vec(np.exp2(-k3.astype(np.float64)).astype(np.float32))
        sc1 = store.vec((np.asarray(bn1[0], np.float64) * np.exp2(-k1.astype(np.float64))).astype(np.float32))
        b3 = store.vec(bias3) if bias3 is not None else None
        ps, pb, b1 = store.vec(pre[0]), store.vec(pre[1]), store.vec(bn1[1])
        self.trunk = torch.full((m + guard_rows, depth), PAIR_SENTINEL, dtype=torch.int32, device=dev)
        self.h1 = torch.full((m + guard_rows, n2), PAIR_SENTINEL, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        if two_launches:
            w3p = store.put(packing.scale_rows(W3, k3), packing.SPLIT)          # [depth][K3] rows, K-contiguous (what hmmr_conv_gemm reads)
            w1p = store.put(packing.scale_rows(W1, k1), packing.SPLIT)
            d = L.ConvDesc()
            d.in_, d.w, d.scale, d.shift, d.out = h2.data_ptr(), w3p.data_ptr(), sc3.data_ptr(), ptr(b3), self.trunk.data_ptr()
            d.in_dtype = d.out_dtype = X3
            d.n_img, d.hin, d.win, d.cin = 1, 1, m, cm
            d.in_img_stride, d.in_row_stride, d.in_px_stride = m * cm, m * cm, cm
            d.kh = d.kw = d.sy = d.sx = 1
            d.ho, d.wo, d.cout, d.ldo = 1, m, depth, depth
            if xp is not None:
                d.in2, d.cin2 = xp.data_ptr(), c_xp
            if rt is not None:
                d.res, d.ldr = rt.data_ptr(), depth
            d.tile = 5
            e = L.ConvDesc()
            e.in_, e.w, e.scale, e.shift, e.out = self.trunk.data_ptr(), w1p.data_ptr(), sc1.data_ptr(), b1.data_ptr(), self.h1.data_ptr()
            e.in_dtype = e.out_dtype = X3
            e.n_img, e.hin, e.win, e.cin = 1, 1, m, depth
            e.in_img_stride, e.in_row_stride, e.in_px_stride = m * depth, m * depth, depth
            e.kh = e.kw = e.sy = e.sx = 1
            e.ho, e.wo, e.cout, e.ldo = 1, m, n2, n2
            e.relu, e.pro_scale, e.pro_shift, e.tile = int(bool(relu1)), ps.data_ptr(), pb.data_ptr(), 5
            self.descs, self._call, self._what = [d, e], self.lib.hmmr_conv_gemm, "hmmr_conv_gemm (one of the pair's two launches)"
        else:
            if stream is None:
                stream = packing.pack_pair_stream(W3, W1)
            self.stream = stream.to(dev)
            assert self.stream.numel() * 2 == self.lib.hmmr_pair_stream_bytes((cm + c_xp) // 16, depth, n2)
            t = L.TailDesc()
            t.dtype, t.h2, t.m, t.c_mid, t.depth = X3, h2.data_ptr(), m, cm, depth
            t.scale3, t.shift3, t.out = sc3.data_ptr(), ptr(b3), self.trunk.data_ptr()
            if xp is not None:
                t.xp, t.c_xp = xp.data_ptr(), c_xp
            if rt is not None:
                t.res, t.ldr = rt.data_ptr(), rt.shape[1]
            t.pre_scale, t.pre_shift = ps.data_ptr(), pb.data_ptr()
            t.scale1, t.shift1, t.relu1, t.n2, t.out_h1 = sc1.data_ptr(), b1.data_ptr(), int(bool(relu1)), n2, self.h1.data_ptr()
            t.pair_stream, t.trunk_keep_stride = self.stream.data_ptr(), int(keep_stride)
            if grid is not None:
                t.ho, t.wo = grid
            self.descs, self._call, self._what = [t], self.lib.hmmr_bottleneck_tail, "hmmr_bottleneck_tail (unit pair)"

    def run(self):
        """launch on the current stream (no synchronisation: tools time this)"""
        st = torch.cuda.current_stream(self.dev).cuda_stream
        for d in self.descs:
            L.check(self._call(C.byref(d), st), self._what)


def unit_pair(h2, W3, bias3, pre, W1, bn1, **kw):
    """UnitPairCall(...) run once: the split device tensors (trunk [M + guard_rows, depth], h1' [M + guard_rows, n2])."""
    c = UnitPairCall(h2, W3, bias3, pre, W1, bn1, **kw)
    c.run()
    torch.cuda.synchronize(c.dev)
    return c.trunk, c.h1


STEM_SENTINEL_BYTE = 0x5a           # every byte of a StemCall's outputs before the launch (bf16 0x5a5a and fp32 0x5a5a5a5a are ~1.5e16)
STEM_GUARD_ROWS = 4                 # 64-channel rows of sentinel behind each output; as many image ROWS of NaN behind the input


def pack_stem(weights, dtype, device="cuda:0"):
    """(hmmr_resnet_weights_t, the DeviceStore that owns its tensors): packing.pack_resnet of a checkpoint-named dict in the shipped
    configuration -- the table a StemCall reads.  Host work; a caller with several calls on one weight set packs once."""
    store = packing.DeviceStore(torch.device(device))
    return packing.pack_resnet(weights, _dt(dtype), store), store


class StemCall(object):
    """Test/utility entry for the ResNet stem ALONE (hmmr_resnet50_stem: the launches hmmr_resnet50_fwd starts with; csrc/stem.hip or the
    three-kernel route of csrc/resnet.hip).  images [n,224,224,3] float (host or device; n may be 0), weights: a checkpoint-named dict
    (packed here with packing.pack_resnet) or packed = pack_stem(...)'s result; route / no_conv1: hmmr_debug_t.stem_route /
    stem_no_conv1 for this call only (the other switches stay as they are).
    The input buffer holds exactly the n images followed by STEM_GUARD_ROWS image rows of NaN; both outputs start as STEM_SENTINEL_BYTE
    in every byte, valid rows included, and are followed by STEM_GUARD_ROWS rows of it.  .pooled / .h1: [(n + n_zero) 56 56 +
    STEM_GUARD_ROWS, 64] in the mode's storage type (bf16, fp32, int32 split words); .h1_written after run()."""

    def __init__(self, images, weights, dtype, n_zero=0, route=0, no_conv1=0, device="cuda:0", packed=None):
        self.lib = L.load()
        dev = self.dev = torch.device(device)
        self.dtype = _dt(dtype)
        self.rw, self.store = packed if packed is not None else pack_stem(weights, self.dtype, dev)
        images = torch.as_tensor(np.asarray(images) if not isinstance(images, torch.Tensor) else images, dtype=torch.float32)
        n = self.n = int(images.shape[0])
        assert n == 0 or tuple(images.shape[1:]) == (224, 224, 3), images.shape
        self.n_zero, self.route, self.no_conv1 = int(n_zero), int(route), int(no_conv1)
        per = 224 * 224 * 3
        self.images = torch.full((n * per + STEM_GUARD_ROWS * 224 * 3,), float("nan"), dtype=torch.float32, device=dev)
        if n:
            self.images[:n * per] = images.reshape(-1).to(dev)
        td = {L.HMMR_F32: torch.float32, L.HMMR_BF16: torch.bfloat16, L.HMMR_F16X3: torch.int32}[self.dtype]
        self.rows = (n + self.n_zero) * 56 * 56
        mk = lambda: torch.full(((self.rows + STEM_GUARD_ROWS) * 64 * td.itemsize,), STEM_SENTINEL_BYTE, dtype=torch.uint8,
                                device=dev).view(td).reshape(self.rows + STEM_GUARD_ROWS, 64)
        self.pooled, self.h1 = mk(), mk()
        self.h1_written = None
        # what run() passes: a test may edit these
        self.args = dict(images=self.images.data_ptr() if n else None, n=n, n_zero=self.n_zero, pooled=self.pooled.data_ptr(),
                         h1=self.h1.data_ptr(), ws="query", ws_bytes="query")

    def run(self):
        """launch on the current stream under this call's two debug switches (no synchronisation)"""
        old, d = L.Debug(), L.Debug()
        self.lib.hmmr_get_debug(C.byref(old))
        self.lib.hmmr_get_debug(C.byref(d))
        d.stem_route, d.stem_no_conv1 = self.route, self.no_conv1
        try:
            self.lib.hmmr_set_debug(C.byref(d))
            a = dict(self.args)
            if a["ws_bytes"] == "query":
                a["ws_bytes"] = self.lib.hmmr_resnet50_stem_workspace_bytes(C.byref(self.rw), a["n"] + a["n_zero"])
            if a["ws"] == "query":
                self.ws = torch.empty(max(int(a["ws_bytes"]), 0), dtype=torch.uint8, device=self.dev) if a["ws_bytes"] else None
                a["ws"] = L.ptr(self.ws)
            written = C.c_int(-1)
            L.check(self.lib.hmmr_resnet50_stem(C.byref(self.rw), a["images"], a["n"], a["n_zero"], a["pooled"], a["h1"], C.byref(written),
                                                a["ws"], a["ws_bytes"], torch.cuda.current_stream(self.dev).cuda_stream),
                    "hmmr_resnet50_stem")
            self.h1_written = bool(written.value)
        finally:
            self.lib.hmmr_set_debug(C.byref(old))


def stem(images, weights, dtype, n_zero=0, route=0, no_conv1=0, device="cuda:0", packed=None):
    """StemCall(...) run once: (pooled, h1 or None) [n + n_zero, 56, 56, 64] as raw storage tensors (packing.from_split decodes f16x3);
    h1 is None where the schedule leaves block1/unit_1's conv1 to its own launch.  Nothing is cached between calls."""
    c = StemCall(images, weights, dtype, n_zero=n_zero, route=route, no_conv1=no_conv1, device=device, packed=packed)
    c.run()
    torch.cuda.synchronize(c.dev)
    nt = c.n + c.n_zero
    return c.pooled[:c.rows].reshape(nt, 56, 56, 64), (c.h1[:c.rows].reshape(nt, 56, 56, 64) if c.h1_written else None)
