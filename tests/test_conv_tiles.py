"""The conv tile list (csrc/conv_tiles.h) as the library exports it: hmmr_conv_tile_info (a row), hmmr_conv_tile_for (the tile a layer runs
for a tuner candidate: HmmrEngine._tile_for) and hmmr_conv_tile_fits (the rule the dispatchers of hmmr_conv_gemm ask).  Host code only."""
import ctypes as C
import json
import os
import re

import pytest

from human_dynamics_amd import _lib, assets, packing
from human_dynamics_amd import engine as E

DTYPES = (_lib.HMMR_F32, _lib.HMMR_BF16, _lib.HMMR_F16X3)


@pytest.fixture(scope="module")
def rows():
    return _lib.conv_tiles()


def _listed():
    """[(family, id, cols, rank, candidate)] of every X(...) row of csrc/conv_tiles.h, read from the source text: the lists as written, a
    row that another one would hide behind the same number included (the last five columns of every family are COLS, TUNE, RANK, CAND, text)"""
    src = open(os.path.join(os.path.dirname(E.__file__), "csrc", "conv_tiles.h")).read()
    out = []
    for fam, macro in enumerate(("HMMR_GENERIC_TILES", "HMMR_PATCH_TILES", "HMMR_S3_TILES", "HMMR_S1_TILES")):
        body = src[src.index("#define %s(X)" % macro):]
        body = body[:body.index("\n\n")]
        for m in re.finditer(r"^\s*X\(([^\"]*),\s*\"", body, re.M):
            c = [int(v) for v in m.group(1).split(",")]
            out.append((fam, c[0], c[-4], c[-2], c[-1]))
    return out


def test_the_table_is_well_formed(rows):
    listed = _listed()
    ids = [t for _, t, _, _, _ in listed]
    assert len(ids) >= 28 and len(ids) == len(set(ids)), sorted(ids)          # unique over all four lists: no id in two families
    assert 1 <= min(ids) and max(ids) <= _lib.CONV_TILE_MAX and 4 not in ids
    assert "#define HMMR_CONV_TILE_MAX %d " % _lib.CONV_TILE_MAX in open(os.path.join(os.path.dirname(os.path.dirname(E.__file__)), "include", "hmmr_hip.h")).read()
    # the library returns exactly the rows that are written, each under its own family, rank and candidate
    assert sorted((r.family, r.tile, r.cols, r.rank, r.candidate) for r in rows) == sorted(listed)
    for fam in range(4):
        of = [x for x in listed if x[0] == fam]
        assert of and [x[1] for x in of] == [r.tile for r in _lib.conv_tiles(fam)]
        ranks = sorted(x[3] for x in of if x[3])
        assert ranks == list(range(1, len(ranks) + 1)), (fam, ranks)       # unique, and 1 .. n: the choice tries them in this order
        for narrow in (False, True):
            cands = [x[4] for x in of if x[4] and (x[2] == 64) == narrow]
            assert len(cands) == len(set(cands)), (fam, narrow, cands)      # a tuner candidate maps to at most one tile of a class
    for r in rows:
        assert r.pixels == 32 * r.wgm * r.fm and r.channels == 32 * r.wgn * r.fn and r.row_blocks * 32 == r.pixels, r.tile
        assert r.narrow == (r.cols == 64) and r.cols in (0, 64, 128, 256) and r.text
        assert not r.tune_cols or not r.cols or r.tune_cols % r.cols == 0    # the tuner's rule is never laxer where it has one
        if r.family in (_lib.TILE_STREAM_3X3, _lib.TILE_STREAM_1X1):
            assert r.wgm * r.wgn == 4 and r.channels == (64 if r.narrow else 128), r.tile       # one wave per SIMD
    assert _lib.load().hmmr_conv_tile_f_movie() == 8


def test_numbers_that_are_no_tile_are_refused():
    lib = _lib.load()
    r = _lib.ConvTileInfo()
    for t in (0, 4, 30, -1):                # (4 is a candidate of the tuner, not a tile)
        assert lib.hmmr_conv_tile_info(t, C.byref(r)) == -1 and b"no tile" in lib.hmmr_last_error(), t
    assert lib.hmmr_conv_tile_info(12, None) == -1
    assert lib.hmmr_conv_tile_info(12, C.byref(r)) == 0 and (r.tile, r.family, r.pixels) == (12, _lib.TILE_STREAM_3X3, 448)


def _layers(rw):
    """(unit, name, the hmmr_layer_t the launch reads, cout, image width, K steps of 16 channels) of every conv launch of the ResNet,
    from the unit table alone (slim resnet_v2: 56 x 56 behind the stem, a block's last unit strides)"""
    h = 56
    for u in range(_lib.RESNET_UNITS):
        U = rw.unit[u]
        for nm in (["shortcut"] if U.shortcut.w else []) + ["conv1", "conv2", "conv3"]:
            lay = U.c3sc if (nm == "conv3" and U.c3sc.w) else getattr(U, nm)
            cout = U.depth + U.base if (nm == "shortcut" and U.sc_c1.w) else (U.base if nm in ("conv1", "conv2") else U.depth)
            cin = U.base + (U.c_in if U.c3sc.w else 0) if nm == "conv3" else U.base if nm == "conv2" else U.c_in
            yield u, nm, lay, cout, (h // U.stride if nm == "conv3" else h), cin // 16
        h //= U.stride


PACKINGS = [{}, dict(unit_pair=False), dict(stream_1x1=False), dict(b1_unit=False), dict(patch_3x3=1)]


@pytest.mark.parametrize("kw", PACKINGS, ids=["shipped"] + ["%s=%s" % kv for p in PACKINGS[1:] for kv in p.items()])
def test_what_tile_for_returns_the_library_accepts(kw):
    """Closure: for every layer of the synthetic ResNet, in the three operand modes, and every candidate 0 .. 40, a non-zero
    hmmr_conv_tile_for passes the fit rule of the layer's dispatcher with the layer's real cout, image width and K steps."""
    lib = _lib.load()
    ws = assets.make_synthetic_weights(0)
    seen = set()
    for dt in DTYPES:
        rw = packing.pack_resnet(ws, dt, packing.DeviceStore("cpu"), **kw)
        for u, nm, lay, cout, win, ksteps in _layers(rw):
            for cand in range(41):
                tile = E.HmmrEngine._tile_for(lay, cand, cout, dt, nm)
                assert tile == lib.hmmr_conv_tile_for(lay.k_order, int(nm != "conv2"), int(nm == "conv3"), cout, dt, cand)
                if tile:
                    rc = lib.hmmr_conv_tile_fits(tile, lay.k_order, int(nm != "conv2"), int(nm == "conv3"), cout, dt, win, ksteps)
                    assert rc == 0, (dt, u, nm, cand, tile, lib.hmmr_last_error())
                    seen.add(tile)
    assert {1, 2, 3, 5, 6, 7, 8} <= seen          # every packing keeps generic layers
    if not kw:
        assert {12, 13, 15, 16, 21, 27, 28, 24, 25, 26, 22, 29} <= seen, sorted(seen)


def test_the_fit_rule_names_the_tile_and_the_reason():
    lib = _lib.load()
    X3, BF = _lib.HMMR_F16X3, _lib.HMMR_BF16
    fits = lambda *a: (lib.hmmr_conv_tile_fits(*a), lib.hmmr_last_error())
    assert fits(13, 2, 0, 0, 256, X3, 28, 0)[0] == 0 and fits(13, 2, 0, 0, 0, -1, 0, 0)[0] == 0         # 0 / -1: not known, not checked
    for args, words in (((13, 2, 0, 0, 256, X3, 56, 0), (b"tile 13", b"28 pixels")), ((13, 2, 0, 0, 64, X3, 28, 0), (b"tile 13", b"cout")),
                        ((19, 2, 0, 0, 128, X3, 28, 0), (b"tile 19", b"cout = 64")), ((21, 2, 0, 0, 256, BF, 14, 0), (b"tile 21", b"split")),
                        ((11, 1, 0, 0, 256, BF, 14, 0), (b"tile 11", b"split")), ((10, 1, 0, 0, 128, X3, 14, 0), (b"tile 10", b"256")),
                        ((8, 0, 0, 0, 128, X3, 0, 0), (b"tile 8", b"256")), ((9, 0, 0, 0, 128, X3, 0, 0), (b"1 .. 3, 5 .. 8", b"not 9")),
                        ((5, 2, 0, 0, 256, X3, 14, 0), (b"12 .. 21, 27, 28", b"not 5")), ((12, 2, 1, 0, 256, X3, 14, 16), (b"22 .. 26, 29", b"not 12")),
                        ((22, 2, 1, 1, 2048, X3, 7, 32), (b"tile 22", b"conv3 form")), ((22, 2, 1, 0, 512, X3, 7, 4), (b"at least 96", b"tile 22")),
                        ((4, 0, 0, 0, 256, X3, 0, 0), (b"not 4",)), ((0, 1, 0, 0, 256, X3, 0, 0), (b"9 .. 11", b"not 0"))):
        rc, msg = fits(*args)
        assert rc == -1 and all(w in msg for w in words), (args, msg)
    assert fits(1, 0, 0, 0, 72, X3, 0, 0)[0] == 0 and lib.hmmr_conv_tile_for(0, 0, 0, 72, X3, 1) == 0      # the tuner's rule is the stricter one here
    assert fits(24, 2, 1, 1, 2048, X3, 7, 4)[0] == 0
    assert all(fits(t, k, 0, 0, -64, X3, 0, 0)[0] == -1 for t, k in ((8, 0), (9, 1), (10, 1), (11, 1)))       # only 0 is "not known"


def test_shipped_tables_name_rows_of_their_layers_family(rows):
    by_id = {r.tile: r for r in rows}
    tabs = json.load(open(os.path.join(os.path.dirname(E.__file__), "tile_tables.json")))
    ws = assets.make_synthetic_weights(0)
    n = 0
    for dt in DTYPES:
        rw = packing.pack_resnet(ws, dt, packing.DeviceStore("cpu"))
        layers = {(u, nm): lay for u, nm, lay, _, _, _ in _layers(rw)}
        for key, tab in tabs.items():
            if key.startswith("_") or int(key.split(":")[0]) != dt:
                continue
            for lk, tile in tab.items():
                lay = layers[(int(lk.split(":")[0]), lk.split(":")[1])]
                fam = (_lib.TILE_STREAM_1X1 if lk.split(":")[1] != "conv2" else _lib.TILE_STREAM_3X3) if lay.k_order == 2 else lay.k_order
                assert tile == 0 or (tile in by_id and by_id[tile].family == fam), (key, lk, tile)
                n += tile != 0
    assert n > 100
