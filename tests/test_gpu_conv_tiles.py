"""Every value of hmmr_conv_desc_t.tile on the GPU, enumerated from the tile list (hmmr_conv_tile_info, csrc/conv_tiles.h): on the smallest
problems that still cross a tile edge -- 49 pixels (less than one tile of any shape, ragged) and 588 or 784 (one more than the largest
tile's pixels, rounded up to whole images) -- a tile the fit rule accepts gives the bits of the library's own choice (every tile of a
family accumulates in the same order), and a tile it refuses makes hmmr_conv_gemm return -1 with nothing launched."""
import numpy as np
import pytest

from human_dynamics_amd import _lib as L

pytestmark = pytest.mark.gpu
F32, BF, X3 = L.HMMR_F32, L.HMMR_BF16, L.HMMR_F16X3

PROBLEMS = [
    # name, k_order, filter, dtype, (n, h, w), cin, cout, dense res (the 1x1 stream kernel's conv3 form)
    ("s3_split_49", 2, 3, X3, (1, 7, 7), 32, 128, False),
    ("s3_split_588", 2, 3, X3, (3, 14, 14), 32, 128, False),
    ("s3_bf16_49", 2, 3, BF, (1, 7, 7), 64, 128, False),
    ("s3_bf16_588", 2, 3, BF, (3, 14, 14), 64, 128, False),
    ("s3_narrow_split_49", 2, 3, X3, (1, 7, 7), 32, 64, False),
    ("s3_narrow_split_784", 2, 3, X3, (1, 28, 28), 32, 64, False),
    ("s3_narrow_bf16_784", 2, 3, BF, (1, 28, 28), 64, 64, False),
    ("s1_49", 2, 1, X3, (1, 7, 7), 128, 128, False),
    ("s1_588", 2, 1, X3, (3, 14, 14), 128, 128, False),
    ("s1_c3_49", 2, 1, X3, (1, 7, 7), 128, 128, True),
    ("s1_c3_588", 2, 1, X3, (3, 14, 14), 128, 128, True),
    ("patch_49", 1, 3, X3, (1, 7, 7), 32, 256, False),
    ("patch_588", 1, 3, X3, (3, 14, 14), 32, 256, False),
    ("generic_f32_49", 0, 1, F32, (1, 7, 7), 64, 256, False),
    ("generic_f32_588", 0, 1, F32, (3, 14, 14), 64, 256, False),
    ("generic_split_49", 0, 1, X3, (1, 7, 7), 64, 256, False),
    ("generic_split_588", 0, 1, X3, (3, 14, 14), 64, 256, False),
]


@pytest.mark.parametrize("problem", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_every_tile_on_a_problem_that_crosses_its_edge(problem, gpu_device):
    from human_dynamics_amd.engine import conv_gemm
    name, k_order, filt, dt, (n, h, w_), cin, cout, with_res = problem
    lib = L.load()
    rows = L.conv_tiles()
    assert len(rows) >= 28
    rng = np.random.default_rng(len(name) + 31 * cin + cout)
    x = rng.normal(size=(n, h, w_, cin)).astype(np.float32)
    w = (rng.normal(size=(filt, filt, cin, cout)) / np.sqrt(filt * filt * cin)).astype(np.float32)
    kw = dict(stride=1, pad=filt // 2, scale=rng.uniform(0.5, 1.5, cout).astype(np.float32), shift=rng.normal(size=cout).astype(np.float32),
              relu=True, in_dtype=dt, out_dtype=dt, device=gpu_device, k_order=k_order)
    if with_res:
        kw["res"] = rng.normal(size=(n, h, w_, cout)).astype(np.float32)
    fam = {0: L.TILE_GENERIC, 1: L.TILE_PATCH}.get(k_order, L.TILE_STREAM_1X1 if filt == 1 else L.TILE_STREAM_3X3)
    largest = max(r.pixels for r in rows if r.family == fam and r.narrow == (cout == 64))
    assert n * h * w_ == 49 or n * h * w_ > largest          # ragged inside one tile, or past the edge of the largest
    ref = conv_gemm(x, w, tile=0, **kw)[0]
    assert np.abs(ref).max() > 0.1
    ran = 0
    for r in rows:
        fits = lib.hmmr_conv_tile_fits(r.tile, k_order, int(filt == 1), int(with_res), cout, dt, w_, cin // 16) == 0
        if fits:
            out = conv_gemm(x, w, tile=r.tile, **kw)[0]
            assert np.array_equal(out, ref), "%s: tile %d differs from the library's choice" % (name, r.tile)
            ran += 1
        else:
            before = L.launch_counts()
            with pytest.raises(L.HmmrError, match=r"failed \(-1\)"):
                conv_gemm(x, w, tile=r.tile, **kw)
            assert L.launch_counts() == before, "%s: refused tile %d was counted as launched" % (name, r.tile)
    assert ran >= 2, (name, ran)
