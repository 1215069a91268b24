// hmmr_conv_desc_t.tile, stated once: what every number means, which problems may take it, when the library picks it for tile = 0 and
// which candidate of the tuner maps onto it.  The four dispatchers (gemm_conv.hip: launch_tiled, launch_patch_tiled; conv3x3_stream.hip;
// conv1x1_stream.hip) expand these lists into their switches, hmmr_conv_tile_info / hmmr_conv_tile_for (api.cpp) export them, and
// HmmrEngine._tile_for, the tests and the tools read them through those two calls.  A new tile shape is ONE new row.
// No HIP include and no HIP call: the file compiles alone with a host compiler (tools/tile_choice_check.cpp does).
#pragma once
#include <stdio.h>

#include "hmmr_hip.h"

// ---- the lists.  Columns every family shares, after its template arguments:
//   COLS  output columns the tile needs: 0 = any, 64 = exactly 64, otherwise cout % COLS == 0 (filter rows are padded to 128)
//   TUNE  HmmrEngine's tuner (hmmr_conv_tile_for) is offered the tile only when cout % TUNE == 0 (0 = at any cout).  Stricter than COLS
//         for the generic tiles 1 / 5 / 7, which hmmr_conv_gemm launches on a ragged cout too: a 128-column tile there is never the fast one
//   RANK  place among the library's own candidates for tile = 0 (1 = tried first: it wins a tie); 0 = never chosen by the library
//   CAND  the tuner candidate (devflags TUNE_TILES) that maps onto the tile; 0 = none, the tile is reached by its own number only

// generic implicit GEMM (k_order 0; conv_gemm_kernel): X(id, BM, BN, waves along M, waves along N, LDS stages, COLS, TUNE, RANK, CAND, text)
#define HMMR_GENERIC_TILES(X)                                                                                                         \
    X(1, 128, 128, 2, 2, 2, 0, 128, 0, 1, "128x128, 4 waves of 64x64")                                                                \
    X(2, 128, 64, 2, 2, 2, 0, 0, 0, 2, "128x64, 4 waves of 64x32")                                                                    \
    X(3, 64, 64, 2, 2, 2, 0, 0, 3, 3, "64x64, 4 waves of 32x32")                                                                      \
    X(5, 128, 128, 4, 2, 2, 0, 128, 1, 5, "128x128, 8 waves of 32x64, two workgroups per CU")                                         \
    X(6, 128, 64, 4, 2, 2, 0, 0, 2, 6, "128x64, 8 waves of 32x32, two workgroups per CU")                                             \
    /* deep ring + ping-pong wave groups, one 8-wave workgroup per CU (256 VGPRs per lane).  128x128 and 256x64 variants of this   */ \
    /* structure were measured 15-40 % slower than tiles 5 / 6 on every ResNet shape and are not instantiated                      */ \
    X(7, 256, 128, 4, 2, 3, 0, 128, 0, 7, "256x128, 8 waves of 64x64, 3-stage ring, ping-pong wave groups")                           \
    X(8, 128, 256, 2, 4, 3, 256, 256, 0, 8, "128x256, likewise: half the A rows, half the fused-preact work per MFMA; the faster 3x3 tile")

// 3x3 patch kernels (k_order 1; conv3x3_patch_kernel, PIPE: conv3x3_pipe_kernel, split operands only):
// X(id, BM, BN, waves along M, waves along N, PIPE, COLS, TUNE, RANK, CAND, text).  The patch depth NPP follows the image (launch_patch_tiled).
// RANK: the 256x128 ping-pong tile -- inside the network the tuner prefers it to tile 11 on ten layers of eleven (profiles/r03p); tile 10
// needs 256 output columns and a narrower image
#define HMMR_PATCH_TILES(X)                                                                                                           \
    X(9, 256, 128, 4, 2, 0, 128, 128, 1, 7, "256x128, the structure of tile 7 with the A operand out of an input patch")              \
    X(10, 128, 256, 2, 4, 0, 256, 256, 0, 8, "128x256, the structure of tile 8 likewise")                                             \
    X(11, 256, 128, 4, 2, 1, 128, 128, 0, 0, "256x128 without a load segment: two fragment sets per wave, one barrier per K step")

// 3x3 stream kernel (k_order 2; conv3x3_stream_kernel: 4 waves, one per SIMD, wave tile FM x FN accumulators of 32 x 32):
// X(id, FM, FN, WGM, WGN, widest image, split only, COLS, TUNE, RANK, CAND, text).  TUNE 0: the tuner's class is "cout == 64 or not" alone.
// Split only: with two MFMAs per step the bf16 form has no room for the tile's fragment reads.
#define HMMR_S3_TILES(X)                                                                                                              \
    X(12, 7, 2, 2, 2, 28, 0, 128, 0, 1, 8, "448 pixels, waves 2 x 2")                                                                 \
    X(13, 4, 2, 2, 2, 28, 0, 128, 0, 2, 5, "256 pixels, waves 2 x 2")                                                                 \
    X(14, 8, 2, 2, 2, 28, 0, 128, 0, 0, 6, "512 pixels, waves 2 x 2")                                                                 \
    X(15, 6, 2, 2, 2, 28, 0, 128, 0, 3, 3, "384 pixels, waves 2 x 2")                                                                 \
    X(16, 5, 2, 2, 2, 28, 0, 128, 0, 4, 1, "320 pixels, waves 2 x 2")                                                                 \
    X(17, 4, 4, 4, 1, 28, 0, 128, 0, 0, 2, "512 pixels, the waves split the pixels")                                                  \
    X(18, 3, 4, 4, 1, 28, 0, 128, 0, 0, 7, "384 pixels, the waves split the pixels")                                                  \
    X(19, 5, 2, 4, 1, 56, 0, 64, 0, 8, 5, "640 pixels x 64 channels")                                                                 \
    X(20, 4, 2, 4, 1, 56, 0, 64, 0, 9, 6, "512 pixels x 64 channels")                                                                 \
    X(21, 7, 1, 1, 4, 28, 1, 128, 0, 5, 11, "224 pixels, every wave all of them and 32 of the 128 channels")                          \
    /* 128- and 192-pixel tiles for SHORT launches -- at the reference's own batch sizes, 64 frames of FeatureExtractor            */ \
    /* and the 160 of Tester.predict, blocks 3-4 are 98 - 245 row blocks: 56 - 140 workgroups of the 224-pixel tile on 256 CUs     */ \
    X(27, 2, 2, 2, 2, 28, 1, 128, 0, 6, 4, "128 pixels, waves 2 x 2: short launches")                                                 \
    X(28, 3, 2, 2, 2, 28, 1, 128, 0, 7, 9, "192 pixels, waves 2 x 2: short launches")

// 1x1 stream kernel (k_order 2 with a 1x1 filter; conv1x1_stream_kernel: 4 waves, one per SIMD, both operands through LDS rings D deep):
// X(id, FM, FN, WGM, WGN, D, workgroups per CU, has a conv3 form, COLS, TUNE, RANK, CAND, text).  The conv3 form's epilogue tiles live in
// the idle rings: a 128-pixel tile's are too small, the 7 x 1 / 8 x 1 wave tiles have none.
#define HMMR_S1_TILES(X)                                                                                                              \
    X(22, 7, 1, 1, 4, 6, 1, 0, 128, 0, 4, 5, "224 pixels, every wave all of them and 32 of the 128 channels")                         \
    X(23, 8, 1, 1, 4, 6, 1, 0, 128, 0, 5, 6, "256 pixels, likewise")                                                                  \
    X(24, 7, 2, 2, 2, 4, 1, 1, 128, 0, 2, 3, "448 pixels, waves 2 x 2")                                                               \
    X(25, 4, 2, 2, 2, 6, 1, 1, 128, 0, 1, 1, "256 pixels, waves 2 x 2")                                                               \
    X(26, 4, 2, 2, 2, 3, 2, 1, 128, 0, 3, 2, "256 pixels, waves 2 x 2, TWO workgroups per CU (rings 3 deep, 256 registers per wave)") \
    /* short launches: block 4's conv1 at 64 frames is 98 row blocks x 4 channel tiles, 52 workgroups of tile 25                  */ \
    X(29, 2, 2, 2, 2, 6, 1, 0, 128, 0, 6, 4, "128 pixels, waves 2 x 2: short launches")

// the tile packing.py and pack.cpp give the f_movie convolutions of a split model: the 128x256 ping-pong tile with 5 K slices
// (csrc/temporal.hip; tools/stage_bench.py, 32 windows: 0.51 -> 0.43 ms per f_movie pass)
#define HMMR_TILE_F_MOVIE 8

// ---- the table: one hmmr_conv_tile_info_t (include/hmmr_hip.h) per row; pixels, channels, row blocks and "narrow" follow from the arguments
namespace conv_tiles {

constexpr hmmr_conv_tile_info_t make_row(int id, int family, int fm, int fn, int wgm, int wgn, int depth, int occ, int wmax, int split_only,
                                         int conv3_form, int cols, int tune, int rank, int cand, const char* text) {
    return {id, family, fm, fn, wgm, wgn, 32 * wgm * fm, 32 * wgn * fn, wgm * fm, depth, occ, wmax, split_only, conv3_form, cols, tune, cols == 64, rank, cand, text};
}

constexpr hmmr_conv_tile_info_t kRows[] = {
#define X(ID, BM, BN, WGM, WGN, NSTAGE, COLS, TUNE, RANK, CAND, TEXT) \
    make_row(ID, HMMR_TILE_GENERIC, BM / (32 * WGM), BN / (32 * WGN), WGM, WGN, NSTAGE, NSTAGE >= 3 ? 1 : 2, 0, 0, 0, COLS, TUNE, RANK, CAND, TEXT),
    HMMR_GENERIC_TILES(X)
#undef X
#define X(ID, BM, BN, WGM, WGN, PIPE, COLS, TUNE, RANK, CAND, TEXT) \
    make_row(ID, HMMR_TILE_PATCH, BM / (32 * WGM), BN / (32 * WGN), WGM, WGN, 3, 1, 0, PIPE, 0, COLS, TUNE, RANK, CAND, TEXT),
    HMMR_PATCH_TILES(X)
#undef X
#define X(ID, FM, FN, WGM, WGN, WMAX, SPLIT_ONLY, COLS, TUNE, RANK, CAND, TEXT) \
    make_row(ID, HMMR_TILE_STREAM_3X3, FM, FN, WGM, WGN, 0, 1, WMAX, SPLIT_ONLY, 0, COLS, TUNE, RANK, CAND, TEXT),
    HMMR_S3_TILES(X)
#undef X
#define X(ID, FM, FN, WGM, WGN, D, OCC, C3, COLS, TUNE, RANK, CAND, TEXT) \
    make_row(ID, HMMR_TILE_STREAM_1X1, FM, FN, WGM, WGN, D, OCC, 0, 0, C3, COLS, TUNE, RANK, CAND, TEXT),
    HMMR_S1_TILES(X)
#undef X
};
constexpr int kCount = (int)(sizeof(kRows) / sizeof(kRows[0]));

// what a row added by mistake breaks, refused at compile time: a number outside 1 .. HMMR_CONV_TILE_MAX or used twice (in one family or in
// two: row() would hide the second), a rank used twice in a family or a gap in its ranks (the choices walk 1 .. n), a tuner candidate
// with two tiles in one (family, narrow) class
constexpr bool well_formed() {
    for (int i = 0; i < kCount; ++i) {
        const auto& a = kRows[i];
        if (a.tile < 1 || a.tile > HMMR_CONV_TILE_MAX || a.rank < 0 || a.candidate < 0) return false;
        int ranked_rows = 0;
        for (int j = 0; j < kCount; ++j) {
            const auto& b = kRows[j];
            if (b.family == a.family && b.rank > 0) ++ranked_rows;
            if (i == j) continue;
            if (a.tile == b.tile) return false;
            if (a.family != b.family) continue;
            if (a.rank && a.rank == b.rank) return false;
            if (a.candidate && a.candidate == b.candidate && a.narrow == b.narrow) return false;
        }
        if (a.rank > ranked_rows) return false;
    }
    return true;
}
static_assert(well_formed(), "conv_tiles.h: a tile number, a rank or a tuner candidate is used twice, or a number is out of range");

inline const hmmr_conv_tile_info_t* row(int tile) {
    for (const auto& r : kRows)
        if (r.tile == tile) return &r;
    return nullptr;
}

// kRows' indices of one family in RANK order (rank 0 left out); n = how many
struct Ranked { int idx[kCount]; int n; };
constexpr Ranked ranked(int family) {
    Ranked o = {};
    for (int rank = 1; rank <= kCount; ++rank)
        for (int i = 0; i < kCount; ++i)
            if (kRows[i].family == family && kRows[i].rank == rank) o.idx[o.n++] = i;
    return o;
}

// the numbers of a family's tiles (narrow: -1 = all, 0 / 1 = that class) as the error texts name them: "12 .. 18, 21, 27, 28"
inline const char* list(int family, int narrow, char* buf, size_t n) {
    size_t at = 0;
    buf[0] = 0;
    for (int t = 1, end = 0; t <= HMMR_CONV_TILE_MAX; t = end + 1) {
        const auto in = [&](int id) { const auto* r = row(id); return r && r->family == family && (narrow < 0 || r->narrow == narrow); };
        end = t;
        if (!in(t)) continue;
        while (in(end + 1)) ++end;
        const int w = snprintf(buf + at, n - at, end >= t + 2 ? "%s%d .. %d" : end > t ? "%s%d, %d" : "%s%d", at ? ", " : "", t, end);
        if (w < 0 || (size_t)w >= n - at) break;
        at += (size_t)w;
    }
    return buf;
}

// ---- one fit rule.  0 in cout / win / ksteps and a negative dtype mean "not known, not checked".
struct Problem {
    int k_order;        // hmmr_conv_desc_t.k_order
    int filter_1x1;     // kh = kw = 1 (read with k_order 2: which of the two stream kernels)
    int conv3_form;     // the 1x1 stream's launch has res / out2 / in2
    int cout;
    int dtype;          // of the operands: HMMR_F32 / HMMR_BF16 / HMMR_F16X3
    int win;            // image width in pixels
    int ksteps;         // K steps of the 1x1 stream kernel: (cin + cin2) / 16
};
inline int family_of(int k_order, int filter_1x1) {
    return k_order == 2 ? (filter_1x1 ? HMMR_TILE_STREAM_1X1 : HMMR_TILE_STREAM_3X3) : k_order ? HMMR_TILE_PATCH : HMMR_TILE_GENERIC;
}
inline const char* family_name(int family) {
    static const char* const name[] = {"k_order 0", "k_order 1", "k_order 2", "k_order 2 (1x1)"};
    return name[family];
}

// does `tile` (a row's number, not 0) take the problem?  0, or -1 with the reason in `why`
inline int fit(int tile, const Problem& p, char* why, size_t n) {
    const int fam = family_of(p.k_order, p.filter_1x1);
    const hmmr_conv_tile_info_t* t = row(tile);
    char ids[96];
    if (!t || t->family != fam) {
        snprintf(why, n, "%s runs tiles %s, not %d", family_name(fam), list(fam, -1, ids, sizeof ids), tile);
        return -1;
    }
    if (p.cout != 0 && (t->cols == 64 ? p.cout != 64 : t->cols && p.cout % t->cols)) {
        snprintf(why, n, "%s, tile %d (%s) needs cout %s %d, not %d (filter rows are padded to 128)", family_name(fam), tile, t->text,
                 t->cols == 64 ? "=" : "a multiple of", t->cols, p.cout);
        return -1;
    }
    if (t->split_only && p.dtype >= 0 && p.dtype != HMMR_F16X3) {
        snprintf(why, n, "%s, tile %d (%s) is built for split (f16x3) operands", family_name(fam), tile, t->text);
        return -1;
    }
    if (t->wmax && p.win > t->wmax) {
        snprintf(why, n, "%s, tile %d takes images up to %d pixels wide, not %d", family_name(fam), tile, t->wmax, p.win);
        return -1;
    }
    if (p.conv3_form && fam == HMMR_TILE_STREAM_1X1 && !t->conv3_form) {
        snprintf(why, n, "%s: tile %d (%s) has no conv3 form (res / out2 / in2)", family_name(fam), tile, t->text);
        return -1;
    }
    if (fam == HMMR_TILE_STREAM_1X1 && p.ksteps > 0 && p.ksteps < t->depth) {
        snprintf(why, n, "%s: cin must be at least %d channels for tile %d (rings %d K steps deep)", family_name(fam), 16 * t->depth, tile, t->depth);
        return -1;
    }
    return 0;
}

// ---- the tile a layer of that kind runs for a tuner candidate or a literal tile number; 0 (the library's choice) where nothing fits.
// HmmrEngine._tile_for's contract: never an error, and the tuner's own offer rule (TUNE), not the library's (COLS).  A 3x3 stream layer's
// class is "64 columns or not"; a bf16 engine is not offered the split-only tiles (an fp32 engine packs no layer of their families).
inline int tile_for(int k_order, int filter_1x1, int conv3_form, int cout, int dtype, int candidate) {
    const int fam = family_of(k_order, filter_1x1);
    const int narrow = fam == HMMR_TILE_STREAM_3X3 && cout == 64;
    const hmmr_conv_tile_info_t* t = nullptr;
    for (const auto& r : kRows)
        if (candidate > 0 && r.family == fam && r.narrow == narrow && r.candidate == candidate) { t = &r; break; }
    if (!t) t = row(candidate);
    if (!t || t->family != fam || t->narrow != narrow) return 0;
    if (t->split_only && dtype == HMMR_BF16) return 0;
    if (conv3_form && fam == HMMR_TILE_STREAM_1X1 && !t->conv3_form) return 0;
    if (t->tune_cols && cout % t->tune_cols) return 0;
    return t->tile;
}

// ---- the library's own choice for tile = 0: a family's rows in RANK order, the first of equal cost wins (strict <).  What is not a
// property of a tile shape -- the measured cost terms -- is written here, next to its measurement, not in the lists.

// generic: measured on the ResNet-50 shapes at batch 256 (tools/conv_bench.py): 8-wave workgroups (4 waves per SIMD at 2 workgroups per
// CU) beat 4-wave ones by 5-20 %, and a tile count of ~1.5x the CU count with 128x128 tiles beats twice as many 128x64 tiles.  A row is
// taken when it yields at least 192 workgroups -- a 128-column one only where cout fills whole tiles of it (the library's own condition,
// written here and not read from the tuner's TUNE column) --; the last one in any case.
inline int choose_generic(long long M, int cout, int slices) {
    constexpr Ranked rk = ranked(HMMR_TILE_GENERIC);
    for (int i = 0; i + 1 < rk.n; ++i) {
        const auto& r = kRows[rk.idx[i]];
        const long long tiles = ((M + r.pixels - 1) / r.pixels) * ((cout + r.channels - 1) / r.channels);
        const bool whole = r.channels < 128 || (cout >= r.channels && cout % r.channels == 0);
        if (whole && tiles * slices >= 192) return r.tile;
    }
    return kRows[rk.idx[rk.n - 1]].tile;
}

inline int choose_patch() { return kRows[ranked(HMMR_TILE_PATCH).idx[0]].tile; }

// both stream kernels: fewest rounds of 256 workgroups x (row blocks per tile + ~1.5 for a tile's prologue and epilogue)
inline int choose_s3(long long M, int cout, bool split) {
    constexpr Ranked rk = ranked(HMMR_TILE_STREAM_3X3);
    const int narrow = cout == 64;
    const long long rbs = (M + 31) / 32, nts = narrow ? 1 : cout / 128;
    int tile = 0;
    double best = 0;
    for (int i = 0; i < rk.n; ++i) {
        const auto& r = kRows[rk.idx[i]];
        if (r.narrow != narrow || (r.split_only && !split)) continue;
        const long long tiles = ((rbs + r.row_blocks - 1) / r.row_blocks) * nts;
        const double cost = (double)((tiles + 255) / 256) * (r.row_blocks + 1.5);
        if (!tile || cost < best) { tile = r.tile; best = cost; }
    }
    return tile;
}

// nk: K steps; c3: the conv3 form.  0 where no ring is shallow enough for nk.
inline int choose_s1(long long M, int cout, int nk, bool c3) {
    constexpr Ranked rk = ranked(HMMR_TILE_STREAM_1X1);
    const long long rbs = (M + 31) / 32, tiles_n = cout / 128;
    int tile = 0;
    double best = 0;
    for (int i = 0; i < rk.n; ++i) {
        const auto& r = kRows[rk.idx[i]];
        if (nk < r.depth || (c3 && !r.conv3_form)) continue;
        const long long tiles = ((rbs + r.row_blocks - 1) / r.row_blocks) * tiles_n;
        // the 7 x 1 / 8 x 1 wave tiles read 16-18 fragments per 21-24 MFMAs and pay ~15 % for it (profiles/r05r: LDS bandwidth)
        double cost = (double)((tiles + 255) / 256) * (r.row_blocks + 1.5) * (r.tile == 22 || r.tile == 23 ? 1.15 : 1.0);
        // tile 26 (two workgroups per CU): a round is 512 workgroups and takes two tiles' time, less what one workgroup's prologue,
        // epilogue and round trips hide under the other's loop -- measured (profiles/r05v): 0.8 of it for the conv3 form (its epilogue is
        // HBM time), 0.88 for a short K loop, nothing gained on a long one
        if (r.tile == 26) cost = (double)((tiles + 511) / 512) * 2.0 * (r.row_blocks + 1.5) * (c3 ? 0.8 : nk <= 32 ? 0.88 : 1.05);
        if (!tile || cost < best) { tile = r.tile; best = cost; }
    }
    return tile;
}

// the shallowest ring of the 1x1 stream kernel's tiles, in K steps (its error text names the channels that takes)
constexpr int s1_min_depth() {
    int d = 1 << 30;
    for (const auto& r : kRows)
        if (r.family == HMMR_TILE_STREAM_1X1 && r.depth < d) d = r.depth;
    return d;
}

}  // namespace conv_tiles
