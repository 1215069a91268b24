// The pose discriminator under training, for gfx950 (include/hmmr_hip.h, "Pose discriminator"): PoseDiscriminator of
// src/discriminators.py, the three losses of src/ops.py:127-136 and the closed loop of compute_losses_prior
// (src/trainer_sequence_fc.py:989-1020).  The function is the exact fp32 one, on an HMMR_F32 bank.  Per row, x[23][9]:
//
//   a1[j] = x[j] . C1 + bc1      h1 = relu(a1)          a3 = flat(h2) . F1 + b1      h3 = relu(a3)
//   a2[j] = h1[j] . C2 + bc2     h2 = relu(a2)          a4 = h3 . F2 + b2            h4 = relu(a4)
//   out[j] = h2[j] . wj[j] + bj[j]                      out[23] = h4 . fo + bo
//
// The front (conv1, conv2, the 23 heads) is one launch with the three small filter sets in LDS; it leaves h2 [n][1024] (736 used, the
// rest zeros: fc1's K padded to a size hmmr_conv_gemm takes).  fc1 / fc2 / fc_out are csrc/tail_sched.h's fc_desc with HMMR_F32 and a
// fixed split-K, as in csrc/ief_grad.hip.  Nothing is kept from a forward call: the backward recomputes it by the same routine.  h1 is
// not stored at all: the front backward recomputes h1 and h2 of its position from x with the forward's own device function (288 + 1024
// fused multiply-adds, against 256 bytes of traffic each way), so the gates are the forward's bits.
// The backward's contractions are csrc/grad_mm.h's kernel, unwindowed, one accumulator set; bias gradients its column sum.  The front
// backward is one launch: d_h2 = d_flat + d_out[j] wj[j], the two gates, d_x, and per tile of 4 rows x 32 joint slots the partial sums
// of its six gradients in double, positions in row-then-joint order; a second small launch adds the tiles in tile order, in double, and
// rounds once.  No atomics anywhere.
#include "common.h"
#include "grad_mm.h"
#include "hmmr_hip.h"
#include "tail_sched.h"
#include "workspace.h"

#include <math.h>

static constexpr int NJ = 23, CH = 32, XW = 207, LDH = 1024, FLAT = NJ * CH;
static constexpr int DISC_SPLIT_K = 4;        // K = 1024, at most n/64 x 16 output tiles: fixed, never a function of n
static constexpr int TILE_ROWS = 4, TILE_POS = TILE_ROWS * 32, LDP = TILE_POS + 1;      // a tile of the front: 4 rows x 32 joint slots
// a tile's partial sums, as doubles: d_C1 [c][i], d_bc1 [c], d_C2 [c][k], d_bc2 [c], d_wj [j][c], d_bj [j]
static constexpr int P_C1 = 0, P_BC1 = P_C1 + CH * 9, P_C2 = P_BC1 + CH, P_BC2 = P_C2 + CH * CH, P_WJ = P_BC2 + CH, P_BJ = P_WJ + NJ * CH,
                     P_N = P_BJ + NJ, P_STRIDE = (P_N + 7) & ~7;

struct Seg { const float* p; long long ld; int n; };
struct DSeg { float* p; long long ld; };
struct FrontBank { const float *c1, *b1, *c2, *b2, *wj, *bj; };

// ---------------------------------------------------------------------------------------------------------------- the front
struct FrontFilters {
    float c1[CH][9], b1[CH], c2[CH][CH], b2[CH], wj[NJ][CH + 1], bj[NJ];
    __device__ __forceinline__ void load(const FrontBank& w) {
        for (int i = threadIdx.x; i < CH * 9; i += blockDim.x) c1[i / 9][i % 9] = w.c1[(i / 9) * 16 + i % 9];
        for (int i = threadIdx.x; i < CH * CH; i += blockDim.x) c2[i / CH][i % CH] = w.c2[i];
        for (int i = threadIdx.x; i < NJ * CH; i += blockDim.x) wj[i / CH][i % CH] = w.wj[i];
        for (int i = threadIdx.x; i < CH; i += blockDim.x) { b1[i] = w.b1[i]; b2[i] = w.b2[i]; }
        for (int i = threadIdx.x; i < NJ; i += blockDim.x) bj[i] = w.bj[i];
    }
    // h1, h2 of one position: every sum starts from the bias and adds its products in index order, one fma each
    __device__ __forceinline__ void point(const float (&x)[9], float (&h1)[CH], float (&h2)[CH]) const {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float a = b1[c];
#pragma unroll
            for (int i = 0; i < 9; ++i) a = fmaf(x[i], c1[c][i], a);
            h1[c] = fmaxf(a, 0.f);
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float a = b2[c];
#pragma unroll
            for (int k = 0; k < CH; ++k) a = fmaf(h1[k], c2[c][k], a);
            h2[c] = fmaxf(a, 0.f);
        }
    }
};
__device__ __forceinline__ const float* seg_row(const Seg& a, const Seg& b, int row) {
    return row < a.n ? a.p + (long long)row * a.ld : b.p + (long long)(row - a.n) * b.ld;
}

// thread = (row, joint slot j of 32): slots 0..22 compute a joint, slots 23..31 write the zeros of h2's padded columns 736..1023
__global__ __launch_bounds__(TILE_POS) void disc_front_fwd_kernel(FrontBank w, Seg a, Seg b, int n, float* __restrict__ h2buf, float* __restrict__ out) {
    __shared__ FrontFilters f;
    f.load(w);
    __syncthreads();
    const int row = blockIdx.x * TILE_ROWS + (threadIdx.x >> 5), j = threadIdx.x & 31;
    if (row >= n) return;
    f32x4* dst = (f32x4*)(h2buf + (long long)row * LDH + j * CH);
    if (j >= NJ) {
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) dst[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float* xp = seg_row(a, b, row) + j * 9;
    float x[9], h1[CH], h2[CH];
#pragma unroll
    for (int i = 0; i < 9; ++i) x[i] = xp[i];
    f.point(x, h1, h2);
    float o = f.bj[j];
#pragma unroll
    for (int c = 0; c < CH; ++c) o = fmaf(h2[c], f.wj[j][c], o);
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) dst[q] = f32x4{h2[4 * q], h2[4 * q + 1], h2[4 * q + 2], h2[4 * q + 3]};
    out[(long long)row * 24 + j] = o;
}

// rows r0 .. r0 + m - 1 of the forward; dflat / d_out are indexed by the local row.  PARTS: also the tile's partial sums.
template <bool PARTS>
__global__ __launch_bounds__(TILE_POS) void disc_front_bwd_kernel(FrontBank w, Seg a, Seg b, int r0, int m, const float* __restrict__ dflat,
                                                                  const float* __restrict__ d_out, DSeg da, DSeg db, int zero9,
                                                                  double* __restrict__ parts) {
    __shared__ FrontFilters f;
    __shared__ float s0[PARTS ? CH : 1][LDP], s1[PARTS ? CH : 1][LDP], s2[PARTS ? CH : 1][LDP], sx[PARTS ? 9 : 1][LDP], sd[PARTS ? TILE_POS : 1];
    f.load(w);
    __syncthreads();
    const int t = threadIdx.x, rl = blockIdx.x * TILE_ROWS + (t >> 5), j = t & 31, row = r0 + rl;
    const bool valid = rl < m && j < NJ;
    float x[9], h1[CH], h2[CH], da2[CH], da1[CH], dj = 0.f;
    if (valid) {
        const float* xp = seg_row(a, b, row) + j * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) x[i] = xp[i];
        f.point(x, h1, h2);
        dj = d_out[(long long)rl * 24 + j];
        const f32x4* g = (const f32x4*)(dflat + (long long)rl * LDH + j * CH);
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const f32x4 v = g[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * q + e;
                da2[c] = h2[c] > 0.f ? fmaf(dj, f.wj[j][c], v[e]) : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) v = fmaf(da2[c], f.c2[c][k], v);
            da1[k] = h1[k] > 0.f ? v : 0.f;
        }
        const DSeg& o = row < a.n ? da : db;
        if (o.p) {
            float* dp = o.p + (long long)(row < a.n ? row : row - a.n) * o.ld;
            if (zero9 && j == 0)
#pragma unroll
                for (int i = 1; i <= 9; ++i) dp[-i] = 0.f;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < CH; ++k) v = fmaf(da1[k], f.c1[k][i], v);
                dp[j * 9 + i] = v;
            }
        }
    }
    if constexpr (PARTS) {
    // the tile's positions into LDS, [value][position]: a position that does not exist is a row of zeros
#pragma unroll
    for (int c = 0; c < CH; ++c) { s0[c][t] = valid ? da2[c] : 0.f; s1[c][t] = valid ? h1[c] : 0.f; s2[c][t] = valid ? da1[c] : 0.f; }
#pragma unroll
    for (int i = 0; i < 9; ++i) sx[i][t] = valid ? x[i] : 0.f;
    sd[t] = valid ? dj : 0.f;
    __syncthreads();
    double* part = parts + (long long)blockIdx.x * P_STRIDE;
    const int c = t & 31, q = t >> 5;
    {   // d_C2[c][k] = sum_p d_a2[p][c] h1[p][k], k = q, q + 4, ...
        double acc[8] = {};
        for (int p = 0; p < TILE_POS; ++p) {
            const double v = (double)s0[c][p];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fma(v, (double)s1[q + 4 * i][p], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) part[P_C2 + c * CH + q + 4 * i] = acc[i];
    }
    {   // d_C1[c][i] = sum_p d_a1[p][c] x[p][i], i = q, q + 4, q + 8
        double acc[3] = {};
        for (int p = 0; p < TILE_POS; ++p) {
            const double v = (double)s2[c][p];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (q + 4 * i < 9) acc[i] = fma(v, (double)sx[q + 4 * i][p], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (q + 4 * i < 9) part[P_C1 + c * 9 + q + 4 * i] = acc[i];
    }
    if (q < 2) {   // d_bc2 (q = 0), d_bc1 (q = 1)
        double acc = 0.0;
        for (int p = 0; p < TILE_POS; ++p) acc += (double)(q ? s2[c][p] : s0[c][p]);
        part[(q ? P_BC1 : P_BC2) + c] = acc;
    } else if (q == 2 && c < NJ) {
        double acc = 0.0;
        for (int r = 0; r < TILE_ROWS; ++r) acc += (double)sd[r * 32 + c];
        part[P_BJ + c] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CH; ++k) s1[k][t] = valid ? h2[k] : 0.f;
    __syncthreads();
    for (int jj = q; jj < NJ; jj += 4) {   // d_wj[j][c] = sum_rows d_out[row][j] h2[row][j][c]
        double acc = 0.0;
        for (int r = 0; r < TILE_ROWS; ++r) acc = fma((double)sd[r * 32 + jj], (double)s1[c][r * 32 + jj], acc);
        part[P_WJ + jj * CH + c] = acc;
    }
    }
}

// the tiles' partial sums added in tile order, in double, rounded once, into the bank's layouts (padding written as zeros)
__global__ void disc_front_reduce_kernel(const double* __restrict__ parts, int tiles, hmmr_disc_pose_grads_t g) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    float* out; int src;
    if (e < 512) { out = g.d_conv1 ? g.d_conv1 + e : nullptr; src = (e & 15) < 9 ? P_C1 + (e >> 4) * 9 + (e & 15) : -1; }
    else if (e < 544) { out = g.d_bc1 ? g.d_bc1 + (e - 512) : nullptr; src = P_BC1 + (e - 512); }
    else if (e < 1568) { out = g.d_conv2 ? g.d_conv2 + (e - 544) : nullptr; src = P_C2 + (e - 544); }
    else if (e < 1600) { out = g.d_bc2 ? g.d_bc2 + (e - 1568) : nullptr; src = P_BC2 + (e - 1568); }
    else if (e < 2624) { out = g.d_heads ? g.d_heads + (e - 1600) : nullptr; src = (e - 1600) < NJ * CH ? P_WJ + (e - 1600) : -1; }
    else if (e < 2656) { out = g.d_bj ? g.d_bj + (e - 2624) : nullptr; src = (e - 2624) < NJ ? P_BJ + (e - 2624) : -1; }
    else return;
    if (!out) return;
    double v = 0.0;
    if (src >= 0)
        for (int t = 0; t < tiles; ++t) v += parts[(long long)t * P_STRIDE + src];
    *out = (float)v;
}

// d_a4[r][c] = d_out[r][23] fo[c] gated by h4 (an outer product: one multiply per element), and dcol [m][128] = d_out[:, 23] in
// column 0, zeros beside it: the operand of d_fc_out / d_bo in the bank's 128-row layout
__global__ void disc_da4_kernel(const float* __restrict__ d_out, const float* __restrict__ fo, const float* __restrict__ h4,
                                float* __restrict__ da4, float* __restrict__ dcol, int m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)m * LDH) return;
    const int r = (int)(i / LDH), c = (int)(i % LDH);
    const float g = d_out[(long long)r * 24 + 23];
    da4[i] = h4[i] > 0.f ? g * fo[c] : 0.f;
    if (c < 128) dcol[(long long)r * 128 + c] = c == 0 ? g : 0.f;
}

// The losses and the two cotangents of hmmr_pose_prior, one workgroup: a thread adds its rows' 24 terms in column order in double,
// then thread k adds loss k's row sums in row order.  cot_e [n_fake][24] = s_e (out - 1); cot_d [n][24] = s_r (out - 1) | s_f out.
__global__ __launch_bounds__(256) void disc_prior_kernel(const float* __restrict__ out, int n_real, int n_fake, float s_e, float s_r, float s_f,
                                                         float* __restrict__ cot_e, float* __restrict__ cot_d, double* __restrict__ rowsum,
                                                         float* __restrict__ losses) {
    const int n = n_real + n_fake;
    for (int r = threadIdx.x; r < n; r += 256) {
        double m1 = 0.0, sq = 0.0;
        for (int k = 0; k < 24; ++k) {
            const float o = out[(long long)r * 24 + k], om = o - 1.f;
            m1 += (double)om * (double)om; sq += (double)o * (double)o;
            if (r < n_real) cot_d[(long long)r * 24 + k] = s_r * om;
            else { cot_d[(long long)r * 24 + k] = s_f * o; cot_e[(long long)(r - n_real) * 24 + k] = s_e * om; }
        }
        rowsum[2 * r] = m1; rowsum[2 * r + 1] = sq;
    }
    __syncthreads();
    if (!losses || threadIdx.x >= 3) return;
    const int k = threadIdx.x, lo = k == 1 ? 0 : n_real, hi = k == 1 ? n_real : n;
    double v = 0.0;
    for (int r = lo; r < hi; ++r) v += rowsum[2 * r + (k == 2 ? 1 : 0)];
    losses[k] = hi > lo ? (float)(v / (double)(hi - lo)) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- the workspace
struct DiscBufs { size_t h2, h3, h4, sk, skbytes, da4, da3, dflat, dcol, parts, out, cot_e, cot_d, rowsum, total; };
static DiscBufs disc_layout(int n) {
    DiscBufs b; WsCarver c;
    const size_t wide = (size_t)n * LDH * 4;
    b.h2 = c.take(wide); b.h3 = c.take(wide); b.h4 = c.take(wide);
    b.skbytes = hmmr_conv_splitk_workspace_bytes(n, LDH, DISC_SPLIT_K);
    b.sk = c.take(b.skbytes);
    b.da4 = c.take(wide); b.da3 = c.take(wide); b.dflat = c.take(wide);
    b.dcol = c.take((size_t)n * 128 * 4);
    b.parts = c.take((size_t)((n + TILE_ROWS - 1) / TILE_ROWS) * P_STRIDE * 8);
    b.out = c.take((size_t)n * 24 * 4);          // the recomputed out (hmmr_disc_pose_bwd, hmmr_pose_prior)
    b.cot_e = c.take((size_t)n * 24 * 4); b.cot_d = c.take((size_t)n * 24 * 4);
    b.rowsum = c.take((size_t)n * 2 * 8);
    b.total = c.total();
    return b;
}
extern "C" size_t hmmr_disc_pose_workspace_bytes(int n) { return n > 0 ? disc_layout(n).total : 0; }

// ---------------------------------------------------------------------------------------------------------------- shared checks
static int disc_check(const hmmr_disc_pose_weights_t* w, const hmmr_rows_t* ra, const hmmr_rows_t* rb, const void* ws, size_t ws_bytes,
                      const char* who, Seg& a, Seg& b) {
    HMMR_REQUIRE(w && ws && (ra || rb), "%s: null argument", who);
    a = ra ? Seg{ra->ptr, (long long)ra->ld, ra->n} : Seg{nullptr, 0, 0};
    b = rb ? Seg{rb->ptr, (long long)rb->ld, rb->n} : Seg{nullptr, 0, 0};
    HMMR_REQUIRE(a.n >= 0 && b.n >= 0, "%s: a negative row count (%d, %d)", who, a.n, b.n);
    HMMR_REQUIRE((long long)a.n + b.n > 0 && (long long)a.n + b.n < (1 << 21), "%s: n_a + n_b = %lld must lie in 1 .. 2^21 - 1", who,
                 (long long)a.n + b.n);
    HMMR_REQUIRE((!a.n || a.p) && (!b.n || b.p), "%s: null argument (the rows of a segment)", who);
    HMMR_REQUIRE((!a.n || a.ld >= XW) && (!b.n || b.ld >= XW), "%s: a row stride below 207 (ld = %lld, %lld)", who, a.ld, b.ld);
    HMMR_REQUIRE(w->dtype == HMMR_F32, "%s: the bank must be packed with dtype HMMR_F32 (it has dtype %d)", who, w->dtype);
    const hmmr_layer_t* l[6] = {&w->conv1, &w->conv2, &w->heads, &w->fc1, &w->fc2, &w->fc_out};
    for (int i = 0; i < 6; ++i) {
        HMMR_REQUIRE(l[i]->w && l[i]->shift, "%s: null argument (a layer of the bank)", who);
        HMMR_REQUIRE(!l[i]->scale, "%s: the bank has a scaled layer: not an HMMR_F32 bank", who);
    }
    const size_t need = disc_layout(a.n + b.n).total;
    HMMR_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes given, %zu needed)", who, ws_bytes, need);
    return 0;
}
static bool any_grad(const hmmr_disc_pose_grads_t& g) {
    return g.d_conv1 || g.d_bc1 || g.d_conv2 || g.d_bc2 || g.d_heads || g.d_bj || g.d_fc1 || g.d_b1 || g.d_fc2 || g.d_b2 || g.d_fc_out || g.d_bo;
}
static FrontBank front_bank(const hmmr_disc_pose_weights_t* w) {
    return FrontBank{(const float*)w->conv1.w, w->conv1.shift, (const float*)w->conv2.w, w->conv2.shift, (const float*)w->heads.w, w->heads.shift};
}

// ---------------------------------------------------------------------------------------------------------------- the forward
// Every entry point runs this.  It leaves h2, h3, h4 [n][1024] in the workspace and out [n][24].
static int disc_forward(const hmmr_disc_pose_weights_t* w, const Seg& a, const Seg& b, float* out, const DiscBufs& L, char* base, hipStream_t s) {
    const int n = a.n + b.n;
    float* h2 = (float*)(base + L.h2); float* h3 = (float*)(base + L.h3); float* h4 = (float*)(base + L.h4);
    hipLaunchKernelGGL(disc_front_fwd_kernel, dim3((unsigned)((n + TILE_ROWS - 1) / TILE_ROWS)), dim3(TILE_POS), 0, s, front_bank(w), a, b, n, h2, out);
    HMMR_CHECK_HIP(hipGetLastError());
    hmmr_conv_desc_t d = fc_desc(h2, HMMR_F32, n, LDH, w->fc1, h3, HMMR_F32, LDH, LDH, DISC_SPLIT_K, base + L.sk, L.skbytes);
    d.relu = 1;
    if (hmmr_conv_gemm(&d, s)) return -2;
    d = fc_desc(h3, HMMR_F32, n, LDH, w->fc2, h4, HMMR_F32, LDH, LDH, DISC_SPLIT_K, base + L.sk, L.skbytes);
    d.relu = 1;
    if (hmmr_conv_gemm(&d, s)) return -2;
    d = fc_desc(h4, HMMR_F32, n, LDH, w->fc_out, out + 23, HMMR_F32, 1, 24, DISC_SPLIT_K, base + L.sk, L.skbytes);
    if (hmmr_conv_gemm(&d, s)) return -2;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the backward
template <bool A_T>
static int mm(const MmOne& p, int M, int N, int K, int lda, int ldb, int ldc, hipStream_t s) {
    return grad_mm_launch<A_T, false, false, 1>("disc_mm_kernel", p, 1, M, N, K, lda, ldb, ldc, 0, 1.f, MmWindow{}, s);
}
// Rows r0 .. r0 + m - 1 of the forward that lies in the workspace, with their cotangent d_out [m][24]: d_x into da / db (the segments'
// outputs, each may be absent) and the wanted gradients.  A data-gradient row does not depend on r0 or m.
static int disc_backward(const hmmr_disc_pose_weights_t* w, const Seg& a, const Seg& b, int r0, int m, const float* d_out, DSeg da, DSeg db,
                         int zero9, const hmmr_disc_pose_grads_t& g, const DiscBufs& L, char* base, hipStream_t s) {
    const long long skip = (long long)r0 * LDH;
    const float* h2 = (const float*)(base + L.h2) + skip; const float* h3 = (const float*)(base + L.h3) + skip;
    const float* h4 = (const float*)(base + L.h4) + skip;
    float* da4 = (float*)(base + L.da4); float* da3 = (float*)(base + L.da3); float* dflat = (float*)(base + L.dflat);
    float* dcol = (float*)(base + L.dcol);
    const bool want_front = g.d_conv1 || g.d_bc1 || g.d_conv2 || g.d_bc2 || g.d_heads || g.d_bj, want_x = da.p || db.p;
    const bool need_flat = want_front || want_x, need_a3 = need_flat || g.d_fc1 || g.d_b1;
    hipLaunchKernelGGL(disc_da4_kernel, dim3((unsigned)(((long long)m * LDH + 255) / 256)), dim3(256), 0, s, d_out, (const float*)w->fc_out.w, h4,
                       da4, dcol, m);
    HMMR_CHECK_HIP(hipGetLastError());
    if (need_a3 && mm<false>(MmOne{da4, (const float*)w->fc2.w, da3, nullptr, h3}, m, LDH, LDH, LDH, LDH, LDH, s)) return -2;      // d_a3 = (d_a4 . F2) gated by h3
    if (need_flat) {
        if (mm<false>(MmOne{da3, (const float*)w->fc1.w, dflat, nullptr, nullptr}, m, FLAT, LDH, LDH, LDH, LDH, s)) return -2;    // d_flat = d_a3 . F1
        const unsigned tiles = (unsigned)((m + TILE_ROWS - 1) / TILE_ROWS);
        double* parts = (double*)(base + L.parts);
        if (want_front) {
            hipLaunchKernelGGL(disc_front_bwd_kernel<true>, dim3(tiles), dim3(TILE_POS), 0, s, front_bank(w), a, b, r0, m, (const float*)dflat, d_out,
                               da, db, zero9, parts);
            HMMR_CHECK_HIP(hipGetLastError());
            hipLaunchKernelGGL(disc_front_reduce_kernel, dim3((2656 + 255) / 256), dim3(256), 0, s, (const double*)parts, (int)tiles, g);
        } else {
            hipLaunchKernelGGL(disc_front_bwd_kernel<false>, dim3(tiles), dim3(TILE_POS), 0, s, front_bank(w), a, b, r0, m, (const float*)dflat, d_out,
                               da, db, zero9, parts);
        }
        HMMR_CHECK_HIP(hipGetLastError());
    }
    // weight gradients over the m batch rows; a gradient nobody asks for is not queued
    if (g.d_fc_out && mm<true>(MmOne{dcol, h4, g.d_fc_out, nullptr, nullptr}, 128, LDH, m, 128, LDH, LDH, s)) return -2;
    if (g.d_fc2 && mm<true>(MmOne{da4, h3, g.d_fc2, nullptr, nullptr}, LDH, LDH, m, LDH, LDH, LDH, s)) return -2;
    if (g.d_fc1 && mm<true>(MmOne{da3, h2, g.d_fc1, nullptr, nullptr}, LDH, LDH, m, LDH, LDH, LDH, s)) return -2;
    if (g.d_bo && grad_colsum_launch(CsOne<128>{dcol, g.d_bo}, 1, m, 128, 128, s)) return -2;
    if (g.d_b2 && grad_colsum_launch(CsOne<LDH>{da4, g.d_b2}, 1, m, LDH, LDH, s)) return -2;
    if (g.d_b1 && grad_colsum_launch(CsOne<LDH>{da3, g.d_b1}, 1, m, LDH, LDH, s)) return -2;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" int hmmr_disc_pose_fwd(const hmmr_disc_pose_weights_t* w, const hmmr_rows_t* rows_a, const hmmr_rows_t* rows_b, float* out, void* ws,
                                  size_t ws_bytes, void* stream) {
    Seg a, b;
    if (int rc = disc_check(w, rows_a, rows_b, ws, ws_bytes, "hmmr_disc_pose_fwd", a, b)) return rc;
    HMMR_REQUIRE(out, "hmmr_disc_pose_fwd: null argument (out)");
    return disc_forward(w, a, b, out, disc_layout(a.n + b.n), (char*)ws, (hipStream_t)stream);
}

extern "C" int hmmr_disc_pose_bwd(const hmmr_disc_pose_weights_t* w, const hmmr_disc_pose_bwd_desc_t* d, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(d, "hmmr_disc_pose_bwd: null descriptor");
    Seg a, b;
    if (int rc = disc_check(w, &d->rows_a, &d->rows_b, ws, ws_bytes, "hmmr_disc_pose_bwd", a, b)) return rc;
    HMMR_REQUIRE(d->d_out, "hmmr_disc_pose_bwd: null argument (d_out)");
    DSeg da = {a.n ? d->d_poses_a : nullptr, (long long)d->ld_a}, db = {b.n ? d->d_poses_b : nullptr, (long long)d->ld_b};
    HMMR_REQUIRE((!da.p || da.ld >= XW) && (!db.p || db.ld >= XW), "hmmr_disc_pose_bwd: a row stride of d_poses below 207 (ld = %lld, %lld)", da.ld,
                 db.ld);
    HMMR_REQUIRE(da.p || db.p || any_grad(d->grads), "hmmr_disc_pose_bwd: no output is requested");
    const DiscBufs L = disc_layout(a.n + b.n);
    hipStream_t s = (hipStream_t)stream;
    if (disc_forward(w, a, b, (float*)((char*)ws + L.out), L, (char*)ws, s)) return -2;
    return disc_backward(w, a, b, 0, a.n + b.n, d->d_out, da, db, 0, d->grads, L, (char*)ws, s);
}

extern "C" int hmmr_pose_prior(const hmmr_disc_pose_weights_t* w, const hmmr_pose_prior_desc_t* d, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(d, "hmmr_pose_prior: null descriptor");
    Seg a, b;
    if (int rc = disc_check(w, &d->real, &d->fake, ws, ws_bytes, "hmmr_pose_prior", a, b)) return rc;
    HMMR_REQUIRE(d->losses || d->d_rs_fake || any_grad(d->grads), "hmmr_pose_prior: no output is requested");
    HMMR_REQUIRE(b.n > 0 || !(d->losses || d->d_rs_fake), "hmmr_pose_prior: e_pose / d_rs_fake need a fake segment that is not empty");
    HMMR_REQUIRE(isfinite(d->w_e) && isfinite(d->w_d), "hmmr_pose_prior: w_e / w_d must be finite");
    const int n = a.n + b.n;
    const DiscBufs L = disc_layout(n);
    char* base = (char*)ws;
    hipStream_t s = (hipStream_t)stream;
    float* out = (float*)(base + L.out); float* cot_e = (float*)(base + L.cot_e); float* cot_d = (float*)(base + L.cot_d);
    if (disc_forward(w, a, b, out, L, base, s)) return -2;
    const float s_e = b.n ? (float)(2.0 * (double)d->w_e / b.n) : 0.f, s_f = b.n ? (float)(2.0 * (double)d->w_d / b.n) : 0.f;
    const float s_r = a.n ? (float)(2.0 * (double)d->w_d / a.n) : 0.f;
    hipLaunchKernelGGL(disc_prior_kernel, dim3(1), dim3(256), 0, s, (const float*)out, a.n, b.n, s_e, s_r, s_f, cot_e, cot_d,
                       (double*)(base + L.rowsum), d->losses);
    HMMR_CHECK_HIP(hipGetLastError());
    // the backward is linear in the cotangent and a data-gradient row stands alone: the encoder's cotangent runs over the fake rows
    // only, the discriminator's over all rows for the weights only, both on the one forward above
    const hmmr_disc_pose_grads_t none = {};
    if (d->d_rs_fake && disc_backward(w, a, b, a.n, b.n, cot_e, DSeg{nullptr, 0}, DSeg{d->d_rs_fake + 9, 216}, 1, none, L, base, s)) return -2;
    if (any_grad(d->grads) && disc_backward(w, a, b, 0, n, cot_d, DSeg{nullptr, 0}, DSeg{nullptr, 0}, 0, d->grads, L, base, s)) return -2;
    return 0;
}
