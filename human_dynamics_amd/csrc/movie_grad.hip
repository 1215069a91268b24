// The derivative of f_movie's temporal encoder and of the hallucinator, for gfx950 (include/hmmr_hip.h, "f_movie / hallucinator backward";
// DESIGN 4.15).  The function is the exact fp32 one on an HMMR_F32 bank; per temporal block, on the rows of one window:
//
//   h1 = relu(GN1(x))     c1[r] = b1 + sum_tap h1[r + tap - 1] . W1[:, tap]     h2 = relu(GN2(c1))     y = x + b2 + conv(h2, W2)
//
// Nothing is kept from a forward call: both entry points recompute the forward into their workspace with the launches of
// csrc/temporal.hip (hmmr_groupnorm_relu, hmmr_conv_gemm with its split-K), except the last layer's output, which no gradient reads.
//
// One contraction kernel on v_mfma_f32_32x32x2_f32 (movie_mm_kernel; csrc/ief_grad.hip's ief_mm_kernel with a tap in the addressing):
// the data gradient dH[r][ci] = sum_tap sum_co dY[r + 1 - tap][co] W[co][tap*2048 + ci] reads the bank as it lies in memory -- B[k][j] is
// W[co][tap*2048 + j], rows of `co` at column offset tap*2048 with ldb = 6144, no transposed copy of the filters -- and dY with a row
// shift per tap and a window guard; the weight gradient dW[co][tap*2048 + ci] = sum_r dY[r][co] h[r + tap - 1][ci] reads both operands by
// row, the h rows shifted per tap and guarded by the window.  A guarded-out value is a zero operand.  Every output tile is one workgroup
// whose waves each take a fixed slice of the contraction; the partial tiles are added in slice order.  No atomics anywhere.
#include "common.h"
#include "hmmr_hip.h"
#include "workspace.h"

static constexpr int C = 2048;                  // channels of phi, of every layer of both modules
static constexpr int GROUPS = 32, CPG = C / GROUPS;
static constexpr float GN_EPS = 1e-6f;          // csrc/temporal.hip
static constexpr int TEMPORAL_SPLIT_K = 4;      // what hmmr_temporal_fwd / hmmr_hallucinator_fwd give hmmr_conv_gemm on an HMMR_F32 bank
static constexpr int HAL_SPLIT_K = 4;

// ---------------------------------------------------------------------------------------------------------------- the contraction
// C[M][N] = sum_k A(i, k) * B(k, j)  (+ res[i][j]; then gated by gate[i][j] > 0), `taps` = 1 or 3, t = rows of a window, c0 = taps / 2.
//   A_T false (data gradient): K = taps * kt.  k = tap * kt + co:  A(i, k) = a[i + c0 - tap][co] if that row lies in i's window,
//                              B(k, j) = b[co][tap * kt + j].
//   A_T true (weight gradient): N = taps * nt.  j = tap * nt + ci:  A(i, k) = a[k][i],  B(k, j) = b[k + tap - c0][ci] if that row lies
//                              in k's window.
// Workgroup = one (32 MI) x (32 NI) tile of C, wave w = slice w of the contraction (ks values each, a multiple of 16; a chunk of 16 lies
// inside one tap); the partial tiles are added in slice order, (((w0 + w1) + w2) + ...).  v_mfma_f32_32x32x2_f32: lane l holds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; result register q of lane l is C[(q & 3) + 8 (q >> 2) + 4 (l >> 5)][l & 31].
// Step s of a chunk of 16 takes k0 + s (lanes 0..31) and k0 + 8 + s (lanes 32..63), so that a row-major A is read as two 16-byte pieces
// per lane.  Eight steps of operands are loaded while the MFMAs of the eight before them run (two register sets).  Every read is
// guarded by the operand's own extent and by the window.
struct MmArgs {
    const float* a; const float* b; float* c; const float* res; const float* gate;
    int M, N, K, lda, ldb, ldc, taps, span, t;      // span = kt (A_T false) or nt (A_T true)
};

template <bool A_T, int MI, int NI, int SLICES>
__global__ __launch_bounds__(64 * SLICES) void movie_mm_kernel(MmArgs p) {
    static_assert((SLICES - 1) * MI * NI * 16 * 64 * 4 <= 64 * 1024, "the partial tiles must fit the static LDS limit");
    __shared__ float red[SLICES - 1][MI * NI][16][64];
    const float* __restrict__ a = p.a;
    const float* __restrict__ b = p.b;
    const int M = p.M, N = p.N, K = p.K, lda = p.lda, ldb = p.ldb, span = p.span, t = p.t, c0 = p.taps >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.y * (32 * MI) + r, j0 = blockIdx.x * (32 * NI) + r;
    const int ks = ((K + SLICES - 1) / SLICES + 15) & ~15;
    const int kb = wave * ks, ke = min(K, kb + ks);
    // the data gradient's long contraction goes to two accumulators, the chunks of 16 in turn (half the length of a rounding chain, and
    // no MFMA waits for the one before it); they are added once, in front of the slices
    constexpr int SETS = A_T ? 1 : 2;
    f32x16 accs[SETS][MI][NI];
#pragma unroll
    for (int e = 0; e < SETS; ++e)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) accs[e][mi][ni][q] = 0.f;
    // what does not change along the contraction: the position of an A row in its window (data gradient), the tap of a B column (weight gradient)
    int it[MI], jtap[NI], jcol[NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) it[mi] = (i0 + 32 * mi) % t;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int j = j0 + 32 * ni;
        jtap[ni] = A_T ? j / span : 0;
        jcol[ni] = A_T ? j - jtap[ni] * span : j;
    }
    float a0[8][MI], b0[8][NI], a1[8][MI], b1[8][NI];
    auto load = [&](float (&av)[8][MI], float (&bv)[8][NI], int k0) {
        if (!A_T) {                                     // a lane's eight values are consecutive in its row: two 16-byte reads
            const int tap = k0 / span, co = k0 - tap * span + 8 * h, sh = c0 - tap;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int i = i0 + 32 * mi;
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
                if (k0 < ke && i < M && (unsigned)(it[mi] + sh) < (unsigned)t) {
                    const f32x4* q = (const f32x4*)(a + (long long)(i + sh) * lda + co);
                    lo = q[0]; hi = q[1];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) { av[s][mi] = lo[s]; av[4 + s][mi] = hi[s]; }
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const bool kok = k0 + 8 * h + s < ke;
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    bv[s][ni] = (kok && j0 + 32 * ni < N) ? b[(long long)(co + s) * ldb + tap * span + jcol[ni]] : 0.f;
            }
        } else {
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int k = k0 + 8 * h + s;
                const bool kok = k < ke;
                const int kt = k % t;
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int i = i0 + 32 * mi;
                    av[s][mi] = (kok && i < M) ? a[(long long)k * lda + i] : 0.f;
                }
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const int sh = jtap[ni] - c0;
                    bv[s][ni] = (kok && j0 + 32 * ni < N && (unsigned)(kt + sh) < (unsigned)t) ? b[(long long)(k + sh) * ldb + jcol[ni]] : 0.f;
                }
            }
        }
    };
    auto mma = [&](const float (&av)[8][MI], const float (&bv)[8][NI], f32x16 (&acc)[MI][NI]) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][mi], bv[s][ni], acc[mi][ni], 0, 0, 0);
    };
    load(a0, b0, kb);
    for (int k0 = kb; k0 < ke; k0 += 32) {                  // (kb, ke and every branch below are the same for a whole wave)
        if (k0 + 16 < ke) load(a1, b1, k0 + 16);
        mma(a0, b0, accs[0]);
        if (k0 + 16 < ke) {
            if (k0 + 32 < ke) load(a0, b0, k0 + 32);
            mma(a1, b1, accs[SETS - 1]);
        }
    }
    f32x16 (&acc)[MI][NI] = accs[0];
    if (SETS == 2) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[mi][ni][q] += accs[SETS - 1][mi][ni][q];
    }
    if (wave) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) red[wave - 1][mi * NI + ni][q][lane] = acc[mi][ni][q];
    }
    __syncthreads();
    if (wave) return;
    float* __restrict__ c = p.c;
    const float* __restrict__ res = p.res;
    const float* __restrict__ gate = p.gate;
    const int ldc = p.ldc;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int j = j0 + 32 * ni;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float v = acc[mi][ni][q];
#pragma unroll
                for (int w = 0; w < SLICES - 1; ++w) v += red[w][mi * NI + ni][q][lane];
                const int row = blockIdx.y * (32 * MI) + 32 * mi + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (row < M && j < N) {
                    if (res) v = res[(long long)row * ldc + j] + v;
                    if (gate) v = gate[(long long)row * ldc + j] > 0.f ? v : 0.f;
                    c[(long long)row * ldc + j] = v;
                }
            }
        }
}

// The data gradient: 32 rows x 32 inputs per workgroup, the contraction over (tap, output channel) in 8 slices -- b*t is a few hundred
// rows at most, so small tiles and the slices are what fills the chip; the split is fixed, it does not depend on the rows.
//   dx[rows][C] = sum_tap dy[row + c0 - tap] . W[:, tap]   (+ res, gated)
static int data_grad(const float* dy, const float* w, int rows, int taps, int t, const float* res, const float* gate, float* dx, hipStream_t s) {
    MmArgs p = {dy, w, dx, res, gate, rows, C, taps * C, C, taps * C, C, taps, C, t};
    hipLaunchKernelGGL((movie_mm_kernel<false, 1, 1, 8>), dim3(C / 32, (unsigned)((rows + 31) / 32)), dim3(64 * 8), 0, s, p);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
// The weight gradient: 64 x 64 per workgroup (each operand value feeds two MFMAs; a tile lies inside one tap), 4 slices of the rows.
//   dw[C][taps * C] = sum_rows dy[row][co] h[row + tap - c0][ci]
static int weight_grad(const float* dy, const float* h, int rows, int taps, int t, float* dw, hipStream_t s) {
    MmArgs p = {dy, h, dw, nullptr, nullptr, C, taps * C, rows, C, C, taps * C, taps, C, t};
    hipLaunchKernelGGL((movie_mm_kernel<true, 2, 2, 4>), dim3((unsigned)(taps * C / 64), C / 64), dim3(64 * 4), 0, s, p);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// out[col] = sum over the K rows of a[K][C], accumulated in double and rounded once (csrc/ief_grad.hip's column sum, DESIGN 4.14: a plain
// fp32 chain over the rows loses bits a blocked sum keeps).  A workgroup owns 32 columns; thread (g, c) adds rows g, g + 8, ... of column
// c in row order, thread (0, c) adds the eight partial sums in g order: a fixed order for a given K.
__global__ __launch_bounds__(256) void movie_colsum_kernel(const float* __restrict__ a, int K, float* __restrict__ out) {
    __shared__ double part[8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + c;                // (C is a multiple of 32: every column exists)
    double v = 0.0;
    for (int k = g; k < K; k += 8) v += (double)a[(long long)k * C + col];
    part[g][c] = v;
    __syncthreads();
    if (g) return;
    for (int q = 1; q < 8; ++q) v += part[q][c];
    out[col] = (float)v;
}
static int col_sum(const float* a, int rows, float* out, hipStream_t s) {
    hipLaunchKernelGGL(movie_colsum_kernel, dim3(C / 32), dim3(256), 0, s, a, rows, out);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm + ReLU backward
__device__ __forceinline__ float gn_block_sum(float v, float* red) {          // csrc/temporal.hip's block_sum_256: the forward's order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// One workgroup per (window b, group g), like the forward's.  x: the GN input, h = relu(GN(x)) as the forward stored it (the gate),
// dh: the cotangent of h.  Mean and rstd are recomputed in the forward's two-pass form; with g = dh * (h > 0) * gamma and
// xhat = (x - mean) * rstd:   dx = rstd * (g - mean(g) - xhat * mean(g * xhat))  (+ res), the means over t x 64.
// pg / pb (or NULL): this window's row of the d_gamma / d_beta partial sums, sum_t dh * gate * xhat and sum_t dh * gate per channel, in
// double: thread (q, c) adds frames q, q + 4, ... in frame order, thread (0, c) adds the four in q order.
__global__ __launch_bounds__(256) void gn_relu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ gamma,
                                                          const float* __restrict__ dh, const float* __restrict__ res, float* __restrict__ dx,
                                                          double* __restrict__ pg, double* __restrict__ pb, int t) {
    __shared__ float red[4];
    __shared__ double part[2][4][CPG];
    const int b = blockIdx.x / GROUPS, g = blockIdx.x % GROUPS;
    const int cnt = t * CPG;
    const long long base = (long long)b * t * C + g * CPG;
    const float* xb = x + base;
    const float* hb = h + base;
    const float* db = dh + base;
    float s = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) s += xb[(i / CPG) * C + (i % CPG)];
    const float mean = gn_block_sum(s, red) / (float)cnt;
    float q = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const float d = xb[(i / CPG) * C + (i % CPG)] - mean;
        q += d * d;
    }
    const float var = gn_block_sum(q, red) / (float)cnt;
    const float rstd = rsqrtf(var + GN_EPS);
    const int ch = threadIdx.x % CPG;                   // 256 % 64 == 0: a thread stays on one channel
    const float gm = gamma[g * CPG + ch];
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int o = (i / CPG) * C + ch;
        const float gv = hb[o] > 0.f ? db[o] * gm : 0.f;
        s1 += gv;
        s2 += gv * ((xb[o] - mean) * rstd);
    }
    const float m1 = gn_block_sum(s1, red) / (float)cnt;
    const float m2 = gn_block_sum(s2, red) / (float)cnt;
    if (dx) {
        float* ob = dx + base;
        const float* rb = res ? res + base : nullptr;
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const int o = (i / CPG) * C + ch;
            const float gv = hb[o] > 0.f ? db[o] * gm : 0.f;
            const float v = rstd * (gv - m1 - ((xb[o] - mean) * rstd) * m2);
            ob[o] = rb ? rb[o] + v : v;
        }
    }
    if (!pg) return;                                    // (the whole workgroup)
    const int qd = threadIdx.x / CPG;
    double sg = 0.0, sb = 0.0;
    for (int tt = qd; tt < t; tt += 4) {
        const int o = tt * C + ch;
        const float gu = hb[o] > 0.f ? db[o] : 0.f;
        sb += (double)gu;
        sg += (double)gu * (double)((xb[o] - mean) * rstd);
    }
    part[0][qd][ch] = sg; part[1][qd][ch] = sb;
    __syncthreads();
    if (qd) return;
    for (int k = 1; k < 4; ++k) { sg += part[0][k][ch]; sb += part[1][k][ch]; }
    pg[(long long)b * C + g * CPG + ch] = sg;
    pb[(long long)b * C + g * CPG + ch] = sb;
}

// d_gamma[c] = sum over the windows of pg[w][c] in window order, in double, rounded once; d_beta alike.  Either output may be NULL.
__global__ void gn_param_sum_kernel(const double* __restrict__ pg, const double* __restrict__ pb, int nb, float* __restrict__ d_gamma,
                                    float* __restrict__ d_beta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sb = 0.0;
    for (int w = 0; w < nb; ++w) { sg += pg[(long long)w * C + c]; sb += pb[(long long)w * C + c]; }
    if (d_gamma) d_gamma[c] = (float)sg;
    if (d_beta) d_beta[c] = (float)sb;
}

// dx = the GN + ReLU backward of (x, h, gamma) on the cotangent dh (+ res); d_gamma / d_beta if wanted
static int gn_backward(const float* x, const float* h, const float* gamma, const float* dh, const float* res, float* dx, float* d_gamma,
                       float* d_beta, double* pg, double* pb, int b, int t, hipStream_t s) {
    const bool params = d_gamma || d_beta;
    hipLaunchKernelGGL(gn_relu_bwd_kernel, dim3((unsigned)(b * GROUPS)), dim3(256), 0, s, x, h, gamma, dh, res, dx, params ? pg : nullptr,
                       params ? pb : nullptr, t);
    HMMR_CHECK_HIP(hipGetLastError());
    if (params) {
        hipLaunchKernelGGL(gn_param_sum_kernel, dim3(C / 256), dim3(256), 0, s, (const double*)pg, (const double*)pb, b, d_gamma, d_beta);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the workspaces
// Temporal: per block its input (block 0 reads phi itself), h1, c1, h2; then the cotangent's two trunk buffers, the cotangent of a
// GN + ReLU output, that of c1, the per-window d_gamma / d_beta partial sums (double) and the split-K planes of the recomputed forward.
struct TemporalGradBufs {
    size_t x[HMMR_MAX_TEMPORAL_BLOCKS], h1[HMMR_MAX_TEMPORAL_BLOCKS], c1[HMMR_MAX_TEMPORAL_BLOCKS], h2[HMMR_MAX_TEMPORAL_BLOCKS];
    size_t dy[2], dh, dc1, pg, pb, sk, skbytes, total;
};
static TemporalGradBufs temporal_grad_layout(int b, int t, int num_blocks) {
    TemporalGradBufs l = {}; WsCarver c;
    const size_t rows = (size_t)b * t * C * 4;
    for (int i = 0; i < num_blocks; ++i) {
        l.x[i] = i ? c.take(rows) : 0;
        l.h1[i] = c.take(rows); l.c1[i] = c.take(rows); l.h2[i] = c.take(rows);
    }
    l.dy[0] = c.take(rows); l.dy[1] = c.take(rows); l.dh = c.take(rows); l.dc1 = c.take(rows);
    l.pg = c.take((size_t)b * C * 8); l.pb = c.take((size_t)b * C * 8);
    l.skbytes = hmmr_conv_splitk_workspace_bytes(b * t, C, TEMPORAL_SPLIT_K);
    l.sk = c.take(l.skbytes);
    l.total = c.total();
    return l;
}
// Hallucinator: h1, h2 of the recomputed forward, d_a2, d_a1, the split-K planes.
struct HalGradBufs { size_t h1, h2, da2, da1, sk, skbytes, total; };
static HalGradBufs hal_grad_layout(int m) {
    HalGradBufs l = {}; WsCarver c;
    const size_t rows = (size_t)m * C * 4;
    l.h1 = c.take(rows); l.h2 = c.take(rows); l.da2 = c.take(rows); l.da1 = c.take(rows);
    l.skbytes = hmmr_conv_splitk_workspace_bytes(m, C, HAL_SPLIT_K);
    l.sk = c.take(l.skbytes);
    l.total = c.total();
    return l;
}

extern "C" size_t hmmr_temporal_bwd_workspace_bytes(int b, int t, int num_blocks) {
    if (b <= 0 || t <= 0 || num_blocks < 1 || num_blocks > HMMR_MAX_TEMPORAL_BLOCKS) return 0;
    return temporal_grad_layout(b, t, num_blocks).total;
}
extern "C" size_t hmmr_hallucinator_bwd_workspace_bytes(int m) { return m > 0 ? hal_grad_layout(m).total : 0; }

static bool plain_f32(const hmmr_layer_t& l) { return l.w && l.shift && !l.scale; }

// ---------------------------------------------------------------------------------------------------------------- the temporal encoder
// one convolution of csrc/temporal.hip's forward: the descriptor hmmr_temporal_fwd builds, on fp32 operands
static int temporal_conv(const float* in, const hmmr_layer_t& l, const float* res, float* out, int b, int t, void* sk, size_t skbytes, hipStream_t s) {
    hmmr_conv_desc_t d = {};
    d.in = in; d.w = l.w; d.scale = l.scale; d.shift = l.shift; d.tile = l.tile;
    d.out = out; d.in_dtype = HMMR_F32; d.out_dtype = HMMR_F32;
    d.n_img = b; d.hin = t; d.win = 1; d.cin = C;
    d.in_img_stride = (int64_t)t * C; d.in_row_stride = C; d.in_px_stride = C;
    d.kh = 3; d.kw = 1; d.sy = d.sx = 1; d.py = 1; d.px = 0; d.ho = t; d.wo = 1; d.cout = C; d.ldo = C;
    d.split_k = TEMPORAL_SPLIT_K; d.ws = sk; d.ws_bytes = skbytes;
    d.res = res; d.ldr = C;
    return hmmr_conv_gemm(&d, s) ? -2 : 0;
}

extern "C" int hmmr_temporal_bwd(const hmmr_temporal_weights_t* w, const hmmr_temporal_bwd_desc_t* d, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(d, "hmmr_temporal_bwd: null descriptor");
    HMMR_REQUIRE(w && d->phi && d->d_strips && ws, "hmmr_temporal_bwd: null argument");
    HMMR_REQUIRE(d->b > 0 && d->t > 0, "hmmr_temporal_bwd: b and t must be positive");
    HMMR_REQUIRE(w->dtype == HMMR_F32, "hmmr_temporal_bwd: the bank must be packed with dtype HMMR_F32 (it has dtype %d)", w->dtype);
    HMMR_REQUIRE(w->num_blocks >= 1 && w->num_blocks <= HMMR_MAX_TEMPORAL_BLOCKS, "hmmr_temporal_bwd: bad num_blocks");
    HMMR_REQUIRE((long long)d->b * d->t <= (1 << 20), "hmmr_temporal_bwd: b * t is limited to 2^20 rows");
    const int nblk = w->num_blocks, b = d->b, t = d->t, rows = b * t;
    int lowest = d->d_phi ? 0 : nblk;                  // the lowest block the chain has to reach
    for (int i = 0; i < nblk; ++i) {
        const hmmr_temporal_block_t& B = w->block[i];
        HMMR_REQUIRE(B.gn1_gamma && B.gn1_beta && B.gn2_gamma && B.gn2_beta && plain_f32(B.conv1) && plain_f32(B.conv2),
                     "hmmr_temporal_bwd: block %d has a null or scaled layer: not an HMMR_F32 bank", i);
        const hmmr_temporal_block_grads_t& g = d->block[i];
        if (i < lowest && (g.d_gn1_gamma || g.d_gn1_beta || g.d_conv1 || g.d_b1 || g.d_gn2_gamma || g.d_gn2_beta || g.d_conv2 || g.d_b2)) lowest = i;
    }
    HMMR_REQUIRE(lowest < nblk, "hmmr_temporal_bwd: no output is requested");
    const TemporalGradBufs L = temporal_grad_layout(b, t, nblk);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_temporal_bwd: workspace too small (%zu bytes given, %zu needed)", ws_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    auto F = [&](size_t off) { return (float*)(base + off); };
    void* sk = base + L.sk;
    double* pg = (double*)(base + L.pg);
    double* pb = (double*)(base + L.pb);

    // the forward, as hmmr_temporal_fwd runs it, every intermediate kept; the last block's conv2 output is not needed
    const float* x[HMMR_MAX_TEMPORAL_BLOCKS];
    for (int i = 0; i < nblk; ++i) {
        const hmmr_temporal_block_t& B = w->block[i];
        x[i] = i ? F(L.x[i]) : d->phi;
        if (hmmr_groupnorm_relu(x[i], B.gn1_gamma, B.gn1_beta, b, t, C, GROUPS, F(L.h1[i]), HMMR_F32, stream)) return -2;
        if (temporal_conv(F(L.h1[i]), B.conv1, nullptr, F(L.c1[i]), b, t, sk, L.skbytes, s)) return -2;
        if (hmmr_groupnorm_relu(F(L.c1[i]), B.gn2_gamma, B.gn2_beta, b, t, C, GROUPS, F(L.h2[i]), HMMR_F32, stream)) return -2;
        if (i + 1 < nblk && temporal_conv(F(L.h2[i]), B.conv2, x[i], F(L.x[i + 1]), b, t, sk, L.skbytes, s)) return -2;
    }

    // the backward, block after block from the last: dy = the cotangent of the block's output
    const float* dy = d->d_strips;
    for (int i = nblk - 1; i >= lowest; --i) {
        const hmmr_temporal_block_t& B = w->block[i];
        const hmmr_temporal_block_grads_t& g = d->block[i];
        const bool need_dx = i > lowest || d->d_phi;                                  // something below reads this block's d(input)
        const bool need_gn1 = need_dx || g.d_gn1_gamma || g.d_gn1_beta;
        const bool need_dc1 = need_gn1 || g.d_conv1 || g.d_b1;
        const bool need_gn2 = need_dc1 || g.d_gn2_gamma || g.d_gn2_beta;
        if (g.d_b2 && col_sum(dy, rows, g.d_b2, s)) return -2;
        if (g.d_conv2 && weight_grad(dy, F(L.h2[i]), rows, 3, t, g.d_conv2, s)) return -2;
        if (!need_gn2) continue;
        if (data_grad(dy, (const float*)B.conv2.w, rows, 3, t, nullptr, nullptr, F(L.dh), s)) return -2;
        if (gn_backward(F(L.c1[i]), F(L.h2[i]), B.gn2_gamma, F(L.dh), nullptr, need_dc1 ? F(L.dc1) : nullptr, g.d_gn2_gamma, g.d_gn2_beta, pg, pb,
                        b, t, s)) return -2;
        if (g.d_b1 && col_sum(F(L.dc1), rows, g.d_b1, s)) return -2;
        if (g.d_conv1 && weight_grad(F(L.dc1), F(L.h1[i]), rows, 3, t, g.d_conv1, s)) return -2;
        if (!need_gn1) continue;
        if (data_grad(F(L.dc1), (const float*)B.conv1.w, rows, 3, t, nullptr, nullptr, F(L.dh), s)) return -2;
        // the residual: d(block input) = dy + dx(GN1)
        float* dxo = !need_dx ? nullptr : (i == 0 ? d->d_phi : F(L.dy[i & 1]));
        if (gn_backward(x[i], F(L.h1[i]), B.gn1_gamma, F(L.dh), dy, dxo, g.d_gn1_gamma, g.d_gn1_beta, pg, pb, b, t, s)) return -2;
        dy = dxo;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the hallucinator
static int hal_fc(const float* in, const hmmr_layer_t& l, float* out, int m, void* sk, size_t skbytes, hipStream_t s) {
    hmmr_conv_desc_t d = {};
    d.in = in; d.w = l.w; d.scale = l.scale; d.shift = l.shift; d.out = out;
    d.in_dtype = HMMR_F32; d.out_dtype = HMMR_F32;
    d.n_img = m; d.hin = d.win = 1; d.cin = C;
    d.in_img_stride = C; d.in_row_stride = C; d.in_px_stride = C;
    d.kh = d.kw = 1; d.sy = d.sx = 1; d.ho = d.wo = 1; d.cout = C; d.ldo = C;
    d.relu = 1; d.ldr = C;
    d.split_k = HAL_SPLIT_K; d.ws = sk; d.ws_bytes = skbytes;
    return hmmr_conv_gemm(&d, s) ? -2 : 0;
}

extern "C" int hmmr_hallucinator_bwd(const hmmr_hallucinator_weights_t* w, const hmmr_hallucinator_bwd_desc_t* d, void* ws, size_t ws_bytes,
                                     void* stream) {
    HMMR_REQUIRE(d, "hmmr_hallucinator_bwd: null descriptor");
    HMMR_REQUIRE(w && d->phi && d->d_out && ws, "hmmr_hallucinator_bwd: null argument");
    HMMR_REQUIRE(d->m > 0, "hmmr_hallucinator_bwd: m must be positive");
    HMMR_REQUIRE(w->dtype == HMMR_F32, "hmmr_hallucinator_bwd: the bank must be packed with dtype HMMR_F32 (it has dtype %d)", w->dtype);
    HMMR_REQUIRE(plain_f32(w->fc1) && plain_f32(w->fc2) && plain_f32(w->fc3), "hmmr_hallucinator_bwd: a null or scaled layer: not an HMMR_F32 bank");
    HMMR_REQUIRE(d->m <= (1 << 20), "hmmr_hallucinator_bwd: m is limited to 2^20 rows");
    HMMR_REQUIRE(d->d_phi || d->d_fc1 || d->d_fc2 || d->d_fc3 || d->d_b1 || d->d_b2 || d->d_b3, "hmmr_hallucinator_bwd: no output is requested");
    const int m = d->m;
    const HalGradBufs L = hal_grad_layout(m);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_hallucinator_bwd: workspace too small (%zu bytes given, %zu needed)", ws_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float *h1 = (float*)(base + L.h1), *h2 = (float*)(base + L.h2), *da2 = (float*)(base + L.da2), *da1 = (float*)(base + L.da1);
    void* sk = base + L.sk;
    const bool need_da1 = d->d_phi || d->d_fc1 || d->d_b1;
    const bool need_da2 = need_da1 || d->d_fc2 || d->d_b2;
    const bool need_h2 = need_da2 || d->d_fc3;
    // the forward's two hidden layers, as hmmr_hallucinator_fwd runs them (fc3's output is read by no gradient)
    if (need_h2) {
        if (hal_fc(d->phi, w->fc1, h1, m, sk, L.skbytes, s)) return -2;
        if (hal_fc(h1, w->fc2, h2, m, sk, L.skbytes, s)) return -2;
    }
    // a row is a window of its own (t = 1), one tap
    if (d->d_b3 && col_sum(d->d_out, m, d->d_b3, s)) return -2;
    if (d->d_fc3 && weight_grad(d->d_out, h2, m, 1, 1, d->d_fc3, s)) return -2;
    if (!need_da2) return 0;
    if (data_grad(d->d_out, (const float*)w->fc3.w, m, 1, 1, nullptr, h2, da2, s)) return -2;            // d_a2 = (d_out . W3) gated by h2
    if (d->d_b2 && col_sum(da2, m, d->d_b2, s)) return -2;
    if (d->d_fc2 && weight_grad(da2, h1, m, 1, 1, d->d_fc2, s)) return -2;
    if (!need_da1) return 0;
    if (data_grad(da2, (const float*)w->fc2.w, m, 1, 1, nullptr, h1, da1, s)) return -2;                 // d_a1 = (d_a2 . W2) gated by h1
    if (d->d_b1 && col_sum(da1, m, d->d_b1, s)) return -2;
    if (d->d_fc1 && weight_grad(da1, d->phi, m, 1, 1, d->d_fc1, s)) return -2;
    if (d->d_phi && data_grad(da1, (const float*)w->fc1.w, m, 1, 1, d->d_out, nullptr, d->d_phi, s)) return -2;   // d_phi = d_out + d_a1 . W1
    return 0;
}
