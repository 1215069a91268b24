// The derivative of f_movie's temporal encoder and of the hallucinator, for gfx950 (include/hmmr_hip.h, "f_movie / hallucinator backward";
// DESIGN 4.15).  The function is the exact fp32 one on an HMMR_F32 bank; per temporal block, on the rows of one window:
//
//   h1 = relu(GN1(x))     c1[r] = b1 + sum_tap h1[r + tap - 1] . W1[:, tap]     h2 = relu(GN2(c1))     y = x + b2 + conv(h2, W2)
//
// Nothing is kept from a forward call: both entry points recompute the forward into their workspace with the launches of
// csrc/temporal.hip (hmmr_groupnorm_relu, hmmr_conv_gemm with its split-K), except the last layer's output, which no gradient reads.
//
// The contractions go through csrc/grad_mm.h's kernel with a window: the data gradient dH[r][ci] = sum_tap sum_co dY[r + 1 - tap][co]
// W[co][tap*2048 + ci] reads the bank as it lies in memory -- B[k][j] is W[co][tap*2048 + j], rows of `co` at column offset tap*2048 with
// ldb = 6144, no transposed copy of the filters -- and dY with a row shift per tap and a window guard; the weight gradient
// dW[co][tap*2048 + ci] = sum_r dY[r][co] h[r + tap - 1][ci] reads both operands by row, the h rows shifted per tap and guarded by the
// window.  The recomputed forward is built from csrc/tail_sched.h, as csrc/temporal.hip's is.  No atomics anywhere.
#include "common.h"
#include "grad_mm.h"
#include "hmmr_hip.h"
#include "tail_sched.h"
#include "workspace.h"

static constexpr int C = TAIL_C;                // channels of phi, of every layer of both modules
static constexpr int GROUPS = GN_GROUPS, CPG = C / GROUPS;

// ---------------------------------------------------------------------------------------------------------------- the contraction
// One problem per launch (MmOne, CsOne: no pointer tables).
// The data gradient: the contraction over (tap, output channel), in two accumulator sets (csrc/grad_mm.h); a window's rows never meet
// another's.  t = rows of a window (a fully-connected layer: one tap, every row a window of its own).  The gate is the plain h > 0.
//   dx[rows][C] = sum_tap dy[row + c0 - tap] . W[:, tap]   (+ res, gated)
static int data_grad(const float* dy, const float* w, int rows, int taps, int t, const float* res, const float* gate, float* dx, hipStream_t s) {
    const MmOne p = {dy, w, dx, res, gate};
    return grad_mm_launch<false, true, false, 2>("movie_grad data_grad", p, 1, rows, C, taps * C, C, taps * C, C, C, 1.f, MmWindow{taps, C, t}, s);
}
// The weight gradient, one accumulator set:
//   dw[C][taps * C] = sum_rows dy[row][co] h[row + tap - c0][ci]
static int weight_grad(const float* dy, const float* h, int rows, int taps, int t, float* dw, hipStream_t s) {
    const MmOne p = {dy, h, dw, nullptr, nullptr};
    return grad_mm_launch<true, true, false, 1>("movie_grad weight_grad", p, 1, C, taps * C, rows, C, C, taps * C, taps * C, 1.f, MmWindow{taps, C, t}, s);
}
// out[C] = the column sum of a[rows][C] (a bias gradient), in double
static int col_sum(const float* a, int rows, float* out, hipStream_t s) {
    const CsOne<C> p = {a, out};
    return grad_colsum_launch(p, 1, rows, C, C, s);
}

// ---------------------------------------------------------------------------------------------------------------- GroupNorm + ReLU backward
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
    const float mean = block_sum_256(s, red) / (float)cnt;
    float q = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const float d = xb[(i / CPG) * C + (i % CPG)] - mean;
        q += d * d;
    }
    const float var = block_sum_256(q, red) / (float)cnt;
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
    const float m1 = block_sum_256(s1, red) / (float)cnt;
    const float m2 = block_sum_256(s2, red) / (float)cnt;
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
    l.skbytes = hmmr_conv_splitk_workspace_bytes(b * t, C, temporal_split_k(HMMR_F32));
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
// one convolution of the forward on fp32 operands: csrc/temporal.hip's descriptor
static int temporal_conv(const float* in, const hmmr_layer_t& l, const float* res, float* out, int b, int t, void* sk, size_t skbytes, hipStream_t s) {
    const hmmr_conv_desc_t d = temporal_conv_desc(in, HMMR_F32, l, res, out, b, t, sk, skbytes);
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
// a hidden layer of the forward on fp32 operands: csrc/temporal.hip's descriptor, relu, no residual
static int hal_fc(const float* in, const hmmr_layer_t& l, float* out, int m, void* sk, size_t skbytes, hipStream_t s) {
    const hmmr_conv_desc_t d = hal_fc_desc(in, HMMR_F32, l, out, HMMR_F32, m, 1, nullptr, sk, skbytes);
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
