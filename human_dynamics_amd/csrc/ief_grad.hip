// The IEF regressors under training, for gfx950 (include/hmmr_hip.h, "IEF backward"): the training form of the forward
// (slim.dropout behind fc1 and fc2, src/models.py:103-105) and its derivative.  The function is the exact fp32 one, on an HMMR_F32 bank:
//
//   a1 = phi . W1[:2048] + b1 + theta_s . W1[2048:]      h1 = relu(a1) * keep[r][s][0] * keep_scale
//   a2 = h1 . W2 + b2                                    h2 = relu(a2) * keep[r][s][1] * keep_scale
//   theta_{s+1} = theta_s + h2 . W3 + b3
//
// Nothing is kept from a forward call: hmmr_ief_bwd recomputes the forward into its workspace through ief_train_forward, the routine
// hmmr_ief_fwd_train runs.  The masked h1 / h2 carry the gate of the backward: h > 0 exactly where a > 0 and keep = 1 (keep_scale > 0),
// so d_a = d_h * (h > 0 ? keep_scale : 0), and relu'(0) = 0.
//
// Two contractions through csrc/grad_mm.h's kernel, unwindowed, one accumulator set: the data gradient dX = dY . W sums over the ROWS of
// the bank as it lies in memory, and the weight gradient dW = d_a^T . x sums over the rows of the batch, the stages of a regressor laid
// end to end ([num_stages * m][...]): one launch per layer.  A data-gradient row does not depend on m.  The recomputed forward is built
// from csrc/tail_sched.h, as csrc/ief.hip's is.
#include "common.h"
#include "grad_mm.h"
#include "hmmr_hip.h"
#include "tail_sched.h"
#include "workspace.h"

#include <math.h>

static constexpr int G = HMMR_MAX_REGRESSORS;

// ---------------------------------------------------------------------------------------------------------------- small kernels
// theta_0[m, :] = [src(row or broadcast)[off : off + nd], 0...] into stage slot 0; slots 1 .. S start as zeros (fc3 writes nd columns of
// them, the others are operands of the K = 128 theta GEMM).  Grid y = problem: its state `set_stride` floats behind the previous one's.
__global__ void ief_train_init_theta_kernel(const float* __restrict__ src, int ld_src, int off, int nd, float* __restrict__ theta, int m,
                                            int slots, long long set_stride) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (long long)m * LDT;
    if (i >= n * slots) return;
    const long long e = i % n;
    const int row = (int)(e / LDT), col = (int)(e % LDT);
    theta[(long long)blockIdx.y * set_stride + i] = (i < n && col < nd) ? src[(long long)row * ld_src + off + col] : 0.f;
}

// h *= keep * keep_scale, in place on relu(a): n = m * 1024 values.  Grid y = problem: h `set_stride` floats, keep `keep_stride` bytes on.
__global__ void ief_keep_kernel(float* __restrict__ h, const unsigned char* __restrict__ keep, float keep_scale, long long n,
                                long long set_stride, long long keep_stride) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* p = h + (long long)blockIdx.y * set_stride + i;
    *p = *p * (keep[(long long)blockIdx.y * keep_stride + i] ? 1.f : 0.f) * keep_scale;
}

// d_theta of the last stage from a regressor's d_omega: mode 0 -> [:, :85]; 1 -> [:, 3:75]; 2 -> [:, :75]; zero padded to LDT
__global__ void ief_bwd_init_kernel(const float* __restrict__ d_omega, int mode, float* __restrict__ dth, int m, long long set_stride) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)m * LDT) return;
    const int row = (int)(i / LDT), col = (int)(i % LDT);
    const float* g = d_omega + (long long)blockIdx.y * m * 85 + (long long)row * 85;
    const int nd = mode == 0 ? 85 : (mode == 1 ? 72 : 75);
    dth[(long long)blockIdx.y * set_stride + i] = col < nd ? g[col + (mode == 1 ? 3 : 0)] : 0.f;
}

// out[m, 85] = base (or zero) + what the delta regressors 1 .. R - 1 pass to their starting omega, added in regressor order:
// their d_theta_0 on the pose (and camera) columns, their own d_omega on the beta columns 75 .. 84 they copy
__global__ void ief_bwd_gather_kernel(const float* __restrict__ base, const float* __restrict__ d_omegas, const float* __restrict__ dth0,
                                      long long set_stride, int R, int mode, float* __restrict__ out, int m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)m * 85) return;
    const int row = (int)(i / 85), col = (int)(i % 85);
    float v = base ? base[i] : 0.f;
    for (int r = 1; r < R; ++r) {
        if (col >= 75) v += d_omegas[(long long)r * m * 85 + i];
        else if (mode == 2) v += dth0[(long long)r * set_stride + (long long)row * LDT + col];
        else if (col >= 3) v += dth0[(long long)r * set_stride + (long long)row * LDT + (col - 3)];
    }
    out[i] = v;
}

// d_omega_start[m, 85] = acc (or nothing) + the present regressor's d_theta_0
__global__ void ief_bwd_start_kernel(const float* __restrict__ acc, const float* __restrict__ dth0, float* __restrict__ out, int m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)m * 85) return;
    const float t = dth0[(i / 85) * LDT + (i % 85)];
    out[i] = acc ? acc[i] + t : t;
}

// out[n] = x[0][n] + x[1][n] + ... in stage order.  Grid y = problem.
__global__ void ief_stage_sum_kernel(const float* __restrict__ x, int stages, long long n, float* __restrict__ out, long long set_stride) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    x += (long long)blockIdx.y * set_stride;
    float v = x[i];
    for (int s = 1; s < stages; ++s) v += x[(long long)s * n + i];
    out[(long long)blockIdx.y * set_stride + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- the contraction
// nb problems of one shape through csrc/grad_mm.h: no window, one accumulator set, the IEF's row strides and keep_scale in the gate
template <bool A_T>
static int mm_launch(const MmPtrs& p, int nb, int M, int N, int K, int lda, int ldb, int ldc, int ldg, float gate_scale, hipStream_t s) {
    return grad_mm_launch<A_T, false, true, 1>("ief_mm_kernel", p, nb, M, N, K, lda, ldb, ldc, ldg, gate_scale, MmWindow{}, s);
}

// ---------------------------------------------------------------------------------------------------------------- the workspace
// One set per regressor (the stages of a buffer end to end), `set_bytes` apart: the grouped launches of the delta regressors step by it.
struct IefGradBufs {
    size_t pre, h1, h2, th, da1, da2, dth, da1sum, set_bytes;      // offsets inside a set: the forward's four, then the backward's
    size_t sets, sk, skbytes, omegas, g0, acc, total;
};
static IefGradBufs ief_grad_layout(int m, int R, int S) {
    IefGradBufs b; WsCarver set, c;
    const size_t wide = (size_t)m * 1024 * 4, narrow = (size_t)m * LDT * 4;
    b.pre = set.take(wide);
    b.h1 = set.take(S * wide);
    b.h2 = set.take(S * wide);
    b.th = set.take((S + 1) * narrow);
    b.da1 = set.take(S * wide);
    b.da2 = set.take(S * wide);
    b.dth = set.take((S + 1) * narrow);
    b.da1sum = set.take(wide);
    b.set_bytes = set.total();
    b.sets = c.take((size_t)R * b.set_bytes);
    b.skbytes = (size_t)(R > 2 ? R - 1 : 1) * hmmr_conv_splitk_workspace_bytes(m, 1024, IEF_SPLIT_K);
    b.sk = c.take(b.skbytes);
    b.omegas = c.take((size_t)R * m * 85 * 4);       // the recomputed omegas (hmmr_ief_bwd; the present one starts the deltas)
    b.g0 = c.take((size_t)m * 85 * 4);               // the present regressor's cotangent with the deltas' contributions
    b.acc = c.take((size_t)m * 85 * 4);              // the deltas' contributions to d_omega_start (delta_from_start)
    b.total = c.total();
    return b;
}

extern "C" size_t hmmr_ief_bwd_workspace_bytes(int m, int num_regressors, int num_stages) {
    if (m <= 0 || num_regressors < 1 || num_regressors > HMMR_MAX_REGRESSORS || num_stages < 1) return 0;
    return ief_grad_layout(m, num_regressors, num_stages).total;
}

// ---------------------------------------------------------------------------------------------------------------- shared checks
static int ief_train_check(const hmmr_ief_weights_t* w, const float* strips, const unsigned char* keep, float keep_scale, int m,
                           const void* ws, size_t ws_bytes, const char* who) {
    HMMR_REQUIRE(w && strips && ws, "%s: null argument", who);
    HMMR_REQUIRE(m > 0, "%s: m must be positive", who);
    HMMR_REQUIRE(w->dtype == HMMR_F32, "%s: the bank must be packed with dtype HMMR_F32 (it has dtype %d)", who, w->dtype);
    HMMR_REQUIRE(w->num_regressors >= 1 && w->num_regressors <= HMMR_MAX_REGRESSORS, "%s: bad num_regressors", who);
    HMMR_REQUIRE(w->num_stages >= 1, "%s: bad num_stages", who);
    HMMR_REQUIRE(w->mean_theta, "%s: null argument (mean_theta)", who);
    const int nd_delta = w->no_optcam ? 75 : 72;
    for (int r = 0; r < w->num_regressors; ++r) {
        const hmmr_ief_regressor_t& g = w->reg[r];
        HMMR_REQUIRE(g.nd == (r == 0 ? 85 : nd_delta), "%s: regressor %d has nd=%d (expected %d)", who, r, g.nd, r == 0 ? 85 : nd_delta);
        HMMR_REQUIRE(g.fc1_phi.w && g.fc1_phi.shift && g.fc1_theta.w && g.fc2.w && g.fc2.shift && g.fc3.w && g.fc3.shift,
                     "%s: null argument (a layer of regressor %d)", who, r);
        HMMR_REQUIRE(!g.fc1_phi.scale && !g.fc1_theta.scale && !g.fc2.scale && !g.fc3.scale,
                     "%s: regressor %d has a scaled layer: not an HMMR_F32 bank", who, r);
    }
    HMMR_REQUIRE(!keep || (isfinite(keep_scale) && keep_scale > 0.f), "%s: keep is given and keep_scale=%g is not a positive finite number", who,
                 (double)keep_scale);
    const size_t need = ief_grad_layout(m, w->num_regressors, w->num_stages).total;
    HMMR_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes given, %zu needed)", who, ws_bytes, need);
    return 0;
}

struct Strides { long long w, scale, shift; };
// the delta regressors' filter banks and vectors at one common, 16-byte aligned stride per layer (csrc/ief.hip's condition)
static bool ief_grouped(const hmmr_ief_weights_t* w, Strides (&st)[4]) {
    static const hmmr_layer_t hmmr_ief_regressor_t::* lay[4] = {&hmmr_ief_regressor_t::fc1_phi, &hmmr_ief_regressor_t::fc1_theta,
                                                               &hmmr_ief_regressor_t::fc2, &hmmr_ief_regressor_t::fc3};
    if (w->num_regressors < 3 || hmmr_debug_state()->ief_no_group) return false;
    for (int l = 0; l < 4; ++l) {
        st[l] = Strides{0, 0, 0};
        for (int r = 2; r < w->num_regressors; ++r) {
            const hmmr_layer_t& a = w->reg[r - 1].*lay[l]; const hmmr_layer_t& b = w->reg[r].*lay[l];
            const Strides cur = {(const char*)b.w - (const char*)a.w, a.scale ? (const char*)b.scale - (const char*)a.scale : 0,
                                 a.shift ? (const char*)b.shift - (const char*)a.shift : 0};
            if (!a.scale != !b.scale || !a.shift != !b.shift) return false;
            if (r > 2 && (cur.w != st[l].w || cur.scale != st[l].scale || cur.shift != st[l].shift)) return false;
            st[l] = cur;
        }
        if ((st[l].w | st[l].scale | st[l].shift) & 15) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the forward
// Both entry points run this.  It leaves in every regressor's set: pre, the masked h1 / h2 of every stage, theta_0 .. theta_S; and the
// omegas in `omegas` [R][m][85].  The GEMMs are csrc/ief.hip's launches (csrc/tail_sched.h's fc_desc with HMMR_F32), so keep == NULL is
// hmmr_ief_fwd_from.
static int ief_train_forward(const hmmr_ief_weights_t* w, const float* strips, const float* omega_start, const unsigned char* keep,
                             float keep_scale, int m, float* omegas, const IefGradBufs& L, char* base, bool grouped, const Strides (&st)[4],
                             hipStream_t s) {
    const int S = w->num_stages, R = w->num_regressors;
    const int nd_delta = w->no_optcam ? 75 : 72;
    const long long set_f = (long long)(L.set_bytes / 4), set_b = (long long)L.set_bytes;
    const long long wide = (long long)m * 1024, narrow = (long long)m * LDT;
    const float* start = omega_start ? omega_start : w->mean_theta;
    const int ld_start = omega_start ? 85 : 0;
    const float* dsrc = w->delta_from_start ? start : (const float*)omegas;
    const int ld_d = w->delta_from_start ? ld_start : 85;
    const unsigned gth = (unsigned)((narrow * (S + 1) + 255) / 256), gfin = (unsigned)(((long long)m * 85 + 255) / 256);
    const unsigned gkeep = (unsigned)((wide + 255) / 256);
    const long long keep_reg = (long long)S * 2 * wide;          // bytes of one regressor's masks
    auto run = [&](int r, int nb, bool grp) -> int {
        const hmmr_ief_regressor_t& Rg = w->reg[r];
        char* set = base + L.sets + (size_t)r * L.set_bytes;
        float* pre = (float*)(set + L.pre); float* h1 = (float*)(set + L.h1); float* h2 = (float*)(set + L.h2); float* th = (float*)(set + L.th);
        auto group = [&](hmmr_conv_desc_t& d, const Strides& z, bool in_sets, bool res_sets) {
            if (!grp) return;
            d.batch = nb; d.batch_in_bytes = in_sets ? set_b : 0; d.batch_w_bytes = z.w; d.batch_out_bytes = set_b;
            d.batch_res_bytes = res_sets ? set_b : 0; d.batch_scale_bytes = z.scale; d.batch_shift_bytes = z.shift;
        };
        if (r == 0)
            hipLaunchKernelGGL(ief_train_init_theta_kernel, dim3(gth, 1), dim3(256), 0, s, start, ld_start, 0, 85, th, m, S + 1, set_f);
        else
            hipLaunchKernelGGL(ief_train_init_theta_kernel, dim3(gth, nb), dim3(256), 0, s, dsrc, ld_d, w->no_optcam ? 0 : 3, nd_delta, th, m,
                               S + 1, set_f);
        HMMR_CHECK_HIP(hipGetLastError());
        hmmr_conv_desc_t d = fc_desc(strips, HMMR_F32, m, 2048, Rg.fc1_phi, pre, HMMR_F32, 1024, 1024, IEF_SPLIT_K, base + L.sk, L.skbytes);
        group(d, st[0], false, false);
        if (hmmr_conv_gemm(&d, s)) return -2;
        for (int t = 0; t < S; ++t) {
            float* th_t = th + t * narrow; float* h1_t = h1 + t * wide; float* h2_t = h2 + t * wide;
            d = fc_desc(th_t, HMMR_F32, m, LDT, Rg.fc1_theta, h1_t, HMMR_F32, 1024, 1024);
            d.res = pre; d.ldr = 1024; d.relu = 1;
            group(d, st[1], true, true);
            if (hmmr_conv_gemm(&d, s)) return -2;
            if (keep) {
                hipLaunchKernelGGL(ief_keep_kernel, dim3(gkeep, nb), dim3(256), 0, s, h1_t, keep + r * keep_reg + (long long)(2 * t) * wide,
                                   keep_scale, wide, set_f, keep_reg);
                HMMR_CHECK_HIP(hipGetLastError());
            }
            d = fc_desc(h1_t, HMMR_F32, m, 1024, Rg.fc2, h2_t, HMMR_F32, 1024, 1024, IEF_SPLIT_K, base + L.sk, L.skbytes);
            d.relu = 1;
            group(d, st[2], true, false);
            if (hmmr_conv_gemm(&d, s)) return -2;
            if (keep) {
                hipLaunchKernelGGL(ief_keep_kernel, dim3(gkeep, nb), dim3(256), 0, s, h2_t, keep + r * keep_reg + (long long)(2 * t + 1) * wide,
                                   keep_scale, wide, set_f, keep_reg);
                HMMR_CHECK_HIP(hipGetLastError());
            }
            d = fc_desc(h2_t, HMMR_F32, m, 1024, Rg.fc3, th_t + narrow, HMMR_F32, Rg.nd, LDT, IEF_SPLIT_K, base + L.sk, L.skbytes);
            d.res = th_t; d.ldr = LDT;
            group(d, st[3], true, true);
            if (hmmr_conv_gemm(&d, s)) return -2;
        }
        hipLaunchKernelGGL(ief_finalize_kernel, dim3(gfin, nb), dim3(256), 0, s, (const float*)(th + S * narrow), dsrc, ld_d,
                           r == 0 ? 0 : (w->no_optcam ? 2 : 1), omegas + (size_t)r * m * 85, m, set_f);
        HMMR_CHECK_HIP(hipGetLastError());
        return 0;
    };
    if (run(0, 1, false)) return -2;
    if (grouped) return run(1, R - 1, true);
    for (int r = 1; r < R; ++r)
        if (run(r, 1, false)) return -2;
    return 0;
}

extern "C" int hmmr_ief_fwd_train(const hmmr_ief_weights_t* w, const float* strips, const float* omega_start, const unsigned char* keep,
                                  float keep_scale, int m, float* omegas, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = ief_train_check(w, strips, keep, keep_scale, m, ws, ws_bytes, "hmmr_ief_fwd_train")) return rc;
    HMMR_REQUIRE(omegas, "hmmr_ief_fwd_train: null argument");
    Strides st[4] = {};
    const bool grouped = ief_grouped(w, st);
    return ief_train_forward(w, strips, omega_start, keep, keep ? keep_scale : 1.f, m, omegas, ief_grad_layout(m, w->num_regressors, w->num_stages),
                             (char*)ws, grouped, st, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- the backward
extern "C" int hmmr_ief_bwd(const hmmr_ief_weights_t* w, const hmmr_ief_bwd_desc_t* d, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(d, "hmmr_ief_bwd: null descriptor");
    if (int rc = ief_train_check(w, d->strips, d->keep, d->keep_scale, d->m, ws, ws_bytes, "hmmr_ief_bwd")) return rc;
    HMMR_REQUIRE(d->d_omegas, "hmmr_ief_bwd: null argument");
    const int R = w->num_regressors, S = w->num_stages, m = d->m;
    bool want_w[G] = {}, any = d->d_strips || d->d_omega_start;
    for (int r = 0; r < R; ++r) {
        const hmmr_ief_reg_grads_t& g = d->reg[r];
        want_w[r] = g.d_fc1_phi || g.d_fc1_theta || g.d_fc2 || g.d_fc3 || g.d_b1 || g.d_b2 || g.d_b3;
        any = any || want_w[r];
    }
    HMMR_REQUIRE(any, "hmmr_ief_bwd: no output is requested");
    const IefGradBufs L = ief_grad_layout(m, R, S);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    Strides st[4] = {};
    const bool grouped = ief_grouped(w, st);
    const float scale = d->keep ? d->keep_scale : 1.f;
    float* omegas = (float*)(base + L.omegas);
    if (ief_train_forward(w, d->strips, d->omega_start, d->keep, scale, m, omegas, L, base, grouped, st, s)) return -2;

    const long long set_f = (long long)(L.set_bytes / 4);
    const long long wide = (long long)m * 1024, narrow = (long long)m * LDT;
    const unsigned gn = (unsigned)((narrow + 255) / 256), g85 = (unsigned)(((long long)m * 85 + 255) / 256), gw = (unsigned)((wide + 255) / 256);
    auto F = [&](int r, size_t off) { return (float*)(base + L.sets + (size_t)r * L.set_bytes + off); };
    const int mode_delta = w->no_optcam ? 2 : 1;
    // the chain of regressors r .. r + nb - 1 (one shape) from their d_omega `cot` ([nb][m][85]): d_a1 / d_a2 / d_theta of every stage
    // into their sets, then their weight gradients
    auto chain = [&](int r, int nb, const float* cot, int mode) -> int {
        hipLaunchKernelGGL(ief_bwd_init_kernel, dim3(gn, nb), dim3(256), 0, s, cot, mode, F(r, L.dth) + S * narrow, m, set_f);
        HMMR_CHECK_HIP(hipGetLastError());
        for (int t = S - 1; t >= 0; --t) {
            MmPtrs p = {};
            // d_a2 = (d_theta_{t+1} . W3) gated by h2
            for (int z = 0; z < nb; ++z) {
                p.a[z] = F(r + z, L.dth) + (t + 1) * narrow; p.b[z] = (const float*)w->reg[r + z].fc3.w;
                p.c[z] = F(r + z, L.da2) + t * wide; p.gate[z] = F(r + z, L.h2) + t * wide;
            }
            if (mm_launch<false>(p, nb, m, 1024, LDT, LDT, 1024, 1024, 1024, scale, s)) return -2;
            // d_a1 = (d_a2 . W2) gated by h1
            p = MmPtrs{};
            for (int z = 0; z < nb; ++z) {
                p.a[z] = F(r + z, L.da2) + t * wide; p.b[z] = (const float*)w->reg[r + z].fc2.w;
                p.c[z] = F(r + z, L.da1) + t * wide; p.gate[z] = F(r + z, L.h1) + t * wide;
            }
            if (mm_launch<false>(p, nb, m, 1024, 1024, 1024, 1024, 1024, 1024, scale, s)) return -2;
            // d_theta_t = d_theta_{t+1} + d_a1 . W1[2048:]
            p = MmPtrs{};
            for (int z = 0; z < nb; ++z) {
                p.a[z] = F(r + z, L.da1) + t * wide; p.b[z] = (const float*)w->reg[r + z].fc1_theta.w;
                p.c[z] = F(r + z, L.dth) + t * narrow; p.res[z] = F(r + z, L.dth) + (t + 1) * narrow;
            }
            if (mm_launch<false>(p, nb, m, LDT, 1024, 1024, LDT, LDT, 0, 1.f, s)) return -2;
        }
        bool sum = d->d_strips != nullptr, wany = false;
        for (int z = 0; z < nb; ++z) { sum = sum || d->reg[r + z].d_fc1_phi; wany = wany || want_w[r + z]; }
        if (sum) {
            hipLaunchKernelGGL(ief_stage_sum_kernel, dim3(gw, nb), dim3(256), 0, s, (const float*)F(r, L.da1), S, wide, F(r, L.da1sum), set_f);
            HMMR_CHECK_HIP(hipGetLastError());
        }
        if (!wany) return 0;
        // weight gradients: one launch per layer over all stages; a NULL output's problem is skipped, a layer nobody asks for is not queued
        auto layer = [&](size_t a_off, long long a_skip, int M, size_t b_off, long long b_skip, const float* b_shared, int N, int K,
                         float* hmmr_ief_reg_grads_t::*out) -> int {
            MmPtrs p = {}; bool q = false;
            for (int z = 0; z < nb; ++z) {
                p.a[z] = F(r + z, a_off) + a_skip; p.b[z] = b_shared ? b_shared : F(r + z, b_off) + b_skip;
                p.c[z] = d->reg[r + z].*out; q = q || p.c[z];
            }
            return q ? mm_launch<true>(p, nb, M, N, K, M == LDT ? LDT : 1024, N == LDT ? LDT : N, N, 0, 1.f, s) : 0;
        };
        if (layer(L.dth, narrow, LDT, L.h2, 0, nullptr, 1024, S * m, &hmmr_ief_reg_grads_t::d_fc3)) return -2;
        if (layer(L.da2, 0, 1024, L.h1, 0, nullptr, 1024, S * m, &hmmr_ief_reg_grads_t::d_fc2)) return -2;
        if (layer(L.da1, 0, 1024, L.th, 0, nullptr, LDT, S * m, &hmmr_ief_reg_grads_t::d_fc1_theta)) return -2;
        if (layer(L.da1sum, 0, 1024, 0, 0, d->strips, 2048, m, &hmmr_ief_reg_grads_t::d_fc1_phi)) return -2;
        auto bias = [&](size_t a_off, long long a_skip, int N, float* hmmr_ief_reg_grads_t::*out) -> int {
            CsPtrs p = {}; bool q = false;
            for (int z = 0; z < nb; ++z) { p.a[z] = F(r + z, a_off) + a_skip; p.out[z] = d->reg[r + z].*out; q = q || p.out[z]; }
            return q ? grad_colsum_launch(p, nb, S * m, N, N, s) : 0;
        };
        if (bias(L.dth, narrow, LDT, &hmmr_ief_reg_grads_t::d_b3)) return -2;
        if (bias(L.da2, 0, 1024, &hmmr_ief_reg_grads_t::d_b2)) return -2;
        if (bias(L.da1, 0, 1024, &hmmr_ief_reg_grads_t::d_b1)) return -2;
        return 0;
    };
    // d_strips (+)= d_a1sum_r . W1_r[:2048], one regressor after the other in the order of the backward
    bool strips_written = false;
    auto strips_grad = [&](int r) -> int {
        if (!d->d_strips) return 0;
        MmPtrs p = {};
        p.a[0] = F(r, L.da1sum); p.b[0] = (const float*)w->reg[r].fc1_phi.w; p.c[0] = d->d_strips; p.res[0] = strips_written ? d->d_strips : nullptr;
        strips_written = true;
        return mm_launch<false>(p, 1, m, 2048, 1024, 1024, 2048, 2048, 0, 1.f, s);
    };
    // a regressor nobody needs is not run: the present one feeds d_strips, d_omega_start and its own weights, a delta those and -- through
    // its start (use_delta_from_pred) -- whatever the present one feeds
    const bool shared = d->d_strips || d->d_omega_start;
    const bool need0 = shared || want_w[0];
    bool need[G] = {}, need_delta = false;
    for (int r = 1; r < R; ++r) { need[r] = shared || want_w[r] || (!w->delta_from_start && need0); need_delta = need_delta || need[r]; }
    // 1. the delta regressors, in regressor order
    if (need_delta) {
        if (grouped) { if (chain(1, R - 1, d->d_omegas + (size_t)m * 85, mode_delta)) return -2; }
        else for (int r = 1; r < R; ++r) if (need[r] && chain(r, 1, d->d_omegas + (size_t)r * m * 85, mode_delta)) return -2;
        for (int r = 1; r < R; ++r) if (strips_grad(r)) return -2;
    }
    // 2. what they pass to their starting omega, added in that order: to the present regressor's cotangent (use_delta_from_pred) or to
    //    d_omega_start (delta_from_start)
    const float* cot0 = d->d_omegas;
    const float* acc = nullptr;
    if (R > 1 && (w->delta_from_start ? d->d_omega_start != nullptr : need0)) {
        float* out = (float*)(base + (w->delta_from_start ? L.acc : L.g0));
        hipLaunchKernelGGL(ief_bwd_gather_kernel, dim3(g85), dim3(256), 0, s, w->delta_from_start ? (const float*)nullptr : d->d_omegas, d->d_omegas,
                           (const float*)F(0, L.dth), set_f, R, mode_delta, out, m);
        HMMR_CHECK_HIP(hipGetLastError());
        if (w->delta_from_start) acc = out; else cot0 = out;
    }
    // 3. the present regressor
    if (!need0) return 0;
    if (chain(0, 1, cot0, 0)) return -2;
    if (strips_grad(0)) return -2;
    if (d->d_omega_start) {
        hipLaunchKernelGGL(ief_bwd_start_kernel, dim3(g85), dim3(256), 0, s, acc, (const float*)F(0, L.dth), d->d_omega_start, m);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
