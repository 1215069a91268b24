// f_movie temporal encoder for gfx950: az_fc2_groupnorm / az_fc_block2
// (src/models.py:121-228).  Per residual block, on a [b, t, 1, 2048] tensor:
//   GN(32 groups, stats over time x 64 channels, eps 1e-6) -> ReLU ->
//   conv [3,1] SAME + bias -> GN -> ReLU -> conv [3,1] SAME + bias -> + input
// The two convolutions run through the implicit-GEMM kernel (M = b*t,
// K = 3*2048, N = 2048; zero rows outside the window come from its bounds
// check); the residual trunk and the GN statistics stay fp32 in every mode,
// only the GEMM operands take the struct's dtype.
#include "common.h"
#include "hmmr_hip.h"
#include "tail_sched.h"
#include "workspace.h"

// One workgroup per (window b, group g).  tf.contrib.layers.group_norm with
// reduction_axes=(-3,-2) on [b,t,1,c]: mean and POPULATION variance over
// (t, c/groups); gain = rsqrt(var+eps)*gamma; offset = -mean*gain + beta.
template <typename TO>
__global__ __launch_bounds__(256) void groupnorm_relu_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             TO* __restrict__ out, int t, int c, int groups) {
    __shared__ float red[4];
    const int cpg = c / groups;
    const int b = blockIdx.x / groups, g = blockIdx.x % groups;
    const int cnt = t * cpg;
    const float* xb = x + (long long)b * t * c + g * cpg;
    float s = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) s += xb[(i / cpg) * c + (i % cpg)];
    const float mean = block_sum_256(s, red) / (float)cnt;
    float q = 0.f;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const float d = xb[(i / cpg) * c + (i % cpg)] - mean;
        q += d * d;
    }
    const float var = block_sum_256(q, red) / (float)cnt;
    const float rstd = rsqrtf(var + GN_EPS);
    TO* ob = out + (long long)b * t * c + g * cpg;
    const int v8 = cpg / 8;                // 8-channel vectors per row of the group (cpg % 8 == 0, host-checked)
    for (int i = threadIdx.x; i < t * v8; i += 256) {
        const int tt = i / v8, j = (i % v8) * 8;
        float xv[8], gm[8], bt[8], o[8];
        load8(xb + tt * c + j, xv); load8(gamma + g * cpg + j, gm); load8(beta + g * cpg + j, bt);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // x*gain + (beta - mean*gain) evaluated as (x - mean)*gain + beta: same value,
            // without the cancellation of two large products when var -> 0
            const float gain = rstd * gm[e];
            o[e] = fmaxf((xv[e] - mean) * gain + bt[e], 0.f);
        }
        store8(ob + tt * c + j, o);
    }
}

extern "C" int hmmr_groupnorm_relu(const float* x, const float* gamma, const float* beta, int b, int t,
                                   int c, int groups, void* out, int out_dtype, void* stream) {
    HMMR_REQUIRE(x && gamma && beta && out, "hmmr_groupnorm_relu: null argument");
    HMMR_REQUIRE(b > 0 && t > 0 && groups > 0 && c % groups == 0 && (c / groups) % 8 == 0,
                 "hmmr_groupnorm_relu: bad shape (channels per group must be a multiple of 8)");
    hipStream_t s = (hipStream_t)stream;
    if (out_dtype == HMMR_BF16)
        hipLaunchKernelGGL(groupnorm_relu_kernel<bf16_t>, dim3(b * groups), dim3(256), 0, s, x, gamma, beta,
                           (bf16_t*)out, t, c, groups);
    else if (out_dtype == HMMR_F32)
        hipLaunchKernelGGL(groupnorm_relu_kernel<float>, dim3(b * groups), dim3(256), 0, s, x, gamma, beta,
                           (float*)out, t, c, groups);
    else if (out_dtype == HMMR_F16X3)
        hipLaunchKernelGGL(groupnorm_relu_kernel<bsplit_t>, dim3(b * groups), dim3(256), 0, s, x, gamma, beta,
                           (bsplit_t*)out, t, c, groups);
    else { hmmr_set_error("hmmr_groupnorm_relu: bad dtype %d", out_dtype); return -1; }
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// One layout for both f_movie stages: `nop` row buffers [m][2048] of the operand dtype, then `nf32` fp32 ones, then the split-K partial planes
struct MovieBufs { size_t buf[4], sk, skbytes, total; };
static MovieBufs movie_layout(size_t m, int dtype, int nop, int nf32) {
    MovieBufs l = {}; WsCarver c;
    for (int i = 0; i < nop + nf32; ++i) l.buf[i] = c.take(m * 2048 * (i < nop && dtype == HMMR_BF16 ? 2 : 4));
    l.skbytes = hmmr_conv_splitk_workspace_bytes((int)m, 2048, TEMPORAL_SPLIT_K_MAX);
    l.sk = c.take(l.skbytes);
    l.total = c.total();
    return l;
}
static MovieBufs temporal_layout(int b, int t, int dtype) { return movie_layout((size_t)b * t, dtype, 1, 3); }      // h | h1, net[0], net[1]
static MovieBufs hallucinator_layout(int m, int dtype) { return movie_layout((size_t)m, dtype, 3, 0); }             // x, h1, h2

extern "C" size_t hmmr_temporal_workspace_bytes(int b, int t, int dtype) {
    return b > 0 && t > 0 ? temporal_layout(b, t, dtype).total : 0;
}

extern "C" int hmmr_temporal_fwd(const hmmr_temporal_weights_t* w, const float* phi, int b, int t,
                                 float* strips, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(w && phi && strips && ws, "hmmr_temporal_fwd: null argument");
    HMMR_REQUIRE(b > 0 && t > 0, "hmmr_temporal_fwd: bad shape");
    HMMR_REQUIRE(w->num_blocks >= 1 && w->num_blocks <= HMMR_MAX_TEMPORAL_BLOCKS, "hmmr_temporal_fwd: bad num_blocks");
    const MovieBufs L = temporal_layout(b, t, w->dtype);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_temporal_fwd: workspace too small");
    constexpr int C = TAIL_C;
    char* base = (char*)ws;
    void* h = base + L.buf[0];
    float *h1 = (float*)(base + L.buf[1]), *net[2] = {(float*)(base + L.buf[2]), (float*)(base + L.buf[3])};
    const float* cur = phi;
    for (int i = 0; i < w->num_blocks; ++i) {
        const hmmr_temporal_block_t& B = w->block[i];
        float* dst = (i == w->num_blocks - 1) ? strips : net[i & 1];
        if (hmmr_groupnorm_relu(cur, B.gn1_gamma, B.gn1_beta, b, t, C, GN_GROUPS, h, w->dtype, stream)) return -2;
        hmmr_conv_desc_t d = temporal_conv_desc(h, w->dtype, B.conv1, nullptr, h1, b, t, base + L.sk, L.skbytes);
        if (hmmr_conv_gemm(&d, stream)) return -2;
        if (hmmr_groupnorm_relu(h1, B.gn2_gamma, B.gn2_beta, b, t, C, GN_GROUPS, h, w->dtype, stream)) return -2;
        d = temporal_conv_desc(h, w->dtype, B.conv2, cur, dst, b, t, base + L.sk, L.skbytes);      // residual adds the BLOCK INPUT (models.py:226)
        if (hmmr_conv_gemm(&d, stream)) return -2;
        cur = dst;
    }
    return 0;
}

// ------------------------------------------------------------------------- //
// Hallucinator fc2_res (src/models.py:270-296, pred_mode == 'hal'):
//   phi + fc3(relu(fc2(relu(fc1(phi)))))     three 2048x2048 fully-connected layers.
extern "C" size_t hmmr_hallucinator_workspace_bytes(int m, int dtype) {
    return m > 0 ? hallucinator_layout(m, dtype).total : 0;
}

template <typename TO>
__global__ void hal_cast_kernel(const float* __restrict__ in, TO* __restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float v[8];
    load8(in + i * 8, v);
    store8(out + i * 8, v);
}

extern "C" int hmmr_hallucinator_fwd(const hmmr_hallucinator_weights_t* w, const float* phi, int m,
                                     float* out, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(w && phi && out && ws, "hmmr_hallucinator_fwd: null argument");
    HMMR_REQUIRE(m > 0, "hmmr_hallucinator_fwd: m must be positive");
    const MovieBufs L = hallucinator_layout(m, w->dtype);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_hallucinator_fwd: workspace too small");
    constexpr int C = TAIL_C;
    char* base = (char*)ws;
    void *x = base + L.buf[0], *h1 = base + L.buf[1], *h2 = base + L.buf[2];
    hipStream_t s = (hipStream_t)stream;
    const void* xin = phi;
    if (w->dtype != HMMR_F32) {
        const long long n8 = (long long)m * C / 8;
        if (w->dtype == HMMR_BF16)
            hipLaunchKernelGGL(hal_cast_kernel<bf16_t>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, phi, (bf16_t*)x, n8);
        else
            hipLaunchKernelGGL(hal_cast_kernel<bsplit_t>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, phi, (bsplit_t*)x, n8);
        HMMR_CHECK_HIP(hipGetLastError());
        xin = x;
    }
    auto fc = [&](const void* in, const hmmr_layer_t& l, void* o, int odt, int relu, const float* res) {
        hmmr_conv_desc_t d = hal_fc_desc(in, w->dtype, l, o, odt, m, relu, res, base + L.sk, L.skbytes);
        return hmmr_conv_gemm(&d, s);
    };
    if (fc(xin, w->fc1, h1, w->dtype, 1, nullptr)) return -2;
    if (fc(h1, w->fc2, h2, w->dtype, 1, nullptr)) return -2;
    if (fc(h2, w->fc3, out, HMMR_F32, 0, phi)) return -2;      // + phi (models.py:295)
    return 0;
}
