// What the forward of the tail (f_movie, the hallucinator, the IEF regressors) queues, stated once: its constants, the descriptors it hands
// hmmr_conv_gemm and the two device helpers its launches share.  csrc/temporal.hip and csrc/ief.hip build the inference forward from
// these; csrc/movie_grad.hip and csrc/ief_grad.hip call the same builders with HMMR_F32 for the forward they recompute, so a retuned
// split or tile reaches the function the backward differentiates.
#pragma once
#include "common.h"
#include "hmmr_hip.h"

// ---------------------------------------------------------------------------------------------------------------- f_movie / hallucinator
static constexpr int TAIL_C = 2048;      // channels of phi, of every layer of both modules
static constexpr float GN_EPS = 1e-6f;
static constexpr int GN_GROUPS = 32;
// K = 3*2048 is long and M = b*t is short (640 rows for 32 windows): 4 K-slices quadruple the
// number of workgroups.  Fixed per layer and operand mode, never derived from b, so a window's result does not
// depend on how many windows share the launch.  Split operands: 5 slices of the 128x256 ring tile (40 tiles x 5 = 200
// workgroups on 256 CUs, 39 K steps each) measured 0.427 ms per f_movie pass of 32 windows against 0.477 for 4 slices
// of the 256x128 tile (tools/stage_bench.py, round 3; 6 / 8 slices and the two-stage tiles are slower).
static constexpr int TEMPORAL_SPLIT_K_MAX = 5;
static inline int temporal_split_k(int dtype) { return dtype == HMMR_F16X3 ? 5 : 4; }
static constexpr int HAL_SPLIT_K = 4;    // (the hallucinator keeps 4 slices in every mode)

// the sum of v over a workgroup of 256 threads, in one fixed order: GroupNorm's statistics, forward and backward
__device__ __forceinline__ float block_sum_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                       // protect `red` from the previous use
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// one [3,1] SAME convolution of a temporal block on [b, t, 1, 2048]: out = conv(in, l) (+ res); the operands take in_dtype, out is fp32
static inline hmmr_conv_desc_t temporal_conv_desc(const void* in, int in_dtype, const hmmr_layer_t& l, const float* res, float* out, int b, int t,
                                                  void* sk, size_t skbytes) {
    constexpr int C = TAIL_C;
    hmmr_conv_desc_t d = {};
    d.in = in; d.w = l.w; d.scale = l.scale; d.shift = l.shift; d.tile = l.tile;
    d.out = out; d.in_dtype = in_dtype; d.out_dtype = HMMR_F32;
    d.n_img = b; d.hin = t; d.win = 1; d.cin = C;
    d.in_img_stride = (int64_t)t * C; d.in_row_stride = C; d.in_px_stride = C;
    d.kh = 3; d.kw = 1; d.sy = d.sx = 1; d.py = 1; d.px = 0; d.ho = t; d.wo = 1; d.cout = C; d.ldo = C;
    d.split_k = temporal_split_k(in_dtype); d.ws = sk; d.ws_bytes = skbytes;
    if (res) { d.res = res; d.ldr = C; }      // (ldr is read only with a residual; each builder sets it as the inference forward did)
    return d;
}

// ---------------------------------------------------------------------------------------------------------------- fully-connected layers
// out[m][cout] (row stride ldo) = in[m][k] . l, in `split_k` K-slices through the planes at sk (0: no split)
static inline hmmr_conv_desc_t fc_desc(const void* in, int in_dtype, int m, int k, const hmmr_layer_t& l, void* out, int out_dtype, int cout,
                                       int ldo, int split_k = 0, void* sk = nullptr, size_t skbytes = 0) {
    hmmr_conv_desc_t d = {};
    d.in = in; d.w = l.w; d.scale = l.scale; d.shift = l.shift; d.out = out;
    d.in_dtype = in_dtype; d.out_dtype = out_dtype;
    d.n_img = m; d.hin = d.win = 1; d.cin = k;
    d.in_img_stride = k; d.in_row_stride = k; d.in_px_stride = k;
    d.kh = d.kw = 1; d.sy = d.sx = 1; d.ho = d.wo = 1; d.cout = cout; d.ldo = ldo;
    if (split_k) { d.split_k = split_k; d.ws = sk; d.ws_bytes = skbytes; }
    return d;
}
// a 2048 x 2048 layer of the hallucinator: out = [relu](in . l) (+ res)
static inline hmmr_conv_desc_t hal_fc_desc(const void* in, int in_dtype, const hmmr_layer_t& l, void* out, int out_dtype, int m, int relu,
                                           const float* res, void* sk, size_t skbytes) {
    hmmr_conv_desc_t d = fc_desc(in, in_dtype, m, TAIL_C, l, out, out_dtype, TAIL_C, TAIL_C, HAL_SPLIT_K, sk, skbytes);
    d.relu = relu; d.res = res; d.ldr = TAIL_C;
    return d;
}

// ---------------------------------------------------------------------------------------------------------------- IEF
static constexpr int LDT = 128;      // row stride of the zero-padded theta state
// The K = 2048 / 1024 GEMMs have at most m/64 x 16 output tiles (m = kept frames of a step, a few
// hundred): 4 K-slices fill the chip.  Fixed per layer so a row's result is batch-independent.
static constexpr int IEF_SPLIT_K = 4;

// omega_out[m, 85] from the last theta, defined in csrc/ief.hip and launched from there and from csrc/ief_grad.hip.  It is declared
// here and not defined: a kernel defined in a header is emitted into every file that includes it, used or not, and csrc/temporal.hip
// and csrc/ief.hip keep the device code they had.  A launch is host code, so it needs no more than this declaration -- as long as both
// files are linked into the one library: the launch in csrc/ief_grad.hip resolves to the host-side kernel handle csrc/ief.hip's object
// defines and registers with its own code object.  It is the only kernel of the tree launched from a second file.
__global__ void ief_finalize_kernel(const float* __restrict__ theta, const float* __restrict__ bsrc, int ld_b, int mode,
                                    float* __restrict__ out, int m, long long th_stride);
