// TF 1.x Adam for gfx950: one fused pass over the trainable tensors of a step (include/hmmr_hip.h, "TF Adam").  Per value the pass
// reads p, g, m, v and writes p, m, v -- 28 bytes and a dozen fp32 operations: the design is about bandwidth and about nothing else.
//
//   launch form  one launch per 64 active segments; their descriptors travel as kernel arguments (as csrc/windows.hip passes its
//                64 track offsets): no device table, no upload, no synchronisation.  A segment is cut into chunks of ADAM_CHUNK
//                values; workgroups map to (segment, chunk) through the prefix table `first` (a wave-uniform binary search), the
//                grid is capped at ADAM_MAX_BLOCKS and strides over the chunks.
//   two paths    a segment whose four pointers are all 16-byte aligned moves 16 bytes per lane (a chunk starts a multiple of 4
//                values into its segment, so the chunk is aligned like the segment); every other segment moves 4 bytes per lane.
//                The arithmetic is the same scalar sequence in both, so a value does not depend on the path it took.
//   arithmetic   this file is compiled with -ffp-contract=off: nothing is fused into an fma, and the division and the square root
//                are the correctly rounded IEEE sequences -- the result is held to the bytes of a float32 NumPy restatement.
//   no atomic, no cross-lane traffic: every value is owned by one lane of one workgroup, so the same inputs give the same bytes
//   and a value does not depend on how the tensors were cut into segments.
#include <math.h>

#include "common.h"
#include "hmmr_hip.h"

static constexpr int ADAM_SEGS = 64;             // segments per launch
static constexpr int ADAM_THREADS = 256;
static constexpr int ADAM_CHUNK = 4096;          // values per (segment, chunk) work item: 4 x 16 bytes per lane and array
static constexpr int ADAM_MAX_BLOCKS = 2048;     // 256 CUs x 8 workgroups

struct AdamTable {
    float* p[ADAM_SEGS];
    const float* g[ADAM_SEGS];
    float* m[ADAM_SEGS];
    float* v[ADAM_SEGS];
    long long n[ADAM_SEGS];
    long long first[ADAM_SEGS + 1];              // chunks in front of segment s; [count] = all chunks; entries past count repeat it
    unsigned long long vec;                      // bit s: all four pointers of segment s are 16-byte aligned
    int count;
    float alpha, one_minus_beta1, one_minus_beta2, eps;
};

// the TF 1.x ApplyAdam functor, operation by operation in fp32
__device__ __forceinline__ void adam_value(float& p, float g, float& m, float& v, float alpha, float omb1, float omb2, float eps) {
    m = m + (g - m) * omb1;
    v = v + (g * g - v) * omb2;
    p = p - (m * alpha) / (sqrtf(v) + eps);
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(const AdamTable A) {
    const long long total = A.first[A.count];
    const int tid = threadIdx.x;
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        // the segment of chunk c: the last s with first[s] <= c (first is non-decreasing, first[0] = 0, c < first[count])
        int lo = 0, hi = A.count - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (A.first[mid] <= c) lo = mid; else hi = mid - 1;
        }
        const int s = lo;
        const long long base = (c - A.first[s]) * ADAM_CHUNK;
        const long long left = A.n[s] - base;
        const int cnt = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;
        float* __restrict__ p = A.p[s] + base;
        const float* __restrict__ g = A.g[s] + base;
        float* __restrict__ m = A.m[s] + base;
        float* __restrict__ v = A.v[s] + base;
        if ((A.vec >> s) & 1ull) {
            const int quads = cnt >> 2;
            for (int q = tid; q < quads; q += ADAM_THREADS) {
                f32x4 pp = ((const f32x4*)p)[q], mm = ((const f32x4*)m)[q], vv = ((const f32x4*)v)[q];
                const f32x4 gg = ((const f32x4*)g)[q];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float a = pp[i], b = mm[i], d = vv[i];
                    adam_value(a, gg[i], b, d, A.alpha, A.one_minus_beta1, A.one_minus_beta2, A.eps);
                    pp[i] = a; mm[i] = b; vv[i] = d;
                }
                ((f32x4*)p)[q] = pp; ((f32x4*)m)[q] = mm; ((f32x4*)v)[q] = vv;
            }
            const int i = (quads << 2) + tid;    // the chunk's last 0..3 values (the segment's: every other chunk is whole)
            if (tid < (cnt & 3)) {
                float a = p[i], b = m[i], d = v[i];
                adam_value(a, g[i], b, d, A.alpha, A.one_minus_beta1, A.one_minus_beta2, A.eps);
                p[i] = a; m[i] = b; v[i] = d;
            }
        } else {
            for (int i = tid; i < cnt; i += ADAM_THREADS) {
                float a = p[i], b = m[i], d = v[i];
                adam_value(a, g[i], b, d, A.alpha, A.one_minus_beta1, A.one_minus_beta2, A.eps);
                p[i] = a; m[i] = b; v[i] = d;
            }
        }
    }
}

extern "C" int hmmr_adam_step(const hmmr_adam_seg_t* segs, int n_segs, const hmmr_adam_hyper_t* h, void* stream) {
    HMMR_REQUIRE(h, "hmmr_adam_step: null hyper-parameters");
    HMMR_REQUIRE(n_segs >= 0 && (segs || n_segs == 0), "hmmr_adam_step: %d segments and %s", n_segs, segs ? "a table" : "a null table");
    const float hv[6] = {h->lr, h->beta1, h->beta2, h->eps, h->beta1_power, h->beta2_power};
    static const char* const hn[6] = {"lr", "beta1", "beta2", "eps", "beta1_power", "beta2_power"};
    for (int i = 0; i < 6; ++i) HMMR_REQUIRE(__builtin_isfinite(hv[i]), "hmmr_adam_step: %s is not finite", hn[i]);
    HMMR_REQUIRE(h->beta1_power > 0.f && h->beta1_power < 1.f, "hmmr_adam_step: beta1_power=%g lies outside (0, 1)", (double)h->beta1_power);
    HMMR_REQUIRE(h->beta2_power > 0.f && h->beta2_power < 1.f, "hmmr_adam_step: beta2_power=%g lies outside (0, 1)", (double)h->beta2_power);
    // every segment is checked before the first launch: a refused call has queued nothing
    for (int i = 0; i < n_segs; ++i) {
        const hmmr_adam_seg_t& s = segs[i];
        HMMR_REQUIRE(s.n >= 0 && s.n <= (1ll << 40), "hmmr_adam_step: segment %d has n=%lld (0 .. 2^40)", i, s.n);
        if (s.n == 0) continue;
        HMMR_REQUIRE(s.p && s.m && s.v, "hmmr_adam_step: segment %d has a null p, m or v with n=%lld", i, s.n);
        HMMR_REQUIRE((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 3) == 0,
                     "hmmr_adam_step: segment %d has a pointer that is not 4-byte aligned", i);
    }
    AdamTable A;
    A.alpha = h->lr * sqrtf(1.0f - h->beta2_power) / (1.0f - h->beta1_power);
    A.one_minus_beta1 = 1.0f - h->beta1;
    A.one_minus_beta2 = 1.0f - h->beta2;
    A.eps = h->eps;
    int i = 0;
    while (i < n_segs) {
        A.count = 0;
        A.vec = 0ull;
        A.first[0] = 0;
        for (; i < n_segs && A.count < ADAM_SEGS; ++i) {
            const hmmr_adam_seg_t& s = segs[i];
            if (s.n == 0 || !s.g) continue;       // a variable without a gradient: p, m and v keep their bytes
            const int k = A.count++;
            A.p[k] = s.p; A.g[k] = s.g; A.m[k] = s.m; A.v[k] = s.v; A.n[k] = s.n;
            if ((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 15) == 0) A.vec |= 1ull << k;
            A.first[k + 1] = A.first[k] + (s.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        }
        if (A.count == 0) break;
        for (int k = A.count; k < ADAM_SEGS; ++k) {
            A.p[k] = nullptr; A.g[k] = nullptr; A.m[k] = nullptr; A.v[k] = nullptr; A.n[k] = 0;
            A.first[k + 1] = A.first[A.count];
        }
        const long long total = A.first[A.count];
        const int blocks = (int)(total < ADAM_MAX_BLOCKS ? total : ADAM_MAX_BLOCKS);
        hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, A);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
