// ResNet-v2-50 image encoder for gfx950: encoder_resnet (src/models.py:50-77)
// -> tf.contrib.slim.nets.resnet_v2.resnet_v2_50(num_classes=None,
// is_training=False).  Layer semantics restated in SURVEY.md App. A.
//
// The 52 convolutions after the stem run through the implicit-GEMM kernel
// (gemm_conv.hip); the stem + pool1 + first preact is one fused kernel
// (stem.hip).  This file holds the launch sequence, pool5, and the unfused stem
// route kept for A/B measurements:
//   stem_repack       fp32 RGB [n,224,224,3] -> zero-padded RGBX [n,230,232,4]
//                     in the operand dtype, so the 7x7/2 stem (explicit pad 3,
//                     VALID) becomes an 8-tap x 32-element implicit GEMM
//                     (tap = ky, 32 elements = 8 pixels x 4 channels)
//   maxpool_bn_relu   3x3/2 TF-SAME max pool (pad bottom/right only) fused with
//                     block1/unit_1's `preact` BN + ReLU (every later unit's preact is fused
//                     into the operand staging of its conv1 / shortcut GEMMs)
//   bn_relu_avgpool   postnorm BN + ReLU + spatial mean (pool5)
// Inference BN is folded to y = x*scale + shift on the host
// (scale = gamma*rsqrt(var+1e-5), shift = beta - mean*scale).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "hmmr_hip.h"
#include "workspace.h"

// csrc/stem.hip
int hmmr_stem_fused(const float* images, int n_real, int n, const void* wts, const float* wscale, const float* bias,
                    const float* pscale, const float* pshift, void* out, int dtype, hipStream_t s,
                    const void* w1, const float* s1, const float* b1, void* out_h1);

static constexpr int IMG = 224, PADH = 230, PADW = 232;

// split (f16x3) image: one 8-"channel" group = two RGBX pixels; PADW is even, so a pair never straddles a row
__global__ void stem_repack_split_kernel(const float* __restrict__ img, bsplit_t* __restrict__ out, long long npairs,
                                         long long n_real) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs;
         i += (long long)gridDim.x * blockDim.x) {
        const int xp = (int)(i % (PADW / 2));
        const long long t = i / (PADW / 2);
        const int y = (int)(t % PADH);
        const long long n = t / PADH;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        const int sy = y - 3;
        if (n < n_real && (unsigned)sy < (unsigned)IMG) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int sx = 2 * xp + q - 3;
                if ((unsigned)sx < (unsigned)IMG) {
                    const float* p = img + ((n * IMG + sy) * IMG + sx) * 3;
                    v[4 * q] = p[0]; v[4 * q + 1] = p[1]; v[4 * q + 2] = p[2];
                }
            }
        }
        store8(out + i * 8, v);
    }
}

template <typename T>
__global__ void stem_repack_kernel(const float* __restrict__ img, T* __restrict__ out, long long npix,
                                   long long n_real) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
         i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % PADW);
        const long long t = i / PADW;
        const int y = (int)(t % PADH);
        const long long n = t / PADH;
        float r = 0.f, g = 0.f, b = 0.f;
        const int sy = y - 3, sx = x - 3;
        if (n < n_real && (unsigned)sy < (unsigned)IMG && (unsigned)sx < (unsigned)IMG) {
            const float* p = img + ((n * IMG + sy) * IMG + sx) * 3;
            r = p[0]; g = p[1]; b = p[2];
        }
        T* o = out + i * 4;
        o[0] = elem_traits<T>::from_f32(r);
        o[1] = elem_traits<T>::from_f32(g);
        o[2] = elem_traits<T>::from_f32(b);
        o[3] = elem_traits<T>::from_f32(0.f);
    }
}

// in [n,112,112,64] -> out [n,56,56,64]; window rows 2oy..2oy+2, cols 2ox..2ox+2,
// out-of-range taps ignored (TF SAME with pad_before = 0).
template <typename T>
__global__ void maxpool_bn_relu_kernel(const T* __restrict__ in, T* __restrict__ out,
                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                       long long nvec) {
    constexpr int HI = 112, HO = 56, C = 64, CV = C / 8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
         i += (long long)gridDim.x * blockDim.x) {
        const int cv = (int)(i % CV);
        long long t = i / CV;
        const int ox = (int)(t % HO); t /= HO;
        const int oy = (int)(t % HO);
        const long long n = t / HO;
        float m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = -3.0e38f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * oy + dy;
            if (iy >= HI) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * ox + dx;
                if (ix >= HI) continue;
                float v[8];
                load8(in + ((n * HI + iy) * HI + ix) * C + cv * 8, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], v[j]);
            }
        }
        float s[8], b[8];
        load8(scale + cv * 8, s); load8(shift + cv * 8, b);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = fmaxf(fmaf(m[j], s[j], b[j]), 0.f);   // one explicit fma: = stem.hip, bit for bit
        store8(out + i * 8, m);
    }
}

// in [n,hw,c] -> phi [n,c] fp32: mean over hw of relu(x*scale+shift)
template <typename T>
__global__ void bn_relu_avgpool_kernel(const T* __restrict__ in, float* __restrict__ phi,
                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                       int n, int hw, int c) {
    const int cv = c / 8;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * cv) return;
    const int v8 = (int)(i % cv);
    const long long img = i / cv;
    float s[8], b[8], acc[8];
    load8(scale + v8 * 8, s); load8(shift + v8 * 8, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int p = 0; p < hw; ++p) {
        float v[8];
        load8(in + (img * hw + p) * c + v8 * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += fmaxf(v[j] * s[j] + b[j], 0.f);
    }
    const float inv = 1.0f / (float)hw;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= inv;
    store8(phi + img * c + v8 * 8, acc);
}

// ------------------------------------------------------------------------- //
struct Prof {
    float* ms; int slot; hipStream_t s; hipEvent_t ev[HMMR_RESNET_PROF_SLOTS + 1];
    bool on() const { return ms != nullptr; }
};

static int prof_begin(Prof& p) {
    if (!p.on()) return 0;
    for (int i = 0; i <= HMMR_RESNET_PROF_SLOTS; ++i) HMMR_CHECK_HIP(hipEventCreate(&p.ev[i]));
    HMMR_CHECK_HIP(hipEventRecord(p.ev[0], p.s));
    p.slot = 0;
    return 0;
}
static int prof_mark(Prof& p) {
    if (!p.on() || p.slot >= HMMR_RESNET_PROF_SLOTS) return 0;
    ++p.slot;
    HMMR_CHECK_HIP(hipEventRecord(p.ev[p.slot], p.s));
    return 0;
}
static int prof_end(Prof& p) {
    if (!p.on()) return 0;
    HMMR_CHECK_HIP(hipStreamSynchronize(p.s));
    for (int i = 0; i < HMMR_RESNET_PROF_SLOTS; ++i) {
        p.ms[i] = 0.f;
        if (i < p.slot) HMMR_CHECK_HIP(hipEventElapsedTime(&p.ms[i], p.ev[i], p.ev[i + 1]));
    }
    for (int i = 0; i <= HMMR_RESNET_PROF_SLOTS; ++i) (void)hipEventDestroy(p.ev[i]);
    return 0;
}

struct ResnetBufs {
    size_t xpad, stem, stem_total, x[2], p[2], t1, t2, total;      // stem_total: what the unfused stem alone needs (xpad + the conv map)
};
static ResnetBufs resnet_layout(int n, int dtype) {
    const size_t e = dtype == HMMR_BF16 ? 2 : 4;
    ResnetBufs b; WsCarver c;
    auto take = [&](size_t elems) { return c.take(elems * e); };
    b.xpad = take((size_t)n * PADH * PADW * 4);
    b.stem = take((size_t)n * 112 * 112 * 64);
    b.stem_total = c.total();
    for (int i = 0; i < 2; ++i) b.x[i] = take((size_t)n * 56 * 56 * 256);
    for (int i = 0; i < 2; ++i) b.p[i] = take((size_t)n * 56 * 56 * 256);
    b.t1 = take((size_t)n * 56 * 56 * 64);
    b.t2 = take((size_t)n * 56 * 56 * 64);
    b.total = c.total();
    return b;
}

extern "C" size_t hmmr_resnet50_workspace_bytes(int n, int dtype) {
    return n > 0 ? resnet_layout(n, dtype).total : 0;
}

// ------------------------------------------------------------------------- //
// The schedule of a pass is a VALUE: hmmr_resnet50_plan decides what every unit launches (plan_unit: a pure host function
// that holds every structural check), resnet_fwd_t then issues the 16 plans in order.
static bool stem_unfused(const hmmr_resnet_weights_t* w, const hmmr_debug_t* dbg) {
    return dbg->stem_route == 1 || (dbg->stem_route == 0 && w->dtype == HMMR_F32);
}
// the fused stem computes block1/unit_1's conv1 on each pooled tile inside the same launch (-> T1): bf16, and f16x3 with the
// fragment-major copy of the conv1 filters (hmmr_resnet_unit_t.conv1_frag, round 5)
static bool stem_writes_conv1(const hmmr_resnet_weights_t* w, const hmmr_debug_t* dbg) {
    const hmmr_resnet_unit_t& U0 = w->unit[0];
    return !stem_unfused(w, dbg) && !dbg->stem_no_conv1 && ((w->dtype == HMMR_BF16 && U0.conv1.w) || (w->dtype == HMMR_F16X3 && U0.conv1_frag)) &&
           !U0.sc_c1.w && U0.c_in == 64 && U0.base == 64 && U0.conv1.scale && U0.conv1.shift;
}

// What both stem routes need of the table and of the image pointer, checked BEFORE anything is queued (hmmr_resnet50_fwd and
// hmmr_resnet50_stem).  The fused kernels read the image as aligned 16-byte groups of 4 floats (image rows and images are multiples of 16
// bytes), so a pointer that is not is refused -- on the three-kernel route too: a route switch never changes what a caller may pass.
// The template (bf16 / fp32) form of the fused kernel has no per-channel scale of the filter rows; the three-kernel route applies
// stem.scale in hmmr_conv_gemm's epilogue.  A table with one would make the routes disagree silently, so the fused route refuses it
// (the shipped packers leave stem.scale NULL in these modes; f16x3 carries the pack-time row scale there and both routes apply it).
static int stem_check(const hmmr_resnet_weights_t* w, const float* images, const hmmr_debug_t* dbg, const char* who) {
    const hmmr_resnet_unit_t& U0 = w->unit[0];
    HMMR_REQUIRE(w->stem.w && w->stem.shift && U0.pre_scale && U0.pre_shift, "%s: null argument (stem filters / bias, block1/unit_1 preact)", who);
    HMMR_REQUIRE(((uintptr_t)images & 15u) == 0, "%s: images must be 16-byte aligned (%p is not)", who, (const void*)images);
    HMMR_REQUIRE(stem_unfused(w, dbg) || w->dtype == HMMR_F16X3 || !w->stem.scale,
                 "%s: the fused %s stem applies no stem.scale (pack it as NULL, or take the three-kernel route)", who,
                 w->dtype == HMMR_BF16 ? "bf16" : "fp32");
    return 0;
}

// Unit u on n images of H x H pixels.  have_raw / h1_ready: what the previous unit (the stem) left behind -- the raw trunk of this
// unit's input, this unit's conv1 output in T1.
// A unit's pre-activation BN + ReLU (`preact`) reaches its 1x1 consumers (conv1 and the conv shortcut) as `fuse_preact` says:
//   1: they read the RAW trunk and apply the preact while staging their A operand (the tensor never exists in HBM);
//   0: the previous unit's conv3 epilogue writes it as a second output (the consumers keep the pure LDS-DMA operand path).
// Measured at batch 256 (bf16): fusing blocks 1-2 cuts the ResNet pass by 4.5 %, blocks 3-4 are neutral; the packer enables it everywhere.
static int plan_unit(const hmmr_resnet_weights_t* w, int u, int n, int H, const hmmr_debug_t* dbg, bool have_raw, bool h1_ready,
                     hmmr_unit_plan_t* out) {
    const hmmr_resnet_unit_t& U = w->unit[u];
    const int Ho = H / U.stride;
    const bool last = (u == HMMR_RESNET_UNITS - 1);
    hmmr_unit_plan_t p = {};
    const bool fused = p.reads_fused_preact = u > 0 && U.fuse_preact;
    HMMR_REQUIRE(!fused || (U.pre_scale && U.pre_shift && have_raw), "resnet: unit %d cannot fuse its preact", u);
    HMMR_REQUIRE(U.shortcut.w || have_raw, "resnet: unit %d has no raw input for its identity shortcut", u);
    // what the NEXT unit needs from this one
    const bool next_fused = !last && w->unit[u + 1].fuse_preact;
    const bool next_identity = !last && !w->unit[u + 1].shortcut.w;
    p.writes_raw = last || next_fused || next_identity;
    // ... and WHICH ROWS of it are live.  A next unit with stride s > 1 and an identity shortcut (HMMR_SC_NONE) reads the raw trunk as
    // x[:, ::s, ::s] (set_residual) -- and as nothing else once this unit's end has computed its conv1 (leaves_h1, below: no conv1 or
    // shortcut launch pre-activates the trunk, and the unit after it reads the NEXT trunk).  The unit pair and the block-1 unit then
    // store only those rows (hmmr_tail_desc_t.trunk_keep_stride); every other end, and every other successor, keeps them all
    const int next_keep_stride = (next_identity && w->unit[u + 1].stride > 1) ? w->unit[u + 1].stride : 0;
    p.writes_pre = !last && !next_fused;
    // a register-resident unit pair (csrc/unit_pair.hip) is one round of 128-pixel workgroups with a ~20 k-cycle prologue however few
    // pixels there are: below ~12 k pixels (61 frames in block 3) the two launches it replaces are faster (profiles/r04_unit_pair_check.log:
    // 0.064 against 0.096 ms at 33 frames), and they produce the same bits, so a short batch simply takes them
    // (hmmr_debug_t.pair_min_pixels moves the switch: tests run one batch on either side of it)
    // round 6 (profiles/r06e_pair_ws_check.log): in block 3 the two launches still win at 12 544 pixels (64 frames, FeatureExtractor's batch:
    // 0.085 against 0.093 ms) -- its switch is at 14 000; a block-2 pair is a shorter tile and wins from ~12 000 (0.034 against 0.043 ms at 15 680)
    const long long pair_min = dbg->pair_min_pixels > 0 ? dbg->pair_min_pixels : (U.base >= 256 ? 14000 : 12000);
    p.pair_demoted = w->dtype == HMMR_F16X3 && U.pair_stream && U.fuse_tail == 1 && (long long)n * Ho * Ho < pair_min;
    const int fuse_tail = p.pair_demoted ? 0 : U.fuse_tail;
    // the conv shortcut folded into conv3: ONE GEMM over {h2, preact} with [W3 | Wsc] (hmmr_conv_desc_t.in2);
    // the shortcut tensor (the widest tensor of the unit) is neither written nor read back
    HMMR_REQUIRE(!U.c3sc.w || (U.shortcut.w && !fused && U.stride == 1 && fuse_tail <= 2 && !U.sc_c1.w),
                 "resnet: unit %d cannot fold its shortcut into conv3", u);
    if (U.c3sc.w) {
        p.shortcut = HMMR_SC_IN_CONV3;
    } else if (fuse_tail == 3) {
        HMMR_REQUIRE(U.shortcut.w && !U.shortcut.scale && !fused && U.c_in == 64 && U.stride == 1,
                     "resnet: unit %d cannot compute its shortcut inside the tail", u);
        p.shortcut = HMMR_SC_IN_TAIL;
    } else if (U.shortcut.w) {
        p.shortcut = (U.sc_c1.w && !h1_ready && U.stride == 1) ? HMMR_SC_LAUNCH_WITH_CONV1 : HMMR_SC_LAUNCH;
    }
    p.conv1 = (h1_ready || p.shortcut == HMMR_SC_LAUNCH_WITH_CONV1) ? HMMR_CONV1_READY : HMMR_CONV1_LAUNCH;
    p.conv2 = fuse_tail >= 2 ? HMMR_CONV2_IN_TAIL : HMMR_CONV2_LAUNCH;       // (4: the single-phase tail of a stride-2 unit)
    HMMR_REQUIRE(!p.writes_pre || (w->unit[u + 1].pre_scale && w->unit[u + 1].pre_shift), "resnet: unit %d lacks its preact BN", u + 1);
    if (fuse_tail == 4) {             // stride-2 last unit of a block: conv2 + conv3 + add in one launch, no next conv1
        HMMR_REQUIRE(!last && w->dtype == HMMR_BF16 && U.conv2.scale && U.conv2.shift && !U.shortcut.w &&
                     ((U.base == 64 && U.depth == 256) || (U.base == 128 && U.depth == 512)),
                     "resnet: unit %d cannot run as a single-phase tail", u);
        p.end = HMMR_END_TAIL_BF16_STRIDE2;
    } else if (fuse_tail) {           // conv3 + add + the next unit's preact + conv1 in one launch
        const bool pair = w->dtype == HMMR_F16X3 && U.pair_stream && fuse_tail == 1;
        HMMR_REQUIRE(!last && (w->dtype == HMMR_BF16 || pair || (w->dtype == HMMR_F16X3 && ((U.w3_frag && U.w1n_frag) || U.unit_stream) && fuse_tail <= 2)) &&
                     U.stride == 1 && p.writes_raw && !p.writes_pre && next_fused &&
                     next_identity && w->unit[u + 1].base == U.base && w->unit[u + 1].c_in == U.depth &&
                     ((U.base == 64 && U.depth == 256) || (U.base == 128 && U.depth == 512) || (pair && U.base == 256 && U.depth == 1024)),
                     "resnet: unit %d cannot fuse its tail", u);
        if (p.conv2 == HMMR_CONV2_IN_TAIL) {
            HMMR_REQUIRE(U.conv2.scale && U.conv2.shift, "resnet: unit %d cannot fuse its conv2", u);
            HMMR_REQUIRE((U.conv2.k_order == 2) == (w->dtype == HMMR_F16X3 && U.unit_stream != nullptr),
                         "resnet: unit %d: a k_order 2 conv2 runs inside the unit only as part of its unit_stream (csrc/b1_unit.hip)", u);
            p.swaps_t1_t2 = 1;        // h2 never exists in HBM; conv1' goes to T2 (neighbouring tiles' halos still read T1), then the two swap roles
        }
        p.end = w->dtype == HMMR_BF16 ? HMMR_END_TAIL_BF16 : pair ? HMMR_END_UNIT_PAIR :
                (p.swaps_t1_t2 && U.unit_stream) ? HMMR_END_B1_UNIT : HMMR_END_TAIL_SPLIT;
        p.leaves_h1 = 1;
        if (p.end == HMMR_END_UNIT_PAIR || p.end == HMMR_END_B1_UNIT) p.trunk_keep_stride = next_keep_stride;
    }
    *out = p;
    return 0;
}

extern "C" int hmmr_resnet50_plan(const hmmr_resnet_weights_t* w, int n_total, hmmr_unit_plan_t out[HMMR_RESNET_UNITS]) {
    HMMR_REQUIRE(w && out && n_total > 0, "hmmr_resnet50_plan: null argument or no image");
    const hmmr_debug_t* dbg = hmmr_debug_state();
    int H = 56;
    bool have_raw = false, h1_ready = stem_writes_conv1(w, dbg);
    for (int u = 0; u < HMMR_RESNET_UNITS; ++u) {
        if (plan_unit(w, u, n_total, H, dbg, have_raw, h1_ready, &out[u])) return -1;
        have_raw = out[u].writes_raw; h1_ready = out[u].leaves_h1; H /= w->unit[u].stride;
    }
    return 0;
}

// a k x k convolution (stride, pad k / 2) of layer L over the dense NHWC tensor in [n][H][H][cin] -> out [n][H / stride][H / stride][cout]
static hmmr_conv_desc_t dense_conv(int dtype, int n, const void* in, int H, int cin, int k, int stride, int cout, const hmmr_layer_t& L,
                                   void* out) {
    hmmr_conv_desc_t d = {};
    d.in = in; d.w = L.w; d.scale = L.scale; d.shift = L.shift; d.tile = L.tile; d.k_order = L.k_order;
    d.out = out; d.in_dtype = d.out_dtype = dtype;
    d.n_img = n; d.hin = d.win = H; d.cin = cin;
    d.in_img_stride = (int64_t)H * H * cin; d.in_row_stride = H * cin; d.in_px_stride = cin;
    d.kh = d.kw = k; d.sy = d.sx = stride; d.py = d.px = k / 2; d.ho = d.wo = H / stride; d.cout = d.ldo = cout;
    return d;
}

// the other operand of a unit's add (hmmr_conv_desc_t or hmmr_tail_desc_t): rows of `depth` elements, or -- stride > 1 --
// max_pool2d(x, [1,1], stride) = x[:, ::s, ::s] of the NHWC tensor x [.][H][H][depth]
template <typename D>
static void set_residual(D& d, const void* x, int depth, int H, int stride) {
    d.res = x;
    if (stride == 1) { d.ldr = depth; return; }
    d.res_strided = 1;
    d.res_img_stride = (int64_t)H * H * depth; d.res_row_stride = stride * H * depth; d.res_px_stride = stride * depth;
}

// ---- the stem of a pass, ALONE: route choice, the fused launch or the three launches, the three profile marks.  resnet_fwd_t and
// hmmr_resnet50_stem both issue exactly this.  7x7/2 conv (+bias, no BN/ReLU) -> pool1 -> preact of block1/unit_1 -> pooled; h1 (may
// be NULL: then nobody wants it) receives that unit's conv1 where stem_writes_conv1 says the fused kernel computes it.
// Default: ONE fused kernel (csrc/stem.hip).  hmmr_debug_t.stem_route = 1 keeps the three-kernel route (re-pack, implicit GEMM, pool)
// for A/B measurements.  In fp32-operand mode the fused kernel needs 104 KB of LDS (one workgroup per CU) and measures ~1 % slower
// than the three-kernel route, which therefore stays the fp32 default.  f16x3 has its own fused kernel (stem_fused_split_kernel:
// hi/lo planes, 32 output channels at a time).  xpad / stem: the re-packed image and the 112 x 112 conv map of the three-kernel route
// (not touched by the fused one).
template <typename T>
static int stem_run(const hmmr_resnet_weights_t* w, const hmmr_debug_t* dbg, const float* images, int n_real, int n, T* pooled, T* h1,
                    T* xpad, T* stem, hipStream_t s, Prof& pf) {
    const int dt = w->dtype;
    const hmmr_resnet_unit_t& U0 = w->unit[0];
    if (!stem_unfused(w, dbg)) {
        const bool stem_c1 = h1 && stem_writes_conv1(w, dbg);
        if (hmmr_stem_fused(images, n_real, n, w->stem.w, w->stem.scale, w->stem.shift, U0.pre_scale, U0.pre_shift, pooled, dt, s,
                            stem_c1 ? (dt == HMMR_F16X3 ? U0.conv1_frag : U0.conv1.w) : nullptr, U0.conv1.scale, U0.conv1.shift,
                            stem_c1 ? h1 : nullptr))
            return -2;
        hmmr_count_launch(stem_c1 ? HMMR_COUNT_STEM_FUSED_CONV1 : HMMR_COUNT_STEM_FUSED);
        if (prof_mark(pf)) return -2;
        if (prof_mark(pf)) return -2;     // (keeps the profile slot numbering of the 3-kernel route)
        if (prof_mark(pf)) return -2;
    } else {
        const long long npix = (long long)n * PADH * PADW;
        const int grid = (int)((npix + 255) / 256 < 8192 ? (npix + 255) / 256 : 8192);
        if constexpr (std::is_same<T, bsplit_t>::value)
            hipLaunchKernelGGL(stem_repack_split_kernel, dim3(grid), dim3(256), 0, s, images, xpad, npix / 2, (long long)n_real);
        else
            hipLaunchKernelGGL(stem_repack_kernel<T>, dim3(grid), dim3(256), 0, s, images, xpad, npix, (long long)n_real);
        HMMR_CHECK_HIP(hipGetLastError());
        hmmr_count_launch(HMMR_COUNT_STEM_REPACK);
        if (prof_mark(pf)) return -2;
        hmmr_conv_desc_t d = {};
        d.in = xpad; d.w = w->stem.w; d.scale = w->stem.scale; d.shift = w->stem.shift;
        d.out = stem; d.in_dtype = d.out_dtype = dt;
        d.n_img = n; d.hin = PADH; d.win = 2 * 111 + 1; d.cin = 32;
        d.in_img_stride = (int64_t)PADH * PADW * 4; d.in_row_stride = PADW * 4; d.in_px_stride = 4;
        d.kh = 8; d.kw = 1; d.sy = 2; d.sx = 2; d.py = 0; d.px = 0;
        d.ho = 112; d.wo = 112; d.cout = 64; d.ldo = 64;
        if (hmmr_conv_gemm(&d, s)) return -2;
        hmmr_count_launch(HMMR_COUNT_STEM_GEMM);
        if (prof_mark(pf)) return -2;
        const long long nvec = (long long)n * 56 * 56 * 8;
        const int g2 = (int)((nvec + 255) / 256 < 16384 ? (nvec + 255) / 256 : 16384);
        hipLaunchKernelGGL(maxpool_bn_relu_kernel<T>, dim3(g2), dim3(256), 0, s, (const T*)stem, pooled, U0.pre_scale, U0.pre_shift, nvec);
        HMMR_CHECK_HIP(hipGetLastError());
        hmmr_count_launch(HMMR_COUNT_STEM_POOL);
        if (prof_mark(pf)) return -2;
    }
    return 0;
}

template <typename T>
static int resnet_fwd_t(const hmmr_resnet_weights_t* w, const float* images, int n_real, int n, float* phi,
                        char* ws, const ResnetBufs& L, hipStream_t s, float* prof_ms) {
    hmmr_unit_plan_t plan[HMMR_RESNET_UNITS];
    if (hmmr_resnet50_plan(w, n, plan)) return -1;       // (nothing has been launched yet)
    const int dt = w->dtype;
    T* xpad = (T*)(ws + L.xpad);
    T* stem = (T*)(ws + L.stem);
    T* X[2] = {(T*)(ws + L.x[0]), (T*)(ws + L.x[1])};
    T* P[2] = {(T*)(ws + L.p[0]), (T*)(ws + L.p[1])};
    T* T1 = (T*)(ws + L.t1);
    T* T2 = (T*)(ws + L.t2);
    Prof pf; pf.ms = prof_ms; pf.s = s; pf.slot = 0;
    if (prof_begin(pf)) return -2;

    // ---- stem: 7x7/2 conv (+bias, no BN/ReLU) -> pool1 -> preact of block1/unit_1 (-> P[0]) [+ that unit's conv1 -> T1]
    if (stem_run<T>(w, hmmr_debug_state(), images, n_real, n, P[0], T1, xpad, stem, s, pf)) return -2;

    // ---- units.  X[cur]: the raw trunk, P[pcur]: its pre-activated form (each where the plan has it written), T1 / T2: conv1's and
    // conv2's outputs.  Every layer owns one profile slot per pass -- [shortcut] conv1 conv2 conv3 -- whether or not the plan gives it a
    // launch of its own: the mark after each step below is that slot.
    int H = 56, cur = 0, pcur = 0;
    for (int u = 0; u < HMMR_RESNET_UNITS; ++u) {
        const hmmr_resnet_unit_t& U = w->unit[u];
        const hmmr_resnet_unit_t& N = w->unit[u + 1 < HMMR_RESNET_UNITS ? u + 1 : u];     // (read only where the plan has a next unit)
        const hmmr_unit_plan_t& p = plan[u];
        const int Ho = H / U.stride;
        const T* xin = p.reads_fused_preact ? (const T*)X[cur] : (const T*)P[pcur];
        const float* ps = p.reads_fused_preact ? U.pre_scale : nullptr;
        const float* pb = p.reads_fused_preact ? U.pre_shift : nullptr;
        T* xn = X[cur ^ 1];
        T* out = p.writes_raw ? xn : nullptr;
        T* pre = p.writes_pre ? P[pcur ^ 1] : nullptr;
        const bool sc_in_c3 = p.shortcut == HMMR_SC_IN_CONV3;
        // the add reads the unit's raw input (subsampled by the unit's stride) or the shortcut launch's output (xn, overwritten in place)
        const T* res = p.shortcut == HMMR_SC_NONE ? X[cur] : xn;
        const int res_stride = p.shortcut == HMMR_SC_NONE ? U.stride : 1;
        hmmr_conv_desc_t d;
        if (p.shortcut == HMMR_SC_LAUNCH || p.shortcut == HMMR_SC_LAUNCH_WITH_CONV1) {   // 1x1 conv on preact, bias, no BN/ReLU
            d = dense_conv(dt, n, xin, H, U.c_in, 1, U.stride, U.depth, U.shortcut, xn);
            d.pro_scale = ps; d.pro_shift = pb;
            d.k_order = 0;            // (shortcut.k_order only names the tile family of the sc_c1 launch: HmmrEngine._tile_for)
            if (p.shortcut == HMMR_SC_LAUNCH_WITH_CONV1) {   // ... and conv1 over the same operand as extra output columns (-> T1, BN + ReLU)
                d.w = U.sc_c1.w; d.scale = U.sc_c1.scale; d.shift = U.sc_c1.shift; d.k_order = U.sc_c1.k_order;
                d.cout = U.depth + U.base; d.out_b = T1; d.ldo_b = U.base; d.n_split = U.depth; d.relu_b = 1;
            }
            if (hmmr_conv_gemm(&d, s)) return -2;
        }
        if (p.shortcut != HMMR_SC_NONE && prof_mark(pf)) return -2;
        if (p.conv1 == HMMR_CONV1_LAUNCH) {   // 1x1 on preact, BN + ReLU (k_order 2: the two-ring stream kernel of csrc/conv1x1_stream.hip; it takes the pre-activated tensor)
            d = dense_conv(dt, n, xin, H, U.c_in, 1, 1, U.base, U.conv1, T1);
            d.pro_scale = ps; d.pro_shift = pb; d.relu = 1;
            if (hmmr_conv_gemm(&d, s)) return -2;
        }
        if (prof_mark(pf)) return -2;
        if (p.conv2 == HMMR_CONV2_LAUNCH) {   // 3x3 conv2d_same(stride): pad 1/1 both for stride 1 (SAME) and stride 2 (explicit pad + VALID)
            d = dense_conv(dt, n, T1, H, U.base, 3, U.stride, U.base, U.conv2, T2);
            d.relu = 1;
            if (hmmr_conv_gemm(&d, s)) return -2;
        }
        if (prof_mark(pf)) return -2;
        if (p.end == HMMR_END_CONV3_LAUNCH) {   // 1x1 + bias, + shortcut (no ReLU after the add); k_order 2: the conv3 form of csrc/conv1x1_stream.hip, block 4
            d = dense_conv(dt, n, T2, Ho, U.base, 1, 1, U.depth, sc_in_c3 ? U.c3sc : U.conv3, out);
            if (sc_in_c3) { d.in2 = xin; d.cin2 = U.c_in; } else set_residual(d, res, U.depth, H, res_stride);
            if (pre) { d.out2 = pre; d.scale2 = N.pre_scale; d.shift2 = N.pre_shift; }
            if (hmmr_conv_gemm(&d, s)) return -2;
        } else {                              // a fused tail (csrc/bottleneck.hip and the kernels behind it)
            hmmr_tail_desc_t t = {};
            t.dtype = dt; t.m = n * Ho * Ho; t.c_mid = U.base; t.depth = U.depth; t.ho = t.wo = Ho;
            t.w3 = U.conv3.w; t.scale3 = U.conv3.scale; t.shift3 = U.conv3.shift;
            if (p.conv2 == HMMR_CONV2_IN_TAIL) {
                t.h1 = T1; t.hin = t.win = H; t.w2 = U.conv2.w; t.scale2 = U.conv2.scale; t.shift2 = U.conv2.shift;
            } else t.h2 = T2;
            if (p.end == HMMR_END_TAIL_BF16_STRIDE2) {
                t.conv2_stride = U.stride;
                set_residual(t, res, U.depth, H, res_stride);
                t.out = out; t.out_pre = pre;
                if (pre) { t.pre_scale = N.pre_scale; t.pre_shift = N.pre_shift; }
            } else {                          // ... with the next unit's preact + conv1 (-> T1, or T2 where this launch still reads T1)
                if (dt == HMMR_F16X3) {       // fragment-major filters (or one fragment stream); a folded shortcut rides in conv3's K
                    t.w3 = U.w3_frag;
                    if (p.conv2 == HMMR_CONV2_IN_TAIL) t.unit_stream = U.unit_stream;
                    if (p.end == HMMR_END_UNIT_PAIR) t.pair_stream = U.pair_stream;
                    if (sc_in_c3) { t.scale3 = U.c3sc.scale; t.shift3 = U.c3sc.shift; t.xp = xin; t.c_xp = U.c_in; }
                }
                if (p.shortcut == HMMR_SC_IN_TAIL) { t.xp = xin; t.wsc = U.shortcut.w; t.shift_sc = U.shortcut.shift; }
                else if (!sc_in_c3) set_residual(t, res, U.depth, H, res_stride);
                t.out = xn; t.pre_scale = N.pre_scale; t.pre_shift = N.pre_shift; t.trunk_keep_stride = p.trunk_keep_stride;
                t.w1 = dt == HMMR_F16X3 ? U.w1n_frag : N.conv1.w;      // (not read with pair_stream)
                t.scale1 = N.conv1.scale; t.shift1 = N.conv1.shift; t.relu1 = 1; t.n2 = N.base;
                t.out_h1 = p.swaps_t1_t2 ? T2 : T1;
            }
            if (hmmr_bottleneck_tail(&t, s)) return -2;
            if (p.swaps_t1_t2) { T* tmp = T1; T1 = T2; T2 = tmp; }
        }
        if (prof_mark(pf)) return -2;
        cur ^= 1; pcur ^= 1; H = Ho;
    }
    // ---- postnorm BN + ReLU + mean over 7x7
    const long long nth = (long long)n * (2048 / 8);
    hipLaunchKernelGGL(bn_relu_avgpool_kernel<T>, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s,
                       (const T*)X[cur], phi, w->post_scale, w->post_shift, n, H * H, 2048);
    HMMR_CHECK_HIP(hipGetLastError());
    if (prof_mark(pf)) return -2;
    return prof_end(pf);
}

extern "C" int hmmr_resnet50_fwd(const hmmr_resnet_weights_t* w, const float* images, int n, int n_zero,
                                 float* phi, void* ws, size_t ws_bytes, void* stream, float* prof_ms) {
    HMMR_REQUIRE(w && phi && ws && (images || n == 0), "hmmr_resnet50_fwd: null argument");
    HMMR_REQUIRE(n >= 0 && n_zero >= 0 && n + n_zero > 0, "hmmr_resnet50_fwd: need at least one image");
    const int nt = n + n_zero;
    const ResnetBufs L = resnet_layout(nt, w->dtype);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_resnet50_fwd: workspace too small (%zu < %zu)", ws_bytes, L.total);
    HMMR_REQUIRE(w->unit[0].c_in == 64 && w->unit[15].depth == 2048, "hmmr_resnet50_fwd: bad unit table");
    HMMR_REQUIRE(w->dtype == HMMR_BF16 || w->dtype == HMMR_F32 || w->dtype == HMMR_F16X3, "hmmr_resnet50_fwd: bad dtype %d", w->dtype);
    if (stem_check(w, images, hmmr_debug_state(), "hmmr_resnet50_fwd")) return -1;
    if (w->dtype == HMMR_BF16) return resnet_fwd_t<bf16_t>(w, images, n, nt, phi, (char*)ws, L, (hipStream_t)stream, prof_ms);
    if (w->dtype == HMMR_F32) return resnet_fwd_t<float>(w, images, n, nt, phi, (char*)ws, L, (hipStream_t)stream, prof_ms);
    return resnet_fwd_t<bsplit_t>(w, images, n, nt, phi, (char*)ws, L, (hipStream_t)stream, prof_ms);
}

// ---- the stem alone (include/hmmr_hip.h): what hmmr_resnet50_fwd launches first, into caller-owned tensors
extern "C" size_t hmmr_resnet50_stem_workspace_bytes(const hmmr_resnet_weights_t* w, int n_total) {
    if (!w || n_total <= 0 || (w->dtype != HMMR_BF16 && w->dtype != HMMR_F32 && w->dtype != HMMR_F16X3)) return 0;
    return stem_unfused(w, hmmr_debug_state()) ? resnet_layout(n_total, w->dtype).stem_total : 0;
}

extern "C" int hmmr_resnet50_stem(const hmmr_resnet_weights_t* w, const float* images, int n, int n_zero, void* pooled, void* h1,
                                  int* h1_written, void* ws, size_t ws_bytes, void* stream) {
    if (h1_written) *h1_written = 0;
    HMMR_REQUIRE(w && pooled && (images || n == 0), "hmmr_resnet50_stem: null argument");
    HMMR_REQUIRE(n >= 0 && n_zero >= 0 && n + n_zero > 0, "hmmr_resnet50_stem: need at least one image");
    HMMR_REQUIRE(w->dtype == HMMR_BF16 || w->dtype == HMMR_F32 || w->dtype == HMMR_F16X3, "hmmr_resnet50_stem: bad dtype %d", w->dtype);
    const int nt = n + n_zero;
    const size_t need = hmmr_resnet50_stem_workspace_bytes(w, nt);
    HMMR_REQUIRE(ws_bytes >= need && (ws || !need), "hmmr_resnet50_stem: workspace too small (%zu < %zu)", ws ? ws_bytes : (size_t)0, need);
    const hmmr_debug_t* dbg = hmmr_debug_state();
    if (stem_check(w, images, dbg, "hmmr_resnet50_stem")) return -1;
    const ResnetBufs L = resnet_layout(nt, w->dtype);
    char* base = need ? (char*)ws : nullptr;           // (the fused route touches neither buffer)
    Prof pf; pf.ms = nullptr; pf.s = (hipStream_t)stream; pf.slot = 0;
    int rc;
    if (w->dtype == HMMR_BF16)
        rc = stem_run<bf16_t>(w, dbg, images, n, nt, (bf16_t*)pooled, (bf16_t*)h1, base ? (bf16_t*)(base + L.xpad) : nullptr, base ? (bf16_t*)(base + L.stem) : nullptr, pf.s, pf);
    else if (w->dtype == HMMR_F32)
        rc = stem_run<float>(w, dbg, images, n, nt, (float*)pooled, (float*)h1, base ? (float*)(base + L.xpad) : nullptr, base ? (float*)(base + L.stem) : nullptr, pf.s, pf);
    else
        rc = stem_run<bsplit_t>(w, dbg, images, n, nt, (bsplit_t*)pooled, (bsplit_t*)h1, base ? (bsplit_t*)(base + L.xpad) : nullptr, base ? (bsplit_t*)(base + L.stem) : nullptr, pf.s, pf);
    if (rc) return rc;
    if (h1_written) *h1_written = (h1 && stem_writes_conv1(w, dbg)) ? 1 : 0;
    return 0;
}
