/* libhmmr_hip.so -- C ABI of the MI355X (gfx950) HMMR inference hot path.
 *
 * Drop-in boundary for akanazawa/human_dynamics `Tester.predict`
 * (src/evaluation/tester.py:229-258).  The reference has no FFI of its own:
 * the path sits behind one `sess.run` of a TF-1.8 graph.  Each entry point
 * below replaces one op-group of that graph (citations are relative to the
 * reference tree) and is what a ctypes binding on the reference side would
 * call.
 *
 * Conventions
 *   - every pointer that carries tensor data is a DEVICE pointer (HBM);
 *     structs themselves live in host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     all work is enqueued asynchronously on it, nothing is allocated or
 *     synchronised inside a call: scratch comes from the caller through
 *     (`ws`, `ws_bytes`) sized by the matching *_workspace_bytes();
 *   - return 0 on success, <0 on error; hmmr_last_error() describes the last
 *     failure of the calling thread;
 *   - activations are NHWC / row-major, fp32 at every stage boundary.  Inside
 *     the ResNet / temporal / IEF stages the GEMM operand type is selected by
 *     `dtype` (HMMR_F32 = exact-fp32 MFMA, HMMR_BF16 = bf16 MFMA with fp32
 *     accumulate).  The SMPL stage is always fp32.
 */
#ifndef HMMR_HIP_H
#define HMMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMMR_ABI_VERSION 19      /* 19: hmmr_clock_probe (measurement aid); also under 19 (the number is pinned by the test suite): hmmr_tail_desc_t.trunk_keep_stride and hmmr_unit_plan_t.trunk_keep_stride APPENDED to their structs (rebuild binders of hmmr_bottleneck_tail / hmmr_resnet50_plan), hmmr_debug_t.keep_dead_rows in the former reserved[2], hmmr_trunk_keep_launches; 18: HMMR_FLAG_NAN, hmmr_debug_t.pair_form (the wave-specialised unit pair), the C-side packers hmmr_pack_*; 17: k_order = 2 on a 1x1 filter (the two-ring stream kernel of csrc/conv1x1_stream.hip, tiles 22 .. 26), hmmr_conv1x1_stream_bytes; 16: hmmr_tail_desc_t.unit_stream, hmmr_resnet_unit_t.unit_stream (the whole-unit kernel of block 1, csrc/b1_unit.hip), hmmr_b1_unit_stream_bytes, hmmr_debug_t.pair_min_pixels / pair_two_tile_min / launch counters, hmmr_resnet_unit_t.conv1_frag (block1/unit_1's conv1 inside the split stem); 15: k_order = 2 (the one-wave-per-SIMD 3x3 stream kernel, tiles 12 .. 18), hmmr_conv3x3_stream_bytes; 14: hmmr_tail_desc_t.pair_stream / c_xp, hmmr_resnet_unit_t.pair_stream (the register-resident unit pair of blocks 2-3), hmmr_run_flags; 13: hmmr_conv_desc_t.batch (grouped launches); 12: k_order = 1, 3x3 SAME convolutions out of an LDS-resident input patch (tiles 9, 10, 11) */

/* HMMR_F16X3: "split" tensors -- every group of 8 consecutive channels is 32 bytes, [hi x8][lo x8] with
 * hi = fp16(x), lo = fp16(x - hi), x clamped to +-65504 (4 bytes per element, 22 mantissa bits while lo is a normal
 * fp16, an absolute 6e-8 below that); GEMMs on them issue three fp16 MFMAs per operand pair (lo*hi + hi*lo + hi*hi,
 * fp32 accumulate; v_mfma_f32_32x32x16_f16 keeps fp16 subnormals).  Filter banks of this dtype are expected with every
 * output-channel row scaled by a power of two to a maximum in [2^13, 2^14) and the inverse factor in the layer's `scale`
 * (packing.row_pow2) -- unscaled filters work too, with fewer bits for small values.  The parity-grade throughput mode:
 * fp32-class operands at the 16-bit MFMA rate / 3.  (Rounds 1-2 used bf16 halves: 16-17 bits.) */
enum { HMMR_F32 = 0, HMMR_BF16 = 1, HMMR_F16X3 = 2 };

int hmmr_abi_version(void);
const char* hmmr_last_error(void);

/* Sticky run flags of the CURRENT device, OR-ed over everything launched on it since the last clear.  HMMR_FLAG_SATURATED: a value
 * beyond the fp16 range (+-65504, or +-inf) reached a split (HMMR_F16X3) store and was clamped -- the results of that call are not
 * the network's; run it with fp32 operands instead (the Python mirror does: Tester.precision["saturated"]).  Synchronises with the
 * device (hipDeviceSynchronize, then a 4-byte copy per translation unit): call it where the results are read, not per launch.
 * clear != 0 resets the flags.
 * HMMR_FLAG_NAN (round 6, together with HMMR_FLAG_SATURATED): the value was a NaN -- a NaN pixel, weight or constant.  The clamp
 * (v_med3_f32) turns a NaN into a finite number, so without this flag it would leave as a plausible result.  Every split store keeps
 * its running maximum with gfx950's NaN-propagating v_maximum3_f32 and tests !(max <= 65504); the split stem applies the same test to
 * the fp32 pixels it reads. */
#define HMMR_FLAG_SATURATED 1u
#define HMMR_FLAG_NAN 2u
int hmmr_run_flags(unsigned* flags, int clear);

/* Development switches for A/B measurements and tests.  Process-wide; all zero = the product defaults.  No
 * switch changes a result beyond what its comment says; the library never reads the environment. */
typedef struct hmmr_debug_s {
    int stem_route;        /* 0: default (fused stem kernel for bf16 / f16x3, re-pack + GEMM + pool for f32);
                              1: always the three-kernel route; 2: always the fused kernel */
    int stem_no_conv1;     /* 1: the fused bf16 stem leaves block1/unit_1's conv1 to its own launch */
    int gemm_probe;        /* read only by the -DHMMR_GEMM_PROBE development build (tools/probe_build.sh): the GEMM K loop
                              drops its MFMAs (1), its operand loads after the first stage (2) or its barriers (4), to see
                              which of the three bounds a shape; results are garbage then.  The product build ignores it. */
    int smpl_blend_mfma;   /* the SMPL blend-shape product [m,218] x [218,3 x 6890]: 0 = the default, split-fp16 operands on the
                              matrix cores (smpl_verts_split_kernel; needs hmmr_smpl_consts_t.dirs_split, else form 2);
                              1 = exact fp32 on the matrix cores (smpl_verts_mfma_kernel, v_mfma_f32_32x32x2_f32);
                              2 = the packed-FMA vector form (smpl_verts_kernel).  1 and 2 agree to one fp32 ulp, 0 with
                              them to ~1e-7 m */
    int ief_no_group;      /* 1: hmmr_ief_fwd runs the delta regressors one after the other instead of as grouped launches (same bits) */
    int reserved[2];
    int keep_dead_rows;    /* (was reserved[2]: the struct keeps its size) 1: every fused-unit launch stores every trunk row, whatever
                              hmmr_tail_desc_t.trunk_keep_stride says -- the A/B of the dead-row stores in one process, and the tests' reference.
                              Same bits in every row the pass reads */
    int pair_min_pixels;   /* hmmr_resnet50_fwd runs a register-resident unit pair (csrc/unit_pair.hip) as the two launches it replaces when
                              the unit has fewer pixels than this (same bits, faster for short batches): 0 = the default (12000 in block 2, 14000 in block 3),
                              1 = always the pair kernel, INT_MAX = never */
    int pair_two_tile_min; /* the pair kernel of the block-2 shapes runs as PERSISTENT workgroups (several 128-pixel tiles each) when the launch has at least
                              this many tiles (same bits; one workgroup per CU then walks tiles b, b + grid, ...): 0 = the default (512 = two rounds of workgroups), 1 = always, INT_MAX = never */
    int pair_form;         /* (ABI 18) the unit pairs with a shortcut tensor (blocks 2-3): 0 = the default, the one-wave-per-SIMD form of round 4;
                              2 = the wave-specialised form of round 6 (two waves per SIMD: conv3 + the trunk epilogue in one, conv1' + all
                              memory traffic in the other).  Same bits; measured equal */
} hmmr_debug_t;
void hmmr_set_debug(const hmmr_debug_t* d);     /* NULL = defaults */
void hmmr_get_debug(hmmr_debug_t* d);

/* Launch counters of the fused-unit kernels, process-wide, since the last clear: how often hmmr_bottleneck_tail / hmmr_conv_gemm ended in
 * each of them.  For tests that must know WHICH kernel a schedule ran (a bit-identity test of two schedules that silently take the same
 * kernels proves nothing). */
typedef struct {
    unsigned long long unit_pair;       /* csrc/unit_pair.hip */
    unsigned long long b1_unit;         /* csrc/b1_unit.hip */
    unsigned long long tail_split;      /* csrc/bottleneck_split.hip (LDS-panel tails) */
    unsigned long long conv3x3_stream;  /* csrc/conv3x3_stream.hip */
    unsigned long long conv1x1_stream;  /* csrc/conv1x1_stream.hip (ABI 17) */
} hmmr_launch_counts_t;
void hmmr_launch_counts(hmmr_launch_counts_t* out, int clear);
/* ... and how many of the unit_pair / b1_unit launches were queued with a trunk_keep_stride > 1 in force (hmmr_tail_desc_t; 3 per pass in
 * the default f16x3 schedule at sizes where the pairs are on, 0 under hmmr_debug_t.keep_dead_rows).  A function of its own, with its own
 * clear, so hmmr_launch_counts_t keeps its size. */
unsigned long long hmmr_trunk_keep_launches(int clear);
/* ... and of the stem's launches, wherever they were issued (hmmr_resnet50_fwd or hmmr_resnet50_stem); a struct of its own, so
 * hmmr_launch_counts_t keeps its size.  One pass adds 1 to `fused` OR `fused_conv1`, or 1 to each of `repack`, `gemm`, `pool`. */
typedef struct {
    unsigned long long fused;           /* csrc/stem.hip, pooled tensor only */
    unsigned long long fused_conv1;     /* csrc/stem.hip with block1/unit_1's conv1 inside the launch */
    unsigned long long repack;          /* the three-kernel route: stem_repack*, */
    unsigned long long gemm;            /* ... its hmmr_conv_gemm, */
    unsigned long long pool;            /* ... maxpool_bn_relu_kernel */
} hmmr_stem_counts_t;
void hmmr_stem_launch_counts(hmmr_stem_counts_t* out, int clear);

/* ------------------------------------------------------------------------- *
 * Generic implicit-GEMM convolution / fully-connected building block.
 * out[m, n] = epilogue( sum_k A[m, k] * W[n, k] ), m = (img, oy, ox) over an
 * NHWC input gathered on the fly, k = (ky, kx, ci).  Replaces every
 * slim.conv2d / tf.contrib.layers.conv2d / slim.fully_connected on the path
 * (src/models.py:65-74 via slim resnet_v2; :102-113; :173-184; :209-221).
 * Exposed so each layer shape can be parity-tested in isolation.
 * ------------------------------------------------------------------------- */
typedef struct {
    /* operands */
    const void* in;        /* activations, dtype in_dtype                        */
    const void* w;         /* [cout_pad][K], K = kh*kw*cin contiguous, in_dtype;
                              cout_pad = cout rounded up to 128                   */
    const float* scale;    /* [cout_pad] or NULL (=1): multiplies the accumulator */
    const float* shift;    /* [cout_pad] or NULL (=0): bias / folded BN shift     */
    const void* res;       /* residual added before the ReLU, out_dtype, or NULL  */
    void* out;             /* [M, ldo] out_dtype, may be NULL if out2 is set      */
    void* out2;            /* optional second output relu(out*scale2+shift2) of the value as STORED in `out`'s
                              dtype (= what a consumer applying pro_scale/pro_shift to `out` computes), or NULL */
    const float* scale2;
    const float* shift2;
    int in_dtype;          /* HMMR_F32 / HMMR_BF16 / HMMR_F16X3 */
    int out_dtype;
    /* input geometry (element strides) */
    int n_img, hin, win, cin;          /* cin: channels per tap, power of two, >= 32B/elt */
    int64_t in_img_stride;
    int in_row_stride, in_px_stride;
    /* filter geometry */
    int kh, kw, sy, sx, py, px;
    int ho, wo;
    int cout;
    int ldo;               /* row stride of out / out2 in elements (multiple of 8) */
    /* residual addressing: flat rows of stride ldr, or strided pixels */
    int ldr;
    int res_strided;       /* 1: res[img*res_img_stride + oy*res_row_stride + ox*res_px_stride + n] */
    int64_t res_img_stride;
    int res_row_stride, res_px_stride;
    int relu;              /* ReLU on `out` after the residual add */
    int tile;              /* 0 = the library's choice; otherwise the number of one tile shape of the kernel family the descriptor selects: the
                              generic implicit GEMM (k_order 0), the 3x3 patch kernels (k_order 1), the 3x3 stream kernel (k_order 2) or the 1x1
                              stream kernel (k_order 2, kh = kw = 1).  csrc/conv_tiles.h lists every tile once -- shape, the columns and operands
                              it takes, its place in the library's choice --, hmmr_conv_tile_info returns a row of that list.  A tile that does
                              not fit the problem is refused (rc -1) before anything is queued; no tile changes a result bit inside its family. */
    /* split-K (for GEMMs with few output tiles and a long K): split_k > 1 slices K into that many
     * contiguous ranges, each range leaves an fp32 partial plane in `ws`, and a second launch adds the
     * planes IN SLICE ORDER and applies the epilogue.  The caller fixes split_k per layer (never from
     * the batch size), so results stay independent of batch composition.  0/1 = off. */
    int split_k;
    void* ws;              /* >= hmmr_conv_splitk_workspace_bytes(M, cout, split_k) */
    size_t ws_bytes;
    /* fused pre-activation of the INPUT: A[m, k] = relu(in * pro_scale[ci] + pro_shift[ci]) applied
     * while the operand is staged (slim bottleneck_v2 `preact` BN + ReLU, consumer side).  [cin]
     * floats each, or both NULL.  Only for 1x1, un-padded convolutions. */
    const float* pro_scale;
    const float* pro_shift;
    /* column split: output channels [n_split, cout) go to out_b (row stride ldo_b, channel n - n_split)
     * with ReLU flag relu_b instead of `out` / `relu` -- two convolutions over the same input as ONE
     * GEMM (the conv shortcut and conv1 of a block's first bottleneck unit).  n_split % 8 == 0; not
     * with out2, res or split_k.  out_b == NULL: off. */
    void* out_b;
    int ldo_b, n_split, relu_b;
    /* second operand source: K = cin + cin2, the first cin elements of a row of A come from `in`, the next cin2 from
     * `in2` -- two 1x1 convolutions over two tensors of the same pixel grid summed in ONE accumulator (a unit's conv3
     * and its conv shortcut: `w` = [W3 | Wsc] along K, `shift` = the sum of the two biases; the shortcut tensor is
     * never stored).  Both tensors dense [M][cin] / [M][cin2] (1x1, stride 1, no padding), cin and cin2 multiples of
     * the 128-byte K step, no pro_scale, no split_k.  in2 == NULL: off. */
    const void* in2;
    int cin2;
    /* order of K inside a filter row.  0: (tap, channel) -- k = (ky*kw + kx)*cin + ci.
     * 1: chunk-major -- k = ((ci / E)*9 + ky*3 + kx)*E + ci % E, E = the elements of one 128-byte K step (32 for a
     * split tensor).  For 3x3 / stride 1 / pad 1 convolutions over a dense NHWC tensor only, and it selects another
     * kernel: a workgroup keeps the 128-byte channel chunk of every input pixel its tile touches (a PATCH: the tile's
     * pixels and a halo of win + 1 pixels on either side) in LDS and reads the nine taps of that chunk as nine shifted
     * fragment sets (out-of-image taps read a zero row), so an input
     * line leaves L2 once per chunk instead of once per tap (the patch tiles; scale/shift/relu epilogue only: no res,
     * out2, out_b, pro_scale, in2, split_k).  The sum over k is the same set of products in another order: results
     * differ from k_order 0 by fp32 rounding of the accumulation only.
     * 2: `w` is not a matrix but the FILTER STREAM of packing.pack_conv3x3_stream (hmmr_conv3x3_stream_bytes(cin, cout) bytes):
     * per 128 output channels, K steps kt = (ci / 16) * 9 + ky*3 + kx of 8 KB = 4 row blocks x (hi plane | lo plane) of MFMA
     * A-operand fragments (lane = 32 * (k half) + row; 8 halves = W[row][16 (ci / 16) + 8 half .. + 7] of that tap), rows scaled
     * like every split filter bank.  Same convolutions and epilogue as k_order 1; split (f16x3) tensors, cin % 32 == 0 -- or bf16 tensors (K steps of 32
     * channels `(ci / 32) * 9 + tap`, the two planes = the two 16-wide MFMA chunks, no row scaling), cin % 64 == 0 --,
     * cout % 128 == 0 or cout = 64, each with tiles of its own and its own widest image (csrc/conv3x3_stream.hip; the 3x3 stream rows of
     * csrc/conv_tiles.h).  Every tile produces the same bits.
     * 2 with kh = kw = 1 (round 5; csrc/conv1x1_stream.hip, the 1x1 stream rows): `w` is the stream of packing.pack_conv1x1_stream
     * (hmmr_conv1x1_stream_bytes(cin + cin2, cout) bytes: K steps of 16 input channels, the same 8 KB per 128 output channels as one tap above).  A
     * stride-1 1x1 convolution over a dense [M][cin] split tensor, cin % 16 == 0 (at least as many K steps as the tile's rings are deep), cout % 128 == 0,
     * scale and shift given; no pro_scale, split_k, batch.  Two epilogues: scale / shift / relu with the out_b column split (n_split % 128 == 0), or
     * -- with any of res / out2 / in2, on the tiles that have one -- the conv3 form: in2 continues K (cin2 % 16 == 0; not together with res), res is a dense
     * shortcut tensor with ldr == ldo, out2 = relu(scale2 * stored(out) + shift2) exactly as k_order 0 defines it.
     * Both operands go through LDS rings (one wave per SIMD), for layers whose K loop is bound by the round trip of
     * a two-stage ring (block 4, block3/unit_1's shortcut + conv1).  Differs from k_order 0 by fp32 rounding of the accumulation only. */
    int k_order;
    /* grouped launch: `batch` > 1 runs that many problems of this one shape as ONE launch (grid z); problem z reads and
     * writes at these BYTE offsets (multiples of 16, negative allowed) from problem 0: `in`, `w`, `out` / `out2`, `res`,
     * `scale` / `scale2` and `shift` / `shift2`.  A stride of 0 shares the operand.  With split_k, `ws` holds batch x the
     * planes.  Not with k_order, out_b, in2, pro_scale.  Problem z's results are those of its own launch, bit for bit
     * (the IEF's two delta regressors, src/models.py:343-361, run this way). */
    int batch;
    int64_t batch_in_bytes, batch_w_bytes, batch_out_bytes, batch_res_bytes, batch_scale_bytes, batch_shift_bytes;
} hmmr_conv_desc_t;

/* One row of the tile list (csrc/conv_tiles.h): everything that is known about one value of hmmr_conv_desc_t.tile. */
#define HMMR_CONV_TILE_MAX 63    /* tile numbers are 1 .. HMMR_CONV_TILE_MAX (csrc/conv_tiles.h refuses a row beyond it at compile time) */
enum { HMMR_TILE_GENERIC = 0, HMMR_TILE_PATCH = 1, HMMR_TILE_STREAM_3X3 = 2, HMMR_TILE_STREAM_1X1 = 3 };
typedef struct {
    int tile, family;          /* HMMR_TILE_* */
    int fm, fn, wgm, wgn;      /* the 32 x 32 accumulators of one wave (pixels x channels), and the waves along pixels x channels */
    int pixels, channels;      /* of one tile: 32 wgm fm x 32 wgn fn */
    int row_blocks;            /* pixels / 32 */
    int depth;                 /* LDS stages of the K loop (the 1x1 stream kernel: ring depth = the fewest K steps it takes; 0: not staged that way) */
    int occupancy;             /* workgroups per CU */
    int wmax;                  /* widest image in pixels; 0 = no limit of the tile's own */
    int split_only;            /* built for split (f16x3) operands only */
    int conv3_form;            /* 1x1 stream: has the res / out2 / in2 epilogue */
    int cols;                  /* cout it takes: 0 = any, 64 = exactly 64, otherwise cout % cols == 0 */
    int tune_cols;             /* hmmr_conv_tile_for offers it only when cout % tune_cols == 0 (0 = any) */
    int narrow;                /* a 64-column tile (cols == 64) */
    int rank;                  /* place among the library's candidates for tile = 0 (1 first); 0 = never chosen */
    int candidate;             /* the tuner candidate that maps onto it; 0 = none */
    const char* text;          /* short description, static storage */
} hmmr_conv_tile_info_t;
/* the row of `tile`; rc -1 for a number that is no tile (0 and the tuner's candidates that are no tile among them) */
int hmmr_conv_tile_info(int tile, hmmr_conv_tile_info_t* out);
/* the tile a layer runs for a tuner candidate or a literal tile number: k_order as packed, filter_1x1 / conv3_form as launched (read with
 * k_order 2), cout columns, operand dtype (negative: not known).  0 = the library's choice, where nothing fits; never an error. */
int hmmr_conv_tile_for(int k_order, int filter_1x1, int conv3_form, int cout, int dtype, int candidate);
/* The next two are part of the ABI like every other entry point, to stay: the fit rule is exported so that the host tests can hold
 * hmmr_conv_tile_for's answers against it, the f_movie tile so that the C packer and the Python packer read one constant.
 * The fit rule every dispatcher of hmmr_conv_gemm asks before it queues anything: does `tile` (not 0) take a problem of that kind?  cout, win (image
 * width) and ksteps (1x1 stream: (cin + cin2) / 16) of 0 and a negative dtype are "not known, not checked".  0, or -1 with the reason in hmmr_last_error. */
int hmmr_conv_tile_fits(int tile, int k_order, int filter_1x1, int conv3_form, int cout, int dtype, int win, int ksteps);
/* the tile the packers give the f_movie convolutions of a split model */
int hmmr_conv_tile_f_movie(void);

int hmmr_conv_gemm(const hmmr_conv_desc_t* d, void* stream);
size_t hmmr_conv_splitk_workspace_bytes(int m, int cout, int split_k);

/* ------------------------------------------------------------------------- *
 * ResNet-v2-50 image encoder: encoder_resnet (src/models.py:50-77) ->
 * tf.contrib.slim.nets.resnet_v2.resnet_v2_50(num_classes=None,
 * is_training=False) + squeeze.  images [n,224,224,3] fp32 in [-1,1] -> phi
 * [n,2048] fp32.
 * ------------------------------------------------------------------------- */
typedef struct {
    const void* w;         /* packed [cout_pad][K] in the struct's dtype */
    const float* scale;    /* folded BN scale or NULL */
    const float* shift;    /* folded BN shift or conv bias */
    int tile;              /* hmmr_conv_desc_t.tile for this layer's launch; 0 = library heuristic.
                              Results do not depend on it (same K order per output element);
                              the host may tune it per layer and batch size. */
    int k_order;           /* hmmr_conv_desc_t.k_order the filter rows of `w` were packed in (read for the 3x3 conv2 layers, and -- 2: the filter stream of
                              csrc/conv1x1_stream.hip -- for conv1 and the shortcut + conv1 bank sc_c1; such a unit has fuse_preact = 0) */
} hmmr_layer_t;

typedef struct {
    hmmr_layer_t conv1, conv2, conv3, shortcut;   /* shortcut.w == NULL: identity / subsample */
    hmmr_layer_t c3sc;         /* optional (stride-1 units with a conv shortcut): [W3 | Wsc] as one [depth][base + c_in]
                                  filter bank, shift = conv3 bias + shortcut bias: conv3 and the shortcut as ONE GEMM over
                                  {h2, preact} (hmmr_conv_desc_t.in2); needs fuse_preact == 0.  w == NULL: separate launches */
    hmmr_layer_t sc_c1;        /* optional: rows [shortcut (depth); conv1 (base)] of one [depth+base][c_in] filter
                                  bank with scale = [1..1; BN scale], shift = [bias; BN shift]: both convs as
                                  one column-split GEMM.  w == NULL: two launches. */
    const void* w3_frag;       /* f16x3 fused tail (fuse_tail == 1): this unit's conv3 filters ([W3 | Wsc] when c3sc is set) */
    const void* w1n_frag;      /* ... and the NEXT unit's conv1 filters, both FRAGMENT-MAJOR (hmmr_tail_desc_t); else NULL */
    const void* pair_stream;   /* f16x3 fused tail of blocks 2-3 (fuse_tail == 1): this unit's conv3 filters ([W3 | Wsc] when c3sc is
                                  set) and the NEXT unit's conv1 filters as ONE fragment stream (hmmr_tail_desc_t.pair_stream); else NULL */
    const void* conv1_frag;    /* f16x3, unit 0 only (optional): this unit's conv1 filters [base][c_in] FRAGMENT-MAJOR (as w3_frag): the fused stem
                                  computes block1/unit_1's conv1 on its pooled tile in the same launch (csrc/stem.hip); else NULL */
    const void* unit_stream;   /* f16x3 whole-unit kernel of block 1 (fuse_tail == 2, conv2.k_order == 2): conv2's, conv3's ([W3 | Wsc]) and
                                  the NEXT unit's conv1 filters as ONE fragment stream (hmmr_tail_desc_t.unit_stream); else NULL */
    const float* pre_scale;    /* this unit's folded `preact` BN, [c_in] */
    const float* pre_shift;
    int c_in, base, depth, stride;
    int fuse_preact;           /* 1: conv1/shortcut apply the preact while staging their operand;
                                  0: the previous unit's conv3 writes the preact tensor */
    int fuse_tail;             /* what the unit ends in (hmmr_unit_plan_t.end, HMMR_END_*: the dtype and the streams above pick the kernel; 0: HMMR_END_CONV3_LAUNCH)
                                  4: stride-2 unit: conv2 + conv3 + add as one launch, no next conv1;
                                  3: as 2, and the unit's conv shortcut is computed in that launch too (c_in 64);
                                  2: as 1, with this unit's conv2 inside the same launch as well;
                                  1: this unit's conv3 + add and the NEXT unit's preact + conv1 run as one
                                  hmmr_bottleneck_tail launch (bf16, stride 1, block1 or block2 shapes, next unit
                                  of the same block with identity shortcut and fuse_preact) */
} hmmr_resnet_unit_t;

#define HMMR_RESNET_UNITS 16

typedef struct {
    int dtype;                         /* operand type of convs + activations */
    hmmr_layer_t stem;                 /* 7x7/2 packed as [128][8 taps x (8 px x 4 ch)] */
    hmmr_resnet_unit_t unit[HMMR_RESNET_UNITS];
    const float* post_scale;           /* postnorm BN folded */
    const float* post_shift;
} hmmr_resnet_weights_t;

/* ------------------------------------------------------------------------- *
 * Fused tail of a bottleneck unit (slim resnet_v2.bottleneck as invoked at src/models.py:65-75):
 *   out    = conv3(h2) * scale3 + shift3 + shortcut         (1x1, c_mid -> depth, no ReLU)
 *   out_h1 = relu(conv1'(relu(out * pre_scale + pre_shift)) * scale1 + shift1)
 * i.e. this unit's `conv3` + add and the NEXT unit's `preact` + `conv1` in one launch, so the next
 * conv1 does not re-read the trunk from HBM.  Bit-identical to the two hmmr_conv_gemm launches it
 * replaces (conv3 with a residual; conv1 with pro_scale/pro_shift).  bf16; (c_mid, depth, n2) = (64, 256, 64)
 * [block1] or (128, 512, 128) [block2].
 * The shortcut is read as rows of `ldr` elements, or (res_strided) as x[:, ::s, ::s] of an NHWC
 * tensor like hmmr_conv_desc_t's strided residual (ho, wo = output grid).
 * dtype HMMR_F16X3 (csrc/bottleneck_split.hip): the next conv1 always; conv2 in front (h1; w2 packed like every filter bank; stride 1, 8 x 8
 * pixel tiles: hin, win multiples of 8) for the 64 -> 256 -> 64 shape only; w3 and w1 are
 * FRAGMENT-MAJOR: [rows / 32][K / 16][64 lanes][hi 16 B | lo 16 B], lane = 32 * (k half) + row, the 16 bytes = the 8
 * bf16 of W[32 rb + row][16 kc + 8 half .. + 7] (one coalesced 2 KB read per MFMA A operand, straight from L2).  With xp
 * (and res == NULL) conv3's K is {h2, xp} against w3 = [W3 | Wsc], shift3 = the summed biases: the conv shortcut folded
 * into conv3 exactly as hmmr_conv_desc_t.in2 does.  Bit-identical to the launches it replaces in either form.
 * ------------------------------------------------------------------------- */
typedef struct {
    int dtype;                      /* HMMR_BF16 or HMMR_F16X3 */
    const void* h2; int m; int c_mid; int depth;
    const void* w3; const float* scale3; const float* shift3;      /* [depth][c_mid]; scale3 may be NULL */
    const void* res; int ldr; int res_strided; int64_t res_img_stride; int res_row_stride, res_px_stride; int ho, wo;
    void* out;                      /* [m][depth] */
    const float* pre_scale; const float* pre_shift;                /* [depth] */
    const void* w1; const float* scale1; const float* shift1; int relu1; int n2;   /* [n2][depth] */
    void* out_h1;                   /* [m][n2] */
    /* optional conv2 in front: h2 = NULL and h2 := relu(conv3x3(h1) * scale2 + shift2),
     * SAME padding, stride 1, computed per tile inside the same launch (slim bottleneck_v2 `conv2`) */
    const void* h1; int hin, win;   /* [m / (hin*win)][hin][win][c_mid] */
    const void* w2; const float* scale2; const float* shift2;      /* [c_mid][9 * c_mid], K = (ky, kx, ci) */
    /* optional conv shortcut computed in the launch (block1/unit_1: needs h1; res = NULL):
     * shortcut = xp x wsc + shift_sc, rounded to bf16 as the separate launch would store it */
    const void* xp;                 /* [m][64]: the (pre-activated) input of the unit */
    const void* wsc; const float* shift_sc;                        /* [depth][64], [depth] */
    /* conv2 stride (0/1 or 2; ho, wo = its output grid, m = images * ho * wo) and the single-phase form for a
     * block's stride-2 last unit: w1 == NULL -> no next conv1; `out` (raw trunk) and/or `out_pre`
     * (relu(out * pre_scale + pre_shift), what the next unit's conv1 AND conv shortcut read) are written */
    int conv2_stride;
    void* out_pre;                  /* [m][depth] or NULL */
    /* HMMR_F16X3, (c_mid, depth, n2) = (256, 1024, 256) [block3] or (128, 512, 128) [block2]: the register-resident unit pair
     * (csrc/unit_pair.hip).  w3 / w1 are not read; `pair_stream` holds both filter banks as the flat sequence of 2 KB MFMA
     * A-operand fragments ([hi plane: 64 lanes x 16 B][lo plane]; lane = 32 * (k half) + row, the 16 bytes = the 8 halves of
     * W[32 rb + row][16 kc + 8 half .. + 7], rows scaled like every split filter bank) the kernel consumes:
     * depth / 32 + 2 iterations; iteration `it` holds the kc3 = (c_mid + c_xp) / 16 fragments of conv3 row block `it` (K chunks in
     * order; zeros for it >= depth / 32) and the n2 / 16 fragments of conv1' K step it - 2 (K chunk 2 (it - 2) + {0, 1}, row blocks in
     * order; zeros for it < 2), fragment i of an iteration being a conv3 fragment when ((i + 1) kc3) / ft > (i kc3) / ft, ft = the
     * iteration's fragment count (hmmr_pair_stream_bytes; packing.pack_pair_stream).  With xp (c_xp = its channels, 256 for the
     * block2 shape; res == NULL) conv3's K is {h2, xp} as in the block1 form.  h2 only (no conv2 in front).  Bit-identical to
     * the launches it replaces. */
    const void* pair_stream;
    int c_xp;
    /* HMMR_F16X3, (c_mid, depth, n2) = (64, 256, 64) [block1] with conv2 in front (h1; hin x win whole images, win <= 56): the whole-unit
     * kernel of csrc/b1_unit.hip.  w2 / w3 / w1 are not read; `unit_stream` holds ALL filters of the unit as the flat sequence of 2 KB
     * MFMA A-operand fragments ([hi plane: 64 lanes x 16 B][lo plane], lane = 32 * (k half) + row, rows scaled like every split filter
     * bank) the kernel consumes (hmmr_b1_unit_stream_bytes; packing.pack_b1_unit_stream): conv2's stream exactly as k_order = 2 packs it
     * for cout = 64 (36 K steps kt = (ci / 16) * 9 + tap of two row blocks), then, with A(c) = the kc3 = (64 + c_xp) / 16 fragments of
     * conv3 row block c (32 output channels; K chunks in order) and B(c) = the four fragments of conv1' K chunks 2 c, 2 c + 1 (row blocks
     * 0, 1 of each): A(0) | A(1) B(0) | A(2) B(1) | ... | A(7) B(6) | B(7) (the order of the kernel's software pipeline).  scale2 / shift2: conv2's folded BN as the k_order 2 layer carries it.  With xp (c_xp = 64; res == NULL)
     * conv3's K is {h2, xp}.  Bit-identical to hmmr_conv_gemm(k_order 2) + conv3 + conv1 as three launches. */
    const void* unit_stream;
    /* HMMR_F16X3 with pair_stream or unit_stream: 0 or 1 = every row of `out` is stored.  s > 1: the caller promises that `out` is read
     * only as x[:, ::s, ::s] of its [m / (ho * wo)][ho][wo][depth] images (unit_stream: hin x win) -- the strided identity shortcut of a
     * stride-s unit whose conv1 this launch computes -- and the launch stores only those rows; the others keep what they held.  out_h1,
     * the run flags and every stored row are the same bits.  Refused (nothing queued) on any other route, with out_pre, s < 0, or a
     * pair_stream launch without whole ho x wo images.  hmmr_resnet50_fwd sets it where its plan says so (hmmr_unit_plan_t); a
     * stand-alone caller's 0 keeps every row. */
    int trunk_keep_stride;
} hmmr_tail_desc_t;
size_t hmmr_pair_stream_bytes(int kc3, int depth, int n2);
size_t hmmr_b1_unit_stream_bytes(int c_xp);
/* measurement aid (bench.py's `roofline.mfma_sustained`): one launch of `workgroups` x 4 waves, one wave per SIMD, each issuing 8 * n8
 * v_mfma_f32_32x32x16_f16 (32768 FLOP each) on four independent accumulators and nothing else.  out: NULL or workgroups * 256 floats.
 * n8 < 0 (ABI 19): -n8 iterations on operands that CHANGE from MFMA to MFMA (four hashed fragment pairs in turn) -- the constant-operand loop is the
 * lowest-power case, so the clock the power cap allows it is higher than any real tensor gets. */
int hmmr_mfma_rate_probe(int workgroups, int n8, float* out, void* stream);
/* (ABI 19) measurement aid: one wave that stores n (s_memtime, s_memrealtime) pairs -- shader-clock ticks against the constant reference counter
 * (hipDeviceAttributeWallClockRate) -- `sleep` x ~4 us apart into `samples` (2 n words, zeroed by the caller), until n are taken or *stop (NULL or a device
 * int set from another stream) is non-zero.  Run on its own stream beside a measured region: the clock the part sustains under that load (bench.py). */
int hmmr_clock_probe(unsigned long long* samples, int n, int sleep, const int* stop, void* stream);
/* bytes of the filter stream of a k_order 2 layer of split tensors: (cout / 128) x 9 (cin / 16) K steps of 8 KB (bf16 tensors: half of it,
 * 9 (cin / 32) K steps) */
size_t hmmr_conv3x3_stream_bytes(int cin, int cout);
/* bytes of the filter stream of a 1x1 layer with k_order 2 (split tensors): (cout / 128) x (cin / 16) K steps of 8 KB */
size_t hmmr_conv1x1_stream_bytes(int cin, int cout);
int hmmr_bottleneck_tail(const hmmr_tail_desc_t* d, void* stream);

size_t hmmr_resnet50_workspace_bytes(int n, int dtype);
/* prof_ms: NULL, or a host array of HMMR_RESNET_PROF_SLOTS floats that receives
 * the HIP-event duration (ms) of every launch (forces a stream sync). */
#define HMMR_RESNET_PROF_SLOTS 64
/* n_zero: that many all-zero images are appended after the n real ones (the padding frames of
 * predict_all_images, tester.py:285-289, are zero IMAGES that still go through the encoder);
 * phi has n + n_zero rows, the workspace must be sized for n + n_zero. */
/* images must be 16-byte aligned (every image then is: 224 x 224 x 3 floats are a multiple of 16 bytes): the fused stem kernels read
 * them as aligned groups of 4 floats.  A pointer that is not is refused before anything is queued, on either stem route. */
int hmmr_resnet50_fwd(const hmmr_resnet_weights_t* w, const float* images, int n, int n_zero,
                      float* phi, void* ws, size_t ws_bytes, void* stream, float* prof_ms);

/* The stem of that pass ALONE: exactly the launches hmmr_resnet50_fwd starts with (one function issues both), into tensors the caller
 * owns -- 7x7/2 conv + bias, the 3x3/2 TF-SAME max pool, the pre-activation BN + ReLU of block1/unit_1 -> pooled [n + n_zero][56][56][64]
 * in the storage type of w->dtype, and, where the schedule has the fused kernel compute it (bf16; f16x3 with unit[0].conv1_frag; not
 * with hmmr_debug_t.stem_no_conv1 or on the three-kernel route), that unit's conv1 + BN + ReLU -> h1 of the same shape.  h1 may be
 * NULL (then it is not computed); *h1_written (may be NULL) says whether h1 was written.  hmmr_debug_t.stem_route / stem_no_conv1 are
 * honoured as in the full pass.  The workspace (the re-packed image and the 112 x 112 conv map) is needed by the three-kernel route only:
 * the query answers 0 for the fused route under the CURRENT debug switches, and ws may then be NULL.
 * Refused before anything is queued: a null argument (images may be NULL only when n == 0), n < 0, n_zero < 0, n + n_zero == 0, a bad
 * dtype, a short workspace, images not 16-byte aligned, and -- on the fused route in bf16 / fp32 mode -- a non-NULL stem.scale: that
 * kernel applies none, the three-kernel route does, so the two would disagree (hmmr_resnet50_fwd refuses the last two as well).
 * For tests and measurements of the stem (tests/test_gpu_stem.py); a product pass calls hmmr_resnet50_fwd. */
size_t hmmr_resnet50_stem_workspace_bytes(const hmmr_resnet_weights_t* w, int n_total);
int hmmr_resnet50_stem(const hmmr_resnet_weights_t* w, const float* images, int n, int n_zero, void* pooled, void* h1,
                       int* h1_written, void* ws, size_t ws_bytes, void* stream);

/* What hmmr_resnet50_fwd launches for one unit: decided for all 16 units, from the unit table, the frame count and hmmr_debug_t,
 * BEFORE the first launch (an inconsistent table is refused with the unit named and nothing queued), then issued in order.
 * Profile slots per unit: [shortcut, when it is not HMMR_SC_NONE] conv1 conv2 conv3 -- a layer without a launch of its own
 * keeps its (empty) slot. */
enum { HMMR_SC_NONE = 0,             /* identity / subsampled shortcut: no filter bank */
       HMMR_SC_LAUNCH,               /* a 1x1 GEMM of its own */
       HMMR_SC_LAUNCH_WITH_CONV1,    /* ... with conv1 as extra output columns (sc_c1) */
       HMMR_SC_IN_CONV3,             /* folded into conv3's K (c3sc), wherever conv3 runs */
       HMMR_SC_IN_TAIL };            /* computed inside the fused tail (fuse_tail 3) */
enum { HMMR_CONV1_LAUNCH = 0,
       HMMR_CONV1_READY };           /* no launch: the stem, the previous unit's tail or this unit's shortcut launch wrote it */
enum { HMMR_CONV2_LAUNCH = 0, HMMR_CONV2_IN_TAIL };
enum { HMMR_END_CONV3_LAUNCH = 0,    /* conv3 + add as one GEMM (fuse_tail 0, or a demoted unit pair) */
       HMMR_END_TAIL_BF16,           /* csrc/bottleneck.hip: conv3 + add + the next unit's preact + conv1 (fuse_tail 1 .. 3) */
       HMMR_END_TAIL_BF16_STRIDE2,   /* csrc/bottleneck.hip, single phase: conv2 + conv3 + add, no next conv1 (fuse_tail 4) */
       HMMR_END_TAIL_SPLIT,          /* csrc/bottleneck_split.hip: the LDS-panel tail (w3_frag / w1n_frag) */
       HMMR_END_B1_UNIT,             /* csrc/b1_unit.hip: conv2 .. the next conv1 of a block-1 unit (unit_stream) */
       HMMR_END_UNIT_PAIR };         /* csrc/unit_pair.hip (pair_stream) */
typedef struct {
    int shortcut, conv1, conv2, end; /* HMMR_SC_* / HMMR_CONV1_* / HMMR_CONV2_* / HMMR_END_* */
    int reads_fused_preact;          /* conv1 / the shortcut read the raw trunk and pre-activate while staging */
    int writes_raw, writes_pre;      /* the end writes the raw trunk / the next unit's pre-activated tensor */
    int pair_demoted;                /* fewer pixels than hmmr_debug_t.pair_min_pixels: the two launches instead of the unit pair */
    int swaps_t1_t2;                 /* the tail wrote the next conv1 into the OTHER bottleneck buffer (conv2 ran inside it) */
    int leaves_h1;                   /* the next unit's conv1 is HMMR_CONV1_READY */
    int trunk_keep_stride;           /* > 1: the end stores only the raw trunk rows x[:, ::s, ::s] (hmmr_tail_desc_t.trunk_keep_stride) */
} hmmr_unit_plan_t;
/* Host only: no HIP call, reads the same hmmr_debug_t as the pass.  n_total = n + n_zero.  -1: the table is inconsistent
 * (hmmr_last_error names the unit). */
int hmmr_resnet50_plan(const hmmr_resnet_weights_t* w, int n_total, hmmr_unit_plan_t out[HMMR_RESNET_UNITS]);

/* ------------------------------------------------------------------------- *
 * f_movie temporal encoder: az_fc2_groupnorm / az_fc_block2
 * (src/models.py:121-228).  phi [b, t, 2048] fp32 -> strips [b, t, 2048] fp32.
 * ------------------------------------------------------------------------- */
typedef struct {
    const float* gn1_gamma; const float* gn1_beta;
    hmmr_layer_t conv1;                /* w [2048][3*2048], shift = bias */
    const float* gn2_gamma; const float* gn2_beta;
    hmmr_layer_t conv2;
} hmmr_temporal_block_t;

#define HMMR_MAX_TEMPORAL_BLOCKS 8

typedef struct {
    int dtype;
    int num_blocks;
    hmmr_temporal_block_t block[HMMR_MAX_TEMPORAL_BLOCKS];
} hmmr_temporal_weights_t;

size_t hmmr_temporal_workspace_bytes(int b, int t, int dtype);
int hmmr_temporal_fwd(const hmmr_temporal_weights_t* w, const float* phi, int b, int t,
                      float* strips, void* ws, size_t ws_bytes, void* stream);

/* Hallucinator fc2_res (src/models.py:270-296, pred_mode == 'hal'): phi [m,2048] fp32 ->
 * phi + fc3(relu(fc2(relu(fc1 phi)))) [m,2048] fp32; each w is [2048][2048], shift = bias. */
typedef struct {
    int dtype;
    hmmr_layer_t fc1, fc2, fc3;
} hmmr_hallucinator_weights_t;

size_t hmmr_hallucinator_workspace_bytes(int m, int dtype);
int hmmr_hallucinator_fwd(const hmmr_hallucinator_weights_t* w, const float* phi, int m,
                          float* out, void* ws, size_t ws_bytes, void* stream);

/* Standalone GroupNorm(+ReLU) over (time, channels-in-group), exposed for tests:
 * tf.contrib.layers.group_norm(reduction_axes=(-3,-2)), src/models.py:155-161. */
int hmmr_groupnorm_relu(const float* x, const float* gamma, const float* beta, int b, int t,
                        int c, int groups, void* out, int out_dtype, void* stream);

/* ------------------------------------------------------------------------- *
 * IEF regressors: batch_pred_omega / call_hmr_ief / hmr_ief /
 * encoder_fc3_dropout (src/models.py:80-116, 233-267, 299-415).
 * strips [m,2048] fp32 -> omega[r] [m,85] fp32 for r = 0 (present) and each
 * delta regressor, already in the final layout.  Default (all flags 0) = the
 * Tester configuration use_optcam=True, use_delta_from_pred=True
 * (tester.py:196-207): a delta regressor starts from omega0[:, 3:75], predicts
 * 72 values and returns [1,0,0 | pose | beta of omega0] (models.py:349-371).
 * no_optcam (use_optcam=False): it starts from [:, :75], predicts 75 values
 * and returns [cam, pose | beta] (models.py:357-373).  delta_from_start
 * (use_delta_from_pred=False): start and beta come from the IEF's own
 * starting point (omega_start / the mean theta) instead of omega0 (:349-351).
 * ------------------------------------------------------------------------- */
typedef struct {
    int nd;                            /* 85 (present); 72 (delta) or 75 (delta with no_optcam) */
    hmmr_layer_t fc1_phi;              /* w [1024][2048], shift = fc1 bias */
    hmmr_layer_t fc1_theta;            /* w [1024][128]: rows of fc1 for theta, zero padded */
    hmmr_layer_t fc2;                  /* w [1024][1024], shift = bias */
    hmmr_layer_t fc3;                  /* w [128][1024] (nd rows used), shift = bias padded */
} hmmr_ief_regressor_t;

#define HMMR_MAX_REGRESSORS 8

typedef struct {
    int dtype;
    int num_regressors;                /* [0] = present, then deltas in sorted delta_t order */
    int num_stages;                    /* 3 */
    hmmr_ief_regressor_t reg[HMMR_MAX_REGRESSORS];
    const float* mean_theta;           /* [85] */
    int no_optcam;                     /* 1: use_optcam=False (every delta regressor has nd == 75) */
    int delta_from_start;              /* 1: use_delta_from_pred=False */
} hmmr_ief_weights_t;

/* One set of layer buffers per delta regressor (num_regressors - 1 of them, at least one): the delta regressors run as
 * grouped launches, one per layer (hmmr_conv_desc_t.batch), when their filter banks / vectors lie at one common byte stride
 * -- always the case for two of them -- and one after the other otherwise; same results either way. */
size_t hmmr_ief_workspace_bytes(int m, int num_regressors, int dtype);
/* omegas: [num_regressors][m][85] fp32.  The IEF starts from w->mean_theta in every row (tester.py:79-83, 181). */
int hmmr_ief_fwd(const hmmr_ief_weights_t* w, const float* strips, int m, float* omegas,
                 void* ws, size_t ws_bytes, void* stream);
/* ... or from a caller-given starting point per row: omega_start [m][85] fp32 (`omega_mean` of batch_pred_omega,
 * src/models.py:231-249); NULL = w->mean_theta. */
int hmmr_ief_fwd_from(const hmmr_ief_weights_t* w, const float* strips, const float* omega_start, int m, float* omegas,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * IEF backward (additive to ABI 19; csrc/ief_grad.hip): the regressors as the trainer runs them
 * (src/trainer_sequence_fc.py on precomputed movie strips; slim.dropout(0.5) behind fc1 and fc2, src/models.py:103-105) and
 * their derivative.  The function differentiated is the exact fp32 one: both entry points take a bank packed with
 * dtype == HMMR_F32 (plain [cout_pad][K] fp32 rows, fc1_theta [1024][128], biases in `shift`, no `scale`) and refuse every other.
 * For regressor r and stage s, theta_0 = the regressor's start:
 *     a1 = phi . W1[:2048] + b1 + theta_s . W1[2048:]      h1 = relu(a1) * keep[r][s][0] * keep_scale
 *     a2 = h1 . W2 + b2                                    h2 = relu(a2) * keep[r][s][1] * keep_scale
 *     theta_{s+1} = theta_s + h2 . W3 + b3
 * keep: uint8 [R][num_stages][2][m][1024] of zeros and ones, or NULL = no dropout (then keep_scale is not read, and the result is
 * bit for bit that of an all-ones mask with keep_scale = 1); keep_scale = 1 / keep_prob.  relu'(0) = 0.  The regressors are wired
 * as in hmmr_ief_fwd_from (no_optcam / delta_from_start) and there is no stop-gradient: with use_delta_from_pred a delta's start
 * omega0[:, 3:75] (or [:, :75]) and the beta columns 75..84 it copies pass their gradient to the present regressor's output, with
 * delta_from_start to omega_start; columns 0..2 of a 72-wide delta's d_omega belong to the constants [1, 0, 0] and are ignored.
 * Order of the backward: the delta regressors in regressor order; their contributions to d_omega0 (or d_omega_start) added in
 * that order; the present regressor; d_strips is added up in the same order.  No floating-point atomics, every contraction in a
 * fixed order with a split that does not depend on m: equal inputs give equal bytes, a row's d_strips / d_omega_start does not
 * depend on the other rows of the call, grouped and ungrouped launches (hmmr_debug_t.ief_no_group) give the same bytes.
 * Nothing is kept from a forward call: hmmr_ief_bwd recomputes it into its workspace by the routine hmmr_ief_fwd_train runs.
 * ------------------------------------------------------------------------- */
typedef struct {                       /* one regressor's gradients in the layouts of the HMMR_F32 bank itself; each may be NULL */
    float* d_fc1_phi;                  /* [1024][2048] */
    float* d_fc1_theta;                /* [1024][128], columns >= nd written as zeros */
    float* d_fc2;                      /* [1024][1024] */
    float* d_fc3;                      /* [128][1024], rows >= nd written as zeros */
    float* d_b1;                       /* [1024] */
    float* d_b2;                       /* [1024] */
    float* d_b3;                       /* [128], entries >= nd written as zeros */
} hmmr_ief_reg_grads_t;

typedef struct {
    const float* strips;               /* [m][2048]: the forward's inputs ... */
    const float* omega_start;          /* [m][85] or NULL = w->mean_theta in every row */
    const unsigned char* keep;         /* [R][num_stages][2][m][1024] or NULL */
    float keep_scale;
    int m;
    const float* d_omegas;             /* [R][m][85]: the gradient of a loss with respect to what hmmr_ief_fwd_train returned */
    float* d_strips;                   /* [m][2048] or NULL.  Outputs: a NULL one is skipped and its launches are not queued; at least */
    float* d_omega_start;              /* [m][85] or NULL      one is required (with omega_start NULL: the gradient of the broadcast rows) */
    hmmr_ief_reg_grads_t reg[HMMR_MAX_REGRESSORS];
} hmmr_ief_bwd_desc_t;

/* One layout for both entry points: 0 for m <= 0, num_regressors outside 1..HMMR_MAX_REGRESSORS or num_stages < 1. */
size_t hmmr_ief_bwd_workspace_bytes(int m, int num_regressors, int num_stages);
/* The training form of hmmr_ief_fwd_from: omegas [num_regressors][m][85] in the same layout.  Workspace:
 * hmmr_ief_bwd_workspace_bytes(m, w->num_regressors, w->num_stages).  Refused with -1 before anything is queued: a null w,
 * strips, omegas or ws; m <= 0; a bank that is not HMMR_F32; bad num_regressors / num_stages / nd; keep given with a
 * keep_scale that is not a positive finite number; a workspace that is too small. */
int hmmr_ief_fwd_train(const hmmr_ief_weights_t* w, const float* strips, const float* omega_start, const unsigned char* keep,
                       float keep_scale, int m, float* omegas, void* ws, size_t ws_bytes, void* stream);
/* Refused with -1 before anything is queued: what hmmr_ief_fwd_train refuses (desc->strips, ...), a null desc or d_omegas, and a
 * descriptor that asks for no output. */
int hmmr_ief_bwd(const hmmr_ief_weights_t* w, const hmmr_ief_bwd_desc_t* desc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * f_movie / hallucinator backward (additive to ABI 19; csrc/movie_grad.hip): the derivative of the two modules the
 * reference's sequence trainer trains in front of the regressors (src/trainer_sequence_fc.py:635-665, 839-846).  Neither has a
 * dropout (src/models.py:121-228, 270-296), so the training forward IS hmmr_temporal_fwd / hmmr_hallucinator_fwd on a bank packed
 * with dtype == HMMR_F32: conv*.w plain [2048][3*2048] fp32 rows with k = tap*2048 + ci (fc*.w [2048][2048]), the bias in `shift`,
 * no `scale`.  The function differentiated is that exact fp32 one; every other dtype is refused.  Per temporal block, on the rows
 * of one window (rows outside it are zeros):
 *     h1 = relu(GN1(x))    c1[r] = b1 + sum_tap h1[r + tap - 1] . W1[:, tap]    h2 = relu(GN2(c1))    y = x + b2 + conv(h2, W2)
 * GN: 32 groups, mean and population variance over (t, 64 channels), eps 1e-6, recomputed in the forward's two-pass form.
 * Hallucinator: h1 = relu(phi . W1^T + b1), h2 = relu(h1 . W2^T + b2), out = phi + h2 . W3^T + b3.
 * Contract:
 *  - Nothing is kept from a forward call.  The backward recomputes the forward into its workspace with the launches
 *    hmmr_temporal_fwd / hmmr_hallucinator_fwd queue on an fp32 bank (hmmr_groupnorm_relu, then hmmr_conv_gemm with the same
 *    split-K); the last layer's output, which no gradient reads, is not recomputed.  Per block it keeps the block input, the
 *    conv1 output and the two GN+ReLU outputs, all fp32.
 *  - The ReLU gate is h > 0 on the stored GN+ReLU (fc+ReLU) output: relu'(0) = 0.
 *  - No floating-point atomics; every contraction and reduction has a fixed order: equal inputs give equal bytes.
 *  - The data-gradient contraction (6144 long for a conv, 2048 for an fc) is cut into 8 fixed slices added in slice order; the
 *    split does not depend on b, t or m, so a window's d_phi (a row's, for the hallucinator) does not depend on the other windows
 *    (rows) of the call.  The weight gradients contract over the b*t (m) rows in 4 slices; d_gamma / d_beta / bias gradients are
 *    summed in window (row) order in double and rounded once.
 *  - A NULL output is skipped and its launches are not queued; with d_phi NULL the chain stops at the lowest block that has a
 *    wanted gradient.
 *  - Refused with -1 before anything is queued: a null w, desc, phi, cotangent or ws; non-positive b, t or m; a bank that is not
 *    HMMR_F32 (or has a scaled / missing layer); num_blocks outside 1..HMMR_MAX_TEMPORAL_BLOCKS; a descriptor that asks for no
 *    output (gradients of blocks >= num_blocks do not count); a workspace that is too small.
 * ------------------------------------------------------------------------- */
typedef struct {                       /* one block's gradients in the layouts of the HMMR_F32 bank itself; each may be NULL */
    float* d_gn1_gamma; float* d_gn1_beta;     /* [2048] */
    float* d_conv1; float* d_b1;               /* [2048][6144], [2048] */
    float* d_gn2_gamma; float* d_gn2_beta;
    float* d_conv2; float* d_b2;
} hmmr_temporal_block_grads_t;

typedef struct {
    const float* phi;                  /* [b][t][2048]: the forward's input */
    int b, t;
    const float* d_strips;             /* [b][t][2048]: the gradient of a loss with respect to what hmmr_temporal_fwd returned */
    float* d_phi;                      /* [b][t][2048] or NULL */
    hmmr_temporal_block_grads_t block[HMMR_MAX_TEMPORAL_BLOCKS];
} hmmr_temporal_bwd_desc_t;

/* 0 for b <= 0, t <= 0 or num_blocks outside 1..HMMR_MAX_TEMPORAL_BLOCKS. */
size_t hmmr_temporal_bwd_workspace_bytes(int b, int t, int num_blocks);
int hmmr_temporal_bwd(const hmmr_temporal_weights_t* w, const hmmr_temporal_bwd_desc_t* desc, void* ws, size_t ws_bytes, void* stream);

typedef struct {
    const float* phi;                  /* [m][2048]: the forward's input */
    int m;
    const float* d_out;                /* [m][2048] */
    float* d_phi;                      /* [m][2048] or NULL */
    float* d_fc1; float* d_fc2; float* d_fc3;  /* [2048][2048] each, or NULL */
    float* d_b1; float* d_b2; float* d_b3;     /* [2048] each, or NULL */
} hmmr_hallucinator_bwd_desc_t;

/* 0 for m <= 0. */
size_t hmmr_hallucinator_bwd_workspace_bytes(int m);
int hmmr_hallucinator_bwd(const hmmr_hallucinator_weights_t* w, const hmmr_hallucinator_bwd_desc_t* desc, void* ws, size_t ws_bytes,
                          void* stream);

/* ------------------------------------------------------------------------- *
 * Pose discriminator (additive to ABI 19; csrc/disc_pose.hip): PoseDiscriminator (src/discriminators.py), the losses
 * of src/ops.py:127-136 and compute_losses_prior (src/trainer_sequence_fc.py:989-1020), forward and derivative.  Per row the
 * input is x[23][9], the rotation matrices of joints 1..23 (the global rotation is dropped, as in poses_comb[:, 1:]):
 *     a1[j] = x[j] . C1 + bc1            h1 = relu(a1)      C1 [9][32]      (D_pose/D_conv1, a 1x1 conv: shared by the joints)
 *     a2[j] = h1[j] . C2 + bc2           h2 = relu(a2)      C2 [32][32]     (D_pose/D_conv2)
 *     out[j] = h2[j] . wj[j] + bj[j]     j = 0..22          wj [23][32]     (D_pose/pose_out_j{j}: one fc per joint)
 *     a3 = flat(h2) . F1 + b1            h3 = relu(a3)      F1 [736][1024], flat index j*32 + c   (D_alljoints_fc1)
 *     a4 = h3 . F2 + b2                  h4 = relu(a4)      F2 [1024][1024]                        (D_alljoints_fc2)
 *     out[23] = h4 . fo + bo                                                                        (D_alljoints_out)
 * relu'(0) = 0.  out is always [n][24] (the reference's tf.squeeze fails for one row).  With rows in two segments, real then fake:
 *     e_pose = mean_fake sum_24 (out - 1)^2    d_real = mean_real sum_24 (out - 1)^2    d_fake = mean_fake sum_24 out^2
 * and d_pose = d_fake + d_real, each mean over its own segment's rows (the reference needs equal counts; here either may be empty).
 * The reference's slim.l2_regularizer(d_wd) fills a collection its gather_losses never reads: weight decay has no effect on
 * d_loss, and none is built here.
 * Rows come as two segments {ptr, ld, n}: ptr is the first of a row's 207 values, ld the floats from one row to the next (>= 207).
 * A caller passes hmmr_smpl_fwd's Rs + 9 with ld = 216, and mocap rows the same way: nothing is concatenated or copied.  Row r
 * of `out` / `d_out` is row r of rows_a for r < n_a, row r - n_a of rows_b otherwise.
 * Bank (HMMR_F32 only, every other dtype is refused): plain [cout_pad][K] fp32 rows, the bias in `shift`, no `scale`, padding zero:
 *     conv1.w [32][16] (K = 9, columns 9..15 zero)   conv2.w [32][32]   heads.w [32][32] (row j = wj[j], rows 23..31 zero; shift = bj)
 *     fc1.w [1024][1024]: K = 736 is not a size hmmr_conv_gemm takes (a power of two), so its rows are padded with zeros to 1024
 *     fc2.w [1024][1024]   fc_out.w [128][1024] (row 0 = fo, shift[0] = bo)
 * Every `shift` is padded with zeros to a multiple of 128 floats.  Gradients have the bank's own layouts (padding written as
 * zeros), so an optimiser step is elementwise.
 * Contract:
 *  - Nothing is kept between calls.  The backward recomputes the forward into its workspace by the routine hmmr_disc_pose_fwd
 *    runs: h2 [n][1024] (736 used: fc1's input and the gate), h3, h4.  h1 is NOT kept: the front backward recomputes it from x.
 *  - fc1 / fc2 / fc_out run through hmmr_conv_gemm with a fixed split-K of 4; the data gradients contract over the rows of the
 *    untransposed bank in 8 fixed slices, the weight gradients over the batch rows in 4; bias gradients and the front's six
 *    gradients are summed in double (per tile of 4 rows in row order, then the tiles in tile order) and rounded once.
 *    No floating-point atomics: equal inputs give equal bytes, and a row's out / d_poses does not depend on the other rows.
 *  - A NULL output is skipped and its launches are not queued; at least one output is required.
 *  - Refused with -1 before anything is queued: null required pointers; a negative count or n_a + n_b <= 0; ld < 207 (of a
 *    non-empty segment, of a wanted d_poses); a bank that is not HMMR_F32 or has a missing / scaled layer; a workspace that is
 *    too small; no output asked for; in hmmr_pose_prior an empty fake segment when d_rs_fake or losses is wanted.
 * ------------------------------------------------------------------------- */
typedef struct { const float* ptr; int64_t ld; int n; } hmmr_rows_t;

typedef struct {
    int dtype;
    hmmr_layer_t conv1, conv2, heads, fc1, fc2, fc_out;
} hmmr_disc_pose_weights_t;

typedef struct {                       /* the twelve gradients in the layouts of the bank itself; each may be NULL */
    float* d_conv1;  float* d_bc1;     /* [32][16], [32] */
    float* d_conv2;  float* d_bc2;     /* [32][32], [32] */
    float* d_heads;  float* d_bj;      /* [32][32], [32] (rows / entries >= 23 written as zeros) */
    float* d_fc1;    float* d_b1;      /* [1024][1024] (columns >= 736 written as zeros), [1024] */
    float* d_fc2;    float* d_b2;      /* [1024][1024], [1024] */
    float* d_fc_out; float* d_bo;      /* [128][1024], [128] (rows / entries >= 1 written as zeros) */
} hmmr_disc_pose_grads_t;

typedef struct {
    hmmr_rows_t rows_a, rows_b;        /* the forward's inputs */
    const float* d_out;                /* [n_a + n_b][24] */
    float* d_poses_a; int64_t ld_a;    /* 207 values per row written at row stride ld, nothing else touched; or NULL */
    float* d_poses_b; int64_t ld_b;
    hmmr_disc_pose_grads_t grads;
} hmmr_disc_pose_bwd_desc_t;

typedef struct {
    hmmr_rows_t real, fake;
    float w_e, w_d;
    float* losses;                     /* [3] = e_pose, d_real, d_fake: sums in double, in row order, rounded once; or NULL.  The loss
                                          of an empty segment is 0 */
    float* d_rs_fake;                  /* [n_fake][216] or NULL: nine zeros, then w_e * d e_pose / d x -- what hmmr_smpl_bwd reads as d_rs */
    hmmr_disc_pose_grads_t grads;      /* the gradients of w_d * d_pose */
} hmmr_pose_prior_desc_t;

/* One layout for the three entry points below; 0 for n <= 0. */
size_t hmmr_disc_pose_workspace_bytes(int n);
/* out [n_a + n_b][24] */
int hmmr_disc_pose_fwd(const hmmr_disc_pose_weights_t* w, const hmmr_rows_t* rows_a, const hmmr_rows_t* rows_b, float* out,
                       void* ws, size_t ws_bytes, void* stream);
int hmmr_disc_pose_bwd(const hmmr_disc_pose_weights_t* w, const hmmr_disc_pose_bwd_desc_t* desc, void* ws, size_t ws_bytes, void* stream);
/* The closed loop of one step on ONE recomputed forward: the losses, and the only two gradients a step needs -- the encoder's
 * (e_opt differentiates e_loss with respect to encoder variables only) and the discriminator's (d_opt: D_var only).  With
 * s_e = (float)(2 w_e / n_fake), s_f = (float)(2 w_d / n_fake), s_r = (float)(2 w_d / n_real), the cotangents are
 * s_e * (out - 1) on the fake rows, and s_r * (out - 1) on the real and s_f * out on the fake rows; each result is byte for
 * byte what hmmr_disc_pose_fwd and two hmmr_disc_pose_bwd calls with those cotangents give.  Workspace:
 * hmmr_disc_pose_workspace_bytes(n_real + n_fake).  Built for the rows of a training step (hundreds to a few thousand): the losses
 * and the two cotangents come from ONE workgroup, whose last step adds the row sums one after the other -- the price of the row
 * order.  Every count the checks admit (n_real + n_fake < 2^21) is computed correctly, but beyond some ten thousand rows that
 * launch is a serial tail of milliseconds. */
int hmmr_pose_prior(const hmmr_disc_pose_weights_t* w, const hmmr_pose_prior_desc_t* desc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * SMPL forward + keypoint projection: SMPL.__call__ (src/tf_smpl/batch_smpl.py:
 * 89-162), batch_rodrigues / batch_global_rigid_transformation
 * (src/tf_smpl/batch_lbs.py:42-60, 133-194), batch_orth_proj_idrot
 * (src/tf_smpl/projection.py:16-29), as driven by OmegasPred.compute_smpl
 * (src/omega.py:263-304).
 * ------------------------------------------------------------------------- */
typedef struct {
    int num_verts;                     /* 6890 */
    int num_kps;                       /* 25 (cocoplus) or 14 (lsp) */
    int lbs_nnz;                       /* ELL width of the skinning weights (<= 24) */
    int vpad;                          /* row stride of `dirs` in floats: a multiple of 128, >= num_verts */
    const float* dirs;                 /* [224][3][vpad] planar re-pack of the tf_smpl bases (rows >= 218 zero):
                                          row 0 v_template,
                                          1..10 shapedirs, 11..217 posedirs; dirs[k][c][v] =
                                          basis[k][3*v + c] (src/tf_smpl/batch_smpl.py:45-63) */
    const float* j_template;           /* [24*3]      J_regressor^T v_template            */
    const float* j_shapedirs;          /* [10][24*3]  J_regressor^T shapedirs (folded)    */
    const int32_t* parents;            /* [24], parents[0] ignored                         */
    const int32_t* lbs_idx;            /* [num_verts][lbs_nnz] joint ids                  */
    const float* lbs_w;                /* [num_verts][lbs_nnz] weights (0 for padding)    */
    const int32_t* kreg_ptr;           /* CSR by keypoint of cocoplus_regressor^T: [num_kps+1] */
    const int32_t* kreg_idx;           /* vertex ids   */
    const float* kreg_val;
    const void* dirs_split;            /* optional (NULL: the blend product runs on the vector units in fp32): `dirs` x 2^13 as fp16 hi/lo
                                          MFMA B-operand fragments, [224 / 16][3][2 (hi, lo)][2 (k half)][vpad][8 halves]:
                                          dirs_split[kc][c][plane][h][v][e] = plane(2^13 * dirs[16 kc + 8 h + e][c][v]), hi = fp16(x),
                                          lo = fp16(x - hi) (packing.pack_smpl).  With it the blend shapes are a split-fp16 MFMA
                                          product (three v_mfma_f32_32x32x16_f16 per operand pair, fp32 accumulate: 22 operand bits) */
} hmmr_smpl_consts_t;

size_t hmmr_smpl_workspace_bytes(int m);
/* theta: m rows of 72 floats with row stride ld_theta; beta: m rows of 10 floats
 * (stride ld_beta); cams: m rows of 3 floats (stride ld_cam) or NULL (no kps).
 * verts [m,V,3], joints [m,K,3], kps [m,K,2] (NULL ok), rs [m,24,3,3] (NULL ok). */
int hmmr_smpl_fwd(const hmmr_smpl_consts_t* c, const float* theta, int ld_theta,
                  const float* beta, int ld_beta, const float* cams, int ld_cam, int m,
                  float* verts, float* joints, float* kps, float* rs,
                  void* ws, size_t ws_bytes, void* stream);
/* Same, but instance i's outputs start at verts + i*ld_out, joints + i*ld_out, ... (floats):
 * the four outputs are fields of one packed per-frame record of ld_out floats, so the
 * record that the multi-GPU all-gather ships is written in place (no re-packing pass). */
int hmmr_smpl_fwd_strided(const hmmr_smpl_consts_t* c, const float* theta, int ld_theta,
                          const float* beta, int ld_beta, const float* cams, int ld_cam, int m,
                          float* verts, float* joints, float* kps, float* rs, int64_t ld_out,
                          void* ws, size_t ws_bytes, void* stream);
/* The tail of build_test_model for ALL containers at once (tester.py:196-227: OmegasPred.compute_all_smpl over the present
 * container and the delta containers + make_fetch_dict): omegas [num_containers][n][85] fp32 (container 0 = present, as
 * hmmr_ief_fwd writes them) -> every field of frame i's packed record rec[i * ld_rec ...]: container r's cams [3], joints
 * [K,3], kps [K,2], poses [24,3,3], shapes [10], verts [V,3] and raw omega [85] at float offset
 * field_offsets[r * 7 + {0..6}] (HOST array, that field order).  Every container is projected with container 0's camera
 * (tester.py:211-213), and `cams` holds that camera.  One launch set (three kernels) whatever num_containers is;
 * workspace = hmmr_smpl_workspace_bytes(num_containers * n). */
int hmmr_smpl_fwd_records(const hmmr_smpl_consts_t* c, const float* omegas, int num_containers, int n,
                          float* rec, int64_t ld_rec, const int32_t* field_offsets, void* ws, size_t ws_bytes,
                          void* stream);
/* batch_global_rigid_transformation on its own (src/tf_smpl/batch_lbs.py:133-194):
 * Rs [m,24,3,3], Js [m,24,3], parents [24] -> new_J [m,24,3], A [m,24,4,4] (relative transforms for LBS).
 * rotate_base != 0: the root rotation is R_0 . diag(1, -1, -1) (batch_lbs.py:151-158; the hot path passes 0). */
int hmmr_global_rigid_transformation(const float* Rs, const float* Js, const int32_t* parents, int m,
                                     float* new_j, float* A, int rotate_base, void* stream);

/* ------------------------------------------------------------------------- *
 * SMPL backward (additive to ABI 19): the derivative of hmmr_smpl_fwd -- SMPL.__call__ (src/tf_smpl/batch_smpl.py:89-162),
 * batch_rodrigues / batch_global_rigid_transformation (src/tf_smpl/batch_lbs.py:42-60, 133-194) and batch_orth_proj_idrot
 * (src/tf_smpl/projection.py:16-29) -- with respect to theta, beta and the camera; what a trainer's losses on kps, joints,
 * poses and verts need (csrc/smpl_grad.hip).
 *
 * The function differentiated is the forward in exact fp32: R = cos I + (1 - cos) r r^T + sin skew(r) with angle = ||theta + 1e-8||
 * and r = theta / angle (not a unit vector; both carry a derivative), J = j_template + beta . j_shapedirs, FK in index order,
 * A = [G_R | G_t - G_R J], v_posed = dirs^T [1, beta, R_1..23 - I], verts = sum_j w[v,j] A_j [v_posed; 1], joints = kreg^T verts,
 * kps = s (joints_xy + t), Rs = R.  A forward that ran its blend product on split-fp16 operands (the default) is differentiated as
 * this exact function.  Every intermediate is recomputed from theta and beta; `joints` (the forward's output) is read for the
 * camera gradient only.  No floating-point atomics: per-tile partials, summed in tile order -- the same inputs give the same bytes.
 * ------------------------------------------------------------------------- */
typedef struct {
    int num_verts;                     /* as in the hmmr_smpl_consts_t it goes with */
    int num_kps;
    const int32_t* vk_ptr;             /* CSR BY VERTEX of cocoplus_regressor (the first 14 columns for lsp): [num_verts+1] */
    const int32_t* vk_idx;             /* keypoint ids, ascending per vertex */
    const float* vk_val;
} hmmr_smpl_grad_consts_t;

size_t hmmr_smpl_bwd_workspace_bytes(const hmmr_smpl_consts_t* c, int m);   /* 0 for m <= 0 or c == NULL */
/* theta, beta, cams: the forward's inputs with the forward's row strides (cams NULL: no camera); joints [m,K,3]: the forward's
 * output, needed iff d_kps.  Upstream gradients d_verts [m,V,3], d_joints [m,K,3], d_kps [m,K,2], d_rs [m,24,3,3]: any of them
 * may be NULL (= zero, never read), at least one must be given.  Outputs d_theta [m,72], d_beta [m,10], d_cams [m,3] or NULL
 * (zeros when d_kps is NULL).  Refused before any launch, with a message in hmmr_last_error: a null c, g, theta, beta, d_theta,
 * d_beta or ws; m <= 0; no upstream gradient; d_kps without cams or joints; d_cams without cams; lbs_nnz outside 1..24; a
 * workspace below hmmr_smpl_bwd_workspace_bytes(c, m). */
int hmmr_smpl_bwd(const hmmr_smpl_consts_t* c, const hmmr_smpl_grad_consts_t* g,
                  const float* theta, int ld_theta, const float* beta, int ld_beta,
                  const float* cams, int ld_cam, const float* joints, int m,
                  const float* d_verts, const float* d_joints, const float* d_kps, const float* d_rs,
                  float* d_theta, float* d_beta, float* d_cams,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Trainer losses (additive to ABI 19): the encoder losses of the sequence trainer on precomputed phis
 * (src/trainer_sequence_fc.py: compute_losses_batched :791-846, compute_losses_deltas :848-953, the shape prior of
 * compute_losses_prior), built from src/ops.py (compute_loss_e_kp, compute_loss_e_kp_optcam, compute_loss_e_3d,
 * compute_loss_mse, compute_loss_e_smooth, compute_loss_shape, align_by_pelvis) and src/tf_smpl/projection.py
 * (batch_orth_proj_optcam, procrustes2d_vis) -- every loss value AND the gradient of total = sum_i weights[i] L_i with respect
 * to what hmmr_smpl_fwd returned, in the layouts hmmr_smpl_bwd reads (csrc/losses.hip).
 *
 * Rows are sequence-major: row n = b T + t, N = B T.
 *
 * Frame slices (compute_losses_deltas :867-884).  delta_t = 0: every frame.  delta_t > 0: pred frames [0, T - delta_t) of each
 * sequence against gt frames [delta_t, T).  delta_t < 0: pred frames [|delta_t|, T) against gt frames [0, T - |delta_t|).  The
 * slices apply to the kp, joints and smpl terms; e_const and e_shape always see all N rows.  A pred row outside the slice gets
 * ZERO cotangents from the sliced terms (written, not left).
 *
 * e_kp (compute_loss_e_kp; tf.losses.absolute_difference, SUM_BY_NONZERO_WEIGHTS with its safe division):
 *   sum_i vis_i (|x_gt - x_pred| + |y_gt - y_pred|) / P over the slice, P = the non-zero elements of the broadcast weight
 *   = 2 #{vis != 0}; 0 when P = 0.  vis is a weight as given, not binarised.  d_kps = w vis sign(pred - gt) / P, sign(0) = 0.
 * KP_OPTCAM (compute_loss_e_kp_optcam, batch_orth_proj_optcam, procrustes2d_vis), per frame: v = (kps_gt_z > 0); masked means
 *   mu1 (pred), mu2 (gt); xmu = v (x - mu1), y = v (x_gt - mu2); A = xmu^T xmu + 1e-6 I; scale = trace(A^-1 xmu^T y) / 2 clipped
 *   to [0.7, 10]; trans = mu2 / scale - mu1; the loss is e_kp on scale (x + trans).  The camera carries NO gradient
 *   (stop_gradient): d_kps = scale x (that cotangent).  The 2x2 inverse is closed form; every sum runs in fp64 on the fp32 inputs
 *   and is rounded once.  A frame of the slice without a visible keypoint has no finite answer in the reference (0 / 0) and none
 *   here: the loss is not finite and HMMR_LOSS_NO_VISIBLE is set in `status`.
 * e_joints, e_smpl_pose, e_smpl_shape (compute_loss_e_3d, compute_loss_mse, align_by_pelvis): joints = the first 14 predicted
 *   joints and the 14 gt joints, each minus the midpoint of joints 3 and 2;  0.5 sum_rows w_row sum (a - b)^2 / (D #{w_row != 0}),
 *   D = 42 (joints), 216 (rotations, the global one included), 10 (shape), w_row = has_gt3d_joints[b] / has_gt3d_smpl[b] (tf_repeat
 *   over the slice's frames); 0 when no row has a non-zero weight.  The joint cotangent goes back through the alignment (joints 2
 *   and 3 receive -0.5 sum_k g_k as well); rows 14 .. K-1 of d_joints are zero.
 * e_const (compute_loss_e_smooth on betas[:, :-1], betas[:, 1:]): 0.5 mean over B (T - 1) 10 values; 0 without gradient for T = 1.
 * e_shape (compute_loss_shape): mean(beta^2) over the N 10 values.
 *
 * Reduction order (no floating-point atomic; the same inputs give the same bytes): every per-frame sum in element order inside
 * one thread, in fp64; the frames of a sequence in frame order; the sequences in sequence order; one rounding to fp32 per loss.
 * The normalisers (P and the row counts) are functions of the ground truth alone.
 * d_beta = ((e_smpl_shape term + e_const term) + e_shape term), formed in fp64 and rounded once.
 * ------------------------------------------------------------------------- */
enum { HMMR_LOSS_KP = 1, HMMR_LOSS_KP_OPTCAM = 2, HMMR_LOSS_JOINTS = 4, HMMR_LOSS_SMPL = 8, HMMR_LOSS_CONST = 16,
       HMMR_LOSS_SHAPE_PRIOR = 32 };
/* slots of `losses` and of `weights` */
enum { HMMR_L_KP = 0, HMMR_L_JOINTS = 1, HMMR_L_SMPL_POSE = 2, HMMR_L_SMPL_SHAPE = 3, HMMR_L_CONST = 4, HMMR_L_SHAPE = 5,
       HMMR_L_TOTAL = 6 };
enum { HMMR_W_KP = 0, HMMR_W_JOINTS = 1, HMMR_W_SMPL = 2, HMMR_W_CONST = 3, HMMR_W_SHAPE = 4 };
#define HMMR_LOSS_NO_VISIBLE 1u      /* status: a frame of the slice had no keypoint with z > 0 under KP_OPTCAM */
#define HMMR_LOSS_NOT_FINITE 2u      /* status: `total` is not finite */
typedef struct {
    int B, T, K;                       /* sequences, frames per sequence, keypoints of the forward */
    int delta_t;                       /* |delta_t| < T */
    unsigned flags;                    /* HMMR_LOSS_*; KP and KP_OPTCAM exclude each other; SMPL = pose + shape */
    float weights[6];                  /* HMMR_W_*: the trainer's loss_weights of e_kp, e_joints, e_smpl (pose and shape share it),
                                          e_const, e_shape; [5] is not read.  The cotangents are those of total = sum w_i L_i */
    /* predictions: the forward's outputs, N rows */
    const float* kps_pred;             /* [N,K,2]; under KP_OPTCAM joints[..., :2] (OmegasPred.compute_smpl with cams [1,0,0]) */
    const float* joints_pred;          /* [N,K,3] */
    const float* rs_pred;              /* [N,24,3,3] */
    const float* beta_pred;            /* N rows of 10 with row stride ld_beta */
    int ld_beta;
    /* ground truth; whatever no set flag needs may be NULL and is never read */
    const float* kps_gt;               /* [N,K,3] (x, y, vis): KP, KP_OPTCAM */
    const float* joints_gt;            /* [N,14,3]: JOINTS */
    const float* rs_gt;                /* [N,24,3,3]: SMPL */
    const float* shapes_gt;            /* [B,10] (OmegasGt.get_shapes tiles it over T): SMPL */
    const float* has_gt3d_smpl;        /* [B] fp32: SMPL */
    const float* has_gt3d_joints;      /* [B] fp32: JOINTS */
    /* outputs */
    float* losses;                     /* [8], HMMR_L_*; [7] = 0; a cleared flag's loss is 0 */
    float* d_kps;                      /* [N,K,2]   any of the four may be NULL: that term's backward is not wanted.  A given one */
    float* d_joints;                   /* [N,K,3]   is written in full -- zeros where no set flag reaches it */
    float* d_rs;                       /* [N,24,3,3] */
    float* d_beta;                     /* [N,10]: the DIRECT shape gradient (e_smpl_shape, e_const, e_shape), to be added to
                                          hmmr_smpl_bwd's d_beta */
    float* best_cam;                   /* [N,3] or NULL: (scale, tx, ty) of the slice's pred rows under KP_OPTCAM; other rows, and
                                          every row without KP_OPTCAM, are left untouched */
    unsigned* status;                  /* one device word or NULL, WRITTEN by the call (not sticky): HMMR_LOSS_NO_VISIBLE / _NOT_FINITE */
    void* ws;                          /* hmmr_seq_losses_workspace_bytes(B, T) */
    size_t ws_bytes;
} hmmr_seq_loss_desc_t;

size_t hmmr_seq_losses_workspace_bytes(int B, int T);     /* 0 for B <= 0 or T <= 0 */
/* Three launches whatever the flags: per-frame partial sums, the sums in order + the normalisers, the cotangents.  Refused
 * before any launch (-1, message in hmmr_last_error): a null descriptor; B, T or K <= 0; B T > 2^24; K < 14 with
 * JOINTS; |delta_t| >= T; KP and KP_OPTCAM together; unknown flag bits; a set flag with a NULL operand (KP / KP_OPTCAM: kps_pred,
 * kps_gt; JOINTS: joints_pred, joints_gt, has_gt3d_joints; SMPL: rs_pred, rs_gt, beta_pred, shapes_gt, has_gt3d_smpl; CONST /
 * SHAPE_PRIOR: beta_pred); a NULL losses; ld_beta < 10 with beta_pred; a workspace that is NULL or too small. */
int hmmr_seq_losses(const hmmr_seq_loss_desc_t* d, void* stream);

/* The closed loop omega [B T, 85] -> losses [8], d_omega [B T, 85]: hmmr_smpl_fwd (theta = omega[:, 3:75], beta = omega[:, 75:85]
 * in place, ld 85), hmmr_seq_losses, hmmr_smpl_bwd (d_verts NULL) and one assembling launch, on one stream out of one workspace.
 * `gt_and_flags` gives B, T, K (= c->num_kps), delta_t, flags, weights, the ground truth, best_cam and status; its predictions,
 * its outputs and its workspace are not read.  use_optcam != 0: the forward runs with cams [1, 0, 0] (kps = joints_xy) and
 * d_omega[:, :3] = 0; otherwise omega[:, :3] are the cams and d_omega[:, :3] = d_cams.  d_omega[:, 3:75] = d_theta;
 * d_omega[:, 75:85] = d_beta of hmmr_smpl_bwd + d_beta of hmmr_seq_losses (one fp32 addition, in that order).  The result
 * equals the three separate calls byte for byte.  Workspace, in order (csrc/losses.hip: omega_layout): the forward's, the
 * backward's and the loss stage's workspaces, cams, verts, joints, kps, Rs, d_kps, d_joints, d_rs, d_beta (direct), d_theta,
 * d_beta (SMPL), d_cams.  Refused before any launch: a null c, g, omega, losses or d_omega; every refusal of hmmr_seq_losses that
 * concerns shape, flags, delta_t and the ground truth; K != c->num_kps; and what hmmr_smpl_fwd / hmmr_smpl_bwd refuse of the
 * constants (lbs_nnz outside 1..24, grad constants of another model, vpad / dirs alignment); a workspace that is NULL or too small. */
size_t hmmr_omega_loss_grad_workspace_bytes(const hmmr_smpl_consts_t* c, int B, int T);     /* 0 for c == NULL, B <= 0 or T <= 0 */
int hmmr_omega_loss_grad(const hmmr_smpl_consts_t* c, const hmmr_smpl_grad_consts_t* g, const hmmr_seq_loss_desc_t* gt_and_flags,
                         const float* omega, int use_optcam, float* losses, float* d_omega,
                         void* ws, size_t ws_bytes, void* stream);

/* e_hallucinate (additive to ABI 19; csrc/losses.hip): tf.losses.mean_squared_error(movie_strip, pred_movie_strip) with its default
 * weight 1 (src/trainer_sequence_fc.py; SUM_BY_NONZERO_WEIGHTS over a scalar weight divides by the element count) -- there is no
 * stop-gradient, so the loss reaches both of its arguments.  a and b are [rows][cols] with row strides lda, ldb (floats):
 *   loss = sum (a - b)^2 / N, N = rows cols;   d_a = weight 2 (a - b) / N;   d_b = -d_a.
 * Summation order (fp64 on the fp32 inputs, no atomic; the same inputs give the same bytes): per row, thread t of 256 sums the
 * elements t, t + 256, ... in index order and the 256 partials fold pairwise (t += t + 128, then 64, ... 1); then the rows in row
 * order; one division by N and one rounding to fp32 -- `loss` is one fp32 device value, as the slots of hmmr_seq_loss_desc_t.losses.
 * d_a = (float)(weight 2 / N x (a - b)) with the product in fp64; d_b is that fp32 value negated.  loss, d_a (row stride ld_da) and
 * d_b (ld_db) may each be NULL and are then never written; `weight` scales the cotangents only.  The workspace (rows doubles) is
 * needed with `loss` alone.  Refused before any launch: a null a or b; rows or cols <= 0; rows > 2^24; a row stride below cols;
 * all three outputs NULL; a weight that is not finite; with `loss`, a workspace that is NULL or too small. */
size_t hmmr_strip_mse_workspace_bytes(int rows);          /* 0 for rows <= 0 */
int hmmr_strip_mse(const float* a, long long lda, const float* b, long long ldb, int rows, int cols, float weight, float* loss,
                   float* d_a, long long ld_da, float* d_b, long long ld_db, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * TF Adam (additive to ABI 19; csrc/adam.hip): one step of tf.train.AdamOptimizer over a list of tensors, as the published
 * TF 1.x ApplyAdam kernel states it, operation by operation in float32 (this is NOT torch.optim.Adam: epsilon is added to sqrt(v)
 * before the bias correction is folded into the step size, and the beta powers are float32 values multiplied once per step):
 *   on the host:  alpha = lr * sqrtf(1 - beta2_power) / (1 - beta1_power)
 *   per element:  m += (g - m) * (1 - beta1);   v += (g * g - v) * (1 - beta2);   p -= (m * alpha) / (sqrtf(v) + eps)
 * with 1 - beta1 and 1 - beta2 formed once in float32.  beta1_power / beta2_power are beta^t of step t = 1, 2, ...: the caller owns
 * them and multiplies them by beta AFTER the step (AdamOptimizer._finish).  The file is compiled without contraction, the division
 * and the square root are the correctly rounded ones: the result is held to the bytes of a float32 NumPy restatement
 * (tests/adam_cases.py).  Agreement with a TensorFlow binary is unmeasured.
 *
 * segs: a HOST array of device pointers, each 4-byte aligned.  A segment with g == NULL or n == 0 is skipped and its p, m and v keep
 * their bytes (TF's treatment of a variable without a gradient).  One launch per 64 active segments, their descriptors as kernel
 * arguments; a segment whose four pointers are all 16-byte aligned moves 16 bytes per lane, any other 4.  No atomic: the same
 * inputs give the same bytes, and a value does not depend on how the tensors are cut into segments.  Segments must not overlap.
 * Refused before anything is queued (-1, message in hmmr_last_error): null h; n_segs < 0, or a null table with n_segs > 0; a
 * hyper-parameter that is not finite; a beta power outside (0, 1); n < 0 or n > 2^40; a NULL p, m or v with n > 0; a pointer of an
 * active segment that is not 4-byte aligned.
 * ------------------------------------------------------------------------- */
typedef struct { float* p; const float* g; float* m; float* v; long long n; } hmmr_adam_seg_t;
typedef struct { float lr, beta1, beta2, eps, beta1_power, beta2_power; } hmmr_adam_hyper_t;
int hmmr_adam_step(const hmmr_adam_seg_t* segs, int n_segs, const hmmr_adam_hyper_t* h, void* stream);

/* ------------------------------------------------------------------------- *
 * Crop before the path (process_image, src/evaluation/run_video.py:56-107; resize_img,
 * src/util/common.py:7-14): frames [n,h,w,3] uint8 -> out [n,224,224,3] fp32 in [-1,1].
 * geom [n][4] int32 = {scaled height, scaled width, u0, v0}: floor(h*scale), floor(w*scale) and the
 * scaled-image coordinates of crop pixel (0,0) (round(centre*factors) - 112, may be negative: the
 * edge padding).  The host mirror (evaluation/run_video.py) computes geom in float64.
 * ------------------------------------------------------------------------- */
int hmmr_crop_frames(const unsigned char* frames, const int32_t* geom, int n, int h, int w,
                     float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Tube augmentation in front of the feature extractor (csrc/tube.hip): the pixel side of
 * TubePreprocessor.preprocess_image (src/util/tube_augmentation.py:114-186; jitter_scale, pad_image_edge, rotate_img,
 * flip_image, rescale_image of src/util/data_utils.py) as one gather kernel.  images [n,h,w,3] on the device, float32 in
 * [0,1] (images_are_u8 == 0) or uint8 (!= 0: byte b is read as (float)((double)b / 255.0), a 256-entry table, so both
 * routes see the same values) -> out [n,S,S,3] float32 in [-1,1].  All operands are DEVICE memory, written by the host
 * mirror (util/tube_augmentation.py):
 *   geom [n][4] int32 = {newH, newW, x0, y0}: the size of the frame's scaled image and the scaled-image coordinates of crop
 *     pixel (0,0) (centre - S/2 after jitter and scaling; may be negative or beyond the image: the edge pad);
 *   flip [n] bytes: != 0 reverses the frame's columns;  rot [n][6] float32 or NULL: the output -> input transform.
 * Everything is float32 and evaluated exactly as written, left to right, without contraction:
 *   crop pixel (x, y): u = clamp(x0 + x, 0, newW - 1), v = clamp(y0 + y, 0, newH - 1) (the clamp is the edge pad); its value is
 *     the TF 1.8 ResizeBilinear sample (align_corners=False, no half-pixel offset) of the frame at (u, v).  Along an axis
 *     of source size src and scaled size dst: in = (float)i * ((float)src / (float)dst), lo = (int)in,
 *     hi = min(lo + 1, src - 1), lerp = in - lo.  top = tl + (tr - tl) * xlerp, bot = bl + (br - bl) * xlerp,
 *     value = top + (bot - top) * ylerp.
 *   rot != NULL (tf.contrib.image.rotate(..., 'BILINEAR'); chosen when the preprocessor has rotate_max != 0): output pixel
 *     (x, y) reads fx = a0 * x + a1 * y + a2, fy = b0 * x + b1 * y + b2 with the row [a0 a1 a2 b0 b1 b2] =
 *     [cos, -sin, xoff, sin, cos, yoff], xoff = ((S-1) - (cos (S-1) - sin (S-1))) / 2, yoff = ((S-1) - (sin (S-1) + cos (S-1))) / 2.
 *     xf = floor(fx), xc = xf + 1, likewise y; row_f = (xc - fx) v(yf, xf) + (fx - xf) v(yf, xc), row_c the same on yc,
 *     value = (yc - fy) row_f + (fy - yf) row_c.  A tap outside [0, S) reads 0.0; a tap inside is the crop pixel above.
 *   flip (tf.reverse(image, [1]), after the rotation): output column x takes column S - 1 - x.
 *   last: (value - 0.5f) * 2.0f.
 * These rules restate the published TF 1.8 kernels (resize_bilinear_op.cc, contrib/image/kernels/image_ops.h); their
 * agreement with a TensorFlow binary is unmeasured.  Nothing is allocated; bad arguments (null images / geom / flip / out,
 * n, h, w or S <= 0) are refused before any launch (-1, hmmr_last_error()).  A geom row that is not a size cannot make
 * the kernel read outside the frame (its taps are clamped), only produce meaningless pixels: the mirror refuses such rows.
 * ------------------------------------------------------------------------- */
int hmmr_tube_augment(const void* images, int images_are_u8, int n, int h, int w, const int32_t* geom,
                      const unsigned char* flip, const float* rot, int S, float* out, void* stream);

/* ------------------------------------------------------------------------- *
 * Track front end (csrc/track.hip): from a person track's 2D keypoints to the geom rows hmmr_crop_frames reads, without a
 * host step.  Replaces src/util/smooth_bbox.py (get_smooth_bbox_params :10-34, kp_to_bbox_param :37-61, get_all_bbox_params
 * :64-105, smooth_bbox_params :108-123) and the per-frame arithmetic of demo_video.predict_on_tracks :136-153 with
 * process_image (src/evaluation/run_video.py:56-107) and resize_img (src/util/common.py:7-14).  fp64 throughout.
 *
 * Tracks lie one after the other along the row axis: track t owns rows [offsets[t], offsets[t + 1]).  `offsets` is HOST memory
 * (n_tracks + 1 values, non-decreasing, offsets[0] >= 0, at most HMMR_TRACK_MAX_ROWS rows); it is checked and then handed to
 * the kernels by value.  gauss_w is HOST memory too: the 2 radius + 1 weights of scipy.ndimage.gaussian_filter1d
 * (exp(-x^2 / 2 sigma^2) normalised to sum 1, radius = int(4 sigma + 0.5)), computed once by the caller; the filter is taken as
 * symmetric, so gauss_w[0 .. radius] is what is read.  Everything else is device memory.  Nothing is allocated, nothing waits for
 * the device, no atomics: the same bits every run.  Bad arguments are refused before any launch (-1, hmmr_last_error()).
 *
 * hmmr_track_bbox
 *   kps [N][k][3] = (x, y, score), 1 <= k <= HMMR_TRACK_MAX_KPS; present [N]: 0 = the reference's None.
 *   A row is valid if it is present, a score is strictly greater than vis_thresh and person_height = |max_pt - min_pt| over
 *   the visible keypoints is >= 0.5; then box = [(min_pt + max_pt) / 2, 150 / person_height].
 *   range [n_tracks][2] = {start, end} relative to the track's first row: the first valid row and one past the last one
 *   (-1, 0: no valid row).  Invalid rows between valid rows p < i < q get prev + (i - p) * ((curr - prev) / (q - p)), which is
 *   np.linspace's arithmetic; gaps of any length (the scan works in steps of HMMR_TRACK_TILE rows with a carry).
 *   bbox_raw [N][3] (may be NULL): the rows of get_all_bbox_params at start..end-1, zero elsewhere.
 *   bbox_smooth [N][3]: over rows [start, end) and per parameter scipy.signal.medfilt(x, kernel_size) -- the window is padded
 *   with ZEROS, kernel_size odd in [1, HMMR_TRACK_MAX_KERNEL] -- then the Gaussian with boundary mode 'reflect'
 *   (d c b a | a b c d | d c b a, repeated as often as the radius asks; radius <= HMMR_TRACK_MAX_RADIUS), summed in SciPy's
 *   order.  Neither filter reads a neighbouring track.  Rows outside [start, end) are zero.
 *   ws: hmmr_track_workspace_bytes(offsets[n_tracks], n_tracks) bytes (0: bad arguments).
 * hmmr_track_smooth: smooth_bbox_params alone, over all rows of every track of params [N][3] -> out [N][3].
 * hmmr_track_crop_geom
 *   for every row of [start, end) (range == NULL: every row) the integers of process_image for box bbox_smooth[row] on an
 *   h x w frame: geom [N][4] = {floor(h scale), floor(w scale), u0, v0} as hmmr_crop_frames reads them, with
 *   centre = round(c * factors) + 224 (x by the HEIGHT factor, y by the WIDTH factor, as the reference has it),
 *   start_pt = centre - 112, u0 / v0 = start_pt - 224; info [N][5] (may be NULL) = {start_pt x, y, centre - start_pt x, y,
 *   scale}.  A row whose box gives no full 224 x 224 crop gets a status [N] of HMMR_TRACK_* bits and the identity geometry
 *   {h, w, 0, 0}, which hmmr_crop_frames can execute; so do rows outside [start, end), with status 0.  A bad box is
 *   reported, never a fault, and hmmr_run_flags is not touched.
 * ------------------------------------------------------------------------- */
#define HMMR_TRACK_MAX_KPS 64
#define HMMR_TRACK_MAX_KERNEL 31
#define HMMR_TRACK_MAX_RADIUS 64
#define HMMR_TRACK_MAX_ROWS (1 << 27)
#define HMMR_TRACK_TILE 256           /* rows per step of the gap scan: no limit, only where tests look for seams */
enum { HMMR_TRACK_EMPTY = 1,          /* floor(h scale) or floor(w scale) < 1 */
       HMMR_TRACK_BEFORE_ORIGIN = 2,  /* start_pt < 0 */
       HMMR_TRACK_CLIPPED = 4,        /* the crop's end point lies beyond the padded image */
       HMMR_TRACK_NOT_FINITE = 8 };   /* NaN, infinity or a value no int32 holds */
size_t hmmr_track_workspace_bytes(int n_total, int n_tracks);
int hmmr_track_bbox(const double* kps, const unsigned char* present, const int32_t* offsets, int n_tracks, int k,
                    double vis_thresh, int kernel_size, const double* gauss_w, int gauss_radius, double* bbox_raw,
                    double* bbox_smooth, int32_t* range, void* ws, size_t ws_bytes, void* stream);
int hmmr_track_smooth(const double* params, const int32_t* offsets, int n_tracks, int kernel_size, const double* gauss_w,
                      int gauss_radius, double* out, void* ws, size_t ws_bytes, void* stream);
int hmmr_track_crop_geom(const double* bbox_smooth, const int32_t* offsets, const int32_t* range, int n_tracks, int h, int w,
                         int32_t* geom, double* info, int32_t* status, void* stream);

/* ------------------------------------------------------------------------- *
 * Hand-off to a rasteriser after the path (SURVEY f-3).  Replaces, for n frames in one launch, the
 * per-frame host code of src/util/render/nmr_renderer.py: the camera / keypoint change from the
 * 224x224 crop to the squared original image (visualize_img_orig :368-401) and the projection that
 * feeds nr.Renderer.render (VisRenderer.__call__ :139-144, torch_utils.py:11-29:
 * [s*(x+tx), -s*(y+ty), z]).  cams / verts / kps are read in place (row strides in floats, e.g.
 * straight out of the packed per-frame records of hmmr_smpl_fwd_strided).
 * geom [n][5] = {undo_scale, start_x, start_y, proc_size, img_size} per frame, or NULL to stay in
 * crop coordinates (visualize_img).  Outputs: new_cam [n][3] (may be NULL), proj_verts [n][nv][3],
 * kp_orig [n][nk][2] (may be NULL).
 * ------------------------------------------------------------------------- */
int hmmr_render_handoff(const float* cams, int64_t ld_cam, const float* verts, int64_t ld_verts,
                        const float* kps, int64_t ld_kps, const float* geom, int n, int nv, int nk,
                        float* new_cam, float* proj_verts, float* kp_orig, void* stream);

/* ------------------------------------------------------------------------- *
 * Rasteriser for the demo views (csrc/render.hip): what src/util/render/nmr_renderer.py's VisRenderer asks of
 * neural_renderer -- camera_mode='look_at', perspective=False, viewing angle 30 deg (eye at z = -2.7320508), near/far
 * 0.1/100, fill_back, 2x anti-aliasing -- for n frames of one mesh topology per call.
 *   projection   p = [s (x + tx), -s (y + ty), z] (VisRenderer.__call__), optionally after a rotation about the fp32
 *                vertex centroid (VisRenderer.rotated) and after the camera change to the original image (geom rows,
 *                as hmmr_render_handoff); depth z' = z + 2.7320508.
 *   coverage     subpixel (c, r) of the 2S x 2S grid, centre u = (2c+1-2S)/2S, v = (2r+1-2S)/2S, is covered by a face
 *                whose (p.x, -p.y) triangle contains (u, v) (edges included); depth 1 / sum(w_i / z'_i) in [0.1, 100];
 *                the nearest wins, ties go to the lower face index.  Non-finite and zero-area faces draw nothing.
 *   shading      tex (I_amb c_amb + I_dir c_dir max(0, n . d)), n = normalize(cross(p0-p1, p2-p1)) turned to n_z <= 0.
 *   output       2x2 mean of the subpixels (background colour where uncovered), uint8 clip(rgb, 0, 1) 255 composited
 *                over the background as trunc(img (1 - alpha) + rend alpha); alpha = covered subpixels / 4.
 * The output is the top-left out_h x out_w of the S x S raster (make_square / remove_pads).
 * ------------------------------------------------------------------------- */
#define HMMR_RENDER_MAX_FRAMES 4096
#define HMMR_RENDER_MIN_SIZE 16
#define HMMR_RENDER_MAX_SIZE 1024
#define HMMR_RENDER_MAX_FACES 65536
enum { HMMR_RENDER_BG_COLOR = 0,      /* the background colour */
       HMMR_RENDER_BG_FLOAT = 1,      /* float [n][S][S][3]: value = (img + bg_add) * bg_mul (fp32) */
       HMMR_RENDER_BG_FRAME = 2 };    /* uint8 [n][frame_h][frame_w][3] frame, bilinearly resized to out_h x out_w as
                                         cv2.resize does (visualize_img_orig): value = ((resized [-1,1] + 1) / 2) 255 */
typedef struct {
    const float* verts; int64_t ld_verts;     /* [n] rows of >= 3 nv floats (e.g. the verts field of packed records) */
    const float* cams; int64_t ld_cam;        /* [n] rows of >= 3 floats: s, tx, ty */
    const float* geom;                        /* NULL, or [n][5] {undo_scale, start_x, start_y, proc_size, img_size}:
                                                 move the cameras to the original image first (hmmr_render_handoff) */
    const int32_t* faces;                     /* [nf][3], indices in [0, nv): the caller's precondition */
    const float* face_colors;                 /* NULL: `color` for every face; else rgb [nf][3] per frame row */
    int64_t ld_face_colors;                   /* floats between frames' face_colors (0: one set for all frames) */
    int n, nv, nf, size;                      /* frames, vertices, faces, S (the square raster is S x S pixels) */
    int rotate;                               /* != 0: v <- rot (v - mean(v)) + mean(v) before projecting */
    float rot[9];                             /* row-major 3x3 */
    float color[3];                           /* mesh colour when face_colors == NULL */
    float bg_color[3];
    float light_dir[3];                       /* used as given (not normalised) */
    float light_int_ambient, light_int_directional;
    float light_color_ambient[3], light_color_directional[3];
    int bg_mode;                              /* HMMR_RENDER_BG_* */
    const void* bg_image;
    float bg_add, bg_mul;                     /* HMMR_RENDER_BG_FLOAT */
    int frame_h, frame_w;                     /* HMMR_RENDER_BG_FRAME */
    int out_h, out_w;                         /* <= size */
    unsigned char* rgb;                       /* [n][out_h][out_w][3] */
    float* alpha;                             /* NULL or [n][out_h][out_w] */
    int32_t* face_index;                      /* NULL or [n][2S][2S]: covering face, -1 where uncovered */
    void* ws; size_t ws_bytes;                /* hmmr_render_workspace_bytes(n, nv, nf) bytes, device memory */
} hmmr_render_desc_t;
/* Device workspace for a call on n frames of an (nv, nf) mesh, at any size and background mode (0: bad arguments). */
size_t hmmr_render_workspace_bytes(int n, int nv, int nf);
int hmmr_render_mesh(const hmmr_render_desc_t* d, void* stream);

/* ------------------------------------------------------------------------- *
 * Scene view (csrc/render.hip; additive to ABI 19): every tracked person of a video in one frame.  The reference has no
 * multi-person view (demo_video.py and run_video.py draw one track per video); the layering rule below is this project's.
 *   tracks       t = 0 .. n_tracks-1 share one topology (nv, nf, faces).  Track t covers frames [start_t, end_t) inside
 *                [0, n_frames); instance (t, f) exists iff start_t <= f < end_t and uses row f - start_t of the track's
 *                verts / cams / geom / priority, which are read in place (row strides, as hmmr_render_handoff).
 *   per instance camera change, projection, face planes, z', depth range, shading and tie rules are hmmr_render_mesh's
 *                (the same device code), with the track's colour and no rotation.
 *   order        the instances of a frame are visited by a key, descending; ties go to the lower track index; a
 *                non-finite key sorts last.  The key is priority[f - start_t] where the track gives one, else the fp32
 *                scale of the camera the projection uses (new_cam[0] after the geom change, cam[0] without geom): under
 *                the weak-perspective camera a larger projected person is the nearer one.
 *   subpixel     its owner is the FIRST instance in that order with any face covering it at depth in [0.1, 100]; its face
 *                is that instance's nearest face (ties: lower face index); its colour that face's shading in the owner's
 *                colour.  A later person never shows through an earlier one, whatever their z: the z of two people's
 *                SMPL frames is not comparable.
 *   pixel        2x2 mean with the background colour for uncovered subpixels, alpha = covered / 4, composited once as
 *                hmmr_render_mesh does, in the modes HMMR_RENDER_BG_COLOR and HMMR_RENDER_BG_FRAME.  A frame without an
 *                instance has alpha 0 everywhere and shows the resized frame (or the background colour).
 * With n_tracks = 1 the result equals hmmr_render_mesh on that track bit for bit in rgb, alpha and face_index.
 * The frames go in slabs of max(1, 64 / n_tracks) frames, so at most 64 instances are in the workspace at a time and
 * it does not grow with n_frames; the order is fixed and nothing passes between workgroups, so a frame renders the
 * same bits alone, in a batch, or beside other streams.
 * ------------------------------------------------------------------------- */
#define HMMR_SCENE_MAX_TRACKS 16
typedef struct {
    const float* verts; int64_t ld_verts;     /* [end - start] rows of >= 3 nv floats */
    const float* cams; int64_t ld_cam;        /* [end - start] rows of >= 3 floats: s, tx, ty */
    const float* geom;                        /* NULL, or [end - start][5] as hmmr_render_desc_t.geom */
    const float* priority;                    /* NULL (order by camera scale), or [end - start] fp32 keys on the device */
    int start, end;                           /* 0 <= start < end <= n_frames */
    float color[3];
} hmmr_scene_track_t;
typedef struct {
    const hmmr_scene_track_t* tracks;         /* HOST array of n_tracks entries; it travels to the kernels by value */
    int n_tracks;                             /* 1 .. HMMR_SCENE_MAX_TRACKS */
    const int32_t* faces;                     /* [nf][3], indices in [0, nv): the caller's precondition */
    int nv, nf, n_frames, size;               /* limits as hmmr_render_mesh's (n_frames as its n) */
    int out_h, out_w;                         /* <= size */
    float bg_color[3];
    float light_dir[3];                       /* used as given (not normalised) */
    float light_int_ambient, light_int_directional;
    float light_color_ambient[3], light_color_directional[3];
    int bg_mode;                              /* HMMR_RENDER_BG_COLOR or HMMR_RENDER_BG_FRAME */
    const void* bg_image;                     /* HMMR_RENDER_BG_FRAME: uint8 [n_frames][frame_h][frame_w][3] */
    int frame_h, frame_w;
    unsigned char* rgb;                       /* [n_frames][out_h][out_w][3] */
    float* alpha;                             /* NULL or [n_frames][out_h][out_w] */
    int32_t* face_index;                      /* NULL or [n_frames][2S][2S]: the owner's covering face, -1 where uncovered */
    int32_t* owner;                           /* NULL or [n_frames][2S][2S]: the owning track's index, -1 where uncovered */
    void* ws; size_t ws_bytes;                /* hmmr_render_scene_workspace_bytes(...) bytes, device memory */
} hmmr_scene_desc_t;
/* Device workspace for a call (0: bad arguments): that of one slab, the same for every n_frames >= max(1, 64 / n_tracks). */
size_t hmmr_render_scene_workspace_bytes(int n_frames, int n_tracks, int nv, int nf);
int hmmr_render_scene(const hmmr_scene_desc_t* d, void* stream);

/* ------------------------------------------------------------------------- *
 * The person-centred view (csrc/person_view.hip; additive to ABI 19): compute_video_bbox of
 * src/util/render/nmr_renderer.py (:519-634) for any number of person tracks in one call -- the one box that holds a person
 * over the whole track, and every frame's camera re-expressed relative to that box, ready for hmmr_render_mesh at size S
 * (visualize_mesh_og's crop branch, :440-464).
 *
 * cams [N][>= 3] and kps [N][>= 2k] (k (x, y) pairs in the [-1, 1] coordinates of the crop) are fp32 rows read in place
 * (ld_cam / ld_kps floats apart, e.g. inside the packed per-frame records); proc [N][3] = {scale, start_x, start_y} of
 * process_image in fp64; proc_size = im_shape[0].  Track t owns rows [offsets[t], offsets[t + 1]); `offsets` is HOST memory,
 * as for the track front end, and goes to the kernel by value.  One workgroup per track, no atomics, no workspace, nothing
 * allocated or waited for: the same bits every run, and a track's result does not depend on its neighbours.
 *
 * fp64 on the fp32 inputs, every operation rounded by itself (no contraction), in the reference's order.  Per frame:
 *   undo = 1 / scale;   p = ((kp + 1) * 0.5) * proc_size;   q = ((p + start) - proc_size) * undo
 *   ymin = max(0, min_k q.y - margin)   ymax = min(img_h - 1, max_k q.y + margin)   xmin, xmax likewise with img_w
 * per track: bbox = {min ymin, max ymax, min xmin, max xmax} over its frames, each cast to int32 toward zero (astype(np.int));
 *   off = (xmin, ymin);   S = max(ymax - ymin, xmax - xmin)
 * per frame again:
 *   start' = start - off * scale
 *   c0 = (proc_size * cam[0]) * 0.5;   c12 = cam[1:] + (2 / cam[0]) * 0.5
 *   o0 = c0 * undo;                    o12 = c12 + (start' - proc_size) / c0
 *   cams_crop = {o0 * (2 / S), o12 - 1 / ((2 / S) * o0)}, rounded once to fp32.
 * status [n_tracks]: HMMR_BBOX_* bits.  A status is a result, never a fault; hmmr_run_flags is not touched.
 *   EMPTY         the track has no frame: bbox = {0, 0, 0, 0}, nothing is written to cams_crop.
 *   NOT_FINITE    an input of the track (cams, kps, proc) or a frame's extreme is NaN / infinite, or an extreme of the track
 *                 does not fit an int32: bbox = 0 and the track's cameras are NaN (this project's rule: the reference has
 *                 no defined answer).
 *   DEGENERATE    S <= 0: the cameras are what the arithmetic above gives (division by zero included).
 *   BEYOND_START  sqrt(start . start) < sqrt(off . off) for some frame: where the reference prints 'crop is more than start
 *                 pt..?' and stops in a debugger (:613-615).  Ordinary footage meets it; the results are those the
 *                 reference computes when it is continued.
 * Refused before any launch (-1, hmmr_last_error()): a null pointer, k outside [1, HMMR_TRACK_MAX_KPS], ld_kps < 2k,
 * ld_cam < 3, n_tracks < 1, offsets that decrease, start below 0 or end beyond HMMR_TRACK_MAX_ROWS, img_h or img_w < 1,
 * proc_size <= 0 (or NaN), a margin that is not finite.
 * ------------------------------------------------------------------------- */
enum { HMMR_BBOX_EMPTY = 1, HMMR_BBOX_NOT_FINITE = 2, HMMR_BBOX_DEGENERATE = 4, HMMR_BBOX_BEYOND_START = 8 };
int hmmr_video_bbox(const float* cams, long long ld_cam, const float* kps, long long ld_kps, int k, const double* proc,
                    double proc_size, const int32_t* offsets, int n_tracks, int img_h, int img_w, double margin,
                    int32_t* bbox, float* cams_crop, int32_t* status, void* stream);

/* ------------------------------------------------------------------------- *
 * The skeleton panel and the 2x2 collage of the demo (csrc/collage.hip; additive to ABI 19).
 *
 * hmmr_draw_skeleton replaces draw_skeleton (src/util/render/render_utils.py:38-234) as visualize_img calls it
 * (src/util/render/nmr_renderer.py:303-316), for n frames per launch.  The DRAW LIST is the reference's: per child, in
 * index order, a white disc of radius r, the child's disc of radius r - 1, the parent's disc of radius r - 1 and a line of
 * thickness r - 2 in the edge colour; an invisible child is skipped, an invisible parent suppresses its disc and the line;
 * draw_edges = 0 draws a 1-pixel ring of radius r - 1 per visible joint and nothing else; parents and colours for 19 and
 * 25 joints.  The PIXELS of a primitive are specified here, in exact integer arithmetic (centres and end points are
 * integers, dx, dy run from the pixel to the centre), because OpenCV's scan conversion could not be recorded:
 *   disc(c, r)       dx dx + dy dy <= r r + r
 *   ring(c, r)       disc(c, r) minus disc(c, r - 1)
 *   line(p0, p1, t)  4 dist^2(q, segment) <= t t: with d = p1 - p0, L = d.d, s = clamp((q - p0).d, 0, L),
 *                    4 |(q - p0) L - s d|^2 <= t t L L; for L = 0, 4 |q - p0|^2 <= t t (a capsule with round caps)
 * Agreement with cv2.circle / cv2.line at the boundary pixels of a primitive has NOT been measured.
 *   joints      (kp + kp_add) * kp_mul in fp32 (kp_add = 1, kp_mul = img_size / 2: the bits of ((kp + 1) * 0.5) * img_size),
 *               rounded half to even, then clamped to [-32768, 32767] (a deviation: the reference keeps any integer);
 *               a joint with a NaN coordinate counts as invisible.
 *   radius      0: max(4, int(mean(h, w) * 0.01)) (hmmr_skeleton_radius); with draw_edges, a radius < 3 is refused (the line's
 *               thickness would be < 1, where OpenCV asserts).
 *   background  bg_float [n][h][w][3]: trunc(clamp((img + bg_add) * bg_mul, 0, 255)) where no primitive covers the pixel (the
 *               astype(uint8) of a float image), or bg_u8 [n][h][w][3], which may be `out` itself (drawn in place).
 * ------------------------------------------------------------------------- */
#define HMMR_SKELETON_MAX_RADIUS 1024
typedef struct {
    const float* kps; int64_t ld_kps;         /* [n] rows of >= 2 nk floats: x0 y0 x1 y1 ... (e.g. the kps field of packed records) */
    const unsigned char* vis;                 /* NULL, or [n][nk]: 0 = invisible */
    int n, nk, h, w;                          /* frames, joints (19 or 25), image rows and columns (as hmmr_render_mesh's size) */
    float kp_add, kp_mul;
    int draw_edges;                           /* 0 or 1 */
    int radius;                               /* 0: the reference's rule */
    const float* bg_float; float bg_add, bg_mul;
    const unsigned char* bg_u8;               /* exactly one of bg_float / bg_u8 */
    unsigned char* out;                       /* [n][h][w][3] */
} hmmr_skeleton_desc_t;
int hmmr_skeleton_radius(int h, int w);       /* the reference's radius for an h x w image (0: bad arguments) */
int hmmr_draw_skeleton(const hmmr_skeleton_desc_t* d, void* stream);

/* hmmr_compose_collage replaces the tail of render_preds (src/evaluation/run_video.py:178-197) for n frames per launch:
 *     | rend_crop | render_og resized to (w', S) |        w' = w S / h (integer division)
 *     | skel_crop | rot_og resized to (S, S)     |        the narrower right panel padded with ones on its right
 * Panels are uint8; the reference's floats are restated: value / 255 (float32 for the skeleton panel), cv2.resize's
 * INTER_LINEAR as hmmr_img::taps has it (fp64, horizontal pass first), padding 1.0, and plt.imsave's trunc(x 255).
 * out [n][2 S][hmmr_collage_width(S, h, w)][3]. */
#define HMMR_COLLAGE_MAX_PANEL_WIDTH 4096
typedef struct {
    const unsigned char* rend_crop;           /* [n][S][S][3] */
    const unsigned char* skel_crop;           /* [n][S][S][3] */
    const unsigned char* render_og;           /* [n][h][w][3] */
    const unsigned char* rot_og;              /* [n][h][w][3] */
    int n, S, h, w;
    unsigned char* out;
} hmmr_collage_desc_t;
/* S + max(w', S); 0 for S outside hmmr_render_mesh's sizes, h or w outside [1, HMMR_RENDER_MAX_SIZE], or w' outside
 * [1, HMMR_COLLAGE_MAX_PANEL_WIDTH] */
int hmmr_collage_width(int S, int h, int w);
int hmmr_compose_collage(const hmmr_collage_desc_t* d, void* stream);

/* ------------------------------------------------------------------------- *
 * Evaluation metrics on device (src/evaluation/eval_util.py): per-frame MPJPE after pelvis alignment
 * and after Procrustes alignment (compute_error_3d :30-60 with align_by_pelvis :158 and
 * compute_similarity_transform :177), acceleration (compute_accel :14) and acceleration error
 * (compute_error_accel :63, before its visibility filter), vertex error (compute_error_verts :140).
 * gt / pred: [n, k, 3] fp32 (k <= 32); outputs [n] / [n-2] fp32; any output pointer may be NULL.
 * ------------------------------------------------------------------------- */
int hmmr_eval_joints(const float* gt, const float* pred, int n, int k, int left_id, int right_id,
                     float* mpjpe, float* pa_mpjpe, float* accel_pred, float* accel_err, void* stream);
/* err[i] = mean_v || gt[i, v] - pred[i, v] ||; row strides in floats (pred may be a field of the
 * packed per-frame record). */
int hmmr_eval_verts(const float* gt, int64_t ld_gt, const float* pred, int64_t ld_pred, int n, int nv,
                    float* err, void* stream);
/* hmmr_eval_joints with row strides in floats (>= 3 k): the first k joints of a wider row -- preds['joints'][:, :14] inside the
 * packed per-frame record -- are read in place.  Same device code; with ld = 3 k the same bits as hmmr_eval_joints. */
int hmmr_eval_joints_ld(const float* gt, int64_t ld_gt, const float* pred, int64_t ld_pred, int n, int k,
                        int left_id, int right_id, float* mpjpe, float* pa_mpjpe, float* accel_pred, float* accel_err,
                        void* stream);
/* compute_error_kp with compute_opt_cam_with_vis (eval_util.py:97-137, :235-260), one frame per lane, k <= 32.
 * kps_gt [n][k][3] = (x, y, vis) with row stride ld_gt >= 3 k, kps_pred [n][k][2] with row stride ld_pred >= 2 k (floats).
 * img_size > 0: the prediction is mapped to image space first, (x + 1) * 0.5 * img_size as three fp32 operations
 * (compute_errors_batched, eval.py:131, in float32); img_size <= 0: it is in pixels already.  vis = (gt[:, 2] != 0).
 * Outputs, each optional: err_kp / err_kp_pa / pck [n] and cam [n][3] = [scale, tx, ty].  Means over the visible keypoints;
 * the alignment keeps the reference's 1e-6 I regulariser and trace(.) / 2; pck = share of visible keypoints whose aligned
 * distance is strictly below alpha.  A frame without a visible keypoint, or with fewer than min_visible, gets NaN in every
 * output: a result, not an error (hmmr_run_flags is not touched). */
int hmmr_eval_kps(const float* kps_gt, int64_t ld_gt, const float* kps_pred, int64_t ld_pred, int n, int k,
                  double alpha, int min_visible, float img_size, float* err_kp, float* err_kp_pa, float* pck,
                  float* cam, void* stream);
/* rot_mat_to_axis_angle / axis_angle_to_rot_mat (eval_util.py:318-343) without OpenCV.  n rows of `per` rotations each:
 * rot rows hold `per` row-major 3x3 matrices (stride ld_rot >= 9 per floats; preds['poses'] inside the packed record), aa rows
 * `per` vectors (stride ld_aa >= 3 per).  The log map returns w with |w| <= pi and Rodrigues(w) = R, conditioned over the whole
 * range (atan2 of the antisymmetric norm and the trace; beyond a quarter turn the axis comes from the symmetric part, so nothing
 * is divided by sin near pi; at exactly pi either sign is right).  fp64 arithmetic on the fp32 input.  The exp map is the fp32
 * Rodrigues of the SMPL pose kernel (batch_rodrigues, src/tf_smpl/batch_lbs.py:42-60). */
int hmmr_rotmat_to_axis_angle(const float* rot, int64_t ld_rot, int n, int per, float* aa, int64_t ld_aa, void* stream);
int hmmr_axis_angle_to_rotmat(const float* aa, int64_t ld_aa, int n, int per, float* rot, int64_t ld_rot, void* stream);

/* ------------------------------------------------------------------------- *
 * Packers (ABI 18; csrc/pack.cpp): checkpoint variables by name -> the layouts and structs above, WITHOUT Python.
 *
 * The reference restores its graph from a TensorFlow checkpoint (src/evaluation/tester.py:92-116); the variable names and shapes are
 * SURVEY App. B's (resnet_v2_50/..., AZ_FC_block..., single_view_ief[_past5 | _future5]/3D_module/fc{1,2,3}, fc2_res/..., mean_param).  A caller
 * hands them over as fp32 host arrays in the checkpoint's own element order (conv filters HWIO, fully-connected [in][out]) and gets,
 * per stage, ONE blob in the device layout plus the stage's struct with every pointer already set to `device_base + offset`:
 *
 *     n = hmmr_pack_resnet_bytes(vars, n_vars, dtype);  hipMalloc(&dev, n);  host = malloc(n);
 *     hmmr_pack_resnet(vars, n_vars, dtype, host, n, dev, &weights);  hipMemcpy(dev, host, n, hipMemcpyHostToDevice);
 *     hmmr_resnet50_fwd(&weights, ...);
 *
 * No HIP call and no allocation in here; the functions are pure (same inputs -> same bytes) and return 0 or -1 with hmmr_last_error()
 * naming the variable that is missing or mis-sized.  They produce the SHIPPED configuration of every operand mode (f16x3: fused stem
 * with block1/unit_1's conv1, whole-unit kernels in block 1, unit pairs in blocks 2-3, the 3x3 / 1x1 filter streams, folded shortcuts;
 * bf16: fused units of blocks 1-2, 3x3 streams of blocks 3-4; f32: layer per launch) -- human_dynamics_amd/packing.py calls them for
 * exactly that and keeps Python forms only for its development switches, pinned to these bytes by tests/test_packers.py.
 * *_bytes(): the blob size for the same arguments (0 on error).
 * ------------------------------------------------------------------------- */
typedef struct {
    const char* name;      /* checkpoint variable name */
    const float* data;     /* fp32, host memory, the checkpoint's element order */
    int64_t numel;         /* number of values (the shape follows from the name; checked) */
} hmmr_var_t;

size_t hmmr_pack_resnet_bytes(const hmmr_var_t* vars, int n_vars, int dtype);
int hmmr_pack_resnet(const hmmr_var_t* vars, int n_vars, int dtype, void* host_blob, size_t blob_bytes, const void* device_base,
                     hmmr_resnet_weights_t* out);
size_t hmmr_pack_temporal_bytes(const hmmr_var_t* vars, int n_vars, int dtype, int num_blocks);
int hmmr_pack_temporal(const hmmr_var_t* vars, int n_vars, int dtype, int num_blocks, void* host_blob, size_t blob_bytes,
                       const void* device_base, hmmr_temporal_weights_t* out);
size_t hmmr_pack_hallucinator_bytes(const hmmr_var_t* vars, int n_vars, int dtype);
int hmmr_pack_hallucinator(const hmmr_var_t* vars, int n_vars, int dtype, void* host_blob, size_t blob_bytes, const void* device_base,
                           hmmr_hallucinator_weights_t* out);
/* delta_t: the delta regressors' offsets (config.delta_t_values, e.g. {-5, 5}): scopes single_view_ief_past5 / _future5; packed in sorted order */
size_t hmmr_pack_ief_bytes(const hmmr_var_t* vars, int n_vars, int dtype, const int* delta_t, int n_delta);
int hmmr_pack_ief(const hmmr_var_t* vars, int n_vars, int dtype, const int* delta_t, int n_delta, int num_stages, void* host_blob,
                  size_t blob_bytes, const void* device_base, hmmr_ief_weights_t* out);
/* D_pose/D_conv1|D_conv2/weights [1,1,9,32] / [1,1,32,32], D_pose/pose_out_j{0..22}/weights [32,1], D_pose/D_alljoints_fc1|fc2|out/
 * weights [736,1024] / [1024,1024] / [1024,1], each with its biases -> the bank of "Pose discriminator"; dtype must be HMMR_F32. */
size_t hmmr_pack_disc_pose_bytes(const hmmr_var_t* vars, int n_vars, int dtype);
int hmmr_pack_disc_pose(const hmmr_var_t* vars, int n_vars, int dtype, void* host_blob, size_t blob_bytes, const void* device_base,
                        hmmr_disc_pose_weights_t* out);

/* The body model in the src/tf_smpl layout (batch_smpl.py:35-80: what SMPL.__init__ builds from the pkl, or the checkpoint's own
 * non-trainable variables of the same names), fp32 host arrays */
typedef struct {
    int num_verts;                 /* 6890 */
    int num_kps;                   /* columns of kp_regressor: 25 (19 cocoplus + 6) */
    const float* v_template;       /* [num_verts][3] */
    const float* shapedirs;        /* [10][3 num_verts]: column 3 v + c */
    const float* posedirs;         /* [207][3 num_verts] */
    const float* J_regressor;      /* [num_verts][24] (stored transposed, batch_smpl.py:51-55) */
    const float* lbs_weights;      /* [num_verts][24] */
    const float* kp_regressor;     /* cocoplus_regressor [num_verts][num_kps] */
    const int32_t* parents;        /* [24] */
} hmmr_smpl_source_t;
/* lsp != 0: joint_type 'lsp', the first 14 keypoints (batch_smpl.py:81-82); split != 0: also the split-fp16 MFMA form of the blend basis
 * (hmmr_smpl_consts_t.dirs_split; 0 for an all-fp32 engine) */
size_t hmmr_pack_smpl_bytes(const hmmr_smpl_source_t* src, int lsp, int split);
int hmmr_pack_smpl(const hmmr_smpl_source_t* src, int lsp, int split, void* host_blob, size_t blob_bytes, const void* device_base,
                   hmmr_smpl_consts_t* out);
/* What hmmr_smpl_bwd needs beside hmmr_smpl_consts_t: kp_regressor by vertex (lsp as above).  A blob of its own, so an
 * inference-only process never packs it. */
size_t hmmr_pack_smpl_grad_bytes(const hmmr_smpl_source_t* src, int lsp);
int hmmr_pack_smpl_grad(const hmmr_smpl_source_t* src, int lsp, void* host_blob, size_t blob_bytes, const void* device_base,
                        hmmr_smpl_grad_consts_t* out);

/* ------------------------------------------------------------------------- *
 * A whole video through one call (additive to ABI 19): Tester.predict_all_images (src/evaluation/tester.py:260-312).
 *
 * The reference pads the video with `margin` zero IMAGES in front and `num_fill` behind, cuts windows of T frames every
 * g = T - 2 margin frames (margin = (fov - 1) / 2), runs each through the graph and keeps the centre g predictions of each
 * (tester.py:281-311).  That scheme is part of the numerical contract -- GroupNorm statistics span the window, the padding
 * frames pass through the encoder -- so it lives here, not in the binder: window w, slot t sits at padded position
 * p = w g + t and holds frame p - margin when 0 <= p - margin < n, else the zero image; slot margin + j of window w
 * (0 <= j < g) is output frame w g + j.
 *
 * `batch_size` is not a parameter.  The reference runs count * batch_size windows, count = ceil(n / (g batch_size)); the
 * windows from ceil(n / g) on keep no frame (their centre slots lie at or beyond frame n), and every stage after the
 * encoder works per window, so they change no kept value: n_windows = ceil(n / g) here, whatever the caller's batch size.
 * ------------------------------------------------------------------------- */
typedef struct {
    int n, T, fov;               /* as given */
    int margin, g;               /* (fov - 1) / 2, T - 2 margin */
    int n_windows;               /* ceil(n / g) */
    int max_frames, max_windows; /* as given */
    int resnet_passes;           /* ceil(n / max_frames): pass i encodes frames [i max_frames, min(n, (i + 1) max_frames)); the
                                    last one carries the zero image (n_zero = 1) */
    int tail_passes;             /* ceil(n_windows / max_windows): pass i runs windows [i max_windows, min(n_windows, ...)) */
} hmmr_video_plan_t;
/* Host only, no HIP call (tester.py:281-289).  Refused (-1): fov even or < 1, g < 1, n < 0, max_frames < 1, max_windows < 1.
 * n = 0: no window, no pass. */
int hmmr_video_plan(int n, int T, int fov, int max_frames, int max_windows, hmmr_video_plan_t* out);

/* Host only: the packed per-frame record of make_fetch_dict (tester.py:216-227) as hmmr_smpl_fwd_records reads it.
 * field_offsets [num_containers][7] (float offsets of cams [3], joints [K,3], kps [K,2], poses [24,3,3], shapes [10], verts
 * [V,3], omegas [85]): container 0 (the present) first, field after field; then every `_delta` field as
 * [num_containers - 1][...], container r at index r - 1.  *ld_rec = the record's length in floats.  Either output may be
 * NULL. */
int hmmr_record_layout(int num_kps, int num_verts, int num_containers, int32_t* field_offsets, int64_t* ld_rec);

/* The two copies of the scheme (csrc/windows.hip), exposed for tests like hmmr_groupnorm_relu.  Pure copies in 16-byte
 * pieces (c % 4 == 0, 16-byte aligned pointers), 64-bit offsets, no atomics, nothing allocated; bad arguments are refused
 * before the launch.  n = 0 (n_total = 0) or n_windows = 0: nothing is launched, 0 is returned.
 * hmmr_gather_windows (tester.py:285-305): phi [n][c] fp32, phi_zero [c] (the feature of the all-zero image) ->
 *   out [n_windows][T][c], windows w0 .. w0 + n_windows - 1.
 * hmmr_keep_rows (tester.py:306-311): strips [n_windows][T][c] of the same windows -> for 0 <= j < g, slot margin + j of
 *   window w is frame f = w g + j and goes to out + (f - w0 g) ld_out if f < n_total (ld_out >= c, ld_out % 4 == 0); rows
 *   with f >= n_total and the columns c .. ld_out - 1 are not touched.
 * Each is the one-track case {0, n} of its _tracks sibling below, run by the same kernel, and accepts more than the sibling
 * does: hmmr_gather_windows takes any w0, n_windows >= 0, also windows past ceil(n / g) (the reference runs count *
 * batch_size of them; their slots from frame n on hold phi_zero), where the sibling refuses a range that leaves the
 * numbering; hmmr_keep_rows clips its windows' rows at n_total and returns 0 without a launch when none is left (w0 g >=
 * n_total), where the sibling refuses. */
int hmmr_gather_windows(const float* phi, int n, const float* phi_zero, int w0, int n_windows, int T, int margin, int g,
                        int c, float* out, void* stream);
int hmmr_keep_rows(const float* strips, int w0, int n_windows, int T, int margin, int g, int c, int n_total, float* out,
                   int64_t ld_out, void* stream);

typedef struct {
    const hmmr_resnet_weights_t* resnet;
    const hmmr_temporal_weights_t* temporal;          /* pred_mode 'pred' (tester.py:183-188) ... */
    const hmmr_hallucinator_weights_t* hallucinator;  /* ... or 'hal' (:189-190): exactly one of the two */
    const hmmr_ief_weights_t* ief;
    const hmmr_smpl_consts_t* smpl;
    int sequence_length, fov;                         /* 20, 4 * num_conv_layers + 1 (tester.py:44-47) */
} hmmr_model_t;

/* hmmr_predict_video: images [n,224,224,3] fp32 in [-1,1] on the device -> rec [n][ld_rec], the packed record of every
 * frame (hmmr_record_layout, or any layout hmmr_smpl_fwd_records accepts: field_offsets is a HOST array
 * [ief->num_regressors][7]).  Everything is queued on `stream`; nothing is allocated or synchronised.  Model pointers, the
 * plan, every unit table, ws_bytes and ld_rec against the end of the last field are checked BEFORE the first launch: a
 * refused call (-1) queues nothing.  n = 0: returns 0, queues nothing.  images must be 16-byte aligned, as for hmmr_resnet50_fwd
 * (every pass then starts on an aligned image); a pointer that is not is among the refusals.
 *   1. ResNet passes of at most max_frames frames (hmmr_resnet50_fwd, one launch sequence each) into phi [n + 1][2048]
 *      inside `ws`; the last pass appends the zero image (n_zero = 1), whose feature fills every padding slot;
 *   2. tail passes of at most max_windows windows: hmmr_gather_windows, hmmr_temporal_fwd (or hmmr_hallucinator_fwd over
 *      the n_windows T slots), hmmr_keep_rows, hmmr_ief_fwd on the kept rows, hmmr_smpl_fwd_records into rec + o0 ld_rec
 *      (o0 = the pass's first frame).
 * Per-frame encoder, per-window tail, split_k never chosen from the batch: the records do not depend on max_frames /
 * max_windows, bit for bit.  The call reads no run flags: read hmmr_run_flags where the records are read.
 * The workspace (0: bad model or plan) holds phi and, one after the other on the stream, the ResNet workspace of
 * min(n, max_frames) + 1 frames and the tail's buffers for min(n_windows, max_windows) windows; it never shrinks as n grows.
 * The call is hmmr_predict_tracks (below) with one track, track_offsets = {0, n}: the same driver, the same workspace, the
 * same refusals under this call's name.  Beyond the sibling it refuses n < 0 itself; like the sibling, and unlike
 * hmmr_video_plan, it refuses n = INT32_MAX (row n, the zero image's, would not be a 32-bit row number), in the call and in
 * the query (0). */
size_t hmmr_predict_video_workspace_bytes(const hmmr_model_t* model, int n, int max_frames, int max_windows);
int hmmr_predict_video(const hmmr_model_t* model, const float* images, int n, float* rec, int64_t ld_rec,
                       const int32_t* field_offsets, int max_frames, int max_windows, void* ws, size_t ws_bytes,
                       void* stream);

/* ------------------------------------------------------------------------- *
 * Every tracked person of a video through one call (additive to ABI 19): the ragged form of the scheme above.
 *
 * Tracks lie one after the other along the frame axis, as for hmmr_track_bbox.  track_offsets: n_tracks + 1 non-decreasing
 * int32 values in HOST memory, track_offsets[0] = 0; it is checked before anything is launched and reaches the kernels as
 * kernel arguments, 64 tracks per launch: no device table, no upload, no synchronisation.  With off = track_offsets:
 *   track k has n_k = off[k + 1] - off[k] frames (0 is legal) and W_k = ceil(n_k / g) windows;
 *   windows are numbered globally, track after track: B_k = W_0 + ... + W_{k-1}, n_windows = B_{n_tracks};
 *   gather: slot t of window B_k + lw holds phi[off[k] + f], f = lw g + t - margin, if 0 <= f < n_k, else phi_zero -- never a
 *           frame of a neighbouring track: every track has its own zero-image padding;
 *   keep:   for 0 <= j < min(g, n_k - lw g), slot margin + j of window B_k + lw is output row off[k] + lw g + j: the kept rows of
 *           consecutive windows are consecutive (also across tracks), and the rows come out in global frame order.
 * Rows [off[k], off[k + 1]) of the result are, byte for byte, what the one-video call writes for track k alone.
 * ------------------------------------------------------------------------- */
typedef struct {
    int n_tracks, T, fov;        /* as given */
    int margin, g;               /* (fov - 1) / 2, T - 2 margin */
    int n_frames;                /* track_offsets[n_tracks] */
    int n_windows;               /* sum of ceil(n_k / g) */
    int max_frames, max_windows; /* as given */
    int resnet_passes;           /* ceil(n_frames / max_frames) over the concatenated frames; the last one carries the zero image */
    int tail_passes;             /* ceil(n_windows / max_windows): pass i runs global windows [i max_windows, min(n_windows, ...)) */
} hmmr_tracks_plan_t;
/* Host only, no HIP call.  Refused (-1): null track_offsets (also for n_tracks = 0: one value is read), n_tracks < 0,
 * track_offsets[0] != 0, a decreasing pair (named), n_frames = INT32_MAX (row n_frames, the zero image's, would not be an
 * int), fov even or < 1, g < 1, max_frames < 1, max_windows < 1.  No track or only empty ones: no window, no pass. */
int hmmr_tracks_plan(const int32_t* track_offsets, int n_tracks, int T, int fov, int max_frames, int max_windows,
                     hmmr_tracks_plan_t* out);
/* Host only.  The owner of global window w: *track = k and *local_window = lw with w = B_k + lw (either may be NULL); -1 if w
 * is not one of the n_windows.  hmmr_tracks_window_rows: the output rows of windows [w0, w0 + n_windows), n_windows >= 1 and all
 * of them existing: *o0 = the first one's first kept row, *keep = how many rows they keep together.  hmmr_tracks_tail_pass:
 * tail pass i of a plan, 0 <= i < tail_passes: its first window, its window count and the two values above. */
int hmmr_tracks_window_owner(const int32_t* track_offsets, int n_tracks, int g, int w, int* track, int* local_window);
int hmmr_tracks_window_rows(const int32_t* track_offsets, int n_tracks, int g, int w0, int n_windows, int* o0, int* keep);
int hmmr_tracks_tail_pass(const int32_t* track_offsets, int n_tracks, const hmmr_tracks_plan_t* plan, int i, int* w0,
                          int* n_windows, int* o0, int* keep);

/* The two copies of the ragged rule (csrc/windows.hip): as hmmr_gather_windows / hmmr_keep_rows (16-byte pieces, 64-bit
 * offsets, nothing allocated, refusals before the launch), for any range [w0, w0 + n_windows) of the global numbering --
 * one that starts inside a track, spans empty tracks or crosses the 64-track boundary of the argument table included; a
 * range that leaves the numbering is refused.  n_windows = 0: nothing is launched.
 * hmmr_gather_windows_tracks: phi [n_frames][c], phi_zero [c] -> out [n_windows][T][c].
 * hmmr_keep_rows_tracks: strips [n_windows][T][c] of the same windows -> the `keep` rows of hmmr_tracks_window_rows, the
 *   first at `out` (= the result's row o0), ld_out floats apart; columns c .. ld_out - 1 and every other row are not touched. */
int hmmr_gather_windows_tracks(const float* phi, const float* phi_zero, const int32_t* track_offsets, int n_tracks, int w0,
                               int n_windows, int T, int margin, int g, int c, float* out, void* stream);
int hmmr_keep_rows_tracks(const float* strips, const int32_t* track_offsets, int n_tracks, int w0, int n_windows, int T,
                          int margin, int g, int c, float* out, int64_t ld_out, void* stream);

/* hmmr_predict_tracks: images [n_frames,224,224,3], the tracks' frames one after the other -> rec [n_frames][ld_rec], row
 * off[k] + f the record of frame f of track k.  hmmr_predict_video's rules hold: everything is queued on `stream`, nothing is
 * allocated or synchronised, every check (track_offsets included) is made before the first launch, a refused call (-1) has
 * queued nothing, -2 comes only from a stage.  No track or only empty ones: returns 0, queues nothing.
 *   1. ResNet passes of at most max_frames of the concatenated frames; the zero image rides on the last one;
 *   2. per tail pass (hmmr_tracks_tail_pass): hmmr_gather_windows_tracks, hmmr_temporal_fwd (or hmmr_hallucinator_fwd),
 *      hmmr_keep_rows_tracks, hmmr_ief_fwd, hmmr_smpl_fwd_records into rec + o0 ld_rec.
 * Windows of several tracks share a tail pass and frames of several tracks a ResNet pass: a crowd of short tracks runs as
 * few large launches instead of many small ones.  The workspace (0: bad model, offsets or plan) is sized like
 * hmmr_predict_video's, for n_frames frames and the largest tail pass. */
size_t hmmr_predict_tracks_workspace_bytes(const hmmr_model_t* model, const int32_t* track_offsets, int n_tracks, int max_frames,
                                           int max_windows);
int hmmr_predict_tracks(const hmmr_model_t* model, const float* images, const int32_t* track_offsets, int n_tracks, float* rec,
                        int64_t ld_rec, const int32_t* field_offsets, int max_frames, int max_windows, void* ws, size_t ws_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMMR_HIP_H */
