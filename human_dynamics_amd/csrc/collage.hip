// The last two panels of the demo's output (include/hmmr_hip.h: hmmr_draw_skeleton, hmmr_compose_collage):
// the 2D skeleton of src/util/render/render_utils.py:38-234 and the 2x2 collage of src/evaluation/run_video.py:178-197.
// Two bandwidth kernels, one launch each, no allocation, no synchronisation, no atomics.  The file is compiled without fp
// contraction: the collage's doubles are those of oracle/preprocess_oracle.py's cv2_resize_linear, product by product.
#include "common.h"
#include "image_geom.h"
#include "hmmr_hip.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = 64, TILE_H = 16;          // pixels of one workgroup of the skeleton kernel: four rows per thread
constexpr int MAX_K = 25, MAX_PRIMS = 4 * MAX_K;
constexpr int COORD_MIN = -32768, COORD_MAX = 32767;

enum { PRIM_NONE = 0, PRIM_DISC = 1, PRIM_RING = 2, PRIM_LINE = 3 };
struct Prim { int kind, x0, y0, x1, y1, r, color, pad; };      // r: radius, or the thickness of a line

// render_utils.py:70-85, in the order of the dict
enum { PINK, LIGHT_PINK, LIGHT_GREEN, GREEN, RED, LIGHT_RED, LIGHT_ORANGE, ORANGE, PURPLE, LIGHT_PURPLE, LIGHT_BLUE, BLUE, GRAY,
       WHITE };
__constant__ unsigned char c_colors[14][3] = {{197, 27, 125}, {233, 163, 201}, {161, 215, 106}, {77, 146, 33}, {215, 48, 39},
                                              {252, 146, 114}, {252, 141, 89}, {200, 90, 39}, {118, 42, 131}, {175, 141, 195},
                                              {145, 191, 219}, {69, 117, 180}, {130, 130, 130}, {255, 255, 255}};
__constant__ signed char c_jcolors[MAX_K] = {LIGHT_PINK, LIGHT_PINK, LIGHT_PINK, PINK, PINK, PINK, LIGHT_BLUE, LIGHT_BLUE, LIGHT_BLUE,
                                             BLUE, BLUE, BLUE, PURPLE, PURPLE, RED, GREEN, GREEN, WHITE, WHITE,
                                             ORANGE, LIGHT_ORANGE, ORANGE, LIGHT_ORANGE, PINK, LIGHT_PINK};
// the edge colour of a child (the first 19 entries serve both skeletons); -1 where the child has no parent
__constant__ signed char c_ecolors[MAX_K] = {LIGHT_PINK, LIGHT_PINK, LIGHT_PINK, PINK, PINK, PINK, LIGHT_BLUE, LIGHT_BLUE, LIGHT_BLUE,
                                             BLUE, BLUE, BLUE, PURPLE, -1, PURPLE, -1, -1, LIGHT_GREEN, LIGHT_GREEN,
                                             ORANGE, LIGHT_ORANGE, ORANGE, LIGHT_ORANGE, GREEN, GRAY};
__constant__ signed char c_parents19[19] = {1, 2, 8, 9, 3, 4, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16};
__constant__ signed char c_parents25[25] = {24, 2, 8, 9, 3, 23, 7, 8, 12, 12, 9, 10, 14, -1, 13, -1, -1, 15, 16, 23, 24, 19, 20, 4, 1};

// disc(c, r): dx^2 + dy^2 <= r^2 + r; nothing for r < 0
__device__ __forceinline__ bool in_disc(long long dx, long long dy, long long r) {
    return r >= 0 && dx * dx + dy * dy <= r * r + r;
}

// line(p0, p1, t): 4 dist^2(q, segment) <= t^2.  With a = q - p0, d = p1 - p0, L = d.d and s = clamp(a.d, 0, L) the header's
// test is 4 |a L - s d|^2 <= t^2 L^2.  At the clamped ends it is 4 |a|^2 <= t^2 and 4 |a - d|^2 <= t^2; between them
// |a L - (a.d) d|^2 = L (a x d)^2, so it is 4 (a x d)^2 <= t^2 L: the same integers' verdict, in products that int64 holds
// (t^2 L < 2^53 for the clamped coordinates, so a cross product beyond 2^27 is outside without being squared).
__device__ __forceinline__ bool in_line(long long ax, long long ay, long long dx, long long dy, long long t) {
    const long long L = dx * dx + dy * dy, s = ax * dx + ay * dy, tt = t * t;
    if (s <= 0) return 4 * (ax * ax + ay * ay) <= tt;                  // (L == 0 comes here too)
    if (s >= L) return 4 * ((ax - dx) * (ax - dx) + (ay - dy) * (ay - dy)) <= tt;
    const long long cr = ax * dy - ay * dx, acr = cr < 0 ? -cr : cr;
    return acr < (1LL << 27) && 4 * cr * cr <= tt * L;
}

__device__ __forceinline__ bool box_meets_tile(int x0, int y0, int x1, int y1, int m, int tx0, int ty0) {
    const int lx = min(x0, x1) - m, hx = max(x0, x1) + m, ly = min(y0, y1) - m, hy = max(y0, y1) + m;
    return hx >= tx0 && lx < tx0 + TILE_W && hy >= ty0 && ly < ty0 + TILE_H;
}

__global__ void __launch_bounds__(THREADS) skeleton_kernel(hmmr_skeleton_desc_t d, int radius, int tiles_x) {
    __shared__ int s_x[MAX_K], s_y[MAX_K], s_ok[MAX_K];
    __shared__ Prim s_prim[MAX_PRIMS];
    const int t = threadIdx.x, f = blockIdx.y;
    const int tx0 = (blockIdx.x % tiles_x) * TILE_W, ty0 = (blockIdx.x / tiles_x) * TILE_H;
    if (t < d.nk) {
        const float* kp = d.kps + (long long)f * d.ld_kps + 2 * t;
        const float x = (kp[0] + d.kp_add) * d.kp_mul, y = (kp[1] + d.kp_add) * d.kp_mul;
        const bool nan = x != x || y != y;
        s_x[t] = nan ? 0 : (int)fminf(fmaxf(rintf(x), (float)COORD_MIN), (float)COORD_MAX);       // np.round: half to even
        s_y[t] = nan ? 0 : (int)fminf(fmaxf(rintf(y), (float)COORD_MIN), (float)COORD_MAX);
        s_ok[t] = !nan && (!d.vis || d.vis[(long long)f * d.nk + t] != 0);
    }
    __syncthreads();
    if (t < d.nk) {                                         // child t: its (at most) four primitives, in painter's order
        Prim p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = Prim{PRIM_NONE, 0, 0, 0, 0, 0, 0, 0};
        if (s_ok[t]) {
            const int x = s_x[t], y = s_y[t];
            if (d.draw_edges) {
                p[0] = Prim{PRIM_DISC, x, y, x, y, radius, WHITE, 0};
                p[1] = Prim{PRIM_DISC, x, y, x, y, radius - 1, c_jcolors[t], 0};
                const int pa = d.nk == 19 ? c_parents19[t] : c_parents25[t];
                if (pa >= 0 && s_ok[pa]) {
                    p[2] = Prim{PRIM_DISC, s_x[pa], s_y[pa], s_x[pa], s_y[pa], radius - 1, c_jcolors[pa], 0};
                    p[3] = Prim{PRIM_LINE, x, y, s_x[pa], s_y[pa], radius - 2, c_ecolors[t], 0};
                }
            } else {
                p[0] = Prim{PRIM_RING, x, y, x, y, radius - 1, c_jcolors[t], 0};
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                       // a primitive that cannot reach this tile is dropped here
            const int m = p[i].kind == PRIM_LINE ? (p[i].r + 1) / 2 : p[i].r;
            if (p[i].kind != PRIM_NONE && !box_meets_tile(p[i].x0, p[i].y0, p[i].x1, p[i].y1, m, tx0, ty0)) p[i].kind = PRIM_NONE;
            s_prim[4 * t + i] = p[i];
        }
    }
    __syncthreads();
    const int X = tx0 + (t % TILE_W);
    if (X >= d.w) return;
    const int np = 4 * d.nk;
    const bool in_place = d.bg_u8 == d.out;
    for (int k = 0; k < TILE_H / (THREADS / TILE_W); ++k) {
        const int Y = ty0 + (t / TILE_W) + k * (THREADS / TILE_W);
        if (Y >= d.h) break;
        int hit = -1;
        for (int i = np - 1; i >= 0 && hit < 0; --i) {      // the last primitive that covers the pixel is the one seen
            const Prim p = s_prim[i];
            if (p.kind == PRIM_NONE) continue;
            const long long ax = X - p.x0, ay = Y - p.y0;
            bool in;
            if (p.kind == PRIM_DISC) in = in_disc(ax, ay, p.r);
            else if (p.kind == PRIM_RING) in = in_disc(ax, ay, p.r) && !in_disc(ax, ay, p.r - 1);
            else in = in_line(ax, ay, p.x1 - p.x0, p.y1 - p.y0, p.r);
            if (in) hit = p.color;
        }
        const long long pix = (((long long)f * d.h + Y) * d.w + X) * 3;
        unsigned char o[3];
        if (hit >= 0) {
            o[0] = c_colors[hit][0]; o[1] = c_colors[hit][1]; o[2] = c_colors[hit][2];
        } else if (d.bg_float) {
            for (int ch = 0; ch < 3; ++ch) {                // astype(uint8) of the float image: truncation (NaN -> 0)
                const float v = (d.bg_float[pix + ch] + d.bg_add) * d.bg_mul;
                o[ch] = (unsigned char)(int)fminf(fmaxf(v, 0.f), 255.f);
            }
        } else {
            if (in_place) continue;
            o[0] = d.bg_u8[pix]; o[1] = d.bg_u8[pix + 1]; o[2] = d.bg_u8[pix + 2];
        }
        d.out[pix] = o[0]; d.out[pix + 1] = o[1]; d.out[pix + 2] = o[2];
    }
}

// The two left panels go through the reference's floats unchanged: trunc((v / 255) * 255) == v for every byte v, with the
// division in float64 (the mesh panel) and in float32 (the skeleton panel) alike (tests/test_collage_oracle.py), so they
// are copied.
__global__ void __launch_bounds__(THREADS) collage_kernel(hmmr_collage_desc_t d, int wr, int W) {
    __shared__ double s_unit[256];
    s_unit[threadIdx.x] = (double)threadIdx.x / 255.0;
    __syncthreads();
    const int X = blockIdx.x * THREADS + threadIdx.x, Y = blockIdx.y, f = blockIdx.z, S = d.S;
    if (X >= W) return;
    unsigned char o[3];
    if (X < S) {                                            // left column: the crop's mesh panel over its skeleton panel
        const bool top = Y < S;
        const unsigned char* src = (top ? d.rend_crop : d.skel_crop) + (((long long)f * S + (top ? Y : Y - S)) * S + X) * 3;
        o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
    } else {                                                // right column: render_og -> (wr, S) over rot_og -> (S, S)
        const bool top = Y < S;
        const int xr = X - S, yr = top ? Y : Y - S, dst_w = top ? wr : S;
        if (xr >= dst_w) {
            o[0] = o[1] = o[2] = 255;                       // np.ones padding of the narrower panel
        } else {
            const unsigned char* src = (top ? d.render_og : d.rot_og) + (long long)f * d.h * d.w * 3;
            int x0, x1, y0, y1; double a0, a1, b0, b1;
            hmmr_img::taps(xr, d.w, dst_w, x0, x1, a0, a1);
            hmmr_img::taps(yr, d.h, S, y0, y1, b0, b1);
            for (int ch = 0; ch < 3; ++ch) {
                auto px = [&](int yy, int xx) { return s_unit[src[((long long)yy * d.w + xx) * 3 + ch]]; };
                const double r0 = px(y0, x0) * a0 + px(y0, x1) * a1, r1 = px(y1, x0) * a0 + px(y1, x1) * a1;      // horizontal pass
                const double v = r0 * b0 + r1 * b1;                                                                // vertical pass
                o[ch] = (unsigned char)(int)(v * 255.0);    // plt.imsave: (x * 255).astype(uint8)
            }
        }
    }
    unsigned char* out = d.out + (((long long)f * 2 * S + Y) * W + X) * 3;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
}

int resized_width(int S, int h, int w) { return (int)((long long)w * S / h); }

}  // namespace

extern "C" int hmmr_skeleton_radius(int h, int w) {
    if (h < 1 || w < 1) return 0;
    const int r = (int)(((double)(h + w) / 2.0) * 0.01);    // max(4, int(np.mean(shape[:2]) * 0.01))
    return r > 4 ? r : 4;
}

extern "C" int hmmr_draw_skeleton(const hmmr_skeleton_desc_t* d, void* stream) {
    HMMR_REQUIRE(d, "hmmr_draw_skeleton: NULL descriptor");
    HMMR_REQUIRE(d->kps && d->out, "hmmr_draw_skeleton: NULL operand");
    HMMR_REQUIRE((d->bg_float != NULL) != (d->bg_u8 != NULL), "hmmr_draw_skeleton: give bg_float or bg_u8, one of them");
    HMMR_REQUIRE(d->nk == 19 || d->nk == 25, "hmmr_draw_skeleton: unknown skeleton, nk = %d (19 or 25)", d->nk);
    HMMR_REQUIRE(d->n >= 1 && d->n <= HMMR_RENDER_MAX_FRAMES, "hmmr_draw_skeleton: n = %d outside [1, %d]", d->n,
                 HMMR_RENDER_MAX_FRAMES);
    HMMR_REQUIRE(d->h >= HMMR_RENDER_MIN_SIZE && d->h <= HMMR_RENDER_MAX_SIZE && d->w >= HMMR_RENDER_MIN_SIZE &&
                 d->w <= HMMR_RENDER_MAX_SIZE, "hmmr_draw_skeleton: image %d x %d outside [%d, %d]", d->h, d->w,
                 HMMR_RENDER_MIN_SIZE, HMMR_RENDER_MAX_SIZE);
    HMMR_REQUIRE(d->ld_kps >= 2LL * d->nk, "hmmr_draw_skeleton: row stride smaller than the rows");
    HMMR_REQUIRE(d->draw_edges == 0 || d->draw_edges == 1, "hmmr_draw_skeleton: draw_edges = %d (0 or 1)", d->draw_edges);
    HMMR_REQUIRE(d->radius >= 0 && d->radius <= HMMR_SKELETON_MAX_RADIUS, "hmmr_draw_skeleton: radius = %d outside [0, %d]",
                 d->radius, HMMR_SKELETON_MAX_RADIUS);
    const int radius = d->radius ? d->radius : hmmr_skeleton_radius(d->h, d->w);
    HMMR_REQUIRE(!d->draw_edges || radius >= 3, "hmmr_draw_skeleton: radius %d < 3 gives a line thickness < 1", radius);
    const int tiles_x = (d->w + TILE_W - 1) / TILE_W, tiles_y = (d->h + TILE_H - 1) / TILE_H;
    hipLaunchKernelGGL(skeleton_kernel, dim3(tiles_x * tiles_y, d->n), dim3(THREADS), 0, (hipStream_t)stream, *d, radius, tiles_x);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hmmr_collage_width(int S, int h, int w) {
    if (S < HMMR_RENDER_MIN_SIZE || S > HMMR_RENDER_MAX_SIZE || h < 1 || h > HMMR_RENDER_MAX_SIZE || w < 1 ||
        w > HMMR_RENDER_MAX_SIZE)
        return 0;
    const int wr = resized_width(S, h, w);
    if (wr < 1 || wr > HMMR_COLLAGE_MAX_PANEL_WIDTH) return 0;
    return S + (wr > S ? wr : S);
}

extern "C" int hmmr_compose_collage(const hmmr_collage_desc_t* d, void* stream) {
    HMMR_REQUIRE(d, "hmmr_compose_collage: NULL descriptor");
    HMMR_REQUIRE(d->rend_crop && d->skel_crop && d->render_og && d->rot_og && d->out, "hmmr_compose_collage: NULL operand");
    HMMR_REQUIRE(d->n >= 1 && d->n <= HMMR_RENDER_MAX_FRAMES, "hmmr_compose_collage: n = %d outside [1, %d]", d->n,
                 HMMR_RENDER_MAX_FRAMES);
    const int W = hmmr_collage_width(d->S, d->h, d->w);
    HMMR_REQUIRE(W > 0, "hmmr_compose_collage: S = %d with %d x %d panels: sizes outside [%d, %d] / [1, %d], or a resized width "
                 "w S / h outside [1, %d]", d->S, d->h, d->w, HMMR_RENDER_MIN_SIZE, HMMR_RENDER_MAX_SIZE, HMMR_RENDER_MAX_SIZE,
                 HMMR_COLLAGE_MAX_PANEL_WIDTH);
    hipLaunchKernelGGL(collage_kernel, dim3((W + THREADS - 1) / THREADS, 2 * d->S, d->n), dim3(THREADS), 0, (hipStream_t)stream,
                       *d, resized_width(d->S, d->h, d->w), W);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
