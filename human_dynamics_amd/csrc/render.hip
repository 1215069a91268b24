// Rasteriser for the demo views (include/hmmr_hip.h: hmmr_render_mesh).
//
// The reference draws each predicted mesh with neural_renderer (NMR) through VisRenderer
// (src/util/render/nmr_renderer.py), one frame at a time.  Here n frames of one topology go through
// three launches per slab of RENDER_CHUNK frames:
//   1. render_prep_kernel    one workgroup per frame: the camera (and the optional change to the original
//                            image), the optional rotation about the centroid, the projection of every
//                            vertex, and the frame's subpixel bbox of the finite vertices;
//   2. render_setup_kernel   one lane per (frame, face): the face's subpixel bbox, its barycentric and 1/z'
//                            planes (fp64, rounded to fp32) and its shaded colour;
//   3. render_raster_kernel  one workgroup per 64x64-subpixel tile of a frame (32x32 output pixels): the
//                            frame's faces are streamed through LDS 256 at a time, culled by bbox against the
//                            tile with an order-keeping ballot compaction, and tested against the lane's 16
//                            subpixels held in registers; then the 2x2 pool, the composite and the stores.
// Nothing is handed between workgroups inside a launch, there are no atomics, and every subpixel visits
// the faces in index order, so the result is bit-reproducible and a frame renders the same alone or in a batch.
// Every face is tested by every tile its bbox overlaps: no fixed-capacity bin can overflow.
//
// The scene view (hmmr_render_scene) draws all persons of a frame into one raster: launches 1 and 2 run per track on the
// track's rows of a slab, and scene_raster_kernel visits the frame's instances in key order, each through the same LDS
// stream, with a subpixel locked once an instance owns it.
#include "common.h"
#include "hmmr_hip.h"
#include "image_geom.h"
#include "workspace.h"

namespace {

constexpr int RENDER_CHUNK = 64;          // frames per launch triple (bounds the workspace)
constexpr int TILE = 64;                  // subpixels per tile side
constexpr int THREADS = 256;
constexpr float EYE_Z = 2.7320508075688772f;   // 1 / tan(30 deg) + 1: look_at eye at (0, 0, -EYE_Z)

struct FaceRec {                          // barycentrics w_i = A_i (u - qx0) + B_i (v - qy0) + [i == 0]
    float qx0, qy0, a0, b0, a1, b1, a2, b2, az, bz, iz0, pad;   // 1/z' = iz0 + az (u - qx0) + bz (v - qy0)
};

struct Ws {                               // carve-up of the caller's workspace for one slab of frames
    float4* pv;                           // [CH][nv] projected vertex {p.x, p.y, z, 0}
    int4* fbox;                           // [CH] frame bbox {c0, c1, r0, r1} in subpixels
    int2* bbox;                           // [CH][nf] {c0 | c1 << 16, r0 | r1 << 16}
    FaceRec* rec;                         // [CH][nf]
    float4* col;                          // [CH][nf] shaded colour
};

struct WsLayout { size_t pv, fbox, bbox, rec, col, total; };      // Ws as offsets: one slab of `ch` instances (frames, or frames x tracks)
inline WsLayout ws_layout(int ch, int nv, int nf) {
    WsLayout l; WsCarver c;
    l.pv = c.take((size_t)ch * nv * sizeof(float4));
    l.fbox = c.take((size_t)ch * sizeof(int4));
    l.bbox = c.take((size_t)ch * nf * sizeof(int2));
    l.rec = c.take((size_t)ch * nf * sizeof(FaceRec));
    l.col = c.take((size_t)ch * nf * sizeof(float4));
    l.total = c.total();
    return l;
}
inline Ws carve(void* base, const WsLayout& l) {
    char* p = (char*)base;
    return Ws{(float4*)(p + l.pv), (int4*)(p + l.fbox), (int2*)(p + l.bbox), (FaceRec*)(p + l.rec), (float4*)(p + l.col)};
}
inline int mesh_slab(int n) { return n < RENDER_CHUNK ? n : RENDER_CHUNK; }      // frames in one slab of a mesh call over n frames

// subpixel index range whose centres (i + 0.5) / S - 1 may lie in [lo, hi] (ndc), widened by one subpixel so that the
// fp32 edge tests decide at the border; clamped to [0, 2S-1] (empty: first > last)
__device__ inline void sub_range(double lo, double hi, int S, int& a, int& b) {
    const double fa = floor(lo * S + S - 0.5) , fb = ceil(hi * S + S - 0.5);
    a = fa < 0.0 ? 0 : (fa > 2.0 * S ? 2 * S : (int)fa);
    b = fb > 2.0 * S - 1 ? 2 * S - 1 : (fb < -1.0 ? -1 : (int)fb);
}

__device__ inline bool finite3(float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// ---- 1. per frame: camera, rotation, projection, frame bbox ------------------------------------------------------
__global__ void __launch_bounds__(THREADS) render_prep_kernel(hmmr_render_desc_t d, int f0, Ws w) {
    const int fl = blockIdx.x, f = f0 + fl, t = threadIdx.x;
    const hmmr_img::FrameCam c = hmmr_img::frame_camera(d.cams + (long long)f * d.ld_cam,
                                                        d.geom ? d.geom + (long long)f * 5 : nullptr);
    const float* v = d.verts + (long long)f * d.ld_verts;
    __shared__ float red[3][THREADS];
    __shared__ float mn[4][THREADS];
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (d.rotate) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int i = t; i < d.nv; i += THREADS) { sx += v[3 * i]; sy += v[3 * i + 1]; sz += v[3 * i + 2]; }
        red[0][t] = sx; red[1][t] = sy; red[2][t] = sz;
        __syncthreads();
        for (int o = THREADS / 2; o > 0; o >>= 1) {
            if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
            __syncthreads();
        }
        cx = red[0][0] / (float)d.nv; cy = red[1][0] / (float)d.nv; cz = red[2][0] / (float)d.nv;
    }
    float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
    for (int i = t; i < d.nv; i += THREADS) {
        float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
        if (d.rotate) {
            const float ax = x - cx, ay = y - cy, az = z - cz;
            const float* R = d.rot;
            x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], ax), __fmul_rn(R[1], ay)), __fmul_rn(R[2], az)), cx);
            y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3], ax), __fmul_rn(R[4], ay)), __fmul_rn(R[5], az)), cy);
            z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[6], ax), __fmul_rn(R[7], ay)), __fmul_rn(R[8], az)), cz);
        }
        float4 p;
        p.x = __fmul_rn(c.s, __fadd_rn(x, c.tx));
        p.y = -__fmul_rn(c.s, __fadd_rn(y, c.ty));                    // image y points down
        p.z = z;
        p.w = 0.f;
        w.pv[(long long)fl * d.nv + i] = p;
        if (finite3(p)) { xlo = fminf(xlo, p.x); xhi = fmaxf(xhi, p.x); ylo = fminf(ylo, -p.y); yhi = fmaxf(yhi, -p.y); }
    }
    mn[0][t] = xlo; mn[1][t] = -xhi; mn[2][t] = ylo; mn[3][t] = -yhi;
    __syncthreads();
    for (int o = THREADS / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < 4; ++k) mn[k][t] = fminf(mn[k][t], mn[k][t + o]);
        __syncthreads();
    }
    if (t == 0) {
        int4 b;
        if (mn[0][0] <= -mn[1][0]) {
            sub_range(mn[0][0], -mn[1][0], d.size, b.x, b.y);
            sub_range(mn[2][0], -mn[3][0], d.size, b.z, b.w);
        } else {
            b = make_int4(1, 0, 1, 0);
        }
        w.fbox[fl] = b;
    }
}

// ---- 2. per (frame, face): bbox, planes, shading -----------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) render_setup_kernel(hmmr_render_desc_t d, int f0, Ws w) {
    const int fl = blockIdx.y, f = f0 + fl;
    const int j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= d.nf) return;
    const long long o = (long long)fl * d.nf + j;
    const int* fi = d.faces + 3LL * j;
    const float4* pv = w.pv + (long long)fl * d.nv;
    const float4 p0 = pv[fi[0]], p1 = pv[fi[1]], p2 = pv[fi[2]];
    int2 bb = make_int2(1, 1);                                         // empty: c0 = 1 > c1 = 0
    FaceRec r = {};
    float4 col = make_float4(0.f, 0.f, 0.f, 0.f);
    // the triangle in the unflipped camera: q = (p.x, -p.y); z' = z + EYE_Z in fp32 (look_at is a pure translation)
    const double qx[3] = {p0.x, p1.x, p2.x}, qy[3] = {-p0.y, -p1.y, -p2.y};
    const double zp[3] = {(double)(p0.z + EYE_Z), (double)(p1.z + EYE_Z), (double)(p2.z + EYE_Z)};
    const double area2 = (qx[1] - qx[0]) * (qy[2] - qy[0]) - (qy[1] - qy[0]) * (qx[2] - qx[0]);
    if (finite3(p0) && finite3(p1) && finite3(p2) && area2 != 0.0 && isfinite(area2)) {
        double A[3], B[3];
        for (int i = 0; i < 3; ++i) {
            const int a = (i + 1) % 3, b = (i + 2) % 3;
            A[i] = (qy[a] - qy[b]) / area2;
            B[i] = (qx[b] - qx[a]) / area2;
        }
        const double iz[3] = {1.0 / zp[0], 1.0 / zp[1], 1.0 / zp[2]};
        r.qx0 = p0.x; r.qy0 = -p0.y;
        r.a0 = (float)A[0]; r.b0 = (float)B[0]; r.a1 = (float)A[1]; r.b1 = (float)B[1]; r.a2 = (float)A[2]; r.b2 = (float)B[2];
        r.az = (float)(A[0] * iz[0] + A[1] * iz[1] + A[2] * iz[2]);
        r.bz = (float)(B[0] * iz[0] + B[1] * iz[1] + B[2] * iz[2]);
        r.iz0 = (float)iz[0];
        int c0, c1, r0, r1;
        sub_range(fmin(qx[0], fmin(qx[1], qx[2])), fmax(qx[0], fmax(qx[1], qx[2])), d.size, c0, c1);
        sub_range(fmin(qy[0], fmin(qy[1], qy[2])), fmax(qy[0], fmax(qy[1], qy[2])), d.size, r0, r1);
        if (c0 <= c1 && r0 <= r1) bb = make_int2(c0 | (c1 << 16), r0 | (r1 << 16));
        // shading with the viewer-facing unit normal of the projected (y-flipped) triangle, before the z shift
        const float e0x = p0.x - p1.x, e0y = p0.y - p1.y, e0z = p0.z - p1.z;
        const float e2x = p2.x - p1.x, e2y = p2.y - p1.y, e2z = p2.z - p1.z;
        float nx = e0y * e2z - e0z * e2y, ny = e0z * e2x - e0x * e2z, nz = e0x * e2y - e0y * e2x;
        if (nz > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
        const float inv = 1.f / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-5f);
        const float cosv = fmaxf(0.f, (nx * d.light_dir[0] + ny * d.light_dir[1] + nz * d.light_dir[2]) * inv);
        float tex[3] = {d.color[0], d.color[1], d.color[2]};
        if (d.face_colors) {
            const float* fc = d.face_colors + (long long)f * d.ld_face_colors + 3LL * j;
            tex[0] = fc[0]; tex[1] = fc[1]; tex[2] = fc[2];
        }
        float lc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            lc[k] = tex[k] * (d.light_int_ambient * d.light_color_ambient[k] +
                              d.light_int_directional * d.light_color_directional[k] * cosv);
        col = make_float4(lc[0], lc[1], lc[2], 0.f);
    }
    w.bbox[o] = bb;
    w.rec[o] = r;
    w.col[o] = col;
}

// ---- 3. per (frame, tile): raster, pool, composite ---------------------------------------------------------------
// lane layout: wave wv owns subpixel rows [16 wv, 16 wv + 16) of the tile; lane l owns subpixel columns 2 (l & 31) + {0, 1}
// and rows 16 wv + 8 (l >> 5) + [0, 8), i.e. output pixels (l & 31, 8 wv + 4 (l >> 5) + [0, 4)): the pool is lane-local
// The pieces below are shared, inlined, by render_raster_kernel and scene_raster_kernel: one text, the same bits.
struct Lane {
    int wv, l, px, col0, row0;            // wave, lane, pixel column in the tile, first subpixel column / row of the lane
    float uc[2], vr[8];                   // subpixel centres (ndc)
};

__device__ __forceinline__ Lane make_lane(int t, int TC, int TR, int S2) {
    Lane L;
    L.wv = t / HMMR_WAVE; L.l = t % HMMR_WAVE;
    L.px = L.l & 31;
    const int g = L.l >> 5;
    L.col0 = TC + 2 * L.px;                             // the lane's subpixel columns col0, col0 + 1
    L.row0 = TR + 16 * L.wv + 8 * g;                    // the lane's subpixel rows row0 .. row0 + 7
    for (int k = 0; k < 2; ++k) L.uc[k] = (float)(2 * (L.col0 + k) + 1 - S2) / (float)S2;
    for (int k = 0; k < 8; ++k) L.vr[k] = (float)(2 * (L.row0 + k) + 1 - S2) / (float)S2;
    return L;
}

// One instance's nf faces against the lane's 16 subpixels: streamed through LDS 256 at a time, culled by bbox against the
// tile (TC, TR) with an order-keeping ballot compaction.  A face replaces (best, bid) where it covers with 1/z' in
// [0.01, 10] and 1/z' > best.  Every thread of the workgroup calls it; it ends on a barrier.
__device__ __forceinline__ void raster_faces(const int2* bbox, const FaceRec* rec, int nf, int TC, int TR, const Lane& L,
                                             float (&best)[8][2], int (&bid)[8][2]) {
    __shared__ FaceRec s_rec[THREADS];
    __shared__ int2 s_bb[THREADS];
    __shared__ int s_id[THREADS];
    __shared__ int s_cnt[THREADS / HMMR_WAVE];
    const int t = threadIdx.x, wv = L.wv, l = L.l, col0 = L.col0, row0 = L.row0;
    const int band_lo = TR + 16 * wv, band_hi = band_lo + 15;
    for (int base = 0; base < nf; base += THREADS) {
        const int j = base + t;
        bool ok = false;
        int2 bb = make_int2(1, 0);
        if (j < nf) {
            bb = bbox[j];
            const int c0 = bb.x & 0xffff, c1 = bb.x >> 16, r0 = bb.y & 0xffff, r1 = bb.y >> 16;
            ok = c0 <= c1 && !(c1 < TC || c0 > TC + TILE - 1 || r1 < TR || r0 > TR + TILE - 1);
        }
        // order-keeping compaction: rank within the wave by ballot, waves in order through LDS
        const unsigned long long m = __ballot(ok);
        const int rank = __popcll(m & ((1ull << l) - 1ull));
        if (l == 0) s_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
        for (int k = 0; k < THREADS / HMMR_WAVE; ++k) { off += k < wv ? s_cnt[k] : 0; total += s_cnt[k]; }
        if (ok) { s_rec[off + rank] = rec[j]; s_bb[off + rank] = bb; s_id[off + rank] = j; }
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const int2 b = s_bb[i];
            const int r0 = b.y & 0xffff, r1 = b.y >> 16;
            if (r1 < band_lo || r0 > band_hi) continue;                 // the same for the whole wave
            const int c0 = b.x & 0xffff, c1 = b.x >> 16;
            if (c1 < col0 || c0 > col0 + 1 || r1 < row0 || r0 > row0 + 7) continue;
            const FaceRec q = s_rec[i];
            const int id = s_id[i];
            float t0[2], t1[2], t2[2], tz[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float du = L.uc[k] - q.qx0;
                t0[k] = fmaf(q.a0, du, 1.f); t1[k] = q.a1 * du; t2[k] = q.a2 * du; tz[k] = fmaf(q.az, du, q.iz0);
            }
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const float dv = L.vr[a] - q.qy0;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float w0 = fmaf(q.b0, dv, t0[k]), w1 = fmaf(q.b1, dv, t1[k]), w2 = fmaf(q.b2, dv, t2[k]);
                    const float iz = fmaf(q.bz, dv, tz[k]);
                    // z' in [0.1, 100] <=> 1/z' in [0.01, 10]; strictly nearer replaces: ties keep the lower index
                    if (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && iz >= 0.01f && iz <= 10.f && iz > best[a][k]) {
                        best[a][k] = iz;
                        bid[a][k] = id;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// Output pixel (X, Y) of frame f from its four subpixel colours (the background colour where uncovered) and the number
// of covered ones: the 2x2 mean, the composite over the background of d.bg_mode, the stores.  s_lut: the 256 values
// ((i / 255.) - 0.5) * 2 of HMMR_RENDER_BG_FRAME.
__device__ __forceinline__ void composite_store(const hmmr_render_desc_t& d, const double* s_lut, int f, int X, int Y,
                                                const float (&sub)[4][3], int cov) {
    const int S = d.size;
    float sum[3] = {0.f, 0.f, 0.f};
    for (int ch = 0; ch < 3; ++ch) sum[ch] = ((sub[0][ch] + sub[1][ch]) + (sub[2][ch] + sub[3][ch])) * 0.25f;
    const float al = (float)cov * 0.25f, om = 1.f - al;
    const long long pix = ((long long)f * d.out_h + Y) * d.out_w + X;
    unsigned char o[3];
    if (d.bg_mode == HMMR_RENDER_BG_FRAME) {
        int x0, x1, y0, y1; double a0, a1, b0, b1;
        hmmr_img::taps(X, d.frame_w, d.out_w, x0, x1, a0, a1);
        hmmr_img::taps(Y, d.frame_h, d.out_h, y0, y1, b0, b1);
        const unsigned char* fr = (const unsigned char*)d.bg_image + (long long)f * d.frame_h * d.frame_w * 3;
        for (int ch = 0; ch < 3; ++ch) {
            auto pxl = [&](int yy, int xx) { return s_lut[fr[((long long)yy * d.frame_w + xx) * 3 + ch]]; };
            const double img = ((pxl(y0, x0) * a0 + pxl(y0, x1) * a1) * b0 + (pxl(y1, x0) * a0 + pxl(y1, x1) * a1) * b1);
            const double bg = ((img + 1.0) * 0.5) * 255.0;
            const float rend = fminf(fmaxf(sum[ch], 0.f), 1.f) * 255.f;
            const double v = bg * (double)om + (double)(rend * al);
            o[ch] = (unsigned char)(int)v;
        }
    } else if (d.bg_mode == HMMR_RENDER_BG_FLOAT) {
        const float* im = (const float*)d.bg_image + (((long long)f * S + Y) * S + X) * 3;
        for (int ch = 0; ch < 3; ++ch) {
            const float bg = (im[ch] + d.bg_add) * d.bg_mul;
            const float rend = fminf(fmaxf(sum[ch], 0.f), 1.f) * 255.f;
            o[ch] = (unsigned char)(int)(bg * om + rend * al);
        }
    } else {
        for (int ch = 0; ch < 3; ++ch) o[ch] = (unsigned char)(int)(fminf(fmaxf(sum[ch], 0.f), 1.f) * 255.f);
    }
    unsigned char* out = d.rgb + pix * 3;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
    if (d.alpha) d.alpha[pix] = al;
}

__global__ void __launch_bounds__(THREADS) render_raster_kernel(hmmr_render_desc_t d, int f0, Ws w, int tiles_x) {
    const int fl = blockIdx.y, f = f0 + fl, t = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int S2 = 2 * d.size;
    const int TC = tx * TILE, TR = ty * TILE;
    if (!d.face_index && (TC / 2 >= d.out_w || TR / 2 >= d.out_h)) return;   // removed by remove_pads

    __shared__ double s_lut[256];
    const Lane L = make_lane(t, TC, TR, S2);
    const int col0 = L.col0, row0 = L.row0;

    float best[8][2];
    int bid[8][2];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { best[a][b] = -1.f; bid[a][b] = -1; }

    const int4 fb = w.fbox[fl];
    const bool any = !(fb.y < TC || fb.x > TC + TILE - 1 || fb.w < TR || fb.z > TR + TILE - 1);
    if (any) raster_faces(w.bbox + (long long)fl * d.nf, w.rec + (long long)fl * d.nf, d.nf, TC, TR, L, best, bid);

    if (d.face_index) {
        int32_t* fim = d.face_index + (long long)f * S2 * S2;
        if (col0 < S2)
#pragma unroll
            for (int a = 0; a < 8; ++a)
                if (row0 + a < S2) *(int2*)(fim + (long long)(row0 + a) * S2 + col0) = make_int2(bid[a][0], bid[a][1]);
    }

    if (d.bg_mode == HMMR_RENDER_BG_FRAME) {
        s_lut[t] = ((double)t / 255.0 - 0.5) * 2.0;                   // ((img / 255.) - 0.5) * 2 (run_video.py)
        __syncthreads();
    }
    const int X = TC / 2 + L.px;
    if (X >= d.out_w) return;
    const float4* col = w.col + (long long)fl * d.nf;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int Y = (row0 >> 1) + k;
        if (Y >= d.out_h) break;
        int cov = 0;
        float sub[4][3];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int id = bid[2 * k + (s >> 1)][s & 1];
            if (id >= 0) {
                const float4 c = col[id];
                sub[s][0] = c.x; sub[s][1] = c.y; sub[s][2] = c.z;
                ++cov;
            } else {
                sub[s][0] = d.bg_color[0]; sub[s][1] = d.bg_color[1]; sub[s][2] = d.bg_color[2];
            }
        }
        composite_store(d, s_lut, f, X, Y, sub, cov);
    }
}

// ---- 4. the scene view: per (frame, tile), the frame's instances in key order ------------------------------------
// Instance (track k, frame F0 + fl) of a slab sits in workspace slot k * cap + fl (cap: the slab's frame capacity), where
// render_prep_kernel / render_setup_kernel put it, launched once per track on the track's rows inside the slab.
constexpr int SCENE_SLAB = 64;            // instances per slab (bounds the workspace, as RENDER_CHUNK does)

struct SceneTracks { hmmr_scene_track_t t[HMMR_SCENE_MAX_TRACKS]; int n; };

__host__ __device__ inline int scene_slab_frames(int n_tracks) { return SCENE_SLAB / n_tracks > 1 ? SCENE_SLAB / n_tracks : 1; }
inline int scene_slab(int n_frames, int n_tracks) { return n_frames < scene_slab_frames(n_tracks) ? n_frames : scene_slab_frames(n_tracks); }

// Six waves per SIMD, as render_raster_kernel gets by itself: the face loop waits on LDS, and other waves are what hides that.
// The bound costs two spilled registers; at the 95 registers (five waves) the compiler takes otherwise, 64 frames of one
// SMPL-sized person at S = 720 took 3.74 ms instead of 3.62 (tools/scene_bench.py).
__global__ void __launch_bounds__(THREADS, 6) scene_raster_kernel(hmmr_render_desc_t d, SceneTracks tr, int32_t* owner, int F0,
                                                                  int cap, Ws w, int tiles_x) {
    const int fl = blockIdx.y, f = F0 + fl, t = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int S2 = 2 * d.size;
    const int TC = tx * TILE, TR = ty * TILE;
    if (!d.face_index && !owner && (TC / 2 >= d.out_w || TR / 2 >= d.out_h)) return;   // removed by remove_pads

    __shared__ double s_lut[256];
    __shared__ float s_key[HMMR_SCENE_MAX_TRACKS];
    __shared__ int s_here[HMMR_SCENE_MAX_TRACKS], s_order[HMMR_SCENE_MAX_TRACKS];
    const Lane L = make_lane(t, TC, TR, S2);
    const int col0 = L.col0, row0 = L.row0;

    // the order: at most 16 keys, ranked the same way in every workgroup of the frame
    if (t < tr.n) {
        const hmmr_scene_track_t& k = tr.t[t];
        const bool here = k.start <= f && f < k.end;
        float key = -INFINITY;
        if (here) {
            const long long r = f - k.start;
            key = k.priority ? k.priority[r] : hmmr_img::frame_camera(k.cams + r * k.ld_cam, k.geom ? k.geom + r * 5 : nullptr).s;
            if (!isfinite(key)) key = -INFINITY;                       // sorts last
        }
        s_key[t] = key;
        s_here[t] = here;
    }
    __syncthreads();
    int cnt = 0;
    for (int u = 0; u < tr.n; ++u) cnt += s_here[u];
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    if (t < tr.n && s_here[t]) {
        int rank = 0;
        for (int u = 0; u < tr.n; ++u)
            rank += s_here[u] && (s_key[u] > s_key[t] || (s_key[u] == s_key[t] && u < t));
        s_order[rank] = t;
    }
    __syncthreads();

    float best[8][2];
    int bid[8][2];                            // while open: the instance's face so far; once owned: face | owner << 16
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { best[a][b] = -1.f; bid[a][b] = -1; }

    for (int oi = 0; oi < cnt; ++oi) {
        const int k = __builtin_amdgcn_readfirstlane(s_order[oi]);    // the same in every lane: keep the slot's addresses scalar
        const long long slot = (long long)k * cap + fl;
        const int4 fb = w.fbox[slot];
        if (fb.y < TC || fb.x > TC + TILE - 1 || fb.w < TR || fb.z > TR + TILE - 1) continue;   // the instance misses the tile
        raster_faces(w.bbox + slot * d.nf, w.rec + slot * d.nf, d.nf, TC, TR, L, best, bid);
        // lock what this instance took: best = +inf marks an owned subpixel, and nothing is > +inf, so a later instance
        // leaves its (best, bid) alone; the face index fits 16 bits (nf <= 65536), the owner goes above it
        int open = 0;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (best[a][b] != INFINITY) {
                    if (bid[a][b] >= 0) { bid[a][b] |= k << 16; best[a][b] = INFINITY; }
                    else open |= col0 < S2 && row0 + a < S2;
                }
        if (oi + 1 < cnt && !__syncthreads_or(open)) break;            // every subpixel of the tile is owned
    }

    if (col0 < S2) {
#pragma unroll
        for (int a = 0; a < 8; ++a)
            if (row0 + a < S2) {
                const long long o = ((long long)f * S2 + (row0 + a)) * S2 + col0;
                if (d.face_index)
                    *(int2*)(d.face_index + o) = make_int2(bid[a][0] < 0 ? -1 : bid[a][0] & 0xffff, bid[a][1] < 0 ? -1 : bid[a][1] & 0xffff);
                if (owner) *(int2*)(owner + o) = make_int2(bid[a][0] >> 16, bid[a][1] >> 16);     // -1 >> 16 == -1
            }
    }

    if (d.bg_mode == HMMR_RENDER_BG_FRAME) {
        s_lut[t] = ((double)t / 255.0 - 0.5) * 2.0;
        __syncthreads();
    }
    const int X = TC / 2 + L.px;
    if (X >= d.out_w) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int Y = (row0 >> 1) + k;
        if (Y >= d.out_h) break;
        int cov = 0;
        float sub[4][3];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int id = bid[2 * k + (s >> 1)][s & 1];
            if (id >= 0) {
                const float4 c = w.col[((long long)(id >> 16) * cap + fl) * d.nf + (id & 0xffff)];
                sub[s][0] = c.x; sub[s][1] = c.y; sub[s][2] = c.z;
                ++cov;
            } else {
                sub[s][0] = d.bg_color[0]; sub[s][1] = d.bg_color[1]; sub[s][2] = d.bg_color[2];
            }
        }
        composite_store(d, s_lut, f, X, Y, sub, cov);
    }
}

}  // namespace

extern "C" size_t hmmr_render_workspace_bytes(int n, int nv, int nf) {
    if (n <= 0 || n > HMMR_RENDER_MAX_FRAMES || nv <= 0 || nf <= 0 || nf > HMMR_RENDER_MAX_FACES) return 0;
    return ws_layout(mesh_slab(n), nv, nf).total;
}

extern "C" int hmmr_render_mesh(const hmmr_render_desc_t* d, void* stream) {
    HMMR_REQUIRE(d, "hmmr_render_mesh: NULL descriptor");
    HMMR_REQUIRE(d->verts && d->cams && d->faces && d->rgb && d->ws, "hmmr_render_mesh: NULL operand");
    HMMR_REQUIRE(d->n >= 1 && d->n <= HMMR_RENDER_MAX_FRAMES, "hmmr_render_mesh: n = %d outside [1, %d]", d->n,
                 HMMR_RENDER_MAX_FRAMES);
    HMMR_REQUIRE(d->size >= HMMR_RENDER_MIN_SIZE && d->size <= HMMR_RENDER_MAX_SIZE,
                 "hmmr_render_mesh: size = %d outside [%d, %d]", d->size, HMMR_RENDER_MIN_SIZE, HMMR_RENDER_MAX_SIZE);
    HMMR_REQUIRE(d->nf >= 1 && d->nf <= HMMR_RENDER_MAX_FACES, "hmmr_render_mesh: nf = %d outside [1, %d]", d->nf,
                 HMMR_RENDER_MAX_FACES);
    HMMR_REQUIRE(d->nv >= 3, "hmmr_render_mesh: nv = %d < 3", d->nv);
    HMMR_REQUIRE(d->ld_verts >= 3LL * d->nv && d->ld_cam >= 3, "hmmr_render_mesh: row strides smaller than the rows");
    HMMR_REQUIRE(!d->face_colors || d->ld_face_colors == 0 || d->ld_face_colors >= 3LL * d->nf,
                 "hmmr_render_mesh: face_colors row stride smaller than the rows");
    HMMR_REQUIRE(d->out_h >= 1 && d->out_w >= 1 && d->out_h <= d->size && d->out_w <= d->size,
                 "hmmr_render_mesh: output %d x %d outside [1, size = %d]", d->out_h, d->out_w, d->size);
    HMMR_REQUIRE(d->bg_mode >= HMMR_RENDER_BG_COLOR && d->bg_mode <= HMMR_RENDER_BG_FRAME, "hmmr_render_mesh: bad bg_mode %d",
                 d->bg_mode);
    HMMR_REQUIRE(d->bg_mode == HMMR_RENDER_BG_COLOR || d->bg_image, "hmmr_render_mesh: bg_mode %d without bg_image", d->bg_mode);
    HMMR_REQUIRE(d->bg_mode != HMMR_RENDER_BG_FRAME || (d->frame_h >= 1 && d->frame_w >= 1),
                 "hmmr_render_mesh: bad frame size %d x %d", d->frame_h, d->frame_w);
    const WsLayout l = ws_layout(mesh_slab(d->n), d->nv, d->nf);
    HMMR_REQUIRE(d->ws_bytes >= l.total, "hmmr_render_mesh: workspace %zu bytes < %zu", d->ws_bytes, l.total);
    const Ws w = carve(d->ws, l);
    const int tiles_x = (2 * d->size + TILE - 1) / TILE;
    hipStream_t st = (hipStream_t)stream;
    for (int f0 = 0; f0 < d->n; f0 += RENDER_CHUNK) {
        const int m = d->n - f0 < RENDER_CHUNK ? d->n - f0 : RENDER_CHUNK;
        hipLaunchKernelGGL(render_prep_kernel, dim3(m), dim3(THREADS), 0, st, *d, f0, w);
        HMMR_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(render_setup_kernel, dim3((d->nf + THREADS - 1) / THREADS, m), dim3(THREADS), 0, st, *d, f0, w);
        HMMR_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(render_raster_kernel, dim3(tiles_x * tiles_x, m), dim3(THREADS), 0, st, *d, f0, w, tiles_x);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" size_t hmmr_render_scene_workspace_bytes(int n_frames, int n_tracks, int nv, int nf) {
    if (n_frames <= 0 || n_frames > HMMR_RENDER_MAX_FRAMES || n_tracks < 1 || n_tracks > HMMR_SCENE_MAX_TRACKS || nv <= 0 ||
        nf <= 0 || nf > HMMR_RENDER_MAX_FACES)
        return 0;
    return ws_layout(scene_slab(n_frames, n_tracks) * n_tracks, nv, nf).total;
}

extern "C" int hmmr_render_scene(const hmmr_scene_desc_t* d, void* stream) {
    HMMR_REQUIRE(d, "hmmr_render_scene: NULL descriptor");
    HMMR_REQUIRE(d->tracks && d->faces && d->rgb && d->ws, "hmmr_render_scene: NULL operand");
    HMMR_REQUIRE(d->n_tracks >= 1 && d->n_tracks <= HMMR_SCENE_MAX_TRACKS, "hmmr_render_scene: n_tracks = %d outside [1, %d]",
                 d->n_tracks, HMMR_SCENE_MAX_TRACKS);
    HMMR_REQUIRE(d->n_frames >= 1 && d->n_frames <= HMMR_RENDER_MAX_FRAMES, "hmmr_render_scene: n_frames = %d outside [1, %d]",
                 d->n_frames, HMMR_RENDER_MAX_FRAMES);
    HMMR_REQUIRE(d->size >= HMMR_RENDER_MIN_SIZE && d->size <= HMMR_RENDER_MAX_SIZE,
                 "hmmr_render_scene: size = %d outside [%d, %d]", d->size, HMMR_RENDER_MIN_SIZE, HMMR_RENDER_MAX_SIZE);
    HMMR_REQUIRE(d->nf >= 1 && d->nf <= HMMR_RENDER_MAX_FACES, "hmmr_render_scene: nf = %d outside [1, %d]", d->nf,
                 HMMR_RENDER_MAX_FACES);
    HMMR_REQUIRE(d->nv >= 3, "hmmr_render_scene: nv = %d < 3", d->nv);
    HMMR_REQUIRE(d->out_h >= 1 && d->out_w >= 1 && d->out_h <= d->size && d->out_w <= d->size,
                 "hmmr_render_scene: output %d x %d outside [1, size = %d]", d->out_h, d->out_w, d->size);
    HMMR_REQUIRE(d->bg_mode == HMMR_RENDER_BG_COLOR || d->bg_mode == HMMR_RENDER_BG_FRAME,
                 "hmmr_render_scene: bad bg_mode %d (the background colour or a uint8 frame)", d->bg_mode);
    HMMR_REQUIRE(d->bg_mode == HMMR_RENDER_BG_COLOR || d->bg_image, "hmmr_render_scene: bg_mode %d without bg_image", d->bg_mode);
    HMMR_REQUIRE(d->bg_mode != HMMR_RENDER_BG_FRAME || (d->frame_h >= 1 && d->frame_w >= 1),
                 "hmmr_render_scene: bad frame size %d x %d", d->frame_h, d->frame_w);
    SceneTracks tr = {};
    tr.n = d->n_tracks;
    for (int k = 0; k < d->n_tracks; ++k) {
        const hmmr_scene_track_t& t = d->tracks[k];
        HMMR_REQUIRE(t.verts && t.cams, "hmmr_render_scene: NULL operand in track %d", k);
        HMMR_REQUIRE(t.start >= 0 && t.start < t.end && t.end <= d->n_frames,
                     "hmmr_render_scene: track %d covers frames [%d, %d) of %d", k, t.start, t.end, d->n_frames);
        HMMR_REQUIRE(t.ld_verts >= 3LL * d->nv && t.ld_cam >= 3, "hmmr_render_scene: row strides of track %d smaller than the rows", k);
        tr.t[k] = t;
    }
    const int cap = scene_slab(d->n_frames, d->n_tracks);      // frames per slab, each with n_tracks instances
    const WsLayout l = ws_layout(cap * d->n_tracks, d->nv, d->nf);
    HMMR_REQUIRE(d->ws_bytes >= l.total, "hmmr_render_scene: workspace %zu bytes < %zu", d->ws_bytes, l.total);

    hmmr_render_desc_t r = {};                // what the tracks share, in hmmr_render_mesh's terms
    r.faces = d->faces;
    r.nv = d->nv; r.nf = d->nf; r.size = d->size;
    for (int i = 0; i < 3; ++i) {
        r.bg_color[i] = d->bg_color[i]; r.light_dir[i] = d->light_dir[i];
        r.light_color_ambient[i] = d->light_color_ambient[i]; r.light_color_directional[i] = d->light_color_directional[i];
    }
    r.light_int_ambient = d->light_int_ambient; r.light_int_directional = d->light_int_directional;
    r.bg_mode = d->bg_mode; r.bg_image = d->bg_image;
    r.frame_h = d->frame_h; r.frame_w = d->frame_w; r.out_h = d->out_h; r.out_w = d->out_w;
    r.rgb = d->rgb; r.alpha = d->alpha; r.face_index = d->face_index;

    const Ws w = carve(d->ws, l);
    const int tiles_x = (2 * d->size + TILE - 1) / TILE;
    hipStream_t st = (hipStream_t)stream;
    for (int F0 = 0; F0 < d->n_frames; F0 += cap) {
        const int m = d->n_frames - F0 < cap ? d->n_frames - F0 : cap;
        for (int k = 0; k < d->n_tracks; ++k) {
            const hmmr_scene_track_t& t = tr.t[k];
            const int lo = t.start > F0 ? t.start : F0, hi = t.end < F0 + m ? t.end : F0 + m;
            if (lo >= hi) continue;
            hmmr_render_desc_t rt = r;        // the track's rows [lo - start, hi - start) into slots k cap + [lo - F0, hi - F0)
            rt.verts = t.verts; rt.ld_verts = t.ld_verts; rt.cams = t.cams; rt.ld_cam = t.ld_cam; rt.geom = t.geom;
            rt.n = t.end - t.start;
            for (int i = 0; i < 3; ++i) rt.color[i] = t.color[i];
            const long long slot = (long long)k * cap + (lo - F0);
            Ws wt = w;
            wt.pv += slot * d->nv; wt.fbox += slot; wt.bbox += slot * d->nf; wt.rec += slot * d->nf; wt.col += slot * d->nf;
            hipLaunchKernelGGL(render_prep_kernel, dim3(hi - lo), dim3(THREADS), 0, st, rt, lo - t.start, wt);
            HMMR_CHECK_HIP(hipGetLastError());
            hipLaunchKernelGGL(render_setup_kernel, dim3((d->nf + THREADS - 1) / THREADS, hi - lo), dim3(THREADS), 0, st, rt,
                               lo - t.start, wt);
            HMMR_CHECK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(scene_raster_kernel, dim3(tiles_x * tiles_x, m), dim3(THREADS), 0, st, r, tr, d->owner, F0, cap, w,
                           tiles_x);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
