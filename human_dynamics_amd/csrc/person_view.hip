// The person-centred view on the device (include/hmmr_hip.h: hmmr_video_bbox): compute_video_bbox of
// src/util/render/nmr_renderer.py (:519-634) for every person track of a video in one call -- the box that holds the person over
// the whole track, then each frame's camera relative to that box.
//
// All arithmetic is fp64 on the fp32 inputs and this file is compiled with -ffp-contract=off (build.py): NumPy rounds every product
// before it adds.  Tracks lie one after the other along the row axis; `offsets` (host memory, checked before anything is launched)
// travels to the kernel by value, VIEW_CHUNK tracks per launch.  One kernel, one workgroup per track:
//   pass one   a strided loop over the track's frames: the four clamped extremes of each frame and whether everything read was
//              finite; then a tree reduction in LDS (min / max are exact, so the order of the tree cannot change a bit)
//   pass two   the same strided loop: the camera of each frame relative to the box, and whether its crop origin lies nearer
//              the image origin than the box does (the reference's breakpoint); a second small reduction ORs that into the status
// No atomics, no workspace, no allocation, no host synchronisation: the same bits every run.
#include <math.h>

#include "common.h"
#include "hmmr_hip.h"

namespace {
constexpr int VIEW_THREADS = 256;
constexpr int VIEW_CHUNK = 64;                    // tracks per launch (their offsets are kernel arguments)

struct Chunk { int n; int off[VIEW_CHUNK + 1]; };          // off: absolute rows

__device__ __forceinline__ bool fits_int32(double v) { return v > -2147483649. && v < 2147483648.; }      // after truncation; false for NaN

__global__ __launch_bounds__(VIEW_THREADS) void person_view_kernel(Chunk c, int track0, const float* __restrict__ cams, long long ld_cam,
                                                                   const float* __restrict__ kps, long long ld_kps, int k,
                                                                   const double* __restrict__ proc, double proc_size, int img_h, int img_w,
                                                                   double margin, int32_t* __restrict__ bbox, float* __restrict__ cams_crop,
                                                                   int32_t* __restrict__ status) {
    __shared__ double s_ext[4][VIEW_THREADS];     // ymin, ymax, xmin, xmax
    __shared__ int s_flag[VIEW_THREADS];
    const int t = threadIdx.x, trk = blockIdx.x;
    const long long base = c.off[trk];
    const int n = c.off[trk + 1] - c.off[trk];
    int32_t* box = bbox + (long long)(track0 + trk) * 4;
    if (n <= 0) {                                  // (the whole workgroup leaves: no barrier is skipped by a part of it)
        if (t == 0) {
            box[0] = box[1] = box[2] = box[3] = 0;
            status[track0 + trk] = HMMR_BBOX_EMPTY;
        }
        return;
    }
    // ---- pass one: the extremes of this lane's frames
    double ymin = INFINITY, ymax = -INFINITY, xmin = INFINITY, xmax = -INFINITY;
    int bad = 0;
    for (int i = t; i < n; i += VIEW_THREADS) {
        const long long row = base + i;
        const double scale = proc[row * 3], sx = proc[row * 3 + 1], sy = proc[row * 3 + 2];
        const float* cam = cams + row * ld_cam;
        const float* kp = kps + row * ld_kps;
        bad |= !(isfinite(scale) && isfinite(sx) && isfinite(sy) && isfinite(cam[0]) && isfinite(cam[1]) && isfinite(cam[2]));
        const double undo = 1. / scale;
        double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        for (int j = 0; j < k; ++j) {
            const double kx = (double)kp[2 * j], ky = (double)kp[2 * j + 1];
            bad |= !(isfinite(kx) && isfinite(ky));
            const double px = ((kx + 1.) * 0.5) * proc_size, py = ((ky + 1.) * 0.5) * proc_size;
            const double qx = ((px + sx) - proc_size) * undo, qy = ((py + sy) - proc_size) * undo;
            x0 = fmin(x0, qx); x1 = fmax(x1, qx); y0 = fmin(y0, qy); y1 = fmax(y1, qy);
        }
        const double fy0 = fmax(0., y0 - margin), fy1 = fmin((double)(img_h - 1), y1 + margin);
        const double fx0 = fmax(0., x0 - margin), fx1 = fmin((double)(img_w - 1), x1 + margin);
        bad |= !(isfinite(fy0) && isfinite(fy1) && isfinite(fx0) && isfinite(fx1));       // e.g. scale = 0 behind finite inputs
        ymin = fmin(ymin, fy0); ymax = fmax(ymax, fy1); xmin = fmin(xmin, fx0); xmax = fmax(xmax, fx1);
    }
    s_ext[0][t] = ymin; s_ext[1][t] = ymax; s_ext[2][t] = xmin; s_ext[3][t] = xmax;
    s_flag[t] = bad;
    __syncthreads();
    for (int d = VIEW_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) {
            s_ext[0][t] = fmin(s_ext[0][t], s_ext[0][t + d]);
            s_ext[1][t] = fmax(s_ext[1][t], s_ext[1][t + d]);
            s_ext[2][t] = fmin(s_ext[2][t], s_ext[2][t + d]);
            s_ext[3][t] = fmax(s_ext[3][t], s_ext[3][t + d]);
            s_flag[t] |= s_flag[t + d];
        }
        __syncthreads();
    }
    const double e0 = s_ext[0][0], e1 = s_ext[1][0], e2 = s_ext[2][0], e3 = s_ext[3][0];
    const bool not_finite = s_flag[0] || !(fits_int32(e0) && fits_int32(e1) && fits_int32(e2) && fits_int32(e3));
    __syncthreads();                               // everyone has read s_flag[0] before pass two writes it
    if (not_finite) {
        const float nanf_ = __builtin_nanf("");
        for (int i = t; i < n; i += VIEW_THREADS)
            for (int a = 0; a < 3; ++a) cams_crop[(base + i) * 3 + a] = nanf_;
        if (t == 0) {
            box[0] = box[1] = box[2] = box[3] = 0;
            status[track0 + trk] = HMMR_BBOX_NOT_FINITE;
        }
        return;
    }
    const int b_ymin = (int)e0, b_ymax = (int)e1, b_xmin = (int)e2, b_xmax = (int)e3;      // toward zero
    // int32 differences can leave int32 (ymax far below zero for a person above the frame): the side in 64 bits, as NumPy's int64 has it
    const long long dy = (long long)b_ymax - b_ymin, dx = (long long)b_xmax - b_xmin;
    const long long S = dy > dx ? dy : dx;
    const double off_x = (double)b_xmin, off_y = (double)b_ymin;
    const double off_norm = sqrt(off_x * off_x + off_y * off_y);
    const double two_over_s = 2. / (double)S;
    // ---- pass two: the cameras
    int beyond = 0;
    for (int i = t; i < n; i += VIEW_THREADS) {
        const long long row = base + i;
        const double scale = proc[row * 3], sx = proc[row * 3 + 1], sy = proc[row * 3 + 2];
        const float* cam = cams + row * ld_cam;
        const double undo = 1. / scale;
        const double nx = sx - off_x * scale, ny = sy - off_y * scale;
        beyond |= sqrt(sx * sx + sy * sy) < off_norm;
        const double cam0 = (double)cam[0];
        const double c0 = (proc_size * cam0) * 0.5;
        const double shift = (2. / cam0) * 0.5;
        const double c1 = (double)cam[1] + shift, c2 = (double)cam[2] + shift;
        const double o0 = c0 * undo;
        const double o1 = c1 + (nx - proc_size) / c0, o2 = c2 + (ny - proc_size) / c0;
        const double back = 1. / (two_over_s * o0);
        cams_crop[row * 3 + 0] = (float)(o0 * two_over_s);
        cams_crop[row * 3 + 1] = (float)(o1 - back);
        cams_crop[row * 3 + 2] = (float)(o2 - back);
    }
    s_flag[t] = beyond;
    __syncthreads();
    for (int d = VIEW_THREADS / 2; d > 0; d >>= 1) {
        if (t < d) s_flag[t] |= s_flag[t + d];
        __syncthreads();
    }
    if (t == 0) {
        box[0] = b_ymin; box[1] = b_ymax; box[2] = b_xmin; box[3] = b_xmax;
        status[track0 + trk] = (S <= 0 ? HMMR_BBOX_DEGENERATE : 0) | (s_flag[0] ? HMMR_BBOX_BEYOND_START : 0);
    }
}
}  // namespace

extern "C" int hmmr_video_bbox(const float* cams, long long ld_cam, const float* kps, long long ld_kps, int k, const double* proc,
                               double proc_size, const int32_t* offsets, int n_tracks, int img_h, int img_w, double margin, int32_t* bbox,
                               float* cams_crop, int32_t* status, void* stream) {
    const char* who = "hmmr_video_bbox";
    HMMR_REQUIRE(cams && kps && proc && offsets && bbox && cams_crop && status,
                 "%s: null argument (cams, kps, proc, offsets, bbox, cams_crop and status are needed)", who);
    HMMR_REQUIRE(k >= 1 && k <= HMMR_TRACK_MAX_KPS, "%s: k = %d, need 1 <= k <= %d", who, k, HMMR_TRACK_MAX_KPS);
    HMMR_REQUIRE(ld_kps >= 2ll * k && ld_cam >= 3, "%s: row strides ld_kps = %lld, ld_cam = %lld, need ld_kps >= 2 k = %d and ld_cam >= 3", who,
                 ld_kps, ld_cam, 2 * k);
    HMMR_REQUIRE(n_tracks >= 1, "%s: n_tracks = %d, need at least one track", who, n_tracks);
    HMMR_REQUIRE(offsets[0] >= 0, "%s: offsets[0] = %d is negative", who, offsets[0]);
    for (int t = 0; t < n_tracks; ++t)
        HMMR_REQUIRE(offsets[t + 1] >= offsets[t], "%s: offsets are not monotone (offsets[%d] = %d > offsets[%d] = %d)", who, t, offsets[t],
                     t + 1, offsets[t + 1]);
    HMMR_REQUIRE(offsets[n_tracks] <= HMMR_TRACK_MAX_ROWS, "%s: %d rows, at most %d", who, offsets[n_tracks], HMMR_TRACK_MAX_ROWS);
    HMMR_REQUIRE(img_h >= 1 && img_w >= 1, "%s: frame of %d x %d, need img_h >= 1 and img_w >= 1", who, img_h, img_w);
    HMMR_REQUIRE(proc_size > 0. && isfinite(proc_size), "%s: proc_size = %g, need a positive size", who, proc_size);
    HMMR_REQUIRE(isfinite(margin), "%s: margin = %g is not finite", who, margin);
    for (int t0 = 0; t0 < n_tracks; t0 += VIEW_CHUNK) {
        Chunk c;
        c.n = n_tracks - t0 < VIEW_CHUNK ? n_tracks - t0 : VIEW_CHUNK;
        for (int t = 0; t <= VIEW_CHUNK; ++t) c.off[t] = offsets[t0 + (t < c.n ? t : c.n)];
        hipLaunchKernelGGL(person_view_kernel, dim3((unsigned)c.n), dim3(VIEW_THREADS), 0, (hipStream_t)stream, c, t0, cams, ld_cam, kps,
                           ld_kps, k, proc, proc_size, img_h, img_w, margin, bbox, cams_crop, status);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
