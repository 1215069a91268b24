// Track front end on the device (include/hmmr_hip.h: hmmr_track_*): what demo_video.predict_on_tracks (:136-153) does per person track
// before a frame reaches process_image -- src/util/smooth_bbox.py's kp_to_bbox_param (:37-61), get_all_bbox_params (:64-105) and
// smooth_bbox_params (:108-123: scipy.signal.medfilt, then scipy.ndimage.gaussian_filter1d) -- and the integers of process_image /
// resize_img (src/evaluation/run_video.py:56-107) for the smoothed boxes, so that hmmr_crop_frames can start without a host step.
//
// All arithmetic is fp64 and this file is compiled with -ffp-contract=off (build.py): NumPy and SciPy round every product before
// they add.  Tracks lie one after the other along the row axis; `offsets` (host memory, checked before anything is launched)
// travels to the kernels by value, TRACK_CHUNK tracks per launch.  Five small kernels in stream order:
//   track_box_kernel      a lane per row: the box of one frame and whether it counts (valid)
//   track_extent_kernel   a workgroup per track: first / last valid row, then the nearest valid row after every row (a suffix-min
//                         scan, tile by tile from the end with a carry) and before it (a prefix-max scan from the start), and with
//                         the two the np.linspace value of every row in a gap.  TRACK_TILE rows per step; gaps and tracks of any
//                         length.
//   track_median_kernel   a lane per (row, parameter): the zero-padded median by rank counting (no sort, no per-lane array)
//   track_gauss_kernel    a lane per (row, parameter): the reflect-boundary correlation in SciPy's summation order
//   track_geom_kernel     a lane per row: {scaled height, scaled width, u0, v0}, the process_image info, and a status word
// No atomics, no allocation, no host synchronisation: the same bits every run.
#include <math.h>

#include "common.h"
#include "hmmr_hip.h"
#include "workspace.h"

namespace {
constexpr int TRACK_TILE = HMMR_TRACK_TILE;       // rows per scan step = threads of every workgroup here
constexpr int TRACK_CHUNK = 64;                   // tracks per launch (their offsets are kernel arguments)
constexpr int IMG = 224;

struct Chunk { int n; int off[TRACK_CHUNK + 1]; };          // off: absolute rows
struct Weights { int radius; double w[HMMR_TRACK_MAX_RADIUS + 1]; };      // w[j] = weight at distance radius - j (the lower half and the centre)

__global__ void track_box_kernel(const double* __restrict__ kps, const unsigned char* __restrict__ present, int row0, int n, int k,
                                 double vis_thresh, double* __restrict__ box, int* __restrict__ valid) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const long long row = (long long)row0 + r;
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    bool any = false;
    if (present[row]) {
        const double* p = kps + row * k * 3;
        for (int j = 0; j < k; ++j) {
            if (p[3 * j + 2] > vis_thresh) {                                   // strictly: smooth_bbox.py:50
                const double x = p[3 * j], y = p[3 * j + 1];
                if (!any) { x0 = x1 = x; y0 = y1 = y; any = true; }
                else { x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y); }
            }
        }
    }
    const double dx = x1 - x0, dy = y1 - y0;
    const double height = sqrt(dx * dx + dy * dy);
    const bool ok = any && !(height < 0.5);                                    // :56
    box[row * 3 + 0] = ok ? (x0 + x1) / 2. : 0.;
    box[row * 3 + 1] = ok ? (y0 + y1) / 2. : 0.;
    box[row * 3 + 2] = ok ? 150. / height : 0.;
    valid[row] = ok ? 1 : 0;
}

// inclusive scans over the TRACK_TILE values of a workgroup (Hillis-Steele in LDS); every thread calls
__device__ __forceinline__ int tile_prefix_max(int v, int* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < TRACK_TILE; d <<= 1) {
        const int o = t >= d ? s[t - d] : v;
        __syncthreads();
        v = max(v, o);
        s[t] = v;
        __syncthreads();
    }
    return v;
}
__device__ __forceinline__ int tile_suffix_min(int v, int* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < TRACK_TILE; d <<= 1) {
        const int o = t + d < TRACK_TILE ? s[t + d] : v;
        __syncthreads();
        v = min(v, o);
        s[t] = v;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(TRACK_TILE) void track_extent_kernel(Chunk c, int track0, const double* __restrict__ box,
                                                                  const int* __restrict__ valid, int* __restrict__ next,
                                                                  double* __restrict__ interp, double* __restrict__ raw_out,
                                                                  int* __restrict__ range) {
    __shared__ int s[TRACK_TILE];
    __shared__ int s_carry;
    const int t = threadIdx.x, trk = blockIdx.x;
    const long long base = c.off[trk];
    const int n = c.off[trk + 1] - c.off[trk];
    const int* ok = valid + base;
    const int BIG = 0x7fffffff;
    // ---- nearest valid row at or after every row, from the last tile down; the carry is the first valid row of the tiles above
    if (t == 0) s_carry = BIG;
    __syncthreads();
    const int tiles = (n + TRACK_TILE - 1) / TRACK_TILE;
    for (int tile = tiles - 1; tile >= 0; --tile) {
        const int i = tile * TRACK_TILE + t;
        const int carry = s_carry;
        const int v = min(tile_suffix_min(i < n && ok[i] ? i : BIG, s), carry);
        if (i < n) next[base + i] = v;
        __syncthreads();                          // everyone has read s_carry
        if (t == 0) s_carry = v;
        __syncthreads();
    }
    const int start = s_carry == BIG ? -1 : s_carry;          // the first valid row of the track
    __syncthreads();
    // ---- nearest valid row at or before every row, from the first tile up, and with it the rows of the track
    if (t == 0) s_carry = -1;
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int i = tile * TRACK_TILE + t;
        const int carry = s_carry;
        const int p = max(tile_prefix_max(i < n && ok[i] ? i : -1, s), carry);
        if (i < n) {
            const int q = next[base + i];
            double v[3] = {0., 0., 0.};
            if (p >= 0 && q != BIG) {                                   // inside [start, end)
                if (p == i) {
                    for (int a = 0; a < 3; ++a) v[a] = box[(base + i) * 3 + a];
                } else {                                                // np.linspace(prev, curr, gap + 2)[i - p] (smooth_bbox.py:98-101)
                    const double div = (double)(q - p), j = (double)(i - p);
                    for (int a = 0; a < 3; ++a) {
                        const double prev = box[(base + p) * 3 + a], curr = box[(base + q) * 3 + a];
                        const double step = (curr - prev) / div;
                        v[a] = j * step + prev;
                    }
                }
            }
            for (int a = 0; a < 3; ++a) {
                interp[(base + i) * 3 + a] = v[a];
                if (raw_out) raw_out[(base + i) * 3 + a] = v[a];
            }
        }
        __syncthreads();
        if (t == TRACK_TILE - 1) s_carry = p;
        __syncthreads();
    }
    if (t == 0) {                                  // s_carry: the last valid row
        range[(track0 + trk) * 2 + 0] = start;
        range[(track0 + trk) * 2 + 1] = start < 0 ? 0 : s_carry + 1;
    }
}

// the rows a track's filters see: [lo, hi) relative to the track's first row
__device__ __forceinline__ void track_rows(const Chunk& c, int trk, int track0, const int* range, int& n, int& lo, int& hi) {
    n = c.off[trk + 1] - c.off[trk];
    lo = 0; hi = n;
    if (range) {
        lo = range[(track0 + trk) * 2]; hi = range[(track0 + trk) * 2 + 1];
        if (lo < 0 || hi > n || hi < lo) { lo = 0; hi = 0; }
    }
}

// scipy.signal.medfilt: the window is padded with zeros at both ends.  The median of ks values is the one with at most ks / 2
// values below it and more than ks / 2 values not above it.  Up to ks^2 (961 for ks = 31) cached reads of `in` per lane: the price of
// keeping no per-lane array (a dynamically indexed one would live in scratch memory), accepted at these sizes (3 N lanes).
__global__ void track_median_kernel(Chunk c, int track0, const int* __restrict__ range, const double* __restrict__ in, int ks,
                                    double* __restrict__ out) {
    const int trk = blockIdx.y;
    int n, lo, hi;
    track_rows(c, trk, track0, range, n, lo, hi);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * 3) return;
    const int i = e / 3, a = e - 3 * i;
    const long long base = c.off[trk];
    if (i < lo || i >= hi) return;
    const int half = ks / 2;
    auto at = [&](int j) { return j >= lo && j < hi ? in[(base + j) * 3 + a] : 0.; };
    double med = at(i);
    for (int u = -half; u <= half; ++u) {
        const double cand = at(i + u);
        int below = 0, not_above = 0;
        for (int v = -half; v <= half; ++v) {
            const double x = at(i + v);
            below += x < cand;
            not_above += x <= cand;
        }
        if (below <= half && not_above > half) { med = cand; break; }
    }
    out[(base + i) * 3 + a] = med;
}

// scipy.ndimage.gaussian_filter1d, mode='reflect' (d c b a | a b c d | d c b a): correlate1d's symmetric branch,
// x[i] w[0] + sum_{j = -r .. -1} (x[i + j] + x[i - j]) w[j], in that order
__global__ void track_gauss_kernel(Chunk c, int track0, const int* __restrict__ range, const double* __restrict__ in, Weights g,
                                   double* __restrict__ out) {
    const int trk = blockIdx.y;
    int n, lo, hi;
    track_rows(c, trk, track0, range, n, lo, hi);
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * 3) return;
    const int i = e / 3, a = e - 3 * i;
    const long long base = c.off[trk];
    double acc = 0.;
    if (i >= lo && i < hi) {
        const int len = hi - lo, li = i - lo, period = 2 * len;
        auto at = [&](int j) {                     // j may lie several track lengths outside
            int m = j % period;
            if (m < 0) m += period;
            if (m >= len) m = period - 1 - m;
            return in[(base + lo + m) * 3 + a];
        };
        acc = at(li) * g.w[g.radius];
        for (int j = -g.radius; j < 0; ++j) acc += (at(li + j) + at(li - j)) * g.w[g.radius + j];
    }
    out[(base + i) * 3 + a] = acc;                 // rows outside [start, end) are zero (get_smooth_bbox_params stacks zeros in front)
}

// crop_geometry of evaluation/run_video.py (process_image, run_video.py:56-107; resize_img, common.py:7-14) per row
__global__ void track_geom_kernel(Chunk c, int track0, const int* __restrict__ range, const double* __restrict__ bbox, int H, int W,
                                  int4* __restrict__ geom, double* __restrict__ info, int* __restrict__ status) {
    const int trk = blockIdx.y;
    int n, lo, hi;
    track_rows(c, trk, track0, range, n, lo, hi);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long row = (long long)c.off[trk] + i;
    int4 g = {H, W, 0, 0};                          // the identity geometry: any frame can be cropped with it
    double o[5] = {0., 0., 0., 0., 0.};
    int st = 0;
    if (i >= lo && i < hi) {
        const double cx = bbox[row * 3], cy = bbox[row * 3 + 1], scale = bbox[row * 3 + 2];
        const double fh = floor((double)H * scale), fw = floor((double)W * scale);
        const double lim = 1e9;                     // beyond this (or NaN) nothing below fits an int32
        if (!(fabs(fh) < lim && fabs(fw) < lim)) st |= HMMR_TRACK_NOT_FINITE;
        else if (fh < 1. || fw < 1.) st |= HMMR_TRACK_EMPTY;
        if (!st) {
            const int hs = (int)fh, ws = (int)fw;
            const double rx = rint(cx * (fh / (double)H)), ry = rint(cy * (fw / (double)W));       // x by the HEIGHT factor (run_video.py:74)
            if (!(fabs(rx) < lim && fabs(ry) < lim)) st |= HMMR_TRACK_NOT_FINITE;
            else {
                const int csx = (int)rx + IMG, csy = (int)ry + IMG;                                 // in the padded image
                const int sx = csx - IMG / 2, sy = csy - IMG / 2;
                if (sx < 0 || sy < 0) st |= HMMR_TRACK_BEFORE_ORIGIN;
                if (csx + IMG / 2 > ws + 2 * IMG || csy + IMG / 2 > hs + 2 * IMG) st |= HMMR_TRACK_CLIPPED;
                if (!st) {
                    g = int4{hs, ws, sx - IMG, sy - IMG};
                    o[0] = sx; o[1] = sy; o[2] = csx - sx; o[3] = csy - sy; o[4] = scale;
                }
            }
        }
    }
    geom[row] = g;
    status[row] = st;
    if (info)
        for (int a = 0; a < 5; ++a) info[row * 5 + a] = o[a];
}

// three double planes [3][n] and two int planes [n] for n = max(rows, 1), packed: 80 bytes per row, no 256-byte rounding
struct TrackOffs { size_t box, interp, med, valid, next, total; };
TrackOffs track_layout(int n_total) {
    const size_t n = n_total > 0 ? n_total : 1;
    WsCarver c;
    return {c.take(24 * n, 8), c.take(24 * n, 8), c.take(24 * n, 8), c.take(4 * n, 4), c.take(4 * n, 4), c.total()};   // (braces: left to right)
}
// the workspace check and carve of hmmr_track_bbox and hmmr_track_smooth
struct Layout { double *box, *interp, *med; int *valid, *next; };
int carve(const char* who, char* ws, size_t ws_bytes, int n_total, Layout* out) {
    const TrackOffs l = track_layout(n_total);
    HMMR_REQUIRE(ws_bytes >= l.total, "%s: workspace of %zu bytes, need %zu", who, ws_bytes, l.total);
    *out = Layout{(double*)(ws + l.box), (double*)(ws + l.interp), (double*)(ws + l.med), (int*)(ws + l.valid), (int*)(ws + l.next)};
    return 0;
}

// offsets: n_tracks + 1 non-decreasing row numbers, the first >= 0, the last within what 32-bit element indices can address
int check_offsets(const char* who, const int32_t* offsets, int n_tracks) {
    HMMR_REQUIRE(offsets, "%s: null offsets", who);
    HMMR_REQUIRE(n_tracks >= 1, "%s: n_tracks = %d, need at least one track", who, n_tracks);
    HMMR_REQUIRE(offsets[0] >= 0, "%s: offsets[0] = %d is negative", who, offsets[0]);
    for (int t = 0; t < n_tracks; ++t)
        HMMR_REQUIRE(offsets[t + 1] >= offsets[t], "%s: offsets are not monotone (offsets[%d] = %d > offsets[%d] = %d)", who, t, offsets[t],
                     t + 1, offsets[t + 1]);
    HMMR_REQUIRE(offsets[n_tracks] <= HMMR_TRACK_MAX_ROWS, "%s: %d rows, at most %d", who, offsets[n_tracks], HMMR_TRACK_MAX_ROWS);
    return 0;
}

Chunk chunk_at(const int32_t* offsets, int n_tracks, int t0, int& longest) {
    Chunk c;
    c.n = n_tracks - t0 < TRACK_CHUNK ? n_tracks - t0 : TRACK_CHUNK;
    longest = 0;
    for (int t = 0; t <= TRACK_CHUNK; ++t) c.off[t] = offsets[t0 + (t < c.n ? t : c.n)];
    for (int t = 0; t < c.n; ++t) longest = c.off[t + 1] - c.off[t] > longest ? c.off[t + 1] - c.off[t] : longest;
    return c;
}

int check_filters(const char* who, int kernel_size, const double* gauss_w, int gauss_radius, Weights& g) {
    HMMR_REQUIRE(kernel_size >= 1 && kernel_size <= HMMR_TRACK_MAX_KERNEL && (kernel_size & 1),
                 "%s: kernel_size = %d, need an odd size in [1, %d]", who, kernel_size, HMMR_TRACK_MAX_KERNEL);
    HMMR_REQUIRE(gauss_radius >= 0 && gauss_radius <= HMMR_TRACK_MAX_RADIUS, "%s: gauss_radius = %d, need a radius in [0, %d]", who,
                 gauss_radius, HMMR_TRACK_MAX_RADIUS);
    HMMR_REQUIRE(gauss_w, "%s: null gauss_w", who);
    g.radius = gauss_radius;
    for (int j = 0; j <= HMMR_TRACK_MAX_RADIUS; ++j) g.w[j] = j <= gauss_radius ? gauss_w[j] : 0.;
    return 0;
}

// median then Gaussian over `in` (rows [start, end) of each track, or all of them with range == NULL) -> out
int smooth(const int32_t* offsets, int n_tracks, const int* range, const double* in, double* med, int kernel_size, const Weights& g,
           double* out, hipStream_t stream) {
    for (int t0 = 0; t0 < n_tracks; t0 += TRACK_CHUNK) {
        int longest;
        const Chunk c = chunk_at(offsets, n_tracks, t0, longest);
        if (!longest) continue;
        const dim3 grid((unsigned)((3ll * longest + TRACK_TILE - 1) / TRACK_TILE), (unsigned)c.n);
        hipLaunchKernelGGL(track_median_kernel, grid, dim3(TRACK_TILE), 0, stream, c, t0, range, in, kernel_size, med);
        HMMR_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(track_gauss_kernel, grid, dim3(TRACK_TILE), 0, stream, c, t0, range, (const double*)med, g, out);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
}  // namespace

extern "C" size_t hmmr_track_workspace_bytes(int n_total, int n_tracks) {
    if (n_total < 0 || n_total > HMMR_TRACK_MAX_ROWS || n_tracks < 1) return 0;
    return track_layout(n_total).total;
}

extern "C" int hmmr_track_bbox(const double* kps, const unsigned char* present, const int32_t* offsets, int n_tracks, int k,
                               double vis_thresh, int kernel_size, const double* gauss_w, int gauss_radius, double* bbox_raw,
                               double* bbox_smooth, int32_t* range, void* ws, size_t ws_bytes, void* stream_) {
    const char* who = "hmmr_track_bbox";
    hipStream_t stream = (hipStream_t)stream_;
    HMMR_REQUIRE(kps && present && bbox_smooth && range && ws, "%s: null argument (kps, present, bbox_smooth, range and ws are needed)", who);
    if (check_offsets(who, offsets, n_tracks)) return -1;
    HMMR_REQUIRE(k >= 1 && k <= HMMR_TRACK_MAX_KPS, "%s: k = %d, need 1 <= k <= %d", who, k, HMMR_TRACK_MAX_KPS);
    Weights g;
    if (check_filters(who, kernel_size, gauss_w, gauss_radius, g)) return -1;
    const int row0 = offsets[0], n = offsets[n_tracks] - offsets[0];
    Layout l;
    if (carve(who, (char*)ws, ws_bytes, offsets[n_tracks], &l)) return -1;
    if (n > 0) {
        hipLaunchKernelGGL(track_box_kernel, dim3((unsigned)((n + TRACK_TILE - 1) / TRACK_TILE)), dim3(TRACK_TILE), 0, stream, kps, present,
                           row0, n, k, vis_thresh, l.box, l.valid);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    for (int t0 = 0; t0 < n_tracks; t0 += TRACK_CHUNK) {
        int longest;
        const Chunk c = chunk_at(offsets, n_tracks, t0, longest);
        hipLaunchKernelGGL(track_extent_kernel, dim3((unsigned)c.n), dim3(TRACK_TILE), 0, stream, c, t0, (const double*)l.box,
                           (const int*)l.valid, l.next, l.interp, bbox_raw, range);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return smooth(offsets, n_tracks, range, l.interp, l.med, kernel_size, g, bbox_smooth, stream);
}

extern "C" int hmmr_track_smooth(const double* params, const int32_t* offsets, int n_tracks, int kernel_size, const double* gauss_w,
                                 int gauss_radius, double* out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "hmmr_track_smooth";
    HMMR_REQUIRE(params && out && ws, "%s: null argument (params, out and ws are needed)", who);
    if (check_offsets(who, offsets, n_tracks)) return -1;
    Weights g;
    if (check_filters(who, kernel_size, gauss_w, gauss_radius, g)) return -1;
    Layout l;
    if (carve(who, (char*)ws, ws_bytes, offsets[n_tracks], &l)) return -1;
    return smooth(offsets, n_tracks, nullptr, params, l.med, kernel_size, g, out, (hipStream_t)stream);
}

extern "C" int hmmr_track_crop_geom(const double* bbox_smooth, const int32_t* offsets, const int32_t* range, int n_tracks, int h, int w,
                                    int32_t* geom, double* info, int32_t* status, void* stream) {
    const char* who = "hmmr_track_crop_geom";
    HMMR_REQUIRE(bbox_smooth && geom && status, "%s: null argument (bbox_smooth, geom and status are needed)", who);
    if (check_offsets(who, offsets, n_tracks)) return -1;
    HMMR_REQUIRE(h >= 1 && w >= 1, "%s: frame of %d x %d, need h >= 1 and w >= 1", who, h, w);
    for (int t0 = 0; t0 < n_tracks; t0 += TRACK_CHUNK) {
        int longest;
        const Chunk c = chunk_at(offsets, n_tracks, t0, longest);
        if (!longest) continue;
        hipLaunchKernelGGL(track_geom_kernel, dim3((unsigned)((longest + TRACK_TILE - 1) / TRACK_TILE), (unsigned)c.n), dim3(TRACK_TILE), 0,
                           (hipStream_t)stream, c, t0, range, bbox_smooth, h, w, (int4*)geom, info, status);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
