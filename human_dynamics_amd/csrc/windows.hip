// The sliding-window scheme of Tester.predict_all_images (src/evaluation/tester.py:260-312) as two device copies, each for any number of
// tracks laid end to end along the frame axis (include/hmmr_hip.h: the ragged rule), so that a caller without Python can run a video, or
// every tracked person of one, through the library (hmmr_predict_video, hmmr_predict_tracks: csrc/video.cpp):
//   gather  (tester.py:285-305)  the features of every track, each padded with the zero image -> windows of T slots every g frames;
//   keep    (tester.py:306-311)  the centre g slots of every window -> consecutive output rows, the rows beyond a track's end dropped.
// The tracks' offsets and window bases reach the kernels as arguments, 64 tracks per launch.  hmmr_gather_windows / hmmr_keep_rows launch
// the same two kernels with the one-track table {0, n}; what they accept beyond the ragged entries is said at each.
// Both are pure copies: a wave moves 1 KiB of one row per instruction (16 bytes per lane, consecutive lanes consecutive pieces); a
// workgroup of four waves works on four rows at a time, so short rows (c = 8) still fill it.  HBM-bound: 8 bytes moved per float.
// Every offset is 64-bit (n * c passes 2^31 for long videos); the row -> (window, slot) division happens once per row, not per piece.
#include "common.h"
#include "hmmr_hip.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;
constexpr unsigned MAX_BLOCKS = 1u << 20;       // the row loop strides by the grid

constexpr int TRACK_CHUNK = 64;                 // tracks per launch: their offsets and window bases are kernel arguments (as csrc/track.hip)
struct TrackTable { int n; int off[TRACK_CHUNK + 1]; int win[TRACK_CHUNK + 1]; };      // absolute frames / absolute windows; entries past n repeat the last

// A row belongs to one wave (threadIdx.y), so its number is wave-uniform; saying so keeps the track search in scalar registers, the
// table in the kernel-argument segment (scalar loads, no scratch copy) and the lane loop below free of it.
__device__ __forceinline__ int wave_row() { return __builtin_amdgcn_readfirstlane((int)threadIdx.y); }
// the k in [0, n) with edge[k] <= v < edge[k + 1], for edge[0] <= v < edge[n]; entries that repeat (empty tracks) are stepped over
__device__ __forceinline__ int track_of(const int* edge, int n, int v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edge[mid + 1] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// out row r = (global window first + r / T, slot r % T): padded position lw g + t of the owner holds its frame lw g + t - margin, or phi_zero
// outside the track.  The windows are owned by tracks of tt -- or tt has ONE track and they may lie past its last (hmmr_gather_windows;
// every slot from frame n on is phi_zero).  So the window number is 64-bit, and the search gets its low half: exact whenever the search
// has to choose (several tracks: w < tt.win[tt.n]), and with one track it runs no step.
__global__ void __launch_bounds__(HMMR_WAVE * ROWS_PER_BLOCK)
gather_windows_tracks_kernel(const f32x4* __restrict__ phi, const f32x4* __restrict__ phi_zero, TrackTable tt, long long first, long long rows,
                             int T, int margin, int g, int c4, f32x4* __restrict__ out) {
    for (long long r = (long long)blockIdx.x * ROWS_PER_BLOCK + wave_row(); r < rows; r += (long long)gridDim.x * ROWS_PER_BLOCK) {
        const long long wl = r / T, w = first + wl;
        const int t = (int)(r - wl * T);
        const int k = track_of(tt.win, tt.n, (int)w);
        const long long f = (w - tt.win[k]) * g + t - margin;
        const f32x4* src = (f >= 0 && f < tt.off[k + 1] - tt.off[k]) ? phi + (tt.off[k] + f) * c4 : phi_zero;
        f32x4* dst = out + r * c4;
        for (int i = threadIdx.x; i < c4; i += HMMR_WAVE) dst[i] = src[i];
    }
}

// out row r is frame first + r, one of tt's: frame f of track k sits in local window f / g at slot margin + f % g; strips starts at global window w0
__global__ void __launch_bounds__(HMMR_WAVE * ROWS_PER_BLOCK)
keep_rows_tracks_kernel(const f32x4* __restrict__ strips, TrackTable tt, int first, int rows, int w0, int T, int margin, int g, int c4,
                        f32x4* __restrict__ out, long long ld4) {
    for (long long r = (long long)blockIdx.x * ROWS_PER_BLOCK + wave_row(); r < rows; r += (long long)gridDim.x * ROWS_PER_BLOCK) {
        const int frame = first + (int)r;
        const int k = track_of(tt.off, tt.n, frame);
        const int f = frame - tt.off[k], lw = f / g;
        const f32x4* src = strips + ((long long)(tt.win[k] + lw - w0) * T + margin + (f - lw * g)) * c4;
        f32x4* dst = out + r * ld4;
        for (int i = threadIdx.x; i < c4; i += HMMR_WAVE) dst[i] = src[i];
    }
}

// tracks [t0, t0 + n) of the table; base = the global number of track t0's first window
TrackTable table_at(const int32_t* off, int n_tracks, int t0, int g, int base) {
    TrackTable tt;
    tt.n = n_tracks - t0 < TRACK_CHUNK ? n_tracks - t0 : TRACK_CHUNK;
    tt.off[0] = off[t0];
    tt.win[0] = base;
    for (int t = 1; t <= TRACK_CHUNK; ++t) {
        const int k = t0 + (t < tt.n ? t : tt.n);
        tt.off[t] = off[k];
        tt.win[t] = tt.win[t - 1] + (int)(((long long)tt.off[t] - tt.off[t - 1] + g - 1) / g);
    }
    return tt;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline unsigned blocks_for(long long rows) {
    const long long b = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return (unsigned)(b < (long long)MAX_BLOCKS ? b : (long long)MAX_BLOCKS);
}

// The refusals the four entry points share, under the caller's name: the window, c and -- keep only, gather passes null -- ld_out; then,
// if there is work (a call with none may pass null pointers), null and misaligned pointers.  `zero` is the gather's second source; keep
// passes its one source twice.
int check_copy(const char* who, int T, int margin, int g, int c, const int64_t* ld_out, bool work, const void* src, const void* zero,
               const void* out) {
    HMMR_REQUIRE(T >= 1 && margin >= 0 && g >= 1 && (long long)margin + g <= T,
                 "%s: bad window (T=%d, margin=%d, g=%d: need g >= 1 and margin + g <= T)", who, T, margin, g);
    const bool pieces = c >= 4 && c % 4 == 0;
    if (!ld_out) HMMR_REQUIRE(pieces, "%s: c=%d must be a positive multiple of 4 (16-byte pieces)", who, c);
    else HMMR_REQUIRE(pieces && *ld_out >= c && *ld_out % 4 == 0,
                      "%s: c=%d and ld_out=%lld must be multiples of 4 with ld_out >= c (16-byte pieces)", who, c, (long long)*ld_out);
    if (!work) return 0;
    HMMR_REQUIRE(src && zero && out, "%s: null argument", who);
    HMMR_REQUIRE(aligned16(src) && aligned16(zero) && aligned16(out), "%s: pointers must be 16-byte aligned", who);
    return 0;
}

}  // namespace

// One video: the one-track table {0, n}.  Any w0, n_windows >= 0 is a range here -- the reference runs count * batch_size windows, past
// ceil(n / g) -- so nothing is refused or clipped at the track's last window: the whole range is launched against the single track.
extern "C" int hmmr_gather_windows(const float* phi, int n, const float* phi_zero, int w0, int n_windows, int T, int margin, int g,
                                   int c, float* out, void* stream) {
    const char* who = "hmmr_gather_windows";
    HMMR_REQUIRE(n >= 0 && w0 >= 0 && n_windows >= 0, "%s: n=%d, w0=%d and n_windows=%d must not be negative", who, n, w0, n_windows);
    const bool work = n != 0 && n_windows != 0;
    if (check_copy(who, T, margin, g, c, nullptr, work, phi, phi_zero, out)) return -1;
    if (!work) return 0;
    const int32_t off[2] = {0, n};
    const long long rows = (long long)n_windows * T;
    hipLaunchKernelGGL(gather_windows_tracks_kernel, dim3(blocks_for(rows)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                       (const f32x4*)phi, (const f32x4*)phi_zero, table_at(off, 1, 0, g, 0), (long long)w0, rows, T, margin, g, c / 4, (f32x4*)out);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// One video: the windows' rows are clipped at n_total, and a range that keeps no frame (w0 g >= n_total) is no refusal: 0, nothing launched.
extern "C" int hmmr_keep_rows(const float* strips, int w0, int n_windows, int T, int margin, int g, int c, int n_total, float* out,
                              int64_t ld_out, void* stream) {
    const char* who = "hmmr_keep_rows";
    HMMR_REQUIRE(n_total >= 0 && w0 >= 0 && n_windows >= 0, "%s: n_total=%d, w0=%d and n_windows=%d must not be negative", who, n_total, w0, n_windows);
    // frames [w0 g, min(n_total, (w0 + n_windows) g)) are these windows' to write
    const long long f0 = (long long)w0 * g, f1 = (long long)(w0 + (long long)n_windows) * g;
    const long long rows = (f1 < n_total ? f1 : (long long)n_total) - f0;
    const bool work = n_total != 0 && n_windows != 0 && rows > 0;
    if (check_copy(who, T, margin, g, c, &ld_out, work, strips, strips, out)) return -1;
    if (!work) return 0;
    const int32_t off[2] = {0, n_total};
    hipLaunchKernelGGL(keep_rows_tracks_kernel, dim3(blocks_for(rows)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                       (const f32x4*)strips, table_at(off, 1, 0, g, 0), (int)f0, (int)rows, w0, T, margin, g, c / 4, (f32x4*)out,
                       (long long)(ld_out / 4));      // (0 <= f0 < f0 + rows <= n_total: ints)
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

int hmmr_tracks_check_offsets(const char* who, const int32_t* off, int n_tracks);       // csrc/video_plan.cpp

extern "C" int hmmr_gather_windows_tracks(const float* phi, const float* phi_zero, const int32_t* track_offsets, int n_tracks, int w0,
                                          int n_windows, int T, int margin, int g, int c, float* out, void* stream) {
    const char* who = "hmmr_gather_windows_tracks";
    if (hmmr_tracks_check_offsets(who, track_offsets, n_tracks)) return -1;
    HMMR_REQUIRE(w0 >= 0 && n_windows >= 0, "%s: w0=%d and n_windows=%d must not be negative", who, w0, n_windows);
    if (check_copy(who, T, margin, g, c, nullptr, n_windows != 0, phi, phi_zero, out)) return -1;
    if (n_windows == 0) return 0;
    const long long w1 = (long long)w0 + n_windows;
    {   // the range lies inside the numbering (checked before the first launch: a later chunk cannot refuse)
        long long total = 0;
        for (int k = 0; k < n_tracks; ++k) total += ((long long)track_offsets[k + 1] - track_offsets[k] + g - 1) / g;
        HMMR_REQUIRE(w1 <= total, "%s: windows [%d, %lld) leave the %lld windows of these tracks", who, w0, w1, total);
    }
    int base = 0;
    for (int t0 = 0; t0 < n_tracks && base < w1; t0 += TRACK_CHUNK) {
        const TrackTable tt = table_at(track_offsets, n_tracks, t0, g, base);
        base = tt.win[tt.n];
        const long long a = w0 > tt.win[0] ? w0 : tt.win[0], b = w1 < base ? w1 : base;      // this chunk's share of the range
        if (a >= b) continue;
        const long long rows = (b - a) * T;
        hipLaunchKernelGGL(gather_windows_tracks_kernel, dim3(blocks_for(rows)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                           (const f32x4*)phi, (const f32x4*)phi_zero, tt, a, rows, T, margin, g, c / 4, (f32x4*)out + (a - w0) * T * (c / 4));
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int hmmr_keep_rows_tracks(const float* strips, const int32_t* track_offsets, int n_tracks, int w0, int n_windows, int T,
                                     int margin, int g, int c, float* out, int64_t ld_out, void* stream) {
    const char* who = "hmmr_keep_rows_tracks";
    if (hmmr_tracks_check_offsets(who, track_offsets, n_tracks)) return -1;
    HMMR_REQUIRE(w0 >= 0 && n_windows >= 0, "%s: w0=%d and n_windows=%d must not be negative", who, w0, n_windows);
    if (check_copy(who, T, margin, g, c, &ld_out, n_windows != 0, strips, strips, out)) return -1;
    if (n_windows == 0) return 0;
    int o0, keep;
    if (hmmr_tracks_window_rows(track_offsets, n_tracks, g, w0, n_windows, &o0, &keep)) return -1;      // refuses a range that leaves the numbering
    const long long o1 = (long long)o0 + keep;
    int base = 0;
    for (int t0 = 0; t0 < n_tracks && track_offsets[t0] < o1; t0 += TRACK_CHUNK) {
        const TrackTable tt = table_at(track_offsets, n_tracks, t0, g, base);
        base = tt.win[tt.n];
        const long long a = o0 > tt.off[0] ? o0 : tt.off[0], b = o1 < tt.off[tt.n] ? o1 : tt.off[tt.n];      // this chunk's share of the rows
        if (a >= b) continue;
        hipLaunchKernelGGL(keep_rows_tracks_kernel, dim3(blocks_for(b - a)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                           (const f32x4*)strips, tt, (int)a, (int)(b - a), w0, T, margin, g, c / 4, (f32x4*)out + (a - o0) * (ld_out / 4),
                           (long long)(ld_out / 4));
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
