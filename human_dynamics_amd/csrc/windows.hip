// The sliding-window scheme of Tester.predict_all_images (src/evaluation/tester.py:260-312) as two device copies, so that a caller
// without Python can run a video through the library (hmmr_predict_video, csrc/video.cpp):
//   gather  (tester.py:285-305)  the features of the zero-image-padded video -> windows of T slots every g frames;
//   keep    (tester.py:306-311)  the centre g slots of every window -> consecutive output rows, the rows beyond the video dropped.
// Both are pure copies: a wave moves 1 KiB of one row per instruction (16 bytes per lane, consecutive lanes consecutive pieces); a
// workgroup of four waves works on four rows at a time, so short rows (c = 8) still fill it.  HBM-bound: 8 bytes moved per float.
// Every offset is 64-bit (n * c passes 2^31 for long videos); the row -> (window, slot) division happens once per row, not per piece.
#include "common.h"
#include "hmmr_hip.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;
constexpr unsigned MAX_BLOCKS = 1u << 20;       // the row loop strides by the grid

// out row r = (window w0 + r / T, slot r % T): padded position p = w g + t holds phi[p - margin], or phi_zero outside the video
__global__ void __launch_bounds__(HMMR_WAVE * ROWS_PER_BLOCK)
gather_windows_kernel(const f32x4* __restrict__ phi, long long n, const f32x4* __restrict__ phi_zero, long long w0, long long rows,
                      int T, int margin, int g, int c4, f32x4* __restrict__ out) {
    for (long long r = (long long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.y; r < rows; r += (long long)gridDim.x * ROWS_PER_BLOCK) {
        const long long wl = r / T;
        const long long f = (w0 + wl) * g + (r - wl * T) - margin;
        const f32x4* src = (f >= 0 && f < n) ? phi + f * c4 : phi_zero;
        f32x4* dst = out + r * c4;
        for (int i = threadIdx.x; i < c4; i += HMMR_WAVE) dst[i] = src[i];
    }
}

// kept row r = (window w0 + r / g, centre slot r % g) is frame f = w0 g + r: strips[wl][margin + j] -> out + r ld_out, if f < n_total
__global__ void __launch_bounds__(HMMR_WAVE * ROWS_PER_BLOCK)
keep_rows_kernel(const f32x4* __restrict__ strips, long long rows, int T, int margin, int g, int c4, f32x4* __restrict__ out,
                 long long ld4) {
    for (long long r = (long long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.y; r < rows; r += (long long)gridDim.x * ROWS_PER_BLOCK) {
        const long long wl = r / g;
        const f32x4* src = strips + (wl * T + margin + (r - wl * g)) * c4;
        f32x4* dst = out + r * ld4;
        for (int i = threadIdx.x; i < c4; i += HMMR_WAVE) dst[i] = src[i];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline unsigned blocks_for(long long rows) {
    const long long b = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return (unsigned)(b < (long long)MAX_BLOCKS ? b : (long long)MAX_BLOCKS);
}

}  // namespace

extern "C" int hmmr_gather_windows(const float* phi, int n, const float* phi_zero, int w0, int n_windows, int T, int margin, int g,
                                   int c, float* out, void* stream) {
    HMMR_REQUIRE(n >= 0 && w0 >= 0 && n_windows >= 0, "hmmr_gather_windows: n=%d, w0=%d and n_windows=%d must not be negative", n, w0, n_windows);
    HMMR_REQUIRE(T >= 1 && margin >= 0 && g >= 1 && (long long)margin + g <= T,
                 "hmmr_gather_windows: bad window (T=%d, margin=%d, g=%d: need g >= 1 and margin + g <= T)", T, margin, g);
    HMMR_REQUIRE(c >= 4 && c % 4 == 0, "hmmr_gather_windows: c=%d must be a positive multiple of 4 (16-byte pieces)", c);
    if (n == 0 || n_windows == 0) return 0;
    HMMR_REQUIRE(phi && phi_zero && out, "hmmr_gather_windows: null argument");
    HMMR_REQUIRE(aligned16(phi) && aligned16(phi_zero) && aligned16(out), "hmmr_gather_windows: pointers must be 16-byte aligned");
    const long long rows = (long long)n_windows * T;
    hipLaunchKernelGGL(gather_windows_kernel, dim3(blocks_for(rows)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                       (const f32x4*)phi, (long long)n, (const f32x4*)phi_zero, (long long)w0, rows, T, margin, g, c / 4, (f32x4*)out);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hmmr_keep_rows(const float* strips, int w0, int n_windows, int T, int margin, int g, int c, int n_total, float* out,
                              int64_t ld_out, void* stream) {
    HMMR_REQUIRE(n_total >= 0 && w0 >= 0 && n_windows >= 0, "hmmr_keep_rows: n_total=%d, w0=%d and n_windows=%d must not be negative", n_total, w0,
                 n_windows);
    HMMR_REQUIRE(T >= 1 && margin >= 0 && g >= 1 && (long long)margin + g <= T,
                 "hmmr_keep_rows: bad window (T=%d, margin=%d, g=%d: need g >= 1 and margin + g <= T)", T, margin, g);
    HMMR_REQUIRE(c >= 4 && c % 4 == 0 && ld_out >= c && ld_out % 4 == 0,
                 "hmmr_keep_rows: c=%d and ld_out=%lld must be multiples of 4 with ld_out >= c (16-byte pieces)", c, (long long)ld_out);
    // frames [w0 g, min(n_total, (w0 + n_windows) g)) are these windows' to write
    const long long f0 = (long long)w0 * g, f1 = (long long)(w0 + (long long)n_windows) * g;
    const long long rows = (f1 < n_total ? f1 : (long long)n_total) - f0;
    if (n_total == 0 || n_windows == 0 || rows <= 0) return 0;
    HMMR_REQUIRE(strips && out, "hmmr_keep_rows: null argument");
    HMMR_REQUIRE(aligned16(strips) && aligned16(out), "hmmr_keep_rows: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(keep_rows_kernel, dim3(blocks_for(rows)), dim3(HMMR_WAVE, ROWS_PER_BLOCK), 0, (hipStream_t)stream,
                       (const f32x4*)strips, rows, T, margin, g, c / 4, (f32x4*)out, (long long)(ld_out / 4));
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
