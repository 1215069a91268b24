// The two kernels every backward of the tail is made of (csrc/ief_grad.hip, csrc/movie_grad.hip): the fp32-MFMA contraction
// and the double-precision column sum, each stated once.
#pragma once
#include "common.h"
#include "hmmr_hip.h"

// ---------------------------------------------------------------------------------------------------------------- the contraction
// The operands, in one of two forms (the kernel's template argument OPS).  MmPtrs: pointer tables, grid z = problem of a grouped launch, a
// problem whose c is NULL is skipped (the IEF's delta regressors).  MmOne: one problem, no table, no skip (f_movie): its kernels keep the
// scalar prologue of a plain argument list -- through the tables a launch fetches and tests the problem's pointer before its other
// arguments, which measured 2-3 us per hmmr_hallucinator_bwd ("Stated once").
struct MmPtrs {
    const float* a[HMMR_MAX_REGRESSORS]; const float* b[HMMR_MAX_REGRESSORS]; float* c[HMMR_MAX_REGRESSORS];
    const float* res[HMMR_MAX_REGRESSORS]; const float* gate[HMMR_MAX_REGRESSORS];
    static constexpr bool TABLES = true;
    __device__ __forceinline__ const float* A() const { return a[blockIdx.z]; }
    __device__ __forceinline__ const float* B() const { return b[blockIdx.z]; }
    __device__ __forceinline__ float* C() const { return c[blockIdx.z]; }
    __device__ __forceinline__ const float* Res() const { return res[blockIdx.z]; }
    __device__ __forceinline__ const float* Gate() const { return gate[blockIdx.z]; }
};
struct MmOne {
    const float* a; const float* b; float* c; const float* res; const float* gate;
    static constexpr bool TABLES = false;
    __device__ __forceinline__ const float* A() const { return a; }
    __device__ __forceinline__ const float* B() const { return b; }
    __device__ __forceinline__ float* C() const { return c; }
    __device__ __forceinline__ const float* Res() const { return res; }
    __device__ __forceinline__ const float* Gate() const { return gate; }
};
// WINDOWED: `taps` = 1 or 3 filter taps, t = rows of a window, span = the values of k (A_T false) or of j (A_T true) one tap holds
struct MmWindow { int taps, span, t; };

// C[M][N] = sum_k A(i, k) * B(k, j)   (+ res[i][j]; then * (gate[i][j] > 0 ? gate_scale : 0)), on v_mfma_f32_32x32x2_f32.
//   WINDOWED false:  A(i, k) = A_T ? a[k][i] : a[i][k],  B(k, j) = b[k][j].
//   WINDOWED true, c0 = taps / 2:
//     A_T false (data gradient): K = taps * span.  k = tap * span + co:  A(i, k) = a[i + c0 - tap][co] if that row lies in i's window,
//                                B(k, j) = b[co][tap * span + j].
//     A_T true (weight gradient): N = taps * span.  j = tap * span + ci:  A(i, k) = a[k][i],  B(k, j) = b[k + tap - c0][ci] if that row
//                                lies in k's window.
// With ONE fp32 value per lane the B operand of this instruction is B[k = lane >> 5][j = lane & 31]: a coalesced read of a row of b as it
// lies in memory, so a data gradient dX = dY . W contracts over the ROWS of the untransposed bank -- no copy, no transposing stage -- and a
// weight gradient dW = d_a^T . x reads both operands by batch row.
// Workgroup = one (32 MI) x (32 NI) tile of C, wave w = slice w of the contraction (ks values each, a multiple of 16; a chunk of 16 lies
// inside one tap); the partial tiles are added in slice order, (((w0 + w1) + w2) + ...).  Lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; result register q of lane l is C[(q & 3) + 8 (q >> 2) + 4 (l >> 5)][l & 31].  The two values an MFMA takes
// need not be neighbours: step s of a chunk of 16 takes k0 + s (lanes 0..31) and k0 + 8 + s (lanes 32..63), so that with a row-major A
// (A_T false, K a multiple of 16) a lane reads its eight values as two 16-byte pieces.  Eight steps of operands are loaded while the
// MFMAs of the eight before them run (two register sets).  SETS = 2 sends the chunks of 16 to two accumulators in turn (half the length
// of a rounding chain, and no MFMA waits for the one before it), added once in front of the slices: it changes the order of the sums, so
// it is a template argument.  Every read is guarded by the operand's own extent and by the window; a guarded-out value is a zero
// operand.  No atomics.
// SCALED_GATE false: the gate lies at the output's row stride and passes v unscaled (ldg and gate_scale are not read).  v * 1.f would be
// the same number; the flag keeps the second set of row addresses and the multiplies out of f_movie's epilogues, which measured 1 % of
// hmmr_temporal_bwd ("Stated once").  The two spellings of an address below (k0 - tap * span + 8 * h written out; the
// unwindowed B row as k) are the ones each file's kernel had: other spellings of the same sums change the compiled loops.
template <class OPS, bool A_T, bool WINDOWED, bool SCALED_GATE, int SETS, int MI, int NI, int SLICES>
__global__ __launch_bounds__(64 * SLICES) void grad_mm_kernel(OPS p, int M, int N, int K, int lda, int ldb, int ldc, int ldg,
                                                              float gate_scale, MmWindow win) {
    static_assert((SLICES - 1) * MI * NI * 16 * 64 * 4 <= 64 * 1024, "the partial tiles must fit the static LDS limit");
    static_assert(SETS == 1 || SETS == 2, "one accumulator set, or two taken in turn");
    __shared__ float red[SLICES - 1][MI * NI][16][64];
    float* __restrict__ c = p.C();
    if (OPS::TABLES && !c) return;                      // (the whole workgroup: blockIdx is uniform)
    const float* __restrict__ a = p.A();
    const float* __restrict__ b = p.B();
    const int span = WINDOWED ? win.span : 1, t = WINDOWED ? win.t : 1, c0 = WINDOWED ? win.taps >> 1 : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.y * (32 * MI) + r, j0 = blockIdx.x * (32 * NI) + r;
    const int ks = ((K + SLICES - 1) / SLICES + 15) & ~15;
    const int kb = wave * ks, ke = min(K, kb + ks);
    f32x16 accs[SETS][MI][NI];
#pragma unroll
    for (int e = 0; e < SETS; ++e)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) accs[e][mi][ni][q] = 0.f;
    // what does not change along the contraction: the position of an A row in its window (data gradient), the tap of a B column (weight gradient)
    int it[MI], jtap[NI], jcol[NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) it[mi] = WINDOWED ? (i0 + 32 * mi) % t : 0;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int j = j0 + 32 * ni;
        jtap[ni] = (WINDOWED && A_T) ? j / span : 0;
        jcol[ni] = j - jtap[ni] * span;
    }
    float a0[8][MI], b0[8][NI], a1[8][MI], b1[8][NI];
    auto load = [&](float (&av)[8][MI], float (&bv)[8][NI], int k0) {
        const int tap = (WINDOWED && !A_T) ? k0 / span : 0, co = k0 - tap * span + 8 * h;      // the data gradient's tap: one per chunk of 16
        if (!A_T) {                                     // a lane's eight values are consecutive in its row: two 16-byte reads (K % 16 == 0)
            const int sh = c0 - tap;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int i = i0 + 32 * mi;
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
                if (k0 < ke && i < M && (!WINDOWED || (unsigned)(it[mi] + sh) < (unsigned)t)) {
                    const f32x4* q = (const f32x4*)(a + (long long)(i + sh) * lda + k0 - tap * span + 8 * h);
                    lo = q[0]; hi = q[1];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) { av[s][mi] = lo[s]; av[4 + s][mi] = hi[s]; }
            }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int k = k0 + 8 * h + s;
            const bool kok = k < ke;
            const int kt = (WINDOWED && A_T) ? k % t : 0;
            if (A_T) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int i = i0 + 32 * mi;
                    av[s][mi] = (kok && i < M) ? a[(long long)k * lda + i] : 0.f;
                }
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int j = j0 + 32 * ni;
                if (!A_T) bv[s][ni] = (kok && j < N) ? b[(long long)(WINDOWED ? co + s : k) * ldb + tap * span + j] : 0.f;
                else {
                    const int sh = jtap[ni] - c0;
                    bv[s][ni] = (kok && j < N && (!WINDOWED || (unsigned)(kt + sh) < (unsigned)t)) ? b[(long long)(k + sh) * ldb + jcol[ni]] : 0.f;
                }
            }
        }
    };
    auto mma = [&](const float (&av)[8][MI], const float (&bv)[8][NI], f32x16 (&acc)[MI][NI]) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][mi], bv[s][ni], acc[mi][ni], 0, 0, 0);
    };
    load(a0, b0, kb);
    for (int k0 = kb; k0 < ke; k0 += 32) {                  // (kb, ke and every branch below are the same for a whole wave)
        if (k0 + 16 < ke) load(a1, b1, k0 + 16);
        mma(a0, b0, accs[0]);
        if (k0 + 16 < ke) {
            if (k0 + 32 < ke) load(a0, b0, k0 + 32);
            mma(a1, b1, accs[SETS - 1]);
        }
    }
    f32x16 (&acc)[MI][NI] = accs[0];
    if (SETS == 2) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[mi][ni][q] += accs[SETS - 1][mi][ni][q];
    }
    if (wave) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int q = 0; q < 16; ++q) red[wave - 1][mi * NI + ni][q][lane] = acc[mi][ni][q];
    }
    __syncthreads();
    if (wave) return;
    const float* __restrict__ res = p.Res();
    const float* __restrict__ gate = p.Gate();
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int j = j0 + 32 * ni;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float v = acc[mi][ni][q];
#pragma unroll
                for (int w = 0; w < SLICES - 1; ++w) v += red[w][mi * NI + ni][q][lane];
                const int row = blockIdx.y * (32 * MI) + 32 * mi + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (row < M && j < N) {
                    if (res) v = res[(long long)row * ldc + j] + v;
                    if (gate) v = gate[(long long)row * (SCALED_GATE ? ldg : ldc) + j] > 0.f ? (SCALED_GATE ? v * gate_scale : v) : 0.f;
                    c[(long long)row * ldc + j] = v;
                }
            }
        }
}

// The data gradient (A_T false): 32 rows x 32 inputs per workgroup, the contraction over the layer's outputs in 8 slices -- the batch is a
// few hundred rows at most, so small tiles and the slices are what fills the chip.  The weight gradient (A_T true): 64 x 64 per workgroup
// (each operand value feeds two MFMAs; a tile lies inside one tap), 4 slices of the batch rows.  Both splits are fixed: they do not depend
// on the rows.
// `who` names the caller in the refusal of a row-major A the 16-byte reads cannot take (no shape of an entry point reaches it).
template <bool A_T, bool WINDOWED, bool SCALED_GATE, int SETS, class OPS>
static int grad_mm_launch(const char* who, const OPS& p, int nb, int M, int N, int K, int lda, int ldb, int ldc, int ldg, float gate_scale,
                          MmWindow win, hipStream_t s) {
    constexpr int MI = A_T ? 2 : 1, NI = A_T ? 2 : 1, SLICES = A_T ? 4 : 8;
    if (!A_T && (K % 16 || lda % 4)) { hmmr_set_error("%s: a row-major A needs K %% 16 == 0 and lda %% 4 == 0", who); return -2; }
    hipLaunchKernelGGL((grad_mm_kernel<OPS, A_T, WINDOWED, SCALED_GATE, SETS, MI, NI, SLICES>),
                       dim3((unsigned)((N + 32 * NI - 1) / (32 * NI)), (unsigned)((M + 32 * MI - 1) / (32 * MI)), (unsigned)nb), dim3(64 * SLICES), 0, s,
                       p, M, N, K, lda, ldb, ldc, ldg, gate_scale, win);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the column sum
// Its operands, in the same two forms: tables (grid y = problem, a NULL output is skipped; N columns at row stride lda), or one problem of
// WIDTH columns at row stride WIDTH, both known when it is compiled (N and lda are not read, by the kernel or by the launcher's grid).
struct CsPtrs {
    const float* a[HMMR_MAX_REGRESSORS]; float* out[HMMR_MAX_REGRESSORS];
    static constexpr bool TABLES = true;
    static constexpr int WIDTH = 0;
    __device__ __forceinline__ const float* A() const { return a[blockIdx.y]; }
    __device__ __forceinline__ float* Out() const { return out[blockIdx.y]; }
};
template <int W>
struct CsOne {
    const float* a; float* out;
    static constexpr bool TABLES = false;
    static constexpr int WIDTH = W;
    __device__ __forceinline__ const float* A() const { return a; }
    __device__ __forceinline__ float* Out() const { return out; }
};
// out[col] = sum over the K rows of a[K][lda], accumulated in double and rounded once: a plain fp32 chain over the rows loses log2(K) bits
// that a blocked sum (what the yardstick's fp32 autograd does) keeps -- 7 x E32 on the IEF's d_b3 at K = 480.  A workgroup owns 32 columns;
// thread (g, c) adds rows g, g + 8, g + 16, ... of column c in row order, and thread (0, c) adds the eight partial sums in g order: a
// fixed order for a given K.
template <class OPS>
__global__ __launch_bounds__(256) void grad_colsum_kernel(OPS p, int K, int N, int lda) {
    constexpr bool EVERY_COL = OPS::WIDTH > 0 && OPS::WIDTH % 32 == 0;      // (no column guard: every column of every workgroup exists)
    __shared__ double part[8][32];
    float* out = p.Out();
    if (OPS::TABLES && !out) return;                    // (the whole workgroup)
    const int n = OPS::WIDTH ? OPS::WIDTH : N, ld = OPS::WIDTH ? OPS::WIDTH : lda;
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + c;
    double v = 0.0;
    if (EVERY_COL || col < n) {
        const float* a = p.A() + col;
        for (int k = g; k < K; k += 8) v += (double)a[(long long)k * ld];
    }
    part[g][c] = v;
    __syncthreads();
    if (g || (!EVERY_COL && col >= n)) return;
    for (int q = 1; q < 8; ++q) v += part[q][c];
    out[col] = (float)v;
}
template <class OPS>
static int grad_colsum_launch(const OPS& p, int nb, int K, int N, int lda, hipStream_t s) {
    const int n = OPS::WIDTH ? OPS::WIDTH : N;          // (the grid follows the width the kernel was compiled for, whatever N says)
    hipLaunchKernelGGL(grad_colsum_kernel<OPS>, dim3((unsigned)((n + 31) / 32), (unsigned)nb), dim3(256), 0, s, p, K, N, lda);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
