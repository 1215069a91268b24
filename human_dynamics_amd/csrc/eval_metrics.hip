// On-device evaluation metrics of src/evaluation/eval_util.py:
//   compute_error_3d     per frame: MPJPE after pelvis alignment and after Procrustes alignment
//                        (eval_util.py:30-60, align_by_pelvis :158-174, compute_similarity_transform :177-232)
//   compute_error_accel  per interior frame: mean || (X[i-1]-2X[i]+X[i+1])_pred - (...)_gt ||   (:63-94)
//   compute_accel        per interior frame: mean || X[i-1]-2X[i]+X[i+1] ||                     (:14-27)
//   compute_error_verts  per frame: mean vertex distance                                        (:140-155)
// so the joints / vertices that the SMPL stage leaves in HBM can be scored without a PCIe trip.
// Inputs fp32, arithmetic fp64 (one lane per frame for the Procrustes problem: the right singular vectors of K by
// cyclic Jacobi on K^T K, the left ones from K itself; a few hundred flops per frame, the kernel is latency-bound).
#include "common.h"
#include "hmmr_hip.h"
#include "so3.h"

namespace {
constexpr int MAXK = 32;

__device__ void jacobi_eig3(double A[3][3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {              // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {              // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {              // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

__device__ double det3(const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// one lane per frame
__global__ void eval_joints_kernel(const float* __restrict__ gt, long long ld_gt, const float* __restrict__ pred,
                                   long long ld_pred, int n, int k, int left_id, int right_id,
                                   float* __restrict__ mpjpe, float* __restrict__ pa_mpjpe) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    double G[MAXK][3], P[MAXK][3];
    const float* g = gt + (long long)f * ld_gt;
    const float* p = pred + (long long)f * ld_pred;
    double pg[3], pp[3];
    for (int c = 0; c < 3; ++c) {
        pg[c] = ((double)g[left_id * 3 + c] + (double)g[right_id * 3 + c]) / 2.0;
        pp[c] = ((double)p[left_id * 3 + c] + (double)p[right_id * 3 + c]) / 2.0;
    }
    double err = 0.0;
    for (int j = 0; j < k; ++j) {
        double d2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            G[j][c] = (double)g[j * 3 + c] - pg[c];
            P[j][c] = (double)p[j * 3 + c] - pp[c];
            const double d = G[j][c] - P[j][c];
            d2 += d * d;
        }
        err += sqrt(d2);
    }
    mpjpe[f] = (float)(err / k);
    // ---- compute_similarity_transform(S1 = pred, S2 = gt)
    double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
    for (int j = 0; j < k; ++j)
        for (int c = 0; c < 3; ++c) { mu1[c] += P[j][c]; mu2[c] += G[j][c]; }
    for (int c = 0; c < 3; ++c) { mu1[c] /= k; mu2[c] /= k; }
    double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
    for (int j = 0; j < k; ++j) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) { x1[c] = P[j][c] - mu1[c]; x2[c] = G[j][c] - mu2[c]; var1 += x1[c] * x1[c]; }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) K[a][b] += x1[a] * x2[b];              // K = X1 X2^T
    }
    // K = U S V^T.  Eigen-decompose K^T K = V S^2 V^T; the left vectors are the DIRECTIONS of K V, taken from K itself.
    // (The singular values of the squared form carry an error of 1e-16 s0^2 / s: dividing K v by them, and deciding the
    // rank by them, left a third column of noise whenever the smallest one vanishes without being an exact zero -- a
    // planar gt or pred in general position.)  u0 = K v0 / |K v0|, u1 = the part of K v1 orthogonal to u0, u2 = u0 x u1:
    // U is orthogonal whatever the rank, as LAPACK's is, and the sign in Z below makes R the proper rotation.
    double KtK[3][3], V[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) KtK[a][b] = K[0][a] * K[0][b] + K[1][a] * K[1][b] + K[2][a] * K[2][b];
    jacobi_eig3(KtK, V);
    int ord[3] = {0, 1, 2};                                                      // descending singular values
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (KtK[ord[b]][ord[b]] > KtK[ord[a]][ord[a]]) { const int t = ord[a]; ord[a] = ord[b]; ord[b] = t; }
    double Vs[3][3], U[3][3];
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < 3; ++r) Vs[r][i] = V[r][ord[i]];
    for (int i = 0; i < 2; ++i)
        for (int r = 0; r < 3; ++r) U[r][i] = K[r][0] * Vs[0][i] + K[r][1] * Vs[1][i] + K[r][2] * Vs[2][i];
    const double n0 = sqrt(U[0][0] * U[0][0] + U[1][0] * U[1][0] + U[2][0] * U[2][0]);   // = s0
    for (int r = 0; r < 3; ++r) U[r][0] = n0 > 0.0 ? U[r][0] / n0 : (r == 0 ? 1.0 : 0.0);   // K == 0: any R (scale is 0 or 0 / 0)
    const double d01 = U[0][0] * U[0][1] + U[1][0] * U[1][1] + U[2][0] * U[2][1];
    for (int r = 0; r < 3; ++r) U[r][1] -= d01 * U[r][0];
    double n1 = sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1]);
    if (!(n1 > 1e-7 * n0)) {       // rank one at the precision of the squared form's vectors: any unit vector across u0
        const int e = fabs(U[0][0]) <= fabs(U[1][0]) ? (fabs(U[0][0]) <= fabs(U[2][0]) ? 0 : 2)
                                                     : (fabs(U[1][0]) <= fabs(U[2][0]) ? 1 : 2);
        for (int r = 0; r < 3; ++r) U[r][1] = (r == e ? 1.0 : 0.0) - U[e][0] * U[r][0];
        n1 = sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1]);
    }
    for (int r = 0; r < 3; ++r) U[r][1] /= n1;
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    // R = V Z U^T with Z = diag(1, 1, sign(det(U V^T)))
    double UVt[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) UVt[a][b] = U[a][0] * Vs[b][0] + U[a][1] * Vs[b][1] + U[a][2] * Vs[b][2];
    const double dz = det3(UVt) < 0 ? -1.0 : 1.0;
    double R[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[a][b] = Vs[a][0] * U[b][0] + Vs[a][1] * U[b][1] + dz * Vs[a][2] * U[b][2];
    double trRK = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) trRK += R[a][b] * K[b][a];
    const double scale = trRK / var1;
    double t[3];
    for (int a = 0; a < 3; ++a) t[a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
    double epa = 0.0;
    for (int j = 0; j < k; ++j) {
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double h = scale * (R[a][0] * P[j][0] + R[a][1] * P[j][1] + R[a][2] * P[j][2]) + t[a];
            const double d = G[j][a] - h;
            d2 += d * d;
        }
        epa += sqrt(d2);
    }
    pa_mpjpe[f] = (float)(epa / k);
}

// one lane per interior frame i in [0, n-2): second difference centred on frame i+1
__global__ void eval_accel_kernel(const float* __restrict__ gt, long long ld_gt, const float* __restrict__ pred,
                                  long long ld_pred, int n, int k, float* __restrict__ accel_pred,
                                  float* __restrict__ accel_err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 2) return;
    double sa = 0.0, se = 0.0;
    for (int j = 0; j < k; ++j) {
        double na = 0.0, ne = 0.0;
        for (int c = 0; c < 3; ++c) {
            const long long o = (long long)i * ld_pred + j * 3 + c, s = ld_pred;
            const double ap = (double)pred[o] - 2.0 * (double)pred[o + s] + (double)pred[o + 2 * s];
            na += ap * ap;
            if (gt) {
                const long long og = (long long)i * ld_gt + j * 3 + c;
                const double ag = (double)gt[og] - 2.0 * (double)gt[og + ld_gt] + (double)gt[og + 2 * ld_gt];
                ne += (ap - ag) * (ap - ag);
            }
        }
        sa += sqrt(na); se += sqrt(ne);
    }
    if (accel_pred) accel_pred[i] = (float)(sa / k);
    if (accel_err && gt) accel_err[i] = (float)(se / k);
}

// one workgroup per frame: mean over vertices of || gt - pred ||
__global__ __launch_bounds__(256) void eval_verts_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         int nv, long long ld_gt, long long ld_pred,
                                                         float* __restrict__ out) {
    __shared__ double red[4];
    const float* g = gt + (long long)blockIdx.x * ld_gt;
    const float* p = pred + (long long)blockIdx.x * ld_pred;
    double s = 0.0;
    for (int v = threadIdx.x; v < nv; v += 256) {
        const double dx = (double)g[v * 3] - (double)p[v * 3], dy = (double)g[v * 3 + 1] - (double)p[v * 3 + 1],
                     dz = (double)g[v * 3 + 2] - (double)p[v * 3 + 2];
        s += sqrt(dx * dx + dy * dy + dz * dz);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)((red[0] + red[1] + red[2] + red[3]) / nv);
}
// compute_error_kp + compute_opt_cam_with_vis (eval_util.py:97-137, :235-260), one lane per frame.  gt row: k x (x, y, vis), pred
// row: k x (x, y); three passes over the (cached) rows instead of per-lane arrays.  img_size > 0: the prediction is brought to
// image space first, (x + 1) * 0.5 * img_size as three separately rounded fp32 operations (eval.py:131 does it in float32).
__device__ __forceinline__ double kp_pred_px(const float* p, float img_size) {
    const float v = *p;
    return (double)(img_size > 0.f ? __fmul_rn(__fmul_rn(__fadd_rn(v, 1.0f), 0.5f), img_size) : v);
}

__global__ void eval_kps_kernel(const float* __restrict__ gt, long long ld_gt, const float* __restrict__ pred, long long ld_pred,
                                int n, int k, double alpha, int min_visible, float img_size, float* __restrict__ err_kp,
                                float* __restrict__ err_kp_pa, float* __restrict__ pck, float* __restrict__ cam) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const float* g = gt + (long long)f * ld_gt;
    const float* p = pred + (long long)f * ld_pred;
    const float qnan = __builtin_nanf("");
    // pass 1: visible count, sums of the zeroed-out coordinates, keypoint error
    int nv = 0;
    double s1[2] = {0, 0}, s2[2] = {0, 0}, ekp = 0.0;
    for (int j = 0; j < k; ++j) {
        if (g[j * 3 + 2] == 0.f) continue;                          // vis = kp_gt[:, 2].astype(bool)
        const double px = kp_pred_px(p + j * 2, img_size), py = kp_pred_px(p + j * 2 + 1, img_size);
        const double gx = (double)g[j * 3], gy = (double)g[j * 3 + 1];
        ++nv;
        s1[0] += px; s1[1] += py; s2[0] += gx; s2[1] += gy;
        ekp += sqrt((gx - px) * (gx - px) + (gy - py) * (gy - py));
    }
    if (nv == 0 || nv < min_visible) {                              // "use nan to signify not visible": a result, no flag
        if (err_kp) err_kp[f] = qnan;
        if (err_kp_pa) err_kp_pa[f] = qnan;
        if (pck) pck[f] = qnan;
        if (cam) { cam[f * 3] = qnan; cam[f * 3 + 1] = qnan; cam[f * 3 + 2] = qnan; }
        return;
    }
    if (err_kp) err_kp[f] = (float)(ekp / nv);
    if (!err_kp_pa && !pck && !cam) return;
    const double mu1[2] = {s1[0] / nv, s1[1] / nv}, mu2[2] = {s2[0] / nv, s2[1] / nv};
    // pass 2: x^T x and x^T y of the centred visible points
    double xx[2][2] = {{0, 0}, {0, 0}}, xy[2][2] = {{0, 0}, {0, 0}};
    for (int j = 0; j < k; ++j) {
        if (g[j * 3 + 2] == 0.f) continue;
        const double x[2] = {kp_pred_px(p + j * 2, img_size) - mu1[0], kp_pred_px(p + j * 2 + 1, img_size) - mu1[1]};
        const double y[2] = {(double)g[j * 3] - mu2[0], (double)g[j * 3 + 1] - mu2[1]};
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) { xx[a][b] += x[a] * x[b]; xy[a][b] += x[a] * y[b]; }
    }
    // scale = trace(inv(x^T x + 1e-6 I) . x^T y) / 2, trans = mu2 / scale - mu1
    const double a00 = xx[0][0] + 1e-6, a01 = xx[0][1], a10 = xx[1][0], a11 = xx[1][1] + 1e-6;
    const double det = a00 * a11 - a01 * a10;
    const double i00 = a11 / det, i01 = -a01 / det, i10 = -a10 / det, i11 = a00 / det;
    const double scale = ((i00 * xy[0][0] + i01 * xy[1][0]) + (i10 * xy[0][1] + i11 * xy[1][1])) / 2.0;
    const double t[2] = {mu2[0] / scale - mu1[0], mu2[1] / scale - mu1[1]};
    if (cam) { cam[f * 3] = (float)scale; cam[f * 3 + 1] = (float)t[0]; cam[f * 3 + 2] = (float)t[1]; }
    if (!err_kp_pa && !pck) return;
    // pass 3: distances after the alignment, and the share of them strictly below alpha
    double epa = 0.0;
    int hit = 0;
    for (int j = 0; j < k; ++j) {
        if (g[j * 3 + 2] == 0.f) continue;
        const double dx = (double)g[j * 3] - scale * (kp_pred_px(p + j * 2, img_size) + t[0]);
        const double dy = (double)g[j * 3 + 1] - scale * (kp_pred_px(p + j * 2 + 1, img_size) + t[1]);
        const double d = sqrt(dx * dx + dy * dy);
        epa += d;
        hit += d < alpha ? 1 : 0;
    }
    if (err_kp_pa) err_kp_pa[f] = (float)(epa / nv);
    if (pck) pck[f] = (float)((double)hit / nv);
}

// log map of SO(3), one lane per matrix: row i holds `per` row-major 3x3 matrices.  The angle is atan2(|antisymmetric part| / 2,
// (trace - 1) / 2), never acos; up to a quarter turn the vector is the antisymmetric part stretched by angle / sin (1 to first
// order near 0), beyond it the axis comes from the symmetric part (R + R^T) / 2 = cos I + (1 - cos) n n^T -- its largest diagonal
// entry, signs from the antisymmetric part -- so nothing is divided by sin near pi.
__global__ void rotmat_to_aa_kernel(const float* __restrict__ rot, long long ld_rot, int n, int per, float* __restrict__ aa,
                                    long long ld_aa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const int row = i / per, q = i - row * per;
    const float* r = rot + (long long)row * ld_rot + q * 9;
    double R[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[a][b] = (double)r[a * 3 + b];
    const double v[3] = {(R[2][1] - R[1][2]) / 2.0, (R[0][2] - R[2][0]) / 2.0, (R[1][0] - R[0][1]) / 2.0};   // sin * axis
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double c = (R[0][0] + R[1][1] + R[2][2] - 1.0) / 2.0;
    const double angle = atan2(s, c);                                                                       // in [0, pi]
    double w[3];
    if (c >= 0.0) {
        const double g = s > 1e-8 ? angle / s : 1.0;
        for (int a = 0; a < 3; ++a) w[a] = g * v[a];
    } else {
        const int m = R[0][0] >= R[1][1] ? (R[0][0] >= R[2][2] ? 0 : 2) : (R[1][1] >= R[2][2] ? 1 : 2);
        double ax[3];
        const double nm2 = (R[m][m] - c) / (1.0 - c);                 // n_m^2 >= 1/3 up to the input's rounding
        ax[m] = sqrt(nm2 > 0.0 ? nm2 : 0.0);
        for (int a = 0; a < 3; ++a)
            if (a != m) ax[a] = ax[m] > 0.0 ? (R[m][a] + R[a][m]) / 2.0 / ((1.0 - c) * ax[m]) : 0.0;
        if (!(ax[m] > 0.0)) ax[m] = 1.0;
        const double nrm = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        const double sgn = (ax[0] * v[0] + ax[1] * v[1] + ax[2] * v[2]) < 0.0 ? -1.0 : 1.0;   // at exactly pi either sign is right
        for (int a = 0; a < 3; ++a) w[a] = sgn * angle * ax[a] / nrm;
    }
    float* o = aa + (long long)row * ld_aa + q * 3;
    o[0] = (float)w[0]; o[1] = (float)w[1]; o[2] = (float)w[2];
}

// exp map: smpl_pose_kernel's Rodrigues (so3.h), one lane per vector
__global__ void aa_to_rotmat_kernel(const float* __restrict__ aa, long long ld_aa, int n, int per, float* __restrict__ rot,
                                    long long ld_rot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * per) return;
    const int row = i / per, q = i - row * per;
    const float* a = aa + (long long)row * ld_aa + q * 3;
    float R[9];
    rodrigues_f32(a[0], a[1], a[2], R);
    float* o = rot + (long long)row * ld_rot + q * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = R[e];
}
}  // namespace

// both joint entry points: `who` names the caller in the messages
static int eval_joints_launch(const char* who, const float* gt, long long ld_gt, const float* pred, long long ld_pred, int n,
                              int k, int left_id, int right_id, float* mpjpe, float* pa_mpjpe, float* accel_pred,
                              float* accel_err, void* stream) {
    HMMR_REQUIRE(pred && n > 0 && k > 0 && k <= MAXK, "%s: bad arguments (k <= %d)", who, MAXK);
    HMMR_REQUIRE(left_id >= 0 && left_id < k && right_id >= 0 && right_id < k, "%s: bad hip ids", who);
    HMMR_REQUIRE(ld_pred >= 3LL * k && (!gt || ld_gt >= 3LL * k), "%s: row strides shorter than a row of k joints", who);
    hipStream_t s = (hipStream_t)stream;
    if (mpjpe || pa_mpjpe) {
        HMMR_REQUIRE(gt && mpjpe && pa_mpjpe, "%s: MPJPE needs gt and both outputs", who);
        hipLaunchKernelGGL(eval_joints_kernel, dim3((n + 63) / 64), dim3(64), 0, s, gt, ld_gt, pred, ld_pred, n, k, left_id,
                           right_id, mpjpe, pa_mpjpe);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    if ((accel_pred || accel_err) && n > 2) {
        hipLaunchKernelGGL(eval_accel_kernel, dim3((n - 2 + 63) / 64), dim3(64), 0, s, gt, ld_gt, pred, ld_pred, n, k,
                           accel_pred, accel_err);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int hmmr_eval_joints(const float* gt, const float* pred, int n, int k, int left_id, int right_id,
                                float* mpjpe, float* pa_mpjpe, float* accel_pred, float* accel_err, void* stream) {
    return eval_joints_launch("hmmr_eval_joints", gt, 3LL * k, pred, 3LL * k, n, k, left_id, right_id, mpjpe, pa_mpjpe,
                              accel_pred, accel_err, stream);
}

extern "C" int hmmr_eval_joints_ld(const float* gt, int64_t ld_gt, const float* pred, int64_t ld_pred, int n, int k,
                                   int left_id, int right_id, float* mpjpe, float* pa_mpjpe, float* accel_pred,
                                   float* accel_err, void* stream) {
    return eval_joints_launch("hmmr_eval_joints_ld", gt, (long long)ld_gt, pred, (long long)ld_pred, n, k, left_id, right_id,
                              mpjpe, pa_mpjpe, accel_pred, accel_err, stream);
}

extern "C" int hmmr_eval_verts(const float* gt, int64_t ld_gt, const float* pred, int64_t ld_pred, int n, int nv,
                               float* err, void* stream) {
    HMMR_REQUIRE(gt && pred && err && n > 0 && nv > 0, "hmmr_eval_verts: bad arguments");
    hipLaunchKernelGGL(eval_verts_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, gt, pred, nv, (long long)ld_gt,
                       (long long)ld_pred, err);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hmmr_eval_kps(const float* kps_gt, int64_t ld_gt, const float* kps_pred, int64_t ld_pred, int n, int k,
                             double alpha, int min_visible, float img_size, float* err_kp, float* err_kp_pa, float* pck,
                             float* cam, void* stream) {
    HMMR_REQUIRE(n > 0 && k > 0 && k <= MAXK, "hmmr_eval_kps: bad arguments (n > 0, 0 < k <= %d)", MAXK);
    HMMR_REQUIRE(err_kp || err_kp_pa || pck || cam, "hmmr_eval_kps: no output requested");
    HMMR_REQUIRE(kps_gt && kps_pred, "hmmr_eval_kps: an output was requested without kps_gt / kps_pred");
    HMMR_REQUIRE(ld_gt >= 3LL * k && ld_pred >= 2LL * k, "hmmr_eval_kps: row strides shorter than a row of k keypoints");
    HMMR_REQUIRE(alpha == alpha && min_visible >= 0 && img_size == img_size, "hmmr_eval_kps: bad alpha / min_visible / img_size");
    hipLaunchKernelGGL(eval_kps_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, kps_gt, (long long)ld_gt, kps_pred,
                       (long long)ld_pred, n, k, alpha, min_visible, img_size, err_kp, err_kp_pa, pck, cam);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hmmr_rotmat_to_axis_angle(const float* rot, int64_t ld_rot, int n, int per, float* aa, int64_t ld_aa,
                                         void* stream) {
    HMMR_REQUIRE(n > 0 && per > 0 && (long long)n * per <= 0x7fffffffLL, "hmmr_rotmat_to_axis_angle: bad arguments (n > 0, per > 0)");
    HMMR_REQUIRE(aa, "hmmr_rotmat_to_axis_angle: no output");
    HMMR_REQUIRE(rot, "hmmr_rotmat_to_axis_angle: output requested without rot");
    HMMR_REQUIRE(ld_rot >= 9LL * per && ld_aa >= 3LL * per, "hmmr_rotmat_to_axis_angle: row strides shorter than a row of matrices");
    hipLaunchKernelGGL(rotmat_to_aa_kernel, dim3((n * per + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot, (long long)ld_rot, n,
                       per, aa, (long long)ld_aa);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int hmmr_axis_angle_to_rotmat(const float* aa, int64_t ld_aa, int n, int per, float* rot, int64_t ld_rot,
                                         void* stream) {
    HMMR_REQUIRE(n > 0 && per > 0 && (long long)n * per <= 0x7fffffffLL, "hmmr_axis_angle_to_rotmat: bad arguments (n > 0, per > 0)");
    HMMR_REQUIRE(rot, "hmmr_axis_angle_to_rotmat: no output");
    HMMR_REQUIRE(aa, "hmmr_axis_angle_to_rotmat: output requested without aa");
    HMMR_REQUIRE(ld_aa >= 3LL * per && ld_rot >= 9LL * per, "hmmr_axis_angle_to_rotmat: row strides shorter than a row of vectors");
    hipLaunchKernelGGL(aa_to_rotmat_kernel, dim3((n * per + 63) / 64), dim3(64), 0, (hipStream_t)stream, aa, (long long)ld_aa, n, per,
                       rot, (long long)ld_rot);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
