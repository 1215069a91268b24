// Trainer losses for gfx950: the encoder losses of src/trainer_sequence_fc.py on precomputed phis (compute_losses_batched,
// compute_losses_deltas, the shape prior) from src/ops.py and src/tf_smpl/projection.py, forward and cotangents together, and the
// closed loop omega -> losses, d_omega (include/hmmr_hip.h, "Trainer losses").  Small data: N = B T rows of a few hundred floats,
// so the design is about launch count and about an order of summation that does not depend on timing, not about bandwidth.
//
// Three launches, no floating-point atomic anywhere (two calls on the same inputs give the same bytes):
//   loss_frame_kernel   one workgroup per pred row, one wave per term (its first lane works: the six terms run side by side instead of
//                       as six divergent branches of one wave): every per-frame sum in fp64, inside ONE thread in element order -- the optimal
//                       camera's 2x2 problem in closed form, sum vis |d|, the count of non-zero vis, and the four row-MSE sums
//                       (row_sse: joints after the pelvis alignment, rotations, shape, beta_t - beta_t+1) + sum beta^2 -> 8 doubles
//   loss_sum_kernel     one workgroup: the frames of a sequence in frame order (one thread per sequence), the sequences in sequence
//                       order (one thread per quantity), the normalisers from the ground truth, losses[8], status
//   loss_grad_kernel    one workgroup per pred row: the cotangents of total = sum w_i L_i, in fp64, rounded once
#include "common.h"
#include "hmmr_hip.h"
#include "workspace.h"

static constexpr int NQ = 8;                 // partial sums per frame
enum { Q_KP = 0, Q_VIS = 1, Q_JOINTS = 2, Q_POSE = 3, Q_SHAPE = 4, Q_CONST = 5, Q_PRIOR = 6, Q_STATUS = 7 };
// scalars of the workspace (doubles): what loss_grad_kernel multiplies by.  1 / normaliser, or 0 where TF's safe division gives 0
enum { S_KP = 0, S_JOINTS = 1, S_SMPL_POSE = 2, S_SMPL_SHAPE = 3, S_CONST = 4, S_PRIOR = 5, NS = 8 };
static constexpr int LSP = 14;               // joints of the 3-D loss (align_by_pelvis: hips 3 and 2)

struct LossArgs {
    int B, T, K, delta_t;
    unsigned flags;
    float w[6];
    const float *kps_pred, *joints_pred, *rs_pred, *beta_pred;
    int ld_beta;
    const float *kps_gt, *joints_gt, *rs_gt, *shapes_gt, *has_smpl, *has_joints;
    float *losses, *d_kps, *d_joints, *d_rs, *d_beta, *best_cam;
    unsigned* status;
    double *part, *seq, *scal;                // [N][NQ], [B][NQ], [NS]
    double* cam;                              // [N][4]: the optimal camera of the slice's rows, unrounded
};

// pred row (b, t) -> its gt row, or -1 outside the slice (compute_losses_deltas :867-884)
__device__ __forceinline__ int gt_row(int b, int t, int T, int delta_t) {
    const int a = delta_t < 0 ? -delta_t : delta_t;
    const int ps = delta_t < 0 ? a : 0, gs = delta_t > 0 ? a : 0;
    return (t >= ps && t < ps + T - a) ? b * T + (t - ps + gs) : -1;
}

// sum (a_i - b_i)^2 over n elements in index order: the one row routine of the four MSE terms (compute_loss_mse / _e_smooth)
__device__ __forceinline__ double row_sse(const float* a, const float* b, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double d = (double)a[i] - (double)b[i];
        s += d * d;
    }
    return s;
}
// the same after align_by_pelvis on both sides: 14 joints minus the midpoint of joints 3 and 2
__device__ __forceinline__ double row_sse_aligned(const float* a, const float* b) {
    double s = 0.0;
    for (int k = 0; k < LSP; ++k)
        for (int c = 0; c < 3; ++c) {
            const double pa = ((double)a[3 * 3 + c] + (double)a[2 * 3 + c]) / 2.0, pb = ((double)b[3 * 3 + c] + (double)b[2 * 3 + c]) / 2.0;
            const double d = ((double)a[k * 3 + c] - pa) - ((double)b[k * 3 + c] - pb);
            s += d * d;
        }
    return s;
}

// procrustes2d_vis for one frame, sums in keypoint order; a frame without a visible keypoint gives NaN (0 / 0), as the reference
__device__ __forceinline__ void optcam(const float* x, const float* g, int K, double (&cam)[3], bool& none) {
    double nv = 0.0, m1x = 0.0, m1y = 0.0, m2x = 0.0, m2y = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = g[3 * k + 2] > 0.f ? 1.0 : 0.0;
        nv += v;
        m1x += v * (double)x[2 * k]; m1y += v * (double)x[2 * k + 1];
        m2x += v * (double)g[3 * k]; m2y += v * (double)g[3 * k + 1];
    }
    none = nv == 0.0;
    m1x /= nv; m1y /= nv; m2x /= nv; m2y /= nv;
    double a = 0.0, b = 0.0, c = 0.0, p = 0.0, q = 0.0, r = 0.0, s = 0.0;        // A = [[a, b], [b, c]], xmu^T y = [[p, q], [r, s]]
    for (int k = 0; k < K; ++k) {
        const double v = g[3 * k + 2] > 0.f ? 1.0 : 0.0;
        const double ux = v * ((double)x[2 * k] - m1x), uy = v * ((double)x[2 * k + 1] - m1y);
        const double yx = v * ((double)g[3 * k] - m2x), yy = v * ((double)g[3 * k + 1] - m2y);
        a += ux * ux; b += ux * uy; c += uy * uy;
        p += ux * yx; q += ux * yy; r += uy * yx; s += uy * yy;
    }
    a += 1e-6; c += 1e-6;
    const double det = a * c - b * b;
    double sc = ((c * p - b * r) + (a * s - b * q)) / det / 2.0;                 // trace(A^-1 xmu^T y) / 2
    sc = sc < 0.7 ? 0.7 : (sc > 10.0 ? 10.0 : sc);                               // (a NaN stays a NaN)
    cam[0] = sc; cam[1] = m2x / sc - m1x; cam[2] = m2y / sc - m1y;
}

__global__ __launch_bounds__(384) void loss_frame_kernel(LossArgs A) {
    __shared__ double sOut[NQ];
    const int n = blockIdx.x, b = n / A.T, t = n - b * A.T, tid = threadIdx.x;
    const int lane = (tid & 63) == 0 ? tid >> 6 : -1;                          // the term this thread owns, if any
    const int g = gt_row(b, t, A.T, A.delta_t);
    if (tid < NQ) sOut[tid] = 0.0;
    __syncthreads();
    // one thread per term; each owns its slot(s) of sOut
    if (lane == 0 && g >= 0 && (A.flags & (HMMR_LOSS_KP | HMMR_LOSS_KP_OPTCAM))) {
        const float* x = A.kps_pred + (long long)n * A.K * 2;
        const float* y = A.kps_gt + (long long)g * A.K * 3;
        double cam[3] = {1.0, 0.0, 0.0};
        if (A.flags & HMMR_LOSS_KP_OPTCAM) {
            bool none;
            optcam(x, y, A.K, cam, none);
            if (none) sOut[Q_STATUS] = 1.0;
            double* o = A.cam + (long long)n * 4;
            o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
            if (A.best_cam) {
                float* bc = A.best_cam + (long long)n * 3;
                bc[0] = (float)cam[0]; bc[1] = (float)cam[1]; bc[2] = (float)cam[2];
            }
        }
        double s = 0.0, cnt = 0.0;
        for (int k = 0; k < A.K; ++k) {
            const double vis = (double)y[3 * k + 2];
            const double px = cam[0] * ((double)x[2 * k] + cam[1]), py = cam[0] * ((double)x[2 * k + 1] + cam[2]);
            s += vis * fabs((double)y[3 * k] - px);
            s += vis * fabs((double)y[3 * k + 1] - py);
            cnt += vis != 0.0 ? 1.0 : 0.0;
        }
        sOut[Q_KP] = s; sOut[Q_VIS] = cnt;
    }
    if (lane == 1 && g >= 0 && (A.flags & HMMR_LOSS_JOINTS))
        sOut[Q_JOINTS] = row_sse_aligned(A.joints_pred + (long long)n * A.K * 3, A.joints_gt + (long long)g * LSP * 3);
    if (lane == 2 && g >= 0 && (A.flags & HMMR_LOSS_SMPL))
        sOut[Q_POSE] = row_sse(A.rs_pred + (long long)n * 216, A.rs_gt + (long long)g * 216, 216);
    if (lane == 3 && g >= 0 && (A.flags & HMMR_LOSS_SMPL))
        sOut[Q_SHAPE] = row_sse(A.beta_pred + (long long)n * A.ld_beta, A.shapes_gt + (long long)b * 10, 10);
    if (lane == 4 && t + 1 < A.T && (A.flags & HMMR_LOSS_CONST))
        sOut[Q_CONST] = row_sse(A.beta_pred + (long long)n * A.ld_beta, A.beta_pred + (long long)(n + 1) * A.ld_beta, 10);
    if (lane == 5 && (A.flags & HMMR_LOSS_SHAPE_PRIOR)) {
        const float* be = A.beta_pred + (long long)n * A.ld_beta;
        double s = 0.0;
        for (int i = 0; i < 10; ++i) s += (double)be[i] * (double)be[i];
        sOut[Q_PRIOR] = s;
    }
    __syncthreads();
    if (tid < NQ) A.part[(long long)n * NQ + tid] = sOut[tid];
}

// the weight of a sequence's rows in the joints / smpl sums; the number of pred rows with a non-zero weight
__global__ __launch_bounds__(256) void loss_sum_kernel(LossArgs A) {
    __shared__ double sTot[NQ + 2];
    const int tid = threadIdx.x;
    const int L = A.T - (A.delta_t < 0 ? -A.delta_t : A.delta_t);                 // frames of the slice
    // frames in frame order: thread per sequence; the row weight (tf_repeat of has_gt3d_*) multiplies the sequence's sum
    for (int b = tid; b < A.B; b += 256) {
        double s[NQ];
        for (int q = 0; q < NQ; ++q) s[q] = 0.0;
        for (int t = 0; t < A.T; ++t) {
            const double* p = A.part + ((long long)b * A.T + t) * NQ;
            for (int q = 0; q < NQ; ++q) s[q] += p[q];
        }
        if (A.flags & HMMR_LOSS_JOINTS) s[Q_JOINTS] *= (double)A.has_joints[b];
        if (A.flags & HMMR_LOSS_SMPL) { s[Q_POSE] *= (double)A.has_smpl[b]; s[Q_SHAPE] *= (double)A.has_smpl[b]; }
        for (int q = 0; q < NQ; ++q) A.seq[(long long)b * NQ + q] = s[q];
    }
    __syncthreads();                             // (one workgroup: its own global stores are visible to it after the barrier)
    // sequences in sequence order: thread per quantity; threads NQ, NQ + 1 count the sequences with a non-zero weight
    if (tid < NQ) {
        double s = 0.0;
        for (int b = 0; b < A.B; ++b) s += A.seq[(long long)b * NQ + tid];
        sTot[tid] = s;
    } else if (tid < NQ + 2) {
        const float* has = tid == NQ ? A.has_joints : A.has_smpl;
        const bool on = (A.flags & (tid == NQ ? HMMR_LOSS_JOINTS : HMMR_LOSS_SMPL)) != 0;
        double c = 0.0;
        if (on)
            for (int b = 0; b < A.B; ++b) c += has[b] != 0.f ? 1.0 : 0.0;
        sTot[tid] = c * (double)L;
    }
    __syncthreads();
    if (tid == 0) {
        // TF 1.x _safe_div: numerator / denominator where the denominator is > 0, else 0
        auto inv = [](double den) { return den > 0.0 ? 1.0 / den : 0.0; };
        const double N10 = (double)A.B * (double)A.T * 10.0;
        double sc[NS];
        for (int i = 0; i < NS; ++i) sc[i] = 0.0;
        sc[S_KP] = inv(2.0 * sTot[Q_VIS]);
        sc[S_JOINTS] = inv(42.0 * sTot[NQ]);
        sc[S_SMPL_POSE] = inv(216.0 * sTot[NQ + 1]);
        sc[S_SMPL_SHAPE] = inv(10.0 * sTot[NQ + 1]);
        sc[S_CONST] = (A.flags & HMMR_LOSS_CONST) ? inv((double)A.B * (double)(A.T - 1) * 10.0) : 0.0;
        sc[S_PRIOR] = (A.flags & HMMR_LOSS_SHAPE_PRIOR) ? inv(N10) : 0.0;
        for (int i = 0; i < NS; ++i) A.scal[i] = sc[i];
        double l[8];
        l[HMMR_L_KP] = sTot[Q_KP] * sc[S_KP];
        l[HMMR_L_JOINTS] = 0.5 * sTot[Q_JOINTS] * sc[S_JOINTS];
        l[HMMR_L_SMPL_POSE] = 0.5 * sTot[Q_POSE] * sc[S_SMPL_POSE];
        l[HMMR_L_SMPL_SHAPE] = 0.5 * sTot[Q_SHAPE] * sc[S_SMPL_SHAPE];
        l[HMMR_L_CONST] = 0.5 * sTot[Q_CONST] * sc[S_CONST];
        l[HMMR_L_SHAPE] = sTot[Q_PRIOR] * sc[S_PRIOR];
        l[HMMR_L_TOTAL] = (double)A.w[HMMR_W_KP] * l[HMMR_L_KP] + (double)A.w[HMMR_W_JOINTS] * l[HMMR_L_JOINTS]
                          + (double)A.w[HMMR_W_SMPL] * (l[HMMR_L_SMPL_POSE] + l[HMMR_L_SMPL_SHAPE]) + (double)A.w[HMMR_W_CONST] * l[HMMR_L_CONST]
                          + (double)A.w[HMMR_W_SHAPE] * l[HMMR_L_SHAPE];
        l[7] = 0.0;
        for (int i = 0; i < 8; ++i) A.losses[i] = (float)l[i];
        if (A.status) {
            const double tot = l[HMMR_L_TOTAL];
            *A.status = (sTot[Q_STATUS] != 0.0 ? HMMR_LOSS_NO_VISIBLE : 0u) | ((tot - tot == 0.0) ? 0u : HMMR_LOSS_NOT_FINITE);
        }
    }
}

__device__ __forceinline__ double sign_of(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d); }      // sign(0) = 0; a NaN stays one

__global__ __launch_bounds__(256) void loss_grad_kernel(LossArgs A) {
    __shared__ double sG[3];                     // sum_k g_k of the aligned joint cotangent, per coordinate
    const int n = blockIdx.x, b = n / A.T, t = n - b * A.T, tid = threadIdx.x;
    const int g = gt_row(b, t, A.T, A.delta_t);
    const int K = A.K;
    if (A.d_kps) {
        float* o = A.d_kps + (long long)n * K * 2;
        const bool on = g >= 0 && (A.flags & (HMMR_LOSS_KP | HMMR_LOSS_KP_OPTCAM));
        double cam[3] = {1.0, 0.0, 0.0};
        if (on && (A.flags & HMMR_LOSS_KP_OPTCAM)) {
            const double* cm = A.cam + (long long)n * 4;
            cam[0] = cm[0]; cam[1] = cm[1]; cam[2] = cm[2];
        }
        const double f = (double)A.w[HMMR_W_KP] * A.scal[S_KP];
        for (int e = tid; e < K * 2; e += 256) {
            double v = 0.0;
            if (on) {
                const int k = e >> 1, c = e & 1;
                const float* y = A.kps_gt + ((long long)g * K + k) * 3;
                const double pr = cam[0] * ((double)A.kps_pred[(long long)n * K * 2 + e] + cam[1 + c]);
                v = f * (double)y[2] * sign_of(pr - (double)y[c]) * cam[0];
            }
            o[e] = (float)v;
        }
    }
    if (A.d_joints) {
        float* o = A.d_joints + (long long)n * K * 3;
        const bool on = g >= 0 && (A.flags & HMMR_LOSS_JOINTS);
        const float* a = A.joints_pred + (long long)n * K * 3;
        const float* bb = on ? A.joints_gt + (long long)g * LSP * 3 : nullptr;
        const double f = on ? (double)A.w[HMMR_W_JOINTS] * (double)A.has_joints[b] * A.scal[S_JOINTS] : 0.0;
        auto gk = [&](int k, int c) {            // the cotangent of aligned joint (k, c)
            const double pa = ((double)a[3 * 3 + c] + (double)a[2 * 3 + c]) / 2.0, pb = ((double)bb[3 * 3 + c] + (double)bb[2 * 3 + c]) / 2.0;
            return f * (((double)a[k * 3 + c] - pa) - ((double)bb[k * 3 + c] - pb));
        };
        if (on && tid < 3) {
            double s = 0.0;
            for (int k = 0; k < LSP; ++k) s += gk(k, tid);
            sG[tid] = s;
        }
        __syncthreads();
        for (int e = tid; e < K * 3; e += 256) {
            const int k = e / 3, c = e - 3 * k;
            double v = 0.0;
            if (on && k < LSP) v = gk(k, c) - ((k == 2 || k == 3) ? 0.5 * sG[c] : 0.0);
            o[e] = (float)v;
        }
    }
    if (A.d_rs) {
        float* o = A.d_rs + (long long)n * 216;
        const bool on = g >= 0 && (A.flags & HMMR_LOSS_SMPL);
        const double f = on ? (double)A.w[HMMR_W_SMPL] * (double)A.has_smpl[b] * A.scal[S_SMPL_POSE] : 0.0;
        for (int e = tid; e < 216; e += 256)
            o[e] = on ? (float)(f * ((double)A.rs_pred[(long long)n * 216 + e] - (double)A.rs_gt[(long long)g * 216 + e])) : 0.f;
    }
    if (A.d_beta && tid < 10) {
        double v = 0.0;
        if (A.flags & (HMMR_LOSS_SMPL | HMMR_LOSS_CONST | HMMR_LOSS_SHAPE_PRIOR)) {
            const double be = (double)A.beta_pred[(long long)n * A.ld_beta + tid];
            double v_smpl = 0.0, v_const = 0.0, v_prior = 0.0;
            if (g >= 0 && (A.flags & HMMR_LOSS_SMPL))
                v_smpl = (double)A.w[HMMR_W_SMPL] * (double)A.has_smpl[b] * A.scal[S_SMPL_SHAPE] * (be - (double)A.shapes_gt[b * 10 + tid]);
            if (A.flags & HMMR_LOSS_CONST) {
                double d = 0.0;
                if (t + 1 < A.T) d += be - (double)A.beta_pred[(long long)(n + 1) * A.ld_beta + tid];
                if (t > 0) d -= (double)A.beta_pred[(long long)(n - 1) * A.ld_beta + tid] - be;
                v_const = (double)A.w[HMMR_W_CONST] * A.scal[S_CONST] * d;
            }
            if (A.flags & HMMR_LOSS_SHAPE_PRIOR) v_prior = (double)A.w[HMMR_W_SHAPE] * A.scal[S_PRIOR] * 2.0 * be;
            v = (v_smpl + v_const) + v_prior;
        }
        A.d_beta[(long long)n * 10 + tid] = (float)v;
    }
}

// ------------------------------------------------------------------------- //
struct LossBufs { size_t part, seq, scal, cam, total; };
static LossBufs loss_layout(int B, int T) {
    WsCarver c;
    const size_t N = (size_t)B * (size_t)T;
    return {c.take(N * NQ * 8), c.take((size_t)B * NQ * 8), c.take(NS * 8), c.take(N * 4 * 8), c.total()};
}
extern "C" size_t hmmr_seq_losses_workspace_bytes(int B, int T) { return (B > 0 && T > 0) ? loss_layout(B, T).total : 0; }

static const unsigned ALL_FLAGS = HMMR_LOSS_KP | HMMR_LOSS_KP_OPTCAM | HMMR_LOSS_JOINTS | HMMR_LOSS_SMPL | HMMR_LOSS_CONST | HMMR_LOSS_SHAPE_PRIOR;

// every refusal of the descriptor that does not concern its pointers (shared with hmmr_omega_loss_grad, which supplies those itself)
static int loss_check_shape(const hmmr_seq_loss_desc_t* d, const char* who) {
    HMMR_REQUIRE(d, "%s: null descriptor", who);
    HMMR_REQUIRE(d->B > 0 && d->T > 0 && d->K > 0, "%s: B=%d, T=%d and K=%d must be positive", who, d->B, d->T, d->K);
    // (rows are counted in int: the grid size, and n * 85 in the assembling launch)
    HMMR_REQUIRE((long long)d->B * d->T <= (1ll << 24), "%s: B T = %lld rows exceed 2^24", who, (long long)d->B * d->T);
    HMMR_REQUIRE((d->flags & ~ALL_FLAGS) == 0, "%s: unknown flag bits 0x%x", who, d->flags & ~ALL_FLAGS);
    HMMR_REQUIRE(!((d->flags & HMMR_LOSS_KP) && (d->flags & HMMR_LOSS_KP_OPTCAM)), "%s: KP and KP_OPTCAM are both set", who);
    HMMR_REQUIRE(!(d->flags & HMMR_LOSS_JOINTS) || d->K >= LSP, "%s: JOINTS needs K >= 14 (K=%d)", who, d->K);
    HMMR_REQUIRE(d->delta_t > -d->T && d->delta_t < d->T, "%s: |delta_t|=%d must be below T=%d", who, d->delta_t < 0 ? -d->delta_t : d->delta_t, d->T);
    return 0;
}
static int loss_check_gt(const hmmr_seq_loss_desc_t* d, const char* who) {
    HMMR_REQUIRE(!(d->flags & (HMMR_LOSS_KP | HMMR_LOSS_KP_OPTCAM)) || d->kps_gt, "%s: KP / KP_OPTCAM is set and kps_gt is NULL", who);
    HMMR_REQUIRE(!(d->flags & HMMR_LOSS_JOINTS) || (d->joints_gt && d->has_gt3d_joints), "%s: JOINTS is set and joints_gt or has_gt3d_joints is NULL", who);
    HMMR_REQUIRE(!(d->flags & HMMR_LOSS_SMPL) || (d->rs_gt && d->shapes_gt && d->has_gt3d_smpl),
                 "%s: SMPL is set and rs_gt, shapes_gt or has_gt3d_smpl is NULL", who);
    return 0;
}

extern "C" int hmmr_seq_losses(const hmmr_seq_loss_desc_t* d, void* stream) {
    if (int rc = loss_check_shape(d, "hmmr_seq_losses")) return rc;
    if (int rc = loss_check_gt(d, "hmmr_seq_losses")) return rc;
    HMMR_REQUIRE(!(d->flags & (HMMR_LOSS_KP | HMMR_LOSS_KP_OPTCAM)) || d->kps_pred, "hmmr_seq_losses: KP / KP_OPTCAM is set and kps_pred is NULL");
    HMMR_REQUIRE(!(d->flags & HMMR_LOSS_JOINTS) || d->joints_pred, "hmmr_seq_losses: JOINTS is set and joints_pred is NULL");
    HMMR_REQUIRE(!(d->flags & HMMR_LOSS_SMPL) || d->rs_pred, "hmmr_seq_losses: SMPL is set and rs_pred is NULL");
    HMMR_REQUIRE(!(d->flags & (HMMR_LOSS_SMPL | HMMR_LOSS_CONST | HMMR_LOSS_SHAPE_PRIOR)) || d->beta_pred,
                 "hmmr_seq_losses: SMPL, CONST or SHAPE_PRIOR is set and beta_pred is NULL");
    HMMR_REQUIRE(!d->beta_pred || d->ld_beta >= 10, "hmmr_seq_losses: ld_beta=%d is below 10", d->ld_beta);
    HMMR_REQUIRE(d->losses, "hmmr_seq_losses: losses is NULL");
    const LossBufs L = loss_layout(d->B, d->T);
    HMMR_REQUIRE(d->ws && d->ws_bytes >= L.total, "hmmr_seq_losses: workspace too small (%zu bytes given, %zu needed)", d->ws ? d->ws_bytes : (size_t)0,
                 L.total);
    LossArgs A;
    A.B = d->B; A.T = d->T; A.K = d->K; A.delta_t = d->delta_t; A.flags = d->flags;
    for (int i = 0; i < 6; ++i) A.w[i] = d->weights[i];
    A.kps_pred = d->kps_pred; A.joints_pred = d->joints_pred; A.rs_pred = d->rs_pred; A.beta_pred = d->beta_pred; A.ld_beta = d->ld_beta;
    A.kps_gt = d->kps_gt; A.joints_gt = d->joints_gt; A.rs_gt = d->rs_gt; A.shapes_gt = d->shapes_gt;
    A.has_smpl = d->has_gt3d_smpl; A.has_joints = d->has_gt3d_joints;
    A.losses = d->losses; A.d_kps = d->d_kps; A.d_joints = d->d_joints; A.d_rs = d->d_rs; A.d_beta = d->d_beta; A.best_cam = d->best_cam;
    A.status = d->status;
    char* base = (char*)d->ws;
    A.part = (double*)(base + L.part); A.seq = (double*)(base + L.seq); A.scal = (double*)(base + L.scal); A.cam = (double*)(base + L.cam);
    hipStream_t s = (hipStream_t)stream;
    const int N = d->B * d->T;
    hipLaunchKernelGGL(loss_frame_kernel, dim3(N), dim3(384), 0, s, A);
    HMMR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(256), 0, s, A);
    HMMR_CHECK_HIP(hipGetLastError());
    if (d->d_kps || d->d_joints || d->d_rs || d->d_beta) {
        hipLaunchKernelGGL(loss_grad_kernel, dim3(N), dim3(256), 0, s, A);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// ---- the closed loop ----------------------------------------------------- //
// cams [1, 0, 0] per row for the forward under use_optcam
__global__ void omega_unit_cams_kernel(float* __restrict__ cams, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { cams[3 * i] = 1.f; cams[3 * i + 1] = 0.f; cams[3 * i + 2] = 0.f; }
}
// d_omega = [d_cams or 0 | d_theta | d_beta (SMPL) + d_beta (direct)]
__global__ void omega_assemble_kernel(const float* __restrict__ d_cams, const float* __restrict__ d_theta, const float* __restrict__ d_beta_smpl,
                                      const float* __restrict__ d_beta_direct, float* __restrict__ d_omega, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 85) return;
    const int n = i / 85, c = i - n * 85;
    float v;
    if (c < 3) v = d_cams ? d_cams[n * 3 + c] : 0.f;
    else if (c < 75) v = d_theta[n * 72 + (c - 3)];
    else v = d_beta_smpl[n * 10 + (c - 75)] + d_beta_direct[n * 10 + (c - 75)];
    d_omega[i] = v;
}

struct OmegaBufs { size_t fwd, bwd, loss, cams, verts, joints, kps, rs, d_kps, d_joints, d_rs, d_beta, d_theta, d_beta_smpl, d_cams, total; };
static OmegaBufs omega_layout(const hmmr_smpl_consts_t* c, int B, int T) {
    WsCarver w;
    const size_t N = (size_t)B * (size_t)T, K = (size_t)c->num_kps, V = (size_t)(c->num_verts > 0 ? c->num_verts : 1);
    OmegaBufs o;
    o.fwd = w.take(hmmr_smpl_workspace_bytes((int)N));
    o.bwd = w.take(hmmr_smpl_bwd_workspace_bytes(c, (int)N));
    o.loss = w.take(hmmr_seq_losses_workspace_bytes(B, T));
    o.cams = w.take(N * 3 * 4);
    o.verts = w.take(N * V * 3 * 4);
    o.joints = w.take(N * K * 3 * 4);
    o.kps = w.take(N * K * 2 * 4);
    o.rs = w.take(N * 216 * 4);
    o.d_kps = w.take(N * K * 2 * 4);
    o.d_joints = w.take(N * K * 3 * 4);
    o.d_rs = w.take(N * 216 * 4);
    o.d_beta = w.take(N * 10 * 4);
    o.d_theta = w.take(N * 72 * 4);
    o.d_beta_smpl = w.take(N * 10 * 4);
    o.d_cams = w.take(N * 3 * 4);
    o.total = w.total();
    return o;
}
extern "C" size_t hmmr_omega_loss_grad_workspace_bytes(const hmmr_smpl_consts_t* c, int B, int T) {
    return (c && B > 0 && T > 0 && (long long)B * T <= (1ll << 24) && c->num_kps > 0) ? omega_layout(c, B, T).total : 0;
}

extern "C" int hmmr_omega_loss_grad(const hmmr_smpl_consts_t* c, const hmmr_smpl_grad_consts_t* g, const hmmr_seq_loss_desc_t* gt,
                                    const float* omega, int use_optcam, float* losses, float* d_omega, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(c && g && omega && losses && d_omega, "hmmr_omega_loss_grad: null argument");
    if (int rc = loss_check_shape(gt, "hmmr_omega_loss_grad")) return rc;
    if (int rc = loss_check_gt(gt, "hmmr_omega_loss_grad")) return rc;
    HMMR_REQUIRE(gt->K == c->num_kps, "hmmr_omega_loss_grad: K=%d is not the model's keypoint count %d", gt->K, c->num_kps);
    // what hmmr_smpl_fwd and hmmr_smpl_bwd would refuse, here: their own checks come after the launches in front of them
    HMMR_REQUIRE(c->lbs_nnz >= 1 && c->lbs_nnz <= 24, "hmmr_omega_loss_grad: lbs_nnz=%d out of range", c->lbs_nnz);
    HMMR_REQUIRE(c->num_verts >= 1 && g->num_verts == c->num_verts && g->num_kps == c->num_kps,
                 "hmmr_omega_loss_grad: the grad constants (%d vertices, %d keypoints) belong to another model (%d, %d)", g->num_verts, g->num_kps,
                 c->num_verts, c->num_kps);
    HMMR_REQUIRE(c->vpad >= (c->num_verts + 127) / 128 * 128 && c->vpad % 128 == 0 && ((uintptr_t)c->dirs & 15) == 0,
                 "hmmr_omega_loss_grad: dirs must be 16-byte aligned with a row stride vpad=%d that is a multiple of 128 covering num_verts=%d", c->vpad,
                 c->num_verts);
    const OmegaBufs L = omega_layout(c, gt->B, gt->T);
    HMMR_REQUIRE(ws && ws_bytes >= L.total, "hmmr_omega_loss_grad: workspace too small (%zu bytes given, %zu needed)", ws ? ws_bytes : (size_t)0, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    auto F = [&](size_t off) { return (float*)(base + off); };
    const int N = gt->B * gt->T;
    const float* cams = omega;
    int ld_cam = 85;
    if (use_optcam) {
        hipLaunchKernelGGL(omega_unit_cams_kernel, dim3((N + 255) / 256), dim3(256), 0, s, F(L.cams), N);
        HMMR_CHECK_HIP(hipGetLastError());
        cams = F(L.cams);
        ld_cam = 3;
    }
    if (int rc = hmmr_smpl_fwd(c, omega + 3, 85, omega + 75, 85, cams, ld_cam, N, F(L.verts), F(L.joints), F(L.kps), F(L.rs), base + L.fwd,
                               hmmr_smpl_workspace_bytes(N), stream))
        return rc;
    hmmr_seq_loss_desc_t d = *gt;
    d.kps_pred = F(L.kps); d.joints_pred = F(L.joints); d.rs_pred = F(L.rs); d.beta_pred = omega + 75; d.ld_beta = 85;
    d.losses = losses; d.d_kps = F(L.d_kps); d.d_joints = F(L.d_joints); d.d_rs = F(L.d_rs); d.d_beta = F(L.d_beta);
    d.ws = base + L.loss; d.ws_bytes = hmmr_seq_losses_workspace_bytes(gt->B, gt->T);
    if (int rc = hmmr_seq_losses(&d, stream)) return rc;
    float* d_cams = use_optcam ? nullptr : F(L.d_cams);
    if (int rc = hmmr_smpl_bwd(c, g, omega + 3, 85, omega + 75, 85, cams, ld_cam, F(L.joints), N, nullptr, F(L.d_joints), F(L.d_kps), F(L.d_rs),
                               F(L.d_theta), F(L.d_beta_smpl), d_cams, base + L.bwd, hmmr_smpl_bwd_workspace_bytes(c, N), stream))
        return rc;
    hipLaunchKernelGGL(omega_assemble_kernel, dim3((N * 85 + 255) / 256), dim3(256), 0, s, (const float*)d_cams, (const float*)F(L.d_theta),
                       (const float*)F(L.d_beta_smpl), (const float*)F(L.d_beta), d_omega, N);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- e_hallucinate ------------------------------------------------------- //
// tf.losses.mean_squared_error(movie_strip, pred_movie_strip) with the default weight 1 (src/trainer_sequence_fc.py: e_hallucinate):
// sum (a - b)^2 / (rows cols) over two [rows][cols] tensors, and both cotangents -- there is no stop-gradient on either side.
// Two launches, no atomic: strip_mse_row_kernel, one workgroup per row -- thread t sums the elements t, t + 256, ... in index order in
// fp64, the 256 partials fold pairwise (t += t + 128, then 64, ... 1: a fixed tree) into part[row], and the row's cotangents
// d_a = weight 2 (a - b) / N (formed in fp64, rounded once) and d_b = -d_a (the same fp32 value negated) are written beside it;
// strip_mse_sum_kernel, one thread: the rows in row order, one division by N, one rounding to fp32.
static constexpr int MSE_THREADS = 256;

__global__ __launch_bounds__(MSE_THREADS) void strip_mse_row_kernel(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                                                     int cols, double scale, float* d_a, long long ld_da, float* d_b, long long ld_db,
                                                                     double* __restrict__ part) {
    __shared__ double sP[MSE_THREADS];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* ar = a + (long long)r * lda;
    const float* br = b + (long long)r * ldb;
    float* da = d_a ? d_a + (long long)r * ld_da : nullptr;
    float* db = d_b ? d_b + (long long)r * ld_db : nullptr;
    double s = 0.0;
    for (int i = tid; i < cols; i += MSE_THREADS) {
        const double d = (double)ar[i] - (double)br[i];
        s += d * d;
        const float g = (float)(scale * d);
        if (da) da[i] = g;
        if (db) db[i] = -g;
    }
    sP[tid] = s;
    __syncthreads();
    for (int w = MSE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) sP[tid] += sP[tid + w];
        __syncthreads();
    }
    if (part && tid == 0) part[r] = sP[0];
}

__global__ void strip_mse_sum_kernel(const double* __restrict__ part, int rows, double inv_n, float* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s += part[r];
    *loss = (float)(s * inv_n);
}

extern "C" size_t hmmr_strip_mse_workspace_bytes(int rows) {
    if (rows <= 0) return 0;
    WsCarver c;
    c.take((size_t)rows * 8);
    return c.total();
}

extern "C" int hmmr_strip_mse(const float* a, long long lda, const float* b, long long ldb, int rows, int cols, float weight, float* loss,
                              float* d_a, long long ld_da, float* d_b, long long ld_db, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(a && b, "hmmr_strip_mse: null a or b");
    HMMR_REQUIRE(rows > 0 && cols > 0, "hmmr_strip_mse: rows=%d and cols=%d must be positive", rows, cols);
    HMMR_REQUIRE(rows <= (1 << 24), "hmmr_strip_mse: rows=%d exceed 2^24", rows);
    HMMR_REQUIRE(lda >= cols && ldb >= cols, "hmmr_strip_mse: lda=%lld or ldb=%lld is below cols=%d", lda, ldb, cols);
    HMMR_REQUIRE(loss || d_a || d_b, "hmmr_strip_mse: nothing to write (loss, d_a and d_b are all NULL)");
    HMMR_REQUIRE((!d_a || ld_da >= cols) && (!d_b || ld_db >= cols), "hmmr_strip_mse: ld_da=%lld or ld_db=%lld is below cols=%d", ld_da, ld_db, cols);
    HMMR_REQUIRE(__builtin_isfinite(weight), "hmmr_strip_mse: weight is not finite");
    const size_t need = hmmr_strip_mse_workspace_bytes(rows);
    HMMR_REQUIRE(!loss || (ws && ws_bytes >= need), "hmmr_strip_mse: workspace too small (%zu bytes given, %zu needed)", ws ? ws_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    const double N = (double)rows * (double)cols;
    hipLaunchKernelGGL(strip_mse_row_kernel, dim3(rows), dim3(MSE_THREADS), 0, s, a, lda, b, ldb, cols, (double)weight * 2.0 / N, d_a, ld_da, d_b, ld_db,
                       loss ? (double*)ws : (double*)nullptr);
    HMMR_CHECK_HIP(hipGetLastError());
    if (loss) {
        hipLaunchKernelGGL(strip_mse_sum_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, rows, 1.0 / N, loss);
        HMMR_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
