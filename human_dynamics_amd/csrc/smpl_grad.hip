// SMPL backward for gfx950: the derivative of what smpl.hip computes -- SMPL.__call__ (src/tf_smpl/batch_smpl.py:89-162),
// batch_rodrigues / batch_global_rigid_transformation (src/tf_smpl/batch_lbs.py:42-60, 133-194) and batch_orth_proj_idrot
// (src/tf_smpl/projection.py:16-29) -- with respect to theta, beta and the camera.  Exact fp32 throughout: the function that is
// differentiated is the fp32 forward (rodrigues_f32 of so3.h with its +1e-8 inside the norm only, FK in index order,
// A = [G_R | G_t - G_R J]), whatever blend form the forward call ran.  Everything is recomputed from theta and beta; only the
// camera gradient needs a forward output (joints).
//
// Three launches, no floating-point atomic anywhere (two calls on the same inputs give the same bytes):
//   smpl_bwd_pose_kernel   per instance: R, J, G, A and the feature row, as smpl_pose_kernel forms them, + a record {R, J} per joint
//   smpl_bwd_verts_kernel  per (128-vertex tile, 8 instances): v_posed again (the packed-FMA chain of smpl_verts_kernel), the vertex
//                          cotangent g = d_verts + kreg (d_joints + s [d_kps, 0]) through the regressor's CSR BY VERTEX, d_v_posed =
//                          T_R^T g; g, v_posed and d_v_posed go to LDS, and then every thread OWNS outputs and walks the tile's
//                          vertices in index order: d_A[i][j][r][:] += w[v,j] g_r [v_posed; 1] (dense weights of the tile in LDS) and
//                          d_feat[i][k] += dirs[k][c][v] d_v_posed[i][c][v] (one basis row per thread, 16-byte reads).  One partial
//                          per (tile, instance) in the workspace.
//   smpl_bwd_tail_kernel   per instance: the partials summed in tile order, d_beta (direct and through J), reverse FK in descending
//                          joint index, d_R from d_A, from the pose features and from d_rs, reverse Rodrigues, the camera gradient.
#include "common.h"
#include "hmmr_hip.h"
#include "so3.h"
#include "workspace.h"

static constexpr int NJ = 24;
static constexpr int NFEAT = 218;        // 1 + 10 + 207
static constexpr int LDF = 224;          // feature row stride (floats)
static constexpr int LDA = NJ * 12;      // A record: 24 x (3x4) floats; the pose record {R 9, J 3} per joint has the same size
static constexpr int NFEAT_PAD = 220;    // blend loop length (rows >= 218 of `dirs` are zero)
static constexpr int VT = 128;           // vertices per workgroup
static constexpr int IBG = 8;            // instances per workgroup

// ---- pass 1 -------------------------------------------------------------- //
// smpl_pose_kernel's arithmetic, expression for expression (csrc/smpl.hip); rows m .. mp - 1 of feat / A are never read as live data.
__global__ __launch_bounds__(256) void smpl_bwd_pose_kernel(
    const float* __restrict__ theta, int ld_theta, const float* __restrict__ beta, int ld_beta,
    const float* __restrict__ j_template, const float* __restrict__ j_shapedirs,
    const int* __restrict__ parents, int m, float* __restrict__ feat, float* __restrict__ Aout, float* __restrict__ prec) {
    __shared__ float sLoc[8][NJ][12];
    __shared__ float sGlb[8][NJ][12];
    __shared__ float sJ[8][NJ][3];
    const int slot = threadIdx.x >> 5, j = threadIdx.x & 31;
    const int inst = blockIdx.x * 8 + slot;
    const bool live = inst < m && j < NJ;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (live) {
        const float* th = theta + (long long)inst * ld_theta + 3 * j;
        rodrigues_f32(th[0], th[1], th[2], R);      // so3.h
        float* f = feat + (long long)inst * LDF;
        float* pr = prec + (long long)inst * LDA + j * 12;
#pragma unroll
        for (int e = 0; e < 9; ++e) pr[e] = R[e];
        if (j >= 1) {
#pragma unroll
            for (int e = 0; e < 9; ++e) f[11 + (j - 1) * 9 + e] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.0f : 0.0f);
        }
        const float* bt = beta + (long long)inst * ld_beta;
        if (j < 10) f[1 + j] = bt[j];
        if (j == 0) f[0] = 1.0f;
        if (j < LDF - NFEAT) f[NFEAT + j] = 0.0f;
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) {
            float acc = j_template[j * 3 + c3];
#pragma unroll
            for (int b = 0; b < 10; ++b) acc += bt[b] * j_shapedirs[b * (NJ * 3) + j * 3 + c3];
            sJ[slot][j][c3] = acc;
            pr[9 + c3] = acc;
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) sLoc[slot][j][e] = R[e];
    }
    __syncthreads();
    if (live) {
        const int p = j == 0 ? -1 : parents[j];
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3)
            sLoc[slot][j][9 + c3] = sJ[slot][j][c3] - (p >= 0 ? sJ[slot][p][c3] : 0.0f);
        if (j == 0) {
#pragma unroll
            for (int e = 0; e < 12; ++e) sGlb[slot][0][e] = sLoc[slot][0][e];
        }
    }
    __syncthreads();
    for (int i = 1; i < NJ; ++i) {
        if (live && j == i) {
            const int p = parents[i];
            const float* G = sGlb[slot][p];
            const float* Lc = sLoc[slot][i];
            float o[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    o[r * 3 + cc] = G[r * 3 + 0] * Lc[0 * 3 + cc] + G[r * 3 + 1] * Lc[1 * 3 + cc] + G[r * 3 + 2] * Lc[2 * 3 + cc];
                o[9 + r] = G[r * 3 + 0] * Lc[9] + G[r * 3 + 1] * Lc[10] + G[r * 3 + 2] * Lc[11] + G[9 + r];
            }
#pragma unroll
            for (int e = 0; e < 12; ++e) sGlb[slot][i][e] = o[e];
        }
        __syncthreads();
    }
    if (live) {
        const float* G = sGlb[slot][j];
        float* o = Aout + (long long)inst * LDA + j * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float bone = G[r * 3 + 0] * sJ[slot][j][0] + G[r * 3 + 1] * sJ[slot][j][1] + G[r * 3 + 2] * sJ[slot][j][2];
            o[r * 4 + 0] = G[r * 3 + 0]; o[r * 4 + 1] = G[r * 3 + 1]; o[r * 4 + 2] = G[r * 3 + 2];
            o[r * 4 + 3] = G[9 + r] - bone;
        }
    }
}

// ---- pass 2 -------------------------------------------------------------- //
// One thread per vertex up to the LDS hand-over, one thread per OUTPUT after it: a reduction over the tile's 128 vertices is a loop in
// index order inside one thread, so its result does not depend on timing.  Vertices beyond num_verts carry g = 0 and d_v_posed = 0
// (the basis columns beyond num_verts are zero as well); instances beyond m carry zero features, zero transforms and g = 0.
__global__ __launch_bounds__(VT) void smpl_bwd_verts_kernel(
    const float* __restrict__ dirs, int vpad, const float* __restrict__ feat, const float* __restrict__ A,
    const int* __restrict__ lbs_idx, const float* __restrict__ lbs_w, int nnz,
    const int* __restrict__ vk_ptr, const int* __restrict__ vk_idx, const float* __restrict__ vk_val,
    int nv, int nk, int m, int mp, const float* __restrict__ cams, int ld_cam,
    const float* __restrict__ d_verts, const float* __restrict__ d_joints, const float* __restrict__ d_kps,
    float* __restrict__ partF, float* __restrict__ partA) {
    __shared__ __attribute__((aligned(16))) float sA[IBG][LDA];
    __shared__ __attribute__((aligned(16))) float sF[NFEAT_PAD][IBG];          // [k][instance]
    __shared__ __attribute__((aligned(16))) float sW[VT][NJ];                  // the tile's skinning weights, dense
    __shared__ __attribute__((aligned(16))) float sGH[IBG][VT][6];             // {g, v_posed} per (instance, vertex)
    __shared__ __attribute__((aligned(16))) float sDv[3][VT][IBG];             // d_v_posed [c][vertex][instance]
    // 1-D grid, instance blocks fastest, XCD-aware as in smpl_verts_kernel: the workgroups of one vertex tile share its basis slice in one L2
    const int nib = mp / IBG;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = L / nib, v0 = tile * VT, t = threadIdx.x, v = v0 + t;     // v < vpad always
    const int i0 = (L % nib) * IBG;
    const bool vlive = v < nv;
    for (int e = t; e < IBG * LDA; e += VT) {
        const int ii = e / LDA;
        sA[ii][e % LDA] = (i0 + ii < m) ? A[(long long)(i0 + ii) * LDA + (e % LDA)] : 0.f;
    }
    for (int e = t; e < IBG * NFEAT_PAD; e += VT) {
        const int ii = e / NFEAT_PAD, k = e % NFEAT_PAD;
        sF[k][ii] = (i0 + ii < m) ? feat[(long long)(i0 + ii) * LDF + k] : 0.f;
    }
    const int* vidx = lbs_idx + (long long)(vlive ? v : 0) * nnz;
    const float* vw = lbs_w + (long long)(vlive ? v : 0) * nnz;
#pragma unroll
    for (int j = 0; j < NJ; ++j) sW[t][j] = 0.f;
    if (vlive)
        for (int z = 0; z < nnz; ++z) sW[t][vidx[z]] += vw[z];                  // (ELL padding: joint 0, weight 0)
    // v_posed = [1, beta, R - I] . dirs for 8 instances: smpl_verts_kernel's chain, two instances per packed FMA
    f32x2 acc[IBG / 2][3];
#pragma unroll
    for (int ip = 0; ip < IBG / 2; ++ip) acc[ip][0] = acc[ip][1] = acc[ip][2] = f32x2{0.f, 0.f};
    float dv[2][4][3];
    auto fetch = [&](int k, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) dv[set][q][c] = (dirs + (long long)((k + q) * 3 + c) * vpad)[v];
    };
    auto blend = [&](int k, int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int i4 = 0; i4 < IBG / 4; ++i4) {
                const f32x4 c4 = *(const f32x4*)&sF[k + q][4 * i4];
                const f32x2 lo = {c4[0], c4[1]}, hi = {c4[2], c4[3]};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x2 b = {dv[set][q][c], dv[set][q][c]};
                    acc[2 * i4][c] = __builtin_elementwise_fma(lo, b, acc[2 * i4][c]);
                    acc[2 * i4 + 1][c] = __builtin_elementwise_fma(hi, b, acc[2 * i4 + 1][c]);
                }
            }
        }
    };
    fetch(0, 0);
    __syncthreads();
    static_assert(NFEAT_PAD % 8 == 4, "the two-set loop below peels one step");
    for (int k = 0; k < NFEAT_PAD - 4; k += 8) {
        fetch(k + 4, 1);
        blend(k, 0);
        fetch(k + 8, 0);
        blend(k + 4, 1);
    }
    blend(NFEAT_PAD - 4, 0);
    // the vertex cotangent and what the two reductions read
    const int e0 = vlive ? vk_ptr[v] : 0, e1 = vlive ? vk_ptr[v + 1] : 0;
#pragma unroll
    for (int g4 = 0; g4 < IBG; g4 += 4) {
        float T[4][12];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 12; ++e) T[q][e] = 0.f;
        if (vlive)
            for (int z = 0; z < nnz; ++z) {
                const int jj = vidx[z] * 12;
                const float wv = vw[z];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4* a4 = (const f32x4*)&sA[g4 + q][jj];
                    const f32x4 r0 = a4[0], r1 = a4[1], r2 = a4[2];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        T[q][e] = fmaf(wv, r0[e], T[q][e]);
                        T[q][4 + e] = fmaf(wv, r1[e], T[q][4 + e]);
                        T[q][8 + e] = fmaf(wv, r2[e], T[q][8 + e]);
                    }
                }
            }
        float dvp[3][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ii = g4 + q, inst = i0 + ii;
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (vlive && inst < m) {
                if (d_verts) {
                    const float* p = d_verts + ((long long)inst * nv + v) * 3;
                    gx = p[0]; gy = p[1]; gz = p[2];
                }
                if (d_joints || d_kps) {
                    const float s = d_kps ? cams[(long long)inst * ld_cam] : 0.f;
                    for (int e = e0; e < e1; ++e) {
                        const int k = vk_idx[e];
                        const float val = vk_val[e];
                        float qx = 0.f, qy = 0.f, qz = 0.f;
                        if (d_joints) {
                            const float* pj = d_joints + ((long long)inst * nk + k) * 3;
                            qx = pj[0]; qy = pj[1]; qz = pj[2];
                        }
                        if (d_kps) {
                            const float* pk = d_kps + ((long long)inst * nk + k) * 2;
                            qx = fmaf(s, pk[0], qx); qy = fmaf(s, pk[1], qy);
                        }
                        gx = fmaf(val, qx, gx); gy = fmaf(val, qy, gy); gz = fmaf(val, qz, gz);
                    }
                }
            }
            float* o = sGH[ii][t];
            o[0] = gx; o[1] = gy; o[2] = gz;
            o[3] = acc[ii >> 1][0][ii & 1]; o[4] = acc[ii >> 1][1][ii & 1]; o[5] = acc[ii >> 1][2][ii & 1];
#pragma unroll
            for (int c = 0; c < 3; ++c) dvp[c][q] = T[q][c] * gx + T[q][4 + c] * gy + T[q][8 + c] * gz;     // T_R^T g
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)&sDv[c][t][g4] = f32x4{dvp[c][0], dvp[c][1], dvp[c][2], dvp[c][3]};
    }
    __syncthreads();
    // d_A[i][j][r][0..3] = sum_v w[v][j] g[i][v][r] [v_posed[i][v]; 1]: item p = (i, j) owns the twelve consecutive floats of the partial
    for (int p = t; p < IBG * NJ; p += VT) {
        const int ii = p / NJ, j = p - ii * NJ;
        float a[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) a[e] = 0.f;
#pragma unroll 2
        for (int vv = 0; vv < VT; ++vv) {
            const float* gh = sGH[ii][vv];
            const float w = sW[vv][j];
            const float h0 = gh[3], h1 = gh[4], h2 = gh[5];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float wg = w * gh[r];
                a[4 * r] = fmaf(wg, h0, a[4 * r]); a[4 * r + 1] = fmaf(wg, h1, a[4 * r + 1]); a[4 * r + 2] = fmaf(wg, h2, a[4 * r + 2]);
                a[4 * r + 3] += wg;
            }
        }
        f32x4* o = (f32x4*)(partA + ((long long)tile * mp + i0) * LDA + p * 12);
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = f32x4{a[4 * r], a[4 * r + 1], a[4 * r + 2], a[4 * r + 3]};
    }
    // d_feat[i][k] = sum_c sum_v dirs[k][c][v] d_v_posed[i][c][v]: thread k reads its basis rows 16 bytes at a time
    for (int k = t; k < NFEAT; k += VT) {
        float a[IBG];
#pragma unroll
        for (int i = 0; i < IBG; ++i) a[i] = 0.f;
        for (int c = 0; c < 3; ++c) {
            const f32x4* row = (const f32x4*)(dirs + (long long)(k * 3 + c) * vpad + v0);
#pragma unroll 2
            for (int q8 = 0; q8 < VT / 8; ++q8) {
                const f32x4 d0 = row[2 * q8], d1 = row[2 * q8 + 1];
                const float d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const f32x4 lo = *(const f32x4*)&sDv[c][8 * q8 + e][0], hi = *(const f32x4*)&sDv[c][8 * q8 + e][4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        a[i] = fmaf(d[e], lo[i], a[i]);
                        a[4 + i] = fmaf(d[e], hi[i], a[4 + i]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < IBG; ++i) partF[((long long)tile * mp + i0 + i) * LDF + k] = a[i];
    }
}

// ---- pass 3 -------------------------------------------------------------- //
// d R(theta) -> d theta for R = cos I + (1 - cos) r r^T + sin skew(r), r = theta / angle, angle = ||theta + 1e-8|| (so3.h): r is NOT a
// unit vector, and both its numerator and the angle carry a derivative.
__device__ __forceinline__ void rodrigues_bwd_f32(float x, float y, float z, const float* M, float (&dth)[3]) {
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float inv = 1.0f / angle;
    const float rx = x * inv, ry = y * inv, rz = z * inv;
    const float c = cosf(angle), s = sinf(angle), oc = 1.0f - c;
    // u = the skew part of M; M r and M^T r
    const float ux = M[7] - M[5], uy = M[2] - M[6], uz = M[3] - M[1];
    const float mr0 = M[0] * rx + M[1] * ry + M[2] * rz, mr1 = M[3] * rx + M[4] * ry + M[5] * rz, mr2 = M[6] * rx + M[7] * ry + M[8] * rz;
    const float mt0 = M[0] * rx + M[3] * ry + M[6] * rz, mt1 = M[1] * rx + M[4] * ry + M[7] * rz, mt2 = M[2] * rx + M[5] * ry + M[8] * rz;
    const float rmr = rx * mr0 + ry * mr1 + rz * mr2;
    const float d_cos = (M[0] + M[4] + M[8]) - rmr;
    const float d_sin = rx * ux + ry * uy + rz * uz;
    const float drx = oc * (mr0 + mt0) + s * ux, dry = oc * (mr1 + mt1) + s * uy, drz = oc * (mr2 + mt2) + s * uz;
    const float d_angle = (c * d_sin - s * d_cos) - (drx * rx + dry * ry + drz * rz) * inv;
    dth[0] = drx * inv + d_angle * (ex * inv);
    dth[1] = dry * inv + d_angle * (ey * inv);
    dth[2] = drz * inv + d_angle * (ez * inv);
}

static_assert(NFEAT + LDA <= 512, "one thread per summed element");
__global__ __launch_bounds__(512) void smpl_bwd_tail_kernel(
    const float* __restrict__ partF, const float* __restrict__ partA, int vtiles, int mp,
    const float* __restrict__ A, const float* __restrict__ prec, const float* __restrict__ j_shapedirs,
    const int* __restrict__ parents, const float* __restrict__ theta, int ld_theta,
    const float* __restrict__ cams, int ld_cam, const float* __restrict__ joints, int nk,
    const float* __restrict__ d_kps, const float* __restrict__ d_rs,
    float* __restrict__ d_theta, float* __restrict__ d_beta, float* __restrict__ d_cams) {
    __shared__ float sdF[LDF], sdA[LDA];
    __shared__ float sR[NJ][9], sJ[NJ][3], sGR[NJ][9];
    __shared__ float dGR[NJ][9], dGt[NJ][3], dJ[NJ][3], dR[NJ][9];
    const int inst = blockIdx.x, t = threadIdx.x;
    // the partials in tile order (one element per thread; the loads of eight tiles are in flight together, the adds stay in order)
    if (t < NFEAT + LDA) {
        const bool isF = t < NFEAT;
        const float* src = isF ? partF + (long long)inst * LDF + t : partA + (long long)inst * LDA + (t - NFEAT);
        const long long stride = (long long)mp * (isF ? LDF : LDA);
        float s = 0.f;
#pragma unroll 8
        for (int tile = 0; tile < vtiles; ++tile) s += src[tile * stride];
        if (isF) sdF[t] = s; else sdA[t - NFEAT] = s;
    }
    if (t < NJ) {
        const float* pr = prec + (long long)inst * LDA + t * 12;
        const float* a = A + (long long)inst * LDA + t * 12;
#pragma unroll
        for (int e = 0; e < 9; ++e) sR[t][e] = pr[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) sJ[t][c] = pr[9 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) sGR[t][r * 3 + c] = a[r * 4 + c];
    }
    __syncthreads();
    if (t < NJ) {
        // A_j = [G_R | G_t - G_R J_j]
        const float* da = sdA + t * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dGR[t][r * 3 + c] = da[r * 4 + c] - da[r * 4 + 3] * sJ[t][c];
            dGt[t][r] = da[r * 4 + 3];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dJ[t][c] = -(sGR[t][0 * 3 + c] * da[3] + sGR[t][1 * 3 + c] * da[7] + sGR[t][2 * 3 + c] * da[11]);
        // the pose features (joints 1..23) and the rotation output itself
#pragma unroll
        for (int e = 0; e < 9; ++e)
            dR[t][e] = (t >= 1 ? sdF[11 + (t - 1) * 9 + e] : 0.f) + (d_rs ? d_rs[((long long)inst * NJ + t) * 9 + e] : 0.f);
    }
    __syncthreads();
    if (t == 0) {
        // G_i = G_p [R_i | J_i - J_p], undone from the last joint to the first (parents[i] < i)
        for (int i = NJ - 1; i >= 1; --i) {
            const int p = parents[i];
            float tl[3], dt[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) tl[c] = sJ[i][c] - sJ[p][c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    dR[i][r * 3 + c] += sGR[p][0 * 3 + r] * dGR[i][0 * 3 + c] + sGR[p][1 * 3 + r] * dGR[i][1 * 3 + c] + sGR[p][2 * 3 + r] * dGR[i][2 * 3 + c];
#pragma unroll
            for (int c = 0; c < 3; ++c) dt[c] = sGR[p][0 * 3 + c] * dGt[i][0] + sGR[p][1 * 3 + c] * dGt[i][1] + sGR[p][2 * 3 + c] * dGt[i][2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    dGR[p][r * 3 + c] += dGR[i][r * 3 + 0] * sR[i][c * 3 + 0] + dGR[i][r * 3 + 1] * sR[i][c * 3 + 1] + dGR[i][r * 3 + 2] * sR[i][c * 3 + 2]
                                         + dGt[i][r] * tl[c];
                dGt[p][r] += dGt[i][r];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { dJ[i][c] += dt[c]; dJ[p][c] -= dt[c]; }
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) dR[0][e] += dGR[0][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) dJ[0][c] += dGt[0][c];
    }
    __syncthreads();
    if (t < NJ) {
        const float* th = theta + (long long)inst * ld_theta + 3 * t;
        float dth[3];
        rodrigues_bwd_f32(th[0], th[1], th[2], dR[t], dth);
        float* o = d_theta + (long long)inst * 72 + 3 * t;
        o[0] = dth[0]; o[1] = dth[1]; o[2] = dth[2];
    } else if (t >= 32 && t < 42) {
        // beta enters as features 1..10 and through J = j_template + beta . j_shapedirs
        const int b = t - 32;
        float s = 0.f;
        for (int e = 0; e < NJ * 3; ++e) s = fmaf((&dJ[0][0])[e], j_shapedirs[b * (NJ * 3) + e], s);
        d_beta[(long long)inst * 10 + b] = sdF[1 + b] + s;
    } else if (t == 64 && d_cams) {
        // kps = s (joints_xy + t)
        float ds = 0.f, dx = 0.f, dy = 0.f;
        if (d_kps) {
            const float* cm = cams + (long long)inst * ld_cam;
            for (int k = 0; k < nk; ++k) {
                const float* g = d_kps + ((long long)inst * nk + k) * 2;
                const float* jo = joints + ((long long)inst * nk + k) * 3;
                ds = fmaf(g[0], jo[0] + cm[1], ds); ds = fmaf(g[1], jo[1] + cm[2], ds);
                dx += g[0]; dy += g[1];
            }
            dx *= cm[0]; dy *= cm[0];
        }
        float* o = d_cams + (long long)inst * 3;
        o[0] = ds; o[1] = dx; o[2] = dy;
    }
}

// ------------------------------------------------------------------------- //
// feat / A rows for m rounded up to a whole instance block; one {d_feat, d_A} partial per (vertex tile, instance)
struct SmplBwdBufs { size_t feat, A, prec, partF, partA, total; };
static SmplBwdBufs smpl_bwd_layout(int num_verts, int m) {
    WsCarver c;
    const size_t mp = ((size_t)m + IBG - 1) / IBG * IBG, vt = ((size_t)(num_verts > 0 ? num_verts : 1) + VT - 1) / VT;
    return {c.take(mp * LDF * 4), c.take(mp * LDA * 4), c.take(mp * LDA * 4), c.take(vt * mp * LDF * 4), c.take(vt * mp * LDA * 4), c.total()};
}
extern "C" size_t hmmr_smpl_bwd_workspace_bytes(const hmmr_smpl_consts_t* c, int m) {
    return (c && m > 0) ? smpl_bwd_layout(c->num_verts, m).total : 0;
}

extern "C" int hmmr_smpl_bwd(const hmmr_smpl_consts_t* c, const hmmr_smpl_grad_consts_t* g,
                             const float* theta, int ld_theta, const float* beta, int ld_beta,
                             const float* cams, int ld_cam, const float* joints, int m,
                             const float* d_verts, const float* d_joints, const float* d_kps, const float* d_rs,
                             float* d_theta, float* d_beta, float* d_cams, void* ws, size_t ws_bytes, void* stream) {
    HMMR_REQUIRE(c && g && theta && beta && d_theta && d_beta && ws, "hmmr_smpl_bwd: null argument");
    HMMR_REQUIRE(m > 0, "hmmr_smpl_bwd: m must be positive");
    HMMR_REQUIRE(d_verts || d_joints || d_kps || d_rs, "hmmr_smpl_bwd: no upstream gradient (d_verts, d_joints, d_kps and d_rs are all NULL)");
    HMMR_REQUIRE(!d_kps || (cams && joints), "hmmr_smpl_bwd: d_kps given without cams or without joints");
    HMMR_REQUIRE(!d_cams || cams, "hmmr_smpl_bwd: d_cams requested without cams");
    HMMR_REQUIRE(c->lbs_nnz >= 1 && c->lbs_nnz <= NJ, "hmmr_smpl_bwd: lbs_nnz=%d out of range", c->lbs_nnz);
    HMMR_REQUIRE(c->num_verts >= 1 && g->num_verts == c->num_verts && g->num_kps == c->num_kps,
                 "hmmr_smpl_bwd: the grad constants (%d vertices, %d keypoints) belong to another model (%d, %d)", g->num_verts, g->num_kps,
                 c->num_verts, c->num_kps);
    HMMR_REQUIRE(c->vpad >= (c->num_verts + VT - 1) / VT * VT && c->vpad % VT == 0 && ((uintptr_t)c->dirs & 15) == 0,
                 "hmmr_smpl_bwd: dirs must be 16-byte aligned with a row stride vpad=%d that is a multiple of %d covering num_verts=%d", c->vpad, VT,
                 c->num_verts);
    const SmplBwdBufs L = smpl_bwd_layout(c->num_verts, m);
    HMMR_REQUIRE(ws_bytes >= L.total, "hmmr_smpl_bwd: workspace too small (%zu bytes given, %zu needed)", ws_bytes, L.total);
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    float *feat = (float*)(base + L.feat), *A = (float*)(base + L.A), *prec = (float*)(base + L.prec);
    float *partF = (float*)(base + L.partF), *partA = (float*)(base + L.partA);
    const int mp = (m + IBG - 1) / IBG * IBG, vtiles = (c->num_verts + VT - 1) / VT;
    hipLaunchKernelGGL(smpl_bwd_pose_kernel, dim3((m + 7) / 8), dim3(256), 0, s, theta, ld_theta, beta, ld_beta, c->j_template, c->j_shapedirs,
                       c->parents, m, feat, A, prec);
    HMMR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(smpl_bwd_verts_kernel, dim3(vtiles * (mp / IBG)), dim3(VT), 0, s, c->dirs, c->vpad, (const float*)feat, (const float*)A,
                       c->lbs_idx, c->lbs_w, c->lbs_nnz, g->vk_ptr, g->vk_idx, g->vk_val, c->num_verts, c->num_kps, m, mp, cams, ld_cam,
                       d_verts, d_joints, d_kps, partF, partA);
    HMMR_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(smpl_bwd_tail_kernel, dim3(m), dim3(512), 0, s, (const float*)partF, (const float*)partA, vtiles, mp, (const float*)A,
                       (const float*)prec, c->j_shapedirs, c->parents, theta, ld_theta, cams, ld_cam, joints, c->num_kps, d_kps, d_rs,
                       d_theta, d_beta, d_cams);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
