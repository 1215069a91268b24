// Axis-angle -> rotation matrix, the one device implementation (smpl.hip: smpl_pose_kernel; eval_metrics.hip:
// hmmr_axis_angle_to_rotmat).
#pragma once
#include <hip/hip_runtime.h>

// batch_rodrigues, src/tf_smpl/batch_lbs.py:42-60, in fp32 like the reference graph: angle = ||theta + 1e-8||,
// r = theta / angle, R = cos*I + (1-cos)*r r^T + sin*skew(r) (row-major R[9]).
__device__ __forceinline__ void rodrigues_f32(float x, float y, float z, float (&R)[9]) {
    // batch_lbs.py:48-50: angle = ||theta + 1e-8||, r = theta / angle
    const float ex = x + 1e-8f, ey = y + 1e-8f, ez = z + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = x / angle, ry = y / angle, rz = z / angle;
    const float c = cosf(angle), s = sinf(angle), oc = 1.0f - c;
    // R = cos*I + (1-cos)*r r^T + sin*skew(r)      (batch_lbs.py:56-59, :24-36)
    R[0] = c + oc * rx * rx;      R[1] = oc * rx * ry - s * rz; R[2] = oc * rx * rz + s * ry;
    R[3] = oc * ry * rx + s * rz; R[4] = c + oc * ry * ry;      R[5] = oc * ry * rz - s * rx;
    R[6] = oc * rz * rx - s * ry; R[7] = oc * rz * ry + s * rx; R[8] = c + oc * rz * rz;
}
