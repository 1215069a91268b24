// Device helpers shared by the kernels that work in image space around the path:
// the crop before it (preprocess.hip), the hand-off after it (handoff.hip) and the rasteriser (render.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace hmmr_img {

// OpenCV's INTER_LINEAR taps along one axis for destination index d of a src -> dst resize:
// pixel-centre alignment in float32, float32 weights, edge clamp (cv2's double-image path).
__device__ __forceinline__ void taps(int d, int src, int dst, int& s0, int& s1, double& w0, double& w1) {
    float f = (float)(((double)d + 0.5) * ((double)src / (double)dst) - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    s0 = s; s1 = min(s + 1, src - 1);
    w0 = (double)(1.0f - f); w1 = (double)f;
}

// TF 1.8 ResizeBilinear's taps (align_corners=False) along one axis for destination index d of a src -> dst resize:
// NO half-pixel offset, all float32 -- in = d * (src / dst), lo = (int)in, hi = min(lo + 1, src - 1), lerp = in - lo.
// The caller interpolates lo + (hi - lo) * lerp.  The clamp of lo changes nothing for 0 <= d < dst (in < src there);
// it keeps the reads inside the frame when a caller hands over a row that is not a size.
__device__ __forceinline__ void tf_taps(int d, int src, int dst, int& lo, int& hi, float& lerp) {
    const float in = (float)d * ((float)src / (float)dst);
    lo = max(min((int)in, src - 1), 0);
    hi = min(lo + 1, src - 1);
    lerp = in - (float)lo;
}

struct FrameCam { float s, tx, ty; };

// The weak-perspective camera [s, tx, ty] moved from the 224x224 crop to the squared (possibly down-scaled) original
// image (visualize_img_orig, nmr_renderer.py:368-401), in fp64 and rounded to fp32 as the reference does.
// geom row = {undo_scale, start_x, start_y, proc_size, img_size}; geom == NULL: stay in the crop
__device__ __forceinline__ FrameCam frame_camera(const float* cam, const float* g) {
    FrameCam c = {cam[0], cam[1], cam[2]};
    if (!g) return c;
    const double undo = g[0], sx = g[1], sy = g[2], proc = g[3], size = g[4];
    const double crop_s = proc * (double)cam[0] * 0.5;                 // camera in crop pixels
    const double half = (2.0 / (double)cam[0]) * 0.5;
    const double crop_tx = (double)cam[1] + half, crop_ty = (double)cam[2] + half;
    const double orig_s = crop_s * undo;                               // camera in original pixels
    const double orig_tx = crop_tx + (sx - proc) / crop_s, orig_ty = crop_ty + (sy - proc) / crop_s;
    const double k = 2.0 / size;                                       // normalised original image
    c.s = (float)(orig_s * k);
    c.tx = (float)(orig_tx - 1.0 / (k * orig_s));
    c.ty = (float)(orig_ty - 1.0 / (k * orig_s));
    return c;
}

}  // namespace hmmr_img
