// Host-only arithmetic of the whole-video call (include/hmmr_hip.h: hmmr_video_plan, hmmr_record_layout): the sliding-window plan of
// Tester.predict_all_images (src/evaluation/tester.py:281-289) and the packed per-frame record of make_fetch_dict (:216-227).  No HIP
// include and no HIP call: the file compiles alone (with a definition of hmmr_set_error) and runs on a machine without a GPU.
#include <stdint.h>

#include "hmmr_hip.h"

void hmmr_set_error(const char* fmt, ...);

namespace {
inline int ceil_div(int a, int b) { return (int)(((long long)a + b - 1) / b); }
}  // namespace

extern "C" int hmmr_video_plan(int n, int T, int fov, int max_frames, int max_windows, hmmr_video_plan_t* out) {
    if (!out) { hmmr_set_error("hmmr_video_plan: null argument"); return -1; }
    if (fov < 1 || fov % 2 == 0) { hmmr_set_error("hmmr_video_plan: fov=%d must be odd and >= 1", fov); return -1; }
    const int margin = (fov - 1) / 2;
    if (T < 1 || (long long)T - 2LL * margin < 1) {
        hmmr_set_error("hmmr_video_plan: a window of T=%d frames keeps none under fov=%d (g = T - (fov - 1) < 1)", T, fov);
        return -1;
    }
    if (n < 0 || max_frames < 1 || max_windows < 1) {
        hmmr_set_error("hmmr_video_plan: n=%d must be >= 0, max_frames=%d and max_windows=%d >= 1", n, max_frames, max_windows);
        return -1;
    }
    hmmr_video_plan_t p = {};
    p.n = n; p.T = T; p.fov = fov;
    p.margin = margin; p.g = T - 2 * margin;
    p.n_windows = ceil_div(n, p.g);
    p.max_frames = max_frames; p.max_windows = max_windows;
    p.resnet_passes = ceil_div(n, max_frames);
    p.tail_passes = ceil_div(p.n_windows, max_windows);
    *out = p;
    return 0;
}

extern "C" int hmmr_record_layout(int num_kps, int num_verts, int num_containers, int32_t* field_offsets, int64_t* ld_rec) {
    if (!field_offsets && !ld_rec) { hmmr_set_error("hmmr_record_layout: null argument"); return -1; }
    if (num_kps < 1 || num_verts < 1 || num_containers < 1 || num_containers > HMMR_MAX_REGRESSORS) {
        hmmr_set_error("hmmr_record_layout: bad shape (num_kps=%d, num_verts=%d, num_containers=%d)", num_kps, num_verts, num_containers);
        return -1;
    }
    // cams, joints, kps, poses, shapes, verts, omegas (tester.py:216-227)
    const int64_t size[7] = {3, 3LL * num_kps, 2LL * num_kps, 24 * 9, 10, 3LL * num_verts, 85};
    int64_t present = 0;
    for (int f = 0; f < 7; ++f) present += size[f];
    const int D = num_containers - 1;
    const int64_t total = present * num_containers;
    if (total > INT32_MAX) { hmmr_set_error("hmmr_record_layout: a record of %lld floats has offsets beyond int32", (long long)total); return -1; }
    if (field_offsets) {
        int64_t off = 0;
        for (int f = 0; f < 7; ++f) { field_offsets[f] = (int32_t)off; off += size[f]; }
        for (int f = 0; f < 7; ++f) {                    // field f of the deltas: [D][...]
            for (int d = 0; d < D; ++d) field_offsets[(d + 1) * 7 + f] = (int32_t)(off + d * size[f]);
            off += D * size[f];
        }
    }
    if (ld_rec) *ld_rec = total;
    return 0;
}
