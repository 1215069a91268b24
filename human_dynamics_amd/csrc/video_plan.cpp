// Host-only arithmetic of the whole-video calls (include/hmmr_hip.h: hmmr_video_plan, hmmr_tracks_plan, hmmr_record_layout): the sliding-window plan of
// Tester.predict_all_images (src/evaluation/tester.py:281-289) and the packed per-frame record of make_fetch_dict (:216-227).  No HIP
// include and no HIP call: the file compiles alone (with a definition of hmmr_set_error) and runs on a machine without a GPU.
#include <stdint.h>

#include "hmmr_hip.h"

void hmmr_set_error(const char* fmt, ...);

namespace {
inline int ceil_div(int a, int b) { return (int)(((long long)a + b - 1) / b); }
}  // namespace

// ----------------------------------------------------------------------------------------------------------------------------------
// Several tracks one after the other along the frame axis (hmmr_predict_tracks): every track has its own zero-image padding, its own
// window grid and its own kept rows; the windows are numbered globally, track after track (include/hmmr_hip.h: the ragged rule).  A
// video is the one-track case {0, n}, and hmmr_video_plan is that plan under the one-video struct.

// the refusals every entry point that takes track_offsets shares (csrc/windows.hip, csrc/video.cpp); `who` names the caller
int hmmr_tracks_check_offsets(const char* who, const int32_t* off, int n_tracks) {
    if (!off) { hmmr_set_error("%s: null track_offsets (n_tracks + 1 host values, also for n_tracks = 0)", who); return -1; }
    if (n_tracks < 0) { hmmr_set_error("%s: n_tracks=%d must not be negative", who, n_tracks); return -1; }
    if (off[0] != 0) { hmmr_set_error("%s: track_offsets[0]=%d must be 0", who, (int)off[0]); return -1; }
    for (int k = 0; k < n_tracks; ++k)
        if (off[k + 1] < off[k]) {
            hmmr_set_error("%s: track_offsets must not decrease (track_offsets[%d]=%d > track_offsets[%d]=%d)", who, k, (int)off[k], k + 1,
                           (int)off[k + 1]);
            return -1;
        }
    // row n_frames is the zero image's (phi [n_frames + 1][c]) and must be an int like every other row number
    if (off[n_tracks] >= INT32_MAX) {
        hmmr_set_error("%s: %d frames in all are beyond what 32-bit row numbers address (at most %d)", who, (int)off[n_tracks], INT32_MAX - 1);
        return -1;
    }
    return 0;
}

namespace {
// What both plans refuse and compute alike.  off: n_tracks + 1 values that start at 0 and do not decrease (hmmr_tracks_check_offsets,
// or {0, n} of hmmr_video_plan -- the only caller whose last value may be negative, or INT32_MAX); `who` names the public caller.
int plan_windows(const char* who, const int32_t* off, int n_tracks, int T, int fov, int max_frames, int max_windows, hmmr_tracks_plan_t* out) {
    if (fov < 1 || fov % 2 == 0) { hmmr_set_error("%s: fov=%d must be odd and >= 1", who, fov); return -1; }
    const int margin = (fov - 1) / 2;
    if (T < 1 || (long long)T - 2LL * margin < 1) {
        hmmr_set_error("%s: a window of T=%d frames keeps none under fov=%d (g = T - (fov - 1) < 1)", who, T, fov);
        return -1;
    }
    if (off[n_tracks] < 0 || max_frames < 1 || max_windows < 1) {
        hmmr_set_error("%s: n=%d must be >= 0, max_frames=%d and max_windows=%d >= 1", who, (int)off[n_tracks], max_frames, max_windows);
        return -1;
    }
    hmmr_tracks_plan_t p = {};
    p.n_tracks = n_tracks; p.T = T; p.fov = fov;
    p.margin = margin; p.g = T - 2 * margin;
    p.n_frames = off[n_tracks];
    for (int k = 0; k < n_tracks; ++k) p.n_windows += ceil_div(off[k + 1] - off[k], p.g);     // <= n_frames: no overflow
    p.max_frames = max_frames; p.max_windows = max_windows;
    p.resnet_passes = ceil_div(p.n_frames, max_frames);
    p.tail_passes = ceil_div(p.n_windows, max_windows);
    *out = p;
    return 0;
}
}  // namespace

// hmmr_tracks_plan under the name of the entry point that plans (csrc/video.cpp: its refusals name the call that was made)
int hmmr_tracks_plan_as(const char* who, const int32_t* track_offsets, int n_tracks, int T, int fov, int max_frames, int max_windows,
                        hmmr_tracks_plan_t* out) {
    if (hmmr_tracks_check_offsets(who, track_offsets, n_tracks)) return -1;
    return plan_windows(who, track_offsets, n_tracks, T, fov, max_frames, max_windows, out);
}

extern "C" int hmmr_tracks_plan(const int32_t* track_offsets, int n_tracks, int T, int fov, int max_frames, int max_windows,
                                hmmr_tracks_plan_t* out) {
    if (!out) { hmmr_set_error("hmmr_tracks_plan: null argument"); return -1; }
    return hmmr_tracks_plan_as("hmmr_tracks_plan", track_offsets, n_tracks, T, fov, max_frames, max_windows, out);
}

// one video: no offsets check -- n = INT32_MAX is a plan (its ceil_div is 64-bit), though no call can run it
extern "C" int hmmr_video_plan(int n, int T, int fov, int max_frames, int max_windows, hmmr_video_plan_t* out) {
    if (!out) { hmmr_set_error("hmmr_video_plan: null argument"); return -1; }
    const int32_t off[2] = {0, n};
    hmmr_tracks_plan_t t;
    if (plan_windows("hmmr_video_plan", off, 1, T, fov, max_frames, max_windows, &t)) return -1;
    *out = {n, T, fov, t.margin, t.g, t.n_windows, max_frames, max_windows, t.resnet_passes, t.tail_passes};      // (the struct's order)
    return 0;
}

// One walk over the tracks: the owner of global window w is the track k with B_k <= w < B_k + W_k (a track without a frame owns none).
extern "C" int hmmr_tracks_window_owner(const int32_t* track_offsets, int n_tracks, int g, int w, int* track, int* local_window) {
    if (hmmr_tracks_check_offsets("hmmr_tracks_window_owner", track_offsets, n_tracks)) return -1;
    if (g < 1 || w < 0) { hmmr_set_error("hmmr_tracks_window_owner: g=%d must be >= 1 and w=%d >= 0", g, w); return -1; }
    int base = 0;
    for (int k = 0; k < n_tracks; ++k) {
        const int wk = ceil_div(track_offsets[k + 1] - track_offsets[k], g);
        if (w < base + wk) {
            if (track) *track = k;
            if (local_window) *local_window = w - base;
            return 0;
        }
        base += wk;
    }
    hmmr_set_error("hmmr_tracks_window_owner: window %d is beyond the %d windows of these tracks", w, base);
    return -1;
}

// The output rows of windows [w0, w0 + nw), nw >= 1: they start at the first window's first kept frame and end behind the last
// window's last one; the kept rows of consecutive windows are consecutive, also across tracks (an empty track lies between no rows).
extern "C" int hmmr_tracks_window_rows(const int32_t* track_offsets, int n_tracks, int g, int w0, int n_windows, int* o0, int* keep) {
    if (n_windows < 1) { hmmr_set_error("hmmr_tracks_window_rows: n_windows=%d must be >= 1", n_windows); return -1; }
    if ((long long)w0 + n_windows - 1 > INT32_MAX) { hmmr_set_error("hmmr_tracks_window_rows: window range beyond int"); return -1; }
    int k0, l0, k1, l1;
    if (hmmr_tracks_window_owner(track_offsets, n_tracks, g, w0, &k0, &l0)) return -1;
    if (hmmr_tracks_window_owner(track_offsets, n_tracks, g, w0 + n_windows - 1, &k1, &l1)) return -1;
    const long long first = (long long)track_offsets[k0] + (long long)l0 * g;
    const long long n1 = track_offsets[k1 + 1] - track_offsets[k1], e1 = ((long long)l1 + 1) * g;
    const long long end = track_offsets[k1] + (e1 < n1 ? e1 : n1);
    if (o0) *o0 = (int)first;
    if (keep) *keep = (int)(end - first);
    return 0;
}

extern "C" int hmmr_tracks_tail_pass(const int32_t* track_offsets, int n_tracks, const hmmr_tracks_plan_t* plan, int i, int* w0,
                                     int* n_windows, int* o0, int* keep) {
    if (!plan) { hmmr_set_error("hmmr_tracks_tail_pass: null plan"); return -1; }
    if (i < 0 || i >= plan->tail_passes || plan->max_windows < 1 || plan->g < 1) {
        hmmr_set_error("hmmr_tracks_tail_pass: pass %d of %d", i, plan->tail_passes);
        return -1;
    }
    const int first = i * plan->max_windows;                 // (i < tail_passes: first < n_windows, no overflow)
    const int nw = plan->max_windows < plan->n_windows - first ? plan->max_windows : plan->n_windows - first;
    if (hmmr_tracks_window_rows(track_offsets, n_tracks, plan->g, first, nw, o0, keep)) return -1;
    if (w0) *w0 = first;
    if (n_windows) *n_windows = nw;
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
