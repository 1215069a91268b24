// hmmr_predict_tracks and hmmr_predict_video (include/hmmr_hip.h): Tester.predict_all_images (src/evaluation/tester.py:260-312) as ONE call of the C ABI -- the
// frames of every track on the device in, the packed per-frame records on the device out, no Python and no torch in between.  There is
// one driver, over tracks; a video is the one-track case {0, n}.  The call only sequences the stage entry points on the caller's
// stream: ResNet passes into phi, then per tail pass gather -> f_movie (or the hallucinator) -> keep -> IEF -> SMPL records.  It owns no
// kernel and makes no HIP call itself; every check that a stage would make is made here first, for every pass, so that a refused call
// has queued nothing.
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "hmmr_hip.h"
#include "workspace.h"

void hmmr_set_error(const char* fmt, ...);
int hmmr_tracks_plan_as(const char* who, const int32_t* track_offsets, int n_tracks, int T, int fov, int max_frames, int max_windows,
                        hmmr_tracks_plan_t* out);      // csrc/video_plan.cpp: hmmr_tracks_plan with the refusals under the caller's name

#define VIDEO_REQUIRE(cond, ...) do { if (!(cond)) { hmmr_set_error(__VA_ARGS__); return -1; } } while (0)

namespace {

constexpr int C = 2048;                  // feature width (phi, movie strips)
inline int imin(int a, int b) { return a < b ? a : b; }

// the carve of `ws`: phi, then ONE region that first serves the ResNet passes and afterwards the tail passes (same stream: in order)
struct Carve {
    size_t phi, region;                                  // offsets
    size_t resnet_bytes;                                 // inside the region, from its start
    size_t windows, strips, kept, omegas, movie_ws, ief_ws, smpl_ws;      // offsets inside the region
    size_t movie_bytes, ief_bytes, smpl_bytes;
    size_t total;
};

struct TailPass { int w0, nw, o0, keep; };      // hmmr_tracks_tail_pass

// model pointers and everything the stages would refuse that does not depend on the frame count
int check_model(const hmmr_model_t* m, const char* who) {
    VIDEO_REQUIRE(m && m->resnet && m->ief && m->smpl, "%s: null model, resnet, ief or smpl", who);
    VIDEO_REQUIRE(!m->temporal != !m->hallucinator, "%s: exactly one of temporal ('pred') and hallucinator ('hal') must be set", who);
    for (int dt : {m->resnet->dtype, m->temporal ? m->temporal->dtype : m->hallucinator->dtype, m->ief->dtype})
        VIDEO_REQUIRE(dt == HMMR_F32 || dt == HMMR_BF16 || dt == HMMR_F16X3, "%s: bad dtype %d", who, dt);
    VIDEO_REQUIRE(m->resnet->unit[0].c_in == 64 && m->resnet->unit[HMMR_RESNET_UNITS - 1].depth == C, "%s: bad ResNet unit table", who);
    VIDEO_REQUIRE(!m->temporal || (m->temporal->num_blocks >= 1 && m->temporal->num_blocks <= HMMR_MAX_TEMPORAL_BLOCKS),
                  "%s: bad temporal num_blocks", who);
    const hmmr_ief_weights_t* w = m->ief;
    VIDEO_REQUIRE(w->num_regressors >= 1 && w->num_regressors <= HMMR_MAX_REGRESSORS, "%s: bad ief num_regressors", who);
    for (int r = 0; r < w->num_regressors; ++r) {
        const int nd = r == 0 ? 85 : (w->no_optcam ? 75 : 72);
        VIDEO_REQUIRE(w->reg[r].nd == nd, "%s: ief regressor %d has nd=%d (expected %d)", who, r, w->reg[r].nd, nd);
    }
    const hmmr_smpl_consts_t* s = m->smpl;
    VIDEO_REQUIRE(s->num_verts >= 1 && s->num_kps >= 1 && s->lbs_nnz >= 1 && s->lbs_nnz <= 24, "%s: bad SMPL constants (num_verts=%d, num_kps=%d, lbs_nnz=%d)",
                  who, s->num_verts, s->num_kps, s->lbs_nnz);
    VIDEO_REQUIRE(s->vpad % 128 == 0 && s->vpad >= s->num_verts, "%s: SMPL vpad=%d must be a multiple of 128 covering num_verts=%d", who, s->vpad,
                  s->num_verts);
    return 0;
}

// what the tail's buffers must hold: the largest window count, the largest kept-row count and the largest workspace of every stage
// over the passes added (the stages' queries are asked per pass size, never assumed monotone)
struct TailNeeds { int mw, mk; size_t movie_bytes, ief_bytes, smpl_bytes; };
void tail_needs_add(const hmmr_model_t* m, int T, const TailPass& t, TailNeeds* need) {
    auto max2 = [](size_t a, size_t b) { return a > b ? a : b; };
    const int R = m->ief->num_regressors;
    const size_t movie = m->temporal ? hmmr_temporal_workspace_bytes(t.nw, T, m->temporal->dtype)
                                     : hmmr_hallucinator_workspace_bytes(t.nw * T, m->hallucinator->dtype);
    const size_t ief = hmmr_ief_workspace_bytes(t.keep, R, m->ief->dtype), smpl = hmmr_smpl_workspace_bytes(R * t.keep);
    need->mw = t.nw > need->mw ? t.nw : need->mw;
    need->mk = t.keep > need->mk ? t.keep : need->mk;
    need->movie_bytes = max2(need->movie_bytes, movie);
    need->ief_bytes = max2(need->ief_bytes, ief);
    need->smpl_bytes = max2(need->smpl_bytes, smpl);
}

// n > 0 frames in all, at most resnet_frames of them (and the zero image) in one ResNet pass
int carve(const hmmr_model_t* m, const char* who, int n, int resnet_frames, int T, const TailNeeds& need, Carve* out) {
    Carve c = {};
    const int R = m->ief->num_regressors;
    WsCarver outer, tail;                                // tail: offsets inside the region
    c.phi = outer.take((size_t)(n + 1) * C * 4);
    c.resnet_bytes = hmmr_resnet50_workspace_bytes(resnet_frames + 1, m->resnet->dtype);
    VIDEO_REQUIRE(c.resnet_bytes > 0, "%s: no ResNet workspace for this dtype", who);
    c.windows = tail.take((size_t)need.mw * T * C * 4);
    c.strips = tail.take((size_t)need.mw * T * C * 4);
    c.kept = tail.take((size_t)need.mk * C * 4);
    c.omegas = tail.take((size_t)R * need.mk * 85 * 4);
    c.movie_bytes = need.movie_bytes; c.ief_bytes = need.ief_bytes; c.smpl_bytes = need.smpl_bytes;
    VIDEO_REQUIRE(c.movie_bytes && c.ief_bytes && c.smpl_bytes, "%s: a stage reports no workspace for this model", who);
    c.movie_ws = tail.take(c.movie_bytes);
    c.ief_ws = tail.take(c.ief_bytes);
    c.smpl_ws = tail.take(c.smpl_bytes);
    c.region = outer.take(tail.total() > c.resnet_bytes ? tail.total() : c.resnet_bytes);      // the union: ResNet passes first, tail passes after
    c.total = outer.total();
    *out = c;
    return 0;
}

// n_frames > 0.  A tail pass may end inside a track's last, short window, so the kept-row count varies from pass to pass: every pass is
// asked (a stage's query runs only when the pass's sizes differ from the pass before: for one track, the first pass and the last).
int carve_tracks(const hmmr_model_t* m, const char* who, const int32_t* off, int n_tracks, const hmmr_tracks_plan_t& p, Carve* out) {
    TailNeeds need = {};
    TailPass last = {0, -1, 0, -1};
    for (int i = 0; i < p.tail_passes; ++i) {
        TailPass t;
        if (hmmr_tracks_tail_pass(off, n_tracks, &p, i, &t.w0, &t.nw, &t.o0, &t.keep)) return -1;
        if (t.nw != last.nw || t.keep != last.keep) tail_needs_add(m, p.T, t, &need);
        last = t;
    }
    return carve(m, who, p.n_frames, imin(p.n_frames, p.max_frames), p.T, need, out);
}

// the record: every field of every container ends inside it
int check_record(const hmmr_model_t* model, const int32_t* field_offsets, int64_t ld_rec, const char* who) {
    VIDEO_REQUIRE(field_offsets, "%s: null field_offsets", who);
    const int64_t K = model->smpl->num_kps, V = model->smpl->num_verts;
    const int64_t size[7] = {3, 3 * K, 2 * K, 24 * 9, 10, 3 * V, 85};
    for (int r = 0; r < model->ief->num_regressors; ++r)
        for (int f = 0; f < 7; ++f) {
            const int64_t o = field_offsets[r * 7 + f];
            VIDEO_REQUIRE(o >= 0 && o + size[f] <= ld_rec, "%s: field %d of container %d (offset %lld, %lld floats) does not fit ld_rec=%lld", who,
                          f, r, (long long)o, (long long)size[f], (long long)ld_rec);
        }
    return 0;
}

// the unit table against both pass sizes the ResNet will see (hmmr_resnet50_plan: host only); last = frames of the last pass
int check_units(const hmmr_model_t* model, int last, int passes, int max_frames) {
    hmmr_unit_plan_t units[HMMR_RESNET_UNITS];
    if (hmmr_resnet50_plan(model->resnet, last + 1, units)) return -1;
    if (passes > 1 && hmmr_resnet50_plan(model->resnet, max_frames, units)) return -1;
    return 0;
}

// ResNet passes over n frames into phi [n + 1][C]; the zero image rides on the last pass
int resnet_passes(const hmmr_model_t* model, const float* images, int n, int max_frames, int passes, float* phi, char* region, const Carve& c,
                  void* stream) {
    for (int i = 0; i < passes; ++i) {
        const int f0 = i * max_frames, nf = imin(max_frames, n - f0), n_zero = i == passes - 1;
        if (hmmr_resnet50_fwd(model->resnet, images + (size_t)f0 * 224 * 224 * 3, nf, n_zero, phi + (size_t)f0 * C, region, c.resnet_bytes,
                              stream, nullptr))
            return -2;
    }
    return 0;
}

size_t workspace_bytes(const char* who, const hmmr_model_t* model, const int32_t* off, int n_tracks, int max_frames, int max_windows) {
    hmmr_tracks_plan_t p;
    if (check_model(model, who) || hmmr_tracks_plan_as(who, off, n_tracks, model->sequence_length, model->fov, max_frames, max_windows, &p)) return 0;
    const int32_t one[2] = {0, 1};
    if (p.n_frames == 0) {                                 // (nothing to run needs nothing: report what one frame takes, never 0 for a good model)
        off = one, n_tracks = 1;
        if (hmmr_tracks_plan_as(who, off, n_tracks, model->sequence_length, model->fov, max_frames, max_windows, &p)) return 0;
    }
    Carve c;
    return carve_tracks(model, who, off, n_tracks, p, &c) ? 0 : c.total;
}

int predict(const char* who, const hmmr_model_t* model, const float* images, const int32_t* off, int n_tracks, float* rec, int64_t ld_rec,
            const int32_t* field_offsets, int max_frames, int max_windows, void* ws, size_t ws_bytes, void* stream) {
    if (check_model(model, who)) return -1;
    hmmr_tracks_plan_t p;
    if (hmmr_tracks_plan_as(who, off, n_tracks, model->sequence_length, model->fov, max_frames, max_windows, &p)) return -1;
    if (check_record(model, field_offsets, ld_rec, who)) return -1;
    const int R = model->ief->num_regressors;
    if (p.n_frames == 0) return 0;
    VIDEO_REQUIRE(images && rec && ws, "%s: null images, rec or ws", who);
    VIDEO_REQUIRE(((uintptr_t)ws & 255u) == 0, "%s: ws must be 256-byte aligned", who);
    VIDEO_REQUIRE(((uintptr_t)images & 15u) == 0, "%s: images must be 16-byte aligned (hmmr_resnet50_fwd reads them as aligned groups of 4 floats)", who);
    Carve c;
    if (carve_tracks(model, who, off, n_tracks, p, &c)) return -1;
    VIDEO_REQUIRE(ws_bytes >= c.total, "%s: workspace too small (%zu < %zu)", who, ws_bytes, c.total);
    if (check_units(model, p.n_frames - (p.resnet_passes - 1) * p.max_frames, p.resnet_passes, p.max_frames)) return -1;

    char* base = (char*)ws;
    float* phi = (float*)(base + c.phi);
    char* region = base + c.region;
    if (resnet_passes(model, images, p.n_frames, p.max_frames, p.resnet_passes, phi, region, c, stream)) return -2;
    float* windows = (float*)(region + c.windows);
    float* strips = (float*)(region + c.strips);
    float* kept = (float*)(region + c.kept);
    float* omegas = (float*)(region + c.omegas);
    for (int i = 0; i < p.tail_passes; ++i) {
        TailPass t;
        if (hmmr_tracks_tail_pass(off, n_tracks, &p, i, &t.w0, &t.nw, &t.o0, &t.keep)) return -2;      // (carve_tracks walked every pass: cannot fail)
        if (hmmr_gather_windows_tracks(phi, phi + (size_t)p.n_frames * C, off, n_tracks, t.w0, t.nw, p.T, p.margin, p.g, C, windows, stream)) return -2;
        if (model->temporal) {
            if (hmmr_temporal_fwd(model->temporal, windows, t.nw, p.T, strips, region + c.movie_ws, c.movie_bytes, stream)) return -2;
        } else if (hmmr_hallucinator_fwd(model->hallucinator, windows, t.nw * p.T, strips, region + c.movie_ws, c.movie_bytes, stream)) {
            return -2;
        }
        if (hmmr_keep_rows_tracks(strips, off, n_tracks, t.w0, t.nw, p.T, p.margin, p.g, C, kept, C, stream)) return -2;
        if (hmmr_ief_fwd(model->ief, kept, t.keep, omegas, region + c.ief_ws, c.ief_bytes, stream)) return -2;
        if (hmmr_smpl_fwd_records(model->smpl, omegas, R, t.keep, rec + (size_t)t.o0 * (size_t)ld_rec, ld_rec, field_offsets,
                                  region + c.smpl_ws, c.smpl_bytes, stream))
            return -2;
    }
    return 0;
}

}  // namespace

extern "C" size_t hmmr_predict_tracks_workspace_bytes(const hmmr_model_t* model, const int32_t* track_offsets, int n_tracks, int max_frames,
                                                      int max_windows) {
    return workspace_bytes("hmmr_predict_tracks_workspace_bytes", model, track_offsets, n_tracks, max_frames, max_windows);
}

extern "C" int hmmr_predict_tracks(const hmmr_model_t* model, const float* images, const int32_t* track_offsets, int n_tracks, float* rec,
                                   int64_t ld_rec, const int32_t* field_offsets, int max_frames, int max_windows, void* ws, size_t ws_bytes,
                                   void* stream) {
    return predict("hmmr_predict_tracks", model, images, track_offsets, n_tracks, rec, ld_rec, field_offsets, max_frames, max_windows, ws, ws_bytes,
                   stream);
}

// A video is one track.  n < 0 is refused here: as an offset it would read "track_offsets must not decrease".
extern "C" size_t hmmr_predict_video_workspace_bytes(const hmmr_model_t* model, int n, int max_frames, int max_windows) {
    if (n < 0) { hmmr_set_error("hmmr_predict_video_workspace_bytes: n=%d must not be negative", n); return 0; }
    const int32_t off[2] = {0, n};
    return workspace_bytes("hmmr_predict_video_workspace_bytes", model, off, 1, max_frames, max_windows);
}

extern "C" int hmmr_predict_video(const hmmr_model_t* model, const float* images, int n, float* rec, int64_t ld_rec,
                                  const int32_t* field_offsets, int max_frames, int max_windows, void* ws, size_t ws_bytes,
                                  void* stream) {
    VIDEO_REQUIRE(n >= 0, "hmmr_predict_video: n=%d must not be negative", n);
    const int32_t off[2] = {0, n};
    return predict("hmmr_predict_video", model, images, off, 1, rec, ld_rec, field_offsets, max_frames, max_windows, ws, ws_bytes, stream);
}
