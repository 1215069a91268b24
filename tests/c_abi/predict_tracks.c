/* Every tracked person of a video through the boundary WITHOUT Python, as a C program: tests/c_abi/predict_video.c with an offsets
 * argument.  The frames file holds the tracks' frames one after the other; <offsets> is the comma-separated list of the n_tracks + 1
 * track offsets ("0,4,4,13": tracks of 4, 0 and 9 frames).  Read a dump of all checkpoint variables and of the SMPL source arrays (the format of pack_and_run.c: count, then per variable name length, name,
 * numel, fp32 data; the body model's arrays are the entries smpl/v_template, smpl/shapedirs, smpl/posedirs, smpl/J_regressor,
 * smpl/lbs_weights, smpl/kp_regressor and smpl/parents, the last as fp32 values of small integers), pack every stage with the C-side
 * packers (hmmr_pack_resnet / _temporal / _ief / _smpl), size everything with the *_bytes and workspace queries, call hmmr_predict_tracks
 * on frames read from a file, read hmmr_run_flags and write the packed per-frame records.  tests/test_gpu_tracks_program.py compiles
 * it with hipcc, runs it and compares every track's records with the Python mirror's for that track alone, byte for byte.
 *   predict_tracks <vars.bin> <frames.bin> <offsets> <dtype> <records_out.bin> */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hmmr_hip.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 2; } } while (0)
#define FAIL(what) do { fprintf(stderr, "%s: %s\n", what, hmmr_last_error()); return 1; } while (0)

static const hmmr_var_t* find_var(const hmmr_var_t* vars, int n, const char* name) {
    for (int i = 0; i < n; ++i)
        if (!strcmp(vars[i].name, name)) return &vars[i];
    fprintf(stderr, "the dump has no variable %s\n", name);
    return NULL;
}

/* one blob per stage: the packer fills a host image, one hipMemcpy moves it */
static int upload(void* host, size_t nb, void* dev) {
    CHECK(hipMemcpy(dev, host, nb, hipMemcpyHostToDevice));
    free(host);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: predict_tracks vars.bin frames.bin off0,off1,... dtype records.bin\n"); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int n_vars = 0;
    if (fread(&n_vars, 4, 1, f) != 1) return 1;
    hmmr_var_t* vars = (hmmr_var_t*)calloc((size_t)n_vars, sizeof(hmmr_var_t));
    for (int i = 0; i < n_vars; ++i) {
        int len = 0; long long numel = 0;
        if (fread(&len, 4, 1, f) != 1) return 1;
        char* name = (char*)calloc((size_t)len + 1, 1);
        if (fread(name, 1, (size_t)len, f) != (size_t)len || fread(&numel, 8, 1, f) != 1) return 1;
        float* data = (float*)malloc((size_t)numel * 4);
        if (fread(data, 4, (size_t)numel, f) != (size_t)numel) return 1;
        vars[i].name = name; vars[i].data = data; vars[i].numel = numel;
    }
    fclose(f);
    int32_t track_offsets[256];
    int n_offsets = 0;
    for (const char* p = argv[3]; *p && n_offsets < 256;) {
        char* end;
        track_offsets[n_offsets++] = (int32_t)strtol(p, &end, 10);
        if (end == p) { fprintf(stderr, "bad offsets list %s\n", argv[3]); return 1; }
        p = *end == ',' ? end + 1 : end;
    }
    if (n_offsets < 1) { fprintf(stderr, "the offsets list holds at least the leading 0\n"); return 1; }
    const int n_tracks = n_offsets - 1, dtype = atoi(argv[4]);
    if (hmmr_abi_version() != HMMR_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    const int num_conv_layers = 3, delta_t[2] = {-5, 5}, T = 20;      /* the Tester configuration of the published checkpoints */

    /* ---- the four stages, each packed into one blob */
    hmmr_resnet_weights_t rw; hmmr_temporal_weights_t tw; hmmr_ief_weights_t iw; hmmr_smpl_consts_t sc;
    void *host, *dev; size_t nb;

    if (!(nb = hmmr_pack_resnet_bytes(vars, n_vars, dtype))) FAIL("hmmr_pack_resnet_bytes");
    host = malloc(nb); CHECK(hipMalloc(&dev, nb));
    if (hmmr_pack_resnet(vars, n_vars, dtype, host, nb, dev, &rw)) FAIL("hmmr_pack_resnet");
    if (upload(host, nb, dev)) return 2;

    if (!(nb = hmmr_pack_temporal_bytes(vars, n_vars, dtype, num_conv_layers))) FAIL("hmmr_pack_temporal_bytes");
    host = malloc(nb); CHECK(hipMalloc(&dev, nb));
    if (hmmr_pack_temporal(vars, n_vars, dtype, num_conv_layers, host, nb, dev, &tw)) FAIL("hmmr_pack_temporal");
    if (upload(host, nb, dev)) return 2;

    if (!(nb = hmmr_pack_ief_bytes(vars, n_vars, dtype, delta_t, 2))) FAIL("hmmr_pack_ief_bytes");
    host = malloc(nb); CHECK(hipMalloc(&dev, nb));
    if (hmmr_pack_ief(vars, n_vars, dtype, delta_t, 2, 3, host, nb, dev, &iw)) FAIL("hmmr_pack_ief");
    if (upload(host, nb, dev)) return 2;

    hmmr_smpl_source_t src;
    const hmmr_var_t *vt = find_var(vars, n_vars, "smpl/v_template"), *sd = find_var(vars, n_vars, "smpl/shapedirs"),
                     *pd = find_var(vars, n_vars, "smpl/posedirs"), *jr = find_var(vars, n_vars, "smpl/J_regressor"),
                     *lw = find_var(vars, n_vars, "smpl/lbs_weights"), *kr = find_var(vars, n_vars, "smpl/kp_regressor"),
                     *pa = find_var(vars, n_vars, "smpl/parents");
    if (!vt || !sd || !pd || !jr || !lw || !kr || !pa || pa->numel != 24) return 1;
    int32_t parents[24];
    for (int i = 0; i < 24; ++i) parents[i] = (int32_t)pa->data[i];
    src.num_verts = (int)(vt->numel / 3); src.num_kps = (int)(kr->numel / (vt->numel / 3));
    src.v_template = vt->data; src.shapedirs = sd->data; src.posedirs = pd->data; src.J_regressor = jr->data;
    src.lbs_weights = lw->data; src.kp_regressor = kr->data; src.parents = parents;
    const int split = dtype != HMMR_F32;          /* an all-fp32 model keeps the blend product on fp32 operands too */
    if (!(nb = hmmr_pack_smpl_bytes(&src, 0, split))) FAIL("hmmr_pack_smpl_bytes");
    host = malloc(nb); CHECK(hipMalloc(&dev, nb));
    if (hmmr_pack_smpl(&src, 0, split, host, nb, dev, &sc)) FAIL("hmmr_pack_smpl");
    if (upload(host, nb, dev)) return 2;

    hmmr_model_t model;
    memset(&model, 0, sizeof(model));
    model.resnet = &rw; model.temporal = &tw; model.ief = &iw; model.smpl = &sc;
    model.sequence_length = T; model.fov = 4 * num_conv_layers + 1;

    /* ---- the record, the frames, the workspace */
    int32_t offsets[HMMR_MAX_REGRESSORS * 7];
    int64_t ld_rec = 0;
    if (hmmr_record_layout(sc.num_kps, sc.num_verts, iw.num_regressors, offsets, &ld_rec)) FAIL("hmmr_record_layout");
    /* the plan refuses bad offsets before anything is read with them; its n_frames sizes the buffers */
    const int max_frames = 1024, max_windows = 128;
    hmmr_tracks_plan_t plan;
    if (hmmr_tracks_plan(track_offsets, n_tracks, model.sequence_length, model.fov, max_frames, max_windows, &plan)) FAIL("hmmr_tracks_plan");
    const int n = plan.n_frames;
    const size_t fbytes = (size_t)n * 224 * 224 * 3 * 4, rbytes = (size_t)n * (size_t)ld_rec * 4;
    float* frames_h = (float*)malloc(fbytes);
    f = fopen(argv[2], "rb");
    if (!f || fread(frames_h, 1, fbytes, f) != fbytes) return 1;
    fclose(f);
    const size_t wsb = hmmr_predict_tracks_workspace_bytes(&model, track_offsets, n_tracks, max_frames, max_windows);
    if (!wsb) FAIL("hmmr_predict_tracks_workspace_bytes");
    float *frames = NULL, *rec = NULL; void* ws = NULL;
    CHECK(hipMalloc((void**)&frames, fbytes ? fbytes : 16)); CHECK(hipMalloc((void**)&rec, rbytes ? rbytes : 16)); CHECK(hipMalloc(&ws, wsb));
    CHECK(hipMemcpy(frames, frames_h, fbytes, hipMemcpyHostToDevice));

    if (hmmr_predict_tracks(&model, frames, track_offsets, n_tracks, rec, ld_rec, offsets, max_frames, max_windows, ws, wsb, NULL))
        FAIL("hmmr_predict_tracks");
    CHECK(hipDeviceSynchronize());
    unsigned flags = 0;
    if (hmmr_run_flags(&flags, 1)) return 1;
    float* rec_h = (float*)malloc(rbytes);
    CHECK(hipMemcpy(rec_h, rec, rbytes, hipMemcpyDeviceToHost));
    f = fopen(argv[5], "wb");
    if (!f || fwrite(rec_h, 1, rbytes, f) != rbytes) return 1;
    fclose(f);
    printf("%d tracks, %d frames, %d windows in %d tail passes, %lld floats per record, workspace %zu bytes, run flags %u\n", n_tracks, n,
           plan.n_windows, plan.tail_passes, (long long)ld_rec, wsb, flags);
    return 0;
}
