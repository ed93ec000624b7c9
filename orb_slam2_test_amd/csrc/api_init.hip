// api_init.hip -- Initializer
#include "orbg_ctx.h"
#include "init_args.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// Initializer: batched H/F RANSAC and two-view reconstruction of
// Tracking::MonocularInitialization (init_kernels.hip)
// ---------------------------------------------------------------------------
namespace {

// The per-iteration outputs a caller may leave out: they are the kernels' working arrays, so
// the ones not given live in the context scratch behind `L`.
struct InitOptional {
    size_t o_sh, o_sf, o_h, o_f, o_mh, o_mf;
    void plan(Layout &L, const InitArgs &A)
    {
        const size_t rows = (size_t)A.npairs * A.max_its, words = (size_t)(A.cap >> 6);
        o_sh = A.scores_h ? 0 : L.take(rows * 4);
        o_sf = A.scores_f ? 0 : L.take(rows * 4);
        o_h = A.H21 ? 0 : L.take(rows * 36);
        o_f = A.F21 ? 0 : L.take(rows * 36);
        o_mh = A.masks_h ? 0 : L.take(rows * words * 8);
        o_mf = A.masks_f ? 0 : L.take(rows * words * 8);
    }
    void place(uint8_t *b, InitArgs *A) const
    {
        if (!A->scores_h) A->scores_h = Layout::at<float>(b, o_sh);
        if (!A->scores_f) A->scores_f = Layout::at<float>(b, o_sf);
        if (!A->H21) A->H21 = Layout::at<float>(b, o_h);
        if (!A->F21) A->F21 = Layout::at<float>(b, o_f);
        if (!A->masks_h) A->masks_h = Layout::at<unsigned long long>(b, o_mh);
        if (!A->masks_f) A->masks_f = Layout::at<unsigned long long>(b, o_mf);
    }
};

}  // namespace

extern "C" int orbg_initialize_batch_device(orbg_ctx *c, const orbg_init_problem *d_problems,
                                            const orbg_keypoint *d_kps, int frame_stride,
                                            const int32_t *d_counts, int nframes,
                                            const int32_t *d_f1, const int32_t *d_f2,
                                            const int32_t *d_matches12, int match_stride,
                                            const int32_t *d_sets, int npairs, int cap, int max_its,
                                            orbg_init_result *d_results, float *d_p3d,
                                            uint8_t *d_triangulated, float *d_scores_h,
                                            float *d_scores_f, float *d_H21, float *d_F21,
                                            uint64_t *d_masks_h, uint64_t *d_masks_f)
{
    if (!c) return set_err(ORBG_EINVAL, "context is NULL");
    if (npairs < 0 || cap < 64 || (cap & 63) || max_its < 1 || frame_stride < 1 || nframes < 1 ||
        match_stride < 1)
        return set_err(ORBG_EINVAL, "bad npairs / cap (a multiple of 64) / max_its / frame_stride / nframes / match_stride");
    if (cap > ORBG_INIT_MAX_N)
        return set_err(ORBG_ENOTSUP, "cap %d (> %d keypoints per frame)", cap, ORBG_INIT_MAX_N);
    if (npairs == 0) return ORBG_OK;
    if ((int64_t)npairs * max_its > INT32_MAX)
        return set_err(ORBG_ENOTSUP, "npairs * max_its too large for one launch");
    if (!d_problems || !d_kps || !d_counts || !d_f1 || !d_f2 || !d_matches12 || !d_sets ||
        !d_results || !d_p3d || !d_triangulated)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    InitArgs A{};
    A.problems = d_problems;
    A.kps = d_kps;
    A.counts = d_counts;
    A.f1 = d_f1;
    A.f2 = d_f2;
    A.matches12 = d_matches12;
    A.sets = d_sets;
    A.frame_stride = frame_stride;
    A.nframes = nframes;
    A.npairs = npairs;
    A.cap = cap;
    A.max_its = max_its;
    A.match_stride = match_stride;
    A.results = d_results;
    A.p3d = d_p3d;
    A.triangulated = d_triangulated;
    A.scores_h = d_scores_h;
    A.scores_f = d_scores_f;
    A.H21 = d_H21;
    A.F21 = d_F21;
    A.masks_h = (unsigned long long *)d_masks_h;
    A.masks_f = (unsigned long long *)d_masks_f;
    Layout L;
    const size_t o_x = L.take(init_scratch_bytes(npairs, cap, max_its));
    InitOptional opt;
    opt.plan(L, A);
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    init_scratch_at(b + o_x, npairs, cap, max_its, &A);
    opt.place(b, &A);
    if ((rc = launch_init(c->stream, A, &c->prof))) return set_err(rc, "Initializer launch failed");
    return ORBG_OK;
}

extern "C" int orbg_initialize(orbg_ctx *c, const orbg_init_problem *problem, const orbg_keypoint *kps1,
                               int n1, const orbg_keypoint *kps2, int n2, const int32_t *matches12,
                               const int32_t *sets, orbg_init_result *result, float *p3d,
                               uint8_t *triangulated, float *scores_h, float *scores_f, float *H21,
                               float *F21, uint64_t *masks_h, uint64_t *masks_f)
{
    if (!c || !problem || !result) return set_err(ORBG_EINVAL, "NULL argument");
    const orbg_init_problem P = *problem;
    if (n1 < 0 || n2 < 0 || P.iterations < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n1 > ORBG_INIT_MAX_N || n2 > ORBG_INIT_MAX_N)
        return set_err(ORBG_ENOTSUP, "%d / %d keypoints (> %d)", n1, n2, ORBG_INIT_MAX_N);
    if (P.iterations > (1 << 20)) return set_err(ORBG_ENOTSUP, "%d iterations", P.iterations);
    if ((n1 && (!kps1 || !matches12 || !p3d || !triangulated)) || (n2 && !kps2))
        return set_err(ORBG_EINVAL, "NULL array");
    int N = 0;
    for (int i = 0; i < n1; i++) N += matches12[i] >= 0 && matches12[i] < n2;
    const int cap = std::max(64, (n1 + 63) & ~63), its = std::max(P.iterations, 1);
    const int run = init_iterations(P, N, its), words = cap / 64, stride = std::max(cap, n2);
    if (run && !sets) return set_err(ORBG_EINVAL, "sets is NULL");
    HIPCHK(hipSetDevice(c->device));
    const int32_t frames[4] = {n1, n2, 0, 1};
    Layout L;
    const size_t o_p = L.take(sizeof(P)), o_k = L.take((size_t)2 * stride * sizeof(orbg_keypoint));
    const size_t o_c = L.take(sizeof(frames)), o_m = L.take((size_t)cap * 4);
    const size_t o_s = L.take((size_t)its * 32), o_r = L.take(sizeof(orbg_init_result));
    const size_t o_3 = L.take((size_t)cap * 12), o_t = L.take((size_t)cap);
    const size_t o_sh = L.take((size_t)its * 4), o_sf = L.take((size_t)its * 4);
    const size_t o_h = L.take((size_t)its * 36), o_f = L.take((size_t)its * 36);
    const size_t o_mh = L.take((size_t)its * words * 8), o_mf = L.take((size_t)its * words * 8);
    const size_t o_x = L.take(init_scratch_bytes(1, cap, its));
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b + o_p, &P, sizeof(P), hipMemcpyHostToDevice, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(b + o_k, kps1, (size_t)n1 * sizeof(orbg_keypoint), hipMemcpyHostToDevice, c->stream));
    if (n2) HIPCHK(hipMemcpyAsync(b + o_k + (size_t)stride * sizeof(orbg_keypoint), kps2, (size_t)n2 * sizeof(orbg_keypoint), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_c, frames, sizeof(frames), hipMemcpyHostToDevice, c->stream));
    if (n1) HIPCHK(hipMemcpyAsync(b + o_m, matches12, (size_t)n1 * 4, hipMemcpyHostToDevice, c->stream));
    if (run) HIPCHK(hipMemcpyAsync(b + o_s, sets, (size_t)run * 32, hipMemcpyHostToDevice, c->stream));
    InitArgs A{};
    A.problems = L.at<orbg_init_problem>(b, o_p);
    A.kps = L.at<orbg_keypoint>(b, o_k);
    A.counts = L.at<int32_t>(b, o_c);
    A.f1 = A.counts + 2;
    A.f2 = A.counts + 3;
    A.matches12 = L.at<int32_t>(b, o_m);
    A.sets = L.at<int32_t>(b, o_s);
    A.frame_stride = stride;
    A.nframes = 2;
    A.npairs = 1;
    A.cap = cap;
    A.max_its = its;
    A.match_stride = cap;
    A.results = L.at<orbg_init_result>(b, o_r);
    A.p3d = L.at<float>(b, o_3);
    A.triangulated = b + o_t;
    A.scores_h = L.at<float>(b, o_sh);
    A.scores_f = L.at<float>(b, o_sf);
    A.H21 = L.at<float>(b, o_h);
    A.F21 = L.at<float>(b, o_f);
    A.masks_h = L.at<unsigned long long>(b, o_mh);
    A.masks_f = L.at<unsigned long long>(b, o_mf);
    init_scratch_at(b + o_x, 1, cap, its, &A);
    if ((rc = launch_init(c->stream, A, &c->prof))) return set_err(rc, "Initializer launch failed");
    const int nout = P.iterations, nw = (N + 63) / 64;
    if (scores_h && nout) HIPCHK(hipMemcpyAsync(scores_h, b + o_sh, (size_t)nout * 4, hipMemcpyDeviceToHost, c->stream));
    if (scores_f && nout) HIPCHK(hipMemcpyAsync(scores_f, b + o_sf, (size_t)nout * 4, hipMemcpyDeviceToHost, c->stream));
    if (H21 && nout) HIPCHK(hipMemcpyAsync(H21, b + o_h, (size_t)nout * 36, hipMemcpyDeviceToHost, c->stream));
    if (F21 && nout) HIPCHK(hipMemcpyAsync(F21, b + o_f, (size_t)nout * 36, hipMemcpyDeviceToHost, c->stream));
    if (masks_h && nout && nw)
        HIPCHK(hipMemcpy2DAsync(masks_h, (size_t)nw * 8, b + o_mh, (size_t)words * 8, (size_t)nw * 8, nout,
                                hipMemcpyDeviceToHost, c->stream));
    if (masks_f && nout && nw)
        HIPCHK(hipMemcpy2DAsync(masks_f, (size_t)nw * 8, b + o_mf, (size_t)words * 8, (size_t)nw * 8, nout,
                                hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(result, b + o_r, sizeof(orbg_init_result), hipMemcpyDeviceToHost, c->stream));
    if (n1) {
        HIPCHK(hipMemcpyAsync(p3d, b + o_3, (size_t)n1 * 12, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(triangulated, b + o_t, (size_t)n1, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    return ORBG_OK;
}
