// api_track.hip -- orbg_search_by_projection_*, orbg_pose_optimization*
#include "orbg_ctx.h"
#include "track_args.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// tracking matchers (ORBmatcher::SearchByProjection x 2)
// ---------------------------------------------------------------------------
static int track_run(orbg_ctx *c, int mode, const orbg_track_batch *tb, int nframes)
{
    if (tb->frame_cap <= 0 || tb->query_cap <= 0 || tb->frame_cap > (1 << 20))
        return set_err(ORBG_EINVAL, "frame_cap / query_cap out of range");
    if (!tb->kps || !tb->desc || !tb->counts || !tb->bounds || !tb->queries || !tb->qdesc ||
        !tb->qcounts || !tb->match || !tb->nmatches)
        return set_err(ORBG_EINVAL, "NULL device array");
    if (mode == ORBG_TRACK_LASTFRAME && !tb->cams) return set_err(ORBG_EINVAL, "cams is NULL");
    if ((mode == ORBG_TRACK_RELOC || mode == ORBG_TRACK_LOOP) && !tb->fcams)
        return set_err(ORBG_EINVAL, "fcams is NULL");
    const size_t tk = al256((size_t)nframes * tb->query_cap * ORBG_MATCH_TOPK * 8);
    const size_t need = tk + al256((size_t)nframes * tb->query_cap * 4);
    if (c->trk_bytes < need) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->d_trk) hipFree(c->d_trk);
        c->d_trk = nullptr;
        c->trk_bytes = 0;
        if (hipMalloc(&c->d_trk, need) != hipSuccess)
            return set_err(ORBG_ENOMEM, "track scratch %zu bytes", need);
        c->trk_bytes = need;
    }
    TrackArgs A{};
    A.kps = tb->kps;
    A.desc = tb->desc;
    A.uright = tb->uright;
    A.taken0 = tb->taken0;
    A.counts = tb->counts;
    A.bounds = tb->bounds;
    A.fc = tb->frame_cap;
    A.q = tb->queries;
    A.qdesc = tb->qdesc;
    A.qcounts = tb->qcounts;
    A.qc = tb->query_cap;
    A.cams = tb->cams;
    for (int l = 0; l < ORBG_MAX_LEVELS; l++)
        A.scale[l] = l < c->p.nlevels ? c->scale[l] : 1.f;
    A.th = tb->th;
    A.nnratio = tb->nnratio;
    A.check_ori = tb->check_ori;
    A.topk = (unsigned long long *)c->d_trk;
    A.topn = (int32_t *)((uint8_t *)c->d_trk + tk);
    A.match = tb->match;
    A.nmatches = tb->nmatches;
    // fcams / orb_dist were appended to orbg_track_batch in round 4: a caller built against
    // the older header passes the shorter struct, so they are read only in the modes that
    // define them (ABI notes)
    if (mode == ORBG_TRACK_RELOC || mode == ORBG_TRACK_LOOP) {
        A.fcams = tb->fcams;
        A.orb_dist = tb->orb_dist;
    }
    if (mode == ORBG_TRACK_LOOP) A.check_ori = 0;
    const int rc = launch_track(c->stream, mode, A, nframes, &c->prof);
    if (rc == ORBG_ENOTSUP)
        return set_err(rc, "frame_cap %d / query_cap %d exceed the LDS budget", tb->frame_cap,
                       tb->query_cap);
    if (rc) return set_err(rc, "track launch failed");
    return ORBG_OK;
}

extern "C" int orbg_search_by_projection_batch_device(orbg_ctx *c, int mode,
                                                      const orbg_track_batch *tb, int nframes)
{
    if (!c || !tb) return set_err(ORBG_EINVAL, "NULL argument");
    if (mode < ORBG_TRACK_LASTFRAME || mode > ORBG_TRACK_LOOP)
        return set_err(ORBG_EINVAL, "mode %d", mode);
    if (nframes <= 0) return ORBG_OK;
    HIPCHK(hipSetDevice(c->device));
    return track_run(c, mode, tb, nframes);
}

// one frame from host arrays: upload, run, download
static int track_host(orbg_ctx *c, int mode, const orbg_keypoint *kps, const uint8_t *desc,
                      const float *uright, int n, const uint8_t *taken0, const orbg_bounds *bounds,
                      const void *q, size_t qrec, const uint8_t *qdesc, int nq,
                      const orbg_track_camera *cam, float th, float nnratio, int check_ori,
                      int32_t *match, int *nmatches, const orbg_frustum_camera *fcam = nullptr,
                      int orb_dist = 0)
{
    if (!c || !bounds || !match || (n > 0 && (!kps || !desc)) || (nq > 0 && (!q || !qdesc)))
        return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0 || nq < 0) return set_err(ORBG_EINVAL, "negative size");
    if (mode == ORBG_TRACK_LASTFRAME && !cam) return set_err(ORBG_EINVAL, "cam is NULL");
    if ((mode == ORBG_TRACK_RELOC || mode == ORBG_TRACK_LOOP) && !fcam)
        return set_err(ORBG_EINVAL, "cam is NULL");
    for (int i = 0; i < n; i++) match[i] = -1;
    if (nmatches) *nmatches = 0;
    if (n == 0 || nq == 0) return ORBG_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t fc = (size_t)n, qc = (size_t)nq;
    Layout L;
    const size_t o_kps = L.take(fc * sizeof(orbg_keypoint)), o_desc = L.take(fc * 32);
    const size_t o_ur = uright ? L.take(fc * 4) : 0, o_tk = taken0 ? L.take(fc) : 0;
    const size_t o_cnt = L.take(8), o_b = L.take(sizeof(orbg_bounds)), o_q = L.take(qc * qrec);
    const size_t o_qd = L.take(qc * 32), o_cam = L.take(sizeof(orbg_track_camera));
    const size_t o_fcam = L.take(sizeof(orbg_frustum_camera));
    const size_t o_match = L.take(fc * 4), o_nm = L.take(4);
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    const int32_t cnts[2] = {n, nq};
    HIPCHK(hipMemcpyAsync(b + o_kps, kps, fc * sizeof(orbg_keypoint), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_desc, desc, fc * 32, hipMemcpyHostToDevice, c->stream));
    if (uright) HIPCHK(hipMemcpyAsync(b + o_ur, uright, fc * 4, hipMemcpyHostToDevice, c->stream));
    if (taken0) HIPCHK(hipMemcpyAsync(b + o_tk, taken0, fc, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_cnt, cnts, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_b, bounds, sizeof(orbg_bounds), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_q, q, qc * qrec, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_qd, qdesc, qc * 32, hipMemcpyHostToDevice, c->stream));
    if (cam)
        HIPCHK(hipMemcpyAsync(b + o_cam, cam, sizeof(*cam), hipMemcpyHostToDevice, c->stream));
    if (fcam)
        HIPCHK(hipMemcpyAsync(b + o_fcam, fcam, sizeof(*fcam), hipMemcpyHostToDevice, c->stream));
    orbg_track_batch tb{};
    tb.kps = L.at<orbg_keypoint>(b, o_kps);
    tb.desc = b + o_desc;
    tb.uright = uright ? L.at<float>(b, o_ur) : nullptr;
    tb.taken0 = taken0 ? b + o_tk : nullptr;
    tb.counts = L.at<int32_t>(b, o_cnt);
    tb.bounds = L.at<orbg_bounds>(b, o_b);
    tb.frame_cap = n;
    tb.queries = b + o_q;
    tb.qdesc = b + o_qd;
    tb.qcounts = L.at<int32_t>(b, o_cnt) + 1;
    tb.query_cap = nq;
    tb.cams = cam ? L.at<orbg_track_camera>(b, o_cam) : nullptr;
    tb.th = th;
    tb.nnratio = nnratio;
    tb.check_ori = check_ori;
    tb.match = L.at<int32_t>(b, o_match);
    tb.nmatches = L.at<int32_t>(b, o_nm);
    tb.fcams = fcam ? L.at<orbg_frustum_camera>(b, o_fcam) : nullptr;
    tb.orb_dist = orb_dist;
    if ((rc = track_run(c, mode, &tb, 1))) return rc;
    int32_t nm = 0;
    HIPCHK(hipMemcpyAsync(match, b + o_match, fc * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&nm, b + o_nm, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    if (nmatches) *nmatches = nm;
    return ORBG_OK;
}

extern "C" int orbg_search_by_projection_lastframe(orbg_ctx *c, const orbg_keypoint *kps,
                                                   const uint8_t *desc, const float *uright,
                                                   int n, const uint8_t *taken0,
                                                   const orbg_bounds *bounds,
                                                   const orbg_lastframe_point *pts,
                                                   const uint8_t *pdesc, int np,
                                                   const orbg_track_camera *cam, float th,
                                                   int check_ori, int32_t *match, int *nmatches)
{
    return track_host(c, ORBG_TRACK_LASTFRAME, kps, desc, uright, n, taken0, bounds, pts,
                      sizeof(orbg_lastframe_point), pdesc, np, cam, th, 0.f, check_ori, match,
                      nmatches);
}

extern "C" int orbg_search_by_projection_local(orbg_ctx *c, const orbg_keypoint *kps,
                                               const uint8_t *desc, const float *uright, int n,
                                               const uint8_t *taken0, const orbg_bounds *bounds,
                                               const orbg_map_projection *mps,
                                               const uint8_t *mdesc, int nm, float th,
                                               float nnratio, int32_t *match, int *nmatches)
{
    return track_host(c, ORBG_TRACK_LOCAL, kps, desc, uright, n, taken0, bounds, mps,
                      sizeof(orbg_map_projection), mdesc, nm, nullptr, th, nnratio, 0, match,
                      nmatches);
}

extern "C" int orbg_search_by_projection_reloc(orbg_ctx *c, const orbg_keypoint *kps,
                                               const uint8_t *desc, int n, const uint8_t *taken0,
                                               const orbg_frustum_camera *cam,
                                               const orbg_reloc_point *pts, const uint8_t *pdesc,
                                               int np, float th, int orb_dist, int check_ori,
                                               int32_t *match, int *nmatches)
{
    if (!cam) return set_err(ORBG_EINVAL, "NULL argument");
    return track_host(c, ORBG_TRACK_RELOC, kps, desc, nullptr, n, taken0, &cam->bounds, pts,
                      sizeof(orbg_reloc_point), pdesc, np, nullptr, th, 0.f, check_ori, match,
                      nmatches, cam, orb_dist);
}

extern "C" int orbg_search_by_projection_sim3(orbg_ctx *c, const orbg_keypoint *kps,
                                              const uint8_t *desc, int n, const uint8_t *taken0,
                                              const orbg_frustum_camera *cam,
                                              const orbg_map_point *mps, const uint8_t *mdesc,
                                              int nm, int th, int32_t *match, int *nmatches)
{
    if (!cam) return set_err(ORBG_EINVAL, "NULL argument");
    return track_host(c, ORBG_TRACK_LOOP, kps, desc, nullptr, n, taken0, &cam->bounds, mps,
                      sizeof(orbg_map_point), mdesc, nm, nullptr, (float)th, 0.f, 0, match,
                      nmatches, cam, 0);
}

// ---------------------------------------------------------------------------
// Optimizer::PoseOptimization
// ---------------------------------------------------------------------------
extern "C" int orbg_pose_optimization_batch_device(orbg_ctx *c, const orbg_pose_edge *edges,
                                                   const int32_t *counts, int edge_cap,
                                                   const orbg_pose_camera *cams,
                                                   const float *tcw_in, double *q_out,
                                                   double *t_out, float *tcw_out,
                                                   uint8_t *outlier, int32_t *ninliers,
                                                   int nframes)
{
    if (!c) return set_err(ORBG_EINVAL, "ctx is NULL");
    if (nframes <= 0) return ORBG_OK;
    if (edge_cap < 0 || !edges || !counts || !cams || !tcw_in || !q_out || !t_out || !tcw_out ||
        !outlier || !ninliers)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    const int rc = launch_pose_opt(c->stream, edges, counts, edge_cap, cams, tcw_in, q_out,
                                   t_out, tcw_out, outlier, ninliers, nframes, &c->prof);
    return rc ? set_err(rc, "pose optimisation launch failed") : ORBG_OK;
}

extern "C" int orbg_pose_optimization(orbg_ctx *c, const orbg_pose_edge *edges, int n,
                                      const orbg_pose_camera *cam, const float tcw_in[12],
                                      double q_out[4], double t_out[3], float tcw_out[12],
                                      uint8_t *outlier, int *ninliers)
{
    if (!c || !cam || !tcw_in || !q_out || !t_out || !tcw_out || (n > 0 && (!edges || !outlier)))
        return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_e = L.take((size_t)std::max(n, 1) * sizeof(orbg_pose_edge)), o_n = L.take(4);
    const size_t o_cam = L.take(sizeof(orbg_pose_camera)), o_tin = L.take(48), o_q = L.take(32);
    const size_t o_t = L.take(24), o_tout = L.take(48), o_out = L.take((size_t)std::max(n, 1));
    const size_t o_ni = L.take(4);
    uint8_t *b;
    int rc = L.device(c, &b);
    if (rc) return rc;
    const int32_t cnt = n;
    if (n) HIPCHK(hipMemcpyAsync(b + o_e, edges, (size_t)n * sizeof(orbg_pose_edge), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_n, &cnt, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_cam, cam, sizeof(*cam), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + o_tin, tcw_in, 48, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_pose_opt(c->stream, L.at<orbg_pose_edge>(b, o_e), L.at<int32_t>(b, o_n),
                              std::max(n, 1), L.at<orbg_pose_camera>(b, o_cam),
                              L.at<float>(b, o_tin), L.at<double>(b, o_q), L.at<double>(b, o_t),
                              L.at<float>(b, o_tout), b + o_out, L.at<int32_t>(b, o_ni), 1,
                              &c->prof)))
        return set_err(rc, "pose optimisation launch failed");
    int32_t ni = 0;
    HIPCHK(hipMemcpyAsync(q_out, b + o_q, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(t_out, b + o_t, 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(tcw_out, b + o_tout, 48, hipMemcpyDeviceToHost, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(outlier, b + o_out, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&ni, b + o_ni, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.collect();
    if (ninliers) *ninliers = ni;
    return ORBG_OK;
}
