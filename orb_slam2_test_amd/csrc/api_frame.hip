// api_frame.hip -- orbg_compute_image_bounds, orbg_set_camera, orbg_batch_keys_un,
// orbg_undistort_*, orbg_rgbd_stereo*, orbg_is_in_frustum*, orbg_distinctive_descriptor*
#include "orbg_ctx.h"
#include "frame_device.h"

#pragma clang fp contract(off)

using namespace orbg;

// ---------------------------------------------------------------------------
// Frame / MapPoint geometry (frame_kernels.hip)
// ---------------------------------------------------------------------------
static bool cam_ok(const orbg_camera *cam)
{
    return cam && std::isfinite(cam->fx) && std::isfinite(cam->fy) && cam->fx != 0.f &&
           cam->fy != 0.f;
}

extern "C" int orbg_compute_image_bounds(const orbg_camera *cam, int w, int h, orbg_bounds *out)
{
    if (!cam || !out) return set_err(ORBG_EINVAL, "NULL argument");
    if (w < 0 || h < 0) return set_err(ORBG_EINVAL, "negative image size");
    if (cam->k1 != 0.0f) {
        if (!cam_ok(cam)) return set_err(ORBG_EINVAL, "fx / fy must be finite and nonzero");
        // the corners (0,0), (cols,0), (0,rows), (cols,rows), Frame.cc:579-600
        float o[8];
        const float in[8] = {0.f, 0.f, (float)w, 0.f, 0.f, (float)h, (float)w, (float)h};
        for (int i = 0; i < 4; i++) orbg::undistort_point(*cam, in[2 * i], in[2 * i + 1], &o[2 * i], &o[2 * i + 1]);
        out->min_x = std::min(o[0], o[4]);
        out->max_x = std::max(o[2], o[6]);
        out->min_y = std::min(o[1], o[3]);
        out->max_y = std::max(o[5], o[7]);
    } else {
        out->min_x = 0.0f;
        out->max_x = (float)w;
        out->min_y = 0.0f;
        out->max_y = (float)h;
    }
    return ORBG_OK;
}

extern "C" int orbg_set_camera(orbg_ctx *c, const orbg_camera *cam)
{
    if (!c) return set_err(ORBG_EINVAL, "NULL context");
    if (cam && cam->k1 != 0.0f && !cam_ok(cam))
        return set_err(ORBG_EINVAL, "fx / fy must be finite and nonzero");
    c->has_cam = cam && cam->k1 != 0.0f;
    if (cam) c->cam = *cam;
    return ORBG_OK;
}

extern "C" int orbg_batch_keys_un(orbg_ctx *c, orbg_keypoint **d_kps_un, int32_t *frame_cap)
{
    if (!c || !d_kps_un) return set_err(ORBG_EINVAL, "NULL argument");
    if (!c->gw || c->last_n <= 0) return set_err(ORBG_EINVAL, "no batch extracted");
    *d_kps_un = c->kps_un_valid ? c->d_kps_un : c->d_kps;
    if (frame_cap) *frame_cap = c->geom.frame_cap;
    return ORBG_OK;
}

extern "C" int orbg_undistort_batch_device(orbg_ctx *c, const orbg_camera *cam,
                                           const orbg_keypoint *d_kps, const int32_t *d_counts,
                                           int frame_cap, int nframes, orbg_keypoint *d_kps_un)
{
    if (!c || !cam) return set_err(ORBG_EINVAL, "NULL argument");
    if (nframes < 0 || frame_cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (nframes == 0 || frame_cap == 0) return ORBG_OK;
    if (!d_kps || !d_counts || !d_kps_un) return set_err(ORBG_EINVAL, "NULL device array");
    if (cam->k1 != 0.0f && !cam_ok(cam)) return set_err(ORBG_EINVAL, "fx / fy must be finite and nonzero");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc = 0;
    PROF_LAUNCH(c, "undistort",
                rc = launch_undistort(st, *cam, d_kps, d_counts, frame_cap, nframes, d_kps_un));
    if (rc) return set_err(ORBG_EIO, "k_undistort launch failed");
    return ORBG_OK;
}

extern "C" int orbg_rgbd_stereo_batch_device(orbg_ctx *c, const void *d_depth, int depth_type,
                                             float factor, int w, int h, size_t pitch,
                                             size_t image_stride, const orbg_keypoint *d_kps,
                                             const orbg_keypoint *d_kps_un,
                                             const int32_t *d_counts, int frame_cap, int nframes,
                                             float mbf, float *d_uright, float *d_depth_out)
{
    if (!c) return set_err(ORBG_EINVAL, "NULL argument");
    if (depth_type != ORBG_DEPTH_F32 && depth_type != ORBG_DEPTH_U16)
        return set_err(ORBG_EINVAL, "depth_type %d", depth_type);
    if (nframes < 0 || frame_cap < 0 || w < 0 || h < 0) return set_err(ORBG_EINVAL, "negative size");
    if (nframes == 0 || frame_cap == 0) return ORBG_OK;
    const size_t px = depth_type == ORBG_DEPTH_U16 ? 2 : 4;
    if (pitch < (size_t)w * px) return set_err(ORBG_EINVAL, "pitch below the row width");
    if (nframes > 1 && image_stride < pitch * (size_t)h)
        return set_err(ORBG_EINVAL, "image_stride below one image");
    if (!d_depth || !d_kps || !d_kps_un || !d_counts || !d_uright || !d_depth_out)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc = 0;
    PROF_LAUNCH(c, "rgbd",
                rc = launch_rgbd(st, d_depth, depth_type == ORBG_DEPTH_U16, factor, w, h, pitch,
                                 image_stride, d_kps, d_kps_un, d_counts, frame_cap, nframes, mbf,
                                 d_uright, d_depth_out));
    if (rc) return set_err(ORBG_EIO, "k_rgbd launch failed");
    return ORBG_OK;
}

extern "C" int orbg_rgbd_stereo(orbg_ctx *c, const void *depth, int depth_type, float factor,
                                int w, int h, size_t pitch, const orbg_keypoint *kps,
                                const orbg_keypoint *kps_un, int n, float mbf, float *uright,
                                float *depth_out)
{
    if (!c) return set_err(ORBG_EINVAL, "NULL argument");
    if (depth_type != ORBG_DEPTH_F32 && depth_type != ORBG_DEPTH_U16)
        return set_err(ORBG_EINVAL, "depth_type %d", depth_type);
    if (n < 0 || w < 0 || h < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!depth || !kps || !kps_un || !uright || !depth_out) return set_err(ORBG_EINVAL, "NULL array");
    const size_t px = depth_type == ORBG_DEPTH_U16 ? 2 : 4;
    if (pitch < (size_t)w * px) return set_err(ORBG_EINVAL, "pitch below the row width");
    HIPCHK(hipSetDevice(c->device));
    // only the keypoints' pixels are read: upload the image rows once (w x h), packed
    Layout L;
    const size_t o_img = L.take((size_t)w * px * h), o_k = L.take((size_t)n * sizeof(orbg_keypoint)),
                 o_ku = L.take((size_t)n * sizeof(orbg_keypoint)), o_cnt = L.take(4),
                 o_ur = L.take((size_t)n * 4), o_d = L.take((size_t)n * 4);
    uint8_t *hs, *db;
    int rc = L.host(c, &hs);
    if (rc) return rc;
    if ((rc = L.device(c, &db))) return rc;
    for (int y = 0; y < h; y++)
        memcpy(hs + o_img + (size_t)y * w * px, (const uint8_t *)depth + (size_t)y * pitch, (size_t)w * px);
    memcpy(hs + o_k, kps, (size_t)n * sizeof(orbg_keypoint));
    memcpy(hs + o_ku, kps_un, (size_t)n * sizeof(orbg_keypoint));
    const int32_t cnt = n;
    memcpy(hs + o_cnt, &cnt, 4);
    HIPCHK(hipMemcpyAsync(db, hs, o_ur, hipMemcpyHostToDevice, c->stream));
    rc = launch_rgbd(c->stream, db + o_img, depth_type == ORBG_DEPTH_U16, factor, w, h,
                     (size_t)w * px, 0, L.at<orbg_keypoint>(db, o_k),
                     L.at<orbg_keypoint>(db, o_ku), L.at<int32_t>(db, o_cnt), n, 1, mbf,
                     L.at<float>(db, o_ur), L.at<float>(db, o_d));
    if (rc) return set_err(ORBG_EIO, "k_rgbd launch failed");
    HIPCHK(hipMemcpyAsync(hs + o_ur, db + o_ur, L.total() - o_ur, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(uright, hs + o_ur, (size_t)n * 4);
    memcpy(depth_out, hs + o_d, (size_t)n * 4);
    return ORBG_OK;
}

extern "C" int orbg_undistort_keypoints(orbg_ctx *c, const orbg_camera *cam,
                                        const orbg_keypoint *kps, int n, orbg_keypoint *kps_un)
{
    if (!c || !cam) return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    if (n == 0) return ORBG_OK;
    if (!kps || !kps_un) return set_err(ORBG_EINVAL, "NULL array");
    if (cam->k1 != 0.0f && !cam_ok(cam)) return set_err(ORBG_EINVAL, "fx / fy must be finite and nonzero");
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_k = L.take((size_t)n * sizeof(orbg_keypoint)), o_cnt = L.take(4),
                 o_un = L.take((size_t)n * sizeof(orbg_keypoint));
    uint8_t *hs, *db;
    int rc = L.host(c, &hs);
    if (rc) return rc;
    if ((rc = L.device(c, &db))) return rc;
    memcpy(hs + o_k, kps, (size_t)n * sizeof(orbg_keypoint));
    const int32_t cnt = n;
    memcpy(hs + o_cnt, &cnt, 4);
    HIPCHK(hipMemcpyAsync(db, hs, o_cnt + 4, hipMemcpyHostToDevice, c->stream));
    rc = launch_undistort(c->stream, *cam, L.at<orbg_keypoint>(db, o_k), L.at<int32_t>(db, o_cnt),
                          n, 1, L.at<orbg_keypoint>(db, o_un));
    if (rc) return set_err(ORBG_EIO, "k_undistort launch failed");
    HIPCHK(hipMemcpyAsync(hs + o_un, db + o_un, (size_t)n * sizeof(orbg_keypoint),
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(kps_un, hs + o_un, (size_t)n * sizeof(orbg_keypoint));
    return ORBG_OK;
}

extern "C" int orbg_is_in_frustum_batch_device(orbg_ctx *c, const orbg_frustum_camera *d_cams,
                                               const orbg_map_point *d_mps,
                                               const int32_t *d_counts, int cap, int nframes,
                                               float viewing_cos_limit,
                                               orbg_map_projection *d_proj, int32_t *d_nvisible)
{
    if (!c) return set_err(ORBG_EINVAL, "NULL context");
    if (nframes < 0 || cap < 0) return set_err(ORBG_EINVAL, "negative size");
    if (nframes == 0 || cap == 0) return ORBG_OK;
    if (!d_cams || !d_mps || !d_counts || !d_proj || !d_nvisible)
        return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc = 0;
    PROF_LAUNCH(c, "frustum",
                rc = launch_frustum(st, d_cams, d_mps, d_counts, cap, nframes, viewing_cos_limit,
                                    d_proj, d_nvisible));
    if (rc) return set_err(ORBG_EIO, "k_frustum launch failed");
    return ORBG_OK;
}

extern "C" int orbg_is_in_frustum(orbg_ctx *c, const orbg_frustum_camera *cam,
                                  const orbg_map_point *mps, int n, float viewing_cos_limit,
                                  orbg_map_projection *proj, int *nvisible)
{
    if (!c || !cam || !nvisible) return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    *nvisible = 0;
    if (n == 0) return ORBG_OK;
    if (!mps || !proj) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_cam = L.take(sizeof(orbg_frustum_camera)), o_cnt = L.take(4),
                 o_mp = L.take((size_t)n * sizeof(orbg_map_point)),
                 o_pr = L.take((size_t)n * sizeof(orbg_map_projection)), o_nv = L.take(4);
    uint8_t *hs, *db;
    int rc = L.host(c, &hs);
    if (rc) return rc;
    if ((rc = L.device(c, &db))) return rc;
    memcpy(hs + o_cam, cam, sizeof(orbg_frustum_camera));
    const int32_t cnt = n;
    memcpy(hs + o_cnt, &cnt, 4);
    memcpy(hs + o_mp, mps, (size_t)n * sizeof(orbg_map_point));
    // the projections a point not in view keeps (only its flags are written)
    memcpy(hs + o_pr, proj, (size_t)n * sizeof(orbg_map_projection));
    HIPCHK(hipMemcpyAsync(db, hs, o_nv, hipMemcpyHostToDevice, c->stream));
    rc = launch_frustum(c->stream, L.at<orbg_frustum_camera>(db, o_cam),
                        L.at<orbg_map_point>(db, o_mp), L.at<int32_t>(db, o_cnt), n, 1,
                        viewing_cos_limit, L.at<orbg_map_projection>(db, o_pr),
                        L.at<int32_t>(db, o_nv));
    if (rc) return set_err(ORBG_EIO, "k_frustum launch failed");
    HIPCHK(hipMemcpyAsync(hs + o_pr, db + o_pr, L.total() - o_pr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(proj, hs + o_pr, (size_t)n * sizeof(orbg_map_projection));
    memcpy(nvisible, hs + o_nv, 4);
    return ORBG_OK;
}

extern "C" int orbg_distinctive_descriptors_batch_device(orbg_ctx *c, const uint8_t *d_pool,
                                                         const int32_t *d_rows,
                                                         const int32_t *d_off, int npoints,
                                                         int32_t *d_best, uint8_t *d_desc)
{
    if (!c) return set_err(ORBG_EINVAL, "NULL context");
    if (npoints < 0) return set_err(ORBG_EINVAL, "negative size");
    if (npoints == 0) return ORBG_OK;
    if (!d_pool || !d_rows || !d_off || !d_best) return set_err(ORBG_EINVAL, "NULL device array");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int rc = 0;
    PROF_LAUNCH(c, "distinctive",
                rc = launch_distinctive(st, d_pool, d_rows, d_off, npoints, d_best, d_desc));
    if (rc) return set_err(ORBG_EIO, "k_distinctive launch failed");
    return ORBG_OK;
}

extern "C" int orbg_distinctive_descriptor(orbg_ctx *c, const uint8_t *desc, int n, int32_t *best)
{
    if (!c || !best) return set_err(ORBG_EINVAL, "NULL argument");
    if (n < 0) return set_err(ORBG_EINVAL, "negative size");
    *best = -1;
    if (n == 0) return ORBG_OK;  // observations empty: the reference returns (MapPoint.cc:356)
    if (!desc) return set_err(ORBG_EINVAL, "NULL array");
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const size_t o_d = L.take((size_t)n * 32), o_r = L.take((size_t)n * 4), o_off = L.take(8),
                 o_b = L.take(4);
    uint8_t *hs, *db;
    int rc = L.host(c, &hs);
    if (rc) return rc;
    if ((rc = L.device(c, &db))) return rc;
    memcpy(hs + o_d, desc, (size_t)n * 32);
    int32_t *hr = L.at<int32_t>(hs, o_r);
    for (int i = 0; i < n; i++) hr[i] = i;
    int32_t *ho = L.at<int32_t>(hs, o_off);
    ho[0] = 0;
    ho[1] = n;
    HIPCHK(hipMemcpyAsync(db, hs, o_b, hipMemcpyHostToDevice, c->stream));
    rc = launch_distinctive(c->stream, db + o_d, L.at<int32_t>(db, o_r),
                            L.at<int32_t>(db, o_off), 1, L.at<int32_t>(db, o_b), nullptr);
    if (rc) return set_err(ORBG_EIO, "k_distinctive launch failed");
    HIPCHK(hipMemcpyAsync(hs + o_b, db + o_b, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(best, hs + o_b, 4);
    return ORBG_OK;
}
