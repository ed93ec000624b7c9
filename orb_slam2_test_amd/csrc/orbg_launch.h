// orbg_launch.h -- the boundary between the kernel files and the host code: every launcher,
// helper and __global__ that is defined in one .hip and used from another, declared once.
// Included by the defining file and by every caller; default arguments appear only here.
// (The launchers that take a *_args.h struct are declared in that header.)
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/orbg.h"
#include "orbg_internal.h"
#include "octree_args.h"
#include "pyramid_args.h"

namespace orbg {
// orbg_api.hip: the launchers' profiling hooks (Prof: orbg_ctx.h, the context's) and the
// developer builds' ORBG_SKIP test
struct Prof;
void prof_begin(Prof *prof, hipStream_t s, const char *n, hipEvent_t *a);
void prof_end(Prof *prof, hipStream_t s, const char *n, hipEvent_t a);
bool prof_skip_name(const char *n);

// extract_kernels.hip
__global__ void k_resize(const uint8_t *, int64_t, int, int, uint8_t *, int64_t, int, int, int,
                         const int2 *, const int2 *, int, int);
// pyramid_kernels.hip
__global__ void k_pyramid(PyrArgs, const OrbgGeom *, const uint4 *, const int4 *, const int4 *,
                          const uint8_t *, int64_t, int, const uint8_t *, uint8_t *, uint8_t *,
                          int);
// octree_kernels.hip
__global__ void k_octree(const OrbgGeom *, const int32_t *, const uint2 *, uint32_t *,
                         uint32_t *, uint32_t *, uint8_t *, int4 *, uint32_t *, uint16_t *,
                         int32_t *, int32_t *, int);
hipError_t launch_octree_lds(bool small, dim3 grid, size_t lds, hipStream_t st, const OrbgGeom *g,
                             const int32_t *cell_cnt, const uint2 *cell_kp, uint32_t *lvl_kp,
                             uint16_t *lvl_idx, int32_t *lvl_cnt, int32_t *err_flag, OctLdsDims D);
hipError_t octree_lds_attr(int bytes);
// blur_kernels.hip
int blur2_seg();
int blur2_tw(bool tiled);
hipError_t launch_blur2(hipStream_t st, const OrbgGeom *g, const int32_t *task_base,
                        const uint8_t *img0, int64_t img_fs, int img_pitch, const uint8_t *pyr,
                        uint8_t *blur, int t_begin, int t_count, int nframes);
hipError_t launch_blur_border(hipStream_t st, const OrbgGeom *g, int tasks_per_frame,
                              const uint8_t *img0, int64_t img_fs, int img_pitch,
                              const uint8_t *pyr, uint8_t *blur, int l0, int l1, int nframes);
// fast_rows_kernels.hip
int fast_rows_wave_bytes();
hipError_t launch_fast_rows(hipStream_t st, const OrbgGeom *g, const OrbgFastTile *tiles,
                            const uint8_t *img0, int64_t img_fs, int img_pitch,
                            const uint8_t *pyr, const uint32_t *ctab, int32_t *cell_cnt,
                            uint2 *cell_kp, int nframes, int t_begin, int t_count);
// fast_kernels.hip
bool fast2_pitch_ok(int p4);
hipError_t launch_fast2(int p4, size_t lds, hipStream_t st, const OrbgGeom *g,
                        const OrbgCell *cells, const uint8_t *img0, int64_t img_fs,
                        int img_pitch, const uint8_t *pyr, const uint32_t *ctab,
                        int32_t *cell_cnt, uint2 *cell_kp, uint8_t *blur, int nframes,
                        int c_begin, int c_count);
// orient_kernels.hip
struct OrbgKeypointDev;
hipError_t launch_orient_desc(bool bfma, bool tiled, dim3 grid, hipStream_t st, const OrbgGeom *g,
                              const uint8_t *img0, int64_t img_fs, int img_pitch,
                              const uint8_t *pyr, const uint8_t *blur, const uint4 *odtab,
                              const uint32_t *lvl_kp, const uint16_t *lvl_idx,
                              const int32_t *lvl_cnt, OrbgKeypointDev *kps, uint8_t *desc,
                              int32_t *counts, uint8_t *hc_base = nullptr,
                              const int32_t *hc_err = nullptr, size_t hc_okp = 0,
                              size_t hc_ods = 0, int32_t hc_tag = 0);
// match_kernels.hip
int launch_match_pairs(hipStream_t st, hipStream_t aux, hipEvent_t evf, hipEvent_t evj,
                       const uint8_t *desc, const orbg_keypoint *kps,
                       const int32_t *counts, int frame_cap, const int32_t *d_f1,
                       const int32_t *d_f2, int npairs, orbg_bounds b, int window, float nnratio,
                       int check_ori, int32_t *knn, int32_t *m12, int32_t *nm, uint32_t *topk,
                       int32_t *topk_n, Prof *prof, int serial, int cap0);
int launch_match_export(hipStream_t st, const int32_t *m12, const int32_t *f1,
                        const int32_t *counts, int frame_cap, int npairs, int32_t *out);
int launch_knn2(hipStream_t st, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *out,
                Prof *prof);
int launch_init_match_single(hipStream_t st, const orbg_keypoint *k1, const uint8_t *d1, int n1,
                             const orbg_keypoint *k2, const uint8_t *d2, int n2,
                             orbg_bounds b, const float *prev, float *prev_out, int32_t *m12,
                             int32_t *nm, int window, float nnratio, int check_ori, uint32_t *topk,
                             int32_t *topk_n, Prof *prof, int cap);
// stereo_kernels.hip
size_t stereo_scratch_bytes(int npairs, int frame_cap);
int launch_stereo(hipStream_t st, const OrbgGeom &g, const orbg_keypoint *kps,
                  const uint8_t *desc, const int32_t *counts, const int32_t *d_left,
                  const int32_t *d_right, int npairs, const uint8_t *img0, int64_t img_fs,
                  int img_pitch, const uint8_t *pyr, float bf, float min_z, void *scratch,
                  float *uright, float *depth, int32_t *nvalid, Prof *prof);
// pose_kernels.hip
int launch_pose_opt(hipStream_t st, const orbg_pose_edge *edges, const int32_t *counts, int cap,
                    const orbg_pose_camera *cams, const float *tcw_in, double *q_out,
                    double *t_out, float *tcw_out, uint8_t *outlier, int32_t *ninliers,
                    int nframes, Prof *prof);
int launch_match_pose(hipStream_t st, const orbg_keypoint *kps, const int32_t *counts, int fc,
                      const int32_t *f1, const int32_t *f2, const int32_t *m12, int npairs,
                      const orbg_pose_camera &cam, float depth, const float *inv_sigma2, int nlev,
                      orbg_pose_edge *edges, int32_t *ecount, orbg_pose_camera *cams,
                      float *tcw0, float *tcw_out, uint8_t *outlier, double *q_out,
                      double *t_out, int32_t *ninliers, Prof *prof);
// ba_kernels.hip
int launch_ba(hipStream_t st, const orbg_pose *poses, int npose, const double *points,
              int npoint, const orbg_edge *edges, int nedge, const int32_t *pose_off,
              const int32_t *pose_edges, const int32_t *point_off, const int32_t *point_edges,
              orbg_edge_out *eout, double *hpose, double *bpose, double *hpoint, double *bpoint,
              void *scratch, Prof *prof);
int launch_ba_device(hipStream_t st, const orbg_pose *poses, int npose, const double *points,
                     int npoint, const orbg_edge *edges, int nedge, const int32_t *pose_off,
                     const int32_t *pose_edges, const int32_t *point_off,
                     const int32_t *point_edges, orbg_edge_out *eout, double *hpose,
                     double *bpose, double *hpoint, double *bpoint, double *scr, Prof *prof,
                     bool jacobians, bool errors, double *hpl);
size_t ba_rows_bytes(int nedge, int npose);
size_t ba_scratch_bytes(int npose, int npoint, int nedge);
int launch_ba_errors(hipStream_t st, const orbg_pose *poses, const double *points,
                     const orbg_edge *edges, int nedge, double *err, double *chi2, double *rho0,
                     uint8_t *depth_ok, Prof *prof);
int launch_ba_errors_packed(hipStream_t st, const orbg_pose *poses, const double *points,
                            const BaPackedEdge *edges, const BaCam *cam, const BaInfo *info,
                            int nedge, double *err, double *chi2, double *rho0,
                            uint8_t *depth_ok, Prof *prof);
int launch_ba_graph(hipStream_t st, const orbg_pose *poses, int npose, const double *points,
                    int npoint, const BaPackedEdge *edges, const BaCam *cam, const BaInfo *info,
                    int nedge, const int32_t *pose_off, const int32_t *pose_edges,
                    const int32_t *point_off, const int32_t *point_edges, const BaGraphDev &gd,
                    double *hpl, double *hpose, double *bpose, double *hpoint, double *bpoint,
                    Prof *prof);
// lm_kernels.hip
int launch_ba_update(hipStream_t st, const orbg_pose *poses, int npose, const double *points,
                     int npoint, const double *dxp, const double *dxq, orbg_pose *pout,
                     double *qout);
int launch_lm_reduce(hipStream_t st, int mode, int n1, int n2, double lambda, const double *a1,
                     const double *a2, const double *b1, const double *b2,
                     const BaPackedEdge *edges, double *part, double *out);
int lm_reduce_groups();
// bow_match_kernels.hip
int launch_bow_match(hipStream_t st, const orbg_bow_frames &kf, const orbg_bow_frames &f, int cap,
                     const int32_t *kf_index, const int32_t *f_index, int npairs, float nnratio,
                     int check_ori, int32_t *match, int32_t *nmatch, bool kfkf = false);
// frame_kernels.hip
int launch_undistort(hipStream_t st, const orbg_camera &cam, const orbg_keypoint *kps,
                     const int32_t *counts, int fc, int nframes, orbg_keypoint *out);
int launch_rgbd(hipStream_t st, const void *depth, int u16, float factor, int w, int h,
                size_t pitch, size_t istride, const orbg_keypoint *kps,
                const orbg_keypoint *kps_un, const int32_t *counts, int fc, int nframes,
                float mbf, float *uright, float *dout);
int launch_frustum(hipStream_t st, const orbg_frustum_camera *cams, const orbg_map_point *mps,
                   const int32_t *counts, int cap, int nframes, float cos_limit,
                   orbg_map_projection *out, int32_t *nvisible);
int launch_distinctive(hipStream_t st, const uint8_t *pool, const int32_t *rows,
                       const int32_t *off, int npoints, int32_t *best, uint8_t *desc_out);
// mapping_kernels.hip
int launch_tri_match(hipStream_t st, const orbg_keyframes &K, int cap, const int32_t *kf1,
                     const int32_t *kf2, const orbg_triangulation_pair *geo, int npairs,
                     const float *scale, const float *sigma2, int nlevels, int only_stereo,
                     int check_ori, int32_t *match, int32_t *nmatch);
int launch_fuse(hipStream_t st, const orbg_keyframes &K, int cap, const int32_t *kf,
                const orbg_frustum_camera *cams, const orbg_map_point *mps, const uint8_t *mdesc,
                const int32_t *mcounts, int mcap, int npairs, float th, const float *scale,
                const float *inv_sigma2, int nlevels, int sim3, int32_t *best_idx,
                int32_t *best_dist, int32_t *nfused, int32_t *err_flag);
int launch_search_by_sim3(hipStream_t st, const orbg_keyframes &K, int cap, const int32_t *kf1,
                          const int32_t *kf2, const orbg_sim3_pair *pairs,
                          const orbg_map_point *mps, const uint8_t *mdesc,
                          const uint8_t *matched1, const uint8_t *matched2, int npairs, float th,
                          const float *scale, int nlevels, int32_t *vn, int32_t *match12,
                          int32_t *nfound, int32_t *err_flag);
// triangulate_kernels.hip
int launch_tri_geometry(hipStream_t st, const orbg_kf_camera *cams, const int32_t *kf1,
                        const int32_t *kf2, int npairs, orbg_triangulation_pair *geo);
int launch_triangulate(hipStream_t st, const orbg_keyframes &K, const orbg_keypoint *kps_raw,
                       const float *depth, int cap, const orbg_kf_camera *cams, const int32_t *kf1,
                       const int32_t *kf2, const int32_t *m12, int npairs, const float *scale,
                       const float *sigma2, int nlevels, float scale_factor, float *x3d,
                       int8_t *status, int32_t *nnew);
}  // namespace orbg
