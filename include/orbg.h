/*
 * orbg.h -- C ABI of the MI355X-native ORB-SLAM2 hot path (liborbg.so).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Each entry point replaces one reference interface (/root/reference):
 *
 *   orbg_create / orbg_params ....... ORBextractor::ORBextractor(nfeatures, scaleFactor,
 *                                     nlevels, iniThFAST, minThFAST)   include/ORBextractor.h:64-65
 *                                                                      src/ORBextractor.cc:432-521
 *   orbg_get_scale_tables ........... GetLevels/GetScaleFactor(s)/GetInverseScaleFactors/
 *                                     GetScaleSigmaSquares/GetInverseScaleSigmaSquares
 *                                                                      include/ORBextractor.h:78-98
 *   orbg_extract .................... ORBextractor::operator()(image, mask, keypoints, descriptors)
 *                                                                      include/ORBextractor.h:74-76
 *                                                                      src/ORBextractor.cc:1330-1397
 *   orbg_get_level .................. public std::vector<cv::Mat> mvImagePyramid
 *                                                                      include/ORBextractor.h:101
 *   orbg_descriptor_distance ........ static ORBmatcher::DescriptorDistance
 *                                                                      src/ORBmatcher.cc:1846-1862
 *   orbg_hamming_knn2 ............... brute-force 2-NN over DescriptorDistance (the matcher
 *                                     loops' strict-< best/second rule, ORBmatcher.cc:541-556)
 *   orbg_search_for_initialization .. ORBmatcher(nnratio,checkOri).SearchForInitialization(
 *                                     F1, F2, vbPrevMatched, vnMatches12, windowSize)
 *                                                                      src/ORBmatcher.cc:487-631
 *   orbg_stereo_batch_device ........ Frame::ComputeStereoMatches  src/Frame.cc:619-834
 *   orbg_search_by_projection_lastframe
 *                                     ORBmatcher(0.9,true).SearchByProjection(CurrentFrame,
 *                                     LastFrame, th, bMono)         src/ORBmatcher.cc:1503-1667
 *   orbg_search_by_projection_local . ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th)
 *                                                                      src/ORBmatcher.cc:59-154
 *   orbg_pose_optimization .......... Optimizer::PoseOptimization(Frame*)  src/Optimizer.cc:356-631
 *   orbg_ba_schur_solve ............. g2o BlockSolver<6,3>::solve (Schur complement + pose solve)
 *                                     Thirdparty/g2o/g2o/core/block_solver.hpp:354-486
 *   orbg_vocab_load_text ............ TemplatedVocabulary::loadFromTextFile
 *                                     Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1337-1420
 *   orbg_bow_transform .............. TemplatedVocabulary::transform(features, BowVector,
 *                                     FeatureVector, levelsup) as Frame::ComputeBoW calls it
 *                                     TemplatedVocabulary.h:1126-1189, 1220-1259; Frame.cc:532-539
 *   orbg_bow_score .................. TemplatedVocabulary::score = L1Scoring::score
 *                                     Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
 *   orbg_kfdb_add / _erase / _clear . KeyFrameDatabase::add / erase / clear
 *                                     src/KeyFrameDatabase.cc:50-83
 *   orbg_kfdb_detect_reloc .......... KeyFrameDatabase::DetectRelocalizationCandidates
 *                                     src/KeyFrameDatabase.cc:291-419 (Tracking.cc:1958)
 *   orbg_kfdb_detect_loop ........... KeyFrameDatabase::DetectLoopCandidates
 *                                     src/KeyFrameDatabase.cc:106-274 (LoopClosing.cc:162-212)
 *   orbg_search_by_bow .............. ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)
 *                                     src/ORBmatcher.cc:195-348 (Tracking.cc:1069, 2009)
 *   orbg_search_by_bow_kf ........... ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)
 *                                     src/ORBmatcher.cc:634-769 (LoopClosing.cc:485)
 *   orbg_undistort_keypoints ........ Frame::UndistortKeyPoints  src/Frame.cc:542-572
 *   orbg_compute_image_bounds ....... Frame::ComputeImageBounds  src/Frame.cc:575-611
 *   orbg_is_in_frustum .............. Frame::isInFrustum(pMP, viewingCosLimit)  src/Frame.cc:342-409
 *                                     (Tracking::SearchLocalPoints, Tracking.cc:1676-1691)
 *   orbg_distinctive_descriptor ..... MapPoint::ComputeDistinctiveDescriptors  src/MapPoint.cc:342-420
 *   orbg_search_for_triangulation ... ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12,
 *                                     vMatchedPairs, bOnlyStereo)  src/ORBmatcher.cc:779-957
 *                                     (LocalMapping::CreateNewMapPoints, LocalMapping.cc:378)
 *   orbg_fuse ....................... ORBmatcher::Fuse(pKF, vpMapPoints, th)'s per-MapPoint search
 *   orbg_fuse_sim3 .................. ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)'s search
 *   orbg_search_by_projection_reloc . ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
 *   orbg_search_by_projection_sim3 .. ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
 *   orbg_rgbd_stereo ................ Frame::ComputeStereoFromRGBD (+ GrabImageRGBD's depth scaling)
 *   orbg_search_by_sim3 ............. ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 *                                     src/ORBmatcher.cc:968-1069 (LocalMapping::SearchInNeighbors,
 *                                     LocalMapping.cc:622-690)
 *   orbg_ba_linearize ............... g2o computeActiveErrors + BlockSolver::buildSystem arithmetic
 *                                     for EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ inside
 *                                     Optimizer::LocalBundleAdjustment  src/Optimizer.cc:633-979
 *   orbg_optimize_sim3 .............. Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2,
 *                                     bFixScale)  src/Optimizer.cc:1366-1578 (LoopClosing.cc:598)
 *   orbg_pnp_solve .................. PnPsolver(F, vpMapPointMatches) + SetRansacParameters +
 *                                     iterate / find  src/PnPsolver.cc:67-900
 *                                     (Tracking::Relocalization, Tracking.cc:2017-2060)
 *   orbg_optimize_essential_graph ... Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF,
 *                                     NonCorrectedSim3, CorrectedSim3, LoopConnections,
 *                                     bFixScale)'s optimisation and write-back arithmetic
 *                                     src/Optimizer.cc:1021-1324 (LoopClosing.cc:914)
 *   orbg_initialize ................. Initializer(ReferenceFrame, sigma, iterations) +
 *                                     Initialize(CurrentFrame, vMatches12, R21, t21, vP3D,
 *                                     vbTriangulated)  src/Initializer.cc:34-1270
 *                                     (Tracking::MonocularInitialization, Tracking.cc:588-676)
 *   orbg_map_update_connections ..... KeyFrame::UpdateConnections (+ AddConnection,
 *                                     UpdateBestCovisibles)  src/KeyFrame.cc:160-205, 375-515
 *   orbg_map_erase_keyframe ......... KeyFrame::SetBadFlag's EraseConnection loop  src/KeyFrame.cc:618-648
 *   orbg_map_local_keyframes ........ Tracking::UpdateLocalKeyFrames  src/Tracking.cc:1769-1925
 *   orbg_map_local_points ........... Tracking::UpdateLocalPoints  src/Tracking.cc:1731-1758
 *                                     (+ SearchLocalPoints' mnLastFrameSeen test, :1644-1683)
 *   orbg_map_update_normal_and_depth_batch_device
 *                                     MapPoint::UpdateNormalAndDepth  src/MapPoint.cc:457-518
 *   orbg_map_set_bad_flag ........... KeyFrame::SetBadFlag in full (+ MapPoint::EraseObservation /
 *                                     SetBadFlag)  src/KeyFrame.cc:622-720, src/MapPoint.cc:159-232
 *   orbg_map_keyframe_culling ....... LocalMapping::KeyFrameCulling  src/LocalMapping.cc:804-877
 *   orbg_map_point_culling .......... LocalMapping::MapPointCulling  src/LocalMapping.cc:227-270
 *
 * Batched, device-resident entry points (orbg_*_device) run the same kernels over many
 * frames at once; they exist for the batched-sequence mode and the bench.
 *
 * Conventions: every int-returning function returns ORBG_OK (0) or a negative errno-style
 * code; orbg_last_error() gives a message for the calling thread.  No C++ exception crosses
 * the ABI.  The caller owns all output buffers.  A context owns its device buffers and one
 * HIP stream; a context is not thread-safe, distinct contexts may run concurrently (the two
 * stereo extractors of Frame.cc:110-113).
 */
#ifndef ORBG_H
#define ORBG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBG_ABI_VERSION 1
#define ORBG_MAX_LEVELS 16

#define ORBG_OK 0
#define ORBG_EIO -5       /* HIP runtime / device error */
#define ORBG_ENOMEM -12
#define ORBG_EINVAL -22
#define ORBG_ERANGE -34   /* caller capacity too small; *n_out holds the needed count */
#define ORBG_ENOTSUP -95  /* configuration outside what the reference defines */

/* cv::resize INTER_LINEAR 8UC1 vertical-pass variant (OpenCV build pin) */
#define ORBG_RESIZE_SCALAR 0
#define ORBG_RESIZE_SSE2_16_4 4
#define ORBG_RESIZE_SIMD_16_8 8

typedef struct orbg_ctx orbg_ctx;

typedef struct {
    /* ORBextractor ctor arguments */
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    /* OpenCV primitive pins (orbg_params_default sets the OpenCV 3.4 values) */
    int32_t resize_mode;   /* ORBG_RESIZE_* */
    int32_t gauss_k[7];    /* GaussianBlur 7x7 sigma=2 fixed-point weights */
    int32_t brief_fma;     /* 1: fuse x*b + y*a in rBRIEF sampling (reference built -ffp-contract=fast) */
    /* batch capacity (frames per orbg_extract_batch_device call); 0 -> 1 */
    int32_t max_batch;
    /* cos/sin of the rBRIEF rotation (ORBextractor.cc:122, (float)cos(float) = glibc cosf):
     * ORBG_SINCOS_GLIBC restates glibc 2.35's sinf/cosf (bit-equal to the host libm on every
     * float in [0, 7)); ORBG_SINCOS_PINNED is round 1's correctly rounded evaluation */
    int32_t sincos_mode;
} orbg_params;

#define ORBG_SINCOS_GLIBC 0
#define ORBG_SINCOS_PINNED 1

/* cv::KeyPoint layout: pt.x, pt.y, size, angle, response, octave, class_id (28 bytes) */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbg_keypoint;

/* ---------------- context / extractor ---------------- */
void orbg_params_default(orbg_params *p);
int orbg_create(int device, const orbg_params *p, orbg_ctx **out);
void orbg_destroy(orbg_ctx *ctx);
const char *orbg_last_error(void);
int orbg_abi_version(void);

/* GetLevels / GetScaleFactor(s) / inverse / sigma^2 tables; any pointer may be NULL.
 * Arrays must hold nlevels entries.  features_per_level = mnFeaturesPerLevel, umax[16]. */
int orbg_get_scale_tables(const orbg_ctx *ctx, int32_t *nlevels, float *scale_factor,
                          float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                          int32_t *features_per_level, int32_t *umax);
/* the 256 rBRIEF test pairs (x0,y0,x1,y1) the kernels use (bit_pattern_31_) */
int orbg_get_pattern(int32_t out[1024]);

/* ORBextractor::operator() on one host image (CV_8UC1, row pitch `step`).
 * w == 0 or h == 0: returns ORBG_OK with *n_out = -1 and outputs untouched (:1333-1334).
 * Otherwise kps[0..n) in level order, desc n x 32 bytes row-major.  If cap < n, returns
 * ORBG_ERANGE with *n_out = n and nothing written. */
int orbg_extract(orbg_ctx *ctx, const uint8_t *img, int w, int h, size_t step,
                 orbg_keypoint *kps, uint8_t *desc, int cap, int *n_out);

/* mvImagePyramid[level] of frame `frame` of the last extraction (host copy). */
int orbg_get_level(orbg_ctx *ctx, int frame, int level, uint8_t *dst, size_t dst_step, int *lw,
                   int *lh);
/* The GaussianBlur(7x7, sigma 2, REFLECT_101) of pyramid level `level` of frame `frame` of the
 * last extraction: the image computeOrbDescriptor samples (ORBextractor.cc:1375-1377, a local
 * cv::Mat there, no public member).  Parity / debugging accessor; same contract as
 * orbg_get_level. */
int orbg_get_blurred_level(orbg_ctx *ctx, int frame, int level, uint8_t *dst, size_t dst_step,
                           int *lw, int *lh);

/* ---------------- batched, device-resident ---------------- */
/* d_imgs: device pointer, nframes images of w x h, row pitch `step`, frame pitch
 * `frame_stride` bytes.  Enqueued on the context stream; the caller keeps d_imgs alive
 * until the next call (level 0 of the pyramid IS the input). */
int orbg_extract_batch_device(orbg_ctx *ctx, const uint8_t *d_imgs, int nframes, int w, int h,
                              size_t step, size_t frame_stride);
/* device pointers to the last batch's outputs: frame f keypoints at d_kps + f*frame_cap,
 * descriptors at d_desc + f*frame_cap*32, count d_counts[f]. */
int orbg_batch_outputs(orbg_ctx *ctx, orbg_keypoint **d_kps, uint8_t **d_desc,
                       int32_t **d_counts, int32_t *frame_cap);
/* copy frame `frame` of the last batch to the host (synchronises) */
int orbg_download_frame(orbg_ctx *ctx, int frame, orbg_keypoint *kps, uint8_t *desc, int cap,
                        int *n_out);

/* Match pairs of frames of the last batch on the device: for pair i, F1 = frame f1[i]
 * (reference / previous), F2 = frame f2[i] (current).
 *  - knn2: for every F2 keypoint, best/second distance and best index over all F1
 *    descriptors (all-pairs Hamming).
 *  - SearchForInitialization(F1, F2, vbPrevMatched = F1 keypoint positions, window)
 *    with image bounds (0, w, 0, h) (undistorted KITTI-style frames, Frame.cc:603-609).
 * Results stay on the device (orbg_match_outputs). */
int orbg_match_batch_device(orbg_ctx *ctx, const int32_t *f1, const int32_t *f2, int npairs,
                            int window, float nnratio, int check_ori);
int orbg_match_outputs(orbg_ctx *ctx, int32_t **d_knn /* [npairs][frame_cap][3] */,
                       int32_t **d_matches12 /* [npairs][frame_cap] */,
                       int32_t **d_nmatches /* [npairs] */, int32_t *frame_cap);
int orbg_download_matches(orbg_ctx *ctx, int pair, int32_t *knn, int32_t *matches12,
                          int cap, int32_t *nmatches);

/* Extraction runs on the context stream; batch matching and the summary run on a second
 * (match) stream so the matching of batch k overlaps the extraction of batch k+1.  The
 * per-frame outputs alternate between two buffers (orbg_batch_outputs returns the ones of
 * the last extraction); every host-side read (download, get_level, stats, sync) drains
 * both streams. */
/* Frame::ComputeStereoMatches (src/Frame.cc:619-834) for npairs (left, right) frames of the
 * last batch: row-band descriptor match, 11x11 SAD refinement at the keypoint's level,
 * parabola, median cut.  bf = Frame::mbf; min_z = Frame::mb, which the reference reads before
 * assigning it (Frame.cc:661 vs :148) -- pass bf / fx, the value assigned right after
 * (min_z <= 0: no maximum disparity).  Runs where the batch's keypoint half ran (it reads
 * this batch's pyramid): the context stream, or with pipelined batches the internal back
 * stream.  Results per pair over the left frame's keypoints: mvuRight, mvDepth (-1 where
 * unmatched) and the number of depths; device readers order themselves after the match
 * stream via orbg_stereo_summary, or call orbg_sync. */
int orbg_stereo_batch_device(orbg_ctx *ctx, const int32_t *left, const int32_t *right,
                             int npairs, float bf, float min_z);
int orbg_stereo_outputs(orbg_ctx *ctx, float **d_uright /* [npairs][frame_cap] */,
                        float **d_depth /* [npairs][frame_cap] */,
                        int32_t **d_nvalid /* [npairs] */, int32_t *frame_cap);
/* The stereo Frame constructor on host images (Frame.cc:86-161): ORBextractor on the left
 * and right image (both CV_8UC1, same size and row pitch) + ComputeStereoMatches.  Outputs
 * as orbg_extract for each image (ORBG_ERANGE with *n_l / *n_r set if a capacity is short);
 * uright / depth receive *n_l entries (mvuRight, mvDepth). */
int orbg_stereo_frame(orbg_ctx *ctx, const uint8_t *left, const uint8_t *right, int w, int h,
                      size_t step, float bf, float min_z, orbg_keypoint *kps_l, uint8_t *desc_l,
                      int cap_l, int *n_l, orbg_keypoint *kps_r, uint8_t *desc_r, int cap_r,
                      int *n_r, float *uright, float *depth);
/* per-pair summary of the last stereo batch, written on the match stream (orbg_match_stream,
 * ordered after the stereo pass, as orbg_batch_summary) into a device buffer: order readers
 * after the match stream, or orbg_sync.  d_out[p] = keypoints of the left frame of pair p,
 * d_out[npairs + p] = keypoints with a depth */
int orbg_stereo_summary(orbg_ctx *ctx, int32_t *d_out);
/* copies cap entries of pair `pair` (synchronises) */
int orbg_download_stereo(orbg_ctx *ctx, int pair, float *uright, float *depth, int cap,
                         int32_t *nvalid);

/* Device error flags are sticky: a frame whose quadtree level overflowed a capacity (its
 * keypoints would be incomplete) sets a flag that stays set until read.  orbg_sync,
 * orbg_check_errors, orbg_batch_stats and orbg_download_frame drain the streams, read and
 * clear it, and return ORBG_ENOTSUP (orbg_last_error names the flags and the first frame)
 * if any batch since the last read raised one.  The device matchers that read per-pair
 * counts from device memory (orbg_fuse[_sim3]_batch_device, orbg_search_by_sim3_batch_device)
 * clamp a count past its capacity (KeyFrame counts to `cap`, MapPoint counts to `mcap`) and
 * raise flag 0x10000; the next read returns ORBG_EINVAL naming the first pair. */
int orbg_sync(orbg_ctx *ctx);
int orbg_check_errors(orbg_ctx *ctx);
void *orbg_stream(orbg_ctx *ctx);       /* hipStream_t of extraction (and host-data calls) */
void *orbg_match_stream(orbg_ctx *ctx); /* hipStream_t of batch matching and the summary */
/* launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * context's own; NULL restores the context stream */
int orbg_set_stream(orbg_ctx *ctx, void *stream);
/* Pipelined batches (batched-sequence mode; no reference counterpart -- the reference
 * extracts one frame per Tracking call): with enable != 0 the image half of a batch
 * (pyramid, FAST cells, GaussianBlur) runs on the context stream and its keypoint half
 * (quadtree, orientation + rBRIEF, stereo) on an internal high-priority stream, so the image
 * half of batch k+1 overlaps the keypoint half of batch k.  Outputs, the batch's errors and
 * the summary are unchanged; the per-frame outputs of a batch are complete when the match
 * stream's work on them is (orbg_match_batch_device / orbg_batch_summary order themselves
 * after it) or after orbg_sync.  The batch's input images must stay unchanged until then.
 * Also selected with the environment variable ORBG_PIPELINE=1 at orbg_create.
 * Synchronises.  ORBG_ENOTSUP without the internal stream. */
int orbg_set_pipeline(orbg_ctx *ctx, int enable);
int orbg_get_pipeline(const orbg_ctx *ctx);
/* Serial execution (measurement; no reference counterpart): with enable != 0 every
 * extraction kernel runs on the context stream, one after the other (no pipelining, no
 * internal streams), so per-kernel event times are the kernels' own.  Outputs unchanged.
 * Synchronises. */
int orbg_set_serial(orbg_ctx *ctx, int enable);
/* Caller buffers written on the match stream (orbg_batch_summary, orbg_batch_matches,
 * orbg_match_pose_batch_device, orbg_stereo_summary) are stream-ordered on the writer side:
 * at entry each records an event on the context stream (orbg_set_stream) and the match
 * stream waits for it, so work the caller queued on the context stream before the call (a
 * fill of d_out, an upload) completes before liborbg writes.  Work on any OTHER stream must
 * be ordered by the caller.  Readers order themselves after orbg_match_stream, or orbg_sync.
 *
 * per-frame trajectory summary of the last batch, written on the match stream into a
 * device buffer: d_out[f] = keypoints of frame f (f < nframes), then
 * d_out[nframes + p] = SearchForInitialization matches of pair p (p < npairs of the last
 * orbg_match_batch_device, 0 if none) */
int orbg_batch_summary(orbg_ctx *ctx, int32_t *d_out);
/* Caller reads of the last batch's device outputs (orbg_batch_outputs, and
 * orbg_stereo_outputs after a stereo pass) on a caller stream (NULL: the match stream), for
 * pipelined batches where they are written on internal streams:
 *   orbg_batch_acquire: `stream` waits until those outputs are written;
 *   orbg_batch_release: every read enqueued on `stream` so far finishes before liborbg
 *   overwrites those outputs (the extraction that reuses the output slot, the next stereo
 *   pass wait for it).  Releases on several reader streams of one batch chain: each waits
 *   for the previous release, so the slot waits for every reader.
 * Enqueue only; no host synchronisation. */
int orbg_batch_acquire(orbg_ctx *ctx, void *stream);
int orbg_batch_release(orbg_ctx *ctx, void *stream);
/* vnMatches12 of every pair of the last orbg_match_batch_device (ORBmatcher.cc:487-631's
 * output; the batched-sequence gather of SURVEY 8e), written on the match stream into a
 * device buffer: d_out[p * frame_cap + i] = index in frame f2[p] matched to keypoint i of
 * frame f1[p], -1 if none or i >= keypoints of f1[p].  *frame_cap (if non-NULL) receives the
 * row length; d_out == NULL only queries it.  ORBG_EINVAL without a match batch. */
int orbg_batch_matches(orbg_ctx *ctx, int32_t *d_out, int32_t *frame_cap);
/* host-side statistics of the last batch (synchronises): FAST candidates over all
 * cells/levels/frames and output keypoints over all frames (for bandwidth accounting) */
int orbg_batch_stats(orbg_ctx *ctx, int64_t *ncandidates, int64_t *nkeypoints);
/* the quadtree launch plan of the last planned image size (DistributeOctTree,
 * ORBextractor.cc:668-951): the FAST-candidate caps of level 0's split pair of k_octree_lds
 * launches in a batch (first_cap; 0 = no split) and of its single launch (level0_cap), and of
 * the levels-1.. launch (upper_cap); a level with more candidates goes to the k_octree
 * fallback.  ORBG_EINVAL before any extraction. */
int orbg_get_quadtree_caps(const orbg_ctx *ctx, int32_t *first_cap, int32_t *level0_cap,
                           int32_t *upper_cap);
/* the GaussianBlur plan of the last planned image size (ORBextractor.cc:1375-1377): *fused =
 * 1 when the FAST cells blur their detection regions from the window tiles they stage (the
 * pixels of every level's rectangle of regions, *interior_px per frame) and a border pass
 * blurs the rest (*border_px per frame); 0 when one blur pass covers every level.  Any
 * pointer may be NULL.  ORBG_EINVAL before any extraction. */
int orbg_get_blur_plan(const orbg_ctx *ctx, int32_t *fused, int64_t *interior_px,
                       int64_t *border_px);
/* the blurred levels' device layout of the last planned image size: *tiled = 1 for 16 x 8-pixel
 * tiles of 128 bytes (k_blur2's default store form, read by the rBRIEF phase), 0 for rows
 * (ORBG_BLUR_TILED=0 at orbg_create, or a blur written by another pass).  Internal; the
 * accessor orbg_get_blurred_level always returns rows.  ORBG_EINVAL before any extraction. */
int orbg_get_blur_layout(const orbg_ctx *ctx, int32_t *tiled);

/* per-kernel timing with HIP events on the context stream (for bench roofline) */
int orbg_profile_enable(orbg_ctx *ctx, int enable);
/* returns number of kernel kinds; fills name/total_ms/launches for index i */
int orbg_profile_read(orbg_ctx *ctx, int i, const char **name, double *total_ms,
                      int64_t *launches);
int orbg_profile_reset(orbg_ctx *ctx);

/* ---------------- matcher (host data) ---------------- */
int orbg_descriptor_distance(const uint8_t *a, const uint8_t *b);

/* best/second over all train descriptors for every query (strict <, lowest index on ties) */
int orbg_hamming_knn2(orbg_ctx *ctx, const uint8_t *qdesc, int nq, const uint8_t *tdesc, int nt,
                      int32_t *best_idx, int32_t *best_dist, int32_t *second_dist);

typedef struct {
    float min_x, max_x, min_y, max_y; /* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY */
} orbg_bounds;

/* kps1/kps2 are mvKeysUn (x, y, angle, octave used); prev_xy (2*n1 floats) is
 * vbPrevMatched, updated in place; matches12[n1] = vnMatches12. */
int orbg_search_for_initialization(orbg_ctx *ctx, const orbg_keypoint *kps1,
                                   const uint8_t *desc1, int n1, const orbg_keypoint *kps2,
                                   const uint8_t *desc2, int n2, const orbg_bounds *bounds2,
                                   float *prev_xy, int32_t *matches12, int window,
                                   float nnratio, int check_ori, int *nmatches);

/* ---------------- tracking matchers ----------------
 * The MapPoint / Frame state the two SearchByProjection loops read enters as flat records;
 * their writes come back as match[N] (CurrentFrame.mvpMapPoints as a query index; -1 = not
 * written; -2 = set to NULL by the rotation-consistency filter) and nmatches.  The frame side is CurrentFrame (F): kps = mvKeysUn,
 * desc = mDescriptors, uright = mvuRight (NULL for monocular), taken0 (NULL = none) =
 * "mvpMapPoints[i] && mvpMapPoints[i]->Observations() > 0" on entry, bounds = mnMinX...
 * Scale factors are the context's (ORBextractor GetScaleFactors). */
#define ORBG_MP_VALID 1    /* lastframe: pMP && !LastFrame.mvbOutlier[i]; local: mbTrackInView && !isBad() */
#define ORBG_MP_HAS_OBS 2  /* pMP->Observations() > 0 */

typedef struct {
    float x, y, z;     /* pMP->GetWorldPos() */
    int32_t octave;    /* LastFrame.mvKeys[i].octave */
    float angle;       /* LastFrame.mvKeysUn[i].angle */
    int32_t flags;     /* ORBG_MP_* */
} orbg_lastframe_point;

typedef struct {
    float u, v, ur;    /* mTrackProjX, mTrackProjY, mTrackProjXR (Frame::isInFrustum) */
    int32_t level;     /* mnTrackScaleLevel */
    float view_cos;    /* mTrackViewCos */
    int32_t flags;     /* ORBG_MP_* */
} orbg_map_projection;

typedef struct {
    float Tcw[12];     /* CurrentFrame.mTcw rows 0..2 (row-major 3x4) */
    float Tlw[12];     /* LastFrame.mTcw rows 0..2 */
    float fx, fy, cx, cy, bf, b;  /* Frame::fx.., mbf, mb */
    int32_t mono;      /* bMono */
    int32_t pad;
} orbg_track_camera;

/* ORBmatcher(nnratio, checkOri).SearchByProjection(CurrentFrame, LastFrame, th, bMono):
 * pts[np] / pdesc = LastFrame.mvpMapPoints[i] (one record per LastFrame keypoint). */
int orbg_search_by_projection_lastframe(orbg_ctx *ctx, const orbg_keypoint *kps,
                                        const uint8_t *desc, const float *uright, int n,
                                        const uint8_t *taken0, const orbg_bounds *bounds,
                                        const orbg_lastframe_point *pts, const uint8_t *pdesc,
                                        int np, const orbg_track_camera *cam, float th,
                                        int check_ori, int32_t *match, int *nmatches);

/* ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th): mps[nm] / mdesc. */
int orbg_search_by_projection_local(orbg_ctx *ctx, const orbg_keypoint *kps,
                                    const uint8_t *desc, const float *uright, int n,
                                    const uint8_t *taken0, const orbg_bounds *bounds,
                                    const orbg_map_projection *mps, const uint8_t *mdesc, int nm,
                                    float th, float nnratio, int32_t *match, int *nmatches);

/* Batched, device-resident form of both (mode ORBG_TRACK_LASTFRAME / ORBG_TRACK_LOCAL) and
 * of the relocalization / loop searches below (ORBG_TRACK_RELOC / ORBG_TRACK_LOOP): every
 * pointer is device memory, frame f's arrays at f * frame_cap (keypoint side) and
 * f * query_cap (query side); enqueued on the context stream. */
#define ORBG_TRACK_LASTFRAME 0
#define ORBG_TRACK_LOCAL 1
#define ORBG_TRACK_RELOC 2
#define ORBG_TRACK_LOOP 3
struct orbg_frustum_camera;
typedef struct {
    const orbg_keypoint *kps;    /* [B][frame_cap] */
    const uint8_t *desc;         /* [B][frame_cap][32] */
    const float *uright;         /* [B][frame_cap] or NULL */
    const uint8_t *taken0;       /* [B][frame_cap] or NULL */
    const int32_t *counts;       /* [B] */
    const orbg_bounds *bounds;   /* [B] */
    int32_t frame_cap;
    const void *queries;         /* [B][query_cap] orbg_lastframe_point / orbg_map_projection /
                                    orbg_reloc_point / orbg_map_point, by mode */
    const uint8_t *qdesc;        /* [B][query_cap][32] */
    const int32_t *qcounts;      /* [B] */
    int32_t query_cap;
    const orbg_track_camera *cams;  /* [B], last-frame mode */
    float th, nnratio;
    int32_t check_ori;
    int32_t *match;              /* [B][frame_cap] out */
    int32_t *nmatches;           /* [B] out */
    /* appended in round 4 (ABI note): read only in the relocalization / loop
     * modes, so a caller built against the older, shorter struct stays valid in the
     * last-frame / local-map modes */
    const struct orbg_frustum_camera *fcams;  /* [B], relocalization / loop modes */
    int32_t orb_dist;            /* relocalization: ORBdist */
} orbg_track_batch;
int orbg_search_by_projection_batch_device(orbg_ctx *ctx, int mode, const orbg_track_batch *tb,
                                           int nframes);

/* ---------------- Frame / MapPoint geometry ---------------- */
/* Frame::mK (fx, fy, cx, cy) and Frame::mDistCoef (k1, k2, p1, p2[, k3]: k3 = 0 when the
 * settings file has none, Tracking.cc's DistCoef of 4 entries) */
typedef struct {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
} orbg_camera;

/* Frame::UndistortKeyPoints (src/Frame.cc:542-572): kps_un[i] = kps[i] with pt replaced by
 * cv::undistortPoints(pt, K, D, noArray(), K) (OpenCV 3.4: 5 fixed-point iterations in
 * double); k1 == 0: a copy (mvKeysUn = mvKeys).  Host arrays; kps_un may alias
 * kps. */
int orbg_undistort_keypoints(orbg_ctx *ctx, const orbg_camera *cam, const orbg_keypoint *kps,
                             int n, orbg_keypoint *kps_un);
/* The same on the device for a batch: frame f's counts[f] keypoints at d_kps + f * frame_cap
 * -> d_kps_un + f * frame_cap (entries past counts[f] untouched).  Context stream. */
int orbg_undistort_batch_device(orbg_ctx *ctx, const orbg_camera *cam, const orbg_keypoint *d_kps,
                                const int32_t *d_counts, int frame_cap, int nframes,
                                orbg_keypoint *d_kps_un);
/* Frame::ComputeStereoFromRGBD (src/Frame.cc:837-858; the RGB-D Frame constructor) after
 * Tracking::GrabImageRGBD's depth conversion (Tracking.cc:233-234: imDepth.convertTo(CV_32F,
 * mDepthMapFactor) when |mDepthMapFactor - 1| > 1e-5 or the image is not CV_32F).  depth:
 * a w x h image, row pitch `pitch` bytes, ORBG_DEPTH_U16 (raw) or ORBG_DEPTH_F32; factor =
 * mDepthMapFactor (1 / DepthMapFactor of the settings); a pixel's depth is raw * factor
 * rounded once to float (convertTo's float alpha), or the float itself when it is F32 and
 * factor is within 1e-5 of 1.  kps = mvKeys (their truncated (x, y) index the depth image;
 * outside it: no depth), kps_un = mvKeysUn.  Per keypoint: d > 0 -> depth[i] = d,
 * uright[i] = kps_un[i].x - mbf / d; else both -1. */
#define ORBG_DEPTH_F32 0
#define ORBG_DEPTH_U16 1
int orbg_rgbd_stereo(orbg_ctx *ctx, const void *depth, int depth_type, float factor, int w, int h,
                     size_t pitch, const orbg_keypoint *kps, const orbg_keypoint *kps_un, int n,
                     float mbf, float *uright, float *depth_out);
/* The same on the device for a batch: frame f's depth image at d_depth + f * image_stride
 * bytes, its counts[f] keypoints at d_kps / d_kps_un + f * frame_cap, outputs at + f * frame_cap
 * (entries past counts[f] untouched).  Context stream. */
int orbg_rgbd_stereo_batch_device(orbg_ctx *ctx, const void *d_depth, int depth_type, float factor,
                                  int w, int h, size_t pitch, size_t image_stride,
                                  const orbg_keypoint *d_kps, const orbg_keypoint *d_kps_un,
                                  const int32_t *d_counts, int frame_cap, int nframes, float mbf,
                                  float *d_uright, float *d_depth_out);
/* Frame::ComputeImageBounds (src/Frame.cc:575-611) for a w x h image: mnMinX .. mnMaxY (the
 * undistorted image corners when k1 != 0, else 0, w, 0, h).  Host only (four points, the
 * expression k_undistort evaluates). */
int orbg_compute_image_bounds(const orbg_camera *cam, int w, int h, orbg_bounds *out);
/* Batched-sequence mode with a distorted camera (TUM / EuRoC settings): after
 * orbg_set_camera(ctx, cam) with cam->k1 != 0, orbg_match_batch_device first undistorts the
 * batch's keypoints on the match stream (Frame::UndistortKeyPoints, as the Frame constructor
 * does after ExtractORB, Frame.cc:259) and SearchForInitialization (and the pose stub)
 * read mvKeysUn with ComputeImageBounds' bounds; orbg_batch_keys_un returns the device array
 * ([frames][frame_cap], valid after that match stream work).  cam == NULL or k1 == 0: the
 * default (mvKeysUn = mvKeys, bounds 0, w, 0, h). */
int orbg_set_camera(orbg_ctx *ctx, const orbg_camera *cam);
int orbg_batch_keys_un(orbg_ctx *ctx, orbg_keypoint **d_kps_un, int32_t *frame_cap);

/* What Frame::isInFrustum reads of a MapPoint: GetWorldPos(), GetNormal(), mfMinDistance,
 * mfMaxDistance; flags: ORBG_MP_VALID = Tracking::SearchLocalPoints tests the point
 * (!isBad() && mnLastFrameSeen != CurrentFrame.mnId, Tracking.cc:1680-1683), ORBG_MP_HAS_OBS
 * passed through to the projection. */
typedef struct {
    float x, y, z;
    float nx, ny, nz;
    float min_dist, max_dist;
    int32_t flags;
} orbg_map_point;
/* The Frame state isInFrustum reads: mTcw rows 0..2 (row-major 3x4), fx, fy, cx, cy, mbf,
 * mfLogScaleFactor (= log(mfScaleFactor), in double then float), mnScaleLevels, mnMinX.. */
typedef struct orbg_frustum_camera {
    float Tcw[12];
    float fx, fy, cx, cy, bf;
    float log_scale_factor;
    int32_t nlevels;
    orbg_bounds bounds;
} orbg_frustum_camera;
/* Frame::isInFrustum(pMP, viewing_cos_limit) for n map points (host arrays): proj[i] = the
 * mTrack* members SearchByProjection(F, vpMapPoints) reads (orbg_map_projection:
 * mTrackProjX/Y/XR, mnTrackScaleLevel, mTrackViewCos; flags ORBG_MP_VALID = mbTrackInView,
 * ORBG_MP_HAS_OBS passed through).  A point not in view gets only its flags written (the
 * reference leaves the other members as they were).  *nvisible = points in view. */
int orbg_is_in_frustum(orbg_ctx *ctx, const orbg_frustum_camera *cam, const orbg_map_point *mps,
                       int n, float viewing_cos_limit, orbg_map_projection *proj, int *nvisible);
/* Batched, device memory: frame f's counts[f] points at d_mps + f * cap, camera d_cams[f],
 * projections at d_proj + f * cap, d_nvisible[f].  Context stream. */
int orbg_is_in_frustum_batch_device(orbg_ctx *ctx, const orbg_frustum_camera *d_cams,
                                    const orbg_map_point *d_mps, const int32_t *d_counts, int cap,
                                    int nframes, float viewing_cos_limit,
                                    orbg_map_projection *d_proj, int32_t *d_nvisible);
/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:342-420) for one map point: the n
 * observation descriptors (n x 32 bytes, in the mObservations order, bad KeyFrames left out)
 * -> *best = BestIdx, the row with the least median distance to the others (the first on
 * ties), -1 if n == 0. */
int orbg_distinctive_descriptor(orbg_ctx *ctx, const uint8_t *desc, int n, int32_t *best);
/* Batched, device memory: map point p's observations are descriptor rows
 * d_pool[d_rows[d_off[p]] .. d_rows[d_off[p+1]-1]] (32 bytes each, e.g. the KeyFrames'
 * mDescriptors resident in HBM); d_best[p] = BestIdx (-1: no observation) and, if d_desc is
 * not NULL, d_desc[p * 32 ..] = that descriptor (mDescriptor).  Context stream. */
int orbg_distinctive_descriptors_batch_device(orbg_ctx *ctx, const uint8_t *d_pool,
                                              const int32_t *d_rows, const int32_t *d_off,
                                              int npoints, int32_t *d_best, uint8_t *d_desc);

/* ---------------- LocalMapping matchers ---------------- */
/* A set of KeyFrames in device memory, frame k's rows at + k * cap (fv_off at + k * (cap + 1)):
 * mDescriptors [cap][32], mvKeysUn [cap] (x, y, angle, octave read), mvuRight [cap] (NULL: all
 * monocular), has_mp [cap] = GetMapPoint(i) != NULL (NULL: none), counts[k] = N, and mFeatVec
 * in orbg_bow_transform_batch_device's layout. */
typedef struct {
    const uint8_t *desc;
    const orbg_keypoint *kps;
    const float *uright;
    const uint8_t *has_mp;
    const int32_t *counts;
    const int32_t *fv_nodes, *fv_off, *fv_feats, *nfv;
} orbg_keyframes;
/* The geometry of one SearchForTriangulation pair: F12 (row-major 3x3, LocalMapping::
 * ComputeF12), pKF1->GetCameraCenter(), pKF2->mTcw rows 0..2 (row-major 3x4) and pKF2's
 * fx, fy, cx, cy (the epipole, ORBmatcher.cc:800-806). */
typedef struct {
    float F12[9];
    float Cw1[3];
    float Tcw2[12];
    float fx2, fy2, cx2, cy2;
} orbg_triangulation_pair;
/* ORBmatcher(nnratio, checkOri).SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs,
 * bOnlyStereo) for pairs p: KeyFrames d_kf1[p], d_kf2[p] of `kfs`, geometry d_geo[p].
 * d_matches12[p * cap + i] = vMatches12[i] (the pKF2 index matched to pKF1's feature i, -1;
 * vMatchedPairs = the (i, d_matches12[i]) with d_matches12[i] >= 0 in i order) for i < N of
 * pKF1; d_nmatches[p] = the return value.  Scale factors and sigma^2 are the context's
 * (pKF2->mvScaleFactors / mvLevelSigma2).  Context stream.  ORBG_ENOTSUP past 65535
 * features per frame. */
int orbg_search_for_triangulation_batch_device(orbg_ctx *ctx, const orbg_keyframes *kfs, int cap,
                                               const int32_t *d_kf1, const int32_t *d_kf2,
                                               const orbg_triangulation_pair *d_geo, int npairs,
                                               int only_stereo, int check_ori,
                                               int32_t *d_matches12, int32_t *d_nmatches);
/* One KeyFrame from host arrays (as orbg_keyframes, one frame; uright / has_mp may be NULL) */
typedef struct {
    const orbg_keypoint *kps;
    const uint8_t *desc;
    const float *uright;
    const uint8_t *has_mp;
    int32_t n;
    const int32_t *fv_nodes, *fv_off, *fv_feats;
    int32_t nfv;
} orbg_keyframe;
/* The same for one pair from host arrays: matches12[kf1->n], *nmatches. */
int orbg_search_for_triangulation(orbg_ctx *ctx, const orbg_keyframe *kf1, const orbg_keyframe *kf2,
                                  const orbg_triangulation_pair *geo, int only_stereo,
                                  int check_ori, int32_t *matches12, int *nmatches);

/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:293-560) around that search: the
 * pair's geometry before it (ComputeF12, :690-707) and the triangulation of its matches after
 * it (:395-560).  A KeyFrame's pose and calibration as they read them: mTcw rows 0..2
 * (row-major 3x4), fx, fy, cx, cy, invfx, invfy, mb, mbf. */
typedef struct {
    float Tcw[12];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} orbg_kf_camera;
/* d_geo[p] = the orbg_triangulation_pair of KeyFrames d_kf1[p] (current) and d_kf2[p]
 * (neighbour), cameras d_cams[kf]: F12 = K1^-T [t12]x R12 K2^-1 in the reference's float
 * evaluation (A.inv()*B as solve(), K2.inv() closed form, gemms in double), pKF1's camera
 * centre, pKF2's pose and intrinsics.  Context stream. */
int orbg_triangulation_geometry_batch_device(orbg_ctx *ctx, const orbg_kf_camera *d_cams,
                                             const int32_t *d_kf1, const int32_t *d_kf2,
                                             int npairs, orbg_triangulation_pair *d_geo);
/* The same for one pair from host structs. */
int orbg_triangulation_geometry(orbg_ctx *ctx, const orbg_kf_camera *cam1,
                                const orbg_kf_camera *cam2, orbg_triangulation_pair *geo);
/* Per-match outcome of the triangulation, the reference's `continue`s in order: */
enum {
    ORBG_TRI_NONE = 0,      /* no match (matches12[i] < 0) */
    ORBG_TRI_NEW = 1,       /* a new MapPoint at x3d */
    ORBG_TRI_PARALLAX = -1, /* no stereo and too little parallax */
    ORBG_TRI_W0 = -2,       /* the homogeneous solution's w == 0 */
    ORBG_TRI_Z1 = -3,       /* behind pKF1 */
    ORBG_TRI_Z2 = -4,       /* behind pKF2 */
    ORBG_TRI_REPROJ1 = -5,  /* chi-square gate in pKF1 (5.991 mono / 7.8 stereo) */
    ORBG_TRI_REPROJ2 = -6,  /* ... in pKF2 */
    ORBG_TRI_DIST0 = -7,    /* at a camera centre */
    ORBG_TRI_SCALE = -8     /* scale inconsistency (ratioFactor = 1.5 mfScaleFactor) */
};
/* For pairs p (KeyFrames d_kf1[p], d_kf2[p] of `kfs`: mvKeysUn, mvuRight, counts read; mvKeys
 * d_kps_raw + kf * cap for UnprojectStereo (NULL: mvKeysUn), mvDepth d_depth + kf * cap
 * (read where mvuRight >= 0; required with uright), cameras d_cams[kf]) and their
 * SearchForTriangulation output d_matches12 + p * cap: d_status[p * cap + i] (ORBG_TRI_*)
 * and d_x3d[3 (p * cap + i) ..] (the new point when NEW, else 0) for i < N of pKF1,
 * d_nnew[p] = new points.  The MapPoint creation itself (new MapPoint, AddObservation,
 * ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mlpRecentAddedMapPoints) is the
 * caller's, in i order.  Scale factors / sigma^2 / mfScaleFactor are the
 * context's.  A match past pKF2's N counts as no match.  Context stream. */
int orbg_triangulate_batch_device(orbg_ctx *ctx, const orbg_keyframes *kfs,
                                  const orbg_keypoint *d_kps_raw, const float *d_depth, int cap,
                                  const orbg_kf_camera *d_cams, const int32_t *d_kf1,
                                  const int32_t *d_kf2, const int32_t *d_matches12, int npairs,
                                  float *d_x3d, int8_t *d_status, int32_t *d_nnew);
/* One KeyFrame's triangulation inputs from host arrays (kps_raw / uright may be NULL; depth
 * required with uright) */
typedef struct {
    const orbg_keypoint *kps;
    const orbg_keypoint *kps_raw;
    const float *uright;
    const float *depth;
    int32_t n;
} orbg_keyframe_geo;
/* One pair from host arrays: status[kf1->n], x3d[3 kf1->n], *nnew. */
int orbg_triangulate(orbg_ctx *ctx, const orbg_keyframe_geo *kf1, const orbg_keyframe_geo *kf2,
                     const orbg_kf_camera *cam1, const orbg_kf_camera *cam2,
                     const int32_t *matches12, float *x3d, int8_t *status, int *nnew);

/* ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:968-1107) splits into a search,
 * per MapPoint independent of the others (projection with pKF's pose, IsInImage, the
 * [0.8 dmin, 1.2 dmax] and 60-degree gates, PredictScale, GetFeaturesInArea(u, v, th *
 * mvScaleFactors[level]), the level window [level - 1, level], the chi-square reprojection
 * gates 5.99 / 7.8, the least descriptor distance -- the first in GetFeaturesInArea's order),
 * and the sequential map update of every point whose best distance is <= TH_LOW (Replace or
 * AddObservation, :1071-1104), which the caller applies in vpMapPoints order.
 * This is the search: best_idx[i] = the pKF feature the reference fuses point i with, -1 if
 * none; best_dist[i] = bestDist (256: no candidate).  mps[i].flags ORBG_MP_VALID = pMP &&
 * !isBad() && !IsInKeyFrame(pKF) when the call starts; cam = pKF's pose, fx.., mbf,
 * mfLogScaleFactor, mnScaleLevels and the Frame's (float) image bounds the KeyFrame's grid was
 * built with: the grid and its cell sizes use them, IsInImage and GetFeaturesInArea's cell
 * range the KeyFrame's int mnMinX .. mnMaxY, their truncation (KeyFrame.h:288-291,
 * KeyFrame.cc:51).  Scale factors / inverse sigma^2 are the context's.  One KeyFrame from host
 * arrays (kf->fv_* unused): */
int orbg_fuse(orbg_ctx *ctx, const orbg_keyframe *kf, const orbg_frustum_camera *cam,
              const orbg_map_point *mps, const uint8_t *mdesc, int nmp, float th,
              int32_t *best_idx, int32_t *best_dist, int *nfused);
/* Batched, device memory: pair p = KeyFrame d_kf[p] of `kfs` (desc, kps, uright, counts
 * read) with camera d_cams[p] and the d_mcounts[p] MapPoints at d_mps + p * mcap (descriptors
 * d_mdesc + p * mcap * 32); outputs at + p * mcap, d_nfused[p] = points with a target
 * (written even when mcap == 0: zero).  Context stream.  ORBG_ENOTSUP past 8192 keypoints per
 * KeyFrame (the grid lives in LDS). */
int orbg_fuse_batch_device(orbg_ctx *ctx, const orbg_keyframes *kfs, int cap, const int32_t *d_kf,
                           const orbg_frustum_camera *d_cams, const orbg_map_point *d_mps,
                           const uint8_t *d_mdesc, const int32_t *d_mcounts, int mcap, int npairs,
                           float th, int32_t *d_best_idx, int32_t *d_best_dist,
                           int32_t *d_nfused);
/* ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1133-1258;
 * caller LoopClosing::SearchAndFuse, LoopClosing.cc:944-980, th 4): the same split.  cam->Tcw
 * holds Scw's rows 0..2 (s*Rcw | s*tcw, Converter::toCvMat of the corrected g2o::Sim3); the
 * kernel decomposes it as the reference does (scw = sqrt of row 0's double dot product, Rcw |
 * tcw = Scw / scw with the float alpha 1 / scw, :1143-1148; Ow = -Rcw^T tcw), then projects
 * and gates exactly as orbg_fuse but ranks the candidates by descriptor distance alone (no
 * reprojection gate; kf->uright and cam->bf unused).  mps[i].flags ORBG_MP_VALID = !isBad() &&
 * not in pKF->GetMapPoints() at the call's start.  Outputs as orbg_fuse; the caller then
 * walks vpPoints in order: best_idx[i] >= 0 -> pKF's MapPoint at best_idx[i], if any and not
 * bad, becomes vpReplacePoint[i], else AddObservation / AddMapPoint (:1239-1254). */
int orbg_fuse_sim3(orbg_ctx *ctx, const orbg_keyframe *kf, const orbg_frustum_camera *cam,
                   const orbg_map_point *mps, const uint8_t *mdesc, int nmp, float th,
                   int32_t *best_idx, int32_t *best_dist, int *nfused);
/* Batched, device memory, as orbg_fuse_batch_device (kfs->uright may be NULL). */
int orbg_fuse_sim3_batch_device(orbg_ctx *ctx, const orbg_keyframes *kfs, int cap,
                                const int32_t *d_kf, const orbg_frustum_camera *d_cams,
                                const orbg_map_point *d_mps, const uint8_t *d_mdesc,
                                const int32_t *d_mcounts, int mcap, int npairs, float th,
                                int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_nfused);

/* ORBmatcher(0.75, checkOri).SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
 * ORBdist) (src/ORBmatcher.cc:1670-1798; Tracking::Relocalization, Tracking.cc:2120 th 10 /
 * ORBdist 100, :2141 th 3 / 64): the CurrentFrame side is kps / desc (mvKeysUn,
 * mDescriptors), taken0[i2] = mvpMapPoints[i2] != NULL on entry (NULL: none), cam =
 * CurrentFrame's pose, fx.., mfLogScaleFactor, mnScaleLevels and mnMinX..; pts[i] =
 * pKF->GetMapPointMatches()[i] with pKF->mvKeysUn[i].angle (flags ORBG_MP_VALID = pMP &&
 * !isBad() && !sAlreadyFound.count(pMP)).  match[i2] = the pKF index written to
 * mvpMapPoints[i2], -1 untouched, -2 set to NULL by the rotation filter. */
typedef struct {
    float x, y, z;            /* GetWorldPos() */
    float min_dist, max_dist; /* mfMinDistance, mfMaxDistance */
    float angle;              /* pKF->mvKeysUn[i].angle */
    int32_t flags;
} orbg_reloc_point;
int orbg_search_by_projection_reloc(orbg_ctx *ctx, const orbg_keypoint *kps, const uint8_t *desc,
                                    int n, const uint8_t *taken0, const orbg_frustum_camera *cam,
                                    const orbg_reloc_point *pts, const uint8_t *pdesc, int np,
                                    float th, int orb_dist, int check_ori, int32_t *match,
                                    int *nmatches);
/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:
 * 353-470; LoopClosing::ComputeSim3, LoopClosing.cc:669, th 10): kps / desc = pKF's,
 * taken0[idx] = vpMatched[idx] != NULL on entry, cam->Tcw = Scw rows 0..2 (decomposed on the
 * device as orbg_fuse_sim3 does), cam->bounds the Frame's float bounds (the KeyFrame's int
 * bounds are their truncation); mps[i] = vpPoints[i] (flags ORBG_MP_VALID = !isBad() && not
 * in vpMatched on entry).  match[idx] = the vpPoints index written to vpMatched[idx], -1. */
int orbg_search_by_projection_sim3(orbg_ctx *ctx, const orbg_keypoint *kps, const uint8_t *desc,
                                   int n, const uint8_t *taken0, const orbg_frustum_camera *cam,
                                   const orbg_map_point *mps, const uint8_t *mdesc, int nm,
                                   int th, int32_t *match, int *nmatches);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:
 * 1262-1470; LoopClosing::ComputeSim3, LoopClosing.cc:594, th 7.5): pKF1's map points
 * projected into pKF2 through the Sim3 and pKF2's into pKF1, each to its least-distance
 * feature (TH_HIGH), kept where the two directions agree.  kf1 / kf2: mvKeysUn, mDescriptors,
 * n (the rest unused); mp1[i] / md1 = pKF1->GetMapPointMatches()[i] (flags ORBG_MP_VALID = pMP
 * && !isBad()), likewise mp2 / md2; matched1[i] = vpMatches12[i] != NULL, matched2[idx2] = 1
 * for each such point's GetIndexInKeyFrame(pKF2) (NULL: none); g = the two poses, the Sim3,
 * pKF1's intrinsics (used both ways, as the reference does), mfLogScaleFactor,
 * mnScaleLevels and the Frame's float bounds.  matches12[i] = the pKF2 index whose MapPoint
 * becomes vpMatches12[i], -1 (slots already set keep theirs); *nfound = nFound. */
typedef struct {
    float T1w[12], T2w[12];      /* pKF1 / pKF2 GetPose() rows 0..2 */
    float R12[9], t12[3], s12;   /* the Sim3 (R12 row-major) */
    float fx, fy, cx, cy;        /* pKF1->fx .. */
    float log_scale_factor;
    int32_t nlevels;
    orbg_bounds bounds;
} orbg_sim3_pair;
int orbg_search_by_sim3(orbg_ctx *ctx, const orbg_keyframe *kf1, const orbg_map_point *mp1,
                        const uint8_t *md1, const uint8_t *matched1, const orbg_keyframe *kf2,
                        const orbg_map_point *mp2, const uint8_t *md2, const uint8_t *matched2,
                        const orbg_sim3_pair *g, float th, int32_t *matches12, int *nfound);
/* Batched, device memory: pair p = KeyFrames d_kf1[p], d_kf2[p] of `kfs` (desc, kps, counts
 * read) with d_pairs[p]; map points per KeyFrame slot at d_mps + kf * cap (descriptors
 * d_mdesc + (kf * cap) * 32); d_matched1 / d_matched2 [npairs][cap] or NULL; outputs
 * d_matches12 + p * cap, d_nfound[p].  Context stream; ORBG_ENOTSUP past 8192 keypoints. */
int orbg_search_by_sim3_batch_device(orbg_ctx *ctx, const orbg_keyframes *kfs, int cap,
                                     const int32_t *d_kf1, const int32_t *d_kf2,
                                     const orbg_sim3_pair *d_pairs, const orbg_map_point *d_mps,
                                     const uint8_t *d_mdesc, const uint8_t *d_matched1,
                                     const uint8_t *d_matched2, int npairs, float th,
                                     int32_t *d_matches12, int32_t *d_nfound);

/* ---------------- Optimizer::PoseOptimization ----------------
 * One edge per Frame keypoint with a MapPoint (index order): EdgeSE3ProjectXYZOnlyPose when
 * mvuRight[i] < 0, else EdgeStereoSE3ProjectXYZOnlyPose (Optimizer.cc:381-460). */
typedef struct {
    float obs[3];      /* kpUn.pt.x, kpUn.pt.y, mvuRight[i] */
    float xw[3];       /* pMP->GetWorldPos() */
    float inv_sigma2;  /* mvInvLevelSigma2[kpUn.octave] */
    int32_t stereo;    /* mvuRight[i] >= 0 */
} orbg_pose_edge;

typedef struct {
    float fx, fy, cx, cy, bf; /* Frame::fx, fy, cx, cy, mbf */
    float pad;
} orbg_pose_camera;

/* Optimizer::PoseOptimization(pFrame): tcw_in = pFrame->mTcw rows 0..2 (row-major 3x4).
 * Outputs the optimised SE3Quat (q x,y,z,w; t), its cv::Mat form tcw_out (SetPose), the
 * mvbOutlier flag per edge and the return value (nInitialCorrespondences - nBad) in
 * *ninliers.  Fewer than 3 edges: pose unchanged, 0. */
int orbg_pose_optimization(orbg_ctx *ctx, const orbg_pose_edge *edges, int n,
                           const orbg_pose_camera *cam, const float tcw_in[12], double q_out[4],
                           double t_out[3], float tcw_out[12], uint8_t *outlier, int *ninliers);

/* Batched, device-resident: frame f's edges at edges + f * edge_cap, counts[f] of them;
 * cams[f], tcw_in[f * 12]; outputs q_out[f * 4], t_out[f * 3], tcw_out[f * 12],
 * outlier[f * edge_cap], ninliers[f].  One workgroup per frame, on the context stream. */
int orbg_pose_optimization_batch_device(orbg_ctx *ctx, const orbg_pose_edge *edges,
                                        const int32_t *counts, int edge_cap,
                                        const orbg_pose_camera *cams, const float *tcw_in,
                                        double *q_out, double *t_out, float *tcw_out,
                                        uint8_t *outlier, int32_t *ninliers, int nframes);

/* The per-frame pose of the batched-sequence mode (SURVEY.md 8e "pose/trajectory stub"):
 * Optimizer::PoseOptimization (src/Optimizer.cc:356-631) of frame f2[p] of every pair of the
 * last orbg_match_batch_device, with that call's SearchForInitialization matches as the map
 * points: F1 keypoint i matched to F2 keypoint j gives one mono edge, obs = F2 keypoint j,
 * Xw = F1 keypoint i back-projected at `depth` in F1's camera ((x - cx) z / fx,
 * (y - cy) z / fy, z), Omega = mvInvLevelSigma2[octave of j]; edges in F2 index order (the
 * reference's loop over pFrame's keypoints); initial pose identity (F1's camera = world).
 * Outputs per pair on the match stream (device memory): d_q[4p..4p+3] the SE3Quat rotation
 * (x, y, z, w), d_t[3p..3p+2] its translation (F2's pose relative to F1) and d_ninliers[p]
 * (PoseOptimization's return value). */
int orbg_match_pose_batch_device(orbg_ctx *ctx, const orbg_pose_camera *cam, float depth,
                                 double *d_q, double *d_t, int32_t *d_ninliers);

/* ---------------- local BA linearisation ---------------- */
typedef struct {
    double q[4]; /* SE3Quat rotation, Eigen coeffs order (x, y, z, w), normalised */
    double t[3];
    int32_t fixed;
    int32_t pad;
} orbg_pose;

typedef struct {
    int32_t point;   /* vertex 0: VertexSBAPointXYZ */
    int32_t pose;    /* vertex 1: VertexSE3Expmap */
    int32_t stereo;  /* 0 EdgeSE3ProjectXYZ, 1 EdgeStereoSE3ProjectXYZ */
    int32_t robust;  /* Huber kernel attached */
    int32_t active;  /* level-0 edge */
    int32_t pad;
    double obs[3];
    double inv_sigma2;
    double fx, fy, cx, cy, bf;
    double huber_delta;
} orbg_edge;

typedef struct {
    double err[3];
    double chi2;
    double rho1;
    double jp[3][3];
    double jt[3][6];
    double hpl[3][6];
} orbg_edge_out;

/* Host arrays in, host arrays out (uploads, runs the device kernels, downloads).
 * eout may be NULL.  hpose npose*36, bpose npose*6, hpoint npoint*9, bpoint npoint*3. */
int orbg_ba_linearize(orbg_ctx *ctx, const orbg_pose *poses, int npose, const double *points,
                      int npoint, const orbg_edge *edges, int nedge, orbg_edge_out *eout,
                      double *hpose, double *bpose, double *hpoint, double *bpoint);

/* Device-resident variant (batched LBA windows): every pointer is device memory, enqueued
 * on the context stream.  pose_off[npose+1] / pose_edges[nedge] and point_off[npoint+1] /
 * point_edges[nedge] list each vertex's edges (CSR, built once per window: the graph does
 * not change across LM iterations; a point's edges in ascending edge order).  d_eout is
 * required; its hpl (and, per orbg_ba_set_edge_errors / _jacobians, the error terms and
 * Jacobians) are overwritten.  Point blocks are summed per point by one thread per point
 * over its edges; pose blocks H_pp | b_p are accumulated with MFMA f64. */
int orbg_ba_linearize_device(orbg_ctx *ctx, const orbg_pose *d_poses, int npose,
                             const double *d_points, int npoint, const orbg_edge *d_edges,
                             int nedge, const int32_t *d_pose_off, const int32_t *d_pose_edges,
                             const int32_t *d_point_off, const int32_t *d_point_edges,
                             orbg_edge_out *d_eout, double *d_hpose, double *d_bpose,
                             double *d_hpoint, double *d_bpoint);

/* buildSystem alone, for an LM iteration kept in HBM: as orbg_ba_linearize_device, but
 * H_pl goes to d_hpl[18e .. 18e+17] (edge e's 3x6 block, row-major, the _Hpl block
 * constructQuadraticForm adds, base_binary_edge.hpp:105-117) instead of the 400-byte
 * orbg_edge_out records, and no per-edge Jacobian or error term is stored (the LM's error
 * pass, orbg_ba_errors_device, provides them): per edge 144 bytes out instead of a strided
 * record.  Same blocks and the same H_pl bits as orbg_ba_linearize_device. */
int orbg_ba_build_system_device(orbg_ctx *ctx, const orbg_pose *d_poses, int npose,
                                const double *d_points, int npoint, const orbg_edge *d_edges,
                                int nedge, const int32_t *d_pose_off, const int32_t *d_pose_edges,
                                const int32_t *d_point_off, const int32_t *d_point_edges,
                                double *d_hpl, double *d_hpose, double *d_bpose,
                                double *d_hpoint, double *d_bpoint);

/* A device-resident LBA graph: the edge set of g2o's SparseOptimizer for one or many windows
 * (Optimizer.cc:662-851 builds it; optimize(5), the outlier pass and optimize(10) at
 * :857-905 rebuild the system over it every LM iteration).  Created once from host edges,
 * kept in HBM packed: 24 bytes per edge (vertices, type / robust / active flags, f32
 * observations) plus deduplicated camera and (inv_sigma2, huber_delta) tables and the
 * per-vertex edge lists, so an iteration reads a quarter of orbg_edge's bytes.  ORB-SLAM2's
 * observations are cv::KeyPoint floats: a graph needs every observation f32-exact (the mono
 * third entry is ignored), at most 256 distinct (fx, fy, cx, cy, bf) and 65536 distinct
 * (inv_sigma2, huber_delta); otherwise ORBG_ENOTSUP, and the record entry points apply.
 * Per-edge outputs (H_pl, errors) are bit-identical to orbg_ba_build_system_device /
 * orbg_ba_errors_device on the same edges.  Block sums are deterministic here: every point
 * block is summed over its edges in edge order (a point whose edges straddle two 256-edge
 * workgroups is summed by a follow-up pass, no atomics), the oracle's order; a pose block is
 * the sum over its 64-edge slices in slice order (each slice an MFMA f64 accumulation).  The
 * record entry points sum a straddling point as two partials and pose slices by fp64
 * atomics, so those blocks agree with the graph's to rounding, not bit for bit.  The graph
 * keeps its slice tables, special-point list and pose partials (built once), so a build is
 * four launches (edges, special points, pose slices, pose reduction) with no zero fills.  A graph belongs to the device of the context that
 * created it. */
typedef struct orbg_ba_graph orbg_ba_graph;
int orbg_ba_graph_create(orbg_ctx *ctx, const orbg_edge *edges, int nedge, int npose,
                         int npoint, orbg_ba_graph **out);
int orbg_ba_graph_destroy(orbg_ba_graph *graph);
/* setLevel(1) / setLevel(0) of the outlier pass (Optimizer.cc:871-901): active[e] (host,
 * 0 or 1) for every edge, in the order given at creation; ordered on the context stream
 * (uploaded from pinned staging: no host synchronisation beyond waiting for the previous
 * call's upload). */
int orbg_ba_graph_set_active(orbg_ctx *ctx, orbg_ba_graph *graph, const uint8_t *active);
/* e->setRobustKernel(0) / the Huber kernel per edge (Optimizer.cc:884, :900 remove it from
 * every edge after the outlier pass): robust[e] (host, 0 or 1), ordered like set_active. */
int orbg_ba_graph_set_robust(orbg_ctx *ctx, orbg_ba_graph *graph, const uint8_t *robust);
/* buildSystem over the graph: outputs as orbg_ba_build_system_device (d_hpl [nedge][3][6]). */
int orbg_ba_graph_build_system(orbg_ctx *ctx, orbg_ba_graph *graph, const orbg_pose *d_poses,
                               const double *d_points, double *d_hpl, double *d_hpose,
                               double *d_bpose, double *d_hpoint, double *d_bpoint);
/* computeActiveErrors over the graph: outputs as orbg_ba_errors_device. */
int orbg_ba_graph_errors(orbg_ctx *ctx, orbg_ba_graph *graph, const orbg_pose *d_poses,
                         const double *d_points, double *d_err, double *d_chi2, double *d_rho0,
                         uint8_t *d_depth_ok);
/* g2o's BlockSolver<6,3>::solve over an orbg_ba_graph, device-resident (Thirdparty/g2o/g2o/
 * core/block_solver.hpp:354-486 after setLambda, optimization_algorithm_levenberg.cpp:61-164):
 * orbg_ba_graph_schur_plan builds the Schur structure once -- free poses (`fixed`: host
 * [npose], g2o's vertex->fixed(), Optimizer.cc:714,729), the pose-pair lists of every shared
 * landmark in landmark order, the independent dense systems (one per LBA window of the
 * graph) -- and uploads it; orbg_ba_graph_set_active rebuilds it for the new active set.
 * orbg_ba_graph_schur_solve then reads the graph build's device blocks (d_hpl [nedge][3][6],
 * H_pp / b_p, H_ll / b_l) and writes the increments d_dx_pose [npose][6] (0 for fixed poses),
 * d_dx_point [npoint][3] and *d_ok (0: a zero / non-finite LDLT pivot, increments 0), in
 * stream order on the context stream with no host copy: build -> errors -> solve -> update
 * is one stream.  The Schur products run on v_mfma_f64_4x4x4f64; every sum in the order
 * oracle/ba_oracle.c orc_ba_schur_solve pins (bit-identical). */
int orbg_ba_graph_schur_plan(orbg_ctx *ctx, orbg_ba_graph *graph, const uint8_t *fixed);
int orbg_ba_graph_schur_solve(orbg_ctx *ctx, orbg_ba_graph *graph, double lambda,
                              const double *d_hpl, const double *d_hpose, const double *d_bpose,
                              const double *d_hpoint, const double *d_bpoint, double *d_dx_pose,
                              double *d_dx_point, int32_t *d_ok);
/* SparseOptimizer::update for LocalBundleAdjustment's vertex types (device memory, context
 * stream): VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:73-76: estimate =
 * SE3Quat::exp(dx) * estimate, se3quat.h:223-257; poses with `fixed` set are copied
 * unchanged) and VertexSBAPointXYZ::oplusImpl (estimate += dx).  In place when the outputs
 * are the inputs. */
int orbg_ba_update_device(orbg_ctx *ctx, const orbg_pose *d_poses, int npose,
                          const double *d_points, int npoint, const double *d_dx_pose,
                          const double *d_dx_point, orbg_pose *d_poses_out, double *d_points_out);
/* optimizer.optimize(iterations) of LocalBundleAdjustment (Optimizer.cc:857, :905) on an
 * orbg_ba_graph, OptimizationAlgorithmLevenberg::solve per iteration
 * (optimization_algorithm_levenberg.cpp:61-164: tau 1e-5, goodStep scales 1/3 and 2/3, 10
 * trials after failure, the (iniChi - chi) * 1e3 < iniChi three-strikes stop): build ->
 * Schur solve -> update -> error pass -> accept or pop, all on the context stream over the
 * estimates in HBM (d_poses / d_points, updated in place); the host reads the trial's three
 * scalars (activeRobustChi2, computeScale, the solver's ok) once per trial.  The scalars
 * are deterministic device reductions (a fixed grid-stride + tree order; g2o sums
 * sequentially).  orbg_ba_graph_schur_plan must have been called (it holds the fixed poses;
 * `fixed` of d_poses must agree); the active edges are the graph's (orbg_ba_graph_set_active).
 * report (may be NULL): iterations run, trials, chi2 before / after, the final lambda, and
 * terminated = 1 (rho == 0 or 10 failed trials) or 2 (three iterations without a 1e-3
 * relative decrease), 0 if every iteration ran. */
typedef struct {
    int32_t iterations, trials, terminated, pad;
    double initial_chi2, final_chi2, lambda;
} orbg_lm_report;
int orbg_ba_graph_optimize(orbg_ctx *ctx, orbg_ba_graph *graph, orbg_pose *d_poses,
                           double *d_points, int iterations, orbg_lm_report *report);

/* orbg_ba_graph_optimize with g2o's force-stop flag and iteration actions
 * (SparseOptimizer::setForceStopFlag(bool*), sparse_optimizer.h:184-188, installed by
 * LocalBundleAdjustment at Optimizer.cc:700-701 and raised by LocalMapping when Tracking
 * inserts a key frame; SparseOptimizer::addPostIterationAction).  Every member may be NULL:
 *   force_stop      the caller's bool (1 byte, read volatile from the host), polled where
 *                   g2o polls terminate(): before every iteration (sparse_optimizer.cpp:376)
 *                   and after every LM trial (optimization_algorithm_levenberg.cpp:149); a
 *                   raised flag ends the call after the current trial with the estimates of
 *                   that point (an accepted trial's, or the pushed state after a rejected one),
 *                   report->terminated = 3 unless the LM itself terminated;
 *   post_iteration  called after each iteration (postIteration(i), sparse_optimizer.cpp:413,
 *                   the terminating one included), on the calling thread;
 *   post_trial      called after each trial's accept / reject (before the flag is polled);
 *   d_last_chi2     device [nedge]: every edge's chi2 from the last error pass the call ran --
 *                   what g2o's edges hold after optimize() (the last trial's _error, accepted or
 *                   not; LocalBundleAdjustment's outlier tests read it, Optimizer.cc:879-901).
 *                   Not written if no iteration ran (g2o computes no error then either).
 * The hooks run on the calling thread between trials (device work may still be queued). */
typedef struct {
    const volatile uint8_t *force_stop;
    void (*post_iteration)(void *user, int iteration);
    void (*post_trial)(void *user, int iteration, int trial);
    void *user;
    double *d_last_chi2;
} orbg_lm_control;
int orbg_ba_graph_optimize_ctl(orbg_ctx *ctx, orbg_ba_graph *graph, orbg_pose *d_poses,
                               double *d_points, int iterations, const orbg_lm_control *control,
                               orbg_lm_report *report);

/* The optimisation of Optimizer::LocalBundleAdjustment (Optimizer.cc:853-935) on one window,
 * host arrays in and out, everything between on the device (the window's graph, estimates and
 * LM in HBM):
 *   optimize(5) (:856-857) with the force-stop flag (:700-701);
 *   bDoMore = the flag is clear (:859-864);
 *   if bDoMore, the outlier pass (:868-901): for every edge whose map point is not bad,
 *     setLevel(1) if chi2 > 5.991 (mono) / 7.815 (stereo) or !isDepthPositive, and
 *     setRobustKernel(0) -- chi2 as g2o's edges hold it (the last error pass of optimize(5),
 *     orbg_lm_control.d_last_chi2), the depth test at the current estimates; then
 *     optimize(10) over the level-0 edges (:904-905);
 *   the vToErase test (:907-937): erase[e] = 1 for an edge whose map point is not bad with
 *     chi2 > threshold or !isDepthPositive -- chi2 again as g2o holds it: the last error pass
 *     of optimize(10) for its active edges, optimize(5)'s for the edges it did not optimise
 *     (g2o's computeActiveErrors skips level-1 edges), the depth test at the final estimates.
 * poses [npose] / points [npoint][3] (host) are the window (build_lba_window's order) and are
 * overwritten with the optimised estimates (Optimizer.cc:949-978 reads them).  edges as
 * orbg_ba_graph_create (active / robust as given: the reference starts with every edge at
 * level 0 with a Huber kernel).  control (NULL: none): force_stop is the caller's bool* (the
 * pbStopFlag both optimize calls poll), post_iteration / post_trial run in both optimize calls
 * (iterations counted from 0 in each), d_last_chi2 is ignored.  point_is_bad
 * (NULL: never): pMP->isBad(), called on the calling thread at the two places the reference
 * calls it (the outlier pass, the vToErase test).  erase [nedge] (host, required).  The caller
 * checks the flag before calling (Optimizer.cc:853-855 returns without any write-back); a flag
 * raised before optimize(5)'s first iteration leaves chi2 at the initial estimates' (g2o has
 * none: its _error is uninitialised then). */
typedef struct {
    orbg_lm_report lm[2];  /* optimize(5), optimize(10) (zeros when not run) */
    int32_t do_more;       /* bDoMore: the outlier pass and optimize(10) ran */
    int32_t n_outliers;    /* edges the outlier pass set to level 1 */
    int32_t n_erase;       /* edges with erase[e] = 1 */
    int32_t pad;
} orbg_lba_report;
int orbg_local_ba_optimize(orbg_ctx *ctx, orbg_pose *poses, int npose, double *points,
                           int npoint, const orbg_edge *edges, int nedge,
                           const orbg_lm_control *control,
                           int (*point_is_bad)(void *user, int point), void *user,
                           uint8_t *erase, orbg_lba_report *report);

/* g2o's per-trial error pass for the two LBA edge types: SparseOptimizer::
 * computeActiveErrors (Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:61-76, computeError
 * types_six_dof_expmap.h:90-95, 122-127) and the terms activeRobustChi2 sums (:100-114,
 * RobustKernelHuber::robustify robust_kernel_impl.cpp:78-91), plus isDepthPositive
 * (types_six_dof_expmap.h:97-101, 129-133) for LocalBundleAdjustment's outlier test
 * (Optimizer.cc:871-901).  The LM calls this after every trial update, buildSystem
 * (orbg_ba_linearize) once per iteration.  For every edge given, active or not:
 *   err[3e .. 3e+2] the error (third entry 0 for mono; NULL: not stored),
 *   chi2[e] = e^T Omega e, rho0[e] = Huber rho[0](chi2) if edges[e].robust else chi2 (NULL:
 *   not stored), depth_ok[e] = camera-frame depth > 0 (NULL: not stored);
 * *active_robust_chi2 (NULL: not computed) = the sum of rho0 over the active edges in the
 * order given (pass them in g2o's _activeEdges order).  Host arrays. */
int orbg_ba_errors(orbg_ctx *ctx, const orbg_pose *poses, int npose, const double *points,
                   int npoint, const orbg_edge *edges, int nedge, double *err, double *chi2,
                   double *rho0, uint8_t *depth_ok, double *active_robust_chi2);
/* Device-resident form (no sum): every pointer device memory, enqueued on the context
 * stream; d_chi2 required, d_err / d_rho0 / d_depth_ok may be NULL. */
int orbg_ba_errors_device(orbg_ctx *ctx, const orbg_pose *d_poses, const double *d_points,
                          const orbg_edge *d_edges, int nedge, double *d_err, double *d_chi2,
                          double *d_rho0, uint8_t *d_depth_ok);

/* Whether orbg_ba_linearize_device stores the per-edge Jacobians eout.jp / eout.jt (g2o's
 * _jacobianOplusXi / Xj; default on).  Off, those fields are left as they are and every
 * other output is unchanged: the blocks, H_pl and orbg_ba_schur_solve do not read them. */
int orbg_ba_set_jacobians(orbg_ctx *ctx, int enable);
/* Whether orbg_ba_linearize_device stores the per-edge error terms eout.err / chi2 / rho1
 * (default on).  Off, they are left as they are and every other output is unchanged: g2o's
 * LM takes them from the per-trial error pass instead (orbg_ba_errors / _device, which the
 * outlier test of Optimizer.cc:871-901 reads too), so buildSystem's pass writes only H_pl
 * and the blocks. */
int orbg_ba_set_edge_errors(orbg_ctx *ctx, int enable);

/* g2o BlockSolver<6,3>::solve with the Schur complement (Thirdparty/g2o/g2o/core/
 * block_solver.hpp:354-486) for one LocalBundleAdjustment window, after setLambda(lambda):
 * inputs are orbg_ba_linearize's outputs (eout[e].hpl = H_pl^T of edge e) for the same
 * poses / edges; only active edges and non-fixed poses take part.  dx_pose[npose*6] (0 for
 * fixed poses), dx_point[npoint*3] (0 for points without an active edge); *ok = the linear
 * solver's success (0: increments are zero). */
int orbg_ba_schur_solve(orbg_ctx *ctx, const orbg_pose *poses, int npose, int npoint,
                        const orbg_edge *edges, int nedge, const orbg_edge_out *eout,
                        const double *hpose, const double *bpose, const double *hpoint,
                        const double *bpoint, double lambda, double *dx_pose, double *dx_point,
                        int *ok);

/* ---------------- DBoW2 vocabulary + transform (Frame::ComputeBoW) ---------------- */
/* WeightingType / ScoringType of Thirdparty/DBoW2/DBoW2/BowVector.h:36-53 */
#define ORBG_TF_IDF 0
#define ORBG_TF 1
#define ORBG_IDF 2
#define ORBG_BINARY 3
#define ORBG_L1_NORM 0
#define ORBG_L2_NORM 1
#define ORBG_CHI_SQUARE 2
#define ORBG_KL 3
#define ORBG_BHATTACHARYYA 4
#define ORBG_DOT_PRODUCT 5

typedef struct orbg_vocab orbg_vocab;   /* device-resident vocabulary tree (one GPU) */

/* The tree exactly as loadFromTextFile builds it: node 0 is the root, nodes 1..nnodes-1 in
 * file order with parent[i] < i; children of a node in node order; is_leaf[i] > 0 gives the
 * node the next word id (leaves numbered in node order).  desc[nnodes][32], weight[nnodes]
 * (the idf of a word; ignored for the root).  k, L, scoring, weighting as in the header line
 * (0 <= k <= 20, 1 <= L <= 10, scoring 0..5, weighting 0..3).  Uploads to ctx's device. */
int orbg_vocab_create(orbg_ctx *ctx, int k, int L, int scoring, int weighting, int nnodes,
                      const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                      const double *weight, orbg_vocab **out);
/* Parses the ORBvoc.txt text format ("k L scoring weighting", then one "parent isLeaf d0..d31
 * weight" line per node).  Blank lines are skipped (the reference appends an uninitialised
 * stopped node under the root for a trailing newline).  ORBG_EINVAL on a
 * malformed file. */
int orbg_vocab_load_text(orbg_ctx *ctx, const char *path, orbg_vocab **out);
void orbg_vocab_destroy(orbg_vocab *v);
/* k, L, scoring, weighting, nnodes, nwords (any pointer may be NULL) */
int orbg_vocab_info(const orbg_vocab *v, int32_t *k, int32_t *L, int32_t *scoring,
                    int32_t *weighting, int32_t *nnodes, int32_t *nwords);

/* transform(descriptors, mBowVec, mFeatVec, levelsup) for n descriptors (n x 32 bytes, host):
 *   BowVector: bow_words[*nbow] ascending word ids, bow_weights[*nbow] (normalised per the
 *   scoring), FeatureVector: fv_nodes[*nfv] ascending node ids, feature indices
 *   fv_feats[fv_off[j] .. fv_off[j+1]) ascending.  Capacities: n for bow_*, fv_nodes, fv_feats;
 *   n + 1 for fv_off.  Bit-identical to the reference (doubles included). */
int orbg_bow_transform(orbg_ctx *ctx, const orbg_vocab *v, const uint8_t *desc, int n,
                       int levelsup, int32_t *bow_words, double *bow_weights, int *nbow,
                       int32_t *fv_nodes, int32_t *fv_off, int32_t *fv_feats, int *nfv);

/* Batched, device-resident: frame f's descriptors at desc + f * cap * 32, counts[f] of them
 * (cap <= 8192); outputs per frame at bow_words / bow_weights / fv_nodes / fv_feats + f * cap,
 * fv_off + f * (cap + 1), nbow[f], nfv[f].  Also word_of[f * cap + i] (word id of feature i,
 * -1 if stopped) and node_of[...] (its levelsup node) when non-NULL. */
int orbg_bow_transform_batch_device(orbg_ctx *ctx, const orbg_vocab *v, const uint8_t *desc,
                                    const int32_t *counts, int cap, int nframes, int levelsup,
                                    int32_t *bow_words, double *bow_weights, int32_t *nbow,
                                    int32_t *fv_nodes, int32_t *fv_off, int32_t *fv_feats,
                                    int32_t *nfv, int32_t *word_of, int32_t *node_of);

/* ---------------- place recognition: BoW score + KeyFrameDatabase ---------------- */
/* A set of BowVectors in device memory, in orbg_bow_transform_batch_device's output layout:
 * vector f's rows at words / weights + f * cap (ascending word ids), nbow[f] entries. */
typedef struct {
    const int32_t *words;
    const double *weights;
    const int32_t *nbow;
} orbg_bow_vectors;

/* TemplatedVocabulary::score(v1, v2) (TemplatedVocabulary.h:1192-1196) = L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), host arrays (ascending word ids).  Only
 * ORBG_L1_NORM vocabularies (ORBvoc.txt's "10 6 0 0"; ORB-SLAM2 uses no other): any other
 * scoring returns ORBG_ENOTSUP.  *score is the reference's double bit for bit: the terms
 * fabs(vi - wi) - fabs(vi) - fabs(wi) of the common words summed in ascending word order, then
 * -score / 2.0, so two vectors without a common word give -0.0 as the reference does. */
int orbg_bow_score(orbg_ctx *ctx, const orbg_vocab *v, const int32_t *words1,
                   const double *weights1, int n1, const int32_t *words2, const double *weights2,
                   int n2, double *score);
/* Batched, device memory, on the context stream: d_score[p] = score(vector d_a_index[p] of a,
 * vector d_b_index[p] of b) for p < npairs (both sets with `cap` rows per vector, cap <= 8192;
 * a NULL index array means vector p).  The host form runs the same kernel. */
int orbg_bow_score_batch_device(orbg_ctx *ctx, const orbg_vocab *v, const orbg_bow_vectors *a,
                                const orbg_bow_vectors *b, int cap, const int32_t *d_a_index,
                                const int32_t *d_b_index, int npairs, double *d_score);

/* KeyFrameDatabase (src/KeyFrameDatabase.cc), device-resident, on ctx's device.  A KeyFrame
 * is a slot in [0, max_keyframes): the caller's handle.  The database keeps each live slot's
 * BowVector (up to cap entries), its add-sequence number (every add takes the next value of
 * a monotonic counter; it is the KeyFrame's position in every inverted list: erase keeps the
 * relative order of the rest, a later add appends) and its mRelocScore (float).  The
 * reference leaves mRelocScore uninitialised (KeyFrame.cc:39-40); here add pins it to 0.
 * Limits: max_keyframes <= 8192 (the per-slot counters and scores of a query live in LDS:
 * 14 bytes per slot + 4 per query word <= 144 KiB of the CU's 160; larger: ORBG_ENOTSUP),
 * cap <= 8192.  A vocabulary whose scoring is not ORBG_L1_NORM: ORBG_ENOTSUP.  All work runs
 * on the context stream. */
typedef struct orbg_kfdb orbg_kfdb;
int orbg_kfdb_create(orbg_ctx *ctx, const orbg_vocab *v, int max_keyframes, int cap,
                     orbg_kfdb **out);
void orbg_kfdb_destroy(orbg_kfdb *db);
/* live slots, max_keyframes, cap, and the largest max_keyframes orbg_kfdb_create accepts
 * (any pointer may be NULL).  Waits for the database's pending work. */
int orbg_kfdb_info(orbg_kfdb *db, int32_t *nlive, int32_t *max_keyframes, int32_t *cap,
                   int32_t *limit);
/* KeyFrameDatabase::add (:50-56), host arrays.  ORBG_EINVAL for a slot out of range or
 * already live, n > cap, word ids not strictly ascending or outside [0, nwords). */
int orbg_kfdb_add(orbg_ctx *ctx, orbg_kfdb *db, int slot, const int32_t *words,
                  const double *weights, int n);
/* add for i < n, in argument order: slot d_slots[i] <- vector d_index[i] (NULL: i) of `v`
 * (vcap rows per vector, vcap <= the database's cap), straight from a transform batch's
 * device outputs.  The validity of the slots (in range, not live, distinct) and of the
 * vectors is the caller's responsibility: an out-of-range slot is skipped, nothing else is
 * checked. */
int orbg_kfdb_add_batch_device(orbg_ctx *ctx, orbg_kfdb *db, const int32_t *d_slots,
                               const orbg_bow_vectors *v, int vcap, const int32_t *d_index,
                               int n);
/* KeyFrameDatabase::erase (:58-77; a slot that is not live: no effect) and clear (:79-83) */
int orbg_kfdb_erase(orbg_ctx *ctx, orbg_kfdb *db, int slot);
int orbg_kfdb_clear(orbg_ctx *ctx, orbg_kfdb *db);
/* The inverted file is rebuilt on the device by the first query after an add / erase /
 * clear; this does it now (no effect when it is current). */
int orbg_kfdb_rebuild(orbg_ctx *ctx, orbg_kfdb *db);
/* mRelocScore of every slot (reloc_score[max_keyframes], host; dead slots: unspecified) */
int orbg_kfdb_reloc_scores(orbg_ctx *ctx, orbg_kfdb *db, float *reloc_score);

/* KeyFrameDatabase::DetectRelocalizationCandidates (:291-419), batched: query i < nq is
 * vector d_qindex[i] (NULL: i) of `q` (qcap rows per vector, qcap <= 8192).  d_neigh
 * [max_keyframes][10]: row s = GetBestCovisibilityKeyFrames(10) of slot s as slots, -1 = unused,
 * a dead slot is skipped.  Outputs: d_cand[i * cand_cap ..] the candidates in the reference's
 * order (lKFsSharingWords' order: ascending (position in the query vector of the first shared
 * word, add-sequence number)), d_ncand[i] the full count (only the first cand_cap are
 * written), and when non-NULL d_max_common[i] = maxCommonWords, d_nscored[i] = nscores.
 * minCommonWords = (int)(maxCommonWords * 0.8f); KeyFrames with more common words are
 * scored (si = (float)score); the accumulation over the neighbours that share a word
 * (mnRelocQuery == F->mnId) adds in neighbour order, and a neighbour that this query did not
 * score contributes its stored mRelocScore, as in the reference; pBestKF by strict >,
 * minScoreToRetain = 0.75f * bestAccScore by strict >, duplicates dropped (first kept).
 * Every query of one call reads the stored mRelocScore as it was when the call started;
 * after the call a slot's stored value is the score from the highest-indexed query that
 * scored it.  With one query per call that is the reference's sequence. */
int orbg_kfdb_detect_reloc_batch_device(orbg_ctx *ctx, orbg_kfdb *db, const orbg_bow_vectors *q,
                                        int qcap, const int32_t *d_qindex, int nq,
                                        const int32_t *d_neigh, int32_t *d_cand, int cand_cap,
                                        int32_t *d_ncand, int32_t *d_max_common,
                                        int32_t *d_nscored);
/* One query from host arrays (neigh[max_keyframes][10], cand[cand_cap]; max_common / nscored
 * may be NULL) on the same kernels. */
int orbg_kfdb_detect_reloc(orbg_ctx *ctx, orbg_kfdb *db, const int32_t *words,
                           const double *weights, int n, const int32_t *neigh, int32_t *cand,
                           int cand_cap, int32_t *ncand, int32_t *max_common, int32_t *nscored);

/* KeyFrameDatabase::DetectLoopCandidates (:106-274), batched as above, plus d_conn
 * [nq][conn_cap] / d_nconn[nq] = the slots of pKF->GetConnectedKeyFrames() and d_min_score[nq].
 * Connected KeyFrames never enter lKFsSharingWords and never count as a neighbour (their
 * mnLoopQuery is never set); a KeyFrame is kept when si >= minScore; bestAccScore starts at
 * minScore; a neighbour counts only if it shares a word, is not connected and has more than
 * minCommonWords common words, so its score is this query's own (no stored state).  The query
 * KeyFrame's own slot, if live, is treated like any other unless listed as connected. */
int orbg_kfdb_detect_loop_batch_device(orbg_ctx *ctx, orbg_kfdb *db, const orbg_bow_vectors *q,
                                       int qcap, const int32_t *d_qindex, int nq,
                                       const int32_t *d_conn, int conn_cap,
                                       const int32_t *d_nconn, const float *d_min_score,
                                       const int32_t *d_neigh, int32_t *d_cand, int cand_cap,
                                       int32_t *d_ncand, int32_t *d_max_common,
                                       int32_t *d_nscored);
int orbg_kfdb_detect_loop(orbg_ctx *ctx, orbg_kfdb *db, const int32_t *words,
                          const double *weights, int n, const int32_t *conn, int nconn,
                          float min_score, const int32_t *neigh, int32_t *cand, int cand_cap,
                          int32_t *ncand, int32_t *max_common, int32_t *nscored);

/* ---------------- the covisibility Map: observations, UpdateConnections, the local map ------
 * The table "which keyframe slot observes which map point", device-resident on ctx's device,
 * and the reference functions that count, sort and gather over it: KeyFrame::UpdateConnections
 * (src/KeyFrame.cc:375-515, with AddConnection / EraseConnection / UpdateBestCovisibles),
 * Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (src/Tracking.cc:1731-1925) and
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:457-518).  A KeyFrame is a slot in
 * [0, max_keyframes) as in orbg_kfdb (the same limit, so the tables interchange); a MapPoint is
 * an id in [0, max_points).
 *
 * Pointer order is slot order.  The reference orders std::map<KeyFrame*, ...> and
 * std::set<KeyFrame*> by pointer value and breaks weight ties with sort(pair<int, KeyFrame*>),
 * so by pointer too: an order that differs between two runs of the reference itself.  Here
 * "ascending pointer" is ascending slot, everywhere (the one departure); a
 * host that allocates its KeyFrames from an arena in slot order gets the reference's behaviour
 * exactly.
 *
 * Observations are the inverse of the keyframe rows: point p is observed by (slot, idx) if and
 * only if the slot is live and its row holds p at idx.  A point id occurs at most once per row
 * (mObservations is a map keyed by KeyFrame): the caller's precondition, not checked.  The
 * caller uploads a KeyFrame's row once ProcessNewKeyFrame has associated it.  The point ->
 * observations index (CSR, each point's observations in ascending slot order) is rebuilt on the
 * device by the first query after a row changed.
 *
 * State per slot: live / bad / root (mnId == 0) flags, N, the point-id row (-1 = none), each
 * feature's mvKeysUn[idx].octave, GetCameraCenter(), the parent slot (-1 = none; the children
 * set is derived from the parents) and mbFirstConnection.  Per point: an orbg_map_point (the
 * position, normal, min / max distance; isBad() is the absence of ORBG_MP_VALID), mDescriptor
 * and the reference KeyFrame's slot.  Covisibility: a dense uint16 W[max_keyframes]
 * [max_keyframes] = mConnectedKeyFrameWeights (0 = not connected; 128 MiB at the limit, 8 MiB at
 * 2048), each slot's ordered list (mvpOrderedConnectedKeyFrames / mvOrderedWeights; stored,
 * because it is not a function of the W row: see orbg_map_update_connections_batch_device) and
 * its first ten entries neigh[max_keyframes][10], -1 padded.  Beside W the ordered lists take
 * 4 bytes per W entry and the observation index 12 bytes per row entry.
 * Limits: max_keyframes <= 8192 (the per-slot counters live in LDS as u32: 32 KiB), kf_cap <=
 * 8192; larger: ORBG_ENOTSUP.  All work runs on the context stream. */
typedef struct orbg_map orbg_map;
#define ORBG_MAP_KF_ROOT 1   /* mnId == 0: never gets a parent */
#define ORBG_MAP_KF_BAD 2    /* isBad() while its row still stands (SetBadFlag under way) */
int orbg_map_create(orbg_ctx *ctx, int max_keyframes, int kf_cap, int max_points, orbg_map **out);
void orbg_map_destroy(orbg_map *map);
/* live slots, max_keyframes, kf_cap, max_points (any pointer may be NULL).  Waits for the
 * map's pending work. */
int orbg_map_info(orbg_map *map, int32_t *nlive, int32_t *max_keyframes, int32_t *kf_cap,
                  int32_t *max_points);

/* Adds or overwrites slot `slot`: its n features' point ids (-1 = none) and octaves, the camera
 * centre (3 floats) and flags (ORBG_MAP_KF_*).  A slot that was not live starts without a
 * parent and with mbFirstConnection set; an overwrite keeps parent, mbFirstConnection, its W row
 * and its ordered list.  ORBG_EINVAL: slot out of range, n > kf_cap, an id >= max_points. */
int orbg_map_set_keyframe(orbg_ctx *ctx, orbg_map *map, int slot, const int32_t *point_ids,
                          const uint8_t *octaves, int n, const float *centre, int flags);
/* The same for i < n from device memory: slot d_slots[i] <- rows d_point_ids / d_octaves +
 * i * row_cap with d_counts[i] entries (clamped to row_cap and kf_cap), d_centres + 3 * i,
 * d_flags[i].  An out-of-range slot is skipped and an id >= max_points stored as -1; nothing
 * else is checked. */
int orbg_map_set_keyframes_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots, int n,
                                  const int32_t *d_point_ids, const uint8_t *d_octaves,
                                  int row_cap, const int32_t *d_counts, const float *d_centres,
                                  const int32_t *d_flags);
/* Records (flags: ORBG_MP_VALID = !isBad(); ORBG_MP_HAS_OBS is ignored, the table knows),
 * descriptors [n][32] and reference KeyFrame slots of points first .. first + n - 1. */
int orbg_map_set_points(orbg_ctx *ctx, orbg_map *map, int first, int n, const orbg_map_point *mps,
                        const uint8_t *desc, const int32_t *ref_kf);
/* The same from device memory for the ids d_ids[i] (NULL: first + i); an id out of range is
 * skipped. */
int orbg_map_set_points_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_ids, int first,
                               int n, const orbg_map_point *d_mps, const uint8_t *d_desc,
                               const int32_t *d_ref_kf);
/* the stored records of points first .. first + n - 1 (host; after UpdateNormalAndDepth) */
int orbg_map_get_points(orbg_ctx *ctx, orbg_map *map, int first, int n, orbg_map_point *mps);
/* SetBadFlag of a MapPoint as far as the table goes: clears ORBG_MP_VALID */
int orbg_map_set_point_bad(orbg_ctx *ctx, orbg_map *map, int id);
/* KeyFrame::ChangeParent (parent -1: none) */
int orbg_map_set_parent(orbg_ctx *ctx, orbg_map *map, int slot, int parent);
/* The table side of KeyFrame::SetBadFlag (:618-720): the slot becomes dead and bad, its row and
 * its W row are cleared, and in every row t with W[t][slot] > 0 the entry is zeroed and t's
 * ordered list re-sorted over all its non-zero weights (EraseConnection -> UpdateBestCovisibles).
 * The spanning-tree repair of :650-715 stays with the caller, through orbg_map_set_parent:
 * children of the slot keep it as their parent until then.  (orbg_map_set_bad_flag below is
 * SetBadFlag in full.) */
int orbg_map_erase_keyframe(orbg_ctx *ctx, orbg_map *map, int slot);
int orbg_map_clear(orbg_ctx *ctx, orbg_map *map);
/* The observation index and the children lists are rebuilt on the device by the first query
 * after a change; this does it now (no effect when they are current). */
int orbg_map_rebuild(orbg_ctx *ctx, orbg_map *map);

/* The device table neigh[max_keyframes][10] (GetBestCovisibilityKeyFrames(10) of every slot),
 * valid after the context stream's work: the d_neigh of the orbg_kfdb detect calls, unchanged. */
int orbg_map_neighbours(orbg_map *map, const int32_t **d_neigh);
/* a host copy of that table (neigh[max_keyframes][10]) */
int orbg_map_get_neighbours(orbg_ctx *ctx, orbg_map *map, int32_t *neigh);
/* GetConnectedKeyFrames() of slots d_slots[i], i < n: the non-zeros of the W row in ascending
 * slot order at d_conn + i * conn_cap, d_nconn[i] the full count (only the first conn_cap are
 * written): orbg_kfdb_detect_loop_batch_device's d_conn / d_nconn. */
int orbg_map_connected_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots, int n,
                              int32_t *d_conn, int conn_cap, int32_t *d_nconn);
/* A host read of slot's ordered list (GetVectorCovisibleKeyFrames / GetCovisiblesByWeight /
 * GetWeight in the essential-graph walk) and parent (may be NULL).  *n is the full length;
 * ORBG_ERANGE when it exceeds cap (the first cap entries are written). */
int orbg_map_get_connections(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *slots,
                             int32_t *weights, int cap, int32_t *n, int32_t *parent);
/* row `slot` of W (weights[max_keyframes], host) */
int orbg_map_get_weights(orbg_ctx *ctx, orbg_map *map, int slot, uint16_t *weights);

/* KeyFrame::UpdateConnections of the n distinct slots d_slots[i].  For slot s: KFcounter = for
 * every other live slot the number of s's good points it observes.  Empty: nothing changes for
 * s.  Else W[s][*] becomes the whole counter (weights below 15 included); vPairs = the slots
 * with weight >= 15, or if there are none the single pKFmax (strict > in ascending slot order:
 * the lowest slot among ties); s's ordered list = vPairs by descending weight, ties by
 * descending slot (the ascending pair sort followed by push_front); for each t in vPairs
 * AddConnection(s, w): if W[t][s] != w it is set and t's ordered list re-sorted over all
 * non-zero weights of row t, sub-threshold ones its own last UpdateConnections left there
 * included, else t's list stays as it is; if mbFirstConnection and s is not root, parent[s] =
 * the list's head.  With distinct slots the sequential result does not depend on the order:
 * the counts are symmetric, so a batch member's row entry is overwritten with the value another
 * member would have written into it, and its list is its own vPairs either way.  The rows of
 * the slots outside the batch that changed are re-sorted once, by a second kernel. */
int orbg_map_update_connections_batch_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots,
                                             int n);
/* one slot from the host (ORBG_EINVAL out of range); synchronises */
int orbg_map_update_connections(orbg_ctx *ctx, orbg_map *map, int slot);

/* Tracking::UpdateLocalKeyFrames for nframes frames: frame f's mvpMapPoints as ids (-1 = NULL)
 * at d_frame_points + f * frame_cap, d_counts[f] of them.  An entry that names a bad point
 * becomes -1 in place, as the reference nulls it.  The slots with votes follow in ascending
 * slot order, bad ones skipped; pKFmax (d_ref_kf[f]; -1: none, mpReferenceKF stays) by strict >.
 * The expansion runs over that initial list only and stops when the list's current size
 * exceeds 80: the first of the ten best neighbours that is neither bad nor listed, the first
 * such child in ascending slot order, then the parent if it exists and is not listed, after
 * which the loop is left (the break of Tracking.cc:1912, reproduced).  Outputs d_local_kfs +
 * f * lkf_cap, d_nlocal[f] = the full length (only the first lkf_cap are written).  An empty
 * counter: d_nlocal[f] = d_ref_kf[f] = -1 (the reference returns without touching
 * mvpLocalKeyFrames). */
int orbg_map_local_keyframes_batch_device(orbg_ctx *ctx, orbg_map *map, int32_t *d_frame_points,
                                          int frame_cap, const int32_t *d_counts, int nframes,
                                          int32_t *d_local_kfs, int lkf_cap, int32_t *d_nlocal,
                                          int32_t *d_ref_kf);
/* Tracking::UpdateLocalPoints plus what SearchLocalPoints needs: frame f's local keyframes
 * (d_local_kfs + f * lkf_cap, d_nlocal[f] of them, clamped to [0, lkf_cap]) in list order,
 * features in index order, each point at its first occurrence, bad points dropped.  Outputs at
 * + f * lp_cap: d_local_ids, d_mps (the stored record with flags = ORBG_MP_VALID unless the
 * point is among the frame's own d_frame_points, mnLastFrameSeen == mCurrentFrame.mnId of
 * Tracking.cc:1644-1683, | ORBG_MP_HAS_OBS), d_qdesc [lp_cap][32]; d_nlocal_points[f] = the
 * full count (only the first lp_cap are written).  These are orbg_is_in_frustum_batch_device's
 * d_mps / d_counts (cap = lp_cap) and orbg_search_by_projection_batch_device(ORBG_TRACK_LOCAL)'s
 * qdesc / qcounts.  frame_cap <= 8192 (ORBG_ENOTSUP), lkf_cap <= max_keyframes, nframes <=
 * 65535 (ORBG_EINVAL). */
int orbg_map_local_points_batch_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_local_kfs,
                                       int lkf_cap, const int32_t *d_nlocal,
                                       const int32_t *d_frame_points, int frame_cap,
                                       const int32_t *d_counts, int nframes, int32_t *d_local_ids,
                                       orbg_map_point *d_mps, uint8_t *d_qdesc, int lp_cap,
                                       int32_t *d_nlocal_points);
/* One frame from host arrays on the same kernels (frame_points is updated in place).
 * ORBG_ERANGE when the result exceeds lkf_cap / lp_cap: *nlocal / *nlocal_points hold the
 * needed count and the first cap entries are written. */
int orbg_map_local_keyframes(orbg_ctx *ctx, orbg_map *map, int32_t *frame_points, int n,
                             int32_t *local_kfs, int lkf_cap, int32_t *nlocal, int32_t *ref_kf);
int orbg_map_local_points(orbg_ctx *ctx, orbg_map *map, const int32_t *local_kfs, int nlocal,
                          const int32_t *frame_points, int n, int32_t *local_ids,
                          orbg_map_point *mps, uint8_t *qdesc, int lp_cap, int32_t *nlocal_points);

/* MapPoint::UpdateNormalAndDepth of the points d_point_ids[i] (NULL: i), i < n, into the stored
 * records.  A bad point, one without observations, or one its reference KeyFrame does not
 * observe is left untouched.  The cv::Mat arithmetic as the reference evaluates it: normali =
 * mWorldPos - Owi in float; cv::norm(normali) accumulates the three squares in double, in
 * order, and takes the double square root; normali / norm is a convertTo with the float alpha
 * (float)(1. / norm), one rounding per element; normal = normal + that in float, over the
 * observations in ascending slot order; mNormalVector = normal / n with the float alpha
 * (float)(1. / n).  dist = (float)cv::norm(Pos - O_ref), the same double norm rounded once;
 * mfMaxDistance = dist * scaleFactor[octave of the point in its reference KeyFrame] and
 * mfMinDistance = mfMaxDistance / scaleFactor[nlevels - 1] in float (the context's tables). */
int orbg_map_update_normal_and_depth_batch_device(orbg_ctx *ctx, orbg_map *map,
                                                  const int32_t *d_point_ids, int n);

/* ---- KeyFrame::SetBadFlag, LocalMapping::KeyFrameCulling / MapPointCulling on the Map ----
 * (src/KeyFrame.cc:560-720, src/LocalMapping.cc:227-270 and 804-877, src/MapPoint.cc:121-232,
 * 325-329).  Further state, all of it defaulting so that the calls above give what they gave
 * without it.  Per feature of a row a flags byte (0 when a slot becomes live; an overwrite of a
 * live slot by orbg_map_set_keyframe* keeps it, these are properties of the keypoints).  Per
 * slot mbNotErase and mbToBeErased (cleared when a slot becomes live).  Per point mnFirstKFid
 * (an mnId, not a slot), mnVisible and mnFound: 0, 1 and 1 after orbg_map_create / clear;
 * orbg_map_set_points* does not touch them.
 * Observations() of a point is the sum over its observations (the live rows that hold it) of 2
 * for a STEREO feature and 1 otherwise: MapPoint::nObs.  A point set bad by the calls below
 * loses ORBG_MP_VALID and is removed from every row that holds it (EraseMapPointMatch). */
#define ORBG_MAP_FEAT_STEREO 1   /* mvuRight[idx] >= 0: the observation counts twice */
#define ORBG_MAP_FEAT_CLOSE 2    /* !(mvDepth[idx] > mThDepth || mvDepth[idx] < 0) */
/* flags[i], i < n, of a live slot's features (the rest of the row: 0).  A dead slot: no change. */
int orbg_map_set_keyframe_features(orbg_ctx *ctx, orbg_map *map, int slot, const uint8_t *flags,
                                   int n);
/* the same for slots d_slots[i], i < n: d_flags + i * row_cap, d_counts[i] entries */
int orbg_map_set_keyframe_features_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots,
                                          int n, const uint8_t *d_flags, int row_cap,
                                          const int32_t *d_counts);
/* on = 1: KeyFrame::SetNotErase.  on = 0: SetErase once the caller has seen mspLoopEdges.empty():
 * clears mbNotErase and, if mbToBeErased is set, runs orbg_map_set_bad_flag (*erased = 1, else
 * 0; may be NULL).  A dead slot: no change.  Synchronises. */
int orbg_map_set_not_erase(orbg_ctx *ctx, orbg_map *map, int slot, int on, int32_t *erased);
/* mnFirstKFid / mnVisible / mnFound of points first .. first + n - 1 (a NULL array leaves that
 * field as it is); the device form takes ids d_ids[i] (NULL: first + i; out of range: skipped) */
int orbg_map_set_point_stats(orbg_ctx *ctx, orbg_map *map, int first, int n,
                             const int32_t *first_kf_id, const int32_t *visible,
                             const int32_t *found);
int orbg_map_set_point_stats_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_ids, int first,
                                    int n, const int32_t *d_first_kf_id, const int32_t *d_visible,
                                    const int32_t *d_found);
/* reads them back, with nobs[i] = Observations() (any array may be NULL) */
int orbg_map_get_point_stats(orbg_ctx *ctx, orbg_map *map, int first, int n, int32_t *first_kf_id,
                             int32_t *visible, int32_t *found, int32_t *nobs);
/* MapPoint::IncreaseVisible(amount) of the points d_ids[i], i < n: an id of -1 (or out of
 * range) is skipped; with d_proj non-NULL entry i counts only if d_proj[i].flags &
 * ORBG_MP_VALID (what orbg_is_in_frustum_batch_device leaves).  Duplicates add up. */
int orbg_map_increase_visible_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_ids,
                                     const orbg_map_projection *d_proj, int n, int amount);
/* MapPoint::IncreaseFound(amount), likewise */
int orbg_map_increase_found_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_ids, int n,
                                   int amount);
/* the row of a slot (mvpMapPoints as ids): *n = its length (0 for a dead slot), the first cap
 * entries written */
int orbg_map_get_keyframe_points(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *ids, int cap,
                                 int32_t *n);
/* mpRefKF of points first .. first + n - 1 as slots (-1: none) */
int orbg_map_get_point_refs(orbg_ctx *ctx, orbg_map *map, int first, int n, int32_t *ref);

/* KeyFrame::SetBadFlag in full.  *status (may be NULL): 0 = the root or a dead slot, nothing
 * happens; 2 = mbNotErase is set: mbToBeErased is set and nothing else; 1 = erased: everything
 * orbg_map_erase_keyframe does, and for every good point p of the row
 * MapPoint::EraseObservation: the entry leaves the row; if mpRefKF[p] was the slot it becomes
 * the lowest remaining observing slot (-1 if none remains: the reference dereferences begin()
 * of an empty map there); if the remaining Observations(p) <= 2 the point goes bad as above.
 * A point that is already bad has no observations and is skipped.  Then the spanning-tree
 * repair of :650-715 over the children (the live slots whose parent is the slot): candidates
 * start as {parent[slot]}; in each round, over the children in ascending slot order (bad ones
 * skipped), their ordered lists in list order and the candidates, the triple with the greatest
 * GetWeight wins by strict >, that is the first one met; that child changes parent and becomes
 * a candidate; when no child is connected to a candidate the remaining children (bad ones
 * included) take parent[slot].  The lists read are the children's lists after this erasure's
 * EraseConnection -> UpdateBestCovisibles (a re-sort over all non-zero weights of the row, so
 * sub-threshold entries may enter); a child not connected to the slot keeps its stored list.
 * parent[slot] itself stays (mTcp is the caller's); a dead slot is never returned as a child:
 * the repair re-parents every live child, and UpdateLocalKeyFrames skips dead and bad ones.
 * Synchronises. */
int orbg_map_set_bad_flag(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *status);

typedef struct {
    int32_t slot;
    int32_t status;      /* 0 kept, 1 erased, 2 marked to-be-erased (mbNotErase), 3 skipped */
    int32_t nmps;        /* nMPs and nRedundantObservations as evaluated at the entry's turn */
    int32_t nredundant;
} orbg_cull_record;
/* LocalMapping::KeyFrameCulling with mpCurrentKeyFrame = slot.  vpLocalKeyFrames is the slot's
 * ordered list as it stands when the call starts.  Per entry t in list order: skipped if root,
 * dead or bad; else over t's features in index order a NULL or bad point is skipped, with
 * !monocular a feature that is not CLOSE is skipped, nMPs++, and if Observations(p) > 3 and at
 * least three other observers have an octave <= this feature's octave + 1 the point is
 * redundant; if (double)nRedundant > 0.9 * (double)nMPs, orbg_map_set_bad_flag runs on t before
 * the next entry is scored: the result is the sequential one.  The start-of-call scores of all
 * entries come from one launch (a workgroup per entry); a sequential pass then re-scores an
 * entry only if an earlier erasure of this call changed Observations() of one of its points.
 * One record per list entry in list order; d_nrec[0] = the list length, only the first rec_cap
 * records are written, the culling acts on all.  The caller forwards status-1 slots to
 * orbg_kfdb_erase and learns which points went bad from orbg_map_get_points. */
int orbg_map_keyframe_culling_device(orbg_ctx *ctx, orbg_map *map, int slot, int monocular,
                                     orbg_cull_record *d_records, int rec_cap, int32_t *d_nrec);
/* host arrays; synchronises.  ORBG_ERANGE when the list is longer than rec_cap. */
int orbg_map_keyframe_culling(orbg_ctx *ctx, orbg_map *map, int slot, int monocular,
                              orbg_cull_record *records, int rec_cap, int32_t *nrec);
/* LocalMapping::MapPointCulling over mlpRecentAddedMapPoints = the n distinct ids d_recent[i],
 * mpCurrentKeyFrame->mnId = current_kf_id.  Per point, in this order: bad (or an id out of
 * range): dropped, status 1; (float)mnFound / (float)mnVisible < 0.25f (the IEEE float
 * division): set bad, 2; current_kf_id - mnFirstKFid >= 2 && Observations() <= (monocular ? 2 :
 * 3): set bad, 3; current_kf_id - mnFirstKFid >= 3: dropped, 4; else kept, 0.  d_recent comes
 * back compacted in its original order, d_nout[0] entries; d_status (may be NULL) is indexed
 * by input position. */
int orbg_map_point_culling_device(orbg_ctx *ctx, orbg_map *map, int32_t *d_recent, int n,
                                  int current_kf_id, int monocular, int32_t *d_nout,
                                  int32_t *d_status);
/* host arrays (recent in place; status may be NULL); synchronises */
int orbg_map_point_culling(orbg_ctx *ctx, orbg_map *map, int32_t *recent, int n,
                           int current_kf_id, int monocular, int32_t *nout, int32_t *status);

/* ---- MapPoint::AddObservation / Replace, ORBmatcher::Fuse(pKF, vpMapPoints, th) and
 * LocalMapping::SearchInNeighbors on the Map ----
 * (src/MapPoint.cc:121-142, 253-303, 342-425, src/ORBmatcher.cc:968-1125, src/LocalMapping.cc:
 * 583-683).  Further state, defaulting so that the calls above give what they gave: per point
 * mpReplaced as an id (-1 = none after orbg_map_create / clear), and the keyframe data that
 * the search and ComputeDistinctiveDescriptors read, attached and not owned.  All calls run on
 * the context stream; the device forms do not synchronise, the host forms do.  After a call
 * that edited rows the observation index is stale and the next query rebuilds it.
 *
 * Replace, as the table sees it: for each observation (KF, idx) of the old point, if the new
 * point is not in KF the row entry becomes the new point (the feature index, and with it the
 * STEREO weight in Observations(), stays), else the entry becomes none; the old point goes bad,
 * mpReplaced[old] = new, the new point gains the old point's mnFound and mnVisible; mpRefKF of
 * both, W, the ordered lists and the parents do not change (only UpdateConnections changes
 * them).  The survivor's ComputeDistinctiveDescriptors runs once per call, after the last pair
 * (after the sequential pass of a Fuse call): its observation set then is the one it has after
 * the last Replace into it, and a survivor that was itself replaced later in the call is bad
 * and keeps the descriptor it had (the reference recomputes it in between; nothing reads it). */
/* mpReplaced of points first .. first + n - 1 as ids (-1: none) */
int orbg_map_get_point_replaced(orbg_ctx *ctx, orbg_map *map, int first, int n, int32_t *replaced);
/* mDescriptor of points first .. first + n - 1 ([n][32], host) */
int orbg_map_get_point_descriptors(orbg_ctx *ctx, orbg_map *map, int first, int n, uint8_t *desc);
/* Attaches the keyframes' data: *kfs is copied, its device arrays (rows of `cap`) and d_cams
 * are indexed by slot and must stay valid while attached; desc, kps, uright (may be NULL) and
 * counts are read, has_mp is not, fv_* only by orbg_map_create_new_points*.  d_cams[slot] =
 * the keyframe's pose, intrinsics and bounds as orbg_fuse reads them.  kfs == NULL detaches.  The calls below return
 * ORBG_EINVAL while nothing is attached (orbg_map_add_observations* needs nothing attached). */
int orbg_map_attach_keyframes(orbg_ctx *ctx, orbg_map *map, const orbg_keyframes *kfs, int cap,
                              const orbg_frustum_camera *d_cams);
/* pMP->AddObservation(pKF, idx) + pKF->AddMapPoint(pMP, idx) for entries i < n in order:
 * CreateNewMapPoints' insertion (after orbg_map_set_points_device wrote the new records) and
 * Fuse's else-branch.  d_status[i] (may be NULL): 0 added; skipped: 1 the slot is dead or out
 * of range, 2 idx outside the slot's N, 3 the id is out of range, 4 the point is bad, 5 the
 * slot already observes the point (mObservations.count(pKF)), 6 the feature holds another
 * point. */
int orbg_map_add_observations_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots,
                                     const int32_t *d_idx, const int32_t *d_point_ids, int n,
                                     int32_t *d_status);
int orbg_map_add_observations(orbg_ctx *ctx, orbg_map *map, const int32_t *slots,
                              const int32_t *idx, const int32_t *point_ids, int n,
                              int32_t *status);
/* MapPoint::ComputeDistinctiveDescriptors of the points d_point_ids[i], i < n, into the map's
 * mDescriptor: the descriptors of the point's observations in ascending slot order, slots
 * flagged ORBG_MAP_KF_BAD (or features past the attached counts) left out, through
 * orbg_distinctive_descriptors_batch_device's kernel.  A bad point, an id out of range or a
 * point with no usable observation keeps its descriptor. */
int orbg_map_distinctive_descriptors_device(orbg_ctx *ctx, orbg_map *map,
                                            const int32_t *d_point_ids, int n);
/* d_old[i]->Replace(d_new[i]) for i < n in order (above), then ComputeDistinctiveDescriptors
 * of the survivors.  d_status[i] (may be NULL): 0 replaced; 1 old == new, nothing; 2 new is bad
 * or out of range, skipped (a precondition of every caller); 3 old is out of range, skipped;
 * 4 old was already bad: it has no observations, so only mpReplaced and the found / visible
 * transfer happen.  Also what LoopClosing::SearchAndFuse applies to vpReplacePoint after
 * orbg_fuse_sim3_batch_device. */
int orbg_map_replace_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_old,
                            const int32_t *d_new, int n, int32_t *d_status);
int orbg_map_replace(orbg_ctx *ctx, orbg_map *map, const int32_t *olds, const int32_t *news, int n,
                     int32_t *status);
/* ORBmatcher::Fuse(pKF = slot, vpMapPoints = d_point_ids, th) in full.  The search inputs are
 * gathered from the map: the record and mDescriptor of each id, ORBG_MP_VALID = in range, good
 * and not in the slot's row when the call starts (-1 is NULL); orbg_fuse_batch_device's kernel
 * runs with the attached keyframe and d_cams[slot]; then the update of :1100-1125 in
 * vpMapPoints order by one workgroup.  d_status[i]: 0 no target (bestDist > TH_LOW = 50, or a
 * feature index outside the slot's N); 1 AddObservation; 2 the point was replaced by the
 * feature's point (pMPinKF->Observations() > pMP->Observations(), strict, as they stand at
 * that moment); 3 the feature's point was replaced by the point; 4 the feature held a bad
 * point (counted, nothing done); 5 it had a target but was bad or in the keyframe by its turn
 * (not counted).  d_nfused[0] = the return value = the number of statuses 1 to 4.  d_best_idx /
 * d_best_dist / d_status [n] may be NULL.  A dead slot: every status 0. */
int orbg_map_fuse_device(orbg_ctx *ctx, orbg_map *map, int slot, const int32_t *d_point_ids, int n,
                         float th, int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_status,
                         int32_t *d_nfused);
int orbg_map_fuse(orbg_ctx *ctx, orbg_map *map, int slot, const int32_t *point_ids, int n,
                  float th, int32_t *best_idx, int32_t *best_dist, int32_t *status,
                  int32_t *nfused);
/* LocalMapping::SearchInNeighbors with mpCurrentKeyFrame = slot, mnId = current_kf_id (only
 * whether it is 0 matters: mnFuseTargetForKF starts at 0, so with id 0 every keyframe counts as
 * marked and both lists are empty).  vpTargetKFs from the stored ordered lists: the first nn =
 * monocular ? 20 : 10 entries of the slot's list, each skipped if bad or marked, else pushed
 * and marked, followed by the first 5 of its own list, each skipped if bad, marked or the slot
 * itself and NOT marked when pushed, so an entry can occur again.  Fuse(target, the slot's row
 * as it stood at the start, th) once per list entry, each with its survivors' descriptors
 * before the next search reads them; vpFuseCandidates = the good points of the entries' rows
 * as they stand then, in list and feature order, each at its first occurrence;
 * Fuse(slot, candidates, th); ComputeDistinctiveDescriptors and UpdateNormalAndDepth of the
 * good points of the slot's row, re-read; UpdateConnections(slot).  d_targets: the first
 * target_cap entries, d_ntargets[0] the full length (at most 120); d_nfused [121]:
 * d_nfused[t] = the return value of entry t's Fuse, d_nfused[ntargets] the second pass's, the
 * rest 0.  The device form never synchronises: the launches are sized by the bounds (6 nn
 * entries, 120 * kf_cap candidates) and the lengths stay on the device.  The workspace
 * belongs to the map and is allocated by the first call. */
int orbg_map_search_in_neighbors_device(orbg_ctx *ctx, orbg_map *map, int slot, int current_kf_id,
                                        int monocular, float th, int32_t *d_targets,
                                        int target_cap, int32_t *d_ntargets, int32_t *d_nfused);
/* host arrays (nfused [121]); ORBG_ERANGE when the list is longer than target_cap */
int orbg_map_search_in_neighbors(orbg_ctx *ctx, orbg_map *map, int slot, int current_kf_id,
                                 int monocular, float th, int32_t *targets, int target_cap,
                                 int32_t *ntargets, int32_t *nfused);

/* ---- LocalMapping::CreateNewMapPoints and ProcessNewKeyFrame on the Map ----
 * Beside orbg_map_attach_keyframes (whose fv_nodes / fv_off / fv_feats / nfv are read here, in
 * orbg_search_for_triangulation_batch_device's layout: ORBG_EINVAL if one is NULL) the rest of
 * what the triangulation reads, indexed by slot with the attached `cap`, not owned: mvKeys
 * d_kps_raw (NULL: mvKeysUn), mvDepth d_depth (required when uright is attached) and
 * d_kf_cams[slot], of which only fx, fy, cx, cy, invfx, invfy, mb, mbf are read.  The pose is the
 * Map's stored Tcw (orbg_map_set_keyframe_poses) and the camera centre its stored Ow, which
 * orbg_map_lba_apply_device keeps current: there is no further copy of a pose.  d_kf_cams ==
 * NULL detaches. */
int orbg_map_attach_keyframe_geometry(orbg_ctx *ctx, orbg_map *map, const orbg_keypoint *d_kps_raw,
                                      const float *d_depth, const orbg_kf_camera *d_kf_cams);
#define ORBG_CNP_POINT_RANGE 1    /* an id reached max_points */
#define ORBG_CNP_RECENT_RANGE 2   /* a d_recent position reached recent_cap */
#define ORBG_CNP_DEAD 4           /* the slot is not live: nothing done */
#define ORBG_CNP_NO_POSE 8        /* the slot has no stored pose: nothing done */
/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:293-576) with mpCurrentKeyFrame = slot,
 * mnId = current_kf_id.  Neighbours: the first nn = monocular ? 20 : 10 entries of the slot's
 * stored ordered list (no bad check, as the reference); d_neigh[i] (-1 past the count).  From
 * neighbour i > 0 on CheckNewKeyFrames() is d_abort (may be NULL; any device-readable address,
 * mapped pinned host memory included), read once per neighbour by one lane and latched: once
 * non-zero that neighbour and all later ones get status 2.  d_neigh_status[i]: 0 processed;
 * 1 skipped by the baseline test (baseline = cv::norm of the stored centres' difference; stereo:
 * baseline < mb of the neighbour; monocular: baseline / ComputeSceneMedianDepth(2) < 0.01, the
 * depths z = Tcw row 2 . X + tz of every row entry of the neighbour, accumulated in double in
 * order, sorted, element (n - 1) / 2); 2 aborted; 3 a dead neighbour, one without a stored pose
 * or, monocular, with an empty row (a departure: the reference indexes an empty vector there).
 * Per processed neighbour in list order: ComputeF12, SearchForTriangulation(cur, nb, F12, .,
 * false) of ORBmatcher(0.6, false) with has_mp = (row[idx] >= 0) of both rows as they stand at
 * that moment, the triangulation (the three kernels of orbg_triangulation_geometry /
 * orbg_search_for_triangulation / orbg_triangulate_batch_device, unchanged), then the insertion
 * in idx1 order: point k of the whole call gets id first_id + k, the record (x3d,
 * ORBG_MP_VALID), mpRefKF = slot, mnFirstKFid = current_kf_id, mnVisible = mnFound = 1,
 * mpReplaced = -1, mnCorrected* = 0, the id in row[slot][idx1] and row[nb][idx2], and the id
 * appended to d_recent at d_nrecent[0] (in / out).  The reference never sets vbMatched2, so two
 * idx1 may match one idx2: both points are created and, as pKF2->AddMapPoint overwrites, the
 * later one keeps the neighbour's feature (a departure: the earlier point then has no
 * observation in the neighbour, where the reference leaves a one-sided one).
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth of the new points run once, after the
 * last neighbour (nothing in between reads them).  W, the ordered lists and the parents do not
 * change.  d_nmatches[i] = the search's return value, d_nnew[i] = points created, d_tri_status
 * (may be NULL) [20][kf_cap of the Map] = the ORBG_TRI_* per idx1.  An id >= max_points or a
 * d_recent position >= recent_cap: that point and all later ones of the call are not created
 * and no row is touched for them (the feature of the slot is still taken as matched by the
 * later neighbours' searches, so that d_out[2] is exact).  d_out: [0] neighbours, [1] points
 * created, [2] points a large enough cap would have created, [3] ORBG_CNP_* bits.  Precondition, not checked: the ids
 * from first_id on are unused.  The device form never synchronises and allocates nothing after
 * its first call on a map (the workspace belongs to the map): the launches are sized by the
 * bounds (20 neighbours, kf_cap features) and every length stays on the device: 4 launches and
 * one 4-byte memset per neighbour slot, nn of them whatever the list holds, plus three of its
 * own and those of the closing index rebuild, descriptors and normals.
 * ORBG_EINVAL: slot out of range, first_id < 0, nothing / no geometry attached, fv_* NULL. */
int orbg_map_create_new_points_device(orbg_ctx *ctx, orbg_map *map, int slot, int current_kf_id,
                                      int monocular, int first_id, const int32_t *d_abort,
                                      int32_t *d_recent, int recent_cap, int32_t *d_nrecent,
                                      int32_t *d_neigh, int32_t *d_neigh_status,
                                      int32_t *d_nmatches, int32_t *d_nnew, int8_t *d_tri_status,
                                      int32_t *d_out);
/* host arrays (abort: one int32 or NULL, read when the call starts; *nrecent in / out;
 * tri_status may be NULL); synchronises.  ORBG_ERANGE for the two range bits (everything is
 * written), ORBG_EINVAL for a dead slot or one without a pose. */
int orbg_map_create_new_points(orbg_ctx *ctx, orbg_map *map, int slot, int current_kf_id,
                               int monocular, int first_id, const int32_t *abort, int32_t *recent,
                               int recent_cap, int32_t *nrecent, int32_t *neigh,
                               int32_t *neigh_status, int32_t *nmatches, int32_t *nnew,
                               int8_t *tri_status, int32_t *out);
/* The table side of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:164-220) for one
 * keyframe: the row (d_point_ids / d_octaves / d_feat_flags [n]; d_feat_flags may be NULL), the
 * pose d_Tcw [12], mnId and the ORBG_MAP_KF_* flags are stored as orbg_map_set_keyframes_device,
 * _features_device and _poses_device store them (the centre is -Rcw^T tcw).  An id that is bad
 * or out of range is stored as -1 (a departure: the reference leaves the bad pointer in
 * mvpMapPoints and every reader skips it).  For each good entry in feature order:
 * d_in_keyframe[i] != 0 (pMP->IsInKeyFrame(pKF) as Tracking left it; NULL: all 0; the table
 * cannot know, the row is the observation set) appends the id to d_recent at d_nrecent[0];
 * otherwise the point's UpdateNormalAndDepth and ComputeDistinctiveDescriptors run once the row
 * is in.  Then UpdateConnections(slot).  d_out: [0] ids appended, [1] points updated, [2] ids
 * a large enough recent_cap would have appended, [3] ORBG_CNP_RECENT_RANGE or 0.  Needs the
 * keyframe data attached (the slot's descriptors included).  Never synchronises. */
int orbg_map_process_new_keyframe_device(orbg_ctx *ctx, orbg_map *map, int slot,
                                         const int32_t *d_point_ids, const uint8_t *d_octaves,
                                         const uint8_t *d_feat_flags, int n, const float *d_Tcw,
                                         int mnid, int kf_flags, const uint8_t *d_in_keyframe,
                                         int32_t *d_recent, int recent_cap, int32_t *d_nrecent,
                                         int32_t *d_out);
/* host arrays; synchronises.  ORBG_ERANGE for the range bit. */
int orbg_map_process_new_keyframe(orbg_ctx *ctx, orbg_map *map, int slot, const int32_t *point_ids,
                                  const uint8_t *octaves, const uint8_t *feat_flags, int n,
                                  const float *Tcw, int mnid, int kf_flags,
                                  const uint8_t *in_keyframe, int32_t *recent, int recent_cap,
                                  int32_t *nrecent, int32_t *out);

/* ---------------- ORBmatcher::SearchByBoW(KeyFrame*, Frame&) ---------------- */
/* One side of SearchByBoW pairs, device memory, in orbg_bow_transform_batch_device's layout
 * (frame f's rows at + f * cap, fv_off at + f * (cap + 1)): descriptors [cap][32], keypoints
 * [cap] (only .angle is read: the KeyFrame's mvKeysUn, the Frame's mvKeys), counts[f] = N,
 * the FeatureVector (fv_nodes / fv_off / fv_feats / nfv) and, on the KeyFrame side, valid
 * [cap] = "pMP && !pMP->isBad()" of mvpMapPoints (NULL: every feature has a good MapPoint;
 * ignored on the Frame side). */
typedef struct {
    const uint8_t *desc;
    const orbg_keypoint *kps;
    const int32_t *counts;
    const int32_t *fv_nodes, *fv_off, *fv_feats, *nfv;
    const uint8_t *valid;
} orbg_bow_frames;
/* ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches)
 * (src/ORBmatcher.cc:195-348; Tracking::TrackReferenceKeyFrame Tracking.cc:1069,
 * Relocalization :2009) for pairs p: KeyFrame kf_index[p] of `kf`, Frame f_index[p] of `f`
 * (device int arrays; the two sides may be the same batch).  match[p * cap + i] = the KeyFrame
 * feature whose MapPoint matched F's feature i (vpMapPointMatches[i] =
 * pKF->GetMapPointMatches()[match]), -1 if NULL, for i < N of the frame; nmatch[p] = the
 * return value.  nnratio = mfNNratio, check_ori = mbCheckOrientation.  On the match stream
 * (orbg_match_stream), ordered after the context stream (as orbg_batch_summary). */
int orbg_search_by_bow_batch_device(orbg_ctx *ctx, const orbg_bow_frames *kf,
                                    const orbg_bow_frames *f, int cap, const int32_t *d_kf_index,
                                    const int32_t *d_f_index, int npairs, float nnratio,
                                    int check_ori, int32_t *d_match, int32_t *d_nmatch);
/* The same for one pair from host arrays: the KeyFrame's n_kf descriptors, mvKeysUn angles
 * (kf_angle), valid flags (NULL: all) and FeatureVector; the Frame's n_f descriptors, mvKeys
 * angles and FeatureVector.  match[n_f] as above; *nmatches = the return value. */
int orbg_search_by_bow(orbg_ctx *ctx, const uint8_t *kf_desc, const float *kf_angle,
                       const uint8_t *kf_valid, int n_kf, const int32_t *kf_fv_nodes,
                       const int32_t *kf_fv_off, const int32_t *kf_fv_feats, int kf_nfv,
                       const uint8_t *f_desc, const float *f_angle, int n_f,
                       const int32_t *f_fv_nodes, const int32_t *f_fv_off,
                       const int32_t *f_fv_feats, int f_nfv, float nnratio, int check_ori,
                       int32_t *match, int *nmatches);

/* ORBmatcher(nnratio, checkOri).SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12)
 * (src/ORBmatcher.cc:634-769; LoopClosing::ComputeSim3, LoopClosing.cc:485): pKF1's features with a good MapPoint
 * (valid1 = pMP && !isBad(), NULL: all) against pKF2's of the same node with a good MapPoint
 * (valid2) not yet matched; bestDist1 < TH_LOW (strict, unlike the KeyFrame-Frame form's
 * <=), the float ratio test, the rotation histogram over mvKeysUn angles.  match12[n1] = the
 * pKF2 feature matched to pKF1's feature i (vpMatches12[i] = pKF2->GetMapPointMatches()[
 * match12[i]]), -1 if NULL; *nmatches = the return value.  Host arrays: */
int orbg_search_by_bow_kf(orbg_ctx *ctx, const uint8_t *desc1, const float *angle1,
                          const uint8_t *valid1, int n1, const int32_t *fv_nodes1,
                          const int32_t *fv_off1, const int32_t *fv_feats1, int nfv1,
                          const uint8_t *desc2, const float *angle2, const uint8_t *valid2,
                          int n2, const int32_t *fv_nodes2, const int32_t *fv_off2,
                          const int32_t *fv_feats2, int nfv2, float nnratio, int check_ori,
                          int32_t *match12, int *nmatches);
/* Batched, device memory (orbg_bow_frames layout, the .valid arrays of both sides read):
 * d_match12[p * cap + i] for i < N of pKF1 = d_kf1_index[p]; on the match stream, ordered after
 * the context stream (as orbg_search_by_bow_batch_device). */
int orbg_search_by_bow_kf_batch_device(orbg_ctx *ctx, const orbg_bow_frames *kf1,
                                       const orbg_bow_frames *kf2, int cap,
                                       const int32_t *d_kf1_index, const int32_t *d_kf2_index,
                                       int npairs, float nnratio, int check_ori,
                                       int32_t *d_match12, int32_t *d_nmatch);

/* ---------------- Sim3Solver (LoopClosing::ComputeSim3) ----------------
 * Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) + SetRansacParameters + iterate / find
 * (src/Sim3Solver.cc:37-364; LoopClosing.cc:530-594), every RANSAC iteration of every
 * candidate pair evaluated in one batch.
 *
 * The caller compacts the correspondences (Sim3Solver.cc:62-102: the pointer tests, isBad()
 * and GetIndexInKeyFrame stay on the host): correspondence i holds the world positions of
 * pMP1 / pMP2, mvLevelSigma2[octave] of the two keypoints and index1 = mvnIndices1[i], the
 * slot in vpMatched12.  The device computes X3Dc = Rcw * Xw + tcw for both cameras, the
 * own-image projections (FromCameraToImage, :405-423) and the thresholds mvnMaxError1 / 2,
 * which the reference keeps in a vector<size_t>: th = (float)(uint64_t)(9.210 * (double)sigma2).
 *
 * An iteration is Horn 1987 on its three sampled correspondences (ComputeSim3, :226-337) and
 * CheckInliers (:340-364: err1 < th1 && err2 < th2, both strict, NaN fails), all in fp32.
 * Departures: the 4x4 eigenvector comes from a fixed number of cyclic Jacobi sweeps, and R is
 * built from the unit quaternion directly where the reference goes quaternion -> angle-axis
 * -> cv::Rodrigues.  That is the same rotation (and +q / -q give the same R), except that the
 * reference's 0 / 0 at an exactly zero rotation angle does not occur here.  A degenerate
 * sample (largest eigenvalue not positive, e.g. three identical points, or a scale that is
 * zero or not finite; the reference then carries NaN or infinity and finds no inlier) counts
 * 0 inliers, with an all-zero mask and an all-zero hypothesis (s = 0).
 *
 * The random draws are an input: samples[it] = the three correspondence indices of iteration
 * it, which the reference takes from rand() (DUtils::Random::RandomInt, Sim3Solver.cc:163-177).
 *
 * Acceptance is the reference's sequential rule (:183-200) from a fresh solver over
 * iterations 0 .. iterations - 1: best is replaced when count >= best (ties go to the later
 * iteration); the first iteration with count >= best && count > min_inliers (strict) is the
 * hit and ends the scan.  hit_iter = that iteration or -1; best_iter = the iteration holding
 * mBestT12 when the scan ended (-1: none ran); nomore = bNoMore (N < min_inliers, or every
 * iteration used without a hit); hyp / ninliers / inliers12 are those of the returned
 * iteration: the hit, else best_iter (all zero if none ran).  N < min_inliers or N < 3 runs
 * no iteration. */
typedef struct {
    float T1w[12], T2w[12];          /* pKF1 / pKF2 GetPose() rows 0..2 */
    float fx1, fy1, cx1, cy1;        /* pKF1->mK */
    float fx2, fy2, cx2, cy2;        /* pKF2->mK */
    int32_t n;                       /* N, the correspondences of this pair */
    int32_t fix_scale;               /* mbFixScale */
    int32_t min_inliers;             /* mRansacMinInliers */
    int32_t iterations;              /* mRansacMaxIts (orbg_sim3_ransac_iterations) */
} orbg_sim3_problem;
typedef struct {
    float Xw1[3], Xw2[3];            /* pMP1 / pMP2 GetWorldPos() */
    float sigma2_1, sigma2_2;        /* mvLevelSigma2[kp.octave] in pKF1 / pKF2 */
    int32_t index1;                  /* mvnIndices1[i] */
} orbg_sim3_corr;
typedef struct {
    float R[9], t[3], s;             /* mR12i (row-major), mt12i, ms12i */
} orbg_sim3_hyp;
typedef struct {
    int32_t hit_iter, best_iter, ninliers, nomore;
    orbg_sim3_hyp hyp;
} orbg_sim3_result;
/* Sim3Solver::SetRansacParameters (:114-138): mRansacMaxIts for N = n correspondences
 * (epsilon a float, pow / log in double; 1 when min_inliers == n; max(1, min(nIterations,
 * max_its))).  LoopClosing uses (0.99, 20, 300).  Host arithmetic only: no GPU, no context. */
int orbg_sim3_ransac_iterations(double prob, int min_inliers, int max_its, int n);
/* One pair from host arrays: corrs[problem->n], samples[problem->iterations][3], n1 =
 * vpMatched12.size().  Outputs: result, inliers12[n1] (vbInliers as bytes) and, where not
 * NULL, counts[iterations] (mnInliersi), hyps[iterations] and masks[iterations][ceil(n / 64)]
 * (bit i % 64 of word i / 64 = mvbInliersi[i]).  ORBG_EINVAL for a NULL context or required
 * pointer, an index1 outside [0, n1), a sample index outside [0, n) or one repeated within its
 * triple; ORBG_ENOTSUP past 8192 correspondences.  Runs the batched kernels with npairs = 1
 * (bit-identical results).  Synchronises. */
int orbg_sim3_solve(orbg_ctx *ctx, const orbg_sim3_problem *problem, const orbg_sim3_corr *corrs,
                    const int32_t *samples, int n1, int32_t *counts, orbg_sim3_hyp *hyps,
                    uint64_t *masks, orbg_sim3_result *result, uint8_t *inliers12);
/* Batched, device memory: pair p = d_problems[p] with d_corrs + p * cap, d_samples +
 * (p * max_its) * 3; cap a multiple of 64 (ORBG_ENOTSUP past 8192), d_problems[p].n <= cap and
 * .iterations <= max_its (a count outside that runs nothing; more iterations are cut at
 * max_its).  Outputs d_counts[npairs][max_its], d_hyps[npairs][max_its], d_masks[npairs]
 * [max_its][cap / 64], d_results[npairs], d_inliers12[npairs][n1cap] (an index1 outside
 * [0, n1cap) is not written).  Iterations past a pair's own and mask words past its n are
 * zero; a triple with an index outside [0, n) or a repeated one is a degenerate iteration.
 * Context stream, no host synchronisation; the only allocation is the context scratch, grown
 * when a call needs more than any before it. */
int orbg_sim3_solve_batch_device(orbg_ctx *ctx, const orbg_sim3_problem *d_problems,
                                 const orbg_sim3_corr *d_corrs, const int32_t *d_samples,
                                 int npairs, int cap, int max_its, int32_t *d_counts,
                                 orbg_sim3_hyp *d_hyps, uint64_t *d_masks,
                                 orbg_sim3_result *d_results, uint8_t *d_inliers12, int n1cap);

/* ---------------- Optimizer::OptimizeSim3 (LoopClosing::ComputeSim3) ----------------
 * Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cc:
 * 1366-1578; LoopClosing.cc:598-603 with th2 = 10), one workgroup per loop candidate: g2o's
 * Levenberg-Marquardt (BlockSolverX + LinearSolverDense) on the one free VertexSim3Expmap,
 * in fp64, with the numeric Jacobian g2o really uses for these edges
 * (BaseBinaryEdge::linearizeOplus: central differences, delta 1e-9, through
 * Sim3(update) * estimate), Huber of delta = (float)sqrt(th2), optimize(5), the drop test,
 * optimize(nBad > 0 ? 10 : 5) on the kept pairs and the final test.
 *
 * The caller compacts the correspondences as the loop of Optimizer.cc:1426-1513 does (the
 * pointer tests, isBad() and GetIndexInKeyFrame stay on the host): correspondence i holds
 * the world positions of pMP1 = vpMapPoints1[index1] and pMP2 = vpMatches1[index1], the
 * undistorted keypoints obs1 = pKF1->mvKeysUn[index1].pt and obs2 = pKF2->mvKeysUn[i2].pt,
 * mvInvLevelSigma2[octave] of the two and index1, the slot in vpMatches1.  The device
 * computes the fixed points P1c = R1w Xw1 + t1w and P2c = R2w Xw2 + t2w in float and widens
 * them.  The initial Sim3 is an orbg_sim3_hyp (float R, t, s), as orbg_sim3_result.hyp holds
 * it: g2o::Sim3(Converter::toMatrix3d(R), toVector3d(t), s), i.e. Eigen's Quaterniond(R).
 *
 * A pair is dropped when e12.chi2() > th2 || e21.chi2() > th2, evaluated in double at the
 * estimate of the last LM trial g2o evaluated, accepted or not (g2o does not recompute the
 * errors after a rejected trial, and OptimizeSim3 classifies on the stored ones).  A NaN is
 * not greater than th2, so the pair stays.  A point with non-positive depth is not treated
 * specially anywhere: z = 0 divides to +-infinity or NaN, z < 0 projects through the
 * camera centre, and the chi2 that results takes the same comparisons as any other.
 *
 * Result: q (x, y, z, w; not re-normalised, as g2o::Sim3 keeps it), t, s of g2oS12 in
 * double; R = Quaterniond::toRotationMatrix(), tf, sf = the same estimate rounded to float
 * once (for orbg_sim3_pair and Scw); ninliers = the return value (0 when fewer than 10 pairs
 * survive the first test, and then q, t, s are the input, as g2oS12 is not written back);
 * nbad = nBad of the first test; ncorr = nCorrespondences; iterations = the LM iterations
 * each optimize() ran.  keep[j] = 1 iff slot j had a correspondence and vpMatches1[j] was
 * not set to NULL (on the return-0 path too: the first test's drops stay dropped). */
typedef struct {
    float T1w[12], T2w[12];          /* pKF1 / pKF2 GetPose() rows 0..2 */
    float fx1, fy1, cx1, cy1;        /* pKF1->mK */
    float fx2, fy2, cx2, cy2;        /* pKF2->mK */
    int32_t n;                       /* nCorrespondences */
    int32_t fix_scale;               /* bFixScale */
    float th2;                       /* th2 (LoopClosing: 10) */
    int32_t pad;
} orbg_sim3opt_problem;
typedef struct {
    float Xw1[3], Xw2[3];            /* pMP1 / pMP2 GetWorldPos() */
    float obs1[2], obs2[2];          /* kpUn1.pt, kpUn2.pt */
    float inv_sigma2_1, inv_sigma2_2;/* mvInvLevelSigma2[kpUn.octave] in pKF1 / pKF2 */
    int32_t index1;                  /* the slot i of vpMatches1 */
} orbg_sim3opt_corr;
typedef struct {
    double q[4], t[3], s;            /* g2oS12 (q = x, y, z, w) */
    float R[9], tf[3], sf;           /* the same, rounded once (R row-major) */
    int32_t ninliers, nbad, ncorr;
    int32_t iterations[2];
} orbg_sim3opt_result;
/* One candidate from host arrays: corrs[problem->n], init = the Sim3 to refine, n1 =
 * vpMatches1.size(); outputs result and keep[n1].  ORBG_EINVAL for a NULL context or required
 * pointer, an index1 outside [0, n1), a th2 that is not finite or <= 0; ORBG_ENOTSUP past
 * 8192 correspondences.  Runs the batched kernel with npairs = 1 (bit-identical results).
 * Synchronises. */
int orbg_optimize_sim3(orbg_ctx *ctx, const orbg_sim3opt_problem *problem,
                       const orbg_sim3opt_corr *corrs, const orbg_sim3_hyp *init, int n1,
                       orbg_sim3opt_result *result, uint8_t *keep);
/* Batched, device memory: candidate p = d_problems[p] with d_corrs + p * cap and d_init[p];
 * cap a multiple of 64 (ORBG_ENOTSUP past 8192).  A count outside [0, cap], or a th2 that is
 * not finite and positive, runs nothing: the record is that of n = 0 (the input Sim3, all
 * counts 0).  d_keep[npairs][n1cap]: every byte of a candidate's row is written, 0 where no
 * correspondence names the slot; an index1 outside [0, n1cap) writes nothing.  Context
 * stream, no host synchronisation, no allocation.  The sums are reduced in a fixed order:
 * results are reproducible run to run and equal to orbg_optimize_sim3's. */
int orbg_optimize_sim3_batch_device(orbg_ctx *ctx, const orbg_sim3opt_problem *d_problems,
                                    const orbg_sim3opt_corr *d_corrs, const orbg_sim3_hyp *d_init,
                                    int npairs, int cap, orbg_sim3opt_result *d_results,
                                    uint8_t *d_keep, int n1cap);

/* ---------------- PnPsolver (Tracking::Relocalization) ----------------
 * PnPsolver(F, vpMapPointMatches) + SetRansacParameters + iterate / find (src/PnPsolver.cc:
 * 67-340, EPnP proper :342-900; Tracking.cc:1958-2180), every RANSAC iteration of every
 * candidate KeyFrame evaluated in one batch.
 *
 * The caller compacts the correspondences (PnPsolver.cc:79-101: the pointer test and isBad()
 * stay on the host): correspondence i holds Xw = pMP->GetWorldPos(), uv = mvKeysUn[k].pt,
 * sigma2 = mvLevelSigma2[octave] and index = mvKeyPointIndices[i] = k, the slot in
 * vpMapPointMatches.  The device forms mvMaxError[i] = sigma2 * th2 as a float product.
 *
 * An iteration is EPnP's compute_pose (:477-525) on its min_set sampled correspondences, in
 * fp64: centroid and PCA control points, barycentric coordinates, M^T M and its four
 * eigenvectors of least eigenvalue, L_6x10 and rho, the three linearised beta starts, five
 * Gauss-Newton steps each, compute_R_and_t (solve_for_sign on the first point's depth; row 2
 * of R negated when det < 0, as :618-622) and the candidate of least mean reprojection error
 * (compared with <: a NaN never wins, candidate 1 stands when all are NaN).  Then CheckInliers
 * (:308-339) with the reference's types: Xc, Yc the double sums rounded to float, invZc =
 * (float)(1 / double sum), ue / ve in double, distX, distY, error2 in float, error2 <
 * mvMaxError[i] strict (a NaN fails).  A hypothesis that is not finite counts 0 inliers, with
 * an all-zero mask and an all-zero hypothesis.
 *
 * Departures: the 12x12 and 3x3 symmetric eigen problems (cvSVD of M^T M and of PW0^T PW0)
 * are solved by a fixed number of cyclic Jacobi sweeps in fp64; the 3x3 SVD of
 * estimate_R_and_t by one-sided Jacobi; the inverse of the control-point matrix
 * (cvInvert(CV_SVD)) is formed from the orthonormal PCA axes; the beta starts
 * (cvSolve(CV_SVD)) are Householder least squares, as the Gauss-Newton steps are in the
 * reference (qr_solve).  These differ from the reference only for rank-deficient systems,
 * e.g. exactly coplanar samples, where cvSVD returns the minimum-norm solution and this code
 * a hypothesis that is not finite (0 inliers).  The sums over a sample's points run in index
 * order.  The sign of a PCA axis is the SVD routine's choice in the reference, and the pose of
 * a noisy sample depends on it (a flipped axis mirrors the control tetrahedron); here every
 * axis has its component of largest magnitude positive.  For min_set = 4 (and 5) M^T M has an exactly four-dimensional null space, the four
 * eigenvectors are an arbitrary basis of it and the beta starts depend on that basis: there
 * the hypotheses are implementation-defined (here: the basis the Jacobi sweeps end with, in
 * ascending eigenvalue order), as they are for cvSVD.
 *
 * The random draws are an input: samples[it][0 .. min_set) = the correspondence indices of
 * iteration it, which the reference takes from rand() (DUtils::Random::RandomInt,
 * PnPsolver.cc:191-201).
 *
 * Acceptance is the reference's rule (:209-255) from a fresh solver over iterations
 * 0 .. iterations - 1 with best = 0: an iteration with count >= min_inliers and count > best
 * (strict: ties keep the earlier one) becomes the best, a "record iteration"; then Refine()
 * runs on the best set so far (EPnP on all its inliers, then CheckInliers), ok = refined
 * count > min_inliers (strict).  The first iteration with count >= min_inliers whose current
 * best has ok is the hit and returns the refined pose, count and mask.  Refine's outcome
 * depends on the best set alone, so it is evaluated once per record iteration: refines[it] =
 * {valid = 1, count, ok, hyp} and refined_masks[it] at a record iteration, all zero elsewhere.
 * Without a hit nomore = 1 and the result is the last record's unrefined hypothesis, count and
 * mask (refined = 0), or all zero if there was none.  N < min_inliers runs nothing and sets
 * nomore = 1.  (After a hit a later iterate() call hits again at the next iteration with
 * count >= min_inliers, as Refine reruns on the unchanged best set.) */
#define ORBG_PNP_MAX_SET 8
typedef struct {
    float fx, fy, cx, cy;            /* F.fx, F.fy, F.cx, F.cy */
    int32_t n;                       /* N, the correspondences of this candidate */
    int32_t min_set;                 /* mRansacMinSet, 4 .. 8 */
    int32_t min_inliers;             /* mRansacMinInliers as SetRansacParameters adjusted it */
    int32_t iterations;              /* mRansacMaxIts (orbg_pnp_ransac_parameters) */
    float th2;                       /* th2 of SetRansacParameters (Tracking: 5.991) */
} orbg_pnp_problem;
typedef struct {
    float Xw[3];                     /* pMP->GetWorldPos() */
    float uv[2];                     /* F.mvKeysUn[index].pt */
    float sigma2;                    /* F.mvLevelSigma2[kp.octave] */
    int32_t index;                   /* mvKeyPointIndices[i] */
} orbg_pnp_corr;
typedef struct {
    double R[9], t[3];               /* mRi (row-major), mti */
} orbg_pnp_hyp;
typedef struct {
    int32_t valid;                   /* 1 at a record iteration */
    int32_t count;                   /* mnRefinedInliers */
    int32_t ok;                      /* Refine()'s return value */
    int32_t pad;
    orbg_pnp_hyp hyp;                /* the refined mRi, mti */
} orbg_pnp_refine;
typedef struct {
    int32_t hit_iter, best_iter, ninliers, nomore, refined;
    float Tcw[12];                   /* rows 0..2 of mRefinedTcw / mBestTcw: the double pose
                                        rounded once, as convertTo(CV_32F); zeros if none */
} orbg_pnp_result;
/* PnPsolver::SetRansacParameters (:121-152) for N = n correspondences, type for type:
 * nMinInliers = (int)(N * epsilon) through float, raised to min_inliers and min_set; epsilon
 * raised to (float)nMinInliers / N; iterations = 1 when nMinInliers == N, else
 * ceil(log(1 - prob) / log(1 - pow(epsilon, 3))) in double; max(1, min(iterations, max_its)).
 * Tracking uses (0.99, 10, 300, 4, 0.5f) and th2 = 5.991f.  ORBG_EINVAL for n < 1 (the
 * reference divides by N) or a NULL output.  Host arithmetic only: no GPU, no context. */
int orbg_pnp_ransac_parameters(double prob, int min_inliers, int max_its, int min_set,
                               float epsilon, int n, int *min_inliers_out, int *iterations_out);
/* One candidate from host arrays: corrs[problem->n], samples[problem->iterations]
 * [problem->min_set], n1 = vpMapPointMatches.size().  Outputs: result, inliers[n1] (vbInliers
 * as bytes) and, where not NULL, counts[iterations] (mnInliersi), hyps[iterations],
 * masks[iterations][ceil(n / 64)] (bit i % 64 of word i / 64 = mvbInliersi[i]),
 * refines[iterations] and refined_masks[iterations][ceil(n / 64)].  ORBG_EINVAL for a NULL
 * context or required pointer, an index outside [0, n1), min_set outside 4 .. 8, a sample
 * index outside [0, n) or one repeated within its sample; ORBG_ENOTSUP past 8192
 * correspondences.  Runs the batched kernels with ncand = 1 (bit-identical results).
 * Synchronises. */
int orbg_pnp_solve(orbg_ctx *ctx, const orbg_pnp_problem *problem, const orbg_pnp_corr *corrs,
                   const int32_t *samples, int n1, int32_t *counts, orbg_pnp_hyp *hyps,
                   uint64_t *masks, orbg_pnp_refine *refines, uint64_t *refined_masks,
                   orbg_pnp_result *result, uint8_t *inliers);
/* Batched, device memory: candidate p = d_problems[p] with d_corrs + p * cap and d_samples +
 * (p * max_its + it) * ORBG_PNP_MAX_SET (the first min_set entries are read); cap a multiple
 * of 64 (ORBG_ENOTSUP past 8192), d_problems[p].n <= cap and .iterations <= max_its (a count
 * outside that, or a min_set outside 4 .. 8, runs nothing; more iterations are cut at
 * max_its).  Outputs d_counts[ncand][max_its], d_hyps[ncand][max_its], d_masks[ncand][max_its]
 * [cap / 64], d_refines[ncand][max_its], d_refined_masks[ncand][max_its][cap / 64],
 * d_results[ncand], d_inliers[ncand][n1cap] (an index outside [0, n1cap) is not written).
 * Iterations past a candidate's own and mask words past its n are zero; a sample with an
 * index outside [0, n) or a repeated one is a degenerate iteration (count 0, zero mask, zero
 * hypothesis).  Context stream, no host synchronisation, no allocation.  No floating-point
 * atomics and fixed summation orders: results are reproducible run to run and equal to
 * orbg_pnp_solve's. */
int orbg_pnp_solve_batch_device(orbg_ctx *ctx, const orbg_pnp_problem *d_problems,
                                const orbg_pnp_corr *d_corrs, const int32_t *d_samples,
                                int ncand, int cap, int max_its, int32_t *d_counts,
                                orbg_pnp_hyp *d_hyps, uint64_t *d_masks,
                                orbg_pnp_refine *d_refines, uint64_t *d_refined_masks,
                                orbg_pnp_result *d_results, uint8_t *d_inliers, int n1cap);

/* ---------------- Optimizer::OptimizeEssentialGraph (LoopClosing::CorrectLoop) ----------------
 * The Sim3 pose graph of src/Optimizer.cc:1021-1324 (LoopClosing.cc:914): one
 * VertexSim3Expmap per keyframe, EdgeSim3 edges with identity information and no robust
 * kernel, g2o's numeric Jacobian (central differences, delta 1e-9), BlockSolver_7_3 with
 * OptimizationAlgorithmLevenberg under setUserLambdaInit(1e-16), optimize(20).  The map
 * bookkeeping (which keyframes, which edges; :1040-1258) is the caller's: vertices are
 * numbered 0 .. nvert - 1, Scw[v] is vScw (the corrected Sim3 where CorrectedSim3 has one,
 * else the keyframe's pose with scale 1), Snc[v] the NonCorrectedSim3 where one exists, else
 * Scw[v].  Edge (i, j, kind): vertex 0 of the EdgeSim3 is i, vertex 1 is j, its measurement
 * Sjw * Swi taken from Scw (kind 0: a LoopConnections edge, :1104-1134) or from Snc (kind 1:
 * spanning tree, loop and covisibility edges, :1140-1258).  Two vertices may share several
 * edges.  Precondition, as in the reference: every free vertex is connected to the fixed one.
 *
 * orbg_eg_graph_create plans a graph once, on the host: a deterministic minimum-degree
 * elimination order, the 7x7 block pattern of the factor L including fill, and the lists the
 * kernels sum in a fixed order.  orbg_eg_graph_info reports the free vertices and the blocks
 * of H and of L (lower triangles, diagonals included).  ORBG_ENOTSUP for more than 262144
 * blocks of H or of L, more than 2^24 block updates in the factorisation, or more than 2^26
 * edges.  ORBG_EINVAL for a NULL pointer, nvert < 1, an edge index outside [0, nvert),
 * i == j, a kind other than 0 or 1, a fixed_vertex outside [0, nvert).
 *
 * orbg_eg_graph_optimize: d_Scw / d_Snc [nvert] in device memory; the LM loop runs on the
 * host over state in HBM and reads three scalars per trial (chi2 = sum e^T e, computeScale,
 * the solver's ok; fixed-order device reductions).  The solve is an LDL^T without pivoting in
 * one workgroup; a pivot that is not positive and finite makes the trial fail as g2o's failed
 * Cholesky does.  Outputs: d_Siw_out [nvert], the optimised estimates (the fixed vertex, and
 * under fix_scale every s, bit-identical to d_Scw), and d_Tiw_out [nvert][12] (may be NULL),
 * the 3x4 [R(q) | t * (1 / s)] of :1266-1286 rounded once to float.  nvert = 1, nedge = 0 or
 * iterations = 0 run no iteration: the input comes back (report->iterations = 0).
 * Synchronises.  Two runs give identical bytes. */
typedef struct {
    double q[4], t[3], s; /* q = x, y, z, w; never re-normalised, as g2o::Sim3 */
} orbg_sim3d;
typedef struct {
    int32_t i, j, kind; /* kind 0: measurement from Scw, 1: from Snc */
} orbg_eg_edge;
typedef struct orbg_eg_graph orbg_eg_graph;
int orbg_eg_graph_create(orbg_ctx *ctx, const orbg_eg_edge *edges, int nedge, int nvert,
                         int fixed_vertex, orbg_eg_graph **out);
int orbg_eg_graph_info(const orbg_eg_graph *graph, int32_t *nfree, int32_t *h_blocks,
                       int32_t *l_blocks);
int orbg_eg_graph_destroy(orbg_eg_graph *graph);
int orbg_eg_graph_optimize(orbg_ctx *ctx, orbg_eg_graph *graph, const orbg_sim3d *d_Scw,
                           const orbg_sim3d *d_Snc, int fix_scale, int iterations,
                           orbg_sim3d *d_Siw_out, float *d_Tiw_out, orbg_lm_report *report);
/* The map points' correction (:1288-1323), device memory: d_out[p] = correctedSwr.map(
 * Srw.map(d_points[p])) with Srw = d_Scw[d_ref[p]] and correctedSwr = d_Siw[d_ref[p]]^-1,
 * computed in double from the float position and rounded once.  d_ref[p] is the caller's
 * (mnCorrectedReference or the reference keyframe); one outside [0, nvert) leaves its point
 * as it is.  d_points / d_out: float [n][3], may be the same array.  Context stream, no host
 * synchronisation. */
int orbg_eg_correct_points_device(orbg_ctx *ctx, const orbg_sim3d *d_Scw, const orbg_sim3d *d_Siw,
                                  int nvert, const int32_t *d_ref, const float *d_points, int n,
                                  float *d_out);
/* One call from host arrays: plans, uploads, optimises, downloads (Siw_out [nvert], Tiw_out
 * [nvert][12] or NULL).  Bit-identical to the graph entry points.  An error return leaves the
 * outputs untouched. */
int orbg_optimize_essential_graph(orbg_ctx *ctx, const orbg_sim3d *Scw, const orbg_sim3d *Snc,
                                  int nvert, const orbg_eg_edge *edges, int nedge,
                                  int fixed_vertex, int fix_scale, int iterations,
                                  orbg_sim3d *Siw_out, float *Tiw_out, orbg_lm_report *report);

/* ---------------- LoopClosing::CorrectLoop on the Map ----------------
 * src/LoopClosing.cc:744-843 and 882-911 on an orbg_map: the state CorrectLoop reads beside
 * the observation table, the Sim3 propagation with its map-point loop, LoopConnections, the
 * walk that turns the map into OptimizeEssentialGraph's arrays (Optimizer.cc:1040-1258) and
 * the application of the optimised poses (:1264-1323), the loop fusion and SearchAndFuse
 * (:848-878), and orbg_map_correct_loop, which chains them.  Pointer order is slot order.
 *
 * State, all with defaults, so a map that never receives any of it behaves as before:
 *  - per slot a pose Tcw (3x4 float, row-major), a "has a pose" flag (0 after create / clear)
 *    and mnId (the slot itself after create / clear).  Setting a pose is KeyFrame::SetPose: it
 *    also rewrites the camera centre the map stores, Ow = -Rcw^T tcw as the float cv::Mat
 *    product (sums in double over k = 0, 1, 2 in order, one rounding to float).  d_Tcw or
 *    d_mnid may be NULL (not both): that half is left as it is.  orbg_map_set_keyframe[s]
 *    does not touch pose or mnId, and a later centre given there overwrites Ow.
 *  - per slot mspLoopEdges, at most ORBG_MAP_MAX_LOOP_EDGES entries.  orbg_map_add_loop_edge
 *    adds b to a's set and a to b's; an edge already there is not added again; ORBG_ERANGE,
 *    nothing changed, when either side is full.  orbg_map_get_loop_edges: ascending slot.
 *    erase_keyframe / set_bad_flag leave the edges alone; orbg_map_clear empties them.
 *  - per point mnCorrectedByKF and mnCorrectedReference (mnId values, 0 after create / clear).
 *
 * orbg_map_propagate[_device] (:744-843 without the loop fusion): UpdateConnections(cur);
 * mvpCurrentConnectedKFs = cur's ordered list followed by cur (d_set, its length in
 * d_nset[0]; entries past it up to set_cap are -1); per member i NonCorrectedSim3 =
 * Sim3(Riw, tiw, 1) and CorrectedSim3 = Sim3(Ric, tic, 1) * Scw, where Tic = Tiw * Twc is the
 * float cv::Mat product (double sums over the four terms, one rounding), Sim3(R, t, 1) takes
 * Eigen's Quaterniond(R) without normalisation and the product is g2o's in double;
 * CorrectedSim3[cur] = Scw.  Both go to tables indexed by SLOT ([max_keyframes]; other entries
 * are not written).  Then the map-point loop over CorrectedSim3 in slot order: a good point
 * whose mnCorrectedByKF is not cur's mnId is moved by the LOWEST member slot that holds it,
 * P = CorrectedSwi.map(Siw.map(P)) in double from the float position, rounded once; its
 * mnCorrectedByKF becomes cur's mnId, its mnCorrectedReference that member's mnId, and its
 * UpdateNormalAndDepth runs at that moment: for a point owned by member i an observing
 * keyframe t contributes its corrected camera centre iff t is a member and t < i (its SetPose
 * has run), else the centre it had; the reference keyframe's centre follows the same rule.
 * Then SetPose([R(q) | t * (1 / s)]) and UpdateConnections per member.
 * d_status [4]: [0] = ORBG_LOOP_* bits, [1] = the set's full length.  With a bit set only
 * UpdateConnections(cur) has run, d_nset[0] = 0 and the tables are not written.  The host form
 * returns ORBG_EINVAL for a cur that is not live or a member without a pose, ORBG_ERANGE for
 * a set longer than set_cap, and then leaves its outputs untouched; ORBG_EINVAL for a slot out
 * of range or a NULL pointer, ORBG_ENOTSUP for set_cap > ORBG_MAP_MAX_LOOP_SET.
 *
 * orbg_map_loop_connections[_device] (:882-911): for the members in VECTOR order, one after
 * another: snapshot of the ordered list, UpdateConnections, then the non-zeros of the W row
 * minus the snapshot minus the set.  The order matters: an earlier member's AddConnection can
 * re-sort a later member's list over all its non-zero weights, the sub-threshold ones
 * included, and those then drop out of that member's result.  d_pairs: (i, j) slot pairs,
 * grouped by i in ascending slot, j ascending (the map-of-sets' iteration order); d_npairs[0]
 * the full count, the first pair_cap pairs written.  A slot repeated in the set is processed
 * each time and reported once, from its last entry.
 *
 * The device forms run on the context stream and never synchronise: the set's length stays on
 * the device and the launches are sized by set_cap.  LoopConnections' workspace belongs to the
 * map and is allocated by the first call. */
#define ORBG_MAP_MAX_LOOP_EDGES 16
#define ORBG_MAP_MAX_LOOP_SET 256
#define ORBG_LOOP_NO_POSE 1
#define ORBG_LOOP_SET_RANGE 2
#define ORBG_LOOP_DEAD 4
int orbg_map_set_keyframe_poses_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_slots, int n,
                                       const float *d_Tcw, const int32_t *d_mnid);
int orbg_map_set_keyframe_poses(orbg_ctx *ctx, orbg_map *map, const int32_t *slots, int n,
                                const float *Tcw, const int32_t *mnid);
/* slots first .. first + n - 1; any output may be NULL.  centres [n][3]: the stored Ow */
int orbg_map_get_keyframe_poses(orbg_ctx *ctx, orbg_map *map, int first, int n, float *Tcw,
                                int32_t *has_pose, int32_t *mnid, float *centres);
int orbg_map_add_loop_edge(orbg_ctx *ctx, orbg_map *map, int a, int b);
int orbg_map_get_loop_edges(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *slots, int cap,
                            int32_t *n);
int orbg_map_get_point_corrected(orbg_ctx *ctx, orbg_map *map, int first, int n,
                                 int32_t *corrected_by_kf, int32_t *corrected_reference);
/* for a map uploaded from host state that carries earlier corrections */
int orbg_map_set_point_corrected(orbg_ctx *ctx, orbg_map *map, int first, int n,
                                 const int32_t *corrected_by_kf, const int32_t *corrected_reference);
int orbg_map_propagate_device(orbg_ctx *ctx, orbg_map *map, int cur, const orbg_sim3d *d_Scw,
                              int32_t *d_set, int set_cap, int32_t *d_nset,
                              orbg_sim3d *d_corrected, orbg_sim3d *d_noncorrected,
                              int32_t *d_status);
int orbg_map_propagate(orbg_ctx *ctx, orbg_map *map, int cur, const orbg_sim3d *Scw, int32_t *set,
                       int set_cap, int32_t *nset, orbg_sim3d *corrected,
                       orbg_sim3d *noncorrected);
int orbg_map_loop_connections_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_set,
                                     int set_cap, const int32_t *d_nset, int32_t *d_pairs,
                                     int pair_cap, int32_t *d_npairs);
/* CorrectLoop's loop fusion (:848-863), keyframes attached: d_matched [n] is
 * mvpCurrentMatchedPoints as ids (-1 = none), walked in feature order over the first min(n, N)
 * features of cur.  A held point is Replace()d by the matched one (MapPoint::Replace's own
 * returns apply: the same point, a matched point that is bad); a free feature takes the
 * matched point unless cur already holds it (AddObservation returns then).  The descriptors
 * of the matched points that were used are recomputed once when the call ends (the rule of
 * orbg_map_replace_device).  d_counts [2]: replaced, added.
 *
 * SearchAndFuse (:944-992), keyframes attached: for the members of the set in SLOT order, one
 * after another, Fuse(pKF, Scw, d_loop_points, th, vpReplacePoints) and then the Replace loop.
 * The search is orbg_fuse_sim3_batch_device's kernel; its camera is d_cams[slot] with the
 * member's corrected Sim3 as Tcw ([s R | t] rounded to float); its inputs are gathered from the
 * map as orbg_map_fuse_device gathers them (a point in the row or a bad point is not valid).
 * The update, in list order: a free feature takes the point; a good point on the feature is
 * recorded; after the list the recorded points are Replace()d by their loop points, in order.
 * A later member's search sees the rows and flags the earlier members left.  d_counts [2]: the
 * sum of nFused, the replacements.  ORBG_EINVAL when nothing is attached.  set_cap sequences of
 * launches are issued whatever the set's length: size set_cap tightly (LoopConnections too). */
int orbg_map_loop_fusion_device(orbg_ctx *ctx, orbg_map *map, int cur, const int32_t *d_matched, int n,
                                int32_t *d_counts);
int orbg_map_loop_fusion(orbg_ctx *ctx, orbg_map *map, int cur, const int32_t *matched, int n,
                         int32_t *counts);
int orbg_map_search_and_fuse_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_set, int set_cap,
                                    const int32_t *d_nset, const orbg_sim3d *d_corrected,
                                    const int32_t *d_loop_points, int n, float th, int32_t *d_counts);
int orbg_map_search_and_fuse(orbg_ctx *ctx, orbg_map *map, const int32_t *set, int nset,
                             const orbg_sim3d *corrected, const int32_t *loop_points, int n, float th,
                             int32_t *counts);
/* host arrays; ORBG_ERANGE when there are more than pair_cap pairs */
int orbg_map_loop_connections(orbg_ctx *ctx, orbg_map *map, const int32_t *set, int nset,
                              int32_t *pairs, int pair_cap, int32_t *npairs);
/* The walk of Optimizer::OptimizeEssentialGraph over the map (src/Optimizer.cc:1040-1258): the
 * arrays orbg_eg_graph_create / orbg_eg_graph_optimize take.  Inputs: cur, loop, the two Sim3
 * tables of Propagate with the set that says which of their entries exist, the LoopConnections
 * pairs.  Vertices: the live, not-bad slots in ascending slot order (d_vert_slot [max_keyframes],
 * d_nvert[0]); d_fixed[0] = loop's vertex.  d_Scw[v] = CorrectedSim3 of the slot where the set
 * has it, else Sim3(Rcw, tcw, 1) of the stored pose; d_Snc[v] = NonCorrectedSim3 where the set
 * has the slot, else d_Scw[v].  Edges {i, j, kind} with i the EdgeSim3's vertex 0, in the
 * reference's order:
 *  - kind 0: the pairs in their order; a pair is kept iff W[i][j] >= 100 or (mnId of i, mnId of
 *    j) = (cur's, loop's); each kept pair enters sInsertedEdges as (min mnId, max mnId);
 *  - kind 1, per vertex in slot order: the parent; the loop edges with a lower mnId, ascending
 *    slot; then GetCovisiblesByWeight(100), which is the entries of the ordered list before the
 *    first weight below 100 and, as in the reference (KeyFrame.cc:237-241), EMPTY when no
 *    weight of the list is below 100: an entry gives an edge iff it is not the parent, not a
 *    child (its parent is not this slot), not a loop edge, a vertex, has a lower mnId and the
 *    pair is not in sInsertedEdges.
 * The one departure: an edge whose other end is not a vertex (a parent or loop-edge keyframe
 * that is dead or bad, a pair with such an end) is left out and counted in d_status[1]; the
 * reference dereferences NULL there.  d_status[0]: ORBG_LOOP_DEAD when loop is no vertex,
 * ORBG_LOOP_NO_POSE when a vertex outside the set has no pose (the host form: ORBG_EINVAL,
 * outputs untouched).  d_nedge[0] is the full count, the first edge_cap edges are written (the
 * host form: ORBG_ERANGE past edge_cap).  ORBG_EINVAL for cur / loop out of range, cur == loop,
 * NULL pointers.  Counts are per vertex, scanned, then emitted: the order needs no atomics. */
int orbg_map_essential_graph_device(orbg_ctx *ctx, orbg_map *map, int cur, int loop,
                                    const orbg_sim3d *d_corrected, const orbg_sim3d *d_noncorrected,
                                    const int32_t *d_set, int set_cap, const int32_t *d_nset,
                                    const int32_t *d_pairs, int pair_cap, const int32_t *d_npairs,
                                    int32_t *d_vert_slot, int32_t *d_nvert, int32_t *d_fixed,
                                    orbg_sim3d *d_Scw, orbg_sim3d *d_Snc, orbg_eg_edge *d_edges,
                                    int edge_cap, int32_t *d_nedge, int32_t *d_status);
int orbg_map_essential_graph(orbg_ctx *ctx, orbg_map *map, int cur, int loop,
                             const orbg_sim3d *corrected, const orbg_sim3d *noncorrected,
                             const int32_t *set, int nset, const int32_t *pairs, int npairs,
                             int32_t *vert_slot, int32_t *nvert, int32_t *fixed, orbg_sim3d *Scw,
                             orbg_sim3d *Snc, orbg_eg_edge *edges, int edge_cap, int32_t *nedge,
                             int32_t *nskipped);
/* Optimizer.cc:1264-1323 with the optimiser's outputs (orbg_eg_graph_optimize's d_Siw_out /
 * d_Tiw_out, vertex-indexed as d_vert_slot): SetPose(Tiw[v]) for every vertex; then every good
 * point p moves to correctedSwr.map(Srw.map(P)) through orbg_eg_correct_points_device's
 * kernel, Srw = d_Scw[r], correctedSwr = d_Siw[r]^-1, r the vertex of mnCorrectedReference's
 * keyframe if mnCorrectedByKF is cur's mnId, else of the reference keyframe (a point whose r is
 * no vertex stays); then UpdateNormalAndDepth of all points.  The workspace belongs to the map
 * and is allocated by the first call. */
int orbg_map_apply_correction_device(orbg_ctx *ctx, orbg_map *map, int cur,
                                     const int32_t *d_vert_slot, const int32_t *d_nvert,
                                     const orbg_sim3d *d_Scw, const orbg_sim3d *d_Siw,
                                     const float *d_Tiw);
int orbg_map_apply_correction(orbg_ctx *ctx, orbg_map *map, int cur, const int32_t *vert_slot,
                              int nvert, const orbg_sim3d *Scw, const orbg_sim3d *Siw,
                              const float *Tiw);
/* LoopClosing::CorrectLoop from mg2oScw to the corrected poses and points in one host call,
 * keyframes attached: Propagate, the loop fusion with `matched` (mvpCurrentMatchedPoints),
 * SearchAndFuse with `loop_points` (mvpLoopMapPoints, th 4), LoopConnections, the essential
 * graph, orbg_eg_graph_create / orbg_eg_graph_optimize (20 iterations), Apply and
 * AddLoopEdge(loop, cur).  counts [8]: set members, fusion replaced / added, SearchAndFuse
 * nFused / replaced, LoopConnections pairs, vertices, edges.  Errors as the stages'; a failure
 * after Propagate leaves the map as that stage left it.  Synchronises; allocates and frees its
 * own device workspace. */
int orbg_map_correct_loop(orbg_ctx *ctx, orbg_map *map, int cur, int loop, const orbg_sim3d *Scw,
                          const int32_t *matched, int nmatched, const int32_t *loop_points,
                          int nloop, int fix_scale, orbg_lm_report *report, int32_t *counts);

/* ---- Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) on the Map ----
 * src/Optimizer.cc:633-979 in three stages and one chaining call.  The keyframe data must be
 * attached (orbg_map_attach_keyframes: mvKeysUn, mvuRight, the cameras) and every window
 * keyframe needs a pose (orbg_map_set_keyframe_poses).  The `_device` forms run on the context
 * stream without synchronising and allocate nothing after the first call of a size; the host
 * forms take host arrays and synchronise.  Pointer order is slot order.
 *
 * The window (:635-851), exactly what the compat layer's build_lba_window produces from the
 * reference's three lists:
 *   kf_slots [npose]   nlocal local keyframes (slot, then its ordered covisibility list without
 *                      the ORBG_MAP_KF_BAD entries), then the fixed cameras in order of first
 *                      appearance over the local points (list order) and each point's observers
 *                      (ascending slot); a bad observer is listed nowhere.
 *   point_ids [npoint] the good points of the local rows, rows in list order, features in order,
 *                      each at its first occurrence.
 *   poses [npose]      Converter::toSE3Quat(kf_Tcw) in double from the float entries (Eigen's
 *                      branch, w >= 0, one normalisation); fixed = 1 for the fixed part and mnId 0.
 *   points [npoint][3] the stored float positions as doubles.
 *   edges [nedge], edge_feat [nedge]
 *                      per local point, per observer that is not bad (ascending slot): stereo =
 *                      mvuRight[idx] >= 0 (no mvuRight attached: mono), obs from mvKeysUn[idx] and
 *                      mvuRight[idx], inv_sigma2 = mvInvLevelSigma2[octave] (a float, widened),
 *                      the intrinsics of the attached camera, huber_delta = (float)sqrt(5.991) /
 *                      (float)sqrt(7.815), robust = active = 1; edge_feat = idx.
 *   counts [4]         nlocal, npose, npoint, nedge: always the full counts.
 *   status [4]         [0] = ORBG_LBA_* bits.
 * Nothing in the Map changes.  point_cap <= 524286.  The host form returns ORBG_ERANGE when a cap
 * is exceeded (counts hold what is needed) and ORBG_EINVAL for a dead slot, nothing attached, a
 * window keyframe without a pose or an observation whose feature index is past the attached
 * count. */
#define ORBG_LBA_NO_POSE 1
#define ORBG_LBA_RANGE 2
#define ORBG_LBA_DEAD 4
#define ORBG_LBA_FEATURE 8
int orbg_map_lba_window_device(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *d_kf_slots,
                               orbg_pose *d_poses, int pose_cap, int32_t *d_point_ids,
                               double *d_points, int point_cap, orbg_edge *d_edges,
                               int32_t *d_edge_feat, int edge_cap, int32_t *d_counts,
                               int32_t *d_status);
int orbg_map_lba_window(orbg_ctx *ctx, orbg_map *map, int slot, int32_t *kf_slots, orbg_pose *poses,
                        int pose_cap, int32_t *point_ids, double *points, int point_cap,
                        orbg_edge *edges, int32_t *edge_feat, int edge_cap, int32_t *counts);
/* The write-back (:943-978) of a window (its arrays as above, d_counts as the window left them;
 * the edges of one point are adjacent, as the window emits them), the optimised d_poses /
 * d_points and the vToErase flags d_erase [nedge]:
 *   erasures  per flagged edge, mono edges first and then stereo edges, each in edge order:
 *             EraseMapPointMatch (the row entry becomes -1) and MapPoint::EraseObservation as
 *             KeyFrameCulling states it (Observations() less 2 for an ORBG_MAP_FEAT_STEREO
 *             feature, else 1; mpRefKF moves to the lowest remaining observing slot; at
 *             Observations() <= 2 the point goes bad and leaves every row).  A flag on an edge
 *             whose point has gone bad earlier in the call does nothing;
 *   poses     SetPose(Converter::toCvMat(pose)) of the first nlocal keyframes, mnId 0 included,
 *             the centres as orbg_map_set_keyframe_poses writes them;
 *   points    every window point's position = (float) of its estimate, bad or not; then
 *             UpdateNormalAndDepth of the window's points over the rebuilt observation index;
 *   cameras   d_cams_out (may be NULL): the Tcw of the local keyframes' entries is rewritten,
 *             nothing else.
 * W and the ordered lists do not change.  d_out [2]: erased observations, points gone bad. */
int orbg_map_lba_apply_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_kf_slots, int pose_cap,
                              const int32_t *d_point_ids, int point_cap, const orbg_edge *d_edges,
                              const int32_t *d_edge_feat, int edge_cap, const int32_t *d_counts,
                              const orbg_pose *d_poses, const double *d_points,
                              const uint8_t *d_erase, orbg_frustum_camera *d_cams_out,
                              int32_t *d_out);
int orbg_map_lba_apply(orbg_ctx *ctx, orbg_map *map, const int32_t *kf_slots, int nlocal, int npose,
                       const int32_t *point_ids, int npoint, const orbg_edge *edges,
                       const int32_t *edge_feat, int nedge, const orbg_pose *poses,
                       const double *points, const uint8_t *erase,
                       orbg_frustum_camera *d_cams_out, int32_t *out);
/* All of it: the window, the stop check (control->force_stop raised: stopped = 1 and nothing
 * written, :853-855), orbg_local_ba_optimize's optimisation on the window's device arrays (the
 * estimates never reach the host; the edge records are read once for orbg_ba_graph_create; the
 * outlier and vToErase decisions stay host reads of chi2 / depth), the write-back.  The workspace
 * belongs to the map and grows on demand.  An empty edge set optimises nothing and still
 * applies.  ORBG_ENOTSUP of orbg_ba_graph_create is returned with the Map untouched. */
typedef struct {
    orbg_lba_report lba;
    int32_t nlocal, nfixed, npoints, nedges;
    int32_t nerased, npoints_bad;  /* observations erased, points gone bad by erasure */
    int32_t stopped, pad;
} orbg_map_lba_report;
int orbg_map_local_ba(orbg_ctx *ctx, orbg_map *map, int slot, const orbg_lm_control *control,
                      orbg_frustum_camera *d_cams_out, orbg_map_lba_report *report);

/* ---------------- GlobalBundleAdjustment (Optimizer::BundleAdjustment) ----------------
 * src/Optimizer.cc:105-320: every keyframe a VertexSE3Expmap (fixed iff mnId == 0), every map
 * point a marginalised VertexSBAPointXYZ, one EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ per
 * observation (Huber deltas sqrt(5.99) / sqrt(7.815) when bRobust), BlockSolver_6_3 under
 * OptimizationAlgorithmLevenberg, optimize(nIterations) with the force-stop flag.  Called by
 * Tracking::CreateInitialMapMonocular (20 iterations, robust) and LoopClosing::
 * RunGlobalBundleAdjustment (10 iterations, &mbStopGBA, not robust).  The edge types, the
 * build, the error pass and the LM are LocalBundleAdjustment's (orbg_ba_graph above); what
 * differs is the reduced camera system: every pose but one is free, so it is kept and
 * factorised as a block-sparse matrix instead of orbg_ba_graph_schur_plan's dense one.
 *
 * orbg_ba_graph_schur_plan_sparse: the graph's second plan kind.  On the host it takes the
 * 6x6 block pattern of S (a block per pair of free poses sharing an active landmark), orders
 * the free poses by minimum degree (the smallest index on ties), finds the pattern of the
 * factor L by symbolic elimination, the list of updates of every block, and a level for every
 * column (greater than the level of every column in its row of L): columns of one level are
 * independent.  orbg_ba_graph_schur_solve / _optimize / _optimize_ctl then use it (they use
 * whichever plan the graph holds; orbg_ba_graph_set_active rebuilds the plan of the same
 * kind): S is written straight into L's pattern and factorised L D L^T without pivoting, one
 * launch per level with a workgroup per column, one workgroup for the single-column levels at
 * the top of the elimination tree; a pivot that is not positive and finite gives *d_ok = 0
 * and zero increments.  Every sum has a fixed order: two solves give identical bytes (they
 * are not the dense plan's bytes: another elimination order).  info (may be NULL) receives
 * the plan's figures.  ORBG_ENOTSUP past ORBG_GBA_MAX_L_BLOCKS blocks of L (288 bytes each:
 * 576 MiB) or ORBG_GBA_MAX_UPDATES block updates (16 bytes each: 1 GiB).  The caps are set
 * by memory alone: how many blocks the global BA of a real map has, has not been measured. */
#define ORBG_GBA_MAX_L_BLOCKS (1 << 21)
#define ORBG_GBA_MAX_UPDATES (1 << 26)
typedef struct orbg_ba_sparse_info {
    int32_t nfree;        /* free poses = block columns */
    int32_t s_blocks;     /* blocks of S, lower triangle with the diagonals */
    int32_t l_blocks;     /* blocks of L: s_blocks + fill */
    int32_t levels;       /* levels of the schedule */
    int32_t tail_columns; /* columns of the single-column levels at the top (one workgroup) */
    int32_t pad;
    int64_t updates;      /* block updates L(r,k) D(k) L(j,k)^T of one factorisation */
} orbg_ba_sparse_info;
int orbg_ba_graph_schur_plan_sparse(orbg_ctx *ctx, orbg_ba_graph *graph, const uint8_t *fixed,
                                    orbg_ba_sparse_info *info);
/* The symbolic work alone, on the host (no context, no device): edges as parallel arrays
 * (pose, point, active), fixed [npose].  order_out [nfree]: the free poses (pose indices) in
 * elimination order; colptr_out [nfree + 1] / rowidx_out [cap]: L by columns in elimination
 * positions, rows ascending, the diagonal first; level_out [nfree]: the level of each column.
 * Any output array may be NULL; rowidx_out with cap < info->l_blocks: ORBG_EINVAL (info is
 * filled).  Errors as above. */
int orbg_ba_sparse_symbolic(const int32_t *epose, const int32_t *epoint, const uint8_t *eactive,
                            int nedge, int npose, int npoint, const uint8_t *fixed,
                            int32_t *order_out, int32_t *colptr_out, int32_t *rowidx_out, int cap,
                            int32_t *level_out, orbg_ba_sparse_info *info);
/* Optimizer::BundleAdjustment's optimisation (Optimizer.cc:113-247) from host arrays: creates
 * the graph (edges as orbg_ba_graph_create; active / robust as given), makes the sparse plan
 * with poses[i].fixed, runs optimize(iterations) under control->force_stop (control may be
 * NULL; d_last_chi2 is honoured), and overwrites poses / points with the estimates.  A fixed
 * pose, and a point without an active edge, come back byte for byte.  nedge = 0: nothing runs
 * (report zero).  Equal to the graph entry points on the same arrays, byte for byte. */
typedef struct {
    orbg_lm_report lm;
    orbg_ba_sparse_info plan;
} orbg_gba_report;
int orbg_global_ba_optimize(orbg_ctx *ctx, orbg_pose *poses, int npose, double *points, int npoint,
                            const orbg_edge *edges, int nedge, int iterations,
                            const orbg_lm_control *control, orbg_gba_report *report);
/* The map points global BA did not optimise (LoopClosing.cc:1101-1113): Xc = Rcw X + tcw with
 * the reference keyframe's mTcwBefGBA, then Rwc Xc + twc with its GetPoseInverse(), both in
 * float by the cv::Mat rule (R * X + t is one cv::gemm: each entry's three products and t
 * accumulated in double, rounded once).  d_Tcw_before / d_Twc_after: float [nkf][12] (3x4, row-major); d_ref[p]
 * the reference keyframe's index, one outside [0, nkf) (a keyframe global BA did not reach)
 * leaves the point as it is.  d_points / d_out: float [n][3], may be the same array.  Context
 * stream, no host synchronisation. */
int orbg_gba_correct_points_device(orbg_ctx *ctx, const float *d_Tcw_before,
                                   const float *d_Twc_after, int nkf, const int32_t *d_ref,
                                   const float *d_points, int n, float *d_out);

/* ---- Optimizer::GlobalBundleAdjustemnt(pMap, ...) and RunGlobalBundleAdjustment on the Map ----
 * src/Optimizer.cc:105-320 and src/LoopClosing.cc:1024-1128 in three stages and two chaining
 * calls.  The keyframe data must be attached (orbg_map_attach_keyframes: mvKeysUn, mvuRight, the
 * cameras) and every keyframe that is not bad needs a pose.  The `_device` forms run on the
 * context stream without synchronising and allocate nothing after the first call on a map; the
 * host forms take host arrays and synchronise.  Pointer order is slot order / id order.
 *
 * State the Map holds for it.  Per slot mTcwGBA and mTcwBefGBA (float [12], 3x4 row-major) and
 * KeyFrame::mnBAGlobalForKF (int32); per point mPosGBA (float [3]) and MapPoint::mnBAGlobalForKF.
 * Both mnBAGlobalForKF are 0 after orbg_map_create / orbg_map_clear; a slot that becomes live
 * (orbg_map_set_keyframe[s] on a slot that was not live, orbg_map_process_new_keyframe) and a
 * point created by orbg_map_create_new_points[_device] start with 0.  A map that never uses them
 * behaves as before.  set / get copy the ranges [first_slot, first_slot + nslots) and
 * [first_point, first_point + npoints); any array may be NULL (that part is left alone). */
int orbg_map_set_gba_state(orbg_ctx *ctx, orbg_map *map, int first_slot, int nslots,
                           const float *TcwGBA, const float *TcwBefGBA, const int32_t *kf_ba_global,
                           int first_point, int npoints, const float *PosGBA,
                           const int32_t *mp_ba_global);
int orbg_map_get_gba_state(orbg_ctx *ctx, orbg_map *map, int first_slot, int nslots, float *TcwGBA,
                           float *TcwBefGBA, int32_t *kf_ba_global, int first_point, int npoints,
                           float *PosGBA, int32_t *mp_ba_global);
/* The flags of slots first .. first + n - 1 (host): ORBG_MAP_KF_ROOT | ORBG_MAP_KF_BAD, and 4 for a
 * live slot.  The live ORBG_MAP_KF_ROOT slots are what a caller without its own list passes as
 * mvpKeyFrameOrigins. */
int orbg_map_get_keyframe_flags(orbg_ctx *ctx, orbg_map *map, int first, int n, int32_t *flags);
/* The window (Optimizer.cc:113-246), exactly what the compat layer's
 * orbg_compat::ref::BundleAdjustment builds from GetAllKeyFrames() / GetAllMapPoints() of the same
 * map:
 *   kf_slots [npose]   the slots that are live and not ORBG_MAP_KF_BAD, ascending.
 *   poses [npose]      Converter::toSE3Quat(kf_Tcw) as orbg_map_lba_window computes it; fixed = 1
 *                      iff the stored mnId is 0 (the slot does not decide it).
 *   point_ids [npoint] the ORBG_MP_VALID points with at least one edge, ascending id.  A good point
 *                      whose observers are all bad or absent is left out (vbNotIncludedMP, :236-244).
 *   points [npoint][3] the stored float positions as doubles.
 *   edges [nedge], edge_feat [nedge]
 *                      per window point, per observer that is live and not bad (ascending slot),
 *                      every field as orbg_map_lba_window fills it, except robust = the argument
 *                      and huber_delta = (float)sqrt(5.99) / (float)sqrt(7.815) (:157-158: 5.99, not
 *                      5.991).  pose and point index the two lists.  The reference's other test,
 *                      mnId > maxKFid (:184), can never hold for a keyframe that is not bad.
 *   counts [4]         npose, npoint, nedge, the good points left out: always the full counts.
 *   status [4]         [0] = ORBG_LBA_NO_POSE | ORBG_LBA_RANGE | ORBG_LBA_FEATURE bits.
 * Nothing in the Map changes.  The host form returns ORBG_ERANGE when a cap is exceeded (counts
 * hold what is needed) and ORBG_EINVAL for nothing attached, a vertex keyframe without a pose or
 * an observation whose feature index is past the attached count. */
int orbg_map_gba_window_device(orbg_ctx *ctx, orbg_map *map, int robust, int32_t *d_kf_slots,
                               orbg_pose *d_poses, int pose_cap, int32_t *d_point_ids,
                               double *d_points, int point_cap, orbg_edge *d_edges,
                               int32_t *d_edge_feat, int edge_cap, int32_t *d_counts,
                               int32_t *d_status);
int orbg_map_gba_window(orbg_ctx *ctx, orbg_map *map, int robust, int32_t *kf_slots,
                        orbg_pose *poses, int pose_cap, int32_t *point_ids, double *points,
                        int point_cap, orbg_edge *edges, int32_t *edge_feat, int edge_cap,
                        int32_t *counts);
/* The store (:273-318) of a window's kf_slots / point_ids (d_counts as the window left them) and
 * the optimised d_poses / d_points.  A keyframe that has gone bad or dead and a point that has
 * gone bad since the window was built are skipped (:279, :303).
 *   loop_kf == 0   SetPose(Converter::toCvMat(pose)) of every window keyframe, the fixed one
 *                  included, the centres as orbg_map_set_keyframe_poses writes them, the Tcw of
 *                  their entries in d_cams_out (may be NULL); then SetWorldPos((float) estimate)
 *                  of every window point and UpdateNormalAndDepth over the current observation
 *                  index.
 *   loop_kf != 0   mTcwGBA = that pose, mPosGBA = that position, both mnBAGlobalForKF = loop_kf.
 *                  Poses, centres, positions, normals and rows do not change.
 * d_out [2]: keyframes written, points written. */
int orbg_map_gba_store_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_kf_slots, int pose_cap,
                              const int32_t *d_point_ids, int point_cap, const int32_t *d_counts,
                              const orbg_pose *d_poses, const double *d_points, int loop_kf,
                              orbg_frustum_camera *d_cams_out, int32_t *d_out);
int orbg_map_gba_store(orbg_ctx *ctx, orbg_map *map, const int32_t *kf_slots, int npose,
                       const int32_t *point_ids, int npoint, const orbg_pose *poses,
                       const double *points, int loop_kf, orbg_frustum_camera *d_cams_out,
                       int32_t *out);
/* The map update of RunGlobalBundleAdjustment (LoopClosing.cc:1056-1116).  origins [norigins]:
 * mvpKeyFrameOrigins as slots.
 *   keyframes  The walk visits every slot reachable from an origin over the children lists (the
 *              slots whose parents lead to an origin).  It does not look at ORBG_MAP_KF_BAD, as
 *              the reference does not; a dead slot ends it.  A visited child whose
 *              mnBAGlobalForKF != loop_kf gets mTcwGBA = (Tcw_child * Twc_parent) * mTcwGBA_parent
 *              and mnBAGlobalForKF = loop_kf: both products the 4x4 float cv::Mat product (each
 *              entry's terms summed in double over k in order, rounded once to float; the
 *              intermediate is a float matrix), Twc_parent = [Rcw^T | Ow] with the stored Ow, both
 *              poses the ones from before this call.  Every visited keyframe then gets
 *              mTcwBefGBA = Tcw, SetPose(mTcwGBA) and its Tcw in d_cams_out (may be NULL).  The
 *              result does not depend on the order in which the slots are handled.
 *   points     every good point: mnBAGlobalForKF == loop_kf: position = mPosGBA.  Otherwise, when
 *              its reference keyframe was visited: orbg_gba_correct_points_device's move with that
 *              keyframe's mTcwBefGBA and its GetPoseInverse() after the walk.  Otherwise it stays.
 *              No UpdateNormalAndDepth: the reference runs none here.
 *   departure  a point whose reference keyframe is -1, is dead, or carries loop_kf but was not
 *              visited in this call stays where it is and is counted; the reference dereferences
 *              a null pointer or reads a stale mTcwBefGBA there.
 * d_out [6]: keyframes visited, of them propagated, points set from mPosGBA, points moved, points
 * skipped by the departure, 0.  d_status [4]: [0] = ORBG_GBA_* bits; when one is set nothing is
 * written.  ORBG_GBA_ORIGIN: an origin is no slot, is dead, has no pose or has
 * mnBAGlobalForKF != loop_kf.  ORBG_GBA_CYCLE: the parents of live slots form a cycle (a walk of
 * more than max_keyframes steps).  ORBG_GBA_NO_POSE: a visited keyframe has no pose.  The host form
 * returns ORBG_EINVAL for any of them and for loop_kf == 0 (both forms). */
#define ORBG_GBA_ORIGIN 1
#define ORBG_GBA_CYCLE 2
#define ORBG_GBA_NO_POSE 4
int orbg_map_gba_update_device(orbg_ctx *ctx, orbg_map *map, const int32_t *d_origins, int norigins,
                               int loop_kf, orbg_frustum_camera *d_cams_out, int32_t *d_out,
                               int32_t *d_status);
int orbg_map_gba_update(orbg_ctx *ctx, orbg_map *map, const int32_t *origins, int norigins,
                        int loop_kf, orbg_frustum_camera *d_cams_out, int32_t *out);
/* Optimizer::GlobalBundleAdjustemnt(pMap, iterations, control->force_stop, loop_kf, robust): the
 * window, orbg_global_ba_optimize's optimisation on the window's device arrays (the estimates
 * never reach the host; the edge records and the fixed flags are read once for
 * orbg_ba_graph_create and the sparse plan), the store.  The workspace belongs to the map and
 * grows on demand.  An empty edge set optimises nothing and stores nothing.  ORBG_ENOTSUP of the
 * plan is returned with the Map untouched.  The store runs whether or not force_stop was raised,
 * as in the reference.  control may be NULL.  Synchronises. */
typedef struct {
    orbg_gba_report gba;
    int32_t nposes, npoints, nedges, nleft_out; /* the window's counts */
    int32_t store[2];                           /* orbg_map_gba_store's d_out */
    int32_t update[6];                          /* orbg_map_gba_update's d_out */
    int32_t stopped, pad;
} orbg_map_gba_report;
int orbg_map_global_ba(orbg_ctx *ctx, orbg_map *map, int iterations, int robust, int loop_kf,
                       const orbg_lm_control *control, orbg_frustum_camera *d_cams_out,
                       orbg_map_gba_report *report);
/* LoopClosing::RunGlobalBundleAdjustment(loop_kf): orbg_map_global_ba with 10 iterations, not
 * robust, then the update unless *control->force_stop != 0 (:1040): then stopped = 1 and poses
 * and positions are untouched (the GBA state is stored).  ORBG_EINVAL for loop_kf == 0 and for
 * the update's status bits. */
int orbg_map_run_global_ba(orbg_ctx *ctx, orbg_map *map, const int32_t *origins, int norigins,
                           int loop_kf, const orbg_lm_control *control,
                           orbg_frustum_camera *d_cams_out, orbg_map_gba_report *report);

/* ---------------- Initializer (Tracking::MonocularInitialization) ----------------
 * src/Initializer.cc:73-187 and everything below it, batched over frame pairs:
 * Initializer::Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) with
 * Normalize (:984-1037), FindHomography / FindFundamental (:201-318), ComputeH21 / ComputeF21
 * (:328-412), CheckHomography / CheckFundamental (:424-597), ReconstructF (:614-722),
 * ReconstructH (:743-924), Triangulate (:939-973), CheckRT (:1056-1233) and DecomposeE
 * (:1245-1270).  Frame 1 is the reference frame, frame 2 the current one.
 *
 * Inputs per pair: the problem record (mK, sigma = 1.0 and iterations = mMaxIterations = 200 in
 * Tracking, minParallax = 1.0 and minTriangulated = 50 as :182-184 pass them), the undistorted
 * keypoints of both frames (orbg_keypoint: only pt is read), vMatches12 [n1] and the
 * eight-index sets.  The draws are an input, as in the other two solvers: the reference fills
 * mvSets before either model runs (:131-150), so sets[it][0 .. 8) serves both H and F.
 *
 * The device compacts mvMatches12 itself (:94-109): the pairs (i, vMatches12[i]) with
 * 0 <= vMatches12[i] < n2 in i order (an index >= n2 is no match); N is their number.
 * Normalize runs over all keys of each frame, matched or not (:210-211).  Departure: the
 * reference adds in a float running sum; here the four sums of a frame run in fp64 in a fixed
 * order (256 strided partial sums, then a binary tree) and mean = (float)(sum / n) is rounded
 * once; sX = (float)(1.0 / meanDevX) and T's entries are the reference's float expressions.
 *
 * Per iteration and model: A of ComputeH21 (16 x 9) / ComputeF21 (8 x 9) holds the reference's
 * float entries (CV_32F products).  From there the linear algebra is fp64 in a fixed operation
 * order with a fixed number of Jacobi sweeps: vt.row(8) is the eigenvector of least eigenvalue
 * of the 9 x 9 A^T A (cyclic Jacobi, round-robin ordering), which for F's 8 x 9 system is its
 * exact null vector, so no basis has to be completed; the 3 x 3 SVDs are one-sided Jacobi.
 * ComputeF21 drops the least singular value; H21i = T2inv Hn T1 and F21i = T2^T Fn T1 are
 * rounded to float once, as the reference holds CV_32F; H12i = H21i.inv() is taken of that float
 * matrix (adjugate over determinant in fp64) and rounded once.  The sign of a null vector is the SVD routine's choice in the
 * reference: H21i and H12i change sign together and both are only used as ratios of their rows,
 * F21i enters CheckFundamental as num^2 / (a^2 + b^2), E21's sign leaves the set {(R1, t),
 * (R2, t), (R1, -t), (R2, -t)} as it is, and A = K^-1 H21 K changes s, U or Vt by a sign that
 * cancels in s U Rp Vt and permutes the eight (R, t, n) among themselves, so no score, mask or
 * final result depends on it.  Which hypothesis index holds which motion does depend on the
 * signs of the 3 x 3 SVDs' vectors; here every right singular vector has its component of
 * largest magnitude positive, and DecomposeE takes u.col(2) = u.col(0) x u.col(1) and
 * vt.row(2) = vt.row(0) x vt.row(1) (E has rank 2; det R = +1 follows).  Even so an index is
 * not comparable with another implementation's: H21's sign reverses each group of four Faugeras
 * hypotheses, and E21's two nearly equal singular values let two SVD routines pair their
 * vectors, and so (R1, R2), differently.  R21, t21, the points and the chosen hypothesis'
 * counts are comparable.
 *
 * CheckHomography / CheckFundamental use the reference's float types and comparisons:
 * w2in1inv = (float)(1.0 / (double)(...)), invSigmaSquare = (float)(1.0 / (double)(sigma *
 * sigma)), chiSquare > th rejects (a NaN chi-square takes the else branch and makes the score
 * NaN), th = 5.991 for H, th = 3.841 and thScore = 5.991 for F.  Departure: a score is the
 * fixed-order fp64 sum of the float terms (lane l of 64 adds matches l, l + 64, ..., chiSquare1's
 * term before chiSquare2's; the 64 sums combine in a butterfly), rounded to float once.
 *
 * An iteration whose set holds an index outside [0, N) or a repeated one, whose matrix is not
 * finite, or whose H21i is singular scores 0 with an all-zero mask and matrix, and can never
 * win.  N < 8 runs nothing.
 *
 * A model's best iteration is the first strict maximum over scores from 0 (currentScore >
 * score: a NaN never wins), -1 if none.  RH = SH / (SH + SF) in float; RH > 0.40 selects
 * ReconstructH (model 1), otherwise ReconstructF (model 2).  Where neither model scored above
 * 0 the reference dereferences an empty matrix; here model = 0 and success = 0.
 *
 * ReconstructF: E21 = K^T F21 K, DecomposeE (t = u.col(2) / |t|, an R of negative determinant
 * negated), the four hypotheses (R1, t), (R2, t), (R1, -t), (R2, -t), nMinGood = max((int)(0.9
 * N), minTriangulated), the > 0.7 maxGood similarity count, the if / else-if chain and
 * parallax > minParallax exactly as written.  ReconstructH: A = K^-1 H21 K, its SVD, s =
 * det(U) det(Vt), the early return d1 / d2 < 1.00001 || d2 / d3 < 1.00001 in float, the eight
 * Faugeras hypotheses (in double, rounded once: the float expressions cancel in d1 - d3 and
 * leave an R that is no rotation when the singular values are close), best and second best with >, and
 * secondBestGood < 0.75 bestGood && bestParallax >= minParallax && bestGood > minTriangulated
 * && bestGood > 0.9 N.  The decompositions run in fp64 on the float matrices and U, w, Vt, R, t
 * are rounded to float once; matrix products of float matrices accumulate in double and round
 * once (the cv::gemm rule).
 *
 * CheckRT: one pass over the chosen model's inliers per hypothesis.  Triangulate's A holds the
 * reference's float entries; x3D is the right singular vector of least singular value of a
 * one-sided Jacobi in fp64, (float)(v[k] / v[3]).  Then in float, in the reference's order: the
 * isfinite test, cosParallax = (float)(dot / (double)(dist1 * dist2)) with dist = (float) of the
 * double norm, the two depth tests each paired with cosParallax < 0.99998, the two reprojection
 * tests against th2 = 4 sigma^2, vP3D[first] and nGood, vbGood[first] only when cosParallax <
 * 0.99998.  The parallax is the order statistic sorted(vCosParallax)[min(50, size - 1)], found
 * by an exact selection on the floats' ordered bit patterns, then (float)(acos((double)c) *
 * 180.0 / pi): the arc cosine in double, rounded once (the reference's float acos differs by an
 * ulp at most).  A cosine above 1 gives NaN and fails >, as in the reference.
 *
 * No atomics and no order-dependent float reduction: results are identical run to run and
 * independent of the batch a pair is put in. */
#define ORBG_INIT_MAX_N 8192
typedef struct {
    float fx, fy, cx, cy;            /* mK */
    float sigma;                     /* mSigma (Tracking: 1.0) */
    float min_parallax;              /* minParallax (:182: 1.0) */
    int32_t min_triangulated;        /* minTriangulated (:182: 50) */
    int32_t iterations;              /* mMaxIterations (Tracking: 200) */
} orbg_init_problem;
typedef struct {
    int32_t n;                       /* N = mvMatches12.size() */
    int32_t best_h, best_f;          /* the iteration FindHomography / FindFundamental kept, -1 if none */
    float SH, SF, RH;
    int32_t model;                   /* 0 none, 1 ReconstructH, 2 ReconstructF */
    int32_t success;                 /* Initialize's return value */
    float R21[9], t21[3];            /* row-major; zero unless success */
    int32_t hyp;                     /* the hypothesis the decision rule looked at last, -1 if none */
    int32_t ntriangulated;           /* true entries of vbTriangulated; zero unless success */
    int32_t ninliers;                /* the N of ReconstructH / ReconstructF: inliers of the chosen model */
    int32_t nhyp;                    /* hypotheses checked: 8 (H), 4 (F), 0 (none or the early return) */
    int32_t ngood[8];                /* CheckRT's return value per hypothesis */
    float parallax[8];
    float hyp_R[8][9], hyp_t[8][3];  /* vR / vt of ReconstructH; (R1,t1) (R2,t1) (R1,t2) (R2,t2) */
} orbg_init_result;
/* One pair from host arrays: kps1[n1] / kps2[n2] = mvKeysUn of the reference / current frame,
 * matches12[n1], sets[problem->iterations][8].  Outputs: result, p3d[n1][3] (vP3D),
 * triangulated[n1] (vbTriangulated as bytes), both zero unless success, and, where not NULL,
 * scores_h / scores_f [iterations], H21 / F21 [iterations][9] (row-major float) and masks_h /
 * masks_f [iterations][ceil(N / 64)] (bit i % 64 of word i / 64 = vbCurrentInliers[i]).
 * ORBG_EINVAL for a NULL context or required pointer or a negative size; ORBG_ENOTSUP for n1 or
 * n2 past 8192 or more than 2^20 iterations.  A set with an index outside [0, N) or a repeated
 * one is not an error: that iteration scores 0.  Runs the batched kernels with npairs = 1
 * (bit-identical results).  Synchronises. */
int orbg_initialize(orbg_ctx *ctx, const orbg_init_problem *problem, const orbg_keypoint *kps1,
                    int n1, const orbg_keypoint *kps2, int n2, const int32_t *matches12,
                    const int32_t *sets, orbg_init_result *result, float *p3d,
                    uint8_t *triangulated, float *scores_h, float *scores_f, float *H21,
                    float *F21, uint64_t *masks_h, uint64_t *masks_f);
/* Batched, device memory, as the arrays lie there after extraction and matching: frame f's
 * keypoints at d_kps + f * frame_stride with d_counts[f] of them (orbg_batch_outputs /
 * orbg_batch_keys_un), pair p = frames d_f1[p] (reference) and d_f2[p] (current) with
 * d_matches12 + p * match_stride (orbg_match_outputs: match_stride = frame_cap) and d_sets +
 * (p * max_its + it) * 8.  cap, the row length of the outputs, is a multiple of 64
 * (ORBG_ENOTSUP past 8192); n1 is cut at cap and at match_stride; a frame index outside
 * [0, nframes) has no keys; d_problems[p].iterations is cut at max_its.  Outputs
 * d_results[npairs], d_p3d[npairs][cap][3] and d_triangulated[npairs][cap] (every byte of the
 * row is written) and, where not NULL, d_scores_h / _f [npairs][max_its], d_H21 / d_F21
 * [npairs][max_its][9], d_masks_h / _f [npairs][max_its][cap / 64]; iterations past a pair's
 * own and mask words past its N are zero.  Context stream, no host synchronisation; the only
 * allocation is the growth of the context scratch.  Results equal orbg_initialize's. */
int orbg_initialize_batch_device(orbg_ctx *ctx, const orbg_init_problem *d_problems,
                                 const orbg_keypoint *d_kps, int frame_stride,
                                 const int32_t *d_counts, int nframes, const int32_t *d_f1,
                                 const int32_t *d_f2, const int32_t *d_matches12,
                                 int match_stride, const int32_t *d_sets, int npairs, int cap,
                                 int max_its,
                                 orbg_init_result *d_results, float *d_p3d,
                                 uint8_t *d_triangulated, float *d_scores_h, float *d_scores_f,
                                 float *d_H21, float *d_F21, uint64_t *d_masks_h,
                                 uint64_t *d_masks_f);

#ifdef __cplusplus
}
#endif
#endif /* ORBG_H */
