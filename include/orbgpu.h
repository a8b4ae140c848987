/* orbgpu.h -- C ABI of the MI355X ORB front-end (liborbgpu.so).
 *
 * Plain C: pointers, sizes, int status codes, no torch / OpenCV / HIP types in signatures
 * (streams travel as void*).  One context per stream/thread; no globals.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * Lynx-MR/orbslam3lib root, cpp/ = app/src/main/cpp/):
 *   - ORBextractor ctor + operator()      cpp/include/ORBextractor_old.h:51-59,
 *                                         cpp/src/ORBextractor_old.cc:411-471, 1088-1191
 *   - stereo operator()(AHardwareBuffer*) cpp/include/ORBextractor.h:52-57 /
 *                                         cpp/src/ORBextractor.cc:118-165
 *   - FastRPC extractFeatures/bfMatchStereo  cpp/inc/orbslam3.idl:15-21 (impl
 *                                         dsp/src/orbslam_dsp.cpp:866-1087)
 *   - LynxHardwareAccelerator::{ctor,ExtractORB,BFMatchORB,dtor}
 *                                         cpp/include/LynxHardwareAcceleration/
 *                                         LynxHardwareAccelerator.h:45-51
 *   - ORBmatcher::DescriptorDistance      cpp/include/ORBmatcher.h:44, cpp/src/ORBmatcher.cc:2107
 *   - cv::BFMatcher(NORM_HAMMING).knnMatch(k=2)  cpp/src/Frame.cc:45,1227
 *   - mvImagePyramid (public member)      cpp/include/ORBextractor_old.h:80
 *   - Frame::ComputeStereoMatches         cpp/include/Frame.h:119, cpp/src/Frame.cc:827-997
 *   - ORBmatcher::SearchByProjection (Frame&, vector<MapPoint*>)  cpp/src/ORBmatcher.cc:44-214
 *   - Frame::UndistortKeyPoints / ComputeImageBounds / AssignFeaturesToGrid
 *                                         cpp/src/Frame.cc:405-436, 741-825
 */
#ifndef ORBGPU_H_
#define ORBGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBGPU_ABI_VERSION 2  /* 2: packed orbgpu_export_batch, ORBGPU_DEVICE_CURRENT */

/* Status codes (the DSP path returned 1/3/7 and callers ignored them; we never exit()). */
enum {
    ORBGPU_OK = 0,
    ORBGPU_ERR_EMPTY_IMAGE = -1,  /* reference operator() returns -1 on an empty image (:1092) */
    ORBGPU_ERR_CAPACITY = -2,     /* caller buffer / context capacity too small */
    ORBGPU_ERR_INVALID = -3,      /* bad argument */
    ORBGPU_ERR_HIP = -4,          /* HIP runtime error (see orbgpu_last_error) */
    ORBGPU_ERR_OVERFLOW = -5,     /* device-side workspace overflow (keys / nodes) */
    ORBGPU_ERR_NO_DEVICE = -6,    /* no usable gfx950 device */
    ORBGPU_ERR_RUNTIME = -7       /* two HIP runtimes mapped into the process (import torch first) */
};

/* The 5 ORB parameters of the ORBextractor ctor / Settings.cc:443-451. */
typedef struct {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} orbgpu_params;

/* cv::KeyPoint field layout (28 B): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbgpu_keypoint;

typedef struct orbgpu_ctx orbgpu_ctx;

/* Build a context for images up to max_width x max_height and batches of up to max_images
 * images.  Allocates all device memory once (nothing is allocated per call).  device = HIP
 * ordinal, or ORBGPU_DEVICE_CURRENT: the calling thread's current HIP device (hipGetDevice), so a
 * multi-camera process places each extractor on the GPU it selected before constructing it (the
 * C++ facades pass it); orbgpu_get_device reports the ordinal a context uses.
 * Replaces the ORBextractor ctor + LynxHardwareAccelerator ctor (orbslam3_open).
 * ORBGPU_ERR_INVALID for nlevels outside [1, 16], scale_factor not above 1 (any value above 1,
 * as ORBextractor; steps above 2 build the pyramid level by level from HBM), negative nfeatures
 * or sizes outside (0, 4112), or a pyramid level under 42 px (at the first batch of that size);
 * ORBGPU_ERR_NO_DEVICE without a HIP device. */
#define ORBGPU_DEVICE_CURRENT (-1)
int orbgpu_create(const orbgpu_params* params, int device, int max_width, int max_height,
                  int max_images, orbgpu_ctx** out_ctx);
int orbgpu_get_device(const orbgpu_ctx* ctx); /* the context's HIP ordinal (ORBGPU_ERR_INVALID: null) */
int orbgpu_destroy(orbgpu_ctx* ctx); /* orbslam3_close */

/* Scale tables exactly as the ORBextractor getters return them (GetScaleFactors, ...). */
int orbgpu_get_scale_tables(const orbgpu_ctx* ctx, float* scale, float* inv_scale,
                            float* sigma2, float* inv_sigma2, int32_t* features_per_level);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea) on one host
 * image (u8, row stride `stride`).  Writes *n keypoints (cv::KeyPoint layout) and n x 32 B
 * descriptors (row i <-> keypoint i), mono first / lapping-area keypoints from the back;
 * *n_mono = return value of the reference (monoIndex).  cap = capacity of kps/desc. */
int orbgpu_extract(orbgpu_ctx* ctx, const uint8_t* image, int width, int height, int stride,
                   int lap0, int lap1, orbgpu_keypoint* kps, uint8_t* desc, int cap, int* n,
                   int* n_mono);

/* Stereo form (ORBextractor.h:52-57 / IDL extractFeatures): left and right images in one call,
 * both on the device together. */
int orbgpu_extract_stereo(orbgpu_ctx* ctx, const uint8_t* left, const uint8_t* right, int width,
                          int height, int stride, const int lap_left[2], const int lap_right[2],
                          orbgpu_keypoint* kps_left, uint8_t* desc_left, int* n_left,
                          int* mono_left, orbgpu_keypoint* kps_right, uint8_t* desc_right,
                          int* n_right, int* mono_right, int cap);

/* ---- device-resident batch API (the throughput path) --------------------------------------
 * Images live in the context's HBM input buffer: [n_images][height][width] u8 (pitch = width).
 * orbgpu_upload_images copies host pixels in (PCIe; not part of the timed hot path).
 * orbgpu_run_batch runs the whole front-end for n_images images on `stream` (void* hipStream_t,
 * NULL = the context's own stream) and leaves keypoints/descriptors/counts in HBM.
 * laps: n_images x {lap0, lap1}, host pointer (copied into the launch arguments). */
int orbgpu_upload_images(orbgpu_ctx* ctx, const uint8_t* images, int n_images, int width,
                         int height, int stride);
uint8_t* orbgpu_device_input(orbgpu_ctx* ctx); /* device pointer of the input buffer */
/* Streaming ingest (C3: one frame pair after another, LynxHardwareAccelerator.cpp:121-123 copies
 * each frame in): stage the NEXT batch's pixels while the current batch computes.  The copy runs
 * on the context's copy stream into the second input buffer, after every kernel that read that
 * buffer; the next orbgpu_run_batch reads it once the copy has landed.  `images` should be pinned
 * (orbgpu_host_alloc) for the copy to run asynchronously at full PCIe rate.  One staged upload at
 * a time (ORBGPU_ERR_INVALID otherwise). */
int orbgpu_upload_images_async(orbgpu_ctx* ctx, const uint8_t* images, int n_images, int width,
                               int height, int stride);
/* Page-locked host memory for the async upload (hipHostMalloc / hipHostFree). */
int orbgpu_host_alloc(size_t bytes, void** ptr);
int orbgpu_host_free(void* ptr);
int orbgpu_run_batch(orbgpu_ctx* ctx, int n_images, int width, int height, const int32_t* laps,
                     void* stream);
/* Copy image i's results to the host (after orbgpu_synchronize or on the same stream). */
int orbgpu_download_result(orbgpu_ctx* ctx, int image, orbgpu_keypoint* kps, uint8_t* desc,
                           int cap, int* n, int* n_mono);
/* Per-image keypoint counts and mono counts of the last batch (host arrays of n_images). */
int orbgpu_download_counts(orbgpu_ctx* ctx, int n_images, int32_t* n, int32_t* n_mono);
/* Per-image number of cell keypoints that entered DistributeOctTree (vToDistributeKeys summed
 * over the levels) in the last batch: the octree's input size, for instrumentation. */
int orbgpu_candidate_counts(orbgpu_ctx* ctx, int n_images, int32_t* counts);
int orbgpu_synchronize(orbgpu_ctx* ctx);

/* Pyramid level `level` of batch image `image` (mvImagePyramid[level]), optionally blurred
 * (the GaussianBlur'd working copy, ORBextractor_old.cc:1146-1147). */
int orbgpu_get_pyramid_level(orbgpu_ctx* ctx, int image, int level, int blurred, uint8_t* dst,
                             int dst_stride, int* width, int* height);

/* Level keypoints before assembly (level coordinates, octree order, with angle) and their
 * descriptors: for per-stage parity tests.  counts[nlevels]. */
int orbgpu_get_level_keypoints(orbgpu_ctx* ctx, int image, orbgpu_keypoint* kps, uint8_t* desc,
                               int cap, int32_t* counts);

/* ---- Hamming matching ---------------------------------------------------------------------
 * cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, 2): for each query row the best
 * and second-best train rows (lexicographic (distance, index): lowest index wins ties);
 * idx = -1 / dist = INT32_MAX when absent (nt < 2).  Host pointers, n x 32 B each. */
int orbgpu_match_knn2(orbgpu_ctx* ctx, const uint8_t* query, int nq, const uint8_t* train, int nt,
                      int32_t* idx1, int32_t* dist1, int32_t* idx2, int32_t* dist2);
/* Device-pointer forms for multi-GPU exchange (C5 cross-camera BFMatch, SURVEY §8e: the
 * descriptors go from this context's HBM straight into a collective's buffer and back into the
 * matcher; nothing touches the host):
 *   orbgpu_export_descriptors: rows [row0, n) of batch image `image` -> device_dst (cap_rows x 32 B),
 *     *n_rows = rows copied (host); device-to-device on `stream` (NULL = the context's stream),
 *     ordered after the batch that produced them;
 *   orbgpu_match_knn2_device: orbgpu_match_knn2 with query / train / outputs in device memory
 *     (idx1, dist1, idx2, dist2: int32 [nq] each), on `stream`. */
int orbgpu_export_descriptors(orbgpu_ctx* ctx, int image, int row0, uint8_t* device_dst, int cap_rows,
                              int* n_rows, void* stream);
int orbgpu_match_knn2_device(orbgpu_ctx* ctx, const uint8_t* d_query, int nq, const uint8_t* d_train, int nt,
                             int32_t* d_idx1, int32_t* d_dist1, int32_t* d_idx2, int32_t* d_dist2, void* stream);

/* The C4 ingest-rank path (frames ingested on one GPU, every result handed back to
 * one caller, as LynxHardwareAccelerator.cpp:146-204 returns each frame's keypoints, descriptors
 * and matches to its caller), device memory throughout so a collective can move both ends:
 *   orbgpu_ingest_images: n images already in device memory (e.g. a scatter's receive buffer;
 *     rows of `stride` bytes) -> the context's input buffer, device to device on `stream`; the
 *     next orbgpu_run_batch / run_batch_match reads them;
 *   orbgpu_export_batch: the last batch's results of images [0, n_images) and stereo pairs
 *     [0, n_pairs) -> one device buffer (e.g. a gather's send buffer, 4-byte aligned), device to
 *     device on `stream`, ordered after the batch.  Only the rows produced are packed:
 *       int32 count[n_images], int32 mono[n_images], int32 n_queries[n_pairs],
 *       then for each image i: orbgpu_keypoint kps[count[i]], uint8 desc[count[i]][32],
 *       then for each pair p: int32 idx1[n_queries[p]], dist1[..], idx2[..], dist2[..]
 *       (the last match call's).
 *     *used = the layout's size in bytes.  The counts size it, so the call waits for the batch;
 *     device_dst = NULL only reports *used (the size query before a collective's allocation).
 *     A count the device replaced by a status (octree workspace overflow, output capacity) is
 *     returned as that status (ORBGPU_ERR_OVERFLOW / ORBGPU_ERR_CAPACITY) and nothing is packed.
 *     orbgpu_export_batch_bytes: the largest such layout (every image at the context's row
 *     capacity), with no device access. */
int orbgpu_ingest_images(orbgpu_ctx* ctx, const uint8_t* device_images, int n_images, int width,
                         int height, int stride, void* stream);
size_t orbgpu_export_batch_bytes(const orbgpu_ctx* ctx, int n_images, int n_pairs);
int orbgpu_export_batch(orbgpu_ctx* ctx, int n_images, int n_pairs, void* device_dst, size_t dst_bytes,
                        size_t* used, void* stream);

/* Batch stereo matching on device-resident results of the last orbgpu_run_batch: pair p
 * matches image 2p (query) against image 2p+1 (train), rows [mono..n) of each when
 * stereo_rows_only != 0 (Frame::ComputeStereoFishEyeMatches, Frame.cc:1142-1148) or all rows.
 * Results stay in HBM; fetch with orbgpu_download_matches. */
int orbgpu_match_stereo_batch(orbgpu_ctx* ctx, int n_pairs, int stereo_rows_only, void* stream);
/* orbgpu_run_batch followed by orbgpu_match_stereo_batch over all n_images / 2 pairs, as ONE
 * submission when the batch runs as one captured graph (the latency shape: the accelerator
 * session's stereo frame, LynxHardwareAccelerator.cpp:133-204, which extracts both eyes and
 * runs BFMatchORB's kNN2 in one device pass); otherwise exactly the two calls.  n_images even. */
int orbgpu_run_batch_match(orbgpu_ctx* ctx, int n_images, int width, int height, const int32_t* laps,
                           int stereo_rows_only, void* stream);
int orbgpu_download_matches(orbgpu_ctx* ctx, int pair, int32_t* idx1, int32_t* dist1,
                            int32_t* idx2, int32_t* dist2, int cap, int* nq);

/* ---- stereo matching ----------------------------------------------------------------------
 * Frame::ComputeStereoMatches (cpp/src/Frame.cc:827-997, called from the stereo Frame ctor
 * :161 and FrameAHB.cc:129) on the device-resident results of the last orbgpu_run_batch:
 * pair p = left image 2p (mvKeys), right image 2p+1 (mvKeysRight), rectified pinhole stereo.
 * mbf = baseline * fx, mb = baseline (Frame::mbf, Frame::mb).  Per left keypoint: mvuRight and
 * mvDepth (-1 = no stereo match), and the accepted SAD distance (-1 = none; also set for
 * matches the median rule rejects).  Results stay in HBM; fetch with orbgpu_download_stereo. */
int orbgpu_stereo_matches_batch(orbgpu_ctx* ctx, int n_pairs, float mbf, float mb, void* stream);
int orbgpu_download_stereo(orbgpu_ctx* ctx, int pair, float* u_right, float* depth, int32_t* sad,
                           int cap, int* n);

/* ---- fisheye stereo ------------------------------------------------------------------------
 * Frame::ComputeStereoFishEyeMatches (cpp/src/Frame.cc:1142-1201, called from the two-camera
 * Frame ctor :1121 and FrameAHB.cc:320) on the device-resident results of the last
 * orbgpu_run_batch: pair p = left image 2p (mvKeys), right image 2p+1 (mvKeysRight).  Runs the
 * stereo-row kNN2 (BFMatchORB, :1164 = orbgpu_match_stereo_batch with stereo_rows_only = 1; its
 * result stays readable through orbgpu_download_matches), then per left stereo row: dist1 == 0
 * skipped, dist1 < 70 triangulated with KannalaBrandt8::TriangulateMatches
 * (CameraModels/KannalaBrandt8.cpp:300-366; sigmas = mvLevelSigma2 of the two octaves) and
 * accepted when the depth > 1e-4.  Parity with the reference is unpinned (Eigen's JacobiSVD
 * order and FMA use, the Android libm's atan2f / tanf): see DESIGN.md and tests/test_fisheye.py. */
typedef struct {
    float cam_left[8], cam_right[8];   /* KannalaBrandt8 mvParameters: fx fy cx cy k0 k1 k2 k3 */
    float precision_left, precision_right;  /* KannalaBrandt8::precision (1e-6 by default) */
    float R12[9];                      /* Frame::mRlr, row-major */
    float t12[3];                      /* Frame::mtlr */
} orbgpu_kb8_rig;
int orbgpu_fisheye_stereo_batch(orbgpu_ctx* ctx, int n_pairs, const orbgpu_kb8_rig* rig, void* stream);
/* Per pair: mvLeftToRightMatch [n_left], mvRightToLeftMatch [n_right] (-1 = none), mvDepth
 * [n_left] (-1 = none), mvStereo3Dpoints [n_left][3] (0 where none), nMatches. */
int orbgpu_download_fisheye(orbgpu_ctx* ctx, int pair, int32_t* l2r, int32_t* r2l, float* depth, float* p3d,
                            int cap, int* n_left, int* n_right, int* n_matches);

/* ---- ORBmatcher::SearchByProjection (cpp/src/ORBmatcher.cc:44-214, pinhole frames) ---------
 * Tracking's local-map search: every map point predicted in view is matched against the frame
 * keypoints in a window around its projection (Frame::GetFeaturesInArea, Frame.cc:673-735, on the
 * grid of orbgpu_undistort_grid_batch), best/second-best Hamming with TH_HIGH = 100 and the
 * nnratio test; the keypoint is then taken (later map points skip it when the taker has
 * observations).  Frames are batch images f * image_step (image_step 2: the left eye of stereo
 * pair f, whose mvuRight from orbgpu_stereo_matches_batch is used when use_uright != 0;
 * image_step 1: monocular frames, mvuRight all -1).
 * A map point carries the MapPoint state the function reads: */
typedef struct {
    float proj_x, proj_y;  /* mTrackProjX, mTrackProjY */
    float proj_xr;         /* mTrackProjXR */
    float view_cos;        /* mTrackViewCos */
    float depth;           /* mTrackDepth */
    int32_t level;         /* mnTrackScaleLevel, in [0, nlevels) (others are skipped) */
    int32_t flags;         /* ORBGPU_MP_* */
    uint8_t desc[32];      /* GetDescriptor() */
    float proj_yr;         /* mTrackProjYR     (two-camera frames) */
    float view_cos_r;      /* mTrackViewCosR   (two-camera frames) */
    int32_t level_r;       /* mnTrackScaleLevelR (two-camera frames) */
} orbgpu_map_point;
#define ORBGPU_MP_IN_VIEW 1    /* mbTrackInView */
#define ORBGPU_MP_BAD 2        /* isBad() */
#define ORBGPU_MP_HAS_OBS 4    /* Observations() > 0 */
#define ORBGPU_MP_IN_VIEW_R 8  /* mbTrackInViewR (two-camera frames) */
/* mps: all frames' map points, frame f's in [mp_offsets[f], mp_offsets[f + 1]) (host arrays).
 * kp_block (optional, [n_frames][kp_stride] u8): 1 where F.mvpMapPoints[k] is already set to a
 * point with observations before the call.  th / nnratio / far_points / th_far as the reference.
 * orbgpu_download_projection_matches: match[k] = index (within the frame's map points) of the
 * point assigned to keypoint k by this call, -1 if none; *nmatches = the reference's return. */
int orbgpu_search_by_projection_batch(orbgpu_ctx* ctx, int n_frames, int image_step, int use_uright,
                                      const orbgpu_map_point* mps, const int32_t* mp_offsets,
                                      const uint8_t* kp_block, int kp_stride, float th, float nnratio,
                                      int far_points, float th_far, void* stream);
/* Two-camera frames (Nleft != -1, the fisheye rig; ORBmatcher.cc:59-214): frame f = left image
 * 2f + right image 2f + 1, both gridded by orbgpu_undistort_grid_batch with no distortion
 * coefficients (the grid is built on the raw positions, Frame.cc:405-436, and the bounds are the
 * image, :798-825).  left_to_right / right_to_left ([n_pairs][lr_stride], -1 = none; NULL: all
 * -1) are Frame::mvLeftToRightMatch / mvRightToLeftMatch.  kp_block and the downloaded match
 * array cover Nleft + Nright keypoints: the left ones, then the right ones (the reference's
 * mvpMapPoints indexing). */
int orbgpu_search_by_projection_stereo(orbgpu_ctx* ctx, int n_pairs, const orbgpu_map_point* mps,
                                       const int32_t* mp_offsets, const int32_t* left_to_right,
                                       const int32_t* right_to_left, int lr_stride, const uint8_t* kp_block,
                                       int kp_stride, float th, float nnratio, int far_points, float th_far,
                                       void* stream);
int orbgpu_download_projection_matches(orbgpu_ctx* ctx, int frame, int32_t* match, int cap, int* n_kp,
                                       int* nmatches);

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) ----------------------
 * Tracking::TrackWithMotionModel's frame-to-frame search (cpp/src/ORBmatcher.cc:1683-1838 with
 * ComputeThreeMaxima :2061-2102; pinhole frames, Nleft == -1: monocular or rectified stereo).  Every
 * valid last-frame point is transformed with the current pose, projected (Pinhole.cpp:40-41) and
 * matched in a window of th * mvScaleFactors[octave] on the grid of orbgpu_undistort_grid_batch:
 * levels >= octave when the camera moved forward (tlc.z > mb, not mono), <= octave backward,
 * octave +-1 otherwise; best Hamming distance <= TH_HIGH = 100, no ratio test; then the rotation
 * histogram (30 bins, factor 1/30 as the reference) and the three-maxima rule when
 * check_orientation != 0.  All arithmetic is IEEE single, evaluated in the reference's order.
 * Frames, kp_block, host arrays and the stream are as in orbgpu_search_by_projection_batch; mbf /
 * mb are Frame::mbf / Frame::mb, K = {fx, fy, cx, cy}.
 * Deviations (the reference reads out of range there): a point whose projection is not finite or
 * whose octave is outside [0, nlevels) is skipped; an event whose bin is outside [0, 30) (angles
 * outside [0, 360)) counts in nmatches but enters no bin.
 * The two-camera branch (:1840-1914) is orbgpu_track_by_projection_stereo below; the
 * relocalisation overload (:1923-2059) is orbgpu_reloc_by_projection_batch, further down.
 * (SearchByBoW, further down, is built for pinhole frames only: its two-camera form is not.) */
typedef struct {
    float pos[3];      /* pMP->GetWorldPos() */
    float angle;       /* LastFrame.mvKeysUn[i].angle */
    int32_t octave;    /* LastFrame.mvKeys[i].octave (nLastOctave) */
    int32_t flags;     /* ORBGPU_LP_VALID: mvpMapPoints[i] && !mvbOutlier[i];
                          ORBGPU_MP_HAS_OBS: pMP->Observations() > 0 */
    uint8_t desc[32];  /* pMP->GetDescriptor() */
} orbgpu_last_point;   /* 56 bytes */
#define ORBGPU_LP_VALID 1

typedef struct {
    float Rcw[9], tcw[3];  /* CurrentFrame.GetPose(), row-major */
    float Rlw[9], tlw[3];  /* LastFrame.GetPose() */
} orbgpu_track_pose;

/* pts: all frames' last-frame points, frame f's in [pt_offsets[f], pt_offsets[f + 1]); poses: one
 * per frame.  orbgpu_download_track_matches: match[k] = index (within the frame's points) of the
 * last-frame point that ends up in CurrentFrame.mvpMapPoints[k], -1 if none; *nmatches = the
 * reference's return value; rot_hist = the 30 bin sizes before the three-maxima rule (all 0 when
 * check_orientation == 0). */
int orbgpu_track_by_projection_batch(orbgpu_ctx* ctx, int n_frames, int image_step, int use_uright,
                                     const orbgpu_last_point* pts, const int32_t* pt_offsets,
                                     const orbgpu_track_pose* poses, const float K[4], float mbf, float mb,
                                     const uint8_t* kp_block, int kp_stride, float th, int mono,
                                     int check_orientation, void* stream);
/* After orbgpu_track_by_projection_stereo: *n_kp = Nleft + Nright and match covers the left
 * keypoints, then (from Nleft on) the right ones. */
int orbgpu_download_track_matches(orbgpu_ctx* ctx, int frame, int32_t* match, int cap, int* n_kp,
                                  int* nmatches, int32_t rot_hist[30]);

/* The same search on two-camera frames (CurrentFrame.Nleft != -1, the KannalaBrandt8 rig;
 * ORBmatcher.cc:1721-1921 with :1840-1914).  Frame f = left image 2f + right image 2f + 1, both
 * gridded by orbgpu_undistort_grid_batch with no distortion coefficients, as for
 * orbgpu_search_by_projection_stereo; kp_block ([n_pairs][kp_stride]) and the downloaded match array
 * cover Nleft + Nright keypoints, left first.  The last frame's points cover its Nleft + Nright
 * keypoints: octave and angle come from mvKeys[i] or mvKeysRight[i - Nleft].  Per valid point:
 *   - x3Dc = Tcw * X; invz = 1 / zc < 0 skips the point (both windows);
 *   - left window: uv = mpCamera->project(x3Dc) (KannalaBrandt8.cpp:61-78, cam_left); outside
 *     [mnMinX, mnMaxX] x [mnMinY, mnMaxY] skips the point; GetFeaturesInArea(bRight = false) on
 *     the left grid and mvKeys with the level range of the direction.  If no keypoint passes its
 *     level and distance tests the point is skipped, right window included (:1778-1779; tested
 *     before occupancy: a window whose keypoints all hold points is not empty).  No mvuRight test.
 *     Best distance <= TH_HIGH: match[best] = i, one event;
 *   - right window: x3Dr = Trl * x3Dc, uv = mpCamera->project(x3Dr) -- the *left* camera model, as
 *     the reference calls it -- with no bounds, 1/z or empty-window test; the same radius and
 *     levels; GetFeaturesInArea(bRight = true) on the right grid and mvKeysRight; a second,
 *     independent event at Nleft + best;
 *   - one rotation histogram and one three-maxima rejection over the events of both sides.
 * Pinned choices: KannalaBrandt8::project as restated for orbgpu_fisheye_stereo_batch (atan2f, cosf
 * and sinf as the host libm computes them); Trl * x3Dc row by row as ((R0 x + R1 y) + R2 z) + t
 * (Sophus's own order is not reproducible here).  Parity with the reference is unpinned, as for
 * the pinhole form.  Deviations: the pinhole form's apply to the point as a whole (left projection
 * not finite, octave outside [0, nlevels), bin outside [0, 30)); a right projection that is not
 * finite skips the right window only. */
typedef struct {
    float cam_left[8];     /* CurrentFrame.mpCamera: KannalaBrandt8 mvParameters fx fy cx cy k0..k3 */
    float Rrl[9], trl[3];  /* CurrentFrame.GetRelativePoseTrl() (mTrl), row-major */
} orbgpu_track_rig;        /* 80 bytes */

int orbgpu_track_by_projection_stereo(orbgpu_ctx* ctx, int n_pairs, const orbgpu_last_point* pts,
                                      const int32_t* pt_offsets, const orbgpu_track_pose* poses,
                                      const orbgpu_track_rig* rig, float mb, const uint8_t* kp_block,
                                      int kp_stride, float th, int mono, int check_orientation, void* stream);

/* ---- ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) -----
 * Tracking::MonocularInitialization's matcher (cpp/src/ORBmatcher.cc:649-764 with
 * ComputeThreeMaxima :2061-2102; the reference calls it with windowSize 100 on ORBmatcher(0.9,
 * true)) over pairs of batch images {F1, F2}, both inside the range of the last
 * orbgpu_undistort_grid_batch.  One image may be F1, or F2, of several pairs (one initial frame
 * against successive current frames), and F1 == F2 is legal.  All arithmetic is IEEE single,
 * evaluated in the reference's order:
 *   1. vnMatches12 has F1's N1 entries, all -1; vMatchedDistance and vnMatches21 have F2's N2
 *      entries, INT_MAX and -1 (:652-660).
 *   2. i1 ascending; a keypoint with octave > 0 is skipped (:662-667).
 *   3. F2.GetFeaturesInArea(prev[i1].x, prev[i1].y, (float)windowSize, 0, 0) (:669, Frame.cc:
 *      673-739): only octave-0 keypoints of F2, fabs(dx) < r && fabs(dy) < r on mvKeysUn, in the
 *      order grid column, row, index within the cell; an empty window skips the point (:671-672).
 *   4. per candidate i2 in that order: skipped when vMatchedDistance[i2] <= dist (:688-689);
 *      otherwise best / second best with strict < from INT_MAX (:691-700), i.e. the two lowest
 *      (distance, window position) that survive; an equal distance becomes the second best.
 *   5. an event when bestDist <= TH_LOW = 50 and (float)bestDist < (float)bestDist2 * nnratio
 *      (:703-705; a lone candidate has bestDist2 = INT_MAX = 2147483648.0f): the previous owner of
 *      the keypoint is robbed (vnMatches12[owner] = -1, nmatches--, :707-711), then vnMatches12[i1]
 *      = best, vnMatches21[best] = i1, vMatchedDistance[best] = bestDist, nmatches++ (:712-715);
 *      with check_orientation, rot = F1.angle[i1] - F2.angle[best] (+360 if negative), bin =
 *      round(rot * (1.0f / 30)) (30 -> 0), and i1 enters that bin (:717-727).  The entry of a
 *      point robbed later stays in its bin and counts towards its size.
 *   6. ComputeThreeMaxima on the 30 bin sizes; every entry of a bin outside the three that is
 *      still matched is cleared and takes one off nmatches (:733-756): an entry already robbed
 *      subtracts nothing.
 *   7. prev[i1] = F2.mvKeysUn[vnMatches12[i1]].pt wherever vnMatches12[i1] >= 0 (:759-761).
 * Deviations (the reference reads out of range there): a point whose prev is not finite is
 * skipped; an event whose bin falls outside [0, 30) counts in nmatches, enters no bin and cannot
 * be rejected.  Parity with the reference is unpinned, as for the other matcher functions: the
 * yardstick is the Python restatement in tests/test_search_for_initialization.py.
 * image_pairs: [n_pairs][2] batch images (host); prev_matched: [n_pairs][pm_stride][2] (host;
 * NULL: F1's mvKeysUn.pt, the reference's state at the first call).  ORBGPU_ERR_INVALID: null
 * context, n_pairs < 0 or above the context's image capacity, an image outside the gridded range,
 * window_size < 0, pm_stride below an F1's keypoint count; n_pairs == 0 succeeds.
 * ORBGPU_ERR_CAPACITY when the context's keypoint capacity exceeds the matcher's LDS budget, as
 * for orbgpu_track_by_projection_batch.
 * orbgpu_download_initialization_matches: match12 [N1] = vnMatches12, prev_matched [N1][2] =
 * vbPrevMatched after the call (may be NULL), *nmatches = the reference's return value, rot_hist =
 * the 30 bin sizes before the three-maxima rule (all 0 when check_orientation == 0). */
int orbgpu_search_for_initialization_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* image_pairs,
                                           const float* prev_matched, int pm_stride, int window_size,
                                           float nnratio, int check_orientation, void* stream);
int orbgpu_download_initialization_matches(orbgpu_ctx* ctx, int pair, int32_t* match12, float* prev_matched,
                                           int cap, int* n1, int* nmatches, int32_t rot_hist[30]);

/* ---- ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) ----
 * The matcher of Tracking::TrackReferenceKeyFrame (ORBmatcher(0.7, true)) and of
 * Tracking::Relocalization (0.75, against every candidate keyframe): cpp/src/ORBmatcher.cc:224-426
 * with ComputeThreeMaxima :2061-2102, on pinhole frames (F.Nleft == -1, so bestDist1R stays 256 and
 * the right-camera block :358-387 never fires).  Pair p = a keyframe given by the host (kf_pts
 * [kf_offsets[p], kf_offsets[p + 1])) and a frame that is image frames[p] of the last
 * orbgpu_run_batch; several pairs may name the same frame.  The vocabulary stays on the host: the
 * node of each keypoint -- mFeatVec, as Frame::ComputeBoW / DBoW2::transform with levelsup = 4
 * compute it -- is an input on both sides.  All arithmetic is IEEE single, evaluated in the
 * reference's order:
 *   1. match has F's N entries, all -1 (:228).
 *   2. the two feature vectors are std::map<NodeId, vector<unsigned>>; a node's list holds keypoint
 *      indices in ascending order (transform adds feature i in index order).
 *   3. the merge :245-403 visits the nodes present in both; nodes do not interact.
 *   4. in a common node, for iKF ascending (:252): a keyframe keypoint without a map point, or with a
 *      bad one, is skipped (:258-262); F's keypoints of the node are walked in ascending index order,
 *      one that holds a match is skipped (:279-280); best and second best with strict < from 256 /
 *      256 (:286-295): an equal distance becomes the second best, never the best.
 *   5. an event when bestDist1 <= TH_LOW = 50 and (float)bestDist1 < nnratio * (float)bestDist2
 *      (:328-330; a lone candidate has bestDist2 = 256): match[bestIdxF] = realIdxKF, nmatches++;
 *      with check_orientation, rot = KF.angle[realIdxKF] - F.angle[bestIdxF] (+360 if negative), bin
 *      = round(rot * (1.0f / 30)) (30 -> 0), and bestIdxF enters that bin (:339-354).  A keypoint of
 *      F is never taken twice.
 *   6. ComputeThreeMaxima on the 30 bin sizes; every entry of a bin outside the three maxima is
 *      cleared and takes one off nmatches (:405-423).
 * Deviations: a negative node means "this keypoint is in no node"; an event whose bin falls
 * outside [0, 30) (angle outside [0, 360) or not finite; the reference asserts) counts in nmatches,
 * enters no bin and cannot be rejected.  Parity with the reference is unpinned, as for the other
 * matcher functions: the yardstick is the Python restatement in tests/test_search_by_bow.py.
 * The frame needs only the last batch's descriptors and angles, not orbgpu_undistort_grid_batch.
 * f_nodes: [n_pairs][node_stride], the node of keypoint k of pair p's frame at [p][k].  Host arrays
 * are pageable and may be reused when the call returns.  ORBGPU_ERR_INVALID: null context, n_pairs
 * < 0 or above the context's image capacity, null arrays when n_pairs > 0, a frame outside the last
 * batch, kf_offsets not ascending from a value >= 0, node_stride below a frame's keypoint count;
 * n_pairs == 0 succeeds and leaves no pair to download.  ORBGPU_ERR_CAPACITY when a pair has more
 * than ORBGPU_BOW_MAX_POINTS keyframe points, or the context's keypoint capacity per image exceeds
 * it: one workgroup orders a side's keypoints by node in LDS (5000 features per image fit).
 * orbgpu_download_bow_matches: match[k] = index, within the pair's keyframe points, of the point that
 * ends up in vpMapPointMatches[k], -1 if none; *n_kp = F.N; *nmatches = the reference's return
 * value; rot_hist = the 30 bin sizes before the three-maxima rule (all 0 when check_orientation ==
 * 0).  Errors as for orbgpu_download_initialization_matches.
 * SearchByBoW on two-camera frames (F.Nleft != -1, :297-324 and :358-387) is not built. */
typedef struct {
    uint8_t desc[32];  /* pKF->mDescriptors.row(i) */
    float angle;       /* pKF->mvKeysUn[i].angle */
    int32_t node;      /* the node of mFeatVec that holds i; < 0: none */
    int32_t flags;     /* ORBGPU_BOW_HAS_POINT: vpMapPointsKF[i] && !isBad() */
} orbgpu_bow_point;    /* 44 bytes */
#define ORBGPU_BOW_HAS_POINT 1
#define ORBGPU_BOW_MAX_POINTS 8192

int orbgpu_search_by_bow_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames,
                               const orbgpu_bow_point* kf_pts, const int32_t* kf_offsets,
                               const int32_t* f_nodes, int node_stride, float nnratio,
                               int check_orientation, void* stream);
int orbgpu_download_bow_matches(orbgpu_ctx* ctx, int pair, int32_t* match, int cap, int* n_kp,
                                int* nmatches, int32_t rot_hist[30]);

/* ---- ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) ----------
 * The matcher LocalMapping::CreateNewMapPoints runs for the new keyframe against each of its 10 (30
 * when monocular) neighbours (LocalMapping.cc:397-472): cpp/src/ORBmatcher.cc:908-1153 with
 * Pinhole::epipolarConstrain (CameraModels/Pinhole.cpp:102-124) and ComputeThreeMaxima :2061-2102,
 * on pinhole keyframes (pKF1->mpCamera2 == nullptr, NLeft == -1).  Pair p = keyframe 1, which is
 * image frames[p] of the last batch, inside the range of the last orbgpu_undistort_grid_batch (its
 * positions are mvKeysUn), against keyframe 2, given by the host as kf_pts [kf_offsets[p],
 * kf_offsets[p + 1]); several pairs may name the same frame.  The vocabulary stays on the host: the
 * node of each keypoint (mFeatVec) is an input on both sides.  F12 and the epipole are inputs per
 * pair: the reference recomputes F12 per candidate with Eigen's 3x3 inverses (Pinhole.cpp:104-107),
 * which does not vary over a pinhole pair, so the host evaluates that expression once.  The level
 * tables mvScaleFactors / mvLevelSigma2 of both keyframes are the context's: both keyframes are
 * assumed to come from the same extractor settings.  All arithmetic is IEEE single, evaluated in the
 * reference's order, unless a step says otherwise:
 *   1. match12 has keyframe 1's N1 entries, all -1 (:957).
 *   2. only the nodes present in both feature vectors are visited (:970-1119); nodes do not
 *      interact; a node's list holds keypoint indices in ascending order.
 *   3. in a common node, for idx1 ascending (:974): a keypoint 1 with ORBGPU_TRI_HAS_POINT is skipped
 *      (:978-984), and with only_stereo one without ORBGPU_TRI_STEREO (:986-990).
 *   4. bestDist = TH_LOW = 50, bestIdx2 = -1 (:1001-1002); for idx2 ascending (:1004) a candidate
 *      continues when it has ORBGPU_TRI_HAS_POINT (:1008-1012; vbMatched2 is never set, and there is no
 *      isBad test here), when only_stereo is on and it lacks ORBGPU_TRI_STEREO (:1014-1018), when
 *      dist > 50 || dist > bestDist (:1024: an equal distance does not continue, so the later
 *      candidate replaces the earlier one), when both keypoints are mono and, with dx = ep[0] - x2,
 *      dy = ep[1] - y2, dx * dx + dy * dy < 100 * mvScaleFactors[octave2] (:1033-1041, an int *
 *      float product), or when coarse is off and the epipolar test fails (:1079); otherwise it
 *      becomes the best (:1081-1082).
 *   5. the epipolar test (Pinhole.cpp:110-123): a = x1 * F(0,0) + y1 * F(1,0) + F(2,0) left to right,
 *      b with column 1, c with column 2; num = a * x2 + b * y2 + c; den = a * a + b * b; false when
 *      den == 0; else (double)(num * num / den) < 3.84 * (double)mvLevelSigma2[octave2]: 3.84 is a
 *      double literal, so the product and the comparison are in double.  sigmaLevel is unused.  A NaN
 *      num * num / den fails, as in the reference.
 *   6. when bestIdx2 >= 0: match12[idx1] = bestIdx2, nmatches++ (:1086-1092); with check_orientation
 *      rot = angle1 - angle2 (+360 if negative), bin = round(rot * (1.0f / 30)) (30 -> 0), no fmodf
 *      (:1094-1104).  One keypoint 2 may end up matched by several keypoints 1: that is the reference's
 *      behaviour and it is kept.
 *   7. ComputeThreeMaxima on the 30 bin sizes; every entry of a bin outside the three maxima is
 *      cleared and takes one off nmatches (:1121-1140).
 * Deviations: a negative node means "this keypoint is in no node"; an event whose bin falls outside
 * [0, 30) (the reference asserts) counts in nmatches, enters no bin and cannot be rejected.  Parity
 * with the reference is unpinned, as for the other matcher functions: the yardstick is the Python
 * restatement in tests/test_search_for_triangulation.py.
 * f_nodes: [n_pairs][node_stride], the node of keypoint k of pair p's keyframe 1 at [p][k]; f_flags:
 * [n_pairs][flag_stride] u8 with the two flag bits for that keypoint, NULL: no map points and no
 * stereo keypoints.  Host arrays are pageable and may be reused when the call returns.
 * ORBGPU_ERR_INVALID: null context, n_pairs < 0 or above the context's image capacity, null arrays
 * when n_pairs > 0, a frame outside the gridded range, kf_offsets not ascending from a value >= 0, a
 * stride below a frame's keypoint count, an octave of a keyframe point outside [0, nlevels); n_pairs ==
 * 0 succeeds and leaves no pair to download.  ORBGPU_ERR_CAPACITY when a side holds more than
 * ORBGPU_BOW_MAX_POINTS keypoints (the context's keypoint capacity per image counts for keyframe 1).
 * Every status is decided before any launch.
 * orbgpu_download_triangulation_matches: match12[k] = the index, within the pair's keyframe points,
 * that the reference leaves in vMatches12[k], -1 if none; *n1 = N1; *nmatches = the reference's
 * return value; rot_hist = the 30 bin sizes before the three-maxima rule (all 0 when
 * check_orientation == 0).  vMatchedPairs is the list of (k, match12[k]) over the non-negative
 * entries, k ascending (:1142-1150).  Errors as for orbgpu_download_bow_matches.
 * Not built: the two-camera SearchForTriangulation (mpCamera2 set: the Tll / Tlr / Trl / Trr
 * selection :1043-1077 and KannalaBrandt8::epipolarConstrain, which triangulates) and SearchBySim3, which
 * has no caller.  SearchByBoW(KeyFrame*, KeyFrame*) is orbgpu_search_by_bow_kf_batch, the Sim3
 * SearchByProjection overloads are orbgpu_sim3_search_by_projection_batch, both below. */
typedef struct {
    uint8_t desc[32];  /* pKF2->mDescriptors.row(i) */
    float x, y;        /* pKF2->mvKeysUn[i].pt */
    float angle;       /* pKF2->mvKeysUn[i].angle */
    int32_t octave;    /* pKF2->mvKeysUn[i].octave */
    int32_t node;      /* the node of mFeatVec that holds i; < 0: none */
    int32_t flags;     /* ORBGPU_TRI_HAS_POINT: pKF2->GetMapPoint(i) != nullptr (no isBad test here, :1008-1012)
                          ORBGPU_TRI_STEREO:    pKF2->mvuRight[i] >= 0 */
} orbgpu_triang_point;   /* 56 bytes */
#define ORBGPU_TRI_HAS_POINT 1
#define ORBGPU_TRI_STEREO 2
typedef struct {
    float F12[9];      /* row-major, K1^-T * [t12]x * R12 * K2^-1 as Pinhole.cpp:104-107 computes it */
    float ep[2];       /* pKF2->mpCamera->project(T2w * Cw1) (:925-927) */
} orbgpu_triang_pair;    /* 44 bytes */

int orbgpu_search_for_triangulation_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames,
                                          const orbgpu_triang_point* kf_pts, const int32_t* kf_offsets,
                                          const orbgpu_triang_pair* pairs, const int32_t* f_nodes,
                                          int node_stride, const uint8_t* f_flags, int flag_stride,
                                          int only_stereo, int coarse, int check_orientation, void* stream);
int orbgpu_download_triangulation_matches(orbgpu_ctx* ctx, int pair, int32_t* match12, int cap, int* n1,
                                          int* nmatches, int32_t rot_hist[30]);

/* ---- ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) ----
 * The search Tracking::Relocalization (Tracking.cc:3670-3829) runs on a candidate keyframe when PnP
 * and pose optimisation left too few inliers, on ORBmatcher(0.9, true) with (th, ORBdist) = (10, 100)
 * and then (3, 64): cpp/src/ORBmatcher.cc:1923-2059 with ComputeThreeMaxima :2061-2102 and
 * MapPoint::PredictScale (MapPoint.cc:533-548), pinhole frames, monocular path (mvKeysUn,
 * GetFeaturesInArea(bRight = false), no mvuRight test).  Pair p = the keyframe points kf_pts
 * [kf_offsets[p], kf_offsets[p + 1]) in the keyframe's keypoint order, batch image frames[p] inside
 * the range of the last orbgpu_undistort_grid_batch, pose p and occupancy row p; several pairs may
 * name the same frame, each with its own pose and occupancy.  All arithmetic is IEEE single,
 * evaluated in the reference's order.  For i ascending:
 *   1. a point without ORBGPU_RP_VALID is skipped (:1941-1944).
 *   2. x3Dc = Tcw * X, row by row as ((R0 x + R1 y) + R2 z) + t; u = fx * xc / zc + cx, v = fy * yc /
 *      zc + cy (Pinhole.cpp:40-41); skipped when u < mnMinX || u > mnMaxX, likewise v (:1953-1956).
 *      This overload has no 1/z test.
 *   3. PO = X - Ow, dist3D = sqrtf((PO.x * PO.x + PO.y * PO.y) + PO.z * PO.z); skipped when dist3D <
 *      0.8f * min_distance || dist3D > 1.2f * max_distance (:1959-1967, MapPoint.cc:504-514).
 *   4. ratio = max_distance / dist3D; nPredictedLevel = (int)ceilf(logf(ratio) / logf(scaleFactor))
 *      clamped to [0, nlevels - 1], logf being the host libm's (orbgpu_predict_scale_table below).
 *   5. GetFeaturesInArea(u, v, th * mvScaleFactors[level], level - 1, level + 1) (:1972-1974).
 *   6. over the window, in the order grid column, row, index within the cell: a keypoint that holds
 *      a point -- before the call, or taken earlier in it -- is skipped (:1988-1989); the best is
 *      the first lowest Hamming distance, strict < from 256; no second best, no ratio test.
 *   7. an event when bestDist <= orb_dist: match[best] = i, nmatches++, the keypoint is taken; with
 *      check_orientation rot = angleKF[i] - angleF[best]; rot < 0 || rot > 360: rot = fmodf(rot,
 *      360.0f); rot < 0: rot += 360.0f; bin = round(rot * (1.0f / 30)) (30 -> 0) (:2010-2027).
 *   8. ComputeThreeMaxima on the 30 bin sizes; every entry of a bin outside the three maxima is
 *      cleared and takes one off nmatches (:2036-2056).
 * Deviations (the reference reads out of range there): a point whose projection, dist3D or ratio is
 * not finite is skipped; an event whose bin is outside [0, 30) counts in nmatches, enters no bin and
 * cannot be rejected.  Parity with the reference is unpinned, as for the other matcher functions:
 * the yardstick is the Python restatement in tests/test_reloc_projection.py.
 * kp_block ([n_pairs][kp_stride] u8, host; NULL: none): [p][k] != 0 where CurrentFrame.mvpMapPoints[k]
 * is set before the call.  K = {fx, fy, cx, cy}.  Host arrays are pageable and may be reused when the
 * call returns.  ORBGPU_ERR_INVALID: null context, n_pairs < 0 or above the context's image
 * capacity, null arrays when n_pairs > 0, a frame outside the gridded range, kf_offsets not
 * ascending from a value >= 0, kp_stride below a frame's keypoint count, orb_dist outside [0, 255]
 * (256 would assign keypoint -1), th negative or not finite; n_pairs == 0 succeeds and leaves no
 * pair to download.  ORBGPU_ERR_CAPACITY when the context's keypoint capacity exceeds the matcher's
 * LDS budget, as for orbgpu_track_by_projection_batch.  Every status is decided before any launch.
 * orbgpu_download_reloc_matches: match[k] = index, within the pair's keyframe points, of the point
 * that ends up in CurrentFrame.mvpMapPoints[k] by this call, -1 if none; *n_kp = N; *nmatches = the
 * reference's return value; rot_hist = the 30 bin sizes before the three-maxima rule (all 0 when
 * check_orientation == 0).  Errors as for orbgpu_download_bow_matches. */
typedef struct {
    float pos[3];        /* pMP->GetWorldPos() */
    float angle;         /* pKF->mvKeysUn[i].angle */
    float min_distance;  /* pMP->mfMinDistance (the 0.8f factor is applied here) */
    float max_distance;  /* pMP->mfMaxDistance (1.2f for the gate, raw for PredictScale) */
    int32_t flags;       /* ORBGPU_RP_VALID: pMP && !isBad() && !sAlreadyFound.count(pMP) */
    uint8_t desc[32];    /* pMP->GetDescriptor() */
} orbgpu_reloc_point;    /* 60 bytes */
#define ORBGPU_RP_VALID 1
typedef struct {
    float Rcw[9], tcw[3], Ow[3];  /* CurrentFrame.GetPose(), row-major; Tcw.inverse().translation() */
} orbgpu_reloc_pose;              /* 60 bytes */

int orbgpu_reloc_by_projection_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames,
                                     const orbgpu_reloc_point* pts, const int32_t* kf_offsets,
                                     const orbgpu_reloc_pose* poses, const float K[4], const uint8_t* kp_block,
                                     int kp_stride, float th, int orb_dist, int check_orientation, void* stream);
int orbgpu_download_reloc_matches(orbgpu_ctx* ctx, int pair, int32_t* match, int cap, int* n_kp,
                                  int* nmatches, int32_t rot_hist[30]);
/* The steps of MapPoint::PredictScale as a function of ratio = mfMaxDistance / dist3D (host
 * computation, no device): thresholds[n], n in [0, nlevels - 1), is the largest float r with
 * ceilf(logf(r) / logf(scale_factor)) <= n under the host libm, found by bisection over the float's
 * bit pattern, so that the clamped level is the number of thresholds below ratio.  The device counts
 * them: its own logf need not equal the host's near a step.  ORBGPU_ERR_INVALID: scale_factor not
 * above 1, nlevels outside [1, 16], a null table with nlevels > 1. */
int orbgpu_predict_scale_table(float scale_factor, int nlevels, float* thresholds);

/* ---- ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false) ----
 * The map-point fusion LocalMapping::SearchInNeighbors (LocalMapping.cc:726-815) runs right after
 * CreateNewMapPoints -- once per neighbour keyframe with the current keyframe's points, once on the
 * current keyframe with every neighbour's points -- cpp/src/ORBmatcher.cc:1155-1345, and the Sim3
 * overload LoopClosing::SearchAndFuse calls (:1347-1462, sim3 != 0: the same search without the
 * chi-square gate), with KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:706-755) and
 * MapPoint::PredictScale (MapPoint.cc:516-531), on pinhole keyframes (NLeft == -1: mvKeysUn, mvuRight).
 * Pair p fuses list lists[p] -- the points pts[list_offsets[l], list_offsets[l + 1]) -- into batch image
 * frames[p], inside the range of the last orbgpu_undistort_grid_batch, under pose p: Rcw, tcw, Ow of
 * pKF->GetPose() / GetCameraCenter(); for the Sim3 overload Scw.rotationMatrix(), Scw.translation() /
 * Scw.scale() and the inverse's translation (:1356-1357).  Several pairs may name one list
 * (SearchInNeighbors' forward leg: one upload of the current keyframe's points for all neighbours)
 * and several pairs one frame.  All arithmetic is IEEE single, evaluated in the reference's order.
 * The points do not see each other.  Each point i gets the decision code of the reference's count_*
 * debug counters (:1183):
 *   1. ORBGPU_FUSE_SKIPPED: the point lacks ORBGPU_FP_VALID (!pMP, isBad(), :1188-1198) or skip[p][i]
 *      is non-zero (IsInKeyFrame(pKF) :1199, spAlreadyFound.count :1372).
 *   2. ORBGPU_FUSE_NEG_DEPTH: p3Dc = Tcw * X, row by row as ((R0 x + R1 y) + R2 z) + t; zc < 0.0f
 *      (:1209).  invz = 1 / zc.
 *   3. ORBGPU_FUSE_NOT_IN_IMAGE: u = fx * xc / zc + cx, v = fy * yc / zc + cy (Pinhole.cpp:40-41) fail
 *      KeyFrame::IsInImage (KeyFrame.cc:752-755), u >= mnMinX && u < mnMaxX && v >= mnMinY && v < mnMaxY:
 *      half-open, unlike the relocalisation search's closed test.  A NaN or infinite projection fails
 *      it, as in the reference (zc == +-0 ends here).
 *   4. ORBGPU_FUSE_DISTANCE: ur = u - bf * invz; PO = X - Ow; dist3D = sqrtf((PO.x * PO.x + PO.y * PO.y)
 *      + PO.z * PO.z); dist3D < 0.8f * min_distance || dist3D > 1.2f * max_distance (:1234,
 *      MapPoint.cc:504-514).  Deviation: a dist3D or max_distance / dist3D that is not finite also
 *      gets this code (the reference would go on into PredictScale with it).
 *   5. ORBGPU_FUSE_NORMAL: (PO.x * n.x + PO.y * n.y) + PO.z * n.z < 0.5 * dist3D (:1242), compared in
 *      double: 0.5 is a double literal.
 *   6. nPredictedLevel = MapPoint::PredictScale(dist3D, pKF) as for orbgpu_reloc_by_projection_batch
 *      (orbgpu_predict_scale_table); radius = th * mvScaleFactors[level] (:1248-1251).
 *   7. ORBGPU_FUSE_EMPTY_WINDOW: KeyFrame::GetFeaturesInArea(u, v, radius) -- the cells of
 *      Frame::GetFeaturesInArea, columns, then rows, then the index within the cell, fabs(dx) < radius
 *      && fabs(dy) < radius, no level filter -- is empty (:1255), before any per-candidate filter.
 *   8. over that list in order: an octave outside [level - 1, level] is passed over (:1276); unless
 *      sim3, the chi-square gate (:1279-1303): with use_uright and mvuRight[k] >= 0, e2 = (ex * ex + ey *
 *      ey) + er * er (er = ur - mvuRight[k]) and the keypoint is passed over when (double)(e2 *
 *      mvInvLevelSigma2[octave]) > 7.8; otherwise e2 = ex * ex + ey * ey and the limit is 5.99.  The
 *      product is a float, the literals are doubles; a NaN product passes, as in the reference.  The
 *      best is the first lowest Hamming distance, strict < from 256.
 *   9. ORBGPU_FUSE_FUSED when bestDist <= 50 (TH_LOW, :1319), else ORBGPU_FUSE_ABOVE_TH_LOW
 *      (count_thcheck), also when every candidate was passed over.
 * Parity with the reference is unpinned, as for the other matcher functions: the yardstick is the
 * Python restatement in tests/test_fuse.py.
 * skip ([n_pairs][skip_stride] u8, host; NULL: none): [p][i] != 0 where point i of the pair's list is
 * already in keyframe p.  use_uright: the mvuRight row orbgpu_search_by_projection_batch reads for
 * that image, under that call's conditions: every frames[p] must then be the left image (2j) of a pair
 * j of the last orbgpu_stereo_matches_batch; with 0 every keypoint takes the monocular gate.  sim3 !=
 * 0 drops the gate and ignores bf and use_uright.  K = {fx, fy, cx, cy}; bf = pKF->mbf.  Host arrays
 * are pageable and may be reused when the call returns.
 * ORBGPU_ERR_INVALID: null context, n_pairs < 0 or above the context's image capacity, null arrays
 * with work to do, a frame outside the gridded range, lists[p] outside [0, n_lists), list_offsets not
 * ascending from a value >= 0, skip_stride below a named list's length, th or (unless sim3) bf
 * negative or not finite, the use_uright conditions not met.  ORBGPU_ERR_CAPACITY: a list above
 * ORBGPU_FUSE_MAX_POINTS.  n_pairs == 0 succeeds and leaves no pair to download.  Every status is
 * decided before any launch.
 * orbgpu_download_fuse_matches, per point of the pair's list: code[i]; best_dist[i] = the lowest
 * distance that survived the filters, 256 when none did or the point never reached them (the Sim3
 * overload starts from INT_MAX, so a 256-bit complement can become its bestIdx: it can never fuse,
 * and 256 stands for it); best_idx[i] = bestIdx when fused, else -1.  Per keypoint k of the frame:
 * first[k] = the lowest i that fused onto k, -1 if none.  *nfused = the reference's return value.
 * The host replays :1321-1337 / :1446-1456 from them: for i ascending with best_idx[i] = k >= 0, the
 * point met in pKF->GetMapPoint(k) is the keyframe's own if it holds one, else none when first[k] == i
 * (AddObservation / AddMapPoint), else point first[k] of the list.  *n_points = the list's length,
 * *n_kp = N; ORBGPU_ERR_CAPACITY when cap_points < *n_points or cap_kp < *n_kp (both counts are
 * written first); otherwise errors as for orbgpu_download_bow_matches.
 * Not built: the two-camera form (bRight, NLeft != -1: mvKeys / mvKeysRight, GetRightPose), SearchBySim3
 * (no caller in LoopClosing.cc), and the host-side Replace / AddObservation bookkeeping.  The Sim3
 * SearchByProjection overloads follow below. */
typedef struct {
    float pos[3];        /* pMP->GetWorldPos() */
    float normal[3];     /* pMP->GetNormal() */
    float min_distance;  /* pMP->mfMinDistance (the 0.8f factor is applied here) */
    float max_distance;  /* pMP->mfMaxDistance (1.2f for the gate, raw for PredictScale) */
    int32_t flags;       /* ORBGPU_FP_VALID: pMP && !pMP->isBad() */
    uint8_t desc[32];    /* pMP->GetDescriptor() */
} orbgpu_fuse_point;     /* 68 bytes */
#define ORBGPU_FP_VALID 1
#define ORBGPU_FUSE_MAX_POINTS 65536
#define ORBGPU_FUSE_SKIPPED 1
#define ORBGPU_FUSE_NEG_DEPTH 2
#define ORBGPU_FUSE_NOT_IN_IMAGE 3
#define ORBGPU_FUSE_DISTANCE 4
#define ORBGPU_FUSE_NORMAL 5
#define ORBGPU_FUSE_EMPTY_WINDOW 6
#define ORBGPU_FUSE_ABOVE_TH_LOW 7
#define ORBGPU_FUSE_FUSED 8

int orbgpu_fuse_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames, const int32_t* lists, int n_lists,
                      const orbgpu_fuse_point* pts, const int32_t* list_offsets, const orbgpu_reloc_pose* poses,
                      const float K[4], const uint8_t* skip, int skip_stride, float th, float bf, int use_uright,
                      int sim3, void* stream);
int orbgpu_download_fuse_matches(orbgpu_ctx* ctx, int pair, int32_t* best_idx, int32_t* best_dist, uint8_t* code,
                                 int cap_points, int32_t* first, int cap_kp, int* n_points, int* n_kp, int* nfused);

/* ---- ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) ----
 * cpp/src/ORBmatcher.cc:428-533, and the overload that also carries vpPointsKFs / vpMatchedKF (:535-647):
 * the searches LoopClosing::DetectCommonRegionsFromBoW runs on a candidate's covisible points
 * (LoopClosing.cc:755: th 8, ratio 1.5, the vpPointsKFs form; :777: th 5, ratio 1.0) and
 * FindMatchesByProjection runs for every keyframe while a loop or merge is being confirmed (:964: th 3,
 * ratio 1.5), with KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:706-755) and MapPoint::PredictScale
 * (MapPoint.cc:516-531), on pinhole keyframes (NLeft == -1: mvKeysUn).
 * Pair p searches list lists[p] -- the points pts[list_offsets[l], list_offsets[l + 1]), orbgpu_fuse_point
 * rows -- in batch image frames[p], inside the range of the last orbgpu_undistort_grid_batch, under pose p:
 * Rcw = Scw.rotationMatrix(), tcw = Scw.translation() / Scw.scale(), Ow = Tcw.inverse().translation()
 * (:437-438, :544-545).  Each pair is one call of the reference with its own vpMatched: pairs do not see
 * each other, several pairs may name one list and several pairs one frame (the coarse searches of several
 * candidates for one current keyframe in one call).  All arithmetic is IEEE single without contraction,
 * evaluated in the reference's order.  Points are taken in ascending index; each gets one decision code:
 *   1. ORBGPU_SIM3_SKIPPED: the point lacks ORBGPU_FP_VALID (isBad()) or skip[p][i] is non-zero
 *      (spAlreadyFound.count(pMP), :452, :560).
 *   2. ORBGPU_SIM3_NEG_DEPTH: p3Dc = Tcw * X, row by row as ((R0 x + R1 y) + R2 z) + t; zc < 0.0 (:462, :570).
 *   3. ORBGPU_SIM3_NOT_IN_IMAGE: the projection fails KeyFrame::IsInImage (KeyFrame.cc:752-755), u >= mnMinX
 *      && u < mnMaxX && v >= mnMinY && v < mnMaxY, half-open; a NaN or infinite projection fails it.  The
 *      projection is where the overloads differ: projection == ORBGPU_SIM3_PROJECT_DIV is the first one,
 *      through Pinhole::project (Pinhole.cpp:40-41), u = fx * xc / zc + cx; ORBGPU_SIM3_PROJECT_INVZ is the
 *      second (:574-579), invz = 1 / zc; x = xc * invz; u = fx * x + cx.  The two round differently: a point
 *      can be inside the image or a window under one and outside under the other.
 *   4. ORBGPU_SIM3_DISTANCE: PO = X - Ow; dist = sqrtf((PO.x * PO.x + PO.y * PO.y) + PO.z * PO.z); dist <
 *      0.8f * min_distance || dist > 1.2f * max_distance (:473-479, MapPoint.cc:504-514).  Deviation, as for
 *      orbgpu_fuse_batch: a dist or max_distance / dist that is not finite also gets this code.
 *   5. ORBGPU_SIM3_NORMAL: (PO.x * n.x + PO.y * n.y) + PO.z * n.z < 0.5 * dist, compared in double (:484, :597).
 *   6. nPredictedLevel = the number of orbgpu_predict_scale_table steps below max_distance / dist; radius =
 *      th * mvScaleFactors[level] (:487-490; th is an int in the reference, a float here as elsewhere).
 *   7. ORBGPU_SIM3_EMPTY_WINDOW: KeyFrame::GetFeaturesInArea(u, v, radius), without a level filter, is empty
 *      (:494).  This is decided before occupancy is looked at: a window whose every keypoint is taken is
 *      not empty.
 *   8. over that list in window order (grid column, row, index within the cell): a keypoint with
 *      vpMatched[idx] set -- held before the call (kp_block) or taken earlier in this call -- is passed over
 *      (:505, :618); an octave outside [level - 1, level] is passed over (:510); the best is the first lowest
 *      Hamming distance, strict < from 256.
 *   9. ORBGPU_SIM3_MATCHED when (float)bestDist <= 50.0f * ratio_hamming (TH_LOW * ratioHamming, :524: the
 *      product is a float and so is the compare): vpMatched[bestIdx] = pMP, the keypoint is taken, nmatches++.
 *      Otherwise ORBGPU_SIM3_NOT_MATCHED, also when every candidate was passed over; such a point takes nothing.
 * The reference would write vpMatched[-1] if the limit reached 256, so such a ratio_hamming is refused.
 * Parity with the reference is unpinned, as for the other matcher functions: the yardstick is the Python
 * restatement in tests/test_sim3_projection.py.
 * skip ([n_pairs][skip_stride] u8, host; NULL: none) as for orbgpu_fuse_batch; kp_block ([n_pairs][kp_stride]
 * u8, host; NULL: none): [p][k] != 0 where vpMatched[k] is set before the call.  K = {fx, fy, cx, cy}.  Host
 * arrays are pageable and may be reused when the call returns.
 * ORBGPU_ERR_INVALID: null context, n_pairs < 0 or above the context's image capacity, null arrays with work
 * to do, a frame outside the gridded range, lists[p] outside [0, n_lists), list_offsets not ascending from a
 * value >= 0, skip_stride below a named list's length, kp_stride below a frame's keypoint count, th negative
 * or not finite, ratio_hamming not finite or 50.0f * ratio_hamming outside [0, 256), projection outside
 * {0, 1}.  ORBGPU_ERR_CAPACITY: a list above ORBGPU_FUSE_MAX_POINTS, or a keypoint capacity above the resolve
 * kernel's LDS budget.  n_pairs == 0 succeeds and leaves no pair to download.  Every status is decided before
 * any launch.  The results live in buffers of their own: they outlive the other searches' calls and leave
 * the other searches' results alone.
 * orbgpu_download_sim3_matches, per keypoint k of the frame: match[k] = the list index of the point this
 * call put on k, else -1 (a keypoint held before the call stays -1); the vpMatchedKF of the second overload
 * needs nothing more: vpMatchedKF[k] = vpPointsKFs[match[k]] (:640).  Per point of the pair's list: code[i];
 * best_idx[i] = the keypoint when matched, else -1; best_dist[i] = its distance when matched, else 256.
 * *nmatches = the reference's return value.  *n_kp = N, *n_points = the list's length; ORBGPU_ERR_CAPACITY
 * when cap_kp < *n_kp or cap_points < *n_points (both counts are written first); otherwise errors as for
 * orbgpu_download_bow_matches.
 * orbgpu_sim3_replay_stats (measurement, tools/sim3_search_time.py): what the replay of pair `pair` did:
 * {points that reached it, passes, lanes found stale over all passes, windows walked again}.
 * Not built: the two-camera form (NLeft != -1), SearchBySim3, and the Sim3Solver / Optimizer::OptimizeSim3
 * between the calls. */
#define ORBGPU_SIM3_PROJECT_DIV 0  /* :428, Pinhole::project */
#define ORBGPU_SIM3_PROJECT_INVZ 1 /* :535, the invz form */
#define ORBGPU_SIM3_SKIPPED 1
#define ORBGPU_SIM3_NEG_DEPTH 2
#define ORBGPU_SIM3_NOT_IN_IMAGE 3
#define ORBGPU_SIM3_DISTANCE 4
#define ORBGPU_SIM3_NORMAL 5
#define ORBGPU_SIM3_EMPTY_WINDOW 6
#define ORBGPU_SIM3_NOT_MATCHED 7
#define ORBGPU_SIM3_MATCHED 8

int orbgpu_sim3_search_by_projection_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames, const int32_t* lists,
                                           int n_lists, const orbgpu_fuse_point* pts, const int32_t* list_offsets,
                                           const orbgpu_reloc_pose* poses, const float K[4], const uint8_t* skip,
                                           int skip_stride, const uint8_t* kp_block, int kp_stride, float th,
                                           float ratio_hamming, int projection, void* stream);
int orbgpu_download_sim3_matches(orbgpu_ctx* ctx, int pair, int32_t* match, int cap_kp, int32_t* best_idx,
                                 int32_t* best_dist, uint8_t* code, int cap_points, int* n_kp, int* n_points,
                                 int* nmatches);
int orbgpu_sim3_replay_stats(orbgpu_ctx* ctx, int pair, int32_t stats[4]);

/* ---- ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) ----------
 * The matcher LoopClosing::DetectCommonRegionsFromBoW runs on ORBmatcher(0.9, true) for the current keyframe
 * against the candidate and each of its 5 covisibles, for up to 3 candidates (LoopClosing.cc:657-668): 6 to 18
 * calls per new keyframe, whose matches feed the Sim3Solver: cpp/src/ORBmatcher.cc:766-906 with
 * ComputeThreeMaxima :2061-2102, on pinhole keyframes (NLeft == -1 on both).  Pair p = keyframe 1, which is
 * image frames[p] of the last orbgpu_run_batch (its descriptors and angles only: undistortion does not change
 * mvKeysUn[i].angle, so orbgpu_undistort_grid_batch is not needed), against keyframe 2, given by the host as
 * kf_pts [kf_offsets[p], kf_offsets[p + 1]); several pairs may name the same frame: one current keyframe against
 * 6 to 18 keyframes is one call.  The vocabulary stays on the host: the node of each keypoint (mFeatVec) is an
 * input on both sides.  It is the mirror of orbgpu_search_by_bow_batch, not the same search with the sides
 * swapped: the batch image is the outer, sequential side, the taken bits live on the host-given side, both sides
 * carry a map-point flag and the distance gate is strict.  All arithmetic is IEEE single, in the reference's
 * order:
 *   1. match12 has keyframe 1's N1 entries, all -1 (:778); vbMatched2 is all false (:779).
 *   2. only the nodes present in both feature vectors are visited (:794-883); nodes do not interact; a node's
 *      list holds keypoint indices in ascending order.
 *   3. in a common node, for idx1 ascending (:798): a keypoint 1 without ORBGPU_BOWKF_HAS_POINT (vpMapPoints1
 *      [idx1] && !isBad()) is skipped (:805-809).  The NLeft test at :801 cannot fire on pinhole keyframes; a host
 *      that feeds a two-camera keyframe 1 would clear the flag of the keypoints that test skips.
 *   4. for idx2 ascending (:817): a keypoint 2 that is taken (vbMatched2) or lacks ORBGPU_BOWKF_HAS_POINT is
 *      passed over (:825-831): it is neither the best nor the second best.  Best and second best with strict <
 *      from 256 / 256 (:837-846): an equal distance becomes the second best, never the best.
 *   5. a match when bestDist1 < TH_LOW = 50 (:849: 49 passes, 50 fails; orbgpu_search_by_bow_batch has <=) and
 *      (float)bestDist1 < nnratio * (float)bestDist2 (:851; a lone candidate has bestDist2 = 256): match12[idx1] =
 *      bestIdx2, keypoint 2 is taken, nmatches++; with check_orientation, rot = angle1[idx1] - angle2[bestIdx2]
 *      (+360 if negative), bin = round(rot * (1.0f / 30)) (30 -> 0), and idx1 enters that bin (:856-866).
 *   6. ComputeThreeMaxima on the 30 bin sizes; every entry of a bin outside the three maxima is cleared and takes
 *      one off nmatches (:885-903).  A cleared match does not free its keypoint 2 for anyone: nothing reads
 *      vbMatched2 after the loop.
 * Deviations: a negative node means "this keypoint is in no node"; an event whose bin falls outside [0, 30)
 * (the reference asserts) counts in nmatches, enters no bin and cannot be rejected.  Parity with the reference
 * is unpinned, as for the other matcher functions: the yardstick is the Python restatement in
 * tests/test_search_by_bow_kf.py.
 * f_nodes: [n_pairs][node_stride], the node of keypoint k of pair p's keyframe 1 at [p][k]; f_flags:
 * [n_pairs][flag_stride] u8, bit 0 = ORBGPU_BOWKF_HAS_POINT of that keypoint, NULL: every keypoint 1 has a map
 * point.  Host arrays are pageable and may be reused when the call returns.
 * ORBGPU_ERR_INVALID: null context, n_pairs < 0 or above the context's image capacity, null arrays when n_pairs
 * > 0, a frame outside the last batch, kf_offsets not ascending from a value >= 0, a stride below a frame's
 * keypoint count, a nnratio that is not finite; n_pairs == 0 succeeds and leaves no pair to download.
 * ORBGPU_ERR_CAPACITY when a side holds more than ORBGPU_BOW_MAX_POINTS keypoints (the context's keypoint
 * capacity per image counts for keyframe 1).  Every status is decided before any launch.  The results live in
 * buffers of their own: they outlive the other searches' calls and leave the other searches' results alone.
 * orbgpu_download_bow_kf_matches, per keypoint k of keyframe 1 (each array may be NULL): match12[k] = the
 * index, within the pair's keyframe points, that the reference leaves in vpMatches12[k] (vpMatches12[k] =
 * vpMapPoints2[match12[k]]), -1 if none; code[k] = the decision it ended with, ORBGPU_BOWKF_*; best[2 k], best[2 k
 * + 1] = bestDist1, bestDist2 of its walk (a side that found nothing holds 256; both are 0 for the codes
 * NO_NODE, NODE_NOT_COMMON and NO_MAP_POINT, which never walk).  *n1 = N1; *nmatches = the reference's return
 * value; rot_hist = the 30 bin sizes before the three-maxima rule (all 0 when check_orientation == 0).  Errors
 * as for orbgpu_download_bow_matches.
 * Not built: the two-camera form, and the union over a candidate's covisibles (LoopClosing.cc:670-687), which
 * needs map-point identity: the host runs it over the downloaded rows. */
typedef orbgpu_bow_point orbgpu_bowkf_point; /* desc, angle, node, flags of a keypoint of keyframe 2; 44 bytes */
#define ORBGPU_BOWKF_HAS_POINT 1          /* vpMapPoints[i] && !isBad(): ORBGPU_BOW_HAS_POINT's bit */
#define ORBGPU_BOWKF_NO_NODE 1            /* the keypoint's node is negative */
#define ORBGPU_BOWKF_NODE_NOT_COMMON 2    /* keyframe 2 has no keypoint in its node */
#define ORBGPU_BOWKF_NO_MAP_POINT 3       /* :805-809 */
#define ORBGPU_BOWKF_NO_CANDIDATE 4       /* every keypoint 2 of the node taken or without a point: bestIdx2 == -1 */
#define ORBGPU_BOWKF_NOT_BELOW_TH_LOW 5   /* :849 */
#define ORBGPU_BOWKF_RATIO_FAILED 6       /* :851 */
#define ORBGPU_BOWKF_MATCHED 7
#define ORBGPU_BOWKF_ROTATION_REJECTED 8  /* matched, then cleared by the three-maxima rule */

int orbgpu_search_by_bow_kf_batch(orbgpu_ctx* ctx, int n_pairs, const int32_t* frames,
                                  const orbgpu_bowkf_point* kf_pts, const int32_t* kf_offsets,
                                  const int32_t* f_nodes, int node_stride, const uint8_t* f_flags, int flag_stride,
                                  float nnratio, int check_orientation, void* stream);
int orbgpu_download_bow_kf_matches(orbgpu_ctx* ctx, int pair, int32_t* match12, uint8_t* code, int16_t* best,
                                   int cap, int* n1, int* nmatches, int32_t rot_hist[30]);

/* ---- wire formats ---------------------------------------------------------------------------
 * Ingest of side-by-side stereo Y8 frames (the headset's 2W x H AHardwareBuffer,
 * ORBextractor.cc:131-143; DSP split orbslam_dsp.cpp:643-648): frame f's left half (columns
 * [0, W)) becomes batch image 2f, its right half (columns [W, 2W)) image 2f + 1.  Frames are
 * height rows of `stride` bytes (stride >= 2W), height * stride bytes apart.
 *   orbgpu_upload_sbs: host frames (PCIe into a staging buffer, then the split kernel);
 *   orbgpu_ingest_sbs: frames already in device memory (e.g. the staging buffer returned by
 *   orbgpu_device_sbs_input, sized for max_images / 2 frames of stride 2 * max_width), on
 *   `stream` -- the zero-copy path. */
uint8_t* orbgpu_device_sbs_input(orbgpu_ctx* ctx);
int orbgpu_upload_sbs(orbgpu_ctx* ctx, const uint8_t* frames, int n_frames, int width, int height,
                      int stride);
int orbgpu_ingest_sbs(orbgpu_ctx* ctx, const uint8_t* device_frames, int n_frames, int width,
                      int height, int stride, void* stream);

/* Egress in the FastRPC result layout (cpp/inc/orbslam3.idl:15-19): per image int32 X, Y (the
 * level-0 coordinates truncated to int), angle ((cos8 & 0xFF) | (sin8 & 0xFF) << 8 with
 * cos8/sin8 = rint(64 cos / 64 sin) of the keypoint angle: what LynxHardwareAccelerator.cpp:
 * 174-178 decodes), level (octave) and the N x 32 B descriptors; per stereo pair the kNN result
 * as int16 indices / distances1 / distances2 (distances clamped to 32767; absent = -1 / 32767).
 * orbgpu_pack_soa converts the first n_images images and n_pairs pairs of the last batch on the
 * device (device-resident SoA), the download functions copy one image / pair out. */
int orbgpu_pack_soa(orbgpu_ctx* ctx, int n_images, int n_pairs, void* stream);
int orbgpu_download_soa(orbgpu_ctx* ctx, int image, int32_t* x, int32_t* y, int32_t* angle,
                        int32_t* level, uint8_t* orb, int cap, int* count, int* mono);
int orbgpu_download_matches16(orbgpu_ctx* ctx, int pair, int16_t* indices, int16_t* dist1,
                              int16_t* dist2, int cap, int* n_queries);

/* orbslam3_extractFeatures (orbslam3.idl:15-19, impl orbslam_dsp.cpp:1003-1087) in one call: one
 * side-by-side frame in, both eyes extracted (lapping areas {l0, l1} / {r0, r1}), the stereo
 * rows ([mono, n) of each eye, Frame.cc:1142-1148) kNN2-matched left -> right, everything out in
 * the SoA layout above.  `threshold` is accepted and ignored, as the DSP does; the context's
 * FAST thresholds apply.  *count_* is the exact keypoint count (the DSP's host wrapper subtracts
 * one from its count, LynxHardwareAccelerator.cpp:158-159; a caller of this ABI must not). */
int orbgpu_extract_features(orbgpu_ctx* ctx, const uint8_t* image, int image_len, int width,
                            int height, int stride, int threshold, int lap_l0, int lap_l1,
                            int lap_r0, int lap_r1, int* count_l, int32_t* x_l, int32_t* y_l,
                            int32_t* angle_l, int32_t* level_l, uint8_t* orb_l, int* count_r,
                            int32_t* x_r, int32_t* y_r, int32_t* angle_r, int32_t* level_r,
                            uint8_t* orb_r, int kp_cap, int* mono_l, int* mono_r, int16_t* indices,
                            int16_t* dist1, int16_t* dist2, int match_cap);

/* ---- Frame post-processing ----------------------------------------------------------------
 * Frame::UndistortKeyPoints (cpp/src/Frame.cc:763-796; cv::undistortPoints with P = K, 5
 * iterations in double) and Frame::AssignFeaturesToGrid + PosInGrid (:405-436, 741-751; 64 x 48
 * cells, Frame.h:46-47) for the first n_images images of the last orbgpu_run_batch.
 * K = {fx, fy, cx, cy}; dist = {k1, k2, p1, p2[, k3]} (ndist 0, 4 or 5; k1 == 0: no undistortion,
 * as :765).  The grid spans Frame::ComputeImageBounds (:798-825) of the batch image size, which
 * orbgpu_image_bounds returns ({mnMinX, mnMaxX, mnMinY, mnMaxY}, host computation).
 * Per image: undistorted positions (mvKeysUn.pt), the cell of each keypoint (posX * 48 + posY,
 * -1 outside the grid) and the cells as CSR lists (cell_start[64*48 + 1], cell_idx: keypoint
 * indices ascending within a cell = mGrid[posX][posY]). */
int orbgpu_image_bounds(int cols, int rows, const float K[4], const float* dist, int ndist, float bounds[4]);
int orbgpu_undistort_grid_batch(orbgpu_ctx* ctx, int n_images, const float K[4], const float* dist,
                                int ndist, void* stream);
int orbgpu_download_grid(orbgpu_ctx* ctx, int image, float* xy_un, int32_t* cell, int32_t* cell_start,
                         int32_t* cell_idx, int cap, int* n);

/* ORBmatcher::DescriptorDistance on two 32-byte descriptors (host, no device work). */
int orbgpu_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* ---- instrumentation ----------------------------------------------------------------------
 * enable = 1: every kernel launch of run_batch/match_stereo_batch is bracketed by HIP events on
 * its stream; enable = (1 << 31) | mask: only the stages whose bit is set; 0: off.  Adding
 * (1 << 30) also launches every stage once over the whole batch (no sub-batch overlap), so each
 * launch's duration is that kernel's alone.
 * orbgpu_stage_times returns the summed milliseconds and launch counts per stage since the last
 * reset.  Stage names via orbgpu_stage_name. */
int orbgpu_set_profiling(orbgpu_ctx* ctx, int enable);
int orbgpu_num_stages(void);
const char* orbgpu_stage_name(int stage);
int orbgpu_stage_times(orbgpu_ctx* ctx, double* ms, int64_t* launches, int max_stages);
int orbgpu_reset_stage_times(orbgpu_ctx* ctx);

/* Measurement knobs (ORBGPU_STREAMS, ORBGPU_OCT_SPLIT, ORBGPU_FAST_PITCH, ...) change launch
 * shapes and kernel variants; the library reads them only when ORBGPU_DIAGNOSTICS=1 is also set.
 * Writes the knobs in effect as "NAME=value;..." (NUL-terminated, truncated to cap) and returns
 * their count: 0 in a deployment. */
int orbgpu_diagnostic_knobs(char* buf, size_t cap);

const char* orbgpu_last_error(void);
int orbgpu_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBGPU_H_ */
