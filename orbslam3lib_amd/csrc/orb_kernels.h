// orb_kernels.h -- launch-argument structs shared by the kernel files and the host runtime
// (orb_geometry.h fills them, orb_runtime.cpp, orb_post.cpp and orb_matchers.cpp bind the pointers and launch).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace orbgpu {

constexpr int kMaxLevels = 16;
constexpr int kMinBorder = 16;   // EDGE_THRESHOLD - 3 (ORBextractor_old.cc:791)
constexpr int kEdge = 19;        // EDGE_THRESHOLD (:75)

// XCD-aware block order (cdna_hip_programming.md T1, bijective form): the dispatcher places
// block b on XCD b % 8, so a grid walked in (b % 8, b / 8) order gives every XCD one
// contiguous range of work -- neighbouring cells / tiles of one image then share that XCD's L2
// instead of being fetched once per XCD.  Speed only: any placement stays correct.
__device__ inline int xcd_remap(int orig, int nwg) {
    const int xcd = orig % 8, q = nwg / 8, r = nwg % 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// Per-level geometry, computed on the host (orb_geometry.h plan_geometry) from the reference formulas.
struct LevelGeom {
    int w, h, pitch;           // plane size; pitch in bytes (level 0: the input's row stride)
    long long img_stride;      // bytes between images for this level's plane
    int bpitch;                // blurred plane pitch (multiple of 64)
    long long bimg_stride;     // bytes between images for the blurred plane
    int nCols, nRows, wCell, hCell, maxBX, maxBY;  // cell grid (:787-805)
    int ncells, cell_cap;      // cells in this level, key capacity per cell
    int cell_first;            // flattened index of this level's first cell
    long long cellkey_off;     // offset (in keys) of this level's cell-key region in an image
    int cellcnt_off;           // offset (in cells) of this level's counts in an image
    int cand_cap;              // ncells * cell_cap
    int N;                     // mnFeaturesPerLevel[level]
    int W, H;                  // octree extents maxBorder - minBorder
    int kp_cap;                // octree output capacity
    int kp_off;                // offset (in keypoints) in an image's level-keypoint region
    int oct_cap;               // node capacity of the octree workspace
    long long oct_off;         // byte offset of this level's octree workspace in an image
    float scale;               // mvScaleFactor[level]
    int patch;                 // (int)(PATCH_SIZE * scale) (:882)
    int tiles_x, tiles_y, tile_first;  // blur tiling (128 x 32)
    int xtab_off, ytab_off, simd_end;  // resize tables (levels >= 1)
    int area2;                 // exact 2x downscale: OpenCV switches to INTER_AREA (2x2 mean)
    // k_blur_resize (levels >= 1): ownership of this level's output rows / column quads by the
    // 128 x 32 blur tiles of level l - 1 (int views of rtab): band_row[b] = first output row whose
    // first source row is >= 32 b (tiles_y(l-1) + 1 entries), tile_quad[j] = first quad whose first
    // source column is >= 128 j (tiles_x(l-1) + 1 entries)
    int band_row_off, tile_quad_off;
    // the resize tables as the resize reads them (levels >= 1 that are not area2), written once by
    // the host: qrec_off = rtab index of two int4 per output quad (its four tap selector pairs, its
    // four coefficient pairs times 16), qbase_off = int view of rtab: the quad's first left tap,
    // yrec_off = rtab index of one int4 per output row {sy0, sy1, b0 << 8, b1 << 8}
    int qrec_off, qbase_off, yrec_off;
    int od_blocks, od_first;   // orientation/descriptor blocks for this level
    int tpitch;                // k_pyr_tail: LDS row pitch of this level (levels >= tail0 - 1)
};

struct BatchArgs {
    int nlevels, nimages;
    int img0;                        // first image of this launch (sub-batches on parallel streams)
    int ini_th, min_th;
    LevelGeom lv[kMaxLevels];
    uint8_t* lvl_base[kMaxLevels];   // plane base of image 0 (level 0 = the input buffer)
    uint8_t* blur_base[kMaxLevels];
    const int4* rtab;                // resize tables (x: {sx,sx1,a0,a1}, y: {sy0,sy1,b0,b1})
    uint32_t* cellkeys;              // [img][cand region]
    long long cellkeys_img_stride;   // keys
    int32_t* cellcnt;                // [img][cells]
    int cellcnt_img_stride;
    uint8_t* octws;                  // [img][octree workspace]
    long long octws_img_stride;
    uint32_t* lvlkey;                // [img][level kps] packed key
    float* lvlangle;                 // [img][level kps]
    uint8_t* lvldesc;                // [img][level kps][32]
    int lvlkp_img_stride;            // keypoints
    int32_t* lvlcnt;                 // [img][kMaxLevels]
    int32_t* status;                 // [img][kMaxLevels]
    void* out_kps;                   // orbgpu_keypoint [img][out_cap]
    uint8_t* out_desc;               // [img][out_cap][32]
    int out_cap;
    int32_t* out_n;                  // [img]
    int32_t* out_mono;               // [img]
    const int32_t* laps;             // [img][2]
    int total_cells, total_tiles, total_od_blocks;
    int fast_tab_off;  // rtab index of k_fast_cells' per-cell records (2 int4 per flattened cell)
    int od_tab_off;    // rtab index of k_orient_desc's per-block records {level, block, 0, 0}
    int fast_n48;  // k_fast_cells records [0, fast_n48) run the 48-byte FAST tile,
    int fast_n64;  // [fast_n48, fast_n64) the 64-byte one, the rest the 80-byte one (records are
                   // grouped by tile, levels in order inside each group)
    // k_fast_cells' small-list path (48- and 64-byte tiles): queued overflow cells [img][fast_qcap] as
    // (image, cell), counters [2 * img0] per launch (queued, finished overflow workgroups);
    // fast_small: -1 for launches of more than kFastMergeMaxImages images, 0 never, 1 always
    // (diagnostics); fast_ovf_all (diagnostics): every small-path cell goes to the overflow pass
    int2* fast_ovf;
    int* fast_ovf_cnt;
    int fast_qcap;  // queue entries per image: the 48- and 64-byte tiles' cells
    int fast_small, fast_ovf_all;
    unsigned long long* octdbg;      // diagnostic: [img][kMaxLevels][8] phase clocks, or null
    int oct_lds_nodes;               // node capacity of k_octree's dynamic LDS (0: all global)
    int oct_lds_bytes;
    int oct_nq_off;                  // byte offset of the per-key labels in that LDS
    // levels [oct_split, nlevels) run in a second k_octree launch of kOctSmallThreads-thread
    // workgroups with their own, smaller LDS layout (more workgroups per CU for the short levels)
    int oct_split;
    int oct_split_min_images;        // below this many images per launch: every level at 512 threads
    int oct2_threads;                // 128 or 256
    int oct2_lds_nodes, oct2_lds_bytes, oct2_nq_off, oct2_lds_keys;
    int oct_may_retry;               // some level can exceed the LDS instantiation of k_octree
    int oct_force_retry;             // diagnostics: every level through the generic instantiation
    int oct_pyr_max;                 // deepest count pyramid of k_octree (0: label passes only)
    int oct_rounds;                  // diagnostics: phase 1 round by round with the pyramid too
    // k_pyr_tail: levels [tail0, nlevels) and the blurs of [tail0 - 1, nlevels) in one launch
    // (tail0 = nlevels + 1: no tail, k_blur_resize for every level and k_blur for the last)
    int tail0;
    int tail_lds, tail_buf1, tail_tab, tail_maxq, tail_maxrows;  // its LDS layout (bytes / entries)
    int tail_min;              // launches of fewer images take the per-level path (host only)
    int fuse_out;              // no image of the batch has a lapping area: k_orient_desc writes the
                               // assembled outputs and counts, k_finalize does not run
};
static_assert(sizeof(BatchArgs) <= 4096, "kernel argument block too large");

struct MatchArgs {
    const uint8_t* desc;      // out_desc
    const int32_t* out_n;
    const int32_t* out_mono;
    int out_cap;
    int stereo_only;
    int32_t* idx1;
    int32_t* dist1;
    int32_t* idx2;
    int32_t* dist2;           // [pair][out_cap]
    int32_t* nq;              // [pair]
    int pair0;                // first pair of this launch
    uint2* part;              // [kKnnSplitSlots][out_cap] partial top-2 keys of split launches, or null
    uint32_t* cnt;            // split launches: per (pair, query block) arrival counters (zero between
                              // launches), so the last split workgroup merges; null: k_knn2_merge does
    int cnt_slots;            // counters allocated at cnt (launch_knn2_pairs checks the grid fits)
};
#ifndef KNN_SPLIT
// round 5, C4 step (one pair, tools/c4_time.py): 4 splits 126.6-126.9 us, 8 splits 125.2-125.5,
// 16 splits 126.6-126.9
#define KNN_SPLIT 8
#endif
constexpr int kKnnMaxSplit = KNN_SPLIT;     // train-row splits of a launch with few pairs
constexpr int kKnnSplitSlots = KNN_SPLIT;   // pairs x splits the partial buffer holds (1 pair: KNN_SPLIT splits)
// queries per k_knn2_mfma_pairs workgroup (orb_knn2.hip); the grid's x extent is
// ceil(out_cap / kKnnQueries) query blocks per pair
constexpr int kKnnQueries = 256;
// arrival counters of the fused split merge: one per (pair of the launch, query block); a split
// launch has at most kKnnSplitSlots / 2 pairs (orb_post.cpp orbgpu_match_stereo_batch), sized for kKnnSplitSlots
__host__ inline size_t knn2_counter_slots(int out_cap) {
    return (size_t)kKnnSplitSlots * (size_t)((out_cap + kKnnQueries - 1) / kKnnQueries);
}

// Frame::ComputeStereoMatches over a batch's device-resident results (orb_stereo.hip).
struct StereoArgs {
    const void* kps;                 // out_kps: orbgpu_keypoint [img][out_cap]
    const uint8_t* desc;             // out_desc: [img][out_cap][32]
    const int32_t* out_n;            // [img]
    int out_cap;
    int nlevels, H0;                 // levels, rows of level 0
    const uint8_t* lvl_base[kMaxLevels];  // unblurred pyramid (mvImagePyramid), image 0
    long long limg_stride[kMaxLevels];
    int lw[kMaxLevels], lh[kMaxLevels], lpitch[kMaxLevels];
    float scale[kMaxLevels], inv_scale[kMaxLevels];  // mvScaleFactors / mvInvScaleFactors
    float mbf, mb;                   // Frame::mbf, Frame::mb
    int32_t* row_start;              // [pair][H0 + 1] right keypoints by row (CSR)
    int32_t* row_idx;                // [pair][out_cap]
    float* u_right;                  // [pair][out_cap] mvuRight
    float* depth;                    // [pair][out_cap] mvDepth
    int32_t* sad;                    // [pair][out_cap] accepted SAD distance, -1 if none
    int pair0;                       // first pair of this launch
};

// Frame::ComputeStereoFishEyeMatches over a batch (orb_fisheye.hip): pair p = left image 2p,
// right image 2p+1, on the stereo-row kNN2 of orbgpu_match_stereo_batch(stereo_only = 1).
struct FisheyeArgs {
    const void* kps;                 // out_kps: orbgpu_keypoint [img][out_cap]
    const int32_t* out_n;            // [img]
    const int32_t* out_mono;         // [img]
    int out_cap;
    const int32_t* idx1;             // [pair][out_cap] kNN2 best train row (stereo rows)
    const int32_t* dist1;            // [pair][out_cap]
    float cam_l[8], cam_r[8];        // KannalaBrandt8 mvParameters: fx fy cx cy k0 k1 k2 k3
    float prec_l, prec_r;            // KannalaBrandt8::precision
    float R12[9], t12[3];            // Frame::mRlr (row-major), Frame::mtlr
    float sigma2[kMaxLevels];        // mvLevelSigma2
    int32_t* l2r;                    // [pair][out_cap] mvLeftToRightMatch
    int32_t* r2l;                    // [pair][out_cap] mvRightToLeftMatch (pre-set to -1)
    float* depth;                    // [pair][out_cap] mvDepth
    float* p3d;                      // [pair][out_cap][3] mvStereo3Dpoints
    int32_t* counts;                 // [pair][2] nMatches, descMatches (pre-set to 0)
    int pair0;                       // first pair of this launch
};
hipError_t launch_fisheye(const FisheyeArgs& f, int npairs, hipStream_t s);

// Frame::UndistortKeyPoints + AssignFeaturesToGrid over a batch's keypoints (orb_frame.hip).
constexpr int kGridCols = 64, kGridRows = 48;  // FRAME_GRID_COLS / ROWS (Frame.h:46-47)
struct GridArgs {
    const void* kps;       // out_kps: orbgpu_keypoint [img][out_cap]
    const int32_t* out_n;  // [img]
    int out_cap;
    int undistort;         // mDistCoef(0) != 0 (Frame.cc:765)
    float K[4];            // fx fy cx cy
    double k[14];          // OpenCV distortion vector (k1 k2 p1 p2 k3, rest 0)
    float bounds[4];       // mnMinX mnMaxX mnMinY mnMaxY
    float grid_inv[2];     // mfGridElementWidthInv / HeightInv
    float* xy_un;          // [img][out_cap][2] mvKeysUn positions
    int32_t* cell;         // [img][out_cap] posX * 48 + posY or -1
    int32_t* cell_start;   // [img][64 * 48 + 1]
    int32_t* cell_idx;     // [img][out_cap]
    int img0;
};

// Octree workspace layout for one (image, level) with n_cap keys and node capacity C.  The node
// state lives in LDS when C <= kOctLdsNodes, otherwise in the `nodemem` part of this block.
constexpr int kOctLdsNodes = 1024;
constexpr int kOdKpBlock = 8;  // keypoints per k_orient_desc pass (256 threads, 32 lanes per keypoint)
// keypoints per k_orient_desc workgroup by default: 3 passes of kOdKpBlock.  Round 5, chunked
// moments, single stream per 512 images: 1 pass 553 us, 2 passes 483, 3 passes 463, 4 passes 467;
// headline at 3 vs 2 passes +0.2 to +2.3% (bench A/B, 3 rounds).  Contexts of a few images take 1
// (orb_geometry.h plan_geometry).
constexpr int kOdBlockKps = 3 * kOdKpBlock;

constexpr int kOctLdsKeys = 16384;  // per-key node labels (u16) kept in LDS up to this many keys
constexpr int kFastMergeMaxImages = 4;  // launches this small run the 48/64 FAST cells as one launch
// candidate list of the small-list k_fast_cells<48> / <64> (orb_fast.hip), split over the waves
template <int CP>
constexpr int kFastSmallList() { return CP == 48 ? 512 : 1280; }
constexpr int kFastOvfBlocks = 32;      // workgroups of k_fast_cells_ovf
// FAST cells of the levels that run the `tile`-byte LDS tile (48, 64 or kCellMax = 80): their
// flattened cell range (smaller tiles = less LDS per workgroup = more cells resident per CU)
inline void fast_cell_range(const BatchArgs& a, int tile, int* c0, int* c1) {
    *c0 = tile == 48 ? 0 : tile == 64 ? a.fast_n48 : a.fast_n64;
    *c1 = tile == 48 ? a.fast_n48 : tile == 64 ? a.fast_n64 : a.total_cells;
}
// What launch_fast_cells(a, tile) launches.  Pure host code: it reads nimages, fast_small,
// fast_n48, fast_n64, total_cells and whether fast_ovf is bound.
struct FastLaunchPlan {
    int tile;    // k_fast_cells<tile, small> over the cells [c0, c1); 0: the call launches nothing
    int c0, c1;
    bool small;  // the small-list kernel
    bool ovf;    // k_fast_cells_ovf<64> follows it
};
inline FastLaunchPlan fast_launch_plan(const BatchArgs& a, int tile) {
    int c0, c1;
    fast_cell_range(a, tile, &c0, &c1);
    // a launch of a few images (the latency shape) leaves the GPU mostly idle: the 48- and 64-byte
    // cells go in ONE 64-byte launch instead of two back to back (every 48 cell fits 64)
    const bool merge = a.nimages <= kFastMergeMaxImages && a.fast_small <= 0 && a.fast_n48 > 0 && a.fast_n64 > a.fast_n48;
    if (merge && tile == 64) return {};  // done by the 48 call
    if (merge && tile == 48) {
        tile = 64;
        c1 = a.fast_n64;
    }
    if (c1 <= c0) return {};
    // the small-list 48- and 64-byte kernels for the batch shape (a.fast_small); the two tiles'
    // launches share the queue slot (one after the other on the stream)
    const bool small = (tile == 48 || tile == 64) && a.fast_ovf &&
                       (a.fast_small > 0 || (a.fast_small < 0 && a.nimages > kFastMergeMaxImages));
    // one overflow pass after both tiles, so after the 48-byte launch only when no 64-byte one
    // follows: the 64-byte full-list kernel redoes the cells either queued and resets the queue
    const bool ovf = small && (tile == 64 || a.fast_n64 <= a.fast_n48);
    return {tile, c0, c1, small, ovf};
}
constexpr int kOctSmallThreads = 256;  // default workgroup size of the short-level k_octree launch
constexpr int kOctSmallMinImages = 32;  // launches with fewer images keep the 512-thread shape
// default dynamic LDS of that launch: a 640x480 level 0's node state (~38 KB) plus its depth-5
// count pyramid (10.9 KB) and path tables (2.1 KB); 3 workgroups per CU with the static part
constexpr int kOctSmallLds = 51 * 1024;

// LDS layout of one k_octree launch
struct OctCfg {
    int nq_off;     // byte offset of the per-key labels
    int lds_nodes;  // node capacity in LDS
    int lds_keys;   // labels kept in LDS up to this many keys (global workspace above)
    int lds_bytes;  // dynamic LDS of the launch (the count pyramid takes what the level leaves)
};

struct OctLayout {
    long long keys, nq, nodemem, total;
};

__host__ __device__ inline long long oct_align(long long x) { return (x + 255) & ~255LL; }

// Bytes of node state per node (orb_octree.h oct_nodemem_carve: cntA / cntB 16, nodesA / nodesB
// 16 each, divrank 4, childpos 8, five u16 arrays 10) -- the one figure both the LDS layouts and
// the workspace below size from; orb_octree.h asserts that the carve adds up to it.
constexpr int kOctNodeMemPerNode = 86;
__host__ __device__ constexpr size_t oct_nodemem_bytes(int C) { return (size_t)C * kOctNodeMemPerNode + 64; }

__host__ __device__ inline OctLayout oct_layout(int n_cap, int C) {
    OctLayout L;
    long long o = 0;
    L.keys = o; o = oct_align(o + 4LL * n_cap);
    L.nq = o; o = oct_align(o + 2LL * n_cap);  // used when n exceeds kOctLdsKeys
    L.nodemem = o;
    // used when C exceeds the LDS capacity (k_octree_retry).  Round 3 grew OctNode from 12 to 16
    // bytes while this reserved the old 78 B per node: levels with their node state here (above
    // ~1000 features per level, e.g. 1920x1080 with 8200 features) wrote 8 B per node into the
    // next level's keys, which that level's workgroup was using at the same time (round 6)
    o = oct_align(o + (long long)oct_nodemem_bytes(C));
    L.total = o;
    return L;
}

// Kernel launchers (orb_pyramid.hip, orb_fast.hip, orb_octree.hip, orb_orient.hip, orb_knn2.hip).
// Each returns hipGetLastError() of its launch.
// k_blur / k_blur_resize tile: kBlurTW x kBlurTH outputs of the blur (kBlurTH a multiple of 16:
// 8 row groups of kBlurTH / 8 rows, an even count, in the vertical pass)
#ifndef BLUR_TH
#define BLUR_TH 32
#endif
constexpr int kBlurTW = 128, kBlurTH = BLUR_TH;
static_assert(kBlurTH % 16 == 0, "blur tile height");
constexpr int kBrMaxQuads = 40;  // k_blur_resize: level-l column quads / rows one blur tile owns
constexpr int kBrMaxRows = kBlurTH + 2;
// The blur of level l - 1 and the resize to level l in one launch (every level except the last
// blur, which launch_blur_level does).
// The resize loop's work split (k_blur_resize per tile, k_pyr_tail per level): thread t of nthreads
// makes output quad q of the nq owned ones for the run of consecutive owned rows [row0, row1), so
// that a row's second source row can serve as the next row's first (resize_row_carried).  The
// threads form nthreads / nq slots per quad and the nrows rows are cut into that many runs of
// ceil(nrows / slots) rows; a run is empty (row0 >= row1) beyond the last row, which covers the
// threads beyond the last slot too (slots * len >= nrows).
// div(n, d) = n / d for 0 <= n <= nthreads + nrows, d >= 1 (the kernels pass a reciprocal form).
struct ResizeRun {
    int q, row0, row1;
};
template <class Div>
__host__ __device__ inline ResizeRun resize_run(int t, int nq, int nrows, int nthreads, Div div) {
    const int d = div(nthreads, nq);
    const int slots = d > 1 ? d : 1;
    const int j = div(t, nq);
    const int len = div(nrows + slots - 1, slots);
    const int row0 = j * len;
    return {t - j * nq, row0, row0 + len < nrows ? row0 + len : nrows};
}
// Inside a run: the horizontal sums of row dy's first source row sy0 are the ones the row before
// formed for its second source row prev_sy1 (-1 at a run's first row: nothing carried yet).
__host__ __device__ inline bool resize_row_carried(int prev_sy1, int sy0) { return prev_sy1 == sy0; }
hipError_t launch_blur_resize(const BatchArgs& a, int level, hipStream_t s);
hipError_t launch_blur_level(const BatchArgs& a, int level, hipStream_t s);
hipError_t launch_level_linear(const BatchArgs& a, int level, hipStream_t s);  // scale steps > 2
constexpr int kTailPad = 16;          // k_pyr_tail: left pad of an LDS row (>= 3 reflected columns)
constexpr int kTailLdsMax = 160 * 1024;  // the LDS one workgroup may hold on gfx950
constexpr int kTailMinImages = 128;     // k_pyr_tail only for launches of >= this many images
hipError_t launch_pyr_tail(const BatchArgs& a, hipStream_t s);
// one call per tile (48, 64, kCellMax = 80), each launching what fast_launch_plan says
hipError_t launch_fast_cells(const BatchArgs& a, int tile, hipStream_t s);
hipError_t launch_octree(const BatchArgs& a, hipStream_t s);
hipError_t launch_orient_desc(const BatchArgs& a, hipStream_t s);
hipError_t launch_finalize(const BatchArgs& a, hipStream_t s);
hipError_t launch_knn2_pairs(const MatchArgs& m, int npairs, hipStream_t s);
hipError_t launch_stereo(const StereoArgs& s, int npairs, hipStream_t st);  // orb_stereo.hip
hipError_t launch_undistort_grid(const GridArgs& g, int nimages, hipStream_t st);  // orb_frame.hip
void grid_dist_table(const float* dist, int ndist, double k[14]);
void image_bounds_host(int cols, int rows, const float K[4], const float* dist, int ndist, float bounds[4]);

// Wire formats (orb_io.hip): side-by-side Y8 ingest and the IDL SoA egress.
struct SbsArgs {
    const uint8_t* src;     // nframes frames of h rows x stride bytes, frame_bytes apart
    long long frame_bytes;
    int stride, w, h, nframes;  // w = one eye's width (the frame is 2w wide)
    uint8_t* dst;           // batch input: image 2f = left, 2f + 1 = right, [h][w] each
};
struct SoaArgs {
    const void* kps;        // out_kps [img][out_cap] (28 B)
    const int32_t* out_n;
    int out_cap, nimages, img0;
    int32_t *x, *y, *angle, *level;  // [img][out_cap]
    const int32_t *nq, *idx1, *dist1, *dist2;  // kNN results [pair][out_cap]
    int16_t *idx16, *d1_16, *d2_16;
};
// ORBmatcher::SearchByProjection over device-resident frames (orb_sbp.hip).
struct MapPointIn {  // orbgpu_map_point (72 B)
    float proj_x, proj_y, proj_xr, view_cos, depth;
    int32_t level, flags;
    uint8_t desc[32];
    float proj_yr, view_cos_r;  // right camera of a two-camera frame
    int32_t level_r;
};
constexpr int kMpInView = 1, kMpBad = 2, kMpHasObs = 4, kMpInViewR = 8;
struct SbpCand {  // k_sbp_candidates -> k_sbp_resolve: 4 lowest (distance, window position)
    int32_t idx[4];
    int32_t key[4];   // dist | octave << 16
    int32_t n;        // candidates after the filters; -1: map point skipped
    int32_t flags;    // the map point's flags (kMpHasObs decides whether its keypoint is taken)
    int32_t idxR[4];  // the same for the right-camera window (two-camera frames)
    int32_t keyR[4];
    int32_t nR;       // -1: no right-camera search
};
struct SbpArgs {
    const MapPointIn* mps;    // all frames' map points, frame f = [mp_off[f], mp_off[f + 1])
    const int32_t* mp_off;
    SbpCand* cand;            // [mp]
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    const float* uright;      // [frame][out_cap] mvuRight or nullptr (pinhole frames)
    const uint8_t* kp_block;  // [frame][2 * out_cap] pre-call occupant with observations, or nullptr
    const int32_t* l2r;       // [frame][out_cap] mvLeftToRightMatch (two-camera frames) or nullptr
    const int32_t* r2l;       // [frame][out_cap] mvRightToLeftMatch or nullptr
    int two_cam;              // Nleft != -1: frame f = images 2f (left) and 2f + 1 (right)
    int image_step, img0;     // frame f = batch image (img0 + f) * image_step; img0 = first frame
    float bounds[4], grid_inv[2];
    float scale[kMaxLevels];
    int nlevels;
    float th, nnratio, th_far;
    int far_points, factor;
    int32_t* match;           // [frame][2 * out_cap]: left keypoints, then right ones
    int32_t* nmatches;        // [frame]
};
size_t sbp_resolve_lds_bytes(int out_cap, int two_cam);
hipError_t launch_sbp(const SbpArgs& a, int nframes, int max_mps, hipStream_t st);

// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (orb_track.hip).
struct LastPointIn {  // orbgpu_last_point (56 B)
    float pos[3], angle;
    int32_t octave, flags;
    uint8_t desc[32];
};
constexpr int kLpValid = 1;  // kMpHasObs (4) is shared with the local-map search
constexpr int kTrackForward = 1, kTrackBackward = 2;
struct TrackFrame {  // per frame, from orbgpu_track_pose (host: the direction, :1727-1734)
    float Rcw[9], tcw[3];
    int32_t dir;  // kTrackForward / kTrackBackward / 0
    int32_t pad[3];
};
struct TrackCand {  // k_track_candidates -> k_track_resolve
    int32_t idx[4];   // 4 lowest (distance, window position)
    int32_t dist[4];
    int32_t n;        // candidates after the filters; -1: point skipped
    int32_t flags;
    int32_t octave;
    float u, v, invz, angle;  // the projection (:1742-1751) and LastFrame.mvKeysUn[i].angle
    int32_t pad;
};
constexpr int kRotBins = 30;  // HISTO_LENGTH
struct TrackArgs {
    const LastPointIn* pts;   // all frames' points, frame f = [pt_off[f], pt_off[f + 1])
    const int32_t* pt_off;
    const TrackFrame* frames; // [frame]
    TrackCand* cand;          // [point]
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    const float* uright;      // [frame][out_cap] mvuRight or nullptr
    const uint8_t* kp_block;  // [frame][out_cap] pre-call occupant with observations, or nullptr
    int image_step;           // frame f = batch image f * image_step
    float bounds[4], grid_inv[2];
    float scale[kMaxLevels];
    int nlevels;
    float K[4], mbf, th;
    int check_orientation;
    int32_t* match;           // [frame][out_cap]
    int32_t* nmatches;        // [frame]
    int32_t* rot_hist;        // [frame][kRotBins] bin sizes before the three-maxima rule
};
size_t track_resolve_lds_bytes(int out_cap);
hipError_t launch_track(const TrackArgs& a, int nframes, int max_pts, hipStream_t st);
// The two-camera branch (Nleft != -1, :1840-1914): frame f = images 2f (left) and 2f + 1 (right),
// image_step = 2, uright = nullptr; kp_block / match are [frame][2 * out_cap], the left keypoints,
// then (from Nleft on) the right ones; cand is [2 * point]: frame f's left records at
// 2 * pt_off[f], its right records after them.
struct TrackRig {  // orbgpu_track_rig (80 B)
    float cam[8];  // the left camera's KannalaBrandt8 parameters: both windows project with it
    float Rrl[9], trl[3];
};
struct TrackStereoArgs : TrackArgs {
    TrackRig rig;
    uint32_t* side_mask;  // [frame][2 * out_cap] bins of each keypoint's events (match's layout)
    int32_t* side_hist;   // [frame][2][kRotBins + 1] each side's bin sizes, then its event count
};
hipError_t launch_track_stereo(const TrackStereoArgs& a, int npairs, int max_pts, hipStream_t st);

// ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (orb_init.hip).
constexpr int kInitTop = 4;
struct InitCand {  // k_init_candidates -> k_init_replay, one per searched F1 keypoint in index order
    int32_t idx[kInitTop];   // the lowest (distance, window position) candidates, -1 when fewer
    int32_t dist[kInitTop];
    int32_t n;               // keypoints of the window that passed GetFeaturesInArea
    int32_t i1;              // the F1 keypoint
    int32_t pad[2];
};
struct InitArgs {
    const int32_t* pairs;     // [pair][2]: the batch images F1, F2
    const float* prev;        // [pair][out_cap][2] vbPrevMatched, or nullptr: F1's mvKeysUn.pt
    InitCand* cand;           // [pair][out_cap]
    int32_t* nsearch;         // [pair] searched F1 keypoints (zeroed before the launch)
    // F2's octave-0 keypoints in grid order (k_init_compact): l0_pre[j] = how many of them precede
    // entry j of cell_idx ([pair][out_cap + 1]); their index, mvKeysUn.pt and descriptor, packed
    int32_t* l0_pre;
    int32_t* l0_idx;          // [pair][out_cap]
    float* l0_xy;             // [pair][out_cap][2]
    uint8_t* l0_desc;         // [pair][out_cap][32]
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    float bounds[4], grid_inv[2];
    float window, nnratio;
    int check_orientation;
    int32_t* match12;         // [pair][out_cap]
    float* prev_out;          // [pair][out_cap][2] vbPrevMatched after the call
    int32_t* nmatches;        // [pair]
    int32_t* rot_hist;        // [pair][kRotBins] bin sizes before the three-maxima rule
};
size_t init_replay_lds_bytes(int out_cap);
hipError_t launch_init_search(const InitArgs& a, int npairs, hipStream_t st);

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (orb_bow.hip).
constexpr int kBowMaxPoints = 8192;  // keypoints per side k_bow_group sorts in LDS (ORBGPU_BOW_MAX_POINTS)
struct BowPoint {  // orbgpu_bow_point
    uint32_t desc[8];
    float angle;
    int32_t node;
    int32_t flags;
};
struct BowArgs {
    const int32_t* frames;    // [pair] the batch image that is F
    const BowPoint* kf_pts;   // all pairs' keyframe points, pair p = [kf_off[p], kf_off[p + 1])
    const int32_t* kf_off;    // [pair + 1], kf_off[0] == 0
    const int32_t* f_nodes;   // [pair][out_cap] the node of each keypoint of F, < 0: none
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const uint8_t* desc;      // out_desc
    float nnratio;
    int check_orientation;
    // k_bow_group -> k_bow_match: each side's keypoints by (node, index) and its node segments
    int32_t* kf_order;        // [kf point]
    int32_t* kf_seg_node;     // [kf point]
    int32_t* kf_seg_start;    // pair p at kf_off[p] + p, one entry more than its points
    int32_t* f_order;         // [pair][out_cap]
    int32_t* f_seg_node;      // [pair][out_cap]
    int32_t* f_seg_start;     // [pair][out_cap + 1]
    uint8_t* f_desc;          // [pair][out_cap][32] F's descriptors in f_order's order
    int32_t* nseg;            // [pair][2] segments of the keyframe, of F
    int32_t* match;           // [pair][out_cap]
    uint8_t* match_bin;       // [pair][out_cap] the bin of the event that wrote match
    int32_t* nmatches;        // [pair]
    int32_t* rot_hist;        // [pair][kRotBins] bin sizes before the three-maxima rule
};
// max_side: the largest keypoint count of a side (<= kBowMaxPoints)
hipError_t launch_bow_search(const BowArgs& a, int npairs, int max_side, hipStream_t st);

// ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (orb_tri.hip),
// pinhole keyframes.  Keyframe 1 is a batch image, keyframe 2 the host's points; the grouping fields
// carry BowArgs' names (orb_bow_group.h reads them from either struct).
struct TriPoint {  // orbgpu_triang_point (56 B)
    uint32_t desc[8];
    float x, y, angle;
    int32_t octave, node, flags;
};
constexpr int kTriHasPoint = 1, kTriStereo = 2;
struct TriPair {  // orbgpu_triang_pair (44 B)
    float F12[9], ep[2];
};
struct TriArgs {
    const int32_t* frames;    // [pair] the batch image that is keyframe 1
    const TriPoint* kf_pts;   // all pairs' keyframe 2 points, pair p = [kf_off[p], kf_off[p + 1])
    const int32_t* kf_off;    // [pair + 1], kf_off[0] == 0
    const TriPair* pairs;     // [pair]
    const int32_t* f_nodes;   // [pair][out_cap] the node of each keypoint of keyframe 1, < 0: none
    const uint8_t* f_flags;   // [pair][out_cap] kTriHasPoint / kTriStereo of keyframe 1's keypoints, or nullptr
    const double* epi_th;     // [kMaxLevels] 3.84 * (double)mvLevelSigma2[level] (Pinhole.cpp:123)
    const float* disc_th;     // [kMaxLevels] 100 * mvScaleFactors[level] (:1037)
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const uint8_t* desc;      // out_desc
    const float* xy_un;       // [img][out_cap][2] mvKeysUn positions (orbgpu_undistort_grid_batch)
    int nlevels;
    int only_stereo, coarse, check_orientation;
    // k_tri_group -> k_tri_match: each side's keypoints by (node, index) and its node segments
    int32_t* kf_order;        // [kf point]
    int32_t* kf_seg_node;     // [kf point]
    int32_t* kf_seg_start;    // pair p at kf_off[p] + p, one entry more than its points
    int32_t* f_order;         // [pair][out_cap]
    int32_t* f_seg_node;      // [pair][out_cap]
    int32_t* f_seg_start;     // [pair][out_cap + 1]
    uint8_t* f_desc;          // [pair][out_cap][32] keyframe 1's descriptors in f_order's order
    uint4* kf_desc;           // [kf point][2] keyframe 2's descriptors in kf_order's order
    float4* kf_meta;          // [kf point] {x, y, angle, bits of octave << 8 | flags} in kf_order's order
    int32_t* nseg;            // [pair][2] segments of keyframe 2, of keyframe 1
    int32_t* match;           // [pair][out_cap] vMatches12
    uint8_t* match_bin;       // [pair][out_cap] the bin of the event that wrote match
    int32_t* nmatches;        // [pair]
    int32_t* rot_hist;        // [pair][kRotBins] bin sizes before the three-maxima rule
};
hipError_t launch_tri_search(const TriArgs& a, int npairs, int max_side, hipStream_t st);

// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (orb_bowkf.hip),
// pinhole keyframes.  Keyframe 1 is a batch image, keyframe 2 the host's points (BowPoint rows); the
// grouping fields carry BowArgs' names (orb_bow_group.h reads them from either struct).
enum BowKfCode : uint8_t {  // ORBGPU_BOWKF_*: what a keypoint of keyframe 1 ended with
    kBowKfNoNode = 1, kBowKfNodeNotCommon, kBowKfNoMapPoint, kBowKfNoCandidate, kBowKfNotBelowThLow, kBowKfRatioFailed,
    kBowKfMatched, kBowKfRotationRejected
};
struct BowKfArgs {
    const int32_t* frames;    // [pair] the batch image that is keyframe 1
    const BowPoint* kf_pts;   // all pairs' keyframe 2 points, pair p = [kf_off[p], kf_off[p + 1])
    const int32_t* kf_off;    // [pair + 1], kf_off[0] == 0
    const int32_t* f_nodes;   // [pair][out_cap] the node of each keypoint of keyframe 1, < 0: none
    const uint8_t* f_flags;   // [pair][out_cap] bit 0: the keypoint of keyframe 1 has a map point; nullptr: all do
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const uint8_t* desc;      // out_desc
    float nnratio;
    int check_orientation;
    // k_bowkf_group -> k_bowkf_match: each side's keypoints by (node, index) and its node segments
    int32_t* kf_order;        // [kf point]
    int32_t* kf_seg_node;     // [kf point]
    int32_t* kf_seg_start;    // pair p at kf_off[p] + p, one entry more than its points
    int32_t* f_order;         // [pair][out_cap]
    int32_t* f_seg_node;      // [pair][out_cap]
    int32_t* f_seg_start;     // [pair][out_cap + 1]
    uint8_t* f_desc;          // [pair][out_cap][32] keyframe 1's descriptors in f_order's order
    uint4* kf_desc;           // [kf point][2] keyframe 2's descriptors in kf_order's order
    float2* kf_meta;          // [kf point] {angle, bits of flags} in kf_order's order
    int32_t* nseg;            // [pair][2] segments of keyframe 2, of keyframe 1
    int32_t* match;           // [pair][out_cap] match12
    short2* best;             // [pair][out_cap] {bestDist1, bestDist2}
    uint8_t* match_bin;       // [pair][out_cap] the bin of the event that wrote match
    uint8_t* code;            // [pair][out_cap] BowKfCode
    int32_t* nmatches;        // [pair]
    int32_t* rot_hist;        // [pair][kRotBins] bin sizes before the three-maxima rule
};
hipError_t launch_bowkf_search(const BowKfArgs& a, int npairs, int max_side, hipStream_t st);

// ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist)
// (orb_reloc.hip).
struct RelocPoint {  // orbgpu_reloc_point (60 B)
    float pos[3], angle, min_distance, max_distance;
    int32_t flags;
    uint8_t desc[32];
};
constexpr int kRpValid = 1;
struct RelocPose {  // orbgpu_reloc_pose (60 B)
    float Rcw[9], tcw[3], Ow[3];
};
struct RelocCand {  // k_reloc_candidates -> k_reloc_resolve
    int32_t idx[4];   // 4 lowest (distance, window position) among those within orb_dist
    int32_t dist[4];
    int32_t n;        // candidates within orb_dist after the filters; -1: point skipped
    int32_t level;    // nPredictedLevel
    float u, v;       // the projection (:1951)
};
struct RelocArgs {
    const int32_t* frames;    // [pair] the batch image that is CurrentFrame
    const RelocPoint* pts;    // all pairs' keyframe points, pair p = [kf_off[p], kf_off[p + 1])
    const int32_t* kf_off;    // [pair + 1], kf_off[0] == 0
    const RelocPose* poses;   // [pair]
    RelocCand* cand;          // [point]
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    const uint8_t* kp_block;  // [pair][out_cap] mvpMapPoints[k] set before the call, or nullptr
    float bounds[4], grid_inv[2];
    float scale[kMaxLevels];
    float level_step[kMaxLevels];  // predict_scale_table: level = #{n < nlevels - 1 : ratio > level_step[n]}
    int nlevels;
    float K[4], th;
    int orb_dist, check_orientation;
    int32_t* match;           // [pair][out_cap]
    int32_t* nmatches;        // [pair]
    int32_t* rot_hist;        // [pair][kRotBins] bin sizes before the three-maxima rule
};
size_t reloc_resolve_lds_bytes(int out_cap);
hipError_t launch_reloc(const RelocArgs& a, int npairs, int max_pts, hipStream_t st);

// ORBmatcher::Fuse(pKF, vpMapPoints, th) and its Sim3 overload on pinhole keyframes (orb_fuse.hip).
struct FusePoint {  // orbgpu_fuse_point (68 B)
    float pos[3], normal[3], min_distance, max_distance;
    int32_t flags;
    uint8_t desc[32];
};
constexpr int kFpValid = 1;
constexpr int kFuseMaxPoints = 65536;  // ORBGPU_FUSE_MAX_POINTS
enum FuseCode : uint8_t {  // ORBGPU_FUSE_*
    kFuseSkipped = 1, kFuseNegDepth, kFuseNotInImage, kFuseDistance, kFuseNormal, kFuseEmptyWindow, kFuseAboveThLow,
    kFuseFused
};
struct FuseArgs {
    const int32_t* frames;    // [pair] the batch image that is pKF
    const int32_t* lists;     // [pair] the list the pair fuses
    const int32_t* out_off;   // [pair + 1] the pair's rows of best_idx / best_dist / code
    const int32_t* list_off;  // [list + 1], list_off[0] == 0
    const FusePoint* pts;     // all lists' points
    const RelocPose* poses;   // [pair]
    const uint8_t* skip;      // [pair][skip_stride] non-zero: the point is skipped for this pair; or nullptr
    int skip_stride;
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    const float* uright;      // mvuRight [stereo pair][out_cap] (pair = image / 2), or nullptr
    float bounds[4], grid_inv[2];
    float scale[kMaxLevels];
    float inv_sigma2[kMaxLevels];  // mvInvLevelSigma2
    float level_step[kMaxLevels];  // predict_scale_table, as in RelocArgs
    int nlevels;
    float K[4], th, bf;
    int sim3;                 // the Sim3 overload: no chi-square gate
    int32_t* best_idx;        // [point row]
    int32_t* best_dist;       // [point row]
    uint8_t* code;            // [point row]
    uint32_t* first;          // [pair][out_cap] lowest point that fused onto the keypoint; 0xFFFFFFFF (-1): none
    int32_t* nfused;          // [pair]
};
hipError_t launch_fuse(const FuseArgs& a, int npairs, int max_pts, hipStream_t st);

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) and the vpPointsKFs
// overload on pinhole keyframes (orb_sim3.hip).  The points are FusePoint rows, the poses RelocPose rows,
// the candidate records RelocCand (n: within the limit, in the band and free before the call; -1: the
// point ended before the loop).
enum Sim3Code : uint8_t {  // ORBGPU_SIM3_*: 1..6 are the FuseCode values
    kSim3Pending = 0,      // between the two kernels: the replay decides
    kSim3NotMatched = 7, kSim3Matched = 8
};
constexpr int kSim3ProjectDiv = 0, kSim3ProjectInvz = 1;  // ORBGPU_SIM3_PROJECT_*
struct Sim3Args {
    const int32_t* frames;    // [pair] the batch image that is pKF
    const int32_t* lists;     // [pair] the list the pair searches
    const int32_t* out_off;   // [pair + 1] the pair's rows of cand / order / best_idx / best_dist / code
    const int32_t* list_off;  // [list + 1], list_off[0] == 0
    const FusePoint* pts;     // all lists' points
    const RelocPose* poses;   // [pair]
    const uint8_t* skip;      // [pair][skip_stride] non-zero: spAlreadyFound holds the point; or nullptr
    int skip_stride;
    const uint8_t* kp_block;  // [pair][out_cap] vpMatched[k] set before the call, or nullptr
    const void* kps;          // out_kps
    const int32_t* out_n;
    int out_cap;
    const float* xy_un;       // grid buffers (orbgpu_undistort_grid_batch)
    const int32_t* cell_start;
    const int32_t* cell_idx;
    const uint8_t* desc;      // out_desc
    float bounds[4], grid_inv[2];
    float scale[kMaxLevels];
    float level_step[kMaxLevels];  // predict_scale_table, as in RelocArgs
    int nlevels;
    float K[4], th;
    float limit;              // TH_LOW * ratioHamming, the float product (:524)
    int projection;           // kSim3ProjectDiv / kSim3ProjectInvz
    RelocCand* cand;          // [point row]
    int32_t* order;           // [point row] the pair's pending points, ascending (k_sim3_resolve's own)
    int32_t* best_idx;        // [point row]
    int32_t* best_dist;       // [point row]
    uint8_t* code;            // [point row]
    int32_t* match;           // [pair][out_cap]
    int32_t* nmatches;        // [pair]
    int32_t* stats;           // [pair][kSim3Stats]: pending points, passes, stale lanes, fresh walks
};
constexpr int kSim3Stats = 4;
size_t sim3_resolve_lds_bytes(int out_cap);
hipError_t launch_sim3(const Sim3Args& a, int npairs, int max_pts, hipStream_t st);

hipError_t launch_sbs_split(const SbsArgs& a, hipStream_t st);
hipError_t launch_pack_soa(const SoaArgs& a, int npairs, hipStream_t st);
// orbgpu_export_batch (orb_io.hip k_pack_export): the produced rows of a batch, packed
struct ExportArgs {
    const void* kps;          // out_kps [img][out_cap] (28 B)
    const uint8_t* desc;      // out_desc [img][out_cap][32]
    const int32_t* out_n;     // [img] (>= 0: the host checked)
    const int32_t* out_mono;  // [img]
    const int32_t* nq;        // [pair]
    const int32_t *idx1, *dist1, *idx2, *dist2;  // [pair][out_cap]
    int out_cap, nimages, npairs;
    void* dst;                // device buffer, 4-byte aligned
};
hipError_t launch_pack_export(const ExportArgs& a, hipStream_t st);
hipError_t launch_knn2_plain(const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* i1,
                             int32_t* d1, int32_t* i2, int32_t* d2, hipStream_t s);

}  // namespace orbgpu
