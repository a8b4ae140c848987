// ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false)
// (cpp/src/ORBmatcher.cc:1155-1345) and its Sim3 overload (:1347-1462), with
// KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:706-755) and MapPoint::PredictScale
// (MapPoint.cc:516-531): the map-point fusion LocalMapping::SearchInNeighbors and
// LoopClosing::SearchAndFuse run, on pinhole keyframes (NLeft == -1: mvKeysUn, mvuRight), over pairs of
// a list of map points the host gives and a batch image whose keypoints, descriptors, grid and
// mvuRight already live in HBM.  Several pairs may name one list (one upload of the current
// keyframe's points for all its neighbours; a per-pair skip row carries IsInKeyFrame) or one frame.
//
// Per point: transform with the pose, the depth test, project (Pinhole.cpp:40-41), the half-open
// image test, the invariance range, the viewing angle against the point's normal, the level from
// the distance (the host's step table, as in orb_reloc.hip: no logarithm runs here), a window of
// th * mvScaleFactors[level] without a level filter, then per candidate the octave band
// [level - 1, level], the chi-square gate on the reprojection error (not in the Sim3 overload) and
// the first lowest Hamming distance; fused when it is <= TH_LOW.  Each point gets the decision code
// of the reference's count_* debug counters (:1183).
//
// Nothing is taken: the points do not see each other, so one kernel runs them in parallel.  What the
// host needs to replay :1321-1337 / :1446-1456 -- which point reached a keypoint first -- is an
// integer minimum per keypoint, and nFused one integer sum per wave; both commute, so the result
// does not depend on the order the waves run in.
//
// A window holds a few entries in 2 to 5 grid columns; at one thread per point the batch is under a
// wave per SIMD and waits on a chain of dependent loads, so kFuseLanes lanes share a point and take
// the window's columns strided and reduce by DPP moves (walk_area_group, orb_window.h).  No LDS, no
// barriers.
//
// Deviation from the reference: a dist3D or max_distance / dist3D that is not finite gets the
// distance code (the reference would go on into PredictScale with it).
#include <hip/hip_runtime.h>

#include "orb_kernels.h"
#include "orb_window.h"

#ifndef ORBGPU_FUSE_G
#define ORBGPU_FUSE_G 4  // lanes per point: 1, 4 and 8 measured
#endif

namespace orbgpu {
namespace {

constexpr int kFuseLanes = ORBGPU_FUSE_G;
constexpr int kThLow = 50;  // ORBmatcher::TH_LOW
static_assert(kFuseLanes >= 1 && kFuseLanes <= 16 && (kFuseLanes & (kFuseLanes - 1)) == 0, "a power of two within a DPP row");

// One point by the G lanes that share it; every lane of the group returns the same code, *bd, *bi.
template <int G>
__device__ inline int fuse_point(const FuseArgs& a, int p, const FusePoint& pt, bool skipped, int sub, int* bd, int* bi) {
    *bd = 256, *bi = -1;
    if (!(pt.flags & kFpValid) || skipped) return kFuseSkipped;  // :1188-1203 / :1372
    const RelocPose T = a.poses[p];
    float xc, yc, zc, u, v;
    project_pinhole(T.Rcw, T.tcw, a.K, pt.pos, &xc, &yc, &zc, &u, &v);
    if (zc < 0.0f) return kFuseNegDepth;  // :1209
    const float invz = 1 / zc;
    // KeyFrame::IsInImage: half-open; a NaN or infinite projection fails it
    if (!(u >= a.bounds[0] && u < a.bounds[1] && v >= a.bounds[2] && v < a.bounds[3])) return kFuseNotInImage;
    const float ur = u - a.bf * invz;  // :1226
    const float px = pt.pos[0] - T.Ow[0], py = pt.pos[1] - T.Ow[1], pz = pt.pos[2] - T.Ow[2];
    const float dist3D = sqrtf((px * px + py * py) + pz * pz);
    if (!isfinite(dist3D)) return kFuseDistance;
    if (dist3D < 0.8f * pt.min_distance || dist3D > 1.2f * pt.max_distance) return kFuseDistance;  // :1234
    const float ratio = pt.max_distance / dist3D;  // MapPoint.cc:521
    if (!isfinite(ratio)) return kFuseDistance;
    const float dot = (px * pt.normal[0] + py * pt.normal[1]) + pz * pt.normal[2];
    if ((double)dot < 0.5 * (double)dist3D) return kFuseNormal;  // :1242: 0.5 is a double
    const int nsteps = min(max(a.nlevels - 1, 0), kMaxLevels - 1);
    int level = 0;
#pragma unroll
    for (int n = 0; n < kMaxLevels - 1; ++n) level += (n < nsteps && ratio > a.level_step[n]) ? 1 : 0;
    const float radius = a.th * a.scale[level];  // :1251
    const int img = a.frames[p];
    const FrameView F = frame_view_of(a, img, a.uright && !a.sim3 ? a.uright + (long long)(img >> 1) * a.out_cap : nullptr);
    uint32_t q[8];
    load_desc(pt.desc, q);
    bool any;
    *bd = walk_area_group<G>(
        a, F, u, v, radius, sub, q,
        [&](int k, int oct) {
            if (oct < level - 1 || oct > level) return false;  // :1276
            if (a.sim3) return true;
            const float2 kp = *reinterpret_cast<const float2*>(F.xy + 2LL * k);
            const float inv = a.inv_sigma2[min(max(oct, 0), kMaxLevels - 1)];
            const float ex = u - kp.x, ey = v - kp.y;
            const float kr = F.uright ? F.uright[k] : -1.0f;
            if (kr >= 0) {  // :1279-1292; the product is a float, the literal a double; NaN passes
                const float er = ur - kr;
                const float e2 = (ex * ex + ey * ey) + er * er;
                return !((double)(e2 * inv) > 7.8);
            }
            const float e2 = ex * ex + ey * ey;  // :1293-1303
            return !((double)(e2 * inv) > 5.99);
        },
        bi, &any);
    if (!any) return kFuseEmptyWindow;  // :1255
    if (*bd <= kThLow) return kFuseFused;  // :1319
    *bi = -1;
    return kFuseAboveThLow;
}

template <int G>
__global__ __launch_bounds__(256) void k_fuse_match(FuseArgs a) {
    const int p = blockIdx.y;
    const int l = a.lists[p];
    const int m0 = a.list_off[l], np = a.list_off[l + 1] - m0;
    const int i = (blockIdx.x * 256 + threadIdx.x) / G, sub = threadIdx.x % G;
    const bool live = i < np;  // the same for every lane of a group
    int code = 0, bd = 256, bi = -1;
    if (live) {
        const bool skipped = a.skip && a.skip[(long long)p * a.skip_stride + i];
        code = fuse_point<G>(a, p, a.pts[m0 + i], skipped, sub, &bd, &bi);
    }
    const bool fused = live && sub == 0 && code == kFuseFused;
    if (live && sub == 0) {
        const long long row = (long long)a.out_off[p] + i;
        a.code[row] = (uint8_t)code;
        a.best_dist[row] = bd;
        a.best_idx[row] = bi;
        if (fused) atomicMin(&a.first[(long long)p * a.out_cap + bi], (uint32_t)i);
    }
    const uint64_t fm = __ballot(fused);  // no lane has left: the whole wave is here
    if (fm && (threadIdx.x & 63) == 0) atomicAdd(&a.nfused[p], (int)__popcll(fm));
}

}  // namespace

hipError_t launch_fuse(const FuseArgs& a, int npairs, int max_pts, hipStream_t st) {
    if (npairs <= 0 || max_pts <= 0) return hipSuccess;
    const int blocks = (int)(((long long)max_pts * kFuseLanes + 255) / 256);
    hipLaunchKernelGGL(k_fuse_match<kFuseLanes>, dim3(blocks, npairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
