// ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, const vector<MapPoint*>& vpPoints,
// vector<MapPoint*>& vpMatched, int th, float ratioHamming) (cpp/src/ORBmatcher.cc:428-533) and the overload
// that also carries vpPointsKFs / vpMatchedKF (:535-647), with KeyFrame::GetFeaturesInArea / IsInImage
// (KeyFrame.cc:706-755) and MapPoint::PredictScale (MapPoint.cc:516-531): the searches
// LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:755, :777) and FindMatchesByProjection (:964) run
// while a loop or merge candidate is found and confirmed, on pinhole keyframes (NLeft == -1: mvKeysUn), over
// pairs of a list of map points the host gives and a batch image whose keypoints, descriptors and grid
// already live in HBM.  Several pairs may name one list or one frame; each pair is one call of the reference
// with its own pose, skip row (spAlreadyFound) and occupancy row (vpMatched).
//
// Per point, in index order: Fuse's gates (orb_fuse.hip) -- the depth test, the projection, the half-open
// image test, the invariance range, the viewing angle in double, the level from the host's step table, a
// window of th * mvScaleFactors[level] without a level filter -- then, unlike Fuse, a loop that passes over
// every keypoint that holds a point (:505, :618), before the call or taken earlier in it, keeps octaves
// [level - 1, level] and takes the first lowest Hamming distance; matched when (float)bestDist <= TH_LOW *
// ratioHamming, and the match takes its keypoint (:526, :639).  There is no rotation histogram and no
// chi-square gate.  The two overloads differ in one thing, the projection: Pinhole::project (fx * xc / zc +
// cx) in the first, invz = 1 / zc; x = xc * invz; fx * x + cx in the second.
//
// The loop is sequential, so, as in orb_reloc.hip:
//   k_sim3_candidates  kSim3Lanes lanes per (pair, point): the gates give the decision code of every point
//                      that ends there; for the rest the group walks the window against the pre-call
//                      occupancy (walk_area_group_top4, orb_window.h) and keeps the 4 lowest (distance, window
//                      position) candidates that are free, in the band and within the limit, and how many
//                      there were.  A point with none is NOT_MATCHED at once; the others are left pending.
//   k_sim3_resolve     one wave per pair.  Lists here are ten times a keyframe's and most points end at a
//                      gate, so the wave first packs the pending points' indices, ascending, and replays
//                      only those, 64 at a time, with the live occupancy in LDS: k_reloc_resolve's scheme
//                      (the first kept candidate not taken so far; a fresh walk by the whole wave when all
//                      kept ones are gone and more had passed; a lane is stale when an earlier pending lane
//                      of the group touched what it looked at; the undisturbed prefix commits).
//
// Deviation from the reference, as in orb_fuse.hip: a dist or max_distance / dist that is not finite gets the
// distance code.
#include <hip/hip_runtime.h>

#include "orb_kernels.h"
#include "orb_window.h"

#ifndef ORBGPU_SIM3_G
#define ORBGPU_SIM3_G 4  // lanes per point in k_sim3_candidates (k_fuse_match's measured choice)
#endif

namespace orbgpu {
namespace {

constexpr int kSim3Lanes = ORBGPU_SIM3_G;
constexpr int kTop = 4;    // candidates kept per point (RelocCand)
constexpr int kScan = 16;  // codes one lane reads per packing step
static_assert(kSim3Lanes >= 1 && kSim3Lanes <= 16 && (kSim3Lanes & (kSim3Lanes - 1)) == 0, "a power of two");

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Pair p: its list's first point, its first output row and its length, clamped to what the launch sized.
__device__ inline void sim3_range(const Sim3Args& a, int p, int* m0, int* row0, int* np) {
    const int l = a.lists[p];
    *m0 = max(a.list_off[l], 0);
    *row0 = max(a.out_off[p], 0);
    *np = max(min(a.list_off[l + 1] - *m0, a.out_off[p + 1] - *row0), 0);
}

// Rules 1 to 7 for one point by the G lanes that share it, then the window walk.  Every lane of the group
// returns the same code and the same record.
template <int G>
__device__ inline int sim3_point(const Sim3Args& a, int p, const FusePoint& pt, bool skipped, int sub, RelocCand* c) {
    if (!(pt.flags & kFpValid) || skipped) return kFuseSkipped;  // :452 / :560
    const RelocPose T = a.poses[p];
    float xc, yc, zc, u, v;
    if (a.projection == kSim3ProjectInvz)
        project_pinhole_invz(T.Rcw, T.tcw, a.K, pt.pos, &xc, &yc, &zc, &u, &v);  // :574-579
    else
        project_pinhole(T.Rcw, T.tcw, a.K, pt.pos, &xc, &yc, &zc, &u, &v);  // :466
    if (zc < 0.0f) return kFuseNegDepth;  // :462 / :570
    // KeyFrame::IsInImage: half-open; a NaN or infinite projection fails it
    if (!(u >= a.bounds[0] && u < a.bounds[1] && v >= a.bounds[2] && v < a.bounds[3])) return kFuseNotInImage;
    const float px = pt.pos[0] - T.Ow[0], py = pt.pos[1] - T.Ow[1], pz = pt.pos[2] - T.Ow[2];
    const float dist3D = sqrtf((px * px + py * py) + pz * pz);
    if (!isfinite(dist3D)) return kFuseDistance;
    if (dist3D < 0.8f * pt.min_distance || dist3D > 1.2f * pt.max_distance) return kFuseDistance;  // :478 / :591
    const float ratio = pt.max_distance / dist3D;  // MapPoint.cc:521
    if (!isfinite(ratio)) return kFuseDistance;
    const float dot = (px * pt.normal[0] + py * pt.normal[1]) + pz * pt.normal[2];
    if ((double)dot < 0.5 * (double)dist3D) return kFuseNormal;  // :484 / :597: 0.5 is a double
    const int nsteps = clampi(a.nlevels - 1, 0, kMaxLevels - 1);
    int level = 0;
#pragma unroll
    for (int n = 0; n < kMaxLevels - 1; ++n) level += (n < nsteps && ratio > a.level_step[n]) ? 1 : 0;
    const float radius = a.th * a.scale[level];  // :490 / :603
    const FrameView F = frame_view_of(a, a.frames[p], nullptr);
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)p * a.out_cap : nullptr;
    uint32_t q[8];
    load_desc(pt.desc, q);
    bool any;
    int n;
    walk_area_group_top4<G>(
        a, F, u, v, radius, sub, q,
        [&](int k, int oct) { return !(blk && blk[k]) && oct >= level - 1 && oct <= level; },  // :505, :510
        [&](int d) { return (float)d <= a.limit; },                                            // :524
        c->idx, c->dist, &n, &any);
    if (!any) return kFuseEmptyWindow;  // :494 / :607, before the occupancy is looked at
    if (n == 0) return kSim3NotMatched;  // nothing the live occupancy could still offer
    c->n = n, c->level = level, c->u = u, c->v = v;
    return kSim3Pending;
}

template <int G>
__global__ __launch_bounds__(256) void k_sim3_candidates(Sim3Args a) {
    const int p = blockIdx.y;
    int m0, row0, np;
    sim3_range(a, p, &m0, &row0, &np);
    const int i = (blockIdx.x * 256 + threadIdx.x) / G, sub = threadIdx.x % G;
    if (i >= np) return;  // the same for every lane of a group
    const bool skipped = a.skip && a.skip[(long long)p * a.skip_stride + i];
    RelocCand c;
    const int code = sim3_point<G>(a, p, a.pts[m0 + i], skipped, sub, &c);
    if (sub != 0) return;
    const long long row = (long long)row0 + i;
    a.code[row] = (uint8_t)code;
    a.best_idx[row] = -1;
    a.best_dist[row] = 256;
    if (code == kSim3Pending) a.cand[row] = c;
}

// Dynamic LDS of k_sim3_resolve for n keypoints per frame: the occupancy bitmap and the owner table.
__host__ __device__ inline int sim3_lds_words(int n) { return (n + 31) / 32 + n; }

__global__ __launch_bounds__(64) void k_sim3_resolve(Sim3Args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int ncap = a.out_cap;
    uint32_t* taken = lds;                       // vpMatched[k] set
    uint32_t* owner = taken + (ncap + 31) / 32;  // lowest pending lane assigning it
    const int p = blockIdx.x, lane = threadIdx.x;
    const int img = a.frames[p];
    const int nk = clampi(a.out_n[img], 0, ncap);
    int m0, row0, npts;
    sim3_range(a, p, &m0, &row0, &npts);
    const RelocCand* cand = a.cand + row0;
    const FusePoint* pts = a.pts + m0;
    int32_t* order = a.order + row0;
    uint8_t* code = a.code + row0;
    int32_t* match = a.match + (long long)p * ncap;
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)p * ncap : nullptr;
    const FrameView F = frame_view_of(a, img, nullptr);
    for (int w = lane; w < (nk + 31) / 32; w += 64) {
        uint32_t bits = 0;
        if (blk)
            for (int b = 0; b < 32 && w * 32 + b < nk; ++b) bits |= (blk[w * 32 + b] ? 1u : 0u) << b;
        taken[w] = bits;
    }
    for (int k = lane; k < nk; k += 64) {
        owner[k] = 64;
        match[k] = -1;
    }
    // the pending points' indices, ascending: a lane reads kScan codes, the wave's prefix sum places them
    int npend = 0;
    for (int g0 = 0; g0 < npts; g0 += 64 * kScan) {
        const int b = g0 + lane * kScan;
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < kScan; ++t)
            if (b + t < npts && code[b + t] == kSim3Pending) mask |= 1u << t;
        const int cnt = __popc(mask);
        int incl = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        int w = npend + incl - cnt;  // at most b: a place in the pair's own rows
        for (uint32_t m = mask; m; m &= m - 1) order[w++] = b + __builtin_ctz(m);
        npend += __shfl(incl, 63);
    }
    __syncthreads();
    auto is_taken = [&](int k) { return ((taken[k >> 5] >> (k & 31)) & 1u) != 0; };
    const uint64_t below = (1ull << lane) - 1;
    int events = 0, passes = 0, stales = 0, walks = 0;
    for (int g0 = 0; g0 < npend; g0 += 64) {
        bool pending = g0 + lane < npend;
        const int i = pending ? clampi(order[g0 + lane], 0, npts - 1) : 0;
        RelocCand c{};
        if (pending) c = cand[i];
#pragma unroll
        for (int t = 0; t < kTop; ++t) c.idx[t] = min(c.idx[t], nk - 1);  // (-1 stays: no candidate)
        c.level = clampi(c.level, 0, kMaxLevels - 1);
        pending = pending && c.n > 0;
        // This loop ends: a lane is stale only through an earlier pending lane of the group, so the lowest
        // pending lane never is, `first` lies above it and every pass commits it.  The pending set shrinks
        // by at least one lane a pass: at most 64 passes a group, whatever the data.
        while (__ballot(pending)) {
            int ak = -1, nexam = 0, bi = -1, bd = 256;
            if (pending) {
#pragma unroll
                for (int t = 0; t < kTop; ++t) {
                    const int k = c.idx[t];
                    if (bi >= 0 || k < 0) break;
                    nexam = t + 1;
                    if (is_taken(k)) continue;
                    bi = k, bd = c.dist[t];
                }
            }
            // every kept candidate is taken and more had passed: the whole wave walks that lane's window
            // again with the live occupancy (the band [level - 1, level] is the walk's level filter)
            const bool walked = pending && bi < 0 && c.n > kTop;
            const uint64_t wm0 = __ballot(walked);
            for (uint64_t wm = wm0; wm; wm &= wm - 1) {
                const int src = __builtin_ctzll(wm);
                const float u = __shfl(c.u, src), v = __shfl(c.v, src);
                const int level = __shfl(c.level, src);
                uint32_t q[8];
                load_desc(pts[__shfl(i, src)].desc, q);
                int wi;
                const int wd = walk_window_wave(a, F, u, v, level - 1, level, a.th * a.scale[level], 0.f, q, is_taken,
                                                lane, &wi);
                if (lane == src) bi = min(wi, nk - 1), bd = wd;
            }
            if (bi >= 0 && (float)bd <= a.limit) ak = bi;  // :524 / :637
            const bool reg = pending && ak >= 0;
            const uint64_t am = __ballot(reg);
            if (reg) atomicMin(&owner[ak], (uint32_t)lane);
            __syncthreads();
            bool stale = false;
            if (pending) {
                stale = walked && (am & below) != 0;
#pragma unroll
                for (int t = 0; t < kTop; ++t)
                    if (t < nexam) stale |= owner[c.idx[t]] < (uint32_t)lane;
            }
            __syncthreads();
            if (reg) owner[ak] = 64;
            const uint64_t st = __ballot(pending && stale);
            const int first = st ? __builtin_ctzll(st) : 64;
            const bool commit = pending && lane < first;
            if (commit) {  // no two committing lanes share a keypoint: the later one is stale
                if (ak >= 0) {  // :526-527 / :639-641
                    match[ak] = i;
                    atomicOr(&taken[ak >> 5], 1u << (ak & 31));
                    a.best_idx[(long long)row0 + i] = ak;
                    a.best_dist[(long long)row0 + i] = bd;
                    code[i] = kSim3Matched;
                } else {
                    code[i] = kSim3NotMatched;
                }
            }
            events += __popcll(__ballot(commit && ak >= 0));
            ++passes, stales += __popcll(st), walks += __popcll(wm0);
            pending = pending && !commit;
            __syncthreads();
        }
    }
    if (lane == 0) {
        a.nmatches[p] = events;
        int32_t* s = a.stats + p * kSim3Stats;
        s[0] = npend, s[1] = passes, s[2] = stales, s[3] = walks;
    }
}

}  // namespace

size_t sim3_resolve_lds_bytes(int out_cap) { return 4 * (size_t)sim3_lds_words(out_cap); }

hipError_t launch_sim3(const Sim3Args& a, int npairs, int max_pts, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    if (max_pts > 0) {
        const int blocks = (int)(((long long)max_pts * kSim3Lanes + 255) / 256);
        hipLaunchKernelGGL(k_sim3_candidates<kSim3Lanes>, dim3(blocks, npairs), dim3(256), 0, st, a);
    }
    const size_t lds = sim3_resolve_lds_bytes(a.out_cap);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_sim3_resolve),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_sim3_resolve, dim3(npairs), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
