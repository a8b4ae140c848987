// ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>&
// sAlreadyFound, th, ORBdist) (cpp/src/ORBmatcher.cc:1923-2059; ComputeThreeMaxima :2061-2102;
// MapPoint::PredictScale, MapPoint.cc:533-548), the search Tracking::Relocalization runs on a
// candidate keyframe after PnP left too few inliers, on pinhole frames (monocular path: mvKeysUn,
// GetFeaturesInArea(bRight = false), no mvuRight test), over pairs of a keyframe's points the host
// gives and a batch image whose keypoints, descriptors and grid already live in HBM.  Several pairs
// may name one frame, each with its own pose and occupancy.
//
// Per keyframe point, in index order: transform with the pose, project (Pinhole.cpp:40-41), gate
// the distance to the camera centre by the point's invariance range, predict the level from that
// distance, search a window of th * mvScaleFactors[level] over levels level +- 1, take the first
// lowest Hamming distance among the keypoints that hold no point, and assign when it is <= ORBdist.
// Each assignment takes its keypoint and is an event in the rotation histogram; after the loop
// every event in a bin outside the three maxima clears its keypoint and takes one off nmatches.
//
// The predicted level is ceil(log(ratio) / log(scaleFactor)) with the host libm's logf; the device
// library's need not equal it near a step.  The level is a step function of the ratio, so the host
// finds the steps once (predict_scale_table, orb_matchers.cpp) and the device counts the steps below
// the ratio: no logarithm runs here.
//
// The loop is sequential -- a keypoint taken by a point is skipped by every later point -- so, as
// in orb_track.hip:
//   k_reloc_candidates  one thread per point: validity, projection, distance gate, level, window
//                       walk against the pre-call occupancy; keeps the 4 lowest (distance, window
//                       position) candidates within ORBdist and how many were within it.
//   k_reloc_resolve     one wave per pair replays the points 64 at a time: a lane's match is the
//                       first of its kept candidates not taken so far (the whole wave walks the
//                       window again with the live occupancy when all kept ones are taken and more
//                       had passed); the prefix of lanes no earlier lane of the group disturbs
//                       commits at once.  Every event takes its keypoint, so a keypoint is assigned
//                       at most once in a call: its match and bin are stored per keypoint, the
//                       bin sizes in an LDS histogram, and the three-maxima rule clears by bin.
//
// Deviations from the reference, which reads out of range in these cases: a point whose
// projection, distance or ratio is not finite is skipped; an event whose bin falls outside
// [0, 30) (angles not finite) counts in nmatches, enters no bin and cannot be rejected.
#include <hip/hip_runtime.h>

#include "orb_kernels.h"
#include "orb_window.h"

namespace orbgpu {
namespace {

constexpr int kTop = 4;

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Pair p's slice of the points, clamped to what the launch sized.
__device__ inline void reloc_range(const RelocArgs& a, int p, int* m0, int* np) {
    *m0 = max(a.kf_off[p], 0);
    *np = max(a.kf_off[p + 1] - *m0, 0);
}

__global__ __launch_bounds__(256) void k_reloc_candidates(RelocArgs a) {
    const int p = blockIdx.y;
    int m0, np;
    reloc_range(a, p, &m0, &np);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const RelocPoint pt = a.pts[m0 + j];
    RelocCand c;
#pragma unroll
    for (int t = 0; t < kTop; ++t) c.idx[t] = -1, c.dist[t] = 256;
    c.n = -1;
    c.level = 0;
    c.u = c.v = 0.f;
    RelocCand& out = a.cand[m0 + j];
    out = c;
    if (!(pt.flags & kRpValid)) return;  // :1941-1944
    const RelocPose T = a.poses[p];
    const float X = pt.pos[0], Y = pt.pos[1], Z = pt.pos[2];
    float xc, yc, zc, u, v;
    project_pinhole(T.Rcw, T.tcw, a.K, pt.pos, &xc, &yc, &zc, &u, &v);
    if (u < a.bounds[0] || u > a.bounds[1]) return;  // :1953-1956
    if (v < a.bounds[2] || v > a.bounds[3]) return;
    if (!isfinite(u) || !isfinite(v)) return;
    const float px = X - T.Ow[0], py = Y - T.Ow[1], pz = Z - T.Ow[2];  // :1959-1960
    const float dist3D = sqrtf((px * px + py * py) + pz * pz);
    if (!isfinite(dist3D)) return;
    if (dist3D < 0.8f * pt.min_distance || dist3D > 1.2f * pt.max_distance) return;  // :1966
    const float ratio = pt.max_distance / dist3D;  // MapPoint.cc:538
    if (!isfinite(ratio)) return;
    const int nsteps = clampi(a.nlevels - 1, 0, kMaxLevels - 1);
    int level = 0;
#pragma unroll
    for (int n = 0; n < kMaxLevels - 1; ++n) level += (n < nsteps && ratio > a.level_step[n]) ? 1 : 0;
    const float radius = a.th * a.scale[level];
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)p * a.out_cap : nullptr;
    const FrameView F = frame_view_of(a, a.frames[p], nullptr);
    uint32_t q[8];
    load_desc(pt.desc, q);
    c.n = 0;
    walk_window(a, F, u, v, level - 1, level + 1, radius, 0.f, q, [&](int k) { return blk && blk[k]; },
                [&](int k, int d, int) {
                    if (d > a.orb_dist) return;  // can never become an event (:2004)
                    ++c.n;
                    top4_insert(c.idx, c.dist, k, d);
                });
    c.level = level, c.u = u, c.v = v;
    out = c;
}

// Dynamic LDS of k_reloc_resolve for n keypoints per frame: the occupancy bitmap, the owner and
// match tables, the bin of each keypoint's event and the histogram (+ the rejected set, its size).
__host__ __device__ inline int reloc_lds_words(int n) { return (n + 31) / 32 + 2 * n + (n + 3) / 4 + kRotBins + 2; }

// The bin of rot = angleKF - angleF (:2013-2024); kNoBin outside [0, 30).
__device__ inline uint32_t reloc_bin(float kang, float fang) {
    float rot = kang - fang;
    if (rot < 0.0f || rot > 360.0f) rot = fmodf(rot, 360.0f);
    if (rot < 0.0f) rot += 360.0f;
    const float rb = roundf(rot * (1.0f / 30));
    if (!(rb >= 0.f && rb <= 30.f)) return kNoBin;
    const int bin = (int)rb;
    return bin == kRotBins ? 0u : (uint32_t)bin;
}

__global__ __launch_bounds__(64) void k_reloc_resolve(RelocArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int ncap = a.out_cap;
    uint32_t* taken = lds;                                          // keypoint holds a point
    uint32_t* owner = taken + (ncap + 31) / 32;                     // lowest pending lane assigning it
    int32_t* matchl = reinterpret_cast<int32_t*>(owner + ncap);
    uint8_t* mbin = reinterpret_cast<uint8_t*>(matchl + ncap);      // bin of the keypoint's event
    uint32_t* hist = reinterpret_cast<uint32_t*>(mbin) + (ncap + 3) / 4;  // [kRotBins], the rejected set, its size
    const int p = blockIdx.x, lane = threadIdx.x;
    const int img = a.frames[p];
    const int nk = clampi(a.out_n[img], 0, ncap);
    int m0, npts;
    reloc_range(a, p, &m0, &npts);
    const RelocCand* cand = a.cand + m0;
    const RelocPoint* pts = a.pts + m0;
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
        matchl[k] = -1;
        mbin[k] = kNoBin;
    }
    if (lane < kRotBins + 2) hist[lane] = 0;
    __syncthreads();
    auto is_taken = [&](int k) { return ((taken[k >> 5] >> (k & 31)) & 1u) != 0; };
    const uint64_t below = (1ull << lane) - 1;
    int events = 0;
    for (int g0 = 0; g0 < npts; g0 += 64) {
        const int i = g0 + lane;
        bool pending = i < npts;
        RelocCand c{};
        c.n = -1;
        if (pending) c = cand[i];
#pragma unroll
        for (int t = 0; t < kTop; ++t) c.idx[t] = min(c.idx[t], nk - 1);  // (-1 stays: no candidate)
        c.level = clampi(c.level, 0, kMaxLevels - 1);
        pending = pending && c.n > 0;  // skipped points and windows with nothing within ORBdist assign nothing
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
            // every kept candidate is taken and more had passed: the whole wave walks that lane's
            // window again with the live occupancy
            const bool walked = pending && bi < 0 && c.n > kTop;
            for (uint64_t wm = __ballot(walked); wm; wm &= wm - 1) {
                const int src = __builtin_ctzll(wm);
                const float u = __shfl(c.u, src), v = __shfl(c.v, src);
                const int level = __shfl(c.level, src);
                uint32_t q[8];
                load_desc(pts[__shfl(i, src)].desc, q);
                int wi;
                const int wd = walk_window_wave(a, F, u, v, level - 1, level + 1, a.th * a.scale[level], 0.f, q,
                                                is_taken, lane, &wi);
                if (lane == src) bi = min(wi, nk - 1), bd = wd;
            }
            if (bd <= a.orb_dist) ak = bi;
            // staleness against the earlier pending lanes of the group: every assignment takes its
            // keypoint from the later ones
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
            const bool ev = commit && ak >= 0;  // no two committing lanes share a keypoint: the later one is stale
            if (ev) {  // :2006-2027
                matchl[ak] = i;
                atomicOr(&taken[ak >> 5], 1u << (ak & 31));
                if (a.check_orientation) {
                    const uint32_t bin = reloc_bin(pts[i].angle, angle_of(F, ak));
                    mbin[ak] = (uint8_t)bin;
                    if (bin < kRotBins) atomicAdd(&hist[bin], 1u);
                }
            }
            events += __popcll(__ballot(ev));
            pending = pending && !commit;
            __syncthreads();
        }
    }
    int nmatches = events;
    if (a.check_orientation) {  // :2036-2056
        if (lane == 0) three_maxima_reject(hist);
        __syncthreads();
        nmatches -= (int)hist[kRotBins + 1];
    }
    const uint32_t rej = hist[kRotBins];
    int32_t* match = a.match + (long long)p * ncap;
    for (int k = lane; k < nk; k += 64) match[k] = ((rej >> (mbin[k] & 31)) & 1u) ? -1 : matchl[k];
    if (lane < kRotBins) a.rot_hist[p * kRotBins + lane] = (int32_t)hist[lane];
    if (lane == 0) a.nmatches[p] = nmatches;
}

}  // namespace

size_t reloc_resolve_lds_bytes(int out_cap) { return 4 * (size_t)reloc_lds_words(out_cap); }

hipError_t launch_reloc(const RelocArgs& a, int npairs, int max_pts, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    if (max_pts > 0)
        hipLaunchKernelGGL(k_reloc_candidates, dim3((max_pts + 255) / 256, npairs), dim3(256), 0, st, a);
    const size_t lds = reloc_resolve_lds_bytes(a.out_cap);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_reloc_resolve),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_reloc_resolve, dim3(npairs), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
