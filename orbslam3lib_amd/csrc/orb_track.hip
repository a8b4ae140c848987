// ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)
// (cpp/src/ORBmatcher.cc:1683-1838: the pinhole branch, Nleft == -1; ComputeThreeMaxima :2061-2102),
// Tracking::TrackWithMotionModel's frame-to-frame search, over current frames whose mvKeysUn,
// octaves, angles, descriptors, grid and mvuRight already live in HBM.
//
// Per last-frame point, in index order: transform with the current pose, project (Pinhole.cpp:
// 40-41), search a window of th * mvScaleFactors[octave] whose level range depends on the motion
// direction (:1767-1776), take the first lowest Hamming distance among the keypoints that do not
// hold a point with observations, and assign when it is <= TH_HIGH.  Each assignment is an event in
// the rotation histogram; after the loop every event in a bin outside the three maxima clears its
// keypoint and takes one off nmatches (:1697-1716).
//
// The loop is sequential -- a keypoint taken by a point with observations is skipped by every
// later point -- so, as in orb_sbp.hip:
//   k_track_candidates  one thread per point: transform, projection, window walk against the
//                       pre-call occupancy; keeps the 4 lowest (distance, window position)
//                       candidates, their count, and u / v / 1/z / the last-frame angle.
//   k_track_resolve     one wave per frame replays the points 64 at a time: a lane's match is the
//                       first of its kept candidates not taken so far (the whole wave walks the
//                       window again with the live occupancy when all kept ones are taken, more
//                       had passed and the last kept one is within TH_HIGH);
//                       the prefix of lanes no earlier lane of the group disturbs commits at once.
//                       Only assignments by points with observations take a keypoint, so the
//                       occupancy only grows and only those can disturb a later lane.  Each
//                       committed event adds to the LDS histogram and ORs its bin into the
//                       keypoint's bin mask; after the replay the three-maxima rule clears every
//                       keypoint whose mask meets a rejected bin.
//
// Deviations from the reference, which reads out of range in these cases: a point whose projection
// is not finite, or whose octave is outside [0, nlevels), is skipped; an event whose bin falls
// outside [0, 30) (angles outside [0, 360) or not finite) counts in nmatches but enters no bin.
//
// The two-camera branch (Nleft != -1, :1840-1914) follows the pinhole kernels below.
#include <hip/hip_runtime.h>

#include "orb_kb8.h"
#include "orb_kernels.h"
#include "orb_window.h"

namespace orbgpu {
namespace {

constexpr int kTop = 4;
constexpr int kThHigh = 100;  // ORBmatcher::TH_HIGH

// The window's level range (:1767-1776).
__device__ inline void track_levels(int dir, int octave, int* minLevel, int* maxLevel) {
    if (dir == kTrackForward) {
        *minLevel = octave, *maxLevel = -1;
    } else if (dir == kTrackBackward) {
        *minLevel = 0, *maxLevel = octave;
    } else {
        *minLevel = octave - 1, *maxLevel = octave + 1;
    }
}

__device__ inline FrameView track_view(const TrackArgs& a, int f) {
    return frame_view_of(a, f * a.image_step, a.uright ? a.uright + (long long)f * a.out_cap : nullptr);
}

__global__ __launch_bounds__(256) void k_track_candidates(TrackArgs a) {
    const int f = blockIdx.y;
    const int m0 = a.pt_off[f], m1 = a.pt_off[f + 1];
    const int i = m0 + blockIdx.x * 256 + threadIdx.x;
    if (i >= m1) return;
    const LastPointIn p = a.pts[i];
    TrackCand c;
#pragma unroll
    for (int j = 0; j < kTop; ++j) c.idx[j] = -1, c.dist[j] = 256;
    c.n = -1;
    c.flags = p.flags;
    c.octave = p.octave;
    c.u = c.v = c.invz = 0.f;
    c.angle = p.angle;
    c.pad = 0;
    TrackCand& out = a.cand[i];
    out = c;
    if (!(p.flags & kLpValid)) return;
    const TrackFrame T = a.frames[f];
    const float X = p.pos[0], Y = p.pos[1], Z = p.pos[2];
    const float xc = ((T.Rcw[0] * X + T.Rcw[1] * Y) + T.Rcw[2] * Z) + T.tcw[0];
    const float yc = ((T.Rcw[3] * X + T.Rcw[4] * Y) + T.Rcw[5] * Z) + T.tcw[1];
    const float zc = ((T.Rcw[6] * X + T.Rcw[7] * Y) + T.Rcw[8] * Z) + T.tcw[2];
    const float invz = 1.0f / zc;
    if (invz < 0) return;
    const float u = a.K[0] * xc / zc + a.K[2];
    const float v = a.K[1] * yc / zc + a.K[3];
    if (u < a.bounds[0] || u > a.bounds[1]) return;
    if (v < a.bounds[2] || v > a.bounds[3]) return;
    if (!isfinite(u) || !isfinite(v)) return;
    if (p.octave < 0 || p.octave >= a.nlevels) return;
    const float radius = a.th * a.scale[p.octave];
    int minLevel, maxLevel;
    track_levels(T.dir, p.octave, &minLevel, &maxLevel);
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)f * a.out_cap : nullptr;
    const FrameView F = track_view(a, f);
    uint32_t q[8];
    load_desc(p.desc, q);
    c.n = 0;
    walk_window(a, F, u, v, minLevel, maxLevel, radius, u - a.mbf * invz, q, [&](int k) { return blk && blk[k]; },
                [&](int k, int d, int) {
                    ++c.n;
                    top4_insert(c.idx, c.dist, k, d);
                });
    c.u = u, c.v = v, c.invz = invz;
    out = c;
}

// Dynamic LDS of k_track_resolve for n keypoints per frame: the occupancy bitmap, four
// per-keypoint tables (owner, writer, bin mask, match) and the histogram (+ the rejected set).
__host__ __device__ inline int track_lds_words(int n) { return (n + 31) / 32 + 4 * n + kRotBins + 2; }

struct ReplayLds {
    uint32_t* taken;    // keypoint held by a point with observations
    uint32_t* owner;    // lowest pending lane with observations assigning it
    int32_t* writer;    // last committing lane assigning it
    uint32_t* binmask;  // bins of the keypoint's events
    int32_t* matchl;
    uint32_t* hist;     // [kRotBins], then the rejected set and its size
};
__device__ inline ReplayLds replay_lds(uint32_t* lds, int ncap) {
    ReplayLds L;
    L.taken = lds;
    L.owner = L.taken + (ncap + 31) / 32;
    L.writer = reinterpret_cast<int32_t*>(L.owner + ncap);
    L.binmask = reinterpret_cast<uint32_t*>(L.writer + ncap);
    L.matchl = reinterpret_cast<int32_t*>(L.binmask + ncap);
    L.hist = reinterpret_cast<uint32_t*>(L.matchl + ncap);
    return L;
}

// The sequential loop of one frame (pinhole) or of one side of a two-camera frame, by one wave:
// the frame's (side's) nk keypoints F with their pre-call occupancy blk, its npts candidate
// records and points.  Leaves the pre-rejection match, the bin masks and the histogram in LDS and
// returns the number of events.
template <class Args>
__device__ inline int track_replay(const Args& a, const FrameView& F, const ReplayLds& L, const TrackCand* cand,
                                   const LastPointIn* pts, int npts, int nk, const uint8_t* blk, int dir, int lane) {
    uint32_t* taken = L.taken;
    uint32_t* owner = L.owner;
    int32_t* writer = L.writer;
    uint32_t* binmask = L.binmask;
    int32_t* matchl = L.matchl;
    uint32_t* hist = L.hist;
    for (int w = lane; w < (nk + 31) / 32; w += 64) {
        uint32_t bits = 0;
        if (blk)
            for (int b = 0; b < 32 && w * 32 + b < nk; ++b) bits |= (blk[w * 32 + b] ? 1u : 0u) << b;
        taken[w] = bits;
    }
    for (int k = lane; k < nk; k += 64) {
        owner[k] = 64;
        writer[k] = -1;
        binmask[k] = 0;
        matchl[k] = -1;
    }
    if (lane < kRotBins + 2) hist[lane] = 0;
    __syncthreads();
    auto is_taken = [&](int k) { return ((taken[k >> 5] >> (k & 31)) & 1u) != 0; };
    const uint64_t below = (1ull << lane) - 1;
    int events = 0;
    for (int g0 = 0; g0 < npts; g0 += 64) {
        const int i = g0 + lane;
        bool pending = i < npts;
        TrackCand c{};
        c.n = -1;
        if (pending) c = cand[i];
        pending = pending && c.n > 0;  // skipped points and empty windows assign nothing
        const bool obs = pending && (c.flags & kMpHasObs) != 0;
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
            // every kept candidate is taken and more had passed: walk the window again with the
            // live occupancy -- unless the last kept one is already above TH_HIGH, as every
            // candidate not kept is at least as far.  The whole wave walks one lane's window.
            const bool walked = pending && bi < 0 && c.n > kTop && c.dist[kTop - 1] <= kThHigh;
            for (uint64_t wm = __ballot(walked); wm; wm &= wm - 1) {
                const int src = __builtin_ctzll(wm);
                const float u = __shfl(c.u, src), v = __shfl(c.v, src), invz = __shfl(c.invz, src);
                const int octave = __shfl(c.octave, src);
                int minLevel, maxLevel;
                track_levels(dir, octave, &minLevel, &maxLevel);
                uint32_t q[8];
                load_desc(pts[__shfl(i, src)].desc, q);
                int wi;
                const int wd = walk_window_wave(a, F, u, v, minLevel, maxLevel, a.th * a.scale[octave], u - a.mbf * invz,
                                                q, is_taken, lane, &wi);
                if (lane == src) bi = wi, bd = wd;
            }
            if (bd <= kThHigh) ak = bi;
            // staleness against the earlier pending lanes of the group: only an assignment by a
            // point with observations takes its keypoint from the later ones
            const bool reg = pending && ak >= 0 && obs;
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
            const bool ev = commit && ak >= 0;
            // the reference keeps the last assignment of a keypoint
            if (ev) atomicMax(&writer[ak], lane);
            __syncthreads();
            const bool last = ev && writer[ak] == lane;
            __syncthreads();
            if (ev) writer[ak] = -1;
            if (last) {
                matchl[ak] = i;
                if (obs) atomicOr(&taken[ak >> 5], 1u << (ak & 31));
            }
            if (ev && a.check_orientation) {  // :1829-1837
                uint32_t bin;
                if (rot_bin(c.angle, angle_of(F, ak), &bin)) {
                    atomicAdd(&hist[bin], 1u);
                    atomicOr(&binmask[ak], 1u << bin);
                }
            }
            events += __popcll(__ballot(ev));
            pending = pending && !commit;
            __syncthreads();
        }
    }
    return events;
}

__global__ __launch_bounds__(64) void k_track_resolve(TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int ncap = a.out_cap;
    const ReplayLds L = replay_lds(lds, ncap);
    const int f = blockIdx.x, lane = threadIdx.x;
    const int nk = min(max(a.out_n[f * a.image_step], 0), ncap);
    const int m0 = a.pt_off[f], m1 = a.pt_off[f + 1];
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)f * ncap : nullptr;
    const int events =
        track_replay(a, track_view(a, f), L, a.cand + m0, a.pts + m0, m1 - m0, nk, blk, a.frames[f].dir, lane);
    int nmatches = events;
    if (a.check_orientation) {
        if (lane == 0) three_maxima_reject(L.hist);
        __syncthreads();
        nmatches -= (int)L.hist[kRotBins + 1];
    }
    const uint32_t rej = L.hist[kRotBins];
    int32_t* match = a.match + (long long)f * ncap;
    for (int k = lane; k < nk; k += 64) match[k] = (L.binmask[k] & rej) ? -1 : L.matchl[k];
    if (lane < kRotBins) a.rot_hist[f * kRotBins + lane] = (int32_t)L.hist[lane];
    if (lane == 0) a.nmatches[f] = nmatches;
}

// ---- the two-camera branch (CurrentFrame.Nleft != -1, :1840-1914) --------------------------------
// Frame f = left image 2f + right image 2f + 1.  A point's left window (the pinhole rules, with the
// KannalaBrandt8 projection and without the mvuRight test) and its right window (the point moved
// by Trl, projected with the *left* camera model as the reference does, no bounds / 1/z test) are
// separate events on disjoint keypoint ranges, and the left result never feeds the right window:
// the two sides are independent sequential chains, coupled by the static "left window
// geometrically empty -> point skipped" rule (:1778-1779), the shared histogram and nmatches.
//   k_track_candidates_stereo  two adjacent lanes per point (side = lane & 1): both transform the
//                       point, each projects and walks its side's window; the left lane's skip
//                       decision reaches the right lane by __shfl_xor.
//   k_track_resolve_stereo     one wave per (frame, side): track_replay on that side; writes the
//                       pre-rejection match, the bin masks, the side's histogram and event count.
//   k_track_finish_stereo      one workgroup per frame: adds the histograms, three maxima, clears
//                       every keypoint whose mask meets a rejected bin.
// Trl * x3Dc is evaluated as ((R0 x + R1 y) + R2 z) + t per row: Sophus's own order is not
// reproducible here, this one is the pinned choice.

__global__ __launch_bounds__(256) void k_track_candidates_stereo(TrackStereoArgs a) {
    const int f = blockIdx.y;
    const int m0 = a.pt_off[f], np = a.pt_off[f + 1] - m0;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int side = t & 1, j = t >> 1;
    if (j >= np) return;  // both lanes of a pair leave together
    const LastPointIn p = a.pts[m0 + j];
    TrackCand c;
#pragma unroll
    for (int s = 0; s < kTop; ++s) c.idx[s] = -1, c.dist[s] = 256;
    c.n = -1;
    c.flags = p.flags;
    c.octave = p.octave;
    c.u = c.v = c.invz = 0.f;
    c.angle = p.angle;
    c.pad = 0;
    const TrackFrame T = a.frames[f];
    const float X = p.pos[0], Y = p.pos[1], Z = p.pos[2];
    const float xc = ((T.Rcw[0] * X + T.Rcw[1] * Y) + T.Rcw[2] * Z) + T.tcw[0];
    const float yc = ((T.Rcw[3] * X + T.Rcw[4] * Y) + T.Rcw[5] * Z) + T.tcw[1];
    const float zc = ((T.Rcw[6] * X + T.Rcw[7] * Y) + T.Rcw[8] * Z) + T.tcw[2];
    const float invz = 1.0f / zc;
    const float* R = a.rig.Rrl;
    float x3[3];
    x3[0] = side ? ((R[0] * xc + R[1] * yc) + R[2] * zc) + a.rig.trl[0] : xc;
    x3[1] = side ? ((R[3] * xc + R[4] * yc) + R[5] * zc) + a.rig.trl[1] : yc;
    x3[2] = side ? ((R[6] * xc + R[7] * yc) + R[8] * zc) + a.rig.trl[2] : zc;
    float uv[2];
    kb8_project(a.rig.cam, x3, uv);
    const float u = uv[0], v = uv[1];
    const bool finite = isfinite(u) && isfinite(v);
    const bool octave_ok = p.octave >= 0 && p.octave < a.nlevels;
    // the point as a whole: the left lane's tests (the right lane's copy of them is overwritten)
    bool skip = !(p.flags & kLpValid) || invz < 0 || !octave_ok || !finite || u < a.bounds[0] || u > a.bounds[1] ||
                v < a.bounds[2] || v > a.bounds[3];
    const bool skip_left = __shfl_xor((int)skip, 1) != 0;
    if (side) skip = skip_left;
    const int nkL = min(max(a.out_n[2 * f], 0), a.out_cap);
    const uint8_t* blk = a.kp_block ? a.kp_block + 2LL * f * a.out_cap + (side ? nkL : 0) : nullptr;
    int seen = 0;  // keypoints that pass GetFeaturesInArea's level and distance tests
    if (!skip && (side == 0 || finite)) {
        const float radius = a.th * a.scale[p.octave];
        int minLevel, maxLevel;
        track_levels(T.dir, p.octave, &minLevel, &maxLevel);
        const FrameView F = frame_view_of(a, 2 * f + side, nullptr);
        uint32_t q[8];
        load_desc(p.desc, q);
        c.n = 0;
        walk_window(a, F, u, v, minLevel, maxLevel, radius, 0.f, q,
                    [&](int k) {
                        ++seen;
                        return blk && blk[k];
                    },
                    [&](int k, int d, int) {
                        ++c.n;
                        top4_insert(c.idx, c.dist, k, d);
                    });
        c.u = u, c.v = v;
    }
    // :1778-1779: an empty left window (before occupancy) skips the point, right window included
    const int seen_left = __shfl_xor(seen, 1);
    if (side && seen_left == 0) {
#pragma unroll
        for (int s = 0; s < kTop; ++s) c.idx[s] = -1, c.dist[s] = 256;
        c.n = -1;
    }
    a.cand[2LL * m0 + (long long)side * np + j] = c;
}

__global__ __launch_bounds__(64) void k_track_resolve_stereo(TrackStereoArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int ncap = a.out_cap;
    const ReplayLds L = replay_lds(lds, ncap);
    const int f = blockIdx.x, side = blockIdx.y, lane = threadIdx.x;
    const int nkL = min(max(a.out_n[2 * f], 0), ncap);
    const int nk = side ? min(max(a.out_n[2 * f + 1], 0), ncap) : nkL;
    const long long row = 2LL * f * ncap + (side ? nkL : 0);  // of kp_block, match and side_mask
    const int m0 = a.pt_off[f], np = a.pt_off[f + 1] - m0;
    const uint8_t* blk = a.kp_block ? a.kp_block + row : nullptr;
    const int events = track_replay(a, frame_view_of(a, 2 * f + side, nullptr), L, a.cand + 2LL * m0 + (long long)side * np,
                                    a.pts + m0, np, nk, blk, a.frames[f].dir, lane);
    for (int k = lane; k < nk; k += 64) {
        a.match[row + k] = L.matchl[k];
        a.side_mask[row + k] = L.binmask[k];
    }
    int32_t* h = a.side_hist + (2LL * f + side) * (kRotBins + 1);
    if (lane < kRotBins) h[lane] = (int32_t)L.hist[lane];
    if (lane == kRotBins) h[lane] = events;
}

__global__ __launch_bounds__(256) void k_track_finish_stereo(TrackStereoArgs a) {
    __shared__ uint32_t hist[kRotBins + 2];
    const int f = blockIdx.x, t = threadIdx.x;
    const int32_t* h = a.side_hist + 2LL * f * (kRotBins + 1);
    if (t < kRotBins + 2) hist[t] = t < kRotBins ? (uint32_t)(h[t] + h[kRotBins + 1 + t]) : 0u;
    __syncthreads();
    int nmatches = h[kRotBins] + h[2 * kRotBins + 1];
    if (a.check_orientation) {
        if (t == 0) three_maxima_reject(hist);
        __syncthreads();
        nmatches -= (int)hist[kRotBins + 1];
        const uint32_t rej = hist[kRotBins];
        const int n = min(max(a.out_n[2 * f], 0), a.out_cap) + min(max(a.out_n[2 * f + 1], 0), a.out_cap);
        const long long row = 2LL * f * a.out_cap;
        for (int k = t; k < n; k += 256)
            if (a.side_mask[row + k] & rej) a.match[row + k] = -1;
    }
    if (t < kRotBins) a.rot_hist[f * kRotBins + t] = (int32_t)hist[t];
    if (t == 0) a.nmatches[f] = nmatches;
}

}  // namespace

size_t track_resolve_lds_bytes(int out_cap) { return 4 * (size_t)track_lds_words(out_cap); }

hipError_t launch_track(const TrackArgs& a, int nframes, int max_pts, hipStream_t st) {
    if (nframes <= 0) return hipSuccess;
    if (max_pts > 0)
        hipLaunchKernelGGL(k_track_candidates, dim3((max_pts + 255) / 256, nframes), dim3(256), 0, st, a);
    const size_t lds = track_resolve_lds_bytes(a.out_cap);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_track_resolve),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_track_resolve, dim3(nframes), dim3(64), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_track_stereo(const TrackStereoArgs& a, int npairs, int max_pts, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    if (max_pts > 0)
        hipLaunchKernelGGL(k_track_candidates_stereo, dim3((2 * max_pts + 255) / 256, npairs), dim3(256), 0, st, a);
    const size_t lds = track_resolve_lds_bytes(a.out_cap);  // one side's keypoints per workgroup
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_track_resolve_stereo),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_track_resolve_stereo, dim3(npairs, 2), dim3(64), lds, st, a);
    hipLaunchKernelGGL(k_track_finish_stereo, dim3(npairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
