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
#include <hip/hip_runtime.h>

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
                    bool shift = false;  // (distance, window position) order: after equal distances
#pragma unroll
                    for (int j = 0; j < kTop; ++j) {
                        shift = shift || d < c.dist[j];
                        if (shift) {
                            const int ti = c.idx[j], td = c.dist[j];
                            c.idx[j] = k, c.dist[j] = d;
                            k = ti, d = td;
                        }
                    }
                });
    c.u = u, c.v = v, c.invz = invz;
    out = c;
}

// Dynamic LDS of k_track_resolve for n keypoints per frame: the occupancy bitmap, four
// per-keypoint tables (owner, writer, bin mask, match) and the histogram (+ the rejected set).
__host__ __device__ inline int track_lds_words(int n) { return (n + 31) / 32 + 4 * n + kRotBins + 2; }

__global__ __launch_bounds__(64) void k_track_resolve(TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int ncap = a.out_cap;
    const int nbits = (ncap + 31) / 32;
    uint32_t* taken = lds;                 // keypoint held by a point with observations
    uint32_t* owner = taken + nbits;       // lowest pending lane with observations assigning it
    int32_t* writer = reinterpret_cast<int32_t*>(owner + ncap);  // last committing lane assigning it
    uint32_t* binmask = reinterpret_cast<uint32_t*>(writer + ncap);  // bins of the keypoint's events
    int32_t* matchl = reinterpret_cast<int32_t*>(binmask + ncap);
    uint32_t* hist = reinterpret_cast<uint32_t*>(matchl + ncap);  // [kRotBins], then the rejected set
    const int f = blockIdx.x, lane = threadIdx.x;
    const int nk = min(max(a.out_n[f * a.image_step], 0), ncap);
    const int m0 = a.pt_off[f], m1 = a.pt_off[f + 1];
    const uint8_t* blk = a.kp_block ? a.kp_block + (long long)f * ncap : nullptr;
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
    const FrameView F = track_view(a, f);
    const int dir = a.frames[f].dir;
    auto is_taken = [&](int k) { return ((taken[k >> 5] >> (k & 31)) & 1u) != 0; };
    const uint64_t below = (1ull << lane) - 1;
    int events = 0;
    for (int g0 = m0; g0 < m1; g0 += 64) {
        const int i = g0 + lane;
        bool pending = i < m1;
        TrackCand c{};
        c.n = -1;
        if (pending) c = a.cand[i];
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
                load_desc(a.pts[__shfl(i, src)].desc, q);
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
                matchl[ak] = i - m0;
                if (obs) atomicOr(&taken[ak >> 5], 1u << (ak & 31));
            }
            if (ev && a.check_orientation) {  // :1829-1837
                float rot = c.angle - angle_of(F, ak);
                if (rot < 0.0f) rot += 360.0f;
                const float b = roundf(rot * (1.0f / 30));
                if (b >= 0.f && b <= 30.f) {
                    int bin = (int)b;
                    if (bin == kRotBins) bin = 0;
                    atomicAdd(&hist[bin], 1u);
                    atomicOr(&binmask[ak], 1u << bin);
                }
            }
            events += __popcll(__ballot(ev));
            pending = pending && !commit;
            __syncthreads();
        }
    }
    // ComputeThreeMaxima (:2061-2102) and the rejection (:1697-1716)
    int nmatches = events;
    if (a.check_orientation) {
        if (lane == 0) {
            int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
            for (int b = 0; b < kRotBins; ++b) {
                const int s = (int)hist[b];
                if (s > max1) {
                    max3 = max2, max2 = max1, max1 = s;
                    ind3 = ind2, ind2 = ind1, ind1 = b;
                } else if (s > max2) {
                    max3 = max2, max2 = s;
                    ind3 = ind2, ind2 = b;
                } else if (s > max3) {
                    max3 = s, ind3 = b;
                }
            }
            if ((float)max2 < 0.1f * (float)max1) {
                ind2 = -1, ind3 = -1;
            } else if ((float)max3 < 0.1f * (float)max1) {
                ind3 = -1;
            }
            uint32_t rej = 0;
            int dropped = 0;
            for (int b = 0; b < kRotBins; ++b)
                if (b != ind1 && b != ind2 && b != ind3) rej |= 1u << b, dropped += (int)hist[b];
            hist[kRotBins] = rej;
            hist[kRotBins + 1] = (uint32_t)dropped;
        }
        __syncthreads();
        nmatches -= (int)hist[kRotBins + 1];
    }
    const uint32_t rej = hist[kRotBins];
    int32_t* match = a.match + (long long)f * ncap;
    for (int k = lane; k < nk; k += 64) match[k] = (binmask[k] & rej) ? -1 : matchl[k];
    if (lane < kRotBins) a.rot_hist[f * kRotBins + lane] = (int32_t)hist[lane];
    if (lane == 0) a.nmatches[f] = nmatches;
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

}  // namespace orbgpu
