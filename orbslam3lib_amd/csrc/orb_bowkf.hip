// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (cpp/src/
// ORBmatcher.cc:766-906; ComputeThreeMaxima :2061-2102), the matcher LoopClosing::
// DetectCommonRegionsFromBoW runs for the current keyframe against every covisible of every candidate
// (LoopClosing.cc:657-668), on pinhole keyframes (NLeft == -1 on both), over pairs of a batch image
// whose descriptors and angles already live in HBM (keyframe 1) and a keyframe the host gives (keyframe
// 2: descriptor, angle, vocabulary node and map-point flag per keypoint).  The node of every keypoint
// (mFeatVec) is an input on both sides.
//
// It is the mirror of orb_bow.hip, not a copy: the batch image is the outer, sequential side (the
// search walks its keypoints and indexes vpMatches12 by them), the taken bits (vbMatched2) live on the
// host-given side, both sides carry an eligibility flag, and the distance gate is strict (bestDist1 <
// TH_LOW, :849).  Only keypoints of the same node are compared (:794-883) and vbMatched2 couples only
// the keypoints of one node, so a pair splits into its common nodes, each replayed in idx1 order:
//   k_bowkf_group   orb_bow_group.h's ordering of both sides by (node, index); side 0 (keyframe 2) also
//                   packs descriptor, angle and flag in that order, so that a node's candidates are
//                   contiguous; side 1 (keyframe 1) packs its descriptors and sets the pair's match row
//                   to -1.
//   k_bowkf_match   first the pair's waves code keyframe 1's keypoints in no node, shared out by index.
//                   Then one wave per node segment of keyframe 1.  Keyframe 2's segment of the same node is
//                   found by binary search; without one, the segment's keypoints get NODE_NOT_COMMON.
//                   Lane l holds keyframe 2's keypoints l, l + 64, ... of the segment: the first 64 in
//                   registers with one "busy" bit (taken, or without a map point: :827-831 pass both
//                   over alike), the chunks above re-read per keypoint 1, their busy bits in LDS.
//                   Keyframe 1's keypoints are staged 64 at a time, one per lane, so that no load sits
//                   in the sequential chain.  Per staged keypoint with a map point, its descriptor
//                   wave-uniform (read from its lane): eight popcounts per lane and chunk, the lane's
//                   two lowest distance << 16 | position keys over the keypoints not busy, two wave
//                   reductions (the first is bestDist1 / bestIdx2 with the reference's strict <, the
//                   second bestDist2), one event test per wave; the busy bit is set, and the staging
//                   lane keeps position, code and the two distances.  After the chain of its 64 each
//                   lane writes match, bin, code and distances of its keypoint.  A keypoint 1 belongs to
//                   one node, hence to one wave: no atomics.
//   k_bowkf_finish  the steps of orb_bow_group.h's finish: bin sizes from the stored bins, three_maxima_reject, the
//                   rejected matches cleared (:885-903) and coded ROTATION_REJECTED, nmatches.  A cleared
//                   match does not free its keypoint 2: nothing reads vbMatched2 afterwards.
// Every keypoint of keyframe 1 is coded exactly once before the finish, in k_bowkf_match: with the others
// in no node, or by the wave of its node segment.
//
// Deviations from the reference: a negative node means "in no node"; an event whose bin falls
// outside [0, 30) (the reference asserts) counts in nmatches, enters no bin and cannot be rejected.
#include <hip/hip_runtime.h>

#include "orb_bow_group.h"

namespace orbgpu {
namespace {

constexpr int kBowKfWaves = 128;   // waves per pair in k_bowkf_match, each striding over the segments (k_bow_match's)
constexpr int kBowKfHasPoint = 1;  // ORBGPU_BOWKF_HAS_POINT

__global__ __launch_bounds__(kGroupThreads) void k_bowkf_group(BowKfArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // [npad]
    bow_group_body(a, keys, [&a](const uint64_t* keys, int m, int n) {
        const int o0 = a.kf_off[blockIdx.x];
        const BowPoint* kf = a.kf_pts + o0;
        for (int j = threadIdx.x; j < m; j += kGroupThreads) {
            const BowPoint& pt = kf[min((int)(uint32_t)keys[j], n - 1)];
            a.kf_desc[2LL * (o0 + j)] = make_uint4(pt.desc[0], pt.desc[1], pt.desc[2], pt.desc[3]);
            a.kf_desc[2LL * (o0 + j) + 1] = make_uint4(pt.desc[4], pt.desc[5], pt.desc[6], pt.desc[7]);
            a.kf_meta[o0 + j] = make_float2(pt.angle, __int_as_float(pt.flags & kBowKfHasPoint));
        }
    });
}

__global__ __launch_bounds__(64) void k_bowkf_match(BowKfArgs a) {
    __shared__ uint64_t busy[kBowMaxPoints / 64];  // per 64 positions of keyframe 2's segment, from 64 on
    const int p = blockIdx.y, lane = threadIdx.x, cap = a.out_cap;
    const BowSide K = bow_kf_side(a, p), F = bow_f_side(a, p);
    const int nsegK = clampi(a.nseg[2 * p], 0, K.n), nsegF = clampi(a.nseg[2 * p + 1], 0, F.n);
    const int o0 = a.kf_off[p];
    const uint4* kdesc = a.kf_desc + 2LL * o0;
    const float2* kmeta = a.kf_meta + o0;
    const uint8_t* fdesc = a.f_desc + 32LL * p * cap;
    const uint8_t* fkps = static_cast<const uint8_t*>(a.kps) + 28LL * a.frames[p] * cap;
    const uint8_t* fflags = a.f_flags ? a.f_flags + (long long)p * cap : nullptr;
    int32_t* match = a.match + (long long)p * cap;
    short2* best = a.best + (long long)p * cap;
    uint8_t* mbin = a.match_bin + (long long)p * cap;
    uint8_t* code = a.code + (long long)p * cap;
    // keyframe 1's keypoints in no node belong to no segment: the pair's waves share them out by index (as a
    // tail of k_bowkf_group this loop cost 22 us per 256 pairs: every workgroup of 1024 ended on its loads)
    const int32_t* fnode = a.f_nodes + (long long)p * cap;
    for (int k = blockIdx.x * 64 + lane; k < F.n; k += gridDim.x * 64)
        if (fnode[k] < 0) {
            code[k] = kBowKfNoNode;
            best[k] = make_short2(0, 0);
        }
    for (int s = blockIdx.x; s < nsegF; s += gridDim.x) {
        const int sk = find_segment(K.seg_node, nsegK, F.seg_node[s], lane);  // keyframe 2's segment of the node
        const int fs = clampi(F.seg_start[s], 0, F.n), fe = clampi(F.seg_start[s + 1], fs, F.n);
        if (sk < 0) {  // a node of keyframe 1 only
            for (int i = fs + lane; i < fe; i += 64) {
                const int idx1 = clampi(F.order[i], 0, F.n - 1);
                code[idx1] = kBowKfNodeNotCommon;
                best[idx1] = make_short2(0, 0);
            }
            continue;
        }
        const int ks = clampi(K.seg_start[sk], 0, K.n), nk = clampi(K.seg_start[sk + 1], ks, K.n) - ks;
        const int nch = (nk + 63) >> 6;
        if (nch > 1) {  // the chunks above the first: busy = without a map point (or beyond the segment)
            __syncthreads();  // the previous segment's last read of busy[]
            for (int c = 1; c < nch; ++c) {
                const int pos = c * 64 + lane;
                const uint64_t free = __ballot(pos < nk && (__float_as_int(kmeta[ks + min(pos, nk - 1)].y) & kBowKfHasPoint));
                if (lane == 0) busy[c] = ~free;
            }
            __syncthreads();
        }
        // keyframe 2's first 64 keypoints of the node, one per lane: descriptor and busy bit
        uint32_t d0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool busy0 = true;
        if (lane < nk) {
            const uint4 x = kdesc[2LL * (ks + lane)], y = kdesc[2LL * (ks + lane) + 1];
            d0[0] = x.x, d0[1] = x.y, d0[2] = x.z, d0[3] = x.w, d0[4] = y.x, d0[5] = y.y, d0[6] = y.z, d0[7] = y.w;
            busy0 = !(__float_as_int(kmeta[ks + lane].y) & kBowKfHasPoint);
        }
        for (int i0 = fs; i0 < fe; i0 += 64) {  // :798, idx1 ascending, 64 keypoints 1 staged per lane
            uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int idx1 = 0;
            bool has1 = false;  // lanes beyond the segment: skipped
            float ang1 = 0.f;
            const bool staged = i0 + lane < fe;
            if (staged) {
                idx1 = clampi(F.order[i0 + lane], 0, F.n - 1);
                has1 = fflags ? (fflags[idx1] & kBowKfHasPoint) != 0 : true;
                const uint4* d = reinterpret_cast<const uint4*>(fdesc + 32LL * (i0 + lane));
                const uint4 x = d[0], y = d[1];
                qd[0] = x.x, qd[1] = x.y, qd[2] = x.z, qd[3] = x.w, qd[4] = y.x, qd[5] = y.y, qd[6] = y.z, qd[7] = y.w;
                ang1 = *reinterpret_cast<const float*>(fkps + 28LL * idx1 + 12);
            }
            // (the staged loads land here, not at their first use inside the chain)
            asm volatile("" ::"v"(qd[0]), "v"(qd[1]), "v"(qd[2]), "v"(qd[3]), "v"(qd[4]), "v"(qd[5]), "v"(qd[6]), "v"(qd[7]),
                         "v"(ang1));
            // what this lane's keypoint 1 ends with: written after the chain
            int my_pos = -1, my_code = kBowKfNoMapPoint, my_best1 = 0, my_best2 = 0;
            for (uint64_t todo = __ballot(has1); todo; todo &= todo - 1) {  // :805-809 skips the others
                const int j = __builtin_ctzll(todo);
                uint32_t q[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) q[w] = lane_value(qd[w], j);
                uint32_t k1 = kNoKey, k2 = kNoKey;  // distance << 16 | position in the segment
                if (!busy0) {
                    int dist = 0;
#pragma unroll
                    for (int w = 0; w < 8; ++w) dist += __popc(q[w] ^ d0[w]);
                    k1 = ((uint32_t)dist << 16) | (uint32_t)lane;
                }
                for (int c = 1; c < nch; ++c) {
                    const int pos = c * 64 + lane;
                    if (pos < nk && !((busy[c] >> lane) & 1ull)) {
                        const uint4 x = kdesc[2LL * (ks + pos)], y = kdesc[2LL * (ks + pos) + 1];
                        const int dist = __popc(q[0] ^ x.x) + __popc(q[1] ^ x.y) + __popc(q[2] ^ x.z) + __popc(q[3] ^ x.w) +
                                         __popc(q[4] ^ y.x) + __popc(q[5] ^ y.y) + __popc(q[6] ^ y.z) + __popc(q[7] ^ y.w);
                        const uint32_t key = ((uint32_t)dist << 16) | (uint32_t)pos;
                        k2 = min(k2, max(k1, key));
                        k1 = min(k1, key);
                    }
                }
                // the wave's two lowest: the second is the lowest once the best's lane gives its own second
                const uint32_t low = wave_min(k1);
                k2 = wave_min(k1 == low ? k2 : k1);
                k1 = low;
                const int best1 = k1 == kNoKey ? 256 : (int)(k1 >> 16), best2 = k2 == kNoKey ? 256 : (int)(k2 >> 16);
                const bool below = best1 < kThLow;                                // :849, strict
                const bool ev = below && (float)best1 < a.nnratio * (float)best2;  // :851
                const int pos = (int)(k1 & 0xFFFFu);
                if (ev && lane == (pos & 63)) {  // the lane that holds keypoint 2: vbMatched2 (:854)
                    if (pos < 64) busy0 = true; else busy[pos >> 6] |= 1ull << (pos & 63);
                }
                if (lane == j) {
                    my_code = k1 == kNoKey ? kBowKfNoCandidate : !below ? kBowKfNotBelowThLow : !ev ? kBowKfRatioFailed : kBowKfMatched;
                    my_best1 = best1, my_best2 = best2;
                    my_pos = ev ? pos : -1;
                }
                if (nch > 1) __syncthreads();  // one wave: orders the busy bit before the next keypoint's reads
            }
            if (staged) {
                if (my_pos >= 0) {  // :853-866
                    const int at = ks + min(my_pos, nk - 1);
                    uint32_t bin = kNoBin;
                    if (a.check_orientation) rot_bin(ang1, kmeta[at].x, &bin);
                    match[idx1] = clampi(K.order[at], 0, K.n - 1);
                    mbin[idx1] = (uint8_t)bin;
                }
                code[idx1] = (uint8_t)my_code;
                best[idx1] = make_short2((short)my_best1, (short)my_best2);
            }
        }
    }
}

// bow_finish_body's steps (orb_bow_group.h), and the code of each cleared match (:885-903).
__global__ __launch_bounds__(256) void k_bowkf_finish(BowKfArgs a) {
    __shared__ uint32_t hist[kRotBins + 2];  // the bins, the rejected set, its size
    __shared__ int32_t wcnt[4];
    const int p = blockIdx.x, t = threadIdx.x, cap = a.out_cap;
    const int n = clampi(a.out_n[a.frames[p]], 0, min(cap, kBowMaxPoints));
    int32_t* match = a.match + (long long)p * cap;
    const uint8_t* mbin = a.match_bin + (long long)p * cap;
    uint8_t* code = a.code + (long long)p * cap;
    if (t < kRotBins + 2) hist[t] = 0;
    __syncthreads();
    for (int k = t; k < n; k += 256)  // the list of a bin holds idx1: one entry per match
        if (match[k] >= 0 && mbin[k] < kRotBins) atomicAdd(&hist[mbin[k]], 1u);
    __syncthreads();
    if (t < kRotBins) a.rot_hist[p * kRotBins + t] = (int32_t)hist[t];
    if (a.check_orientation && t == 0) three_maxima_reject(hist);
    __syncthreads();
    const uint32_t rej = hist[kRotBins];
    int nm = 0;
    for (int k = t; k < n; k += 256) {
        if (match[k] < 0) continue;
        if ((rej >> (mbin[k] & 31)) & 1u) match[k] = -1, code[k] = kBowKfRotationRejected; else ++nm;
    }
    for (int o = 32; o >= 1; o >>= 1) nm += __shfl_xor(nm, o);
    if ((t & 63) == 0) wcnt[t >> 6] = nm;
    __syncthreads();
    if (t == 0) a.nmatches[p] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

}  // namespace

hipError_t launch_bowkf_search(const BowKfArgs& a, int npairs, int max_side, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    size_t lds;
    if (const hipError_t e = bow_group_lds(k_bowkf_group, max_side, &lds)) return e;
    hipLaunchKernelGGL(k_bowkf_group, dim3(npairs, 2), dim3(kGroupThreads), lds, st, a);
    hipLaunchKernelGGL(k_bowkf_match, dim3(kBowKfWaves, npairs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_bowkf_finish, dim3(npairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
