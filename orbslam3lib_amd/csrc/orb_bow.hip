// ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&) (cpp/src/ORBmatcher.cc:
// 224-426; ComputeThreeMaxima :2061-2102), the matcher of Tracking::TrackReferenceKeyFrame and
// Tracking::Relocalization, on pinhole frames (F.Nleft == -1), over pairs of a keyframe the host
// gives (descriptor, angle, vocabulary node and map-point flag per keypoint) and a batch image whose
// descriptors and angles already live in HBM.  The vocabulary stays on the host: the node of every
// keypoint (mFeatVec, DBoW2::transform with levelsup = 4) is an input.
//
// Only keypoints of the same node are compared (:245-403), and the one sequential rule -- a keypoint
// of F that holds a match is skipped by every later keyframe keypoint (:279-280) -- couples only the
// keypoints of one node.  So a pair splits into its common nodes, each a small all-pairs Hamming
// problem replayed in keyframe index order:
//   k_bow_group   one workgroup per (pair, side) orders the side's keypoints by (node, index) with
//                 a bitonic sort of 64-bit keys in LDS -- node ids are arbitrary 31-bit values, so
//                 there is nothing to count over -- and writes the ordered index list and the node
//                 segment table.  Keypoints with a negative node drop out here; keyframe keypoints
//                 without a map point stay in the order (they are skipped at replay).  The frame
//                 side also packs its descriptors in that order, so that a node's descriptors are
//                 contiguous, and sets the pair's match row to -1.
//   k_bow_match   one wave per keyframe node segment.  The frame's segment of the same node is
//                 found by binary search; lane l holds the frame's descriptors l, l + 64, ... of
//                 the segment (the first 64 in registers with their index, angle and taken bit,
//                 the chunks above re-read per keyframe keypoint, their taken bits in LDS).  The
//                 keyframe's keypoints are staged 64 at a time, one per lane, so that no load
//                 sits in the sequential chain.  Per keyframe keypoint in index order, its
//                 descriptor wave-uniform (read from its lane):
//                 eight popcounts per lane and chunk, the lane's two lowest distance << 16 |
//                 position keys over the keypoints not taken, two wave reductions for the two lowest
//                 (the first is bestDist1 / bestIdxF with the reference's strict <, the second is
//                 bestDist2), one event test per wave; then the taken bit, match and bin are
//                 written.  A frame keypoint belongs to one node, hence to one wave: no atomics on
//                 match, and none on the bins: the bin is stored beside the match.  The writes of
//                 the first 64 keypoints of a segment wait in registers until its chain has ended.
//   k_bow_finish  one workgroup per pair: the 30 bin sizes are counted from the stored bins (LDS
//                 integer atomics: order-independent), then three_maxima_reject, the matches whose
//                 bin is rejected are cleared (:405-423), nmatches is what is left.
//
// Deviations from the reference: a negative node means "in no node"; an event whose bin falls
// outside [0, 30) (the reference asserts) counts in nmatches, enters no bin and cannot be rejected.
// The bodies of k_bow_group and k_bow_finish and the wave minimum are in orb_bow_group.h, which
// orb_tri.hip shares.
#include <hip/hip_runtime.h>

#include "orb_bow_group.h"

namespace orbgpu {
namespace {

constexpr int kMatchWaves = 128;     // waves per pair in k_bow_match, each striding over the segments (measured:
                                     // 16 / 32 / 64 / 128 -> 0.228 / 0.218 / 0.208 / 0.199 ms per 256 pairs)

__global__ __launch_bounds__(kGroupThreads) void k_bow_group(BowArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // [npad]
    bow_group_body(a, keys, [](const uint64_t*, int, int) {});
}

// An event's writes (:332-354) by the lane that holds frame keypoint idxF: match and the bin of rot =
// kang - angF.  A frame keypoint is taken once, so k_bow_finish counts the bins from these.
__device__ inline void bow_commit(const BowArgs& a, int32_t* match, uint8_t* mbin, int idxF, float angF, int kidx,
                                  float kang) {
    uint32_t bin = kNoBin;
    if (a.check_orientation) rot_bin(kang, angF, &bin);
    match[idxF] = kidx;
    mbin[idxF] = (uint8_t)bin;
}

__global__ __launch_bounds__(64) void k_bow_match(BowArgs a) {
    __shared__ uint64_t taken[kBowMaxPoints / 64];  // per 64 positions of the frame's segment, from 64 on
    const int p = blockIdx.y, lane = threadIdx.x, cap = a.out_cap;
    const BowSide K = bow_kf_side(a, p), F = bow_f_side(a, p);
    const int nsegK = clampi(a.nseg[2 * p], 0, K.n), nsegF = clampi(a.nseg[2 * p + 1], 0, F.n);
    const BowPoint* kf = a.kf_pts + a.kf_off[p];
    const uint8_t* fdesc = a.f_desc + 32LL * p * cap;
    const uint8_t* fkps = static_cast<const uint8_t*>(a.kps) + 28LL * a.frames[p] * cap;
    int32_t* match = a.match + (long long)p * cap;
    uint8_t* mbin = a.match_bin + (long long)p * cap;
    for (int s = blockIdx.x; s < nsegK; s += gridDim.x) {
        const int node = K.seg_node[s];
        // the frame's segment of the node: halve while the first node >= it lies in [lo, hi], then one
        // probe per lane
        int lo = 0, hi = nsegF;
        while (hi - lo > 63) {
            const int mid = (lo + hi) >> 1;
            if (F.seg_node[mid] < node) lo = mid + 1; else hi = mid;
        }
        const uint64_t hit = __ballot(lo + lane <= hi && lo + lane < nsegF && F.seg_node[lo + lane] == node);
        if (!hit) continue;  // a node of the keyframe only
        lo += __builtin_ctzll(hit);
        const int ks = clampi(K.seg_start[s], 0, K.n), ke = clampi(K.seg_start[s + 1], ks, K.n);
        const int fs = clampi(F.seg_start[lo], 0, F.n), nf = clampi(F.seg_start[lo + 1], fs, F.n) - fs;
        const int nch = (nf + 63) >> 6;
        if (nch > 1) {
            __syncthreads();  // the previous segment's last read of taken[]
            for (int c = 1 + lane; c < nch; c += 64) taken[c] = 0;
            __syncthreads();
        }
        // the frame's first 64 keypoints of the node, one per lane: descriptor, index, angle, taken
        uint32_t d0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int idx0 = 0;
        float ang0 = 0.f;
        bool taken0 = false;
        int kidx0 = 0;      // the keyframe keypoint that took it, and its angle: written after the loop,
        float kang0 = 0.f;  // so that the sequential chain of the first 64 holds no memory operation
        if (lane < nf) {
            const uint4* d = reinterpret_cast<const uint4*>(fdesc + 32LL * (fs + lane));
            const uint4 x = d[0], y = d[1];
            d0[0] = x.x, d0[1] = x.y, d0[2] = x.z, d0[3] = x.w, d0[4] = y.x, d0[5] = y.y, d0[6] = y.z, d0[7] = y.w;
            idx0 = clampi(F.order[fs + lane], 0, F.n - 1);
            ang0 = *reinterpret_cast<const float*>(fkps + 28LL * idx0 + 12);
        }
        for (int i0 = ks; i0 < ke; i0 += 64) {  // :252, iKF ascending, 64 keyframe keypoints staged per lane
            uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int kidx_l = 0, flags_l = 0;
            float kang_l = 0.f;
            if (i0 + lane < ke) {
                kidx_l = clampi(K.order[i0 + lane], 0, K.n - 1);
                const BowPoint& pt = kf[kidx_l];
                flags_l = pt.flags, kang_l = pt.angle;
#pragma unroll
                for (int w = 0; w < 8; ++w) qd[w] = pt.desc[w];
            }
            // (the staged loads land here, not at their first use inside the chain)
            asm volatile("" ::"v"(qd[0]), "v"(qd[1]), "v"(qd[2]), "v"(qd[3]), "v"(qd[4]), "v"(qd[5]), "v"(qd[6]), "v"(qd[7]),
                         "v"(kang_l));
            for (uint64_t todo = __ballot(flags_l & 1); todo; todo &= todo - 1) {  // :258-262 skips the others
                const int j = __builtin_ctzll(todo);
                uint32_t q[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) q[w] = lane_value(qd[w], j);
                uint32_t k1 = kNoKey, k2 = kNoKey;  // distance << 16 | position in the segment
                if (lane < nf && !taken0) {
                    int dist = 0;
#pragma unroll
                    for (int w = 0; w < 8; ++w) dist += __popc(q[w] ^ d0[w]);
                    k1 = ((uint32_t)dist << 16) | (uint32_t)lane;
                }
                for (int c = 1; c < nch; ++c) {
                    const int pos = c * 64 + lane;
                    if (pos < nf && !((taken[c] >> lane) & 1ull)) {
                        const uint32_t key = ((uint32_t)hamming32(q, fdesc + 32LL * (fs + pos)) << 16) | (uint32_t)pos;
                        k2 = min(k2, max(k1, key));
                        k1 = min(k1, key);
                    }
                }
                // the wave's two lowest: the second is the lowest once the best's lane gives its own second
                const uint32_t low = wave_min(k1);
                k2 = wave_min(k1 == low ? k2 : k1);
                k1 = low;
                const int best1 = k1 == kNoKey ? 256 : (int)(k1 >> 16), best2 = k2 == kNoKey ? 256 : (int)(k2 >> 16);
                const bool ev = best1 <= kThLow && (float)best1 < a.nnratio * (float)best2;  // :328-330
                const int pos = (int)(k1 & 0xFFFFu);
                const int kidx = (int)lane_value((uint32_t)kidx_l, j);
                const float kang = __uint_as_float(lane_value(__float_as_uint(kang_l), j));
                if (ev && lane == (pos & 63)) {  // the lane that holds the keypoint
                    if (pos < 64) {
                        taken0 = true, kidx0 = kidx, kang0 = kang;
                    } else {
                        const int idxF = clampi(F.order[fs + pos], 0, F.n - 1);
                        taken[pos >> 6] |= 1ull << (pos & 63);
                        bow_commit(a, match, mbin, idxF, *reinterpret_cast<const float*>(fkps + 28LL * idxF + 12), kidx,
                                   kang);
                    }
                }
                if (nch > 1) __syncthreads();  // one wave: orders the taken bit before the next keypoint's reads
            }
        }
        if (taken0) bow_commit(a, match, mbin, idx0, ang0, kidx0, kang0);
    }
}

__global__ __launch_bounds__(256) void k_bow_finish(BowArgs a) { bow_finish_body(a); }

}  // namespace

hipError_t launch_bow_search(const BowArgs& a, int npairs, int max_side, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    size_t lds;
    if (const hipError_t e = bow_group_lds(k_bow_group, max_side, &lds)) return e;
    hipLaunchKernelGGL(k_bow_group, dim3(npairs, 2), dim3(kGroupThreads), lds, st, a);
    hipLaunchKernelGGL(k_bow_match, dim3(kMatchWaves, npairs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_bow_finish, dim3(npairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
