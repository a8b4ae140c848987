// orb_bow_group.h -- what the searches over vocabulary nodes share (orb_bow.hip: SearchByBoW(KeyFrame,
// Frame), orb_tri.hip: SearchForTriangulation, orb_bowkf.hip: SearchByBoW(KeyFrame, KeyFrame)): a pair's
// two sides ordered by (node, index) with their node segment tables, the segment lookup, the wave-wide
// minimum, and the rotation-histogram finish.  Args is the search's argument struct (BowArgs / TriArgs /
// BowKfArgs, orb_kernels.h): the bodies read the fields all declare under the same names.
#pragma once
#include <hip/hip_runtime.h>

#include "orb_kernels.h"
#include "orb_window.h"

namespace orbgpu {
namespace {

constexpr int kThLow = 50;  // ORBmatcher::TH_LOW
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint64_t kNoNode = ~0ull;  // sorts behind every node id
constexpr int kGroupThreads = 1024;

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// The ordered lists of one (pair, side).
struct BowSide {
    int32_t* order;      // keypoint indices by (node, index)
    int32_t* seg_node;   // node of segment s
    int32_t* seg_start;  // [segments + 1] into order
    int n;               // keypoints of the side
};
template <class Args>
__device__ inline BowSide bow_kf_side(const Args& a, int p) {
    const int o0 = a.kf_off[p];
    BowSide s;
    s.order = a.kf_order + o0;
    s.seg_node = a.kf_seg_node + o0;
    s.seg_start = a.kf_seg_start + o0 + p;
    s.n = clampi(a.kf_off[p + 1] - o0, 0, kBowMaxPoints);
    return s;
}
template <class Args>
__device__ inline BowSide bow_f_side(const Args& a, int p) {
    BowSide s;
    s.order = a.f_order + (long long)p * a.out_cap;
    s.seg_node = a.f_seg_node + (long long)p * a.out_cap;
    s.seg_start = a.f_seg_start + (long long)p * (a.out_cap + 1);
    s.n = clampi(a.out_n[a.frames[p]], 0, min(a.out_cap, kBowMaxPoints));
    return s;
}

// One workgroup of kGroupThreads per (pair, side): blockIdx.x = pair, blockIdx.y = side (0: the host's
// keyframe points, 1: the batch image).  keys: the launch's dynamic LDS, [npad] 64-bit keys.
// pack_kf(keys, m, n) runs on side 0 after the sort, keys[0 .. m) being the side's (node << 32 | index)
// in order.
template <class Args, class PackKf>
__device__ inline void bow_group_body(const Args& a, uint64_t* keys, PackKf pack_kf) {
    __shared__ int32_t wsum[kGroupThreads / 64];
    __shared__ int32_t nvalid;
    const int p = blockIdx.x, side = blockIdx.y, t = threadIdx.x, cap = a.out_cap;
    const BowSide S = side == 0 ? bow_kf_side(a, p) : bow_f_side(a, p);
    const int n = S.n;
    const auto* kf = a.kf_pts + a.kf_off[p];
    const int32_t* fnode = a.f_nodes + (long long)p * cap;
    int npad = 1;
    while (npad < n) npad <<= 1;  // <= kBowMaxPoints: the launch sized keys[] for it
    if (t == 0) nvalid = 0;
    __syncthreads();
    int mine = 0;
    for (int j = t; j < npad; j += kGroupThreads) {
        const int node = j < n ? (side == 0 ? kf[j].node : fnode[j]) : -1;
        keys[j] = node < 0 ? kNoNode : (((uint64_t)(uint32_t)node << 32) | (uint32_t)j);
        mine += node >= 0 ? 1 : 0;
    }
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & 63) == 0 && mine) atomicAdd(&nvalid, mine);
    __syncthreads();
    // bitonic sort, ascending: the keys are distinct but for the padding, which ends up last
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = t; q < (npad >> 1); q += kGroupThreads) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const uint64_t x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) keys[i] = y, keys[l] = x;
            }
            __syncthreads();
        }
    }
    const int m = min(nvalid, n);
    if (side == 1) {  // the call's initial state (:228) and the descriptors in node order
        int32_t* match = a.match + (long long)p * cap;
        for (int k = t; k < n; k += kGroupThreads) match[k] = -1;
        const uint8_t* desc = a.desc + 32LL * a.frames[p] * cap;
        uint4* packed = reinterpret_cast<uint4*>(a.f_desc + 32LL * p * cap);
        for (int j = t; j < 2 * m; j += kGroupThreads) {
            const int k = min((int)(uint32_t)keys[j >> 1], n - 1);
            packed[j] = reinterpret_cast<const uint4*>(desc + 32LL * k)[j & 1];
        }
    } else {
        pack_kf(keys, m, n);
    }
    int nseg = 0;
    for (int j0 = 0; j0 < m; j0 += kGroupThreads) {
        const int j = j0 + t;
        const bool valid = j < m;
        const uint32_t node = valid ? (uint32_t)(keys[j] >> 32) : 0u;
        const bool head = valid && (j == 0 || (uint32_t)(keys[j - 1] >> 32) != node);
        const uint64_t bal = __ballot(head);
        if ((t & 63) == 0) wsum[t >> 6] = __popcll(bal);
        __syncthreads();
        int rank = nseg + __popcll(bal & ((1ull << (t & 63)) - 1));
        for (int w = 0; w < kGroupThreads / 64; ++w) {
            rank += w < (t >> 6) ? wsum[w] : 0;
            nseg += wsum[w];
        }
        if (valid) S.order[j] = min((int)(uint32_t)keys[j], n - 1);
        if (head) S.seg_node[rank] = (int32_t)node, S.seg_start[rank] = j;
        __syncthreads();
    }
    if (t == 0) {
        S.seg_start[nseg] = m;  // nseg <= m <= n: within the side's n + 1 entries
        a.nseg[2 * p + side] = nseg;
    }
}

// Dynamic LDS of a bow_group_body launch whose largest side holds max_side keypoints (<= kBowMaxPoints:
// at most 64 KiB, beside the static arrays); raises the kernel's limit where that needs it.
template <class Kernel>
inline hipError_t bow_group_lds(Kernel kernel, int max_side, size_t* lds) {
    int npad = 1;
    while (npad < max_side) npad <<= 1;
    *lds = 8 * (size_t)npad;
    if (*lds + 256 > 65536)
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)*lds);
    return hipSuccess;
}

// The segment of `node` among a side's nseg segments (seg_node ascending), by the whole wave as in
// k_bow_match: halve while the first node >= it lies in [lo, hi], then one probe per lane.  -1: the side
// has no such node.
__device__ inline int find_segment(const int32_t* seg_node, int nseg, int node, int lane) {
    int lo = 0, hi = nseg;
    while (hi - lo > 63) {
        const int mid = (lo + hi) >> 1;
        if (seg_node[mid] < node) lo = mid + 1; else hi = mid;
    }
    const uint64_t hit = __ballot(lo + lane <= hi && lo + lane < nseg && seg_node[lo + lane] == node);
    return hit ? lo + __builtin_ctzll(hit) : -1;
}

// Lane j's value of a wave-uniform j.
__device__ inline uint32_t lane_value(uint32_t v, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); }

// The wave's lowest value, to every lane; all 64 lanes must be active.  Within a row of 16 by DPP (lane
// ^ 1, lane ^ 2, mirror of 8, mirror of 16), then the four rows.
template <int kCtrl>
__device__ inline uint32_t dpp_min(uint32_t v) {
    return min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, kCtrl, 0xF, 0xF, false));
}
__device__ inline uint32_t wave_min(uint32_t v) {
    v = dpp_min<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_min<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_min<0x141>(v);  // row_half_mirror
    v = dpp_min<0x140>(v);  // row_mirror
    return min(min(lane_value(v, 0), lane_value(v, 16)), min(lane_value(v, 32), lane_value(v, 48)));
}

// One workgroup of 256 per pair, after the match kernel left match [pair][out_cap] and, beside each
// match, the bin of the event that wrote it: the 30 bin sizes are counted from the stored bins (LDS
// integer atomics: order-independent), then three_maxima_reject, the matches whose bin is rejected
// are cleared, nmatches is what is left.  A row entry is written by at most one event.  (orb_bowkf.hip has
// a finish of its own, which also codes the cleared entries: a hook here changed k_bow_finish's and
// k_tri_finish's instruction order.)
template <class Args>
__device__ inline void bow_finish_body(const Args& a) {
    __shared__ uint32_t hist[kRotBins + 2];  // the bins, the rejected set, its size
    __shared__ int32_t wcnt[4];
    const int p = blockIdx.x, t = threadIdx.x, cap = a.out_cap;
    const int n = clampi(a.out_n[a.frames[p]], 0, min(cap, kBowMaxPoints));
    int32_t* match = a.match + (long long)p * cap;
    const uint8_t* mbin = a.match_bin + (long long)p * cap;
    if (t < kRotBins + 2) hist[t] = 0;
    __syncthreads();
    for (int k = t; k < n; k += 256)  // a keypoint is taken at most once: the bin sizes are those of the matches
        if (match[k] >= 0 && mbin[k] < kRotBins) atomicAdd(&hist[mbin[k]], 1u);
    __syncthreads();
    if (t < kRotBins) a.rot_hist[p * kRotBins + t] = (int32_t)hist[t];
    if (a.check_orientation && t == 0) three_maxima_reject(hist);  // :405-423
    __syncthreads();
    const uint32_t rej = hist[kRotBins];
    int nm = 0;
    for (int k = t; k < n; k += 256) {
        if (match[k] < 0) continue;
        if ((rej >> (mbin[k] & 31)) & 1u) match[k] = -1; else ++nm;
    }
    for (int o = 32; o >= 1; o >>= 1) nm += __shfl_xor(nm, o);
    if ((t & 63) == 0) wcnt[t >> 6] = nm;
    __syncthreads();
    if (t == 0) a.nmatches[p] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

}  // namespace
}  // namespace orbgpu
