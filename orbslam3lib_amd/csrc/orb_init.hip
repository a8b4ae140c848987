// ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
// (cpp/src/ORBmatcher.cc:649-764; ComputeThreeMaxima :2061-2102; Frame::GetFeaturesInArea,
// Frame.cc:673-739), Tracking::MonocularInitialization's matcher, over pairs of batch images whose
// mvKeysUn, octaves, angles, descriptors and grid already live in HBM.
//
// Per F1 keypoint of octave 0, in index order (:662-667): the F2 keypoints of octave 0 within
// windowSize of vbPrevMatched[i1] (:669), in grid order; a candidate whose matched distance is not
// above its Hamming distance is skipped (:688-689); best and second best of the rest with strict <
// (:691-700); when best <= TH_LOW and best < second * nnratio (:703-705) the keypoint's previous
// owner is robbed (:707-711), the keypoint is taken with its distance (:712-715) and i1 enters its
// rotation bin (:717-727).  After the loop every entry of a bin outside the three maxima that is
// still matched is cleared (:733-756), and vbPrevMatched moves to the matched keypoints (:759-761).
//
// What couples the points is the matched distance of each F2 keypoint, which only falls, so the
// loop is replayed as in orb_sbp.hip / orb_track.hip:
//   k_init_compact     one workgroup per pair packs F2's octave-0 keypoints (index, mvKeysUn.pt,
//                      descriptor) in grid order, with the count of them before every entry of
//                      the grid lists.  At windowSize 100 a window spans 21 grid columns of ~14
//                      keypoints each, four fifths of them at other levels: walked on the frame's
//                      own lists that is ~290 chains of index -> octave -> position -> descriptor
//                      gathers; on the packed list it is ~58 records, contiguous per column.
//   k_init_candidates  256 F1 keypoints per workgroup.  The searched ones (octave 0, finite
//                      vbPrevMatched) are compacted in LDS -- the others cost their octave load --
//                      and numbered across workgroups by counting the searched keypoints before
//                      the block.  One lane per window walks the packed records of its 21 columns
//                      and keeps the 4 lowest distance << 16 | packed position keys (the packed
//                      order is the window order).  On the packed list 2 to 64 lanes per window
//                      measured no faster.  Against the pre-call state,
//                      i.e. without the matched-distance filter.
//   k_init_replay      one wave per pair, 64 searched keypoints at a time.  LDS holds the matched
//                      distance (0xFFFF: none), the owner and the owner's bin of every F2
//                      keypoint.  A lane's best and second best are the first two of its kept
//                      candidates whose matched distance is above their distance; with fewer than
//                      two of them and more than 4 in the window, the 4th kept distance decides
//                      where it can (best above TH_LOW; best passing the ratio test against it:
//                      every candidate not kept is at least as far) and the whole wave walks the
//                      window with the live table otherwise, a column per lane.  A lane is stale
//                      when an earlier lane of its group takes a keypoint it examined; the lanes
//                      before the first stale one commit at once -- they take distinct keypoints,
//                      so robbing an owner is overwriting its entry.  vnMatches12 is the inverse
//                      of the owner table: after the three-maxima rule, every owner whose bin
//                      survives is a match.
//
// Deviations from the reference, which reads out of range in these cases: a keypoint whose
// vbPrevMatched is not finite is skipped; an event whose bin falls outside [0, 30) counts in
// nmatches, enters no bin and cannot be rejected.  Octaves are in [0, nlevels) here (the extractor
// wrote them): "octave > 0 is skipped" and "octave 0 is searched" are the same rule.
#include <hip/hip_runtime.h>

#include "orb_kernels.h"
#include "orb_window.h"

namespace orbgpu {
namespace {

constexpr int kThLow = 50;         // ORBmatcher::TH_LOW
constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kNoDist = 0xFFFFu;  // vMatchedDistance's INT_MAX

// vbPrevMatched of the pair (the caller's, or F1's mvKeysUn.pt).
__device__ inline const float* init_prev(const InitArgs& a, int pair, const FrameView& F1) {
    return a.prev ? a.prev + 2LL * pair * a.out_cap : F1.xy;
}

__device__ inline void load_desc_row(const uint8_t* d, uint32_t q[8]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(d), hi = *reinterpret_cast<const uint4*>(d + 16);
    q[0] = lo.x, q[1] = lo.y, q[2] = lo.z, q[3] = lo.w;
    q[4] = hi.x, q[5] = hi.y, q[6] = hi.z, q[7] = hi.w;
}

// F2's packed octave-0 keypoints (k_init_compact) of one pair.
struct Level0 {
    const int32_t* pre;   // [entries of the grid lists + 1]
    const int32_t* idx;
    const float* xy;
    const uint8_t* desc;
};
__device__ inline Level0 level0_of(const InitArgs& a, int pair) {
    Level0 L;
    L.pre = a.l0_pre + (long long)pair * (a.out_cap + 1);
    L.idx = a.l0_idx + (long long)pair * a.out_cap;
    L.xy = a.l0_xy + 2LL * pair * a.out_cap;
    L.desc = a.l0_desc + 32LL * pair * a.out_cap;
    return L;
}

__global__ __launch_bounds__(256) void k_init_compact(InitArgs a) {
    __shared__ int32_t wsum[4];
    const int p = blockIdx.x, t = threadIdx.x, cap = a.out_cap;
    const FrameView F2 = frame_view_of(a, a.pairs[2 * p + 1], nullptr);
    const int total = min(max(F2.cs[kGridCols * kGridRows], 0), cap);  // keypoints inside the grid
    int32_t* pre = a.l0_pre + (long long)p * (cap + 1);
    int32_t* pidx = a.l0_idx + (long long)p * cap;
    float* pxy = a.l0_xy + 2LL * p * cap;
    uint8_t* pdesc = a.l0_desc + 32LL * p * cap;
    int base = 0;
    for (int j0 = 0; j0 < total; j0 += 256) {
        const int j = j0 + t;
        const int k = j < total ? F2.ci[j] : -1;
        const bool keep = k >= 0 && octave_of(F2, k) == 0;
        const uint64_t bal = __ballot(keep);
        if ((t & 63) == 0) wsum[t >> 6] = __popcll(bal);
        __syncthreads();
        int rank = base + __popcll(bal & ((1ull << (t & 63)) - 1));
        for (int w = 0; w < (t >> 6); ++w) rank += wsum[w];
        if (j < total) pre[j] = rank;
        if (keep) {
            pidx[rank] = k;
            *reinterpret_cast<float2*>(pxy + 2LL * rank) = *reinterpret_cast<const float2*>(F2.xy + 2LL * k);
            const uint4* d = reinterpret_cast<const uint4*>(F2.desc + 32LL * k);
            reinterpret_cast<uint4*>(pdesc + 32LL * rank)[0] = d[0];
            reinterpret_cast<uint4*>(pdesc + 32LL * rank)[1] = d[1];
        }
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (t == 0) pre[total] = base;
}

__global__ __launch_bounds__(256) void k_init_candidates(InitArgs a) {
    __shared__ int32_t list[256];
    __shared__ int32_t cnt[5];  // searched keypoints of each wave, then of the blocks before
    const int p = blockIdx.y, t = threadIdx.x, cap = a.out_cap;
    const int f1 = a.pairs[2 * p], f2 = a.pairs[2 * p + 1];
    const int n1 = min(max(a.out_n[f1], 0), cap);
    const int i0 = blockIdx.x * 256;
    if (i0 >= n1) return;
    const FrameView F1 = frame_view_of(a, f1, nullptr), F2 = frame_view_of(a, f2, nullptr);
    const Level0 L = level0_of(a, p);
    const float* prev = init_prev(a, p, F1);
    auto searched = [&](int i) {
        if (i >= n1 || octave_of(F1, i) != 0) return false;  // :665-667
        const float2 pt = *reinterpret_cast<const float2*>(prev + 2LL * i);
        return isfinite(pt.x) && isfinite(pt.y);
    };
    if (t < 5) cnt[t] = 0;
    __syncthreads();
    int before = 0;
    for (int i = t; i < i0; i += 256) before += searched(i) ? 1 : 0;
    for (int o = 32; o >= 1; o >>= 1) before += __shfl_xor(before, o);
    if ((t & 63) == 0 && before) atomicAdd(&cnt[4], before);
    const int i = i0 + t;
    const bool s = searched(i);
    const uint64_t bal = __ballot(s);
    if ((t & 63) == 0) cnt[t >> 6] = __popcll(bal);
    if (i < n1) {  // the call's initial state: no match, vbPrevMatched unchanged
        a.match12[(long long)p * cap + i] = -1;
        *reinterpret_cast<float2*>(a.prev_out + 2 * ((long long)p * cap + i)) =
            *reinterpret_cast<const float2*>(prev + 2LL * i);
    }
    __syncthreads();
    int rank = __popcll(bal & ((1ull << (t & 63)) - 1));
    for (int w = 0; w < (t >> 6); ++w) rank += cnt[w];
    if (s) list[rank] = i;
    const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3], base = cnt[4];
    if (t == 0 && i0 + 256 >= n1) a.nsearch[p] = base + total;
    __syncthreads();

    if (t >= total) return;
    const int i1 = list[t];
    const float2 pt = *reinterpret_cast<const float2*>(prev + 2LL * i1);
    uint32_t q[8];
    load_desc_row(F1.desc + 32LL * i1, q);
    uint32_t key[kInitTop];  // distance << 16 | packed position, ascending
#pragma unroll
    for (int j = 0; j < kInitTop; ++j) key[j] = kNoKey;
    InitCand c;
    c.n = 0;
    CellRange cr;
    if (window_cells(a, pt.x, pt.y, a.window, &cr)) {
        for (int ix = cr.minX; ix <= cr.maxX; ++ix) {
            const int j1 = L.pre[F2.cs[ix * kGridRows + cr.maxY + 1]];
            for (int j = L.pre[F2.cs[ix * kGridRows + cr.minY]]; j < j1; ++j) {
                const float2 p2 = *reinterpret_cast<const float2*>(L.xy + 2LL * j);
                if (!(fabsf(p2.x - pt.x) < a.window && fabsf(p2.y - pt.y) < a.window)) continue;  // Frame.cc:719-722
                ++c.n;
                uint32_t kk = ((uint32_t)hamming32(q, L.desc + 32LL * j) << 16) | (uint32_t)j;
                bool shift = false;
#pragma unroll
                for (int s4 = 0; s4 < kInitTop; ++s4) {
                    shift = shift || kk < key[s4];
                    if (shift) {
                        const uint32_t tk = key[s4];
                        key[s4] = kk;
                        kk = tk;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int s4 = 0; s4 < kInitTop; ++s4) {
        const bool kept = key[s4] != kNoKey;
        c.idx[s4] = kept ? L.idx[min((int)(key[s4] & 0xFFFFu), cap - 1)] : -1;
        c.dist[s4] = kept ? (int)(key[s4] >> 16) : 256;
    }
    c.i1 = i1;
    c.pad[0] = c.pad[1] = 0;
    a.cand[(long long)p * cap + base + t] = c;
}

// Dynamic LDS of k_init_replay for n keypoints per image: matched distance, owner, the owner's bin
// and the round's claims per F2 keypoint, then the histogram (+ the rejected set and its size).
__host__ __device__ inline int init_lds_words(int n) { return 4 * n + kRotBins + 2; }

// The window of one searched keypoint walked by the whole wave against the live matched
// distances, a grid column per lane (every lane passes the same arguments): the two lowest
// distance << 16 | packed position keys among the candidates that :688-689 lets through, to every
// lane.
__device__ inline void init_walk_wave(const InitArgs& a, const FrameView& F2, const Level0& L, float x, float y,
                                      const uint32_t q[8], const uint32_t* md, int lane, uint32_t* best,
                                      int* best_idx, uint32_t* second) {
    uint32_t k1 = kNoKey, k2 = kNoKey;
    int idx = -1;
    CellRange cr;
    if (window_cells(a, x, y, a.window, &cr)) {
        for (int ix = cr.minX + lane; ix <= cr.maxX; ix += 64) {
            const int j1 = L.pre[F2.cs[ix * kGridRows + cr.maxY + 1]];
            for (int j = L.pre[F2.cs[ix * kGridRows + cr.minY]]; j < j1; ++j) {
                const float2 p2 = *reinterpret_cast<const float2*>(L.xy + 2LL * j);
                if (!(fabsf(p2.x - x) < a.window && fabsf(p2.y - y) < a.window)) continue;
                const int k = L.idx[j];
                const uint32_t d = (uint32_t)hamming32(q, L.desc + 32LL * j);
                if (md[k] <= d) continue;
                const uint32_t kk = (d << 16) | (uint32_t)j;
                if (kk < k1) {
                    k2 = k1, k1 = kk, idx = k;
                } else if (kk < k2) {
                    k2 = kk;
                }
            }
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t o1 = __shfl_xor(k1, o), o2 = __shfl_xor(k2, o);
        const int oi = __shfl_xor(idx, o);
        const uint32_t hi = max(k1, o1);
        if (o1 < k1) k1 = o1, idx = oi;
        k2 = min(hi, min(k2, o2));
    }
    *best = k1, *best_idx = idx, *second = k2;
}

__global__ __launch_bounds__(64) void k_init_replay(InitArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int cap = a.out_cap, p = blockIdx.x, lane = threadIdx.x;
    uint32_t* md = lds;                                      // vMatchedDistance
    int32_t* own = reinterpret_cast<int32_t*>(md + cap);     // vnMatches21
    uint32_t* obin = reinterpret_cast<uint32_t*>(own + cap);  // the bin of the owner's event
    uint32_t* claim = obin + cap;                            // lowest lane taking it this round
    uint32_t* hist = claim + cap;                            // [kRotBins], the rejected set, its size
    const int f1 = a.pairs[2 * p], f2 = a.pairs[2 * p + 1];
    const int nk2 = min(max(a.out_n[f2], 0), cap);
    const int ns = min(max(a.nsearch[p], 0), cap);
    const FrameView F1 = frame_view_of(a, f1, nullptr), F2 = frame_view_of(a, f2, nullptr);
    const Level0 L = level0_of(a, p);
    const float* prev = init_prev(a, p, F1);
    const InitCand* cand = a.cand + (long long)p * cap;
    for (int k = lane; k < nk2; k += 64) md[k] = kNoDist, own[k] = -1, obin[k] = kNoBin, claim[k] = 64;
    if (lane < kRotBins + 2) hist[lane] = 0;
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1;
    const float int_max = 2147483648.0f;  // (float)INT_MAX, the second best of a lone candidate
    for (int g0 = 0; g0 < ns; g0 += 64) {
        bool pending = g0 + lane < ns;
        InitCand c{};
        if (pending) c = cand[g0 + lane];
        pending = pending && c.n > 0;  // :671-672
        while (__ballot(pending)) {
            int b = -1, bd = 256, nexam = 0;
            float second = int_max;
            bool walk = false;
            if (pending) {
                bool two = false;
#pragma unroll
                for (int t = 0; t < kInitTop; ++t) {
                    const int k = c.idx[t];
                    if (two || k < 0) break;
                    nexam = t + 1;
                    if (md[k] <= (uint32_t)c.dist[t]) continue;  // :688-689
                    if (b < 0) {
                        b = k, bd = c.dist[t];
                    } else {
                        second = (float)c.dist[t], two = true;
                    }
                }
                if (!two && c.n > kInitTop) {
                    // what was not kept is at least as far as the last kept candidate
                    const int far = c.dist[kInitTop - 1];
                    if ((b >= 0 ? bd : far) > kThLow) {
                        b = -1;  // the best is above TH_LOW
                    } else if (b >= 0 && a.nnratio >= 0.f && (float)bd < (float)far * a.nnratio) {
                        second = (float)far;  // passes against any second best from far up
                    } else {
                        walk = true;
                    }
                }
            }
            for (uint64_t wm = __ballot(walk); wm; wm &= wm - 1) {
                const int src = __builtin_ctzll(wm);
                const int i1 = __shfl(c.i1, src);
                const float2 pt = *reinterpret_cast<const float2*>(prev + 2LL * i1);
                uint32_t q[8];
                load_desc_row(F1.desc + 32LL * i1, q);
                uint32_t k1, k2;
                int wi;
                init_walk_wave(a, F2, L, pt.x, pt.y, q, md, lane, &k1, &wi, &k2);
                if (lane == src) {
                    b = wi, bd = wi >= 0 ? (int)(k1 >> 16) : 256;
                    second = k2 != kNoKey ? (float)(k2 >> 16) : int_max;
                }
            }
            const bool ev = pending && b >= 0 && bd <= kThLow && (float)bd < second * a.nnratio;  // :703-705
            // staleness against the earlier pending lanes of the group: an event lowers the
            // matched distance of its keypoint for every later point that examines it
            const uint64_t am = __ballot(ev);
            if (ev) atomicMin(&claim[b], (uint32_t)lane);
            __syncthreads();
            bool stale = false;
            if (pending) {
                stale = walk && (am & below) != 0;
#pragma unroll
                for (int t = 0; t < kInitTop; ++t)
                    if (t < nexam) stale |= claim[c.idx[t]] < (uint32_t)lane;
            }
            __syncthreads();
            if (ev) claim[b] = 64;
            const uint64_t st = __ballot(pending && stale);
            const int first = st ? __builtin_ctzll(st) : 64;
            const bool commit = pending && lane < first;
            if (commit && ev) {  // :707-727; the lanes of one commit take distinct keypoints
                own[b] = c.i1;
                md[b] = (uint32_t)bd;
                uint32_t bin = kNoBin;
                if (a.check_orientation) {
                    if (rot_bin(angle_of(F1, c.i1), angle_of(F2, b), &bin)) atomicAdd(&hist[bin], 1u);
                }
                obin[b] = bin;
            }
            pending = pending && !commit;
            __syncthreads();
        }
    }
    if (a.check_orientation) {
        if (lane == 0) three_maxima_reject(hist);
        __syncthreads();
    }
    // vnMatches12 = the owners whose bin survives (:741-761)
    const uint32_t rej = hist[kRotBins];
    int nmatches = 0;
    for (int k = lane; k < nk2; k += 64) {
        const int o = own[k];
        if (o < 0 || ((rej >> obin[k]) & 1u)) continue;
        a.match12[(long long)p * cap + o] = k;
        *reinterpret_cast<float2*>(a.prev_out + 2 * ((long long)p * cap + o)) =
            *reinterpret_cast<const float2*>(F2.xy + 2LL * k);
        ++nmatches;
    }
    for (int o = 32; o >= 1; o >>= 1) nmatches += __shfl_xor(nmatches, o);
    if (lane < kRotBins) a.rot_hist[p * kRotBins + lane] = (int32_t)hist[lane];
    if (lane == 0) a.nmatches[p] = nmatches;
}

}  // namespace

size_t init_replay_lds_bytes(int out_cap) { return 4 * (size_t)init_lds_words(out_cap); }

hipError_t launch_init_search(const InitArgs& a, int npairs, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_compact, dim3(npairs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_init_candidates, dim3((a.out_cap + 255) / 256, npairs), dim3(256), 0, st, a);
    const size_t lds = init_replay_lds_bytes(a.out_cap);
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_init_replay),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_init_replay, dim3(npairs), dim3(64), lds, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
