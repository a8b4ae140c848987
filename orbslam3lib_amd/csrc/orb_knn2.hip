// cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) between descriptor sets in HBM (Frame.cc:45,
// 1224-1250: the left / right match of a stereo pair), on the FP4 matrix cores:
//   k_knn2_mfma_pairs  the pairs of a batch, 256 queries per workgroup; launches of few pairs split
//                      the train rows over several workgroups, the last to arrive merging
//   k_knn2_merge       that merge as its own launch, where the arrival counters are not bound
//   k_knn2_mfma_plain  one query set against one train set (orb_post.cpp)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "orb_kernels.h"

namespace orbgpu {

__device__ inline uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
    return max(min(a, b), min(max(a, b), c));  // lowers to v_med3_u32
}

__device__ inline void knn2_store(uint32_t k1, uint32_t k2, int qi, int32_t* i1, int32_t* d1,
                                  int32_t* i2, int32_t* d2) {
    i1[qi] = k1 == 0xFFFFFFFFu ? -1 : (int32_t)(k1 & 0xFFFF);
    d1[qi] = k1 == 0xFFFFFFFFu ? 0x7fffffff : (int32_t)(k1 >> 16);
    i2[qi] = k2 == 0xFFFFFFFFu ? -1 : (int32_t)(k2 & 0xFFFF);
    d2[qi] = k2 == 0xFFFFFFFFu ? 0x7fffffff : (int32_t)(k2 >> 16);
}

// ---------------------------------------------------------------------------------------------
// k_knn2_mfma: BFMatcher(NORM_HAMMING).knnMatch(k=2) on the block-scaled FP4 matrix cores.
// Every descriptor bit becomes one e2m1 element, +1 (0x2) for a clear bit and -1 (0xA) for a set
// one, on both operands; with an E8M0 scale of 2^6 per 32-element block on each side,
// v_mfma_scale_f32_32x32x64_f8f6f4 gives 4096 * (64 - 2 H) over its K = 64 bits, so a train tile
// of 32 rows against 32 queries is 4 MFMAs over the 256 bits, at twice the MACs per cycle of the
// i8 form (MI355X_MICROARCH.md: FP4 32x32x64 takes the cycles of BF16 32x32x16).  The f32
// accumulator is preloaded with 4095 - (t mod 4096), so acc = 4096 (256 - 2H) + 4095 - t_local
// (every value an integer below 2^24, exact) orders like (H, t) ascending and the best two train
// rows are the two largest accumulators: no popcount, no per-pair VALU beyond the top-2 update.
// Train rows are walked in 4096-row segments (12-bit local index); each segment's winners are
// folded into (H << 16 | t) keys.
//   workgroup = 8 waves x 32 queries; per 32-row train tile each wave issues 4 MFMAs: A = the
//   train tile (expanded once per workgroup into LDS, double-buffered), B = the wave's queries
//   (expanded once into registers).
// C/D layout (cdna_hip_programming.md §3): lane l holds column l & 31 (its query) and rows
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of the tile (train rows); the K order inside a fragment is
// the same map for A and B, so any consistent bit -> element assignment is exact.
// Measured and replaced (round 6, single stream, 512 images): the i8 form
// (v_mfma_i32_32x32x32_i8, bits as +-64 bytes, 8 MFMAs per tile) 230-238 us against 159-167 us;
// two query sets per wave on the i8 form (each LDS-read train fragment feeding two MFMAs; 186
// VGPRs, 2 waves per SIMD) 256 us, and with one accumulator set selected after its own tile 237 us.
// Round 2's FP4 attempt lost to its nibble expansion; here a dword expands to its 32 nibbles with
// one shift and one v_and_or_b32 per 8 nibbles.
typedef int knn_v8i __attribute__((ext_vector_type(8)));
typedef float knn_v16f __attribute__((ext_vector_type(16)));
constexpr int kKnnWaves = 8;
constexpr int kKnnThreads = 64 * kKnnWaves;
constexpr int kKnnQ = 32 * kKnnWaves;    // queries per workgroup
static_assert(kKnnQ == kKnnQueries, "orb_kernels.h kKnnQueries (grid and arrival counters)");
constexpr int kKnnSeg = 4096;            // train rows per key segment
constexpr int kKnnPitch4 = 144;          // bytes per expanded train row (128 + 16: conflict-free b128 reads)
// bit 3 of each nibble from ws, nibble = 0x2 (+1) or 0xA (-1): one v_and_or_b32
__device__ inline uint32_t knn_nib_of(uint32_t ws) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(ws), "v"(0x88888888u), "v"(0x22222222u));
    return r;
}
// 8 nibbles of output dword m (m = 0..3) = bits m, m + 4, .., m + 28 of w, each +1 (0x2) or -1 (0xA)
__device__ inline knn_v8i knn4_expand(uint32_t w) {
    knn_v8i v;
    v[0] = (int)knn_nib_of(w << 3);
    v[1] = (int)knn_nib_of(w << 2);
    v[2] = (int)knn_nib_of(w << 1);
    v[3] = (int)knn_nib_of(w);
    v[4] = v[5] = v[6] = v[7] = 0;  // the e2m1 form reads four registers
    return v;
}
__device__ inline float knn_med3_f32(float a, float b, float c) {
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ inline float knn_max3_f32(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __attribute__((always_inline)) inline void knn2_fp4_block(
    const uint8_t* q, int nq, const uint8_t* t, int nt, int qb, int ts, int te, int32_t* i1, int32_t* d1,
    int32_t* i2, int32_t* d2, uint2* part, uint8_t* lds) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int qi = qb * kKnnQ + wave * 32 + r;
    // B fragments: lane (r, h) of MFMA s holds bits 64 s + 32 h + [0, 32) = dword 2 s + h of query qi
    knn_v8i qf[4];
    {
        const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)min(qi, max(nq - 1, 0)) * 32);
        const uint4 qa = qp[0], qc = qp[1];
        qf[0] = knn4_expand(h ? qa.y : qa.x);
        qf[1] = knn4_expand(h ? qa.w : qa.z);
        qf[2] = knn4_expand(h ? qc.y : qc.x);
        qf[3] = knn4_expand(h ? qc.w : qc.z);
    }
    uint32_t g1 = 0xFFFFFFFFu, g2 = 0xFFFFFFFFu;
    // expansion: threads < 256 take (row tid >> 3, dword tid & 7) of a tile, one 16-byte store
    // (8 lanes write 128 contiguous bytes)
    const int er = tid >> 3, ed = tid & 7;
    const bool expander = tid < 256;
    auto load_packed = [&](int tile) __attribute__((always_inline)) {
        const int row = min(tile * 32 + er, nt - 1);
        return expander ? *reinterpret_cast<const uint32_t*>(t + (long long)row * 32 + 4 * ed) : 0u;
    };
    auto tile_lds = [&](int u) __attribute__((always_inline)) { return lds + ((u - ts) & 1) * (32 * kKnnPitch4); };
    auto store_expanded = [&](int u, uint32_t w) __attribute__((always_inline)) {
        if (expander) {
            const knn_v8i v = knn4_expand(w);
            *reinterpret_cast<uint4*>(tile_lds(u) + er * kKnnPitch4 + 16 * ed) = make_uint4(v[0], v[1], v[2], v[3]);
        }
    };
    uint32_t pk0 = 0, pk1 = 0;
    if (te > ts) {
        store_expanded(ts, load_packed(ts));
        pk1 = load_packed(ts + 1);  // ts is even
    }
    auto rowc = [](int g) { return (g & 3) + 8 * (g >> 2); };
    knn_v16f C0;
#pragma unroll
    for (int g = 0; g < 16; ++g) C0[g] = (float)(4095 - 4 * h - rowc(g));
    const float kNone = -1073741824.0f;  // -2^30: below every key, and stays below after +32 per tile
    for (int seg0 = (ts * 32 / kKnnSeg) * kKnnSeg; seg0 < te * 32; seg0 += kKnnSeg) {
        const int tile0 = max(seg0 >> 5, ts), tile1 = min(te, (seg0 + kKnnSeg) >> 5);
        float ka1 = kNone, ka2 = kNone, kb1 = kNone, kb2 = kNone;
        auto select = [&](const knn_v16f& v, bool shift) __attribute__((always_inline)) {
            if (shift) {
                ka1 += 32.f;
                ka2 += 32.f;
                kb1 += 32.f;
                kb2 += 32.f;
            }
#pragma unroll
            for (int g = 0; g < 16; g += 4) {
                const float x0 = v[g], y0 = v[g + 1], x1 = v[g + 2], y1 = v[g + 3];
                ka2 = fmaxf(ka2, knn_med3_f32(ka1, x0, y0));
                ka1 = knn_max3_f32(ka1, x0, y0);
                kb2 = fmaxf(kb2, knn_med3_f32(kb1, x1, y1));
                kb1 = knn_max3_f32(kb1, x1, y1);
            }
        };
        auto body = [&](int ti, auto par, knn_v16f& acc, const knn_v16f& prev) __attribute__((always_inline)) {
            constexpr int PAR = decltype(par)::value;
            uint32_t& pk_use = PAR ? pk0 : pk1;
            uint32_t& pk_load = PAR ? pk1 : pk0;
            __syncthreads();  // tile ti expanded; the other buffer is free
            pk_load = load_packed(ti + 2);
            const uint8_t* ab = tile_lds(ti) + r * kKnnPitch4 + 16 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint4 a4 = *reinterpret_cast<const uint4*>(ab + 32 * s);
                const knn_v8i a = {(int)a4.x, (int)a4.y, (int)a4.z, (int)a4.w, 0, 0, 0, 0};
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, qf[s], s ? acc : C0, 4, 4, 0, 133, 0, 133);
            }
            if (ti > tile0) select(prev, ti - 1 > tile0);
            if (ti + 1 < te) store_expanded(ti + 1, pk_use);
            if (ti * 32 + 32 > nt) {  // partial last tile: padding rows never win
#pragma unroll
                for (int g = 0; g < 16; ++g)
                    if (ti * 32 + rowc(g) + 4 * h >= nt) acc[g] = kNone;
            }
        };
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        knn_v16f acc0, acc1;
        int ti = tile0;
        for (; ti + 1 < tile1; ti += 2) {
            body(ti, P0{}, acc0, acc1);
            body(ti + 1, P1{}, acc1, acc0);
        }
        if (ti < tile1) {
            body(ti, P0{}, acc0, acc1);
            select(acc0, ti > tile0);
        } else if (tile1 > tile0) {
            select(acc1, tile1 - 1 > tile0);
        }
        const int unbias = 32 * (tile1 - 1 - tile0);
        const int k1 = (int)fmaxf(ka1, kb1) - unbias;
        const int k2 = (int)fmaxf(fminf(ka1, kb1), fmaxf(ka2, kb2)) - unbias;
        auto fold = [&](int k) __attribute__((always_inline)) {
            if (k < -(1 << 24)) return;  // padding rows only
            const int tl = 4095 - (k & 4095), dotp = k >> 12;
            const uint32_t key = ((uint32_t)((256 - dotp) >> 1) << 16) | (uint32_t)(32 * tile0 + tl);
            g2 = med3_u32(g1, g2, key);
            g1 = min(g1, key);
        };
        fold(k1);
        fold(k2);
    }
    const uint32_t o1 = __shfl_xor(g1, 32), o2 = __shfl_xor(g2, 32);
    g2 = med3_u32(g1, g2, o1);
    g1 = min(g1, o1);
    g2 = med3_u32(g1, g2, o2);
    g1 = min(g1, o2);
    if (h == 0 && qi < nq) {
        if (part) part[qi] = make_uint2(g1, g2);
        else knn2_store(g1, g2, qi, i1, d1, i2, d2);
    }
}
constexpr int kKnnLdsBytes = 2 * 32 * kKnnPitch4;  // two expanded train tiles

__global__ __launch_bounds__(kKnnThreads) void k_knn2_mfma_pairs(MatchArgs m) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kKnnLdsBytes];
    const int pair = m.pair0 + blockIdx.y;
    const int qimg = 2 * pair, timg = 2 * pair + 1;
    const int qn = m.out_n[qimg], tn = m.out_n[timg];
    const int q0 = m.stereo_only ? m.out_mono[qimg] : 0;
    const int tq0 = m.stereo_only ? m.out_mono[timg] : 0;
    const int nq = qn > q0 ? qn - q0 : 0, nt = tn > tq0 ? tn - tq0 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) m.nq[pair] = nq;
    if ((int)blockIdx.x * kKnnQ >= nq) return;
    const uint8_t* q = m.desc + ((long long)qimg * m.out_cap + q0) * 32;
    const uint8_t* t = m.desc + ((long long)timg * m.out_cap + tq0) * 32;
    const long long o = (long long)pair * m.out_cap;
    // train split blockIdx.z of gridDim.z: tile ranges on 2-tile boundaries
    const int npt = (((nt + 31) >> 5) + 1) >> 1, S = gridDim.z, sp = blockIdx.z;  // tile pairs
    const int ts = 2 * (npt * sp / S), te = min((nt + 31) >> 5, 2 * (npt * (sp + 1) / S));
    uint2* part = m.part ? m.part + ((long long)(blockIdx.y * S + sp)) * m.out_cap : nullptr;
    knn2_fp4_block(q, nq, t, nt, blockIdx.x, ts, te, m.idx1 + o, m.dist1 + o, m.idx2 + o, m.dist2 + o, part, lds);
    if (!part || !m.cnt || S == 1) return;
    // fused merge: the last of the S split workgroups of this query block merges their partial
    // top-2 lists (k_knn2_merge's work, without its launch).  The hand-off follows
    // cdna_hip_programming.md Guideline 16 (counter form): every wave drains its partial stores,
    // one lane releases at agent scope (other XCDs' L2s), waits, and takes a ticket; the last
    // arriver resets the counter (zeroed when allocated) and acquires before any wave reads the
    // other splits' partials.  The "last" verdict goes through the kernel's one LDS array (a second
    // __shared__ object can add vmcnt waits to the tile loop).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* s_last = reinterpret_cast<int*>(lds);  // every wave is past its last tile read
    if (threadIdx.x == 0) {
        uint32_t* c = m.cnt + blockIdx.y * gridDim.x + blockIdx.x;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool last = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)(S - 1);
        if (last) {
            __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *s_last = last ? 1 : 0;
    }
    __syncthreads();
    if (!*s_last) return;
    const long long pb = (long long)blockIdx.y * S * m.out_cap;
    for (int i = threadIdx.x; i < kKnnQ; i += kKnnThreads) {
        const int qi = blockIdx.x * kKnnQ + i;
        if (qi >= nq) break;
        uint32_t g1 = 0xFFFFFFFFu, g2 = 0xFFFFFFFFu;
        for (int k = 0; k < S; ++k) {
            const uint2 kk = m.part[pb + (long long)k * m.out_cap + qi];
            g2 = med3_u32(g1, g2, kk.x);
            g1 = min(g1, kk.x);
            g2 = med3_u32(g1, g2, kk.y);
            g1 = min(g1, kk.y);
        }
        knn2_store(g1, g2, qi, m.idx1 + o, m.dist1 + o, m.idx2 + o, m.dist2 + o);
    }
}

// The split launch's partial top-2 lists of one query, merged (keys are distinct train rows).
__global__ __launch_bounds__(256) void k_knn2_merge(MatchArgs m, int nsplit) {
    const int pair = m.pair0 + blockIdx.y;
    const int qimg = 2 * pair, timg = 2 * pair + 1;
    const int qn = m.out_n[qimg], tn = m.out_n[timg];
    const int q0 = m.stereo_only ? m.out_mono[qimg] : 0;
    const int nq = qn > q0 ? qn - q0 : 0;
    (void)tn;
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    uint32_t g1 = 0xFFFFFFFFu, g2 = 0xFFFFFFFFu;
    for (int sp = 0; sp < nsplit; ++sp) {
        const uint2 k = m.part[((long long)(blockIdx.y * nsplit + sp)) * m.out_cap + qi];
        g2 = med3_u32(g1, g2, k.x);
        g1 = min(g1, k.x);
        g2 = med3_u32(g1, g2, k.y);
        g1 = min(g1, k.y);
    }
    const long long o = (long long)pair * m.out_cap;
    knn2_store(g1, g2, qi, m.idx1 + o, m.dist1 + o, m.idx2 + o, m.dist2 + o);
}

__global__ __launch_bounds__(kKnnThreads) void k_knn2_mfma_plain(const uint8_t* q, int nq, const uint8_t* t, int nt,
                                                         int32_t* i1, int32_t* d1, int32_t* i2, int32_t* d2) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kKnnLdsBytes];
    knn2_fp4_block(q, nq, t, nt, blockIdx.x, 0, (nt + 31) >> 5, i1, d1, i2, d2, nullptr, lds);
}

hipError_t launch_knn2_pairs(const MatchArgs& m, int npairs, hipStream_t s) {
    // few pairs (the latency shape): the train rows split over S workgroups per query block, so
    // the launch has ~256 workgroups instead of 8 per pair, and k_knn2_merge combines the splits
    const int S = m.part ? std::max(1, std::min(kKnnMaxSplit, kKnnSplitSlots / std::max(npairs, 1))) : 1;
    const int qblocks = (m.out_cap + kKnnQ - 1) / kKnnQ;
    if (S > 1) {
        // the partial lists take npairs * S slots of out_cap rows, the fused merge one arrival
        // counter per (pair, query block): refuse a launch that would index past either
        if (npairs * S > kKnnSplitSlots || (m.cnt && (long long)npairs * qblocks > m.cnt_slots))
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_knn2_mfma_pairs, dim3(qblocks, npairs, S), dim3(kKnnThreads), 0, s, m);
        if (!m.cnt) hipLaunchKernelGGL(k_knn2_merge, dim3((m.out_cap + 255) / 256, npairs), dim3(256), 0, s, m, S);
        return hipGetLastError();
    }
    MatchArgs m1 = m;
    m1.part = nullptr;
    hipLaunchKernelGGL(k_knn2_mfma_pairs, dim3(qblocks, npairs), dim3(kKnnThreads), 0, s, m1);
    return hipGetLastError();
}
hipError_t launch_knn2_plain(const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* i1,
                             int32_t* d1, int32_t* i2, int32_t* d2, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(k_knn2_mfma_plain, dim3((nq + kKnnQ - 1) / kKnnQ), dim3(kKnnThreads), 0, s, q, nq, t, nt, i1,
                       d1, i2, d2);
    return hipGetLastError();
}

}  // namespace orbgpu
