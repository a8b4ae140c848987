// ORBextractor::DistributeOctTree (ORBextractor_old.cc:557-781) per (image, level) of a batch; the
// algorithm itself is orb_octree.h (shared with the host harness).
//   k_octree<NT>    one NT-thread workgroup per (image, level), node state in dynamic LDS: the
//                   leading levels at 512 threads, the short ones at 256 or 128 with a smaller layout
//   k_octree_retry  the levels that did not fit that LDS layout, redone with generic pointers
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "orb_kernels.h"
#include "orb_octree.h"
#include "orb_policy.h"

namespace orbgpu {

// ---------------------------------------------------------------------------------------------
// k_octree: one workgroup per (level, image).  Gathers the level's cell lists in cell order
// (vToDistributeKeys, :807-871) then runs DistributeOctTree (orb_octree.h) with the node
// state in LDS (80 KB: two workgroups per CU).
// kOctRetry: the level did not fit the LDS instantiation (node capacity, cell offsets or more
// than kOctLdsKeys candidates); k_octree_retry then redoes it with generic pointers.
constexpr int kOctRetry = -7;

template <bool kLdsPath>
__device__ __attribute__((always_inline)) inline void octree_level(const BatchArgs& a, int img, int l,
                                                                   uint8_t* nodemem_lds, int* scratch,
                                                                   OctShared& sh, const OctCfg q) {
    const LevelGeom G = a.lv[l];
    DevPolicy p{scratch};
    const int32_t* cnt = a.cellcnt + (long long)img * a.cellcnt_img_stride + G.cellcnt_off;
    const uint32_t* ck = a.cellkeys + (long long)img * a.cellkeys_img_stride + G.cellkey_off;
    uint8_t* ws = a.octws + (long long)img * a.octws_img_stride + G.oct_off;
    const OctLayout L = oct_layout(G.cand_cap, G.oct_cap);
    uint32_t* keys = reinterpret_cast<uint32_t*>(ws + L.keys);
    void* nm = G.oct_cap <= q.lds_nodes ? (void*)nodemem_lds : (void*)(ws + L.nodemem);
    // exclusive scan of the cell counts into LDS (the node area is free until the octree's
    // gather has read it)
    int32_t* cell_off = reinterpret_cast<int32_t*>(nodemem_lds);
    const bool off_in_lds = G.ncells <= q.nq_off / 4;
    if (!off_in_lds) cell_off = reinterpret_cast<int32_t*>(ws + L.nq);  // huge levels only
    auto scan_cells = [&]() {
        int carry = 0;
        for (int base = 0; base < G.ncells; base += blockDim.x) {
            const int i = base + threadIdx.x;
            const int v = i < G.ncells ? cnt[i] : 0;
            int tot;
            const int ex = p.scan_excl(v, &tot);
            if (i < G.ncells) cell_off[i] = carry + ex;
            carry += tot;
        }
        __syncthreads();
        return carry;
    };
    const int n = scan_cells();
    uint32_t* out_keys = a.lvlkey + (long long)img * a.lvlkp_img_stride + G.kp_off;
    unsigned long long* dbg = a.octdbg ? a.octdbg + ((long long)img * kMaxLevels + l) * 8 : nullptr;
    int r = n > G.cand_cap ? -3 : 0;
    // node state and cell offsets in LDS; the per-key labels too up to q.lds_keys keys, in the
    // global workspace above that (dense levels of large frames: the label passes are parallel
    // and streaming, the serial node phases stay in LDS)
    const bool nodes_fit = off_in_lds && G.oct_cap <= q.lds_nodes && !a.oct_force_retry;
    // the count pyramid takes the LDS the level's node state and cell offsets leave (orb_octree.h)
    const int pyr_off = (int)((max(oct_nodemem_bytes(G.oct_cap), (size_t)(4 * G.ncells)) + 15) & ~(size_t)15);
    // (the pyramid names keys by cell * cell_cap + slot in 24 bits)
    const int pyrD = kLdsPath && q.lds_bytes > pyr_off && (long long)G.ncells * G.cell_cap < (1 << 24)
                         ? oct_pyr_depth((size_t)(q.lds_bytes - pyr_off), G.W, G.H, a.oct_pyr_max)
                         : 0;
    uint16_t* xtbl = reinterpret_cast<uint16_t*>(nodemem_lds + pyr_off + oct_pyr_bytes(pyrD, oct_nini(G.W, G.H)));
    if (kLdsPath && r == 0 && !nodes_fit) r = kOctRetry;
    if (kLdsPath && r == 0 && n > q.lds_keys) {
        OctWST<kLdsAS, kGlobalAS, kGlobalAS> w;
        w.keys = (asp<kGlobalAS, uint32_t>)keys;
        w.n = n;
        w.nq = (asp<kGlobalAS, uint16_t>)(ws + L.nq);
        w.m = oct_nodemem_carve<kLdsAS>(nodemem_lds, G.oct_cap);
        w.cap = G.oct_cap;
        w.out_keys = (asp<kGlobalAS, uint32_t>)out_keys;
        w.out_cap = G.kp_cap;
        w.dbg = dbg;
        w.cell_off = (asp<kLdsAS, const int32_t>)cell_off;
        w.cellkeys = (asp<kGlobalAS, const uint32_t>)ck;
        w.ncells = G.ncells;
        w.cell_cap = G.cell_cap;
        w.pyr = (asp<kLdsAS, uint32_t>)(nodemem_lds + pyr_off);
        w.pyrD = pyrD;
        w.rounds = a.oct_rounds;
        w.xcode = (asp<kLdsAS, uint16_t>)xtbl;
        w.ycode = (asp<kLdsAS, uint16_t>)(xtbl + G.W + 1);
        r = octree_distribute(p, w, (asp<kLdsAS, OctShared>)&sh, G.W, G.H, G.N);
        if (r == kOctDeep) {  // deeper than the pyramid: the label passes from the start
            __syncthreads();
            scan_cells();  // the node state overwrote the cell offsets
            w.pyrD = 0;
            r = octree_distribute(p, w, (asp<kLdsAS, OctShared>)&sh, G.W, G.H, G.N);
        }
    } else if (kLdsPath && r == 0) {
        // everything node- and label-sized in LDS: ds_* accesses throughout
        OctWST<kLdsAS, kGlobalAS> w;
        w.keys = (asp<kGlobalAS, uint32_t>)keys;
        w.n = n;
        w.nq = (asp<kLdsAS, uint16_t>)(nodemem_lds + q.nq_off);
        w.m = oct_nodemem_carve<kLdsAS>(nodemem_lds, G.oct_cap);
        w.cap = G.oct_cap;
        w.out_keys = (asp<kGlobalAS, uint32_t>)out_keys;
        w.out_cap = G.kp_cap;
        w.dbg = dbg;
        w.cell_off = (asp<kLdsAS, const int32_t>)cell_off;
        w.cellkeys = (asp<kGlobalAS, const uint32_t>)ck;
        w.ncells = G.ncells;
        w.cell_cap = G.cell_cap;
        w.pyr = (asp<kLdsAS, uint32_t>)(nodemem_lds + pyr_off);
        w.pyrD = pyrD;
        w.rounds = a.oct_rounds;
        w.xcode = (asp<kLdsAS, uint16_t>)xtbl;
        w.ycode = (asp<kLdsAS, uint16_t>)(xtbl + G.W + 1);
        r = octree_distribute(p, w, (asp<kLdsAS, OctShared>)&sh, G.W, G.H, G.N);
        if (r == kOctDeep) {  // deeper than the pyramid: the label passes from the start
            __syncthreads();
            scan_cells();  // the node state overwrote the cell offsets
            w.pyrD = 0;
            r = octree_distribute(p, w, (asp<kLdsAS, OctShared>)&sh, G.W, G.H, G.N);
        }
    } else if (!kLdsPath && r == 0) {
        // huge levels: node state / labels / cell offsets in the global workspace where needed
        OctWST<kGeneric, kGeneric> w;
        w.keys = keys;
        w.n = n;
        w.nq = n <= q.lds_keys && off_in_lds ? reinterpret_cast<uint16_t*>(nodemem_lds + q.nq_off)
                                             : reinterpret_cast<uint16_t*>(ws + L.nq);
        w.m = oct_nodemem_carve<kGeneric>(nm, G.oct_cap);
        w.cap = G.oct_cap;
        w.out_keys = out_keys;
        w.out_cap = G.kp_cap;
        w.dbg = dbg;
        w.cell_off = cell_off;
        w.cellkeys = ck;
        w.ncells = G.ncells;
        w.cell_cap = G.cell_cap;
        w.pyr = nullptr;
        w.pyrD = 0;
        w.xcode = w.ycode = nullptr;
        if (!off_in_lds && n > q.lds_keys) r = -3;  // cell offsets occupy L.nq
        else r = octree_distribute(p, w, &sh, G.W, G.H, G.N);
    }
    if (threadIdx.x == 0) {
        a.lvlcnt[img * kMaxLevels + l] = r < 0 ? 0 : r;
        a.status[img * kMaxLevels + l] = r < 0 ? r : 0;
    }
}

// One workgroup per (image, level l0 + blockIdx.y), level-major dispatch: the long level-0
// groups go first.  NT = 512 for the leading levels, kOctSmallThreads for the short ones.
template <int NT>
__global__ __launch_bounds__(NT) void k_octree(BatchArgs a, int l0, OctCfg q) {
    extern __shared__ __attribute__((aligned(16))) uint8_t nodemem_lds[];  // per-launch size
    __shared__ int scratch[16];
    __shared__ OctShared sh;
    octree_level<true>(a, a.img0 + blockIdx.x, l0 + blockIdx.y, nodemem_lds, scratch, sh, q);
}

// The levels k_octree left with kOctRetry, redone with generic pointers: a small persistent
// grid walks all (image, level) slots, so the usual no-retry case costs one status read each.
__global__ __launch_bounds__(512, 1) void k_octree_retry(BatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t nodemem_lds[];  // a.oct_lds_bytes
    __shared__ int scratch[16];
    __shared__ OctShared sh;
    for (int s = blockIdx.x; s < a.nimages * a.nlevels; s += gridDim.x) {
        const int img = a.img0 + s / a.nlevels, l = s % a.nlevels;
        if (a.status[img * kMaxLevels + l] != kOctRetry) continue;  // uniform per workgroup
        octree_level<false>(a, img, l, nodemem_lds, scratch, sh, OctCfg{a.oct_nq_off, a.oct_lds_nodes, kOctLdsKeys, a.oct_lds_bytes});
        __syncthreads();
    }
}

hipError_t launch_octree(const BatchArgs& a, hipStream_t s) {
    // the dynamic-LDS limit is raised once per size and device (the attribute is per device; not
    // on every launch: the launch sequence may be captured into a hipGraph, orb_runtime.cpp)
    constexpr int kMaxDevices = 64;
    static std::atomic<int> lds_set[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = kMaxDevices - 1;
    std::atomic<int>& set = lds_set[dev];
    if (a.oct_lds_bytes > 65536 && a.oct_lds_bytes > set.load()) {
        for (const void* f : {reinterpret_cast<const void*>(k_octree<512>),
                              reinterpret_cast<const void*>(k_octree_retry)}) {
            hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, a.oct_lds_bytes);
            if (e != hipSuccess) return e;
        }
        int cur = set.load();
        while (a.oct_lds_bytes > cur && !set.compare_exchange_weak(cur, a.oct_lds_bytes)) {}
    }
    const int split = a.nimages < a.oct_split_min_images ? a.nlevels : std::min(a.oct_split, a.nlevels);
    if (split > 0)
        hipLaunchKernelGGL(k_octree<512>, dim3(a.nimages, split), dim3(512), a.oct_lds_bytes, s, a, 0,
                           OctCfg{a.oct_nq_off, a.oct_lds_nodes, kOctLdsKeys, a.oct_lds_bytes});
    if (split < a.nlevels) {
        const OctCfg q{a.oct2_nq_off, a.oct2_lds_nodes, a.oct2_lds_keys, a.oct2_lds_bytes};
        if (a.oct2_threads == 128)
            hipLaunchKernelGGL(k_octree<128>, dim3(a.nimages, a.nlevels - split), dim3(128), a.oct2_lds_bytes, s, a,
                               split, q);
        else
            hipLaunchKernelGGL(k_octree<256>, dim3(a.nimages, a.nlevels - split), dim3(256), a.oct2_lds_bytes, s, a,
                               split, q);
    }
    // levels that did not fit the LDS instantiation (rare: node state or cell offsets too large)
    if (a.oct_may_retry)
        hipLaunchKernelGGL(k_octree_retry, dim3(std::min(a.nimages * a.nlevels, 64)), dim3(512),
                           a.oct_lds_bytes, s, a);
    return hipGetLastError();
}

}  // namespace orbgpu
