// The cell loop of ORBextractor::ComputeKeyPointsOctTree (ORBextractor_old.cc:783-874) for a batch
// of images; the per-cell algorithm is orb_fast_cell.h (shared with the host harness).
//   k_fast_cells<CP, kSmall>  one workgroup per (image, 35-px cell) of the levels whose cells fit
//                             the CP-byte LDS tile (48, 64 or 80); kSmall: a capped candidate list
//   k_fast_cells_ovf<64>      the cells a small-list launch queued, redone with the full list
// Which of them one call launches is fast_launch_plan (orb_kernels.h, pure host code).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_kernels.h"
#include "orb_fast_cell.h"
#include "orb_policy.h"

namespace orbgpu {

// ---------------------------------------------------------------------------------------------
// k_fast_cells: one workgroup per (level, cell), image = blockIdx.y.  Restates the cell loop of
// ComputeKeyPointsOctTree (ORBextractor_old.cc:807-871) with cv::FAST(cell, kps, th, true):
// detection on [3,rows-3)x[3,cols-3) of the cell ROI, 3x3 nonmax inside the cell only, iniTh
// then minTh if the cell yields nothing, keys emitted in row-major order.

// k_fast_cells' policy.  A 64-thread workgroup is one wave per cell: the wave's corner list is
// the cell's, so fast_cell_detect writes the keys in its nonmax pass (orb_fast_cell.h).
template <int NT>
struct FastCellPolicy : FixedDevPolicy<NT> {
    static constexpr bool kOneWavePerCell = NT == 64;
};

// One cell of image img (flattened cell index gcell) with a candidate list of kCap entries;
// returns the kept count (written to the cell's count) or kFastOverflow (nothing written).
template <int CP, int kCap>
__device__ __attribute__((always_inline)) inline int fast_cell_one(const BatchArgs& a, int img, int gcell, uint8_t* T,
                                                                   uint8_t* M, uint16_t* list, uint2* lut,
                                                                   uint32_t* emask, int32_t* wcnt, int32_t* wovf,
                                                                   int* scratch) {
    constexpr int kFastThreads = fast_threads<CP>();
    // the cell's record (host: the cell loop's geometry, :807-821)
    const int4 e0 = a.rtab[a.fast_tab_off + 2 * gcell];
    const int4 e1 = a.rtab[a.fast_tab_off + 2 * gcell + 1];
    const int l = e0.x;
    const LevelGeom G = a.lv[l];
    int32_t* cnt_out = a.cellcnt + (long long)img * a.cellcnt_img_stride + e1.x;
    uint32_t* key_out = a.cellkeys + (long long)img * a.cellkeys_img_stride + e1.y;
    CellGeom g;
    g.iniX = e0.y;
    g.iniY = e0.z;
    g.minBorder = kMinBorder;
    if (e1.z) {  // :812, :821
        if (threadIdx.x == 0) *cnt_out = 0;
        return 0;
    }
    g.rows = e0.w & 0xFFFF;
    g.cols = e0.w >> 16;
    const bool dword_ok = ((G.pitch | G.img_stride) & 3) == 0;
    const int sh = dword_ok ? (g.iniX & 3) : 0;
    const uint8_t* base = a.lvl_base[l] + (long long)img * G.img_stride;
    const long long roi = (long long)g.iniY * G.pitch + (g.iniX - sh);
    const uint8_t* src = base + roi;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)base, (short)0, (int)min(G.img_stride, 0x7fffffffLL), 0x00020000);
    const int roi32 = (int)roi;  // planes are < 2 GB (buffer offsets are 32-bit)
    auto ld16 = [&](long long off) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, roi32 + (int)off, 0, 0);
        return make_uint4(v[0], v[1], v[2], v[3]);
    };
    FastCellPolicy<kFastThreads> p{{{scratch}}};
    fast_cell_tables<CP>(g, sh, lut, emask);  // synced with the ROI staging (fast_cell_run)
    CellScratch cs{T, M, list, wcnt, lut, emask, wovf};
    const int n = fast_cell_run<CP, kCap>(p, src, G.pitch, sh, dword_ok, g, a.ini_th, a.min_th, cs, key_out, ld16);
    if (n != kFastOverflow && threadIdx.x == 0) *cnt_out = n;
    return n;
}

// k_fast_cells<CP, kSmall>: one workgroup per (image, cell) of the tile's cells.  kSmall (the
// 48- and 64-byte tiles of launches of more than kFastMergeMaxImages images): a capped candidate
// list, kFastSmallList<CP> entries split over the waves (48: LDS 5.9 instead of 8.4 KB per
// workgroup, 26 instead of 19 resident per CU; 64: 11 instead of 15.2 KB; round 6: residency
// moves this kernel by up to ~20%).  A cell whose pre-test passes more pixels than fit (none of
// the bench frames' cells at iniThFAST, where the most is 441 of 1225 in a 48-byte cell) is
// queued (a.fast_ovf, per-launch slice by img0) and redone by k_fast_cells_ovf.
template <int CP, bool kSmall>
__global__ __launch_bounds__(fast_threads<CP>()) void k_fast_cells(BatchArgs a, int cell0, uint32_t ncell_magic) {
    constexpr int kList = kSmall ? kFastSmallList<CP>() : cell_list_cap<CP>(), kFastThreads = fast_threads<CP>();
    __shared__ __attribute__((aligned(16))) uint8_t T[CP * CP];
    __shared__ __attribute__((aligned(16))) uint8_t M[CP * CP];  // 16-byte rows when CP % 16 == 0
    __shared__ __attribute__((aligned(8))) uint16_t list[kList + fast_list_slack(kFastThreads / 64)];
    __shared__ uint2 lut[16];
    __shared__ uint32_t emask[32];
    __shared__ int32_t wcnt[kFastThreads / 64], wovf[kFastThreads / 64];
    __shared__ int scratch[16];
    const int wg = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    // wg / gridDim.x by the host's magic multiplier (exact for wg < 2^32 / gridDim.x)
    const int irel = gridDim.x == 1 ? wg : (int)__umulhi((uint32_t)wg, ncell_magic);
    const int img = a.img0 + irel;
    const int gcell = cell0 + (wg - irel * (int)gridDim.x);  // flattened over the levels
    const int n = (kSmall && a.fast_ovf_all) ? kFastOverflow  // diagnostics: every cell to the full-list pass
                                             : fast_cell_one<CP, kList>(a, img, gcell, T, M, list, lut, emask, wcnt, wovf, scratch);
    if (kSmall && n == kFastOverflow && threadIdx.x == 0) {
        const int q = __hip_atomic_fetch_add(a.fast_ovf_cnt + 2 * a.img0, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.fast_ovf[(long long)a.img0 * a.fast_qcap + q] = make_int2(img, gcell);
    }
}

// The cells k_fast_cells<CP, true> queued, with the full candidate list: a small grid walks the
// launch's queue (the count is read after the queueing launch finished: same stream); the last
// workgroup to finish resets the count and its own arrival counter for the next launch.
template <int CP>
__global__ __launch_bounds__(fast_threads<CP>()) void k_fast_cells_ovf(BatchArgs a) {
    constexpr int kList = cell_list_cap<CP>(), kFastThreads = fast_threads<CP>();
    __shared__ __attribute__((aligned(16))) uint8_t T[CP * CP];
    __shared__ __attribute__((aligned(16))) uint8_t M[CP * CP];
    __shared__ __attribute__((aligned(8))) uint16_t list[kList + fast_list_slack(kFastThreads / 64)];
    __shared__ uint2 lut[16];
    __shared__ uint32_t emask[32];
    __shared__ int32_t wcnt[kFastThreads / 64], wovf[kFastThreads / 64];
    __shared__ int scratch[16];
    int* const cnt = a.fast_ovf_cnt + 2 * a.img0;  // [0] queued cells, [1] finished workgroups
    // written by the previous launch on this stream (complete before this one starts): a plain
    // load; with nothing queued (the usual case) the launch ends here, no counter to reset
    const int nq = *cnt;
    if (nq == 0) return;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int2 e = a.fast_ovf[(long long)a.img0 * a.fast_qcap + q];
        fast_cell_one<CP, kList>(a, e.x, e.y, T, M, list, lut, emask, wcnt, wovf, scratch);
        __syncthreads();  // the LDS scratch is reused by the next cell
    }
    if (threadIdx.x == 0) {
        // every workgroup has read the count once it arrives here (the loop above depends on the
        // value), so the last one may clear both; the counters order nothing else (relaxed)
        const int done = __hip_atomic_fetch_add(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == (int)gridDim.x - 1) {
            __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(cnt + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

static_assert(kCellPitchTiny == 48 && kCellPitchSmall == 64, "fast_launch_plan's tile widths (orb_kernels.h)");

template <int CP, bool kSmall>
static void launch_cells(const BatchArgs& a, const FastLaunchPlan& p, hipStream_t s) {
    const uint32_t d = (uint32_t)(p.c1 - p.c0);
    const uint32_t magic = d > 1 ? 0xFFFFFFFFu / d + 1u : 0u;  // ceil(2^32 / d) for d >= 2
    hipLaunchKernelGGL((k_fast_cells<CP, kSmall>), dim3(d, a.nimages), dim3(fast_threads<CP>()), 0, s, a, p.c0, magic);
}

// What to launch is fast_launch_plan's decision (orb_kernels.h); this turns it into launches.
hipError_t launch_fast_cells(const BatchArgs& a, int tile, hipStream_t s) {
    const FastLaunchPlan p = fast_launch_plan(a, tile);
    switch (p.tile) {
        case 0: return hipSuccess;
        case kCellPitchTiny: p.small ? launch_cells<kCellPitchTiny, true>(a, p, s) : launch_cells<kCellPitchTiny, false>(a, p, s); break;
        case kCellPitchSmall: p.small ? launch_cells<kCellPitchSmall, true>(a, p, s) : launch_cells<kCellPitchSmall, false>(a, p, s); break;
        default: launch_cells<kCellMax, false>(a, p, s);
    }
    if (p.ovf)
        hipLaunchKernelGGL(k_fast_cells_ovf<kCellPitchSmall>, dim3(kFastOvfBlocks), dim3(fast_threads<kCellPitchSmall>()), 0, s, a);
    return hipGetLastError();
}

}  // namespace orbgpu
