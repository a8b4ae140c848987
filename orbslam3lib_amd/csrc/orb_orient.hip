// The per-keypoint work of ORBextractor::operator() (ORBextractor_old.cc) and its output assembly,
// for a batch of images:
//   k_orient_desc  32 lanes per keypoint: IC_Angle on the raw level (:78-105), then the rBRIEF
//                  descriptor on the blurred one (:108-148); with no lapping area in the batch it
//                  also writes the assembled outputs (fuse_out) and k_finalize does not run
//   k_finalize     one workgroup per image: scale to level 0, mono / stereo partition (:1130-1190)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_kernels.h"
#include "orb_math.h"
#include "orb_octree.h"  // the packed key's fields
#include "orb_pattern_data.h"

namespace orbgpu {

// rBRIEF pattern decoded at compile time from the hex data: 256 pairs (x0,y0,x1,y1) int8.
struct PatternTable {
    int8_t v[1024];
};
constexpr int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
constexpr PatternTable make_pattern() {
    PatternTable t{};
    const char* h = ORBGPU_PATTERN_HEX;
    for (int i = 0; i < 1024; ++i) t.v[i] = (int8_t)(hexval(h[2 * i]) * 16 + hexval(h[2 * i + 1]));
    return t;
}

// umax[] of the ORBextractor ctor (ORBextractor_old.cc:455-470) for HALF_PATCH_SIZE = 15.
__constant__ int c_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

// ---------------------------------------------------------------------------------------------
constexpr int kOdLanes = 32;                   // lanes per keypoint
constexpr int kOdPairs = 256 / kOdLanes;       // test pairs per lane
static_assert(kOdLanes == 32, "k_orient_desc: one disc row and 8 test pairs per lane");
static_assert(kOdKpBlock == 256 / kOdLanes, "orb_kernels.h kOdKpBlock");

constexpr int kOdPatchR = 18;                    // |rotated pattern offset| <= 13*sqrt(2) < 19
constexpr int kOdPatchRows = 2 * kOdPatchR + 1;  // 37
constexpr int kOdPatchPitch = 48;                // 3 x 16 B: covers x-18..x+18 from the dword below
constexpr int kOdPatchChunks = kOdPatchRows * 3; // 16-byte chunks per patch
constexpr int kOdPatchIt = (kOdPatchChunks + kOdLanes - 1) / kOdLanes;

// Sum of v over each 32-lane group of the wave, in every lane: DPP quad_perm xor 1 / xor 2, row
// half-mirror (pairs the two quads of 8 lanes) and row mirror (the two halves of a 16-lane row),
// then the other row of the 32 through ds_swizzle (xor mask 16).
__device__ inline int od_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);  // row_mirror
    return v + __builtin_amdgcn_ds_swizzle(v, 0x401F);               // lane ^ 16 within 32
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// k_orient_desc's two LDS tables, built at compile time and copied once per workgroup (building
// them in the kernel took ~200 VALU per wave, comparable to a whole keypoint pass):
//   rng[m * 17 + n]: 0xFF in bytes [m, n) of a 16-byte chunk (none if n <= m);
//   pat[b * kOdLanes + lane]: float bit patterns {x0, x1, y0, y1} of test pair 8 lane + b.
struct OdTables {
    uint32_t rng[17 * 17][4];
    uint32_t pat[kOdPairs * kOdLanes][4];
};
constexpr OdTables make_od_tables() {
    OdTables t{};
    for (int m = 0; m < 17; ++m)
        for (int n = 0; n < 17; ++n)
            for (int j = 0; j < 16; ++j)
                if (j >= m && j < n) t.rng[m * 17 + n][j >> 2] |= 0xFFu << (8 * (j & 3));
    const PatternTable pt = make_pattern();
    for (int b = 0; b < kOdPairs; ++b)
        for (int lane = 0; lane < kOdLanes; ++lane) {
            const int8_t* pv = pt.v + 4 * (kOdPairs * lane + b);  // x0, y0, x1, y1
            t.pat[b * kOdLanes + lane][0] = __builtin_bit_cast(uint32_t, (float)pv[0]);
            t.pat[b * kOdLanes + lane][1] = __builtin_bit_cast(uint32_t, (float)pv[2]);
            t.pat[b * kOdLanes + lane][2] = __builtin_bit_cast(uint32_t, (float)pv[1]);
            t.pat[b * kOdLanes + lane][3] = __builtin_bit_cast(uint32_t, (float)pv[3]);
        }
    return t;
}
__constant__ OdTables c_od_tab = make_od_tables();

// cv::KeyPoint as written to the outputs (orbgpu_keypoint): pt.x, pt.y, size, angle, response,
// octave, class_id
struct KP28 {
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

// k_orient_desc: IC_Angle on the raw level (ORBextractor_old.cc:78-105) then
// computeOrbDescriptor on the blurred level (:108-148): a = (float)cos, b = (float)sin of
// angle*pi/180 (float), sample center[cvRound(x*b + y*a)*step + cvRound(x*a - y*b)].
// 32 lanes per keypoint (two independent groups per wave): lane `sub` owns disc row v = sub - 15
// for the moments and test pairs [8 sub, 8 sub + 8), sampled from the keypoint's blurred patch
// staged in LDS.  The kernel waits on dependent memory round trips per keypoint (key, moment
// rows + patch); few vector-memory instructions and registers per lane keep many of them in
// flight.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void k_orient_desc(
    BatchArgs a, uint32_t nblk_magic) {
    // per keypoint group: the blurred patch around the keypoint, staged with 16-byte loads
    __shared__ __attribute__((aligned(16))) uint8_t patch[kOdKpBlock][kOdPatchRows * kOdPatchPitch];
    const int wg = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    // wg / gridDim.x by the host's magic multiplier; the block's level from a host record (no
    // level search with dependent kernarg loads)
    const int irel = gridDim.x == 1 ? wg : (int)__umulhi((uint32_t)wg, nblk_magic);
    const int img = a.img0 + irel, bx = wg - irel * (int)gridDim.x;
    const int l = a.rtab[a.od_tab_off + bx].x;
    const LevelGeom G = a.lv[l];
    const int sub = threadIdx.x % kOdLanes, grp = threadIdx.x / kOdLanes;
    const int count = a.lvlcnt[img * kMaxLevels + l];
    const long long kbase = (long long)img * a.lvlkp_img_stride + G.kp_off;
    const uint8_t* lvl = a.lvl_base[l] + (long long)img * G.img_stride;
    const uint8_t* blr = a.blur_base[l] + (long long)img * G.bimg_stride;
    const bool raw_dw = ((G.pitch | G.img_stride) & 3) == 0;
    // raw buffer over this image's blurred level (dword 3 = gfx9 raw-buffer format word)
    const __amdgpu_buffer_rsrc_t brs =
        __builtin_amdgcn_make_buffer_rsrc((void*)blr, (short)0, G.bpitch * G.h, 0x00020000);
    const int stride_k = G.od_blocks * kOdKpBlock;
    // a.fuse_out (every image of the batch has no lapping area, so every keypoint is mono): the
    // assembly of k_finalize (ORBextractor_old.cc:1130-1190) is done here -- keypoint j of level l
    // goes to output row off[l] + j, with pt *= mvScaleFactor[l], size, octave, class_id -1 --
    // and k_finalize does not run.  off[l] and the image's total come from the level counts (16
    // scalar loads); a level the octree could not finish or a total past out_cap writes the status
    // word instead, as k_finalize does.
    int out_row0 = 0;
    bool out_ok = false;
    if (a.fuse_out) {
        int total = 0;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < kMaxLevels; ++k)
            if (k < a.nlevels) {
                if (k < l) out_row0 += a.lvlcnt[img * kMaxLevels + k];
                total += a.lvlcnt[img * kMaxLevels + k];
                bad |= a.status[img * kMaxLevels + k] != 0;
            }
        out_ok = !bad && total <= a.out_cap;
        if (bx == 0 && threadIdx.x == 0) {  // one workgroup per image writes the counts
            a.out_n[img] = bad ? -5 : total > a.out_cap ? -2 : total;
            a.out_mono[img] = out_ok ? total : 0;
        }
    }
    KP28* const out_kp = reinterpret_cast<KP28*>(a.out_kps) + (long long)img * a.out_cap + out_row0;
    uint8_t* const out_d = a.out_desc + ((long long)img * a.out_cap + out_row0) * 32;
    // Moments from coalesced row chunks: the 31 disc rows of a keypoint are read as 16-byte
    // aligned chunks of the 48-byte window that starts at xa16 = (x - 15) & ~15 (it holds
    // x - 15 .. x + 15 for every x).  Chunk slot i = sub + 32 it (it < 3) is disc row r = i / 3
    // (v = r - 15; r = 31 lies past the disc) and part i % 3, so the three lanes of a row read 48
    // contiguous bytes -- one or two cache lines per row instead of three 16-byte / dword loads
    // per row lane (round 4: ~105 of the ~160 L1 accesses per keypoint were those).  Each chunk
    // adds its masked byte sums: s = sum of p, c = sum of (column - xa16) p over the disc span
    // |u| <= umax[|v|], i.e. chunk bytes [m, n) with m, n from the alignment a = (x - 15) & 15 and
    // two per-lane constants; the byte masks of every [m, n) are an LDS table, so a chunk is one
    // b128 LDS read, 4 ANDs and 8 v_dot4_u32_u8.  Then m_10 = sum c - (15 + a) sum s and
    // m_01 = sum v s.
    __shared__ __attribute__((aligned(16))) uint4 s_rng[17][17];  // bytes [m, n) of 16 (none if n <= m)
    __shared__ __attribute__((aligned(16))) uint4 s_pat[kOdPairs][kOdLanes];
    static_assert(kOdPairs * kOdLanes == 256 && 17 * 17 <= 2 * 256, "table copy: one / two entries per thread");
    const uint4* rng_src = reinterpret_cast<const uint4*>(c_od_tab.rng);
    const uint4 rng0 = rng_src[threadIdx.x];
    const uint4 pat0 = reinterpret_cast<const uint4*>(c_od_tab.pat)[threadIdx.x];
    if (threadIdx.x < 17 * 17 - 256) (&s_rng[0][0])[threadIdx.x + 256] = rng_src[threadIdx.x + 256];
    (&s_rng[0][0])[threadIdx.x] = rng0;
    (&s_pat[0][0])[threadIdx.x] = pat0;
    __syncthreads();
    // this lane's three chunk slots: row v, chunk bytes [lo + a, hi + a) clamped to [0, 16) are
    // the disc span (lo = 15 - d - 16 part, hi = 16 + d - 16 part, d = umax[|v|], -1 past the
    // disc), the part's column offset and the byte offset from the window
    int mv[3], mlo[3], mhi[3], mofs[3], mp16[3];
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int i = sub + 32 * it, r = i / 3, part = i - 3 * r;
        mv[it] = r - 15;
        const int d = r < 31 ? c_umax[mv[it] < 0 ? -mv[it] : mv[it]] : -1;
        mlo[it] = 15 - d - 16 * part;
        mhi[it] = 16 + d - 16 * part;
        mofs[it] = (r < 31 ? mv[it] : 15) * G.pitch + 16 * part;
        mp16[it] = 16 * part;
    }
    const __amdgpu_buffer_rsrc_t lrs =
        __builtin_amdgcn_make_buffer_rsrc((void*)lvl, (short)0, (int)min((long long)G.pitch * G.h, 0x7fffffffLL), 0x00020000);
    uint8_t* pt = patch[grp];
    // uniform trip count per wave so the group shuffles see all lanes
    const int wave_first = (bx - G.od_first) * kOdKpBlock + (threadIdx.x >> 6) * 2;
    // each iteration's key is loaded one iteration ahead, so its round trip overlaps the
    // previous keypoint's work
    auto key_at = [&](int kb) {
        const int kp = kb + (grp & 1);
        return kp < count ? a.lvlkey[kbase + kp] : a.lvlkey[kbase + kb];
    };
    uint32_t key_next = wave_first < count ? key_at(wave_first) : 0u;
    for (int kb = wave_first; kb < count; kb += stride_k) {
        const int kp = kb + (grp & 1);
        const bool valid = kp < count;
        const uint32_t key = key_next;
        if (kb + stride_k < count) key_next = key_at(kb + stride_k);
        const int x = key_x(key) + kMinBorder, y = key_y(key) + kMinBorder;
        const int al = (x - 15) & 15;
        const int wofs = y * G.pitch + (x - 15 - al);  // the 48-byte window of disc row 0
        // the three moment chunks (round trip 1) and the 37 x 37 blurred patch (rows y-18..y+18
        // from the dword at or below x-18, 16-byte buffer loads, out-of-range bytes read as 0
        // and never sampled) are both requested before either is used, so the two round trips
        // overlap; window bytes past x + 15 (or past the plane: 0) only meet zero masks
        uint4 mc[3];
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            if (raw_dw) {
                const auto q = __builtin_amdgcn_raw_buffer_load_b128(lrs, wofs + mofs[it], 0, 0);
                mc[it] = make_uint4(q[0], q[1], q[2], q[3]);
            } else {  // level-0 rows not 4-byte aligned: bytes
                const uint8_t* q = lvl + wofs + mofs[it];
                uint32_t d4[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    d4[k] = (uint32_t)q[4 * k] | ((uint32_t)q[4 * k + 1] << 8) | ((uint32_t)q[4 * k + 2] << 16) |
                            ((uint32_t)q[4 * k + 3] << 24);
                mc[it] = make_uint4(d4[0], d4[1], d4[2], d4[3]);
            }
        }
        const int xb = (x - kOdPatchR) & ~3;
        const int pofs = (y - kOdPatchR) * G.bpitch + xb;
        uint4 pv[kOdPatchIt];
#pragma unroll
        for (int it = 0; it < kOdPatchIt; ++it) {
            const int c = sub + it * kOdLanes;
            const int r = c / 3, part = c - 3 * r;
            if (c < kOdPatchChunks) {
                const auto q = __builtin_amdgcn_raw_buffer_load_b128(brs, pofs + r * G.bpitch + 16 * part, 0, 0);
                pv[it] = make_uint4(q[0], q[1], q[2], q[3]);
            }
        }
        // IC_Angle (:78-105) over this lane's three chunks
        int s_all = 0, c_all = 0, m01p = 0;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int m = min(max(mlo[it] + al, 0), 16), n = min(max(mhi[it] + al, 0), 16);
            const uint4 mk = s_rng[m][n];
            const uint32_t p0 = mc[it].x & mk.x, p1 = mc[it].y & mk.y, p2 = mc[it].z & mk.z, p3 = mc[it].w & mk.w;
            uint32_t sc = __builtin_amdgcn_udot4(p0, 0x01010101u, 0u, false);
            sc = __builtin_amdgcn_udot4(p1, 0x01010101u, sc, false);
            sc = __builtin_amdgcn_udot4(p2, 0x01010101u, sc, false);
            sc = __builtin_amdgcn_udot4(p3, 0x01010101u, sc, false);
            uint32_t cc = __builtin_amdgcn_udot4(p0, 0x03020100u, 0u, false);  // column within the chunk
            cc = __builtin_amdgcn_udot4(p1, 0x07060504u, cc, false);
            cc = __builtin_amdgcn_udot4(p2, 0x0B0A0908u, cc, false);
            cc = __builtin_amdgcn_udot4(p3, 0x0F0E0D0Cu, cc, false);
            s_all += (int)sc;
            c_all += (int)cc + mp16[it] * (int)sc;
            m01p += mv[it] * (int)sc;
        }
        // sums over the keypoint's lanes (DPP, no LDS round trip but the last step)
        const int m10 = od_sum(c_all - (15 + al) * s_all), m01 = od_sum(m01p);
        const float angle = fast_atan2_deg((float)m01, (float)m10);
        // computeOrbDescriptor (:108-148): lane `sub` makes bits [8 sub, 8 sub + 8)
        const float factorPI = (float)(3.14159265358979323846 / 180.0);
        float sn, ca;  // std::sin(float) / std::cos(float) (:114-115): libm sinf / cosf
        libm_sincosf(angle * factorPI, &sn, &ca);
        // the patch to LDS: every sample is then an LDS byte read (4 vector-memory instructions
        // per lane instead of one scattered byte load per sample)
#pragma unroll
        for (int it = 0; it < kOdPatchIt; ++it) {
            const int c = sub + it * kOdLanes;
            const int r = c / 3, part = c - 3 * r;
            if (c < kOdPatchChunks) *reinterpret_cast<uint4*>(pt + r * kOdPatchPitch + 16 * part) = pv[it];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the group's own lanes read it
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int pc = kOdPatchR * kOdPatchPitch + (x - xb);  // patch offset of the keypoint
        // both samples of a test pair as packed f32 (each element an IEEE single operation, no
        // contraction): row = x*b + y*a, col = x*a - y*b as the reference's float expressions
        // (:116-121), then cvRound by adding 1.5 * 2^23 (round to nearest even, |value| < 19),
        // whose low 24 bits are 2^22 + the rounded value: the LDS offset is one v_mad_u32_u24 of
        // the two bit patterns and a per-keypoint constant (no v_rndne / v_cvt per sample)
        const float magic = 12582912.0f;
        const uint32_t kofs = (uint32_t)pc - 0x4B400000u - 0x400000u * (uint32_t)kOdPatchPitch;
        const f32x2 snv = {sn, sn}, cav = {ca, ca}, mg = {magic, magic};
        // the LDS address of a sample is v_mad_u32_u24(R, pitch, C) + kpb, the patch base folded
        // into the per-keypoint constant: one full-rate v_add_u32 per sample where the compiler's
        // own association gave a v_add3_u32 (slow class, profiles/r06/valu_rates.json)
        typedef const __attribute__((address_space(3))) uint8_t lds_u8;
        const uint32_t kpb = kofs + (uint32_t)(uintptr_t)(lds_u8*)pt;
        uint32_t bits = 0;
#pragma unroll
        for (int b = kOdPairs - 1; b >= 0; --b) {  // bit b of the byte is pair b's test
            uint4 pw = s_pat[b][sub];  // float bit patterns {x0, x1, y0, y1}
            asm volatile("" : "+v"(pw.x), "+v"(pw.y), "+v"(pw.z), "+v"(pw.w));  // not hoisted
            const f32x2 X = {__uint_as_float(pw.x), __uint_as_float(pw.y)};
            const f32x2 Y = {__uint_as_float(pw.z), __uint_as_float(pw.w)};
            const f32x2 R = (X * snv + Y * cav) + mg;
            const f32x2 C = (X * cav - Y * snv) + mg;
            // the unsigned sums wrap to the small patch offsets
            uint32_t m0 = __umul24(__float_as_uint(R.x), (uint32_t)kOdPatchPitch) + __float_as_uint(C.x);
            uint32_t m1 = __umul24(__float_as_uint(R.y), (uint32_t)kOdPatchPitch) + __float_as_uint(C.y);
            asm volatile("" : "+v"(m0), "+v"(m1));  // keep the mad's addend C (not re-associated)
            const uint32_t p0 = *(lds_u8*)(uintptr_t)(m0 + kpb), p1 = *(lds_u8*)(uintptr_t)(m1 + kpb);
            // p0 < p1 <=> the sign of p0 - p1: shifted to bit b and merged by one v_bitop3
            // (A | (B & C)) -- full-rate ops instead of v_cmp + v_cndmask + a shift-or
            bits = __builtin_amdgcn_bitop3_b32(bits, (p0 - p1) >> (31 - b), 1u << b, 0xf8);
        }
        if (valid && !out_ok) {  // the level arrays, for k_finalize (or a status image)
            if (sub == 0) a.lvlangle[kbase + kp] = angle;
            a.lvldesc[(kbase + kp) * 32 + sub] = (uint8_t)bits;
        }
        if (valid) {
            if (out_ok) {  // the assembled output row (k_finalize's arithmetic): lanes 0-6 its 7 dwords
                out_d[kp * 32 + sub] = (uint8_t)bits;
                if (sub < 7) {
                    float px = (float)(x), py = (float)(y);
                    if (l != 0) {
                        px = px * G.scale;
                        py = py * G.scale;
                    }
                    const uint32_t w7[7] = {__float_as_uint(px), __float_as_uint(py), __float_as_uint((float)G.patch),
                                            __float_as_uint(angle), __float_as_uint((float)key_resp(key)),
                                            (uint32_t)l, 0xFFFFFFFFu};
                    uint32_t v = w7[0];
#pragma unroll
                    for (int k = 1; k < 7; ++k) v = sub == k ? w7[k] : v;
                    reinterpret_cast<uint32_t*>(out_kp + kp)[sub] = v;
                }
            }
        }
    }
}

hipError_t launch_orient_desc(const BatchArgs& a, hipStream_t s) {
    const uint32_t d = (uint32_t)a.total_od_blocks;
    const uint32_t magic = d > 1 ? 0xFFFFFFFFu / d + 1u : 0u;  // ceil(2^32 / d) for d >= 2
    hipLaunchKernelGGL(k_orient_desc, dim3(a.total_od_blocks, a.nimages), dim3(256), 0, s, a, magic);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_finalize: ORBextractor::operator() assembly (ORBextractor_old.cc:1130-1190): levels in
// order, pt *= mvScaleFactor[level] for level > 0, keypoints inside [lap0, lap1] written from
// the back, the others from the front; returns monoIndex.

// The image's keypoints are walked as one sequence (level l's keypoint j at off[l] + j), in
// batches of kFinU chunks of kFinThreads whose loads are all issued before the first chunk's partition,
// so a batch costs one memory round trip instead of one per level and chunk.  The mono / stereo
// ranks come from per-wave ballots and one barrier per chunk.
constexpr int kFinU = 2;
#ifndef FIN_WIDE_MAX
#define FIN_WIDE_MAX 8
#endif
constexpr int kFinWideMaxImages = FIN_WIDE_MAX;

template <int kFinThreads>  // a chunk is one keypoint per thread
__global__ __launch_bounds__(kFinThreads) void k_finalize(BatchArgs a) {
    __shared__ int4 s_lv[kMaxLevels];  // {level key base (image-relative), off[l], scale bits, patch}
    __shared__ int s_wave[2][kFinThreads / 64];  // per-wave stereo counts, double-buffered over chunks
    const int img = a.img0 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int L = a.nlevels;
    int off[kMaxLevels];  // uniform: first sequence index of each level
    int total = 0;
    bool bad = false;
#pragma unroll
    for (int l = 0; l < kMaxLevels; ++l) {
        off[l] = total;
        if (l < L) {
            total += a.lvlcnt[img * kMaxLevels + l];
            bad |= a.status[img * kMaxLevels + l] != 0;
        }
    }
    if (bad || total > a.out_cap) {
        if (tid == 0) {
            a.out_n[img] = bad ? -5 : -2;
            a.out_mono[img] = 0;
        }
        return;
    }
    if (tid == 0) {  // uniform level loop: the level records are read with scalar loads
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l)
            if (l < L) s_lv[l] = make_int4(a.lv[l].kp_off, off[l], __float_as_int(l == 0 ? 1.f : a.lv[l].scale), a.lv[l].patch);
    }
    __syncthreads();
    const float lap0 = (float)a.laps[2 * img], lap1 = (float)a.laps[2 * img + 1];
    KP28* out = reinterpret_cast<KP28*>(a.out_kps) + (long long)img * a.out_cap;
    uint8_t* od = a.out_desc + (long long)img * a.out_cap * 32;
    const long long ibase = (long long)img * a.lvlkp_img_stride;
    const uint64_t lt = (1ull << lane) - 1ull;
    int mono = 0, stereo = 0, chunk_no = 0;
    for (int base = 0; base < total; base += kFinThreads * kFinU) {
        uint32_t key[kFinU];
        float ang[kFinU];
        uint4 d0[kFinU], d1[kFinU];
        int lev[kFinU];
#pragma unroll
        for (int u = 0; u < kFinU; ++u) {
            const int i = base + u * kFinThreads + tid;
            int l = 0;
#pragma unroll
            for (int k = 1; k < kMaxLevels; ++k) l += (k < L && i >= off[k]) ? 1 : 0;
            lev[u] = l;
            if (i < total) {
                const int4 info = s_lv[l];
                const long long kb = ibase + info.x + (i - info.y);
                key[u] = a.lvlkey[kb];
                ang[u] = a.lvlangle[kb];
                const uint4* s4 = reinterpret_cast<const uint4*>(a.lvldesc + kb * 32);
                d0[u] = s4[0];
                d1[u] = s4[1];
            }
        }
#pragma unroll
        for (int u = 0; u < kFinU; ++u) {
            const int cb = base + u * kFinThreads;
            if (cb >= total) continue;  // uniform (the batch's last chunks)
            const int i = cb + tid;
            const bool valid = i < total;
            KP28 k;
            bool st = false;
            if (valid) {
                const int l = lev[u];
                const int4 info = s_lv[l];
                k.x = (float)(key_x(key[u]) + kMinBorder);
                k.y = (float)(key_y(key[u]) + kMinBorder);
                if (l != 0) {
                    k.x = k.x * __int_as_float(info.z);
                    k.y = k.y * __int_as_float(info.z);
                }
                k.size = (float)info.w;
                k.angle = ang[u];
                k.response = (float)key_resp(key[u]);
                k.octave = l;
                k.class_id = -1;
                st = (k.x >= lap0 && k.x <= lap1);
            }
            const uint64_t bal = __ballot(st);
            const int buf = chunk_no & 1;
            if (lane == 0) s_wave[buf][w] = __popcll(bal);
            __syncthreads();
            int before = 0, tst = 0;
#pragma unroll
            for (int v = 0; v < kFinThreads / 64; ++v) {
                const int c = s_wave[buf][v];
                tst += c;
                before += v < w ? c : 0;
            }
            const int exs = before + __popcll(bal & lt);
            const int exm = tid - exs;  // earlier lanes of this chunk are all valid
            if (valid) {
                const int dst = st ? (total - 1 - (stereo + exs)) : (mono + exm);
                out[dst] = k;
                uint4* d4 = reinterpret_cast<uint4*>(od + (long long)dst * 32);
                d4[0] = d0[u];
                d4[1] = d1[u];
            }
            const int chunk = min(kFinThreads, total - cb);
            stereo += tst;
            mono += chunk - tst;
            ++chunk_no;
        }
    }
    if (threadIdx.x == 0) {
        a.out_n[img] = total;
        a.out_mono[img] = mono;
    }
}

hipError_t launch_finalize(const BatchArgs& a, hipStream_t s) {
    // few images (the latency shape): 1024 / 512 threads per image (one load round trip covers
    // 2048 / 1024 keypoints); full batches: 256
    if (a.nimages <= 2) hipLaunchKernelGGL(k_finalize<1024>, dim3(a.nimages), dim3(1024), 0, s, a);
    else if (a.nimages <= kFinWideMaxImages) hipLaunchKernelGGL(k_finalize<512>, dim3(a.nimages), dim3(512), 0, s, a);
    else hipLaunchKernelGGL(k_finalize<256>, dim3(a.nimages), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace orbgpu
