// ORBextractor::ComputePyramid and the per-level GaussianBlur of operator() (ORBextractor_old.cc:
// 1331-1356, 1146-1147), bit-exact fixed point, for a batch of images:
//   k_blur_resize   level l - 1's 7x7 blur (matrix cores) and the INTER_LINEAR / exact-2x resize to
//                   level l from one read of level l - 1
//   k_blur          the blur alone: the last level, or every level when the scale step exceeds 2
//   k_level_linear  the resize alone, for scale steps above 2
//   k_pyr_tail      the small levels' resizes and blurs in one launch, one workgroup per image
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "orb_kernels.h"

namespace orbgpu {

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ inline u16x2 as_u16x2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ inline uint32_t as_u32(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }

// cv::resize INTER_LINEAR (canonical ComputePyramid, ORBextractor_old.cc:1342-1344), fixed point.
// Four output pixels dx0 .. dx0+3 of one output row from source rows r0 / r1 (LDS window rows,
// indexed by source column).  The quad's taps lie in the 8 source bytes from its first left tap
// `base` (scale <= 2: the last right tap is at most base + 7), read as three aligned dwords per
// row and byte-aligned with v_alignbyte; sel[k] picks output k's two taps as a u16 pair (v_perm)
// and cw[k] holds its two x coefficients times 16 as a u16 pair (16 c <= 32768), so each
// horizontal sum is one v_dot2_u32_u16 yielding 16 D (exact: < 2^23).  Vertical rounding:
// OpenCV's SIMD body (VResizeLinearVec_32s8u) below simd_end,
//   out = (((D0 >> 4) b0 >> 16) + ((D1 >> 4) b1 >> 16) + 2) >> 2,
// where (D >> 4) << 8 = 16 D & ~0xFF and the row weights come as b << 8 (B0 / B1 <= 2^19), so
// each ((D >> 4) b) >> 16 is one v_mul_hi_u32_u24 of two 24-bit operands (the 48-bit product
// >> 32); the sum is <= 1022 (c0 + c1 = b0 + b1 = 2048), so no clamp is needed.  FixedPtCast
// after simd_end (only the last quads of a row take that branch).
// The two halves are separate functions because consecutive output rows share source rows: at scale
// 1.2 row dy + 1's first source row is row dy's second one in 4 of 5 steps, so a thread that walks
// a run of consecutive rows (resize_run) keeps that row's four sums instead of forming them again.
// (a * b) >> 32 for 24-bit a, b: one v_mul_hi_u32_u24 (the masks tell the compiler the operand
// widths; both are no-ops on rs_vert's operands)
__device__ inline uint32_t mulhi_u24(uint32_t a, uint32_t b) {
    return (uint32_t)(((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)) >> 32);
}

// resize_run's divisions: n / d by v_rcp_f32 (1 ulp).  (n + 0.5) / d lies >= 0.5 / d from an integer
// and the product's error is below 3e-7 n / d, so the floor is exact for n < 10^6 (a full integer
// division costs ~20 VALU per thread; the runs need three per tile or level)
struct RcpDiv {
    __device__ int operator()(int n, int d) const {
        return (int)(((float)n + 0.5f) * __builtin_amdgcn_rcpf((float)d));
    }
};

// The horizontal half: the four sums 16 D of one source row r for one quad.
__device__ inline void rs_hsum(const uint8_t* r, int base, int4 sel, int4 cw, uint32_t D[4]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(r + (base & ~3));
    const uint32_t sh = (uint32_t)(base & 3);
    const uint32_t a0 = p[0], a1 = p[1], a2 = p[2];
    const uint32_t lo = __builtin_amdgcn_alignbyte(a1, a0, sh), hi = __builtin_amdgcn_alignbyte(a2, a1, sh);
    const int sl[4] = {sel.x, sel.y, sel.z, sel.w};
    const int cl[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        D[k] = __builtin_amdgcn_udot2(as_u16x2(__builtin_amdgcn_perm(hi, lo, (uint32_t)sl[k])),
                                      as_u16x2((uint32_t)cl[k]), 0u, false);
}

// The vertical half: the quad's four output bytes from the sums of its two source rows.
__device__ inline uint32_t rs_vert(const uint32_t D0[4], const uint32_t D1[4], int B0, int B1, int dx0, int simd_end) {
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = (mulhi_u24(D0[k] & 0x7FFF00u, (uint32_t)B0) + mulhi_u24(D1[k] & 0x7FFF00u, (uint32_t)B1) + 2u) >> 2;
    if (dx0 + 3 >= simd_end) {
        const unsigned b0 = (unsigned)B0 >> 8, b1 = (unsigned)B1 >> 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (dx0 + k >= simd_end) {
                // D < 2^19, b <= 2048: both 24-bit, products < 2^30 (full-rate multiplies)
                const uint32_t v = (__umul24(D0[k] >> 4, b0) + __umul24(D1[k] >> 4, b1) + (1u << 21)) >> 22;
                o[k] = v < 255u ? v : 255u;
            }
        }
    }
    return o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
}

// ---------------------------------------------------------------------------------------------
// k_blur: cv::GaussianBlur(Size(7,7), 2, 2, BORDER_REFLECT_101) on each level
// (ORBextractor_old.cc:1146-1147), bit-exact fixed point: kernel {18,34,48,56,48,34,18}/256,
// out = (sum_v w_v sum_h w_h p + 2^15) >> 16 with the horizontal sums exact (<= 65280, u16).
// Byte offset of (row y, column x) inside one plane: planes are < 16 M rows of < 16 MB pitch
// and < 2^32 bytes, so the row product is one full-rate 24-bit multiply (no 64-bit multiply
// per access).
__device__ inline size_t plane_off(int y, int pitch, int x) {
    uint32_t o;  // v_mad_u32_u24 kept as such (not re-associated into a 64-bit multiply-add)
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(o) : "v"(y), "v"(pitch), "v"(x));
    return (size_t)o;
}

__device__ inline int refl101(int p, int n) {
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - p - 2 : p;
}

// Horizontal 7-tap sums of 4 columns of two rows as u16 pairs (row a low, row b high), from the
// 12 window bytes of each row that start 1 byte before the first output's first tap (A[0] byte 1 =
// column x-3 of output 0): per row and output, the taps x-3 .. x as one byte window (v_alignbyte)
// times {18, 34, 48, 56} and x+1 .. x+3 times {48, 34, 18, 0}, two v_dot4_u32_u8 (sums <= 65280).
// 32 VALU per two rows of 4 columns (the u16-pair form with v_perm / v_pk_mad_u16 took 38).
__device__ inline void hsum_pair(const uint32_t A[3], const uint32_t B[3], uint32_t out[4]) {
    constexpr uint32_t W03 = 18u | (34u << 8) | (48u << 16) | (56u << 24);
    constexpr uint32_t W46 = 48u | (34u << 8) | (18u << 16);
    auto row = [&](const uint32_t* X, uint32_t h[4]) {
        const uint32_t lo[4] = {__builtin_amdgcn_alignbyte(X[1], X[0], 1), __builtin_amdgcn_alignbyte(X[1], X[0], 2),
                                __builtin_amdgcn_alignbyte(X[1], X[0], 3), X[1]};
        const uint32_t hi[4] = {__builtin_amdgcn_alignbyte(X[2], X[1], 1), __builtin_amdgcn_alignbyte(X[2], X[1], 2),
                                __builtin_amdgcn_alignbyte(X[2], X[1], 3), X[2]};
#pragma unroll
        for (int o = 0; o < 4; ++o)
            h[o] = __builtin_amdgcn_udot4(hi[o], W46, __builtin_amdgcn_udot4(lo[o], W03, 0u, false), false);
    };
    uint32_t ha[4], hb[4];
    row(A, ha);
    row(B, hb);
#pragma unroll
    for (int o = 0; o < 4; ++o) out[o] = ha[o] | (hb[o] << 16);
}

// Tile 128 x 32 outputs; the input window is rows ty0-4 .. ty0+35 (one spare row each side so
// rows pair up) x cols tx0-16 .. tx0+143, staged in LDS with 16-byte loads.
// Horizontal pass in "row-pair" u16x2 lanes: lane lo = row 2rp, lane hi = row 2rp+1 of the
// same column, 7 taps as two v_dot4_u32_u8 per row and column (hsum_pair).
// Vertical pass: each output row is 4 v_dot2_u32_u16 over row pairs with weight pairs
// {0,18}{34,48}{56,48}{34,18} (even rows) or {18,34}{48,56}{48,34}{18,0} (odd rows), the
// accumulator seeded with the 2^15 rounding term.

struct BlurTile {
    int l, ty0, tx0;
    const uint8_t* src;
    uint8_t* dst;
};

__device__ inline BlurTile blur_tile(const BatchArgs& a, int t) {
    BlurTile bt;
    const int img = a.img0 + t / a.total_tiles;
    int k = t % a.total_tiles;
    int l = 0;
    while (l + 1 < a.nlevels && k >= a.lv[l + 1].tile_first) ++l;
    const LevelGeom G = a.lv[l];
    k -= G.tile_first;
    bt.l = l;
    bt.ty0 = (k / G.tiles_x) * kBlurTH;
    bt.tx0 = (k % G.tiles_x) * kBlurTW;
    bt.src = a.lvl_base[l] + (long long)img * G.img_stride;
    bt.dst = a.blur_base[l] + (long long)img * G.bimg_stride;
    return bt;
}

// Window chunk i (16 bytes) of tile bt: rows reflected here (REFLECT_101), columns loaded as
// they are (bounds-checked buffer load; chunks left of the plane, or wholly beyond the 3 columns
// the taps reach past its right edge, are zero and not loaded) -- the few column bytes outside the
// plane that the taps reach are reflected in LDS afterwards (blur_tile_compute_mfma).
template <int kAux = 0>
__device__ inline uint4 blur_chunk(const BatchArgs& a, const BlurTile& bt, int i, int IWQ) {
    const LevelGeom G = a.lv[bt.l];
    const int r = i / IWQ, cq = i - r * IWQ;
    // rows beyond the reflected range feed only zero weights or unwritten outputs: clamp
    const int y = min(max(refl101(bt.ty0 + r - 4, G.h), 0), G.h - 1);
    const int x = bt.tx0 - 16 + 16 * cq;
    if (x < 0 || x >= G.w + 3) return make_uint4(0, 0, 0, 0);
    // the range covers the dword that holds the plane's last byte whatever the row pitch's
    // alignment (a dword that straddles the range's end reads as zero: the corner pixel of a level 0
    // whose size is no multiple of 4); every buffer has that much room behind its last image
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)bt.src, (short)0, (int)min(G.img_stride + 3, 0x7fffffffLL), 0x00020000);
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, y * G.pitch + x, 0, kAux);
    return make_uint4(v[0], v[1], v[2], v[3]);
}


// The same 128 x 32 blur tile as two int8 GEMMs on the matrix cores (v_mfma_i32_32x32x32_i8; the
// 7-tap kernel is banded, the zeros cost MFMA cycles that are otherwise idle, and the VALU keeps
// only the operand and result packing).  Wave w owns output columns 32w .. 32w+31 of the tile.
//   pass 1 (horizontal): D1[y][x] = sum_j (p[y][j] - 128) g[j - x - 13] over window columns
//     32w .. 32w+63 (two K-steps), rows 0..31 and 32..63 of the window (two M-blocks; rows past
//     the window's 40 read row 39 and only meet zero weights).  A = pixel rows straight from LDS
//     (16 bytes per lane, ^0x80 makes them int8), B = the constant band.
//   the pass-1 results (lane: column x, rows (g&3) + 8(g>>2) + 4h of the M-block) are split into
//     two int8 planes, hi = byte 1 and lo = byte 0 ^ 0x80 of D1, so D1 + 128 = 256 hi + lo + 256;
//     they are pass 2's A operand as they stand (lane = column x, its 16 rows = the K slots; the
//     constant B is laid out for exactly that row order).
//   pass 2 (vertical, transposed): D2[x][y'] = sum_y A2[x][y] g[y - y' - 1] -- lane = output
//     row y', its 16 registers = columns (g&3) + 8(g>>2) + 4h, i.e. four runs of 4 consecutive
//     bytes.  With S = the integer blur sum (sum of g = 256): 256 D2hi + D2lo = S - 2^23 - 2^15, so
//     the rounded output byte (S + 2^15) >> 16 is byte 2 of 256 D2hi + D2lo + 2^16 (which stays
//     in [-2^23, 2^23)) with bit 7 flipped.  The + 2^16 rides in K slot 4 of M-block 1 (a row >= 40
//     that no output reads) in both lane halves: A2hi = -1 there, B = -128, 2 x 128 into D2hi.
// Exact integer arithmetic throughout (no intermediate rounding), so bit-exact with the fixed-point
// filter the oracle restates (tests/test_blur_mfma_model.py replays the lane layouts on the CPU).
typedef int blur_v4i __attribute__((ext_vector_type(4)));
typedef int blur_v16i __attribute__((ext_vector_type(16)));
struct BlurMfmaTab {
    uint32_t b1[2][64][4];  // pass-1 B: [K-step s][lane (x = l & 31, h)], byte j: window column 32s + 16h + j
    uint32_t b2[2][64][4];  // pass-2 B: [M-block mb][lane (y' = l & 31, h)], byte g: window row of slot g
};
constexpr BlurMfmaTab make_blur_mfma_tab() {
    BlurMfmaTab t{};
    const int g7[7] = {18, 34, 48, 56, 48, 34, 18};
    for (int k = 0; k < 2; ++k)
        for (int l = 0; l < 64; ++l) {
            const int n = l & 31, h = l >> 5;
            for (int j = 0; j < 16; ++j) {
                const int d1 = 32 * k + 16 * h + j - (n + 13);                            // column tap
                const int rho = 32 * k + (j & 3) + 8 * (j >> 2) + 4 * h, d2 = rho - (n + 1);  // row tap
                const uint32_t w1 = d1 >= 0 && d1 < 7 ? (uint32_t)g7[d1] : 0u;
                uint32_t w2 = d2 >= 0 && d2 < 7 ? (uint32_t)g7[d2] : 0u;
                if (k == 1 && j == 4) w2 = 0x80u;  // -128: the + 2^16 slot (both halves h: 2 x 128)
                t.b1[k][l][j >> 2] |= w1 << (8 * (j & 3));
                t.b2[k][l][j >> 2] |= w2 << (8 * (j & 3));
            }
        }
    return t;
}
__constant__ BlurMfmaTab c_blur_mfma = make_blur_mfma_tab();

__device__ inline void blur_tile_compute_mfma(const LevelGeom& G, int tx0, int ty0, uint8_t* dst,
                                              uint4 (*tin4)[(kBlurTW + 32) / 16],
                                              uint4 (*hp)[kBlurTW / 4], int rlo, int rhi) {
    constexpr int IW = kBlurTW + 32, IH = kBlurTH + 8;
    static_assert(kBlurTW == 128 && kBlurTH == 32, "one 32-column strip per wave, one output block");
    constexpr int OP = kBlurTW + 4;  // output staging pitch: 33 dwords, conflict-free column writes
    if (tx0 == 0 || tx0 + kBlurTW + 3 > G.w) {  // REFLECT_101 of the 3 columns past each edge
        uint8_t* wb = reinterpret_cast<uint8_t*>(&tin4[0][0]);
        for (int i = threadIdx.x; i < IH * 6; i += 256) {
            const int r = i / 6, k = i - 6 * r;
            const int xx = k < 3 ? -1 - k : G.w + (k - 3);
            const int wx = xx - (tx0 - 16);
            if (wx >= 0 && wx < IW && (k < 3 ? tx0 == 0 : true)) {
                const int sx = refl101(xx, G.w) - (tx0 - 16);
                wb[r * IW + wx] = wb[r * IW + sx];
            }
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, h = lane >> 5;
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(&tin4[0][0]);
    // a strip that starts at or beyond the plane's right edge holds no pixel (a level's last tile
    // column: widths 533, 444, 370 fill 4.2, 3.5, 2.9 tiles): its wave skips both passes and the
    // staging writes -- the store loop below never reads those columns of ob (x >= G.w), and the
    // resize reads the raw window only -- and only joins the barriers
    uint32_t* ob = reinterpret_cast<uint32_t*>(&hp[0][0]);  // output staging; hp is free: callers sync before reusing it
    if (tx0 + 32 * w < G.w) {
        auto ldc = [&](const uint32_t* p) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            return blur_v4i{(int)v.x, (int)v.y, (int)v.z, (int)v.w};
        };
        const blur_v4i B1[2] = {ldc(c_blur_mfma.b1[0][lane]), ldc(c_blur_mfma.b1[1][lane])};
        const blur_v4i B2[2] = {ldc(c_blur_mfma.b2[0][lane]), ldc(c_blur_mfma.b2[1][lane])};
        blur_v4i hi[2], lo[2];
        const blur_v16i zero = {};
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const int row = min(32 * mb + n, IH - 1);
            const uint8_t* src = wb + row * IW + 32 * w + 16 * h;
            blur_v16i acc = zero;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + 32 * k);
                const blur_v4i a = {(int)(v.x ^ 0x80808080u), (int)(v.y ^ 0x80808080u), (int)(v.z ^ 0x80808080u),
                                    (int)(v.w ^ 0x80808080u)};
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, B1[k], acc, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (mb == 1 && q > 0) {  // rows >= 40: no output row reads them; slot 4 carries the + 2^16
                    hi[mb][q] = q == 1 ? 0x000000FF : 0;
                    lo[mb][q] = 0;
                    continue;
                }
                const uint32_t u0 = acc[4 * q], u1 = acc[4 * q + 1], u2 = acc[4 * q + 2], u3 = acc[4 * q + 3];
                hi[mb][q] = (int)(__builtin_amdgcn_perm(u1, u0, 0x0c0c0501u) | (__builtin_amdgcn_perm(u3, u2, 0x0c0c0501u) << 16));
                lo[mb][q] = (int)((__builtin_amdgcn_perm(u1, u0, 0x0c0c0400u) | (__builtin_amdgcn_perm(u3, u2, 0x0c0c0400u) << 16)) ^ 0x80808080u);
            }
        }
        blur_v16i ah = zero, al = zero;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(hi[mb], B2[mb], ah, 0, 0, 0);
            al = __builtin_amdgcn_mfma_i32_32x32x32_i8(lo[mb], B2[mb], al, 0, 0, 0);
        }
        // output row n: columns 32w + 8q + 4h .. +3 from registers 4q .. 4q+3, staged row-major in LDS
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t t4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t4[k] = ((uint32_t)ah[4 * q + k] << 8) + (uint32_t)al[4 * q + k];
            const uint32_t packed = (__builtin_amdgcn_perm(t4[1], t4[0], 0x0c0c0602u) |
                                     (__builtin_amdgcn_perm(t4[3], t4[2], 0x0c0c0602u) << 16)) ^ 0x80808080u;
            ob[n * (OP / 4) + 8 * w + 2 * q + h] = packed;
        }
    }
    __syncthreads();
    // stores as the VALU path: thread -> column quad cq, rows R rg .. R rg + R - 1
    constexpr int R = kBlurTH / 8;
    const int cq = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int x = tx0 + 4 * cq;
    const int ybase = ty0 + R * rg;
    const int ylo = max(rlo, ybase), yhi = x < G.w ? min(min(rhi, G.h), ybase + R) : ybase;
    const int olo = ylo - ybase, ohi = yhi - ybase;
    uint8_t* dbase = dst + plane_off(ybase, G.bpitch, x);
#pragma unroll
    for (int o = 0; o < R; ++o)
        if (o >= olo && o < ohi) *reinterpret_cast<uint32_t*>(dbase + o * G.bpitch) = ob[(R * rg + o) * (OP / 4) + cq];
}

// Persistent over the tiles of the launch (images x levels x tiles): the next tile's window
// is loaded into registers while the current one is filtered, so the global-memory round
// trip is hidden behind the arithmetic of the previous tile.
__global__ __launch_bounds__(256) void k_blur(BatchArgs a, int tile0, int ntile) {
    constexpr int IW = kBlurTW + 32, IH = kBlurTH + 8, IWQ = IW / 16, NRP = IH / 2;
    constexpr int NCH = (IH * IWQ + 255) / 256;  // window chunks per thread
    __shared__ uint4 tin4[IH][IWQ];
    __shared__ uint4 hp[NRP][kBlurTW / 4];  // [row pair][column quad]: 4 columns x (row0,row1)
    // tiles [tile0, tile0 + ntile) of every image (all levels: 0, total_tiles)
    auto tile_of = [&](int t) { return (t / ntile) * a.total_tiles + tile0 + t % ntile; };
    const int total = ntile * a.nimages;
    // a contiguous run of tiles per workgroup, runs placed XCD-contiguously (xcd_remap)
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int t_end = (int)((long long)(lb + 1) * total / gridDim.x);
    int t = (int)((long long)lb * total / gridDim.x);
    if (t >= t_end) return;
    BlurTile bt = blur_tile(a, tile_of(t));
    uint4 pre[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = threadIdx.x + 256 * c;
        if (i < IH * IWQ) pre[c] = blur_chunk(a, bt, i, IWQ);
    }
    for (; t < t_end; ++t) {
        const BlurTile cur = bt;
        const LevelGeom G = a.lv[cur.l];
        const int ty0 = cur.ty0, tx0 = cur.tx0;
        uint8_t* dst = cur.dst;
        __syncthreads();  // the previous tile's passes are done with tin4 / hp
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = threadIdx.x + 256 * c;
            if (i < IH * IWQ) (&tin4[0][0])[i] = pre[c];
        }
        const int tn = t + 1;
        if (tn < t_end) {  // prefetch the next window
            bt = blur_tile(a, tile_of(tn));
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int i = threadIdx.x + 256 * c;
                if (i < IH * IWQ) pre[c] = blur_chunk(a, bt, i, IWQ);
            }
        }
        __syncthreads();
        blur_tile_compute_mfma(G, tx0, ty0, dst, tin4, hp, 0, G.h);
    }
}

hipError_t launch_blur_level(const BatchArgs& a, int l, hipStream_t s) {
    const LevelGeom G = a.lv[l];
    const int n = G.tiles_x * G.tiles_y;
    hipLaunchKernelGGL(k_blur, dim3(std::min(n * a.nimages, 8192)), dim3(256), 0, s, a, G.tile_first, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_blur_resize: one read of level l - 1 serves two stages.  A workgroup stages the 128 x 32
// blur tile's window of level l - 1 (rows ty0-4 .. ty0+35, columns tx0-16 .. tx0+143, 16-byte
// buffer loads, REFLECT_101 rows) once, filters it (GaussianBlur of level l - 1, :1146-1147) and
// makes the level-l outputs whose first source row / column fall inside the tile (cv::resize of
// ComputePyramid, :1342-1344; exact-2x levels by INTER_AREA): their taps (source rows <= ty0+32,
// columns <= tx0+134 for scales <= 2) all lie in the window's real pixels, so level l needs no
// second read of level l - 1 and the blur of level l - 1 none of its own.  Ownership tables
// (band_row / tile_quad) come from the host with the resize coefficients.
static_assert(kBrMaxQuads >= kBlurTW / 4 + 1 && kBrMaxRows >= kBlurTH + 1, "ownership caps");
static_assert(kBrMaxQuads <= 64 && kBrMaxRows <= 64, "br_tile copies each table with one wave");

struct BrSmem {
    uint4 tin4[kBlurTH + 8][(kBlurTW + 32) / 16];
    uint4 hp[(kBlurTH + 8) / 2][kBlurTW / 4];
    // per owned output quad (rs_hsum): tap selectors, coefficient pairs, first left tap; one
    // array per field so a wave's consecutive quads read consecutive entries
    int4 xsel[kBrMaxQuads];
    int4 xcw[kBrMaxQuads];
    int xbase[kBrMaxQuads];
    int4 yts[kBrMaxRows];
};

// Blur tile k of level s = l - 1 of image img, and (resize) the level-l outputs it owns.  kAux:
// cache policy of the window loads (sc1 where level s was written by this launch).
template <int kAux>
__device__ inline void br_tile(const BatchArgs& a, int l, bool resize, int img, int by, int bx, BrSmem& sm) {
    constexpr int IW = kBlurTW + 32, IH = kBlurTH + 8, IWQ = IW / 16;
    constexpr int NCH = (IH * IWQ + 255) / 256;
    const LevelGeom S = a.lv[l - 1];
    const LevelGeom G = a.lv[resize ? l : l - 1];
    BlurTile bt;
    bt.l = l - 1;
    bt.ty0 = by * kBlurTH;
    bt.tx0 = bx * kBlurTW;
    bt.src = a.lvl_base[l - 1] + (long long)img * S.img_stride;
    bt.dst = a.blur_base[l - 1] + (long long)img * S.bimg_stride;
    uint4 pre[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = threadIdx.x + 256 * c;
        if (i < IH * IWQ) pre[c] = blur_chunk<kAux>(a, bt, i, IWQ);
    }
    // the level-l outputs this tile owns, and their coefficients
    int r0 = 0, nr = 0, q0 = 0, nq = 0;
    if (resize) {
        const int* band_row = reinterpret_cast<const int*>(a.rtab) + G.band_row_off;
        const int* tile_quad = reinterpret_cast<const int*>(a.rtab) + G.tile_quad_off;
        r0 = band_row[by];
        q0 = tile_quad[bx];
        nr = min(band_row[by + 1] - r0, kBrMaxRows);
        nq = min(tile_quad[bx + 1] - q0, kBrMaxQuads);
        if (!G.area2) {
            // the host's finished records (orb_geometry.h resize_level), copied as they are: one
            // field per wave, so no wave carries more than one load and one LDS store to the barrier
            const int f = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), i = threadIdx.x & 63;
            if (f < 2) {
                if (i < nq) (f ? sm.xcw : sm.xsel)[i] = a.rtab[G.qrec_off + 2 * (q0 + i) + f];
            } else if (f == 2) {
                if (i < nq) sm.xbase[i] = reinterpret_cast<const int*>(a.rtab)[G.qbase_off + q0 + i];
            } else if (i < nr) {
                sm.yts[i] = a.rtab[G.yrec_off + r0 + i];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int i = threadIdx.x + 256 * c;
        if (i < IH * IWQ) (&sm.tin4[0][0])[i] = pre[c];
    }
    __syncthreads();
    blur_tile_compute_mfma(S, bt.tx0, bt.ty0, bt.dst, sm.tin4, sm.hp, 0, S.h);  // fixes only off-plane columns
    if (!resize) return;
    // resize from the window: window row r = source row ty0 - 4 + r, column c = tx0 - 16 + c
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(&sm.tin4[0][0]);
    const int wy0 = bt.ty0 - 4, wx0 = bt.tx0 - 16;
    uint8_t* dst = a.lvl_base[l] + (long long)img * G.img_stride;
    // thread -> (quad q, the run of consecutive owned rows [row0, row1)) (resize_run): the quad's
    // selectors and coefficients are read once per tile, and inside the run a source row that two
    // output rows share has its sums formed once
    if (nq <= 0) return;
    const ResizeRun run = resize_run((int)threadIdx.x, nq, nr, 256, RcpDiv{});
    const int q = run.q;
    const int dx0 = 4 * (q0 + q);
    if (G.area2) {
        for (int rr = run.row0; rr < run.row1; ++rr) {
            const int dy = r0 + rr;
            const uint8_t* s0 = wb + __mul24(2 * dy - wy0, IW) - wx0;
            const uint8_t* s1 = s0 + IW;
            uint32_t packed = 0;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int dx = min(dx0 + kk, G.w - 1);
                const int o = (s0[2 * dx] + s0[2 * dx + 1] + s1[2 * dx] + s1[2 * dx + 1] + 2) >> 2;
                packed |= (uint32_t)o << (8 * kk);
            }
            *reinterpret_cast<uint32_t*>(dst + plane_off(dy, G.pitch, dx0)) = packed;
        }
    } else {
        if (run.row0 >= run.row1) return;
        const int4 xsel = sm.xsel[q], xcw = sm.xcw[q];
        const int xbase = sm.xbase[q];
        const int woff = -__mul24(wy0, IW) - wx0;  // window byte offset of source (row 0, column 0)
        int carried = -1;  // the source row whose sums the previous output row left behind
        // one output row: F holds the first source row's sums (the previous row's S when that row
        // is carried), S takes the second one's; two steps per trip with the sets swapped, so the
        // carried sums never move between registers
        auto step = [&](uint32_t (&F)[4], uint32_t (&S)[4], int rr) {
            const int4 yt = sm.yts[rr];
            if (!resize_row_carried(carried, yt.x)) rs_hsum(wb + (woff + __mul24(yt.x, IW)), xbase, xsel, xcw, F);
            rs_hsum(wb + (woff + __mul24(yt.y, IW)), xbase, xsel, xcw, S);
            carried = yt.y;
            *reinterpret_cast<uint32_t*>(dst + plane_off(r0 + rr, G.pitch, dx0)) = rs_vert(F, S, yt.z, yt.w, dx0, G.simd_end);
        };
        uint32_t Da[4], Db[4];
        for (int rr = run.row0;;) {
            step(Da, Db, rr);
            if (++rr >= run.row1) break;
            step(Db, Da, rr);
            if (++rr >= run.row1) break;
        }
    }
}

// n / d for a launch constant d by a mul-high with the host's magic ceil(2^32 / d) (d >= 2;
// magic 0 stands for d == 1); exact for 0 <= n < 2^32 / d
__device__ inline int div_magic(int n, uint32_t magic) {
    return magic ? (int)__umulhi((uint32_t)n, magic) : n;
}

__global__ __launch_bounds__(256) void k_blur_resize(BatchArgs a, int l, uint32_t per_magic, uint32_t tx_magic) {
    __shared__ BrSmem sm;
    const LevelGeom S = a.lv[l - 1];
    const int per = S.tiles_x * S.tiles_y;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);  // an image's tiles on one XCD
    const int irel = div_magic(wg, per_magic);
    const int k = wg - irel * per;
    const int by = div_magic(k, tx_magic), bx = k - by * S.tiles_x;
    br_tile<0>(a, l, true, a.img0 + irel, by, bx, sm);
}


// k_level_linear: level l from level l - 1 in HBM for any scale step (ComputePyramid's cv::resize
// INTER_LINEAR, ORBextractor_old.cc:1342-1344; the generic 2-tap path of OpenCV 4.2's resize, as
// oracle/orb_oracle.cpp resize_linear restates it).  k_blur_resize stages one blur tile of level
// l - 1 and makes the outputs whose taps it holds, which needs scale steps <= 2 (rs_hsum reads the
// 8 source bytes from a quad's first tap); scale factors above 2 (accepted by ORBextractor, not
// used by ORB-SLAM3's configurations) take this kernel and then k_blur per level.  Thread = one
// output quad of one row; every tap is a byte load from the previous level.
__global__ __launch_bounds__(256) void k_level_linear(BatchArgs a, int l) {
    const LevelGeom G = a.lv[l], S = a.lv[l - 1];
    const int nq = (G.w + 3) >> 2;
    const int item = blockIdx.x * 256 + threadIdx.x;
    if (item >= nq * G.h) return;
    const int img = a.img0 + blockIdx.y;
    const int dy = item / nq, q = item - dy * nq;
    const uint8_t* src = a.lvl_base[l - 1] + (long long)img * S.img_stride;
    uint8_t* dst = a.lvl_base[l] + (long long)img * G.img_stride;
    const int4 yt = a.rtab[G.ytab_off + dy];  // (sy0, sy1, b0, b1), rows clamped
    const uint8_t* r0 = src + plane_off(yt.x, S.pitch, 0);
    const uint8_t* r1 = src + plane_off(yt.y, S.pitch, 0);
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dx = min(4 * q + k, G.w - 1);
        const int4 xt = a.rtab[G.xtab_off + dx];  // (sx0, sx1, a0, a1), a1 = 0 past the last pair
        const int d0 = r0[xt.x] * xt.z + r0[xt.y] * xt.w;
        const int d1 = r1[xt.x] * xt.z + r1[xt.y] * xt.w;
        int o;
        if (dx < G.simd_end) {  // VResizeLinearVec_32s8u: v_mul_hi of the packed (D >> 4), v_rshr_pack_u<2>
            const int t0 = min(d0 >> 4, 32767), t1 = min(d1 >> 4, 32767);
            const int sum = min(max(((t0 * yt.z) >> 16) + ((t1 * yt.w) >> 16), -32768), 32767);
            o = (sum + 2) >> 2;
        } else {  // FixedPtCast<int, uchar, 22>
            o = (d0 * yt.z + d1 * yt.w + (1 << 21)) >> 22;
        }
        packed |= (uint32_t)min(max(o, 0), 255) << (8 * k);
    }
    *reinterpret_cast<uint32_t*>(dst + plane_off(dy, G.pitch, 4 * q)) = packed;
}

hipError_t launch_level_linear(const BatchArgs& a, int l, hipStream_t s) {
    const LevelGeom G = a.lv[l];
    const int items = ((G.w + 3) >> 2) * G.h;
    hipLaunchKernelGGL(k_level_linear, dim3((items + 255) / 256, a.nimages), dim3(256), 0, s, a, l);
    return hipGetLastError();
}

hipError_t launch_blur_resize(const BatchArgs& a, int l, hipStream_t s) {
    const LevelGeom S = a.lv[l - 1];
    auto magic = [](uint32_t d) { return d > 1 ? 0xFFFFFFFFu / d + 1u : 0u; };  // exact for n < 2^32 / d
    hipLaunchKernelGGL(k_blur_resize, dim3(S.tiles_x * S.tiles_y * a.nimages), dim3(256), 0, s, a, l,
                       magic((uint32_t)(S.tiles_x * S.tiles_y)), magic((uint32_t)S.tiles_x));
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// k_pyr_tail: the small levels of the pyramid in ONE launch, one 1024-thread workgroup per image.
// Level s0 = tail0 - 1 (made by the last k_blur_resize) is loaded into LDS once; then for
// s = s0 .. L-1 the workgroup writes level s's blur (GaussianBlur 7x7, :1146-1147) and makes level
// s + 1 (cv::resize INTER_LINEAR / exact-2x INTER_AREA, :1342-1344) from the LDS copy into the
// other LDS buffer and to HBM.  Each of these levels took its own launch of a few thousand
// 128 x 32 tiles before, and every such launch was latency-bound (level 7: 32 us per 512 images
// for 24 K pixels per image).  Two buffers alternate (level s0 + 2k in buffer 0, s0 + 2k + 1 in
// buffer 1; each level is smaller than the one two steps before).  Row pitch Pitch(l) holds kTailPad
// bytes on the left (REFLECT_101 columns -3 .. -1) and >= 12 on the right (resize reads 12
// bytes from a quad's first tap), so the blur and rs_hsum read the same window layout as k_blur.
constexpr int kTailThreads = 1024;

__device__ inline void tail_fill_pads(uint8_t* buf, int P, int w, int h) {
    for (int i = threadIdx.x; i < h * 6; i += kTailThreads) {
        const int y = i / 6, k = i - 6 * y;
        uint8_t* row = buf + __mul24(y, P) + kTailPad;
        if (k < 3) row[-1 - k] = row[1 + k];          // columns -1, -2, -3 <- 1, 2, 3
        else row[w + k - 3] = row[w - 2 - (k - 3)];    // columns w, w+1, w+2 <- w-2, w-3, w-4
    }
}

// Horizontal 7-tap sums of the 4 columns 4cq .. 4cq+3 of two LDS rows as u16 pairs (row a, row b):
// hsum_pair, as blur_tile_compute (window bytes 4cq+12 .. 4cq+23).
__device__ inline void tail_hpair(const uint8_t* ra, const uint8_t* rb, int cq, uint32_t out[4]) {
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(ra) + cq + 3;
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(rb) + cq + 3;
    uint32_t A[3], B[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        A[d] = pa[d];
        B[d] = pb[d];
    }
    hsum_pair(A, B, out);
}

// Blur of one LDS-resident level.  Task = (column quad, segment of R rows), with the segment
// count chosen so the workgroup's 1024 threads get one task each where the level allows; a task
// slides down its rows with the last five row pairs in registers, so every row's horizontal sums
// are formed once (plus four pairs of prologue).  Row pair j of a task covers rows
// y0-4+2j, y0-3+2j (REFLECT_101 by index); output rows y0+2m / y0+2m+1 take pairs m .. m+3 with the
// even weights / m+1 .. m+4 with the odd ones (blur_tile_compute's vertical pass).
__device__ inline void tail_blur(const uint8_t* buf, int P, const LevelGeom& G, uint8_t* dst) {
    const int nq = (G.w + 3) >> 2;
    const int per = kTailThreads / nq > 0 ? kTailThreads / nq : 1;  // segments per column
    int R = (G.h + per - 1) / per;
    R = (R + 1) & ~1;
    const int nseg = (G.h + R - 1) / R;
    const u16x2 WE[4] = {as_u16x2(0u | (18u << 16)), as_u16x2(34u | (48u << 16)),
                         as_u16x2(56u | (48u << 16)), as_u16x2(34u | (18u << 16))};
    const u16x2 WO[4] = {as_u16x2(18u | (34u << 16)), as_u16x2(48u | (56u << 16)),
                         as_u16x2(48u | (34u << 16)), as_u16x2(18u | (0u << 16))};
    // REFLECT_101 of rows -4 .. h + 4 as min(|y|, 2h - 2 - |y|): one reflection suffices, every
    // level has >= 2 kEdge + 4 rows (the host's level check); rows >= 0 skip the |y|
    const int h2 = 2 * G.h - 2;
    auto row = [&](int y) {
        const int ay = max(y, -y);
        return buf + __mul24(min(ay, h2 - ay), P);
    };
    auto row_lo = [&](int y) { return buf + __mul24(min(y, h2 - y), P); };
    for (int t0 = 0; t0 < nq * nseg; t0 += kTailThreads) {
        const int t = t0 + (int)threadIdx.x;
        const int sg = t / nq, cq = t - sg * nq;  // one division per task
        if (sg >= nseg) break;
        const int y0 = sg * R, y1 = min(y0 + R, G.h);
        // the last five row pairs' sums in five register sets, the loop unrolled by five so that
        // each step names them in rotated order (no register moves between rows)
        uint32_t V0[4], V1[4], V2[4], V3[4], V4[4];
        tail_hpair(row(y0 - 4), row(y0 - 3), cq, V0);
        tail_hpair(row(y0 - 2), row(y0 - 1), cq, V1);
        tail_hpair(row(y0), row(y0 + 1), cq, V2);
        tail_hpair(row(y0 + 2), row(y0 + 3), cq, V3);
        uint8_t* d = dst + plane_off(y0, G.bpitch, 4 * cq);
        using Pair4 = uint32_t[4];
        // output row from pairs p0 .. p3 (weights W): 4 columns, bytes 2 of the sums
        auto vsum = [&](const Pair4& p0, const Pair4& p1, const Pair4& p2, const Pair4& p3, const u16x2* W) {
            uint32_t sv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t acc = 1u << 15;
                acc = __builtin_amdgcn_udot2(as_u16x2(p0[c]), W[0], acc, false);
                acc = __builtin_amdgcn_udot2(as_u16x2(p1[c]), W[1], acc, false);
                acc = __builtin_amdgcn_udot2(as_u16x2(p2[c]), W[2], acc, false);
                acc = __builtin_amdgcn_udot2(as_u16x2(p3[c]), W[3], acc, false);
                sv[c] = acc;
            }
            return __builtin_amdgcn_perm(sv[1], sv[0], 0x0c0c0602u) | __builtin_amdgcn_perm(sv[3], sv[2], 0x06020c0cu);
        };
        // rows y, y + 1 from pairs m .. m + 3 (even weights) and m + 1 .. m + 4 (odd), pair m + 4
        // (rows y + 4, y + 5) loaded into n
        auto step = [&](const Pair4& a, const Pair4& b, const Pair4& c, const Pair4& e, Pair4& n, int y) {
            tail_hpair(row_lo(y + 4), row_lo(y + 5), cq, n);
            *reinterpret_cast<uint32_t*>(d) = vsum(a, b, c, e, WE);
            if (y + 1 < y1) *reinterpret_cast<uint32_t*>(d + G.bpitch) = vsum(b, c, e, n, WO);
            d += 2 * G.bpitch;
        };
        for (int y = y0;;) {  // y0 < y1: at least one step
            step(V0, V1, V2, V3, V4, y);
            if ((y += 2) >= y1) break;
            step(V1, V2, V3, V4, V0, y);
            if ((y += 2) >= y1) break;
            step(V2, V3, V4, V0, V1, y);
            if ((y += 2) >= y1) break;
            step(V3, V4, V0, V1, V2, y);
            if ((y += 2) >= y1) break;
            step(V4, V0, V1, V2, V3, y);
            if ((y += 2) >= y1) break;
        }
    }
}

__global__ __launch_bounds__(kTailThreads) void k_pyr_tail(BatchArgs a) {
    extern __shared__ uint4 tail_lds[];
    uint8_t* lds = reinterpret_cast<uint8_t*>(tail_lds);
    const int img = a.img0 + blockIdx.x;
    const int s0 = a.tail0 - 1, L = a.nlevels;
    // buffers as offsets from the LDS base (an array of pointers would decay to generic
    // pointers: flat accesses, which fault on the 4-byte-aligned 12-byte row reads)
    auto buf = [&](int k) { return lds + (k ? a.tail_buf1 : 0); };
    int4* xsel = reinterpret_cast<int4*>(lds + a.tail_tab);
    int4* xcw = xsel + a.tail_maxq;
    int4* yts = xcw + a.tail_maxq;
    int* xbase = reinterpret_cast<int*>(yts + a.tail_maxrows);
    {   // level s0 from HBM (16-byte loads, 16-byte aligned LDS rows)
        const LevelGeom S = a.lv[s0];
        const uint8_t* src = a.lvl_base[s0] + (long long)img * S.img_stride;
        const int nch = (S.w + 15) >> 4, P = S.tpitch;
        for (int i = threadIdx.x; i < nch * S.h; i += kTailThreads) {
            const int y = i / nch, c = i - y * nch;
            *reinterpret_cast<uint4*>(buf(0) + __mul24(y, P) + kTailPad + 16 * c) =
                *reinterpret_cast<const uint4*>(src + plane_off(y, S.pitch, 16 * c));
        }
        __syncthreads();
        tail_fill_pads(buf(0), P, S.w, S.h);
        __syncthreads();
    }
    for (int s = s0; s < L; ++s) {
        const LevelGeom S = a.lv[s];
        const uint8_t* cur = buf((s - s0) & 1);
        const bool resize = s + 1 < L;
        const LevelGeom G = a.lv[resize ? s + 1 : s];
        const int nq = (G.w + 3) >> 2;
        if (resize && !G.area2) {  // level s + 1's quad and row coefficients (as br_tile)
            // the host's finished records, copied as they are: the x fields from the workgroup's
            // first threads, the rows from its last ones (other waves: they overlap)
            for (int i = threadIdx.x; i < 2 * nq; i += kTailThreads) {
                const int q = i >> 1;
                ((i & 1) ? xcw : xsel)[q] = a.rtab[G.qrec_off + i];
                if (!(i & 1)) xbase[q] = reinterpret_cast<const int*>(a.rtab)[G.qbase_off + q];
            }
            for (int r = kTailThreads - 1 - (int)threadIdx.x; r < G.h; r += kTailThreads) yts[r] = a.rtab[G.yrec_off + r];
        }
        tail_blur(cur, S.tpitch, S, a.blur_base[s] + (long long)img * S.bimg_stride);
        if (!resize) break;
        __syncthreads();  // coefficient tables
        uint8_t* nxt = buf((s + 1 - s0) & 1);
        uint8_t* dst = a.lvl_base[s + 1] + (long long)img * G.img_stride;
        const uint8_t* rowp = cur + kTailPad;
        // thread -> (quad q, the run of consecutive rows [row0, row1)) as br_tile (resize_run)
        const ResizeRun run = resize_run((int)threadIdx.x, nq, G.h, kTailThreads, RcpDiv{});
        const int q = run.q, dx0 = 4 * q;
        auto put = [&](int dy, uint32_t packed) {
            *reinterpret_cast<uint32_t*>(nxt + __mul24(dy, G.tpitch) + kTailPad + dx0) = packed;
            *reinterpret_cast<uint32_t*>(dst + plane_off(dy, G.pitch, dx0)) = packed;
        };
        if (G.area2) {
            for (int dy = run.row0; dy < run.row1; ++dy) {
                const uint8_t* s0r = rowp + __mul24(2 * dy, S.tpitch);
                const uint8_t* s1r = s0r + S.tpitch;
                uint32_t packed = 0;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int dx = min(dx0 + kk, G.w - 1);
                    const int o = (s0r[2 * dx] + s0r[2 * dx + 1] + s1r[2 * dx] + s1r[2 * dx + 1] + 2) >> 2;
                    packed |= (uint32_t)o << (8 * kk);
                }
                put(dy, packed);
            }
        } else if (run.row0 < run.row1) {
            const int4 qsel = xsel[q], qcw = xcw[q];
            const int qbase = xbase[q];
            int carried = -1;
            auto step = [&](uint32_t (&F)[4], uint32_t (&Sn)[4], int dy) {  // br_tile's step
                const int4 yt = yts[dy];
                if (!resize_row_carried(carried, yt.x)) rs_hsum(rowp + __mul24(yt.x, S.tpitch), qbase, qsel, qcw, F);
                rs_hsum(rowp + __mul24(yt.y, S.tpitch), qbase, qsel, qcw, Sn);
                carried = yt.y;
                put(dy, rs_vert(F, Sn, yt.z, yt.w, dx0, G.simd_end));
            };
            uint32_t Da[4], Db[4];
            for (int dy = run.row0;;) {
                step(Da, Db, dy);
                if (++dy >= run.row1) break;
                step(Db, Da, dy);
                if (++dy >= run.row1) break;
            }
        }
        __syncthreads();  // level s + 1 complete in LDS; level s's buffer and the tables are free
        tail_fill_pads(nxt, G.tpitch, G.w, G.h);
        __syncthreads();
    }
}

hipError_t launch_pyr_tail(const BatchArgs& a, hipStream_t s) {
    // the dynamic-LDS limit is raised once per size and device (see launch_octree, orb_octree.hip)
    constexpr int kMaxDevices = 64;
    static std::atomic<int> lds_set[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = kMaxDevices - 1;
    if (a.tail_lds > 65536 && a.tail_lds > lds_set[dev].load()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pyr_tail),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, a.tail_lds);
        if (e != hipSuccess) return e;
        int cur = lds_set[dev].load();
        while (a.tail_lds > cur && !lds_set[dev].compare_exchange_weak(cur, a.tail_lds)) {}
    }
    hipLaunchKernelGGL(k_pyr_tail, dim3(a.nimages), dim3(kTailThreads), a.tail_lds, s, a);
    return hipGetLastError();
}

}  // namespace orbgpu
