// host_harness.hip -- TEST INFRASTRUCTURE: runs the device algorithm headers of the product
// (orb_octree.h, orb_fast_cell.h, orb_introsort.h, orb_math.h) on the host with SerialPolicy, and
// the runtime's geometry planner (orb_geometry.h) and the matchers' buffer layout (orb_layout.h), so
// they can be checked against the CPU oracle without a GPU.  Not part of liborbgpu.so.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../orbslam3lib_amd/csrc/orb_fast_cell.h"
#include "../../orbslam3lib_amd/csrc/orb_geometry.h"
#include "../../orbslam3lib_amd/csrc/orb_introsort.h"
#include "../../orbslam3lib_amd/csrc/orb_layout.h"
#include "../../orbslam3lib_amd/csrc/orb_math.h"
#include "../../orbslam3lib_amd/csrc/orb_octree.h"
#include "../../orbslam3lib_amd/csrc/orb_policy.h"

using namespace orbgpu;

// node state is read and written as 16-byte records (orb_octree.h on_ld / on_st)
static uint8_t* align16(uint8_t* p) { return (uint8_t*)(((uintptr_t)p + 15) & ~(uintptr_t)15); }

extern "C" {

// libm_sincosf (orb_math.h) against the host's own sinf / cosf on every `stride`-th float of
// [lo, hi): returns the number of mismatching values (sin or cos), *checked = floats visited.
long long harness_libm_sincosf_mismatches(float lo, float hi, int stride, long long* checked) {
    uint32_t u = __builtin_bit_cast(uint32_t, lo);
    const uint32_t end = __builtin_bit_cast(uint32_t, hi);
    long long bad = 0, n = 0;
    for (; u < end; u += (uint32_t)stride) {
        volatile float y = __builtin_bit_cast(float, u);
        const float c = cosf(y), s = sinf(y);
        float ms, mc;
        libm_sincosf(y, &ms, &mc);
        bad += (__builtin_bit_cast(uint32_t, c) != __builtin_bit_cast(uint32_t, mc)) ||
               (__builtin_bit_cast(uint32_t, s) != __builtin_bit_cast(uint32_t, ms));
        ++n;
    }
    if (checked) *checked = n;
    return bad;
}

// libm_atanf / libm_tanf (orb_math.h) against the host's atanf / tanf on every `stride`-th float
// of [lo, hi) (lo >= 0, or both negative: floats are walked by bit pattern).
long long harness_libm_atanf_tanf_mismatches(float lo, float hi, int stride, int which, long long* checked) {
    uint32_t u = __builtin_bit_cast(uint32_t, lo);
    const uint32_t end = __builtin_bit_cast(uint32_t, hi);
    long long bad = 0, n = 0;
    for (; u < end; u += (uint32_t)stride) {
        volatile float y = __builtin_bit_cast(float, u);
        const float ref = which ? tanf(y) : atanf(y);
        const float got = which ? libm_tanf(y) : libm_atanf(y);
        bad += __builtin_bit_cast(uint32_t, ref) != __builtin_bit_cast(uint32_t, got);
        ++n;
    }
    if (checked) *checked = n;
    return bad;
}

// libm_atan2f against the host's atan2f on n pseudo-random pairs (xorshift from seed): raw bit
// patterns, [-3, 3]^2 and the |y| ~ |x| band, one quarter each.
long long harness_libm_atan2f_random(long long n, unsigned long long seed) {
    unsigned long long s = seed | 1;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)s;
    };
    long long bad = 0;
    for (long long i = 0; i < n; ++i) {
        const uint32_t a = rnd(), b = rnd();
        float y, x;
        switch (i & 3) {
            case 0: y = __builtin_bit_cast(float, a); x = __builtin_bit_cast(float, b); break;
            case 1: y = (float)(int32_t)a / 2147483648.0f * 3.0f; x = (float)(int32_t)b / 2147483648.0f * 3.0f; break;
            case 2: y = __builtin_bit_cast(float, a & 0x3fffffffu); x = __builtin_bit_cast(float, b & 0x3fffffffu) * ((b >> 31) ? -1.f : 1.f); break;
            default:
                y = __builtin_bit_cast(float, 0x3f000000u + (a & 0x00ffffffu));
                x = y * (0.5f + (float)(b & 0xffff) / 65536.0f) * ((a >> 31) ? -1.f : 1.f);
        }
        volatile float vy = y, vx = x;
        const float ref = atan2f(vy, vx), got = libm_atan2f(vy, vx);
        bad += __builtin_bit_cast(uint32_t, ref) != __builtin_bit_cast(uint32_t, got) && !(ref != ref && got != got);
    }
    return bad;
}

int harness_octree(const uint32_t* keys, int n, int W, int H, int N, uint32_t* out, int out_cap) {
    const int nIni = std::max(1, (int)std::round((float)W / (float)H));
    const int cap = std::max(N + 3, 4 * nIni) + 8;
    std::vector<uint16_t> nq(n + 1);
    std::vector<uint8_t> mem(oct_nodemem_bytes(cap) + 64);
    OctWST<kGeneric, kGeneric> w;
    w.keys = const_cast<uint32_t*>(keys);  // read-only without a cell gather
    w.n = n;
    w.nq = nq.data();
    w.cell_off = nullptr;
    w.cellkeys = nullptr;
    w.ncells = 0;
    w.cell_cap = 0;
    w.m = oct_nodemem_carve<kGeneric>(align16(mem.data()), cap);
    w.cap = cap;
    w.out_keys = out;
    w.out_cap = out_cap;
    w.dbg = nullptr;
    w.pyr = nullptr;
    w.pyrD = 0;
    w.xcode = w.ycode = nullptr;
    OctShared sh;
    SerialPolicy p;
    return octree_distribute(p, w, &sh, W, H, N);
}

// The count-pyramid formulation with a pyramid of depth D (orb_octree.h), rerun with the label
// passes when a node below depth D must be divided, as the kernel does.  *deep = 1 when it was.
// ncells > 0: the keys arrive as per-cell lists (cell c holds counts[c] keys at cells[c * cap]),
// the kernel's layout, so the cell search and the pyramid's cell-slot key names are exercised.
int harness_octree_cells(const uint32_t* cells, const int32_t* counts, int ncells, int cap, int W, int H, int N,
                         uint32_t* out, int out_cap, int D, int* deep) {
    const int nIni = oct_nini(W, H);
    const int ocap = std::max(N + 3, 4 * nIni) + 8;
    std::vector<int32_t> off(ncells + 1, 0);
    for (int c = 0; c < ncells; ++c) off[c + 1] = off[c] + counts[c];
    const int n = off[ncells];
    std::vector<uint32_t> keys(n + 1);
    std::vector<uint16_t> nq(n + 1);
    std::vector<uint8_t> mem(oct_nodemem_bytes(ocap) + 64);
    std::vector<uint32_t> pyr(oct_pyr_bytes(D, nIni) / 4 + 1);
    std::vector<uint16_t> tbl(W + H + 2);
    OctWST<kGeneric, kGeneric> w;
    w.keys = keys.data();
    w.n = n;
    w.nq = nq.data();
    w.cell_off = off.data();
    w.cellkeys = cells;
    w.ncells = ncells;
    w.cell_cap = cap;
    w.m = oct_nodemem_carve<kGeneric>(align16(mem.data()), ocap);
    w.cap = ocap;
    w.out_keys = out;
    w.out_cap = out_cap;
    w.dbg = nullptr;
    w.pyr = pyr.data();
    w.pyrD = D;
    w.xcode = tbl.data();
    w.ycode = tbl.data() + W + 1;
    OctShared sh;
    SerialPolicy p;
    int r = octree_distribute(p, w, &sh, W, H, N);
    *deep = r == kOctDeep;
    if (r == kOctDeep) {
        w.pyrD = 0;
        r = octree_distribute(p, w, &sh, W, H, N);
    }
    return r;
}

int harness_octree_pyr(const uint32_t* keys, int n, int W, int H, int N, uint32_t* out, int out_cap, int D,
                       int* deep) {
    const int nIni = oct_nini(W, H);
    const int cap = std::max(N + 3, 4 * nIni) + 8;
    std::vector<uint16_t> nq(n + 1);
    std::vector<uint8_t> mem(oct_nodemem_bytes(cap) + 64);
    std::vector<uint32_t> pyr(oct_pyr_bytes(D, nIni) / 4 + 1);
    std::vector<uint16_t> tbl(W + H + 2);
    OctWST<kGeneric, kGeneric> w;
    w.keys = const_cast<uint32_t*>(keys);
    w.n = n;
    w.nq = nq.data();
    w.cell_off = nullptr;
    w.cellkeys = nullptr;
    w.ncells = 0;
    w.cell_cap = 0;
    w.m = oct_nodemem_carve<kGeneric>(align16(mem.data()), cap);
    w.cap = cap;
    w.out_keys = out;
    w.out_cap = out_cap;
    w.dbg = nullptr;
    w.pyr = pyr.data();
    w.pyrD = D;
    w.xcode = tbl.data();
    w.ycode = tbl.data() + W + 1;
    OctShared sh;
    SerialPolicy p;
    int r = octree_distribute(p, w, &sh, W, H, N);
    *deep = r == kOctDeep;
    if (r == kOctDeep) {
        w.pyrD = 0;
        r = octree_distribute(p, w, &sh, W, H, N);
    }
    return r;
}

void harness_introsort(const int32_t* size, const int32_t* ulx, int n, int32_t* perm) {
    std::vector<SortElem> a(n);
    for (int i = 0; i < n; ++i) a[i] = SortElem{size[i], ulx[i], i};
    introsort_like_libstdcxx(a.data(), n);
    for (int i = 0; i < n; ++i) perm[i] = a[i].node;
}

void harness_introsort_parallel(const int32_t* size, const int32_t* ulx, int n, int32_t* perm) {
    std::vector<SortElem> a(n + 1), tmp(n + 1);
    for (int i = 0; i < n; ++i) a[i] = SortElem{size[i], ulx[i], i};
    std::vector<uint16_t> lex(n + 2), rex(n + 2), segof(n + 1), lpos(n + 1), rpos(n + 1), rank(n + 1);
    const int S = n / 16 + 4;
    std::vector<uint16_t> seg(6 * S);
    std::vector<int32_t> segK(S);
    SortScratch ss;
    ss.tmp = tmp.data();
    ss.lex = lex.data();
    ss.rex = rex.data();
    ss.segof = segof.data();
    ss.lpos = lpos.data();
    ss.rpos = rpos.data();
    ss.rank = rank.data();
    for (int b = 0; b < 2; ++b) {
        ss.segF[b] = seg.data() + (3 * b + 0) * S;
        ss.segL[b] = seg.data() + (3 * b + 1) * S;
        ss.segD[b] = seg.data() + (3 * b + 2) * S;
    }
    ss.segK = segK.data();
    int nseg = 0;
    SerialPolicy p;
    introsort_parallel<kGeneric>(p, a.data(), n, ss, &nseg);
    for (int i = 0; i < n; ++i) perm[i] = a[i].node;
}

int harness_fast_strength(const uint8_t* img, int stride, int x, int y, int tlow) {
    return fast_strength(img + (long long)y * stride + x, stride, tlow);
}

float harness_fast_atan2(float y, float x) { return fast_atan2_deg(y, x); }

// Packed (both polarities per word) strength vs the scalar corner strength on the same pixel.
int harness_fast_strength_packed64(const uint8_t* img, int x, int y) {
    return fast_strength_packed<64>(img + (long long)y * 64 + x);
}
int harness_fast_strength_corner(const uint8_t* img, int stride, int x, int y) {
    return fast_strength_corner(img + (long long)y * stride + x, stride);
}

// The planner (orb_geometry.h plan_geometry) with the product's knobs, for Python: lv gets
// kPlanLevelFields int64 per level, sc kPlanScalars int64, rtab up to rtab_cap int4 as 4 int32
// each (*rtab_n = how many the plan has).  The two name lists give the order.  Returns the
// planner's status; err receives its message.
#define PLAN_LEVEL_FIELDS(X)                                                                          \
    X(w) X(h) X(pitch) X(img_stride) X(bpitch) X(bimg_stride) X(nCols) X(nRows) X(wCell) X(hCell)     \
    X(maxBX) X(maxBY) X(ncells) X(cell_cap) X(cell_first) X(cellkey_off) X(cellcnt_off) X(cand_cap)   \
    X(N) X(W) X(H) X(kp_cap) X(kp_off) X(oct_cap) X(oct_off) X(patch) X(tiles_x) X(tiles_y)           \
    X(tile_first) X(xtab_off) X(ytab_off) X(simd_end) X(area2) X(band_row_off) X(tile_quad_off)       \
    X(od_blocks) X(od_first) X(tpitch)
#define PLAN_ARG_SCALARS(X)                                                                           \
    X(nlevels) X(out_cap) X(tail0) X(tail_lds) X(tail_buf1) X(tail_tab) X(tail_maxq) X(tail_maxrows)  \
    X(tail_min) X(oct_lds_nodes) X(oct_lds_bytes) X(oct_nq_off) X(oct_split) X(oct_split_min_images)  \
    X(oct2_threads) X(oct2_lds_nodes) X(oct2_lds_bytes) X(oct2_nq_off) X(oct2_lds_keys)               \
    X(oct_may_retry) X(oct_force_retry) X(oct_pyr_max) X(total_cells) X(total_tiles)                  \
    X(total_od_blocks) X(fast_tab_off) X(od_tab_off) X(fast_n48) X(fast_n64) X(fast_qcap)             \
    X(cellkeys_img_stride) X(cellcnt_img_stride) X(octws_img_stride) X(lvlkp_img_stride)
#define PLAN_NAME(f) #f ","
const char* harness_plan_level_fields() {
    return PLAN_LEVEL_FIELDS(PLAN_NAME) "scale_bits,pyr_off,blur_off,oct_total,oct_nodemem,oct_nodemem_need";
}
const char* harness_plan_scalars() {
    return PLAN_ARG_SCALARS(PLAN_NAME) "pyr_img,blur_img,cellkeys_img,octws_img,cellcnt_img,lvlkp_img,plan_out_cap,"
                                       "generic_pyr,rtab_n,kBrMaxRows,kBrMaxQuads,kTailLdsMax,kOctLdsNodes,kBlurTW,kBlurTH";
}
int harness_plan_geometry(int w, int h, int nlevels, float scale_factor, int nfeatures, int max_images,
                          long long* lv, long long* sc, int32_t* rtab, int rtab_cap, int* rtab_n, char* err,
                          int err_cap) {
    const orbgpu_params prm{nfeatures, scale_factor, nlevels, 20, 7};
    GeomPlan P;
    std::string msg;
    const int r = plan_geometry(build_tables(prm), prm, w, h, max_images, GeomKnobs{}, &P, &msg);
    if (err && err_cap > 0) {
        std::strncpy(err, msg.c_str(), err_cap - 1);
        err[err_cap - 1] = 0;
    }
    if (r) return r;
#define PLAN_PUT(f) *o++ = (long long)G.f;
    long long* o = lv;
    for (int l = 0; l < nlevels; ++l) {
        const LevelGeom& G = P.A.lv[l];
        PLAN_LEVEL_FIELDS(PLAN_PUT)
        const OctLayout ol = oct_layout(G.cand_cap, G.oct_cap);
        *o++ = __builtin_bit_cast(uint32_t, G.scale);
        *o++ = P.pyr_off[l];
        *o++ = P.blur_off[l];
        *o++ = ol.total;
        *o++ = ol.nodemem;
        *o++ = (long long)oct_nodemem_bytes(G.oct_cap);
    }
    o = sc;
    {
        const BatchArgs& G = P.A;
        PLAN_ARG_SCALARS(PLAN_PUT)
    }
    for (long long v : {P.pyr_img, P.blur_img, P.cellkeys_img, P.octws_img, (long long)P.cellcnt_img,
                        (long long)P.lvlkp_img, (long long)P.out_cap, (long long)P.generic_pyr,
                        (long long)P.rtab.size(), (long long)kBrMaxRows, (long long)kBrMaxQuads,
                        (long long)kTailLdsMax, (long long)kOctLdsNodes, (long long)kBlurTW, (long long)kBlurTH})
        *o++ = v;
    *rtab_n = (int)P.rtab.size();
    std::memcpy(rtab, P.rtab.data(), sizeof(int4) * std::min<size_t>(P.rtab.size(), (size_t)std::max(rtab_cap, 0)));
    return 0;
}

// ComputeKeyPointsOctTree cell loop over one level: the cell grid and the per-cell records are the
// planner's (a one-level plan of w x h, orb_geometry.h), the cells run through fast_cell_run.
int harness_level_candidates(const uint8_t* lvl, int w, int h, int ini, int mn, uint32_t* out,
                             int cap) {
    const orbgpu_params prm{0, 1.2f, 1, ini, mn};
    GeomPlan P;
    if (plan_geometry(build_tables(prm), prm, w, h, 1, GeomKnobs{}, &P, nullptr)) return -1;
    const LevelGeom& G = P.A.lv[0];
    std::vector<uint32_t> T32(kCellMax * kCellMax / 4), M32(kCellMax * kCellMax / 4);
    uint8_t* T = reinterpret_cast<uint8_t*>(T32.data());
    uint8_t* M = reinterpret_cast<uint8_t*>(M32.data());
    std::vector<uint16_t> list(cell_list_cap<kCellMax>() + 1);
    std::vector<int32_t> wcnt(4);
    std::vector<uint32_t> tmp(kCellMax * kCellMax);
    int total = 0;
    SerialPolicy p;
    // the small tile whenever the cells fit it (as the runtime picks it), else the general one
    const bool small = P.A.fast_n64 > 0;
    for (int cell = 0; cell < G.ncells; ++cell) {
        const int4 rec = P.rtab[P.A.fast_tab_off + 2 * cell], rec2 = P.rtab[P.A.fast_tab_off + 2 * cell + 1];
        if (rec2.z) continue;  // skip
        const int i = cell / G.nCols, j = cell % G.nCols;
        CellGeom g;
        g.iniX = rec.y;
        g.iniY = rec.z;
        g.minBorder = kMinBorder;
        g.rows = rec.w & 0xFFFF;
        g.cols = rec.w >> 16;
        // alternate the two load paths (dword-aligned window / plain bytes) across cells
        const bool dw = ((i + j) & 1) == 0 && (w & 3) == 0;
        const int sh = dw ? (g.iniX & 3) : 0;
        CellScratch cs{T, M, list.data(), wcnt.data()};
        const long long roi = (long long)g.iniY * w + g.iniX - sh;
        const uint8_t* src = lvl + roi;
        const long long size = (long long)w * h;
        auto ld16 = [&](long long off) {  // bounds-checked like the device buffer load
            uint8_t b[16];
            for (int k = 0; k < 16; ++k) b[k] = roi + off + k < size ? src[off + k] : 0;
            uint4 v;
            std::memcpy(&v, b, 16);
            return v;
        };
        const int m = small ? fast_cell_run<kCellPitchSmall>(p, src, w, sh, dw, g, ini, mn, cs, tmp.data(), ld16)
                            : fast_cell_run<kCellMax>(p, src, w, sh, dw, g, ini, mn, cs, tmp.data(), ld16);
        for (int k = 0; k < m; ++k) {
            if (total < cap) out[total] = tmp[k];
            ++total;
        }
    }
    return total;
}

// launch_fast_cells' decision for one tile call (orb_kernels.h fast_launch_plan), from the fields it
// reads: out = {tile (0: nothing launched), c0, c1, small-list kernel, overflow pass follows, 0}.
void harness_fast_launch_plan(int nimages, int fast_small, int n48, int n64, int total_cells, int has_ovf, int tile,
                              int32_t out[6]) {
    static int2 queue;  // only its address is looked at
    BatchArgs a{};
    a.nimages = nimages;
    a.fast_small = fast_small;
    a.fast_n48 = n48;
    a.fast_n64 = n64;
    a.total_cells = total_cells;
    a.fast_ovf = has_ovf ? &queue : nullptr;
    const FastLaunchPlan p = fast_launch_plan(a, tile);
    const int32_t v[6] = {p.tile, p.c0, p.c1, p.small, p.ovf, 0};
    std::memcpy(out, v, sizeof(v));
}

// The matchers' Layout (orb_layout.h) over n slots in a buffer at `base` (0: sizing only), slot i of
// counts[i] elements of elem_bytes[i] bytes (1, 2, 4, 8, 16, 44 or 60): addr[i] = the address add() gave
// it.  Returns Layout::bytes, or -1 for an element size that is not instantiated here.
long long harness_layout(unsigned long long base, int n, const long long* counts, const int32_t* elem_bytes,
                         unsigned long long* addr) {
    struct B44 { uint8_t b[44]; };
    struct B60 { uint8_t b[60]; };
    Layout lay{(uintptr_t)base};
    for (int i = 0; i < n; ++i) {
        const size_t k = (size_t)counts[i];
        switch (elem_bytes[i]) {
            case 1: addr[i] = (uintptr_t)lay.add<uint8_t>(k); break;
            case 2: addr[i] = (uintptr_t)lay.add<int16_t>(k); break;
            case 4: addr[i] = (uintptr_t)lay.add<int32_t>(k); break;
            case 8: addr[i] = (uintptr_t)lay.add<double>(k); break;
            case 16: addr[i] = (uintptr_t)lay.add<uint4>(k); break;
            case 44: addr[i] = (uintptr_t)lay.add<B44>(k); break;
            case 60: addr[i] = (uintptr_t)lay.add<B60>(k); break;
            default: return -1;
        }
    }
    return (long long)lay.bytes;
}

}  // extern "C"
