// orb_geometry.h -- the host-side geometry planner of liborbgpu.so, header-only and pure: the
// ORBextractor scale tables, the per-level geometry, the OpenCV resize tables, every per-image
// buffer offset and every LDS layout of a w x h image, from the reference's own float / double
// formulas.  No HIP API call, no environment, no context: orb_runtime.cpp allocates and binds what
// plan_geometry() sized, and the host harness (tests/harness) reads the same plan on the CPU.
#pragma once
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/orbgpu.h"
#include "orb_fast_cell.h"
#include "orb_kernels.h"
#include "orb_octree.h"

namespace orbgpu {

inline int round_up(int x, int a) { return (x + a - 1) / a * a; }
inline long long round_up_ll(long long x, long long a) { return (x + a - 1) / a * a; }
inline int cv_round_f(float v) { return (int)std::lrintf(v); }
inline int cv_round_d(double v) { return (int)std::lrint(v); }
inline int cv_floor_f(float v) { return (int)std::floor(v); }
inline short sat_short(float v) {
    int i = cv_round_f(v);
    return (short)std::min(std::max(i, (int)SHRT_MIN), (int)SHRT_MAX);
}

// ORBextractor tables (ORBextractor_old.cc:416-447)
struct ScaleTables {
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> nper;
};

inline ScaleTables build_tables(const orbgpu_params& prm) {
    ScaleTables t;
    const int L = prm.nlevels;
    const double scaleFactor = (double)prm.scale_factor;  // double member (ORBextractor_old.h:98)
    t.scale.assign(L, 0.f);
    t.sigma2.assign(L, 0.f);
    t.inv_scale.assign(L, 0.f);
    t.inv_sigma2.assign(L, 0.f);
    t.scale[0] = 1.0f;
    t.sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        t.scale[i] = (float)(t.scale[i - 1] * scaleFactor);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < L; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
    }
    t.nper.assign(L, 0);
    const int nfeatures = prm.nfeatures;
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        t.nper[l] = cv_round_f(nDesired);
        sum += t.nper[l];
        nDesired *= factor;
    }
    t.nper[L - 1] = std::max(nfeatures - sum, 0);
    return t;
}

// OpenCV cv::resize INTER_LINEAR coefficient tables (resize.cpp, fixed point, ksize 2), host-side.
// Returns true when OpenCV would take the INTER_AREA 2x path instead.
inline bool resize_tables(int sw, int sh, int dw, int dh, std::vector<int4>& xt, std::vector<int4>& yt) {
    double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    int iscale_x = cv_round_d(scale_x), iscale_y = cv_round_d(scale_y);
    bool area_fast = std::abs(scale_x - iscale_x) < DBL_EPSILON &&
                     std::abs(scale_y - iscale_y) < DBL_EPSILON && iscale_x == 2 && iscale_y == 2;
    xt.resize(dw);
    yt.resize(dh);
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor_f(fx);
        fx -= sx;
        if (sx < 0) fx = 0, sx = 0;
        if (sx + 1 >= sw && sx >= sw - 1) fx = 0, sx = sw - 1;
        const short a0 = sat_short((1.f - fx) * 2048), a1 = sat_short(fx * 2048);
        xt[dx] = make_int4(sx, std::min(sx + 1, sw - 1), a0, a1);
    }
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor_f(fy);
        fy -= sy;
        const short b0 = sat_short((1.f - fy) * 2048), b1 = sat_short(fy * 2048);
        yt[dy] = make_int4(std::min(std::max(sy, 0), sh - 1), std::min(std::max(sy + 1, 0), sh - 1),
                           b0, b1);
    }
    return area_fast;
}

inline int simd_end(int width) {  // VResizeLinearVec_32s8u coverage (oracle pins the same rule)
    int x = 0;
    for (; x <= width - 16; x += 16) {}
    for (; x <= width - 8; x += 8) {}
    return x;
}

// The diagnostics that change the plan (ORBGPU_* knobs, honoured only under ORBGPU_DIAGNOSTICS=1):
// plain values, the defaults are the product's.
struct GeomKnobs {
    int od_iters = 0;                          // ORBGPU_OD_ITERS: passes of kOdKpBlock per workgroup (0: policy)
    bool no_tail = false;                      // ORBGPU_NO_TAIL: per-level pyramid launches only
    int tail_min = kTailMinImages;             // ORBGPU_TAIL_MIN
    int oct_small_lds = kOctSmallLds;          // ORBGPU_OCT_SMALL_LDS
    int oct_small_threads = kOctSmallThreads;  // ORBGPU_OCT_SMALL_THREADS (128 or the default)
    int oct_split = -1;                        // ORBGPU_OCT_SPLIT: forced split level (-1: policy)
    bool oct_generic = false;                  // ORBGPU_OCT_GENERIC: every level through k_octree_retry
    int oct_pyr_max = kOctPyrMaxD;             // ORBGPU_OCT_PYR: cap of the count pyramid's depth
    bool oct_rounds = false;                   // ORBGPU_OCT_ROUNDS=1: phase 1 round by round with the pyramid too
    int fast_min_tier = 0;                     // ORBGPU_FAST_PITCH: 64 -> 1, 80 -> 2 (force the larger tiles)
};

// Everything set_geometry needs for a w x h image: the launch arguments with every non-pointer
// field filled (pointers null), the table the device reads, and the per-image strides the
// buffers are sized from.
struct GeomPlan {
    BatchArgs A{};
    std::vector<int4> rtab;
    long long pyr_off[kMaxLevels] = {}, blur_off[kMaxLevels] = {};
    long long pyr_img = 0, blur_img = 0, cellkeys_img = 0, octws_img = 0;
    int cellcnt_img = 0, lvlkp_img = 0, out_cap = 0;
    // scale factors above 2: k_blur_resize's staged window does not hold a resize step's taps, so
    // the pyramid is k_level_linear per level, then k_blur per level (no k_pyr_tail)
    bool generic_pyr = false;
};

namespace geom {

// running offsets of the per-level regions inside one image's share of each buffer
struct Cursor {
    long long pyr = 0, blr = 0, ck = 0, ows = 0;
    int cc = 0, kpo = 0, cell_first = 0, tile_first = 0, od_first = 0;
};

inline int invalid(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return ORBGPU_ERR_INVALID;
}

// Level size, pitches and the plane offsets in the pyramid / blur buffers.
inline int level_size(const ScaleTables& T, int w, int h, int l, GeomPlan& P, Cursor& cur, std::string* err) {
    LevelGeom& G = P.A.lv[l];
    G.w = cv_round_f((float)w * T.inv_scale[l]);   // ComputePyramid :1336
    G.h = cv_round_f((float)h * T.inv_scale[l]);
    if (G.w < 2 * kEdge + 4 || G.h < 2 * kEdge + 4)
        return invalid(err, "pyramid level " + std::to_string(l) + " too small");
    G.bpitch = round_up(G.w, 64);
    if (l == 0) {
        G.pitch = w;
        G.img_stride = (long long)w * h;
    } else {
        G.pitch = G.bpitch;
        P.pyr_off[l] = cur.pyr;
        cur.pyr += round_up_ll((long long)G.pitch * G.h, 256);
    }
    P.blur_off[l] = cur.blr;
    cur.blr += round_up_ll((long long)G.bpitch * G.h, 256);
    G.scale = T.scale[l];
    G.patch = (int)(31 * T.scale[l]);
    G.tiles_x = (G.w + kBlurTW - 1) / kBlurTW;  // k_blur tile kBlurTW x kBlurTH
    G.tiles_y = (G.h + kBlurTH - 1) / kBlurTH;
    G.tile_first = cur.tile_first;
    cur.tile_first += G.tiles_x * G.tiles_y;
    return 0;
}

// cell grid (ComputeKeyPointsOctTree :787-805) and the cell-key / cell-count regions
inline int cell_grid(int l, GeomPlan& P, Cursor& cur, std::string* err) {
    LevelGeom& G = P.A.lv[l];
    G.maxBX = G.w - kEdge + 3;
    G.maxBY = G.h - kEdge + 3;
    const float width = (float)(G.maxBX - kMinBorder), height = (float)(G.maxBY - kMinBorder);
    G.nCols = (int)(width / 35.f);
    G.nRows = (int)(height / 35.f);
    if (G.nCols < 1 || G.nRows < 1)
        return invalid(err, "pyramid level " + std::to_string(l) + " has no cells");
    G.wCell = (int)std::ceil(width / G.nCols);
    G.hCell = (int)std::ceil(height / G.nRows);
    if (G.wCell > 69 || G.hCell > 69) return invalid(err, "cell too large");
    G.ncells = G.nCols * G.nRows;
    // (a multiple of 4: k_octree reads a cell's keys as 16-byte chunks)
    G.cell_cap = (((G.wCell + 1) / 2) * ((G.hCell + 1) / 2) + 3) & ~3;
    G.cell_first = cur.cell_first;
    cur.cell_first += G.ncells;
    G.cellkey_off = cur.ck;
    G.cand_cap = G.ncells * G.cell_cap;
    cur.ck += round_up_ll(G.cand_cap, 64);
    G.cellcnt_off = cur.cc;
    cur.cc += round_up(G.ncells, 16);
    return 0;
}

// octree capacities, the level-keypoint region, the octree workspace and the k_orient_desc blocks
inline void octree_caps(const ScaleTables& T, int l, int od_per_block, GeomPlan& P, Cursor& cur) {
    LevelGeom& G = P.A.lv[l];
    G.N = T.nper[l];
    G.W = G.maxBX - kMinBorder;
    G.H = G.maxBY - kMinBorder;
    const int nIni = std::max(1, (int)std::round((float)G.W / (float)G.H));
    // live octree nodes never exceed max(N + 3, 4 * nIni) (orb_octree.h)
    G.oct_cap = std::max(G.N + 3, 4 * nIni) + 8;
    G.kp_cap = G.oct_cap;
    G.kp_off = cur.kpo;
    cur.kpo += round_up(G.kp_cap, 16);
    G.oct_off = cur.ows;
    cur.ows += oct_layout(G.cand_cap, G.oct_cap).total;
    G.od_blocks = std::max(1, (G.N + 16 + od_per_block - 1) / od_per_block);  // k_orient_desc blocks
    G.od_first = cur.od_first;
    cur.od_first += G.od_blocks;
}

// resize tables of level l >= 1 (from level l - 1) plus k_blur_resize's band / quad ownership
inline int resize_level(int l, GeomPlan& P, std::string* err) {
    BatchArgs& A = P.A;
    LevelGeom& G = A.lv[l];
    G.area2 = 0;
    if (l < 1) return 0;
    const LevelGeom& S = A.lv[l - 1];
    std::vector<int4> xt, yt;
    G.area2 = resize_tables(S.w, S.h, G.w, G.h, xt, yt) ? 1 : 0;
    G.xtab_off = (int)P.rtab.size();
    P.rtab.insert(P.rtab.end(), xt.begin(), xt.end());
    G.ytab_off = (int)P.rtab.size();
    P.rtab.insert(P.rtab.end(), yt.begin(), yt.end());
    G.simd_end = simd_end(G.w);
    // k_blur_resize ownership: output row dy / column quad q belongs to the blur tile of
    // level l - 1 holding its first source row / column (monotone in dy / q)
    auto push_ints = [&](const std::vector<int>& v) {
        const int off = 4 * (int)P.rtab.size();
        for (size_t i = 0; i < v.size(); i += 4)
            P.rtab.push_back(make_int4(v[i], i + 1 < v.size() ? v[i + 1] : 0,
                                       i + 2 < v.size() ? v[i + 2] : 0, i + 3 < v.size() ? v[i + 3] : 0));
        return off;
    };
    std::vector<int> band(S.tiles_y + 1), tq(S.tiles_x + 1);
    const int nquads = (G.w + 3) / 4;
    for (int b = 0, dy = 0; b <= S.tiles_y; ++b) {
        while (dy < G.h && (b == S.tiles_y || (G.area2 ? 2 * dy : yt[dy].x) < kBlurTH * b)) ++dy;
        band[b] = b == S.tiles_y ? G.h : dy;
    }
    for (int j = 0, q = 0; j <= S.tiles_x; ++j) {
        while (q < nquads && (j == S.tiles_x || (G.area2 ? 8 * q : xt[4 * q].x) < kBlurTW * j)) ++q;
        tq[j] = j == S.tiles_x ? nquads : q;
    }
    for (int b = 0; b < S.tiles_y; ++b)
        if (band[b + 1] - band[b] > kBrMaxRows) return invalid(err, "resize band table");
    for (int j = 0; j < S.tiles_x; ++j)
        if (tq[j + 1] - tq[j] > kBrMaxQuads) return invalid(err, "resize quad table");
    G.band_row_off = push_ints(band);
    G.tile_quad_off = push_ints(tq);
    G.qrec_off = G.qbase_off = G.yrec_off = 0;
    if (G.area2) return 0;
    // the same tables in the form the resize loops read (orb_pyramid.hip rs_hsum / rs_vert): per
    // output quad the taps of its four outputs relative to the quad's first left tap as v_perm
    // selector pairs (0 .. 7 for scale steps <= 2) and the coefficient pairs times 16 as u16 pairs,
    // per output row the weights as b << 8; the last quad repeats the last column
    std::vector<int> qbase(nquads);
    G.qrec_off = (int)P.rtab.size();
    for (int q = 0; q < nquads; ++q) {
        const int base = xt[std::min(4 * q, G.w - 1)].x;
        unsigned sl[4], cl[4];
        for (int k = 0; k < 4; ++k) {
            const int4 x = xt[std::min(4 * q + k, G.w - 1)];
            sl[k] = (unsigned)(x.x - base) | 0x0c00u | ((unsigned)(x.y - base) << 16) | 0x0c000000u;
            cl[k] = ((unsigned)x.z << 4) | ((unsigned)x.w << 20);
        }
        P.rtab.push_back(make_int4((int)sl[0], (int)sl[1], (int)sl[2], (int)sl[3]));
        P.rtab.push_back(make_int4((int)cl[0], (int)cl[1], (int)cl[2], (int)cl[3]));
        qbase[q] = base;
    }
    G.yrec_off = (int)P.rtab.size();
    for (int dy = 0; dy < G.h; ++dy)
        P.rtab.push_back(make_int4(yt[dy].x, yt[dy].y, (int)((unsigned)yt[dy].z << 8), (int)((unsigned)yt[dy].w << 8)));
    G.qbase_off = push_ints(qbase);
    return 0;
}

// k_pyr_tail: the smallest t >= 2 such that level t - 1 and level t (and level t's resize
// tables) fit one workgroup's LDS together; the tail then makes levels t .. L-1 and blurs
// t - 1 .. L-1 (ORBGPU_NO_TAIL under diagnostics: per-level launches only).  Its pad columns
// and row reflection take one REFLECT_101 step, exact for levels of >= 4 px: every level
// passed the 2 * kEdge + 4 check of level_size.
inline void tail_layout(const GeomKnobs& K, GeomPlan& P) {
    BatchArgs& A = P.A;
    const int L = A.nlevels;
    for (int l = 0; l < L; ++l) A.lv[l].tpitch = round_up(A.lv[l].w + 28, 16);
    A.tail0 = L + 1;
    if (!K.no_tail && !P.generic_pyr)
        for (int t = 2; t <= L; ++t) {
            const LevelGeom& S0 = A.lv[t - 1];
            const long long b0 = round_up_ll((long long)S0.tpitch * S0.h, 16);
            const long long b1 = t < L ? round_up_ll((long long)A.lv[t].tpitch * A.lv[t].h, 16) : 0;
            const int maxq = t < L ? (A.lv[t].w + 3) / 4 : 0, maxrows = t < L ? A.lv[t].h : 0;
            const long long tab = (long long)maxq * (16 + 16 + 4) + (long long)maxrows * 16;
            if (b0 + b1 + tab + 16 <= kTailLdsMax && (S0.w + 3) / 4 <= 1024) {  // one resize quad per thread
                A.tail0 = t;
                A.tail_buf1 = (int)b0;
                A.tail_tab = (int)(b0 + b1);
                A.tail_maxq = maxq;
                A.tail_maxrows = maxrows;
                A.tail_lds = (int)round_up_ll(b0 + b1 + tab, 16);
                break;
            }
        }
    // the tail runs for launches of at least tail_min images (one 1024-thread workgroup per image
    // makes levels tail0 .. L-1 serially: 46 us for one pair, where the per-level launches take
    // ~20 us; with hundreds of images the tail's single pass wins)
    A.tail_min = K.tail_min;
}

// k_octree's LDS layouts, the split between its two launch shapes and the retry flags
inline void octree_lds(const GeomKnobs& K, GeomPlan& P) {
    BatchArgs& A = P.A;
    const int L = A.nlevels;
    // k_octree dynamic LDS: the largest node capacity that fits kOctLdsNodes (levels above it
    // keep their node state in the global workspace) and room for the cell offsets.
    int lds_nodes = 0, max_cells = 0;
    for (int l = 0; l < L; ++l) {
        if (A.lv[l].oct_cap <= kOctLdsNodes) lds_nodes = std::max(lds_nodes, A.lv[l].oct_cap);
        max_cells = std::max(max_cells, A.lv[l].ncells);
    }
    A.oct_lds_nodes = lds_nodes;
    A.oct_nq_off = ((int)oct_nodemem_bytes(std::max(lds_nodes, 1)) + 15) & ~15;
    A.oct_lds_bytes = std::max(A.oct_nq_off + 2 * kOctLdsKeys, std::min(4 * max_cells, 65536));
    A.oct_lds_bytes = (A.oct_lds_bytes + 15) & ~15;
    // Levels [oct_split, L) run as a second k_octree launch of smaller workgroups (kOctSmallThreads)
    // with an LDS layout of kOctSmallLds: node state + cell offsets of those levels, then labels
    // for as many keys as fit (the global workspace above that).  More workgroups fit a CU, which
    // is what the node phases' serial latency needs.  oct_split = the first level from which on
    // the node state leaves room for >= 1024 labels (0 for 640x480-class pyramids: every level).
    const int budget = K.oct_small_lds;
    A.oct2_threads = K.oct_small_threads;
    auto layout = [&](int s0) {
        int n2 = 0, c2 = 0;
        for (int l = s0; l < L; ++l) {
            if (A.lv[l].oct_cap <= kOctLdsNodes) n2 = std::max(n2, A.lv[l].oct_cap);
            c2 = std::max(c2, A.lv[l].ncells);
        }
        A.oct2_lds_nodes = n2;
        A.oct2_nq_off = std::max(((int)oct_nodemem_bytes(std::max(n2, 1)) + 15) & ~15, (4 * c2 + 15) & ~15);
        A.oct2_lds_keys = std::max(0, (budget - A.oct2_nq_off) / 2);
        A.oct2_lds_bytes = (A.oct2_nq_off + 2 * A.oct2_lds_keys + 15) & ~15;
        return A.oct2_lds_keys >= 1024;
    };
    // Default: every level in the small shape when all of them fit it (640x480-class
    // pyramids), else every level in the 512-thread shape: a partial split runs the two
    // launches back to back and measured slower (C5: 90 vs 98 Mfeatures/s).  Launches of
    // fewer than kOctSmallMinImages images stay in the 512-thread shape too (latency, not
    // occupancy, bounds them: C4 0.31 vs 0.26 ms per pair).  ORBGPU_OCT_SPLIT forces a split.
    if (K.oct_split >= 0) {
        A.oct_split = std::min(L, K.oct_split);
        if (A.oct_split < L && !layout(A.oct_split)) A.oct_split = L;
        A.oct_split_min_images = 0;
    } else {
        A.oct_split = layout(0) ? 0 : L;
        A.oct_split_min_images = kOctSmallMinImages;
    }
    // a level misses k_octree (labels in LDS or in the workspace) only if its node capacity or
    // its cell offsets do not fit LDS; then k_octree_retry redoes it with generic pointers
    A.oct_may_retry = 0;
    for (int l = 0; l < L; ++l) {
        const LevelGeom& G = A.lv[l];
        if (G.oct_cap > lds_nodes || G.ncells > A.oct_nq_off / 4) A.oct_may_retry = 1;
        if (l >= A.oct_split && (G.oct_cap > A.oct2_lds_nodes || G.ncells > A.oct2_nq_off / 4)) A.oct_may_retry = 1;
    }
    A.oct_force_retry = K.oct_generic ? 1 : 0;  // diagnostics / tests
    // ORBGPU_OCT_PYR=<d>: cap the count pyramid's depth (0: the label-pass formulation only)
    A.oct_pyr_max = K.oct_pyr_max;
    A.oct_rounds = K.oct_rounds ? 1 : 0;  // A/B and tests: the round-by-round phase 1 (orb_octree.h)
    if (A.oct_force_retry) A.oct_may_retry = 1;
}

// FAST LDS tiles: each level takes the smallest tile its cell ROIs (+3 alignment bytes) fit:
// 48 bytes, else 64, else 80.  Cells grow as the levels shrink (fewer, wider cells) but not
// monotonically in both directions (640x480: level 6's cells are 51 rows tall, level 7's 42),
// so the tiers are chosen per level.
// k_fast_cells per-cell records, two int4 per cell: {level, iniX, iniY, rows | cols << 16} and
// {cell-count index, cell-key index, skip, 0} (the cell loop's :807-821 geometry), grouped by
// tier.  One scalar load replaces each workgroup's level search and cell-grid divisions.
inline void fast_records(const GeomKnobs& K, GeomPlan& P) {
    BatchArgs& A = P.A;
    const int L = A.nlevels;
    auto fits = [&](int l, int pitch) { return A.lv[l].wCell + 9 <= pitch && A.lv[l].hCell + 6 <= pitch; };
    int tier[kMaxLevels];
    for (int l = 0; l < L; ++l) {
        const int t = fits(l, kCellPitchTiny) ? 0 : fits(l, kCellPitchSmall) ? 1 : 2;
        tier[l] = std::max(t, K.fast_min_tier);
    }
    A.fast_tab_off = (int)P.rtab.size();
    int tier_end[3] = {0, 0, 0}, nrec = 0;
    for (int t = 0; t < 3; ++t) {
        for (int l = 0; l < L; ++l) {
            if (tier[l] != t) continue;
            const LevelGeom& G = A.lv[l];
            for (int cell = 0; cell < G.ncells; ++cell) {
                const int ci = cell / G.nCols, cj = cell % G.nCols;
                const int iniY = kMinBorder + ci * G.hCell, iniX = kMinBorder + cj * G.wCell;
                const int skip = (iniY >= G.maxBY - 3 || iniX >= G.maxBX - 6) ? 1 : 0;  // :812, :821
                const int rows = skip ? 0 : std::min(iniY + G.hCell + 6, G.maxBY) - iniY;
                const int cols = skip ? 0 : std::min(iniX + G.wCell + 6, G.maxBX) - iniX;
                P.rtab.push_back(make_int4(l, iniX, iniY, rows | (cols << 16)));
                P.rtab.push_back(make_int4(G.cellcnt_off + cell,
                                           (int)(G.cellkey_off + (long long)cell * G.cell_cap), skip, 0));
                ++nrec;
            }
        }
        tier_end[t] = nrec;
    }
    A.fast_n48 = tier_end[0];
    A.fast_n64 = tier_end[1];
    A.fast_qcap = tier_end[1];  // the 48- and 64-byte tiles' cells share one queue per launch
}

// k_orient_desc's per-block records {level, block, 0, 0}
inline void od_records(GeomPlan& P) {
    BatchArgs& A = P.A;
    A.od_tab_off = (int)P.rtab.size();
    for (int l = 0; l < A.nlevels; ++l)
        for (int b = 0; b < A.lv[l].od_blocks; ++b) P.rtab.push_back(make_int4(l, b, 0, 0));
}

}  // namespace geom

// Level geometry for a w x h image (input row stride = w in the batch buffer) of a context that
// holds up to max_images images.  Returns ORBGPU_OK, or ORBGPU_ERR_INVALID with *err set.
inline int plan_geometry(const ScaleTables& T, const orbgpu_params& prm, int w, int h, int max_images,
                         const GeomKnobs& K, GeomPlan* out, std::string* err) {
    GeomPlan& P = *out;
    P = GeomPlan{};
    BatchArgs& A = P.A;
    const int L = prm.nlevels;
    A.nlevels = L;
    A.ini_th = prm.ini_th_fast;
    A.min_th = prm.min_th_fast;
    A.fast_small = -1;
    // keypoints per k_orient_desc workgroup (orb_kernels.h kOdBlockKps; ORBGPU_OD_ITERS: passes of
    // kOdKpBlock instead, for A/B).  A context that never holds more than a few images (the
    // latency shape) takes one pass per workgroup: more, shorter workgroups for its few keypoints
    // (C4 step 124.3 us at one pass, 125.4 at two, 126.4 at three)
    const int od_per_block = K.od_iters > 0 ? kOdKpBlock * K.od_iters
                                            : max_images <= kFastMergeMaxImages ? kOdKpBlock : kOdBlockKps;
    geom::Cursor cur;
    for (int l = 0; l < L; ++l) {
        if (int e = geom::level_size(T, w, h, l, P, cur, err)) return e;
        if (int e = geom::cell_grid(l, P, cur, err)) return e;
        geom::octree_caps(T, l, od_per_block, P, cur);
        if (int e = geom::resize_level(l, P, err)) return e;
    }
    P.generic_pyr = prm.scale_factor > 2.0f;
    geom::tail_layout(K, P);
    P.pyr_img = round_up_ll(cur.pyr, 256);
    P.blur_img = round_up_ll(cur.blr, 256);
    P.cellkeys_img = cur.ck;
    P.cellcnt_img = cur.cc;
    P.octws_img = round_up_ll(cur.ows, 256);
    P.lvlkp_img = cur.kpo;
    P.out_cap = cur.kpo;
    geom::octree_lds(K, P);
    A.total_cells = cur.cell_first;
    geom::fast_records(K, P);
    A.total_tiles = cur.tile_first;
    A.total_od_blocks = cur.od_first;
    geom::od_records(P);
    for (int l = 0; l < L; ++l) {
        if (l > 0) A.lv[l].img_stride = P.pyr_img;
        A.lv[l].bimg_stride = P.blur_img;
    }
    A.cellkeys_img_stride = P.cellkeys_img;
    A.cellcnt_img_stride = P.cellcnt_img;
    A.octws_img_stride = P.octws_img;
    A.lvlkp_img_stride = P.lvlkp_img;
    A.out_cap = P.out_cap;
    return ORBGPU_OK;
}

}  // namespace orbgpu
