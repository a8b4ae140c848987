// orb_window.h -- Frame::GetFeaturesInArea (Frame.cc:673-739) over a frame whose keypoints,
// descriptors, grid and mvuRight live in HBM, shared by the two projection searches
// (orb_sbp.hip: the local-map search, orb_track.hip: the motion-model search) and, with
// ComputeThreeMaxima, by the initialisation search (orb_init.hip); the relocalisation and
// bag-of-words searches (orb_reloc.hip, orb_bow.hip) share its candidate and rotation-bin helpers,
// and the fusion (orb_fuse.hip) and the Sim3 projection searches (orb_sim3.hip) walk
// KeyFrame::GetFeaturesInArea, the same cells, by a group of lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "orb_kernels.h"

namespace orbgpu {

struct FrameView {
    const float* xy;       // keypoint positions [out_cap][2] (mvKeysUn, or mvKeys / mvKeysRight)
    const uint8_t* kp;     // out_kps rows (angle at +12, octave at +20)
    const int32_t* cs;     // cell_start [3073]
    const int32_t* ci;     // cell_idx
    const uint8_t* desc;   // [out_cap][32]
    const float* uright;   // mvuRight or nullptr
};

__device__ inline int octave_of(const FrameView& F, int k) {
    return *reinterpret_cast<const int32_t*>(F.kp + (long long)k * 28 + 20);
}

__device__ inline float angle_of(const FrameView& F, int k) {
    return *reinterpret_cast<const float*>(F.kp + (long long)k * 28 + 12);
}

__device__ inline int hamming32(const uint32_t q[8], const uint8_t* d) {
    const uint4 a = *reinterpret_cast<const uint4*>(d);
    const uint4 b = *reinterpret_cast<const uint4*>(d + 16);
    return __popc(q[0] ^ a.x) + __popc(q[1] ^ a.y) + __popc(q[2] ^ a.z) + __popc(q[3] ^ a.w) +
           __popc(q[4] ^ b.x) + __popc(q[5] ^ b.y) + __popc(q[6] ^ b.z) + __popc(q[7] ^ b.w);
}

__device__ inline void load_desc(const uint8_t desc[32], uint32_t q[8]) {
    for (int w = 0; w < 8; ++w)
        q[w] = (uint32_t)desc[4 * w] | ((uint32_t)desc[4 * w + 1] << 8) | ((uint32_t)desc[4 * w + 2] << 16) |
               ((uint32_t)desc[4 * w + 3] << 24);
}

// The cells GetFeaturesInArea(x, y, rs) visits (Frame.cc:680-694); false: none.  a: the caller's
// argument struct (bounds[4] = {mnMinX, mnMaxX, mnMinY, mnMaxY}, grid_inv[2]).
struct CellRange {
    int minX, maxX, minY, maxY;
};
template <class Args>
__device__ inline bool window_cells(const Args& a, float x, float y, float rs, CellRange* r) {
    r->minX = max(0, (int)floorf((x - a.bounds[0] - rs) * a.grid_inv[0]));
    if (r->minX >= kGridCols) return false;
    r->maxX = min(kGridCols - 1, (int)ceilf((x - a.bounds[0] + rs) * a.grid_inv[0]));
    if (r->maxX < 0) return false;
    r->minY = max(0, (int)floorf((y - a.bounds[2] - rs) * a.grid_inv[1]));
    if (r->minY >= kGridRows) return false;
    r->maxY = min(kGridRows - 1, (int)ceilf((y - a.bounds[2] + rs) * a.grid_inv[1]));
    return r->maxY >= 0;
}

// The level and distance tests of GetFeaturesInArea (:705-722) and the callers' per-candidate
// filters (ORBmatcher.cc:86-95 / :164-170 / :1790-1799) on keypoint k; *oct: its octave.
// proj_xr: the projection the mvuRight test compares with (used when F.uright is set).
template <class Blocked>
__device__ inline bool window_accepts(const FrameView& F, int k, float x, float y, int minLevel, int maxLevel,
                                      float rs, float proj_xr, Blocked blocked, int* oct) {
    *oct = octave_of(F, k);
    if ((minLevel > 0) || (maxLevel >= 0)) {  // bCheckLevels
        if (*oct < minLevel) return false;
        if (maxLevel >= 0 && *oct > maxLevel) return false;
    }
    const float2 p = *reinterpret_cast<const float2*>(F.xy + 2LL * k);
    if (!(fabsf(p.x - x) < rs && fabsf(p.y - y) < rs)) return false;
    if (blocked(k)) return false;
    if (F.uright) {
        const float ur = F.uright[k];
        if (ur > 0 && fabsf(proj_xr - ur) > rs) return false;
    }
    return true;
}

// GetFeaturesInArea(x, y, rs, minLevel, maxLevel) + the filters and the distance, calling
// emit(idx, dist, octave) for each surviving candidate in window order.
template <class Args, class Blocked, class Emit>
__device__ inline void walk_window(const Args& a, const FrameView& F, float x, float y, int minLevel, int maxLevel,
                                   float rs, float proj_xr, const uint32_t q[8], Blocked blocked, Emit emit) {
    CellRange r;
    if (!window_cells(a, x, y, rs, &r)) return;
    for (int ix = r.minX; ix <= r.maxX; ++ix) {
        const int j1 = F.cs[ix * kGridRows + r.maxY + 1];
        for (int j = F.cs[ix * kGridRows + r.minY]; j < j1; ++j) {  // cells iy = minY..maxY are adjacent
            const int k = F.ci[j];
            int oct;
            if (!window_accepts(F, k, x, y, minLevel, maxLevel, rs, proj_xr, blocked, &oct)) continue;
            emit(k, hamming32(q, F.desc + 32LL * k), oct);
        }
    }
}

// The same walk by a whole wave for one window (every lane passes the same arguments): lane l
// takes entries l, l + 64, ... of each grid column's list.  Returns the first lowest distance in
// window order to every lane (*best_idx = -1, distance 256 when nothing survives).
template <class Args, class Blocked>
__device__ inline int walk_window_wave(const Args& a, const FrameView& F, float x, float y, int minLevel,
                                       int maxLevel, float rs, float proj_xr, const uint32_t q[8], Blocked blocked,
                                       int lane, int* best_idx) {
    uint32_t key = 0xFFFFFFFFu;  // distance << 16 | window position
    int idx = -1;
    CellRange r;
    if (window_cells(a, x, y, rs, &r)) {
        int base = 0;
        for (int ix = r.minX; ix <= r.maxX; ++ix) {
            const int j0 = F.cs[ix * kGridRows + r.minY], j1 = F.cs[ix * kGridRows + r.maxY + 1];
            for (int j = j0 + lane; j < j1; j += 64) {
                const int k = F.ci[j];
                int oct;
                if (!window_accepts(F, k, x, y, minLevel, maxLevel, rs, proj_xr, blocked, &oct)) continue;
                const uint32_t kk = ((uint32_t)hamming32(q, F.desc + 32LL * k) << 16) | (uint32_t)(base + j - j0);
                if (kk < key) key = kk, idx = k;
            }
            base += j1 - j0;
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t ok = __shfl_xor(key, o);
        const int oi = __shfl_xor(idx, o);
        if (ok < key) key = ok, idx = oi;
    }
    *best_idx = idx;
    return idx >= 0 ? (int)(key >> 16) : 256;
}

// KeyFrame::GetFeaturesInArea(x, y, rs) (KeyFrame.cc:706-750: the cells and the order of
// Frame::GetFeaturesInArea, no level filter) by a group of G adjacent lanes for one window (every
// lane of the group passes the same arguments, sub = its place in the group): lane sub takes grid
// columns minX + sub, minX + sub + G, ... whole.  keep(k, octave) is the caller's per-candidate filter,
// run before the distance.  Returns the first lowest distance in window order to every lane of the
// group (*best_idx = -1, distance 256 when nothing survives); *any: the area held a keypoint at all.
// A column belongs to one lane, which meets its entries in order and keeps the first of equal
// distances; between lanes the column decides, so the key is distance << 6 | column.  A lane that
// saw a keypoint and kept none holds kAreaSeen, above every real key and below "nothing at all".
constexpr uint32_t kAreaNone = 0xFFFFFFFFu, kAreaSeen = 0xFFFFFFFEu;

// One step of the group's minimum by a DPP move within the row of 16 (no LDS round trip): the
// lower key of this lane and its partner under kCtrl, with the key's keypoint.
template <int kCtrl>
__device__ inline void dpp_lower_key(uint32_t& key, int& idx) {
    const uint32_t ok = (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, kCtrl, 0xF, 0xF, false);
    const int oi = __builtin_amdgcn_update_dpp(idx, idx, kCtrl, 0xF, 0xF, false);
    if (ok < key) key = ok, idx = oi;
}

template <int G, class Args, class Keep>
__device__ inline int walk_area_group(const Args& a, const FrameView& F, float x, float y, float rs, int sub,
                                      const uint32_t q[8], Keep keep, int* best_idx, bool* any) {
    static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "a group lies within a DPP row");
    uint32_t key = kAreaNone;
    int idx = -1;
    CellRange r;
    if (window_cells(a, x, y, rs, &r)) {
        for (int ix = r.minX + sub; ix <= r.maxX; ix += G) {
            const int j1 = F.cs[ix * kGridRows + r.maxY + 1];
            for (int j = F.cs[ix * kGridRows + r.minY]; j < j1; ++j) {
                const int k = F.ci[j];
                const float2 p = *reinterpret_cast<const float2*>(F.xy + 2LL * k);
                if (!(fabsf(p.x - x) < rs && fabsf(p.y - y) < rs)) continue;
                key = min(key, kAreaSeen);
                if (!keep(k, octave_of(F, k))) continue;
                const uint32_t kk = ((uint32_t)hamming32(q, F.desc + 32LL * k) << 6) | (uint32_t)ix;
                if (kk < key) key = kk, idx = k;
            }
        }
    }
    // after each step the lanes that exchanged agree, so the mirrors pair what xor 4 and xor 8 would
    if (G >= 2) dpp_lower_key<0xB1>(key, idx);    // quad_perm [1, 0, 3, 2]
    if (G >= 4) dpp_lower_key<0x4E>(key, idx);    // quad_perm [2, 3, 0, 1]
    if (G >= 8) dpp_lower_key<0x141>(key, idx);   // row_half_mirror
    if (G >= 16) dpp_lower_key<0x140>(key, idx);  // row_mirror
    *best_idx = idx;
    *any = key != kAreaNone;
    return idx >= 0 ? (int)(key >> 6) : 256;
}

// The frame's buffers: a.xy_un / kps / cell_start / cell_idx / desc over batch image img.
template <class Args>
__device__ inline FrameView frame_view_of(const Args& a, int img, const float* uright) {
    FrameView F;
    F.xy = a.xy_un + 2LL * img * a.out_cap;
    F.kp = static_cast<const uint8_t*>(a.kps) + 28LL * img * a.out_cap;
    F.cs = a.cell_start + (long long)img * (kGridCols * kGridRows + 1);
    F.ci = a.cell_idx + (long long)img * a.out_cap;
    F.desc = a.desc + 32LL * img * a.out_cap;
    F.uright = uright;
    return F;
}

// Rcw * pos + tcw and its pinhole projection (K = {fx, fy, cx, cy}).  The build keeps the operation
// order (no contraction): it is the result.
__device__ inline void project_pinhole(const float Rcw[9], const float tcw[3], const float K[4], const float pos[3],
                                       float* xc, float* yc, float* zc, float* u, float* v) {
    const float X = pos[0], Y = pos[1], Z = pos[2];
    *xc = ((Rcw[0] * X + Rcw[1] * Y) + Rcw[2] * Z) + tcw[0];
    *yc = ((Rcw[3] * X + Rcw[4] * Y) + Rcw[5] * Z) + tcw[1];
    *zc = ((Rcw[6] * X + Rcw[7] * Y) + Rcw[8] * Z) + tcw[2];
    *u = K[0] * *xc / *zc + K[2];
    *v = K[1] * *yc / *zc + K[3];
}

// The same transform with the projection the vpPointsKFs overload of the Sim3 SearchByProjection writes out
// (ORBmatcher.cc:574-579): invz = 1 / zc; x = xc * invz; u = fx * x + cx.  It rounds three times where
// Pinhole::project rounds twice, so the two can land a float apart.  Every step is a named single-precision
// value under contract(off): no fused multiply-add, no reciprocal folded into a division.
__device__ inline void project_pinhole_invz(const float Rcw[9], const float tcw[3], const float K[4], const float pos[3],
                                            float* xc, float* yc, float* zc, float* u, float* v) {
#pragma clang fp contract(off)
    const float X = pos[0], Y = pos[1], Z = pos[2];
    *xc = ((Rcw[0] * X + Rcw[1] * Y) + Rcw[2] * Z) + tcw[0];
    *yc = ((Rcw[3] * X + Rcw[4] * Y) + Rcw[5] * Z) + tcw[1];
    *zc = ((Rcw[6] * X + Rcw[7] * Y) + Rcw[8] * Z) + tcw[2];
    const float invz = 1.0f / *zc;
    const float x = *xc * invz;
    const float y = *yc * invz;
    const float fxx = K[0] * x;
    const float fyy = K[1] * y;
    *u = fxx + K[2];
    *v = fyy + K[3];
}

// KeyFrame::GetFeaturesInArea(x, y, rs) by a group of G adjacent lanes as in walk_area_group, keeping not the
// best alone but the four lowest (distance, window position) among the keypoints keep(k, octave) lets
// through whose distance within(d) accepts, and counting them: idx[t] / dist[t] (-1 / 256 where there are
// fewer) and *n, the same in every lane of the group; *any: the area held a keypoint at all.  A lane meets
// its columns' entries in window order, so its key is distance << 22 | column << 16 | place in the column's
// list; keys of different lanes differ in the column.  The group's lists merge by four rounds of "lowest
// head", the minimum taken by shuffles that stay inside the group.
template <int G, class Args, class Keep, class Within>
__device__ inline void walk_area_group_top4(const Args& a, const FrameView& F, float x, float y, float rs, int sub,
                                            const uint32_t q[8], Keep keep, Within within, int32_t idx[4],
                                            int32_t dist[4], int* n, bool* any) {
    static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "a power of two below the wave");
    uint32_t key[4] = {kAreaNone, kAreaNone, kAreaNone, kAreaNone};
    int kid[4] = {-1, -1, -1, -1};
    int count = 0, seen = 0;
    CellRange r;
    if (window_cells(a, x, y, rs, &r)) {
        for (int ix = r.minX + sub; ix <= r.maxX; ix += G) {
            const int j0 = F.cs[ix * kGridRows + r.minY], j1 = F.cs[ix * kGridRows + r.maxY + 1];
            for (int j = j0; j < j1; ++j) {
                int k = F.ci[j];
                const float2 p = *reinterpret_cast<const float2*>(F.xy + 2LL * k);
                if (!(fabsf(p.x - x) < rs && fabsf(p.y - y) < rs)) continue;
                seen = 1;
                if (!keep(k, octave_of(F, k))) continue;
                const int d = hamming32(q, F.desc + 32LL * k);
                if (!within(d)) continue;
                ++count;
                uint32_t kk = ((uint32_t)d << 22) | ((uint32_t)ix << 16) | (uint32_t)min(j - j0, 0xFFFF);
                bool shift = false;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    shift = shift || kk < key[t];
                    if (shift) {
                        const uint32_t tk = key[t];
                        const int ti = kid[t];
                        key[t] = kk, kid[t] = k;
                        kk = tk, k = ti;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < G; o <<= 1) count += __shfl_xor(count, o), seen |= __shfl_xor(seen, o);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t m = key[0];
#pragma unroll
        for (int o = 1; o < G; o <<= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
        const bool mine = m != kAreaNone && key[0] == m;
        int mi = mine ? kid[0] : -1;
#pragma unroll
        for (int o = 1; o < G; o <<= 1) mi = max(mi, __shfl_xor(mi, o));
        idx[t] = mi;
        dist[t] = m != kAreaNone ? (int)(m >> 22) : 256;
        if (mine) {
            key[0] = key[1], key[1] = key[2], key[2] = key[3], key[3] = kAreaNone;
            kid[0] = kid[1], kid[1] = kid[2], kid[2] = kid[3], kid[3] = -1;
        }
    }
    *n = count;
    *any = seen != 0;
}

// Candidate k at distance d into the four lowest (distance, window position) records: the candidates
// come in window order, so k goes after the records of equal distance.
__device__ inline void top4_insert(int32_t idx[4], int32_t dist[4], int k, int d) {
    bool shift = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        shift = shift || d < dist[j];
        if (shift) {
            const int ti = idx[j], td = dist[j];
            idx[j] = k, dist[j] = d;
            k = ti, d = td;
        }
    }
}

// The histogram bin of rot = angle_a - angle_b as ORBmatcher.cc:1829-1837 finds it (no fmodf: the angles
// lie in [0, 360)); false, and *bin as it was, where the reference's assert would fail.
constexpr int kNoBin = 31;  // what the callers keep for such an event, or without an orientation check
__device__ inline bool rot_bin(float angle_a, float angle_b, uint32_t* bin) {
    float rot = angle_a - angle_b;
    if (rot < 0.0f) rot += 360.0f;
    const float rb = roundf(rot * (1.0f / 30));
    if (!(rb >= 0.f && rb <= 30.f)) return false;
    *bin = (uint32_t)(int)rb;
    if (*bin == kRotBins) *bin = 0;
    return true;
}

// ComputeThreeMaxima (ORBmatcher.cc:2061-2102) on hist[0 .. kRotBins) by one lane: hist[kRotBins] = the set of
// bins the rejection (e.g. :1697-1716) clears, hist[kRotBins + 1] = the events in them.
__device__ inline void three_maxima_reject(uint32_t* hist) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int b = 0; b < kRotBins; ++b) {
        const int s = (int)hist[b];
        if (s > max1) {
            max3 = max2, max2 = max1, max1 = s;
            ind3 = ind2, ind2 = ind1, ind1 = b;
        } else if (s > max2) {
            max3 = max2, max2 = s;
            ind3 = ind2, ind2 = b;
        } else if (s > max3) {
            max3 = s, ind3 = b;
        }
    }
    if ((float)max2 < 0.1f * (float)max1) {
        ind2 = -1, ind3 = -1;
    } else if ((float)max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    uint32_t rej = 0;
    int dropped = 0;
    for (int b = 0; b < kRotBins; ++b)
        if (b != ind1 && b != ind2 && b != ind3) rej |= 1u << b, dropped += (int)hist[b];
    hist[kRotBins] = rej;
    hist[kRotBins + 1] = (uint32_t)dropped;
}

}  // namespace orbgpu
