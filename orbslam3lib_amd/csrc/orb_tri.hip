// ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (cpp/src/
// ORBmatcher.cc:908-1153; Pinhole::epipolarConstrain, Pinhole.cpp:102-124; ComputeThreeMaxima
// :2061-2102), the matcher of LocalMapping::CreateNewMapPoints, on pinhole keyframes (mpCamera2 ==
// nullptr, NLeft == -1), over pairs of a batch image whose descriptors, angles and mvKeysUn already
// live in HBM (keyframe 1) and a keyframe the host gives (keyframe 2: descriptor, mvKeysUn position,
// angle, octave, vocabulary node and flags per keypoint).  F12 and the epipole are per-pair inputs.
//
// Only keypoints of the same node are compared (:970-1119), and vbMatched2 (:956) is never set: a
// keypoint of keyframe 2 is never taken, so every keypoint of keyframe 1 is decided on its own.  Of
// the candidates that pass every test other than the distance gate, the loop :1004-1084 keeps the one
// of the lowest distance <= TH_LOW and, among equal distances, the last one (`dist > bestDist`
// continues, an equal distance replaces): the lowest key distance << 16 | (0xFFFF - position).
//   k_tri_group   orb_bow_group.h's ordering of both sides by (node, index); side 0 (keyframe 2) also
//                 packs descriptor, position, angle, octave and flags in that order, so that a node's
//                 candidates are contiguous; side 1 (keyframe 1) packs its descriptors and sets the
//                 pair's match row to -1.
//   k_tri_match   one wave per node segment of keyframe 1.  Keyframe 2's segment of the same node is
//                 found by binary search.  Keyframe 1's keypoints are staged 64 at a time, one per
//                 lane, with their epipolar line (a, b, c, den: Pinhole.cpp:110-116); keyframe 2's
//                 candidates are held 64 at a time, one per lane, with their thresholds and the
//                 epipole-disc test (:1035-1037), which does not depend on keypoint 1.  Per staged
//                 keypoint 1, its descriptor and line wave-uniform (read from its lane): eight
//                 popcounts, the tests, the key, one wave reduction; its lane keeps the lowest key over
//                 the chunks and writes match and bin at the end.  A keypoint 1 belongs to one node,
//                 hence to one wave: no atomics, no taken table, no chain from one keypoint to the next.
//   k_tri_finish  orb_bow_group.h's finish: bin sizes from the stored bins, three_maxima_reject, the
//                 rejected matches cleared (:1121-1140), nmatches.
//
// Deviations from the reference: a negative node means "in no node"; an event whose bin falls
// outside [0, 30) (the reference asserts) counts in nmatches, enters no bin and cannot be rejected.
#include <hip/hip_runtime.h>

#include "orb_bow_group.h"

namespace orbgpu {
namespace {

constexpr int kTriWaves = 128;  // waves per pair in k_tri_match, each striding over the segments (k_bow_match's)

__global__ __launch_bounds__(kGroupThreads) void k_tri_group(TriArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // [npad]
    bow_group_body(a, keys, [&a](const uint64_t* keys, int m, int n) {
        const int o0 = a.kf_off[blockIdx.x];
        const TriPoint* kf = a.kf_pts + o0;
        for (int j = threadIdx.x; j < m; j += kGroupThreads) {
            const TriPoint& pt = kf[min((int)(uint32_t)keys[j], n - 1)];
            a.kf_desc[2LL * (o0 + j)] = make_uint4(pt.desc[0], pt.desc[1], pt.desc[2], pt.desc[3]);
            a.kf_desc[2LL * (o0 + j) + 1] = make_uint4(pt.desc[4], pt.desc[5], pt.desc[6], pt.desc[7]);
            const int bits = (clampi(pt.octave, 0, kMaxLevels - 1) << 8) | (pt.flags & (kTriHasPoint | kTriStereo));
            a.kf_meta[o0 + j] = make_float4(pt.x, pt.y, pt.angle, __int_as_float(bits));
        }
    });
}

__device__ inline float lane_float(float v, int j) { return __uint_as_float(lane_value(__float_as_uint(v), j)); }

__global__ __launch_bounds__(64) void k_tri_match(TriArgs a) {
    const int p = blockIdx.y, lane = threadIdx.x, cap = a.out_cap;
    const BowSide K = bow_kf_side(a, p), F = bow_f_side(a, p);
    const int nsegK = clampi(a.nseg[2 * p], 0, K.n), nsegF = clampi(a.nseg[2 * p + 1], 0, F.n);
    const int o0 = a.kf_off[p], img = a.frames[p];
    const uint4* kdesc = a.kf_desc + 2LL * o0;
    const float4* kmeta = a.kf_meta + o0;
    const uint8_t* fdesc = a.f_desc + 32LL * p * cap;
    const uint8_t* fkps = static_cast<const uint8_t*>(a.kps) + 28LL * img * cap;
    const float* fxy = a.xy_un + 2LL * img * cap;
    const uint8_t* fflags = a.f_flags ? a.f_flags + (long long)p * cap : nullptr;
    const TriPair& P = a.pairs[p];
    int32_t* match = a.match + (long long)p * cap;
    uint8_t* mbin = a.match_bin + (long long)p * cap;
    for (int s = blockIdx.x; s < nsegF; s += gridDim.x) {
        const int sk = find_segment(K.seg_node, nsegK, F.seg_node[s], lane);  // keyframe 2's segment of the node
        if (sk < 0) continue;  // a node of keyframe 1 only
        const int fs = clampi(F.seg_start[s], 0, F.n), fe = clampi(F.seg_start[s + 1], fs, F.n);
        const int ks = clampi(K.seg_start[sk], 0, K.n), nk = clampi(K.seg_start[sk + 1], ks, K.n) - ks;
        for (int i0 = fs; i0 < fe; i0 += 64) {  // :974, idx1 ascending, 64 keypoints 1 staged per lane
            uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int idx1 = 0, flags1 = kTriHasPoint;  // lanes beyond the segment: skipped
            float la = 0.f, lb = 0.f, lc = 0.f, den = 0.f;
            if (i0 + lane < fe) {
                idx1 = clampi(F.order[i0 + lane], 0, F.n - 1);
                flags1 = fflags ? fflags[idx1] : 0;
                const uint4* d = reinterpret_cast<const uint4*>(fdesc + 32LL * (i0 + lane));
                const uint4 x = d[0], y = d[1];
                qd[0] = x.x, qd[1] = x.y, qd[2] = x.z, qd[3] = x.w, qd[4] = y.x, qd[5] = y.y, qd[6] = y.z, qd[7] = y.w;
                const float2 pt = *reinterpret_cast<const float2*>(fxy + 2LL * idx1);
                la = (pt.x * P.F12[0] + pt.y * P.F12[3]) + P.F12[6];  // Pinhole.cpp:110-112
                lb = (pt.x * P.F12[1] + pt.y * P.F12[4]) + P.F12[7];
                lc = (pt.x * P.F12[2] + pt.y * P.F12[5]) + P.F12[8];
                den = la * la + lb * lb;  // :116
            }
            const bool stereo1 = (flags1 & kTriStereo) != 0;
            const bool search1 = !(flags1 & kTriHasPoint) && (!a.only_stereo || stereo1);  // :981-990
            const uint64_t todo0 = __ballot(search1);
            uint32_t best = kNoKey;  // this lane's keypoint 1: its lowest key over the chunks
            for (int c0 = 0; todo0 && c0 < nk; c0 += 64) {  // keyframe 2's candidates, one per lane
                const int pos = c0 + lane;
                uint32_t d2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                float x2 = 0.f, y2 = 0.f;
                double epi_th = 0.0;
                bool cand = false, stereo2 = false, in_disc = false;
                if (pos < nk) {
                    const uint4 x = kdesc[2LL * (ks + pos)], y = kdesc[2LL * (ks + pos) + 1];
                    d2[0] = x.x, d2[1] = x.y, d2[2] = x.z, d2[3] = x.w, d2[4] = y.x, d2[5] = y.y, d2[6] = y.z, d2[7] = y.w;
                    const float4 mt = kmeta[ks + pos];
                    const int bits = __float_as_int(mt.w), oct = clampi(bits >> 8, 0, kMaxLevels - 1);
                    x2 = mt.x, y2 = mt.y;
                    stereo2 = (bits & kTriStereo) != 0;
                    cand = !(bits & kTriHasPoint) && (!a.only_stereo || stereo2);  // :1011-1018
                    epi_th = a.epi_th[oct];
                    const float ex = P.ep[0] - x2, ey = P.ep[1] - y2;  // :1035-1037
                    in_disc = ex * ex + ey * ey < a.disc_th[oct];
                }
                for (uint64_t todo = todo0; todo; todo &= todo - 1) {
                    const int j = __builtin_ctzll(todo);
                    int dist = 0;
#pragma unroll
                    for (int w = 0; w < 8; ++w) dist += __popc(lane_value(qd[w], j) ^ d2[w]);
                    const float ja = lane_float(la, j), jb = lane_float(lb, j), jc = lane_float(lc, j);
                    const float jden = lane_float(den, j);
                    const bool jstereo = (lane_value((uint32_t)flags1, j) & kTriStereo) != 0;
                    bool ok = cand && dist <= kThLow;           // :1024: the gate against bestDist is the key's order
                    ok = ok && (jstereo || stereo2 || !in_disc);  // :1033-1041
                    if (!a.coarse) {  // Pinhole.cpp:114-123; the comparison is in double
                        const float num = (ja * x2 + jb * y2) + jc;
                        const float dsqr = num * num / jden;
                        ok = ok && jden != 0.f && (double)dsqr < epi_th;
                    }
                    const uint32_t low = wave_min(ok ? ((uint32_t)dist << 16) | (uint32_t)(0xFFFF - pos) : kNoKey);
                    if (lane == j) best = min(best, low);
                }
            }
            if (best != kNoKey) {  // :1086-1105
                const int pos = 0xFFFF - (int)(best & 0xFFFFu);
                uint32_t bin = kNoBin;
                if (a.check_orientation)
                    rot_bin(*reinterpret_cast<const float*>(fkps + 28LL * idx1 + 12), kmeta[ks + pos].z, &bin);
                match[idx1] = clampi(K.order[ks + pos], 0, K.n - 1);
                mbin[idx1] = (uint8_t)bin;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_tri_finish(TriArgs a) { bow_finish_body(a); }

}  // namespace

hipError_t launch_tri_search(const TriArgs& a, int npairs, int max_side, hipStream_t st) {
    if (npairs <= 0) return hipSuccess;
    size_t lds;
    if (const hipError_t e = bow_group_lds(k_tri_group, max_side, &lds)) return e;
    hipLaunchKernelGGL(k_tri_group, dim3(npairs, 2), dim3(kGroupThreads), lds, st, a);
    hipLaunchKernelGGL(k_tri_match, dim3(kTriWaves, npairs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_tri_finish, dim3(npairs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace orbgpu
