"""ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) -- the matcher
of LocalMapping::CreateNewMapPoints (cpp/src/ORBmatcher.cc:908-1153, with Pinhole::epipolarConstrain,
CameraModels/Pinhole.cpp:102-124, and ComputeThreeMaxima :2061-2102), pinhole keyframes (mpCamera2 ==
nullptr, NLeft == -1).  Keyframe 1 is a batch image, keyframe 2 is given by the host; the vocabulary
stays on the host (the node of each keypoint is an input on both sides), and so do F12 and the epipole.

The yardstick is _py_tri below: a literal sequential transcription of those lines with np.float32
scalars, which also returns a Counter of the rules it hit.  It runs the reference's loop -- bestDist
from TH_LOW down, `dist > bestDist` continues, an equal distance replaces -- and not the closed form
the kernel computes (the eligible candidate of the lowest distance <= 50 with the highest index), so
that the GPU cases check that equivalence.
CPU: the restatement against hand-built known answers (one rule each); conditions on the scenes the
GPU cases use; the exported symbols, struct layouts and the statuses decided before any launch.
GPU: k_tri_group + k_tri_match + k_tri_finish against the restatement, equal on match12, nmatches and
the 30 histogram bins, with no tolerance.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs the SLAM stack; no
fixtures ship for it) -- restatement only, as for the other matcher functions."""
from collections import Counter, namedtuple

import numpy as np
import pytest

from orbslam3lib_amd import TRI_HAS_POINT, TRI_STEREO, TRIANG_PAIR_DTYPE, TRIANG_POINT_DTYPE, synth
from tests.test_search_by_bow import (BOW_MAX_POINTS, CHUNK_N, FB, KF, NODE_MAX, TH_LOW, _cell_nodes, _desc_nodes, _env,
                                      _feat_vec, _hamming_matrix, _kf_points, _py_bow)
from tests.test_search_for_initialization import RNG_D, Fr, _bits, _images
from tests.test_track_projection import D_, F32, K_, _flip, _header_struct_bytes, _rot_bin, _three_maxima

HAS_POINT, STEREO = TRI_HAS_POINT, TRI_STEREO  # ORBGPU_TRI_HAS_POINT, ORBGPU_TRI_STEREO

K1 = namedtuple("K1", "desc xy ang node flag")       # keyframe 1: mDescriptors, mvKeysUn.pt / .angle, node, flags
K2 = namedtuple("K2", "desc xy ang octv node flag")  # keyframe 2: the same and mvKeysUn.octave


def _levels(nlevels=8, scale_factor=1.2):
    """mvScaleFactors, mvLevelSigma2 (ORBextractor.cc:417-424: a float table, a double factor)."""
    sf = float(F32(scale_factor))
    scale = [F32(1.0)]
    for _ in range(1, nlevels):
        scale.append(F32(float(scale[-1]) * sf))
    return scale, [s * s for s in scale]


SCALE, SIGMA2 = _levels()


def _epipolar(x1, y1, x2, y2, F, unc):
    """Pinhole::epipolarConstrain (Pinhole.cpp:110-123) with F12 given; every operand is an np.float32."""
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    dsqr = num * num / den
    return bool(float(dsqr) < 3.84 * float(unc))  # the double literal: product and comparison in double


def _py_tri(k1, k2, F12, ep, only_stereo=False, coarse=False, check=False, scale=SCALE, sigma2=SIGMA2):
    """-> vMatches12 [N1] (index into keyframe 2's points or -1), nmatches, bin sizes [30] (before the
    three-maxima rule), Counter of the rules."""
    n1 = len(k1.node)
    match = [-1] * n1  # :957
    H = _hamming_matrix(k1.desc, k2.desc)
    fv1, fv2 = _feat_vec(k1.node), _feat_vec(k2.node)
    F = np.asarray(F12, F32).reshape(3, 3)
    ep = np.asarray(ep, F32).reshape(2)
    xy1, xy2 = np.asarray(k1.xy, F32).reshape(-1, 2), np.asarray(k2.xy, F32).reshape(-1, 2)
    flag1, flag2 = [int(f) for f in k1.flag], [int(f) for f in k2.flag]
    bins = [[] for _ in range(30)]
    cnt = Counter()
    nm = 0
    with np.errstate(all="ignore"):
        for node in sorted(fv1):  # :970-1119: the nodes present in both, ascending
            if node not in fv2:
                continue
            cnt["common_nodes"] += 1
            cnt["max_seg_1"] = max(cnt["max_seg_1"], len(fv1[node]))
            cnt["max_seg_2"] = max(cnt["max_seg_2"], len(fv2[node]))
            for idx1 in fv1[node]:  # :974
                if flag1[idx1] & HAS_POINT:  # :978-984
                    cnt["has_point_1"] += 1
                    continue
                stereo1 = bool(flag1[idx1] & STEREO)  # :986
                if only_stereo and not stereo1:  # :988-990
                    cnt["mono_skipped_1"] += 1
                    continue
                x1, y1 = xy1[idx1]
                row = H[idx1].tolist()
                best_dist, best_idx2 = TH_LOW, -1  # :1001-1002
                for idx2 in fv2[node]:  # :1004
                    if flag2[idx2] & HAS_POINT:  # :1008-1012 (vbMatched2 is never set)
                        cnt["has_point_2"] += 1
                        continue
                    stereo2 = bool(flag2[idx2] & STEREO)  # :1014
                    if only_stereo and not stereo2:  # :1016-1018
                        cnt["mono_skipped_2"] += 1
                        continue
                    dist = row[idx2]
                    if dist > TH_LOW or dist > best_dist:  # :1024
                        continue
                    x2, y2 = xy2[idx2]
                    octave2 = int(k2.octv[idx2])
                    if not stereo1 and not stereo2:  # :1033-1041
                        dx = ep[0] - x2
                        dy = ep[1] - y2
                        if dx * dx + dy * dy < F32(100) * scale[octave2]:
                            cnt["epipole_disc"] += 1
                            continue
                    if not (coarse or _epipolar(x1, y1, x2, y2, F, sigma2[octave2])):  # :1079
                        cnt["epipolar_rejected"] += 1
                        continue
                    if best_idx2 >= 0:  # instrumentation only
                        cnt["equal_replaced" if dist == best_dist else "closer_replaced"] += 1
                    best_idx2, best_dist = idx2, dist  # :1081-1082
                if best_idx2 < 0:  # :1086
                    continue
                cnt["events"] += 1
                match[idx1] = best_idx2  # :1091
                nm += 1  # :1092
                if check:  # :1094-1104
                    bn = _rot_bin(k1.ang[idx1], k2.ang[best_idx2])
                    if bn is None:  # deviation
                        cnt["bin_out_of_range"] += 1
                    else:
                        bins[bn].append(idx1)
    partners = Counter(m for m in match if m >= 0)
    cnt["shared"] = sum(1 for v in partners.values() if v > 1)  # keypoints 2 matched more than once
    hist = np.array([len(e) for e in bins], np.int32)
    if check:  # :1121-1140
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn in keep:
                continue
            for idx1 in bins[bn]:
                match[idx1] = -1
                nm -= 1
                cnt["rejected"] += 1
    return np.array(match, np.int32).reshape(-1), nm, hist, cnt


# ---- hand-built keyframes -----------------------------------------------------------------------

# x1' F x2 = y2 - y1: a = 0, b = 1, c = -y1, den = 1, dsqr = (y2 - y1)^2
F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)
FAR = (F32(-1000.0), F32(-1000.0))  # an epipole away from every keypoint


def _k1(points):
    """points: (desc [32] u8, x, y, angle, node[, flags = 0])."""
    return K1(np.array([p[0] for p in points], np.uint8).reshape(-1, 32), np.array([p[1:3] for p in points], F32).reshape(-1, 2),
              np.array([p[3] for p in points], F32), np.array([p[4] for p in points], np.int64),
              np.array([p[5] if len(p) > 5 else 0 for p in points], np.int32))


def _k2(points):
    """points: (desc [32] u8, x, y, angle, octave, node[, flags = 0])."""
    return K2(np.array([p[0] for p in points], np.uint8).reshape(-1, 32), np.array([p[1:3] for p in points], F32).reshape(-1, 2),
              np.array([p[3] for p in points], F32), np.array([p[4] for p in points], np.int32),
              np.array([p[5] for p in points], np.int64), np.array([p[6] if len(p) > 6 else 0 for p in points], np.int32))


Z = _bits()


def test_the_later_of_two_equal_distances_wins():
    k2 = _k2([(_bits((0, 7)), 10, 50, 0.0, 0, 3), (_bits((7, 14)), 20, 50, 0.0, 0, 3), (_bits((14, 22)), 30, 50, 0.0, 0, 3)])
    m, nm, _, cnt = _py_tri(_k1([(Z, 5, 50, 0.0, 3)]), k2, F_ROWS, FAR)
    assert list(m) == [1] and nm == 1 and cnt["equal_replaced"] == 1  # 7, 7, 8: the second 7 replaces the first
    # SearchByBoW's strict < keeps the first on the same descriptors
    kf = KF(k2.desc, k2.ang, k2.node, np.ones(3, np.int32))
    assert list(_py_bow(kf, FB(Z.reshape(1, 32), np.zeros(1, F32), np.array([3])), 1.5, False)[0]) == [0]


def test_one_keypoint_2_is_matched_by_two_keypoints_1():
    D = RNG_D[0]
    k1 = _k1([(_flip(D, 3), 5, 50, 0.0, 1), (_flip(D, 5, 1), 8, 50, 0.0, 1)])
    m, nm, _, cnt = _py_tri(k1, _k2([(D, 10, 50, 0.0, 0, 1)]), F_ROWS, FAR)
    assert list(m) == [0, 0] and nm == 2 and cnt["shared"] == 1 and cnt["events"] == 2


def test_distance_50_passes_and_51_fails():
    for nbits, want in ((50, 1), (51, 0)):
        _, nm, _, _ = _py_tri(_k1([(Z, 5, 50, 0.0, 0)]), _k2([(_bits((0, nbits)), 10, 50, 0.0, 0, 0)]), F_ROWS, FAR)
        assert nm == want


def test_a_closer_candidate_that_fails_a_test_does_not_block_a_farther_one():
    k1 = _k1([(Z, 5, 50, 0.0, 2)])
    # the closer one lies 3 rows off: 9 > 3.84; the farther one on the row
    k2 = _k2([(_bits((0, 4)), 10, 53, 0.0, 0, 2), (_bits((0, 30)), 20, 50, 0.0, 0, 2)])
    m, nm, _, cnt = _py_tri(k1, k2, F_ROWS, FAR)
    assert list(m) == [1] and nm == 1 and cnt["epipolar_rejected"] == 1
    assert list(_py_tri(k1, k2, F_ROWS, FAR, coarse=True)[0]) == [0]
    # the same with the closer one inside the epipole disc (both on the row)
    k2 = _k2([(_bits((0, 4)), 10, 50, 0.0, 0, 2), (_bits((0, 30)), 40, 50, 0.0, 0, 2)])
    m, nm, _, cnt = _py_tri(k1, k2, F_ROWS, (F32(12.0), F32(50.0)))
    assert list(m) == [1] and nm == 1 and cnt["epipole_disc"] == 1 and cnt["epipolar_rejected"] == 0
    # in the other visiting order too: bestDist only ever holds an eligible candidate's distance
    m, _, _, cnt = _py_tri(k1, K2(*(v[::-1] for v in k2)), F_ROWS, (F32(12.0), F32(50.0)))
    assert list(m) == [0] and cnt["epipole_disc"] == 1


def test_the_epipole_disc_uses_octave_2_strict_less_and_needs_two_mono_keypoints():
    assert F32(100) * SCALE[0] == F32(100) and F32(100) * SCALE[2] > F32(121)
    k1 = _k1([(Z, 5, 50, 0.0, 0)])
    ep = (F32(0.0), F32(50.0))

    def nm(x2, octave, f1=0, f2=0, coarse=True):
        return _py_tri(k1._replace(flag=np.array([f1])), _k2([(Z, x2, 50, 0.0, octave, 0, f2)]), F_ROWS, ep, coarse=coarse)[1]
    assert nm(10, 0) == 1   # 100 < 100 is false
    assert nm(9.5, 0) == 0  # 90.25 < 100
    assert nm(11, 0) == 1 and nm(11, 2) == 0  # 121 < 100 * 1.44: keypoint 2's octave
    assert nm(9.5, 0, f1=STEREO) == 1 and nm(9.5, 0, f2=STEREO) == 1 and nm(9.5, 0, STEREO, STEREO) == 1
    assert nm(9.5, 0, coarse=False) == 0 and nm(9.5, 0, f1=STEREO, coarse=False) == 1


def test_a_zero_f12_matches_nothing_unless_coarse():
    k1, k2 = _k1([(Z, 5, 50, 0.0, 0)]), _k2([(Z, 10, 50, 0.0, 0, 0)])
    m, nm, _, cnt = _py_tri(k1, k2, np.zeros(9, F32), FAR)
    assert nm == 0 and cnt["epipolar_rejected"] == 1  # den == 0
    assert _py_tri(k1, k2, np.zeros(9, F32), FAR, coarse=True)[1] == 1
    # a NaN dsqr fails too
    assert _py_tri(k1, k2, np.full(9, np.inf, F32), FAR)[1] == 0


def test_the_epipolar_comparison_is_in_double():
    v = F32(1.9595917463302612)
    dsqr = v * v / F32(1.0)
    assert dsqr == F32(3.84) and type(dsqr) is F32
    in_float = bool(dsqr < F32(3.84) * SIGMA2[0])
    in_double = bool(float(dsqr) < 3.84 * float(SIGMA2[0]))
    assert in_double and not in_float  # float32(3.84) lies below the double 3.84
    # a = 0, b = 1, c = F(2,2) = v with keypoint 1 at the origin and y2 = 0: num = v, den = 1
    F = np.array([[0, 0, 0], [0, 0, 0], [0, 1, v]], F32)
    k1, k2 = _k1([(Z, 0, 0, 0.0, 0)]), _k2([(Z, 300, 0, 0.0, 0, 0)])
    assert _py_tri(k1, k2, F, FAR)[1] == 1
    F[2, 2] = np.nextafter(v, F32(2.0), dtype=F32)
    assert _py_tri(k1, k2, F, FAR)[1] == 0
    # unc is keyframe 2's level: at octave 1 the bound is 3.84 * 1.44
    assert _py_tri(k1, k2._replace(octv=np.array([1])), F, FAR)[1] == 1


def test_only_stereo_skips_mono_keypoints_on_both_sides():
    D = RNG_D
    k1 = _k1([(D[0], 5, 50, 0.0, 0, 0), (D[1], 5, 60, 0.0, 0, STEREO)])
    k2 = _k2([(D[0], 9, 50, 0.0, 0, 0, STEREO), (D[1], 9, 60, 0.0, 0, 0, 0), (_flip(D[1], 9), 19, 60, 0.0, 0, 0, STEREO)])
    assert list(_py_tri(k1, k2, F_ROWS, FAR)[0]) == [0, 1]
    m, nm, _, cnt = _py_tri(k1, k2, F_ROWS, FAR, only_stereo=True)
    assert list(m) == [-1, 2] and nm == 1 and cnt["mono_skipped_1"] == 1 and cnt["mono_skipped_2"] == 1


def test_a_map_point_on_either_side_skips_the_keypoint():
    D = RNG_D[2]
    k2 = _k2([(D, 9, 50, 0.0, 0, 4, HAS_POINT), (_flip(D, 6), 19, 50, 0.0, 0, 4, 0)])
    m, nm, _, cnt = _py_tri(_k1([(D, 5, 50, 0.0, 4)]), k2, F_ROWS, FAR)
    assert list(m) == [1] and nm == 1 and cnt["has_point_2"] == 1
    m, nm, _, cnt = _py_tri(_k1([(D, 5, 50, 0.0, 4, HAS_POINT)]), k2, F_ROWS, FAR)
    assert list(m) == [-1] and nm == 0 and cnt["has_point_1"] == 1
    # HAS_POINT | STEREO is still a map point
    assert _py_tri(_k1([(D, 5, 50, 0.0, 4, HAS_POINT | STEREO)]), k2, F_ROWS, FAR)[1] == 0


def test_nodes_of_one_side_negative_unsorted_and_very_large_ids():
    D = RNG_D
    nodes1 = [NODE_MAX, 5, -1, 7, 0, 1 << 30, -7]
    nodes2 = [0, 9, -1, 5, NODE_MAX, -7, 1 << 30, NODE_MAX - 1]
    k1 = _k1([(D[i], 5, 50, 0.0, nd) for i, nd in enumerate(nodes1)])
    k2 = _k2([(D[i], 9, 50, 0.0, 0, nd) for i, nd in zip((4, 3, 2, 1, 0, 6, 5, 0), nodes2)])
    m, nm, _, cnt = _py_tri(k1, k2, F_ROWS, FAR)
    # node 7 is keyframe 1's only, 9 and NODE_MAX - 1 keyframe 2's only; equal negative values are no node
    assert list(m) == [4, 3, -1, -1, 0, 6, -1] and nm == 4 and cnt["common_nodes"] == 4


@pytest.mark.parametrize("a1,a2,expect", [(14.9, 0.0, 0), (15.0, 0.0, 1), (359.0, 0.0, 12), (0.0, 0.5, 12),
                                          (44.9, 0.0, 1), (45.1, 0.0, 2), (10.0, 350.0, 1)])
def test_rotation_bin_edges(a1, a2, expect):
    """rot = keyframe 1's angle - keyframe 2's angle, the factor is 1 / 30, 30 -> 0, no fmodf."""
    D = RNG_D[1]
    _, nm, hist, _ = _py_tri(_k1([(D, 5, 50, a1, 0)]), _k2([(D, 9, 50, a2, 0, 0)]), F_ROWS, FAR, check=True)
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1


def _bin_scene(sizes, extra1=(), extra2=()):
    """{bin: events}: every event in a node of its own."""
    p1, p2, k = list(extra1), list(extra2), 0
    for bn, n in sizes.items():
        for _ in range(n):
            p1.append((RNG_D[k], 5, 50, 30.0 * bn, 100 + k))
            p2.append((RNG_D[k], 9, 50, 0.0, 0, 100 + k))
            k += 1
    return _k1(p1), _k2(p2)


def test_three_maxima_ties_and_cutoffs():
    def scene(sizes):
        return _py_tri(*_bin_scene(sizes), F_ROWS, FAR, check=True)
    # strict >: the earlier bins win the tie, the fourth is rejected
    m, nm, hist, cnt = scene({2: 5, 5: 5, 7: 5, 9: 5})
    assert list(hist[[2, 5, 7, 9]]) == [5, 5, 5, 5] and nm == 15 and cnt["rejected"] == 5 and (m[15:] == -1).all()
    assert scene({0: 10, 3: 1})[1] == 11  # exactly 10%: 0.1f * 10.0f rounds to 1.0f
    _, nm, _, cnt = scene({4: 22, 1: 2, 8: 2})  # max2 below 10%: the second and the third are dropped together
    assert nm == 22 and cnt["rejected"] == 4
    assert scene({4: 22, 1: 3, 8: 2})[1] == 25  # only max3 below 10%


def test_the_bin_out_of_range_deviation_and_no_orientation_check():
    D = RNG_D
    k1, k2 = _bin_scene({1: 11}, [(D[40], 5, 50, 1000.0, 1), (D[41], 5, 50, 150.0, 2)],
                        [(D[40], 9, 50, 0.0, 0, 1), (D[41], 9, 50, 0.0, 0, 2)])
    m, nm, hist, cnt = _py_tri(k1, k2, F_ROWS, FAR, check=True)
    assert cnt["bin_out_of_range"] == 1 and hist.sum() == 12 and hist[1] == 11 and hist[5] == 1
    assert cnt["rejected"] == 1 and m[0] == 0 and m[1] == -1 and nm == 12
    k1.ang[0] = np.nan
    assert _py_tri(k1, k2, F_ROWS, FAR, check=True)[1] == 12
    # no orientation check (the default of CreateNewMapPoints' ORBmatcher(0.6, false)): no bins, nothing rejected
    m, nm, hist, cnt = _py_tri(k1, k2, F_ROWS, FAR, check=False)
    assert hist.sum() == 0 and nm == 13 and cnt["rejected"] == 0 and (m >= 0).all()


# ---- ABI ----------------------------------------------------------------------------------------

def test_symbols_layouts_and_statuses_decided_before_any_launch():
    import orbslam3lib_amd as og
    names = {"orbgpu_search_for_triangulation_batch", "orbgpu_download_triangulation_matches"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "search_for_triangulation") and hasattr(og.BatchExtractor, "triangulation_matches")
    assert og.TRIANG_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_triang_point") == 56
    assert og.TRIANG_PAIR_DTYPE.itemsize == _header_struct_bytes("orbgpu_triang_pair") == 44
    assert [og.TRIANG_POINT_DTYPE.fields[f][1] for f in ("desc", "x", "y", "angle", "octave", "node", "flags")] == \
        [0, 32, 36, 40, 44, 48, 52]
    assert [og.TRIANG_PAIR_DTYPE.fields[f][1] for f in ("F12", "ep")] == [0, 36]
    assert (og.TRI_HAS_POINT, og.TRI_STEREO) == (HAS_POINT, STEREO) == (1, 2)
    txt = open(og.os.path.join(og.os.path.dirname(og.HERE), "include", "orbgpu.h")).read()
    assert "#define ORBGPU_TRI_HAS_POINT 1" in txt and "#define ORBGPU_TRI_STEREO 2" in txt
    one = np.zeros(1, np.int32)
    assert lib.orbgpu_search_for_triangulation_batch(None, 1, og._p(one), None, None, None, None, 0, None, 0, 0, 0, 0, None) == -3
    assert lib.orbgpu_search_for_triangulation_batch(None, 0, None, None, None, None, None, 0, None, 0, 0, 0, 0, None) == -3
    assert lib.orbgpu_download_triangulation_matches(None, 0, None, 0, None, None, None) == -3
    # the wrapper refuses lists that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, og.TRIANG_POINT_DTYPE)
    pr = np.zeros(2, og.TRIANG_PAIR_DTYPE)
    nodes, flags = np.zeros(4, np.int32), np.zeros(4, np.uint8)
    for args in (([0, 1], [pts], pr, [nodes, nodes]),                                         # keyframes
                 ([0, 1], [pts, pts], pr[:1], [nodes, nodes]),                                # pairs
                 ([0, 1], [pts, pts], pr, [nodes]),                                           # node rows
                 ([0, 1], [pts, pts], pr, np.zeros((3, 4), np.int32)),
                 ([0, 1], [pts, pts], pr, [nodes, nodes], [flags]),                           # flag rows
                 ([0, 1], (pts, np.array([0, 3], np.int32)), pr, [nodes, nodes]),             # offsets
                 ([0], (pts, np.array([0, 4], np.int32)), pr[:1], [nodes])):                  # offsets beyond the points
        with pytest.raises(ValueError):
            be.search_for_triangulation(*args)


# ---- scenes -------------------------------------------------------------------------------------

def _f12(K, R, t):
    """K1^-T * [t12]x * R12 * K2^-1 (Pinhole.cpp:104-107) with both cameras K, in float32 products."""
    fx, fy, cx, cy = (F32(v) for v in K)
    one, zero = F32(1), F32(0)
    Kinv = np.array([[one / fx, zero, -cx / fx], [zero, one / fy, -cy / fy], [zero, zero, one]], F32)
    t = [F32(v) for v in t]
    tx = np.array([[zero, -t[2], t[1]], [t[2], zero, -t[0]], [-t[1], t[0], zero]], F32)
    F = ((Kinv.T @ tx) @ np.asarray(R, F32).reshape(3, 3)) @ Kinv
    assert F.dtype == F32
    return F


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F32)


F_STEREO = _f12(K_, np.eye(3), (0.11, 0.0, 0.0))  # R = I, t = (b, 0, 0): the epipolar lines are the image rows


def _dense_spot(k1, k2):
    """Where the tests aim the epipole: the searchable mono keypoint of keyframe 2 with the most of its
    kind within 8 pixels, among those within TH_LOW of some searchable mono keypoint of keyframe 1 in
    their node (the candidates the disc test :1033-1041 can meet)."""
    free1, free2 = np.asarray(k1.flag) == 0, np.asarray(k2.flag) == 0
    near = (_hamming_matrix(k2.desc, k1.desc) <= TH_LOW) & (np.asarray(k2.node)[:, None] == np.asarray(k1.node)[None, :])
    hit = np.flatnonzero(free2 & (np.asarray(k2.node) >= 0) & (near & free1[None, :]).any(1))
    if len(hit) == 0:
        return np.array([-1000.0, -1000.0], F32)
    xy = np.asarray(k2.xy, np.float64)[hit]
    d = xy[:, None, :] - xy[None, :, :]
    return np.asarray(k2.xy[hit[int(np.argmax(((d * d).sum(-1) < 64.0).sum(1)))]], F32)


def _flags(n, stereo_every=7):
    """A map point on every fifth keypoint, a stereo keypoint on every stereo_every-th."""
    i = np.arange(n)
    return ((i % 5 == 4) * HAS_POINT | (i % stereo_every == 1) * STEREO).astype(np.int32)


# name -> (keyframe 1's image (the batch image), keyframe 2's image, nodes, geometry, only_stereo, coarse,
# check_orientation); geometry "rows": F_STEREO with the epipole on keyframe 2's densest spot
SCENES = {
    "left_right": ("L0", "R0", "cell", "rows", False, False, False),
    "left_right_coarse": ("L0", "R0", "cell", "rows", False, True, False),
    "left_right_only_stereo": ("L0", "R0", "cell", "rows", True, False, False),
    "unrelated": ("L0", "L1", "cell", "rows", False, False, True),
    "one_node": ("L0", "R0", "one", "rows", False, False, True),
    "tiled": ("T0", "TQ", "desc", "rows", False, True, True),
    "tiled_rows": ("T0", "TQ", "desc", "rows", False, False, False),
    "rotated_180": ("L0", "rot", "desc", "rows", False, True, True),
    "sparse": ("T0", "TQ", "sparse", "rows", False, True, True),
}
SCENES.update({"seg2_%d" % n: ("T0", "TQ", ("second", n), "rows", False, True, True) for n in CHUNK_N})
SCENES.update({"seg1_%d" % n: ("T0", "TQ", ("first", n), "rows", False, True, True) for n in CHUNK_N})
ENV1 = ("left_right", "left_right_coarse", "left_right_only_stereo", "unrelated", "one_node")  # images L0 R0 L1 R1


def _scene(frames, name):
    """-> (K1, K2, F12, ep, only_stereo, coarse, check) of a scene on frames (Fr records by image name)."""
    i1, i2, nodes, _, only_stereo, coarse, check = SCENES[name]
    A, B = frames[i1], frames[i2]
    n1, n2 = len(A.ang), len(B.ang)
    if nodes == "desc":
        nd1, nd2 = _desc_nodes(A), _desc_nodes(B)
    elif nodes == "cell":
        nd1, nd2 = _cell_nodes(A), _cell_nodes(B)
    elif nodes == "one":
        nd1, nd2 = np.zeros(n1, np.int64), np.zeros(n2, np.int64)
    elif nodes == "sparse":
        nd1, nd2 = _desc_nodes(A), _desc_nodes(B)
        nd1 = np.where(nd1 % 2 == 0, nd1 * 1000003 % NODE_MAX, -1)
        nd2 = np.where(nd2 % 3 == 0, nd2 * 1000003 % NODE_MAX, -1)
    elif nodes[0] == "second":  # keyframe 2's segment of nodes[1] keypoints, keyframe 1 whole
        nd1 = np.full(n1, 7, np.int64)
        nd2 = np.where(np.arange(n2) < nodes[1], 7, -1).astype(np.int64)
    else:
        nd1 = np.where(np.arange(n1) < nodes[1], 7, -1).astype(np.int64)
        nd2 = np.full(n2, 7, np.int64)
    every = 3 if only_stereo else 7
    k1 = K1(A.desc, A.xy, A.ang, nd1, _flags(n1, every))
    k2 = K2(B.desc, B.xy, B.ang, B.octv, nd2, _flags(n2, every)[::-1].copy())
    return k1, k2, F_STEREO, _dense_spot(k1, k2), only_stereo, coarse, check


@pytest.fixture(scope="module")
def cpu_frames(oracle):
    imgs = _images()
    frames = {}
    for k in ("L0", "R0", "L1", "rot", "T0", "TQ"):
        kps, desc, _ = oracle.extract(imgs[k], nfeatures=1000)
        xy, _, _, cs, ci = oracle.undistort_grid(kps, K_, D_, 640, 480)
        frames[k] = Fr(xy, kps["octave"].astype(np.int32), kps["angle"].astype(F32), desc.reshape(-1, 32), cs, ci)
    return frames


def test_scenes_exercise_every_rule(cpu_frames):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the
    oracle's extraction at 1000 features, meets every situation the GPU cases are there to compare."""
    res = {}
    for name in SCENES:
        args = _scene(cpu_frames, name)
        res[name] = _py_tri(*args)
        print(name, "nmatches", res[name][1], dict(res[name][3]), "bins", np.flatnonzero(res[name][2]).tolist())
    c = res["left_right"][3]
    assert c["events"] >= 200 and c["epipolar_rejected"] >= 8 and c["epipole_disc"] >= 4 and c["shared"] >= 15
    assert c["has_point_1"] >= 100 and c["has_point_2"] >= 1500 and c["closer_replaced"] >= 25
    c2 = res["left_right_coarse"][3]
    assert c2["events"] > c["events"] and c2["epipolar_rejected"] == 0 and c2["epipole_disc"] >= 4
    c = res["left_right_only_stereo"][3]
    assert c["events"] >= 25 and c["mono_skipped_1"] >= 300 and c["mono_skipped_2"] >= 1500 and c["epipole_disc"] == 0
    assert res["unrelated"][1] == 0 and res["unrelated"][3]["events"] == 0 and res["unrelated"][3]["common_nodes"] >= 40
    c = res["one_node"][3]  # the longest segments, far above one wave on both sides
    assert c["max_seg_1"] == len(cpu_frames["L0"].ang) >= 500 and c["max_seg_2"] == len(cpu_frames["R0"].ang) >= 500
    assert c["events"] >= 250 and c["epipolar_rejected"] >= 35 and c["epipole_disc"] >= 4 and c["rejected"] >= 1
    c = res["tiled"][3]  # repeating textures: equal distances and shared partners
    assert c["events"] >= 450 and c["equal_replaced"] >= 300 and c["shared"] >= 100 and c["rejected"] >= 150
    assert c["max_seg_1"] >= 129 and c["max_seg_2"] >= 129 and c["epipole_disc"] >= 6
    assert np.flatnonzero(res["tiled"][2]).tolist() == [0, 3, 6, 9, 12]
    c = res["tiled_rows"][3]
    assert c["epipolar_rejected"] >= 9000 and c["epipole_disc"] >= 80 and c["events"] >= 150 and c["equal_replaced"] >= 8
    assert res["rotated_180"][1] >= 350 and int(np.argmax(res["rotated_180"][2])) == 6 and res["rotated_180"][3]["rejected"] >= 1
    c = res["sparse"][3]
    assert c["common_nodes"] >= 5 and c["events"] >= 80 and c["equal_replaced"] >= 20
    c = res["seg2_1"][3]
    assert c["max_seg_2"] == 1 and c["events"] >= 5 and c["shared"] == 1
    assert res["seg1_1"][3]["max_seg_1"] == 1 and res["seg1_1"][3]["max_seg_2"] >= 500
    for n in CHUNK_N[1:]:
        c = res["seg2_%d" % n][3]
        assert c["max_seg_2"] == n and c["max_seg_1"] >= 500 and c["events"] >= 100 and c["equal_replaced"] >= 30, n
        c = res["seg1_%d" % n][3]
        assert c["max_seg_1"] == n and c["max_seg_2"] >= 500 and c["events"] >= 30 and c["equal_replaced"] >= 40, n


# ---- GPU ----------------------------------------------------------------------------------------

def _points(k2):
    pts = np.zeros(len(k2.node), TRIANG_POINT_DTYPE)
    pts["desc"], pts["x"], pts["y"], pts["angle"] = k2.desc, k2.xy[:, 0], k2.xy[:, 1], k2.ang
    pts["octave"], pts["node"], pts["flags"] = k2.octv, k2.node, k2.flag
    return pts


def _pairs(geometry):
    pr = np.zeros(len(geometry), TRIANG_PAIR_DTYPE)
    for p, (F12, ep) in enumerate(geometry):
        pr["F12"][p], pr["ep"][p] = np.asarray(F12, F32).reshape(9), np.asarray(ep, F32).reshape(2)
    return pr


@pytest.fixture(scope="module")
def gpu_env():
    """Two 640x480 stereo pairs at 1000 features (images L0 R0 L1 R1), extracted and gridded once."""
    env = _env(["L0", "R0", "L1", "R1"])
    yield env
    env[0].close()


@pytest.fixture(scope="module")
def gpu_env2():
    """A second extractor: L0, L0 turned by 180 degrees, the two repeating textures."""
    env = _env(["L0", "rot", "T0", "TQ"])
    yield env
    env[0].close()


def _gpu_compare(env, pairs, only_stereo, coarse, check, packed=False, flags=True):
    """pairs: (keyframe 1's image name, K1, K2, F12, ep) per pair of one call -> the restatement's
    results.  Keyframe 1's descriptors, positions and angles are the batch's own; K1 holds their copy."""
    be, _, names = env
    pts = [_points(k2) for _, _, k2, _, _ in pairs]
    if packed:
        off = np.zeros(len(pts) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in pts])
        pts = (np.concatenate(pts), off)
    be.search_for_triangulation([names.index(f) for f, _, _, _, _ in pairs], pts, _pairs([g[3:] for g in pairs]),
                                [k1.node.astype(np.int32) for _, k1, _, _, _ in pairs],
                                [k1.flag.astype(np.uint8) for _, k1, _, _, _ in pairs] if flags else None,
                                only_stereo=only_stereo, coarse=coarse, check_orientation=check)
    out = []
    for p, (_, k1, k2, F12, ep) in enumerate(pairs):
        m, nm, hist, cnt = _py_tri(k1, k2, F12, ep, only_stereo, coarse, check)
        gm, gnm, ghist = be.triangulation_matches(p)
        np.testing.assert_array_equal(gm, m, err_msg="pair %d match12" % p)
        assert gnm == nm, (p, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="pair %d histogram" % p)
        out.append((m, nm, hist, cnt))
    return out


def _gpu_scene(env, name):
    k1, k2, F12, ep, only_stereo, coarse, check = _scene(env[1], name)
    (res,) = _gpu_compare(env, [(SCENES[name][0], k1, k2, F12, ep)], only_stereo, coarse, check)
    print(name, "nmatches", res[1], dict(res[3]))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENV1)
def test_gpu_search_for_triangulation_stereo_scenes(gpu_env, name):
    _, nm, _, cnt = _gpu_scene(gpu_env, name)
    if name == "left_right":
        assert cnt["events"] >= 200 and cnt["epipolar_rejected"] >= 8 and cnt["epipole_disc"] >= 4 and cnt["shared"] >= 15
    if name == "left_right_coarse":
        assert cnt["events"] >= 200 and cnt["epipolar_rejected"] == 0
    if name == "left_right_only_stereo":
        assert cnt["events"] >= 25 and cnt["mono_skipped_1"] >= 300
    if name == "unrelated":
        assert nm == 0
    if name == "one_node":  # segments far above one wave on both sides
        assert cnt["max_seg_1"] >= 500 and cnt["max_seg_2"] >= 500 and cnt["events"] >= 250 and cnt["rejected"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SCENES if n not in ENV1])
def test_gpu_search_for_triangulation_texture_scenes(gpu_env2, name):
    _, nm, hist, cnt = _gpu_scene(gpu_env2, name)
    if name == "tiled":
        assert cnt["equal_replaced"] >= 300 and cnt["shared"] >= 100 and cnt["rejected"] >= 150
    if name == "tiled_rows":
        assert cnt["epipolar_rejected"] >= 9000 and cnt["epipole_disc"] >= 80 and hist.sum() == 0
    if name == "rotated_180":
        assert nm >= 350 and int(np.argmax(hist)) == 6
    if name == "sparse":
        assert cnt["common_nodes"] >= 5 and cnt["events"] >= 80
    if name.startswith("seg") and not name.endswith("_1"):
        assert cnt["events"] >= 30 and cnt["equal_replaced"] >= 30


def _geometries(k2s):
    """Three different F12 / epipoles: rows, a slightly turned camera, and columns (t along y)."""
    Fs = (F_STEREO, _f12(K_, _rot_y(0.002), (0.11, 0.0, 0.002)), _f12(K_, np.eye(3), (0.0, 0.11, 0.0)))
    return [(F, np.asarray(k2.xy[len(k2.xy) // (p + 2)], F32)) for p, (F, k2) in enumerate(zip(Fs, k2s))]


@pytest.mark.gpu
def test_gpu_search_for_triangulation_one_frame_against_three_keyframes(gpu_env):
    """CreateNewMapPoints: one keyframe 1 in three pairs of one call, keyframe 2 point counts, F12 and
    epipoles that differ; the packed form and the list form give equal results."""
    fr = gpu_env[1]
    A = fr["R0"]
    k1 = K1(A.desc, A.xy, A.ang, _cell_nodes(A), _flags(len(A.ang)))
    k2s = []
    for name, n in (("L0", None), ("L0", 700), ("L1", 333)):
        B = fr[name]
        n = len(B.ang) if n is None else n
        k2s.append(K2(B.desc[:n], B.xy[:n], B.ang[:n], B.octv[:n], _cell_nodes(B)[:n], _flags(n)[::-1].copy()))
    pairs = [("R0", k1, k2, F, ep) for k2, (F, ep) in zip(k2s, _geometries(k2s))]
    res = _gpu_compare(gpu_env, pairs, False, False, True)
    same_f = _py_tri(k1, k2s[0], *_geometries(k2s)[2], check=True)
    assert res[0][1] >= 150 and res[0][3]["epipolar_rejected"] >= 5
    assert 50 <= res[1][1] != res[0][1] and res[1][3]["epipolar_rejected"] >= 5
    assert not np.array_equal(same_f[0], res[0][0])  # the pair's own F12 matters
    got = [gpu_env[0].triangulation_matches(p) for p in range(3)]
    _gpu_compare(gpu_env, pairs, False, False, True, packed=True)
    for p in range(3):
        again = gpu_env[0].triangulation_matches(p)
        assert np.array_equal(got[p][0], again[0]) and got[p][1] == again[1] and np.array_equal(got[p][2], again[2])
    # no flag rows: no map points and no stereo keypoints on keyframe 1
    bare = [(f, k._replace(flag=np.zeros_like(k.flag)), k2, F, ep) for f, k, k2, F, ep in pairs]
    res = _gpu_compare(gpu_env, bare, False, False, True, flags=False)
    assert res[0][3]["has_point_1"] == 0 and res[0][1] >= 150


@pytest.mark.gpu
def test_gpu_search_for_triangulation_empty_sides_and_no_pairs():
    import orbslam3lib_amd as og
    env = _env(["blank", "L0"])
    be, fr, _ = env
    L = fr["L0"]
    n = len(L.ang)
    assert len(fr["blank"].ang) == 0
    k1 = K1(L.desc, L.xy, L.ang, _desc_nodes(L), np.zeros(n, np.int32))
    k2 = K2(L.desc, L.xy, L.ang, L.octv, _desc_nodes(L), np.zeros(n, np.int32))
    e1, e2 = K1(*(v[:0] for v in k1)), K2(*(v[:0] for v in k2))
    neg = np.full(n, -3, np.int64)
    res = _gpu_compare(env, [("L0", k1, e2, F_STEREO, FAR),        # no keyframe 2 points
                             ("blank", e1, k2, F_STEREO, FAR)],    # no keyframe 1 keypoints
                       False, True, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][0] == -1).all() and len(res[0][0]) == n and len(res[1][0]) == 0
    res = _gpu_compare(env, [("L0", k1._replace(node=neg), k2, F_STEREO, FAR),   # keyframe 1 in no node
                             ("L0", k1, k2._replace(node=neg), F_STEREO, FAR)], False, True, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][0] == -1).all() and (res[1][0] == -1).all()
    (res,) = _gpu_compare(env, [("L0", k1, k2, F_STEREO, FAR)], False, True, True)  # against itself: every keypoint
    assert res[1] >= n - 10
    be.search_for_triangulation([], [], [], [])  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.triangulation_matches(0)
    assert e.value.code == -3
    be.close()


@pytest.mark.gpu
def test_gpu_search_for_triangulation_status_codes_and_the_capacity_limit():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    (kl, dl, _), (kr, dr, _) = be.result(0), be.result(1)
    n1 = len(kr)
    k2 = K2(dl.reshape(-1, 32), np.stack([kl["x"], kl["y"]], 1).astype(F32), kl["angle"].astype(F32),
            kl["octave"].astype(np.int32), (dl.reshape(-1, 32)[:, 0] >> 2).astype(np.int64), _flags(len(kl)))
    pts, pr = _points(k2), _pairs([(F_STEREO, FAR)])
    nodes, flags = (dr.reshape(-1, 32)[:, 0] >> 2).astype(np.int32), _flags(n1).astype(np.uint8)

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.search_for_triangulation(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.triangulation_matches(0)
    assert e.value.code == -3
    assert code([1], [pts], pr, [nodes]) == -3  # keyframe 1's positions are mvKeysUn: no grid yet
    be.undistort_grid(K_, D_)
    be.synchronize()
    assert code([2], [pts], pr, [nodes]) == -3 and code([-1], [pts], pr, [nodes]) == -3  # outside the gridded range
    assert code([1], [pts], pr, [nodes[:n1 - 1]]) == -3  # node_stride below N1
    assert code([1], [pts], pr, [nodes], [flags[:n1 - 1]]) == -3  # flag_stride below N1
    assert code([1, 1], (pts, np.array([0, len(pts), 5], np.int32)), _pairs([(F_STEREO, FAR)] * 2), [nodes, nodes]) == -3
    assert code([1] * 3, [pts] * 3, _pairs([(F_STEREO, FAR)] * 3), [nodes] * 3) == -3  # above the context's image capacity
    for octave in (-1, 8):  # the level tables have nlevels entries
        bad = pts.copy()
        bad["octave"][len(bad) // 2] = octave
        assert code([1], [bad], pr, [nodes]) == -3
    # at the capacity limit itself: 8192 keyframe 2 points
    assert BOW_MAX_POINTS == 8192
    xy1 = be.grid_result(1)[0]
    k1 = K1(dr.reshape(-1, 32), xy1, kr["angle"].astype(F32), nodes.astype(np.int64), flags.astype(np.int32))
    big = K2(*(np.concatenate([v] * (8192 // len(k2.node) + 1))[:8192] for v in k2))
    ep = _dense_spot(k1, k2)
    (res, _) = _gpu_compare((be, None, ["L", "R"]), [("R", k1, big, F_STEREO, ep), ("R", k1, k2, F_STEREO, ep)], False, False, True)
    assert res[1] >= 50 and res[3]["equal_replaced"] >= 50  # the copies are equal distances: the last one wins
    m, nm, hist = be.triangulation_matches(1)
    assert len(m) == n1 and nm == int((m >= 0).sum())
    with pytest.raises(og.OrbGpuError) as e:
        be.triangulation_matches(2)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # caller capacity below N1
        be.triangulation_matches(0, cap=n1 - 1)
    assert e.value.code == -2
    over = np.concatenate([_points(big), pts[:1]])
    assert code([1], [over], pr, [nodes]) == -2  # one keyframe 2 point above the limit
    be.close()


@pytest.mark.gpu
def test_gpu_earlier_bow_matches_stay_downloadable_after_a_triangulation_search(gpu_env):
    """The new keyframe was a Frame one step earlier: what SearchByBoW left for it is still there."""
    be, fr, names = gpu_env
    A, B = fr["L0"], fr["R0"]
    kf = KF(A.desc, A.ang, _desc_nodes(A), np.ones(len(A.ang), np.int32))
    be.search_by_bow([names.index("R0")], [_kf_points(kf)], [_desc_nodes(B).astype(np.int32)], nnratio=0.7)
    before = be.bow_matches(0)
    assert before[1] >= 50
    _gpu_scene(gpu_env, "left_right")
    after = be.bow_matches(0)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and np.array_equal(before[2], after[2])
    m, nm, hist, _ = _py_bow(kf, FB(B.desc, B.ang, _desc_nodes(B)), 0.7, True)
    assert np.array_equal(after[0], m) and after[1] == nm and np.array_equal(after[2], hist)
