"""ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) -- the matcher
LoopClosing::DetectCommonRegionsFromBoW runs for the current keyframe against every covisible of every
candidate (cpp/src/ORBmatcher.cc:766-906, with ComputeThreeMaxima :2061-2102), pinhole keyframes (NLeft ==
-1 on both).  Keyframe 1 is the batch image: the search walks its keypoints and indexes vpMatches12 by them;
keyframe 2 is the host's, and holds the taken bits (vbMatched2).  The node of each keypoint (mFeatVec) is an
input on both sides.

The yardstick is _py_bow_kf below: a restatement written from those lines with np.float32 scalars, which
returns the five outputs (match12, nmatches, the 30 bin sizes, a decision code and the two distances per
keypoint 1) and a Counter of the rules it hit.  _py_bow_kf_blocks is a second form written on its own -- per
common node, the node's block of the Hamming matrix, a boolean free mask over keypoints 2, the two lowest by
a stable argsort -- which must equal it on every output of every scene and hand-built case.
CPU: hand-built known answers on tiny keyframes; conditions on the scenes the GPU cases use; the exported
symbols and the statuses decided before any launch.
GPU: k_bowkf_group + k_bowkf_match + k_bowkf_finish against the restatement, equal on all five outputs.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs the SLAM stack; no fixtures ship
for it) -- restatement only, as for the other matcher functions."""
import re
from collections import Counter, namedtuple

import numpy as np
import pytest

from orbslam3lib_amd import (BOW_MAX_POINTS, BOWKF_HAS_POINT, BOWKF_MATCHED, BOWKF_NO_CANDIDATE, BOWKF_NO_MAP_POINT,
                             BOWKF_NO_NODE, BOWKF_NODE_NOT_COMMON, BOWKF_NOT_BELOW_TH_LOW, BOWKF_POINT_DTYPE,
                             BOWKF_RATIO_FAILED, BOWKF_ROTATION_REJECTED, synth)
from tests.test_search_by_bow import (FB, KF, NODE_MAX, TH_LOW, _cell_nodes, _desc_nodes, _env, _feat_vec,
                                      _hamming_matrix, _py_bow)
from tests.test_search_for_initialization import RNG_D, Fr, _bits, _images
from tests.test_track_projection import D_, F32, K_, _flip, _rot_bin, _three_maxima

# a keyframe, either side: mDescriptors, mvKeysUn.angle, node, (map point && !isBad())
KP = namedtuple("KP", "desc ang node flag")


def _py_bow_kf(k1, k2, nnratio, check):
    """-> match12 [N1] (index into keyframe 2's points or -1), nmatches, bin sizes [30] (before the
    three-maxima rule), code [N1] u8, best [N1, 2] int16, Counter of the rules."""
    n1 = len(k1.node)
    match = [-1] * n1  # :778
    matched2 = [False] * len(k2.node)  # :779
    code = [BOWKF_NO_NODE if nd < 0 else BOWKF_NODE_NOT_COMMON for nd in k1.node]
    best = [[0, 0] for _ in range(n1)]
    H = _hamming_matrix(k1.desc, k2.desc)
    fv1, fv2 = _feat_vec(k1.node), _feat_vec(k2.node)
    bins = [[] for _ in range(30)]
    cnt = Counter()
    ratio = F32(nnratio)
    nm = 0
    for node in sorted(fv1):  # :794-883: the nodes present in both, ascending
        if node not in fv2:
            continue
        cnt["common_nodes"] += 1
        idx2s = fv2[node]
        cnt["max_seg_1"] = max(cnt["max_seg_1"], len(fv1[node]))
        cnt["max_seg_2"] = max(cnt["max_seg_2"], len(idx2s))
        for idx1 in fv1[node]:  # :798
            if not (int(k1.flag[idx1]) & 1):  # :805-809
                code[idx1] = BOWKF_NO_MAP_POINT
                continue
            row = H[idx1].tolist()
            best1 = best2 = 256  # :813-815
            bi = -1
            low, low_taken = 257, False  # instrumentation only: the lowest distance among keypoints 2 with a point
            for idx2 in idx2s:  # :817
                if not (int(k2.flag[idx2]) & 1):  # :825-831, !pMP2 || isBad()
                    cnt["flagless_passed"] += 1
                    continue
                d = row[idx2]
                if d < low:
                    low, low_taken = d, matched2[idx2]
                if matched2[idx2]:  # :827
                    cnt["taken_passed"] += 1
                    continue
                if d < best1:  # :837-846
                    best2, best1, bi = best1, d, idx2
                elif d < best2:
                    best2 = d
            best[idx1] = [best1, best2]
            cnt["at_50"] += best1 == 50
            if bi == -1:
                code[idx1] = BOWKF_NO_CANDIDATE
                continue
            if not best1 < TH_LOW:  # :849
                code[idx1] = BOWKF_NOT_BELOW_TH_LOW
                continue
            if not bool(F32(best1) < ratio * F32(best2)):  # :851
                code[idx1] = BOWKF_RATIO_FAILED
                continue
            cnt["events"] += 1
            cnt["at_49"] += best1 == 49
            cnt["lone"] += best2 == 256
            cnt["promoted"] += low_taken
            match[idx1] = bi  # :853
            matched2[bi] = True  # :854
            code[idx1] = BOWKF_MATCHED
            nm += 1  # :867
            if check:  # :856-866
                bn = _rot_bin(k1.ang[idx1], k2.ang[bi])
                if bn is None:  # deviation
                    cnt["bin_out_of_range"] += 1
                else:
                    bins[bn].append(idx1)
    hist = np.array([len(e) for e in bins], np.int32)
    if check:  # :885-903
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn in keep:
                continue
            for idx1 in bins[bn]:
                match[idx1] = -1
                code[idx1] = BOWKF_ROTATION_REJECTED
                nm -= 1
    code = np.array(code, np.uint8).reshape(-1)
    for name, c in (("no_node", BOWKF_NO_NODE), ("node_not_common", BOWKF_NODE_NOT_COMMON), ("no_map_point", BOWKF_NO_MAP_POINT),
                    ("no_candidate", BOWKF_NO_CANDIDATE), ("not_below_th_low", BOWKF_NOT_BELOW_TH_LOW),
                    ("ratio_failed", BOWKF_RATIO_FAILED), ("rejected", BOWKF_ROTATION_REJECTED)):
        cnt[name] = int((code == c).sum())
    return np.array(match, np.int32).reshape(-1), nm, hist, code, np.array(best, np.int16).reshape(-1, 2), cnt


def _py_bow_kf_blocks(k1, k2, nnratio, check):
    """The second form -> match12, nmatches, bin sizes, code, best."""
    node1, node2 = np.asarray(k1.node, np.int64), np.asarray(k2.node, np.int64)
    has1 = (np.asarray(k1.flag) & 1).astype(bool)
    free = (np.asarray(k2.flag) & 1).astype(bool)  # keypoints 2 that may still be chosen
    n1 = len(node1)
    match = np.full(n1, -1, np.int32)
    code = np.where(node1 < 0, BOWKF_NO_NODE, BOWKF_NODE_NOT_COMMON).astype(np.uint8)
    best = np.zeros((n1, 2), np.int16)
    mbin = np.full(n1, -1, np.int64)
    for node in np.intersect1d(node1[node1 >= 0], node2[node2 >= 0]):
        rows, cols = np.flatnonzero(node1 == node), np.flatnonzero(node2 == node)
        block = _hamming_matrix(np.asarray(k1.desc)[rows], np.asarray(k2.desc)[cols])
        for r, i in zip(rows, range(len(rows))):
            if not has1[r]:
                code[r] = BOWKF_NO_MAP_POINT
                continue
            cand = cols[free[cols]]
            d = block[i][free[cols]]
            two = np.argsort(d, kind="stable")[:2]
            lowest = [int(d[j]) for j in two] + [256, 256]
            best[r] = lowest[:2]
            if len(cand) == 0:
                code[r] = BOWKF_NO_CANDIDATE
            elif lowest[0] >= TH_LOW:
                code[r] = BOWKF_NOT_BELOW_TH_LOW
            elif not F32(lowest[0]) < F32(nnratio) * F32(lowest[1]):
                code[r] = BOWKF_RATIO_FAILED
            else:
                match[r], code[r] = cand[two[0]], BOWKF_MATCHED
                free[cand[two[0]]] = False
                bn = _rot_bin(k1.ang[r], k2.ang[cand[two[0]]]) if check else None
                mbin[r] = -1 if bn is None else bn
    hist = np.bincount(mbin[mbin >= 0], minlength=30).astype(np.int32)
    if check:
        keep = _three_maxima(hist)
        gone = (mbin >= 0) & ~np.isin(mbin, [b for b in keep if b >= 0])
        match[gone], code[gone] = -1, BOWKF_ROTATION_REJECTED
    return match, int((match >= 0).sum()), hist, code, best


def _both(k1, k2, nnratio=0.9, check=True):
    """The restatement's result, after the second form agreed with it on every output."""
    res = _py_bow_kf(k1, k2, nnratio, check)
    for name, a, b in zip(("match12", "nmatches", "hist", "code", "best"), res, _py_bow_kf_blocks(k1, k2, nnratio, check)):
        np.testing.assert_array_equal(a, b, err_msg=name)
    return res


# ---- hand-built keyframes -----------------------------------------------------------------------

def _kp(points):
    """points: (desc [32] u8, angle, node[, flag = 1])."""
    return KP(np.array([p[0] for p in points], np.uint8).reshape(-1, 32), np.array([p[1] for p in points], F32),
              np.array([p[2] for p in points], np.int64), np.array([p[3] if len(p) > 3 else 1 for p in points], np.int32))


Z, E = _bits(), _bits((100, 140))


def test_an_earlier_keypoint_1_takes_what_a_later_closer_one_would_have_won():
    k2 = _kp([(Z, 0.0, 5), (E, 0.0, 5)])
    # a0 is 10 from b0 (50 from b1) and takes it; a1, 3 from b0, finds it taken: its next best is b1 at 43
    m, nm, _, code, best, cnt = _both(_kp([(_bits((0, 10)), 0.0, 5), (_bits((0, 3)), 0.0, 5)]), k2)
    assert list(m) == [0, 1] and nm == 2 and cnt["taken_passed"] == 1 and cnt["promoted"] == 1 and cnt["lone"] == 1
    assert best.tolist() == [[10, 50], [43, 256]] and list(code) == [BOWKF_MATCHED] * 2
    # seven bits farther (50 from b1) the later one takes nothing
    m, nm, _, code, best, _ = _both(_kp([(_bits((0, 10)), 0.0, 5), (_bits((0, 3), (200, 207)), 0.0, 5)]), k2)
    assert list(m) == [0, -1] and nm == 1 and code[1] == BOWKF_NOT_BELOW_TH_LOW and best[1].tolist() == [50, 256]
    # the other order: the closer one comes first and wins b0, the farther one is left with b1 (50): nothing
    m, nm, _, _, _, _ = _both(_kp([(_bits((0, 3)), 0.0, 5), (_bits((0, 10)), 0.0, 5)]), k2)
    assert list(m) == [0, -1] and nm == 1


def test_a_taken_keypoint_2_no_longer_counts_as_second_best():
    X, Y = _bits((0, 10)), _bits((10, 20))
    k2 = _kp([(X, 0.0, 1), (Y, 0.0, 1)])
    # alone, Z is 10 from both: 10 < 0.9 * 10 fails
    m, nm, _, code, best, _ = _both(_kp([(Z, 0.0, 1)]), k2)
    assert nm == 0 and list(m) == [-1] and list(code) == [BOWKF_RATIO_FAILED] and best.tolist() == [[10, 10]]
    # after X's own keypoint took X, Y is a lone candidate for Z: 10 < 0.9 * 256 passes
    m, nm, _, code, best, cnt = _both(_kp([(X, 0.0, 1), (Z, 0.0, 1)]), k2)
    assert list(m) == [0, 1] and nm == 2 and cnt["lone"] == 1 and cnt["promoted"] == 1 and best[1].tolist() == [10, 256]


def test_a_keypoint_2_without_a_map_point_is_neither_best_nor_second_best_even_at_distance_0():
    D = RNG_D[0]
    # b0 equals a0 but has no point: b1, 3 away, is a lone candidate
    m, nm, _, code, best, cnt = _both(_kp([(D, 0.0, 4)]), _kp([(D, 0.0, 4, 0), (_flip(D, 3), 0.0, 4)]))
    assert list(m) == [1] and nm == 1 and best.tolist() == [[3, 256]] and cnt["flagless_passed"] == 1
    # as the second best it would have failed the ratio: with its point 3 < 0.9 * 0 ... the best is itself
    m, _, _, _, best, _ = _both(_kp([(D, 0.0, 4)]), _kp([(D, 0.0, 4, 1), (_flip(D, 3), 0.0, 4)]))
    assert list(m) == [0] and best.tolist() == [[0, 3]]
    # flagless as second best: 10 and 10 fail the ratio with both points, pass with one
    X, Y = _bits((0, 10)), _bits((10, 20))
    assert _both(_kp([(Z, 0.0, 1)]), _kp([(X, 0.0, 1), (Y, 0.0, 1)]))[1] == 0
    assert list(_both(_kp([(Z, 0.0, 1)]), _kp([(X, 0.0, 1), (Y, 0.0, 1, 0)]))[0]) == [0]
    # only bit 0 of the flags counts
    assert _both(_kp([(D, 0.0, 4)]), _kp([(D, 0.0, 4, 2)]))[3][0] == BOWKF_NO_CANDIDATE


def test_a_keypoint_1_without_a_map_point_neither_matches_nor_takes():
    D = RNG_D[0]
    m, nm, _, code, best, cnt = _both(_kp([(D, 0.0, 4, 0), (_flip(D, 3), 0.0, 4, 1)]), _kp([(D, 0.0, 4)]))
    assert list(m) == [-1, 0] and nm == 1 and list(code) == [BOWKF_NO_MAP_POINT, BOWKF_MATCHED]
    assert best.tolist() == [[0, 0], [3, 256]] and cnt["taken_passed"] == 0
    assert _both(_kp([(D, 0.0, 4, 2)]), _kp([(D, 0.0, 4)]))[1] == 0  # only bit 0 counts


def test_49_matches_and_50_does_not_where_the_frame_search_matches_at_50():
    for nbits, want in ((49, 1), (50, 0), (51, 0)):
        d = _bits((0, nbits))
        m, nm, _, code, best, cnt = _both(_kp([(Z, 0.0, 0)]), _kp([(d, 0.0, 0)]), 0.7)
        assert nm == want and best.tolist() == [[nbits, 256]]
        assert code[0] == (BOWKF_MATCHED if want else BOWKF_NOT_BELOW_TH_LOW) and cnt["at_50"] == (nbits == 50)
    # the same descriptors under SearchByBoW(KeyFrame*, Frame&): <= TH_LOW (:328), so 50 is a match
    kf = KF(np.array([_bits((0, 50))], np.uint8), np.zeros(1, F32), np.zeros(1, np.int64), np.ones(1, np.int32))
    assert _py_bow(kf, FB(np.array([Z], np.uint8), np.zeros(1, F32), np.zeros(1, np.int64)), 0.7, True)[1] == 1


def test_ratio_fails_at_equality_and_a_lone_candidate_is_compared_against_256():
    assert F32(0.7) * F32(10) == F32(7) and F32(0.9) * F32(10) == F32(9)  # both products round to the integer
    for ratio, b in ((0.7, 7), (0.9, 9)):
        k2 = _kp([(_bits((0, b)), 0.0, 3), (_bits((b, b + 10)), 0.0, 3)])  # b and 10 from zero
        _, nm, _, code, _, _ = _both(_kp([(Z, 0.0, 3)]), k2, ratio)
        assert nm == 0 and code[0] == BOWKF_RATIO_FAILED  # b < b.0f is false
        k2 = _kp([(_bits((0, b - 1)), 0.0, 3), (_bits((b, b + 10)), 0.0, 3)])
        assert _both(_kp([(Z, 0.0, 3)]), k2, ratio)[1] == 1
    # a lone candidate: bestDist2 stays 256: 49 < 0.7 * 256, but not 49 < 0.19 * 256 = 48.64
    lone = _kp([(_bits((0, 49)), 0.0, 3)])
    assert _both(_kp([(Z, 0.0, 3)]), lone, 0.7)[1] == 1
    assert _both(_kp([(Z, 0.0, 3)]), lone, 0.19)[3][0] == BOWKF_RATIO_FAILED
    assert _both(_kp([(Z, 0.0, 3)]), lone, 0.2)[1] == 1  # 51.2


def test_an_equal_distance_is_the_second_best_not_the_best():
    k2 = _kp([(_bits((0, 7)), 0.0, 2), (_bits((7, 14)), 0.0, 2)])  # both 7 from zero
    m, nm, _, _, best, _ = _both(_kp([(Z, 0.0, 2)]), k2, 1.5)
    assert list(m) == [0] and nm == 1 and best.tolist() == [[7, 7]]  # the first keeps the best; 7 < 1.5 * 7
    assert _both(_kp([(Z, 0.0, 2)]), k2, 1.0)[1] == 0  # the equal one is the second best: 7 < 7 fails


def test_a_node_whose_keypoints_2_are_all_taken_or_flagless_gives_no_candidate():
    D = RNG_D
    k1 = _kp([(D[0], 0.0, 8), (D[0], 0.0, 8), (D[1], 0.0, 9)])
    k2 = _kp([(D[0], 0.0, 8), (D[0], 0.0, 8, 0), (D[1], 0.0, 9, 0)])
    m, nm, _, code, best, cnt = _both(k1, k2)
    assert list(m) == [0, -1, -1] and nm == 1 and list(code) == [BOWKF_MATCHED, BOWKF_NO_CANDIDATE, BOWKF_NO_CANDIDATE]
    assert best.tolist() == [[0, 256], [256, 256], [256, 256]] and cnt["no_candidate"] == 2


def test_nodes_of_one_side_negative_unsorted_and_very_large_ids():
    D = RNG_D
    k1 = _kp([(D[4], 0.0, 0), (D[3], 0.0, 9), (D[2], 0.0, -1), (D[1], 0.0, 5), (D[0], 0.0, NODE_MAX),
              (D[6], 0.0, -7), (D[5], 0.0, 1 << 30), (D[0], 0.0, NODE_MAX - 1)])
    k2 = _kp([(D[0], 0.0, NODE_MAX), (D[1], 0.0, 5), (D[2], 0.0, -1), (D[3], 0.0, 7), (D[4], 0.0, 0),
              (D[5], 0.0, 1 << 30), (D[6], 0.0, -7)])
    m, nm, _, code, best, cnt = _both(k1, k2, 0.7)
    # node 7 is keyframe 2's only, 9 and NODE_MAX - 1 keyframe 1's only; equal negative values are no node
    assert list(m) == [4, -1, -1, 1, 0, -1, 5, -1] and nm == 4 and cnt["common_nodes"] == 4 and cnt["lone"] == 4
    NC, NN, M = BOWKF_NODE_NOT_COMMON, BOWKF_NO_NODE, BOWKF_MATCHED
    assert list(code) == [M, NC, NN, M, M, NN, M, NC] and (best[[1, 2, 5, 7]] == 0).all()
    assert cnt["no_node"] == 2 and cnt["node_not_common"] == 2


@pytest.mark.parametrize("a1,a2,expect", [(14.9, 0.0, 0), (15.0, 0.0, 1), (359.0, 0.0, 12), (0.0, 0.5, 12),
                                          (44.9, 0.0, 1), (45.1, 0.0, 2), (10.0, 350.0, 1)])
def test_rotation_bin_edges(a1, a2, expect):
    """rot = keyframe 1's angle - keyframe 2's angle, the factor is 1 / 30."""
    D = RNG_D[1]
    _, nm, hist, _, _, _ = _both(_kp([(D, a1, 0)]), _kp([(D, a2, 0)]), 0.7)
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1


def _bin_scene(sizes, extra1=(), extra2=()):
    """{bin: events}: every event in a node of its own."""
    k1, k2, k = list(extra1), list(extra2), 0
    for bn, n in sizes.items():
        for _ in range(n):
            k1.append((RNG_D[k], 30.0 * bn, 100 + k))
            k2.append((RNG_D[k], 0.0, 100 + k))
            k += 1
    return _kp(k1), _kp(k2)


def test_three_maxima_ties_and_cutoffs_and_the_list_holds_idx1():
    def scene(sizes):
        return _both(*_bin_scene(sizes), 0.7)
    # strict >: the earlier bins win the tie, the fourth is rejected
    m, nm, hist, code, _, cnt = scene({2: 5, 5: 5, 7: 5, 9: 5})
    assert list(hist[[2, 5, 7, 9]]) == [5, 5, 5, 5] and nm == 15 and cnt["rejected"] == 5
    assert (m[15:] == -1).all() and (code[15:] == BOWKF_ROTATION_REJECTED).all() and (code[:15] == BOWKF_MATCHED).all()
    # exactly 10%: 0.1f * 10.0f rounds to 1.0f, so one event beside ten is kept
    assert scene({0: 10, 3: 1})[1] == 11
    # max2 below 10%: the second and the third are dropped together
    _, nm, _, _, _, cnt = scene({4: 22, 1: 2, 8: 2})
    assert nm == 22 and cnt["rejected"] == 4
    # only max3 below 10%
    assert scene({4: 22, 1: 3, 8: 2})[1] == 25
    # the list of a bin holds idx1, not idx2: keyframe 2 reversed, the rejected entries are keyframe 1's last five
    k1, k2 = _bin_scene({2: 5, 5: 5, 7: 5, 9: 5})
    rev = KP(*(v[::-1].copy() for v in k2))
    m, nm, _, code, _, _ = _both(k1, rev, 0.7)
    assert list(m[:15]) == list(range(19, 4, -1)) and (m[15:] == -1).all() and nm == 15


def test_a_rejected_match_leaves_its_keypoint_2_taken():
    D = RNG_D
    # eleven events in bin 1; a0 (bin 5, alone: rejected) takes b0 of node 1; a1 of node 1, 3 bits from b0, finds
    # it taken and b1 (unrelated) too far
    k1, k2 = _bin_scene({1: 11}, [(D[40], 150.0, 1), (_flip(D[40], 3), 30.0, 1)], [(D[40], 0.0, 1), (D[41], 0.0, 1)])
    m, nm, hist, code, best, cnt = _both(k1, k2, 0.7)
    assert m[0] == -1 and code[0] == BOWKF_ROTATION_REJECTED and best[0, 0] == 0
    assert m[1] == -1 and code[1] == BOWKF_NOT_BELOW_TH_LOW and cnt["taken_passed"] == 1 and nm == 11 and hist[5] == 1


def test_the_bin_out_of_range_deviation_and_no_orientation_check():
    # an angle far outside [0, 360): the event counts, enters no bin and survives the rejection that takes
    # the lone event of bin 5
    D = RNG_D
    k1, k2 = _bin_scene({1: 11}, [(D[40], 1000.0, 1), (D[41], 150.0, 2)], [(D[40], 0.0, 1), (D[41], 0.0, 2)])
    m, nm, hist, code, _, cnt = _both(k1, k2, 0.7)
    assert cnt["bin_out_of_range"] == 1 and hist.sum() == 12 and hist[1] == 11 and hist[5] == 1
    assert cnt["rejected"] == 1 and m[0] == 0 and m[1] == -1 and nm == 12 and code[0] == BOWKF_MATCHED
    k1.ang[0] = np.nan
    assert _both(k1, k2, 0.7)[1] == 12
    # no orientation check: no bins, nothing rejected
    m, nm, hist, code, _, cnt = _both(k1, k2, 0.7, False)
    assert hist.sum() == 0 and nm == 13 and cnt["rejected"] == 0 and (m >= 0).all() and (code == BOWKF_MATCHED).all()


# ---- ABI ----------------------------------------------------------------------------------------

def test_symbols_and_statuses_decided_before_any_launch():
    import orbslam3lib_amd as og
    names = {"orbgpu_search_by_bow_kf_batch", "orbgpu_download_bow_kf_matches"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "search_by_bow_kf") and hasattr(og.BatchExtractor, "bow_kf_matches")
    assert BOWKF_POINT_DTYPE.itemsize == 44 and BOWKF_HAS_POINT == og.BOW_HAS_POINT == 1
    assert [BOWKF_NO_NODE, BOWKF_NODE_NOT_COMMON, BOWKF_NO_MAP_POINT, BOWKF_NO_CANDIDATE, BOWKF_NOT_BELOW_TH_LOW,
            BOWKF_RATIO_FAILED, BOWKF_MATCHED, BOWKF_ROTATION_REJECTED] == list(range(1, 9))
    header = open(og.os.path.join(og.os.path.dirname(og.HERE), "include", "orbgpu.h")).read()
    for k, name in enumerate(("NO_NODE", "NODE_NOT_COMMON", "NO_MAP_POINT", "NO_CANDIDATE", "NOT_BELOW_TH_LOW", "RATIO_FAILED",
                              "MATCHED", "ROTATION_REJECTED")):
        assert re.search(r"#define ORBGPU_BOWKF_%s\s+%d\b" % (name, k + 1), header), name
    one = np.zeros(1, np.int32)
    f = og.C.c_float
    assert lib.orbgpu_search_by_bow_kf_batch(None, 1, og._p(one), None, None, None, 0, None, 0, f(0.9), 1, None) == -3
    assert lib.orbgpu_search_by_bow_kf_batch(None, 0, None, None, None, None, 0, None, 0, f(0.9), 1, None) == -3
    assert lib.orbgpu_download_bow_kf_matches(None, 0, None, None, None, 0, None, None, None) == -3
    # the wrapper refuses lists that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, BOWKF_POINT_DTYPE)
    nodes, flags = np.zeros(4, np.int32), np.ones(4, np.uint8)
    with pytest.raises(ValueError):
        be.search_by_bow_kf([0, 1], [pts], [nodes, nodes])
    with pytest.raises(ValueError):
        be.search_by_bow_kf([0, 1], [pts, pts], [nodes])
    with pytest.raises(ValueError):
        be.search_by_bow_kf([0, 1], [pts, pts], [nodes, nodes], [flags])
    with pytest.raises(ValueError):
        be.search_by_bow_kf([0, 1], (pts, np.array([0, 3], np.int32)), [nodes, nodes])
    with pytest.raises(ValueError):  # offsets beyond the points
        be.search_by_bow_kf([0], (pts, np.array([0, 4], np.int32)), [nodes])


# ---- scenes -------------------------------------------------------------------------------------

def _flags1(n):
    return (np.arange(n) % 5 != 0).astype(np.int32)


def _flags2(n):
    return (np.arange(n) % 7 != 0).astype(np.int32)


SEG_N = (1, 63, 64, 65, 129)  # keypoints in the node: around the 64-lane chunks and the 64-keypoint staging

# name -> (keyframe 1: the batch image, keyframe 2, nodes, nnratio, check_orientation): row 9's scenes, mirrored
SCENES = {
    "tiled_desc": ("TQ", "T0", "desc", 0.9, True),
    "tiled_no_orientation": ("TQ", "T0", "desc", 0.9, False),
    "left_right_cells": ("R0", "L0", "cell", 0.7, True),
    "rotated_180": ("rot", "L0", "desc", 0.7, True),
    "unrelated_cells": ("L1", "L0", "cell", 0.7, True),
    "one_node": ("R0", "L0", "one", 0.9, True),
}
SCENES.update({"first2_%d" % n: ("TQ", "T0", ("first2", n), 0.9, True) for n in SEG_N})
SCENES.update({"first1_%d" % n: ("TQ", "T0", ("first1", n), 0.9, True) for n in SEG_N})
ENV1 = ("left_right_cells", "unrelated_cells", "one_node")  # images L0 R0 L1 R1; the rest: L0 rot T0 TQ


def _scene(frames, name):
    """-> (keyframe 1, keyframe 2, nnratio, check) of a scene on frames (Fr records by image name)."""
    f1, f2, nodes, ratio, check = SCENES[name]
    A, B = frames[f1], frames[f2]
    n1, n2 = len(A.ang), len(B.ang)
    if nodes == "desc":
        nd1, nd2 = _desc_nodes(A), _desc_nodes(B)
    elif nodes == "cell":
        nd1, nd2 = _cell_nodes(A), _cell_nodes(B)
    elif nodes == "one":
        nd1, nd2 = np.zeros(n1, np.int64), np.zeros(n2, np.int64)
    elif nodes[0] == "first2":  # keyframe 2's node 7 holds its first n keypoints, all of keyframe 1 in node 7
        nd1, nd2 = np.full(n1, 7, np.int64), np.where(np.arange(n2) < nodes[1], 7, -1).astype(np.int64)
    else:  # the mirror
        nd1, nd2 = np.where(np.arange(n1) < nodes[1], 7, -1).astype(np.int64), np.full(n2, 7, np.int64)
    return KP(A.desc, A.ang, nd1, _flags1(n1)), KP(B.desc, B.ang, nd2, _flags2(n2)), ratio, check


@pytest.fixture(scope="module")
def cpu_frames(oracle):
    imgs = _images()
    frames = {}
    for k in ("L0", "R0", "L1", "rot", "T0", "TQ"):
        kps, desc, _ = oracle.extract(imgs[k], nfeatures=1000)
        xy, _, _, cs, ci = oracle.undistort_grid(kps, K_, D_, 640, 480)
        frames[k] = Fr(xy, kps["octave"].astype(np.int32), kps["angle"].astype(F32), desc.reshape(-1, 32), cs, ci)
    return frames


def _scene_conditions(name, res, frames):
    """The floors on a scene's inputs: below the counts the restatement gave when the scenes were made, they
    are conditions on the inputs, not tolerances."""
    _, nm, hist, _, _, c = res
    if name == "tiled_desc":
        assert c["events"] >= 200 and c["promoted"] >= 40 and c["taken_passed"] >= 3000 and c["ratio_failed"] >= 150
        assert c["not_below_th_low"] >= 150 and c["at_50"] >= 1 and c["rejected"] >= 50 and c["no_candidate"] >= 1
        assert c["max_seg_1"] >= 129 and c["max_seg_2"] >= 129
    if name == "tiled_no_orientation":
        assert hist.sum() == 0 and c["rejected"] == 0 and nm == c["events"] >= 200
    if name == "left_right_cells":
        assert c["events"] >= 200 and c["at_49"] >= 1
    if name == "rotated_180":
        assert c["events"] >= 300 and int(np.argmax(hist)) == 6
    if name == "unrelated_cells":
        assert nm == 0
    if name == "one_node":
        f1, f2 = SCENES[name][:2]
        assert (c["max_seg_1"], c["max_seg_2"]) == (len(frames[f1].ang), len(frames[f2].ang)) and c["events"] >= 200
    if name == "first2_1":  # keyframe 2's keypoint 0 has no map point (0 % 7): every walk comes back empty
        assert c["events"] == 0 and c["no_candidate"] == c["max_seg_1"] - c["no_map_point"] >= 500
    elif name.startswith("first2_"):
        assert c["max_seg_2"] == int(name[7:]) and c["events"] >= 30 and c["promoted"] >= 10
    if name == "first1_1":  # keyframe 1's keypoint 0 has no map point (0 % 5)
        assert c["events"] == 0 and c["no_map_point"] == 1
    elif name.startswith("first1_"):
        assert c["max_seg_1"] == int(name[7:]) and c["events"] >= 20


def test_scenes_exercise_every_rule_and_the_second_form_agrees(cpu_frames):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the oracle's
    extraction at 1000 features, meets every situation the GPU cases are there to compare; and the
    second form equals it on every output of every scene."""
    for name in SCENES:
        k1, k2, ratio, check = _scene(cpu_frames, name)
        res = _both(k1, k2, ratio, check)
        print(name, "nmatches", res[1], dict(res[5]), "bins", np.flatnonzero(res[2]).tolist())
        _scene_conditions(name, res, cpu_frames)


# ---- GPU ----------------------------------------------------------------------------------------

def _points(k2):
    pts = np.zeros(len(k2.node), BOWKF_POINT_DTYPE)
    pts["desc"], pts["angle"], pts["node"], pts["flags"] = k2.desc, k2.ang, k2.node, k2.flag
    return pts


@pytest.fixture(scope="module")
def gpu_env():
    """Two 640x480 stereo pairs at 1000 features (images L0 R0 L1 R1), extracted once."""
    env = _env(["L0", "R0", "L1", "R1"])
    yield env
    env[0].close()


@pytest.fixture(scope="module")
def gpu_env2():
    """A second extractor: L0, L0 turned by 180 degrees, the two repeating textures."""
    env = _env(["L0", "rot", "T0", "TQ"])
    yield env
    env[0].close()


def _assert_pair(be, p, want, what=""):
    gm, gnm, ghist, gcode, gbest = be.bow_kf_matches(p)
    m, nm, hist, code, best = want[:5]
    np.testing.assert_array_equal(gm, m, err_msg="%s pair %d match12" % (what, p))
    assert gnm == nm, (what, p, gnm, nm)
    np.testing.assert_array_equal(ghist, hist, err_msg="%s pair %d histogram" % (what, p))
    np.testing.assert_array_equal(gcode, code, err_msg="%s pair %d code" % (what, p))
    np.testing.assert_array_equal(gbest, best, err_msg="%s pair %d best" % (what, p))


def _gpu_compare(env, pairs, ratio, check, pts=None, flags=True):
    """pairs: (keyframe 1's image name, K1, K2) per pair of one call -> the restatement's results.  Keyframe
    1's descriptors and angles are the batch's own; K1 holds their copy.  pts: the points in another form."""
    be, _, names = env
    be.search_by_bow_kf([names.index(f) for f, _, _ in pairs], [_points(k2) for _, _, k2 in pairs] if pts is None else pts,
                        [k1.node.astype(np.int32) for _, k1, _ in pairs],
                        [k1.flag.astype(np.uint8) for _, k1, _ in pairs] if flags else None,
                        nnratio=ratio, check_orientation=check)
    out = []
    for p, (_, k1, k2) in enumerate(pairs):
        out.append(_py_bow_kf(k1, k2, ratio, check))
        _assert_pair(be, p, out[-1])
    return out


def _gpu_scene(env, name):
    k1, k2, ratio, check = _scene(env[1], name)
    (res,) = _gpu_compare(env, [(SCENES[name][0], k1, k2)], ratio, check)
    print(name, "nmatches", res[1], dict(res[5]))
    _scene_conditions(name, res, env[1])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENV1)
def test_gpu_search_by_bow_kf_stereo_scenes(gpu_env, name):
    _gpu_scene(gpu_env, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SCENES if n not in ENV1])
def test_gpu_search_by_bow_kf_texture_scenes(gpu_env2, name):
    _gpu_scene(gpu_env2, name)


def _three_keyframes(fr):
    """The current keyframe R0 against three keyframes whose point counts differ."""
    A = fr["R0"]
    k1 = KP(A.desc, A.ang, _desc_nodes(A), _flags1(len(A.ang)))
    pairs = []
    for name, n in (("L0", None), ("L1", 700), ("R1", 333)):
        B = fr[name]
        n = len(B.ang) if n is None else n
        pairs.append(("R0", k1, KP(B.desc[:n], B.ang[:n], _desc_nodes(B)[:n], _flags2(n))))
    return pairs


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_one_frame_against_three_keyframes(gpu_env):
    """DetectCommonRegionsFromBoW: one current keyframe in three pairs of one call equals three single calls,
    also with the points packed from an offset above 0, a run of points no pair names before them."""
    be = gpu_env[0]
    pairs = _three_keyframes(gpu_env[1])
    res = _gpu_compare(gpu_env, pairs, 0.9, True)
    assert res[0][1] >= 100 and res[0][1] != res[1][1]
    got = [be.bow_kf_matches(p) for p in range(3)]
    for p in range(3):  # three single calls
        _gpu_compare(gpu_env, [pairs[p]], 0.9, True)
        for x, y in zip(be.bow_kf_matches(0), got[p]):
            np.testing.assert_array_equal(x, y)
    pts = [_points(k2) for _, _, k2 in pairs]
    junk = _points(pairs[0][2])[:37]
    junk["node"] = 3
    off = (37 + np.concatenate([[0], np.cumsum([len(p) for p in pts])])).astype(np.int32)
    _gpu_compare(gpu_env, pairs, 0.9, True, pts=(np.concatenate([junk] + pts + [junk]), off))
    for p in range(3):
        for x, y in zip(be.bow_kf_matches(p), got[p]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_flag_rows(gpu_env):
    """Two pairs with the same keyframe 2 and different f_flags rows; f_flags = None equals a row of ones."""
    be, fr, _ = gpu_env
    (_, k1, k2) = _three_keyframes(fr)[0]
    other = k1._replace(flag=(np.arange(len(k1.flag)) % 3 != 1).astype(np.int32))
    res = _gpu_compare(gpu_env, [("R0", k1, k2), ("R0", other, k2)], 0.9, True)
    assert not np.array_equal(res[0][0], res[1][0]) and res[0][5]["no_map_point"] != res[1][5]["no_map_point"]
    ones = k1._replace(flag=np.ones_like(k1.flag))
    (res,) = _gpu_compare(gpu_env, [("R0", ones, k2)], 0.9, True)
    with_row = be.bow_kf_matches(0)
    assert res[5]["no_map_point"] == 0 and res[1] >= 100
    _gpu_compare(gpu_env, [("R0", ones, k2)], 0.9, True, flags=False)
    for x, y in zip(be.bow_kf_matches(0), with_row):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_one_scene_twice_gives_identical_bytes(gpu_env2):
    be = gpu_env2[0]
    _gpu_scene(gpu_env2, "tiled_desc")
    first = [np.asarray(x).tobytes() for x in be.bow_kf_matches(0)]
    _gpu_scene(gpu_env2, "first2_129")
    _gpu_scene(gpu_env2, "tiled_desc")
    assert [np.asarray(x).tobytes() for x in be.bow_kf_matches(0)] == first


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_empty_sides_clear_flags_and_no_pairs():
    import orbslam3lib_amd as og
    env = _env(["blank", "L0"])
    be, fr, _ = env
    L = fr["L0"]
    n = len(L.ang)
    assert len(fr["blank"].ang) == 0
    k = KP(L.desc, L.ang, _desc_nodes(L), np.ones(n, np.int32))
    none = KP(*(v[:0] for v in k))
    neg = np.full(n, -3, np.int64)
    res = _gpu_compare(env, [("L0", k, none),       # no keyframe 2 points
                             ("blank", none, k)],   # no keyframe 1 keypoints
                       0.9, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][0] == -1).all() and len(res[0][0]) == n and len(res[1][0]) == 0
    assert (res[0][3] == BOWKF_NODE_NOT_COMMON).all()
    res = _gpu_compare(env, [("L0", k._replace(node=neg), k),   # keyframe 1 in no node
                             ("L0", k, k._replace(node=neg))], 0.9, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][3] == BOWKF_NO_NODE).all() and (res[1][3] == BOWKF_NODE_NOT_COMMON).all()
    clear = np.zeros(n, np.int32)
    res = _gpu_compare(env, [("L0", k._replace(flag=clear), k),   # all flags clear on side 1, on side 2
                             ("L0", k, k._replace(flag=clear))], 0.9, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][3] == BOWKF_NO_MAP_POINT).all()
    assert (res[1][3] == BOWKF_NO_CANDIDATE).all() and (res[1][4] == 256).all()
    (res,) = _gpu_compare(env, [("L0", k, k)], 0.9, False)  # against itself: every keypoint at distance 0
    assert res[1] >= n - 10 and (res[4][res[0] >= 0, 0] == 0).all()
    be.search_by_bow_kf([], [], [])  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.bow_kf_matches(0)
    assert e.value.code == -3
    be.close()


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_status_codes_and_the_capacity_limit():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    (kl, dl, _), (kr, dr, _) = be.result(0), be.result(1)
    dl, dr = dl.reshape(-1, 32), dr.reshape(-1, 32)
    n1 = len(kr)
    k2 = KP(dl, kl["angle"].astype(F32), (dl[:, 0] >> 2).astype(np.int64), _flags2(len(kl)))
    k1 = KP(dr, kr["angle"].astype(F32), (dr[:, 0] >> 2).astype(np.int64), _flags1(n1))
    pts, nodes, flags = _points(k2), k1.node.astype(np.int32), k1.flag.astype(np.uint8)

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.search_by_bow_kf(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.bow_kf_matches(0)
    assert e.value.code == -3
    assert code([2], [pts], [nodes]) == -3 and code([-1], [pts], [nodes]) == -3  # outside the last batch
    assert code([1], [pts], [nodes[:n1 - 1]]) == -3  # node_stride below N1
    assert code([1], [pts], [nodes], [flags[:n1 - 1]]) == -3  # flag_stride below N1
    assert code([1, 1], (pts, np.array([0, len(pts), 5], np.int32)), [nodes, nodes]) == -3  # descending offsets
    assert code([1] * 3, [pts] * 3, [nodes] * 3) == -3  # above the context's image capacity
    for bad in (np.nan, np.inf, -np.inf):
        assert code([1], [pts], [nodes], nnratio=bad) == -3
    with pytest.raises(og.OrbGpuError) as e:  # none of them left a pair
        be.bow_kf_matches(0)
    assert e.value.code == -3
    # the call works before undistort_grid, and at the capacity limit itself: 8192 keyframe 2 points
    assert BOW_MAX_POINTS == 8192
    big = KP(*(np.concatenate([v] * (8192 // len(k2.node) + 1))[:8192] for v in k2))
    # (a copy is an equal distance, so with its map point it fails every ratio test; without, it is passed over)
    bare = big._replace(flag=np.where(np.arange(8192) < len(k2.node), big.flag, 0))
    env = (be, None, ["L", "R"])
    (rbig, rbare) = _gpu_compare(env, [("R", k1, big), ("R", k1, bare)], 0.9, True)
    (_, res) = _gpu_compare(env, [("R", k1, big), ("R", k1, k2)], 0.9, True)
    assert res[1] >= 50 and rbig[5]["ratio_failed"] >= 50 and rbig[5]["max_seg_2"] >= 129
    assert np.array_equal(rbare[0], res[0]) and rbare[5]["flagless_passed"] > 10 * res[5]["flagless_passed"]
    m, nm, hist, cd, best = be.bow_kf_matches(1)
    assert len(m) == len(cd) == len(best) == n1 and nm == int((m >= 0).sum()) == int((cd == BOWKF_MATCHED).sum())
    with pytest.raises(og.OrbGpuError) as e:
        be.bow_kf_matches(2)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # caller capacity below N1
        be.bow_kf_matches(0, cap=n1 - 1)
    assert e.value.code == -2
    over = np.concatenate([_points(big), pts[:1]])
    assert code([1], [over], [nodes]) == -2  # one keyframe 2 point above the limit
    be.close()


@pytest.mark.gpu
def test_gpu_search_by_bow_kf_keeps_its_results_and_leaves_the_other_searches_theirs(gpu_env, oracle):
    import orbslam3lib_amd as og
    be, fr, names = gpu_env
    A, B = fr["L0"], fr["R0"]
    kps, desc, _ = be.result(0)
    desc = desc.reshape(-1, 32)
    bounds = [float(v) for v in oracle.undistort_grid(kps, K_, D_, 640, 480)[1]]
    a = 0.02
    scw = (1.7, np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]), 1.7 * np.array([0.1, -0.05, 0.2]))
    sp = synth.sim3_points(A.xy, kps, desc, K_, scw, n=600, seed=5, bounds=bounds)
    poses = np.array([synth.sim3_pose(scw)[0]], og.RELOC_POSE_DTYPE)
    bp = np.zeros(len(B.ang), og.BOW_POINT_DTYPE)
    bp["desc"], bp["angle"], bp["node"], bp["flags"] = B.desc, B.ang, _desc_nodes(B), og.BOW_HAS_POINT
    tp = np.zeros(len(B.ang), og.TRIANG_POINT_DTYPE)
    tp["desc"], tp["x"], tp["y"], tp["angle"] = B.desc, B.xy[:, 0], B.xy[:, 1], B.ang
    tp["octave"], tp["node"] = B.octv, _desc_nodes(B)
    nodes = [_desc_nodes(A).astype(np.int32)]

    def others(n):
        be.search_by_bow([0], [bp[:n]], nodes)
        be.search_for_triangulation([0], [tp[:n]], np.zeros(1, og.TRIANG_PAIR_DTYPE), nodes, coarse=True, check_orientation=True)
        be.sim3_search_by_projection([0], [0], [sp[:n]], poses, K_, th=8.0, ratio_hamming=1.5, projection=og.SIM3_PROJECT_INVZ)
        return be.bow_matches(0), be.triangulation_matches(0), be.sim3_matches(0)
    before = others(600)
    assert before[0][1] >= 50 and before[1][1] >= 50 and before[2][4] >= 50
    pairs = _three_keyframes(fr)
    want = _gpu_compare(gpu_env, pairs, 0.9, True)
    for got, was in zip((be.bow_matches(0), be.triangulation_matches(0), be.sim3_matches(0)), before):
        for x, y in zip(got, was):
            np.testing.assert_array_equal(x, y)
    others(300)  # a following search_by_bow, search_for_triangulation and sim3_search_by_projection
    for p in range(3):
        _assert_pair(be, p, want[p], "after the others")
    assert want[0][1] >= 100
