"""ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&) -- the matcher of
Tracking::TrackReferenceKeyFrame and Tracking::Relocalization (cpp/src/ORBmatcher.cc:224-426, with
ComputeThreeMaxima :2061-2102), pinhole frames (F.Nleft == -1).  The vocabulary stays on the host:
the node of each keypoint (mFeatVec) is an input on both sides.

The yardstick is _py_bow below: an independent restatement written from those lines with
np.float32 scalars, which also returns a Counter of the rules it hit.
CPU: the restatement against hand-built known answers on tiny frames (taken keypoints, the ratio
test at equality, the lone candidate against 256, TH_LOW, equal distances, nodes of one side only,
negative / unsorted / very large node ids, the map-point flag, bin edges, three-maxima ties, the two
deviations, no orientation check); conditions on the scenes the GPU cases use; the exported symbols
and the statuses decided before any launch.
GPU: k_bow_group + k_bow_match + k_bow_finish against the restatement, equal on match, nmatches and
the 30 histogram bins.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs the SLAM stack; no
fixtures ship for it) -- restatement only, as for the other matcher functions."""
from collections import Counter, namedtuple

import numpy as np
import pytest

from orbslam3lib_amd import BOW_HAS_POINT, BOW_MAX_POINTS, BOW_POINT_DTYPE, synth
from tests.test_search_for_initialization import RNG_D, Fr, _bits, _extractor, _gpu_frames, _images
from tests.test_track_projection import D_, F32, K_, _flip, _header_struct_bytes, _rot_bin, _three_maxima

TH_LOW = 50
NODE_MAX = 2 ** 31 - 1

KF = namedtuple("KF", "desc ang node flag")  # the keyframe: mDescriptors, mvKeysUn.angle, node, map point and not bad
FB = namedtuple("FB", "desc ang node")       # the frame: mDescriptors, mvKeys.angle, node


def _hamming_matrix(a, b):
    """[len(a), len(b)] Hamming distances of two [n, 32] uint8 descriptor arrays."""
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int32)
    x = np.unpackbits(np.asarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    y = np.unpackbits(np.asarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (x @ (1 - y).T + (1 - x) @ y.T).astype(np.int32)  # sums of at most 256 ones: exact


def _feat_vec(nodes):
    """mFeatVec: node -> keypoint indices in ascending order; a negative node is in none."""
    fv = {}
    for i, nd in enumerate(nodes):
        if nd >= 0:
            fv.setdefault(int(nd), []).append(i)
    return fv


def _py_bow(kf, F, nnratio, check):
    """-> match [N] (index into the keyframe's points or -1), nmatches, bin sizes [30] (before the
    three-maxima rule), Counter of the rules."""
    n = len(F.node)
    match = [-1] * n  # :228
    H = _hamming_matrix(kf.desc, F.desc)
    fvk, fvf = _feat_vec(kf.node), _feat_vec(F.node)
    bins = [[] for _ in range(30)]
    cnt = Counter()
    ratio = F32(nnratio)
    nm = 0
    for node in sorted(fvk):  # :245-403: the nodes present in both, ascending
        if node not in fvf:
            continue
        cnt["common_nodes"] += 1
        idx_f = fvf[node]
        cnt["max_f_in_node"] = max(cnt["max_f_in_node"], len(idx_f))
        for rk in fvk[node]:  # :252
            if not (int(kf.flag[rk]) & 1):  # :258-262
                cnt["no_map_point"] += 1
                continue
            row = H[rk].tolist()
            best1 = best2 = 256  # :266-268
            bi = -1
            low, low_taken, free = 257, False, 0
            for rf in idx_f:  # :274
                d = row[rf]
                if d < low:  # instrumentation only
                    low, low_taken = d, match[rf] != -1
                if match[rf] != -1:  # :279-280
                    cnt["taken_skipped"] += 1
                    continue
                free += 1
                if d < best1:  # :286-295
                    best2, best1, bi = best1, d, rf
                elif d < best2:
                    best2 = d
            if best1 > TH_LOW:  # :328
                cnt["above_th_low"] += 1
                continue
            if not bool(F32(best1) < ratio * F32(best2)):  # :330
                cnt["ratio_failed"] += 1
                continue
            cnt["events"] += 1
            cnt["lone"] += free == 1
            cnt["promoted"] += low_taken
            match[bi] = rk  # :332
            nm += 1  # :355
            if check:  # :339-354
                bn = _rot_bin(kf.ang[rk], F.ang[bi])
                if bn is None:  # deviation
                    cnt["bin_out_of_range"] += 1
                else:
                    bins[bn].append(bi)
    hist = np.array([len(e) for e in bins], np.int32)
    if check:  # :405-423
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn in keep:
                continue
            for bi in bins[bn]:
                match[bi] = -1
                nm -= 1
                cnt["rejected"] += 1
    return np.array(match, np.int32).reshape(-1), nm, hist, cnt


# ---- hand-built frames --------------------------------------------------------------------------

def _kf(points):
    """points: (desc [32] u8, angle, node[, flag = 1])."""
    return KF(np.array([p[0] for p in points], np.uint8).reshape(-1, 32), np.array([p[1] for p in points], F32),
              np.array([p[2] for p in points], np.int64), np.array([p[3] if len(p) > 3 else 1 for p in points], np.int32))


def _fb(points):
    """points: (desc [32] u8, angle, node)."""
    return FB(np.array([p[0] for p in points], np.uint8).reshape(-1, 32), np.array([p[1] for p in points], F32),
              np.array([p[2] for p in points], np.int64))


Z, E = _bits(), _bits((100, 140))


def test_an_earlier_keypoint_takes_what_a_later_closer_one_would_have_won():
    F = _fb([(Z, 0.0, 5), (E, 0.0, 5)])
    # k0 is 10 from f0 (50 from f1) and takes it; k1, 3 from f0, finds it taken: its next best is f1 at 43
    m, nm, _, cnt = _py_bow(_kf([(_bits((0, 10)), 0.0, 5), (_bits((0, 3)), 0.0, 5)]), F, 0.9, True)
    assert list(m) == [0, 1] and nm == 2 and cnt["taken_skipped"] == 1 and cnt["promoted"] == 1 and cnt["lone"] == 1
    # eight bits farther (51 from f1) the later one takes nothing
    m, nm, _, cnt = _py_bow(_kf([(_bits((0, 10)), 0.0, 5), (_bits((0, 3), (200, 208)), 0.0, 5)]), F, 0.9, True)
    assert list(m) == [0, -1] and nm == 1 and cnt["above_th_low"] == 1 and cnt["promoted"] == 0
    # the other order: the closer one comes first and wins f0, the farther one is left with f1 (50)
    m, nm, _, _ = _py_bow(_kf([(_bits((0, 3)), 0.0, 5), (_bits((0, 10)), 0.0, 5)]), F, 0.9, True)
    assert list(m) == [0, 1] and nm == 2


def test_a_taken_keypoint_no_longer_counts_as_second_best():
    X, Y = _bits((0, 10)), _bits((10, 20))
    F = _fb([(X, 0.0, 1), (Y, 0.0, 1)])
    # alone, Z is 10 from both: 10 < 0.9 * 10 fails
    m, nm, _, cnt = _py_bow(_kf([(Z, 0.0, 1)]), F, 0.9, True)
    assert nm == 0 and list(m) == [-1, -1] and cnt["ratio_failed"] == 1
    # after X's own point took X, Y is a lone candidate for Z: 10 < 0.9 * 256 passes
    m, nm, _, cnt = _py_bow(_kf([(X, 0.0, 1), (Z, 0.0, 1)]), F, 0.9, True)
    assert list(m) == [0, 1] and nm == 2 and cnt["lone"] == 1 and cnt["promoted"] == 1 and cnt["ratio_failed"] == 0


def test_ratio_fails_at_equality_and_a_lone_candidate_passes_against_256():
    assert F32(0.7) * F32(10) == F32(7) and F32(0.9) * F32(10) == F32(9)  # both products round to the integer
    for ratio, best in ((0.7, 7), (0.9, 9)):
        F = _fb([(_bits((0, best)), 0.0, 3), (_bits((best, best + 10)), 0.0, 3)])  # best and 10 from zero
        _, nm, _, cnt = _py_bow(_kf([(Z, 0.0, 3)]), F, ratio, True)
        assert nm == 0 and cnt["ratio_failed"] == 1  # best < best.0f is false
        F = _fb([(_bits((0, best - 1)), 0.0, 3), (_bits((best, best + 10)), 0.0, 3)])
        assert _py_bow(_kf([(Z, 0.0, 3)]), F, ratio, True)[1] == 1
    # a lone candidate: bestDist2 stays 256 (not INT_MAX): 50 < 0.7 * 256, but not 50 < 0.19 * 256 = 48.64
    lone = _fb([(_bits((0, 50)), 0.0, 3)])
    m, nm, _, cnt = _py_bow(_kf([(Z, 0.0, 3)]), lone, 0.7, True)
    assert nm == 1 and list(m) == [0] and cnt["lone"] == 1
    assert _py_bow(_kf([(Z, 0.0, 3)]), lone, 0.19, True)[1] == 0
    assert _py_bow(_kf([(Z, 0.0, 3)]), lone, 0.2, True)[1] == 1  # 51.2


def test_best_50_passes_and_51_fails():
    for nbits, want in ((50, 1), (51, 0)):
        _, nm, _, cnt = _py_bow(_kf([(Z, 0.0, 0)]), _fb([(_bits((0, nbits)), 0.0, 0)]), 0.7, True)
        assert nm == want and cnt["above_th_low"] == 1 - want


def test_an_equal_distance_is_the_second_best_not_the_best():
    F = _fb([(_bits((0, 7)), 0.0, 2), (_bits((7, 14)), 0.0, 2)])  # both 7 from zero
    m, nm, _, _ = _py_bow(_kf([(Z, 0.0, 2)]), F, 1.5, True)
    assert list(m) == [0, -1] and nm == 1  # the first keeps the best; 7 < 1.5 * 7
    assert _py_bow(_kf([(Z, 0.0, 2)]), F, 1.0, True)[1] == 0  # the equal one is the second best: 7 < 7 fails


def test_nodes_of_one_side_negative_unsorted_and_very_large_ids():
    D = RNG_D
    kf = _kf([(D[0], 0.0, NODE_MAX), (D[1], 0.0, 5), (D[2], 0.0, -1), (D[3], 0.0, 7), (D[4], 0.0, 0),
              (D[5], 0.0, 1 << 30), (D[6], 0.0, -7)])
    F = _fb([(D[4], 0.0, 0), (D[3], 0.0, 9), (D[2], 0.0, -1), (D[1], 0.0, 5), (D[0], 0.0, NODE_MAX),
             (D[6], 0.0, -7), (D[5], 0.0, 1 << 30), (D[0], 0.0, NODE_MAX - 1)])
    m, nm, _, cnt = _py_bow(kf, F, 0.7, True)
    # node 7 is the keyframe's only, 9 and NODE_MAX - 1 the frame's only; equal negative values are no node
    assert list(m) == [4, -1, -1, 1, 0, -1, 5, -1] and nm == 4 and cnt["common_nodes"] == 4 and cnt["lone"] == 4


def test_a_keyframe_keypoint_without_a_map_point_neither_matches_nor_blocks():
    D = RNG_D[0]
    m, nm, _, cnt = _py_bow(_kf([(D, 0.0, 4, 0), (_flip(D, 3), 0.0, 4, 1)]), _fb([(D, 0.0, 4)]), 0.7, True)
    assert list(m) == [1] and nm == 1 and cnt["no_map_point"] == 1 and cnt["taken_skipped"] == 0
    assert _py_bow(_kf([(D, 0.0, 4, 0)]), _fb([(D, 0.0, 4)]), 0.7, True)[1] == 0
    # only bit 0 of the flags counts
    assert _py_bow(_kf([(D, 0.0, 4, 2)]), _fb([(D, 0.0, 4)]), 0.7, True)[1] == 0


@pytest.mark.parametrize("a1,a2,expect", [(14.9, 0.0, 0), (15.0, 0.0, 1), (359.0, 0.0, 12), (0.0, 0.5, 12),
                                          (44.9, 0.0, 1), (45.1, 0.0, 2), (10.0, 350.0, 1)])
def test_rotation_bin_edges(a1, a2, expect):
    """rot = keyframe angle - frame angle, the factor is 1 / 30."""
    D = RNG_D[1]
    _, nm, hist, _ = _py_bow(_kf([(D, a1, 0)]), _fb([(D, a2, 0)]), 0.7, True)
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1


def _bin_scene(sizes, extra_kf=(), extra_f=()):
    """{bin: events}: every event in a node of its own."""
    kf, fb, k = list(extra_kf), list(extra_f), 0
    for bn, n in sizes.items():
        for _ in range(n):
            kf.append((RNG_D[k], 30.0 * bn, 100 + k))
            fb.append((RNG_D[k], 0.0, 100 + k))
            k += 1
    return _kf(kf), _fb(fb)


def test_three_maxima_ties_and_cutoffs():
    def scene(sizes):
        return _py_bow(*_bin_scene(sizes), 0.7, True)
    # strict >: the earlier bins win the tie, the fourth is rejected
    m, nm, hist, cnt = scene({2: 5, 5: 5, 7: 5, 9: 5})
    assert list(hist[[2, 5, 7, 9]]) == [5, 5, 5, 5] and nm == 15 and cnt["rejected"] == 5 and (m[15:] == -1).all()
    # exactly 10%: 0.1f * 10.0f rounds to 1.0f, so one event beside ten is kept
    assert scene({0: 10, 3: 1})[1] == 11
    # max2 below 10%: the second and the third are dropped together
    _, nm, _, cnt = scene({4: 22, 1: 2, 8: 2})
    assert nm == 22 and cnt["rejected"] == 4
    # only max3 below 10%
    assert scene({4: 22, 1: 3, 8: 2})[1] == 25


def test_the_bin_out_of_range_deviation_and_no_orientation_check():
    # an angle far outside [0, 360): the event counts, enters no bin and survives the rejection that takes
    # the lone event of bin 5
    D = RNG_D
    kf, fb = _bin_scene({1: 11}, [(D[40], 1000.0, 1), (D[41], 150.0, 2)], [(D[40], 0.0, 1), (D[41], 0.0, 2)])
    m, nm, hist, cnt = _py_bow(kf, fb, 0.7, True)
    assert cnt["bin_out_of_range"] == 1 and hist.sum() == 12 and hist[1] == 11 and hist[5] == 1
    assert cnt["rejected"] == 1 and m[0] == 0 and m[1] == -1 and nm == 12
    kf.ang[0] = np.nan
    assert _py_bow(kf, fb, 0.7, True)[1] == 12
    # no orientation check: no bins, nothing rejected
    m, nm, hist, cnt = _py_bow(kf, fb, 0.7, False)
    assert hist.sum() == 0 and nm == 13 and cnt["rejected"] == 0 and (m >= 0).all()


# ---- ABI ----------------------------------------------------------------------------------------

def test_symbols_and_statuses_decided_before_any_launch():
    import orbslam3lib_amd as og
    names = {"orbgpu_search_by_bow_batch", "orbgpu_download_bow_matches"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "search_by_bow") and hasattr(og.BatchExtractor, "bow_matches")
    assert BOW_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_bow_point") == 44 and BOW_HAS_POINT == 1
    assert [og.BOW_POINT_DTYPE.fields[f][1] for f in ("desc", "angle", "node", "flags")] == [0, 32, 36, 40]
    one = np.zeros(1, np.int32)
    assert lib.orbgpu_search_by_bow_batch(None, 1, og._p(one), None, None, None, 0, og.C.c_float(0.7), 1, None) == -3
    assert lib.orbgpu_search_by_bow_batch(None, 0, None, None, None, None, 0, og.C.c_float(0.7), 1, None) == -3
    assert lib.orbgpu_download_bow_matches(None, 0, None, 0, None, None, None) == -3
    # the wrapper refuses lists that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, og.BOW_POINT_DTYPE)
    nodes = np.zeros(4, np.int32)
    with pytest.raises(ValueError):
        be.search_by_bow([0, 1], [pts], [nodes, nodes])
    with pytest.raises(ValueError):
        be.search_by_bow([0, 1], [pts, pts], [nodes])
    with pytest.raises(ValueError):
        be.search_by_bow([0, 1], [pts, pts], np.zeros((3, 4), np.int32))
    with pytest.raises(ValueError):
        be.search_by_bow([0, 1], (pts, np.array([0, 3], np.int32)), [nodes, nodes])
    with pytest.raises(ValueError):  # offsets beyond the points
        be.search_by_bow([0], (pts, np.array([0, 4], np.int32)), [nodes])


# ---- scenes -------------------------------------------------------------------------------------

def _desc_nodes(fr):
    return (fr.desc[:, 0] >> 2).astype(np.int64)


def _cell_nodes(fr):
    """floor(x / 80) * 64 + floor(y / 60) on mvKeysUn (negative left of or above the image: no node)."""
    return (np.floor(fr.xy[:, 0] / F32(80)).astype(np.int64) * 64 + np.floor(fr.xy[:, 1] / F32(60)).astype(np.int64))


def _flags(n):
    return (np.arange(n) % 5 != 0).astype(np.int32)


CHUNK_N = (1, 63, 64, 65, 129)  # frame keypoints in the node: around the 64-lane chunks of k_bow_match

# name -> (keyframe image, frame image, nodes, nnratio, check_orientation)
SCENES = {
    "tiled_desc": ("T0", "TQ", "desc", 0.9, True),
    "tiled_no_orientation": ("T0", "TQ", "desc", 0.9, False),
    "left_right_cells": ("L0", "R0", "cell", 0.7, True),
    "rotated_180": ("L0", "rot", "desc", 0.7, True),
    "unrelated_cells": ("L0", "L1", "cell", 0.7, True),
    "left_right_one_node": ("L0", "R0", "one", 0.9, True),
    "tiled_sparse": ("T0", "TQ", "sparse", 0.9, True),
}
SCENES.update({"tiled_first_%d" % n: ("T0", "TQ", ("first", n), 0.9, True) for n in CHUNK_N})
ENV1 = ("left_right_cells", "unrelated_cells", "left_right_one_node")  # images L0 R0 L1 R1; the rest: L0 rot T0 TQ


def _scene(frames, name):
    """-> (KF, FB, nnratio, check) of a scene on frames (Fr records by image name)."""
    k, f, nodes, ratio, check = SCENES[name]
    A, B = frames[k], frames[f]
    if nodes == "desc":
        nk, nf = _desc_nodes(A), _desc_nodes(B)
    elif nodes == "cell":
        nk, nf = _cell_nodes(A), _cell_nodes(B)
    elif nodes == "one":
        nk, nf = np.zeros(len(A.ang), np.int64), np.zeros(len(B.ang), np.int64)
    elif nodes == "sparse":
        nk, nf = _desc_nodes(A), _desc_nodes(B)
        nk = np.where(nk % 2 == 0, nk * 1000003 % NODE_MAX, -1)
        nf = np.where(nf % 3 == 0, nf * 1000003 % NODE_MAX, -1)
    else:
        nk = np.full(len(A.ang), 7, np.int64)
        nf = np.where(np.arange(len(B.ang)) < nodes[1], 7, -1).astype(np.int64)
    return KF(A.desc, A.ang, nk, _flags(len(A.ang))), FB(B.desc, B.ang, nf), ratio, check


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
        kf, fb, ratio, check = _scene(cpu_frames, name)
        res[name] = _py_bow(kf, fb, ratio, check)
        print(name, "nmatches", res[name][1], dict(res[name][3]), "bins", np.flatnonzero(res[name][2]).tolist())
    c = res["tiled_desc"][3]
    assert c["events"] >= 200 and c["promoted"] >= 40 and c["taken_skipped"] >= 3000 and c["ratio_failed"] >= 150
    assert c["above_th_low"] >= 70 and c["rejected"] >= 50 and c["lone"] >= 1 and c["max_f_in_node"] >= 129
    assert np.flatnonzero(res["tiled_desc"][2]).tolist() == [0, 3, 6, 9, 12]
    assert res["tiled_no_orientation"][2].sum() == 0 and res["tiled_no_orientation"][3]["rejected"] == 0
    c = res["left_right_cells"][3]
    assert c["events"] >= 200 and c["promoted"] >= 3 and c["above_th_low"] >= 200 and c["no_map_point"] >= 100
    assert res["rotated_180"][1] >= 300 and int(np.argmax(res["rotated_180"][2])) == 6
    assert res["unrelated_cells"][1] == 0
    c = res["left_right_one_node"][3]
    assert c["max_f_in_node"] == len(cpu_frames["R0"].ang) and c["events"] >= 200 and c["rejected"] >= 3
    c = res["tiled_first_1"][3]
    assert c["events"] == 1 and c["lone"] == 1
    for n in CHUNK_N[1:]:
        c = res["tiled_first_%d" % n][3]
        assert c["max_f_in_node"] == n and c["events"] >= 30 and c["promoted"] >= 10, n
    c = res["tiled_sparse"][3]
    assert c["common_nodes"] >= 5 and c["events"] >= 30


# ---- GPU ----------------------------------------------------------------------------------------

def _kf_points(kf):
    pts = np.zeros(len(kf.node), BOW_POINT_DTYPE)
    pts["desc"], pts["angle"], pts["node"], pts["flags"] = kf.desc, kf.ang, kf.node, kf.flag
    return pts


def _env(names):
    be = _extractor([_images()[k] for k in names])
    return be, _gpu_frames(be, names), names


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


def _gpu_compare(env, pairs, ratio, check, packed=False):
    """pairs: (frame image name, KF, FB) per pair of one call -> the restatement's results."""
    be, _, names = env
    pts = [_kf_points(kf) for _, kf, _ in pairs]
    if packed:
        off = np.zeros(len(pts) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in pts])
        pts = (np.concatenate(pts), off)
    be.search_by_bow([names.index(f) for f, _, _ in pairs], pts, [fb.node.astype(np.int32) for _, _, fb in pairs],
                     nnratio=ratio, check_orientation=check)
    out = []
    for p, (_, kf, fb) in enumerate(pairs):
        m, nm, hist, cnt = _py_bow(kf, fb, ratio, check)
        gm, gnm, ghist = be.bow_matches(p)
        np.testing.assert_array_equal(gm, m, err_msg="pair %d match" % p)
        assert gnm == nm, (p, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="pair %d histogram" % p)
        out.append((m, nm, hist, cnt))
    return out


def _gpu_scene(env, name):
    kf, fb, ratio, check = _scene(env[1], name)
    (res,) = _gpu_compare(env, [(SCENES[name][1], kf, fb)], ratio, check)
    print(name, "nmatches", res[1], dict(res[3]))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENV1)
def test_gpu_search_by_bow_stereo_scenes(gpu_env, name):
    _, nm, _, cnt = _gpu_scene(gpu_env, name)
    if name == "left_right_cells":
        assert cnt["events"] >= 200 and cnt["promoted"] >= 3 and cnt["no_map_point"] >= 100
    if name == "unrelated_cells":
        assert nm == 0
    if name == "left_right_one_node":  # the longest sequential chain, a segment far above one wave
        assert cnt["max_f_in_node"] == len(gpu_env[1]["R0"].ang) >= 500 and cnt["events"] >= 200 and cnt["rejected"] >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in SCENES if n not in ENV1])
def test_gpu_search_by_bow_texture_scenes(gpu_env2, name):
    _, nm, hist, cnt = _gpu_scene(gpu_env2, name)
    if name == "tiled_desc":
        assert cnt["promoted"] >= 40 and cnt["taken_skipped"] >= 3000 and cnt["rejected"] >= 50 and cnt["max_f_in_node"] >= 129
    if name == "tiled_no_orientation":
        assert hist.sum() == 0 and nm == cnt["events"] >= 200
    if name == "rotated_180":
        assert nm >= 300 and int(np.argmax(hist)) == 6
    if name == "tiled_sparse":
        assert cnt["common_nodes"] >= 5 and cnt["events"] >= 30
    if name.startswith("tiled_first_") and name != "tiled_first_1":
        assert cnt["events"] >= 30 and cnt["promoted"] >= 10


@pytest.mark.gpu
def test_gpu_search_by_bow_one_frame_against_three_keyframes(gpu_env):
    """Relocalization: one frame in three pairs of one call, keyframe point counts that differ; the
    packed form and the list form give equal results."""
    fr = gpu_env[1]
    fb = FB(fr["R0"].desc, fr["R0"].ang, _desc_nodes(fr["R0"]))
    pairs = []
    for name, n in (("L0", None), ("L1", 700), ("R1", 333)):
        A = fr[name]
        n = len(A.ang) if n is None else n
        pairs.append(("R0", KF(A.desc[:n], A.ang[:n], _desc_nodes(A)[:n], _flags(n)), fb))
    res = _gpu_compare(gpu_env, pairs, 0.75, True)
    assert res[0][1] >= 100 and res[0][1] != res[1][1]
    got = [gpu_env[0].bow_matches(p) for p in range(3)]
    _gpu_compare(gpu_env, pairs, 0.75, True, packed=True)
    for p in range(3):
        again = gpu_env[0].bow_matches(p)
        assert np.array_equal(got[p][0], again[0]) and got[p][1] == again[1] and np.array_equal(got[p][2], again[2])


@pytest.mark.gpu
def test_gpu_search_by_bow_empty_sides_and_no_pairs():
    import orbslam3lib_amd as og
    env = _env(["blank", "L0"])
    be, fr, _ = env
    L = fr["L0"]
    assert len(fr["blank"].ang) == 0
    kf = KF(L.desc, L.ang, _desc_nodes(L), _flags(len(L.ang)))
    none = KF(L.desc[:0], L.ang[:0], _desc_nodes(L)[:0], _flags(0))
    neg = np.full(len(L.ang), -3, np.int64)
    res = _gpu_compare(env, [("L0", none, FB(L.desc, L.ang, _desc_nodes(L))),     # no keyframe points
                             ("blank", kf, FB(L.desc[:0], L.ang[:0], neg[:0])),   # no frame keypoints
                             ], 0.7, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][0] == -1).all() and len(res[0][0]) == len(L.ang) and len(res[1][0]) == 0
    res = _gpu_compare(env, [("L0", kf, FB(L.desc, L.ang, neg)),                          # the frame in no node
                             ("L0", kf._replace(node=neg), FB(L.desc, L.ang, _desc_nodes(L)))], 0.7, True)
    assert [r[1] for r in res] == [0, 0] and (res[0][0] == -1).all() and (res[1][0] == -1).all()
    be.search_by_bow([], [], [])  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.bow_matches(0)
    assert e.value.code == -3
    be.close()


@pytest.mark.gpu
def test_gpu_search_by_bow_status_codes_and_the_capacity_limit():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    (kl, dl, _), (kr, dr, _) = be.result(0), be.result(1)
    n1 = len(kr)
    kf = KF(dl.reshape(-1, 32), kl["angle"].astype(F32), (dl.reshape(-1, 32)[:, 0] >> 2).astype(np.int64), _flags(len(kl)))
    fb = FB(dr.reshape(-1, 32), kr["angle"].astype(F32), (dr.reshape(-1, 32)[:, 0] >> 2).astype(np.int64))
    pts, nodes = _kf_points(kf), fb.node.astype(np.int32)

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.search_by_bow(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.bow_matches(0)
    assert e.value.code == -3
    assert code([2], [pts], [nodes]) == -3 and code([-1], [pts], [nodes]) == -3  # outside the last batch
    assert code([1], [pts], [nodes[:n1 - 1]]) == -3  # node_stride below N
    assert code([1, 1], (pts, np.array([0, len(pts), 5], np.int32)), [nodes, nodes]) == -3  # descending offsets
    assert code([1] * 3, [pts] * 3, [nodes] * 3) == -3  # above the context's image capacity
    # the call works before undistort_grid, and at the capacity limit itself: 8192 keyframe points
    assert BOW_MAX_POINTS == 8192
    big = KF(*(np.concatenate([v] * (8192 // len(kf.node) + 1))[:8192] for v in kf))
    (res, _) = _gpu_compare((be, None, ["L", "R"]), [("R", big, fb), ("R", kf, fb)], 0.7, True)
    assert res[1] >= 50
    m, nm, hist = be.bow_matches(1)
    assert len(m) == n1 and nm == int((m >= 0).sum())
    with pytest.raises(og.OrbGpuError) as e:
        be.bow_matches(2)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # caller capacity below N
        be.bow_matches(0, cap=n1 - 1)
    assert e.value.code == -2
    over = np.concatenate([_kf_points(big), pts[:1]])
    assert code([1], [over], [nodes]) == -2  # one keyframe point above the limit
    be.close()
