"""ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) -- the matcher
of Tracking::MonocularInitialization (cpp/src/ORBmatcher.cc:649-764, with ComputeThreeMaxima
:2061-2102 and Frame::GetFeaturesInArea, Frame.cc:673-739).

The yardstick is _py_init below: an independent restatement written from those lines with
np.float32 scalars, which also returns a Counter of the rules it hit.
CPU: the restatement against hand-built known answers on a tiny frame (robbed owners, the
matched-distance filter, the ratio test at equality, TH_LOW, robbed entries in rejected bins, bin
edges, three-maxima ties, the level rule, empty windows, vbPrevMatched, the two deviations);
conditions on the scenes the GPU cases use; the exported symbols and the statuses decided before
any launch.
GPU: k_init_candidates + k_init_replay against the restatement, bit for bit on vnMatches12,
nmatches, the 30 histogram bins and the returned vbPrevMatched.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs the SLAM stack; no
fixtures ship for it) -- restatement only, as for the other matcher functions."""
from collections import Counter, namedtuple

import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_track_projection import BT, D_, F32, K_, POP, _flip, _grid, _rot_bin, _three_maxima, _window

INT_MAX = 2147483647
TH_LOW = 50
KEPT = 4  # candidates k_init_candidates keeps per window (instrumentation only)

Fr = namedtuple("Fr", "xy octv ang desc cs ci")


def _py_init(F1, F2, prev, bounds, window, nnratio, check):
    """-> vnMatches12 [N1], vbPrevMatched [N1, 2], nmatches, bin sizes [30] (before the
    three-maxima rule), Counter of the rules."""
    n1, n2 = len(F1.octv), len(F2.octv)
    prev = np.array(F1.xy if prev is None else prev, F32).reshape(-1, 2).copy()
    m12 = np.full(n1, -1, np.int32)  # :652
    md = [INT_MAX] * n2  # :659
    m21 = [-1] * n2  # :660
    bins = [[] for _ in range(30)]
    cnt = Counter()
    b = np.asarray(bounds, F32)
    r, ratio = F32(window), F32(nnratio)
    nm = 0
    for i1 in range(n1):  # :662
        level1 = int(F1.octv[i1])
        if level1 > 0:  # :665-667
            cnt["level_skipped"] += 1
            continue
        x, y = prev[i1]
        if not (np.isfinite(x) and np.isfinite(y)):  # deviation
            cnt["not_finite"] += 1
            continue
        cand = _window(F2.xy, F2.octv, F2.cs, F2.ci, b, x, y, r, level1, level1)  # :669
        if not cand:  # :671-672
            cnt["empty_window"] += 1
            continue
        cnt["searched"] += 1
        best = best2 = INT_MAX
        bi = -1
        seen = []  # (distance, window position, filtered)
        for pos, i2 in enumerate(cand):
            d = int(POP[np.bitwise_xor(F1.desc[i1], F2.desc[i2])].sum())
            if md[i2] <= d:  # :688-689
                seen.append((d, pos, True))
                cnt["filtered"] += 1
                continue
            seen.append((d, pos, False))
            if d < best:  # :691-700
                best2, best, bi = best, d, i2
            elif d < best2:
                best2 = d
        # instrumentation only
        low = sorted(seen)
        dry = len(low) > KEPT and sum(not f for _, _, f in low[:KEPT]) < 2
        cnt["second_walk"] += dry
        event = best <= TH_LOW and bool(F32(best) < F32(best2) * ratio)  # :703-705
        if not event:
            cnt["above_th_low" if best > TH_LOW else "ratio_failed"] += 1
            continue
        cnt["events"] += 1
        cnt["lone"] += best2 == INT_MAX
        cnt["second_walk_event"] += dry
        cnt["promoted"] += low[0][2]  # the lowest distance of the window was filtered
        if not low[0][2] and len(low) > 1 and low[1][2]:
            cnt["second_freed"] += not bool(F32(low[0][0]) < F32(low[1][0]) * ratio)
        if m21[bi] >= 0:  # :707-711
            m12[m21[bi]] = -1
            nm -= 1
            cnt["robbed"] += 1
        m12[i1] = bi  # :712-715
        m21[bi] = i1
        md[bi] = best
        nm += 1
        if check:  # :717-727
            bn = _rot_bin(F1.ang[i1], F2.ang[bi])
            if bn is None:  # deviation
                cnt["bin_out_of_range"] += 1
            else:
                bins[bn].append(i1)
    hist = np.array([len(e) for e in bins], np.int32)
    if check:  # :733-756
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn in keep:
                continue
            cnt["rejected_bin_max"] = max(cnt["rejected_bin_max"], len(bins[bn]))
            for i1 in bins[bn]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nm -= 1
                    cnt["rejected"] += 1
                else:
                    cnt["rejected_already_robbed"] += 1
    for i1 in range(n1):  # :759-761
        if m12[i1] >= 0:
            prev[i1] = F2.xy[m12[i1]]
    return m12, prev, nm, hist, cnt


# ---- hand-built frames --------------------------------------------------------------------------

def _frame(points):
    """points: (x, y, octave, angle, desc [32] u8)."""
    xy = np.array([(p[0], p[1]) for p in points], F32).reshape(-1, 2)
    cs, ci = _grid(xy, BT)
    return Fr(xy, np.array([p[2] for p in points], np.int32), np.array([p[3] for p in points], F32),
              np.array([p[4] for p in points], np.uint8).reshape(-1, 32), cs, ci)


def _bits(*ranges):
    """A descriptor with the bits of the given [lo, hi) ranges set."""
    v = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        v[lo:hi] = 1
    return np.packbits(v)


RNG_D = np.random.default_rng(11).integers(0, 256, (64, 32), dtype=np.uint8)  # unrelated descriptors
SPOTS = [(60.0 + 70 * i, 60.0 + 70 * j) for j in range(5) for i in range(8)]  # windows of 20 do not meet


def _run(F1, F2, prev=None, window=20, nnratio=0.9, check=True):
    return _py_init(F1, F2, prev, BT, window, nnratio, check)


def _fill(n, angle=30.0, first=8):
    """n matched pairs at SPOTS[first:], every one an event of bin round(angle / 30)."""
    return ([(SPOTS[first + k][0], SPOTS[first + k][1], 0, angle, RNG_D[first + k]) for k in range(n)],
            [(SPOTS[first + k][0], SPOTS[first + k][1], 0, 0.0, RNG_D[first + k]) for k in range(n)])


def test_a_later_closer_point_robs_the_earlier_owner():
    D = RNG_D[0]
    F2 = _frame([(60, 60, 0, 0.0, D)])
    F1 = _frame([(60, 60, 0, 0.0, _flip(D, 10)), (62, 60, 0, 0.0, _flip(D, 3, 1))])
    m, prev, nm, _, cnt = _run(F1, F2)
    assert list(m) == [-1, 0] and nm == 1 and cnt["robbed"] == 1 and cnt["events"] == 2 and cnt["lone"] == 2
    np.testing.assert_array_equal(prev, np.array([(60, 60), (60, 60)], F32))  # only the match moves
    # the other order: the later, farther point is filtered and finds nothing else
    F1 = _frame([(62, 60, 0, 0.0, _flip(D, 3, 1)), (60, 60, 0, 0.0, _flip(D, 10))])
    m, _, nm, _, cnt = _run(F1, F2)
    assert list(m) == [0, -1] and nm == 1 and cnt["robbed"] == 0 and cnt["filtered"] == 1


def test_a_later_farther_or_equal_point_is_filtered_and_takes_its_next_best_or_nothing():
    D, A, B, C = _bits(), _bits((0, 3)), _bits((3, 6)), _bits((0, 6), (100, 104))
    F1 = _frame([(60, 60, 0, 0.0, A), (60, 60, 0, 0.0, B), (60, 60, 0, 0.0, C)])
    m, _, nm, _, cnt = _run(F1, _frame([(60, 60, 0, 0.0, D)]))
    assert list(m) == [0, -1, -1] and nm == 1 and cnt["filtered"] == 2  # equal (3 <= 3) and farther (3 <= 10)
    # a second keypoint 8 px away, 40 bits from the first: the next best of B (43), which C (42) then robs
    E = _bits((100, 140))
    m, _, nm, _, cnt = _run(F1, _frame([(60, 60, 0, 0.0, D), (68, 60, 0, 0.0, E)]))
    assert list(m) == [0, -1, 1] and nm == 2 and cnt["robbed"] == 1 and cnt["promoted"] == 2
    # one bit farther, C is filtered on both keypoints and takes nothing
    F1.desc[2] = _bits((0, 6), (100, 103))
    m, _, nm, _, cnt = _run(F1, _frame([(60, 60, 0, 0.0, D), (68, 60, 0, 0.0, E)]))
    assert list(m) == [0, 1, -1] and nm == 2 and cnt["robbed"] == 0 and cnt["filtered"] == 3


def test_a_filtered_keypoint_no_longer_counts_as_second_best():
    X, Y, Z = _bits((0, 10)), _bits((10, 20)), _bits()
    F2 = _frame([(60, 60, 0, 0.0, X), (64, 60, 0, 0.0, Y)])
    # alone, the point Z is 10 from both: 10 < 10 * 0.9 fails
    m, _, nm, _, cnt = _run(_frame([(60, 60, 0, 0.0, Z)]), F2)
    assert nm == 0 and cnt["ratio_failed"] == 1
    # after an earlier point took X at distance 0, X is filtered for Z: Y is a lone candidate and passes
    m, _, nm, _, cnt = _run(_frame([(60, 60, 0, 0.0, X), (60, 60, 0, 0.0, Z)]), F2)
    assert list(m) == [0, 1] and nm == 2 and cnt["promoted"] == 1 and cnt["lone"] == 1
    # the same with the filtered keypoint as the second best of the window: P is 1 from Y and 19 from X
    P = (60, 60, 0, 0.0, _bits((10, 19)))
    assert _run(_frame([P]), F2, nnratio=0.05)[2] == 0  # 1 < 19 * 0.05 fails
    m, _, nm, _, cnt = _run(_frame([(60, 60, 0, 0.0, X), P]), F2, nnratio=0.05)
    assert list(m) == [0, 1] and cnt["second_freed"] == 1 and cnt["promoted"] == 0  # 1 < INT_MAX * 0.05 passes


def test_ratio_fails_at_equality_and_a_lone_candidate_passes():
    X, Y = _bits((0, 5)), _bits((5, 15))
    F2 = _frame([(60, 60, 0, 0.0, X), (64, 60, 0, 0.0, Y)])
    F1 = _frame([(60, 60, 0, 0.0, _bits())])  # 5 and 10
    assert _run(F1, F2, nnratio=0.5)[2] == 0  # 5 < 10 * 0.5 is false
    assert _run(F1, F2, nnratio=0.51)[2] == 1
    assert F32(10) * F32(0.9) == F32(9)  # 0.9f * 10 rounds up to 9
    F2 = _frame([(60, 60, 0, 0.0, _bits((0, 9))), (64, 60, 0, 0.0, _bits((9, 19)))])  # 9 and 10 from zero
    assert _run(_frame([(60, 60, 0, 0.0, _bits())]), F2)[2] == 0  # 9 < 9.0f is false
    assert _run(_frame([(60, 60, 0, 0.0, _bits())]), F2, nnratio=1.0)[2] == 1
    # equal distances: the second of the window is the second best, never the best
    F2 = _frame([(60, 60, 0, 0.0, _bits((0, 7))), (64, 60, 0, 0.0, _bits((7, 14)))])
    m, _, nm, _, _ = _run(_frame([(60, 60, 0, 0.0, _bits())]), F2, nnratio=1.5)
    assert nm == 1 and m[0] == int(F2.ci[0])
    # a lone candidate: bestDist2 stays INT_MAX, which is 2147483648.0f
    assert F32(INT_MAX) == F32(2147483648.0)
    m, _, nm, _, cnt = _run(_frame([(60, 60, 0, 0.0, _bits())]), _frame([(60, 60, 0, 0.0, _bits((0, 50)))]))
    assert nm == 1 and cnt["lone"] == 1
    assert _run(_frame([(60, 60, 0, 0.0, _bits())]), _frame([(60, 60, 0, 0.0, _bits((0, 50)))]), nnratio=0.0)[2] == 0


def test_best_50_passes_and_51_fails():
    for nbits, want in ((50, 1), (51, 0)):
        m, _, nm, _, cnt = _run(_frame([(60, 60, 0, 0.0, _bits())]), _frame([(60, 60, 0, 0.0, _bits((0, nbits)))]))
        assert nm == want and cnt["above_th_low"] == 1 - want


def test_a_robbed_entry_still_sizes_its_bin_and_is_not_subtracted_again():
    D = RNG_D[0]
    f1, f2 = _fill(11)  # one event beside eleven is below 10% of the maximum
    A = (60, 60, 0, 150.0, _flip(D, 10))  # bin 5, alone
    B = (60, 60, 0, 30.0, _flip(D, 3, 1))  # bin 1 with the fillers: robs A
    F2 = _frame([(60, 60, 0, 0.0, D)] + f2)
    m, _, nm, hist, cnt = _run(_frame([A, B] + f1), F2)
    assert hist[5] == 1 and hist[1] == 12 and hist.sum() == 13
    assert cnt["robbed"] == 1 and cnt["rejected"] == 0 and cnt["rejected_already_robbed"] == 1
    assert nm == 12 and m[0] == -1 and m[1] == 0 and list(m[2:]) == list(range(1, 12))
    # without the robber the rejection takes A's match
    m, _, nm, hist, cnt = _run(_frame([A] + f1), F2)
    assert hist[5] == 1 and hist[1] == 11 and cnt["rejected"] == 1 and nm == 11 and m[0] == -1
    # the robber in the rejected bin, the robbed one in a kept bin: the keypoint ends up free
    A2, B2 = (60, 60, 0, 30.0, _flip(D, 10)), (60, 60, 0, 150.0, _flip(D, 3, 1))
    m, _, nm, hist, cnt = _run(_frame([A2, B2] + f1), F2)
    assert hist[1] == 12 and hist[5] == 1 and cnt["rejected"] == 1 and nm == 11 and m[0] == -1 and m[1] == -1
    # no orientation check: no bins, nothing rejected
    m, _, nm, hist, _ = _run(_frame([A, B] + f1), F2, check=False)
    assert hist.sum() == 0 and nm == 12 and m[1] == 0


@pytest.mark.parametrize("a1,a2,expect", [(14.9, 0.0, 0), (15.0, 0.0, 1), (359.0, 0.0, 12), (0.0, 0.5, 12),
                                          (44.9, 0.0, 1), (45.1, 0.0, 2), (10.0, 350.0, 1)])
def test_rotation_bin_edges(a1, a2, expect):
    """rot = F1 angle - F2 angle, the factor is 1 / 30 (row 6's parameter set)."""
    D = RNG_D[1]
    _, _, nm, hist, _ = _run(_frame([(60, 60, 0, a1, D)]), _frame([(60, 60, 0, a2, D)]))
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1


def test_three_maxima_ties_and_cutoffs():
    def scene(sizes):  # {bin: events}
        f1, f2, k = [], [], 0
        for bn, n in sizes.items():
            for _ in range(n):
                f1.append((SPOTS[k][0], SPOTS[k][1], 0, 30.0 * bn, RNG_D[k]))
                f2.append((SPOTS[k][0], SPOTS[k][1], 0, 0.0, RNG_D[k]))
                k += 1
        return _run(_frame(f1), _frame(f2))
    # strict >: the earlier bins win the tie, the fourth is rejected
    m, _, nm, hist, cnt = scene({2: 5, 5: 5, 7: 5, 9: 5})
    assert list(hist[[2, 5, 7, 9]]) == [5, 5, 5, 5] and nm == 15 and cnt["rejected"] == 5 and (m[15:] == -1).all()
    # exactly 10%: 0.1f * 10.0f rounds to 1.0f, so one event beside ten is kept
    assert scene({0: 10, 3: 1})[2] == 11
    # max2 below 10%: the second and the third are dropped together
    _, _, nm, _, cnt = scene({4: 22, 1: 2, 8: 2})
    assert nm == 22 and cnt["rejected"] == 4 and cnt["rejected_bin_max"] == 2
    # only max3 below 10%
    assert scene({4: 22, 1: 3, 8: 2})[2] == 25


def test_levels_empty_windows_and_prev():
    D = RNG_D[:4]
    F2 = _frame([(60, 60, 0, 0.0, D[0]), (130, 60, 1, 0.0, D[1]), (200, 60, 0, 0.0, D[2])])
    F1 = _frame([(60, 60, 1, 0.0, D[0]),    # octave 1 in F1: skipped
                 (130, 60, 0, 0.0, D[1]),   # its only neighbour is an octave-1 keypoint: empty window
                 (330, 200, 0, 0.0, D[2]),  # nothing near
                 (203, 64, 0, 0.0, D[2])])
    m, prev, nm, _, cnt = _run(F1, F2)
    assert list(m) == [-1, -1, -1, 2] and nm == 1
    assert cnt["level_skipped"] == 1 and cnt["empty_window"] == 2 and cnt["searched"] == 1
    np.testing.assert_array_equal(prev, np.array([(60, 60), (130, 60), (330, 200), (200, 60)], F32))
    # vbPrevMatched, not the keypoint's own position, centres the window; the strict test excludes the edge
    given = np.array([(0, 0), (0, 0), (180.5, 79.5), (400, 400)], F32)
    m, prev, nm, _, _ = _run(F1, F2, prev=given)
    assert list(m) == [-1, -1, 2, -1] and nm == 1
    np.testing.assert_array_equal(prev, np.array([(0, 0), (0, 0), (200, 60), (400, 400)], F32))
    given[2] = (180.0, 80.0)  # |dx| = 20 is not < 20
    assert _run(F1, F2, prev=given)[2] == 0


def test_the_two_deviations():
    D = RNG_D[0]
    f1, f2 = _fill(11)
    # a prev that is not finite skips the point
    F1, F2 = _frame([(60, 60, 0, 0.0, D)] + f1), _frame([(60, 60, 0, 0.0, D)] + f2)
    for bad in ((np.nan, 60), (60, np.inf), (-np.inf, np.nan)):
        given = F1.xy.copy()
        given[0] = bad
        m, prev, nm, _, cnt = _run(F1, F2, prev=given)
        assert m[0] == -1 and nm == 11 and cnt["not_finite"] == 1
        np.testing.assert_array_equal(prev[0], np.array(bad, F32))
    # an angle far outside [0, 360): the event counts, enters no bin and survives the rejection that
    # takes the lone event of bin 5
    F1 = _frame([(60, 60, 0, 1000.0, D), (SPOTS[20][0], SPOTS[20][1], 0, 150.0, RNG_D[20])] + f1)
    F2 = _frame([(60, 60, 0, 0.0, D), (SPOTS[20][0], SPOTS[20][1], 0, 0.0, RNG_D[20])] + f2)
    m, _, nm, hist, cnt = _run(F1, F2)
    assert cnt["bin_out_of_range"] == 1 and hist.sum() == 12 and hist[1] == 11 and hist[5] == 1
    assert cnt["rejected"] == 1 and m[0] == 0 and m[1] == -1 and nm == 12
    F1.ang[0] = np.nan
    assert _run(F1, F2)[2] == 12


# ---- ABI ----------------------------------------------------------------------------------------

def test_symbols_and_statuses_decided_before_any_launch():
    import orbslam3lib_amd as og
    names = {"orbgpu_search_for_initialization_batch", "orbgpu_download_initialization_matches"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "search_for_initialization") and hasattr(og.BatchExtractor, "initialization_matches")
    pairs = np.array([[0, 1]], np.int32)
    assert lib.orbgpu_search_for_initialization_batch(None, 1, pairs.ctypes.data_as(og.C.c_void_p), None, 0, 100,
                                                      og.C.c_float(0.9), 1, None) == -3
    assert lib.orbgpu_search_for_initialization_batch(None, 0, None, None, 0, 100, og.C.c_float(0.9), 1, None) == -3
    assert lib.orbgpu_download_initialization_matches(None, 0, None, None, 0, None, None, None) == -3
    # the wrapper refuses a prev_matched that does not give one row per pair before any device call
    be = object.__new__(og.BatchExtractor)
    with pytest.raises(ValueError):
        be.search_for_initialization([(0, 1), (0, 2)], prev_matched=[np.zeros((3, 2), np.float32)])
    with pytest.raises(ValueError):
        be.search_for_initialization([(0, 1)], prev_matched=np.zeros((1, 3, 3), np.float32))


# ---- scenes -------------------------------------------------------------------------------------

# name -> (F1 image, F2 image, prev, window, nnratio, check_orientation); images: L0 R0 L1 R1 of two
# stereo pairs, "rot": L0 turned by 180 degrees, "blank", "T0" / "TQ": one 48 x 48 texture repeated over
# the image, in TQ turned by 0 / 90 / 180 / 270 degrees in the four quadrants and with other noise
SCENES = {
    "left_right": ("L0", "R0", None, 100, 0.9, True),
    "no_orientation": ("L0", "R0", None, 100, 0.9, False),
    "self_window_20": ("L0", "L0", None, 20, 0.9, True),
    "unrelated_ratio_1": ("L0", "L1", None, 100, 1.0, True),
    "rotated_180": ("L0", "rot", "rotated", 100, 0.9, True),
    "collapsed": ("L0", "R0", "centre", 60, 0.9, True),
    # the repeating texture: every keypoint has near copies within the window, so owners are robbed,
    # filtered bests make way for seconds and lists of 4 run dry; four rotations spread the bins
    "tiled_quadrants": ("T0", "TQ", None, 100, 0.9, True),
    "tiled_collapsed": ("T0", "TQ", "centre", 100, 1.0, True),
}
SEED = 90


def _tiled(quadrants, noise_seed, tile=48, seed=1):
    t = synth.scene(tile, tile, seed)

    def plane(turns, h, w):
        return np.tile(np.rot90(t, turns), (h // tile + 1, w // tile + 1))[:h, :w]
    img = plane(0, 480, 640)
    if quadrants:
        img = np.block([[plane(0, 240, 320), plane(1, 240, 320)], [plane(2, 240, 320), plane(3, 240, 320)]])
    noisy = img + np.random.default_rng(noise_seed).normal(0.0, 2.0, img.shape)
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


def _images():
    (L0, R0), (L1, R1) = (synth.stereo_pair(480, 640, SEED + s) for s in range(2))
    return {"L0": L0, "R0": R0, "L1": L1, "R1": R1, "rot": np.ascontiguousarray(L0[::-1, ::-1]),
            "blank": np.full((480, 640), 128, np.uint8), "T0": _tiled(False, 5), "TQ": _tiled(True, 6)}


def _scene_prev(kind, F1):
    if kind is None:
        return None
    if kind == "centre":
        return np.tile(np.array([(320.0, 240.0)], F32), (len(F1.octv), 1))
    assert kind == "rotated"
    return (np.array([(639.0, 479.0)], F32) - F1.xy).astype(F32)


def _restate_scene(frames, name):
    f1, f2, kind, window, ratio, check = SCENES[name]
    return _py_init(frames[f1], frames[f2], _scene_prev(kind, frames[f1]), frames["bounds"], window, ratio, check)


@pytest.fixture(scope="module")
def cpu_frames(oracle):
    imgs = _images()
    frames = {}
    for k in ("L0", "R0", "L1", "rot", "T0", "TQ"):
        kps, desc, _ = oracle.extract(imgs[k], nfeatures=1000)
        xy, b, _, cs, ci = oracle.undistort_grid(kps, K_, D_, 640, 480)
        frames[k] = Fr(xy, kps["octave"].astype(np.int32), kps["angle"].astype(F32), desc.reshape(-1, 32), cs, ci)
        frames["bounds"] = b
    return frames


@pytest.fixture(scope="module")
def cpu_counters(cpu_frames):
    return {name: _restate_scene(cpu_frames, name) for name in SCENES}


def test_scenes_exercise_every_rule(cpu_counters):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the
    oracle's extraction, meets every situation the GPU cases are there to compare.  The stereo
    frames match one to one (their descriptors are unambiguous below TH_LOW); the conflicts come
    from the repeating texture."""
    cnts = {k: v[4] for k, v in cpu_counters.items()}
    for name, c in cnts.items():
        print(name, "nmatches", cpu_counters[name][2], dict(c))
    for name in ("left_right", "no_orientation", "self_window_20", "rotated_180", "tiled_quadrants"):
        assert cpu_counters[name][2] >= 50, name
    t = cnts["tiled_quadrants"]
    assert t["robbed"] >= 20 and t["promoted"] >= 20 and t["second_freed"] >= 1
    assert t["rejected_bin_max"] >= 5 and t["rejected"] >= 5 and t["rejected_already_robbed"] >= 1
    print("windows of more than %d candidates whose kept list runs dry (all, those that end in an event):" % KEPT,
          {k: (c["second_walk"], c["second_walk_event"]) for k, c in cnts.items()})
    assert t["second_walk"] >= 20 and t["second_walk_event"] >= 5
    assert cnts["collapsed"]["second_walk"] >= 20 and cnts["tiled_collapsed"]["second_walk"] >= 20
    for name, c in cnts.items():
        assert c["level_skipped"] >= 100, name
        assert c["filtered"] >= 1 or name == "unrelated_ratio_1", name
    assert cnts["unrelated_ratio_1"]["above_th_low"] == cnts["unrelated_ratio_1"]["searched"]
    assert cnts["self_window_20"]["lone"] >= 50 and cnts["left_right"]["ratio_failed"] + cnts["left_right"]["above_th_low"] >= 50
    hist = cpu_counters["rotated_180"][3]
    assert int(np.argmax(hist)) == 6 and hist[6] >= 50  # true matches away from bin 0
    assert (cpu_counters["tiled_quadrants"][3] >= 5).sum() >= 4  # four populated bins: one is rejected
    assert cpu_counters["no_orientation"][3].sum() == 0


# ---- GPU ----------------------------------------------------------------------------------------

def _gpu_frames(be, names):
    frames = {}
    for i, k in enumerate(names):
        kps, desc, _ = be.result(i)
        xy, _, cs, ci = be.grid_result(i)
        frames[k] = Fr(xy, kps["octave"].astype(np.int32), kps["angle"].astype(F32), desc.reshape(-1, 32), cs, ci)
    return frames


def _extractor(images):
    import orbslam3lib_amd as og
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=4)
    be.upload(np.stack(images))
    be.run()
    be.undistort_grid(K_, D_)
    be.synchronize()
    return be


@pytest.fixture(scope="module")
def gpu_env(oracle):
    """Two 640x480 stereo pairs at 1000 features (images L0 R0 L1 R1), extracted and gridded once."""
    imgs = _images()
    names = ["L0", "R0", "L1", "R1"]
    be = _extractor([imgs[k] for k in names])
    frames = _gpu_frames(be, names)
    frames["bounds"] = oracle.undistort_grid(be.result(0)[0], K_, D_, 640, 480)[1]
    yield be, frames, names
    be.close()


@pytest.fixture(scope="module")
def gpu_env2(oracle):
    """A second extractor: L0, L0 turned by 180 degrees, the two repeating textures."""
    imgs = _images()
    names = ["L0", "rot", "T0", "TQ"]
    be = _extractor([imgs[k] for k in names])
    frames = _gpu_frames(be, names)
    frames["bounds"] = oracle.undistort_grid(be.result(0)[0], K_, D_, 640, 480)[1]
    yield be, frames, names
    be.close()


def _gpu_compare(env, calls, one_call=True):
    """calls: (F1 name, F2 name, prev or None, window, ratio, check), one parameter set per call of
    the C entry point (the pairs of a call share window / ratio / check).  -> the restatement's
    results."""
    be, frames, names = env
    _, _, _, window, ratio, check = calls[0]
    pairs = [(names.index(f1), names.index(f2)) for f1, f2, *_ in calls]
    prevs = [c[2] for c in calls]
    given = None
    if any(p is not None for p in prevs):
        given = [frames[c[0]].xy if p is None else p for c, p in zip(calls, prevs)]
    be.search_for_initialization(pairs, given, window_size=window, nnratio=ratio, check_orientation=check)
    be.synchronize()
    out = []
    for p, (f1, f2, prev, *_rest) in enumerate(calls):
        m, pm, nm, hist, cnt = _py_init(frames[f1], frames[f2], prev, frames["bounds"], window, ratio, check)
        gm, gpm, gnm, ghist = be.initialization_matches(p)
        np.testing.assert_array_equal(gm, m, err_msg="pair %d vnMatches12" % p)
        assert gnm == nm, (p, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="pair %d histogram" % p)
        assert gpm.tobytes() == np.ascontiguousarray(pm, F32).tobytes(), "pair %d vbPrevMatched" % p
        out.append((m, pm, nm, hist, cnt))
    return out


def _call(frames, name):
    f1, f2, kind, window, ratio, check = SCENES[name]
    return (f1, f2, _scene_prev(kind, frames[f1]), window, ratio, check)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["left_right", "no_orientation", "self_window_20", "unrelated_ratio_1", "collapsed"])
def test_gpu_search_for_initialization_bit_exact(gpu_env, name):
    (m, _, nm, _, cnt), = _gpu_compare(gpu_env, [_call(gpu_env[1], name)])
    print(name, "nmatches", nm, dict(cnt))
    if name in ("left_right", "no_orientation", "self_window_20"):
        assert nm >= 50
    if name == "collapsed":
        assert cnt["second_walk"] >= 20 and cnt["filtered"] >= 100


@pytest.mark.gpu
def test_gpu_search_for_initialization_rotated_by_180(gpu_env2):
    (_, _, nm, hist, _), = _gpu_compare(gpu_env2, [_call(gpu_env2[1], "rotated_180")])
    assert nm >= 50 and int(np.argmax(hist)) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("name,nnratio", [("tiled_quadrants", 0.9), ("tiled_quadrants", 0.6), ("tiled_collapsed", 1.0),
                                          ("tiled_collapsed", 0.0)])
def test_gpu_search_for_initialization_repeating_texture(gpu_env2, name, nnratio):
    """Robbed owners, promoted seconds, rejected bins with robbed entries, kept lists that run dry."""
    f1, f2, prev, window, _, check = _call(gpu_env2[1], name)
    (_, _, nm, hist, cnt), = _gpu_compare(gpu_env2, [(f1, f2, prev, window, nnratio, check)])
    print(name, nnratio, "nmatches", nm, dict(cnt))
    if nnratio == 0.0:
        assert nm == 0 and cnt["ratio_failed"] >= 20
    else:
        assert cnt["robbed"] >= 10 and cnt["promoted"] >= 10 and cnt["second_walk"] >= 5 and cnt["rejected"] >= 5
    if name == "tiled_quadrants" and nnratio == 0.9:
        assert cnt["robbed"] >= 20 and cnt["promoted"] >= 20 and cnt["second_walk"] >= 20
        assert cnt["rejected_bin_max"] >= 5 and cnt["rejected_already_robbed"] >= 1


@pytest.mark.gpu
def test_gpu_search_for_initialization_chained(gpu_env):
    """The returned vbPrevMatched fed back with a narrower window, as MonocularInitialization does
    from frame to frame."""
    frames = gpu_env[1]
    (_, pm, nm, _, _), = _gpu_compare(gpu_env, [("L0", "R0", None, 100, 0.9, True)])
    assert nm >= 50 and (pm != frames["L0"].xy).any()
    (_, _, nm2, _, _), = _gpu_compare(gpu_env, [("L0", "R0", pm, 30, 0.9, True)])
    assert nm2 >= 50


@pytest.mark.gpu
def test_gpu_search_for_initialization_one_f1_in_two_pairs(gpu_env):
    frames = gpu_env[1]
    res = _gpu_compare(gpu_env, [("L0", "R0", None, 100, 0.9, True), ("L0", "L1", None, 100, 0.9, True),
                                 ("L1", "R0", None, 100, 0.9, True)])
    assert res[0][2] >= 50 and res[0][2] != res[1][2]
    # the same with vbPrevMatched given for one of them (rows of different lengths)
    jitter = (frames["L0"].xy + F32(3.0)).astype(F32)
    _gpu_compare(gpu_env, [("L0", "R0", jitter, 100, 0.9, True), ("L1", "R1", None, 100, 0.9, True)])


@pytest.mark.gpu
@pytest.mark.parametrize("nsearch", [63, 64, 65, 129])
def test_gpu_search_for_initialization_replay_group_boundary(gpu_env2, nsearch):
    """Exactly nsearch searched keypoints (the rest of the octave-0 ones marked not finite): the
    replay takes 64 at a time.  On the repeating texture, so that the points of a group conflict."""
    F1 = gpu_env2[1]["T0"]
    zero = np.flatnonzero(F1.octv == 0)
    assert len(zero) > nsearch
    prev = F1.xy.copy()
    prev[zero[nsearch:]] = np.nan
    (_, _, _, _, cnt), = _gpu_compare(gpu_env2, [("T0", "TQ", prev, 100, 0.9, True)])
    assert cnt["searched"] == nsearch and cnt["not_finite"] == len(zero) - nsearch
    assert cnt["robbed"] >= 3 and cnt["filtered"] >= 50


@pytest.mark.gpu
def test_gpu_search_for_initialization_blank_images_and_no_pairs(oracle):
    import orbslam3lib_amd as og
    imgs = _images()
    names = ["blank", "L0"]
    be = _extractor([imgs[k] for k in names])
    frames = _gpu_frames(be, names)
    frames["bounds"] = oracle.undistort_grid(be.result(1)[0], K_, D_, 640, 480)[1]
    assert len(frames["blank"].octv) == 0
    res = _gpu_compare((be, frames, names), [("blank", "L0", None, 100, 0.9, True), ("L0", "blank", None, 100, 0.9, True),
                                             ("blank", "blank", None, 100, 0.9, True)])
    assert [r[2] for r in res] == [0, 0, 0] and len(res[0][0]) == 0 and (res[1][0] == -1).all()
    be.search_for_initialization(np.zeros((0, 2), np.int32))  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.initialization_matches(0)
    assert e.value.code == -3
    be.close()


@pytest.mark.gpu
def test_gpu_search_for_initialization_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.search_for_initialization(*a, **k)
        return e.value.code
    assert code([(0, 1)]) == -3  # before undistort_grid
    be.undistort_grid(K_, D_)
    assert code([(0, 2)]) == -3 and code([(-1, 0)]) == -3  # outside the gridded range
    assert code([(0, 1)], window_size=-1) == -3
    assert code([(0, 1)] * 3) == -3  # above the context's image capacity
    n1 = len(be.result(0)[0])
    assert code([(0, 1)], prev_matched=np.zeros((1, n1 - 1, 2), np.float32)) == -3  # pm_stride below N1
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.initialization_matches(0)
    assert e.value.code == -3
    be.search_for_initialization([(0, 1)], prev_matched=np.zeros((1, n1, 2), np.float32) + F32(100.0))
    m, pm, nm, hist = be.initialization_matches(0)
    assert len(m) == n1 and pm.shape == (n1, 2) and nm == int((m >= 0).sum())
    with pytest.raises(og.OrbGpuError) as e:
        be.initialization_matches(1)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # caller capacity below N1
        be.initialization_matches(0, cap=n1 - 1)
    assert e.value.code == -2
    be.close()
