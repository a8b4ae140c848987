"""ORBmatcher::SearchByProjection(KeyFrame* pKF, Sophus::Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming)
(cpp/src/ORBmatcher.cc:428-533) and the overload that also carries vpPointsKFs / vpMatchedKF (:535-647) --
the searches LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:755, :777) and FindMatchesByProjection
(:964) run -- with KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:706-755) and MapPoint::PredictScale
(MapPoint.cc:504-531), on pinhole keyframes.

The yardstick is _py_sim3_search below: a restatement written from those lines with np.float32 scalars
(every product and sum rounds to single, in the reference's order; both projection forms; the comparisons
against double literals in double; the limit TH_LOW * ratioHamming as a float product compared in float),
the host libm's logf for the level.  It returns, per keypoint, the point this call put on it, per point the
decision code, the keypoint and its distance, nmatches, and a Counter of what the scene exercised: each
code, the candidates passed over for occupancy (held before the call / taken in it) and for their octave,
each level, the clamps, and per matched point the rank it took among its pre-call free, in-band,
within-limit candidates ordered by (distance, window position).
CPU: a second, independent form (_brute_sim3: array arithmetic for the gates, the level from
orbgpu_predict_scale_table, per point a scan of every gridded keypoint with the box test and the live
occupancy) against the restatement on every scene; hand-built known answers on a tiny frame; a seeded search
for a point the two projections decide differently; conditions on the scenes the GPU cases use; the dtypes,
symbols and statuses.
GPU: k_sim3_candidates + k_sim3_resolve against the restatement, equal on every output.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs Sophus, Eigen and the SLAM stack;
no fixtures ship for it) -- restatement only, as for the other matcher functions."""
import math
from collections import Counter

import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_fuse import _aim, _octaves_frame, _on_axis
from tests.test_reloc_projection import _Tiny, _bits, _predict_scale, _reloc_pose
from tests.test_track_projection import D_, F32, K_, POP, _flip, _header_struct_bytes, _window

SKIPPED, NEG_DEPTH, NOT_IN_IMAGE, DISTANCE, NORMAL, EMPTY_WINDOW, NOT_MATCHED, MATCHED = range(1, 9)
CODES = {SKIPPED: "skipped", NEG_DEPTH: "neg_depth", NOT_IN_IMAGE: "not_in_image", DISTANCE: "distance",
         NORMAL: "normal", EMPTY_WINDOW: "empty_window", NOT_MATCHED: "not_matched", MATCHED: "matched"}
DIV, INVZ = 0, 1
TH_LOW = 50
KEPT = 4  # candidates k_sim3_candidates keeps per point: a match of rank >= KEPT needs the fresh walk


def _project(proj, fx, fy, cx, cy, xc, yc, zc):
    with np.errstate(all="ignore"):
        if proj == DIV:  # Pinhole.cpp:40-41
            return fx * xc / zc + cx, fy * yc / zc + cy
        invz = F32(1) / zc  # :574-579
        x = xc * invz
        y = yc * invz
        return fx * x + cx, fy * y + cy


def _py_sim3_search(pts, pose, K, xy, octv, desc, bounds, cs, ci, skip, blk, th, ratio_hamming, proj, scale,
                    scale_factor=1.2, nlevels=8):
    """-> match [n_kp], best_idx [n_points], best_dist [n_points], code [n_points], nmatches, Counter.
    skip: the pair's row or None; blk: vpMatched before the call (non-zero = set) or None."""
    npts, nkp = len(pts), len(octv)
    xy = np.asarray(xy, F32)
    held = np.zeros(nkp, bool) if blk is None else (np.asarray(blk)[:nkp] != 0)
    held0 = held.copy()
    match = np.full(nkp, -1, np.int32)
    best_idx = np.full(npts, -1, np.int32)
    best_dist = np.full(npts, 256, np.int32)
    code = np.zeros(npts, np.uint8)
    cnt = Counter()
    b = np.asarray(bounds, F32)
    R, t, Ow = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Ow"))
    fx, fy, cx, cy = (F32(v) for v in K)
    limit = F32(TH_LOW) * F32(ratio_hamming)  # :524: int * float, a float
    pts = np.atleast_1d(pts)
    P, N = np.asarray(pts["pos"], F32), np.asarray(pts["normal"], F32)
    MN, MX = np.asarray(pts["min_distance"], F32), np.asarray(pts["max_distance"], F32)
    FL, DS = np.asarray(pts["flags"]), np.asarray(pts["desc"])
    nm = 0
    for i in range(npts):
        if not (int(FL[i]) & 1) or (skip is not None and skip[i]):  # :452 / :560
            code[i] = SKIPPED
            cnt["skip_byte"] += bool(int(FL[i]) & 1)
            continue
        X, Y, Z = P[i]
        with np.errstate(all="ignore"):
            xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]  # :459
            yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
            zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        if zc < 0.0:  # :462 / :570
            code[i] = NEG_DEPTH
            continue
        u, v = _project(proj, fx, fy, cx, cy, xc, yc, zc)
        if not (u >= b[0] and u < b[1] and v >= b[2] and v < b[3]):  # KeyFrame.cc:752-755
            code[i] = NOT_IN_IMAGE
            continue
        with np.errstate(all="ignore"):
            px, py, pz = X - Ow[0], Y - Ow[1], Z - Ow[2]  # :475
            dist = np.sqrt((px * px + py * py) + pz * pz)
            lo, hi = F32(0.8) * MN[i], F32(1.2) * MX[i]  # MapPoint.cc:504-514
            ratio = MX[i] / dist  # MapPoint.cc:521
        if not np.isfinite(dist) or dist < lo or dist > hi or not np.isfinite(ratio):  # :478 + the deviation
            code[i] = DISTANCE
            continue
        with np.errstate(all="ignore"):
            dot = (px * N[i, 0] + py * N[i, 1]) + pz * N[i, 2]
        if float(dot) < 0.5 * float(dist):  # :484 / :597, in double
            code[i] = NORMAL
            continue
        level, raw = _predict_scale(ratio, scale_factor, nlevels)  # :487
        cnt["level_%d" % level] += 1
        cnt["clamped_low"] += raw < 0
        cnt["clamped_high"] += raw >= nlevels
        radius = F32(th) * F32(scale[level])  # :490
        cand = _window(xy, octv, cs, ci, b, u, v, radius, -1, -1)  # KeyFrame::GetFeaturesInArea: no level filter
        if not cand:  # :494
            code[i] = EMPTY_WINDOW
            continue
        best, bi, bpos = 256, -1, -1
        free = []  # instrumentation: (distance, window position) of the pre-call free, in-band, within-limit ones
        for pos, k in enumerate(cand):
            inband = level - 1 <= int(octv[k]) <= level
            if held[k]:  # :505 / :618
                cnt["held" if held0[k] else "taken"] += 1
                cnt["taken_across_64"] += bool((not held0[k]) and match[k] < 64 <= i)
                if not held0[k] and inband:
                    d = int(POP[np.bitwise_xor(DS[i], desc[k])].sum())
                    if F32(d) <= limit:
                        free.append((d, pos))
                continue
            if not inband:  # :510
                cnt["octave"] += 1
                continue
            d = int(POP[np.bitwise_xor(DS[i], desc[k])].sum())
            if F32(d) <= limit:
                free.append((d, pos))
            if d < best:  # :517
                best, bi, bpos = d, k, pos
        if F32(best) <= limit:  # :524
            assert match[bi] < 0 and not held[bi]
            match[bi] = i  # :526
            held[bi] = True
            nm += 1
            code[i], best_idx[i], best_dist[i] = MATCHED, bi, best
            rank = sorted(free).index((best, bpos))
            cnt["rank_%d" % min(rank, 9)] += 1
            cnt["not_first"] += rank > 0
            cnt["beyond_kept"] += rank >= KEPT
        else:
            code[i] = NOT_MATCHED
            cnt["not_matched_all_passed_over"] += bi < 0
    cnt["occupied"] = cnt["held"] + cnt["taken"]
    for c, name in CODES.items():
        cnt[name] = int((code == c).sum())
    return match, best_idx, best_dist, code, nm, cnt


def _brute_sim3(pts, pose, K, xy, octv, desc, bounds, ci, skip, blk, th, ratio_hamming, proj, scale, steps):
    """The second form: array arithmetic over all points for rules 1 to 6, the level as the number of
    orbgpu_predict_scale_table entries below the ratio, then per point, in order, a scan of every gridded
    keypoint (cell_idx is in window order for any window: grid column, row, index within the cell) with the
    box test and the live occupancy -> match, best_idx, best_dist, code, nmatches."""
    n, nkp = len(pts), len(octv)
    xy = np.asarray(xy, F32)
    b = np.asarray(bounds, F32)
    R, t, Ow = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Ow"))
    fx, fy, cx, cy = (F32(v) for v in K)
    P = np.asarray(pts["pos"], F32)
    N = np.asarray(pts["normal"], F32)
    kk = np.asarray(ci)
    octk = np.asarray(octv)[kk]
    code = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        cam = [((R[3 * r] * P[:, 0] + R[3 * r + 1] * P[:, 1]) + R[3 * r + 2] * P[:, 2]) + t[r] for r in range(3)]
        if proj == DIV:
            u = fx * cam[0] / cam[2] + cx
            v = fy * cam[1] / cam[2] + cy
        else:
            invz = F32(1) / cam[2]
            u = fx * (cam[0] * invz) + cx
            v = fy * (cam[1] * invz) + cy
        PO = P - Ow[None, :]
        dist = np.sqrt((PO[:, 0] * PO[:, 0] + PO[:, 1] * PO[:, 1]) + PO[:, 2] * PO[:, 2])
        ratio = np.asarray(pts["max_distance"], F32) / dist
        dot = (PO[:, 0] * N[:, 0] + PO[:, 1] * N[:, 1]) + PO[:, 2] * N[:, 2]
        inside = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        in_range = np.isfinite(dist) & np.isfinite(ratio) & ~(dist < F32(0.8) * np.asarray(pts["min_distance"], F32)) \
            & ~(dist > F32(1.2) * np.asarray(pts["max_distance"], F32))
        facing = ~(dot.astype(np.float64) < 0.5 * dist.astype(np.float64))
    level = np.searchsorted(np.asarray(steps, F32), ratio, side="left")
    skipped = (np.asarray(pts["flags"]) & 1) == 0
    if skip is not None:
        skipped |= np.asarray(skip)[:n] != 0
    for mask, c in [(skipped, SKIPPED), (cam[2] < 0, NEG_DEPTH), (~inside, NOT_IN_IMAGE), (~in_range, DISTANCE), (~facing, NORMAL)]:
        code[(code == 0) & mask] = c
    occupied = np.zeros(nkp, bool) if blk is None else (np.asarray(blk)[:nkp] != 0).copy()
    match = np.full(nkp, -1, np.int32)
    best_dist = np.full(n, 256, np.int32)
    best_idx = np.full(n, -1, np.int32)
    limit = np.float32(TH_LOW) * np.float32(ratio_hamming)
    for i in np.flatnonzero(code == 0):
        r = F32(th) * F32(scale[level[i]])
        with np.errstate(all="ignore"):
            box = (np.abs(xy[kk, 0] - u[i]) < r) & (np.abs(xy[kk, 1] - v[i]) < r)
        if not box.any():
            code[i] = EMPTY_WINDOW
            continue
        code[i] = NOT_MATCHED
        k = kk[box & ~occupied[kk] & (octk >= level[i] - 1) & (octk <= level[i])]
        if len(k):
            d = POP[np.bitwise_xor(desc[k], pts["desc"][i][None, :])].sum(1)
            j = int(np.argmin(d))  # the first lowest
            if np.float32(d[j]) <= limit:
                code[i], best_idx[i], best_dist[i] = MATCHED, k[j], d[j]
                match[k[j]] = i
                occupied[k[j]] = True
    return match, best_idx, best_dist, code, int((code == MATCHED).sum())


# ---- hand-built frames --------------------------------------------------------------------------

SC = (F32(1.2) ** np.arange(8)).astype(F32)  # stands for mvScaleFactors in the hand-built cases


def _run(T, pts, th=10.0, ratio=1.5, proj=DIV, skip=None, blk=None, pose=None):
    return _py_sim3_search(np.atleast_1d(pts), _reloc_pose() if pose is None else pose, T.K, T.xy, T.octv, T.desc, T.B,
                           T.cs, T.ci, skip, blk, th, ratio, proj, SC)


def _both(T, pts, **kw):
    """The restatement under both projections, which must agree (the cases are exact under either)."""
    a, c = _run(T, pts, proj=DIV, **kw), _run(T, pts, proj=INVZ, **kw)
    for x, y in zip(a[:4], c[:4]):
        np.testing.assert_array_equal(x, y)
    assert a[4] == c[4]
    return a


def _near(extra_bits, seed=2):
    """The tiny frame with one more keypoint 8 px right of keypoint 0, `extra_bits` bits from it."""
    base = _Tiny()
    return _Tiny(extra=[(-252.0, -180.0, 0, _flip(base.desc[0], extra_bits, seed))])


def test_an_earlier_point_takes_the_keypoint_a_later_closer_one_would_have_won():
    T = _near(40)
    A = _aim(-260, -180, _flip(T.desc[0], 10))
    B = _aim(-260, -180, T.desc[0])
    m, bi, bd, code, nm, cnt = _both(T, np.array([A, B]))
    assert list(code) == [MATCHED, MATCHED] and list(bi) == [0, 40] and list(bd) == [10, 40] and nm == 2
    assert m[0] == 0 and m[40] == 1 and (np.delete(m, [0, 40]) == -1).all()
    assert cnt["taken"] == 1 and cnt["held"] == 0 and cnt["rank_0"] == 1 and cnt["rank_1"] == 1 and cnt["not_first"] == 1
    # the other order: the closer one comes first and wins, the farther one is left with the neighbour
    m, bi, bd, code, nm, _ = _both(T, np.array([B, A]))
    assert list(bi) == [0, 40] and bd[0] == 0 and nm == 2 and m[0] == 0 and m[40] == 1


def test_the_later_point_is_not_matched_when_its_next_best_is_above_the_limit():
    T = _near(80)
    A = _aim(-260, -180, _flip(T.desc[0], 10))
    B = _aim(-260, -180, T.desc[0])
    m, bi, bd, code, nm, cnt = _both(T, np.array([A, B]))
    assert list(code) == [MATCHED, NOT_MATCHED] and list(bi) == [0, -1] and list(bd) == [10, 256] and nm == 1
    assert m[0] == 0 and m[40] == -1 and cnt["taken"] == 1 and cnt["not_matched_all_passed_over"] == 0
    # alone, the later point would have had the keypoint
    assert _both(T, B)[1][0] == 0


def test_a_chain_three_deep():
    base = _Tiny()
    d0 = base.desc[0]
    T = _Tiny(extra=[(-252.0, -180.0, 0, _flip(d0, 20, 2)), (-255.0, -172.0, 0, _flip(d0, 40, 3))])
    pts = np.array([_aim(-260, -180, d0)] * 4)
    m, bi, bd, code, nm, cnt = _both(T, pts)
    assert list(bi) == [0, 40, 41, -1] and list(bd) == [0, 20, 40, 256] and nm == 3
    assert list(code) == [MATCHED, MATCHED, MATCHED, NOT_MATCHED] and [m[0], m[40], m[41]] == [0, 1, 2]
    assert cnt["taken"] == 1 + 2 + 3 and [cnt["rank_%d" % r] for r in range(3)] == [1, 1, 1]
    assert cnt["not_matched_all_passed_over"] == 1  # the fourth finds every keypoint of its window taken


def test_an_unmatched_point_takes_nothing():
    T = _Tiny()
    far = _aim(-260, -180, _flip(T.desc[0], 100))
    m, bi, bd, code, nm, cnt = _both(T, np.array([far, _aim(-260, -180, T.desc[0])]))
    assert list(code) == [NOT_MATCHED, MATCHED] and list(bi) == [-1, 0] and list(bd) == [256, 0]
    assert m[0] == 1 and nm == 1 and cnt["taken"] == 0


def test_a_pre_held_keypoint_is_passed_over_and_receives_no_match():
    T = _near(40)
    blk = np.zeros(41, np.uint8)
    blk[0] = 7  # any non-zero value
    m, bi, bd, code, nm, cnt = _both(T, _aim(-260, -180, T.desc[0]), blk=blk)
    assert code[0] == MATCHED and bi[0] == 40 and bd[0] == 40 and m[0] == -1 and m[40] == 0 and nm == 1
    assert cnt["held"] == 1 and cnt["taken"] == 0 and cnt["rank_0"] == 1  # the held one was never a candidate


def test_a_window_whose_only_keypoints_are_held_is_not_matched_and_a_bare_one_is_empty():
    T = _near(40)
    blk = np.zeros(41, np.uint8)
    blk[[0, 40]] = 1
    m, bi, bd, code, nm, cnt = _both(T, _aim(-260, -180, T.desc[0]), blk=blk)
    assert code[0] == NOT_MATCHED and bi[0] == -1 and bd[0] == 256 and nm == 0 and (m == -1).all()
    assert cnt["held"] == 2 and cnt["not_matched_all_passed_over"] == 1
    # and taken in the call rather than held before it: the same
    pts = np.array([_aim(-260, -180, T.desc[0]), _aim(-260, -180, T.desc[40]), _aim(-260, -180, T.desc[0])])
    assert list(_both(T, pts)[3]) == [MATCHED, MATCHED, NOT_MATCHED]
    # no keypoint within the radius at all: 35 px from the nearest four
    assert _both(T, _aim(-225, -145, T.desc[0]))[3][0] == EMPTY_WINDOW


def test_the_octave_band_is_level_minus_one_to_level_and_the_clamps():
    T = _octaves_frame()

    def sees(ratio):
        out = []
        for target in range(8):
            p = _on_axis(2.0, T.desc[target], mn=0.0, mx=F32(2.0) * F32(ratio))
            m, bi, bd, code, nm, cnt = _both(T, p, th=3.0)
            assert code[0] in (MATCHED, NOT_MATCHED)  # never EMPTY_WINDOW: the area holds all eight
            if code[0] == MATCHED:
                assert bi[0] == target and bd[0] == 0 and m[target] == 0
                out.append(target)
        return out, [k for k in cnt if k.startswith("level_")][0], cnt["clamped_low"], cnt["clamped_high"]
    assert sees(0.95) == ([0], "level_0", 0, 0)  # level 0: octaves -1 .. 0
    assert sees(1.0) == ([0], "level_0", 0, 0)
    assert sees(1.01) == ([0, 1], "level_1", 0, 0)
    assert sees(1.2 ** 2.5) == ([2, 3], "level_3", 0, 0)  # octave level + 1 = 4 is filtered, level - 1 = 2 taken
    assert sees(1.2 ** 6.5) == ([6, 7], "level_7", 0, 0)
    assert sees(1.2 ** 8.5) == ([6, 7], "level_7", 0, 1)  # nScale = 9, clamped from above
    assert sees(0.84)[:3] == ([0], "level_0", 0)           # ceil(-0.96) = 0: no clamp yet
    # the clamp from below needs a ratio under 1 / 1.2, which only a point beyond 1.2 max_distance has: the gate
    p = _on_axis(2.0, T.desc[0], mn=0.0, mx=F32(2.0) * F32(0.8))
    assert _both(T, p, th=3.0)[3][0] == DISTANCE and _predict_scale(F32(0.8), 1.2, 8) == (0, -1)
    # every candidate filtered: not matched with nothing surviving, not an empty window
    p = _on_axis(2.0, T.desc[5], mn=0.0, mx=F32(2.0) * F32(1.2 ** 2.5))
    m, bi, bd, code, nm, cnt = _both(T, p, th=3.0)
    assert code[0] == NOT_MATCHED and bd[0] == 256 and cnt["octave"] == 6 and cnt["not_matched_all_passed_over"] == 0


@pytest.mark.parametrize("ratio,nbits,want", [(1.5, 75, MATCHED), (1.5, 76, NOT_MATCHED), (1.0, 50, MATCHED),
                                              (1.0, 51, NOT_MATCHED), (1.51, 75, MATCHED), (1.51, 76, NOT_MATCHED)])
def test_the_limit_is_the_float_product_of_th_low_and_the_ratio(ratio, nbits, want):
    """50 * 1.51f = 75.5 as a float: 75 is within it and 76 is not."""
    T = _Tiny(extra=[(0.0, 0.0, 0, _bits((0, nbits)))])
    m, bi, bd, code, nm, _ = _both(T, _aim(0, 0, _bits()), ratio=ratio)
    assert code[0] == want and nm == (want == MATCHED) and bi[0] == (40 if want == MATCHED else -1)
    assert bd[0] == (nbits if want == MATCHED else 256) and m[40] == (0 if want == MATCHED else -1)


def test_an_equal_distance_keeps_the_earlier_window_position():
    Z = _bits()
    # window order: grid column, then row, then index: the keypoint further left comes first whatever its index
    T = _Tiny(extra=[(6.0, 0.0, 0, _bits((0, 7))), (-6.0, 0.0, 0, _bits((7, 14)))])
    m, bi, bd, code, _, _ = _both(T, np.array([_aim(0, 0, Z)] * 2), th=8.0)
    assert list(code) == [MATCHED, MATCHED] and list(bi) == [41, 40] and list(bd) == [7, 7]
    # in one cell the lower index comes first
    T = _Tiny(extra=[(1.0, 0.0, 0, _bits((0, 7))), (0.5, 0.0, 0, _bits((7, 14)))])
    assert list(_both(T, np.array([_aim(0, 0, Z)] * 2), th=3.0)[1]) == [40, 41]


@pytest.mark.parametrize("axis,bound,inside", [(0, -320.0, 1), (0, 320.0, -1), (1, -240.0, 1), (1, 240.0, -1)])
def test_the_image_test_is_half_open(axis, bound, inside):
    """At mnMin and one float above passes, one float below fails; one float below mnMax passes, at mnMax and one
    float above fails.  zc = 1: u = 512 x
    under either projection.  The last grid cell ends 5 px inside mnMax, so the keypoint sits 8 px inside."""
    kp = [0.0, 0.0]
    kp[axis] = bound + 8 * inside
    T = _Tiny(extra=[(kp[0], kp[1], 0, None)])
    if inside > 0:
        cases = ((F32(bound), MATCHED), (np.nextafter(F32(bound), F32(-1e9)), NOT_IN_IMAGE),
                 (np.nextafter(F32(bound), F32(0)), MATCHED))
    else:
        cases = ((np.nextafter(F32(bound), F32(0)), MATCHED), (F32(bound), NOT_IN_IMAGE),
                 (np.nextafter(F32(bound), F32(1e9)), NOT_IN_IMAGE))
    for target, want in cases:
        xyz = [0.0, 0.0, 1.0]
        xyz[axis] = target / F32(512)
        p = _on_axis(1.0, T.desc[40], x=xyz[0], y=xyz[1])
        p["normal"] = p["pos"] / np.linalg.norm(p["pos"])
        assert F32(512) * p["pos"][axis] / F32(1) + F32(0) == target
        m, bi, bd, code, nm, _ = _both(T, p)
        assert code[0] == want and nm == (want == MATCHED) and bi[0] == (40 if want == MATCHED else -1)
        assert bd[0] == (0 if want == MATCHED else 256) and m[40] == (0 if want == MATCHED else -1)


def test_each_invariance_limit_at_the_limit_passes_and_one_float_beyond_is_distance():
    """On the optical axis under the identity pose dist = sqrtf(z * z) = z exactly."""
    T = _Tiny(extra=[(1.0, 0.0, 0, None)])
    mx = F32(3.3)
    far = F32(1.2) * mx
    assert _both(T, _on_axis(far, T.desc[40], mx=mx))[3][0] == MATCHED
    assert _both(T, _on_axis(np.nextafter(far, F32(1e9)), T.desc[40], mx=mx))[3][0] == DISTANCE
    mn = F32(2.7)
    near = F32(0.8) * mn
    assert _both(T, _on_axis(near, T.desc[40], mn=mn, mx=near))[3][0] == MATCHED
    out = _both(T, _on_axis(np.nextafter(near, F32(0)), T.desc[40], mn=mn, mx=near))
    assert out[3][0] == DISTANCE and out[2][0] == 256 and out[1][0] == -1


def test_the_normal_test_at_equality_passes_and_one_float_less_is_normal():
    """PO = (0, 0, 2), n = (0, 0, nz): the dot product 2 nz is exact; 0.5 * dist = 1."""
    T = _Tiny(extra=[(1.0, 0.0, 0, None)])
    assert _both(T, _on_axis(2.0, T.desc[40], normal=(0, 0, 0.5)))[3][0] == MATCHED
    assert _both(T, _on_axis(2.0, T.desc[40], normal=(0, 0, np.nextafter(F32(0.5), F32(0)))))[3][0] == NORMAL
    assert _both(T, _on_axis(2.0, T.desc[40], normal=(0, 0, -1.0)))[3][0] == NORMAL
    assert _both(T, _on_axis(2.0, T.desc[40], normal=(0, 0, np.nan)))[3][0] == MATCHED  # a NaN fails no comparison


def test_depth_one_float_below_zero_is_neg_depth_and_zero_is_not_in_image():
    """zc = Z + tcw.z with tcw.z = 1: Z = -1 gives 0, the float below -1 a negative zc."""
    T = _Tiny()
    pose = _reloc_pose(t=(0.0, 0.0, 1.0))
    d = T.desc[0]
    assert _both(T, _on_axis(np.nextafter(F32(-1), F32(-2)), d), pose=pose)[3][0] == NEG_DEPTH
    assert _both(T, _on_axis(-1.0, d), pose=pose)[3][0] == NOT_IN_IMAGE          # 0 / 0, 0 * inf
    assert _both(T, _on_axis(-1.0, d, x=0.25), pose=pose)[3][0] == NOT_IN_IMAGE  # x / 0 = inf
    assert _both(T, _on_axis(-0.0, d, x=0.25))[3][0] == NOT_IN_IMAGE             # zc = -0.0 is not < 0
    assert _both(T, _on_axis(-2.0, d))[3][0] == NEG_DEPTH


def test_not_finite_positions():
    T = _Tiny()
    d = T.desc[0]
    nan = _aim(-260, -180, d)
    nan["pos"][0] = np.nan
    assert _both(T, nan)[3][0] == NOT_IN_IMAGE
    nanz = _aim(-260, -180, d)
    nanz["pos"][2] = np.nan  # zc < 0 is false for a NaN
    assert _both(T, nanz)[3][0] == NOT_IN_IMAGE
    huge = _aim(0, 0, d)
    huge["pos"] = (0, 0, 1e30)  # projects to the centre; dist overflows
    huge["max_distance"] = np.inf
    assert _both(T, huge)[3][0] == DISTANCE
    inf = _aim(-260, -180, d)
    inf["max_distance"] = np.inf  # passes the gate, the ratio is not finite
    out = _both(T, inf)
    assert out[3][0] == DISTANCE and out[1][0] == -1 and out[2][0] == 256 and out[4] == 0 and (out[0] == -1).all()


def test_a_skip_byte_does_what_the_flag_does():
    T = _Tiny()
    pts = np.array([_aim(-260, -180, T.desc[0]), _aim(-260, -180, T.desc[0]), _aim(-260, -180, T.desc[0], valid=False)])
    m, bi, bd, code, nm, cnt = _both(T, pts, skip=np.array([9, 0, 0], np.uint8))
    assert list(code) == [SKIPPED, MATCHED, SKIPPED] and list(bi) == [-1, 0, -1] and m[0] == 1 and nm == 1
    assert cnt["skip_byte"] == 1
    assert _both(T, pts)[0][0] == 0  # without it the first point has the keypoint


def test_the_two_projections_decide_a_point_differently():
    """fx * xc / zc + cx rounds twice, fx * (xc * (1 / zc)) + cx three times.  A seeded search over depths and
    the floats next to x = 320 z / 512 finds a point one form puts at mnMaxX = 320 (outside: the test is
    half-open) and the other one float below it (inside, where a keypoint 8 px in waits), and one a window
    edge decides: |u - x_k| < radius under one form and not under the other."""
    rng = np.random.default_rng(11)
    fx = F32(512)
    T = _Tiny(extra=[(312.0, 0.0, 0, None)])
    edge = image = None
    radius = F32(10)  # th 10 at level 0
    for _ in range(4000):
        z = F32(rng.uniform(1.0, 4.0))
        for target, kind in ((F32(320), "image"), (F32(322), "edge")):
            x = F32(target) * z / fx
            for _ in range(4):
                x = np.nextafter(x, F32(0))
                ud, ui = (_project(f, fx, fx, F32(0), F32(0), x, F32(0), z)[0] for f in (DIV, INVZ))
                if ud == ui:
                    continue
                if kind == "image" and image is None and min(ud, ui) < F32(320) <= max(ud, ui):
                    image = (x, z, ud, ui)
                # a keypoint at 312 and radius 10: the window's open edge is at u = 322
                if kind == "edge" and edge is None and (abs(F32(312) - ud) < radius) != (abs(F32(312) - ui) < radius):
                    edge = (x, z, ud, ui)
        if image and edge:
            break
    assert image is not None and edge is not None, "no straddling point within the budget"
    x, z, ud, ui = image
    p = _on_axis(float(z), T.desc[40], x=float(x))
    p["normal"] = p["pos"] / np.linalg.norm(p["pos"])
    want = {f: (MATCHED if u < F32(320) else NOT_IN_IMAGE) for f, u in ((DIV, ud), (INVZ, ui))}
    assert set(want.values()) == {MATCHED, NOT_IN_IMAGE}
    for f in (DIV, INVZ):
        m, bi, bd, code, nm, _ = _run(T, p, proj=f)
        assert code[0] == want[f] and m[40] == (0 if want[f] == MATCHED else -1) and nm == (want[f] == MATCHED)
    # the window edge, on a frame whose bounds reach further so that both projections are inside the image
    W = _Tiny(extra=[(312.0, 0.0, 0, None)])
    W.B = np.array([-400, 400, -240, 240], F32)
    from tests.test_track_projection import _grid
    W.cs, W.ci = _grid(W.xy, W.B)
    x, z, ud, ui = edge
    p = _on_axis(float(z), W.desc[40], x=float(x))
    p["normal"] = p["pos"] / np.linalg.norm(p["pos"])
    want = {f: (MATCHED if abs(F32(312) - u) < radius else EMPTY_WINDOW) for f, u in ((DIV, ud), (INVZ, ui))}
    assert set(want.values()) == {MATCHED, EMPTY_WINDOW}
    for f in (DIV, INVZ):
        m, bi, bd, code, nm, _ = _run(W, p, proj=f)
        assert code[0] == want[f] and bi[0] == (40 if want[f] == MATCHED else -1)


# ---- wrapper and ABI ----------------------------------------------------------------------------

def test_dtypes_match_the_header_structs_and_the_symbols_are_exported():
    import orbslam3lib_amd as og
    assert og.FUSE_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_fuse_point") == 68
    assert og.RELOC_POSE_DTYPE.itemsize == _header_struct_bytes("orbgpu_reloc_pose") == 60
    txt = open(og.os.path.join(og.os.path.dirname(og.HERE), "include", "orbgpu.h")).read()
    for name, value in (("SKIPPED", SKIPPED), ("NEG_DEPTH", NEG_DEPTH), ("NOT_IN_IMAGE", NOT_IN_IMAGE), ("DISTANCE", DISTANCE),
                        ("NORMAL", NORMAL), ("EMPTY_WINDOW", EMPTY_WINDOW), ("NOT_MATCHED", NOT_MATCHED), ("MATCHED", MATCHED)):
        assert "#define ORBGPU_SIM3_%s %d\n" % (name, value) in txt
        assert getattr(og, "SIM3_" + name) == value
    assert "#define ORBGPU_SIM3_PROJECT_DIV 0 " in txt and "#define ORBGPU_SIM3_PROJECT_INVZ 1 " in txt
    assert (og.SIM3_PROJECT_DIV, og.SIM3_PROJECT_INVZ) == (DIV, INVZ)
    names = {"orbgpu_sim3_search_by_projection_batch", "orbgpu_download_sim3_matches", "orbgpu_sim3_replay_stats"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "sim3_search_by_projection") and hasattr(og.BatchExtractor, "sim3_matches")
    # a null context is refused whatever else is passed: good arguments, no pairs, a bad projection, a bad ratio
    one = np.zeros(1, np.int32)
    f = og.C.c_float
    call = lib.orbgpu_sim3_search_by_projection_batch
    assert call(None, 1, og._p(one), og._p(one), 1, None, None, None, None, None, 0, None, 0, f(8), f(1.5), 0, None) == -3
    assert call(None, 0, None, None, 0, None, None, None, None, None, 0, None, 0, f(8), f(1.5), 0, None) == -3
    assert call(None, 0, None, None, 0, None, None, None, None, None, 0, None, 0, f(8), f(1.5), 2, None) == -3
    assert call(None, 0, None, None, 0, None, None, None, None, None, 0, None, 0, f(8), f(5.12), 0, None) == -3
    assert lib.orbgpu_download_sim3_matches(None, 0, None, 0, None, None, None, 0, None, None, None) == -3
    assert lib.orbgpu_sim3_replay_stats(None, 0, og._p(np.zeros(4, np.int32))) == -3
    # the wrapper refuses rows that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, og.FUSE_POINT_DTYPE)
    poses = np.zeros(2, og.RELOC_POSE_DTYPE)
    with pytest.raises(ValueError):
        be.sim3_search_by_projection([0, 1], [0], [pts], poses, K_)  # one list index per pair
    with pytest.raises(ValueError):
        be.sim3_search_by_projection([0, 1], [0, 0], [pts], poses[:1], K_)  # one pose per pair
    with pytest.raises(ValueError):
        be.sim3_search_by_projection([0, 1], [0, 0], [pts], poses, K_, skip=[np.zeros(3, np.uint8)])  # one skip row per pair
    with pytest.raises(ValueError):
        be.sim3_search_by_projection([0, 1], [0, 0], [pts], poses, K_, kp_block=[np.zeros(3, np.uint8)])  # one occupancy row per pair
    with pytest.raises(ValueError):  # offsets beyond the points
        be.sim3_search_by_projection([0, 1], [0, 1], (pts, np.array([0, 2, 4], np.int32)), poses, K_)
    # the generator's pose: Rcw = R, tcw = t / s, Ow = -R^T tcw
    c, s = math.cos(0.3), math.sin(0.3)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    pose, (R, tcw) = synth.sim3_pose((2.0, Rz, (2.0, 4.0, -6.0)))
    np.testing.assert_allclose(tcw, (1.0, 2.0, -3.0))
    np.testing.assert_allclose(pose["Ow"], -Rz.T @ tcw, rtol=1e-6)
    np.testing.assert_allclose(np.asarray(pose["Rcw"]).reshape(3, 3), Rz, rtol=1e-6)


# ---- scenes -------------------------------------------------------------------------------------

# name -> (th, ratioHamming, projection, kp_block and skip rows, generator arguments): the three LoopClosing
# call sites (LoopClosing.cc:755, :777, :964), then the occupancy-heavy ones
CASES = {
    "coarse": (8.0, 1.5, INVZ, False, {}),
    "fine": (5.0, 1.0, DIV, False, {}),
    "confirm": (3.0, 1.5, DIV, False, {}),
    "held": (8.0, 1.5, DIV, True, {}),
    # many points on few keypoints under a wide window and limit: the kept candidates run out
    "dense": (25.0, 3.2, INVZ, False, dict(n=3000, pool=150, contested=0.5, contested_pool=40,
                                            contested_flips=(0, 2, 5, 10, 20, 35, 60, 90))),
}


def _scene_sim3():
    """Scw with scale 1.7: a small rotation about y and a translation that is 1.7 times the camera's."""
    a = 0.02
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    return 1.7, R, 1.7 * np.array([0.1, -0.05, 0.2])


def _scene_points(name, seed, xy, kps, desc, bounds, sim3=None, **kw):
    th = CASES[name][0]
    sim3 = _scene_sim3() if sim3 is None else sim3
    args = dict(n=1000, seed=seed, th=th, bounds=[float(v) for v in bounds])
    args.update(CASES[name][4])
    args.update(kw)
    return synth.sim3_points(xy, kps, desc, K_, sim3, **args), synth.sim3_pose(sim3)[0]


def _scene_rows(name, npts, nkp, seed):
    """(skip row, kp_block row) of a scene: a third of the keypoints held, a tenth of the points skipped."""
    if not CASES[name][3]:
        return None, None
    rng = np.random.default_rng(seed)
    return (rng.random(npts) < 0.1).astype(np.uint8) * 3, (rng.random(nkp) < 1 / 3).astype(np.uint8) * 5


def _restate(name, pts, pose, kps, desc, xy, bounds, cs, ci, skip, blk, scale):
    th, ratio, proj = CASES[name][:3]
    return _py_sim3_search(pts, pose, K_, xy, kps["octave"], desc, bounds, cs, ci, skip, blk, th, ratio, proj, scale)


def _scene_conditions(name, nm, cnt):
    """Conditions on the inputs."""
    for c in CODES.values():
        assert cnt[c] >= 5, (c, dict(cnt))
    assert nm == cnt["matched"] >= 100
    assert cnt["octave"] >= 20 and cnt["occupied"] >= 20, dict(cnt)
    assert cnt["clamped_high"] >= 1 and all(cnt["level_%d" % lv] >= 1 for lv in range(8)), dict(cnt)
    if CASES[name][3]:
        assert cnt["held"] >= 20 and cnt["taken"] >= 20 and cnt["skip_byte"] >= 5, dict(cnt)
    if name == "dense":
        assert cnt["not_first"] >= 100 and cnt["beyond_kept"] >= 20, dict(cnt)


@pytest.fixture(scope="module")
def cpu_frame(oracle):
    L, _ = synth.stereo_pair(480, 640, 5)
    kl, dl, _ = oracle.extract(L, nfeatures=500)
    xy, b, _, cs, ci = oracle.undistort_grid(kl, K_, D_, 640, 480)
    return kl, dl.reshape(-1, 32), xy, b, cs, ci, oracle.scale_factors()[0]


@pytest.fixture(scope="module")
def cpu_scenes(cpu_frame):
    """name -> (points, pose, skip, blk, the restatement's outputs), computed once."""
    kl, dl, xy, b, cs, ci, scale = cpu_frame
    out = {}
    for name in CASES:
        pts, pose = _scene_points(name, 100, xy, kl, dl, b)
        skip, blk = _scene_rows(name, len(pts), len(kl), 7)
        out[name] = (pts, pose, skip, blk, _restate(name, pts, pose, kl, dl, xy, b, cs, ci, skip, blk, scale))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_scene_exercises_every_rule(cpu_scenes, name):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the oracle's
    extraction, meets every situation the GPU cases are there to compare."""
    pts, _, _, blk, (m, bi, bd, code, nm, cnt) = cpu_scenes[name]
    print(name, "nmatches", nm, dict(cnt))
    assert (m >= 0).sum() == (bi >= 0).sum() == nm and set(bi[bi >= 0]) == set(np.flatnonzero(m >= 0))
    assert all(m[bi[i]] == i for i in np.flatnonzero(bi >= 0)) and ((bd < 256) == (code == MATCHED)).all()
    if blk is not None:
        assert (m[blk != 0] == -1).all()
    _scene_conditions(name, nm, cnt)


@pytest.mark.parametrize("name", list(CASES))
def test_brute_force_scan_agrees_with_the_restatement(cpu_frame, cpu_scenes, name):
    import orbslam3lib_amd as og
    kl, dl, xy, b, cs, ci, scale = cpu_frame
    th, ratio, proj = CASES[name][:3]
    pts, pose, skip, blk, (m, bi, bd, code, nm, _) = cpu_scenes[name]
    m2, bi2, bd2, c2, nm2 = _brute_sim3(pts, pose, K_, xy, kl["octave"], dl, b, ci, skip, blk, th, ratio, proj, scale,
                                        og.predict_scale_table(1.2, 8))
    np.testing.assert_array_equal(c2, code)
    np.testing.assert_array_equal(bd2, bd)
    np.testing.assert_array_equal(bi2, bi)
    np.testing.assert_array_equal(m2, m)
    assert nm2 == nm


# ---- GPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_env(oracle):
    """Two 640x480 stereo pairs at 1000 features, extracted and gridded once."""
    import orbslam3lib_amd as og
    pairs = [synth.stereo_pair(480, 640, 90 + s) for s in range(2)]
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=4)
    be.upload(np.stack([im for pr in pairs for im in pr]))
    be.run()
    be.undistort_grid(K_, D_)
    be.synchronize()
    imgs = []
    for i in range(4):
        kps, desc, _ = be.result(i)
        xy, _, cs, ci = be.grid_result(i)
        imgs.append((kps, desc.reshape(-1, 32), xy, cs, ci))
    b = oracle.undistort_grid(imgs[0][0], K_, D_, 640, 480)[1]
    yield be, imgs, b, oracle.scale_factors()[0]
    be.close()


def _same(got, want, nkp, q=0):
    gm, gbi, gbd, gcode, gnm = got
    m, bi, bd, code, nm = want[:5]
    assert len(gm) == nkp == len(m) and len(gbi) == len(gbd) == len(gcode) == len(bi)
    np.testing.assert_array_equal(gcode, code, err_msg="pair %d code" % q)
    np.testing.assert_array_equal(gbd, bd, err_msg="pair %d best_dist" % q)
    np.testing.assert_array_equal(gbi, bi, err_msg="pair %d best_idx" % q)
    np.testing.assert_array_equal(gm, m, err_msg="pair %d match" % q)
    assert gnm == nm, (q, gnm, nm)


def _gpu_compare(env, name, frames, lists, point_lists, poses, skips=None, blks=None):
    """One call; every pair against the restatement -> the restatement's outputs per pair."""
    import orbslam3lib_amd as og
    be, imgs, b, scale = env
    th, ratio, proj = CASES[name][:3]
    be.sim3_search_by_projection(frames, lists, point_lists, np.array(poses, og.RELOC_POSE_DTYPE), K_, skip=skips,
                                 kp_block=blks, th=th, ratio_hamming=ratio, projection=proj)
    out = []
    for q, (f, l) in enumerate(zip(frames, lists)):
        kps, desc, xy, cs, ci = imgs[f]
        want = _restate(name, point_lists[l], poses[q], kps, desc, xy, b, cs, ci, None if skips is None else skips[q],
                        None if blks is None else blks[q], scale)
        _same(be.sim3_matches(q), want, len(kps), q)
        out.append(want)
    return out


def _frame_points(env, name, f, seed, **kw):
    _, imgs, b, _ = env
    kps, desc, xy, _, _ = imgs[f]
    return _scene_points(name, seed, xy, kps, desc, b, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_sim3_scenes(gpu_env, name):
    be, imgs = gpu_env[0], gpu_env[1]
    pts, poses = zip(*[_frame_points(gpu_env, name, f, 200 + f) for f in (0, 2)])
    rows = [_scene_rows(name, len(p), len(imgs[f][0]), 40 + f) for p, f in zip(pts, (0, 2))]
    skips, blks = ([r[k] for r in rows] if CASES[name][3] else None for k in (0, 1))
    res = _gpu_compare(gpu_env, name, [0, 2], [0, 1], list(pts), list(poses), skips, blks)
    for r in res:
        _scene_conditions(name, r[4], r[5])
    if name == "dense":  # the conflicts again: identical bytes
        a = [be.sim3_matches(q) for q in range(2)]
        _gpu_compare(gpu_env, name, [0, 2], [0, 1], list(pts), list(poses), skips, blks)
        for q in range(2):
            for x, y in zip(be.sim3_matches(q), a[q]):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        stats = [be.sim3_replay_stats(q) for q in range(2)]
        assert all(s[0] >= 1000 and s[3] >= 20 and s[1] >= (s[0] + 63) // 64 for s in stats), stats


@pytest.mark.gpu
def test_gpu_sim3_one_list_against_three_frames_under_three_poses(gpu_env):
    """Several candidates' coarse searches in one call: one upload of the points, three frames, each pair with
    its own pose, skip row and occupancy; the same as three calls with the skip row folded into the flags."""
    import orbslam3lib_amd as og
    be, imgs = gpu_env[0], gpu_env[1]
    pts, pose = _frame_points(gpu_env, "coarse", 1, 300)
    a = 0.6
    axis = np.array([0.3, 0.8, -0.52]) / np.linalg.norm([0.3, 0.8, -0.52])
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    pose2 = synth.sim3_pose((0.6, np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx, (0.9, -0.5, 1.5)))[0]
    pose3 = synth.sim3_pose((1.0, np.eye(3), (0.02, 0.01, -0.05)))[0]
    poses = [pose, pose2, pose3]
    rng = np.random.default_rng(8)
    skips = [(rng.random(len(pts)) < s).astype(np.uint8) * 5 for s in (0.1, 0.0, 0.5)]
    blks = [(rng.random(len(imgs[f][0])) < s).astype(np.uint8) for f, s in zip((1, 0, 3), (0.0, 0.3, 0.1))]
    res = _gpu_compare(gpu_env, "coarse", [1, 0, 3], [0, 0, 0], [pts], poses, skips, blks)
    assert res[0][4] >= 100 and res[2][5]["skipped"] >= 400
    shared = [be.sim3_matches(q) for q in range(3)]
    for q, f in enumerate((1, 0, 3)):
        folded = pts.copy()
        folded["flags"] = np.where(skips[q] != 0, 0, folded["flags"])
        be.sim3_search_by_projection([f], [0], [folded], np.array([poses[q]], og.RELOC_POSE_DTYPE), K_, kp_block=[blks[q]],
                                     th=8.0, ratio_hamming=1.5, projection=INVZ)
        _same(be.sim3_matches(0), shared[q], len(shared[q][0]), q)


@pytest.mark.gpu
def test_gpu_sim3_two_lists_against_one_frame_and_points_plus_offsets(gpu_env):
    import orbslam3lib_amd as og
    be, imgs = gpu_env[0], gpu_env[1]
    a, pose = _frame_points(gpu_env, "fine", 0, 310)
    c, _ = _frame_points(gpu_env, "fine", 0, 311, n=777)
    rng = np.random.default_rng(4)
    blks = [(rng.random(len(imgs[0][0])) < s).astype(np.uint8) * 2 for s in (0.4, 0.05)]
    _gpu_compare(gpu_env, "fine", [0, 0], [0, 1], [a, c], [pose, pose], None, blks)
    lists = [be.sim3_matches(q) for q in range(2)]
    assert lists[0][4] != lists[1][4]
    # the C ABI's form, not starting at 0, with a list no pair names in between and the lists named out of order
    packed = (np.concatenate([a[:5], a, a[:9], c]), np.array([5, 5 + len(a), 14 + len(a), 14 + len(a) + len(c)], np.int32))
    be.sim3_search_by_projection([0, 0], [2, 0], packed, np.array([pose, pose], og.RELOC_POSE_DTYPE), K_,
                                 kp_block=[blks[1], blks[0]], th=5.0, ratio_hamming=1.0, projection=DIV)
    _same(be.sim3_matches(0), lists[1], len(lists[1][0]))
    _same(be.sim3_matches(1), lists[0], len(lists[0][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(0, 1, 63, 64), (65, 127, 128, 129), (255, 256, 257, 64)])
def test_gpu_sim3_list_lengths_at_the_group_and_block_boundaries(gpu_env, sizes):
    """Every point reaches the replay (no misses in the generator) and aims at one of n / 8 keypoints, so the
    replay's groups of 64 are the list's, and chains of points that want one keypoint cross from one group
    into the next."""
    pts, poses = [], []
    clean = dict(contested=1.0, contested_flips=(0, 2, 5, 10))
    for q, n in enumerate(sizes):
        p, pose = _frame_points(gpu_env, "coarse", q, 400 + n, n=n, contested_pool=max(n // 8, 1), **clean)
        pts.append(p)
        poses.append(pose)
    res = _gpu_compare(gpu_env, "coarse", [0, 1, 2, 3], [0, 1, 2, 3], pts, poses)
    for n, r in zip(sizes, res):
        assert len(r[1]) == n and r[4] >= min(n, max(n // 8, 1)) // 2, (n, r[4])
        if n >= 65:
            assert r[5]["taken_across_64"] >= 1 and r[5]["skipped"] == 0, (n, dict(r[5]))


@pytest.mark.gpu
def test_gpu_sim3_one_list_of_20000_points(gpu_env):
    """The LoopClosing shape: the points of a matched keyframe and its covisibles, most of which end at a gate
    (half are already found or bad), against one keyframe."""
    pts, pose = _frame_points(gpu_env, "confirm", 2, 500, n=20000, invalid=0.3, behind=0.1, outside=0.15, contested=0.1,
                              contested_pool=300)
    skip = (np.random.default_rng(5).random(20000) < 0.2).astype(np.uint8)
    ((m, bi, bd, code, nm, cnt),) = _gpu_compare(gpu_env, "confirm", [2], [0], [pts], [pose], [skip])
    assert nm >= 500 and cnt["skipped"] >= 8000 and cnt["taken"] >= 1000, (nm, dict(cnt))
    pending, passes, stale, walks = gpu_env[0].sim3_replay_stats(0)
    assert nm <= pending <= 20000 - cnt["skipped"] and passes >= (pending + 63) // 64


@pytest.mark.gpu
def test_gpu_sim3_all_skipped_and_no_pairs(gpu_env):
    import orbslam3lib_amd as og
    be = gpu_env[0]
    pts, pose = _frame_points(gpu_env, "coarse", 2, 600, n=200)
    ((m, bi, bd, code, nm, _),) = _gpu_compare(gpu_env, "coarse", [2], [0], [pts], [pose], [np.ones(200, np.uint8)])
    assert nm == 0 and (code == SKIPPED).all() and (bi == -1).all() and (bd == 256).all() and (m == -1).all()
    pts["flags"] = 0
    ((m, _, _, code, nm, _),) = _gpu_compare(gpu_env, "coarse", [2], [0], [pts], [pose])
    assert nm == 0 and (code == SKIPPED).all() and (m == -1).all()
    assert be.sim3_replay_stats(0) == (0, 0, 0, 0)
    be.sim3_search_by_projection([], [], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_)  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.sim3_matches(0)
    assert e.value.code == -3


@pytest.mark.gpu
def test_gpu_sim3_ratio_on_a_table_threshold(gpu_env):
    """Points whose ratio max_distance / dist sits exactly on a step of the level, and one float above."""
    import orbslam3lib_amd as og
    steps = og.predict_scale_table(1.2, 8)
    base, pose = _frame_points(gpu_env, "coarse", 0, 9, n=400, contested=0.0, invalid=0.0, behind=0.0, outside=0.0,
                               too_near=0.0, too_far=0.0, bad_normal=0.0, empty=0.0, not_finite=0.0, flips=(0, 2, 5))
    Ow = np.asarray(pose["Ow"], F32)
    pts, want = [], []
    for j, p in enumerate(base):
        n = j % 7
        P = [F32(v) - o for v, o in zip(p["pos"], Ow)]
        d = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
        for target, lv in ((steps[n], n), (np.nextafter(steps[n], F32(np.inf)), n + 1)):
            mx = target * d
            for _ in range(8):  # the float whose quotient by d is the target, if there is one
                if mx / d < target:
                    mx = np.nextafter(mx, F32(np.inf))
                elif mx / d > target:
                    mx = np.nextafter(mx, F32(0))
            if mx / d != target:
                continue
            q = p.copy()
            q["max_distance"], q["min_distance"] = mx, 0.0
            pts.append(q)
            want.append(lv)
    pts = np.array(pts)
    assert len(pts) >= 300 and min(Counter(want).values()) >= 10 and set(want) == set(range(8))
    ((_, _, _, code, nm, cnt),) = _gpu_compare(gpu_env, "coarse", [0], [0], [pts], [pose])
    levels = [cnt["level_%d" % lv] for lv in range(8)]
    assert all(0 < got <= Counter(want)[lv] for lv, got in enumerate(levels)) and sum(levels) >= 0.9 * len(pts)
    assert nm >= 50


@pytest.mark.gpu
def test_gpu_sim3_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    pose = synth.sim3_pose(_scene_sim3())[0]
    pts = np.zeros(4, og.FUSE_POINT_DTYPE)
    poses = np.array([pose], og.RELOC_POSE_DTYPE)
    lib = og.load_library()

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.sim3_search_by_projection(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.sim3_matches(0)
    assert e.value.code == -3
    assert code([0], [0], [pts], poses, K_) == -3  # before undistort_grid
    be.undistort_grid(K_, D_)
    n0, n1 = len(be.result(0)[0]), len(be.result(1)[0])
    be.sim3_search_by_projection([0], [0], [pts], poses, K_)
    assert code([2], [0], [pts], poses, K_) == -3 and code([-1], [0], [pts], poses, K_) == -3  # outside the gridded range
    assert code([0], [1], [pts], poses, K_) == -3 and code([0], [-1], [pts], poses, K_) == -3  # lists[p] outside [0, n_lists)
    assert code([0], [0], [pts], poses, K_, th=-1.0) == -3 and code([0], [0], [pts], poses, K_, th=float("nan")) == -3
    assert code([0], [0], [pts], poses, K_, th=float("inf")) == -3
    # the ratio rule: 0 <= 50.0f * ratio_hamming < 256 and finite
    assert code([0], [0], [pts], poses, K_, ratio_hamming=5.12) == -3  # 50 * 5.12f = 256
    assert code([0], [0], [pts], poses, K_, ratio_hamming=-0.01) == -3
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert code([0], [0], [pts], poses, K_, ratio_hamming=bad) == -3
    be.sim3_search_by_projection([0], [0], [pts], poses, K_, ratio_hamming=float(np.nextafter(F32(5.12), F32(0))))
    be.sim3_search_by_projection([0], [0], [pts], poses, K_, ratio_hamming=0.0)
    assert code([0], [0], [pts], poses, K_, projection=2) == -3 and code([0], [0], [pts], poses, K_, projection=-1) == -3
    assert code([0], [0], [pts], poses, K_, skip=[np.zeros(3, np.uint8)]) == -3  # skip_stride below the list's length
    assert code([0], [0], [pts], poses, K_, kp_block=[np.zeros(n0 - 1, np.uint8)]) == -3  # kp_stride below the keypoint count
    be.sim3_search_by_projection([0], [0], [pts], poses, K_, kp_block=[np.zeros(n0, np.uint8)])
    pp = np.array([pose] * 2, og.RELOC_POSE_DTYPE)
    assert code([1, 1], [0, 1], (pts, np.array([0, 4, 2], np.int32)), pp, K_) == -3  # offsets descend
    assert code([1] * 3, [0] * 3, [pts], np.array([pose] * 3, og.RELOC_POSE_DTYPE), K_) == -3  # above the image capacity
    # null arrays with work to do, a negative first offset and negative counts, straight at the ABI
    fr, off, Kf = np.zeros(1, np.int32), np.array([0, 4], np.int32), np.asarray(K_, np.float32)
    f = og.C.c_float
    args = [be.ctx.handle, 1, og._p(fr), og._p(fr), 1, og._p(pts), og._p(off), og._p(poses), og._p(Kf), None, 0, None, 0,
            f(8), f(1.5), 0, None]
    call = lib.orbgpu_sim3_search_by_projection_batch
    assert call(*args) == 0
    for k in (2, 3, 5, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert call(*bad) == -3, k
    neg = np.array([-1, 3], np.int32)
    assert call(*(args[:6] + [og._p(neg)] + args[7:])) == -3
    assert call(*([args[0], -1] + args[2:])) == -3
    assert call(*(args[:4] + [0] + args[5:])) == -3  # no lists
    blk = np.zeros(n0, np.uint8)
    assert call(*(args[:11] + [og._p(blk), -1] + args[13:])) == -3  # negative kp_stride
    long_list = np.zeros(og.FUSE_MAX_POINTS + 1, og.FUSE_POINT_DTYPE)
    assert code([0], [0], [long_list], poses, K_) == -2  # ORBGPU_ERR_CAPACITY
    assert code([0], [0], [pts, long_list], poses, K_) == -2  # any list, named or not
    # the result of the last good call is still there: the error paths launched nothing
    be.sim3_search_by_projection([1], [0], [pts], poses, K_, skip=[np.zeros(4, np.uint8)], th=0.0)
    assert code([0], [0], [long_list], poses, K_) == -2 and code([0], [0], [pts], poses, K_, projection=2) == -3
    m, bi, bd, cd, nm = be.sim3_matches(0)
    assert len(bi) == 4 and (cd == SKIPPED).all() and len(m) == n1 and nm == 0 and (m == -1).all()
    with pytest.raises(og.OrbGpuError) as e:
        be.sim3_matches(1)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:
        be.sim3_replay_stats(1)
    assert e.value.code == -3
    for kw in (dict(cap_points=3), dict(cap_kp=n1 - 1)):  # each capacity on its own
        with pytest.raises(og.OrbGpuError) as e:
            be.sim3_matches(0, **kw)
        assert e.value.code == -2
    assert len(be.sim3_matches(0, cap_points=4, cap_kp=n1)[0]) == n1 and n0 > 0
    be.close()
    # a keypoint capacity above the resolve kernel's LDS budget (160 KiB: a bit and a word per keypoint).  It is
    # the context's own limit, met before the batch is looked at: the upload sizes the context, nothing runs
    big = og.BatchExtractor(41000, 1.2, 8, 20, 7, width=640, height=480, max_images=1)
    big.upload(L[None])
    with pytest.raises(og.OrbGpuError) as e:
        big.sim3_search_by_projection([0], [0], [pts], poses, K_)
    assert e.value.code == -2
    big.sim3_search_by_projection([], [], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_)  # no pairs: nothing to hold
    big.close()


@pytest.mark.gpu
def test_gpu_sim3_keeps_its_results_and_leaves_the_other_searches_theirs(gpu_env):
    import orbslam3lib_amd as og
    be, imgs, b, _ = gpu_env
    kps, desc, xy, _, _ = imgs[0]
    kr, dr = imgs[1][0], imgs[1][1]
    sim3 = _scene_sim3()
    pose, Rt = synth.sim3_pose(sim3)
    poses = np.array([pose], og.RELOC_POSE_DTYPE)
    bounds = [float(v) for v in b]
    fp = synth.fuse_points(xy, kps, desc, K_, Rt, n=500, seed=4, bounds=bounds)
    rp = synth.reloc_points(xy, kps, desc, K_, Rt, n=500, seed=3, bounds=bounds)
    bp = np.zeros(len(kr), og.BOW_POINT_DTYPE)
    bp["desc"], bp["angle"], bp["node"], bp["flags"] = dr, kr["angle"], dr[:, 0] >> 2, og.BOW_HAS_POINT
    nodes = [(desc[:, 0] >> 2).astype(np.int32)]

    def others(n):
        be.fuse([0], [0], [fp[:n]], poses, K_, sim3=True)
        be.reloc_by_projection([0], [rp[:n]], poses, K_)
        be.search_by_bow([0], [bp[:n]], nodes)
        return be.fuse_matches(0), be.reloc_matches(0), be.bow_matches(0)
    before = others(500)
    assert before[0][4] > 0 and before[1][1] > 0
    pts, _ = _frame_points(gpu_env, "coarse", 0, 700)
    (want,) = _gpu_compare(gpu_env, "coarse", [0], [0], [pts], [pose])
    for got, was in zip((be.fuse_matches(0), be.reloc_matches(0), be.bow_matches(0)), before):
        for x, y in zip(got, was):
            np.testing.assert_array_equal(x, y)
    others(300)  # a following fuse, reloc_by_projection and search_by_bow
    _same(be.sim3_matches(0), want, len(kps))
    assert want[4] >= 100
