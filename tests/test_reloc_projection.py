"""ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) --
the search Tracking::Relocalization runs on a candidate keyframe after PnP left too few inliers
(cpp/src/ORBmatcher.cc:1923-2059, with ComputeThreeMaxima :2061-2102, MapPoint::PredictScale,
MapPoint.cc:533-548, and Frame::GetFeaturesInArea, Frame.cc:673-739), pinhole frames, monocular path.

The yardstick is _py_reloc below: an independent restatement written from those lines with
np.float32 scalars (every product and sum rounds to single, in the reference's order), which takes
logf from the host libm through ctypes -- not numpy's own logf, not the library's table -- and also
returns a Counter of the rules it hit.
CPU: the restatement against hand-built known answers on a tiny frame (taken and pre-occupied
keypoints, ORBdist at equality, equal distances, every bound and both invariance limits at the limit
and one float beyond, invalid points, the first and the last level, the fmodf branch, bin edges, the
three-maxima rule, the two deviations, no orientation check); orbgpu_predict_scale_table against logf;
the dtypes, symbols and the statuses decided before any launch; conditions on the scenes the GPU
cases use.
GPU: k_reloc_candidates + k_reloc_resolve against the restatement, equal on match, nmatches and the
30 histogram bins.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs Sophus, Eigen and the SLAM
stack; no fixtures ship for it) -- restatement only, as for the other matcher functions."""
import ctypes
import ctypes.util
import math
from collections import Counter

import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_track_projection import (D_, F32, K_, POP, _c_round, _flip, _grid, _header_struct_bytes, _three_maxima,
                                         _window)

_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.logf.restype = ctypes.c_float
_LIBM.logf.argtypes = [ctypes.c_float]


def _logf(x):
    """The host libm's logf on a float32."""
    return F32(_LIBM.logf(float(F32(x))))


def _predict_scale(ratio, scale_factor, nlevels):
    """MapPoint::PredictScale (MapPoint.cc:541-547) -> (clamped level, the value before the clamps)."""
    with np.errstate(all="ignore"):
        q = _logf(ratio) / _logf(F32(scale_factor))  # mfLogScaleFactor = log(mfScaleFactor), Frame.cc:132
    n = int(math.ceil(float(q))) if np.isfinite(q) else -2 ** 31  # (int) of a non-finite float on x86
    return min(max(n, 0), nlevels - 1), n


def _reloc_bin(angle_kf, angle_f):
    """:2013-2024; None outside [0, 30) (the reference's assert)."""
    with np.errstate(all="ignore"):
        rot = F32(angle_kf) - F32(angle_f)
        if rot < 0.0 or rot > 360.0:
            rot = F32(math.fmod(float(rot), 360.0)) if np.isfinite(rot) else F32(np.nan)  # fmodf is exact
        if rot < 0.0:
            rot = rot + F32(360.0)
        x = rot * (F32(1.0) / F32(30))
    if not np.isfinite(x):
        return None
    b = _c_round(x)
    if b == 30:
        b = 0
    return b if 0 <= b < 30 else None


def _py_reloc(pts, pose, K, xy, octv, ang, desc, bounds, cs, ci, blk, th, orb_dist, check, scale, scale_factor=1.2,
              nlevels=8):
    """-> match [n_kp] (index into pts or -1), nmatches, hist [30] (before the three-maxima rule),
    Counter of the rules."""
    n = len(octv)
    xy = np.asarray(xy, F32)
    held = np.zeros(n, bool) if blk is None else (np.asarray(blk)[:n] != 0)
    held0 = held.copy()
    match = np.full(n, -1, np.int32)
    events = [[] for _ in range(30)]
    cnt = Counter()
    b = np.asarray(bounds, F32)
    R, t, Ow = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Ow"))
    fx, fy, cx, cy = (F32(v) for v in K)
    nm = 0
    for i, p in enumerate(pts):
        if not (int(p["flags"]) & 1):  # :1941-1944
            cnt["invalid"] += 1
            continue
        X, Y, Z = (F32(v) for v in p["pos"])
        with np.errstate(all="ignore"):
            xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]  # :1949
            yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
            zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
            u = fx * xc / zc + cx  # Pinhole.cpp:40-41
            v = fy * yc / zc + cy
        if u < b[0] or u > b[1]:  # :1953-1956
            cnt["out_min_x" if u < b[0] else "out_max_x"] += 1
            continue
        if v < b[2] or v > b[3]:
            cnt["out_min_y" if v < b[2] else "out_max_y"] += 1
            continue
        if not (np.isfinite(u) and np.isfinite(v)):  # deviation
            cnt["not_finite"] += 1
            continue
        with np.errstate(all="ignore"):
            px, py, pz = X - Ow[0], Y - Ow[1], Z - Ow[2]  # :1959-1960
            dist3d = np.sqrt((px * px + py * py) + pz * pz)
            lo, hi = F32(0.8) * F32(p["min_distance"]), F32(1.2) * F32(p["max_distance"])  # MapPoint.cc:504-514
        if not np.isfinite(dist3d):  # deviation
            cnt["not_finite"] += 1
            continue
        if dist3d < lo or dist3d > hi:  # :1966
            cnt["too_near" if dist3d < lo else "too_far"] += 1
            continue
        with np.errstate(all="ignore"):
            ratio = F32(p["max_distance"]) / dist3d  # MapPoint.cc:538
        if not np.isfinite(ratio):  # deviation
            cnt["not_finite"] += 1
            continue
        level, raw = _predict_scale(ratio, scale_factor, nlevels)
        cnt["level_%d" % level] += 1
        cnt["clamped_low"] += raw < 0
        cnt["clamped_high"] += raw >= nlevels
        radius = F32(th) * F32(scale[level])  # :1972
        cand = _window(xy, octv, cs, ci, b, u, v, radius, level - 1, level + 1)  # :1974
        if not cand:
            cnt["empty_window"] += 1
            continue
        best, bi = 256, -1
        passed = []  # (distance, window position, taken by now) of what the pre-call state lets within ORBdist
        for pos, k in enumerate(cand):
            if held[k]:  # :1988-1989
                cnt["blocked" if held0[k] else "taken"] += 1
                if held0[k]:
                    continue
            d = int(POP[np.bitwise_xor(p["desc"], desc[k])].sum())
            if d <= orb_dist:
                passed.append((d, pos, bool(held[k])))
            if held[k]:
                continue
            if d < best:  # :1995
                best, bi = d, k
        # instrumentation only: the four lowest (distance, position) within ORBdist are all taken and more passed
        dry = len(passed) > 4 and all(tk for _, _, tk in sorted(passed)[:4])
        cnt["list_dry"] += dry
        cnt["list_dry_matched"] += dry and best <= orb_dist
        if best <= orb_dist:  # :2004
            assert match[bi] < 0
            match[bi] = i
            nm += 1
            held[bi] = True
            cnt["events"] += 1
            if check:
                bn = _reloc_bin(p["angle"], ang[bi])
                if bn is None:  # deviation
                    cnt["bin_out_of_range"] += 1
                else:
                    events[bn].append(bi)
        else:
            cnt["above_orb_dist"] += 1
    hist = np.array([len(e) for e in events], np.int32)
    if check:  # :2036-2056
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn not in keep:
                for k in events[bn]:
                    match[k] = -1
                    nm -= 1
                    cnt["rejected"] += 1
    return match, nm, hist, cnt


# ---- hand-built frames --------------------------------------------------------------------------

SC = (F32(1.2) ** np.arange(8)).astype(F32)  # stands for mvScaleFactors in the hand-built cases


def _reloc_pose(R=None, t=(0.0, 0.0, 0.0)):
    import orbslam3lib_amd as og
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    p = np.zeros((), og.RELOC_POSE_DTYPE)
    p["Rcw"], p["tcw"], p["Ow"] = R.reshape(9), t, -R.T @ t  # Tcw.inverse().translation()
    return p


class _Tiny:
    """8 x 5 keypoints 70 px apart (windows of levels 0-2 at th 10 do not meet), octave 0, angle 0,
    random descriptors; `extra`: more (x, y, octave, desc) keypoints.  K = (512, 512, 0, 0) -- a
    projection u = 512 x / z that reaches every float -- and bounds centred on the principal point."""
    K = (512.0, 512.0, 0.0, 0.0)
    B = np.array([-320, 320, -240, 240], F32)

    def __init__(self, extra=(), seed=0):
        rng = np.random.default_rng(seed)
        pts = [(-260.0 + 70 * i, -180.0 + 70 * j) for j in range(5) for i in range(8)]
        self.desc = rng.integers(0, 256, (len(pts) + len(extra), 32), dtype=np.uint8)
        octv = [0] * len(pts)
        for j, (x, y, o, d) in enumerate(extra):
            pts.append((x, y))
            octv.append(o)
            if d is not None:
                self.desc[40 + j] = d
        self.xy = np.array(pts, F32)
        self.octv = np.array(octv, np.int32)
        self.ang = np.zeros(len(pts), F32)
        self.cs, self.ci = _grid(self.xy, self.B)
        assert len(self.ci) == len(pts)

    def run(self, pts, th=10.0, orb_dist=100, check=True, blk=None, pose=None):
        return _py_reloc(pts, _reloc_pose() if pose is None else pose, self.K, self.xy, self.octv, self.ang, self.desc,
                         self.B, self.cs, self.ci, blk, th, orb_dist, check, SC)


def _aim(x, y, desc, angle=0.0, level=0, z=2.0, valid=True):
    """A keyframe point that projects to (x, y) under the identity pose and _Tiny.K and whose
    distance predicts `level`."""
    import orbslam3lib_amd as og
    p = np.zeros((), og.RELOC_POINT_DTYPE)
    pos = np.array((x / _Tiny.K[0] * z, y / _Tiny.K[1] * z, z))
    p["pos"] = pos
    dist = float(np.linalg.norm(pos))
    p["max_distance"] = dist * (0.95 if level == 0 else 1.2 ** (level - 0.5))
    p["min_distance"] = p["max_distance"] / 1.2 ** 7
    p["angle"], p["flags"], p["desc"] = angle, (og.RP_VALID if valid else 0), desc
    return p


def _bits(*ranges):
    b = np.zeros(256, np.uint8)
    for lo, hi in ranges:
        b[lo:hi] = 1
    return np.packbits(b)


def test_an_earlier_point_takes_the_keypoint_a_later_closer_one_would_have_won():
    base = _Tiny()
    A = _aim(-260, -180, _flip(base.desc[0], 10))
    B = _aim(-260, -180, base.desc[0])
    # nothing else in the window: the second point, though closer, finds its keypoint taken
    m, nm, _, cnt = base.run(np.array([A, B]), check=False)
    assert m[0] == 0 and nm == 1 and cnt["taken"] == 1 and cnt["events"] == 1
    # a second keypoint 8 px away, 40 bits from the first: the later point's next best
    T = _Tiny(extra=[(-252.0, -180.0, 0, _flip(base.desc[0], 40, 2))])
    m, nm, _, cnt = T.run(np.array([A, B]), check=False)
    assert m[0] == 0 and m[40] == 1 and nm == 2 and cnt["taken"] == 1
    # the other order: the closer one comes first and wins, the farther one is left with the neighbour (50 bits)
    m, nm, _, _ = T.run(np.array([B, A]), check=False)
    assert m[0] == 0 and m[40] == 1 and nm == 2


def test_a_pre_occupied_keypoint_is_skipped_and_the_next_best_taken():
    base = _Tiny()
    T = _Tiny(extra=[(-252.0, -180.0, 0, _flip(base.desc[0], 40, 2))])
    blk = np.zeros(41, np.uint8)
    blk[0] = 7  # any non-zero value
    m, nm, _, cnt = T.run(np.array([_aim(-260, -180, T.desc[0])]), check=False, blk=blk)
    assert m[0] == -1 and m[40] == 0 and nm == 1 and cnt["blocked"] == 1
    blk[40] = 1
    m, nm, _, cnt = T.run(np.array([_aim(-260, -180, T.desc[0])]), check=False, blk=blk)
    assert nm == 0 and (m == -1).all() and cnt["blocked"] == 2


def test_best_equal_to_orb_dist_passes_and_one_more_fails():
    Z = _bits()
    T = _Tiny(extra=[(0.0, 0.0, 0, _bits((0, 64)))])
    T.desc[:40] = 255  # nothing else comes near
    p = np.array([_aim(0, 0, Z)])
    assert T.run(p, orb_dist=64)[1] == 1 and T.run(p, orb_dist=63)[1] == 0
    assert T.run(p, orb_dist=63)[3]["above_orb_dist"] == 1
    T = _Tiny(extra=[(0.0, 0.0, 0, _bits((0, 100)))])
    T.desc[:40] = 255
    assert T.run(p, orb_dist=100)[1] == 1 and T.run(p, orb_dist=99)[1] == 0
    T = _Tiny(extra=[(0.0, 0.0, 0, Z)])
    assert T.run(p, orb_dist=0)[1] == 1  # distance 0 at ORBdist 0


def test_an_equal_distance_keeps_the_earlier_window_position():
    Z = _bits()
    # window order: grid column, then row, then index: the keypoint further left comes first whatever its index
    T = _Tiny(extra=[(8.0, 0.0, 0, _bits((0, 7))), (-8.0, 0.0, 0, _bits((7, 14)))])
    m, nm, _, _ = T.run(np.array([_aim(0, 0, Z)]), th=15.0, check=False)
    assert nm == 1 and m[41] == 0 and m[40] == -1
    # in one cell the lower index comes first
    T = _Tiny(extra=[(1.0, 0.0, 0, _bits((0, 7))), (0.5, 0.0, 0, _bits((7, 14)))])
    m, nm, _, _ = T.run(np.array([_aim(0, 0, Z)]), check=False)
    assert nm == 1 and m[40] == 0 and m[41] == -1


@pytest.mark.parametrize("axis,bound,inside", [(0, -320.0, 1), (0, 320.0, -1), (1, -240.0, 1), (1, 240.0, -1)])
def test_each_bound_at_the_bound_passes_and_one_float_beyond_is_skipped(axis, bound, inside):
    """u = 512 x / 1 + 0 is exact, so the projection lands on the bound and on the float next to it."""
    import orbslam3lib_amd as og
    kp = [0.0, 0.0]
    kp[axis] = bound + 8 * inside  # a keypoint 8 px inside the bound, within the level-0 radius of 10
    T = _Tiny(extra=[(kp[0], kp[1], 0, None)])
    why = ("out_min_x", "out_max_x", "out_min_y", "out_max_y")[2 * axis + (inside < 0)]
    for target, want in ((F32(bound), 1), (np.nextafter(F32(bound), F32(-inside * 1e9)), 0)):
        p = np.zeros((), og.RELOC_POINT_DTYPE)
        p["pos"][axis], p["pos"][2] = target / F32(512), 1.0
        p["max_distance"], p["min_distance"] = float(np.linalg.norm(p["pos"])) * 0.95, 0.01
        p["flags"], p["desc"] = og.RP_VALID, T.desc[40]
        assert F32(512) * p["pos"][axis] / F32(1) + F32(0) == target and (target == F32(bound)) == bool(want)
        m, nm, _, cnt = T.run(np.array([p]))
        assert nm == want and cnt[why] == 1 - want and (m[40] == 0) == bool(want)


def test_each_invariance_limit_at_the_limit_passes_and_one_float_beyond_is_skipped():
    """On the optical axis under the identity pose dist3D = sqrtf(z * z) = z exactly."""
    import orbslam3lib_amd as og
    T = _Tiny(extra=[(2.0, 0.0, 0, None)])

    def run(z, mn, mx):
        p = np.zeros((), og.RELOC_POINT_DTYPE)
        p["pos"][2], p["min_distance"], p["max_distance"] = z, mn, mx
        p["flags"], p["desc"] = og.RP_VALID, T.desc[40]
        assert np.sqrt(F32(z) * F32(z)) == F32(z)
        return T.run(np.array([p]))
    mx = F32(3.3)
    far = F32(1.2) * mx  # 1.2f * mfMaxDistance in single
    _, nm, _, cnt = run(far, 0.1, mx)
    assert nm == 1 and cnt["level_0"] == 1
    _, nm, _, cnt = run(np.nextafter(far, F32(1e9)), 0.1, mx)
    assert nm == 0 and cnt["too_far"] == 1
    mn = F32(2.7)
    near = F32(0.8) * mn
    _, nm, _, cnt = run(near, mn, near)  # max_distance = dist3D: ratio 1, level 0
    assert nm == 1 and cnt["level_0"] == 1
    _, nm, _, cnt = run(np.nextafter(near, F32(0)), mn, near)
    assert nm == 0 and cnt["too_near"] == 1


def test_an_invalid_point_neither_matches_nor_blocks():
    T = _Tiny()
    d = T.desc[0]
    m, nm, _, cnt = T.run(np.array([_aim(-260, -180, d, valid=False), _aim(-260, -180, _flip(d, 3))]))
    assert m[0] == 1 and nm == 1 and cnt["invalid"] == 1 and cnt["taken"] == 0
    assert T.run(np.array([_aim(-260, -180, d, valid=False)]))[1] == 0
    p = _aim(-260, -180, d)
    p["flags"] = 2  # only bit 0 counts
    assert T.run(np.array([p]))[1] == 0


def test_not_finite_points_are_skipped():
    T = _Tiny()
    d = T.desc[0]
    nan = _aim(-260, -180, d)
    nan["pos"][0] = np.nan
    zero = _aim(-260, -180, d, z=0.0)  # zc = 0: no 1/z test here, 0 / 0 is not finite
    huge = _aim(0, 0, d)
    huge["pos"] = (0, 0, 1e30)  # projects to the centre; dist3D overflows
    huge["max_distance"] = np.inf
    inf = _aim(-260, -180, d)
    inf["max_distance"] = np.inf  # passes the gate, the ratio is not finite
    for p in (nan, zero, huge, inf):
        m, nm, _, cnt = T.run(np.array([p]))
        assert nm == 0 and (m == -1).all() and cnt["not_finite"] == 1
    behind = _aim(-260, -180, d, z=-2.0)  # no 1/z test (:1951-1956): a point behind the camera projects and matches
    assert T.run(np.array([behind]))[1] == 1


def test_first_and_last_level_windows_and_the_clamps():
    """Eight keypoints of octaves 0..7 within a few px: level 0 searches minLevel = -1 .. 1, which still
    applies maxLevel; a ratio above the last step is clamped to nlevels - 1, one below the first to 0."""
    T = _Tiny()
    T.xy = np.array([(2.0 * o - 7, 0.0) for o in range(8)], F32)
    T.octv = np.arange(8, dtype=np.int32)
    T.ang = np.zeros(8, F32)
    T.desc = np.random.default_rng(5).integers(0, 256, (8, 32), dtype=np.uint8)
    T.cs, T.ci = _grid(T.xy, T.B)

    def sees(ratio):
        out, key = [], None
        for target in range(8):
            p = _aim(0, 0, T.desc[target])
            p["max_distance"] = F32(2.0) * F32(ratio)  # dist3D = 2 exactly
            p["min_distance"] = 0.0
            m, nm, _, cnt = T.run(np.array([p]))
            key = [k for k in cnt if k.startswith("level_")] + [cnt["clamped_low"], cnt["clamped_high"]]
            if nm:
                assert m[target] == 0
                out.append(target)
        return out, key
    assert sees(0.95) == ([0, 1], ["level_0", 0, 0])
    assert sees(1.0) == ([0, 1], ["level_0", 0, 0])  # logf(1) = 0: ceil(0 / logs) = 0
    assert sees(1.01) == ([0, 1, 2], ["level_1", 0, 0])
    assert sees(1.2 ** 2.5) == ([2, 3, 4], ["level_3", 0, 0])
    assert sees(1.2 ** 6.5) == ([6, 7], ["level_7", 0, 0])
    assert sees(1.2 ** 8.5) == ([6, 7], ["level_7", 0, 1])  # nScale = 9, clamped from above
    # the gate keeps the ratio at or above 1 / 1.2f: the furthest point still let through
    assert sees(1 / 1.2)[0] == [0, 1]
    assert _predict_scale(F32(0.5), 1.2, 8) == (0, -3) and _predict_scale(F32(1.2) ** 20, 1.2, 8)[0] == 7
    assert _predict_scale(F32(0.0), 1.2, 8)[0] == 0


@pytest.mark.parametrize("akf,af,expect", [(390.0, 0.0, 1), (-400.0, 0.0, 11), (14.9, 0.0, 0), (15.0, 0.0, 1),
                                           (359.0, 0.0, 12), (0.0, 0.5, 12), (44.9, 0.0, 1), (45.1, 0.0, 2),
                                           (10.0, 350.0, 1), (360.0, 0.0, 12), (720.0, 0.0, 0), (0.0, 0.0, 0),
                                           (-15.0, 0.0, 12), (1000.0, 0.0, 9)])
def test_rotation_bins_and_the_fmodf_branch(akf, af, expect):
    """rot = 390 -> fmodf -> 30 -> bin 1; rot = -400 -> fmodf -> -40 -> +360 = 320 -> bin 11; the factor is
    1 / 30 on [0, 360], so bins end at 12 and the 30 -> 0 wrap (:2023-2024) is out of reach."""
    assert _reloc_bin(akf, af) == expect
    T = _Tiny()
    T.ang[3] = af
    _, nm, hist, _ = T.run(np.array([_aim(T.xy[3, 0], T.xy[3, 1], T.desc[3], angle=akf)]))
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1
    assert max(_reloc_bin(a, 0.0) for a in np.linspace(-2000, 2000, 4001)) == 12


def _bin_scene(T, sizes):
    """{bin: events}, one keypoint each, in keypoint order."""
    pts, k = [], 0
    for bn, n in sizes.items():
        for _ in range(n):
            pts.append(_aim(T.xy[k, 0], T.xy[k, 1], T.desc[k], angle=30.0 * bn))
            k += 1
    return np.array(pts)


def test_three_maxima_ties_and_cutoffs():
    T = _Tiny()
    # strict >: the earlier bins win the tie, the fourth is rejected
    m, nm, hist, cnt = T.run(_bin_scene(T, {2: 5, 5: 5, 7: 5, 9: 5}))
    assert list(hist[[2, 5, 7, 9]]) == [5, 5, 5, 5] and nm == 15 and cnt["rejected"] == 5 and (m[15:20] == -1).all()
    # exactly 10%: 0.1f * 10.0f rounds to 1.0f, so one event beside ten is kept
    assert T.run(_bin_scene(T, {0: 10, 3: 1}))[1] == 11
    # max2 below 10%: the second and the third are dropped together
    _, nm, _, cnt = T.run(_bin_scene(T, {4: 22, 1: 2, 8: 2}))
    assert nm == 22 and cnt["rejected"] == 4
    # only max3 below 10%
    assert T.run(_bin_scene(T, {4: 22, 1: 3, 8: 2}))[1] == 25


def test_the_bin_out_of_range_deviation_and_no_orientation_check():
    T = _Tiny()
    pts = _bin_scene(T, {1: 12, 5: 1})
    pts[0]["angle"] = np.nan  # the event counts, enters no bin and survives the rejection that takes bin 5's
    m, nm, hist, cnt = T.run(pts)
    assert cnt["bin_out_of_range"] == 1 and hist.sum() == 12 and hist[1] == 11 and hist[5] == 1
    assert cnt["rejected"] == 1 and m[0] == 0 and m[12] == -1 and nm == 12
    pts[0]["angle"] = np.inf
    assert T.run(pts)[1] == 12
    # no orientation check: no bins, nothing rejected
    m, nm, hist, cnt = T.run(pts, check=False)
    assert hist.sum() == 0 and nm == 13 and cnt["rejected"] == 0 and (m[:13] >= 0).all()


# ---- the level table ----------------------------------------------------------------------------

def _levels_by_logf(ratios, scale_factor, nlevels):
    lg = np.array(list(map(_LIBM.logf, ratios.tolist())), F32)
    q = lg / _logf(F32(scale_factor))
    return np.clip(np.ceil(q.astype(np.float64)), 0, nlevels - 1).astype(np.int64)


@pytest.mark.parametrize("scale_factor,nlevels", [(1.2, 8), (2.0, 8), (1.1, 12), (1.05, 12)])
def test_predict_scale_table_equals_logf(scale_factor, nlevels):
    import orbslam3lib_amd as og
    t = og.predict_scale_table(scale_factor, nlevels)
    assert t.dtype == F32 and len(t) == nlevels - 1 and t[0] == 1.0 and (np.diff(t) > 0).all()
    bits = (t.view(np.uint32).astype(np.int64)[:, None] + np.arange(-64, 65)[None, :]).reshape(-1)
    near = bits.astype(np.uint32).view(F32)
    s = float(F32(scale_factor))
    rnd = np.random.default_rng(int(scale_factor * 100)).uniform(0.5, s ** (nlevels + 1), 10 ** 6).astype(F32)
    for r in (near, rnd):
        np.testing.assert_array_equal(np.searchsorted(t, r, side="left"), _levels_by_logf(r, scale_factor, nlevels))
    # each entry is the last float of its step
    lv = _levels_by_logf(np.concatenate([t, np.nextafter(t, F32(np.inf))]), scale_factor, nlevels)
    assert list(lv[:nlevels - 1]) == list(range(nlevels - 1)) and list(lv[nlevels - 1:]) == list(range(1, nlevels))


def test_predict_scale_table_arguments():
    import orbslam3lib_amd as og
    lib = og.load_library()
    assert len(og.predict_scale_table(1.2, 1)) == 0
    assert len(og.predict_scale_table(1.2, 16)) == 15
    buf = np.zeros(16, F32)
    for s, n in ((1.0, 8), (0.5, 8), (float("nan"), 8), (float("inf"), 8), (1.2, 0), (1.2, 17)):
        assert lib.orbgpu_predict_scale_table(og.C.c_float(s), n, og._p(buf)) == -3
    assert lib.orbgpu_predict_scale_table(og.C.c_float(1.2), 8, None) == -3
    # a step so large that float has no value above it: the table ends at FLT_MAX
    assert og.predict_scale_table(1e30, 4)[2] == np.finfo(F32).max


# ---- wrapper and ABI ----------------------------------------------------------------------------

def test_dtypes_match_the_header_structs_and_the_statuses_decided_before_any_launch():
    import orbslam3lib_amd as og
    assert og.RELOC_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_reloc_point") == 60
    assert og.RELOC_POSE_DTYPE.itemsize == _header_struct_bytes("orbgpu_reloc_pose") == 60 and og.RP_VALID == 1
    f = og.RELOC_POINT_DTYPE.fields
    assert [f[k][1] for k in ("pos", "angle", "min_distance", "max_distance", "flags", "desc")] == [0, 12, 16, 20, 24, 28]
    assert [og.RELOC_POSE_DTYPE.fields[k][1] for k in ("Rcw", "tcw", "Ow")] == [0, 36, 48]
    names = {"orbgpu_reloc_by_projection_batch", "orbgpu_download_reloc_matches", "orbgpu_predict_scale_table"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "reloc_by_projection") and hasattr(og.BatchExtractor, "reloc_matches")
    one = np.zeros(1, np.int32)
    assert lib.orbgpu_reloc_by_projection_batch(None, 1, og._p(one), None, None, None, None, None, 0,
                                                og.C.c_float(10), 100, 1, None) == -3
    assert lib.orbgpu_reloc_by_projection_batch(None, 0, None, None, None, None, None, None, 0,
                                                og.C.c_float(10), 100, 1, None) == -3
    assert lib.orbgpu_download_reloc_matches(None, 0, None, 0, None, None, None) == -3
    # the wrapper refuses lists that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, og.RELOC_POINT_DTYPE)
    poses = np.zeros(2, og.RELOC_POSE_DTYPE)
    with pytest.raises(ValueError):
        be.reloc_by_projection([0, 1], [pts], poses, K_)
    with pytest.raises(ValueError):
        be.reloc_by_projection([0, 1], [pts, pts], poses[:1], K_)
    with pytest.raises(ValueError):
        be.reloc_by_projection([0, 1], (pts, np.array([0, 3], np.int32)), poses, K_)
    with pytest.raises(ValueError):  # offsets beyond the points
        be.reloc_by_projection([0, 1], (pts, np.array([0, 2, 4], np.int32)), poses, K_)
    with pytest.raises(ValueError):
        be.reloc_by_projection([0, 1], [pts, pts], poses, K_, kp_block=[np.zeros(4, np.uint8)])


# ---- scenes -------------------------------------------------------------------------------------

# name -> (th, orb_dist, check_orientation, kp_block, pose kind, generator arguments)
CASES = {
    "th10_d100": (10.0, 100, True, False, "small", {}),
    "th3_d64": (3.0, 64, True, False, "small", {}),
    "th10_no_orientation": (10.0, 100, False, False, "small", {}),
    "th3_no_orientation": (3.0, 64, False, False, "small", {}),
    "kp_block": (10.0, 100, True, True, "small", {}),
    "rotated_translated": (10.0, 100, True, False, "large", {}),
    # many points on few keypoints, every keypoint of a window within ORBdist: the kept lists run dry
    "dense": (15.0, 160, True, False, "small", dict(n=4000, pool=100)),
}


def _scene_pose(kind):
    """-> (RELOC_POSE_DTYPE record, (Rcw, tcw))."""
    if kind == "small":
        a, axis, t = 0.02, np.array([0.0, 1.0, 0.0]), np.array([0.1, -0.05, 0.2])
    else:
        a, axis, t = 0.6, np.array([0.3, 0.8, -0.52]), np.array([1.5, -0.8, 2.5])
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx
    return _reloc_pose(R, t), (R, t)


def _scene_points(name, seed, xy, kps, desc, bounds, **kw):
    th, _, _, _, kind, gen = CASES[name]
    pose, Rt = _scene_pose(kind)
    args = dict(n=1000, seed=seed, th=th, bounds=[float(v) for v in bounds])
    args.update(gen)
    args.update(kw)
    return synth.reloc_points(xy, kps, desc, K_, Rt, **args), pose


def _scene_block(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.08).astype(np.uint8) * 3


def _restate(name, pts, pose, kps, desc, xy, bounds, cs, ci, blk, scale):
    th, orb_dist, check = CASES[name][:3]
    return _py_reloc(pts, pose, K_, xy, kps["octave"], kps["angle"], desc, bounds, cs, ci, blk, th, orb_dist, check, scale)


SKIPS = ("invalid", "out_min_x", "out_max_x", "out_min_y", "out_max_y", "too_near", "too_far", "not_finite")


def _scene_conditions(name, nm, hist, cnt, nlevels=8):
    assert nm >= 100 and cnt["events"] >= 100
    assert cnt["taken"] >= 5
    if CASES[name][2]:
        assert cnt["rejected"] >= 5 and hist.sum() + cnt["bin_out_of_range"] == cnt["events"]
    else:
        assert hist.sum() == 0 and nm == cnt["events"]
    for why in SKIPS:
        assert cnt[why] >= 1, why
    for lv in range(nlevels):
        assert cnt["level_%d" % lv] >= 1, lv
    assert cnt["clamped_high"] >= 1
    if CASES[name][3]:
        assert cnt["blocked"] >= 1
    if name == "dense":
        assert cnt["list_dry"] >= cnt["list_dry_matched"] >= 5


@pytest.fixture(scope="module")
def cpu_frame(oracle):
    L, _ = synth.stereo_pair(480, 640, 5)
    kl, dl, _ = oracle.extract(L, nfeatures=500)
    xy, b, _, cs, ci = oracle.undistort_grid(kl, K_, D_, 640, 480)
    return kl, dl.reshape(-1, 32), xy, b, cs, ci, oracle.scale_factors()[0]


@pytest.mark.parametrize("name", list(CASES))
def test_scene_exercises_every_rule(cpu_frame, name):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the
    oracle's extraction, meets every situation the GPU cases are there to compare."""
    kl, dl, xy, b, cs, ci, scale = cpu_frame
    pts, pose = _scene_points(name, 100, xy, kl, dl, b)
    blk = _scene_block(len(kl), 7) if CASES[name][3] else None
    m, nm, hist, cnt = _restate(name, pts, pose, kl, dl, xy, b, cs, ci, blk, scale)
    print(name, "nmatches", nm, dict(cnt))
    assert (m >= 0).sum() == nm
    _scene_conditions(name, nm, hist, cnt)


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


def _gpu_compare(env, name, pairs, packed=False, **kw):
    """pairs: (frame image, points, pose, kp_block or None) per pair of one call -> the restatement's results."""
    import orbslam3lib_amd as og
    be, imgs, b, scale = env
    th, orb_dist, check = CASES[name][:3]
    points = [p[1] for p in pairs]
    if packed:
        off = np.concatenate([[0], np.cumsum([len(x) for x in points])]).astype(np.int32)
        points = (np.concatenate(points), off)
    blks = [p[3] for p in pairs]
    if all(x is None for x in blks):
        blks = None
    else:
        blks = [np.zeros(1, np.uint8) if x is None else x for x in blks]
    be.reloc_by_projection([p[0] for p in pairs], points, np.array([p[2] for p in pairs], og.RELOC_POSE_DTYPE), K_,
                           kp_block=blks, th=th, orb_dist=orb_dist, check_orientation=check, **kw)
    out = []
    for q, (f, pts, pose, blk) in enumerate(pairs):
        kps, desc, xy, cs, ci = imgs[f]
        m, nm, hist, cnt = _restate(name, pts, pose, kps, desc, xy, b, cs, ci, blk, scale)
        gm, gnm, ghist = be.reloc_matches(q)
        np.testing.assert_array_equal(gm, m, err_msg="pair %d match" % q)
        assert gnm == nm, (q, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="pair %d histogram" % q)
        out.append((m, nm, hist, cnt))
    return out


def _gpu_scene(env, name, packed=False):
    _, imgs, b, _ = env
    pairs = []
    for f in range(4):
        kps, desc, xy, _, _ = imgs[f]
        pts, pose = _scene_points(name, 200 + f, xy, kps, desc, b)
        pairs.append((f, pts, pose, _scene_block(len(kps), 30 + f) if CASES[name][3] else None))
    res = _gpu_compare(env, name, pairs, packed)
    for _, nm, hist, cnt in res:
        _scene_conditions(name, nm, hist, cnt)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "dense"])
def test_gpu_reloc_by_projection_scenes(gpu_env, name):
    _gpu_scene(gpu_env, name)


@pytest.mark.gpu
def test_gpu_reloc_by_projection_points_plus_offsets(gpu_env):
    a = _gpu_scene(gpu_env, "th10_d100", packed=True)
    got = [gpu_env[0].reloc_matches(q) for q in range(4)]
    b = _gpu_scene(gpu_env, "th10_d100")
    for q in range(4):
        again = gpu_env[0].reloc_matches(q)
        assert np.array_equal(got[q][0], again[0]) and got[q][1] == again[1] and np.array_equal(got[q][2], again[2])
        assert a[q][1] == b[q][1]


@pytest.mark.gpu
def test_gpu_reloc_by_projection_one_frame_against_three_keyframes(gpu_env):
    """Relocalization: one frame in three pairs of one call that differ in points, pose and occupancy."""
    _, imgs, b, _ = gpu_env
    kps, desc, xy, _, _ = imgs[1]
    pairs = []
    for q, (name, n) in enumerate((("th10_d100", 1000), ("rotated_translated", 700), ("th10_d100", 333))):
        pts, pose = _scene_points(name, 500 + q, xy, kps, desc, b, n=n)
        pairs.append((1, pts, pose, (None, _scene_block(len(kps), 50), None)[q]))
    res = _gpu_compare(gpu_env, "th10_d100", pairs)
    assert res[0][1] >= 100 and len({r[1] for r in res}) == 3 and res[1][3]["blocked"] >= 1


@pytest.mark.gpu
def test_gpu_reloc_by_projection_dense_conflicts(gpu_env):
    """4000 points pooled on 100 keypoints of one frame: the kept candidate lists run dry and windows
    are walked again."""
    _, imgs, b, _ = gpu_env
    kps, desc, xy, _, _ = imgs[0]
    pts, pose = _scene_points("dense", 300, xy, kps, desc, b)
    assert len(pts) == 4000
    ((_, nm, _, cnt),) = _gpu_compare(gpu_env, "dense", [(0, pts, pose, None)])
    print("dense", nm, dict(cnt))
    assert nm >= 50 and cnt["list_dry"] >= cnt["list_dry_matched"] >= 5 and cnt["taken"] >= 1000


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(0, 1, 63), (64, 65, 129)])
def test_gpu_reloc_by_projection_replay_group_boundaries(gpu_env, sizes):
    """Pairs of exactly 0, 1, 63, 64, 65 and 129 points: the resolve pass replays 64 lanes at a time."""
    _, imgs, b, _ = gpu_env
    pairs = []
    for q, n in enumerate(sizes):
        kps, desc, xy, _, _ = imgs[q]
        pts, pose = _scene_points("th10_d100", 400 + n, xy, kps, desc, b, n=n, pool=20, invalid=0.0, outside=0.0,
                                  too_near=0.0, too_far=0.0, not_finite=0.0, over_top=0.0, flips=(0, 2, 5, 10))
        pairs.append((q, pts, pose, None))
    res = _gpu_compare(gpu_env, "th10_d100", pairs)
    for n, (m, nm, _, cnt) in zip(sizes, res):
        assert len(m) > 0 and (nm == 0 if n == 0 else cnt["events"] >= min(n, 10)), (n, nm, dict(cnt))
        assert n < 63 or cnt["taken"] >= 5


@pytest.mark.gpu
def test_gpu_reloc_by_projection_all_invalid_and_no_pairs(gpu_env):
    import orbslam3lib_amd as og
    be, imgs, b, _ = gpu_env
    kps, desc, xy, _, _ = imgs[2]
    pts, pose = _scene_points("th10_d100", 600, xy, kps, desc, b, n=200)
    pts["flags"] = 0
    ((m, nm, hist, cnt),) = _gpu_compare(gpu_env, "th10_d100", [(2, pts, pose, None)])
    assert nm == 0 and (m == -1).all() and len(m) == len(kps) and hist.sum() == 0 and cnt["invalid"] == 200
    be.reloc_by_projection([], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_)  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.reloc_matches(0)
    assert e.value.code == -3


@pytest.mark.gpu
def test_gpu_reloc_by_projection_ratio_on_a_table_threshold(gpu_env):
    """Points whose ratio max_distance / dist3D sits exactly on a step of the level, and one float above."""
    import orbslam3lib_amd as og
    _, imgs, b, _ = gpu_env
    kps, desc, xy, _, _ = imgs[0]
    steps = og.predict_scale_table(1.2, 8)
    pose, Rt = _scene_pose("small")
    Ow = np.asarray(pose["Ow"], F32)
    base = synth.reloc_points(xy, kps, desc, K_, Rt, n=400, seed=9, th=10.0, bounds=[float(v) for v in b], invalid=0.0,
                              outside=0.0, too_near=0.0, too_far=0.0, not_finite=0.0, flips=(0, 2, 5))
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
    ((_, nm, _, cnt),) = _gpu_compare(gpu_env, "th10_d100", [(0, pts, pose, None)])
    # (the few whose projection the position noise put outside the bounds predict no level)
    levels = [cnt["level_%d" % lv] for lv in range(8)]
    assert all(0 < got <= Counter(want)[lv] for lv, got in enumerate(levels)) and sum(levels) >= 0.9 * len(pts)
    assert sum(levels) + sum(cnt[why] for why in SKIPS) == len(pts) and nm >= 50


@pytest.mark.gpu
def test_gpu_reloc_by_projection_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    pose, _ = _scene_pose("small")
    pts = np.zeros(4, og.RELOC_POINT_DTYPE)
    poses = np.array([pose], og.RELOC_POSE_DTYPE)

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.reloc_by_projection(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.reloc_matches(0)
    assert e.value.code == -3
    assert code([0], [pts], poses, K_) == -3  # before undistort_grid
    be.undistort_grid(K_, D_)
    n1 = len(be.result(1)[0])
    assert code([2], [pts], poses, K_) == -3 and code([-1], [pts], poses, K_) == -3  # outside the gridded range
    assert code([0], [pts], poses, K_, orb_dist=-1) == -3 and code([0], [pts], poses, K_, orb_dist=256) == -3
    assert code([0], [pts], poses, K_, th=-1.0) == -3 and code([0], [pts], poses, K_, th=float("nan")) == -3
    assert code([0], [pts], poses, K_, th=float("inf")) == -3
    assert code([1], [pts], poses, K_, kp_block=[np.zeros(n1 - 1, np.uint8)]) == -3  # kp_stride below N
    assert code([1, 1], (pts, np.array([0, 4, 2], np.int32)), np.array([pose] * 2, og.RELOC_POSE_DTYPE), K_) == -3
    assert code([1] * 3, [pts] * 3, np.array([pose] * 3, og.RELOC_POSE_DTYPE), K_) == -3  # above the image capacity
    be.reloc_by_projection([1], [pts], poses, K_, kp_block=[np.zeros(n1, np.uint8)], orb_dist=255, th=0.0)
    m, nm, hist = be.reloc_matches(0)
    assert len(m) == n1 and nm == 0 and (m == -1).all()  # four invalid points
    with pytest.raises(og.OrbGpuError) as e:
        be.reloc_matches(1)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # caller capacity below N
        be.reloc_matches(0, cap=n1 - 1)
    assert e.value.code == -2
    be.close()
