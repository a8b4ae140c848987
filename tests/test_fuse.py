"""ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false) -- the
map-point fusion LocalMapping::SearchInNeighbors runs after CreateNewMapPoints
(cpp/src/ORBmatcher.cc:1155-1345) -- and its Sim3 overload (:1347-1462, LoopClosing::SearchAndFuse),
with KeyFrame::GetFeaturesInArea / IsInImage (KeyFrame.cc:706-755) and MapPoint::PredictScale
(MapPoint.cc:504-531), on pinhole keyframes.

The yardstick is _py_fuse below: a restatement written from those lines with np.float32 scalars
(every product and sum rounds to single, in the reference's order; the three comparisons against
double literals in double), the host libm's logf for the level, returning per point the decision
code (the reference's count_* counters), the lowest surviving distance and the keypoint fused onto,
per keypoint the first point that fused onto it, nFused, and a Counter of what the filters did.
CPU: a second, independent form (_brute_fuse: array arithmetic over the points, the level from
orbgpu_predict_scale_table, a scan of every gridded keypoint instead of the grid walk) against the
restatement on every scene; hand-built known answers on a tiny frame (every image bound and
invariance limit at the limit and one float beyond, the normal test at equality, the depth test at
zero, the octave band and its clamps, both chi-square limits, TH_LOW, equal distances, not-finite
positions, several points on one keypoint); conditions on the scenes the GPU cases use; the dtypes,
symbols and null-context statuses.
GPU: k_fuse_match against the restatement, equal on every output.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs Sophus, Eigen and the SLAM
stack; no fixtures ship for it) -- restatement only, as for the other matcher functions."""
from collections import Counter

import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_reloc_projection import _Tiny, _bits, _predict_scale, _reloc_pose, _scene_pose
from tests.test_track_projection import D_, F32, K_, MB, MBF, POP, _flip, _header_struct_bytes, _window

SKIPPED, NEG_DEPTH, NOT_IN_IMAGE, DISTANCE, NORMAL, EMPTY_WINDOW, ABOVE_TH_LOW, FUSED = range(1, 9)
CODES = {SKIPPED: "skipped", NEG_DEPTH: "neg_depth", NOT_IN_IMAGE: "not_in_image", DISTANCE: "distance",
         NORMAL: "normal", EMPTY_WINDOW: "empty_window", ABOVE_TH_LOW: "above_th_low", FUSED: "fused"}
TH_LOW = 50


def _py_fuse(pts, pose, K, xy, octv, desc, ur, bounds, cs, ci, skip, th, bf, sim3, scale, inv_sigma2,
             scale_factor=1.2, nlevels=8):
    """-> best_idx [n_points], best_dist [n_points], code [n_points], first [n_kp], nfused, Counter.
    ur: mvuRight or None (use_uright = 0); skip: the pair's row or None."""
    npts, nkp = len(pts), len(octv)
    xy = np.asarray(xy, F32)
    best_idx = np.full(npts, -1, np.int32)
    best_dist = np.full(npts, 256, np.int32)
    code = np.zeros(npts, np.uint8)
    first = np.full(nkp, -1, np.int32)
    claims = np.zeros(nkp, np.int32)
    cnt = Counter()
    b = np.asarray(bounds, F32)
    R, t, Ow = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Ow"))
    fx, fy, cx, cy = (F32(v) for v in K)
    nfused = 0
    for i, p in enumerate(pts):
        if not (int(p["flags"]) & 1) or (skip is not None and skip[i]):  # :1188-1203, :1372
            code[i] = SKIPPED
            continue
        X, Y, Z = (F32(v) for v in p["pos"])
        with np.errstate(all="ignore"):
            xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]  # :1206
            yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
            zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        if zc < F32(0.0):  # :1209
            code[i] = NEG_DEPTH
            continue
        with np.errstate(all="ignore"):
            invz = F32(1) / zc  # :1215
            u = fx * xc / zc + cx  # Pinhole.cpp:40-41
            v = fy * yc / zc + cy
        if not (u >= b[0] and u < b[1] and v >= b[2] and v < b[3]):  # KeyFrame.cc:752-755
            code[i] = NOT_IN_IMAGE
            continue
        with np.errstate(all="ignore"):
            ur_p = u - F32(bf) * invz  # :1226
            px, py, pz = X - Ow[0], Y - Ow[1], Z - Ow[2]  # :1230-1231
            dist3d = np.sqrt((px * px + py * py) + pz * pz)
            lo, hi = F32(0.8) * F32(p["min_distance"]), F32(1.2) * F32(p["max_distance"])  # MapPoint.cc:504-514
            ratio = F32(p["max_distance"]) / dist3d  # MapPoint.cc:521
        if not np.isfinite(dist3d) or dist3d < lo or dist3d > hi or not np.isfinite(ratio):  # :1234 + the deviation
            code[i] = DISTANCE
            continue
        nx, ny, nz = (F32(w) for w in p["normal"])
        with np.errstate(all="ignore"):
            dot = (px * nx + py * ny) + pz * nz
        if float(dot) < 0.5 * float(dist3d):  # :1242, in double
            code[i] = NORMAL
            continue
        level, raw = _predict_scale(ratio, scale_factor, nlevels)  # :1248
        cnt["level_%d" % level] += 1
        cnt["clamped_low"] += raw < 0
        cnt["clamped_high"] += raw >= nlevels
        radius = F32(th) * F32(scale[level])  # :1251
        cand = _window(xy, octv, cs, ci, b, u, v, radius, -1, -1)  # KeyFrame::GetFeaturesInArea: no level filter
        if not cand:  # :1255
            code[i] = EMPTY_WINDOW
            continue
        best, bi = (2 ** 31 - 1 if sim3 else 256), -1  # :1265 / :1422
        for k in cand:
            o = int(octv[k])
            if o < level - 1 or o > level:  # :1276
                cnt["octave"] += 1
                continue
            if not sim3:
                with np.errstate(all="ignore"):
                    ex, ey = u - xy[k, 0], v - xy[k, 1]
                    if ur is not None and ur[k] >= 0:  # :1279-1292
                        er = ur_p - F32(ur[k])
                        e2 = (ex * ex + ey * ey) + er * er
                        out = float(e2 * F32(inv_sigma2[o])) > 7.8
                        cnt["chi_stereo"] += out
                        cnt["chi_stereo_seen"] += 1
                    else:  # :1293-1303
                        e2 = ex * ex + ey * ey
                        out = float(e2 * F32(inv_sigma2[o])) > 5.99
                        cnt["chi_mono"] += out
                        cnt["chi_mono_seen"] += 1
                if out:
                    continue
            d = int(POP[np.bitwise_xor(p["desc"], desc[k])].sum())
            if d < best:  # :1311
                best, bi = d, k
        best_dist[i] = min(best, 256)
        if best <= TH_LOW:  # :1319
            code[i] = FUSED
            best_idx[i] = bi
            if first[bi] < 0:  # the point every later claimant meets as pMPinKF (:1321, :1446)
                first[bi] = i
            claims[bi] += 1
            nfused += 1
        else:
            code[i] = ABOVE_TH_LOW
    cnt["multi_claimed"] = int((claims >= 2).sum())
    for c, name in CODES.items():
        cnt[name] = int((code == c).sum())
    return best_idx, best_dist, code, first, nfused, cnt


def _brute_fuse(pts, pose, K, xy, octv, desc, ur, bounds, ci, skip, th, bf, sim3, scale, inv_sigma2, steps):
    """The second form: array arithmetic over all points at once, the level as the number of
    orbgpu_predict_scale_table entries below the ratio, and per point a scan of every gridded keypoint
    with the box test instead of the grid walk -> code, best_dist, best_idx, unique (the lowest
    distance is held by one keypoint)."""
    n = len(pts)
    xy = np.asarray(xy, F32)
    b = np.asarray(bounds, F32)
    R, t, Ow = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Ow"))
    fx, fy, cx, cy = (F32(v) for v in K)
    P = np.asarray(pts["pos"], F32)
    N = np.asarray(pts["normal"], F32)
    gridded = np.zeros(len(octv), bool)
    gridded[ci] = True
    kk = np.flatnonzero(gridded)
    code = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        cam = [((R[3 * r] * P[:, 0] + R[3 * r + 1] * P[:, 1]) + R[3 * r + 2] * P[:, 2]) + t[r] for r in range(3)]
        u = fx * cam[0] / cam[2] + cx
        v = fy * cam[1] / cam[2] + cy
        urp = u - F32(bf) * (F32(1) / cam[2])
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
    stage = [(skipped, SKIPPED), (cam[2] < 0, NEG_DEPTH), (~inside, NOT_IN_IMAGE), (~in_range, DISTANCE), (~facing, NORMAL)]
    for mask, c in stage:
        code[(code == 0) & mask] = c
    best_dist = np.full(n, 256, np.int32)
    best_idx = np.full(n, -1, np.int32)
    unique = np.zeros(n, bool)
    for i in np.flatnonzero(code == 0):
        r = F32(th) * F32(scale[level[i]])
        with np.errstate(all="ignore"):
            dx, dy = xy[kk, 0] - u[i], xy[kk, 1] - v[i]
            box = (np.abs(dx) < r) & (np.abs(dy) < r)
        if not box.any():
            code[i] = EMPTY_WINDOW
            continue
        k = kk[box]
        o = octv[k]
        keep = (o >= level[i] - 1) & (o <= level[i])
        if not sim3:
            with np.errstate(all="ignore"):
                ex, ey = u[i] - xy[k, 0], v[i] - xy[k, 1]
                kr = np.asarray(ur, F32)[k] if ur is not None else np.full(len(k), -1, F32)
                er = urp[i] - kr
                mono = (ex * ex + ey * ey) * np.asarray(inv_sigma2, F32)[o]
                ster = ((ex * ex + ey * ey) + er * er) * np.asarray(inv_sigma2, F32)[o]
                keep &= np.where(kr >= 0, ~(ster.astype(np.float64) > 7.8), ~(mono.astype(np.float64) > 5.99))
        k = k[keep]
        if len(k):
            d = POP[np.bitwise_xor(desc[k], pts["desc"][i][None, :])].sum(1)
            best_dist[i] = d.min()
            unique[i] = (d == d.min()).sum() == 1
            if d.min() <= TH_LOW:
                best_idx[i] = k[np.argmin(d)]
        code[i] = FUSED if best_dist[i] <= TH_LOW else ABOVE_TH_LOW
    return code, best_dist, best_idx, unique


# ---- hand-built frames --------------------------------------------------------------------------

SC = (F32(1.2) ** np.arange(8)).astype(F32)  # stands for mvScaleFactors in the hand-built cases
IS2 = (F32(1) / (SC * SC)).astype(F32)        # and for mvInvLevelSigma2


def _run(T, pts, th=3.0, bf=0.0, ur=None, sim3=False, skip=None, pose=None):
    return _py_fuse(np.atleast_1d(pts), _reloc_pose() if pose is None else pose, T.K, T.xy, T.octv, T.desc, ur, T.B,
                    T.cs, T.ci, skip, th, bf, sim3, SC, IS2)


def _aim(x, y, desc, level=0, z=2.0, valid=True):
    """A map point that projects to (x, y) under the identity pose and _Tiny.K, seen head-on, whose
    distance predicts `level`."""
    import orbslam3lib_amd as og
    p = np.zeros((), og.FUSE_POINT_DTYPE)
    pos = np.array((x / _Tiny.K[0] * z, y / _Tiny.K[1] * z, z))
    p["pos"] = pos
    dist = float(np.linalg.norm(pos))
    p["normal"] = pos / dist
    p["max_distance"] = dist * (0.95 if level == 0 else 1.2 ** (level - 0.5))
    p["min_distance"] = p["max_distance"] / 1.2 ** 7
    p["flags"], p["desc"] = (og.FP_VALID if valid else 0), desc
    return p


def _on_axis(z, desc, mn=0.01, mx=None, normal=(0.0, 0.0, 1.0), x=0.0, y=0.0):
    """pos = (x, y, z) as given (u = 512 x / z exactly where the quotients are exact), level 0."""
    import orbslam3lib_amd as og
    p = np.zeros((), og.FUSE_POINT_DTYPE)
    p["pos"] = (x, y, z)
    p["normal"] = normal
    p["min_distance"] = mn
    p["max_distance"] = float(np.linalg.norm(p["pos"])) * 0.95 if mx is None else mx
    p["flags"], p["desc"] = og.FP_VALID, desc
    return p


@pytest.mark.parametrize("axis,bound,inside", [(0, -320.0, 1), (0, 320.0, -1), (1, -240.0, 1), (1, 240.0, -1)])
def test_the_image_test_is_half_open(axis, bound, inside):
    """At mnMin passes, one float below fails; one float below mnMax passes, at mnMax fails (u = 512 x / 1 is exact).
    The last grid cell ends 5 px inside mnMax, so the keypoint sits 8 px inside and the search runs at th 10, in the
    form without the chi-square gate: both overloads share the image test."""
    kp = [0.0, 0.0]
    kp[axis] = bound + 8 * inside
    T = _Tiny(extra=[(kp[0], kp[1], 0, None)])
    if inside > 0:
        cases = ((F32(bound), FUSED), (np.nextafter(F32(bound), F32(-1e9)), NOT_IN_IMAGE))
    else:
        cases = ((np.nextafter(F32(bound), F32(0)), FUSED), (F32(bound), NOT_IN_IMAGE))
    for target, want in cases:
        xyz = [0.0, 0.0, 1.0]
        xyz[axis] = target / F32(512)
        p = _on_axis(1.0, T.desc[40], x=xyz[0], y=xyz[1])
        p["normal"] = p["pos"] / np.linalg.norm(p["pos"])
        assert F32(512) * p["pos"][axis] / F32(1) + F32(0) == target
        bi, bd, code, first, nf, _ = _run(T, p, th=10.0, sim3=True)
        assert code[0] == want and nf == (want == FUSED) and bi[0] == (40 if want == FUSED else -1)
        assert bd[0] == (0 if want == FUSED else 256) and first[40] == (0 if want == FUSED else -1)


def test_each_invariance_limit_at_the_limit_passes_and_one_float_beyond_is_distance():
    """On the optical axis under the identity pose dist3D = sqrtf(z * z) = z exactly."""
    T = _Tiny(extra=[(1.0, 0.0, 0, None)])
    mx = F32(3.3)
    far = F32(1.2) * mx
    assert _run(T, _on_axis(far, T.desc[40], mx=mx))[2][0] == FUSED
    assert _run(T, _on_axis(np.nextafter(far, F32(1e9)), T.desc[40], mx=mx))[2][0] == DISTANCE
    mn = F32(2.7)
    near = F32(0.8) * mn
    assert _run(T, _on_axis(near, T.desc[40], mn=mn, mx=near))[2][0] == FUSED
    out = _run(T, _on_axis(np.nextafter(near, F32(0)), T.desc[40], mn=mn, mx=near))
    assert out[2][0] == DISTANCE and out[1][0] == 256 and out[0][0] == -1


def test_the_normal_test_at_equality_passes_and_one_float_less_is_normal():
    """PO = (0, 0, 2), n = (0, 0, nz): the dot product 2 nz is exact; 0.5 * dist3D = 1."""
    T = _Tiny(extra=[(1.0, 0.0, 0, None)])
    assert _run(T, _on_axis(2.0, T.desc[40], normal=(0, 0, 0.5)))[2][0] == FUSED
    assert _run(T, _on_axis(2.0, T.desc[40], normal=(0, 0, np.nextafter(F32(0.5), F32(0)))))[2][0] == NORMAL
    assert _run(T, _on_axis(2.0, T.desc[40], normal=(0.9, 0.9, 0.5)))[2][0] == FUSED  # PO.x = PO.y = 0
    assert _run(T, _on_axis(2.0, T.desc[40], normal=(0, 0, -1.0)))[2][0] == NORMAL
    # a NaN normal fails no comparison, as in the reference
    assert _run(T, _on_axis(2.0, T.desc[40], normal=(0, 0, np.nan)))[2][0] == FUSED


def test_depth_one_float_below_zero_is_neg_depth_and_zero_is_not_in_image():
    """zc = Z + tcw.z with tcw.z = 1: Z = -1 gives 0, the float below -1 a negative zc."""
    T = _Tiny()
    pose = _reloc_pose(t=(0.0, 0.0, 1.0))
    d = T.desc[0]
    assert _run(T, _on_axis(np.nextafter(F32(-1), F32(-2)), d), pose=pose)[2][0] == NEG_DEPTH
    assert _run(T, _on_axis(-1.0, d), pose=pose)[2][0] == NOT_IN_IMAGE          # 0 / 0
    assert _run(T, _on_axis(-1.0, d, x=0.25), pose=pose)[2][0] == NOT_IN_IMAGE  # x / 0 = inf
    neg_zero = _on_axis(-0.0, d, x=0.25)  # zc = -0.0 is not < 0
    assert _run(T, neg_zero)[2][0] == NOT_IN_IMAGE
    assert _run(T, _on_axis(-2.0, d))[2][0] == NEG_DEPTH


def _octaves_frame():
    """Eight keypoints of octaves 0..7 within 1.4 px of the centre."""
    T = _Tiny()
    T.xy = np.array([(0.2 * o - 0.7, 0.0) for o in range(8)], F32)
    T.octv = np.arange(8, dtype=np.int32)
    T.ang = np.zeros(8, F32)
    T.desc = np.random.default_rng(5).integers(0, 256, (8, 32), dtype=np.uint8)
    from tests.test_track_projection import _grid
    T.cs, T.ci = _grid(T.xy, T.B)
    return T


def test_the_octave_band_is_level_minus_one_to_level_and_the_clamps():
    T = _octaves_frame()

    def sees(ratio, sim3=False):
        out = []
        for target in range(8):
            p = _on_axis(2.0, T.desc[target], mn=0.0, mx=F32(2.0) * F32(ratio))
            bi, bd, code, _, nf, cnt = _run(T, p, sim3=sim3)
            assert code[0] in (FUSED, ABOVE_TH_LOW)  # never EMPTY_WINDOW: the area holds all eight
            if code[0] == FUSED:
                assert bi[0] == target and bd[0] == 0
                out.append(target)
            else:
                assert bi[0] == -1
        return out, [k for k in cnt if k.startswith("level_")][0], cnt["clamped_low"], cnt["clamped_high"]
    assert sees(0.95) == ([0], "level_0", 0, 0)       # level 0: octaves -1 .. 0
    assert sees(1.0) == ([0], "level_0", 0, 0)
    assert sees(1.01) == ([0, 1], "level_1", 0, 0)
    assert sees(1.2 ** 2.5) == ([2, 3], "level_3", 0, 0)   # octave level + 1 = 4 is filtered, level - 1 = 2 taken
    assert sees(1.2 ** 2.5, sim3=True) == ([2, 3], "level_3", 0, 0)
    assert sees(1.2 ** 6.5) == ([6, 7], "level_7", 0, 0)
    assert sees(1.2 ** 8.5) == ([6, 7], "level_7", 0, 1)   # nScale = 9, clamped from above
    assert sees(1 / 1.2)[:2] == ([0], "level_0")            # the furthest point the gate lets through
    # every candidate filtered: above TH_LOW with nothing surviving, not an empty window
    p = _on_axis(2.0, T.desc[5], mn=0.0, mx=F32(2.0) * F32(1.2 ** 2.5))
    bi, bd, code, first, nf, cnt = _run(T, p)
    assert code[0] == ABOVE_TH_LOW and bd[0] > TH_LOW and cnt["octave"] == 6
    T.octv[:] = 5
    bi, bd, code, first, nf, cnt = _run(T, p)
    assert code[0] == ABOVE_TH_LOW and bd[0] == 256 and bi[0] == -1 and nf == 0 and (first == -1).all()
    # the Sim3 overload's INT_MAX start: a 256-bit complement becomes its bestIdx and still cannot fuse; 256 stands for it
    T.octv[:] = 3
    T.desc[:] = 255
    bi, bd, code, _, nf, _ = _run(T, _on_axis(2.0, _bits(), mn=0.0, mx=F32(2.0) * F32(1.2 ** 2.5)), sim3=True)
    assert code[0] == ABOVE_TH_LOW and bd[0] == 256 and bi[0] == -1 and nf == 0


def _last_at_or_below(limit, f):
    """The largest float32 e in [1, 4] with float(f(e)) <= limit (f increasing), and the next float."""
    lo, hi = F32(1.0), F32(4.0)
    assert float(f(lo)) <= limit < float(f(hi))
    a, b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while b - a > 1:
        m = (a + b) // 2
        if float(f(np.uint32(m).view(F32))) <= limit:
            a = m
        else:
            b = m
    return np.uint32(a).view(F32), np.uint32(b).view(F32)


def test_both_chi_square_limits_and_sim3_ignoring_them():
    """A keypoint at the origin, the point at u = e exactly, v = 0: ex = e, ey = 0.  Monocular: e2 = e * e against
    5.99; stereo with bf = 0 and mvuRight = 0: er = e, e2 = e * e + e * e against 7.8."""
    T = _Tiny(extra=[(0.0, 0.0, 0, None)])
    ur = np.full(41, -1, F32)
    mono = _last_at_or_below(5.99, lambda e: e * e * IS2[0])
    assert float(mono[0] * mono[0]) <= 5.99 < float(mono[1] * mono[1]) and mono[1] == np.nextafter(mono[0], F32(9))
    for use in (None, ur):  # without mvuRight, and with a keypoint that has no right coordinate
        for e, want in zip(mono, (FUSED, ABOVE_TH_LOW)):
            p = _on_axis(1.0, T.desc[40], x=e / F32(512))
            bi, bd, code, _, _, cnt = _run(T, p, ur=use)
            assert code[0] == want and cnt["chi_mono"] == (want != FUSED) and bd[0] == (0 if want == FUSED else 256)
            assert _run(T, p, ur=use, sim3=True)[2][0] == FUSED
    ur[40] = 0.0  # >= 0: a right coordinate
    ster = _last_at_or_below(7.8, lambda e: (e * e + e * e) * IS2[0])
    assert ster[0] < mono[0]
    for e, want in zip(ster, (FUSED, ABOVE_TH_LOW)):
        p = _on_axis(1.0, T.desc[40], x=e / F32(512))
        bi, bd, code, _, _, cnt = _run(T, p, ur=ur)
        assert code[0] == want and cnt["chi_stereo"] == (want != FUSED) and cnt["chi_mono_seen"] == 0
        assert _run(T, p, ur=ur, sim3=True)[2][0] == FUSED
        assert _run(T, p, ur=None)[2][0] == FUSED  # use_uright = 0: the monocular limit, which it is within
    # bf enters through ur = u - bf / zc: the same point with a disparity the keypoint does not share
    p = _on_axis(1.0, T.desc[40], x=F32(1) / F32(512))
    assert _run(T, p, ur=ur, bf=0.0)[2][0] == FUSED and _run(T, p, ur=ur, bf=4.0)[2][0] == ABOVE_TH_LOW
    # a higher octave: the limit scales with mvInvLevelSigma2
    T.octv[40] = 1
    p = _on_axis(2.0, T.desc[40], x=F32(2.9) * F32(2) / F32(512), mn=0.0, mx=F32(2.0) * F32(1.1))
    assert _run(T, p, th=3.0)[2][0] == FUSED and float(F32(2.9) * F32(2.9) * IS2[1]) < 5.99 < 2.9 * 2.9


def test_distance_50_fuses_and_51_does_not():
    Z = _bits()
    for nbits, want in ((50, FUSED), (51, ABOVE_TH_LOW)):
        T = _Tiny(extra=[(0.0, 0.0, 0, _bits((0, nbits)))])
        bi, bd, code, first, nf, _ = _run(T, _aim(0, 0, Z))
        assert code[0] == want and bd[0] == nbits and nf == (want == FUSED) and bi[0] == (40 if want == FUSED else -1)


def test_an_equal_distance_keeps_the_earlier_window_position():
    Z = _bits()
    # window order: grid column, then row, then index: the keypoint further left comes first whatever its index
    T = _Tiny(extra=[(6.0, 0.0, 0, _bits((0, 7))), (-6.0, 0.0, 0, _bits((7, 14)))])
    bi, bd, code, _, _, _ = _run(T, _aim(0, 0, Z), th=8.0, sim3=True)
    assert code[0] == FUSED and bi[0] == 41 and bd[0] == 7
    # in one cell the lower index comes first
    T = _Tiny(extra=[(1.0, 0.0, 0, _bits((0, 7))), (0.5, 0.0, 0, _bits((7, 14)))])
    bi, _, code, _, _, _ = _run(T, _aim(0, 0, Z))
    assert code[0] == FUSED and bi[0] == 40


def test_not_finite_positions():
    T = _Tiny()
    d = T.desc[0]
    nan = _aim(-260, -180, d)
    nan["pos"][0] = np.nan
    assert _run(T, nan)[2][0] == NOT_IN_IMAGE
    nanz = _aim(-260, -180, d)
    nanz["pos"][2] = np.nan  # zc < 0 is false for a NaN
    assert _run(T, nanz)[2][0] == NOT_IN_IMAGE
    huge = _aim(0, 0, d)
    huge["pos"] = (0, 0, 1e30)  # projects to the centre; dist3D overflows
    huge["max_distance"] = np.inf
    assert _run(T, huge)[2][0] == DISTANCE
    inf = _aim(-260, -180, d)
    inf["max_distance"] = np.inf  # passes the gate, the ratio is not finite
    out = _run(T, inf)
    assert out[2][0] == DISTANCE and out[0][0] == -1 and out[1][0] == 256 and out[4] == 0


def test_three_points_on_one_keypoint_all_fuse_and_first_is_the_lowest():
    T = _Tiny()
    d = T.desc[7]
    x, y = T.xy[7]
    pts = np.array([_aim(x, y, d, valid=False), _aim(x, y, _flip(d, 20)), _aim(T.xy[3, 0], T.xy[3, 1], T.desc[3]),
                    _aim(x + 1, y, d), _aim(x, y - 1, _flip(d, 5))])
    bi, bd, code, first, nf, cnt = _run(T, pts)
    assert list(code) == [SKIPPED, FUSED, FUSED, FUSED, FUSED] and list(bi) == [-1, 7, 3, 7, 7] and list(bd) == [256, 20, 0, 0, 5]
    assert nf == 4 and first[7] == 1 and first[3] == 2 and (np.delete(first, [3, 7]) == -1).all() and cnt["multi_claimed"] == 1
    # the pair's skip row does what the flag does
    skip = np.array([0, 1, 0, 0, 0], np.uint8)
    bi, bd, code, first, nf, _ = _run(T, pts, skip=skip)
    assert list(code) == [SKIPPED, SKIPPED, FUSED, FUSED, FUSED] and nf == 3 and first[7] == 3


# ---- wrapper and ABI ----------------------------------------------------------------------------

def test_dtypes_match_the_header_structs_and_the_symbols_are_exported():
    import orbslam3lib_amd as og
    assert og.FUSE_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_fuse_point") == 68 and og.FP_VALID == 1
    f = og.FUSE_POINT_DTYPE.fields
    assert [f[k][1] for k in ("pos", "normal", "min_distance", "max_distance", "flags", "desc")] == [0, 12, 24, 28, 32, 36]
    assert og.RELOC_POSE_DTYPE.itemsize == _header_struct_bytes("orbgpu_reloc_pose") == 60
    txt = open(og.os.path.join(og.os.path.dirname(og.HERE), "include", "orbgpu.h")).read()
    for name, value in (("SKIPPED", SKIPPED), ("NEG_DEPTH", NEG_DEPTH), ("NOT_IN_IMAGE", NOT_IN_IMAGE), ("DISTANCE", DISTANCE),
                        ("NORMAL", NORMAL), ("EMPTY_WINDOW", EMPTY_WINDOW), ("ABOVE_TH_LOW", ABOVE_TH_LOW), ("FUSED", FUSED),
                        ("MAX_POINTS", 65536)):
        assert "#define ORBGPU_FUSE_%s %d\n" % (name, value) in txt
        assert getattr(og, "FUSE_" + name) == value
    names = {"orbgpu_fuse_batch", "orbgpu_download_fuse_matches"}
    assert names <= set(og.EXPORTED)
    lib = og.load_library()
    assert all(hasattr(lib, n) for n in names)
    assert hasattr(og.BatchExtractor, "fuse") and hasattr(og.BatchExtractor, "fuse_matches")
    one = np.zeros(1, np.int32)
    assert lib.orbgpu_fuse_batch(None, 1, og._p(one), og._p(one), 1, None, None, None, None, None, 0, og.C.c_float(3),
                                 og.C.c_float(0), 0, 0, None) == -3
    assert lib.orbgpu_fuse_batch(None, 0, None, None, 0, None, None, None, None, None, 0, og.C.c_float(3),
                                 og.C.c_float(0), 0, 0, None) == -3
    assert lib.orbgpu_download_fuse_matches(None, 0, None, None, None, 0, None, 0, None, None, None) == -3
    # the wrapper refuses lists that do not give one entry per pair before any device call
    be = object.__new__(og.BatchExtractor)
    pts = np.zeros(3, og.FUSE_POINT_DTYPE)
    poses = np.zeros(2, og.RELOC_POSE_DTYPE)
    with pytest.raises(ValueError):
        be.fuse([0, 1], [0], [pts], poses, K_)
    with pytest.raises(ValueError):
        be.fuse([0, 1], [0, 0], [pts], poses[:1], K_)
    with pytest.raises(ValueError):
        be.fuse([0, 1], [0, 0], [pts], poses, K_, skip=[np.zeros(3, np.uint8)])
    with pytest.raises(ValueError):  # offsets beyond the points
        be.fuse([0, 1], [0, 1], (pts, np.array([0, 2, 4], np.int32)), poses, K_)


# ---- scenes -------------------------------------------------------------------------------------

# name -> (th, use_uright, sim3, generator arguments)
CASES = {
    "base": (3.0, False, False, {}),
    "stereo": (3.0, True, False, {}),
    "sim3": (3.0, False, True, {}),
    "coarse": (4.0, False, False, dict(z_range=(10.0, 120.0), over_top=0.05)),
    "dense": (3.0, False, False, dict(n=3000, pool=150)),
}


def _scene_points(name, seed, xy, kps, desc, ur, bounds, **kw):
    th, use_ur, _, gen = CASES[name]
    pose, Rt = _scene_pose("small")
    args = dict(n=1000, seed=seed, th=th, bounds=[float(v) for v in bounds])
    if use_ur:
        args.update(uright=ur, bf=MBF)
    args.update(gen)
    args.update(kw)
    return synth.fuse_points(xy, kps, desc, K_, Rt, **args), pose


def _restate(name, pts, pose, kps, desc, xy, ur, bounds, cs, ci, skip, tabs):
    th, use_ur, sim3, _ = CASES[name]
    return _py_fuse(pts, pose, K_, xy, kps["octave"], desc, ur if use_ur else None, bounds, cs, ci, skip, th, MBF, sim3,
                    tabs[0], tabs[3])


def _scene_conditions(name, nfused, cnt):
    """Conditions on the inputs.  The chi-square gates exist where the scene runs them: none under sim3, the
    stereo one only with use_uright (where keypoints without a right coordinate still take the monocular one)."""
    for c in CODES.values():
        assert cnt[c] >= 5, (c, dict(cnt))
    assert nfused == cnt["fused"] >= 100
    _, use_ur, sim3, _ = CASES[name]
    assert cnt["chi_mono"] >= (0 if sim3 else 5) and cnt["chi_stereo"] >= (5 if use_ur else 0), dict(cnt)
    if sim3:
        assert cnt["chi_mono_seen"] == cnt["chi_stereo_seen"] == 0
    if not use_ur:
        assert cnt["chi_stereo_seen"] == 0
    assert cnt["octave"] >= 5 and cnt["multi_claimed"] >= (20 if name == "dense" else 1)


@pytest.fixture(scope="module")
def cpu_frame(oracle):
    L, R = synth.stereo_pair(480, 640, 5)
    kl, dl, _ = oracle.extract(L, nfeatures=500)
    kr, dr, _ = oracle.extract(R, nfeatures=500)
    ur = oracle.stereo_matches(kl, dl, kr, dr, oracle.pyramid(L), oracle.pyramid(R), MBF, MB)[0]
    xy, b, _, cs, ci = oracle.undistort_grid(kl, K_, D_, 640, 480)
    return kl, dl.reshape(-1, 32), xy, ur, b, cs, ci, oracle.scale_factors()


@pytest.fixture(scope="module")
def cpu_scenes(cpu_frame):
    """name -> (points, pose, the restatement's outputs), computed once."""
    kl, dl, xy, ur, b, cs, ci, tabs = cpu_frame
    out = {}
    for name in CASES:
        pts, pose = _scene_points(name, 100, xy, kl, dl, ur, b)
        out[name] = (pts, pose, _restate(name, pts, pose, kl, dl, xy, ur, b, cs, ci, None, tabs))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_scene_exercises_every_rule(cpu_scenes, name):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the oracle's
    extraction, meets every situation the GPU cases are there to compare."""
    pts, _, (bi, bd, code, first, nf, cnt) = cpu_scenes[name]
    print(name, "nfused", nf, dict(cnt))
    assert (bi >= 0).sum() == nf and ((first >= 0).sum() + cnt["multi_claimed"]) <= nf
    assert set(np.flatnonzero(first >= 0)) == set(bi[bi >= 0])
    _scene_conditions(name, nf, cnt)


@pytest.mark.parametrize("name", list(CASES))
def test_brute_force_scan_agrees_with_the_restatement(cpu_frame, cpu_scenes, name):
    import orbslam3lib_amd as og
    kl, dl, xy, ur, b, cs, ci, tabs = cpu_frame
    th, use_ur, sim3, _ = CASES[name]
    pts, pose, (bi, bd, code, first, nf, cnt) = cpu_scenes[name]
    c2, bd2, bi2, unique = _brute_fuse(pts, pose, K_, xy, kl["octave"], dl, ur if use_ur else None, b, ci, None, th, MBF,
                                       sim3, tabs[0], tabs[3], og.predict_scale_table(1.2, 8))
    np.testing.assert_array_equal(c2, code)
    np.testing.assert_array_equal(bd2, bd)
    assert unique.sum() >= 100
    np.testing.assert_array_equal(bi2[unique], bi[unique])


# ---- GPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_env(oracle):
    """Two 640x480 stereo pairs at 1000 features, extracted, stereo-matched and gridded once."""
    import orbslam3lib_amd as og
    pairs = [synth.stereo_pair(480, 640, 90 + s) for s in range(2)]
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=16)
    be.upload(np.stack([im for pr in pairs for im in pr]))
    be.run()
    be.stereo_matches(MBF, MB)
    be.undistort_grid(K_, D_)
    be.synchronize()
    imgs = []
    for i in range(4):
        kps, desc, _ = be.result(i)
        xy, _, cs, ci = be.grid_result(i)
        imgs.append((kps, desc.reshape(-1, 32), xy, cs, ci, be.stereo_result(i // 2)[0] if i % 2 == 0 else None))
    b = oracle.undistort_grid(imgs[0][0], K_, D_, 640, 480)[1]
    yield be, imgs, b, oracle.scale_factors()
    be.close()


def _gpu_compare(env, name, frames, lists, point_lists, poses, skips=None):
    """One fuse call; every pair against the restatement -> the restatement's outputs per pair."""
    import orbslam3lib_amd as og
    be, imgs, b, tabs = env
    th, use_ur, sim3, _ = CASES[name]
    be.fuse(frames, lists, point_lists, np.array(poses, og.RELOC_POSE_DTYPE), K_, skip=skips, th=th, bf=MBF,
            use_uright=use_ur, sim3=sim3)
    out = []
    for q, (f, l) in enumerate(zip(frames, lists)):
        kps, desc, xy, cs, ci, ur = imgs[f]
        want = _restate(name, point_lists[l], poses[q], kps, desc, xy, ur, b, cs, ci, None if skips is None else skips[q], tabs)
        _same(be.fuse_matches(q), want, len(kps), q)
        out.append(want)
    return out


def _same(got, want, nkp, q=0):
    gbi, gbd, gcode, gfirst, gnf = got
    bi, bd, code, first, nf = want[:5]
    assert len(gfirst) == nkp == len(first) and len(gbi) == len(gbd) == len(gcode) == len(bi)
    np.testing.assert_array_equal(gcode, code, err_msg="pair %d code" % q)
    np.testing.assert_array_equal(gbd, bd, err_msg="pair %d best_dist" % q)
    np.testing.assert_array_equal(gbi, bi, err_msg="pair %d best_idx" % q)
    np.testing.assert_array_equal(gfirst, first, err_msg="pair %d first" % q)
    assert gnf == nf, (q, gnf, nf)


def _frame_points(env, name, f, seed, **kw):
    _, imgs, b, _ = env
    kps, desc, xy, _, _, ur = imgs[f]
    return _scene_points(name, seed, xy, kps, desc, ur, b, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_fuse_scenes(gpu_env, name):
    pts, poses = zip(*[_frame_points(gpu_env, name, f, 200 + f) for f in (0, 2)])
    res = _gpu_compare(gpu_env, name, [0, 2], [0, 1], list(pts), list(poses))
    for r in res:
        _scene_conditions(name, r[4], r[5])
    if name == "dense":  # the conflicts again: the atomics commute, so the outputs are the same
        be = gpu_env[0]
        a = [be.fuse_matches(q) for q in range(2)]
        _gpu_compare(gpu_env, name, [0, 2], [0, 1], list(pts), list(poses))
        for q in range(2):
            _same(be.fuse_matches(q), a[q], len(a[q][3]), q)
        assert all(r[5]["multi_claimed"] >= 20 for r in res)


@pytest.mark.gpu
def test_gpu_fuse_one_list_against_three_frames(gpu_env):
    """SearchInNeighbors' forward leg: the current keyframe's points, uploaded once, into three neighbours
    with their own poses and IsInKeyFrame rows; the same as three calls with the row folded into the flags."""
    import orbslam3lib_amd as og
    be = gpu_env[0]
    pts, pose = _frame_points(gpu_env, "base", 1, 300)
    pose2, _ = _scene_pose("large")
    pose3 = _reloc_pose(np.eye(3), (0.02, 0.01, -0.05))
    poses = [pose, pose2, pose3]
    rng = np.random.default_rng(8)
    skips = [(rng.random(len(pts)) < s).astype(np.uint8) * 5 for s in (0.1, 0.0, 0.5)]
    res = _gpu_compare(gpu_env, "base", [1, 0, 3], [0, 0, 0], [pts], poses, skips)
    assert res[0][4] >= 100 and res[2][5]["skipped"] >= 400
    shared = [be.fuse_matches(q) for q in range(3)]
    for q, f in enumerate((1, 0, 3)):
        folded = pts.copy()
        folded["flags"] = np.where(skips[q] != 0, 0, folded["flags"])
        be.fuse([f], [0], [folded], np.array([poses[q]], og.RELOC_POSE_DTYPE), K_, th=3.0, bf=MBF)
        _same(be.fuse_matches(0), shared[q], len(shared[q][3]), q)


@pytest.mark.gpu
def test_gpu_fuse_two_lists_against_one_frame_and_points_plus_offsets(gpu_env):
    import orbslam3lib_amd as og
    be = gpu_env[0]
    a, pose = _frame_points(gpu_env, "stereo", 0, 310)
    c, _ = _frame_points(gpu_env, "stereo", 0, 311, n=777)
    _gpu_compare(gpu_env, "stereo", [0, 0], [0, 1], [a, c], [pose, pose])
    lists = [be.fuse_matches(q) for q in range(2)]
    # the C ABI's form, with a list no pair names in between and the lists named out of order
    packed = (np.concatenate([a[:5], a, a[:9], c]), np.array([5, 5 + len(a), 14 + len(a), 14 + len(a) + len(c)], np.int32))
    be.fuse([0, 0], [2, 0], packed, np.array([pose, pose], og.RELOC_POSE_DTYPE), K_, th=3.0, bf=MBF, use_uright=True)
    _same(be.fuse_matches(0), lists[1], len(lists[1][3]))
    _same(be.fuse_matches(1), lists[0], len(lists[0][3]))


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(0, 1, 63, 64), (65, 255, 256, 257)])
def test_gpu_fuse_list_lengths_at_the_group_wave_and_block_boundaries(gpu_env, sizes):
    pts, poses = [], []
    for q, n in enumerate(sizes):
        p, pose = _frame_points(gpu_env, "base", q, 400 + n, n=n, pool=max(n // 3, 1))
        pts.append(p)
        poses.append(pose)
    res = _gpu_compare(gpu_env, "base", [0, 1, 2, 3], [0, 1, 2, 3], pts, poses)
    for n, r in zip(sizes, res):
        assert len(r[0]) == n and (r[4] >= n // 6 if n >= 63 else True), (n, r[4])


@pytest.mark.gpu
def test_gpu_fuse_one_list_of_20000_points(gpu_env):
    """SearchInNeighbors' backward leg: one long list.  A scene's points repeated under a permutation: the
    points do not see each other, so each copy gets its source's result; first and nFused follow from them."""
    import orbslam3lib_amd as og
    be, imgs, b, tabs = gpu_env
    base, pose = _frame_points(gpu_env, "base", 2, 500)
    kps, desc, xy, cs, ci, ur = imgs[2]
    bi, bd, code, _, _, _ = _restate("base", base, pose, kps, desc, xy, ur, b, cs, ci, None, tabs)
    src = np.random.default_rng(3).permutation(np.arange(20000) % len(base))
    be.fuse([2], [0], [base[src]], np.array([pose], og.RELOC_POSE_DTYPE), K_, th=3.0, bf=MBF)
    first = np.full(len(kps), -1, np.int32)
    hit = np.flatnonzero(bi[src] >= 0)
    for i in hit[::-1]:
        first[bi[src][i]] = i
    _same(be.fuse_matches(0), (bi[src], bd[src], code[src], first, len(hit)), len(kps))
    assert len(hit) >= 2000


@pytest.mark.gpu
def test_gpu_fuse_all_skipped_and_no_pairs(gpu_env):
    import orbslam3lib_amd as og
    be = gpu_env[0]
    pts, pose = _frame_points(gpu_env, "base", 2, 600, n=200)
    ((bi, bd, code, first, nf, _),) = _gpu_compare(gpu_env, "base", [2], [0], [pts], [pose], [np.ones(200, np.uint8)])
    assert nf == 0 and (code == SKIPPED).all() and (bi == -1).all() and (bd == 256).all() and (first == -1).all()
    pts["flags"] = 0
    ((_, _, code, first, nf, _),) = _gpu_compare(gpu_env, "base", [2], [0], [pts], [pose])
    assert nf == 0 and (code == SKIPPED).all() and (first == -1).all()
    be.fuse([], [], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_)  # n_pairs = 0 succeeds and leaves no pair
    with pytest.raises(og.OrbGpuError) as e:
        be.fuse_matches(0)
    assert e.value.code == -3


@pytest.mark.gpu
def test_gpu_fuse_ratio_on_a_table_threshold(gpu_env):
    """Points whose ratio max_distance / dist3D sits exactly on a step of the level, and one float above."""
    import orbslam3lib_amd as og
    steps = og.predict_scale_table(1.2, 8)
    base, pose = _frame_points(gpu_env, "base", 0, 9, n=400, invalid=0.0, behind=0.0, outside=0.0, too_near=0.0,
                               too_far=0.0, bad_normal=0.0, empty=0.0, not_finite=0.0, flips=(0, 2, 5))
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
    ((_, _, code, _, nf, cnt),) = _gpu_compare(gpu_env, "base", [0], [0], [pts], [pose])
    levels = [cnt["level_%d" % lv] for lv in range(8)]
    assert all(0 < got <= Counter(want)[lv] for lv, got in enumerate(levels)) and sum(levels) >= 0.9 * len(pts)
    assert nf >= 50


@pytest.mark.gpu
def test_gpu_fuse_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    pose, _ = _scene_pose("small")
    pts = np.zeros(4, og.FUSE_POINT_DTYPE)
    poses = np.array([pose], og.RELOC_POSE_DTYPE)
    lib = og.load_library()

    def code(*a, **k):
        with pytest.raises(og.OrbGpuError) as e:
            be.fuse(*a, **k)
        return e.value.code
    with pytest.raises(og.OrbGpuError) as e:  # nothing has run yet
        be.fuse_matches(0)
    assert e.value.code == -3
    assert code([0], [0], [pts], poses, K_) == -3  # before undistort_grid
    be.undistort_grid(K_, D_)
    assert code([0], [0], [pts], poses, K_, use_uright=True) == -3  # before stereo_matches
    be.fuse([0], [0], [pts], poses, K_, use_uright=True, sim3=True)  # sim3 ignores use_uright and bf
    be.fuse([0], [0], [pts], poses, K_, bf=float("nan"), sim3=True)
    be.stereo_matches(MBF, MB)
    n0, n1 = len(be.result(0)[0]), len(be.result(1)[0])
    be.fuse([0], [0], [pts], poses, K_, use_uright=True)
    assert code([1], [0], [pts], poses, K_, use_uright=True) == -3  # a right image
    assert code([2], [0], [pts], poses, K_) == -3 and code([-1], [0], [pts], poses, K_) == -3  # outside the gridded range
    assert code([0], [1], [pts], poses, K_) == -3 and code([0], [-1], [pts], poses, K_) == -3  # lists[p] outside [0, n_lists)
    assert code([0], [0], [pts], poses, K_, th=-1.0) == -3 and code([0], [0], [pts], poses, K_, th=float("nan")) == -3
    assert code([0], [0], [pts], poses, K_, th=float("inf")) == -3
    assert code([0], [0], [pts], poses, K_, bf=-1.0) == -3 and code([0], [0], [pts], poses, K_, bf=float("inf")) == -3
    assert code([0], [0], [pts], poses, K_, skip=[np.zeros(3, np.uint8)]) == -3  # skip_stride below the list's length
    pp = np.array([pose] * 2, og.RELOC_POSE_DTYPE)
    assert code([1, 1], [0, 1], (pts, np.array([0, 4, 2], np.int32)), pp, K_) == -3  # offsets descend
    assert code([1] * 3, [0] * 3, [pts], np.array([pose] * 3, og.RELOC_POSE_DTYPE), K_) == -3  # above the image capacity
    # null arrays with work to do, and a negative first offset, straight at the ABI
    fr, off, Kf = np.zeros(1, np.int32), np.array([0, 4], np.int32), np.asarray(K_, np.float32)
    args = [be.ctx.handle, 1, og._p(fr), og._p(fr), 1, og._p(pts), og._p(off), og._p(poses), og._p(Kf), None, 0,
            og.C.c_float(3), og.C.c_float(0), 0, 0, None]
    assert lib.orbgpu_fuse_batch(*args) == 0
    for k in (2, 3, 5, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert lib.orbgpu_fuse_batch(*bad) == -3, k
    neg = np.array([-1, 3], np.int32)
    assert lib.orbgpu_fuse_batch(*(args[:6] + [og._p(neg)] + args[7:])) == -3
    assert lib.orbgpu_fuse_batch(*([args[0], -1] + args[2:])) == -3
    long_list = np.zeros(og.FUSE_MAX_POINTS + 1, og.FUSE_POINT_DTYPE)
    assert code([0], [0], [long_list], poses, K_) == -2  # ORBGPU_ERR_CAPACITY
    assert code([0], [0], [pts, long_list], poses, K_) == -2  # any list, named or not
    # the result of the last good call is still there: the error paths launched nothing
    be.fuse([1], [0], [pts], poses, K_, skip=[np.zeros(4, np.uint8)], th=0.0)
    assert code([0], [0], [long_list], poses, K_) == -2
    bi, bd, cd, first, nf = be.fuse_matches(0)
    assert len(bi) == 4 and (cd == SKIPPED).all() and len(first) == n1 and nf == 0 and (first == -1).all()
    with pytest.raises(og.OrbGpuError) as e:
        be.fuse_matches(1)
    assert e.value.code == -3
    for kw in (dict(cap_points=3), dict(cap_kp=n1 - 1)):  # each capacity on its own
        with pytest.raises(og.OrbGpuError) as e:
            be.fuse_matches(0, **kw)
        assert e.value.code == -2
    assert len(be.fuse_matches(0, cap_points=4, cap_kp=n1)[3]) == n1 and n0 > 0
    be.close()


@pytest.mark.gpu
def test_gpu_fuse_keeps_its_results_and_leaves_the_other_searches_theirs(gpu_env):
    import orbslam3lib_amd as og
    be, imgs, b, _ = gpu_env
    kps, desc, xy, _, _, _ = imgs[0]
    kr, dr, xyr = imgs[1][0], imgs[1][1], imgs[1][2]
    pose, Rt = _scene_pose("small")
    k2 = np.zeros(len(kr), og.TRIANG_POINT_DTYPE)
    k2["desc"], k2["x"], k2["y"], k2["angle"], k2["octave"], k2["node"] = dr, xyr[:, 0], xyr[:, 1], kr["angle"], kr["octave"], dr[:, 0] >> 2
    be.search_for_triangulation([0], [k2], np.zeros(1, og.TRIANG_PAIR_DTYPE), [(desc[:, 0] >> 2).astype(np.int32)], coarse=True)
    rp = synth.reloc_points(xy, kps, desc, K_, Rt, n=500, seed=3, bounds=[float(v) for v in b])
    rposes = np.array([pose], og.RELOC_POSE_DTYPE)
    be.reloc_by_projection([0], [rp], rposes, K_)
    tri, rel = be.triangulation_matches(0), be.reloc_matches(0)
    assert tri[1] > 0 and rel[1] > 0
    pts, _ = _frame_points(gpu_env, "base", 0, 700)
    (want,) = _gpu_compare(gpu_env, "base", [0], [0], [pts], [pose])
    for got, before in ((be.triangulation_matches(0), tri), (be.reloc_matches(0), rel)):
        for x, y in zip(got, before):
            np.testing.assert_array_equal(x, y)
    be.reloc_by_projection([1], [rp[:100]], rposes, K_, th=3.0, orb_dist=64)
    _same(be.fuse_matches(0), want, len(kps))
    assert want[4] >= 100
