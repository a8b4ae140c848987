"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) on two-camera frames
(CurrentFrame.Nleft != -1, the KannalaBrandt8 rig; cpp/src/ORBmatcher.cc:1721-1921, the right
window :1840-1912) -- orbgpu_track_by_projection_stereo.

The yardstick is _py_track2 below: an independent restatement written from those lines with
np.float32 scalars, every product and sum rounding to single in the reference's order.  The
projection (KannalaBrandt8.cpp:61-78) is computed step by step; atan2f, cosf and sinf are the host
libm's, called through ctypes: the functions oracle/orb_fisheye.cpp links and orb_math.h is pinned
to (tests/test_host_harness.py).  Trl * x3Dc is evaluated row by row as ((R0 x + R1 y) + R2 z) + t:
Sophus's own order is not reproducible here, this order is the pinned choice.
CPU: the restatement against hand-built known answers on tiny frames (the rules that exist only in
this branch), the projection against float64, the struct layout and the ABI, and a check that the
scene generator really produces the situations the GPU cases are meant to cover.
GPU: k_track_candidates_stereo + k_track_resolve_stereo + k_track_finish_stereo against the
restatement, bit-exact on every keypoint's last-frame point, on nmatches and on the 30 bins.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs Sophus, Eigen and the
SLAM stack; no fixtures ship for it) -- restatement only, as for the pinhole form."""
import ctypes as C
import math
from collections import Counter

import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_track_projection import (BT, F32, MB, POP, SC, _direction, _flip, _grid, _header_struct_bytes,
                                         _pose, _py_track, _rot_bin, _scene_pose, _three_maxima, _window)

_libm = C.CDLL("libm.so.6")
for _f in (_libm.atan2f, _libm.cosf, _libm.sinf):
    _f.restype = C.c_float
_libm.atan2f.argtypes = [C.c_float, C.c_float]
_libm.cosf.argtypes = _libm.sinf.argtypes = [C.c_float]

# a 640 x 480 KannalaBrandt8 camera whose image bounds lie inside the front half space (theta_d at
# pi / 2 is about 440 px), and a right camera 10 cm to the right, slightly rotated
CAM = (280.0, 280.0, 320.0, 240.0, 0.0034823894, 0.00071503485, -0.0020532361, 0.00020293674)
K_ = CAM[:4]
BASE = 0.1


def _rig(cam=CAM, R=None, t=(-BASE, 0.0, 0.0)):
    import orbslam3lib_amd as og
    r = np.zeros((), og.TRACK_RIG_DTYPE)
    r["cam_left"] = cam
    r["Rrl"] = np.eye(3).reshape(9) if R is None else np.asarray(R, np.float64).reshape(9)
    r["trl"] = t
    return r


def _scene_rig():
    a, b = 0.002, -0.001
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return _rig(R=Ry @ Rx, t=(-BASE, 0.002, 0.001))


def _kb8_project(P, x3):
    """KannalaBrandt8::project(const Eigen::Vector3f&) (KannalaBrandt8.cpp:61-78), float32."""
    P = [F32(v) for v in P]
    x, y, z = (F32(v) for v in x3)
    with np.errstate(all="ignore"):
        x2_plus_y2 = x * x + y * y
        theta = F32(_libm.atan2f(float(np.sqrt(x2_plus_y2)), float(z)))
        psi = F32(_libm.atan2f(float(y), float(x)))
        theta2 = theta * theta
        theta3 = theta * theta2
        theta5 = theta3 * theta2
        theta7 = theta5 * theta2
        theta9 = theta7 * theta2
        r = theta + P[4] * theta3 + P[5] * theta5 + P[6] * theta7 + P[7] * theta9
        u = P[0] * r * F32(_libm.cosf(float(psi))) + P[2]
        v = P[1] * r * F32(_libm.sinf(float(psi))) + P[3]
    return u, v


def _kb8_project64(P, x3):
    x, y, z = (float(v) for v in x3)
    theta, psi = math.atan2(math.sqrt(x * x + y * y), z), math.atan2(y, x)
    r = theta + P[4] * theta ** 3 + P[5] * theta ** 5 + P[6] * theta ** 7 + P[7] * theta ** 9
    return P[0] * r * math.cos(psi) + P[2], P[1] * r * math.sin(psi) + P[3]


def _kb8_rays(P, uv):
    """Unit rays through the pixels uv [n, 2] (float64, Newton on the theta polynomial)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    mx, my = (uv[:, 0] - P[2]) / P[0], (uv[:, 1] - P[3]) / P[1]
    td = np.hypot(mx, my)
    th = td.copy()
    for _ in range(20):
        t2 = th * th
        f = th * (1 + t2 * (P[4] + t2 * (P[5] + t2 * (P[6] + t2 * P[7])))) - td
        df = 1 + t2 * (3 * P[4] + t2 * (5 * P[5] + t2 * (7 * P[6] + t2 * 9 * P[7])))
        th = th - f / df
    psi = np.arctan2(my, mx)
    return np.stack([np.sin(th) * np.cos(psi), np.sin(th) * np.sin(psi), np.cos(th)], 1)


def _transform(pos, pose):
    """x3Dc = Tcw * x3Dw and 1 / zc (:1742-1747), float32."""
    R, t = np.asarray(pose["Rcw"], F32).reshape(-1), np.asarray(pose["tcw"], F32).reshape(-1)
    X, Y, Z = (F32(v) for v in pos)
    with np.errstate(all="ignore"):
        xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        invz = F32(1.0) / zc
    return (xc, yc, zc), invz


def _to_right(x3, rig):
    """x3Dr = Trl * x3Dc (:1841), the pinned order."""
    R, t = np.asarray(rig["Rrl"], F32).reshape(-1), np.asarray(rig["trl"], F32).reshape(-1)
    xc, yc, zc = x3
    with np.errstate(all="ignore"):
        return (((R[0] * xc + R[1] * yc) + R[2] * zc) + t[0], ((R[3] * xc + R[4] * yc) + R[5] * zc) + t[1],
                ((R[6] * xc + R[7] * yc) + R[8] * zc) + t[2])


def _py_track2(pts, pose, rig, mb, left, right, bounds, blk, th, mono, check, scale, nlevels=8):
    """left / right: (xy, octave, angle, desc, cell_start, cell_idx) of mvKeys / mvKeysRight.
    -> match [Nleft + Nright], nmatches, hist [30] (before the three-maxima rule), Counter."""
    sides = []
    for xy, octv, ang, desc, cs, ci in (left, right):
        sides.append((np.asarray(xy, F32).reshape(-1, 2), np.asarray(octv), np.asarray(ang, F32),
                      np.asarray(desc, np.uint8).reshape(-1, 32), cs, ci))
    nl = len(sides[0][1])
    n = nl + len(sides[1][1])
    held = np.zeros(n, bool)
    if blk is not None:
        held[:min(n, len(blk))] = np.asarray(blk).astype(bool)[:n]
    held0 = held.copy()
    match = np.full(n, -1, np.int32)
    events = [[] for _ in range(30)]
    cnt = Counter()
    fwd, bwd = _direction(pose, mb, mono)
    b = np.asarray(bounds, F32)
    cam = np.asarray(rig["cam_left"], F32).reshape(-1)
    nm = 0

    def search(sd, cand, p, i):
        """One window's match (:1781-1838 / :1852-1910): True if it is an event."""
        nonlocal nm
        _, _, ang, desc, _, _ = sides[sd]
        off, tag = (nl, "_R") if sd else (0, "_L")
        best, bi = 256, -1
        passed = []  # (distance, window position, taken by now) of what passes the pre-call filters
        for pos, k in enumerate(cand):
            g = off + k
            if held[g]:
                cnt[("taken" if not held0[g] else "blocked") + tag] += 1
                if held0[g]:
                    continue
            d = int(POP[np.bitwise_xor(p["desc"], desc[k])].sum())
            passed.append((d, pos, bool(held[g])))
            if held[g]:
                continue
            if d < best:
                best, bi = d, k
        low = sorted(passed)[:4]  # instrumentation only, as in _py_track
        dry = len(passed) > 4 and all(t for _, _, t in low)
        cnt["list_dry"] += dry
        cnt["list_dry_needed"] += dry and low[3][0] <= 100
        cnt["list_dry_matched"] += dry and best <= 100
        if best > 100:
            return False
        g = off + bi
        if match[g] >= 0:
            cnt["overwrite" + tag] += 1
        match[g] = i
        nm += 1
        held[g] = bool(int(p["flags"]) & 4)
        cnt["events"] += 1
        cnt["events" + tag] += 1
        if check:
            bn = _rot_bin(p["angle"], ang[bi])
            if bn is not None:
                events[bn].append(g)
        return True

    for i, p in enumerate(pts):
        if not (int(p["flags"]) & 1):
            cnt["invalid"] += 1
            continue
        x3, invz = _transform(p["pos"], pose)
        if invz < 0:
            cnt["behind"] += 1
            continue
        u, v = _kb8_project(cam, x3)
        if u < b[0] or u > b[1]:
            cnt["out_min_x" if u < b[0] else "out_max_x"] += 1
            continue
        if v < b[2] or v > b[3]:
            cnt["out_min_y" if v < b[2] else "out_max_y"] += 1
            continue
        if not (np.isfinite(u) and np.isfinite(v)):
            cnt["not_finite"] += 1
            continue
        o = int(p["octave"])
        if o < 0 or o >= nlevels:
            cnt["bad_octave"] += 1
            continue
        radius = F32(th) * F32(scale[o])
        if fwd:
            lv = (o, -1)
        elif bwd:
            lv = (0, o)
        else:
            lv = (o - 1, o + 1)
        xy, octv, _, _, cs, ci = sides[0]
        cand = _window(xy, octv, cs, ci, b, u, v, radius, *lv)
        # the right window's geometry does not depend on the left result
        ur, vr = _kb8_project(cam, _to_right(x3, rig))
        right_ok = bool(np.isfinite(ur) and np.isfinite(vr))
        xy, octv, _, _, cs, ci = sides[1]
        cand_r = _window(xy, octv, cs, ci, b, ur, vr, radius, *lv) if right_ok else []
        if not cand:  # :1778-1779, before any occupancy test: the right window is not searched
            cnt["empty_window"] += 1
            cnt["left_empty_right_candidate"] += bool(cand_r)
            continue
        ev_l = search(0, cand, p, i)
        if not right_ok:
            cnt["right_not_finite"] += 1
            continue
        if not (b[0] <= ur <= b[1] and b[2] <= vr <= b[3]):
            cnt["right_out_of_bounds_searched"] += bool(cand_r)
        ev_r = search(1, cand_r, p, i)
        cnt["both_sides"] += ev_l and ev_r
    hist = np.array([len(e) for e in events], np.int32)
    if check:
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn not in keep:
                for g in events[bn]:
                    match[g] = -1
                    nm -= 1
                    cnt["rejected"] += 1
                    cnt["rejected_R" if g >= nl else "rejected_L"] += 1
    return match, nm, hist, cnt


# ---- hand-built frames --------------------------------------------------------------------------

FAR = 400.0  # at this range the two cameras see a point within 0.1 px of the same pixel


class _Side:
    """Keypoints (x, y, octave, desc or None) of one camera, angle 0."""

    def __init__(self, kps, seed):
        rng = np.random.default_rng(seed)
        self.desc = rng.integers(0, 256, (len(kps), 32), dtype=np.uint8)
        for j, (_, _, _, d) in enumerate(kps):
            if d is not None:
                self.desc[j] = d
        self.xy = np.array([(x, y) for x, y, _, _ in kps], F32).reshape(-1, 2)
        self.octv = np.array([o for _, _, o, _ in kps], np.int32)
        self.ang = np.zeros(len(kps), F32)
        self.cs, self.ci = _grid(self.xy, BT)

    def view(self):
        return self.xy, self.octv, self.ang, self.desc, self.cs, self.ci


def _lattice(extra=()):
    """8 x 5 keypoints 70 px apart, octave 0 (windows of octaves 0-2 at th 15 do not meet)."""
    return [(60.0 + 70 * i, 60.0 + 70 * j, 0, None) for j in range(5) for i in range(8)] + list(extra)


class _Tiny2:
    def __init__(self, left=(), right=(), rig=None):
        self.L, self.R = _Side(_lattice(left), 0), _Side(_lattice(right), 1)
        self.rig = _rig() if rig is None else rig
        self.nl = len(self.L.octv)

    def run(self, pts, pose=None, th=15.0, mono=False, check=True, blk=None):
        return _py_track2(pts, _pose() if pose is None else pose, self.rig, MB, self.L.view(), self.R.view(), BT, blk,
                          th, mono, check, SC)


def _aim2(x, y, desc, side=0, rig=None, angle=0.0, octave=0, obs=True, rng_=FAR, valid=True):
    """A last-frame point `rng_` metres along the ray of pixel (x, y) of the left (side 0) or right
    camera, under the identity pose."""
    import orbslam3lib_amd as og
    rig = _rig() if rig is None else rig
    X = _kb8_rays(CAM, [(x, y)])[0] * rng_
    if side:
        X = np.asarray(rig["Rrl"], np.float64).reshape(3, 3).T @ (X - np.asarray(rig["trl"], np.float64))
    p = np.zeros((), og.LAST_POINT_DTYPE)
    p["pos"] = X
    p["angle"], p["octave"] = angle, octave
    p["flags"] = (og.LP_VALID if valid else 0) | (og.MP_HAS_OBS if obs else 0)
    p["desc"] = desc
    return p


def _where(p, rig=None):
    """(left, right) float32 projections of point p under the identity pose."""
    rig = _rig() if rig is None else rig
    x3, _ = _transform(p["pos"], _pose())
    return _kb8_project(CAM, x3), _kb8_project(CAM, _to_right(x3, rig))


D0 = np.random.default_rng(77).integers(0, 256, 32, dtype=np.uint8)


def test_a_empty_left_window_skips_the_right_window():
    """(a) nothing of the left image lies in the window: the right keypoint carrying the point's own
    descriptor, right on the right projection, is not searched (:1778-1779)."""
    T = _Tiny2(right=[(200.0, 95.0, 0, D0)])
    m, nm, _, cnt = T.run(np.array([_aim2(200, 95, D0)]))
    assert (nm, cnt["empty_window"], cnt["left_empty_right_candidate"], (m == -1).all()) == (0, 1, 1, True)


def test_a_blocked_left_window_is_not_empty():
    """(a, the contrast) the left window holds one keypoint that is occupied before the call: not
    empty, so the right keypoint is matched."""
    T = _Tiny2(left=[(200.0, 95.0, 0, D0)], right=[(200.0, 95.0, 0, D0)])
    blk = np.zeros(82, np.uint8)
    blk[40] = 1
    m, nm, _, cnt = T.run(np.array([_aim2(200, 95, D0)]), blk=blk)
    assert (nm, m[40], m[T.nl + 40], cnt["blocked_L"], cnt["empty_window"]) == (1, -1, 0, 1, 0)


def test_b_left_projection_out_of_bounds_skips_both_windows():
    T = _Tiny2(left=[(3.0, 60.0, 0, D0)], right=[(3.0, 60.0, 0, D0)])
    m, nm, _, cnt = T.run(np.array([_aim2(-5, 60, D0)]))
    assert (nm, cnt["out_min_x"], (m == -1).all()) == (0, 1, True)


def test_b_right_projection_out_of_bounds_still_matches():
    """(b) the right window has no bounds test: a right projection left of the image, within the
    radius of an edge keypoint, matches it."""
    p = _aim2(-5, 60, D0, side=1, rng_=2.3)
    (ul, vl), (ur, vr) = _where(p)
    assert 0 < ul < 15 and ur < 0 and abs(ur - F32(2)) < 15  # the input is what the case needs
    T = _Tiny2(left=[(float(ul), 60.0, 0, None)], right=[(2.0, 60.0, 0, D0)])
    m, nm, _, cnt = T.run(np.array([p]))
    assert (nm, m[T.nl + 40], cnt["right_out_of_bounds_searched"]) == (1, 0, 1)


def test_c_one_point_matches_both_sides():
    T = _Tiny2()
    T.R.desc[0] = _flip(T.L.desc[0], 3)
    m, nm, hist, cnt = T.run(np.array([_aim2(60, 60, T.L.desc[0])]))
    assert (nm, m[0], m[T.nl], hist[0], hist.sum(), cnt["both_sides"]) == (2, 0, 0, 2, 2, 1)


def test_d_lone_right_event_in_a_rejected_bin_is_cleared_at_nleft_plus_k():
    T = _Tiny2()
    fill = [_aim2(T.L.xy[k, 0], T.L.xy[k, 1], T.L.desc[k], angle=30.0) for k in range(10, 21)]  # bin 1, left
    lone = _aim2(60, 60, T.R.desc[0], angle=150.0)  # bin 5: no left match, right keypoint 0
    m, nm, hist, cnt = T.run(np.array(fill + [lone]))
    assert (hist[1], hist[5], hist.sum(), cnt["events_R"], cnt["rejected_R"]) == (11, 1, 12, 1, 1)
    assert (nm, m[T.nl]) == (11, -1) and list(m[10:21]) == list(range(11))
    m, nm, _, _ = T.run(np.array(fill + [lone]), check=False)
    assert (nm, m[T.nl]) == (12, 11)


def test_e_right_occupancy_block_taken_overwrite():
    base = _Tiny2()
    d = base.R.desc[0]
    T = _Tiny2(right=[(68.0, 60.0, 0, _flip(d, 40, 2))])  # a second right keypoint 8 px away
    A, B = _aim2(60, 60, _flip(d, 10)), _aim2(60, 60, d)
    # A (with observations) takes right keypoint 0: B, though closer, goes to its next best
    m, nm, _, cnt = T.run(np.array([A, B]), check=False)
    assert (nm, m[T.nl], m[T.nl + 40], cnt["taken_R"]) == (2, 0, 1, 1)
    # without observations A leaves it free: B overwrites
    A["flags"] &= ~4
    m, nm, _, cnt = T.run(np.array([A, B]), check=False)
    assert (nm, m[T.nl], m[T.nl + 40], cnt["overwrite_R"]) == (2, 1, -1, 1)
    # occupied before the call: kp_block is indexed Nleft + k
    blk = np.zeros(T.nl + 41, np.uint8)
    blk[T.nl] = 1
    m, nm, _, cnt = T.run(np.array([B]), check=False, blk=blk)
    assert (nm, m[T.nl], m[T.nl + 40], cnt["blocked_R"]) == (1, -1, 0, 1)


def test_f_negative_inverse_depth_skips_both_windows():
    """(f) zc < 0 in the left camera while the right camera, 5 m behind it, sees the point in front."""
    rig = _rig(t=(-BASE, 0.0, 5.0))
    p = _aim2(60, 60, D0, side=1, rig=rig, rng_=3.0)
    x3, invz = _transform(p["pos"], _pose())
    assert invz < 0 and _to_right(x3, rig)[2] > 0
    (_, _), (ur, vr) = _where(p, rig)
    assert abs(ur - 60) < 0.01 and abs(vr - 60) < 0.01
    T = _Tiny2(rig=rig)
    T.R.desc[0] = D0
    m, nm, _, cnt = T.run(np.array([p]))
    assert (nm, cnt["behind"], (m == -1).all()) == (0, 1, True)


@pytest.mark.parametrize("tz,mono,want", [(0.5, False, [2, 3, 4]), (-0.5, False, [0, 1, 2]), (0.0, False, [1, 2, 3]),
                                          (0.5, True, [1, 2, 3])])
def test_g_level_ranges_apply_to_both_windows(tz, mono, want):
    kps = [(300.0 + 2 * o, 200.0, o, None) for o in range(5)]
    T = _Tiny2()
    T.L, T.R, T.nl = _Side(kps, 5), _Side(kps, 6), 5
    for target in range(5):  # a point of octave 2 carrying each side's keypoint `target`
        for sd, S in enumerate((T.L, T.R)):
            m, nm, _, _ = T.run(np.array([_aim2(304, 200, S.desc[target], octave=2)]), pose=_pose(tz), mono=mono)
            assert (nm == 1 and m[sd * 5 + target] == 0) if target in want else nm == 0, (target, sd)


def test_h_non_finite_right_projection_drops_only_the_right_event():
    T = _Tiny2(rig=_rig(t=(np.nan, 0.0, 0.0)))
    T.R.desc[0] = T.L.desc[0]
    m, nm, hist, cnt = T.run(np.array([_aim2(60, 60, T.L.desc[0])]))
    assert (nm, m[0], m[T.nl], hist.sum(), cnt["right_not_finite"]) == (1, 0, -1, 1, 1)


def test_projection_float32_agrees_with_float64():
    """A sanity check of the restatement (loose on purpose), not a parity claim."""
    rng = np.random.default_rng(9)
    pts = np.concatenate([rng.uniform(-5, 5, (300, 3)), rng.uniform(-5, 5, (50, 3)) * (1, 1, 0),
                          [(0, 0, 1), (0, 0, 3.5), (0, 0, -2), (1, 2, 0), (-3, 0.5, -0.25), (0, 0, 0)]]).astype(np.float32)
    assert (pts[:, 2] <= 0).sum() >= 50
    worst = 0.0
    for x in pts:
        u, v = _kb8_project(CAM, x)
        u64, v64 = _kb8_project64(CAM, x)
        worst = max(worst, abs(float(u) - u64), abs(float(v) - v64))
    assert worst < 1e-3, worst
    assert _kb8_project(CAM, (0, 0, 2)) == (F32(320), F32(240))


def test_rig_layout_and_abi():
    import orbslam3lib_amd as og
    assert og.TRACK_RIG_DTYPE.itemsize == _header_struct_bytes("orbgpu_track_rig") == 80
    assert [og.TRACK_RIG_DTYPE.fields[f][1] for f in ("cam_left", "Rrl", "trl")] == [0, 32, 68]
    assert "orbgpu_track_by_projection_stereo" in og.EXPORTED


def test_null_context_is_invalid():
    import orbslam3lib_amd as og
    lib = og.load_library()
    assert lib.orbgpu_track_by_projection_stereo(None, 1, None, None, None, None, og.C.c_float(1), None, 0,
                                                 og.C.c_float(15), 0, 1, None) == -3


def test_wrapper_refuses_malformed_points_before_any_device_call():
    import orbslam3lib_amd as og
    be = object.__new__(og.BatchExtractor)  # no context at all
    pts = np.zeros(12, og.LAST_POINT_DTYPE)
    poses = np.zeros(3, og.TRACK_POSE_DTYPE)
    for bad in ([1, 5, 5, 12], [0, 5, 4, 12], [0, 5, 5, 11]):
        with pytest.raises(ValueError):
            be.track_by_projection_stereo((pts, np.array(bad)), poses, _rig(), MB)
    with pytest.raises(ValueError):  # one pose per pair
        be.track_by_projection_stereo([pts, pts, pts], poses[:2], _rig(), MB)


# ---- scenes -------------------------------------------------------------------------------------

def stereo_last_frame_points(left, right, rig, pose, n=1000, seed=0, th=15.0, pool=None, obs_fraction=0.7,
                             disparity=12.0, nlevels=8, scale_factor=1.2):
    """Synthetic last-frame points for the two-camera search: half aim at left keypoints, half at
    right ones (left / right: (xy, kps, desc); the pixel is unprojected through the KannalaBrandt8
    model in float64 and moved back through Trl and pose = (Rcw, tcw)); half of the ranges put the
    other camera's projection `disparity` px away, where synth.stereo_pair shows the same feature.
    Position noise, flipped bits, octave +-1, angles and the mixed-in fractions are those of
    synth.last_frame_points: invalid 5%, no observations 1 - obs_fraction, random angles 10%,
    behind the camera 3%, left projections outside the bounds 4% (every side), octaves outside
    [0, nlevels) 1%, non-finite positions 0.5%."""
    import orbslam3lib_amd as og
    rng = np.random.default_rng(seed)
    out = np.zeros(n, og.LAST_POINT_DTYPE)
    cam = [float(v) for v in rig["cam_left"]]
    Rrl, trl = np.asarray(rig["Rrl"], np.float64).reshape(3, 3), np.asarray(rig["trl"], np.float64)
    Rcw, tcw = np.asarray(pose[0], np.float64).reshape(3, 3), np.asarray(pose[1], np.float64).reshape(3)
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    side = (rng.random(n) < 0.5).astype(int)
    outside = rng.random(n) < 0.04
    side[outside] = 0  # only the left window has a bounds test
    uv = np.zeros((n, 2))
    oct_l = np.zeros(n, np.int64)
    ang = np.zeros(n)
    desc = np.zeros((n, 32), np.uint8)
    nothing = np.zeros(n, bool)
    for sd, (xy, kps, dsc) in enumerate((left, right)):
        sel = np.flatnonzero(side == sd)
        nk = len(kps)
        if nk == 0:
            nothing[sel] = True  # nothing to aim at: left invalid
            continue
        npool = max(1, min(nk, (n // 4) if pool is None else int(pool) // 2))
        k = rng.choice(nk, size=npool, replace=False)[rng.integers(0, npool, len(sel))]
        oct_l[sel] = np.clip(np.asarray(kps["octave"], np.int64)[k] + rng.choice([-1, 0, 0, 0, 1], len(sel)), 0,
                             nlevels - 1)
        radius = th * scale[oct_l[sel]]
        uv[sel] = np.asarray(xy, np.float64).reshape(-1, 2)[k] + \
            np.clip(rng.normal(0.0, 0.2, (len(sel), 2)), -0.8, 0.8) * radius[:, None]
        ang[sel] = np.asarray(kps["angle"], np.float64)[k]
        desc[sel] = np.asarray(dsc, np.uint8).reshape(-1, 32)[k]
    for j, i in enumerate(np.flatnonzero(outside)):  # every side in turn
        d = rng.uniform(10.0, 90.0)
        if j % 4 < 2:
            uv[i] = (-d if j % 4 == 0 else 640.0 + d, np.clip(uv[i, 1], 140.0, 340.0))
        else:
            uv[i] = (np.clip(uv[i, 0], 220.0, 420.0), -d if j % 4 == 2 else 480.0 + d)
    rho = rng.uniform(1.0, 20.0, n)
    near = rng.random(n) < 0.5
    rho = np.where(near, cam[0] * abs(trl[0]) / np.maximum(disparity + rng.normal(0.0, 1.0, n), 2.0), rho)
    rho = np.where(rng.random(n) < 0.03, -rho, rho)
    X = _kb8_rays(cam, uv) * rho[:, None]
    X = np.where(side[:, None] == 1, (X - trl) @ Rrl, X)  # Rrl^T (X - trl)
    pw = (X - tcw) @ Rcw
    pw[rng.random(n) < 0.005] = np.nan
    out["pos"] = pw.astype(np.float32)
    out["octave"] = np.where(rng.random(n) < 0.01, rng.choice([-1, nlevels], n), oct_l)
    a = np.mod(ang + 20.0 + rng.normal(0.0, 3.0, n), 360.0)
    out["angle"] = np.where(rng.random(n) < 0.10, rng.uniform(0.0, 360.0, n), a).astype(np.float32)
    out["flags"] = np.where(rng.random(n) < 0.95, og.LP_VALID, 0) | np.where(rng.random(n) < obs_fraction,
                                                                            og.MP_HAS_OBS, 0)
    out["flags"][nothing] &= ~og.LP_VALID
    nflip = rng.choice([0, 2, 5, 10, 20, 35], n)
    for i in range(n):
        if nflip[i]:
            bits = np.unpackbits(desc[i])
            bits[rng.choice(256, nflip[i], replace=False)] ^= 1
            desc[i] = np.packbits(bits)
    out["desc"] = desc
    return out


# (name, tlc_z, th, mono, check_orientation, kp_block)
CASES = [("forward", 0.5, 15.0, False, True, False),
         ("backward", -0.5, 15.0, False, True, False),
         ("neither", 0.01, 15.0, False, True, False),
         ("no_orientation", 0.01, 15.0, False, False, False),
         ("kp_block", 0.01, 15.0, False, True, True)]


def _scene(case, seed, sides, n=1000, **kw):
    """sides: per camera (kps, desc, xy, cs, ci)."""
    pose, Rt = _scene_pose(case[1])
    gen = [(xy, kps, desc) for kps, desc, xy, _, _ in sides]
    return stereo_last_frame_points(gen[0], gen[1], _scene_rig(), Rt, n=n, seed=seed, th=case[2], **kw), pose


def _scene_block(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.08).astype(np.uint8)


def _restate(case, pts, pose, sides, blk, scale, rig=None):
    _, _, th, mono, check, _ = case
    views = [(xy, kps["octave"], kps["angle"], desc, cs, ci) for kps, desc, xy, cs, ci in sides]
    return _py_track2(pts, pose, _scene_rig() if rig is None else rig, MB, views[0], views[1], BT, blk, th, mono, check,
                      scale)


@pytest.fixture(scope="module")
def cpu_pair(oracle):
    L, R = synth.stereo_pair(480, 640, 5)
    sides = []
    for img in (L, R):
        k, d, _ = oracle.extract(img, nfeatures=500)
        xy, b, _, cs, ci = oracle.undistort_grid(k, K_, (), 640, 480)
        assert np.array_equal(b, BT)
        sides.append((k, d.reshape(-1, 32), xy, cs, ci))
    return sides, oracle.scale_factors()[0]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scene_exercises_every_rule(cpu_pair, case):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the
    oracle's extraction, meets every situation the GPU cases are there to compare."""
    sides, scale = cpu_pair
    pts, pose = _scene(case, 100, sides)
    blk = _scene_block(len(sides[0][0]) + len(sides[1][0]), 7) if case[5] else None
    m, nm, hist, cnt = _restate(case, pts, pose, sides, blk, scale)
    assert nm >= 100 and (m >= 0).sum() >= 100
    for tag in ("_L", "_R"):
        assert cnt["overwrite" + tag] >= 5 and cnt["taken" + tag] >= 5, (tag, cnt)
    if case[4]:
        assert cnt["rejected"] >= 5 and hist.sum() == cnt["events"]
    else:
        assert hist.sum() == 0 and nm == cnt["events"]
    for why in ("invalid", "behind", "out_min_x", "out_max_x", "out_min_y", "out_max_y", "not_finite", "bad_octave",
                "empty_window", "left_empty_right_candidate", "both_sides"):
        assert cnt[why] >= 1, (why, cnt)
    if case[5]:
        assert cnt["blocked_L"] >= 1 and cnt["blocked_R"] >= 1
    assert _direction(pose, MB, case[3]) == (case[1] > MB and not case[3], -case[1] > MB and not case[3])


# ---- GPU ----------------------------------------------------------------------------------------

def _gpu_sides(be, pair):
    sides = []
    for i in (2 * pair, 2 * pair + 1):
        kps, desc, _ = be.result(i)
        xy, _, cs, ci = be.grid_result(i)
        sides.append((kps, desc.reshape(-1, 32), xy, cs, ci))
    return sides


@pytest.fixture(scope="module")
def gpu_env(oracle):
    """Two 640x480 stereo pairs at 1000 features, extracted and gridded (raw positions) once."""
    import orbslam3lib_amd as og
    pairs = [synth.stereo_pair(480, 640, 90 + s) for s in range(2)]
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=4)
    be.upload(np.stack([im for pr in pairs for im in pr]))
    be.run()
    be.undistort_grid(K_, ())
    be.synchronize()
    yield be, [_gpu_sides(be, p) for p in range(2)], oracle.scale_factors()[0]
    be.close()


def _gpu_compare(be, frames, scale, case, point_lists, pose, blks, packed=False, rig=None):
    import orbslam3lib_amd as og
    _, _, th, mono, check, _ = case
    rig = _scene_rig() if rig is None else rig
    poses = np.array([pose] * len(point_lists), og.TRACK_POSE_DTYPE)
    points = point_lists
    if packed:
        off = np.concatenate([[0], np.cumsum([len(x) for x in point_lists])]).astype(np.int32)
        points = (np.concatenate(point_lists), off)
    be.track_by_projection_stereo(points, poses, rig, MB, kp_block=blks, th=th, mono=mono, check_orientation=check)
    be.synchronize()
    total, cnts = 0, []
    for f, pts in enumerate(point_lists):
        m, nm, hist, cnt = _restate(case, pts, pose, frames[f], blks[f] if blks else None, scale, rig)
        gm, gnm, ghist = be.track_matches(f)
        assert len(gm) == len(frames[f][0][0]) + len(frames[f][1][0])
        np.testing.assert_array_equal(gm, m, err_msg="frame %d" % f)
        assert gnm == nm, (f, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="frame %d histogram" % f)
        total += nm
        cnts.append(cnt)
    return total, cnts


def _gpu_scene(env, case, packed=False):
    be, frames, scale = env
    lists, blks, pose = [], [], None
    for f in range(2):
        pts, pose = _scene(case, 200 + f, frames[f])
        lists.append(pts)
        blks.append(_scene_block(len(frames[f][0][0]) + len(frames[f][1][0]), 30 + f))
    total, cnts = _gpu_compare(be, frames, scale, case, lists, pose, blks if case[5] else None, packed)
    assert total >= 200
    assert all(c["both_sides"] >= 1 and c["events_L"] >= 50 and c["events_R"] >= 50 for c in cnts)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_track_stereo_bit_exact(gpu_env, case):
    _gpu_scene(gpu_env, case)


@pytest.mark.gpu
def test_gpu_track_stereo_points_plus_offsets(gpu_env):
    _gpu_scene(gpu_env, CASES[0], packed=True)


@pytest.mark.gpu
def test_gpu_track_stereo_dense_conflicts(gpu_env):
    """4000 points aimed at 100 keypoints (50 per side) of one frame, half of them without
    observations: the kept candidate lists run dry and windows are walked again."""
    be, frames, scale = gpu_env
    case = CASES[2]
    pts, pose = _scene(case, 300, frames[0], n=4000, pool=100, obs_fraction=0.5)
    total, (cnt,) = _gpu_compare(be, frames, scale, case, [pts], pose, None)
    assert total >= 50
    # the input does what the case is for: lists run dry, and some of those points still match
    assert cnt["list_dry"] > cnt["list_dry_needed"] >= cnt["list_dry_matched"] >= 5
    assert cnt["overwrite_L"] >= 5 and cnt["overwrite_R"] >= 5


@pytest.mark.gpu
def test_gpu_track_stereo_resolve_group_boundary(gpu_env):
    """Frames of exactly 64 and of 65 points: the resolve pass replays 64 lanes at a time."""
    be, frames, scale = gpu_env
    case = CASES[2]
    lists, pose = [], None
    for f, n in enumerate((64, 65)):
        pts, pose = _scene(case, 400 + f, frames[f], n=n, pool=20)
        lists.append(pts)
    assert _gpu_compare(be, frames, scale, case, lists, pose, None)[0] >= 10


@pytest.mark.gpu
def test_gpu_track_stereo_empty_point_list(gpu_env):
    import orbslam3lib_amd as og
    be, frames, _ = gpu_env
    pose, _ = _scene_pose(0.01)
    be.track_by_projection_stereo([np.zeros(0, og.LAST_POINT_DTYPE)], np.array([pose], og.TRACK_POSE_DTYPE),
                                  _scene_rig(), MB)
    gm, gnm, ghist = be.track_matches(0)
    assert len(gm) == len(frames[0][0][0]) + len(frames[0][1][0])
    assert gnm == 0 and (gm == -1).all() and (ghist == 0).all()


@pytest.mark.gpu
def test_gpu_track_stereo_non_finite_right_projection(gpu_env):
    """A rig whose Trl is not finite: every right window is skipped, the left events stay."""
    be, frames, scale = gpu_env
    case = CASES[2]
    pts, pose = _scene(case, 500, frames[0], n=300)
    rig = _scene_rig()
    rig["trl"][0] = np.nan
    total, (cnt,) = _gpu_compare(be, frames, scale, case, [pts], pose, None, rig=rig)
    assert total >= 20 and cnt["events_R"] == 0 and cnt["right_not_finite"] >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("blank", [1, 0], ids=["right_constant", "left_constant"])
def test_gpu_track_stereo_one_sided_frames(oracle, blank):
    """A pair one of whose images is constant: Nright == 0, or Nleft == 0 -- then every left window
    is empty and nothing matches although right keypoints exist."""
    import orbslam3lib_amd as og
    imgs = list(synth.stereo_pair(480, 640, 93))
    imgs[blank] = np.full_like(imgs[blank], 128)
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack(imgs))
    be.run()
    be.undistort_grid(K_, ())
    be.synchronize()
    sides = _gpu_sides(be, 0)
    assert len(sides[blank][0]) == 0 and len(sides[1 - blank][0]) >= 500
    case = CASES[2]
    # aim at the live image's keypoints through both cameras
    kps, desc, xy, _, _ = sides[1 - blank]
    pose, Rt = _scene_pose(case[1])
    pts = stereo_last_frame_points((xy, kps, desc), (xy, kps, desc), _scene_rig(), Rt, n=600, seed=600)
    total, (cnt,) = _gpu_compare(be, [sides], oracle.scale_factors()[0], case, [pts], pose, None)
    if blank == 1:
        assert total >= 50 and cnt["events_R"] == 0
    else:
        assert total == 0 and cnt["left_empty_right_candidate"] >= 50
    be.close()


@pytest.mark.gpu
def test_gpu_track_stereo_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    pose, _ = _scene_pose(0.01)
    args = ([np.zeros(4, og.LAST_POINT_DTYPE)], np.array([pose], og.TRACK_POSE_DTYPE))
    with pytest.raises(og.OrbGpuError) as e:  # before undistort_grid
        be.track_by_projection_stereo(*args, _scene_rig(), MB)
    assert e.value.code == -3
    be.undistort_grid(K_, ())
    with pytest.raises(og.OrbGpuError) as e:  # more pairs than the gridded batch holds
        be.track_by_projection_stereo(args[0] * 2, np.array([pose] * 2, og.TRACK_POSE_DTYPE), _scene_rig(), MB)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # null rig
        be.track_by_projection_stereo(*args, None, MB)
    assert e.value.code == -3
    be.track_by_projection_stereo(*args, _scene_rig(), MB)
    assert be.track_matches(0)[1] == 0  # four invalid points
    be.close()


@pytest.mark.gpu
def test_gpu_track_stereo_then_pinhole_on_one_context(gpu_env):
    """track_matches reports the last call's form: n_kp = Nleft + Nright after a two-camera call,
    n_kp = N and the pinhole result after a pinhole call, in either order."""
    import orbslam3lib_amd as og
    be, frames, scale = gpu_env
    case = CASES[2]
    pts2, pose = _scene(case, 700, frames[0], n=300)
    kps, desc, xy, cs, ci = frames[0][0]
    Rt = _scene_pose(case[1])[1]
    pts1 = synth.last_frame_points(xy, kps, desc, K_, Rt, None, n=300, seed=701, bounds=[0.0, 640.0, 0.0, 480.0])
    m1, nm1, h1, _ = _py_track(pts1, pose, K_, 0.0, MB, xy, kps["octave"], kps["angle"], desc, None, BT, cs, ci, None,
                               15.0, False, True, scale)
    assert nm1 >= 20
    poses = np.array([pose], og.TRACK_POSE_DTYPE)

    def pinhole():
        be.track_by_projection([pts1], poses, K_, 0.0, MB, image_step=2, use_uright=False)
        gm, gnm, gh = be.track_matches(0)
        assert len(gm) == len(kps) and gnm == nm1
        np.testing.assert_array_equal(gm, m1)
        np.testing.assert_array_equal(gh, h1)

    pinhole()
    assert _gpu_compare(be, frames, scale, case, [pts2], pose, None)[0] >= 20
    pinhole()
    assert _gpu_compare(be, frames, scale, case, [pts2], pose, None)[0] >= 20
