"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) -- the motion-model search
of Tracking::TrackWithMotionModel (cpp/src/ORBmatcher.cc:1683-1838, pinhole branch, with
ComputeThreeMaxima :2061-2102 and Frame::GetFeaturesInArea, Frame.cc:673-739).

The yardstick is _py_track below: an independent restatement written from those lines with
np.float32 scalars (every product and sum rounds to single, in the reference's order).
CPU: the restatement against hand-built known answers on a tiny frame (overwrites, rejected bins,
bin edges, the three-maxima rule, level ranges, the skips, the mvuRight tolerance); a check that
synth.last_frame_points really produces the situations the GPU cases are meant to cover; the
wrapper's dtypes and point forms.
GPU: k_track_candidates + k_track_resolve against the restatement, bit-exact on every keypoint's
last-frame point, on nmatches and on the 30 histogram bins.

Parity status: unpinned against the reference itself (ORBmatcher.cc needs Sophus, Eigen and the
SLAM stack; no fixtures ship for it) -- restatement only, as for the other matcher functions."""
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

from orbslam3lib_amd import synth

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_ = (458.654, 457.296, 367.215, 248.375)
D_ = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
MBF = 47.9
MB = float(np.float32(47.9) / np.float32(435.2))
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _c_round(x):
    """C round(): half away from zero."""
    x = float(x)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _direction(pose, mb, mono):
    """bForward, bBackward (:1727-1734)."""
    Rcw, tcw, Rlw, tlw = (np.asarray(pose[k], F32).reshape(-1) for k in ("Rcw", "tcw", "Rlw", "tlw"))
    twc = [-((Rcw[k] * tcw[0] + Rcw[3 + k] * tcw[1]) + Rcw[6 + k] * tcw[2]) for k in range(3)]
    tlc_z = ((Rlw[6] * twc[0] + Rlw[7] * twc[1]) + Rlw[8] * twc[2]) + tlw[2]
    return bool(tlc_z > F32(mb)) and not mono, bool(-tlc_z > F32(mb)) and not mono


def _project(pos, pose, K):
    """(u, v, invz, zc): Tcw * x3Dw and Pinhole::project (Pinhole.cpp:40-41), float32."""
    R, t = np.asarray(pose["Rcw"], F32).reshape(-1), np.asarray(pose["tcw"], F32).reshape(-1)
    X, Y, Z = (F32(v) for v in pos)
    fx, fy, cx, cy = (F32(v) for v in K)
    with np.errstate(all="ignore"):
        xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        invz = F32(1.0) / zc
        u = fx * xc / zc + cx
        v = fy * yc / zc + cy
    return u, v, invz, zc


def _window(xy, octv, cs, ci, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel): indices in the reference's order."""
    b = np.asarray(bounds, F32)
    wi = F32(64) / (b[1] - b[0])
    hi = F32(48) / (b[3] - b[2])
    x0 = max(0, int(math.floor(((x - b[0]) - r) * wi)))
    if x0 >= 64:
        return []
    x1 = min(63, int(math.ceil(((x - b[0]) + r) * wi)))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(((y - b[2]) - r) * hi)))
    if y0 >= 48:
        return []
    y1 = min(47, int(math.ceil(((y - b[2]) + r) * hi)))
    if y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for k in ci[cs[ix * 48 + iy]:cs[ix * 48 + iy + 1]]:
                if check:
                    if octv[k] < min_level:
                        continue
                    if max_level >= 0 and octv[k] > max_level:
                        continue
                if abs(xy[k, 0] - x) < r and abs(xy[k, 1] - y) < r:
                    out.append(int(k))
    return out


def _three_maxima(hist):
    """ComputeThreeMaxima (:2061-2102) on the bin sizes -> (ind1, ind2, ind3)."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        s = int(s)
        if s > m1:
            m3, m2, m1 = m2, m1, s
            i3, i2, i1 = i2, i1, i
        elif s > m2:
            m3, m2 = m2, s
            i3, i2 = i2, i
        elif s > m3:
            m3, i3 = s, i
    if F32(m2) < F32(0.1) * F32(m1):
        i2 = i3 = -1
    elif F32(m3) < F32(0.1) * F32(m1):
        i3 = -1
    return i1, i2, i3


def _rot_bin(angle_last, angle_cur):
    """:1829-1834; None outside [0, 30) (the reference's assert)."""
    rot = F32(angle_last) - F32(angle_cur)
    if rot < 0.0:
        rot = rot + F32(360.0)
    x = rot * (F32(1.0) / F32(30))
    if not np.isfinite(x):
        return None
    b = _c_round(x)
    if b == 30:
        b = 0
    return b if 0 <= b < 30 else None


def _py_track(pts, pose, K, mbf, mb, xy, octv, ang, desc, uright, bounds, cs, ci, blk, th, mono, check, scale,
              nlevels=8):
    """-> match [n_kp], nmatches, hist [30] (before the three-maxima rule), Counter of the rules."""
    n = len(octv)
    xy = np.asarray(xy, F32)
    held = np.zeros(n, bool) if blk is None else np.asarray(blk).astype(bool)[:n].copy()
    held0 = held.copy()
    match = np.full(n, -1, np.int32)
    events = [[] for _ in range(30)]
    cnt = Counter()
    fwd, bwd = _direction(pose, mb, mono)
    b = np.asarray(bounds, F32)
    nm = 0
    for i, p in enumerate(pts):
        if not (int(p["flags"]) & 1):
            cnt["invalid"] += 1
            continue
        u, v, invz, _ = _project(p["pos"], pose, K)
        if invz < 0:
            cnt["behind"] += 1
            continue
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
        cand = _window(xy, octv, cs, ci, b, u, v, radius, *lv)
        if not cand:
            cnt["empty_window"] += 1
            continue
        ur = u - F32(mbf) * invz
        best, bi = 256, -1
        passed = []  # (distance, window position, taken by now) of what passes the pre-call filters
        for pos, k in enumerate(cand):
            if held[k]:
                cnt["taken" if not held0[k] else "blocked"] += 1
                if held0[k]:
                    continue
            if uright is not None and uright[k] > 0:
                if abs(ur - F32(uright[k])) > radius:
                    cnt["uright"] += not held[k]
                    continue
            d = int(POP[np.bitwise_xor(p["desc"], desc[k])].sum())
            passed.append((d, pos, bool(held[k])))
            if held[k]:
                continue
            if d < best:
                best, bi = d, k
        # instrumentation only: the four lowest (distance, position) are all taken and more passed
        # (needed: the fourth is within TH_HIGH, so a fifth could still be accepted)
        low = sorted(passed)[:4]
        dry = len(passed) > 4 and all(t for _, _, t in low)
        cnt["list_dry"] += dry
        cnt["list_dry_needed"] += dry and low[3][0] <= 100
        cnt["list_dry_matched"] += dry and best <= 100
        if best <= 100:
            if match[bi] >= 0:
                cnt["overwrite"] += 1
            match[bi] = i
            nm += 1
            held[bi] = bool(int(p["flags"]) & 4)
            cnt["events"] += 1
            if check:
                bn = _rot_bin(p["angle"], ang[bi])
                if bn is not None:
                    events[bn].append(bi)
    hist = np.array([len(e) for e in events], np.int32)
    if check:
        keep = _three_maxima(hist)
        for bn in range(30):
            if bn not in keep:
                for k in events[bn]:
                    match[k] = -1
                    nm -= 1
                    cnt["rejected"] += 1
    return match, nm, hist, cnt


# ---- hand-built frames --------------------------------------------------------------------------

KT = (500.0, 500.0, 320.0, 240.0)
BT = np.array([0, 640, 0, 480], F32)
SC = (F32(1.2) ** np.arange(8)).astype(F32)  # stands for mvScaleFactors in the hand-built cases


def _grid(xy, bounds):
    """Frame::AssignFeaturesToGrid + PosInGrid (Frame.cc:405-436, 741-751) as CSR lists."""
    b = np.asarray(bounds, F32)
    wi = F32(64) / (b[1] - b[0])
    hi = F32(48) / (b[3] - b[2])
    cells = []
    for k, (x, y) in enumerate(np.asarray(xy, F32)):
        px, py = _c_round((x - b[0]) * wi), _c_round((y - b[2]) * hi)
        if 0 <= px < 64 and 0 <= py < 48:
            cells.append((px * 48 + py, k))
    cells.sort()
    cs = np.zeros(64 * 48 + 1, np.int32)
    for c, _ in cells:
        cs[c + 1] += 1
    return np.cumsum(cs).astype(np.int32), np.array([k for _, k in cells], np.int32)


def _pose(tlc_z=0.0):
    p = np.zeros((), [("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("Rlw", "<f4", (9,)), ("tlw", "<f4", (3,))])
    p["Rcw"] = p["Rlw"] = np.eye(3, dtype=F32).reshape(9)
    p["tlw"][2] = tlc_z  # Tcw = identity: twc = 0 and tlc = tlw
    return p


class _Tiny:
    """8 x 5 keypoints 70 px apart (windows of octaves 0-2 at th 15 do not meet), octave 0,
    angle 0, random descriptors; `extra`: more (x, y, octave, desc) keypoints."""

    def __init__(self, extra=(), seed=0):
        rng = np.random.default_rng(seed)
        pts = [(60.0 + 70 * i, 60.0 + 70 * j) for j in range(5) for i in range(8)]
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
        self.ur = None
        self.cs, self.ci = _grid(self.xy, BT)

    def run(self, pts, pose=None, th=15.0, mono=False, check=True, blk=None, mbf=MBF):
        return _py_track(pts, _pose() if pose is None else pose, KT, mbf, MB, self.xy, self.octv, self.ang,
                         self.desc, self.ur, BT, self.cs, self.ci, blk, th, mono, check, SC)


def _flip(d, nbits, seed=0):
    b = np.unpackbits(np.asarray(d, np.uint8))
    b[np.random.default_rng(seed).choice(256, nbits, replace=False)] ^= 1
    return np.packbits(b)


def _aim(x, y, desc, angle=0.0, octave=0, obs=True, z=2.0, valid=True):
    """A last-frame point that projects to (x, y) under the identity pose and KT."""
    import orbslam3lib_amd as og
    p = np.zeros((), og.LAST_POINT_DTYPE)
    p["pos"] = ((x - KT[2]) / KT[0] * z, (y - KT[3]) / KT[1] * z, z)
    p["angle"], p["octave"] = angle, octave
    p["flags"] = (og.LP_VALID if valid else 0) | (og.MP_HAS_OBS if obs else 0)
    p["desc"] = desc
    return p


def _fillers(T, ks, angle=30.0):
    return [_aim(T.xy[k, 0], T.xy[k, 1], T.desc[k], angle=angle) for k in ks]


def test_two_overwrites_one_rejected_bin_clears_the_keypoint():
    """A then B (neither with observations) take keypoint 0; A's bin is rejected, B's is kept: the
    keypoint is cleared although its last event survived, and nmatches drops by exactly one."""
    T = _Tiny()
    A = _aim(60, 60, _flip(T.desc[0], 3), angle=150.0, obs=False)  # bin 5, alone
    B = _aim(60, 60, _flip(T.desc[0], 5, 1), angle=30.0, obs=False)  # bin 1 with the fillers
    pts = np.array([A, B] + _fillers(T, range(10, 20)))
    m, nm, hist, cnt = T.run(pts)
    assert hist[1] == 11 and hist[5] == 1 and hist.sum() == 12
    assert cnt["overwrite"] == 1 and cnt["rejected"] == 1
    assert m[0] == -1 and nm == 11
    assert list(m[10:20]) == list(range(2, 12))
    # without the orientation check B keeps the keypoint
    m, nm, hist, _ = T.run(pts, check=False)
    assert m[0] == 1 and nm == 12 and hist.sum() == 0


def test_two_overwrites_both_bins_rejected_subtract_two():
    T = _Tiny()
    A = _aim(60, 60, _flip(T.desc[0], 3), angle=150.0, obs=False)  # bin 5
    B = _aim(60, 60, _flip(T.desc[0], 5, 1), angle=210.0, obs=False)  # bin 7
    pts = np.array([A, B] + _fillers(T, range(10, 21)))  # 11: one event is below 10% of the maximum
    m, nm, hist, cnt = T.run(pts)
    assert hist[1] == 11 and hist[5] == 1 and hist[7] == 1
    assert m[0] == -1 and nm == 11 and cnt["rejected"] == 2


def test_taken_keypoint_sends_a_closer_point_to_its_next_best_or_nothing():
    base = _Tiny()
    # nothing else in the window: the second point, though closer, finds its keypoint taken
    A = _aim(60, 60, _flip(base.desc[0], 10), obs=True)
    B = _aim(60, 60, base.desc[0], obs=True)
    m, nm, _, cnt = base.run(np.array([A, B]), check=False)
    assert m[0] == 0 and nm == 1 and cnt["taken"] == 1
    # a second keypoint 8 px away, 40 bits from the first: the next best
    T = _Tiny(extra=[(68.0, 60.0, 0, _flip(base.desc[0], 40, 2))])
    m, nm, _, cnt = T.run(np.array([A, B]), check=False)
    assert m[0] == 0 and m[40] == 1 and nm == 2 and cnt["taken"] == 1
    # a first point without observations leaves the keypoint free: the second overwrites it
    A["flags"] &= ~4
    m, nm, _, cnt = T.run(np.array([A, B]), check=False)
    assert m[0] == 1 and m[40] == -1 and nm == 2 and cnt["overwrite"] == 1
    # occupied before the call: never assigned
    blk = np.zeros(41, np.uint8)
    blk[0] = 1
    m, nm, _, cnt = T.run(np.array([B]), check=False, blk=blk)
    assert m[0] == -1 and m[40] == 0 and cnt["blocked"] == 1


@pytest.mark.parametrize("last,cur,expect", [(14.9, 0.0, 0), (15.0, 0.0, 1), (359.0, 0.0, 12), (0.0, 0.5, 12),
                                             (44.9, 0.0, 1), (45.1, 0.0, 2), (10.0, 350.0, 1)])
def test_rotation_bin_edges(last, cur, expect):
    """The factor is 1 / 30 (not 30 / 360): float 15 * (1 / 30) is at least 0.5 and rounds away."""
    assert _rot_bin(last, cur) == expect
    T = _Tiny()
    T.ang[3] = cur
    _, nm, hist, _ = T.run(np.array([_aim(T.xy[3, 0], T.xy[3, 1], T.desc[3], angle=last)]))
    assert nm == 1 and hist[expect] == 1 and hist.sum() == 1


def test_three_maxima_ties_and_cutoffs():
    h = np.zeros(30, int)
    assert _three_maxima(h) == (-1, -1, -1)
    h[[2, 5, 7, 9]] = 5  # strict >: the earlier bins win the tie
    assert _three_maxima(h) == (2, 5, 7)
    h = np.zeros(30, int)
    h[[4, 1, 8]] = (100, 9, 9)  # max2 < 10%: ind2 and ind3 dropped
    assert _three_maxima(h) == (4, -1, -1)
    h[[4, 1, 8]] = (100, 11, 9)  # only max3 < 10%
    assert _three_maxima(h) == (4, 1, -1)
    h[[4, 1, 8]] = (100, 11, 11)
    assert _three_maxima(h) == (4, 1, 8)
    h[[4, 1, 8]] = (100, 50, 120)  # a later larger bin shifts the earlier ones down
    assert _three_maxima(h) == (8, 4, 1)
    # exactly 10%: `<` in float, 0.1f * 10.0f rounds to 1.0f, so one event beside ten is kept
    h = np.zeros(30, int)
    h[[0, 3]] = (10, 1)
    assert bool(F32(1) < F32(0.1) * F32(10)) is False
    assert _three_maxima(h) == (0, 3, -1)


def test_level_ranges_by_direction():
    """Five keypoints of octaves 0..4 within 8 px: forward keeps >= octave (at octave 0 no level
    test at all), backward <= octave, otherwise octave +-1."""
    xy = np.array([(300.0 + 2 * o, 200.0) for o in range(5)], F32)
    octv = np.arange(5, dtype=np.int32)
    cs, ci = _grid(xy, BT)

    def octs(lo, hi):
        return sorted(int(octv[k]) for k in _window(xy, octv, cs, ci, BT, F32(304), F32(200), F32(15), lo, hi))
    assert octs(2, -1) == [2, 3, 4] and octs(0, -1) == [0, 1, 2, 3, 4] and octs(4, -1) == [4]
    assert octs(0, 2) == [0, 1, 2] and octs(0, 0) == [0]
    assert octs(1, 3) == [1, 2, 3] and octs(-1, 1) == [0, 1] and octs(3, 5) == [3, 4]
    # through the whole function: the direction comes from the two poses and mb
    desc = np.random.default_rng(5).integers(0, 256, (5, 32), dtype=np.uint8)
    T = _Tiny()
    T.xy, T.octv, T.ang, T.desc, T.cs, T.ci = xy, octv, np.zeros(5, F32), desc, cs, ci
    assert _direction(_pose(0.5), MB, False) == (True, False)
    assert _direction(_pose(-0.5), MB, False) == (False, True)
    assert _direction(_pose(0.01), MB, False) == (False, False)
    assert _direction(_pose(0.5), MB, True) == (False, False)
    for tz, mono, want in ((0.5, False, [2, 3, 4]), (-0.5, False, [0, 1, 2]), (0.0, False, [1, 2, 3]),
                           (0.5, True, [1, 2, 3])):
        for target in range(5):  # a point of octave 2 carrying keypoint `target`'s descriptor
            m, nm, _, _ = T.run(np.array([_aim(304, 200, desc[target], octave=2)]), pose=_pose(tz), mono=mono)
            assert (nm == 1 and m[target] == 0) if target in want else nm == 0, (tz, mono, target)


def test_skips_and_uright_tolerance():
    T = _Tiny()
    d = T.desc[0]
    cases = [(_aim(60, 60, d, valid=False), "invalid"), (_aim(60, 60, d, z=-2.0), "behind"),
             (_aim(-5, 60, d), "out_min_x"), (_aim(645, 60, d), "out_max_x"), (_aim(60, -5, d), "out_min_y"),
             (_aim(60, 485, d), "out_max_y"), (_aim(60, 60, d, octave=8), "bad_octave"),
             (_aim(60, 60, d, octave=-1), "bad_octave"), (_aim(200, 95, d), "empty_window")]
    nan = _aim(60, 60, d)
    nan["pos"][0] = np.nan
    zero = _aim(60, 60, d, z=0.0)  # zc = 0: invz = +inf is not < 0, the projection is not finite
    cases += [(nan, "not_finite"), (zero, "not_finite")]
    for p, why in cases:
        m, nm, _, cnt = T.run(np.array([p]))
        assert nm == 0 and (m == -1).all() and cnt[why] == 1, why
    # on the bounds themselves the point is kept (the reference's tests are strict)
    edge = _Tiny(extra=[(2.0, 60.0, 0, None)])
    m, nm, _, _ = edge.run(np.array([_aim(0, 60, edge.desc[40])]))
    assert nm == 1 and m[40] == 0
    # mvuRight: er == radius is kept, one ulp more is not
    p = _aim(60, 60, d)
    u, _, invz, _ = _project(p["pos"], _pose(), KT)
    ur = u - F32(MBF) * invz
    T.ur = np.full(40, -1, F32)
    T.ur[0] = ur - F32(15)
    assert abs(ur - T.ur[0]) == F32(15)
    m, nm, _, cnt = T.run(np.array([p]))
    assert nm == 1 and m[0] == 0 and cnt["uright"] == 0
    T.ur[0] = np.nextafter(T.ur[0], F32(-1e9))
    m, nm, _, cnt = T.run(np.array([p]))
    assert nm == 0 and cnt["uright"] == 1
    T.ur[0] = -1  # no stereo match: no test
    assert T.run(np.array([p]))[1] == 1


# ---- wrapper and ABI ----------------------------------------------------------------------------

def _header_struct_bytes(name):
    txt = open(os.path.join(ROOT, "include", "orbgpu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"float": 4, "int32_t": 4, "uint8_t": 1}
    total = 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ty, rest = decl.split(None, 1)
        for item in rest.split(","):
            dim = re.search(r"\[(\d+)\]", item)
            total += size[ty] * (int(dim.group(1)) if dim else 1)
    return total


def test_dtypes_match_the_header_structs():
    import orbslam3lib_amd as og
    assert og.LAST_POINT_DTYPE.itemsize == _header_struct_bytes("orbgpu_last_point") == 56
    assert og.TRACK_POSE_DTYPE.itemsize == _header_struct_bytes("orbgpu_track_pose") == 96
    assert [og.LAST_POINT_DTYPE.fields[f][1] for f in ("pos", "angle", "octave", "flags", "desc")] == [0, 12, 16, 20, 24]
    assert [og.TRACK_POSE_DTYPE.fields[f][1] for f in ("Rcw", "tcw", "Rlw", "tlw")] == [0, 36, 48, 84]
    assert {"orbgpu_track_by_projection_batch", "orbgpu_download_track_matches"} <= set(og.EXPORTED)
    lib = og.load_library()
    assert lib.orbgpu_track_by_projection_batch(None, 1, 2, 0, None, None, None, None, og.C.c_float(1),
                                                og.C.c_float(1), None, 0, og.C.c_float(15), 0, 1, None) == -3
    assert lib.orbgpu_download_track_matches(None, 0, None, 0, None, None, None) == -3


def test_point_forms_reach_the_abi_identically():
    import orbslam3lib_amd as og
    rng = np.random.default_rng(3)
    parts = []
    for n in (5, 0, 7):
        a = np.zeros(n, og.LAST_POINT_DTYPE)
        a.view(np.uint8)[:] = rng.integers(0, 256, a.nbytes, dtype=np.uint8)
        parts.append(a)
    rows = og.BatchExtractor._map_point_rows
    m1, o1, n1 = rows(parts, og.LAST_POINT_DTYPE)
    m2, o2, n2 = rows((np.concatenate(parts), np.array([0, 5, 5, 12])), og.LAST_POINT_DTYPE)
    assert n1 == n2 == 3 and o1.dtype == o2.dtype == np.int32 and m1.dtype == m2.dtype == og.LAST_POINT_DTYPE
    np.testing.assert_array_equal(o1, o2)
    assert m1.tobytes() == m2.tobytes() and m1.nbytes == 12 * 56
    # malformed offsets are refused before any device call: this extractor has no context at all
    be = object.__new__(og.BatchExtractor)
    poses = np.zeros(3, og.TRACK_POSE_DTYPE)
    for bad in ([1, 5, 5, 12], [0, 5, 4, 12], [0, 5, 5, 11]):
        with pytest.raises(ValueError):
            be.track_by_projection((np.concatenate(parts), np.array(bad)), poses, K_, MBF, MB)
    with pytest.raises(ValueError):  # one pose per frame
        be.track_by_projection(parts, poses[:2], K_, MBF, MB)


# ---- scenes -------------------------------------------------------------------------------------

# (name, stereo / use_uright, tlc_z, th, mono, check_orientation, kp_block, image_step)
CASES = [("stereo_forward", True, 0.5, 15.0, False, True, False, 2),
         ("stereo_backward", True, -0.5, 15.0, False, True, False, 2),
         ("stereo_neither", True, 0.01, 15.0, False, True, False, 2),
         ("mono_th7", False, 0.5, 7.0, True, True, False, 1),
         ("no_orientation", True, 0.01, 15.0, False, False, False, 2),
         ("kp_block", True, 0.01, 15.0, False, True, True, 2)]


def _scene_pose(tlc_z):
    """A small rotation and translation for the current frame; the last frame sits tlc_z behind
    the current camera centre along its own axis (Rlw = I, tlw = -twc + (0, 0, tlc_z))."""
    a = 0.02
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    t = np.array([0.1, -0.05, 0.2])
    p = _pose()
    p["Rcw"], p["tcw"] = R.reshape(9), t
    p["tlw"] = R.T @ t + np.array([0, 0, tlc_z])
    return p, (R, t)


def _scene_points(case, seed, xy, kps, desc, ur, bounds, n=1000, **kw):
    _, stereo, tz, th, _, _, _, _ = case
    pose, Rt = _scene_pose(tz)
    pts = synth.last_frame_points(xy, kps, desc, K_, Rt, ur if stereo else None, n=n, seed=seed,
                                  mbf=MBF if stereo else None, th=th, bounds=[float(v) for v in bounds], **kw)
    return pts, pose


def _scene_block(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.08).astype(np.uint8)


def _restate(case, pts, pose, kps, desc, xy, ur, bounds, cs, ci, blk, scale):
    _, stereo, _, th, mono, check, _, _ = case
    return _py_track(pts, pose, K_, MBF, MB, xy, kps["octave"], kps["angle"], desc, ur if stereo else None, bounds, cs,
                     ci, blk, th, mono, check, scale)


@pytest.fixture(scope="module")
def cpu_frame(oracle):
    L, R = synth.stereo_pair(480, 640, 5)
    kl, dl, _ = oracle.extract(L, nfeatures=500)
    kr, dr, _ = oracle.extract(R, nfeatures=500)
    xy, b, _, cs, ci = oracle.undistort_grid(kl, K_, D_, 640, 480)
    ur, _, _ = oracle.stereo_matches(kl, dl, kr, dr, oracle.pyramid(L), oracle.pyramid(R), MBF, MB)
    return kl, dl.reshape(-1, 32), xy, b, cs, ci, ur, oracle.scale_factors()[0]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scene_exercises_every_rule(cpu_frame, case):
    """Conditions on the generated inputs (not measurements): the restatement alone, on the
    oracle's extraction, meets every situation the GPU cases are there to compare."""
    kl, dl, xy, b, cs, ci, ur, scale = cpu_frame
    pts, pose = _scene_points(case, 100, xy, kl, dl, ur, b)
    blk = _scene_block(len(kl), 7) if case[6] else None
    m, nm, hist, cnt = _restate(case, pts, pose, kl, dl, xy, ur, b, cs, ci, blk, scale)
    assert nm >= 100 and (m >= 0).sum() >= 100
    assert cnt["overwrite"] >= 5 and cnt["taken"] >= 5
    if case[5]:
        assert cnt["rejected"] >= 5 and hist.sum() == cnt["events"]
    else:
        assert hist.sum() == 0 and nm == cnt["events"]
    for why in ("invalid", "behind", "out_min_x", "out_max_x", "out_min_y", "out_max_y", "not_finite", "bad_octave"):
        assert cnt[why] >= 1, why
    if case[1]:
        assert cnt["uright"] >= 1
    if case[6]:
        assert cnt["blocked"] >= 1
    assert _direction(pose, MB, case[4]) == (case[2] > MB and not case[4], -case[2] > MB and not case[4])


# ---- GPU ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu_env(oracle):
    """Two 640x480 stereo pairs at 1000 features, extracted, gridded and stereo-matched once."""
    import orbslam3lib_amd as og
    pairs = [synth.stereo_pair(480, 640, 90 + s) for s in range(2)]
    be = og.BatchExtractor(1000, 1.2, 8, 20, 7, width=640, height=480, max_images=4)
    be.upload(np.stack([im for pr in pairs for im in pr]))
    be.run()
    be.undistort_grid(K_, D_)
    be.stereo_matches(MBF, MB)
    be.synchronize()
    imgs = []
    for i in range(4):
        kps, desc, _ = be.result(i)
        xy, _, cs, ci = be.grid_result(i)
        imgs.append((kps, desc, xy, cs, ci, be.stereo_result(i // 2)[0] if i % 2 == 0 else None))
    b = oracle.undistort_grid(imgs[0][0], K_, D_, 640, 480)[1]
    yield be, imgs, b, oracle.scale_factors()[0]
    be.close()


def _gpu_compare(env, case, point_lists, pose, blks, packed=False):
    import orbslam3lib_amd as og
    be, imgs, b, scale = env
    _, stereo, _, cth, mono, check, _, step = case
    poses = np.array([pose] * len(point_lists), og.TRACK_POSE_DTYPE)
    points = point_lists
    if packed:
        off = np.concatenate([[0], np.cumsum([len(x) for x in point_lists])]).astype(np.int32)
        points = (np.concatenate(point_lists), off)
    be.track_by_projection(points, poses, K_, MBF, MB, image_step=step, use_uright=stereo, kp_block=blks,
                           th=cth, mono=mono, check_orientation=check)
    be.synchronize()
    total = 0
    for f, pts in enumerate(point_lists):
        kps, desc, xy, cs, ci, ur = imgs[f * step]
        m, nm, hist, _ = _restate(case, pts, pose, kps, desc, xy, ur, b, cs, ci, blks[f] if blks else None, scale)
        gm, gnm, ghist = be.track_matches(f)
        np.testing.assert_array_equal(gm, m, err_msg="frame %d" % f)
        assert gnm == nm, (f, gnm, nm)
        np.testing.assert_array_equal(ghist, hist, err_msg="frame %d histogram" % f)
        total += nm
    return total


def _gpu_scene(env, case, packed=False):
    _, imgs, b, _ = env
    step = case[7]
    nf = 2 if step == 2 else 4
    lists, blks, pose = [], [], None
    for f in range(nf):
        kps, desc, xy, _, _, ur = imgs[f * step]
        pts, pose = _scene_points(case, 200 + f, xy, kps, desc, ur, b)
        lists.append(pts)
        blks.append(_scene_block(len(kps), 30 + f))
    total = _gpu_compare(env, case, lists, pose, blks if case[6] else None, packed)
    assert total >= 100 * nf


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gpu_track_by_projection_bit_exact(gpu_env, case):
    _gpu_scene(gpu_env, case)


@pytest.mark.gpu
def test_gpu_track_by_projection_points_plus_offsets(gpu_env):
    _gpu_scene(gpu_env, CASES[0], packed=True)


@pytest.mark.gpu
def test_gpu_track_by_projection_dense_conflicts(gpu_env):
    """4000 points aimed at 100 keypoints of one frame, half of them without observations: the
    kept candidate lists run dry and windows are walked again."""
    _, imgs, b, _ = gpu_env
    case = CASES[2]
    kps, desc, xy, _, _, ur = imgs[0]
    pts, pose = _scene_points(case, 300, xy, kps, desc, ur, b, n=4000, pool=100, obs_fraction=0.5)
    assert _gpu_compare(gpu_env, case, [pts], pose, None) >= 50
    # the input does what the case is for: lists run dry, and some of those points still match
    kps, desc, xy, cs, ci, ur = imgs[0]
    cnt = _restate(case, pts, pose, kps, desc, xy, ur, b, cs, ci, None, gpu_env[3])[3]
    assert cnt["list_dry"] > cnt["list_dry_needed"] >= cnt["list_dry_matched"] >= 5 and cnt["overwrite"] >= 5


@pytest.mark.gpu
def test_gpu_track_by_projection_empty_point_list(gpu_env):
    import orbslam3lib_amd as og
    be = gpu_env[0]
    pose, _ = _scene_pose(0.01)
    be.track_by_projection([np.zeros(0, og.LAST_POINT_DTYPE)], np.array([pose], og.TRACK_POSE_DTYPE), K_, MBF, MB)
    gm, gnm, ghist = be.track_matches(0)
    assert gnm == 0 and len(gm) > 0 and (gm == -1).all() and (ghist == 0).all()


@pytest.mark.gpu
def test_gpu_track_by_projection_resolve_group_boundary(gpu_env):
    """Frames of exactly 64 and of 65 points: the resolve pass replays 64 lanes at a time."""
    _, imgs, b, _ = gpu_env
    case = CASES[2]
    lists, pose = [], None
    for f, n in enumerate((64, 65)):
        kps, desc, xy, _, _, ur = imgs[2 * f]
        pts, pose = _scene_points(case, 400 + f, xy, kps, desc, ur, b, n=n, pool=20)
        lists.append(pts)
    assert _gpu_compare(gpu_env, case, lists, pose, None) >= 10


@pytest.mark.gpu
def test_gpu_track_by_projection_status_codes():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    pose, _ = _scene_pose(0.01)
    args = ([np.zeros(4, og.LAST_POINT_DTYPE)], np.array([pose], og.TRACK_POSE_DTYPE), K_, MBF, MB)
    with pytest.raises(og.OrbGpuError) as e:  # before undistort_grid
        be.track_by_projection(*args, use_uright=False)
    assert e.value.code == -3
    be.undistort_grid(K_, D_)
    with pytest.raises(og.OrbGpuError) as e:  # mvuRight before stereo_matches
        be.track_by_projection(*args, use_uright=True)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:
        be.track_by_projection(*args, use_uright=False, image_step=3)
    assert e.value.code == -3
    with pytest.raises(og.OrbGpuError) as e:  # more frames than the gridded batch holds
        be.track_by_projection(args[0] * 2, np.array([pose] * 2, og.TRACK_POSE_DTYPE), K_, MBF, MB, use_uright=False)
    assert e.value.code == -3
    be.track_by_projection(*args, use_uright=False)
    assert be.track_matches(0)[1] == 0  # four invalid points
    be.close()
