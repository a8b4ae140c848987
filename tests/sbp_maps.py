"""Directed map-point sets for ORBmatcher::SearchByProjection (numpy and the CPU oracle's extractor
only, seeded, no files).  Every field of a map point is an input of the search, so each point here
is aimed: at a keypoint, a window edge, a grid exit, or at what an earlier point of the same call
left behind.  tests/test_sbp_reach.py runs the coded CPU oracle over every set in the three modes
(pinhole without / with mvuRight, two-camera), asserts the reach table MINIMA and the per-point
expectations the builders record (test_maps_exercise_every_path), and then runs the gfx950
kernels on the same sets.

Frames (synth.stereo_pair(., ., 50), CPU-extracted):
  a640     640 x 480, 8 levels, 1000 features, no distortion (level-0 coordinates are integers)
  a640d    the same keypoints under the EuRoC distortion coefficients (pinhole modes only)
  c320     320 x 240, 6 levels, 500 features, no distortion (grid_inv 0.2 instead of 0.1)
  flat320  a constant image: no keypoints at all
The device contexts the GPU tests build are CONTEXTS: "640" holds one pair, "320" holds the c320
pair nine times and the flat pair once, so a set can give every frame slot its own points.  Ten
pairs are more than the two or three a context was meant to hold: the count batch needs nine point
counts and a flat frame in one call, the frames are 320 x 240, and each GPU test stays under 0.5 s.

A set is a Set tuple; mps / blk / l2r / r2l are lists with one entry per frame slot of its context.
`expect` maps a replay event to the points built for it, each (mode, slot, point, window, fields):
the oracle's record of that point must show exactly `fields`, else the construction did not do what
it was built for.  Constructions that need a configuration a frame may lack search for it; what they
found is counted in `found` and asserted through MINIMA like the oracle's own counts.

Measured with the CPU oracle over all sets and modes (every count stands in brackets next to its
minimum in MINIMA at the end of this module; the minimum asserted is half the count).  The replay
events, read with the kernels' constants (4 list slots, groups of 64, chunks of 128): the left list
runs dry 234 times (59 of them in windows of exactly five), the right list 11 times (all of exactly
five: no window of 4 scale[level] px on these frames holds six keypoints of two levels); 30 points
free a keypoint taken in the same call, 6 free one occupied before it (at point 0, in the last
tenth, or not at all, per replay set); the right best is the point's own left partner 12 times, and
12 points assign one keypoint twice; two chains of 64 points each stale behind the one before; six
groups of 64 in which nothing is stale; dry windows whose takers sit in the victim's group, the
next group and the next chunk (24 / 24 / 24 left, 6 / 3 / 2 right).  The dry windows are built
with three takers, which leave one live entry in the list (the form whose outcome depends on the
second walk); six more have all four entries taken (dry_window(drain_all=True) says what that
form can and cannot tell).  Windows that cross one side of the grid alone and hold a keypoint: 20 to
24 per side (built.clip_*)."""
import collections
import functools

import numpy as np

from orbslam3lib_amd import synth

F32 = np.float32
K_ = (458.654, 457.296, 367.215, 248.375)
D_ = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
MBF, MB = 47.9, float(np.float32(47.9) / np.float32(435.2))
IN_VIEW, BAD, HAS_OBS, IN_VIEW_R = 1, 2, 4, 8
MODES = ("pin", "pinur", "two")  # use_uright False / True, search_by_projection_stereo

CONTEXTS = {
    "640": dict(width=640, height=480, nlevels=8, nfeatures=1000, frames=("a640",)),
    "320": dict(width=320, height=240, nlevels=6, nfeatures=500, frames=("c320",) * 9 + ("flat320",)),
}

Frame = collections.namedtuple("Frame", "name width height nlevels nfeatures images kps L R cell bounds uright scale")
Set = collections.namedtuple("Set", "name ctx dist th nnratio far th_far mps blk l2r r2l expect found")

_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int64)


def ham(a, b):
    return int(_POP[a ^ b].sum())


@functools.lru_cache(maxsize=None)
def frames():
    """name -> Frame.  L / R = (xy, octave, desc, cell_start, cell_idx) as the oracle takes them."""
    from oracle import oracle_py as O
    out = {}

    def add(name, images, w, h, nlevels, nf, dist):
        sides, kps, cells = [], [], []
        for img in images:
            k, d, _ = O.extract(img, nfeatures=nf, nlevels=nlevels)
            xy, b, cell, cs, ci = O.undistort_grid(k, K_, dist, w, h)
            sides.append((xy, k["octave"].astype(np.int32), d.reshape(-1, 32), cs, ci))
            kps.append(k)
            cells.append(cell)
        ur = np.zeros(0, np.float32)
        if len(kps[0]):
            ur = O.stereo_matches(kps[0], sides[0][2], kps[1], sides[1][2], O.pyramid(images[0], nlevels=nlevels),
                                  O.pyramid(images[1], nlevels=nlevels), MBF, MB)[0]
        for a in images:
            a.setflags(write=False)
        out[name] = Frame(name, w, h, nlevels, nf, images, tuple(kps), sides[0], sides[1] if not dist else None,
                          tuple(cells), b, ur, O.scale_factors(1.2, nlevels)[0])
    pair = tuple(a.copy() for a in synth.stereo_pair(480, 640, 50))
    add("a640", pair, 640, 480, 8, 1000, ())
    add("a640d", pair, 640, 480, 8, 1000, D_)
    add("c320", tuple(a.copy() for a in synth.stereo_pair(240, 320, 50)), 320, 240, 6, 500, ())
    flat = np.full((240, 320), 128, np.uint8)
    add("flat320", (flat, flat.copy()), 320, 240, 6, 500, ())
    return out


def frame_of(s, slot):
    name = CONTEXTS[s.ctx]["frames"][slot]
    return frames()[name + "d" if s.dist else name]


def mp_dtype():
    from oracle import oracle_py as O
    return O.MP_DTYPE


# ---- descriptor surgery ---------------------------------------------------------------------------

def flipped(d, positions):
    b = np.unpackbits(d)
    b[np.asarray(positions, np.int64)] ^= 1
    return np.packbits(b)


def flip_n(d, n, rng):
    return flipped(d, rng.choice(256, n, replace=False))


def between(da, db, A, B, rng):
    """A descriptor at Hamming distance A from da and B from db, or None: t of the bits where they
    differ are taken from db, c of the bits where they agree are flipped (A = t + c, B = H - t + c)."""
    ba, bb = np.unpackbits(da), np.unpackbits(db)
    diff, same = np.flatnonzero(ba != bb), np.flatnonzero(ba == bb)
    H = len(diff)
    if (A - B + H) % 2:
        return None
    t = (A - B + H) // 2
    c = A - t
    if not (0 <= t <= H and 0 <= c <= len(same)):
        return None
    q = ba.copy()
    q[rng.choice(diff, t, replace=False)] ^= 1
    q[rng.choice(same, c, replace=False)] ^= 1
    return np.packbits(q)


def step(x, n):
    """x moved by n float32 ulps."""
    x = F32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, F32(np.inf) if n > 0 else F32(-np.inf))
    return x


def solve_offset(target, rs, sign):
    """Coordinates x on the `sign` side of `target` whose float32 distance |target - x| is exactly rs
    ("eq", None when the float grid has no such x), the largest one below rs ("in") and the smallest
    one above it ("out")."""
    x0 = F32(target - F32(sign) * rs)
    best = {"eq": None, "in": None, "out": None}
    for n in range(-6, 7):
        x = step(x0, n)
        d = abs(F32(target - x))
        if d == rs:
            best["eq"] = x
        elif d < rs and (best["in"] is None or d > abs(F32(target - best["in"]))):
            best["in"] = x
        elif d > rs and (best["out"] is None or d < abs(F32(target - best["out"]))):
            best["out"] = x
    return best


# ---- the builder ----------------------------------------------------------------------------------

class Builder:
    """Points for one frame.  Keypoints inside the windows of a finished construction are claimed:
    a later construction is placed only where its windows touch none of them, so constructions do
    not disturb each other (unless a point has no observations and leaves nothing behind)."""

    def __init__(self, fr, th, seed):
        self.fr, self.th = fr, F32(th)
        self.rng = np.random.default_rng(seed)
        self.pts = []
        nl = len(fr.L[1])
        nr = len(fr.R[1]) if fr.R is not None else 0
        self.nl, self.nr = nl, nr
        self.used = (set(), set())
        self.l2r = np.full(nl, -1, np.int32)
        self.r2l = np.full(nr, -1, np.int32)
        self.blk = np.zeros(nl + nr, np.uint8)
        self.expect = collections.defaultdict(list)
        self.found = collections.Counter()
        self._windows, self._order = {}, {}

    def side(self, eye):
        return self.fr.L if eye == 0 else self.fr.R

    def radius(self, eye, lvl, r=4.0):
        r = F32(r)
        if eye == 0 and self.th != 1.0:
            r = F32(r * self.th)
        return F32(r * self.fr.scale[lvl])

    def window(self, eye, x, y, lvl, rs):
        """Keypoints of GetFeaturesInArea(x, y, rs, lvl - 1, lvl), in window order (grid column,
        row, index)."""
        xy, octv = self.side(eye)[:2]
        if len(octv) == 0:
            return np.zeros(0, np.int64)
        ok = (octv >= lvl - 1) & (octv <= lvl) & (np.abs((xy[:, 0] - F32(x)).astype(F32)) < rs) \
            & (np.abs((xy[:, 1] - F32(y)).astype(F32)) < rs) & (self.fr.cell[eye] >= 0)
        k = np.flatnonzero(ok)
        return k[np.lexsort((k, self.fr.cell[eye][k]))]

    def window_at(self, eye, k, r=4.0):
        """The window of a point projected on keypoint k of `eye` at k's level (cached)."""
        key = (eye, int(k), float(r))
        if key not in self._windows:
            xy, octv = self.side(eye)[:2]
            lvl = int(octv[k])
            self._windows[key] = self.window(eye, xy[k, 0], xy[k, 1], lvl, self.radius(eye, lvl, r))
        return self._windows[key]

    def take(self, eye=0, r=4.0, levels=None, need=1, ok=None):
        """Claims and returns a keypoint of `eye` (the first in a seeded order) whose own window of
        radius r holds exactly `need` keypoints and touches no claimed one.  need None: any unclaimed
        keypoint, and only the keypoint itself is claimed -- enough for a point that carries the
        keypoint's own descriptor, which takes it at distance 0 whatever else its window holds."""
        octv = self.side(eye)[1]
        if eye not in self._order:
            self._order[eye] = self.rng.permutation(len(octv))
        for k in self._order[eye]:
            if levels is not None and int(octv[k]) not in levels:
                continue
            w = [k] if need is None else self.window_at(eye, k, r)
            if (need is None or len(w) == need) and self.free(eye, w) and (ok is None or ok(int(k))):
                self.claim(eye, w)
                return int(k)
        raise RuntimeError("no isolated keypoint left (eye %d, r %g, levels %s)" % (eye, r, levels))

    def free(self, eye, kps):
        return not (set(int(k) for k in kps) & self.used[eye])

    def claim(self, eye, kps):
        self.used[eye].update(int(k) for k in kps)

    def point(self, **kw):
        p = np.zeros((), mp_dtype())
        p["view_cos"] = p["view_cos_r"] = F32(0.99)
        p["depth"] = F32(5.0)
        p["level_r"] = -1
        p["proj_x"] = p["proj_y"] = p["proj_xr"] = p["proj_yr"] = F32(-1000.0)
        for key, val in kw.items():
            p[key] = val
        return p

    def aim(self, k=None, kr=None, obs=True, desc=None, **kw):
        """A point whose left window is centred on left keypoint k and / or whose right window is
        centred on right keypoint kr, with that keypoint's level and (by default) descriptor.  In
        the pinhole mode with mvuRight, proj_xr agrees with mvuRight[k] unless kr moves it."""
        f = dict(flags=(HAS_OBS if obs else 0))
        if k is not None:
            xy, octv, dsc = self.fr.L[:3]
            f.update(proj_x=xy[k, 0], proj_y=xy[k, 1], level=int(octv[k]), desc=dsc[k])
            f["flags"] |= IN_VIEW
            f["proj_xr"] = self.fr.uright[k] if self.fr.uright[k] > 0 else xy[k, 0]
        if kr is not None:
            xy, octv, dsc = self.fr.R[:3]
            f.update(proj_xr=xy[kr, 0], proj_yr=xy[kr, 1], level_r=int(octv[kr]))
            if k is None:
                f["desc"] = dsc[kr]
            f["flags"] |= IN_VIEW_R
        if desc is not None:
            f["desc"] = desc
        flags = kw.pop("flags", None)
        f.update(kw)
        if flags is not None:
            f["flags"] = flags
        return self.point(**f)

    def add(self, p):
        self.pts.append(p)
        return len(self.pts) - 1

    def pad_to(self, offset, modulus=64):
        """Points that are not in view until the next index is `offset` modulo `modulus`."""
        while len(self.pts) % modulus != offset:
            self.add(self.point())

    def want(self, event, idx, win, modes=MODES, **fields):
        for m in modes:
            if m != "two" or self.fr.R is not None:
                self.expect[event].append((m, idx, win, fields))

    def result(self):
        return np.stack(self.pts) if self.pts else np.zeros(0, mp_dtype())


def isolated(b, eye, r=4.0, levels=None, need=1):
    """Keypoints of `eye` in a seeded order whose own window (radius r) holds exactly `need`
    keypoints of its levels and touches no claimed keypoint."""
    octv = b.side(eye)[1]
    for k in b.rng.permutation(len(octv)):
        if levels is not None and int(octv[k]) not in levels:
            continue
        w = b.window_at(eye, k, r)
        if len(w) == need and b.free(eye, w):
            yield int(k), w


# ---- boundary sets ----------------------------------------------------------------------------------

def gates(fr, seed):
    """The map-point prologue and the radius rule: view flags, isBad, the far-point cull at
    equality, levels at both ends and beyond, the viewing cosine at float32(0.998) and beside it."""
    from oracle import oracle_py as O
    b = Builder(fr, 1.0, seed)
    two = fr.R is not None
    nlv = fr.nlevels
    th_far = F32(20.0)

    def nxt(levels=None, r=4.0):
        return b.take(0, r, levels)
    for rep in range(3):
        k = nxt()
        i = b.add(b.aim(k, flags=HAS_OBS))
        b.want("gate", i, 0, code=O.SBP_NOT_IN_VIEW)
        i = b.add(b.aim(k, flags=IN_VIEW | BAD | HAS_OBS))
        b.want("gate", i, 0, code=O.SBP_BAD)
        i = b.add(b.aim(k, depth=np.nextafter(th_far, F32(np.inf))))
        b.want("gate", i, 0, code=O.SBP_FAR)
        i = b.add(b.aim(k, depth=th_far))  # equality passes the cull
        b.want("far_eq", i, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_LEVELS, flags=O.SBPF_FAR_EQ)
        # levels: -1, nlevels, 127 are refused; 0 and nlevels - 1 are searched
        for lvl in (-1, nlv, 127):
            i = b.add(b.aim(nxt(), level=lvl))
            b.want("level", i, 0, code=O.SBP_LEVEL_RANGE)
        for lvl in (0, nlv - 1):
            i = b.add(b.aim(nxt(levels=(lvl,))))
            b.want("level", i, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_LEVELS)
        # the viewing cosine: the keypoint 3 scale[level] px beside the projection lies inside the
        # 4.0 window and outside the 2.5 one.  float32(0.998) is above 0.998 as a double.
        c = F32(0.998)
        for vc, near in ((c, True), (np.nextafter(c, F32(2)), True), (np.nextafter(c, F32(0)), False)):
            k = nxt(r=8.0)
            dx = F32(3.0) * fr.scale[fr.L[1][k]]
            i = b.add(b.aim(k, proj_x=F32(fr.L[0][k, 0] + dx), view_cos=vc))
            b.want("view_cos", i, 0, modes=("pin", "two"),
                   code=O.SBP_NO_KEYPOINT if near else O.SBP_ACCEPT_LEVELS)
    if two:
        def nxtr(levels=None, r=4.0):
            return b.take(1, r, levels)
        for rep in range(3):
            for lvl, code in ((-1, O.SBP_LEVEL_R_M1), (nlv, O.SBP_LEVEL_RANGE), (127, O.SBP_LEVEL_RANGE)):
                i = b.add(b.aim(None, nxtr(), level_r=lvl))
                b.want("level_r", i, 1, modes=("two",), code=code)
            for lvl in (0, nlv - 1):
                i = b.add(b.aim(None, nxtr(levels=(lvl,))))
                b.want("level_r", i, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS)
            c = F32(0.998)
            for vc, near in ((c, True), (np.nextafter(c, F32(2)), True), (np.nextafter(c, F32(0)), False)):
                k = nxtr(r=8.0)
                dx = F32(3.0) * fr.scale[fr.R[1][k]]
                i = b.add(b.aim(None, k, proj_xr=F32(fr.R[0][k, 0] + dx), view_cos_r=vc))
                b.want("view_cos_r", i, 1, modes=("two",), code=O.SBP_NO_KEYPOINT if near else O.SBP_ACCEPT_LEVELS)
            # a left window that matches with a right level of -1 behind it
            i = b.add(b.aim(nxt(), nxtr(), level_r=-1))
            b.want("level_r", i, 1, modes=("two",), code=O.SBP_LEVEL_R_M1)
    return Set("gates_" + fr.name, "640" if fr.width == 640 else "320", fr.name.endswith("d"), 1.0, 0.8, True,
               float(th_far), [b.result()], None, None, None, dict(b.expect), b.found)


def edges(fr, seed, per_level=3):
    """The strict `<` of the window test and the `>` of the mvuRight test, per level: a projection
    whose float32 distance to the keypoint is the half-size exactly, the nearest one inside and the
    nearest one outside.  The points carry no observations, so the three of a keypoint do not see
    each other; the order (inside, equal, outside) leaves the inside point's match standing."""
    from oracle import oracle_py as O
    b = Builder(fr, 1.0, seed)
    xy, octv = fr.L[:2]
    for lvl in range(fr.nlevels):
        n = 0
        for k, w in isolated(b, 0, r=8.0, levels=(lvl,)):
            if n == per_level:
                break
            axis, sign = n % 2, (1, -1)[(n // 2) % 2]
            rs = b.radius(0, lvl, 4.0)
            sol = solve_offset(xy[k, axis], rs, sign)
            if sol["in"] is None or sol["out"] is None:
                continue
            b.claim(0, w)
            n += 1
            b.found["edge_pair_level_%d" % lvl] += 1
            key = ("proj_x", "proj_y")[axis]
            for kind in ("in", "eq", "out"):
                if sol[kind] is None:
                    continue
                i = b.add(b.aim(k, obs=False, **{key: sol[kind]}))
                b.found["edge_" + kind] += 1
                if kind == "in":
                    b.want("edge", i, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_LEVELS)
                else:  # (another keypoint may sit on the edge by chance: level-0 coordinates are integers)
                    b.want("edge", i, 0, code=O.SBP_NO_KEYPOINT, flags=O.SBPF_EDGE if kind == "eq" else 0)
        assert n, "no inside / outside pair at level %d of %s" % (lvl, fr.name)  # "per level" holds per frame
    # mvuRight: |proj_xr - mvuRight[k]| > rs rejects, equality does not
    n = 0
    for k, w in isolated(b, 0):
        if fr.uright[k] <= 0:
            continue
        if n == 4 * per_level:
            break
        rs = b.radius(0, int(octv[k]), 4.0)
        sol = solve_offset(fr.uright[k], rs, (1, -1)[n % 2])
        if sol["in"] is None or sol["out"] is None:
            continue
        b.claim(0, w)
        n += 1
        for kind in ("in", "eq", "out"):
            if sol[kind] is None:
                continue
            i = b.add(b.aim(k, obs=False, proj_xr=sol[kind]))
            b.found["uright_" + kind] += 1
            if kind == "out":
                b.want("uright", i, 0, modes=("pinur",), code=O.SBP_ALL_TAKEN, flags=O.SBPF_URIGHT_REJECT)
            else:
                b.want("uright", i, 0, modes=("pinur",), code=O.SBP_ACCEPT_LEVELS,
                       flags=O.SBPF_URIGHT_EQ if kind == "eq" else 0)
    return Set("edges_" + fr.name, "640" if fr.width == 640 else "320", fr.name.endswith("d"), 1.0, 0.8, False,
               50.0, [b.result()], None, None, None, dict(b.expect), b.found)


def pairs_in_window(b, same_octave):
    """Ordered pairs (i, j) of left keypoints: a point projected on i at i's level (radius 4.0) sees
    exactly i and j; j has i's octave, or the one below it."""
    octv = b.fr.L[1]
    for i in b.rng.permutation(len(octv)):
        w = b.window_at(0, i)
        if len(w) != 2:
            continue
        j = int(w[0] if w[1] == i else w[1])
        if (octv[j] == octv[i]) == same_octave:
            yield int(i), j, [int(v) for v in w]


def descriptors(fr, seed, nnratio):
    """Distances made by bit surgery between two keypoints' descriptors: TH_HIGH at 99 / 100 / 101,
    the ratio test at equality and one bit either side (nnratio 0.5 and 0.75 are exact in float),
    ties on different levels in both window orders, a ratio reject with a right window pending."""
    from oracle import oracle_py as O
    b = Builder(fr, 1.0, seed)
    two = fr.R is not None
    desc, octv = fr.L[2], fr.L[1]
    num, den = (1, 2) if nnratio == 0.5 else (3, 4)
    for n, (k, w) in enumerate(isolated(b, 0)):
        if n == 9:
            break
        b.claim(0, w)
        d = (99, 100, 101)[n % 3]
        i = b.add(b.aim(k, desc=flip_n(desc[k], d, b.rng)))
        b.want("th_high", i, 0, modes=("pin", "two"), code=O.SBP_TH_HIGH if d > 100 else O.SBP_ACCEPT_LEVELS,
               flags=O.SBPF_BD_100 if d == 100 else 0)
    # the ratio test: best on i at A, second on j at B, A * den == B * num
    n = 0
    for i, j, w in pairs_in_window(b, True):
        if not b.free(0, w):
            continue
        H = ham(desc[i], desc[j])
        sols = [(m * num, m * den) for m in range(1, 100 // num + 1)
                if (m * (num + den) - H) % 2 == 0 and m * (num + den) >= H + 2 and m * num + 1 <= 100 and m * num < H]
        if not sols:
            continue
        A, B = sols[len(sols) // 2]
        qs = [between(desc[i], desc[j], A + e, B + e, b.rng) for e in (0, 1, -1)]
        if any(q is None for q in qs):
            continue
        b.claim(0, w)
        kr = None
        if two:
            kr = b.take(1)
        for e, q in zip((0, 1, -1), qs):
            # the rejected one has a right window pending, which the `continue` skips
            p = b.aim(i, kr if e == 1 else None, obs=False, desc=q)
            idx = b.add(p)
            if e == 1:
                b.want("ratio", idx, 0, modes=("pin",), code=O.SBP_RATIO)
                if two:
                    b.want("ratio_skips_right", idx, 0, modes=("two",), code=O.SBP_RATIO, flags=O.SBPF_SKIPPED_RIGHT)
                    b.want("ratio_skips_right", idx, 1, modes=("two",), code=O.SBP_SKIPPED)
            else:
                b.want("ratio", idx, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_RATIO,
                       flags=O.SBPF_RATIO_EQ if e == 0 else 0)
        n += 1
        if n == 8:
            break
    b.found["ratio_pairs"] = n
    # ties on different levels (accepted whatever the ratio): the first in window order wins
    n = 0
    for i, j, w in pairs_in_window(b, False):
        if not b.free(0, w):
            continue
        H = ham(desc[i], desc[j])
        A = (H + 1) // 2 + 3
        if H % 2 or A > 100:
            continue
        q = between(desc[i], desc[j], A, A, b.rng)
        if q is None:
            continue
        b.claim(0, w)
        idx = b.add(b.aim(i, desc=q))
        b.want("tie", idx, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_LEVELS,
               flags=O.SBPF_TIE_BEST | O.SBPF_BEST_EQ_SECOND)
        b.found["tie_window_order_is_index_order" if w == sorted(w) else "tie_window_order_differs"] += 1
        n += 1
        if n == 12:
            break
    # a tie on one level is rejected by the ratio test whatever the order
    for i, j, w in pairs_in_window(b, True):
        if not b.free(0, w) or ham(desc[i], desc[j]) % 2:
            continue
        A = ham(desc[i], desc[j]) // 2 + 2
        q = between(desc[i], desc[j], A, A, b.rng)
        if q is None:
            continue
        b.claim(0, w)
        idx = b.add(b.aim(i, desc=q))
        b.want("tie_same_level", idx, 0, modes=("pin", "two"), code=O.SBP_RATIO,
               flags=O.SBPF_TIE_BEST | O.SBPF_BEST_EQ_SECOND)
        break
    name = "desc%d_%s" % (round(nnratio * 100), fr.name)
    return Set(name, "640" if fr.width == 640 else "320", fr.name.endswith("d"), 1.0, nnratio, False, 50.0,
               [b.result()], None, None, None, dict(b.expect), b.found)


def tie_second(fr, seed, th=3.0):
    """A tie between the second and the third candidate that lie on different levels: which one is
    kept as second decides whether the ratio test applies at all.  The point's descriptor is the
    best keypoint's with bits moved until the two others are equally far."""
    from oracle import oracle_py as O
    b = Builder(fr, th, seed)
    desc, octv = fr.L[2], fr.L[1]
    n = 0
    for k in b.rng.permutation(len(octv)):
        w = [int(v) for v in b.window_at(0, k)]
        if len(w) != 3 or not b.free(0, w):
            continue
        o1, o2 = [v for v in w if v != k]
        if octv[o1] == octv[o2]:
            continue
        d1, d2 = ham(desc[k], desc[o1]), ham(desc[k], desc[o2])
        if (d1 - d2) % 2:
            continue
        far_, near = (o1, o2) if d1 > d2 else (o2, o1)
        # bits where far_ and near differ and the best agrees with near: flipping one brings far_
        # one closer and near one further
        bk, bf, bn = (np.unpackbits(desc[v]) for v in (k, far_, near))
        pos = np.flatnonzero((bf != bn) & (bk == bn))
        need = abs(d1 - d2) // 2
        if need > len(pos) or need >= min(d1, d2) - need:
            continue
        q = flipped(desc[k], pos[:need]) if need else desc[k].copy()
        if not (ham(q, desc[k]) < ham(q, desc[o1]) == ham(q, desc[o2]) and need > 0):
            continue
        b.claim(0, w)
        idx = b.add(b.aim(k, desc=q))
        b.want("tie_second", idx, 0, modes=("pin", "two"), flags=O.SBPF_TIE_SECOND)
        n += 1
        if n == 8:
            break
    return Set("tie2_" + fr.name, "640" if fr.width == 640 else "320", False, th, 0.8, False, 50.0,
               [b.result()], None, None, None, dict(b.expect), b.found)


def grid(fr, seed):
    """The four early returns of GetFeaturesInArea, each just inside and just outside; windows
    clipped on every side; cell-range products that are integers (x - rs == 0, x + rs == maxX) or
    that ceil turns into -0."""
    from oracle import oracle_py as O
    b = Builder(fr, 1.0, seed)
    x0, x1, y0, y1 = (F32(v) for v in fr.bounds)
    wi, hi = F32(F32(64) / F32(x1 - x0)), F32(F32(48) / F32(y1 - y0))
    rs = b.radius(0, 0, 2.5)
    cx, cy = F32((x0 + x1) / 2), F32((y0 + y1) / 2)

    def prod(v, lo, s, inv):
        return F32(F32(F32(v - lo) + F32(s) * rs) * inv)

    def scan(start, lo, s, inv, pred):
        """From `start`, where pred(product) is false, upwards: the last coordinate where it is still
        false and the first where it is true (bisection; the product is monotonic in the coordinate)."""
        a, c = F32(start), F32(start + F32(100))
        assert not pred(prod(a, lo, s, inv)) and pred(prod(c, lo, s, inv))
        while step(a, 1) != c:
            m = F32((np.float64(a) + np.float64(c)) / 2)
            if m == a or m == c:
                m = step(a, 1)
            if pred(prod(m, lo, s, inv)):
                c = m
            else:
                a = m
        return a, c
    pts = {}
    # nMinCellX >= 64 / nMinCellY >= 48: the first coordinate whose floor reaches the grid's end
    ins, out = scan(x1 - F32(1), x0, -1, wi, lambda p: np.floor(p) >= 64)
    pts["exit_minx"] = (dict(proj_x=ins, proj_y=cy), dict(proj_x=out, proj_y=cy), O.SBP_EXIT_MINX)
    ins, out = scan(y1 - F32(1), y0, -1, hi, lambda p: np.floor(p) >= 48)
    pts["exit_miny"] = (dict(proj_x=cx, proj_y=ins), dict(proj_x=cx, proj_y=out), O.SBP_EXIT_MINY)
    # nMaxCellX < 0 / nMaxCellY < 0: scanning upwards, the last coordinate whose ceil is still negative
    out, ins = scan(x0 - F32(40), x0, 1, wi, lambda p: np.ceil(p) >= 0)
    pts["exit_maxx"] = (dict(proj_x=ins, proj_y=cy), dict(proj_x=out, proj_y=cy), O.SBP_EXIT_MAXX)
    out, ins = scan(y0 - F32(40), y0, 1, hi, lambda p: np.ceil(p) >= 0)
    pts["exit_maxy"] = (dict(proj_x=cx, proj_y=ins), dict(proj_x=cx, proj_y=out), O.SBP_EXIT_MAXY)
    for name, (inside, outside, code) in pts.items():
        i = b.add(b.point(flags=IN_VIEW | HAS_OBS, level=0, view_cos=F32(0.9995), **inside))
        b.want("grid_exit", i, 0, code=O.SBP_NO_KEYPOINT)
        i = b.add(b.point(flags=IN_VIEW | HAS_OBS, level=0, view_cos=F32(0.9995), **outside))
        b.want("grid_exit", i, 0, code=code)
        if fr.R is not None:  # the same two through the right window
            for kw, c in ((inside, O.SBP_NO_KEYPOINT), (outside, code)):
                i = b.add(b.point(flags=IN_VIEW_R | HAS_OBS, level_r=0, view_cos_r=F32(0.9995),
                                  proj_xr=kw["proj_x"], proj_yr=kw["proj_y"]))
                b.want("grid_exit_right", i, 1, modes=("two",), code=c)
    # integer products and the -0 of ceil
    for kw in (dict(proj_x=F32(x0 + rs), proj_y=cy), dict(proj_x=F32(x1 - rs), proj_y=cy),
               dict(proj_x=cx, proj_y=F32(y0 + rs)), dict(proj_x=cx, proj_y=F32(y1 - rs))):
        i = b.add(b.point(flags=IN_VIEW | HAS_OBS, level=0, view_cos=F32(0.9995), **kw))
        if not fr.name.endswith("d"):  # round bounds: the product is 0 or the grid size exactly
            b.want("cell_int", i, 0, flags=O.SBPF_CELL_INT)
    for kw in (dict(proj_x=F32(x0 - rs - F32(0.5)), proj_y=cy), dict(proj_x=cx, proj_y=F32(y0 - rs - F32(0.5)))):
        i = b.add(b.point(flags=IN_VIEW | HAS_OBS, level=0, view_cos=F32(0.9995), **kw))
        b.want("minus_zero", i, 0, code=O.SBP_NO_KEYPOINT, flags=O.SBPF_CLIPPED)
    return Set("grid_" + fr.name, "640" if fr.width == 640 else "320", fr.name.endswith("d"), 1.0, 0.8, False, 50.0,
               [b.result()], None, None, None, dict(b.expect), b.found)


SIDES = ("minx", "maxx", "miny", "maxy")


def clipped(fr, seed, th=5.0, per_side=3):
    """Windows that cross exactly one side of the grid and still hold a keypoint.  Keypoints keep
    19 scale[octave] px from the image border, which a th = 1 window (at most 4 scale px) never
    bridges, so this set runs at th = 5: the keypoints nearest to a side in units of their window's
    half-size, the projection moved 0.9 of that towards the side.  The builder checks with the
    search's own cell arithmetic that the other three sides stay inside."""
    from oracle import oracle_py as O
    b = Builder(fr, th, seed)
    xy, octv = fr.L[:2]
    x0, x1, y0, y1 = (F32(v) for v in fr.bounds)
    wi, hi = F32(F32(64) / F32(x1 - x0)), F32(F32(48) / F32(y1 - y0))
    rs_k = np.array([b.radius(0, int(o)) for o in octv], F32)

    def crossed(x, y, rs):
        return (np.floor(F32(F32(F32(x - x0) - rs) * wi)) < 0, np.ceil(F32(F32(F32(x - x0) + rs) * wi)) > 63,
                np.floor(F32(F32(F32(y - y0) - rs) * hi)) < 0, np.ceil(F32(F32(F32(y - y0) + rs) * hi)) > 47)
    for side, name in enumerate(SIDES):
        dist = (xy[:, 0] - x0, x1 - xy[:, 0], xy[:, 1] - y0, y1 - xy[:, 1])[side] / rs_k
        n = 0
        for k in np.argsort(dist, kind="stable"):
            k = int(k)
            x, y = F32(xy[k, 0]), F32(xy[k, 1])
            shift = F32(F32(0.9) * rs_k[k]) * F32((-1, 1)[side % 2])
            x, y = (F32(x + shift), y) if side < 2 else (x, F32(y + shift))
            if crossed(x, y, rs_k[k]) != tuple(j == side for j in range(4)) or not b.free(0, [k]):
                continue
            b.claim(0, [k])
            i = b.add(b.aim(k, obs=False, proj_x=x, proj_y=y))
            b.want("clip_" + name, i, 0, flags=O.SBPF_CLIPPED, ncand_min=1)
            n += 1
            if n == per_side:
                break
        assert n, "no window of %s crosses %s alone" % (fr.name, name)
    return Set("clip_" + fr.name, "640" if fr.width == 640 else "320", fr.name.endswith("d"), th, 0.8, False, 50.0,
               [b.result()], None, None, None, dict(b.expect), b.found)


# ---- replay sets ------------------------------------------------------------------------------------

def chain(fr, seed, length=64, th=200.0):
    """th = 200: every window covers the whole grid.  Point i sits between keypoints u[i] and
    u[i + 1] in descriptor space, nearer to u[i]: before the call its best is u[i], but point i - 1
    takes u[i], so it takes u[i + 1] -- `length` consecutive points of one group, each made stale by
    the one before.  (The group in which nothing is stale is in replay().)"""
    from oracle import oracle_py as O
    b = Builder(fr, th, seed)
    desc, octv = fr.L[2], fr.L[1]
    lvl = 0
    pool = [int(k) for k in np.flatnonzero(octv == lvl)]
    u = [pool.pop(int(b.rng.integers(len(pool))))]
    while len(u) < length + 1 and pool:  # the nearest unused descriptor next
        d = [ham(desc[u[-1]], desc[k]) for k in pool]
        u.append(pool.pop(int(np.argmin(d))))
    b.add(b.aim(u[0]))  # takes u[0]
    for i in range(len(u) - 1):
        H = ham(desc[u[i]], desc[u[i + 1]])
        q = between(desc[u[i]], desc[u[i + 1]], (H - 1) // 2, H - (H - 1) // 2, b.rng)
        idx = b.add(b.aim(u[i], desc=q))
        b.want("chain", idx, 0, modes=("pin", "two"), code=O.SBP_ACCEPT_RATIO, rank_best=1,
               assigned=[u[i + 1], -1])
    b.found["chain_length"] = len(u) - 1
    # two more points over the whole grid, at other levels: clipped on every side, every keypoint of
    # two octaves a candidate
    for lv in (1, fr.nlevels - 1):
        k = int(np.flatnonzero(octv == lv)[0])
        i = b.add(b.aim(k, obs=False, desc=flip_n(desc[k], 7, b.rng)))
        b.want("whole_grid", i, 0, modes=("pin", "two"), flags=O.SBPF_CLIPPED,
               ncand=int(((octv == lv) | (octv == lv - 1)).sum()))
    return Set("chain_" + fr.name, "640" if fr.width == 640 else "320", False, th, 0.8, False, 50.0,
               [b.result()], None, None, None, dict(b.expect), b.found)


PLACEMENTS = ("same_group", "next_group", "next_chunk")


def place(b, where, n_before):
    """Leaves room so that `n_before` points and then the victim fall as `where` says: all in one
    group of 64; the victim first of the next group of the same chunk of 128; first of the next chunk."""
    if where == "same_group":
        if len(b.pts) % 64 + n_before + 1 > 64:
            b.pad_to(0)
    elif where == "next_group":
        b.pad_to((64 - n_before) % 128, 128)
    else:
        b.pad_to((128 - n_before) % 128, 128)


def dry_window(b, eye, where, walked_stale=False, drain_all=False):
    """A window of five or more candidates whose list runs dry.  The victim's descriptor is 90 bits
    from keypoint w's and further from every other; three takers with observations, aimed exactly,
    take ranks 1, 2, 3 of its four-slot list before it runs, so one live candidate is left in the
    list and the window has to be walked again for the second.  That second (rank 4, on w's level)
    rejects the victim by the ratio test at nnratio 0.5; without the second it would be accepted.
    walked_stale: the window holds exactly five, the takers sit in an earlier group, and a fourth
    taker in the victim's own group takes rank 4 -- which is in no list the victim examined -- so the
    victim is accepted with no second at all.
    drain_all: a fourth taker takes rank 0 as well, so none of the four list entries is live.  What
    the second walk then finds is rank 4, beyond TH_HIGH on these frames (five keypoints within 100
    bits of one descriptor, four of them nearer than the fifth, are not to be had), so this one
    reaches the branch without telling a kernel that skips the walk from one that does not; the
    three-taker form above is the one that tells."""
    from oracle import oracle_py as O
    xy, octv, desc = b.side(eye)[:3]
    for k in b.rng.permutation(len(octv)):
        w = b.window_at(eye, k)
        if len(w) < 5 or (walked_stale and len(w) != 5) or not b.free(eye, w):
            continue
        region = [int(v) for v in w]  # (the takers carry their targets' descriptors: distance 0 wins anywhere)
        for attempt in range(8):
            q = flip_n(desc[k], 90, b.rng)
            d = [ham(q, desc[v]) for v in w]
            order = sorted(range(len(w)), key=lambda j: d[j])  # stable: (distance, window position)
            ranked = [int(w[j]) for j in order]
            if ranked[0] != k or d[order[1]] <= 90:
                continue
            e = ranked[4]
            if octv[e] != octv[k] or 2 * 90 <= d[order[4]]:
                continue
            break
        else:
            continue
        b.claim(eye, region)
        aim = (lambda t, **kw: b.aim(t, **kw)) if eye == 0 else (lambda t, **kw: b.aim(None, t, **kw))
        if drain_all:
            place(b, where, 4)
            for t in ranked[0:4]:
                b.add(aim(t))
            v = b.add(aim(k, desc=q))
            b.want("dry_all_four_%s" % ("right" if eye else "left"), v, eye, modes=("two",) if eye else ("pin", "two"),
                   ncand=len(w), rank_best=4, flags=O.SBPF_TAKEN_SKIP)
        elif walked_stale:
            b.pad_to((64 - 3) % 128, 128)
            for t in ranked[1:4]:
                b.add(aim(t))
            b.add(aim(e))
            v = b.add(aim(k, desc=q))
            b.want("walked_stale", v, eye, modes=("two",) if eye else ("pin", "two"), code=O.SBP_ACCEPT_LEVELS,
                   ncand=5, rank_best=0, rank_second=5)
        else:
            place(b, where, 3)
            for t in ranked[1:4]:
                b.add(aim(t))
            v = b.add(aim(k, desc=q))
            b.want("dry_%s_%s" % ("right" if eye else "left", where), v, eye, modes=("two",) if eye else ("pin", "two"),
                   code=O.SBP_RATIO, ncand=len(w), rank_best=0, rank_second=4)
            if len(w) == 5:
                b.found["dry_with_exactly_five"] += 1
        return True
    return False


def stereo_pairing(b):
    """An unclaimed left keypoint and a right keypoint alone in its window, both claimed."""
    return b.take(0, need=None), b.take(1)


def precall_free(b, where):
    """Right keypoint r is occupied before the call; B, without observations, matches left keypoint
    x whose partner is r, which frees r; C's right window, aimed at r, takes it.  r is in no candidate
    list, so C must walk: stale behind B in B's group, and by the walk-all state in a later one."""
    from oracle import oracle_py as O
    x, r = stereo_pairing(b)
    b.l2r[x] = r
    b.blk[b.nl + r] = 1
    place(b, where, 1)
    i = b.add(b.aim(x, obs=False))
    b.want("precall_free", i, 0, modes=("two",), flags=O.SBPF_PARTNER | O.SBPF_FREED_PRECALL,
           assigned=[x, b.nl + r])
    c = b.add(b.aim(None, r))
    b.want("precall_free_" + where, c, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS, ncand=0, rank_best=0,
           assigned=[-1, b.nl + r])


def incall_free(b, where):
    """A (with observations) takes right keypoint r; B (without) matches left keypoint x whose partner
    is r, which frees it; C's right window takes r again."""
    from oracle import oracle_py as O
    x, r = stereo_pairing(b)
    b.l2r[x] = r
    if where == "same_group":
        place(b, where, 2)
    b.add(b.aim(None, r))
    if where != "same_group":
        b.pad_to(0)
    i = b.add(b.aim(x, obs=False))
    if where == "next_chunk":
        b.pad_to(0, 128)
    elif where == "next_group":
        b.pad_to(0)
    c = b.add(b.aim(None, r))
    b.want("incall_free", i, 0, modes=("two",), flags=O.SBPF_PARTNER | O.SBPF_FREED_INCALL | O.SBPF_OVERWROTE,
           assigned=[x, b.nl + r])
    b.want("incall_free_" + where, c, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS, flags=O.SBPF_OVERWROTE,
           assigned=[-1, b.nl + r])


def right_owner(b):
    """A's right window takes r; C, later in the same group, has r first in its right list."""
    from oracle import oracle_py as O
    r = b.take(1)
    place(b, "same_group", 1)
    b.add(b.aim(None, r))
    c = b.add(b.aim(None, r, desc=flip_n(b.fr.R[2][r], 4, b.rng)))
    b.want("right_owner", c, 1, modes=("two",), code=O.SBP_ALL_TAKEN, flags=O.SBPF_TAKEN_SKIP)


def own_partner(b, obs, taken_before):
    """One point whose right window is aimed at the partner p of its own left match x.  With
    observations its own assignment of p blocks the right window; without, p is free again (even
    when an earlier point with observations held it) and is assigned a second time, with x."""
    from oracle import oracle_py as O
    # p: alone in its right window and within 90 bits of x, whose descriptor the point carries
    dR = b.fr.R[2]
    x = b.take(0, need=None, ok=lambda k: any(
        len(b.window_at(1, c)) == 1 and b.free(1, [c]) for c in np.flatnonzero(_POP[dR ^ b.fr.L[2][k]].sum(1) <= 90)))
    p = b.take(1, ok=lambda c: ham(dR[c], b.fr.L[2][x]) <= 90)
    b.l2r[x] = p
    if not taken_before:
        b.r2l[p] = x
    place(b, "same_group", 1)
    if taken_before:
        b.add(b.aim(None, p))
    i = b.add(b.aim(x, p, obs=obs))
    if obs:
        b.want("own_partner_obs", i, 1, modes=("two",), code=O.SBP_ALL_TAKEN, flags=O.SBPF_TAKEN_SKIP)
    elif taken_before:
        b.want("own_partner_freed", i, 0, modes=("two",), flags=O.SBPF_PARTNER | O.SBPF_FREED_INCALL | O.SBPF_OVERWROTE)
        b.want("own_partner_freed", i, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS,
               flags=O.SBPF_OWN_PARTNER | O.SBPF_OVERWROTE | O.SBPF_DOUBLE_ASSIGN, assigned=[-1, b.nl + p])
    else:
        b.want("own_partner_no_obs", i, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS,
               flags=O.SBPF_OWN_PARTNER | O.SBPF_PARTNER | O.SBPF_OVERWROTE | O.SBPF_DOUBLE_ASSIGN,
               assigned=[x, b.nl + p])


def shared_keypoint(b):
    """Three points without observations and then one with, all in one group and all assigning left
    keypoint k; a point of the next group, four bits off k, must find k occupied."""
    from oracle import oracle_py as O
    k = b.take(0, need=None)
    place(b, "same_group", 4)
    for _ in range(3):
        b.add(b.aim(k, obs=False))
    o = b.add(b.aim(k))
    b.want("shared_keypoint", o, 0, modes=("pin", "two"), flags=O.SBPF_OVERWROTE, assigned=[k, -1])
    b.pad_to(0)
    z = b.add(b.aim(k, desc=flip_n(b.fr.L[2][k], 4, b.rng)))
    b.want("shared_keypoint_later", z, 0, modes=("pin", "two"), flags=O.SBPF_TAKEN_SKIP)


def shared_partner(b, obs_first):
    """Four points of one group whose left matches x[0..3] all have right keypoint p as partner: none
    of them examined p, so all four commit in one round and the last one decides p's occupancy.  One
    of the four has observations: the first (p ends free, and a point of the next group aimed at p
    takes it) or the last (p ends occupied, and that point finds it taken).  Whatever order a kernel
    applied the four in, if it did not keep the last alone, one of the two forms comes out wrong."""
    from oracle import oracle_py as O
    p = b.take(1)
    xs = [b.take(0, need=None) for _ in range(4)]
    for x in xs:
        b.l2r[x] = p
    place(b, "same_group", 4)
    for j, x in enumerate(xs):
        i = b.add(b.aim(x, obs=(j == 0) if obs_first else (j == 3)))
        b.want("shared_partner", i, 0, modes=("two",), flags=O.SBPF_PARTNER, assigned=[x, b.nl + p])
    b.pad_to(0)
    z = b.add(b.aim(None, p))
    if obs_first:
        b.want("shared_partner_ends_free", z, 1, modes=("two",), code=O.SBP_ACCEPT_LEVELS, assigned=[-1, b.nl + p])
    else:
        b.want("shared_partner_ends_taken", z, 1, modes=("two",), code=O.SBP_ALL_TAKEN, flags=O.SBPF_TAKEN_SKIP)


def replay(fr, seed, free_at, th=5.0):
    """The replay constructions on one frame at th = 5, nnratio 0.5.  free_at: where the one free of
    a keypoint occupied before the call goes -- "absent" (the candidate lists stay complete for the
    whole call), "first" (point 0: everything after it walks whole windows) or "late" (the last
    tenth of the points)."""
    from oracle import oracle_py as O
    b = Builder(fr, th, seed)
    if free_at == "first":
        precall_free(b, "same_group")
    # a group in which nothing is stale: 64 exact points whose windows hold none of the others' targets,
    # before anything else is taken
    b.pad_to(0)
    g, targets, seen = 0, set(), set()
    for k in b.rng.permutation(b.nl):
        w = set(int(v) for v in b.window_at(0, k))
        if int(k) in seen or w & targets or not b.free(0, [k]):
            continue
        targets.add(int(k))
        seen |= w
        i = b.add(b.aim(int(k)))
        b.want("quiet_group", i, 0, modes=("pin", "two"), assigned=[int(k), -1], not_flags=O.SBPF_TAKEN_SKIP)
        g += 1
        if g == 64:
            break
    b.claim(0, targets)
    b.found["quiet_group"] = g
    for where in PLACEMENTS:
        for eye in (0, 1):
            for _ in range(2 - eye):  # right windows of five are rare: one per placement
                if dry_window(b, eye, where):
                    b.found["dry_%s" % ("right" if eye else "left")] += 1
    for _ in range(2):
        if dry_window(b, 0, None, walked_stale=True):
            b.found["walked_stale"] += 1
    for where in PLACEMENTS:
        incall_free(b, where)
    right_owner(b)
    right_owner(b)
    own_partner(b, True, False)
    own_partner(b, False, False)
    own_partner(b, False, True)
    shared_keypoint(b)
    shared_partner(b, True)
    shared_partner(b, False)
    for eye in (0, 1):
        if dry_window(b, eye, "next_group", drain_all=True):
            b.found["dry_all_four_%s" % ("right" if eye else "left")] += 1
    if free_at == "late":
        while len(b.pts) < 1408 or len(b.pts) % 64:  # the 132 points that follow are the last tenth
            b.add(b.point())
        precall_free(b, "same_group")
        precall_free(b, "next_group")
    blk = b.blk.copy()
    # a tenth of the other keypoints occupied before the call, away from every construction
    rng = np.random.default_rng(seed + 1)
    for eye, base, n in ((0, 0, b.nl), (1, b.nl, b.nr)):
        for k in range(n):
            if k not in b.used[eye] and rng.random() < 0.1:
                blk[base + k] = 1
    return Set("replay_%s_%s" % (free_at, fr.name), "640" if fr.width == 640 else "320", False, th, 0.5, False, 50.0,
               [b.result()], [blk], [b.l2r], [b.r2l], dict(b.expect), b.found)


def random_points(fr, n, seed):
    """n aimed points with a few flipped bits, 80% with observations, for the count batch."""
    b = Builder(fr, 1.0, seed)
    nk = len(fr.L[1])
    for _ in range(n):
        if nk == 0:
            b.add(b.point(flags=IN_VIEW | HAS_OBS, level=int(b.rng.integers(fr.nlevels)),
                          proj_x=F32(b.rng.uniform(0, fr.width)), proj_y=F32(b.rng.uniform(0, fr.height)),
                          desc=b.rng.integers(0, 256, 32, dtype=np.uint8)))
            continue
        k = int(b.rng.integers(nk))
        kr = int(b.rng.integers(b.nr)) if b.nr and b.rng.random() < 0.5 else None
        b.add(b.aim(k, kr, obs=bool(b.rng.random() < 0.8), desc=flip_n(fr.L[2][k], int(b.rng.integers(0, 30)), b.rng)))
    return b.result()


COUNTS = (63, 1, 64, 65, 0, 127, 128, 129, 257)  # an empty frame between full ones


def counts(seed):
    """Per-frame point counts around the group (64) and chunk (128) sizes in one batch, and a flat
    frame (no keypoints) that has map points."""
    fs = frames()
    names = CONTEXTS["320"]["frames"]
    mps = [random_points(fs[nm], n, seed + i) for i, (nm, n) in enumerate(zip(names, COUNTS + (40,)))]
    return Set("counts_320", "320", False, 1.0, 0.8, False, 50.0, mps, None, None, None, {}, collections.Counter())


@functools.lru_cache(maxsize=None)
def sets():
    """The named list.  Arrays are shared between callers: treat them as read-only."""
    fs = frames()
    out = []
    for s, name in enumerate(("a640", "a640d", "c320")):
        fr = fs[name]
        out += [gates(fr, 10 + s), edges(fr, 20 + s), descriptors(fr, 30 + s, 0.5), descriptors(fr, 40 + s, 0.75),
                grid(fr, 50 + s), clipped(fr, 55 + s)]
    for s, name in enumerate(("a640", "c320")):
        fr = fs[name]
        out += [tie_second(fr, 60 + s), chain(fr, 70 + s)]
        out += [replay(fr, 80 + 3 * s + j, where) for j, where in enumerate(("absent", "first", "late"))]
    out.append(counts(90))
    # every set gives its context's frame slots one entry each
    full = []
    for st in out:
        nf = len(CONTEXTS[st.ctx]["frames"])
        pad = lambda rows, fill: None if rows is None else list(rows) + [fill(i) for i in range(len(rows), nf)]
        mps = pad(st.mps, lambda i: np.zeros(0, mp_dtype()))

        def width(i, st=st):
            fr = frame_of(st, i)
            return len(fr.L[1]), (len(fr.R[1]) if fr.R is not None else 0)
        full.append(st._replace(mps=mps, blk=pad(st.blk, lambda i: np.zeros(sum(width(i)), np.uint8)),
                                l2r=pad(st.l2r, lambda i: np.full(width(i)[0], -1, np.int32)),
                                r2l=pad(st.r2l, lambda i: np.full(width(i)[1], -1, np.int32))))
        for m in full[-1].mps:
            m.setflags(write=False)
    return tuple(full)


# What the sets reach, summed over every set and mode (left window / right window codes, flags, the
# replay events read with the kernels' constants in tests/test_sbp_reach.py::reach, the points the
# builders aimed per event, and what their searches found).  In brackets: the count the CPU oracle
# measures; the minimum asserted is half of it.
MINIMA = {
    "built.cell_int": 12,  # [24]
    "built.chain": 128,  # [256]
    "built.clip_maxx": 12,  # [24]
    "built.clip_maxy": 12,  # [24]
    "built.clip_minx": 10,  # [20]
    "built.clip_miny": 11,  # [22]
    "built.dry_all_four_left": 6,  # [12]
    "built.dry_left_next_chunk": 12,  # [24]
    "built.dry_left_next_group": 12,  # [24]
    "built.dry_left_same_group": 12,  # [24]
    "built.dry_right_next_chunk": 1,  # [2]
    "built.dry_right_next_group": 1,  # [3]
    "built.dry_right_same_group": 3,  # [6]
    "built.edge": 145,  # [290]
    "built.far_eq": 7,  # [15]
    "built.gate": 36,  # [72]
    "built.grid_exit": 32,  # [64]
    "built.grid_exit_right": 8,  # [16]
    "built.incall_free": 9,  # [18]
    "built.incall_free_next_chunk": 3,  # [6]
    "built.incall_free_next_group": 3,  # [6]
    "built.incall_free_same_group": 3,  # [6]
    "built.level": 51,  # [102]
    "built.level_r": 18,  # [36]
    "built.minus_zero": 8,  # [16]
    "built.own_partner_freed": 6,  # [12]
    "built.own_partner_no_obs": 3,  # [6]
    "built.own_partner_obs": 3,  # [6]
    "built.precall_free": 3,  # [6]
    "built.precall_free_next_group": 1,  # [2]
    "built.precall_free_same_group": 2,  # [4]
    "built.quiet_group": 384,  # [768]
    "built.ratio": 59,  # [118]
    "built.ratio_skips_right": 20,  # [40]
    "built.right_owner": 6,  # [12]
    "built.shared_keypoint": 6,  # [12]
    "built.shared_keypoint_later": 6,  # [12]
    "built.shared_partner": 24,  # [48]
    "built.shared_partner_ends_free": 3,  # [6]
    "built.shared_partner_ends_taken": 3,  # [6]
    "built.th_high": 45,  # [90]
    "built.tie": 60,  # [120]
    "built.tie_second": 12,  # [24]
    "built.uright": 45,  # [90]
    "built.view_cos": 22,  # [45]
    "built.view_cos_r": 9,  # [18]
    "built.walked_stale": 11,  # [22]
    "built.whole_grid": 4,  # [8]
    "flag.bd_100": 25,  # [51]
    "flag.best_eq_second": 93,  # [187]
    "flag.cell_int": 598,  # [1196]
    "flag.clipped": 366,  # [732]
    "flag.double_assign": 6,  # [12]
    "flag.edge": 225,  # [451]
    "flag.far_eq": 15,  # [30]
    "flag.freed_incall": 15,  # [30]
    "flag.freed_precall": 3,  # [6]
    "flag.overwrote": 201,  # [402]
    "flag.own_partner": 6,  # [12]
    "flag.partner": 48,  # [96]
    "flag.ratio_eq": 34,  # [68]
    "flag.skipped_right": 10,  # [20]
    "flag.taken_skip": 773,  # [1547]
    "flag.tie_best": 93,  # [187]
    "flag.tie_second": 42,  # [84]
    "flag.uright_eq": 9,  # [18]
    "flag.uright_reject": 255,  # [511]
    "found.chain_length": 64,  # [128]
    "found.dry_all_four_left": 3,  # [6]
    "found.dry_left": 18,  # [36]
    "found.dry_right": 5,  # [11]
    "found.dry_with_exactly_five": 8,  # [16]
    "found.edge_eq": 6,  # [13]
    "found.edge_in": 30,  # [61]
    "found.edge_out": 30,  # [61]
    "found.edge_pair_level_0": 4,  # [9]
    "found.edge_pair_level_1": 4,  # [9]
    "found.edge_pair_level_2": 4,  # [9]
    "found.edge_pair_level_3": 4,  # [8]
    "found.edge_pair_level_4": 3,  # [7]
    "found.edge_pair_level_5": 3,  # [7]
    "found.edge_pair_level_6": 3,  # [6]
    "found.edge_pair_level_7": 3,  # [6]
    "found.quiet_group": 192,  # [384]
    "found.ratio_pairs": 13,  # [26]
    "found.tie_window_order_differs": 3,  # [6]
    "found.tie_window_order_is_index_order": 33,  # [66]
    "found.uright_eq": 9,  # [18]
    "found.uright_in": 18,  # [36]
    "found.uright_out": 18,  # [36]
    "found.walked_stale": 5,  # [11]
    "left.accept_levels": 2097,  # [4195]
    "left.accept_ratio": 720,  # [1440]
    "left.all_taken": 210,  # [420]
    "left.bad": 12,  # [24]
    "left.exit_maxx": 4,  # [8]
    "left.exit_maxy": 4,  # [8]
    "left.exit_minx": 4,  # [8]
    "left.exit_miny": 4,  # [8]
    "left.far": 12,  # [24]
    "left.level_range": 36,  # [72]
    "left.no_keypoint": 220,  # [440]
    "left.not_in_view": 12265,  # [24531]
    "left.ratio": 80,  # [160]
    "left.th_high": 42,  # [84]
    "replay.double_assign": 6,  # [12]
    "replay.dry_left": 117,  # [234]
    "replay.dry_left_exactly_5": 29,  # [59]
    "replay.dry_right": 5,  # [11]
    "replay.dry_right_exactly_5": 5,  # [11]
    "replay.incall_free": 15,  # [30]
    "replay.list_short_left": 2157,  # [4315]
    "replay.list_short_right": 269,  # [539]
    "replay.own_partner": 6,  # [12]
    "replay.precall_free": 3,  # [6]
    "replay.taken_skip_in_assigning_group": 645,  # [1291]
    "right.accept_levels": 85,  # [171]
    "right.accept_ratio": 5,  # [10]
    "right.all_taken": 12,  # [25]
    "right.bad": 3,  # [6]
    "right.exit_maxx": 1,  # [2]
    "right.exit_maxy": 1,  # [2]
    "right.exit_minx": 1,  # [2]
    "right.exit_miny": 1,  # [2]
    "right.far": 3,  # [6]
    "right.level_r_m1": 6,  # [12]
    "right.level_range": 6,  # [12]
    "right.no_keypoint": 10,  # [20]
    "right.not_in_view": 4847,  # [9695]
    "right.ratio": 8,  # [17]
    "right.skipped": 10,  # [20]
    "right.th_high": 170,  # [340]
}

# Events that cannot happen, with the reason; asserted to be zero.
UNREACHABLE = {
    "left.level_r_m1": "mnTrackScaleLevelR belongs to the right window",
    "left.skipped": "only the right window can be skipped by the left one's `continue`",
}
