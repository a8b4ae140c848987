"""Deterministic synthetic stereo frames — there is no dataset on the box.

Image = value-noise octaves (cells 64/16/4 px, weights .5/.3/.2, seed s) + 48 rectangles and
24 discs of random intensity (seed s+1) + a zero-mean 3-px texture octave (weight .35, seed s+7;
lifts the level-0 FAST candidate count at th=20 into the 5k-20k band SURVEY §8d asks for) +
Gaussian noise sigma=2 (seed s+2), clipped to u8.
The right eye is the clean left scene shifted by `disparity` px with its own noise (seed s+3).
Frame k uses s = 42 + 4k.  Pure numpy, so CPU tests and the GPU bench see identical pixels.
"""
from __future__ import annotations

import numpy as np

__all__ = ["scene", "frame", "stereo_pair", "stereo_batch"]


def _value_noise(rng, h, w, cell):
    gh, gw = h // cell + 2, w // cell + 2
    grid = rng.random((gh, gw), dtype=np.float64)
    ys = np.arange(h, dtype=np.float64) / cell
    xs = np.arange(w, dtype=np.float64) / cell
    y0 = np.floor(ys).astype(np.int64)
    x0 = np.floor(xs).astype(np.int64)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    fy = fy * fy * (3 - 2 * fy)  # smoothstep
    fx = fx * fx * (3 - 2 * fx)
    g00 = grid[y0][:, x0]
    g01 = grid[y0][:, x0 + 1]
    g10 = grid[y0 + 1][:, x0]
    g11 = grid[y0 + 1][:, x0 + 1]
    top = g00 * (1 - fx) + g01 * fx
    bot = g10 * (1 - fx) + g11 * fx
    return top * (1 - fy) + bot * fy


def scene(h: int, w: int, seed: int, pad: int = 0) -> np.ndarray:
    """Clean float scene of size h x (w + pad) (pad gives room for the stereo shift)."""
    W = w + pad
    rng = np.random.default_rng(seed)
    img = np.zeros((h, W), dtype=np.float64)
    for cell, wt in ((64, 0.5), (16, 0.3), (4, 0.2)):
        img += wt * 255.0 * _value_noise(rng, h, W, cell)
    rng2 = np.random.default_rng(seed + 1)
    yy, xx = np.mgrid[0:h, 0:W]
    for _ in range(48):
        x0, y0 = rng2.integers(0, W), rng2.integers(0, h)
        rw, rh = rng2.integers(8, max(9, W // 6)), rng2.integers(8, max(9, h // 6))
        val = rng2.integers(0, 256)
        img[y0:y0 + rh, x0:x0 + rw] = 0.35 * img[y0:y0 + rh, x0:x0 + rw] + 0.65 * val
    for _ in range(24):
        cx, cy = rng2.integers(0, W), rng2.integers(0, h)
        r = rng2.integers(5, max(6, min(h, W) // 10))
        val = rng2.integers(0, 256)
        m = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        img[m] = 0.3 * img[m] + 0.7 * val
    rng3 = np.random.default_rng(seed + 7)
    img += 0.35 * 255.0 * (_value_noise(rng3, h, W, 3) - 0.5)
    return img


def _finish(img: np.ndarray, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    noisy = img + rng.normal(0.0, 2.0, size=img.shape)
    return np.clip(np.rint(noisy), 0, 255).astype(np.uint8)


def frame(h: int, w: int, k: int = 0) -> np.ndarray:
    """Mono frame k (h x w, uint8)."""
    s = 42 + 4 * k
    return _finish(scene(h, w, s), s + 2)


def stereo_pair(h: int, w: int, k: int = 0, disparity: int = 12):
    """(left, right) uint8 frames of pair k; right = left scene shifted by `disparity` px."""
    s = 42 + 4 * k
    sc = scene(h, w, s, pad=disparity)
    left = _finish(np.ascontiguousarray(sc[:, :w]), s + 2)
    right = _finish(np.ascontiguousarray(sc[:, disparity:disparity + w]), s + 3)
    return left, right


def stereo_batch(h: int, w: int, npairs: int, first: int = 0, disparity: int = 12) -> np.ndarray:
    """[2*npairs, h, w] uint8, images ordered L0, R0, L1, R1, ..."""
    out = np.empty((2 * npairs, h, w), dtype=np.uint8)
    for i in range(npairs):
        out[2 * i], out[2 * i + 1] = stereo_pair(h, w, first + i, disparity)
    return out


def map_points(xy_un, octave, desc, uright=None, n=2000, seed=0, nlevels=8, scale_factor=1.2):
    """Synthetic local-map points for ORBmatcher::SearchByProjection (a MAP_POINT_DTYPE array):
    projections near frame keypoints (several points per keypoint, so they compete), descriptors
    with 0..60 flipped bits (some unrelated), both RadiusByViewingCos branches, bad / not-in-view /
    observation-less / far points, and a few projections outside the image."""
    from . import MAP_POINT_DTYPE, MP_BAD, MP_HAS_OBS, MP_IN_VIEW
    rng = np.random.default_rng(seed)
    xy_un = np.asarray(xy_un, np.float32).reshape(-1, 2)
    octave = np.asarray(octave, np.int32)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    nk = len(octave)
    out = np.zeros(n, MAP_POINT_DTYPE)
    if nk == 0 or n == 0:
        return out
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    pool = rng.choice(nk, size=max(1, min(nk, n // 2)), replace=False)
    k = pool[rng.integers(0, len(pool), n)]
    lvl = np.clip(octave[k] + rng.choice([-1, 0, 0, 0, 1], n), 0, nlevels - 1)
    noise = rng.normal(0.0, 1.5, (n, 2)) * scale[octave[k]][:, None]
    p = xy_un[k] + noise
    outside = rng.random(n) < 0.03
    p[outside] = rng.uniform(-200, 1200, (int(outside.sum()), 2))
    out["proj_x"], out["proj_y"] = p[:, 0], p[:, 1]
    if uright is not None:
        ur = np.asarray(uright, np.float32)[k]
        out["proj_xr"] = np.where(ur > 0, ur + rng.normal(0, 2.0, n), p[:, 0] - 20)
    else:
        out["proj_xr"] = p[:, 0] - 20
    out["view_cos"] = rng.choice(np.array([0.9995, 0.999, 0.99, 0.95], np.float32), n)
    out["depth"] = rng.uniform(0.5, 80.0, n)
    out["level"] = lvl
    flags = np.where(rng.random(n) < 0.9, MP_IN_VIEW, 0) | np.where(rng.random(n) < 0.05, MP_BAD, 0) \
        | np.where(rng.random(n) < 0.9, MP_HAS_OBS, 0)
    out["flags"] = flags
    d = desc[k].copy()
    nflip = rng.choice([0, 2, 5, 10, 20, 35, 60], n)
    for i in range(n):
        if nflip[i]:
            b = np.unpackbits(d[i])
            b[rng.choice(256, nflip[i], replace=False)] ^= 1
            d[i] = np.packbits(b)
    unrelated = rng.random(n) < 0.05
    d[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), 32), dtype=np.uint8)
    out["desc"] = d
    return out


def map_points_stereo(xyL, octL, descL, xyR, octR, l2r, n=2000, seed=0, nlevels=8, scale_factor=1.2):
    """Map points for the two-camera SearchByProjection: the left-window fields as map_points(),
    plus a right-camera projection next to the stereo partner of the source keypoint (or a random
    right keypoint), its own level / viewing cosine, and mbTrackInViewR on ~80% of the points."""
    from . import MP_IN_VIEW, MP_IN_VIEW_R
    rng = np.random.default_rng(seed + 1000)
    out = map_points(xyL, octL, descL, None, n=n, seed=seed, nlevels=nlevels, scale_factor=scale_factor)
    xyR = np.asarray(xyR, np.float32).reshape(-1, 2)
    octR = np.asarray(octR, np.int32)
    if len(octR) == 0 or n == 0:
        return out
    l2r = np.asarray(l2r, np.int32)
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    # the source keypoint map_points drew from is the closest left keypoint to the projection
    src = np.argmin(((xyL[None, :, :] - np.stack([out["proj_x"], out["proj_y"]], 1)[:, None, :]) ** 2).sum(2), 1) \
        if len(xyL) <= 4096 else rng.integers(0, len(xyL), n)
    partner = l2r[src]
    kr = np.where(partner >= 0, partner, rng.integers(0, len(octR), n))
    noise = rng.normal(0.0, 1.5, (n, 2)) * scale[octR[kr]][:, None]
    out["proj_xr"] = xyR[kr, 0] + noise[:, 0]
    out["proj_yr"] = xyR[kr, 1] + noise[:, 1]
    out["level_r"] = np.clip(octR[kr] + rng.choice([-1, 0, 0, 0, 1], n), 0, nlevels - 1)
    out["level_r"][rng.random(n) < 0.03] = -1
    out["view_cos_r"] = rng.choice(np.array([0.9995, 0.999, 0.99, 0.95], np.float32), n)
    inr = rng.random(n) < 0.8
    out["flags"] = (out["flags"] & ~MP_IN_VIEW_R) | np.where(inr, MP_IN_VIEW_R, 0)
    # some points only in the right view
    only_r = rng.random(n) < 0.05
    out["flags"] = np.where(only_r, (out["flags"] & ~MP_IN_VIEW) | MP_IN_VIEW_R, out["flags"])
    return out


def stereo_partners(descL, descR, seed=0, frac=0.6):
    """Synthetic mvLeftToRightMatch / mvRightToLeftMatch: a consistent one-to-one pairing of a
    fraction of the left keypoints with right keypoints (mutual best Hamming where possible)."""
    rng = np.random.default_rng(seed)
    nl, nr = len(descL), len(descR)
    l2r = np.full(nl, -1, np.int32)
    r2l = np.full(nr, -1, np.int32)
    if nl == 0 or nr == 0:
        return l2r, r2l
    cand = rng.permutation(nl)[:int(frac * nl)]
    free = np.ones(nr, bool)
    for i in cand:
        j = int(rng.integers(0, nr))
        if free[j]:
            l2r[i], r2l[j] = j, i
            free[j] = False
    return l2r, r2l


def last_frame_points(xy_un, kps, desc, K, pose, uright=None, n=1000, seed=0, mbf=None, th=15.0,
                      bounds=(0.0, 640.0, 0.0, 480.0), pool=None, obs_fraction=0.7, nlevels=8, scale_factor=1.2):
    """Synthetic last-frame points for the motion-model SearchByProjection (a LAST_POINT_DTYPE
    array): the current keypoints (xy_un, kps: KEYPOINT_DTYPE, desc) unprojected at random depths
    through the inverse of pose = (Rcw 3x3, tcw 3) -- with uright and mbf the depth is
    mbf / (u - uright) where a stereo match exists -- with sub-radius position noise, a few flipped
    descriptor bits, the keypoint's octave +-1 and its angle plus a common offset and small noise.
    Several points aim at each of `pool` keypoints (default n // 2).  Mixed in by fixed fractions:
    invalid points (5%), points without observations (1 - obs_fraction), random angles (10%),
    points behind the camera (3%), projections outside the bounds (4%, every side), octaves outside
    [0, nlevels) (1%), non-finite positions (0.5%) and, with stereo, depths that disagree with
    mvuRight (5%)."""
    from . import LAST_POINT_DTYPE, LP_VALID, MP_HAS_OBS
    rng = np.random.default_rng(seed)
    xy_un = np.asarray(xy_un, np.float64).reshape(-1, 2)
    octave = np.asarray(kps["octave"], np.int64)
    kangle = np.asarray(kps["angle"], np.float64)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    nk = len(octave)
    out = np.zeros(n, LAST_POINT_DTYPE)
    if nk == 0 or n == 0:
        return out
    fx, fy, cx, cy = (float(v) for v in K)
    Rcw = np.asarray(pose[0], np.float64).reshape(3, 3)
    tcw = np.asarray(pose[1], np.float64).reshape(3)
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    npool = max(1, min(nk, n // 2 if pool is None else int(pool)))
    k = rng.choice(nk, size=npool, replace=False)[rng.integers(0, npool, n)]
    oct_l = np.clip(octave[k] + rng.choice([-1, 0, 0, 0, 1], n), 0, nlevels - 1)
    radius = th * scale[oct_l]
    uv = xy_un[k] + np.clip(rng.normal(0.0, 0.2, (n, 2)), -0.8, 0.8) * radius[:, None]
    z = rng.uniform(1.0, 20.0, n)
    if uright is not None and mbf is not None:
        disp = xy_un[k, 0] - np.asarray(uright, np.float64)[k]
        has = (np.asarray(uright, np.float64)[k] > 0) & (disp > 0.1)
        z = np.where(has, mbf / np.where(has, disp, 1.0), z)
        wrong = has & (rng.random(n) < 0.05)  # a disparity off by four radii
        z = np.where(wrong, mbf / (np.where(has, disp, 1.0) + 4.0 * radius), z)
    behind = rng.random(n) < 0.03
    z = np.where(behind, -z, z)
    outside = np.flatnonzero(rng.random(n) < 0.04)
    far = rng.uniform(50.0, 300.0, len(outside))
    for j, (i, d) in enumerate(zip(outside, far)):  # every side in turn
        side = j % 4
        if side == 0:
            uv[i, 0] = bounds[0] - d
        elif side == 1:
            uv[i, 0] = bounds[1] + d
        elif side == 2:
            uv[i, 1] = bounds[2] - d
        else:
            uv[i, 1] = bounds[3] + d
    pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    pw = (pc - tcw) @ Rcw  # Rcw^T (pc - tcw)
    pw[rng.random(n) < 0.005] = np.nan
    out["pos"] = pw.astype(np.float32)
    oct_l = np.where(rng.random(n) < 0.01, rng.choice([-1, nlevels], n), oct_l)
    out["octave"] = oct_l
    ang = np.mod(kangle[k] + 20.0 + rng.normal(0.0, 3.0, n), 360.0)
    ang = np.where(rng.random(n) < 0.10, rng.uniform(0.0, 360.0, n), ang)
    out["angle"] = ang.astype(np.float32)
    out["flags"] = np.where(rng.random(n) < 0.95, LP_VALID, 0) | np.where(rng.random(n) < obs_fraction, MP_HAS_OBS, 0)
    d = desc[k].copy()
    nflip = rng.choice([0, 2, 5, 10, 20, 35], n)
    for i in range(n):
        if nflip[i]:
            b = np.unpackbits(d[i])
            b[rng.choice(256, nflip[i], replace=False)] ^= 1
            d[i] = np.packbits(b)
    out["desc"] = d
    return out


def reloc_points(xy_un, kps, desc, K, pose, n=1000, seed=0, th=10.0, bounds=(0.0, 640.0, 0.0, 480.0), pool=None,
                 nlevels=8, scale_factor=1.2, invalid=0.05, outside=0.04, too_near=0.03, too_far=0.03,
                 not_finite=0.01, level_offsets=(-1, 0, 0, 0, 1), over_top=0.02, wild_angles=0.02,
                 flips=(0, 2, 5, 10, 20, 35, 50, 80, 120)):
    """Synthetic keyframe points for the relocalisation SearchByProjection (a RELOC_POINT_DTYPE
    array): the frame's keypoints (xy_un, kps: KEYPOINT_DTYPE, desc) unprojected at random depths
    through the inverse of pose = (Rcw 3x3, tcw 3), with sub-radius position noise, `flips` flipped
    descriptor bits and the keypoint's angle plus a common offset and small noise.  The level
    MapPoint::PredictScale gives is steered through max_distance: the distance to the camera centre
    is max_distance / scale_factor ** (level - 0.5), level = the keypoint's octave plus one of
    `level_offsets` (a ratio in (1 / 1.2, 1] for level 0), and for a share `over_top` the ratio lies
    above the last step, where the level is clamped; min_distance = max_distance / scale_factor **
    (nlevels - 1).  Several points aim at each of `pool` keypoints (default n // 2).  Mixed in by the
    given shares: invalid points, projections outside the bounds (every side in turn), points nearer
    than 0.8 min_distance, farther than 1.2 max_distance, not finite (position, a position that
    overflows the distance, an infinite max_distance, in turn), and angles moved by +-720 degrees
    (`wild_angles`; 10% of the angles are random)."""
    from . import RELOC_POINT_DTYPE, RP_VALID
    rng = np.random.default_rng(seed)
    xy_un = np.asarray(xy_un, np.float64).reshape(-1, 2)
    octave = np.asarray(kps["octave"], np.int64)
    kangle = np.asarray(kps["angle"], np.float64)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    nk = len(octave)
    out = np.zeros(n, RELOC_POINT_DTYPE)
    if nk == 0 or n == 0:
        return out
    fx, fy, cx, cy = (float(v) for v in K)
    Rcw = np.asarray(pose[0], np.float64).reshape(3, 3)
    tcw = np.asarray(pose[1], np.float64).reshape(3)
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    npool = max(1, min(nk, n // 2 if pool is None else int(pool)))
    k = rng.choice(nk, size=npool, replace=False)[rng.integers(0, npool, n)]
    level = np.clip(octave[k] + rng.choice(list(level_offsets), n), 0, nlevels - 1)
    radius = th * scale[level]
    uv = xy_un[k] + np.clip(rng.normal(0.0, 0.2, (n, 2)), -0.8, 0.8) * radius[:, None]
    z = rng.uniform(1.0, 20.0, n)
    side = np.flatnonzero(rng.random(n) < outside)
    far = rng.uniform(50.0, 300.0, len(side))
    for j, (i, d) in enumerate(zip(side, far)):  # every side in turn
        if j % 4 == 0:
            uv[i, 0] = bounds[0] - d
        elif j % 4 == 1:
            uv[i, 0] = bounds[1] + d
        elif j % 4 == 2:
            uv[i, 1] = bounds[2] - d
        else:
            uv[i, 1] = bounds[3] + d
    pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    pw = (pc - tcw) @ Rcw  # Rcw^T (pc - tcw)
    dist = np.linalg.norm(pc, axis=1)  # |X - Ow|
    ratio = np.where(level == 0, rng.uniform(0.86, 0.99, n), scale_factor ** (level - 0.5))
    ratio = np.where(rng.random(n) < over_top, scale_factor ** (nlevels - 1) * 1.1, ratio)
    maxd = dist * ratio
    mind = maxd / scale_factor ** (nlevels - 1)
    near = rng.random(n) < too_near
    mind = np.where(near, dist * 1.3, mind)
    maxd = np.where(rng.random(n) < too_far, dist / 1.3, maxd)
    bad = np.flatnonzero(rng.random(n) < not_finite)
    for j, i in enumerate(bad):  # every kind in turn
        if j % 3 == 0:
            pw[i, j % 2] = np.nan
        elif j % 3 == 1:
            pw[i] = pw[i] / np.linalg.norm(pw[i]) * 1e30
            maxd[i], mind[i] = np.inf, 0.0
        else:
            maxd[i] = np.inf
    out["pos"] = pw.astype(np.float32)
    out["min_distance"] = mind.astype(np.float32)
    out["max_distance"] = maxd.astype(np.float32)
    ang = np.mod(kangle[k] + 20.0 + rng.normal(0.0, 3.0, n), 360.0)
    ang = np.where(rng.random(n) < 0.10, rng.uniform(0.0, 360.0, n), ang)
    ang = ang + np.where(rng.random(n) < wild_angles, rng.choice([-720.0, 720.0], n), 0.0)
    out["angle"] = ang.astype(np.float32)
    out["flags"] = np.where(rng.random(n) < 1.0 - invalid, RP_VALID, 0)
    d = desc[k].copy()
    nflip = rng.choice(list(flips), n)
    for i in range(n):
        if nflip[i]:
            b = np.unpackbits(d[i])
            b[rng.choice(256, nflip[i], replace=False)] ^= 1
            d[i] = np.packbits(b)
    out["desc"] = d
    return out


def fuse_points(xy_un, kps, desc, K, pose, uright=None, bf=None, n=1000, seed=0, th=3.0,
                bounds=(0.0, 640.0, 0.0, 480.0), pool=None, nlevels=8, scale_factor=1.2, z_range=(1.0, 20.0),
                invalid=0.04, behind=0.03, outside=0.04, too_near=0.03, too_far=0.03, bad_normal=0.04, empty=0.04,
                not_finite=0.01, chi=0.10, level_offsets=(0, 0, 0, 0, 1, 1, -1, 2), over_top=0.02,
                flips=(0, 2, 5, 10, 20, 35, 45, 60, 80, 120)):
    """Synthetic map points for ORBmatcher::Fuse (a FUSE_POINT_DTYPE array): the frame's keypoints
    (xy_un, kps: KEYPOINT_DTYPE, desc) back-projected through the inverse of pose = (Rcw 3x3, tcw 3)
    at a depth from `z_range` -- with uright and bf the depth bf / (x - uright) where the keypoint
    has a right coordinate, so that the stereo reprojection error follows the image offset -- with
    sub-radius position noise and `flips` flipped descriptor bits.  The normal is the viewing
    direction turned by up to 55 degrees.  The predicted level is steered through max_distance as
    in reloc_points: level = the keypoint's octave plus one of `level_offsets` (Fuse keeps octaves
    level - 1 and level, so offsets 0 and 1 reach the keypoint and -1 and 2 have it filtered).
    Several points aim at each of `pool` keypoints (default n // 2).  Mixed in by the given shares,
    one kind of miss each: invalid points, points behind the camera, projections outside the
    bounds (every side in turn), points nearer than 0.8 min_distance, farther than 1.2
    max_distance, normals turned 70 to 180 degrees away, points aimed at a place of the image with
    no keypoint within the radius (`empty`), not-finite values (a NaN coordinate, a position that
    overflows the distance, an infinite max_distance, in turn) and, for `chi`, a clean descriptor
    2.1 to 2.9 sigma of the keypoint's octave to the side: beyond the stereo chi-square limit, and
    on either side of the monocular one."""
    from . import FP_VALID, FUSE_POINT_DTYPE
    rng = np.random.default_rng(seed)
    xy_un = np.asarray(xy_un, np.float64).reshape(-1, 2)
    octave = np.asarray(kps["octave"], np.int64)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    nk = len(octave)
    out = np.zeros(n, FUSE_POINT_DTYPE)
    if nk == 0 or n == 0:
        return out
    fx, fy, cx, cy = (float(v) for v in K)
    Rcw = np.asarray(pose[0], np.float64).reshape(3, 3)
    tcw = np.asarray(pose[1], np.float64).reshape(3)
    scale = scale_factor ** np.arange(nlevels, dtype=np.float64)
    npool = max(1, min(nk, n // 2 if pool is None else int(pool)))
    k = rng.choice(nk, size=npool, replace=False)[rng.integers(0, npool, n)]
    level = np.clip(octave[k] + rng.choice(list(level_offsets), n), 0, nlevels - 1)
    nflip = rng.choice(list(flips), n)
    radius = th * scale[level]
    uv = xy_un[k] + np.clip(rng.normal(0.0, 0.2, (n, 2)), -0.8, 0.8) * radius[:, None]
    # the chi-square share: the keypoint's own level, a clean descriptor, an offset along x alone
    gate = np.flatnonzero(rng.random(n) < chi)
    level[gate] = octave[k[gate]]
    nflip[gate] = rng.choice([0, 2, 5], len(gate))
    uv[gate] = xy_un[k[gate]]
    uv[gate, 0] += rng.choice([-1.0, 1.0], len(gate)) * rng.uniform(2.1, 2.9, len(gate)) * scale[octave[k[gate]]]
    # the empty share: a low level, and a place whose nearest keypoint is more than two radii away
    for i in np.flatnonzero(rng.random(n) < empty):
        level[i] = rng.integers(0, 2)
        for _ in range(200):
            c = np.array([rng.uniform(bounds[0] + 20, bounds[1] - 20), rng.uniform(bounds[2] + 20, bounds[3] - 20)])
            if np.abs(xy_un - c).max(1).min() > 2.0 * th * scale[level[i]]:
                uv[i] = c
                break
    z = rng.uniform(z_range[0], z_range[1], n)
    if uright is not None and bf is not None:
        ur = np.asarray(uright, np.float64)[k]
        disp = xy_un[k, 0] - ur
        has = (ur >= 0) & (disp > 0.1)
        z = np.where(has, bf / np.where(has, disp, 1.0), z)
    z = np.where(rng.random(n) < behind, -z, z)
    side = np.flatnonzero(rng.random(n) < outside)
    far = rng.uniform(50.0, 300.0, len(side))
    for j, (i, d) in enumerate(zip(side, far)):  # every side in turn
        if j % 4 == 0:
            uv[i, 0] = bounds[0] - d
        elif j % 4 == 1:
            uv[i, 0] = bounds[1] + d
        elif j % 4 == 2:
            uv[i, 1] = bounds[2] - d
        else:
            uv[i, 1] = bounds[3] + d
    pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    pw = (pc - tcw) @ Rcw  # Rcw^T (pc - tcw)
    dist = np.linalg.norm(pc, axis=1)  # |X - Ow|
    ratio = np.where(level == 0, rng.uniform(0.86, 0.99, n), scale_factor ** (level - 0.5))
    ratio = np.where(rng.random(n) < over_top, scale_factor ** (nlevels - 1) * 1.1, ratio)
    maxd = dist * ratio
    mind = maxd / scale_factor ** (nlevels - 1)
    mind = np.where(rng.random(n) < too_near, dist * 1.3, mind)
    maxd = np.where(rng.random(n) < too_far, dist / 1.3, maxd)
    # the normal: the viewing direction PO / |PO| (in world axes) turned about a random axis across it
    view = (pc / dist[:, None]) @ Rcw
    across = np.cross(view, rng.normal(0.0, 1.0, (n, 3)))
    across /= np.linalg.norm(across, axis=1)[:, None]
    turn = np.radians(np.where(rng.random(n) < bad_normal, rng.uniform(70.0, 180.0, n), rng.uniform(0.0, 55.0, n)))
    normal = view * np.cos(turn)[:, None] + across * np.sin(turn)[:, None]
    for j, i in enumerate(np.flatnonzero(rng.random(n) < not_finite)):  # every kind in turn
        if j % 3 == 0:
            pw[i, j % 2] = np.nan
        elif j % 3 == 1:
            pw[i] = pw[i] / np.linalg.norm(pw[i]) * 1e30
            maxd[i], mind[i] = np.inf, 0.0
        else:
            maxd[i] = np.inf
    out["pos"] = pw.astype(np.float32)
    out["normal"] = normal.astype(np.float32)
    out["min_distance"] = mind.astype(np.float32)
    out["max_distance"] = maxd.astype(np.float32)
    out["flags"] = np.where(rng.random(n) < 1.0 - invalid, FP_VALID, 0)
    d = desc[k].copy()
    for i in range(n):
        if nflip[i]:
            b = np.unpackbits(d[i])
            b[rng.choice(256, nflip[i], replace=False)] ^= 1
            d[i] = np.packbits(b)
    out["desc"] = d
    return out


def sim3_pose(sim3):
    """The RELOC_POSE_DTYPE record the Sim3 searches take for Scw = (scale, rotation 3x3, translation 3):
    Rcw = Scw.rotationMatrix(), tcw = Scw.translation() / Scw.scale(), Ow = Tcw.inverse().translation()
    (ORBmatcher.cc:437-438), and (Rcw, tcw) in double for the generators."""
    from . import RELOC_POSE_DTYPE
    s, R, t = sim3
    R = np.asarray(R, np.float64).reshape(3, 3)
    tcw = np.asarray(t, np.float64).reshape(3) / float(s)
    p = np.zeros((), RELOC_POSE_DTYPE)
    p["Rcw"], p["tcw"], p["Ow"] = R.reshape(9), tcw, -R.T @ tcw
    return p, (R, tcw)


def sim3_points(xy_un, kps, desc, K, sim3, n=1000, seed=0, th=8.0, bounds=(0.0, 640.0, 0.0, 480.0), pool=None,
                contested=0.25, contested_pool=24, contested_flips=(0, 2, 5, 10, 20, 35), **shares):
    """Synthetic map points for the Sim3 SearchByProjection overloads (a FUSE_POINT_DTYPE array): the
    frame's keypoints back-projected through the inverse of the pose sim3_pose derives from Scw =
    (scale, rotation, translation), as fuse_points does (whose shares of each rejection -- invalid,
    behind, outside, too_near, too_far, bad_normal, empty, not_finite, level_offsets, over_top, flips,
    z_range -- pass through `shares`; there is no chi-square share).  A share `contested` of the points
    has none of those misses and aims at `contested_pool` keypoints only, at the keypoint's own level or
    the one above, so that several points in a row want one keypoint, the later ones fall to their next
    best and, with a wide window and limit, past the few candidates a kernel keeps.  The two kinds are
    interleaved at random, so chains of contested points run through the whole list."""
    rng = np.random.default_rng(seed + 7919)
    _, pose = sim3_pose(sim3)
    nc = int(round(n * contested))
    common = dict(th=th, bounds=bounds, chi=0.0)
    a = fuse_points(xy_un, kps, desc, K, pose, n=n - nc, seed=seed, pool=pool, **common, **shares)
    clean = dict(invalid=0.0, behind=0.0, outside=0.0, too_near=0.0, too_far=0.0, bad_normal=0.0, empty=0.0,
                 not_finite=0.0, over_top=0.0, level_offsets=(0, 0, 1), flips=contested_flips)
    if "z_range" in shares:
        clean["z_range"] = shares["z_range"]
    b = fuse_points(xy_un, kps, desc, K, pose, n=nc, seed=seed + 1, pool=contested_pool, **common, **clean)
    out = np.concatenate([a, b])
    return out[rng.permutation(len(out))]
