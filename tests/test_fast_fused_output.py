"""k_fast_cells with one wave per cell writes a cell's keys in its nonmax pass (orb_fast_cell.h,
fast_cell_detect: the running kept count is the write position, no verdict bit, no second loop).

Batches of 6 images (more than kFastMergeMaxImages = 4, so the small-list kernels of the batch
shape run), 3 levels, bit-exact against the oracle: the level keypoints and descriptors against
extract_levels, the keys that entered DistributeOctTree against level_candidates.  Two sizes:
* 160 x 128: every level's cells take the 64-byte tile (two waves per cell: the three loops);
* 176 x 144: level 0 (cells 36 x 38) takes the 48-byte tile, level 2 (45 x 68) the 80-byte one,
  both one wave per cell: the fused loop.  test_one_wave_tiles_ran pins that.

Cases: cells that keep more than 64 corners (several batches of the loop, a running offset);
cells that keep nothing at iniThFAST 20 and something at minThFAST 7 (the rerun after a pass
that wrote nothing); all-flat frames after a dense batch on the same context (counts 0 whatever
the key buffer held); a cell that keeps exactly 64 of exactly 64 and of exactly 128 corners.
What each frame is built to contain is checked on the CPU with the oracle before the GPU runs."""
import functools

import numpy as np
import pytest

from orbslam3lib_amd import synth

pytestmark = pytest.mark.gpu

NIMG, LEVELS, NFEAT, INI, MIN = 6, 3, 4000, 20, 7
SHAPES = [(160, 128), (176, 144)]
MIN_BORDER = 16  # EDGE_THRESHOLD - 3


def _cell_grid(w, h):
    """nCols, nRows, wCell, hCell of a level (ORBextractor_old.cc:790-800)."""
    W, H = w - 2 * MIN_BORDER, h - 2 * MIN_BORDER
    nc, nr = W // 35, H // 35
    return nc, nr, -(-W // nc), -(-H // nr)


def _kept_per_cell(oracle, lvl, ini=INI, mn=MIN):
    """Kept keys per cell of one level image: the detection areas of the cells tile the level."""
    nc, nr, wc, hc = _cell_grid(lvl.shape[1], lvl.shape[0])
    k = oracle.level_candidates(lvl, ini, mn)
    cnt = np.zeros((nr, nc), np.int64)
    np.add.at(cnt, (np.minimum((k["y"].astype(int) - 3) // hc, nr - 1),
                    np.minimum((k["x"].astype(int) - 3) // wc, nc - 1)), 1)
    return cnt


def _corners_in_cell00(oracle, img, th):
    """FAST corners at th (before nonmax) in cell (0, 0)'s detection area of level 0: cornerScore
    of a corner at th is >= th, of any other pixel th - 1."""
    _, _, wc, hc = _cell_grid(img.shape[1], img.shape[0])
    return sum(oracle.corner_score(img, x, y, th) >= th
               for y in range(MIN_BORDER + 3, MIN_BORDER + 3 + hc)
               for x in range(MIN_BORDER + 3, MIN_BORDER + 3 + wc))


@functools.lru_cache(maxsize=None)
def _dense(w, h):
    """Three synth frames and three frames of 2-px value noise."""
    rng = np.random.default_rng(5)
    tex = [np.clip(np.rint(255 * synth._value_noise(rng, h, w, 2)), 0, 255).astype(np.uint8) for _ in range(3)]
    return np.stack([synth.frame(h, w, k) for k in range(3)] + tex)


def _checker(w, h, k):
    """Flat 100 but for one 11 x 11 checker patch of 5-px squares 12 above it."""
    img = np.full((h, w), 100, np.uint8)
    x0, y0 = 33 + 3 * k, 31 + 2 * k
    for j in range(11):
        for i in range(11):
            if (i + j) % 2 == 0:
                img[y0 + 5 * j:y0 + 5 * j + 5, x0 + 5 * i:x0 + 5 * i + 5] = 112
    return img


def _dots(w, h, pairs):
    """An 8 x 8 grid of single bright pixels, 4 px apart, inside cell (0, 0)'s detection area of
    level 0: each is one corner and is kept.  pairs: a dimmer pixel beside each, a second corner
    that the nonmax drops (128 corners, 64 kept).  One more dot in each other quadrant keeps
    DistributeOctTree dividing (a lone child ends it: :687), so the 64 keys reach the output."""
    img = np.full((h, w), 100, np.uint8)
    img[30, w - 30] = img[h - 30, 30] = img[h - 30, w - 30] = 200
    for j in range(8):
        for i in range(8):
            img[21 + 4 * j, 21 + 4 * i] = 200
            if pairs:
                img[21 + 4 * j, 22 + 4 * i] = 170
    return img


_contexts = {}


def _context(w, h):
    import orbslam3lib_amd as og
    if (w, h) not in _contexts:
        _contexts[(w, h)] = og.BatchExtractor(NFEAT, 1.2, LEVELS, INI, MIN, width=w, height=h, max_images=NIMG)
    return _contexts[(w, h)]


def _level_keypoints(be, image, cap=16384):
    import orbslam3lib_amd as og
    kps = np.zeros(cap, og.KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    cnt = np.zeros(LEVELS, np.int32)
    og._check(og._lib.orbgpu_get_level_keypoints(be.ctx.handle, image, og._p(kps), og._p(desc), cap, og._p(cnt)))
    off = np.concatenate([[0], np.cumsum(cnt)])
    return [(kps[off[l]:off[l + 1]], desc[off[l]:off[l + 1]]) for l in range(LEVELS)]


_refs = {}


def _reference(oracle, key, img):
    """(extract_levels, candidates over the levels) of one frame, computed once."""
    if key not in _refs:
        pyr = oracle.pyramid(img, 1.2, LEVELS)
        ncand = sum(len(oracle.level_candidates(lvl, INI, MIN)) for lvl in pyr)
        _refs[key] = (oracle.extract_levels(img, nfeatures=NFEAT, nlevels=LEVELS, ini_th=INI, min_th=MIN), ncand)
    return _refs[key]


def _run_and_compare(oracle, name, imgs):
    h, w = imgs.shape[1:]
    be = _context(w, h)
    be.upload(imgs)
    be.run()
    be.synchronize()
    cand = be.candidate_counts()
    n, _ = be.counts()
    for i in range(len(imgs)):
        ref, ncand = _reference(oracle, (name, w, h, i), imgs[i])
        assert cand[i] == ncand, (name, i)
        got = _level_keypoints(be, i)
        for l in range(LEVELS):
            (gk, gd), (rk, rd) = got[l], ref[l]
            assert len(gk) == len(rk), (name, i, l)
            for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
                np.testing.assert_array_equal(gk[f], rk[f], err_msg="%s image %d level %d %s" % (name, i, l, f))
            np.testing.assert_array_equal(gd, rd.reshape(-1, 32), err_msg="%s image %d level %d desc" % (name, i, l))
        assert n[i] == sum(len(r[0]) for r in ref)
    return cand, n


@pytest.mark.parametrize("w,h", SHAPES)
def test_dense_corners(oracle, w, h):
    imgs = _dense(w, h)
    for img in imgs:  # every frame has level-0 cells that keep more than one batch of 64
        assert _kept_per_cell(oracle, img).max() > 64
    _run_and_compare(oracle, "dense", imgs)


@pytest.mark.parametrize("w,h", SHAPES)
def test_two_step_cell(oracle, w, h):
    imgs = np.stack([_checker(w, h, k) for k in range(NIMG)])
    for img in imgs:  # level 0: nothing at iniThFAST alone, cells with keys once minThFAST follows
        assert _kept_per_cell(oracle, img, INI, 255).sum() == 0
        assert (_kept_per_cell(oracle, img, INI, MIN) > 0).sum() >= 2
    cand, _ = _run_and_compare(oracle, "checker", imgs)
    assert (cand > 0).all()


@pytest.mark.parametrize("w,h", SHAPES)
def test_empty_cells_after_dense(oracle, w, h):
    _run_and_compare(oracle, "dense", _dense(w, h))  # leaves keys in every cell's slots
    flat = np.stack([np.full((h, w), 60 + 30 * k, np.uint8) for k in range(NIMG)])
    cand, n = _run_and_compare(oracle, "flat", flat)
    assert not cand.any() and not n.any()


@pytest.mark.parametrize("w,h", SHAPES)
def test_exactly_64(oracle, w, h):
    imgs = np.stack([_dots(w, h, pairs=bool(k & 1)) for k in range(NIMG)])
    for k in (0, 1):
        assert _kept_per_cell(oracle, imgs[k])[0, 0] == 64
        assert _corners_in_cell00(oracle, imgs[k], INI) == (128 if k else 64)
    _run_and_compare(oracle, "dots", imgs)


def test_one_wave_tiles_ran():
    """176 x 144, 3 levels: the 48-byte and the 80-byte tile (one wave per cell) both have cells
    in a 6-image batch; 160 x 128 runs the 64-byte tile only."""
    for (w, h), want in (((176, 144), (True, True, True)), ((160, 128), (False, True, False))):
        be = _context(w, h)
        be.set_profiling(True)
        be.reset_stage_times()
        be.upload(_dense(w, h))
        be.run()
        be.synchronize()
        st = be.stage_times()
        be.set_profiling(False)
        ran = tuple(st[s][1] > 0 for s in ("k_fast_cells<48>", "k_fast_cells<64>", "k_fast_cells<80>"))
        assert ran == want, ((w, h), st)
