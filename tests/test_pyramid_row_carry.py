"""The resize loops that carry a shared source row through consecutive output rows (orb_pyramid.hip
br_tile and k_pyr_tail, orb_kernels.h resize_run), the resize tables the host writes in their final
form, and the blur that skips strips outside the plane: every pyramid level and every blurred level
of a 4-image batch, bit-exact against the oracle, read back with orbgpu_get_pyramid_level.

Sizes: 176x144; 257x97 (a third tile column with 1 valid column, a fourth tile row with 1 valid
row); 300x200.  Scale factors: 1.2 (the carry hits in most rows), 1.5 (hits and misses alternate),
1.9 (mostly misses), 2.0 (the exact-2x area path, no carry).  Each case runs once with
k_blur_resize for every level (ORBGPU_NO_TAIL) and once with k_pyr_tail forced on
(ORBGPU_TAIL_MIN=0), so both copies of the carried loop run.

Levels: 3 where the planner accepts 3 -- a level needs one 35-px FAST cell, i.e. 67 px both ways
(orb_geometry.h cell_grid) -- else as many as it accepts; LEVELS states the count per case and the
test checks that the library refuses one more, so no case shrinks silently.  The cases left with one
level (257x97 above scale 1.2) still run the blur of a plane that ends 1 px into a tile column and
a tile row."""
import ctypes as C

import numpy as np
import pytest

from orbslam3lib_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(176, 144), (257, 97), (300, 200)]
SCALES = [1.2, 1.5, 1.9, 2.0]
NIMG = 4
# levels of at least 67 x 67 among the first three (level l = round(size / scale^l))
LEVELS = {
    (176, 144, 1.2): 3, (176, 144, 1.5): 2, (176, 144, 1.9): 2, (176, 144, 2.0): 2,
    (257, 97, 1.2): 3, (257, 97, 1.5): 1, (257, 97, 1.9): 1, (257, 97, 2.0): 1,
    (300, 200, 1.2): 3, (300, 200, 1.5): 3, (300, 200, 1.9): 2, (300, 200, 2.0): 2,
}
_refs = {}


def _images(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    imgs = [synth.frame(h, w, k) for k in range(NIMG - 1)]
    imgs.append(rng.integers(0, 256, (h, w), dtype=np.uint8))  # every rounding case of the fixed point
    return np.stack(imgs)


def _reference(oracle, w, h, sf):
    """[image][level] -> (level, blurred level), computed once per (size, scale)."""
    key = (w, h, sf)
    if key not in _refs:
        L = LEVELS[key]
        out = []
        for img in _images(w, h):
            pyr = oracle.pyramid(img, sf, L)
            out.append([(lv, oracle.blur(lv)) for lv in pyr])
        _refs[key] = out
    return _refs[key]


def _level(og, be, image, level, blurred):
    w, h = C.c_int(0), C.c_int(0)
    og._check(og._lib.orbgpu_get_pyramid_level(be.ctx.handle, image, level, int(blurred), None, 0,
                                               C.byref(w), C.byref(h)))
    out = np.zeros((h.value, w.value), np.uint8)
    og._check(og._lib.orbgpu_get_pyramid_level(be.ctx.handle, image, level, int(blurred), og._p(out),
                                               w.value, None, None))
    return out


@pytest.mark.parametrize("tail", [False, True], ids=["per_level", "tail"])
@pytest.mark.parametrize("sf", SCALES)
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_pyramid_and_blur_bit_exact(oracle, monkeypatch, size, sf, tail):
    import orbslam3lib_amd as og
    w, h = size
    L = LEVELS[(w, h, sf)]
    monkeypatch.setenv("ORBGPU_DIAGNOSTICS", "1")
    monkeypatch.setenv("ORBGPU_TAIL_MIN" if tail else "ORBGPU_NO_TAIL", "0" if tail else "1")
    if L < 3:
        with pytest.raises(og.OrbGpuError):
            og.BatchExtractor(300, sf, L + 1, 20, 7, width=w, height=h, max_images=NIMG)
    ref = _reference(oracle, w, h, sf)
    be = og.BatchExtractor(300, sf, L, 20, 7, width=w, height=h, max_images=NIMG)
    try:
        be.upload(_images(w, h))
        be.run()
        be.synchronize()
        for i in range(NIMG):
            for l in range(L):
                np.testing.assert_array_equal(_level(og, be, i, l, False), ref[i][l][0],
                                              err_msg="img %d level %d" % (i, l))
                np.testing.assert_array_equal(_level(og, be, i, l, True), ref[i][l][1],
                                              err_msg="img %d blur level %d" % (i, l))
    finally:
        be.close()
