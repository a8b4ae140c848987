"""GPU: k_octree with the direct phase 1 (orb_octree.h: the phase-1 node list built straight from
the count pyramid) against the reference-made fixtures tests/golden/ref_*.npz, in both launch
shapes, and against the round-by-round phase 1 (ORBGPU_OCT_ROUNDS=1) on the same images.

A 2-image context takes the 512-thread launch for every level; a batch of 40 images (at least
kOctSmallMinImages) takes the 256-thread one.  Every comparison is exact.  The round counters that
show the switch is alive are checked on the CPU (tests/test_octree_direct.py)."""
import numpy as np
import pytest

from tests import ref_cases as RC

pytestmark = pytest.mark.gpu

# the two mixed groups of tests/ref_cases.py: one parameter set per frame shape
SMALL = [c for c in RC.CASES if (c.h, c.w, c.nfeatures, c.ini_th) == (120, 160, 300, 20)]
MID = [c for c in RC.CASES if (c.h, c.w, c.nfeatures) == (240, 320, 1000)]


@pytest.fixture(scope="module")
def loaded():
    return {c.name: RC.load(RC.fixture_path(c)) for c in SMALL + MID}


def test_case_groups():
    assert len(SMALL) == 5 and len(MID) == 4


@pytest.mark.parametrize("name", [c.name for c in SMALL + MID])
def test_extractor_equals_fixture(loaded, name):
    import orbslam3lib_amd as og
    c, img, z = loaded[name]
    ex = og.ORBextractor(c.nfeatures, c.scale_factor, c.nlevels, c.ini_th, c.min_th, max_width=c.w, max_height=c.h,
                         max_images=2)
    k, d, mono = ex(img, None, c.lap)
    assert mono == z["mono"], name
    RC.same_kps(k, z["kps"], name)
    np.testing.assert_array_equal(d, z["desc"], err_msg=name)
    if c.levels:
        for level, ((gk, _), wk) in enumerate(zip(ex.level_keypoints(0), RC.split_levels(z))):
            RC.same_kps(gk, wk, "%s level %d" % (name, level))


def _batch(og, cases, loaded, reps):
    c = cases[0]
    order = [cases[i % len(cases)] for i in range(reps)]
    imgs = np.stack([loaded[k.name][1] for k in order])
    laps = np.array([k.lap for k in order], np.int32)
    be = og.BatchExtractor(c.nfeatures, c.scale_factor, c.nlevels, c.ini_th, c.min_th, width=c.w, height=c.h,
                           max_images=reps)
    be.upload(imgs)
    return be, order, laps


def test_mixed_batch_of_40_equals_fixtures(loaded):
    import orbslam3lib_amd as og
    be, order, laps = _batch(og, MID, loaded, 40)
    be.run(laps)
    be.synchronize()
    for i, c in enumerate(order):
        z = loaded[c.name][2]
        k, d, mono = be.result(i)
        assert mono == z["mono"], (i, c.name)
        RC.same_kps(k, z["kps"], "%s (image %d)" % (c.name, i))
        np.testing.assert_array_equal(d, z["desc"], err_msg="%s (image %d)" % (c.name, i))
    be.close()


def test_direct_equals_rounds_knob(loaded, monkeypatch):
    """One 320x240 batch on a context with the direct phase 1 and on one created with
    ORBGPU_OCT_ROUNDS=1, each run twice: counts, keypoints and descriptors are identical."""
    import orbslam3lib_amd as og
    runs = {}
    for rounds in (False, True):
        if rounds:
            monkeypatch.setenv("ORBGPU_DIAGNOSTICS", "1")
            monkeypatch.setenv("ORBGPU_OCT_ROUNDS", "1")
            assert og.diagnostic_knobs().get("ORBGPU_OCT_ROUNDS") == "1"
        else:
            assert "ORBGPU_OCT_ROUNDS" not in og.diagnostic_knobs()
        be, order, laps = _batch(og, MID, loaded, 8)
        for rep in range(2):
            be.run(laps)
            be.synchronize()
            runs[rounds, rep] = [be.result(i) for i in range(len(order))]
        be.close()
    base = runs[False, 0]
    assert sum(len(k) for k, _, _ in base) > 2000
    for key, got in runs.items():
        for i, ((k, d, m), (bk, bd, bm)) in enumerate(zip(got, base)):
            assert m == bm and len(k) == len(bk), (key, i)
            RC.same_kps(k, bk, "%r image %d" % (key, i))
            np.testing.assert_array_equal(d, bd, err_msg="%r image %d" % (key, i))
