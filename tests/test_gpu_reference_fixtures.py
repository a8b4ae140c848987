"""GPU parity against fixtures the oracle did not write: tests/golden/ref_*.npz hold the output of
the reference's own ORBextractor_old.cc (oracle/ref/README.md).  These tests read the fixtures
and regenerate their images; they call neither the oracle nor the reference.

Every fixture through ORBextractor.__call__ (mono index, keypoints, descriptors, and the
per-level keypoints where recorded), then the same cases through BatchExtractor, one mixed batch
per frame shape and parameter set with each image's own lapping area, so the batch octree and the
fused assembly see reference-made answers too.
"""
import os
from collections import OrderedDict

import numpy as np
import pytest

from tests import ref_cases as RC

pytestmark = pytest.mark.gpu

FIXTURES = RC.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


@pytest.fixture(scope="module")
def loaded():
    return {p: RC.load(p) for p in FIXTURES}


def test_fixtures_present():
    assert len(FIXTURES) == len(RC.CASES) >= 15


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_extractor_equals_reference_fixture(loaded, path):
    import orbslam3lib_amd as og
    c, img, z = loaded[path]
    ex = og.ORBextractor(c.nfeatures, c.scale_factor, c.nlevels, c.ini_th, c.min_th, max_width=c.w, max_height=c.h,
                         max_images=2)
    k, d, mono = ex(img, None, c.lap)
    assert mono == z["mono"], c.name
    RC.same_kps(k, z["kps"], c.name)
    np.testing.assert_array_equal(d, z["desc"], err_msg=c.name)
    if c.levels:
        got = ex.level_keypoints(0)
        want = RC.split_levels(z)
        assert len(got) == len(want) == c.nlevels
        for level, ((gk, _), wk) in enumerate(zip(got, want)):
            RC.same_kps(gk, wk, "%s level %d" % (c.name, level))


def _batches(loaded):
    groups = OrderedDict()
    for p in FIXTURES:
        c = loaded[p][0]
        groups.setdefault((c.h, c.w, c.nfeatures, c.scale_factor, c.nlevels, c.ini_th, c.min_th), []).append(p)
    return groups


def test_batch_extractor_equals_reference_fixtures(loaded):
    import orbslam3lib_amd as og
    groups = _batches(loaded)
    assert max(len(g) for g in groups.values()) >= 4  # the mixed batches: five contents at 160x120, four at 320x240
    for (h, w, nf, sf, L, ini, mn), paths in groups.items():
        imgs = np.stack([loaded[p][1] for p in paths])
        laps = np.array([loaded[p][0].lap for p in paths], np.int32)
        be = og.BatchExtractor(nf, sf, L, ini, mn, width=w, height=h, max_images=len(paths))
        be.upload(imgs)
        be.run(laps)
        be.synchronize()
        for i, p in enumerate(paths):
            c, _, z = loaded[p]
            k, d, mono = be.result(i)
            assert mono == z["mono"], c.name
            RC.same_kps(k, z["kps"], c.name + " (batch)")
            np.testing.assert_array_equal(d, z["desc"], err_msg=c.name + " (batch)")
        be.close()
