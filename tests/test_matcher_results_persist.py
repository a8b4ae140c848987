"""Every matcher keeps its own results and its own record of what they cover: a search's rows stay
downloadable, unchanged, after the other four searches have run, and a call over no pairs leaves no
row behind.  (The five downloads share one function and one kind of coverage record in the context.)"""
import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_reloc_projection import _scene_pose as _reloc_scene_pose
from tests.test_track_projection import D_, K_, MB, MBF
from tests.test_track_projection import _scene_pose as _track_scene_pose


def _same(a, b):
    """Two downloads (tuples of arrays and counts) hold the same values."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_results_of_each_search_survive_the_other_four():
    import orbslam3lib_amd as og
    L, R = synth.stereo_pair(480, 640, 61)
    be = og.BatchExtractor(500, 1.2, 8, 20, 7, width=640, height=480, max_images=2)
    be.upload(np.stack([L, R]))
    be.run()
    be.stereo_matches(MBF, MB)
    be.undistort_grid(K_, D_)
    ur = be.stereo_result(0)[0]
    fr = []
    for i in range(2):
        kps, desc, _ = be.result(i)
        fr.append((kps, desc.reshape(-1, 32), be.grid_result(i)[0]))
    (kps0, desc0, xy0), (kps1, desc1, _) = fr
    assert len(kps0) >= 100 and len(kps1) >= 100

    mps = [synth.map_points(xy0, kps0["octave"], desc0, ur, n=300, seed=1)]
    tpose, tRt = _track_scene_pose(0.0)
    lps = [synth.last_frame_points(xy0, kps0, desc0, K_, tRt, ur, n=300, seed=2, mbf=MBF)]
    tposes = np.array([tpose], og.TRACK_POSE_DTYPE)
    kf = []  # two keyframes against image 0: the other eye's keypoints, whole and every second one
    for sel in (slice(None), slice(0, None, 2)):
        p = np.zeros(len(kps1[sel]), og.BOW_POINT_DTYPE)
        p["desc"], p["angle"], p["node"], p["flags"] = desc1[sel], kps1["angle"][sel], desc1[sel][:, 0] >> 4, 1
        kf.append(p)
    nodes = [(desc0[:, 0] >> 4).astype(np.int32)] * 2
    rpose, rRt = _reloc_scene_pose("small")
    rps = [synth.reloc_points(xy0, kps0, desc0, K_, rRt, n=n, seed=3 + n) for n in (300, 200)]
    rposes = np.array([rpose] * 2, og.RELOC_POSE_DTYPE)

    searches = [  # (the call, its download, its rows)
        (lambda: be.search_by_projection(mps), be.projection_matches, 1),
        (lambda: be.track_by_projection(lps, tposes, K_, MBF, MB), be.track_matches, 1),
        (lambda: be.search_for_initialization([[0, 1], [1, 0]]), be.initialization_matches, 2),
        (lambda: be.search_by_bow([0, 0], kf, nodes), be.bow_matches, 2),
        (lambda: be.reloc_by_projection([0, 0], rps, rposes, K_), be.reloc_matches, 2),
    ]
    first = []
    for call, download, rows in searches:  # each search's results right after its call
        call()
        first.append([download(r) for r in range(rows)])
    for got in first:  # the inputs are not degenerate: every row of every search matched something
        assert all(row[-2] > 0 if len(row) > 2 else row[-1] > 0 for row in got), [row[1:] for row in got]
    assert not np.array_equal(first[3][0][0], first[3][1][0]) and not np.array_equal(first[4][0][0], first[4][1][0])

    for call, _, _ in searches:  # all five back to back ...
        call()
    for (_, download, rows), want in reversed(list(zip(searches, first))):  # ... and every result at the end
        for r in reversed(range(rows)):
            _same(download(r), want[r])

    empty = [
        (lambda: be.search_for_initialization(np.zeros((0, 2), np.int32)), be.initialization_matches),
        (lambda: be.search_by_bow([], [], []), be.bow_matches),
        (lambda: be.reloc_by_projection([], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_), be.reloc_matches),
    ]
    for call, download in empty:  # a call over no pairs leaves no row, here or in another search
        call()
        with pytest.raises(og.OrbGpuError) as e:
            download(0)
        assert e.value.code == -3
    _same(be.projection_matches(0), first[0][0])
    _same(be.track_matches(0), first[1][0])
    be.close()
