"""Every matcher keeps its own results and its own record of what they cover, while all nine lay their
inputs and scratch out in one workspace they share: a search's rows stay downloadable, unchanged, after
the other eight searches have run, in either order, and a call over no pairs leaves no row behind.  (The
nine downloads share one function and one kind of record in the context.)"""
import numpy as np
import pytest

from orbslam3lib_amd import synth
from tests.test_reloc_projection import _scene_pose as _reloc_scene_pose
from tests.test_search_for_triangulation import F_STEREO, FAR
from tests.test_search_for_triangulation import _pairs as _tri_pairs
from tests.test_sim3_projection import _scene_sim3
from tests.test_track_projection import D_, K_, MB, MBF
from tests.test_track_projection import _scene_pose as _track_scene_pose


def _same(a, b):
    """Two downloads (tuples of arrays and counts) hold the same values."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_results_of_each_search_survive_the_other_eight():
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
    (kps0, desc0, xy0), (kps1, desc1, xy1) = fr
    assert len(kps0) >= 100 and len(kps1) >= 100

    mps = [synth.map_points(xy0, kps0["octave"], desc0, ur, n=300, seed=1)]
    tpose, tRt = _track_scene_pose(0.0)
    lps = [synth.last_frame_points(xy0, kps0, desc0, K_, tRt, ur, n=300, seed=2, mbf=MBF)]
    tposes = np.array([tpose], og.TRACK_POSE_DTYPE)
    # two keyframes against image 0: the other eye's keypoints, whole and every second one, as the rows of
    # the two bag-of-words searches and of the triangulation search
    kf, kf2, tri = [], [], []
    for sel in (slice(None), slice(0, None, 2)):
        for dtype, rows in ((og.BOW_POINT_DTYPE, kf), (og.BOWKF_POINT_DTYPE, kf2), (og.TRIANG_POINT_DTYPE, tri)):
            p = np.zeros(len(kps1[sel]), dtype)
            p["desc"], p["angle"], p["node"] = desc1[sel], kps1["angle"][sel], desc1[sel][:, 0] >> 4
            if rows is tri:
                p["x"], p["y"], p["octave"] = xy1[sel, 0], xy1[sel, 1], kps1["octave"][sel]
            else:
                p["flags"] = 1
            rows.append(p)
    nodes = [(desc0[:, 0] >> 4).astype(np.int32)] * 2
    has1 = [(np.arange(len(kps0)) % 5 != 0).astype(np.uint8)] * 2
    tpairs = _tri_pairs([(F_STEREO, FAR)] * 2)
    rpose, rRt = _reloc_scene_pose("small")
    rps = [synth.reloc_points(xy0, kps0, desc0, K_, rRt, n=n, seed=3 + n) for n in (300, 200)]
    rposes = np.array([rpose] * 2, og.RELOC_POSE_DTYPE)
    fps = [synth.fuse_points(xy0, kps0, desc0, K_, rRt, n=n, seed=5 + n) for n in (400, 250)]
    scw = _scene_sim3()
    sps = [synth.sim3_points(xy0, kps0, desc0, K_, scw, n=n, seed=7 + n) for n in (350, 220)]
    sposes = np.array([synth.sim3_pose(scw)[0]] * 2, og.RELOC_POSE_DTYPE)

    searches = {  # name -> (the call, its download, its rows, where the download has the row's count)
        "sbp": (lambda: be.search_by_projection(mps), be.projection_matches, 1, 1),
        "track": (lambda: be.track_by_projection(lps, tposes, K_, MBF, MB), be.track_matches, 1, 1),
        "init": (lambda: be.search_for_initialization([[0, 1], [1, 0]]), be.initialization_matches, 2, 2),
        "bow": (lambda: be.search_by_bow([0, 0], kf, nodes), be.bow_matches, 2, 1),
        "reloc": (lambda: be.reloc_by_projection([0, 0], rps, rposes, K_), be.reloc_matches, 2, 1),
        "tri": (lambda: be.search_for_triangulation([0, 0], tri, tpairs, nodes, coarse=True, check_orientation=True),
                be.triangulation_matches, 2, 1),
        "bowkf": (lambda: be.search_by_bow_kf([0, 0], kf2, nodes, has1), be.bow_kf_matches, 2, 1),
        "fuse": (lambda: be.fuse([0, 0], [0, 1], fps, rposes, K_), be.fuse_matches, 2, 4),
        "sim3": (lambda: be.sim3_search_by_projection([0, 0], [0, 1], sps, sposes, K_, projection=og.SIM3_PROJECT_INVZ),
                 lambda r: be.sim3_matches(r) + (be.sim3_replay_stats(r),), 2, 4),
    }
    first = {}
    for name, (call, download, rows, _) in searches.items():  # each search's results right after its call
        call()
        first[name] = [download(r) for r in range(rows)]
    for name, got in first.items():  # the inputs are not degenerate: every row of every search matched or fused something
        assert all(row[searches[name][3]] > 0 for row in got), (name, [row[searches[name][3]] for row in got])
    for name in ("bow", "reloc", "tri", "bowkf", "fuse", "sim3"):  # nor are a search's two rows one result twice
        assert not np.array_equal(first[name][0][0], first[name][1][0]), name

    # all nine back to back and every result at the end, last search first; then the calls themselves in
    # reverse order, so that another search is the one that grows the workspace
    for order in (list(searches), list(reversed(searches))):
        for name in order:
            searches[name][0]()
        for name in reversed(list(searches)):
            for r in reversed(range(searches[name][2])):
                _same(searches[name][1](r), first[name][r])

    empty = [
        (lambda: be.search_for_initialization(np.zeros((0, 2), np.int32)), be.initialization_matches),
        (lambda: be.search_by_bow([], [], []), be.bow_matches),
        (lambda: be.reloc_by_projection([], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_), be.reloc_matches),
        (lambda: be.search_for_triangulation([], [], np.zeros(0, og.TRIANG_PAIR_DTYPE), []), be.triangulation_matches),
        (lambda: be.search_by_bow_kf([], [], []), be.bow_kf_matches),
        (lambda: be.fuse([], [], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_), be.fuse_matches),
        (lambda: be.sim3_search_by_projection([], [], [], np.zeros(0, og.RELOC_POSE_DTYPE), K_), be.sim3_matches),
        (lambda: None, be.sim3_replay_stats),  # the Sim3 search's stats go with its rows
    ]
    for call, download in empty:  # a call over no pairs leaves no row, here or in another search
        call()
        with pytest.raises(og.OrbGpuError) as e:
            download(0)
        assert e.value.code == -3
    _same(be.projection_matches(0), first["sbp"][0])
    _same(be.track_matches(0), first["track"][0])
    be.close()
