"""Stage time of orbgpu_search_for_triangulation_batch beside
orbgpu_search_by_bow_batch on the same frames and nodes in the same run: PAIRS = 256 pairs = 8
distinct 640x480 stereo pairs repeated (keyframe 1 = the right image, a batch image; keyframe 2 = the
left image's result, 2000 features, about 100 nodes per pair (node = desc[0] * 100 >> 8), R = I and
t = (b, 0, 0), the epipole on a keypoint), and CreateNewMapPoints' own shape: one frame against 10
and against 30 keyframes of 2000 points, each with its own F12 and epipole; the k_sbp stage over
CALLS calls after a warm-up.  Asserts that the first pair equals the restatement and prints its counts.
    python tools/tri_search_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/tri_search_time.py   (no stage timer)
ORBGPU_LIB names another build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_search_for_triangulation as T  # noqa: E402
from tests.test_track_projection import D_, K_  # noqa: E402

PAIRS, CALLS = int(os.environ.get("PAIRS", 256)), 10
DISTINCT = min(8, PAIRS)
TRACE = os.environ.get("TRACE") == "1"


def nodes_of(desc):
    return (desc[:, 0].astype(np.int32) * 100) >> 8


frames = [synth.stereo_pair(480, 640, 50 + s) for s in range(DISTINCT)]
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=2 * PAIRS)
be.upload(np.stack([im for f in range(PAIRS) for im in frames[f % DISTINCT]]))
be.run()
be.undistort_grid(K_, D_)
be.synchronize()

tri, bow, fnodes, fflags, geo = [], [], [], [], []
for s in range(DISTINCT):
    (k, d, _), (kr, dr, _) = be.result(2 * s), be.result(2 * s + 1)
    d, dr, xy = d.reshape(-1, 32), dr.reshape(-1, 32), be.grid_result(2 * s)[0]
    k2 = T.K2(d, xy, k["angle"].astype(np.float32), k["octave"].astype(np.int32), nodes_of(d).astype(np.int64),
              T._flags(len(k))[::-1].copy())
    tri.append(T._points(k2))
    pts = np.zeros(len(k), og.BOW_POINT_DTYPE)
    pts["desc"], pts["angle"], pts["node"], pts["flags"] = d, k["angle"], nodes_of(d), og.BOW_HAS_POINT
    bow.append(pts)
    fnodes.append(nodes_of(dr))
    fflags.append(T._flags(len(kr)).astype(np.uint8))
    geo.append((T.F_STEREO, xy[len(xy) // 2]))


def packed(lists, which):
    counts = [len(lists[w]) for w in which]
    return (np.concatenate([lists[w] for w in which]), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))


def rows(lists, which, fill, dtype):
    out = np.full((len(which), max(len(r) for r in lists)), fill, dtype)
    for p, w in enumerate(which):
        out[p, :len(lists[w])] = lists[w]
    return out


def shape(frame_ids, which):
    """(frames, tri points, bow points, pairs, node rows, flag rows): pair p = frame frame_ids[p], keyframe which[p]."""
    return (np.asarray(frame_ids, np.int32), packed(tri, which), packed(bow, which), T._pairs([geo[w] for w in which]),
            rows(fnodes, [(f - 1) // 2 % DISTINCT for f in frame_ids], -1, np.int32),
            rows(fflags, [(f - 1) // 2 % DISTINCT for f in frame_ids], 0, np.uint8))


shapes = {"%d pairs" % PAIRS: shape(np.arange(PAIRS) * 2 + 1, [f % DISTINCT for f in range(PAIRS)])}
for nkf in (10, 30):  # CreateNewMapPoints: the new keyframe (image 1) against its neighbours
    if nkf <= 2 * PAIRS:
        shapes["1 frame x %d keyframes" % nkf] = shape(np.ones(nkf, np.int32), [c % DISTINCT for c in range(nkf)])

for name, (fr, tpts, bpts, pr, nrows, frows) in shapes.items():
    calls = {"search_for_triangulation": lambda: be.search_for_triangulation(fr, tpts, pr, nrows, frows),
             "search_for_triangulation coarse": lambda: be.search_for_triangulation(fr, tpts, pr, nrows, frows, coarse=True),
             "search_by_bow": lambda: be.search_by_bow(fr, bpts, nrows, nnratio=0.7)}
    for what, call in calls.items():
        call()
        be.synchronize()
        if not TRACE:
            be.set_profiling(True, stages=["k_sbp"])
            be.reset_stage_times()
        for _ in range(CALLS):
            call()
        be.synchronize()
        if TRACE:
            print(name, what)
            continue
        ms, n = be.stage_times()["k_sbp"]
        be.set_profiling(False)
        per = ms / n
        print("%s, %s: %.3f ms per call (%d calls), %.2f us per pair" % (name, what, per, n, per * 1e3 / len(fr)))

fr, tpts, bpts, pr, nrows, frows = shapes["%d pairs" % PAIRS]
be.search_for_triangulation(fr, tpts, pr, nrows, frows)
gm, gnm, ghist = be.triangulation_matches(0)
k1r, d1r, _ = be.result(1)
k1 = T.K1(d1r.reshape(-1, 32), be.grid_result(1)[0], k1r["angle"].astype(np.float32), fnodes[0].astype(np.int64),
          fflags[0].astype(np.int32))
p0 = tri[0]
k2 = T.K2(p0["desc"], np.stack([p0["x"], p0["y"]], 1), p0["angle"], p0["octave"], p0["node"].astype(np.int64), p0["flags"])
m, nm, hist, cnt = T._py_tri(k1, k2, *geo[0])
assert np.array_equal(gm, m) and gnm == nm and np.array_equal(ghist, hist)
print("first pair, restatement: %d + %d keypoints, %d common nodes (segments up to %d and %d), %d events, %d equal "
      "replaced, %d shared partners, %d failed the epipolar test within TH_LOW, %d in the epipole disc, nmatches %d"
      % (len(k1.node), len(k2.node), cnt["common_nodes"], cnt["max_seg_1"], cnt["max_seg_2"], cnt["events"],
         cnt["equal_replaced"], cnt["shared"], cnt["epipolar_rejected"], cnt["epipole_disc"], nm))
be.close()
