"""Stage time of orbgpu_search_by_bow_batch beside
orbgpu_search_for_initialization_batch on the same frames: 256 pairs = 8 distinct 640x480 stereo
pairs repeated (keyframe = the left image's result, frame = the right image), 2000 features, about
100 nodes per pair (node = desc[0] * 100 >> 8), ORBmatcher(0.7, true); the k_sbp stage over CALLS
calls after a warm-up.  Asserts that the first pair equals the restatement and prints its counts.
    python tools/bow_search_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/bow_search_time.py   (no stage timer)
PAIRS=1 times a single pair (one TrackReferenceKeyFrame call); ORBGPU_LIB names another build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_search_by_bow as T  # noqa: E402
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
be.undistort_grid(K_, D_)  # for the initialisation search only
be.synchronize()

kfs, fnodes = [], []
for s in range(DISTINCT):
    (k, d, _), (_, dr, _) = be.result(2 * s), be.result(2 * s + 1)
    d, dr = d.reshape(-1, 32), dr.reshape(-1, 32)
    pts = np.zeros(len(k), og.BOW_POINT_DTYPE)
    pts["desc"], pts["angle"], pts["node"], pts["flags"] = d, k["angle"], nodes_of(d), og.BOW_HAS_POINT
    kfs.append(pts)
    fnodes.append(nodes_of(dr))
counts = [len(kfs[f % DISTINCT]) for f in range(PAIRS)]
packed = (np.concatenate([kfs[f % DISTINCT] for f in range(PAIRS)]),
          np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
stride = max(len(n) for n in fnodes)
node_rows = np.full((PAIRS, stride), -1, np.int32)
for f in range(PAIRS):
    node_rows[f, :len(fnodes[f % DISTINCT])] = fnodes[f % DISTINCT]
frame_ids = np.arange(PAIRS, dtype=np.int32) * 2 + 1
image_pairs = np.array([(2 * f, 2 * f + 1) for f in range(PAIRS)], np.int32)

calls = {"search_by_bow": lambda: be.search_by_bow(frame_ids, packed, node_rows, nnratio=0.7),
         "search_for_initialization": lambda: be.search_for_initialization(image_pairs, window_size=100)}
for what, call in calls.items():
    call()
    be.synchronize()
    if what == "search_by_bow":
        nm = sum(be.bow_matches(p)[1] for p in range(DISTINCT))
    else:
        nm = sum(be.initialization_matches(p)[2] for p in range(DISTINCT))
    if not TRACE:
        be.set_profiling(True, stages=["k_sbp"])
        be.reset_stage_times()
    for _ in range(CALLS):
        call()
    be.synchronize()
    if TRACE:
        print("%s: %d matches in the first %d pairs" % (what, nm, DISTINCT))
        continue
    ms, n = be.stage_times()["k_sbp"]
    be.set_profiling(False)
    per = ms / n
    print("%s: %.3f ms per call (%d calls), %.2f us per pair; %d matches in the first %d pairs"
          % (what, per, n, per * 1e3 / PAIRS, nm, DISTINCT))

calls["search_by_bow"]()
gm, gnm, ghist = be.bow_matches(0)
k0, d0, _ = be.result(0)
k1, d1, _ = be.result(1)
kf = T.KF(d0.reshape(-1, 32), k0["angle"].astype(np.float32), kfs[0]["node"].astype(np.int64), kfs[0]["flags"])
fb = T.FB(d1.reshape(-1, 32), k1["angle"].astype(np.float32), fnodes[0].astype(np.int64))
m, nm, hist, cnt = T._py_bow(kf, fb, 0.7, True)
assert np.array_equal(gm, m) and gnm == nm and np.array_equal(ghist, hist)
print("first pair, restatement: %d + %d keypoints, %d common nodes (at most %d frame keypoints in one), %d events, "
      "%d promoted, %d taken skipped, %d ratio failed, %d above TH_LOW, %d rejected, nmatches %d"
      % (len(kf.node), len(fb.node), cnt["common_nodes"], cnt["max_f_in_node"], cnt["events"], cnt["promoted"],
         cnt["taken_skipped"], cnt["ratio_failed"], cnt["above_th_low"], cnt["rejected"], nm))
be.close()
