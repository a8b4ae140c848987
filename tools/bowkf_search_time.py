"""Stage time of orbgpu_search_by_bow_kf_batch at the loop closer's shapes: one current
keyframe against 6 keyframes, against 18, and 256 pairs of their own (8 distinct 640x480 stereo pairs repeated;
keyframe 1 = the right image in the batch, keyframe 2 = the left image's result given by the host), 2000
features, about 100 nodes per pair (node = desc[0] * 100 >> 8), ORBmatcher(0.9, true); the k_sbp stage over
CALLS calls after a warm-up, REPEATS times per shape.  Asserts that the first pair equals the restatement.
    python tools/bowkf_search_time.py             the new search
    MODE=bow python tools/bowkf_search_time.py    the yardstick: orbgpu_search_by_bow_batch on the mirrored
                                                  inputs (keyframe = the left image's result, frame = the right
                                                  image): the same descriptors, nodes and amount of work
ORBGPU_LIB names another build (the yardstick runs on the parent commit's library); alternate the two modes in
separate processes.  TRACE=1 (under rocprofv3 --kernel-trace --stats ... --) runs the calls without the stage
timer."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_search_by_bow as T9  # noqa: E402

MODE = os.environ.get("MODE", "bowkf")
CALLS, REPEATS = 10, int(os.environ.get("REPEATS", 3))
TRACE = os.environ.get("TRACE") == "1"
DISTINCT, MAX_PAIRS, RATIO = 8, 256, 0.9
assert MODE in ("bowkf", "bow")


def nodes_of(desc):
    return (desc[:, 0].astype(np.int32) * 100) >> 8


frames = [synth.stereo_pair(480, 640, 50 + s) for s in range(DISTINCT)]
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=2 * MAX_PAIRS)
be.upload(np.stack([im for f in range(MAX_PAIRS) for im in frames[f % DISTINCT]]))
be.run()
be.synchronize()

left, right_nodes = [], []
for s in range(DISTINCT):
    (k, d, _), (_, dr, _) = be.result(2 * s), be.result(2 * s + 1)
    d, dr = d.reshape(-1, 32), dr.reshape(-1, 32)
    pts = np.zeros(len(k), og.BOW_POINT_DTYPE)
    pts["desc"], pts["angle"], pts["node"], pts["flags"] = d, k["angle"], nodes_of(d), og.BOW_HAS_POINT
    left.append(pts)
    right_nodes.append(nodes_of(dr))
stride = max(len(n) for n in right_nodes)


def shape(npairs, one_frame):
    """-> (frames [npairs], packed host points, node rows): pair p = batch image 1 (one_frame) or 2 p + 1
    against the left result p % DISTINCT."""
    kf = [left[p % DISTINCT] for p in range(npairs)]
    packed = (np.concatenate(kf), np.concatenate([[0], np.cumsum([len(k) for k in kf])]).astype(np.int32))
    ids = np.ones(npairs, np.int32) if one_frame else np.arange(npairs, dtype=np.int32) * 2 + 1
    rows = np.full((npairs, stride), -1, np.int32)
    for p in range(npairs):
        n = right_nodes[0] if one_frame else right_nodes[p % DISTINCT]
        rows[p, :len(n)] = n
    return ids, packed, rows


def call(ids, packed, rows):
    if MODE == "bowkf":
        be.search_by_bow_kf(ids, packed, rows, nnratio=RATIO)
    else:
        be.search_by_bow(ids, packed, rows, nnratio=RATIO)


for name, npairs, one_frame in (("1 frame x 6", 6, True), ("1 frame x 18", 18, True), ("256 pairs", 256, False)):
    args = shape(npairs, one_frame)
    call(*args)
    be.synchronize()
    series = []
    for _ in range(REPEATS):
        if not TRACE:
            be.set_profiling(True, stages=["k_sbp"])
            be.reset_stage_times()
        for _ in range(CALLS):
            call(*args)
        be.synchronize()
        if not TRACE:
            ms, n = be.stage_times()["k_sbp"]
            be.set_profiling(False)
            series.append(ms / n)
    print("%s %s: %s ms per call (%d calls each)" % (MODE, name, " ".join("%.4f" % v for v in series), CALLS), flush=True)

# the first pair of the last shape against the restatement
k0, d0, _ = be.result(0)
k1, d1, _ = be.result(1)
d0, d1 = d0.reshape(-1, 32), d1.reshape(-1, 32)
a0, a1 = k0["angle"].astype(np.float32), k1["angle"].astype(np.float32)
n0, n1 = left[0]["node"].astype(np.int64), right_nodes[0].astype(np.int64)
if MODE == "bowkf":
    from tests import test_search_by_bow_kf as T14  # noqa: E402
    got = be.bow_kf_matches(0)
    want = T14._py_bow_kf(T14.KP(d1, a1, n1, np.ones(len(n1), np.int32)), T14.KP(d0, a0, n0, left[0]["flags"]), RATIO, True)
    for g, w in zip(got, want[:5]):
        assert np.array_equal(g, w)
    cnt = want[5]
    print("first pair, restatement: %d + %d keypoints, %d common nodes (segments up to %d / %d), %d events, %d promoted, "
          "%d taken passed over, %d ratio failed, %d not below TH_LOW, %d rejected, nmatches %d"
          % (len(n1), len(n0), cnt["common_nodes"], cnt["max_seg_1"], cnt["max_seg_2"], cnt["events"], cnt["promoted"],
             cnt["taken_passed"], cnt["ratio_failed"], cnt["not_below_th_low"], cnt["rejected"], want[1]))
else:
    gm, gnm, ghist = be.bow_matches(0)
    m, nm, hist, cnt = T9._py_bow(T9.KF(d0, a0, n0, left[0]["flags"]), T9.FB(d1, a1, n1), RATIO, True)
    assert np.array_equal(gm, m) and gnm == nm and np.array_equal(ghist, hist)
    print("first pair, restatement: %d + %d keypoints, %d common nodes, %d events, %d taken skipped, nmatches %d"
          % (len(n0), len(n1), cnt["common_nodes"], cnt["events"], cnt["taken_skipped"], nm))
be.close()
