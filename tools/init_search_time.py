"""Stage time of orbgpu_search_for_initialization_batch beside
orbgpu_track_by_projection_batch on the same frames: 256 pairs = 8 distinct 640x480 stereo pairs
repeated (F1 = left, F2 = right), 2000 features, windowSize 100, ORBmatcher(0.9, true); the k_sbp
stage over CALLS calls after a warm-up.  Prints the restatement's counts for the first pair.
    python tools/init_search_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/init_search_time.py   (no stage timer)
PAIRS=1 times a single pair (one MonocularInitialization call); ORBGPU_LIB names another build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_search_for_initialization as T  # noqa: E402
from tests.test_track_projection import D_, K_, MB, MBF, _scene_pose  # noqa: E402

PAIRS, NPTS, CALLS, WINDOW = int(os.environ.get("PAIRS", 256)), 2000, 10, 100
DISTINCT = min(8, PAIRS)
TRACE = os.environ.get("TRACE") == "1"

frames = [synth.stereo_pair(480, 640, 50 + s) for s in range(DISTINCT)]
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=2 * PAIRS)
be.upload(np.stack([im for f in range(PAIRS) for im in frames[f % DISTINCT]]))
be.run()
be.undistort_grid(K_, D_)
be.stereo_matches(MBF, MB)
be.synchronize()
image_pairs = np.array([(2 * f, 2 * f + 1) for f in range(PAIRS)], np.int32)

pose, Rt = _scene_pose(0.01)
pts = []
for s in range(DISTINCT):
    k, d, _ = be.result(2 * s)
    pts.append(synth.last_frame_points(be.grid_result(2 * s)[0], k, d, K_, Rt, be.stereo_result(s)[0], n=NPTS, seed=s,
                                       mbf=MBF))
packed = (np.concatenate([pts[f % DISTINCT] for f in range(PAIRS)]), np.arange(PAIRS + 1, dtype=np.int32) * NPTS)
poses = np.array([pose] * PAIRS, og.TRACK_POSE_DTYPE)

calls = {"search_for_initialization": lambda: be.search_for_initialization(image_pairs, window_size=WINDOW),
         "track_by_projection": lambda: be.track_by_projection(packed, poses, K_, MBF, MB, image_step=2, use_uright=True)}
for what, call in calls.items():
    call()
    be.synchronize()
    if what == "search_for_initialization":
        nm = sum(be.initialization_matches(p)[2] for p in range(DISTINCT))
    else:
        nm = sum(be.track_matches(f)[1] for f in range(DISTINCT))
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

F = T._gpu_frames(be, ["F1", "F2"])
gm, _, gnm, _ = be.initialization_matches(0)
bounds, Kf, Df = np.zeros(4, np.float32), np.array(K_, np.float32), np.array(D_, np.float32)
og._check(og.load_library().orbgpu_image_bounds(640, 480, og._p(Kf), og._p(Df), len(Df), og._p(bounds)))
m, _, nm, hist, cnt = T._py_init(F["F1"], F["F2"], None, bounds, WINDOW, 0.9, True)
assert np.array_equal(gm, m) and gnm == nm
print("first pair, restatement: %d keypoints, %d searched, %d events, %d robbed, %d promoted, %d filtered, "
      "%d kept lists run dry (%d of them end in an event), nmatches %d"
      % (len(m), cnt["searched"], cnt["events"], cnt["robbed"], cnt["promoted"], cnt["filtered"], cnt["second_walk"],
         cnt["second_walk_event"], nm))
be.close()
