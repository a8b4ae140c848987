"""Stage time of orbgpu_reloc_by_projection_batch beside
orbgpu_track_by_projection_batch on the same frames and point count: PAIRS = 256 pairs on 256
images (8 distinct 640x480 left images repeated, 2000 features) x 2000 points at (th, ORBdist) =
(10, 100), and Relocalization's own shape: 1 frame x 8 candidate keyframes x 2000 points, each with
its own points and pose; the k_sbp stage over CALLS calls after a warm-up.  Asserts that the first
pair equals the restatement and prints its counts.
    python tools/reloc_search_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/reloc_search_time.py   (no stage timer)
ORBGPU_LIB names another build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_reloc_projection as T  # noqa: E402
from tests.test_track_projection import D_, K_  # noqa: E402

PAIRS, CALLS, NPTS = int(os.environ.get("PAIRS", 256)), 10, 2000
DISTINCT = min(8, PAIRS)
TRACE = os.environ.get("TRACE") == "1"
MBF, MB = 47.9, float(np.float32(47.9) / np.float32(435.2))

lefts = [synth.stereo_pair(480, 640, 50 + s)[0] for s in range(DISTINCT)]
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=PAIRS)
be.upload(np.stack([lefts[f % DISTINCT] for f in range(PAIRS)]))
be.run()
be.undistort_grid(K_, D_)
be.synchronize()
lib = og.load_library()
b, Kf, Df = np.zeros(4, np.float32), np.asarray(K_, np.float32), np.asarray(D_, np.float32)
og._check(lib.orbgpu_image_bounds(640, 480, og._p(Kf), og._p(Df), len(Df), og._p(b)))
bounds = [float(v) for v in b]
scale = np.zeros(8, np.float32)
og._check(lib.orbgpu_get_scale_tables(be.ctx.handle, og._p(scale), None, None, None, None))

pose, Rt = T._scene_pose("small")
reloc, track = [], []
for s in range(DISTINCT):
    kps, desc, _ = be.result(s)
    xy = be.grid_result(s)[0]
    reloc.append(synth.reloc_points(xy, kps, desc, K_, Rt, n=NPTS, seed=s, th=10.0, bounds=bounds))
    track.append(synth.last_frame_points(xy, kps, desc, K_, Rt, None, n=NPTS, seed=s, th=10.0, bounds=bounds))


def packed(lists, n):
    return (np.concatenate([lists[f % DISTINCT] for f in range(n)]), np.arange(n + 1, dtype=np.int32) * NPTS)


tpose = np.zeros(PAIRS, og.TRACK_POSE_DTYPE)
tpose["Rcw"], tpose["tcw"] = pose["Rcw"], pose["tcw"]
tpose["Rlw"], tpose["tlw"] = np.eye(3).reshape(9), Rt[0].T @ Rt[1]
rposes = np.array([pose] * PAIRS, og.RELOC_POSE_DTYPE)
all_reloc, all_track = packed(reloc, PAIRS), packed(track, PAIRS)
# Relocalization: image 0 against 8 candidate keyframes; the points of candidate c are another draw on the same frame
kps0, desc0, _ = be.result(0)
xy0 = be.grid_result(0)[0]
NCAND = min(8, PAIRS)
cands = [synth.reloc_points(xy0, kps0, desc0, K_, Rt, n=NPTS, seed=100 + c, th=10.0, bounds=bounds) for c in range(NCAND)]
cand_pts = (np.concatenate(cands), np.arange(NCAND + 1, dtype=np.int32) * NPTS)

calls = {
    "reloc_by_projection %d pairs x %d" % (PAIRS, NPTS):
        (PAIRS, lambda: be.reloc_by_projection(np.arange(PAIRS), all_reloc, rposes, K_, th=10.0, orb_dist=100)),
    "reloc_by_projection 1 frame x %d keyframes x %d" % (NCAND, NPTS):
        (NCAND, lambda: be.reloc_by_projection(np.zeros(NCAND, np.int32), cand_pts, rposes[:NCAND], K_, th=10.0,
                                               orb_dist=100)),
    "track_by_projection %d frames x %d" % (PAIRS, NPTS):
        (PAIRS, lambda: be.track_by_projection(all_track, tpose, K_, MBF, MB, image_step=1, use_uright=False, th=10.0,
                                               mono=True)),
}
for what, (npairs, call) in calls.items():
    call()
    be.synchronize()
    if not TRACE:
        be.set_profiling(True, stages=["k_sbp"])
        be.reset_stage_times()
    for _ in range(CALLS):
        call()
    be.synchronize()
    if TRACE:
        print(what)
        continue
    ms, n = be.stage_times()["k_sbp"]
    be.set_profiling(False)
    per = ms / n
    print("%s: %.3f ms per call (%d calls), %.2f us per pair, %.1f ns per point"
          % (what, per, n, per * 1e3 / npairs, per * 1e6 / (npairs * NPTS)))

list(calls.values())[0][1]()
gm, gnm, ghist = be.reloc_matches(0)
xy, _, cs, ci = be.grid_result(0)
m, nm, hist, cnt = T._py_reloc(reloc[0], pose, K_, xy, kps0["octave"], kps0["angle"], desc0.reshape(-1, 32), bounds, cs, ci,
                               None, 10.0, 100, True, scale)
assert np.array_equal(gm, m) and gnm == nm and np.array_equal(ghist, hist)
print("first pair, restatement: %d keypoints, %d points, %d events, %d taken skipped, %d above ORBdist, %d lists dry "
      "(%d still matched), %d rejected, nmatches %d"
      % (len(kps0), NPTS, cnt["events"], cnt["taken"], cnt["above_orb_dist"], cnt["list_dry"], cnt["list_dry_matched"],
         cnt["rejected"], nm))
be.close()
