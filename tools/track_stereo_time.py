"""Stage time of orbgpu_track_by_projection_stereo beside orbgpu_track_by_projection_batch on the
same left images: 256 frames = 8 distinct 640x480 stereo pairs repeated, 2000
last-frame points per frame, th 15; the k_sbp stage over CALLS calls after a warm-up.
    python tools/track_stereo_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/track_stereo_time.py   (no stage timer)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_track_projection_stereo as T  # noqa: E402
from tests.test_track_projection import MB, MBF, _scene_pose  # noqa: E402

FRAMES, DISTINCT, NPTS, CALLS = 256, 8, 2000, 10
TRACE = os.environ.get("TRACE") == "1"

pairs = [synth.stereo_pair(480, 640, 50 + s) for s in range(DISTINCT)]
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=2 * FRAMES)
be.upload(np.stack([im for f in range(FRAMES) for im in pairs[f % DISTINCT]]))
be.run()
be.undistort_grid(T.K_, ())
be.stereo_matches(MBF, MB)
be.synchronize()
rig = T._scene_rig()
for name, tz in (("neither", 0.01), ("forward", 0.5)):
    pose, Rt = _scene_pose(tz)
    two, one = [], []
    for s in range(DISTINCT):
        sides = T._gpu_sides(be, s)
        two.append(T.stereo_last_frame_points(*[(xy, k, d) for k, d, xy, _, _ in sides], rig, Rt, n=NPTS, seed=s))
        k, d, xy, _, _ = sides[0]
        one.append(synth.last_frame_points(xy, k, d, T.K_, Rt, be.stereo_result(s)[0], n=NPTS, seed=s, mbf=MBF))
    poses = np.array([pose] * FRAMES, og.TRACK_POSE_DTYPE)

    def packed(lists):
        rows = np.concatenate([lists[f % DISTINCT] for f in range(FRAMES)])
        return rows, np.arange(FRAMES + 1, dtype=np.int32) * NPTS

    calls = {"two-camera": lambda p=packed(two): be.track_by_projection_stereo(p, poses, rig, MB),
             "pinhole": lambda p=packed(one): be.track_by_projection(p, poses, T.K_, MBF, MB, image_step=2,
                                                                       use_uright=True)}
    for what, call in calls.items():
        call()
        be.synchronize()
        nm = sum(be.track_matches(f)[1] for f in range(DISTINCT))
        if not TRACE:
            be.set_profiling(True, stages=["k_sbp"])
            be.reset_stage_times()
        for _ in range(CALLS):
            call()
        be.synchronize()
        if TRACE:
            print("%s %s: %d matches in the first %d frames" % (name, what, nm, DISTINCT))
            continue
        ms, n = be.stage_times()["k_sbp"]
        be.set_profiling(False)
        per = ms / n
        print("%s %s: %.3f ms per call (%d calls), %.2f us per frame, %.2f ns per point; %d matches in the first %d "
              "frames" % (name, what, per, n, per * 1e3 / FRAMES, per * 1e6 / (FRAMES * NPTS), nm, DISTINCT))
be.close()
