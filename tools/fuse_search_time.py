"""Stage time of orbgpu_fuse_batch beside orbgpu_reloc_by_projection_batch on the
same frames, positions, descriptors, th and poses (the relocalisation search does the same
projection, level and window walk, plus a sequential replay), on PAIRS images (8 distinct 640x480
left images repeated, 2000 features), in LocalMapping::SearchInNeighbors' shapes:
  (a) one list of 2000 points against 10 and against 30 frames, with skip rows (the forward leg; the
      relocalisation search has no shared list: it gets the points once per pair);
  (b) one list of 40000 points -- 20 frames' points under their own back-projection -- into one frame
      (the backward leg);
  (c) PAIRS pairs of 2000 points.
The k_sbp stage over CALLS calls after a warm-up.  Asserts that the first pair of (c) equals the
restatement and prints its counts.
    python tools/fuse_search_time.py            stage timer
    TRACE=1 rocprofv3 --kernel-trace --stats ... -- python tools/fuse_search_time.py   (no stage timer)
ORBGPU_LIB names another build (ORBGPU_FUSE_G = 1, 4, 8 lanes per point)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_fuse as T  # noqa: E402
from tests.test_reloc_projection import _scene_pose  # noqa: E402
from tests.test_track_projection import D_, K_, MBF  # noqa: E402

PAIRS, CALLS, NPTS, TH = int(os.environ.get("PAIRS", 256)), 10, 2000, 3.0
DISTINCT = min(8, PAIRS)
TRACE = os.environ.get("TRACE") == "1"

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
tabs = [np.zeros(8, np.float32) for _ in range(4)]
og._check(lib.orbgpu_get_scale_tables(be.ctx.handle, og._p(tabs[0]), None, None, og._p(tabs[3]), None))

pose, Rt = _scene_pose("small")
frames = []
for s in range(DISTINCT):
    kps, desc, _ = be.result(s)
    frames.append((kps, desc.reshape(-1, 32), be.grid_result(s)[0]))
fuse = [synth.fuse_points(xy, kps, desc, K_, Rt, n=NPTS, seed=s, th=TH, bounds=bounds) for s, (kps, desc, xy) in enumerate(frames)]


def as_reloc(pts):
    r = np.zeros(len(pts), og.RELOC_POINT_DTYPE)
    for f in ("pos", "min_distance", "max_distance", "flags", "desc"):
        r[f] = pts[f]
    return r


def offsets(n, step):
    return np.arange(n + 1, dtype=np.int32) * step


poses = np.array([pose] * PAIRS, og.RELOC_POSE_DTYPE)
rng = np.random.default_rng(1)
calls = {}
for nf in (10, 30):  # (a)
    if nf > PAIRS:
        continue
    skip = (rng.random((nf, NPTS)) < 0.3).astype(np.uint8)
    rl = (np.concatenate([as_reloc(fuse[0])] * nf), offsets(nf, NPTS))
    calls["(a) 1 list x %d frames x %d" % (nf, NPTS)] = (
        nf * NPTS,
        lambda nf=nf, skip=skip: be.fuse(np.arange(nf), np.zeros(nf, np.int32), [fuse[0]], poses[:nf], K_, skip=skip, th=TH, bf=MBF),
        lambda nf=nf, rl=rl: be.reloc_by_projection(np.arange(nf), rl, poses[:nf], K_, th=TH, orb_dist=50))
long_list = np.concatenate([synth.fuse_points(frames[s % DISTINCT][2], frames[s % DISTINCT][0], frames[s % DISTINCT][1], K_, Rt,
                                              n=NPTS, seed=100 + s, th=TH, bounds=bounds) for s in range(20)])
long_reloc = as_reloc(long_list)
calls["(b) 1 list of %d x 1 frame" % len(long_list)] = (
    len(long_list),
    lambda: be.fuse([0], [0], [long_list], poses[:1], K_, th=TH, bf=MBF),
    lambda: be.reloc_by_projection([0], [long_reloc], poses[:1], K_, th=TH, orb_dist=50))
all_fuse = (np.concatenate([fuse[f % DISTINCT] for f in range(PAIRS)]), offsets(PAIRS, NPTS))
all_reloc = (as_reloc(all_fuse[0]), all_fuse[1])
calls["(c) %d pairs x %d" % (PAIRS, NPTS)] = (
    PAIRS * NPTS,
    lambda: be.fuse(np.arange(PAIRS), np.arange(PAIRS), all_fuse, poses, K_, th=TH, bf=MBF),
    lambda: be.reloc_by_projection(np.arange(PAIRS), all_reloc, poses, K_, th=TH, orb_dist=50))

for what, (npoints, fuse_call, reloc_call) in calls.items():
    for name, call in (("fuse", fuse_call), ("reloc_by_projection", reloc_call)):
        call()
        be.synchronize()
        if not TRACE:
            be.set_profiling(True, stages=["k_sbp"])
            be.reset_stage_times()
        for _ in range(CALLS):
            call()
        be.synchronize()
        if TRACE:
            print(what, name)
            continue
        ms, n = be.stage_times()["k_sbp"]
        be.set_profiling(False)
        per = ms / n
        print("%s %s: %.3f ms per call (%d calls), %.1f ns per point" % (what, name, per, n, per * 1e6 / npoints))

list(calls.values())[-1][1]()
got = be.fuse_matches(0)
kps0, desc0, _ = frames[0]
xy0, _, cs, ci = be.grid_result(0)
want = T._py_fuse(fuse[0], pose, K_, xy0, kps0["octave"], desc0, None, bounds, cs, ci, None, TH, MBF, False, tabs[0], tabs[3])
T._same(got, want, len(kps0))
cnt = want[5]
print("first pair, restatement: %d keypoints, %d points, %s, %d keypoints claimed more than once, nfused %d"
      % (len(kps0), NPTS, ", ".join("%d %s" % (cnt[c], c) for c in T.CODES.values()), cnt["multi_claimed"], want[4]))
be.close()
