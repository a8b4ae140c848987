"""Stage time of orbgpu_sim3_search_by_projection_batch at the shapes LoopClosing calls it
in, on 2000-keypoint 640x480 frames: the points of a matched keyframe and its best covisibles against one
keyframe -- 1 pair x 8000 points, 3 pairs x 8000 points (three candidates' lists against one current
keyframe, each under its own pose) and 1 pair x 20000 points -- at th 8 / ratio 1.5 (the coarse search,
LoopClosing.cc:755, the vpPointsKFs overload) and th 3 / ratio 1.5 (FindMatchesByProjection, :964).  A
third of the points are in spAlreadyFound (a skip row), a third of the keypoints hold a point already.
Beside each: orbgpu_fuse_batch with sim3 = 1 on the same lists, frames, poses, skip rows and th -- the same
gates and window walk with no occupancy and no replay, the floor for the parallel part -- and what the
replay did, from orbgpu_sim3_replay_stats: the points that reached it, its passes, the lanes found stale
and the windows walked again.  The k_sbp stage over CALLS calls after a warm-up.  Asserts that the 1 x 8000
call equals the restatement.
    python tools/sim3_search_time.py
ORBGPU_LIB names another build: one without the Sim3 search (the parent's) prints the floor alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orbslam3lib_amd as og  # noqa: E402
from orbslam3lib_amd import synth  # noqa: E402
from tests import test_sim3_projection as T  # noqa: E402
from tests.test_track_projection import D_, K_  # noqa: E402

CALLS = 10
be = og.BatchExtractor(2000, 1.2, 8, 20, 7, width=640, height=480, max_images=3)
be.upload(np.stack([synth.stereo_pair(480, 640, 50 + s)[0] for s in range(3)]))
be.run()
be.undistort_grid(K_, D_)
be.synchronize()
lib = og.load_library()
HAVE_SIM3 = hasattr(lib, "orbgpu_sim3_search_by_projection_batch")
b, Kf, Df = np.zeros(4, np.float32), np.asarray(K_, np.float32), np.asarray(D_, np.float32)
og._check(lib.orbgpu_image_bounds(640, 480, og._p(Kf), og._p(Df), len(Df), og._p(b)))
bounds = [float(v) for v in b]
scale = np.zeros(8, np.float32)
og._check(lib.orbgpu_get_scale_tables(be.ctx.handle, og._p(scale), None, None, None, None))
kps, desc, _ = be.result(0)
desc = desc.reshape(-1, 32)
xy, _, cs, ci = be.grid_result(0)
print("frame 0: %d keypoints" % len(kps))

s0, R0, t0 = T._scene_sim3()
sims = [(s0, R0, t0), (s0 * 1.1, R0, t0 * 1.1 + 0.02), (s0 * 0.9, R0, t0 * 0.9 - 0.02)]
poses = np.array([synth.sim3_pose(s)[0] for s in sims], og.RELOC_POSE_DTYPE)
rng = np.random.default_rng(1)
blk = (rng.random((3, len(kps))) < 1 / 3).astype(np.uint8)


def time_call(call):
    call()
    be.synchronize()
    be.set_profiling(True, stages=["k_sbp"])
    be.reset_stage_times()
    for _ in range(CALLS):
        call()
    be.synchronize()
    ms, n = be.stage_times()["k_sbp"]
    be.set_profiling(False)
    return ms / n


for th, ratio, proj in ((8.0, 1.5, og.SIM3_PROJECT_INVZ), (3.0, 1.5, og.SIM3_PROJECT_DIV)):
    lists = {n: [synth.sim3_points(xy, kps, desc, K_, sims[q], n=n, seed=10 * q + n % 7, th=th, bounds=bounds,
                                   contested=0.1, contested_pool=400) for q in range(npairs)]
             for n, npairs in ((8000, 3), (20000, 1))}
    for npairs, n in ((1, 8000), (3, 8000), (1, 20000)):
        pts = lists[n][:npairs]
        skip = (rng.random((npairs, n)) < 1 / 3).astype(np.uint8)
        fr, ls = np.zeros(npairs, np.int32), np.arange(npairs, dtype=np.int32)
        what = "th %g ratio %g, %d pair(s) x %d points" % (th, ratio, npairs, n)
        floor = time_call(lambda: be.fuse(fr, ls, pts, poses[:npairs], K_, skip=skip, th=th, sim3=True))
        print("%s: k_fuse_match (sim3 = 1) %.3f ms per call, %.1f ns per point" % (what, floor, floor * 1e6 / (npairs * n)))
        if not HAVE_SIM3:
            continue

        def search():
            be.sim3_search_by_projection(fr, ls, pts, poses[:npairs], K_, skip=skip, kp_block=blk[:npairs], th=th,
                                         ratio_hamming=ratio, projection=proj)
        per = time_call(search)
        print("%s: sim3_search_by_projection %.3f ms per call, %.1f ns per point, %.1f times the floor"
              % (what, per, per * 1e6 / (npairs * n), per / floor))
        for q in range(npairs):
            pend, passes, stale, walks = be.sim3_replay_stats(q)
            groups = (pend + 63) // 64
            print("    pair %d: %d of %d points reach the replay (%d groups of 64), %d passes (%.2f a group), %d stale lanes, "
                  "%d windows walked again, nmatches %d" % (q, pend, n, groups, passes, passes / max(groups, 1), stale, walks,
                                                            be.sim3_matches(q)[4]))
        if (npairs, n) == (1, 8000):
            want = T._py_sim3_search(pts[0], poses[0], K_, xy, kps["octave"], desc, bounds, cs, ci, skip[0], blk[0], th, ratio,
                                     proj, scale)
            T._same(be.sim3_matches(0), want, len(kps))
            cnt = want[5]
            print("    restatement: %s, %d passed over as held, %d as taken, %d for their octave"
                  % (", ".join("%d %s" % (cnt[c], c) for c in T.CODES.values()), cnt["held"], cnt["taken"], cnt["octave"]))
be.close()
