"""bench.py --dump-outputs: the files hold what the timed path's last step computed.

* CPU: dump_outputs over a host stand-in -- every pair when they fit, a fixed seeded sample with
  the first and last pair under a smaller limit, the same sample on every call, float32 files.
* GPU: one small `bench.py --dump-outputs` run against the same batch extracted in this process
  (inputs are seeded, so two runs of one build agree row for row)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
NAMES = ("counts", "sample_pairs", "keypoints", "descriptors", "matches")


class _FakeBatch:
    """counts / result / matches of a batch whose image i has 5 + i % 3 keypoints."""

    def __init__(self, n_pairs):
        from orbslam3lib_amd import KEYPOINT_DTYPE
        self.n, self.dtype = 2 * n_pairs, KEYPOINT_DTYPE

    def _n(self, i):
        return 5 + i % 3

    def counts(self):
        n = np.array([self._n(i) for i in range(self.n)], np.int32)
        return n, n - 1

    def result(self, i, cap=65536):
        k = np.zeros(self._n(i), self.dtype)
        k["x"], k["octave"], k["class_id"] = 1000 * i + np.arange(len(k)), i % 8, -1
        return k, np.full((len(k), 32), i % 256, np.uint8), self._n(i) - 1

    def matches(self, pair, cap=65536):
        n = self._n(2 * pair)
        return tuple(np.full(n, 10 * pair + c, np.int32) for c in range(4))


def _load(d, suffix=""):
    out = {n: np.load(os.path.join(str(d), n + suffix + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 for a in out.values())
    return out


def test_dump_outputs_all_pairs_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    P = 40
    be = _FakeBatch(P)
    bench.dump_outputs(be, str(tmp_path / "all"), P)
    a = _load(tmp_path / "all")
    nk, mono = be.counts()
    np.testing.assert_array_equal(a["counts"], np.stack([nk, mono], 1))
    np.testing.assert_array_equal(a["sample_pairs"], np.arange(P))
    assert len(a["keypoints"]) == len(a["descriptors"]) == nk.sum() and a["keypoints"].shape[1] == 7
    assert len(a["matches"]) == nk[0::2].sum() and a["matches"].shape[1] == 4
    np.testing.assert_array_equal(a["keypoints"][:nk[0] + nk[1], 0],
                                  np.concatenate([np.arange(nk[0]), 1000 + np.arange(nk[1])]))
    # a limit that holds 6 pairs of the largest image size (and the counts): a sample, the same
    # one on every call, with the first and the last pair, rows in pair order
    per_pair = 4 * (2 * (7 + 32) + 4) * int(nk.max())
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 2 * P + 6 * per_pair + 17)
    bench.dump_outputs(be, str(tmp_path / "s1"), P)
    bench.dump_outputs(be, str(tmp_path / "s2"), P, rank=1, world=1)
    s1, s2 = _load(tmp_path / "s1"), _load(tmp_path / "s2", "_rank1")
    sample = s1["sample_pairs"].astype(int)
    assert len(sample) == 6 and sample[0] == 0 and sample[-1] == P - 1 and np.all(np.diff(sample) > 0)
    for n in NAMES:
        np.testing.assert_array_equal(s1[n], s2[n])
    assert sum(os.path.getsize(str(tmp_path / "s1" / (n + ".npy"))) - 128 for n in NAMES) <= bench.DUMP_BYTES
    np.testing.assert_array_equal(s1["matches"][:, 0], np.concatenate([np.full(nk[2 * p], 10 * p) for p in sample]))
    np.testing.assert_array_equal(s1["descriptors"][:, 0],
                                  np.concatenate([np.full(nk[i], i % 256) for p in sample for i in (2 * p, 2 * p + 1)]))


@pytest.mark.gpu
def test_bench_dump_matches_the_batch(tmp_path):
    import orbslam3lib_amd as og
    from orbslam3lib_amd import synth
    from orbslam3lib_amd.dist import pair_seed_base
    P, U, W, H, L, NF = 3, 2, 640, 480, 8, 2000  # the headline's frame shape, a batch of 6 images
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--pairs", str(P), "--unique-pairs", str(U), "--width", str(W), "--height", str(H), "--nlevels", str(L),
           "--nfeatures", str(NF), "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["full"] is False and line["ms_per_step"] > 0
    a = _load(tmp_path)
    uniq = [synth.stereo_pair(H, W, pair_seed_base(0) + i) for i in range(U)]
    be = og.BatchExtractor(NF, 1.2, L, 20, 7, width=W, height=H, max_images=2 * P)
    be.upload(np.stack([uniq[p % U][e] for p in range(P) for e in range(2)]))
    be.run(np.zeros((2 * P, 2), np.int32))
    be.match_stereo(stereo_rows_only=False)
    be.synchronize()
    nk, mono = be.counts()
    assert line["features_per_step_per_gpu"] == nk.sum() > 0
    np.testing.assert_array_equal(a["counts"], np.stack([nk, mono], 1))
    np.testing.assert_array_equal(a["sample_pairs"], np.arange(P))
    res = [be.result(i) for i in range(2 * P)]
    np.testing.assert_array_equal(a["keypoints"], np.concatenate(
        [np.stack([k[f].astype(np.float32) for f in FIELDS], 1) for k, _, _ in res]))
    np.testing.assert_array_equal(a["descriptors"], np.concatenate([d for _, d, _ in res]))
    np.testing.assert_array_equal(a["matches"], np.concatenate([np.stack(be.matches(p), 1) for p in range(P)]))
    be.close()
