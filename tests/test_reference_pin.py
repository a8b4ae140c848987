"""CPU: the oracle pinned to the reference extractor's own code.

tests/golden/ref_*.npz were written by the reference's ORBextractor_old.cc, compiled unchanged
(two generated edits) against stand-in headers by oracle/ref/Makefile (oracle/ref/README.md).

* Everywhere: oracle.extract / extract_levels equal every fixture, bit-exact.
* Where the reference is built (ref_py.available()): the fixtures regenerate from it, its
  constructor tables equal the oracle's, and seeded sweeps compare DistributeOctTree (also with
  the GPU's policy code, harness_octree) and whole extractions.  All comparisons are exact.
* The sanitized stand-alone program gives the digest of the unsanitized library.

What this pins and what it does not: oracle/ref/README.md.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_py
from tests import ref_cases as RC

FIXTURES = RC.fixture_paths()
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
live = pytest.mark.skipif(not ref_py.available(),
                          reason="oracle/_ref/libref_extractor.so is not built: no reference checkout at %s "
                                 "(oracle/ref/README.md)" % ref_py.reference_dir())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same_arrays(got, want, msg):
    assert int(got["mono"]) == int(want["mono"]), msg
    RC.same_kps(got["kps"], want["kps"], msg)
    np.testing.assert_array_equal(got["desc"], want["desc"], err_msg=msg)
    if "lvl_count" in want:
        np.testing.assert_array_equal(got["lvl_count"], want["lvl_count"], err_msg=msg)
        RC.same_kps(got["lvl_kps"], want["lvl_kps"], msg + " levels")


def test_fixture_set_is_the_case_list():
    assert IDS == sorted(c.name for c in RC.CASES)
    for c in RC.CASES:
        RC.assert_in_domain(c)
    assert sum(c.levels for c in RC.CASES) >= 2
    for p in FIXTURES:
        assert os.path.getsize(p) <= RC.MAX_FIXTURE_BYTES, p
    assert {c.lap for c in RC.CASES} == {(0, 0), (100, 250), (0, 1000)}


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_oracle_equals_reference_fixture(oracle, path):
    c, img, want = RC.load(path)
    assert RC.level_sizes(c) == oracle.level_sizes(c.w, c.h, c.scale_factor, c.nlevels)
    _, got = RC.compute(c, oracle)
    _same_arrays(got, want, c.name)
    sha = ref_py.reference_sha256()
    assert want["ref_cc_sha256"] == sha["ORBextractor_old.cc"] and want["ref_h_sha256"] == sha["ORBextractor_old.h"]


def test_fixtures_reach_the_paths_they_are_named_for(oracle):
    """The content each case is there for, checked on the fixtures and (for what a fixture does
    not record) on the oracle, which the test above ties to them."""
    by = {os.path.basename(p)[:-4]: RC.load(p) for p in FIXTURES}
    for name in ("ref_noise_160x120", "ref_noise_320x240"):  # N reached on every level
        c, img, z = by[name]
        want = oracle.features_per_level(c.nfeatures, c.scale_factor, c.nlevels)
        got = np.bincount(z["kps"]["octave"], minlength=c.nlevels).tolist()
        assert all(g >= w for g, w in zip(got, want)), (name, got, want)
    c, img, z = by["ref_lowcontrast_160x120"]
    assert 0 < len(z["kps"]) < 10
    for name in ("ref_dots_160x120", "ref_dots_320x240"):
        c, img, z = by[name]
        lvl0 = oracle.pyramid(img, c.scale_factor, c.nlevels)[0]
        with_fallback = len(oracle.level_candidates(lvl0, c.ini_th, c.min_th))
        without = len(oracle.level_candidates(lvl0, c.ini_th, 255))
        assert 0 < without < with_fallback, name  # some cells keep iniThFAST corners, some take the rerun
    c, img, z = by["ref_checker3_160x120"]
    lvl0 = z["kps"][z["kps"]["octave"] == 0]
    assert len(lvl0) == 0  # level 0: every pixel a candidate, every score equal, none passes the strict nonmax
    resp = z["kps"]["response"].astype(np.int64)
    assert np.bincount(resp).max() >= 16  # and long runs of equal responses on the resized levels
    c, img, z = by["ref_frame_160x120_n50"]
    assert 50 <= len(z["kps"]) < 70
    c, img, z = by["ref_frame_320x272_sf2"]
    assert RC.level_sizes(c) == [(320, 272), (160, 136), (80, 68)]  # exact 2x: the area path
    for name in ("ref_noise_160x120", "ref_frame_320x240", "ref_frame_641x401"):  # both sides of the lap
        c, img, z = by[name]
        assert 0 < z["mono"] < len(z["kps"]), name
    # keypoints exactly on the inclusive bounds of the lapping area (:1171), in the stereo part
    c, img, z = by["ref_noise_160x120"]
    assert (z["kps"]["x"][z["mono"]:] == 100).any()
    c, img, z = by["ref_frame_320x240"]
    assert (z["kps"]["x"][z["mono"]:] == 100).any() and (z["kps"]["x"][z["mono"]:] == 250).any()


def test_reference_is_built_where_it_exists():
    """A silently failed build of the recipe would turn every live test below into a skip."""
    if not ref_py.reference_present():
        pytest.skip("no reference checkout at %s" % ref_py.reference_dir())
    assert ref_py.available(), "reference checkout present but oracle/_ref/libref_extractor.so is missing: run make"
    assert os.path.exists(ref_py.SELFTEST_PATH), "oracle/_ref/ref_selftest is missing: run make"


@live
@pytest.mark.parametrize("c", RC.CASES, ids=[c.name for c in RC.CASES])
def test_fixture_regenerates_from_live_reference(c):
    _, img, want = RC.load(RC.fixture_path(c))
    _, got = RC.compute(c, ref_py)
    _same_arrays(got, want, c.name)


@live
@pytest.mark.parametrize("nf,sf,L", [(1000, 1.2, 8), (2000, 1.2, 8), (5000, 1.2, 12), (500, 2.0, 3), (3000, 2.5, 4),
                                     (50, 1.2, 8)])
def test_constructor_tables(oracle, nf, sf, L):
    t = ref_py.tables(nf, sf, L)
    assert t["levels"] == L and t["scale_factor"] == float(np.float32(sf))
    assert t["umax"].tolist() == oracle.umax()
    assert t["features_per_level"].tolist() == oracle.features_per_level(nf, sf, L)
    for a, b in zip((t["scale"], t["inv_scale"], t["sigma2"], t["inv_sigma2"]), oracle.scale_factors(sf, L)):
        np.testing.assert_array_equal(a, b)
    with open(os.path.join(RC.GOLD, "pattern.json")) as f:
        pat = json.load(f)
    flat = t["pattern"].reshape(-1)
    assert len(flat) == 4 * pat["n_pairs"] and np.abs(flat).max() < 128
    assert hashlib.sha256(flat.astype(np.int8).tobytes()).hexdigest() == pat["sha256_int8"]
    assert flat[:4].tolist() == pat["first_pair"] and flat[-4:].tolist() == pat["last_pair"]


# ---- DistributeOctTree sweep ------------------------------------------------------------------
WIDTHS, HEIGHTS = (64, 127, 300, 608, 1888), (40, 64, 200, 448, 1048)
# every (W, H) of the two lists with nIni = round(W / H) >= 1, as the reference computes it: built
# from the lists, so no drawn case is ever rejected
WH = [(w, h) for w in WIDTHS for h in HEIGHTS if int(np.rint(np.float32(w) / np.float32(h))) >= 1]
NS, CAPS = (0, 1, 2, 5, 50, 400, 3000), (0, 1, 7, 60, 500, 5000)
FAMILIES = ("clusters", "lattice", "row", "ties")
N_OCTREE_CASES = 336


def _keys(rng, family, n, W, H, wide_response):
    """n candidate keys in [0, W) x [0, H), integer coordinates as FAST gives them."""
    if family == "clusters":    # a few tight clusters, with exact duplicates
        k = int(rng.integers(1, 5))
        cx, cy = rng.integers(0, W, k), rng.integers(0, H, k)
        pick = rng.integers(0, k, n)
        x = np.clip(cx[pick] + rng.integers(-6, 7, n), 0, W - 1)
        y = np.clip(cy[pick] + rng.integers(-6, 7, n), 0, H - 1)
        if n > 3:
            dup = rng.integers(0, n, n // 3)
            x[dup], y[dup] = x[(dup + 1) % n], y[(dup + 1) % n]
    elif family == "lattice":   # a regular grid: equal node sizes, so compareNodes ties on size
        step = int(rng.choice([2, 3, 4, 8]))
        gx, gy = np.meshgrid(np.arange(1, W, step), np.arange(1, H, step))
        idx = rng.permutation(gx.size)[:n] if rng.random() < 0.5 else np.arange(min(n, gx.size))
        x, y = gx.reshape(-1)[idx], gy.reshape(-1)[idx]
        if len(x) < n:
            extra = rng.integers(0, len(x), n - len(x))
            x, y = np.concatenate([x, x[extra]]), np.concatenate([y, y[extra]])
    elif family == "row":       # one row
        x, y = rng.integers(0, W, n), np.full(n, int(rng.integers(0, H)))
    else:                       # uniform positions; the response range makes the ties
        x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    keys = np.zeros(n, RC.KP_DTYPE)
    keys["x"], keys["y"] = x, y
    keys["response"] = rng.integers(0, 256, n) if wide_response else rng.integers(20, 23, n)
    keys["size"], keys["angle"], keys["class_id"] = 7, -1, -1
    return keys


def _octree_cases():
    rng = np.random.default_rng(2025)
    for i in range(N_OCTREE_CASES):
        W, H = WH[i % len(WH)]
        family = FAMILIES[(i // len(WH)) % 4]
        n, N = int(rng.choice(NS)), int(rng.choice(CAPS))
        yield i, family, W, H, N, _keys(rng, family, n, W, H, wide_response=bool(i & 1))


@live
def test_distribute_octree_sweep(oracle, harness):
    """reference == oracle == the GPU's policy code on the CPU (harness_octree), per case."""
    seen = set()
    for i, family, W, H, N, keys in _octree_cases():
        msg = "case %d %s %dx%d n=%d N=%d" % (i, family, W, H, len(keys), N)
        ref = ref_py.distribute_octree(keys, 16, 16 + W, 16, 16 + H, N)
        RC.same_kps(oracle.distribute_octree(keys, 16, 16 + W, 16, 16 + H, N), ref, msg)
        packed = (keys["x"].astype(np.uint32) | (keys["y"].astype(np.uint32) << 12) |
                  (keys["response"].astype(np.uint32) << 24)).astype(np.uint32)
        out = np.zeros(len(keys) + 4 * N + 64, np.uint32)
        m = harness.harness_octree(_p(packed), len(keys), W, H, N, _p(out), len(out))
        assert m == len(ref), msg
        o = out[:m]
        np.testing.assert_array_equal((o & 0xFFF).astype(np.float32), ref["x"], err_msg=msg)
        np.testing.assert_array_equal(((o >> 12) & 0xFFF).astype(np.float32), ref["y"], err_msg=msg)
        np.testing.assert_array_equal((o >> 24).astype(np.float32), ref["response"], err_msg=msg)
        seen.add((family, i & 1))
    assert len(seen) == 8 and N_OCTREE_CASES >= 300


@live
def test_whole_extraction_sweep(oracle):
    """36 seeded extractions at 160x120 and 320x240: every generator, parameter sets and lapping
    areas drawn per case, reference against oracle."""
    rng = np.random.default_rng(77)
    kinds = ("frame", "noise", "checker3", "dots", "lowcontrast", "frame")
    for i in range(36):
        small = i % 2 == 0
        h, w = (120, 160) if small else (240, 320)
        c = RC.Case("sweep%d" % i, h, w, kinds[i % 6], 100 + i, int(rng.choice([50, 300, 500, 1000])), 1.2,
                    int(rng.integers(1, 5 if small else 7)), *[(20, 7), (0, 0), (40, 3), (12, 4)][int(rng.integers(0, 4))],
                    [(0, 0), (100, 250), (0, 1000)][i % 3], i % 4 == 0)
        RC.assert_in_domain(c)
        _, want = RC.compute(c, ref_py)
        _, got = RC.compute(c, oracle)
        _same_arrays(got, want, repr(c))


@live
def test_sanitized_selftest_digest():
    """oracle/ref/selftest.cpp built with AddressSanitizer as a stand-alone program (no Python, no
    preloading): clean exit, and the digest of the unsanitized library."""
    r = subprocess.run([ref_py.SELFTEST_PATH], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    digest, n = ref_py.selftest_digest()
    assert r.stdout.split() == ["ref_selftest", "digest", "%016x" % digest, "keypoints", str(n)], r.stdout
    assert n > 100
