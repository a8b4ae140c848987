"""CPU: the direct phase 1 of orb_octree.h (the node list straight from the count pyramid) against
the round-by-round phase 1, the oracle and, where it is built, the reference's DistributeOctTree.

Every comparison is exact: the same count and the same keys in the same order.  The harness
(tests/harness/octree_direct_harness.hip, host compile, SerialPolicy) reports how many rounds of
the loop ran and how many of them were phase-1 rounds, so a dead switch cannot pass."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_py
from orbslam3lib_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "octree_direct_harness.hip")
LIB = os.path.join(ROOT, "tests", "harness", "build", "liboctree_direct_harness.so")
CAPS_N = (1, 5, 50, 434, 2000)
SHAPES = ((608, 448), (1245, 600), (633, 211))  # nIni = 1, 2, 3
DEPTHS = (1, 3, 5, 7)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def direct():
    csrc = os.path.join(ROOT, "orbslam3lib_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC",
                               "-ffp-contract=off", "-shared", "-o", LIB, SRC])
    lib = C.CDLL(LIB)
    lib.octd_key_of_path.restype = C.c_uint32
    lib.octd_path_of_key.restype = C.c_uint32
    return lib


def _pack(keys):
    return (keys["x"].astype(np.uint32) | (keys["y"].astype(np.uint32) << 12) |
            (keys["response"].astype(np.uint32) << 24)).astype(np.uint32)


def _run(lib, packed, W, H, N, D, rounds, cap=0):
    out = np.zeros(len(packed) + 4 * max(N, 1) + 64, np.uint32)
    deep = C.c_int(0)
    counts = (C.c_longlong * 2)()
    m = lib.octd_octree(_p(packed), len(packed), W, H, N, cap, D, rounds, _p(out), len(out), C.byref(deep), counts)
    return m, out[:max(m, 0)], deep.value, counts[0], counts[1]


def _same(out, ref, msg):
    np.testing.assert_array_equal((out & 0xFFF).astype(np.float32), ref["x"], err_msg=msg)
    np.testing.assert_array_equal(((out >> 12) & 0xFFF).astype(np.float32), ref["y"], err_msg=msg)
    np.testing.assert_array_equal((out >> 24).astype(np.float32), ref["response"], err_msg=msg)


def _check(lib, oracle, keys, W, H, N, depths=DEPTHS, seen=None):
    """direct == rounds == oracle (== reference), and the round counters, at every depth."""
    ref = oracle.distribute_octree(keys, 16, 16 + W, 16, 16 + H, N)
    if ref_py.available():
        live = ref_py.distribute_octree(keys, 16, 16 + W, 16, 16 + H, N)
        assert len(live) == len(ref)
        for f in ("x", "y", "response"):
            np.testing.assert_array_equal(live[f], ref[f])
    packed = _pack(keys)
    for D in depths:
        msg = "%dx%d n=%d N=%d D=%d" % (W, H, len(keys), N, D)
        md, od, deep_d, rd, p1d = _run(lib, packed, W, H, N, D, 0)
        mr, orr, deep_r, rr, p1r = _run(lib, packed, W, H, N, D, 1)
        assert md == len(ref) and mr == len(ref), msg
        _same(od, ref, msg + " direct")
        _same(orr, ref, msg + " rounds")
        assert deep_d == deep_r, msg  # both hand over to the label passes on the same inputs
        assert p1d == 0 and p1r >= 1, msg
        if not deep_d:
            assert rd == rr - p1r, msg  # the same final-phase rounds
        if seen is not None:
            seen.add((deep_d, rd > 0))
    return ref


def _keys(oracle, pts, resp):
    k = np.zeros(len(pts), oracle.KP_DTYPE)
    if len(pts):
        k["x"], k["y"] = np.asarray(pts).T
    k["response"] = resp
    k["size"], k["angle"], k["class_id"] = 7, -1, -1
    return k


def test_key_order_closed_form(direct):
    """oct_key_path inverts the push_front recurrence at every depth and initial-node count."""
    for nIni in (1, 2, 3):
        for d in range(0, 6):
            n = nIni << (2 * d)
            keys = [direct.octd_key_of_path(d, idx, nIni) for idx in range(n)]
            assert sorted(keys) == list(range(n))
            assert all(direct.octd_path_of_key(d, k, nIni) == idx for idx, k in enumerate(keys))


@pytest.mark.parametrize("frame", [0, 3])
def test_frame_all_levels(direct, oracle, frame):
    img = synth.stereo_pair(480, 640, frame)[frame % 2]
    seen = set()
    for li, lvl in enumerate(oracle.pyramid(img)):
        h, w = lvl.shape
        oc = oracle.level_candidates(lvl, 20, 7)
        _check(direct, oracle, oc, w - 32, h - 32, oracle.features_per_level(2000)[li], seen=seen)
    # handed over and not, with and without final-phase rounds after the direct build
    assert {s[0] for s in seen} == {0, 1} and (0, True) in seen


@pytest.mark.parametrize("W,H", SHAPES)
def test_random_key_sets(direct, oracle, W, H):
    rng = np.random.default_rng(W)
    for N in CAPS_N:
        for n in (0, 1, 2, N - 1, N, N + 1, 10 * N):
            x, y = rng.integers(0, W, n), rng.integers(0, H, n)
            keys = _keys(oracle, np.stack([x, y], 1), rng.integers(0, 256, n) if n & 1 else rng.integers(20, 23, n))
            _check(direct, oracle, keys, W, H, N)


def test_corner_cluster_hands_over(direct, oracle):
    """All keys in one small corner.  Alone they end after one round (one child: size == prevSize);
    with one lone key in the opposite quadrant at each of six depths the list grows by one node
    per round, so shallow pyramids take the kOctDeep fallback, and still agree."""
    rng = np.random.default_rng(5)
    for W, H in SHAPES:
        pts = sorted({(int(a), int(b)) for a, b in rng.integers(0, 8, (150, 2))})
        keys = _keys(oracle, pts, rng.integers(0, 60, len(pts)))
        for N in (5, 50, 434):
            assert len(_check(direct, oracle, keys, W, H, N)) == 1
        x1, y1 = int(np.float32(W) / np.float32(round(W / H))), H
        for _ in range(6):  # the seam corner of the corner node: its n4 child
            x1, y1 = (x1 + 1) // 2, (y1 + 1) // 2
            pts.append((x1, y1))
        keys = _keys(oracle, pts, rng.integers(0, 60, len(pts)))
        seen = set()
        for N in (5, 50, 434):
            _check(direct, oracle, keys, W, H, N, seen=seen)
        assert {s[0] for s in seen} == {0, 1}


def test_one_pixel_never_splits(direct, oracle):
    """Many keys on one pixel: every division has one child, the list ends on size == prevSize."""
    for W, H in SHAPES:
        for pts in ([(37, 41)] * 50, [(37, 41)] * 30 + [(W - 9, H - 7)] * 30):
            keys = _keys(oracle, pts, np.arange(len(pts)) % 7 + 20)
            ref = _check(direct, oracle, keys, W, H, 10)
            assert len(ref) == len(set(pts))


def test_every_key_alone(direct, oracle):
    """One key per quadrant: nothing left to divide, the next round changes nothing."""
    W, H = 608, 448
    keys = _keys(oracle, [(10, 10), (400, 10), (10, 300), (400, 300)], [30, 31, 32, 33])
    ref = _check(direct, oracle, keys, W, H, 50)
    assert len(ref) == 4
    m, _, deep, r, p1 = _run(direct, _pack(keys), W, H, 50, 5, 0)
    assert (m, deep, r, p1) == (4, 0, 0, 0)


def _lattice(W, H, cells):
    """Two keys in each named cell (cx, cy) of the depth-2 grid of a 608 x 448 level."""
    xs, ys = (0, 152, 304, 456), (0, 112, 224, 336)
    return [(xs[cx] + o, ys[cy] + o) for cx, cy in cells for o in (5, 20)]


def test_round_lands_on_N(direct, oracle):
    """16 depth-2 nodes of two keys each, N = 16: round 1 continues (4 + 3 * 4 = 16), round 2 ends on N."""
    W, H = 608, 448
    keys = _keys(oracle, _lattice(W, H, [(a, b) for a in range(4) for b in range(4)]), 25)
    ref = _check(direct, oracle, keys, W, H, 16)
    assert len(ref) == 16
    m, _, deep, r, p1 = _run(direct, _pack(keys), W, H, 16, 5, 1)
    assert (m, deep, r, p1) == (16, 0, 2, 2)


def test_final_phase_after_first_round(direct, oracle):
    W, H = 608, 448
    keys = _keys(oracle, _lattice(W, H, [(a, b) for a in range(4) for b in range(4)]), 25)
    ref = _check(direct, oracle, keys, W, H, 5)
    assert len(ref) >= 5
    m, _, deep, r, p1 = _run(direct, _pack(keys), W, H, 5, 5, 1)
    assert (deep, p1) == (0, 1) and r >= 2  # one phase-1 round, then the final phase
    assert _run(direct, _pack(keys), W, H, 5, 5, 0)[3] == r - 1


def test_small_capacity_gives_minus_3(direct, oracle):
    """Ten depth-2 nodes against a capacity of 12 (8 usable): both forms report -3 in round 2."""
    W, H = 608, 448
    cells = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 1), (1, 2), (3, 2), (0, 3), (3, 3)]
    packed = _pack(_keys(oracle, _lattice(W, H, cells), 25))
    for D in (2, 5):
        for rounds in (0, 1):
            m, _, deep, _, _ = _run(direct, packed, W, H, 50, D, rounds, cap=12)
            assert (m, deep) == (-3, 0), (D, rounds)
    assert _run(direct, packed, W, H, 50, 5, 0)[0] == 10  # the planned capacity holds them
