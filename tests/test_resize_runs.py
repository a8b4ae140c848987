"""The resize loops' work split and tables on the CPU (no GPU): orb_kernels.h resize_run /
resize_row_carried -- thread -> (output quad, run of consecutive owned rows), and whether a row's
first source row is the one the previous row left behind -- and the finished resize records
orb_geometry.h writes for rs_hsum / rs_vert, through tests/cpp/resize_run_harness.cpp.

For every k_blur_resize tile (256 threads, the tile's owned quads and rows) and every whole level as
k_pyr_tail splits it (1024 threads) of the level geometries below:
  * every owned (quad, row) is produced exactly once, by a thread whose run is no longer than
    ceil(rows / slots) (the strided split's longest, so no thread works longer than before);
  * walking a run as the kernels do, the carry is taken exactly when ytab[dy].x == ytab[dy - 1].y
    and dy is not the run's first row;
  * the finished records are the x / y tables converted as the kernels converted them per tile.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resize_run_harness.cpp")
LIB = os.path.join(ROOT, "tests", "cpp", "build", "libresize_run.so")

# w, h, nlevels, scale factor: the workloads' sizes, 1080p with 12 levels, and the small sizes of
# tests/test_pyramid_row_carry.py (with the scale steps that leave them more than one level)
GEOMS = [
    (640, 480, 8, 1.2), (752, 480, 8, 1.2), (1920, 1080, 12, 1.2),
    (176, 144, 3, 1.2), (257, 97, 3, 1.2), (300, 200, 3, 1.2),
    (300, 200, 3, 1.5), (176, 144, 2, 1.9), (300, 200, 2, 1.9), (300, 200, 2, 2.0),
]


@pytest.fixture(scope="module")
def lib():
    csrc = os.path.join(ROOT, "orbslam3lib_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC",
                               "-ffp-contract=off", "-shared", "-o", LIB, SRC])
    lib = C.CDLL(LIB)
    lib.rr_level_fields.restype = C.c_char_p
    return lib


class Plan:
    def __init__(self, lv, sc, rtab):
        self.lv, self.rtab = lv, rtab
        self.tail0, self.generic, self.max_quads, self.max_rows = sc

    def ints(self, off, n):
        return self.rtab.reshape(-1)[off:off + n]


@pytest.fixture(scope="module")
def plans(lib):
    names = lib.rr_level_fields().decode().split(",")
    out = {}
    for g in GEOMS:
        w, h, L, sf = g
        lv = np.zeros((16, len(names)), np.int32)
        sc = np.zeros(4, np.int32)
        cap = 1 << 18
        rtab = np.zeros((cap, 4), np.int32)
        n = C.c_int32(0)
        r = lib.rr_plan(w, h, L, C.c_float(sf), 2000, lv.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                        rtab.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        assert r == 0 and n.value <= cap, g
        out[g] = Plan([dict(zip(names, row.tolist())) for row in lv[:L]], sc.tolist(), rtab[:n.value].copy())
    return out


def _runs(lib, nq, nrows, nthreads, cache={}):
    key = (nq, nrows, nthreads)
    if key not in cache:
        out = (C.c_int32 * 3)()
        runs = []
        for t in range(nthreads):
            lib.rr_resize_run(t, nq, nrows, nthreads, out)
            runs.append(tuple(out))
        cache[key] = runs
    return cache[key]


def _splits(p):
    """(level, nthreads, nq, first owned row, rows) of every k_blur_resize tile shape and of every level
    as k_pyr_tail splits it."""
    for l in range(1, len(p.lv)):
        S, G = p.lv[l - 1], p.lv[l]
        band = p.ints(G["band_row_off"], S["tiles_y"] + 1)
        tq = p.ints(G["tile_quad_off"], S["tiles_x"] + 1)
        for by in range(S["tiles_y"]):
            for nq in sorted(set(np.diff(tq).tolist())):
                yield l, 256, min(nq, p.max_quads), int(band[by]), min(int(band[by + 1] - band[by]), p.max_rows)
        if (G["w"] + 3) // 4 <= 1024:
            yield l, 1024, (G["w"] + 3) // 4, 0, G["h"]


def test_every_owned_quad_row_once(lib, plans):
    seen = 0
    for g, p in plans.items():
        for l, nthreads, nq, r0, nr in _splits(p):
            if nq <= 0:
                continue  # br_tile returns before the split
            times = np.zeros((max(nr, 1), nq), np.int64)
            slots = max(nthreads // nq, 1)
            longest = -(-nr // slots)
            for q, a, b in _runs(lib, nq, nr, nthreads):
                if a >= b:
                    continue
                assert 0 <= q < nq and 0 <= a and b <= nr and b - a <= longest, (g, l, nq, nr)
                times[a:b, q] += 1
            assert nr == 0 or (times == 1).all(), (g, l, nthreads, nq, nr)
            seen += 1
    assert seen > 100


def test_carry_exactly_when_the_source_row_is_shared(lib, plans):
    hits = misses = 0
    for g, p in plans.items():
        for l, nthreads, nq, r0, nr in _splits(p):
            G = p.lv[l]
            if G["area2"] or p.generic or nq <= 0:
                continue  # the area path and k_level_linear carry nothing
            yt = p.rtab[G["ytab_off"]:G["ytab_off"] + G["h"]]
            yrec = p.rtab[G["yrec_off"]:G["yrec_off"] + G["h"]]
            for a, b in sorted({(a, b) for _, a, b in _runs(lib, nq, nr, nthreads) if a < b}):
                carried = -1
                for rr in range(a, b):
                    dy = r0 + rr
                    got = lib.rr_row_carried(carried, int(yrec[dy, 0]))
                    want = rr > a and yt[dy, 0] == yt[dy - 1, 1]
                    assert got == int(want), (g, l, dy)
                    carried = int(yrec[dy, 1])
                    hits += got
                    misses += 1 - got
    assert hits > 1000 and misses > 1000


def test_finished_records_are_the_tables_converted(plans):
    checked = 0
    for g, p in plans.items():
        for l in range(1, len(p.lv)):
            G = p.lv[l]
            if G["area2"]:
                assert (G["qrec_off"], G["qbase_off"], G["yrec_off"]) == (0, 0, 0)
                continue
            w, h = G["w"], G["h"]
            nquads = (w + 3) // 4
            xt = p.rtab[G["xtab_off"]:G["xtab_off"] + w].astype(np.int64)
            yt = p.rtab[G["ytab_off"]:G["ytab_off"] + h].astype(np.int64)
            cols = np.minimum(4 * np.arange(nquads)[:, None] + np.arange(4)[None, :], w - 1)  # [quad, k]
            base = xt[cols[:, 0], 0]
            sel = (xt[cols, 0] - base[:, None]) | 0x0c00 | ((xt[cols, 1] - base[:, None]) << 16) | 0x0c000000
            cw = (xt[cols, 2] << 4) | (xt[cols, 3] << 20)
            rec = p.rtab[G["qrec_off"]:G["qrec_off"] + 2 * nquads].view(np.uint32).astype(np.int64).reshape(nquads, 2, 4)
            np.testing.assert_array_equal(rec[:, 0], sel & 0xFFFFFFFF, err_msg="%s level %d selectors" % (g, l))
            np.testing.assert_array_equal(rec[:, 1], cw & 0xFFFFFFFF, err_msg="%s level %d coefficients" % (g, l))
            np.testing.assert_array_equal(p.ints(G["qbase_off"], nquads), base)
            yrec = p.rtab[G["yrec_off"]:G["yrec_off"] + h].astype(np.int64)
            np.testing.assert_array_equal(yrec, np.stack([yt[:, 0], yt[:, 1], yt[:, 2] << 8, yt[:, 3] << 8], 1))
            if not p.generic:  # scale steps <= 2: the taps lie in the 8 bytes rs_hsum aligns
                assert ((sel & 0xFF) <= 7).all() and (((sel >> 16) & 0xFF) <= 7).all(), (g, l)
                assert (cw & 0xFFFF).max() <= 32768 and (cw >> 16).max() <= 32768
            checked += 1
    assert checked >= 30
