"""Which kernels launch_fast_cells starts (orbslam3lib_amd/csrc/orb_kernels.h fast_launch_plan), on
the CPU through the host harness: the three tile calls (48, 64, 80) of one batch, against a
transcription of the launcher as it was before the decision became a function, and against what
the decision is for -- every cell detected once in a tile that holds it, one overflow pass after
the last small-list launch, one merged launch for the latency shape.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.test_plan_geometry import GEOMS, _plan

TILES = (48, 64, 80)
MERGE_MAX = 4  # kFastMergeMaxImages
OVF = ("ovf",)  # k_fast_cells_ovf<64>; a k_fast_cells launch is (tile, c0, c1, small)


def _parent_launches(nimages, fast_small, n48, n64, total, has_ovf, tile):
    """launch_fast_cells(a, tile) before fast_launch_plan existed, branch by branch."""
    c0, c1 = {48: (0, n48), 64: (n48, n64), 80: (n64, total)}[tile]
    merge = nimages <= MERGE_MAX and fast_small <= 0 and n48 > 0 and n64 > n48
    if merge and tile == 64:
        return []
    if merge and tile == 48:
        tile, c1 = 64, n64
    if c1 <= c0:
        return []
    small = tile in (48, 64) and bool(has_ovf) and (fast_small > 0 or (fast_small < 0 and nimages > MERGE_MAX))
    if small and tile == 48:
        return [(48, c0, c1, True)] + ([OVF] if n64 <= n48 else [])
    if small:
        return [(64, c0, c1, True), OVF]
    return [(tile, c0, c1, False)]


def _planned_launches(harness, case, tile):
    out = (C.c_int32 * 6)(*[-1] * 6)
    harness.harness_fast_launch_plan(*case, tile, out)
    ptile, c0, c1, small, ovf, pad = list(out)
    assert small in (0, 1) and ovf in (0, 1) and pad == 0
    if ptile == 0:
        assert (c0, c1, small, ovf) == (0, 0, 0, 0)
        return []
    return [(ptile, c0, c1, bool(small))] + ([OVF] if ovf else [])


@pytest.fixture(scope="module")
def trios(harness):
    """(nimages, fast_small, n48, n64, total, has_ovf) -> the launches of its 48, 64 and 80 call."""
    harness.harness_fast_launch_plan.restype = None
    harness.harness_fast_launch_plan.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int32)]
    shapes = [(a, b, c) for a, b, c in itertools.product((0, 3, 10), repeat=3) if a <= b <= c]
    for g in GEOMS:
        r, p = _plan(harness, *g)
        assert r == 0, (g, p)
        shapes.append((p.sc["fast_n48"], p.sc["fast_n64"], p.sc["total_cells"]))
    assert len(shapes) == 10 + len(GEOMS) and all(0 <= a <= b <= c for a, b, c in shapes)
    out = {}
    for nimages, fast_small, has_ovf, (n48, n64, total) in itertools.product((1, 4, 5, 256), (-1, 0, 1), (0, 1), shapes):
        case = (nimages, fast_small, n48, n64, total, has_ovf)
        out[case] = [_planned_launches(harness, case, t) for t in TILES]
    return out


def test_same_launches_as_the_parent(trios):
    for case, got in trios.items():
        assert got == [_parent_launches(*case, t) for t in TILES], case


def test_every_cell_once_in_a_tile_that_holds_it(trios):
    for case, got in trios.items():
        _, _, n48, n64, total, _ = case
        times = np.zeros(total, np.int64)
        width = np.zeros(total, np.int64)
        for tile, c0, c1, _ in (k for call in got for k in call if k != OVF):
            assert tile in TILES and 0 <= c0 < c1 <= total, case
            times[c0:c1] += 1
            width[c0:c1] = tile
        assert (times == 1).all(), case
        tier = np.array(TILES)[np.searchsorted([n48, n64], np.arange(total), side="right")]
        assert (width >= tier).all(), case


def test_one_overflow_pass_after_the_last_small_list_launch(trios):
    seen_small = 0
    for case, got in trios.items():
        seq = [k for call in got for k in call]
        small_at = [i for i, k in enumerate(seq) if k != OVF and k[3]]
        ovf_at = [i for i, k in enumerate(seq) if k == OVF]
        if small_at:
            assert case[5] == 1, case  # the queue is bound
            assert ovf_at == [small_at[-1] + 1], case
            seen_small += 1
        else:
            assert not ovf_at, case
    assert seen_small > 0


def test_latency_shape_merges_the_lower_tiers(trios):
    merged = 0
    for case, got in trios.items():
        nimages, fast_small, n48, n64, _, _ = case
        if not (nimages <= MERGE_MAX and fast_small <= 0 and n48 > 0 and n64 > n48):
            continue
        below = [k for call in got for k in call if k != OVF and k[1] < n64]
        assert len(below) == 1 and below[0][1:3] == (0, n64) and not below[0][3], case
        merged += 1
    assert merged > 0
