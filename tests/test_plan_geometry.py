"""The geometry planner (orbslam3lib_amd/csrc/orb_geometry.h plan_geometry) on the CPU, through
the host harness: the level, cell, octree, resize and FAST-tier tables and every per-image buffer
offset of the runtime, against the oracle (never against the planner itself), plus the layout
invariants whose violation was round 6's octree workspace overrun.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

INVALID = -3  # ORBGPU_ERR_INVALID (include/orbgpu.h)

# w, h, nlevels, scale factor, nfeatures: the smallest legal size (one 35-px cell), the workloads'
# own sizes, 1080p levels whose oct_cap exceeds kOctLdsNodes (5000 and 8200 features), exact 2x
# steps (area2 on every level) and steps above 2 (generic_pyr, no tail)
GEOMS = [
    (67, 67, 1, 1.2, 2000),
    (640, 480, 8, 1.2, 2000), (640, 400, 8, 1.2, 2000), (641, 401, 8, 1.2, 2000), (752, 480, 8, 1.2, 2000),
    (1920, 1080, 12, 1.2, 5000), (1920, 1080, 12, 1.2, 8200),
    (640, 480, 3, 2.0, 2000), (640, 480, 3, 2.5, 2000), (640, 480, 2, 3.0, 2000),
]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_parent.json")


class Plan:
    def __init__(self, lv, sc, rtab):
        self.lv, self.sc, self.rtab = lv, sc, rtab  # per-level dicts, scalar dict, int32 [n, 4]

    def ints(self, off, n):
        """n ints of the table's int view starting at int offset off (band / quad tables)."""
        return self.rtab.reshape(-1)[off:off + n]


def _plan(harness, w, h, L, sf, nf, max_images=2):
    harness.harness_plan_level_fields.restype = C.c_char_p
    harness.harness_plan_scalars.restype = C.c_char_p
    lnames = harness.harness_plan_level_fields().decode().split(",")
    snames = harness.harness_plan_scalars().decode().split(",")
    lv = np.zeros((16, len(lnames)), np.int64)
    sc = np.zeros(len(snames), np.int64)
    cap = 1 << 18
    rtab = np.zeros((cap, 4), np.int32)
    n = C.c_int(0)
    err = C.create_string_buffer(256)
    r = harness.harness_plan_geometry(w, h, L, C.c_float(sf), nf, max_images, lv.ctypes.data_as(C.c_void_p),
                                      sc.ctypes.data_as(C.c_void_p), rtab.ctypes.data_as(C.c_void_p), cap,
                                      C.byref(n), err, 256)
    if r:
        return r, err.value.decode()
    assert n.value <= cap
    levels = [dict(zip(lnames, row.tolist())) for row in lv[:L]]
    return 0, Plan(levels, dict(zip(snames, sc.tolist())), rtab[:n.value].copy())


@pytest.fixture(scope="module")
def plans(harness):
    out = {}
    for g in GEOMS:
        r, p = _plan(harness, *g)
        assert r == 0, (g, p)
        out[g] = p
    return out


def test_must_fail_cases(harness):
    r, msg = _plan(harness, 66, 67, 1, 1.2, 2000)
    assert r == INVALID and "has no cells" in msg
    # a third level of 40 x 40 (under 2 * 19 + 4 px) after an 80 x 80 one that still has a cell
    r, msg = _plan(harness, 160, 160, 3, 2.0, 2000)
    assert r == INVALID and "level 2 too small" in msg
    assert _plan(harness, 160, 160, 2, 2.0, 2000)[0] == 0


@pytest.mark.parametrize("g", GEOMS)
def test_tables_match_oracle(oracle, plans, g):
    w, h, L, sf, nf = g
    p = plans[g]
    assert [(v["w"], v["h"]) for v in p.lv] == oracle.level_sizes(w, h, sf, L)
    assert [v["N"] for v in p.lv] == oracle.features_per_level(nf, sf, L)
    scale = oracle.scale_factors(sf, L)[0]
    assert [v["scale_bits"] for v in p.lv] == scale.view(np.uint32).tolist()
    for v in p.lv[1:]:
        assert v["simd_end"] == oracle.resize_simd_end(v["w"])
    assert p.sc["generic_pyr"] == (1 if sf > 2.0 else 0)
    if sf == 2.0:
        assert all(v["area2"] == 1 for v in p.lv[1:])


def test_unchanged_against_parent(plans):
    """out_cap (orbgpu_export_batch_bytes(ctx, 1, 0)) and the level sizes (orbgpu_get_pyramid_level)
    read through the C ABI on an MI355X at the commit before the planner was split out."""
    golden = json.load(open(GOLDEN))
    assert len(golden) == len(GEOMS)
    for rec in golden:
        g = (rec["width"], rec["height"], rec["nlevels"], rec["scale_factor"], rec["nfeatures"])
        p = plans[g]
        assert p.sc["plan_out_cap"] == p.sc["out_cap"] == rec["out_cap"]
        assert 8 + 60 * p.sc["out_cap"] == rec["export_batch_bytes_1_0"]
        assert [[v["w"], v["h"]] for v in p.lv] == rec["level_sizes"]


def _resize_with_tables(src, xt, yt, simd_end):
    """cv::resize INTER_LINEAR (8-bit, fixed point) from coefficient tables, the two roundings of
    oracle/orb_oracle.cpp resize_linear: with D = S[sx] * a0 + S[sx1] * a1 per source row,
      columns below simd_end (OpenCV's vector path):
        t = min(D >> 4, 32767) as int16; s = clamp(((t0 * b0) >> 16) + ((t1 * b1) >> 16), int16);
        out = sat_u8((s + 2) >> 2)
      the remaining columns (scalar path): out = sat_u8((D0 * b0 + D1 * b1 + (1 << 21)) >> 22)."""
    S = src.astype(np.int64)
    sx, sx1, a0, a1 = (xt[:, k].astype(np.int64) for k in range(4))
    sy0, sy1, b0, b1 = (yt[:, k].astype(np.int64)[:, None] for k in range(4))
    D = S[:, sx] * a0 + S[:, sx1] * a1  # [sh, dw]
    D0, D1 = D[sy0[:, 0]], D[sy1[:, 0]]
    t0, t1 = np.minimum(D0 >> 4, 32767), np.minimum(D1 >> 4, 32767)
    vec = np.clip(((t0 * b0) >> 16) + ((t1 * b1) >> 16), -32768, 32767)
    vec = np.clip((vec + 2) >> 2, 0, 255)
    sca = np.clip((D0 * b0 + D1 * b1 + (1 << 21)) >> 22, 0, 255)
    col = np.arange(xt.shape[0])[None, :]
    return np.where(col < simd_end, vec, sca).astype(np.uint8)


def test_resize_tables_reproduce_oracle_resize(oracle, plans):
    rng = np.random.default_rng(7)
    seen = set()
    for g, p in plans.items():
        for l in range(1, len(p.lv)):
            S, G = p.lv[l - 1], p.lv[l]
            key = (S["w"], S["h"], G["w"], G["h"])
            if G["area2"] or key in seen:
                continue
            seen.add(key)
            src = rng.integers(0, 256, (S["h"], S["w"]), dtype=np.uint8)
            xt = p.rtab[G["xtab_off"]:G["xtab_off"] + G["w"]]
            yt = p.rtab[G["ytab_off"]:G["ytab_off"] + G["h"]]
            got = _resize_with_tables(src, xt, yt, G["simd_end"])
            np.testing.assert_array_equal(got, oracle.resize(src, G["w"], G["h"]), err_msg="%s level %d" % (g, l))
    assert len(seen) >= 30


@pytest.mark.parametrize("g", GEOMS)
def test_cell_records(oracle, plans, g):
    """k_fast_cells' per-cell records: every cell of every level exactly once, in the tier whose
    tile its ROI fits (wCell + 9 and hCell + 6 bytes within 48, else 64, else 80), rows / cols /
    skip as the reference cell loop clips them (ORBextractor_old.cc:787-821, float32 arithmetic)."""
    w, h, L, sf, nf = g
    p = plans[g]
    sizes = oracle.level_sizes(w, h, sf, L)
    f32 = np.float32
    total = p.sc["total_cells"]
    rec = p.rtab[p.sc["fast_tab_off"]:p.sc["fast_tab_off"] + 2 * total].reshape(total, 2, 4)
    assert p.sc["od_tab_off"] == p.sc["fast_tab_off"] + 2 * total
    tier_of = np.searchsorted([p.sc["fast_n48"], p.sc["fast_n64"]], np.arange(total), side="right")
    seen = {}
    for k in range(total):
        (l, iniX, iniY, rc), (cnt_idx, key_idx, skip, zero) = rec[k].tolist()
        assert zero == 0
        seen.setdefault(l, []).append((iniY, iniX, rc & 0xFFFF, rc >> 16, skip, cnt_idx, key_idx, int(tier_of[k])))
    assert sorted(seen) == list(range(L))
    for l, (lw, lh) in enumerate(sizes):
        minB, maxBX, maxBY = 16, lw - 19 + 3, lh - 19 + 3
        width, height = f32(maxBX - minB), f32(maxBY - minB)
        nCols, nRows = int(width / f32(35)), int(height / f32(35))
        wCell, hCell = int(np.ceil(width / f32(nCols))), int(np.ceil(height / f32(nRows)))
        v = p.lv[l]
        assert (v["nCols"], v["nRows"], v["wCell"], v["hCell"], v["maxBX"], v["maxBY"]) == \
               (nCols, nRows, wCell, hCell, maxBX, maxBY)
        tier = 0 if wCell + 9 <= 48 and hCell + 6 <= 48 else 1 if wCell + 9 <= 64 and hCell + 6 <= 64 else 2
        want = []
        for i in range(nRows):
            for j in range(nCols):
                iniY, iniX = minB + i * hCell, minB + j * wCell
                skip = int(iniY >= maxBY - 3 or iniX >= maxBX - 6)
                rows = 0 if skip else min(iniY + hCell + 6, maxBY) - iniY
                cols = 0 if skip else min(iniX + wCell + 6, maxBX) - iniX
                cell = i * nCols + j
                want.append((iniY, iniX, rows, cols, skip, v["cellcnt_off"] + cell,
                             v["cellkey_off"] + cell * v["cell_cap"], tier))
        assert seen[l] == want, "level %d" % l


def _disjoint_inside(regions, stride, what):
    regions = sorted(regions)
    for (a0, a1), (b0, b1) in zip(regions, regions[1:]):
        assert a1 <= b0, what
    assert regions[0][0] >= 0 and regions[-1][1] <= stride, what


@pytest.mark.parametrize("g", GEOMS)
def test_layout_invariants(plans, g):
    p = plans[g]
    lv, sc = p.lv, p.sc
    L = len(lv)
    _disjoint_inside([(v["pyr_off"], v["pyr_off"] + v["pitch"] * v["h"]) for v in lv[1:]] or [(0, 0)],
                     sc["pyr_img"], "pyramid")
    _disjoint_inside([(v["blur_off"], v["blur_off"] + v["bpitch"] * v["h"]) for v in lv], sc["blur_img"], "blur")
    _disjoint_inside([(v["cellkey_off"], v["cellkey_off"] + v["cand_cap"]) for v in lv], sc["cellkeys_img"],
                     "cell keys")
    _disjoint_inside([(v["cellcnt_off"], v["cellcnt_off"] + v["ncells"]) for v in lv], sc["cellcnt_img"],
                     "cell counts")
    _disjoint_inside([(v["kp_off"], v["kp_off"] + v["kp_cap"]) for v in lv], sc["lvlkp_img"], "level keypoints")
    _disjoint_inside([(v["oct_off"], v["oct_off"] + v["oct_total"]) for v in lv], sc["octws_img"],
                     "octree workspace")
    for name in ("pyr_img", "blur_img"):
        assert sc[name] % 256 == 0
    assert (sc["cellkeys_img_stride"], sc["cellcnt_img_stride"], sc["octws_img_stride"], sc["lvlkp_img_stride"]) == \
           (sc["cellkeys_img"], sc["cellcnt_img"], sc["octws_img"], sc["lvlkp_img"])
    for l, v in enumerate(lv):
        assert v["pitch"] >= v["w"] and v["bpitch"] >= v["w"]
        assert v["img_stride"] == (v["w"] * v["h"] if l == 0 else sc["pyr_img"])
        assert v["bimg_stride"] == sc["blur_img"]
        # the round-6 overrun: the workspace's node part holds what the carve takes
        assert v["oct_total"] - v["oct_nodemem"] >= v["oct_nodemem_need"]
        assert v["cell_cap"] % 4 == 0
        assert v["cand_cap"] == v["ncells"] * v["cell_cap"]
    assert sc["out_cap"] == sum((v["kp_cap"] + 15) // 16 * 16 for v in lv)
    if g[4] == 8200:  # the case that overran: node state in the workspace (5000 features: 949 nodes, in LDS)
        assert any(v["oct_cap"] > sc["kOctLdsNodes"] for v in lv)
    # band / quad ownership of k_blur_resize
    for l in range(1, L):
        S, G = lv[l - 1], lv[l]
        nquads = (G["w"] + 3) // 4
        band = p.ints(G["band_row_off"], S["tiles_y"] + 1)
        tq = p.ints(G["tile_quad_off"], S["tiles_x"] + 1)
        assert (S["tiles_x"], S["tiles_y"]) == (-(-S["w"] // sc["kBlurTW"]), -(-S["h"] // sc["kBlurTH"]))
        assert band[0] == 0 and band[-1] == G["h"] and np.all(np.diff(band) >= 0)
        assert tq[0] == 0 and tq[-1] == nquads and np.all(np.diff(tq) >= 0)
        assert np.diff(band).max() <= sc["kBrMaxRows"] and np.diff(tq).max() <= sc["kBrMaxQuads"]
    if sc["tail0"] <= L:
        assert not sc["generic_pyr"] and 2 <= sc["tail0"]
        assert 0 < sc["tail_lds"] <= sc["kTailLdsMax"]
    else:
        assert sc["tail0"] == L + 1
    if sc["generic_pyr"]:
        assert sc["tail0"] == L + 1
    assert sc["oct_lds_bytes"] <= 160 * 1024 and sc["oct2_lds_bytes"] <= 160 * 1024
    # the k_orient_desc block records follow the FAST records to the table's end
    assert sc["rtab_n"] == sc["od_tab_off"] + sc["total_od_blocks"]
    od = p.rtab[sc["od_tab_off"]:]
    want = [(l, b, 0, 0) for l, v in enumerate(lv) for b in range(v["od_blocks"])]
    assert [tuple(r) for r in od.tolist()] == want
