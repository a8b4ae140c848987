"""ORBmatcher::SearchByProjection on the directed map-point sets of tests/sbp_maps.py.

CPU: the coded oracle (decision code, flags and replay ranks per map point and window) against the
Python restatement of tests/test_projection.py on every set and mode; the reach table
(sbp_maps.MINIMA) and the per-point expectations of the builders; restatement mutants, one per
boundary, that must each disagree with the oracle somewhere on the sets.
GPU: k_sbp_candidates + k_sbp_resolve on every set, in the three modes and both map-point forms,
bit-exact on matches and nmatches against the oracle.

The ranks the oracle reports are reference semantics.  What they mean for the kernels is said here,
with the kernels' constants (orbslam3lib_amd/csrc/orb_sbp.hip):"""
import collections
import functools

import numpy as np
import pytest

from tests import sbp_maps as SM
from tests.test_projection import MUTANTS, _py_sbp_coded

K_TOP = 4            # kTop: slots of a candidate list (k_sbp_candidates)
K_GROUP = 64         # lanes of k_sbp_resolve: map points replayed at once
K_CHUNK = 128        # kResolveChunk: candidate records staged in LDS at a time


def _args(s, mode, slot):
    fr = SM.frame_of(s, slot)
    blk = None if s.blk is None else s.blk[slot]
    return fr, s.mps[slot], blk


def _modes(s):
    return [m for m in SM.MODES if m != "two" or not s.dist]


def _oracle(oracle, s, mode, slot, coded=True):
    fr, mps, blk = _args(s, mode, slot)
    kw = dict(th=s.th, nnratio=s.nnratio, far_points=s.far, th_far=s.th_far, nlevels=fr.nlevels)
    if mode == "two":
        f = oracle.search_by_projection2_coded if coded else oracle.search_by_projection2
        return f(mps, fr.L, fr.R, fr.bounds, None if s.l2r is None else s.l2r[slot],
                 None if s.r2l is None else s.r2l[slot], blk, **kw)
    f = oracle.search_by_projection_coded if coded else oracle.search_by_projection
    xy, octv, desc, cs, ci = fr.L
    return f(mps, xy, octv, desc, fr.uright if mode == "pinur" else None, fr.bounds, cs, ci,
             None if blk is None else blk[:len(octv)], **kw)


def _restatement(s, mode, slot, mut=frozenset()):
    fr, mps, blk = _args(s, mode, slot)
    two = mode == "two"
    return _py_sbp_coded(mps, fr.L, fr.R if two else None, fr.bounds, fr.uright if mode == "pinur" else None,
                         s.l2r[slot] if two and s.l2r is not None else None,
                         s.r2l[slot] if two and s.r2l is not None else None, blk, s.th, s.nnratio, s.far, s.th_far,
                         fr.scale, fr.nlevels, mut)


@functools.lru_cache(maxsize=None)
def _coded(name, mode, slot):
    """The coded oracle's answer, computed once and shared (read-only) by every test here."""
    from oracle import oracle_py
    s = {st.name: st for st in SM.sets()}[name]
    m, nm, recs = _oracle(oracle_py, s, mode, slot)
    m.setflags(write=False)
    recs.setflags(write=False)
    return m, nm, recs


def _cases():
    for s in SM.sets():
        for mode in _modes(s):
            for slot in range(len(s.mps)):
                if len(s.mps[slot]):
                    yield s, mode, slot


def reach():
    """What the sets reach, from the oracle's records: codes per window, flags, and the replay
    events -- the reference's ranks read with the kernels' constants."""
    from oracle import oracle_py as O
    ev = collections.Counter()
    for s, mode, slot in _cases():
        _, _, recs = _coded(s.name, mode, slot)
        for w, side in enumerate(("left", "right")):
            r = recs[:, w]
            for c, n in zip(*np.unique(r["code"], return_counts=True)):
                if c != O.SBP_NO_WINDOW:
                    ev["%s.%s" % (side, O.SBP_CODE_NAMES[c])] += int(n)
            for bit, name in enumerate(O.SBP_FLAG_NAMES):
                ev["flag." + name] += int(((r["flags"] >> bit) & 1).sum())
            walked = r["code"] >= O.SBP_ALL_TAKEN
            live_in_list = (r["rank_best"] < K_TOP).astype(int) + (r["rank_second"] < K_TOP)
            dry = walked & (r["ncand"] > K_TOP) & (live_in_list < 2)
            ev["replay.dry_" + side] += int(dry.sum())
            ev["replay.dry_%s_exactly_%d" % (side, K_TOP + 1)] += int((dry & (r["ncand"] == K_TOP + 1)).sum())
            ev["replay.list_short_" + side] += int((walked & (r["ncand"] <= K_TOP) & (r["ncand"] > 0)).sum())
        # points that skipped a keypoint taken in this call while an earlier point of their own
        # 64-group assigned something (an upper bound on the points disturbed inside their group;
        # the directed ones are the built.*_same_group, built.chain and built.right_owner rows)
        taken = (recs["flags"] & O.SBPF_TAKEN_SKIP).any(1)
        assigned = recs["assigned"].reshape(len(recs), 4)
        for i in np.flatnonzero(taken):
            g0 = i - i % K_GROUP
            if (assigned[g0:i] >= 0).any():
                ev["replay.taken_skip_in_assigning_group"] += 1
        for name, bit in (("incall_free", O.SBPF_FREED_INCALL), ("precall_free", O.SBPF_FREED_PRECALL),
                          ("own_partner", O.SBPF_OWN_PARTNER), ("double_assign", O.SBPF_DOUBLE_ASSIGN)):
            ev["replay." + name] += int((recs["flags"] & bit).any(1).sum())
        for tag, wants in s.expect.items():
            ev["built." + tag] += sum(1 for w in wants if w[0] == mode)
        for tag, n in s.found.items():
            if mode == "pin":
                ev["found." + tag] += n
        n = len(recs)
        ev["points.frames_of_%d" % n] += 1 if s.name.startswith("counts") else 0
    return ev


def test_coded_oracle_matches_restatement_and_plain_entry_points(oracle):
    """Codes, flags, ranks, assigned keypoints, matches and nmatches on every set and mode; the plain
    entry points give the coded ones' matches byte for byte."""
    for s, mode, slot in _cases():
        m, nm, recs = _coded(s.name, mode, slot)
        pm, pnm, precs = _restatement(s, mode, slot)
        where = "%s %s frame %d" % (s.name, mode, slot)
        for field in recs.dtype.names:
            bad = np.flatnonzero((recs[field] != precs[field]).reshape(len(recs), -1).any(1))
            assert len(bad) == 0, (where, field, bad[:5], recs[bad[:5]], precs[bad[:5]])
        np.testing.assert_array_equal(m, pm, err_msg=where)
        assert nm == pnm, where
        m0, nm0 = _oracle(oracle, s, mode, slot, coded=False)
        assert m0.tobytes() == m.tobytes() and nm0 == nm, where


def test_maps_exercise_every_path(oracle):
    """The reach table: every code, flag and replay event at least MINIMA times; every point a
    builder aimed shows what it was aimed at; the frees of pre-call occupants sit where the three
    replay sets say."""
    from oracle import oracle_py as O
    for s, mode, slot in _cases():
        if slot:
            continue
        _, _, recs = _coded(s.name, mode, slot)
        for tag, wants in s.expect.items():
            for m, idx, win, fields in wants:
                if m != mode:
                    continue
                r = recs[idx, win]
                for key, val in fields.items():
                    if key == "flags":
                        ok = (r["flags"] & val) == val
                    elif key == "not_flags":
                        ok = (r["flags"] & val) == 0
                    elif key == "ncand_min":
                        ok = r["ncand"] >= val
                    else:
                        ok = np.array_equal(r[key], val)
                    assert ok, (s.name, mode, tag, idx, win, key, val, r)
        if mode == "two" and s.name.startswith("replay"):
            frees = np.flatnonzero((recs["flags"] & O.SBPF_FREED_PRECALL).any(1))
            if "absent" in s.name:
                assert len(frees) == 0
            elif "first" in s.name:
                assert frees[0] == 0
            else:
                assert frees[0] >= 0.9 * len(recs) and len(frees) >= 2
    ev = reach()
    short = {k: (ev[k], v) for k, v in SM.MINIMA.items() if ev[k] < v}
    assert not short, short
    # no live event goes unasserted, and none is asserted at zero
    assert all(v > 0 for v in SM.MINIMA.values())
    unlisted = sorted(k for k, v in ev.items() if v > 0 and k not in SM.MINIMA and not k.startswith("points."))
    assert not unlisted, unlisted
    for k in SM.UNREACHABLE:
        assert ev[k] == 0, k


def test_count_batch_covers_group_and_chunk_sizes():
    s = {st.name: st for st in SM.sets()}["counts_320"]
    n = [len(m) for m in s.mps]
    assert n[:9] == list(SM.COUNTS) and n[9] > 0 and len(SM.frame_of(s, 9).L[1]) == 0
    assert {0, 1, K_GROUP - 1, K_GROUP, K_GROUP + 1, K_CHUNK - 1, K_CHUNK, K_CHUNK + 1, 2 * K_CHUNK + 1} <= set(n)
    assert 0 in n[1:8]  # an empty frame between full ones


@pytest.mark.parametrize("mut", MUTANTS)
def test_restatement_mutants_disagree_with_oracle(oracle, mut):
    """Teeth: each boundary of the search got wrong on purpose in the restatement (`<` for `<=`, 99
    for 100, a float compare against 0.998, trunc for floor, ...) must change a match, a count, a
    code, a flag or a rank somewhere on the sets."""
    where = MUTANT_SETS[mut]
    hits = 0
    for s, mode, slot in _cases():
        if slot or not s.name.startswith(where):
            continue
        m, nm, recs = _coded(s.name, mode, slot)
        pm, pnm, precs = _restatement(s, mode, slot, {mut})
        hits += int(not np.array_equal(m, pm)) + int(nm != pnm) + int(recs.tobytes() != precs.tobytes())
    assert hits > 0, mut


# the sets built for each mutant's boundary (a prefix of the set names)
MUTANT_SETS = {
    "far_ge": "gates", "cos_float": "gates", "level_lo_le": "gates", "level_hi_m1": "gates",
    "level_r_lo_le": "gates", "level_r_hi_m1": "gates",
    "floor_trunc": "grid", "ceil_trunc": "grid", "exit_minx_gt": "grid", "exit_maxx_le": "grid",
    "exit_miny_gt": "grid", "exit_maxy_le": "grid",
    "edge_x_le": "edges", "edge_y_le": "edges", "uright_ge": "edges",
    "octave_lo_le": "desc", "octave_hi_ge": "desc", "best_le": "desc", "th_high_99": "desc", "ratio_ge": "desc",
    "second_le": "tie2",
}


# ---- GPU ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _context(ctx, dist):
    """One device context per frame size, its frames extracted, undistorted and stereo-matched;
    checked against the CPU-extracted frames the sets were built on."""
    import orbslam3lib_amd as og
    c = SM.CONTEXTS[ctx]
    fs = SM.frames()
    imgs = [im for name in c["frames"] for im in fs[name].images]
    be = og.BatchExtractor(c["nfeatures"], 1.2, c["nlevels"], 20, 7, width=c["width"], height=c["height"],
                           max_images=len(imgs))
    be.upload(np.stack(imgs))
    be.run()
    be.stereo_matches(SM.MBF, SM.MB)
    be.undistort_grid(SM.K_, SM.D_ if dist else ())
    be.synchronize()
    for slot, name in enumerate(c["frames"]):
        fr = fs[name + "d" if dist else name]
        for eye in (0, 1):
            kps, desc, _ = be.result(2 * slot + eye)
            side = (fr.L, fs[name].R)[eye]
            assert np.array_equal(kps["octave"], side[1]) and np.array_equal(desc, side[2]), (name, eye)
            if eye == 0 or not dist:
                assert np.array_equal(be.grid_result(2 * slot + eye)[0], side[0]), (name, eye)
        if len(fr.uright):
            assert np.array_equal(be.stereo_result(slot)[0], fr.uright), name
    return be


def _gpu_run(be, s, mode, form):
    mps = s.mps if form == "list" else (np.concatenate(s.mps),
                                        np.concatenate([[0], np.cumsum([len(m) for m in s.mps])]).astype(np.int32))
    kw = dict(th=s.th, nnratio=s.nnratio, far_points=s.far, th_far=s.th_far)
    if mode == "two":
        be.search_by_projection_stereo(mps, s.l2r, s.r2l, s.blk, **kw)
    else:
        blk = None
        if s.blk is not None:
            blk = [b[:len(SM.frame_of(s, i).L[1])] for i, b in enumerate(s.blk)]
        be.search_by_projection(mps, image_step=2, use_uright=mode == "pinur", kp_block=blk, **kw)
    be.synchronize()
    return [be.projection_matches(slot) for slot in range(len(s.mps))]


def _gpu_check(s, mode, got):
    for slot, (gm, gnm) in enumerate(got):
        fr = SM.frame_of(s, slot)
        n = len(fr.L[1]) + (len(fr.R[1]) if mode == "two" else 0)
        if len(s.mps[slot]):
            m, nm, _ = _coded(s.name, mode, slot)
        else:
            m, nm = np.full(n, -1, np.int32), 0
        where = "%s %s frame %d" % (s.name, mode, slot)
        bad = np.flatnonzero(gm != m) if len(gm) == len(m) else None
        assert bad is not None and len(bad) == 0, (where, len(gm), len(m), None if bad is None else
                                                   [(int(k), int(gm[k]), int(m[k])) for k in bad[:8]])
        assert gnm == nm, (where, gnm, nm)


# the two-camera form searches the raw keypoints, so the distorted context has no such mode
GPU_GROUPS = [(ctx, dist, mode) for ctx, dist in (("640", False), ("640", True), ("320", False))
              for mode in SM.MODES if not (dist and mode == "two")]


@pytest.mark.gpu
@pytest.mark.parametrize("ctx,dist,mode", GPU_GROUPS)
def test_gpu_sbp_directed_sets_bit_exact(oracle, ctx, dist, mode):
    """Every set of one context in one mode, as a list of per-frame arrays and as points + offsets."""
    be = _context(ctx, dist)
    failed = []  # every set is run, so a failure names all the sets that see it
    for s in SM.sets():
        if (s.ctx, s.dist) != (ctx, dist):
            continue
        for form in ("list", "offsets"):
            try:
                _gpu_check(s, mode, _gpu_run(be, s, mode, form))
            except AssertionError as e:
                failed.append((s.name, form, str(e)[:300]))
    assert not failed, (sorted(set(f[0] for f in failed)), failed[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", SM.MODES)
def test_gpu_sbp_context_reused_with_fewer_points(oracle, mode):
    """A call with many points per frame, then one with fewer on the same context: nothing of the
    first call's candidate records, matches or occupancy survives into the second."""
    be = _context("320", False)
    by_name = {s.name: s for s in SM.sets()}
    big, small = by_name["replay_late_c320"], by_name["counts_320"]
    assert len(big.mps[0]) > 4 * len(small.mps[0])
    _gpu_check(big, mode, _gpu_run(be, big, mode, "list"))
    _gpu_check(small, mode, _gpu_run(be, small, mode, "list"))
    _gpu_check(small, mode, _gpu_run(be, small, mode, "offsets"))
