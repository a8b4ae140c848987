"""Stereo pairs for Frame::ComputeStereoMatches that reach every live branch of the function
(numpy only, seeded, no files).  tests/test_stereo.py runs the coded CPU oracle over them and
asserts the reach table below (test_scenes_exercise_every_rule), then the gfx950 kernels on the
same pairs (test_gpu_stereo_scenes and friends).

A scene is (name, left, right, mbf, mb, nfeatures, scale_factor, nlevels).  The counts in brackets
are left keypoints per decision code / flag of oracle.stereo_matches_coded, measured with the CPU
oracle; MINIMA holds what the test asserts, set well under them."""
import collections
import functools

import numpy as np

from orbslam3lib_amd import synth

Scene = collections.namedtuple("Scene", "name left right mbf mb nfeatures scale_factor nlevels")

MBF = 47.9
MB = float(np.float32(47.9) / np.float32(435.2))  # maxD = 435.2 px: wider than the frame
H, W = 240, 320


def blocks(h, w, block, cols, seed, values=(20, 220)):
    """Random block x block squares of `values`, `cols` block-columns wide, tiled horizontally:
    a texture of horizontal period block * cols."""
    rng = np.random.default_rng(seed)
    rows = -(-h // block)
    strip = np.asarray(values, np.uint8)[rng.integers(0, len(values), (rows, cols))]
    strip = np.kron(strip, np.ones((block, block), np.uint8))[:h]
    return np.ascontiguousarray(np.tile(strip, (1, -(-w // strip.shape[1])))[:, :w])


def _periodic(block, cols, seed):
    left = blocks(H, W, block, cols, seed)
    return left, np.ascontiguousarray(np.roll(left, -1, axis=1))  # 1 px disparity


def _zero_visible():
    """Identical piecewise-constant thirds (SAD 0 at the true shift, disparity exactly 0 or a
    hair below) beside a noisy natural two thirds that keep the median SAD above 0."""
    left, right = (a.copy() for a in synth.stereo_pair(H, W, 0))
    noise = np.random.default_rng(7).integers(-6, 7, right.shape)
    right = np.clip(right.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    third = W // 3
    tex = np.asarray((30, 95, 160, 225), np.uint8)[np.random.default_rng(8).integers(0, 4, (H // 6, -(-third // 6)))]
    tex = np.kron(tex, np.ones((6, 6), np.uint8))[:, :third]
    left[:, :third] = tex
    right[:, :third] = tex
    return left, right


# synth pairs at 160 x 120, 30 features, 4 levels (a fifth level would be too small for one 35-px
# cell, which the extractor refuses): 21, 22, 24, 17 accepted matches.  The seeds are those where
# the median index matters: with k = count / 2 - 1 / k / k + 1 the median rule keeps 18 / 19 / 20
# rows of pair 3 and 17 / 18 / 19 of pair 31 (test_scenes_exercise_every_rule recomputes this).
SPARSE = (3, 31, 30, 13)
ODD_W, ODD_H = 637, 403   # tests/test_geometry.py::test_odd_level0_sizes


@functools.lru_cache(maxsize=None)
def scenes():
    """The named list.  Arrays are shared between callers: treat them as read-only."""
    nat_l, nat_r = synth.stereo_pair(H, W, 0)
    out = []

    def add(name, left, right, mbf=MBF, mb=MB, nfeatures=1000, scale_factor=1.2, nlevels=8):
        for a in (left, right):
            a.setflags(write=False)
        out.append(Scene(name, left, right, mbf, mb, nfeatures, scale_factor, nlevels))

    # codes 4 [44] 5 [238] 8 [6] 12 [633] 14 [80]; octave-gate [927], neighbour-octave [249]
    add("natural12", nat_l, nat_r)
    # maxD = 8 px against a 12 px disparity: codes 4 [702] 5 [253] 11 [40]
    add("narrow8", nat_l, nat_r, mbf=8.0, mb=1.0)
    # the right eye 5 rows lower: the row band of k_stereo_match; codes 5 [616] 8 [31] 12 [279]
    add("vshift5", nat_l, np.ascontiguousarray(np.roll(nat_r, 5, axis=0)))
    # code 2 on every row [1001] / no left keypoints at all (nL == 0)
    add("blank_right", nat_l, np.zeros_like(nat_l))
    add("blank_left", np.zeros_like(nat_r), nat_r)
    # period 4: the SAD minimum repeats inside the 11 shifts (first minimum wins): SAD-tie [2],
    # Hamming-tie [71], codes 2 [8] 8 [78] 10 [13] 12 [475] 14 [39]
    add("period4", *_periodic(2, 2, 11))
    # period 6: Hamming ties between the copies of a corner, SADs of 2^14 and more among the 11
    # shifts: Hamming-tie [240, 268], SAD-tie [7, 4], SAD >= 2^14 [51, 155], code 8 [185, 214],
    # 14 [158, 107]
    add("period6a", *_periodic(2, 3, 12))
    add("period6b", *_periodic(3, 2, 13))
    # code 13 that survives the median rule [19], and codes 10 [48] 14 [21]
    add("zero_visible", *_zero_visible())
    # a period-12 texture of 0 / 85 whose right eye is 170 brighter: the descriptors agree, every
    # accepted SAD is >= 2^14 [596]: the upper bins of k_stereo_median's first radix pass
    dark = blocks(H, W, 3, 4, 16, values=(0, 85))
    add("bright_right", dark, (np.roll(dark, -1, axis=1) + np.uint8(170)).astype(np.uint8))
    # few accepted matches: k = count / 2 of the radix select at small even and odd counts
    for seed in SPARSE:
        add("sparse_%d" % seed, *synth.stereo_pair(120, 160, seed), nfeatures=30, nlevels=4)
    # another scale table and row band: ceil(2 * scale[omax]) + 1 = 5 .. 9 rows (640 x 480: at
    # 320 x 240 the third level is too small for one 35-px cell); codes 2 [1] 4 [58] 5 [367] 8 [10]
    # 12 [557] 14 [8]
    add("sf2", *synth.stereo_pair(480, 640, 3), scale_factor=2.0, nlevels=3)
    # odd level widths: every level pitch / window address under load_bytes; codes 12 [592] 14 [61]
    add("odd_size", *synth.stereo_pair(ODD_H, ODD_W, 5))
    return tuple(out)


# What test_scenes_exercise_every_rule asserts over the whole set: rows (left keypoints) at least,
# [measured].  Codes 3, 6, 7 and 9 are asserted to be 0 (dead guards: see the test).
MINIMA = collections.OrderedDict([
    ("code2", 10),    # empty row list [1016]
    ("code4", 10),    # no gated candidate [1118]
    ("code5", 10),    # best Hamming distance >= 75 [2528]
    ("code8", 5),     # bestincR == +-5 [726]
    ("code10", 10),   # disparity < 0 [124]
    ("code11", 10),   # disparity >= maxD [40]
    ("code12", 10),   # accepted and kept [4765]
    ("code13", 5),    # accepted through disparity <= 0 AND kept by the median rule [19]
    ("code14", 10),   # median-rejected [494]
    ("row_list_missing", 1),                     # code 1 or 2 in a pair that has left rows [1016]
    ("no_left_rows", 1),                         # pairs with nL == 0 [1]
    ("pairs_with_kept_and_median_rejected", 1),  # pairs with >= 10 rows of code 12 and of code 14 [6]
    ("hamming_tie_then_sad", 20),                # Hamming-tie flag on rows of code >= 6 [766]
    ("sad_tie", 5),                              # SAD minimum at two or more shifts [242]
    ("octave_gate", 100),                        # in-range candidate dropped by the octave gate [7932]
    ("neighbour_octave", 10),                    # best candidate in a neighbouring octave [1528]
    ("accepted_sad_high", 10),                   # accepted rows whose own SAD is >= 2^14 [596]
    ("band_edge", 3),                            # best candidate on the outermost row of the row band [6]
    ("sad_high", 10),                            # one of the 11 SADs >= 2^14 [1034]
])


def by_name(name):
    return next(s for s in scenes() if s.name == name)


# Scenes grouped by what one BatchExtractor context can hold (one frame shape and parameter set);
# static, so that collecting the tests builds no image.
CONTEXTS = collections.OrderedDict([
    ("320x240", ("natural12", "narrow8", "vshift5", "blank_right", "blank_left", "period4", "period6a", "period6b",
                 "zero_visible", "bright_right")),
    ("160x120_sparse", tuple("sparse_%d" % seed for seed in SPARSE)),
    ("sf2", ("sf2",)),
    ("odd_size", ("odd_size",)),
])
NAMES = tuple(n for names in CONTEXTS.values() for n in names)


def check_contexts():
    """CONTEXTS names every scene once, and the scenes of a context share its shape and parameters."""
    assert NAMES == tuple(s.name for s in scenes())
    for names in CONTEXTS.values():
        assert len({(s.left.shape, s.nfeatures, s.scale_factor, s.nlevels) for s in map(by_name, names)}) == 1
