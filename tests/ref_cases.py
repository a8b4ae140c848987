"""The cases behind tests/golden/ref_*.npz: fixtures written by the reference's own extractor
(oracle/ref/README.md), their image generators and their loader.

Shared by tests/golden/make_ref_golden.py (writes them where the reference is built),
tests/test_reference_pin.py (oracle == fixtures everywhere, live regeneration where the
reference is built) and tests/test_gpu_reference_fixtures.py (GPU == fixtures; reads nothing but
the .npz files and this module).  No raw image is stored: a fixture names its generator and seed
and carries the image's sha256, as tests/test_golden.py's load_case does.
"""
import glob
import hashlib
import os
from collections import namedtuple

import numpy as np

from orbslam3lib_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
MAX_FIXTURE_BYTES = 89739  # the largest golden committed before these (c2_left_640x480_n2000.npz)


def image(kind, seed, h, w):
    """The frame generators, by name."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "frame":      # the bench's synthetic scene
        return synth.frame(h, w, seed)
    if kind == "noise":      # iid uniform: the densest candidate lists, N reached on every level
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "checker3":   # 3-px checkerboard: every pixel a one-sided candidate, all responses tie
        return (((x // 3 + y // 3) % 2) * 200 + 20).astype(np.uint8)
    if kind == "dots":
        # flat ground with sparse 3x3 dots, the centre pixel a little brighter (a flat dot's nine
        # equal scores all lose the strict nonmax).  Faint ones (+12, centre +16) are corners only at
        # minThFAST, and only where their cell holds no strong dot (+90, centre +120): cells with
        # the fallback beside cells without, empty cells, octree nodes that hold a single key
        img = np.full((h, w), 100, np.int32)
        n = h * w // 250
        for cy, cx, strong in zip(rng.integers(4, h - 4, n), rng.integers(4, w - 4, n), rng.random(n) < 0.08):
            img[cy - 1:cy + 2, cx - 1:cx + 2] += 90 if strong else 12
            img[cy, cx] += 30 if strong else 4
        return np.clip(img, 0, 255).astype(np.uint8)
    if kind == "lowcontrast":  # 128 +- 6: no corner at iniThFAST 20 (|difference| <= 12), few at 7
        return (128 + rng.integers(-6, 7, (h, w))).astype(np.uint8)
    raise ValueError(kind)


Case = namedtuple("Case", "name h w kind seed nfeatures scale_factor nlevels ini_th min_th lap levels")

# Seeds are chosen so that the content a case is named for is really there
# (tests/test_reference_pin.py: test_fixtures_reach_the_paths_they_are_named_for); among others the
# (100, 250) cases hold keypoints exactly on a bound of the lapping area, which is inclusive.
CASES = [
    # 160x120, 4 levels, 300 features: one mixed batch on the GPU
    Case("ref_frame_160x120", 120, 160, "frame", 5, 300, 1.2, 4, 20, 7, (0, 0), True),
    Case("ref_noise_160x120", 120, 160, "noise", 13, 300, 1.2, 4, 20, 7, (100, 250), False),
    Case("ref_checker3_160x120", 120, 160, "checker3", 0, 300, 1.2, 4, 20, 7, (0, 1000), False),
    Case("ref_dots_160x120", 120, 160, "dots", 3, 300, 1.2, 4, 20, 7, (0, 0), True),
    Case("ref_lowcontrast_160x120", 120, 160, "lowcontrast", 8, 300, 1.2, 4, 20, 7, (0, 1000), False),
    # 160x120 with other parameters
    Case("ref_frame_160x120_n50", 120, 160, "frame", 6, 50, 1.2, 4, 20, 7, (100, 250), False),
    Case("ref_frame_160x120_th0", 120, 160, "frame", 7, 300, 1.2, 4, 0, 0, (0, 0), False),
    Case("ref_frame_160x120_th40", 120, 160, "frame", 7, 300, 1.2, 4, 40, 3, (0, 1000), False),
    # 320x240, 6 levels, 1000 features: one mixed batch on the GPU
    Case("ref_frame_320x240", 240, 320, "frame", 5, 1000, 1.2, 6, 20, 7, (100, 250), True),
    Case("ref_noise_320x240", 240, 320, "noise", 12, 1000, 1.2, 6, 20, 7, (0, 0), False),
    Case("ref_checker3_320x240", 240, 320, "checker3", 0, 1000, 1.2, 6, 20, 7, (0, 0), False),
    Case("ref_dots_320x240", 240, 320, "dots", 4, 1000, 1.2, 6, 20, 7, (0, 1000), False),
    Case("ref_frame_320x240_n500", 240, 320, "frame", 3, 500, 1.2, 6, 20, 7, (0, 1000), False),
    # scale factor 2 (exact 2x levels: the pyramid's area path downstream).  320x240 would leave
    # level 2 at 80x60, outside the reference's defined domain (nRows = 0), so 272 rows: 80x68
    Case("ref_frame_320x272_sf2", 272, 320, "frame", 9, 500, 2.0, 3, 20, 7, (0, 0), False),
    # the headset eye plus one pixel: odd level sizes, more than one octree iteration per level
    Case("ref_frame_641x401", 401, 641, "frame", 1, 2000, 1.2, 8, 20, 7, (100, 250), False),
]


def level_sizes(c):
    """Level sizes as the reference's constructor and canonical pyramid loop give them: float
    scale factors, round-half-even (numpy.rint on float32 is lrintf)."""
    sizes, s = [], np.float32(1.0)
    for level in range(c.nlevels):
        if level:
            s = np.float32(np.float64(s) * np.float64(np.float32(c.scale_factor)))
        inv = np.float32(1.0) / s
        sizes.append((int(np.rint(np.float32(c.w) * inv)), int(np.rint(np.float32(c.h) * inv))))
    return sizes


def assert_in_domain(c):
    """The reference's defined domain (ORBextractor_old.cc:799-805, :561): every level has at
    least one 35-px cell each way (else nCols or nRows is 0 and ceil(width / 0) is converted to
    int), and DistributeOctTree's nIni = round(width / height) is at least 1 (else a division by
    zero and an out-of-range node index)."""
    for lw, lh in level_sizes(c):
        assert lw - 32 >= 35 and lh - 32 >= 35, (c.name, lw, lh)
        assert int(np.rint(np.float32(lw - 32) / np.float32(lh - 32))) >= 1, (c.name, lw, lh)


def case_image(c):
    return image(c.kind, c.seed, c.h, c.w)


def case_kwargs(c):
    return dict(nfeatures=c.nfeatures, scale_factor=c.scale_factor, nlevels=c.nlevels, ini_th=c.ini_th,
                min_th=c.min_th)


def compute(c, impl):
    """The fixture's arrays from an implementation with oracle_py's extract / extract_levels
    (oracle.ref_py where the reference is built, oracle.oracle_py for the comparison)."""
    img = case_image(c)
    k, d, mono = impl.extract(img, lap=c.lap, **case_kwargs(c))
    out = dict(mono=np.int32(mono), kps=k, desc=d)
    if c.levels:
        lv = [(e[0] if isinstance(e, tuple) else e) for e in impl.extract_levels(img, **case_kwargs(c))]
        out["lvl_count"] = np.array([len(a) for a in lv], np.int32)
        out["lvl_kps"] = np.concatenate(lv) if lv else k[:0]
    return img, out


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])  # cv::KeyPoint, as oracle_py.KP_DTYPE


def pack_kps(prefix, kps):
    """Keypoints as one array per field (compresses far better than the 28-byte records)."""
    return {"%s_%s" % (prefix, f): np.ascontiguousarray(kps[f]) for f in KP_FIELDS}


def unpack_kps(z, prefix):
    out = np.zeros(len(z[prefix + "_x"]), KP_DTYPE)
    for f in KP_FIELDS:
        out[f] = z[prefix + "_" + f]
    return out


def fixture_path(c):
    return os.path.join(GOLD, c.name + ".npz")


def fixture_paths():
    return sorted(glob.glob(os.path.join(GOLD, "ref_*.npz")))


def load(path):
    """(case, image, arrays) of one committed fixture; the image is regenerated and verified."""
    z = np.load(path)
    c = Case(os.path.basename(path)[:-4], int(z["shape"][0]), int(z["shape"][1]), str(z["gen_kind"]),
             int(z["gen_seed"]), int(z["nfeatures"]), float(z["scale_factor"]), int(z["nlevels"]),
             int(z["ini_th"]), int(z["min_th"]), tuple(int(v) for v in z["lap"]), "lvl_count" in z.files)
    img = case_image(c)
    assert hashlib.sha256(img.tobytes()).hexdigest() == str(z["img_sha256"]), "image generator drifted: " + path
    arrays = dict(mono=int(z["mono"]), kps=unpack_kps(z, "kps"), desc=z["desc"])
    if c.levels:
        arrays.update(lvl_count=z["lvl_count"], lvl_kps=unpack_kps(z, "lvl_kps"))
    arrays.update(ref_cc_sha256=str(z["ref_cc_sha256"]), ref_h_sha256=str(z["ref_h_sha256"]))
    return c, img, arrays


def split_levels(z):
    out, off = [], 0
    for n in z["lvl_count"].tolist():
        out.append(z["lvl_kps"][off:off + n])
        off += n
    return out


def same_kps(a, b, msg=""):
    assert len(a) == len(b), (msg, len(a), len(b))
    for f in KP_FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s %s" % (msg, f))
