"""ctypes binding of oracle/_ref/libref_extractor.so -- TEST INFRASTRUCTURE ONLY.

That library is the reference's own ORBextractor_old.cc, compiled by oracle/ref/Makefile where a
reference checkout exists (oracle/ref/README.md).  available() tells whether it was built; the
functions mirror oracle_py's (extract, extract_levels, distribute_octree) plus tables().
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .oracle_py import KP_DTYPE, _p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_ref", "libref_extractor.so")
SELFTEST_PATH = os.path.join(HERE, "_ref", "ref_selftest")
SHA_FILE = os.path.join(HERE, "ref", "reference.sha256")

_lib = None


def reference_dir():
    """The reference checkout the recipe reads (oracle/ref/Makefile's REFERENCE_DIR)."""
    return os.environ.get("REFERENCE_DIR", "/root/reference")


def reference_present():
    return os.path.isdir(reference_dir())


def available():
    return os.path.exists(LIB_PATH)


def reference_sha256():
    """{file name: sha256} of the two reference files the recipe verifies before it builds."""
    out = {}
    with open(SHA_FILE) as f:
        for line in f:
            digest, path = line.split()
            out[os.path.basename(path)] = digest
    return out


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError("oracle/_ref/libref_extractor.so is not built (no reference checkout?)")
        _lib = C.CDLL(LIB_PATH)
        _lib.ref_selftest_digest.restype = C.c_uint64
    return _lib


def extract(img, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, lap=(0, 0)):
    """The reference's operator() -> (keypoints[KP_DTYPE], descriptors[N,32], monoIndex)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    cap = 4 * nfeatures + 64 * nlevels
    kps = np.zeros(cap, KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int(0)
    mono = lib().ref_extract(nfeatures, C.c_float(scale_factor), nlevels, ini_th, min_th, _p(img), w, h, w,
                             int(lap[0]), int(lap[1]), _p(kps), _p(desc), cap, C.byref(n))
    if mono < 0:
        raise RuntimeError("ref_extract failed: %d" % mono)
    return kps[:n.value], desc[:n.value], mono


def extract_levels(img, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
    """The reference's ComputeKeyPointsOctTree -> per level keypoints (level coordinates, octree
    order, with angle)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    cap = 4 * nfeatures + 64 * nlevels
    kps = np.zeros(cap, KP_DTYPE)
    cnt = np.zeros(nlevels, np.int32)
    n = lib().ref_extract_levels(nfeatures, C.c_float(scale_factor), nlevels, ini_th, min_th, _p(img), w, h, w,
                                 _p(kps), cap, _p(cnt))
    if n < 0:
        raise RuntimeError("ref_extract_levels failed: %d" % n)
    out, off = [], 0
    for c in cnt.tolist():
        out.append(kps[off:off + c])
        off += c
    return out


def distribute_octree(keys, minX, maxX, minY, maxY, N):
    keys = np.ascontiguousarray(keys, dtype=KP_DTYPE)
    cap = max(16, 4 * max(N, 1) + len(keys))
    out = np.zeros(cap, KP_DTYPE)
    m = lib().ref_distribute_octree(_p(keys), len(keys), minX, maxX, minY, maxY, N, _p(out), cap)
    assert m <= cap
    return out[:m]


def tables(nfeatures, scale_factor, nlevels):
    """The reference constructor's tables: dict with levels, scale_factor (the getters' values),
    scale, inv_scale, sigma2, inv_sigma2, features_per_level, umax, pattern [512, 2]."""
    levels, sf = C.c_int(0), C.c_float(0)
    f = [np.zeros(nlevels, np.float32) for _ in range(4)]
    fpl = np.zeros(nlevels, np.int32)
    umax = np.zeros(16, np.int32)
    pattern = np.zeros((512, 2), np.int32)
    lib().ref_tables(nfeatures, C.c_float(scale_factor), nlevels, C.byref(levels), C.byref(sf), *[_p(a) for a in f],
                     _p(fpl), _p(umax), _p(pattern))
    return dict(levels=levels.value, scale_factor=sf.value, scale=f[0], inv_scale=f[1], sigma2=f[2],
                inv_sigma2=f[3], features_per_level=fpl, umax=umax, pattern=pattern)


def selftest_digest():
    """(digest, keypoints) of oracle/ref/selftest.cpp's workload in the unsanitized library."""
    n = C.c_int(0)
    d = lib().ref_selftest_digest(C.byref(n))
    return int(d), n.value
