"""Generates tests/golden/ref_*.npz from the REFERENCE's extractor (oracle/_ref/libref_extractor.so,
its ORBextractor_old.cc compiled by oracle/ref/Makefile), not from the oracle: fixtures the oracle
did not write, for the oracle (tests/test_reference_pin.py) and the GPU
(tests/test_gpu_reference_fixtures.py) to be checked against.  Runs only where the reference is
built.  From the repo root:
    python tests/golden/make_ref_golden.py
The cases, their generators and the defined-domain assertion are in tests/ref_cases.py.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_py as O  # noqa: E402
from oracle import ref_py as R  # noqa: E402
from tests import ref_cases as RC  # noqa: E402


def arrays(c):
    """Everything a fixture stores, from the live reference."""
    RC.assert_in_domain(c)
    assert RC.level_sizes(c) == O.level_sizes(c.w, c.h, c.scale_factor, c.nlevels), c.name
    img, out = RC.compute(c, R)
    for key in ("kps", "lvl_kps"):
        if key in out:
            out.update(RC.pack_kps(key, out.pop(key)))
    sha = R.reference_sha256()
    out.update(img_sha256=hashlib.sha256(img.tobytes()).hexdigest(), shape=np.array([c.h, c.w]), gen_kind=c.kind,
               gen_seed=c.seed, nfeatures=c.nfeatures, scale_factor=np.float32(c.scale_factor), nlevels=c.nlevels,
               ini_th=c.ini_th, min_th=c.min_th, lap=np.array(c.lap),
               ref_cc_sha256=sha["ORBextractor_old.cc"], ref_h_sha256=sha["ORBextractor_old.h"])
    return out


def main():
    if not R.available():
        sys.exit("the reference extractor is not built (oracle/ref/README.md)")
    for c in RC.CASES:
        a = arrays(c)
        path = RC.fixture_path(c)
        np.savez_compressed(path, **a)
        size = os.path.getsize(path)
        assert size <= RC.MAX_FIXTURE_BYTES, (c.name, size)
        print("%-28s %5d keypoints, mono %5d, per level %s, %6d bytes" % (
            c.name, len(a["kps_x"]), int(a["mono"]), a["lvl_count"].tolist() if c.levels else "-", size))


if __name__ == "__main__":
    main()
