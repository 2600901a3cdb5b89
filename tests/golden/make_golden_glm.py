"""Generates tests/golden/glm_check_n2000.npy: the raw float32 output of oracle/_ref/check_glm (mat3 products, dot
products and lengths of LCG-random inputs computed by the reference's vendored GLM; built by oracle/Makefile where the
reference tree is available), one row of 22 floats per input set.  tests/test_oracle.py pins the oracle's restated
small-matrix helpers to these rows bit for bit.

Run from the repo root:  python tests/golden/make_golden_glm.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import oracle as O  # noqa: E402

N = 2000


def main():
    exe = O.build_ref()
    if exe is None:
        sys.exit("oracle/_ref/check_glm not built (needs the reference's GLM)")
    rows = np.frombuffer(subprocess.check_output([exe, str(N)]), dtype=np.float32).reshape(N, 22)
    out = os.path.join(HERE, "glm_check_n%d.npy" % N)
    np.save(out, rows)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
