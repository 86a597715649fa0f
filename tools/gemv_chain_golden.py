#!/usr/bin/env python3
"""Record the outputs of tests/test_gemv_m1_chain_gpu.py's cases from one library build (needs a GPU).

  NAD_LIB_PATH=/path/to/earlier/libneural_amd.so python tools/gemv_chain_golden.py OUT.npz

The test compares the current build with tests/golden/gemv_m1_chain_parent.npz bit for bit; that file was written by
this tool from the build before woq_gemv_m1s_kernel's arguments and reduce changed.  The inputs are seeded and the
weights are packed by the oracle on the CPU, so the arrays depend on the library alone.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from tests import test_gemv_m1_chain_gpu as t
    from tests.oracle_lib import Oracle
    orc = Oracle.get()
    out = {}
    for name in t.CASES:
        ys, _ = t.run_case(name, orc, check_plan=False)
        for i, y in enumerate(ys):
            out[f"{name}.{i}"] = y
    np.savez(sys.argv[1], **out)
    print("wrote", sys.argv[1], len(out), "arrays")


if __name__ == "__main__":
    main()
