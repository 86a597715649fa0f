"""Host cost of a forward as tests/test_capi_cpu.py::test_host_cost_per_forward_under_3us measures it --
nad_plan_forward against the same call refused at its first check, best of five runs of 4000 calls each -- printed as
one JSON line of the four cost - base values in microseconds.  No GPU needed.  To compare two builds, alternate them:

  for r in 1 2 3 4 5; do for l in OLD.so NEW.so; do NAD_LIB_PATH=$l python tools/plan_host_times.py; done; done
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from neural_amd import _lib  # noqa: E402

SHAPES = ((4, 4096, 4096, 128, 1), (4, 22016, 4096, 128, 1), (2, 4096, 14336, 64, 1), (4, 4096, 4096, 128, 2048))


def main():
    L = _lib.lib()
    o = np.zeros(6, np.int64)
    ptr = o.ctypes.data

    def per_call(bits, n, k, g, m):
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(4000):
                L.nad_plan_forward(bits, n, k, g, 2, 0, m, 0, ptr, 6)
            best = min(best, (time.perf_counter() - t0) / 4000)
        return best

    res = {"lib": os.environ.get("NAD_LIB_PATH", "libneural_amd.so")}
    for bits, n, k, g, m in SHAPES:
        assert L.nad_plan_forward(bits, n, k, g, 2, 0, m, 0, ptr, 6) == 6
        base = per_call(3, n, k, g, m)
        res["int%d %dx%d M=%d" % (bits, n, k, m)] = round((per_call(bits, n, k, g, m) - base) * 1e6, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
