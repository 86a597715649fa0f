"""Launch arguments in SGPRs at dispatch, and the lean reduce of the down projection, read from the gfx950 code of
the specialised M = 1 decode GEMV (tools/gemv_path_bytes.py; no GPU needed).

woq_gemv_m1s_kernel's leading scalar parameters are preloaded (the kernel descriptor's kernarg preload length), so a
one-weight or pair launch reaches its first weight-tile load without waiting for a scalar load; the walk starts at the
real entry, behind the 256-byte block that hardware without preload support runs.  The down projection (11 slots per
column) reduces with reduce_fixed: its code behind the barrier was 1172 B with the runtime reduce
(profiles/gemv_dedup_path_bytes.txt), the 16-slot tail is 292 B, and 11 slots take three 16-B LDS reads where 16 take
four.
"""
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gemv_path_bytes", os.path.join(REPO, "tools", "gemv_path_bytes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def rows():
    tool = _tool()
    if tool.hipcc_path() is None or tool.find_tool("llvm-objdump") is None or tool.find_tool("llvm-readelf") is None:
        pytest.skip("hipcc / llvm-objdump / llvm-readelf not found")
    src = os.path.join(REPO, "neural_amd", "csrc", "woq_gemv.h")
    return {label: (tid, f) for label, tid, f in tool.report(src, tool.kernel_sets(False)["all"])}


def test_every_specialised_row_is_preloaded(rows):
    spec = {l: f for l, (tid, f) in rows.items() if tid.startswith("woq_gemv_m1s_kernel<")}
    assert len(spec) == 6
    for label, f in spec.items():
        print(label, f)
        assert f["preload"] > 0, (label, f)
    for label, (tid, f) in rows.items():  # the kernels that take a struct are not touched by the flag
        if not tid.startswith("woq_gemv_m1s_kernel<"):
            assert f["preload"] == 0, (label, f)


@pytest.mark.parametrize("label", ["o (1 weight)", "down", "lm_head", "gate/up (pair)"])
def test_first_tile_load_waits_for_no_scalar_load(rows, label):
    f = rows[label][1]
    print(label, f)
    assert f["pro_ins"] > 0, (label, "no live tile load found")
    assert f["lgkm"] == 0, (label, f)
    assert f["vm"] == 0, (label, f)


def test_down_tail(rows):
    down, o = rows["down"][1], rows["o (1 weight)"][1]
    print(down, o)
    assert rows["down"][0].endswith(",1,11>"), rows["down"][0]  # one weight, 11 slots per column
    assert down["tail_B"] < 600, down
    assert down["barriers"] == 1 and down["scratch"] == 0, down
