"""Structure of the M = 1 decode GEMV instantiations of a decode token, read from their gfx950 code (no GPU needed).

A decode launch pays for the code it runs where no memory latency hides it.  tools/gemv_path_bytes.py cross-compiles
just these kernels and walks their disassembly; this test pins what the specialised kernel was built for:
everything up to the first weight-tile load arrives with one scalar wait, nothing waits for the activation loads
before the first weight stage goes out, nothing spills, and the only barrier is the cross-wave reduction.
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
    return tool.report(src, tool.kernel_sets(False)["all"])


def _check_structure(rows):
    for label, tid, f in rows:
        print(label, tid, f)
        assert f["pro_ins"] > 0, (label, "no live tile load found")
        assert f["lgkm"] <= 1, (label, f)      # one batch of scalar loads
        assert f["vm"] == 0, (label, f)        # the first weight stage does not wait for the activations
        assert f["scratch"] == 0, (label, f)
        assert f["barriers"] == 1, (label, f)


def test_headline_instantiations_structure(rows):
    head = rows[:2]  # the tool's headline set
    assert [label for label, _, _ in head] == ["o (1 weight)", "down"]
    _check_structure(head)


def test_every_specialised_instantiation_structure(rows):
    """All six woq_gemv_m1s_kernel rows of the tool's `all` set: o, down, qkv, gate/up, lm_head and asym."""
    spec = [r for r in rows if r[1].startswith("woq_gemv_m1s_kernel<")]
    assert len(spec) == 6
    _check_structure(spec)
