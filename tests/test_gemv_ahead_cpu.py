"""The load-ahead forms of the specialised M = 1 decode GEMV (woq_gemv_m1s_kernel<..., AHEAD>), without a GPU.

1. Their gfx950 code, walked by tools/gemv_path_bytes.py (set `ahead`: every form next to the present form of the same
   launch): the way from the entry to the first weight-tile load and its waits are the present form's, nothing spills,
   16 waves still fit (at most 128 VGPRs), one barrier, and inside the stream every stage's loads are issued behind a
   vmcnt(0) and in front of the stage's first MFMA, with no further vector-memory wait before the MFMAs.
2. The launcher's choice, through the host dry runs: with NAD_GEMV_AHEAD=1, and with the knob unset, the Llama-2-7B QKV
   and gate/up launches take the form; down (its form was measured and not kept), O (one stage per wave), lm_head (two
   register stages), other formats and activation types, M > 1 and everything at NAD_GEMV_AHEAD=0 never do; nor does
   the QKV of two formats (int2 Q, K + int4 V: the dual launch), asked through geometry-only descriptors.  The batched
   launch needs device tensors: tests/test_gemv_ahead_gpu.py asks it.
"""
import importlib.util
import os

import pytest

from neural_amd import bestla

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
    return tool.report(src, tool.kernel_sets(False)["ahead"], with_code=True)


def test_structure_of_every_form(rows):
    assert len(rows) == 12
    for (label, tid, f, _), (label_a, tid_a, fa, _) in zip(rows[0::2], rows[1::2]):
        print(label_a, tid_a, fa)
        assert label_a == label + " ahead" and tid_a == tid[:-1] + ",true>"
        # entry -> first tile load: the same waits as the present form; the same instructions for the symmetric forms
        # (the asymmetric ones differ by one scheduling choice of the compiler: one instruction more or less)
        assert (fa["lgkm"], fa["vm"]) == (f["lgkm"], f["vm"]) and fa["vm"] == 0, (label_a, f, fa)
        if "asym" in label:
            assert abs(fa["pro_ins"] - f["pro_ins"]) <= 1 and abs(fa["pro_B"] - f["pro_B"]) <= 8, (label_a, f, fa)
        else:
            assert (fa["pro_ins"], fa["pro_B"]) == (f["pro_ins"], f["pro_B"]), (label_a, f, fa)
        assert fa["scratch"] == 0 and fa["vgpr"] <= 128, (label_a, fa)
        assert fa["barriers"] == 1 and fa["tail_B"] <= f["tail_B"] + 8, (label_a, f, fa)


def test_stream_issues_the_next_stage_before_it_computes(rows):
    """Between the prologue and the barrier: [vmcnt(0), the next stage's tile loads, MFMAs without a vector-memory wait
    among or before them], twice (the two register sets)."""
    for label, tid, f, code in rows[1::2]:
        ntiles = int(tid.split("<")[1].split(",")[4])  # KSN: tile loads per stage
        ev = []
        for mn, ops in code:
            if mn == "s_barrier":
                break
            if mn == "buffer_load_dwordx4" and " nt" in " " + ops:
                ev.append("T")
            elif mn.startswith("v_mfma"):
                ev.append("M")
            elif mn == "s_waitcnt" and "vmcnt" in ops:
                ev.append("W0" if "vmcnt(0)" in ops else "W")
        s = "".join(ev)
        first_m = s.index("M")
        loop = s[s.rindex("W0", 0, first_m):]  # from the vmcnt(0) in front of the first in-loop stage request
        half = "W0" + "T" * ntiles + "M" * (4 * ntiles)
        assert loop.startswith(half + half), (label, s)
        assert "T" not in loop[2 * len(half):] and "M" not in loop[2 * len(half):], (label, s)


LLAMA = {
    "qkv": lambda: bestla.plan_qkv_forward(4, 4096, 4096, 4096, 4096),
    "gate_up": lambda: bestla.plan_gate_up_forward(4, 11008, 4096),
}
NEVER = {
    "down": lambda: bestla.plan_forward(4, 4096, 11008),  # its form was measured and not kept
    "o": lambda: bestla.plan_forward(4, 4096, 4096),
    "lm_head": lambda: bestla.plan_forward(4, 32000, 4096),
    "qkv_asym_fp16_act": lambda: bestla.plan_qkv_forward(4, 4096, 4096, 4096, 4096, asym=True, act="fp16"),
    "int2_qkv": lambda: bestla.plan_qkv_forward(2, 4096, 4096, 4096, 4096, 64),
    "down_m2": lambda: bestla.plan_forward(4, 4096, 11008, m=2),
}


def _dual_qkv():
    """Q, K int2 g128 + V int4 g128: the QKV of two formats, one launch of woq_gemv_m1_dual_kernel"""
    q, k, v = (bestla.plan_only_weight(b, 4096, 4096, 128) for b in (2, 2, 4))
    p = bestla.plan_qkv(q, k, v, 1)
    assert p["kernel"] == "woq_gemv_m1_kernel" and p["launches"] == 1 and p["threads"] == 1024, p
    return p


NEVER["dual_qkv"] = _dual_qkv


def test_launcher_choice(knob):
    knob("NAD_GEMV_AHEAD", None)
    for name, plan in LLAMA.items():  # both classes are on by default
        assert plan()["ahead"] is True, (name, plan())
    knob("NAD_GEMV_AHEAD", "1")
    for name, plan in LLAMA.items():
        p = plan()
        assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is True and p["ahead"] is True, (name, p)
    assert LLAMA["qkv"]()["threads"] == 1024 and LLAMA["gate_up"]()["threads"] == 1024
    # ... by name: 16 waves of one 2-tile slice, one register stage, 3 weights / the pair, 16 slots, load-ahead
    assert LLAMA["qkv"]()["instance"] == "woq_gemv_m1s_kernel<4, 1, 0, false, 2, 1, 1, -1, 3, 16, true>"
    assert LLAMA["gate_up"]()["instance"] == "woq_gemv_m1s_kernel<4, 1, 0, false, 2, 1, 1, -1, 2, 16, true>"
    assert NEVER["dual_qkv"]()["instance"] is None  # woq_gemv_m1_dual_kernel: not one of the three named families
    p = bestla.plan_qkv_forward(4, 4096, 4096, 4096, 4096, scale_dtype="bf16", asym=True)
    assert p["ahead"] is True, p
    for name, plan in list(NEVER.items()):
        assert plan()["ahead"] is False, (name, plan())
    knob("NAD_GEMV_AHEAD", "0")
    for name, plan in list(LLAMA.items()) + list(NEVER.items()):
        assert plan()["ahead"] is False, (name, plan())
    knob("NAD_GEMV_M1_SPEC", "0")
    knob("NAD_GEMV_AHEAD", "1")
    for name, plan in LLAMA.items():
        p = plan()
        assert p["m1_spec"] is False and p["ahead"] is False, (name, p)
