"""nad_moe_gate_route / nad_plan_moe_gate_route, the host side, and the numpy model of its logits: no GPU needed.

The refusals are checked with aligned fake pointers: every one comes before any launch.  The model (tests/gate_model.py)
is held to the float64 dot product under its derived bound, depth * 2^-24 * sum |x w|; the GPU tests hold the kernel to
the model's bits.
"""
import ctypes as C

import numpy as np
import pytest

from neural_amd import _lib, bestla
from neural_amd._lib import lib
from tests import gate_model

KS = (4, 36, 4096, 4100, 12292)
NES = (1, 3, 8, 64)
F32, F16, BF16 = 0, 1, 2


def test_symbols_are_declared_exported_and_signed():
    for name in ("nad_moe_gate_route", "nad_plan_moe_gate_route"):
        assert name in _lib.header_symbols()
        assert name in _lib.SIGNATURES
        assert hasattr(lib(), name)
    assert len(_lib.SIGNATURES["nad_moe_gate_route"][1]) == 16
    assert len(_lib.SIGNATURES["nad_plan_moe_gate_route"][1]) == 7
    header = open(_lib.HEADER).read()
    assert "#define NAD_KERNEL_MOE_GATE_ROUTE 24" in header
    assert bestla.KERNELS[24] == "moe_gate_route_kernel"


@pytest.mark.parametrize("m", [1, 5, 2048])
@pytest.mark.parametrize("ne,dtype", [(8, "fp32"), (64, "fp16"), (3, "bf16")])
def test_plan_is_one_launch_of_m_workgroups(m, ne, dtype):
    o = np.full(8, -7, np.int64)
    code = {"fp32": F32, "fp16": F16, "bf16": BF16}[dtype]
    assert lib().nad_plan_moe_gate_route(m, 4096, ne, 2 if ne > 1 else 1, code, bestla._ptr(o), 8) == 5
    assert o.tolist() == [24, m, 1024, 16 * ne * 4, 1, -7, -7, -7]
    plan = bestla.plan_moe_gate_route(m, 4096, ne, 1, dtype)
    assert plan == dict(kernel="moe_gate_route_kernel", grid=m, threads=1024, lds=16 * ne * 4, launches=1)
    # a short buffer: the first values, and their count
    o2 = np.full(3, -7, np.int64)
    assert lib().nad_plan_moe_gate_route(m, 4096, ne, 1, code, bestla._ptr(o2), 3) == 3
    assert o2.tolist() == [24, m, 1024]


def test_plan_refuses_what_the_entry_refuses():
    o = np.zeros(5, np.int64)
    assert lib().nad_plan_moe_gate_route(1, 4098, 8, 2, F32, bestla._ptr(o), 5) == -1
    assert "nad_plan_moe_gate_route: k (4098)" in bestla.last_error()
    assert lib().nad_plan_moe_gate_route(0, 4096, 8, 2, F32, bestla._ptr(o), 5) == -1
    assert "m=0" in bestla.last_error()
    with pytest.raises(RuntimeError, match=r"n_expert \(65\)"):
        bestla.plan_moe_gate_route(1, 4096, 65, 2, "fp32")


# aligned fake addresses: never dereferenced, the checks come before any launch
ACT, GATE, IDS, WTS, LOGITS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
GOOD = dict(act=ACT, lda=4096, gate=GATE, gate_dtype=F32, ldw=4096, m=3, k=4096, n_expert=8, top_k=2, ids=IDS, ids_ld=2,
            wts=WTS, wts_ld=2, logits=LOGITS, logits_ld=8)
ORDER = ("act", "lda", "gate", "gate_dtype", "ldw", "m", "k", "n_expert", "top_k", "ids", "ids_ld", "wts", "wts_ld",
         "logits", "logits_ld")


def _call(**change):
    a = dict(GOOD, **change)
    bestla.lib().nad_clear_error()
    return lib().nad_moe_gate_route(*[a[n] for n in ORDER], None)


REFUSALS = [
    (dict(act=None), "act is null"),
    (dict(gate=None), "gate is null"),
    (dict(ids=None), "ids is null"),
    (dict(wts=None), "wts is null"),
    (dict(m=-1), r"m \(-1\) is negative"),
    (dict(k=0, lda=0, ldw=0), r"k \(0\) must be a multiple of 4, at least 4"),
    (dict(k=4094), r"k \(4094\) must be a multiple of 4"),
    (dict(n_expert=0), r"n_expert \(0\) is outside 1\.\.64"),
    (dict(n_expert=65, logits_ld=65), r"n_expert \(65\) is outside 1\.\.64"),
    (dict(top_k=0), r"top_k \(0\) is outside 1\.\.n_expert \(8\)"),
    (dict(top_k=9, ids_ld=9, wts_ld=9), r"top_k \(9\) is outside 1\.\.n_expert \(8\)"),
    (dict(gate_dtype=3), r"gate_dtype \(3\) is none of"),
    (dict(gate_dtype=-1), r"gate_dtype \(-1\) is none of"),
    (dict(lda=4092), r"lda \(4092\) must be a multiple of 4, at least k \(4096\)"),
    (dict(lda=4098), r"lda \(4098\) must be a multiple of 4"),
    (dict(ldw=4092), r"ldw \(4092\) must be a multiple of 4, at least k \(4096\)"),
    (dict(ldw=4102), r"ldw \(4102\) must be a multiple of 4"),
    (dict(ids_ld=1), r"ids_ld \(1\) is below top_k \(2\)"),
    (dict(wts_ld=1), r"wts_ld \(1\) is below top_k \(2\)"),
    (dict(logits_ld=7), r"logits_ld \(7\) is below n_expert \(8\)"),
    (dict(act=ACT + 4), "act is not 16-byte aligned"),
    (dict(gate=GATE + 8), "gate is not 16-byte aligned"),
]


@pytest.mark.parametrize("change,text", REFUSALS, ids=[t.split(" ")[0] + "_" + str(i) for i, (_, t) in enumerate(REFUSALS)])
def test_refusals_name_the_argument(change, text):
    import re

    assert _call(**change) == -1
    err = bestla.last_error()
    assert err.startswith("nad_moe_gate_route: ") and re.search(text, err), err


def test_empty_call_returns_zero_and_a_narrow_logits_ld_is_fine_without_logits():
    assert _call(m=0) == 0
    assert bestla.last_error() == ""
    assert _call(m=0, logits=None, logits_ld=0) == 0
    # an m = 0 call is still checked
    assert _call(m=0, k=6) == -1 and "k (6)" in bestla.last_error()


# ------------------------------------------------------------------------------------------------ the model
def _case(k, ne, m=2, seed=0):
    rng = np.random.default_rng(seed + 7 * k + ne)
    return (rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32),
            rng.uniform(-0.5, 0.5, size=(ne, k)).astype(np.float32))


def test_model_is_within_the_derived_bound_of_the_exact_dot_product():
    worst, worst_ratio = 0.0, 0.0
    for k in KS:
        for ne in NES:
            x, w = _case(k, ne)
            got = gate_model.logits(x, w)
            ref = x.astype(np.float64) @ w.astype(np.float64).T
            err = np.abs(got.astype(np.float64) - ref)
            bnd = gate_model.bound(x, w)
            print(f"K {k} n_expert {ne}: err {err.max():.3e} bound (min) {bnd.min():.3e}")
            assert (err <= bnd).all(), (k, ne, float(err.max()), float(bnd.min()))
            worst = max(worst, float(err.max()))
            worst_ratio = max(worst_ratio, float((err / bnd).max()))
    print(f"worst error {worst:.3e}; worst error / bound {worst_ratio:.3e}")


def test_model_order_by_hand_at_small_k():
    """K = 36: nine live slots, all in wave 0; the butterfly over lanes 0..8 written out"""
    x, w = _case(36, 1, m=1)
    s = []
    for t in range(9):
        a = np.float32(0.0)
        for j in range(4):
            a = np.float32(a + np.float32(x[0, 4 * t + j] * w[0, 4 * t + j]))
        s.append(a)
    lanes = np.array(s + [np.float32(0)] * 55, np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
    total = lanes[0]
    for _ in range(15):
        total = np.float32(total + np.float32(0))
    assert gate_model.logits(x, w)[0, 0].view(np.uint32) == total.view(np.uint32)


def test_model_invariances():
    x, w = _case(4100, 8, m=5)
    full = gate_model.logits(x, w)
    perm = np.random.default_rng(3).permutation(8)
    assert np.array_equal(gate_model.logits(x, w[perm]).view(np.uint32), full[:, perm].view(np.uint32))
    for r in (0, 4):  # a row alone, and among other rows
        assert np.array_equal(gate_model.logits(x[r:r + 1], w).view(np.uint32), full[r:r + 1].view(np.uint32))
    other = x.copy()
    other[1:4] = 0.25
    assert np.array_equal(gate_model.logits(other, w)[[0, 4]].view(np.uint32), full[[0, 4]].view(np.uint32))
    assert np.array_equal(gate_model.logits(x, w[:3]).view(np.uint32), full[:, :3].view(np.uint32))  # nor on n_expert


def test_stable_top_k_breaks_ties_to_the_lower_index():
    lg = np.array([[1.0, 3.0, 3.0, -2.0]], np.float32)
    assert gate_model.stable_top_k(lg, 3).tolist() == [[1, 2, 0]]
