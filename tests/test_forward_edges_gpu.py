"""Stride, padding and epilogue edges of every forward path (tests/edges.py holds the harness and the invariant).

One parametrised test per kernel family.  Each case first asserts, with DeviceWeight.plan, that its shape and knobs
select the kernel it is about (and the split-K / specialised-M=1 form where named), so a change in kernel choice fails
here instead of silently moving the case to another kernel; then it runs the seven single-weight epilogues x the two
alignment variants on canaried operands, each call twice.  The shapes are the smallest that select each family: N = 203
(12.7 stripes of 16, not a multiple of 4), K = 300 (a tail inside a K tile and, at groups of 32 / 128, inside a group)
wherever the kernel takes it and K = 1024 where it needs K % 8 == 0, M off the 16 / 64 / 256-row tiles.

The plan is the aligned, contiguous call's: the "odd" variant's activation rows are not 16-byte aligned, which the
mid-M kernel does not take (such a call falls through to the next kernel of run_gemm / forward_one, at that kernel's
tolerance or tighter); the "aligned" variant runs the planned kernel with lda > k.

Tolerances are the existing ones of each path, on the error normalised by the un-epilogued product: TOL_DECODE for the
M <= 16 kernels and the mid-M kernel, test_gemm2_gpu's per-dtype TOL (FOLD_TOL where the plan reports the folded
scale) for the prefill GEMMs, TOL_I8 against the oracle's int8 forward for the int8 arithmetic, test_gguf_types_gpu's
_tol for the GGUF types in fp mode and its 1e-5 against the block model (gguf_blocks.forward_int / the oracle's Q4_0
forward) in the int8 mode, test_more_bits_gpu's 1e-3 for the NFloat 4-bit weight."""
import numpy as np
import pytest

from tests import edges
from tests import gguf_blocks as gb
from tests.conftest import gpu_available
from tests.oracle_lib import F16, F32, F4_NF4, S2, S4, S8
from tests.test_gemm2_gpu import FOLD_TOL, TOL
from tests.test_gguf_types_gpu import _tol as gguf_tol, _weight as gguf_weight
from tests.test_gpu_parity import TOL_DECODE, _blob
from tests.test_int8_compute_gpu import TOL_I8

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

ACTS = ["fp32", "fp16", "bf16"]
N = 203
DECODE = ("woq_gemv_m1_kernel", "woq_gemv_kernel", "woq_skinny_kernel", "woq_mid_kernel")
F4_TOL = 1e-3  # NFloat 4-bit weights: the LUT entries enter the MFMA rounded to fp16 (test_more_bits_gpu's bar for them)

_WEIGHTS = {}


def _int_weight(oracle, n, k, bs, qt, st, asym, comp=4, seed=0):
    key = (n, k, bs, qt, st, asym, comp, seed)
    if key not in _WEIGHTS:
        blob = _blob(oracle, n, k, bs, qt, st, asym, comp, seed=n + k + bs + qt + seed)
        _WEIGHTS[key] = (blob, bestla.DeviceWeight(blob))
    return _WEIGHTS[key]


def _activations(m, k, act, seed=0):
    A = np.random.default_rng(m * 7 + k + seed).uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    return edges.round_to(A, act)


def _set_knobs(knob, knobs):
    for name, value in knobs.items():
        knob(name, value)


def _path_tol(plan, act):
    if plan["kernel"] in DECODE:
        return TOL_DECODE
    return max(TOL[act], FOLD_TOL) if plan["fold"] else TOL[act]


# ------------------------------------------------------------------------------------------------ fp families
def C(id, qt, k, bs, m, kernel, knobs=None, asym=False, st=F16, **expect):
    return pytest.param((qt, k, bs, st, asym, m, kernel, knobs or {}, expect), id=id)


FP_CASES = [
    # the M = 1 GEMV: the specialised kernel, the general one, an int2 weight
    C("gemv_m1_spec", S4, 1024, 128, 1, "woq_gemv_m1_kernel", m1_spec=True),
    C("gemv_m1_general", S4, 1024, 128, 1, "woq_gemv_m1_kernel", {"NAD_GEMV_M1_SPEC": 0}, m1_spec=False),
    C("gemv_m1_int2", S2, 1024, 64, 1, "woq_gemv_m1_kernel"),
    # the stripe-stream GEMV
    C("gemv_m3_ktail", S4, 300, 32, 3, "woq_gemv_kernel"),
    C("gemv_m16", S4, 1024, 128, 16, "woq_gemv_kernel", {"NAD_MID_MAX_M": 0}),
    # the per-stripe skinny kernel; NFloat weights take it by default
    C("skinny_m1", S4, 300, 32, 1, "woq_skinny_kernel", {"NAD_GEMV_DISABLE": 1}),
    C("skinny_m9", S4, 300, 32, 9, "woq_skinny_kernel", {"NAD_GEMV_DISABLE": 1}),
    C("skinny_nf4_m5", F4_NF4, 300, 32, 5, "woq_skinny_kernel", st=F32),
    # mid-M: one run, and K runs whose reduce applies the epilogue
    C("mid_m12", S4, 1024, 128, 12, "woq_mid_kernel", ksplit=1),
    C("mid_m40", S4, 1024, 128, 40, "woq_mid_kernel", ksplit=1),
    C("mid_m40_ks2", S4, 1024, 128, 40, "woq_mid_kernel", {"NAD_MID_KS": 2}, ksplit=2),
    # gemm7 (int4 g128): split K with the reduce, whole K with a K tail
    C("gemm7_m65_splitk", S4, 1024, 128, 65, "woq_gemm7_kernel", ksplit=4),
    C("gemm7_m130_ktail", S4, 300, 128, 130, "woq_gemm7_kernel", ksplit=1),
    C("gemm3_m65_splitk", S4, 1024, 128, 65, "woq_gemm3_kernel", {"NAD_GEMM_KERNEL": 3}, ksplit=4),
    C("gemm3_m65_ktail", S4, 300, 128, 65, "woq_gemm3_kernel", {"NAD_GEMM_KERNEL": 3}, ksplit=1),
    C("gemm2_m65", S4, 1024, 128, 65, "woq_gemm2_kernel", {"NAD_GEMM_KERNEL": 2}, ksplit=1),
    # gemm4: int4 g32, int2 g64 (split K), int8
    C("gemm4_int4_g32_ktail", S4, 300, 32, 65, "woq_gemm4_kernel", {"NAD_GEMM_KERNEL": 3}, ksplit=1),
    C("gemm4_int2_g64_splitk", S2, 1024, 64, 40, "woq_gemm4_kernel", {"NAD_GEMM_KERNEL": 3}, ksplit=2),
    C("gemm4_int8_g32_ktail", S8, 300, 32, 40, "woq_gemm4_kernel", {"NAD_GEMM_KERNEL": 3, "NAD_MID_MAX_M": 0}),
    # the register-staged fallback, forced as test_gemm4_takes_the_fallback_configs forces it
    C("gemm_fallback_int2", S2, 1024, 64, 40, "woq_gemm_kernel", {"NAD_GEMM_KERNEL": 3, "NAD_GEMM4_DISABLE": 1}),
]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", FP_CASES)
def test_fp_family_edges(oracle, knob, case, act):
    qt, k, bs, st, asym, m, kernel, knobs, expect = case
    blob, w = _int_weight(oracle, N, k, bs, qt, st, asym, comp=1 if qt == F4_NF4 else 4)
    _set_knobs(knob, knobs)
    plan = w.plan(m, act)
    assert plan["kernel"] == kernel, plan
    for key, value in expect.items():
        assert plan[key] == value, (key, plan)
    tol = {"aligned": _path_tol(plan, act), "odd": _path_tol(plan, act)}
    if qt == F4_NF4:
        tol = F4_TOL
    if kernel == "woq_mid_kernel":
        # the mid-M kernel takes 16-byte aligned rows only: the "odd" variant goes on to the kernel the same call takes
        # with the mid-M range switched off, and is held to that kernel's bar
        knob("NAD_MID_MAX_M", 0)
        tol["odd"] = _path_tol(w.plan(m, act), act)
        knob("NAD_MID_MAX_M", None)
    xt, xv = _activations(m, k, act)
    prod = oracle.forward(xv, blob, N, k).astype(np.float64)
    edges.check_forward_matrix(w, xt, prod, tol, f"{kernel} m={m} {act}")


# ------------------------------------------------------------------------------------------------ int8 arithmetic
def I(id, qt, k, bs, m, asym=False, st=F32):
    return pytest.param((qt, k, bs, st, asym, m), id=id)


I8_EDGE_CASES = [
    # woq_i8_kernel: KSPLIT at M <= 16 (the K-split partials combined in LDS), RT = 4 above
    I("int4_asym_g32_ktail_m3", S4, 300, 32, 3, asym=True),
    I("int4_asym_g32_ktail_m16", S4, 300, 32, 16, asym=True),
    I("int4_asym_g32_ktail_m17", S4, 300, 32, 17, asym=True),
    I("int4_asym_g32_ktail_m70", S4, 300, 32, 70, asym=True),
    I("int2_g64_m16", S2, 1024, 64, 16),
    I("int2_g64_m17", S2, 1024, 64, 17),
    I("int8_g32_m3", S8, 512, 32, 3),
    I("int8_g32_m70", S8, 512, 32, 70),
]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", I8_EDGE_CASES)
def test_int8_compute_edges(oracle, case, act):
    qt, k, bs, st, asym, m = case
    blob, w = _int_weight(oracle, N, k, bs, qt, st, asym, comp=4)
    assert oracle.info(blob)["has_reduce"] == 1
    w.set_compute(bestla.COMPUTE_INT8)
    try:
        plan = w.plan(m, act)
        assert plan["kernel"] == "woq_i8_kernel", plan
        xt, xv = _activations(m, k, act, seed=1)
        prod = oracle.forward_int8(xv, blob, N, k).astype(np.float64)
        edges.check_forward_matrix(w, xt, prod, TOL_I8, f"woq_i8_kernel m={m} {act}")
    finally:
        w.set_compute(None)


# ------------------------------------------------------------------------------------------------ GGUF types
GGUF_N, GGUF_K = 75, 320  # 4.7 stripes, ten blocks of 32: a partial stripe and a partial K tile
Q4_0 = bestla.GGUF_Q4_0 if gpu_available() else 2


def _gguf(oracle, type):
    """(DeviceWeight, fp64 dequantized [n][k], int8-mode model(a fp32 [m][k]) -> [m][n])"""
    n, k = GGUF_N, GGUF_K
    if type != Q4_0:
        blocks, deq, w = gguf_weight(type, n, k)
        return w, deq, lambda a: gb.forward_int(type, blocks, n, k, a)
    key = ("q4_0", n, k)
    if key not in _WEIGHTS:
        W = np.random.default_rng(40).uniform(-1, 1, size=(n, k)).astype(np.float32)
        blocks = oracle.q4_0_quantize(W)
        _WEIGHTS[key] = (blocks, oracle.q4_0_dequant(blocks, n, k).astype(np.float64),
                         bestla.DeviceWeight.from_gguf(Q4_0, blocks, n, k))
    blocks, deq, w = _WEIGHTS[key]
    return w, deq, lambda a: oracle.q4_0_forward(a, blocks, n, k)


# fp mode: the kernel that computes X (q d)^T; the types with mins add the min-term pass (the small kernel at M <= 16,
# the block-sum pre-pass and the tiled kernel above), which applies the epilogue
GGUF_FP_KERNEL = {5: "woq_gemv_kernel", 40: "woq_gemm7_kernel"}


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("mode", ["int8", "fp"])
@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("type", [Q4_0, gb.Q8_0, gb.Q4_1, gb.Q5_1], ids=["q4_0", "q8_0", "q4_1", "q5_1"])
def test_gguf_edges(oracle, type, m, mode, act):
    w, deq, model = _gguf(oracle, type)
    has_min = type in (gb.Q4_1, gb.Q5_1)
    w.set_compute(bestla.COMPUTE_INT8 if mode == "int8" else bestla.COMPUTE_FP)
    try:
        plan = w.plan(m, act)
        xt, xv = _activations(m, GGUF_K, act, seed=type)
        if mode == "int8":
            # the activation quantizer, woq_i8_kernel and, with mins, the min-term pass on the Q8_1 sums
            assert plan["kernel"] == "woq_i8_kernel" and plan["launches"] == (3 if has_min else 2), plan
            prod, tol = model(xv).astype(np.float64), 1e-5
        else:
            assert plan["kernel"] == GGUF_FP_KERNEL[m], plan
            prod, tol = xv.astype(np.float64) @ deq.T, gguf_tol(m, act, w)
        edges.check_forward_matrix(w, xt, prod, tol, f"gguf type={type} {mode} m={m} {act}")
    finally:
        w.set_compute(None)


# ------------------------------------------------------------------------------------------------ fused QKV
def _qkv_windows(m, ns):
    """three output windows of three different strides (n + 5, n + 8, n + 3) in one canary buffer, guard gaps between"""
    lds = [ns[0] + 5, ns[1] + 8, ns[2] + 3]
    gap = 2 * max(lds)
    offs, o = [], gap
    for n, ld in zip(ns, lds):
        offs.append(o)
        o += m * ld + gap
    can = edges.Canary(o)
    wins = [can.window(off, m, n, ld) for off, n, ld in zip(offs, ns, lds)]
    assert len({w.stride(0) for w in wins}) == 3
    return can, wins


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("m", [1, 5, 40])
@pytest.mark.parametrize("kind", ["int8_compute", "q5_1_q8_0_mix", "int4_g128"])
def test_qkv_edges(oracle, knob, kind, m, act):
    tols_odd = None
    if kind == "int4_g128":  # the fp kernels' fused forms: one stream launch at M <= 16, the weights in turn above
        k, ns = 1024, (N, 75, 75)
        made = [_int_weight(oracle, n, k, 128, S4, F16, False, comp=4, seed=i) for i, n in enumerate(ns)]
        ws = [w for _, w in made]
        refs = [lambda a, b=b, n=n: oracle.forward(a, b, n, k).astype(np.float64) for (b, _), n in zip(made, ns)]
        tols = [_path_tol(w.plan(m, act), act) for w in ws]
        knob("NAD_MID_MAX_M", 0)  # rows that are not 16-byte aligned: past the mid-M kernel (test_fp_family_edges)
        tols_odd = [_path_tol(w.plan(m, act), act) for w in ws]
        knob("NAD_MID_MAX_M", None)
        mode = bestla.COMPUTE_FP
    elif kind == "int8_compute":
        k, ns = 300, (N, 75, 75)
        made = [_int_weight(oracle, n, k, 32, S4, F32, i == 1, comp=4) for i, n in enumerate(ns)]
        ws = [w for _, w in made]
        refs = [lambda a, b=b, n=n: oracle.forward_int8(a, b, n, k).astype(np.float64) for (b, _), n in zip(made, ns)]
        tols = [TOL_I8] * 3
        mode = bestla.COMPUTE_INT8
    else:
        k, ns = 256, (72, 40, 72)
        made = [gguf_weight(t, n, k, seed=s) for t, n, s in ((gb.Q5_1, 72, 11), (gb.Q8_0, 40, 12), (gb.Q5_1, 72, 13))]
        ws = [w for _, _, w in made]
        refs = [lambda a, d=d: a.astype(np.float64) @ d.T for _, d, _ in made]
        tols = [gguf_tol(m, act, w) for w in ws]
        mode = bestla.COMPUTE_FP
    for w in ws:
        w.set_compute(mode)
    try:
        if kind == "int8_compute":
            assert all(w.plan(m, act)["kernel"] == "woq_i8_kernel" for w in ws)
        xt, xv = _activations(m, k, act, seed=3)
        for align in edges.ALIGNS:
            x = edges.act_window(xt, align)
            can, wins = _qkv_windows(m, ns)
            what = f"qkv {kind} m={m} {act} {align}"
            ys = edges.twice(can, lambda: bestla.qkv_forward(x, *ws, out=wins), what)
            for i, (y, ref, tol) in enumerate(zip(ys, refs, tols_odd if tols_odd and align == "odd" else tols)):
                prod = ref(xv)
                err = edges.rel_err(y, prod, prod)
                print(f"{what} output {i}: err {err:.3e} bound {tol:.3e}")
                assert err <= tol, (what, i, err, tol)
    finally:
        for w in ws:
            w.set_compute(None)


# ------------------------------------------------------------------------------------------------ FFN gate/up
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("m,with_tmp1", [(3, True), (3, False), (16, False), (40, True)])
def test_ffn_gate_up_edges(oracle, m, with_tmp1, act):
    """tmp2 = silu(x.W1^T) * (x.W3^T) and, when given, tmp1 = silu(x.W1^T): both contiguous [m][fmid] inside one canary
    buffer, x strided.  The bars are test_capi_fused_gpu's for the same intermediates (1e-4 at M <= 16, 1e-3 above)."""
    fin, fmid = 300, N
    (b1, w1), (b3, w3) = (_int_weight(oracle, fmid, fin, 32, S4, F16, False, comp=4, seed=s) for s in (1, 3))
    xt, xv = _activations(m, fin, act, seed=5)
    gate = edges.silu64(oracle.forward(xv, b1, fmid, fin).astype(np.float64))
    ref = gate * oracle.forward(xv, b3, fmid, fin).astype(np.float64)
    tol = 1e-4 if m <= 16 else 1e-3
    for align in edges.ALIGNS:
        x = edges.act_window(xt, align)
        gap = 2 * fmid + 3
        can = edges.Canary(gap + 2 * (m * fmid + gap))
        tmp2 = can.window(gap, m, fmid, fmid)
        tmp1 = can.window(gap + m * fmid + gap, m, fmid, fmid) if with_tmp1 else None
        what = f"ffn_gate_up m={m} tmp1={with_tmp1} {act} {align}"
        ys = edges.twice(can, lambda: bestla.ffn_gate_up(x, w1, w3, act="silu", tmp1=tmp1, tmp2=tmp2), what)
        err = edges.rel_err(ys[0], ref, ref)
        print(f"{what}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (what, err, tol)
        if with_tmp1:
            err1 = edges.rel_err(ys[1], gate, gate)
            print(f"{what} tmp1: err {err1:.3e} bound {tol:.3e}")
            assert err1 <= tol, (what, err1, tol)


# ------------------------------------------------------------------------------------------------ the harness itself
class _Wrong:
    """A stand-in 'weight' (torch arithmetic, no kernel of the library) that breaks one rule of the invariant, to show
    that the harness notices each: the checks above pass because the kernels keep the rules, not because nothing looks."""

    def __init__(self, wt, fault):
        self.wt, self.fault = wt, fault

    def forward(self, x, out, epilogue, bias, residual):
        m, k = x.shape
        n = self.wt.shape[1]
        y = x.float() @ self.wt
        if self.fault == "reads_padding":  # one element past the window's last column
            y = y + x.as_strided((m, 1), (x.stride(0), 1), x.storage_offset() + k).float() * 0
        if self.fault == "accumulates":
            y = torch.where(torch.isnan(out), y, out + y * 1e-3)
        out.copy_(y)
        if self.fault == "skips_element":
            out[m - 1, n - 1] = float("nan")
        if self.fault == "writes_past_n":
            out.as_strided((1, 1), (1, 1), out.storage_offset() + n).fill_(0.0)
        if self.fault == "writes_row_m":
            out.as_strided((1, 1), (1, 1), out.storage_offset() + m * out.stride(0)).fill_(0.0)
        return out


@pytest.mark.parametrize("fault,message", [("writes_past_n", "outside the output window"),
                                           ("writes_row_m", "outside the output window"),
                                           ("skips_element", "NaN element"), ("reads_padding", "NaN element"),
                                           ("accumulates", "differs on a second call"), (None, None)])
def test_harness_notices_each_violation(fault, message):
    m, n, k = 5, 19, 40
    rng = np.random.default_rng(0)
    W = rng.uniform(-0.5, 0.5, size=(k, n)).astype(np.float32)
    xt, xv = _activations(m, k, "fp32")
    prod = xv.astype(np.float64) @ W.astype(np.float64)
    w = _Wrong(torch.from_numpy(W).cuda(), fault)
    for align in edges.ALIGNS:
        if fault is None:
            edges.check_forward_matrix(w, xt, prod, 1e-5, "torch", aligns=(align,), epilogues=("none",))
        else:
            with pytest.raises(AssertionError, match=message):
                edges.check_forward_matrix(w, xt, prod, 1e-5, fault, aligns=(align,), epilogues=("none",))
