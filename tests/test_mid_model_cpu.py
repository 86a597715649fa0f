"""The mid-M model (tests/mid_model.py) pinned without a GPU, on the shapes of tests/test_mid_matrix_gpu.py (N = 203,
K = 9 K tiles + 40, the 61 rows every launch there takes its first M of):

  (a) the model against the oracle on the same activation values sits inside TOL of test_mid_gpu (2e-5 of max|ref|),
      the bar the existing GPU tests already hold the kernel to against the oracle -- it differs from the oracle by the
      rounding of lo (2^-22 of an activation at most) and the oracle's fp32 (q - zp) * s (2^-24);
  (b) what the bar has to cover: the float32-numpy product of the model's operands (per group the hi and the lo
      product, scaled, summed in float32) against the float64 model, at most 2e-5;
  (c) the drawn fields do their job: a scale or a zero point taken from the neighbouring column or group moves the
      product by more than 1000 bars;

and the geometry table of the GPU matrix against the host's dry-run plan (nad_plan_forward needs no GPU), so that a
table that no longer matches mid_geometry shows on a machine without one.  The figures printed here are recorded in
profiles/mid_matrix_errors.txt."""
import numpy as np
import pytest

from tests import fold_model as fm
from tests import mid_model as mm
from tests.fold_model import BF16, F16, F32
from tests.test_mid_matrix_gpu import (ACTS, BAR, FORMATS, GEOMETRY, K_TILE, M_MAX, M_OF_RF, N, NS, ST_NAME, VARIANTS,
                                       act_values, geometries, gpt_of, variant_k)

CASES = [(qt, bs, asym, st) for qt, bs in FORMATS for asym in (False, True) for st in (F32, BF16, F16)]


def rel(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


def test_round_act_and_split():
    """round_act is torch's rounding (so the GPU tensors hold the model's values), and hi + lo is the activation to
    2^-22: fp16 and (away from the subnormals) bf16 values come back unchanged."""
    import torch
    A = np.random.default_rng(0).uniform(-0.5, 0.5, size=(M_MAX, 1192)).astype(np.float32)
    A[0, :4] = [0.0, 2.0 ** -20, -3.0 * 2.0 ** -24, 0.49999997]
    t = torch.from_numpy(A)
    assert np.array_equal(mm.round_act(A, "fp16"), t.half().float().numpy())
    assert np.array_equal(mm.round_act(A, "bf16"), t.bfloat16().float().numpy())
    assert mm.round_act(A, "fp32") is A or np.array_equal(mm.round_act(A, "fp32"), A)
    x16 = mm.round_act(A, "fp16")
    assert np.array_equal(mm.split_hi_lo(x16), x16.astype(np.float64))
    hi, lo = mm.hi_lo(A)
    assert hi.dtype == lo.dtype == np.float16
    assert np.array_equal(hi, A.astype(np.float16))
    eff = mm.split_hi_lo(A)
    assert eff.dtype == np.float64
    # lo is the fp32 difference rounded once to fp16: half an ulp of lo, itself at most half an ulp of hi
    assert np.abs(eff - A).max() <= 2.0 ** -22 * np.abs(A).max() + 2.0 ** -25
    big = np.abs(mm.round_act(A, "bf16")) >= 2.0 ** -14
    assert np.array_equal(mm.split_hi_lo(mm.round_act(A, "bf16"))[big], mm.round_act(A, "bf16").astype(np.float64)[big])


@pytest.mark.parametrize("qt,bs,asym,st", CASES,
                         ids=[f"int{fm.BITS[q]}_g{b}_{'asym' if a else 'sym'}_{ST_NAME[s]}" for q, b, a, s in CASES])
def test_mid_model_against_the_oracle(oracle, qt, bs, asym, st):
    k = variant_k(qt)
    bits = fm.BITS[qt]
    blob, (Q, S, Z) = fm.make(oracle, N, k, bs, qt, st, asym, seed=k + bs)
    ng = -(-k // bs)
    assert Q.shape == (k, N) and S.shape == Z.shape == (ng, N) and ng >= 10
    assert Q.min() == -(1 << (bits - 1)) and Q.max() == (1 << (bits - 1)) - 1
    assert fm.S_LO * 0.99 <= S.min() and S.max() <= fm.S_HI * 1.01 and S.max() / S.min() > 5
    d = Q.astype(np.int32) - Z.astype(np.int32)[mm.group_index(k, bs)]
    if asym:
        assert d.max() == (1 << bits) - 1 and d.min() == -((1 << bits) - 1)
    else:
        assert not Z.any()
    assert np.array_equal(oracle.unpack_fp32(blob), d.astype(np.float32) * S[mm.group_index(k, bs)])  # the blob's
    name = f"int{bits} g{bs} {'asym' if asym else 'sym'} {ST_NAME[st]} K={k}"
    for act in ACTS:
        xv = act_values(k, act)
        ref = oracle.forward(xv, blob, N, k).astype(np.float64)
        prod = mm.product(mm.split_hi_lo(xv), Q, S, Z, bs)
        dist = rel(prod, ref)                                   # (a)
        acc = rel(mm.product_f32(xv, Q, S, Z, bs), prod)        # (b)
        print(f"{name} {act} rows: model vs oracle {dist:.3e} (bar {BAR:.0e}), float32 vs float64 product of the "
              f"model {acc:.3e} (bar {BAR:.0e})")
        assert dist <= BAR, dist
        assert acc <= BAR, acc
    # (c) on the fp32 rows' product: the scale of the neighbouring column / group, the zero point of the neighbouring
    # group / column
    x_eff = mm.split_hi_lo(act_values(k, "fp32"))
    prod = mm.product(x_eff, Q, S, Z, bs)
    wrong = {"S column": mm.product(x_eff, Q, np.roll(S, 1, axis=1), Z, bs),
             "S group": mm.product(x_eff, Q, np.roll(S, 1, axis=0), Z, bs)}
    if asym:
        wrong["Z group"] = mm.product(x_eff, Q, S, np.roll(Z, 1, axis=0), bs)
        wrong["Z column"] = mm.product(x_eff, Q, S, np.roll(Z, 1, axis=1), bs)
    moved = {what: rel(p, prod) for what, p in wrong.items()}
    print(f"    {name}: misaddressed by one: " + ", ".join(f"{what} {v:.2e}" for what, v in moved.items()))
    assert min(moved.values()) > 1000 * BAR, moved


def test_mid_geometry_table_matches_the_plan(knob):
    """Every row of the GPU matrix's literal table, and the two gates, against the host's dry run of the same launch."""
    from neural_amd import bestla
    knob("NAD_MID_XCD", None)
    seen = set()
    for qt, bs in FORMATS:
        bits, k = fm.BITS[qt], variant_k(qt)
        assert -(-k // K_TILE[qt]) == 10 and k % 8 == 0 and k % 32 == 8
        for act in ACTS:
            for wide, rf, s, nw, spw in geometries(qt, bs, act):
                knob("NAD_MID_WIDE", wide)
                for asym in (False, True):
                    for st in ("fp32", "bf16", "fp16"):
                        for ks in VARIANTS.values():
                            knob("NAD_MID_KS", ks)
                            plan = bestla.plan_forward(bits, N, k, bs, st, asym, M_OF_RF[rf], act)
                            want = dict(kernel="woq_mid_kernel", fold=False, threads=nw * 64, grid=-(-NS // s) * ks,
                                        ksplit=ks, launches=1 if ks == 1 else 2)
                            assert {key: plan[key] for key in want} == want, (bits, bs, act, wide, rf, plan, want)
                seen.add((bits, gpt_of(qt, bs), act, rf, s, nw, spw))
        if bits == 2 or bs == 32:
            knob("NAD_MID_WIDE", 0)
            for act in ACTS:
                assert bestla.plan_forward(bits, N, k, bs, "fp16", True, M_OF_RF[3], act)["kernel"] != "woq_mid_kernel"
    assert len(seen) == 60 and sum(len(row[2]) * len(row[4]) for row in GEOMETRY) == 60


def test_more_than_four_row_fragments_are_declined(knob):
    """NAD_MID_MAX_M above 64 does not stretch the kernel: it has shapes for 4 row fragments (M <= 64), so the host's
    dry run sends M = 65 and 80 to another kernel, and M = 64 still to this one."""
    from neural_amd import bestla
    knob("NAD_MID_MAX_M", 80)
    for qt, bs in [(fm.S4, 128), (fm.S4, 64)]:
        k = variant_k(qt)
        for act in ACTS:
            for asym in (False, True):
                assert bestla.plan_forward(4, N, k, bs, "fp16", asym, 64, act)["kernel"] == "woq_mid_kernel"
                for m in (65, 80):
                    assert bestla.plan_forward(4, N, k, bs, "fp16", asym, m, act)["kernel"] != "woq_mid_kernel", (bs, m)
