"""The fold model (tests/fold_model.py) against the oracle, no GPU: the model's fp16 weights are the reference's
dequantized weights rounded twice, its product sits inside the bar the suite already holds folded launches to
(FOLD_TOL), and for fp32 scales it sits further from the oracle than TOL["fp16"] -- the distance the old bar spends on
the fold itself and the new bar (the kernel against the model at TOL["fp16"], tests/test_gemm7_matrix_gpu.py) resolves.

Shapes are the GPU matrix's: M = 130, N = 203, K = 300 and the seven-K-tile K of the format.  The figures printed here
are recorded in profiles/gemm7_matrix_errors.txt."""
import numpy as np
import pytest

from tests import fold_model as fm
from tests.fold_model import BF16, F16, F32, S2, S4, S8
from tests.test_gemm2_gpu import FOLD_TOL, TOL

M, N = 130, 203
SPLIT_K = {S4: 896, S2: 1792, S8: 448}
ST_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
# one group size per format, as the oracle's dequantization does not depend on it
CASES = [(qt, bs, asym, st) for qt, bs in ((S4, 128), (S2, 64), (S8, 32)) for asym in (False, True)
         for st in (F32, BF16, F16)]


def activations(m, k, seed):
    """fp16 values (as fp32) drawn as the GPU matrix draws them"""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=(m, k)).astype(np.float16).astype(np.float32)


def rel(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("qt,bs,asym,st", CASES,
                         ids=[f"int{fm.BITS[q]}_g{b}_{'asym' if a else 'sym'}_{ST_NAME[s]}" for q, b, a, s in CASES])
def test_fold_model_against_the_oracle(oracle, qt, bs, asym, st):
    for k in (300, SPLIT_K[qt]):
        blob, (Q, S, Z) = fm.make(oracle, N, k, bs, qt, st, asym, seed=k + bs)
        bits = fm.BITS[qt]
        assert Q.min() == -(1 << (bits - 1)) and Q.max() == (1 << (bits - 1)) - 1
        assert fm.S_LO * 0.99 <= S.min() and S.max() <= fm.S_HI * 1.01 and S.max() / S.min() > 5
        d = Q.astype(np.int32) - Z.astype(np.int32)[np.arange(k) // bs]
        if asym:
            assert d.max() == (1 << bits) - 1 and d.min() == -((1 << bits) - 1)
        w16 = fm.folded_weights(Q, S, Z, bs)
        assert w16.dtype == np.float16 and w16.shape == (k, N)
        # (a) two roundings to nearest even of 2^-11 each (the scale, the product) from the reference's weights
        # (W itself carries the fp32 rounding of (q - zp) * s, 2^-24: inside the 2^-22 the bound leaves over)
        W32 = oracle.unpack_fp32(blob)
        assert np.array_equal(W32, d.astype(np.float32) * S[np.arange(k) // bs])  # the fields are the blob's
        W = W32.astype(np.float64)
        excess = np.abs(w16.astype(np.float64) - W) - (2.0 ** -10 + 2.0 ** -21) * np.abs(W)
        assert excess.max() <= 0, excess.max()
        # (b) the model is consistent with the bar folded launches are held to today
        x = activations(M, k, seed=k)
        ref = oracle.forward(x, blob, N, k).astype(np.float64)
        prod = fm.model_product(x, w16)
        dist = rel(prod, ref)
        # (c) what fp32 accumulation itself costs: float32 numpy against float64 on the same fp16 operands
        acc = rel(x @ w16.astype(np.float32), prod)
        print(f"int{bits} g{bs} {'asym' if asym else 'sym'} {ST_NAME[st]} K={k}: model vs oracle {dist:.3e} "
              f"(FOLD_TOL {FOLD_TOL:.0e}), float32 vs float64 product of the model {acc:.3e} (bar {TOL['fp16']:.0e})")
        assert dist <= FOLD_TOL, dist
        assert acc <= TOL["fp16"], acc
        if st == F32:
            assert dist > TOL["fp16"], dist
        # what the drawn fields are for: the scale of the neighbouring column, or the zero point of the neighbouring
        # group, is an error no bar could hide
        wrong = [rel(fm.model_product(x, fm.folded_weights(Q, np.roll(S, 1, axis=1), Z, bs)), prod)]
        if asym:
            wrong.append(rel(fm.model_product(x, fm.folded_weights(Q, S, np.roll(Z, 1, axis=0), bs)), prod))
        print("    a misaddressed scale / zero point: " + " ".join(f"{v:.2e}" for v in wrong))
        assert min(wrong) > 1000 * TOL["fp16"], wrong
