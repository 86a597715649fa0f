"""Weights with known fields, and a bit-exact host model of the fp16 weights woq_gemm7_kernel hands to the MFMA.

gemm7 folds the group scale into its fp16 B operand.  As read from woq_gemm7.hip:

  * scale_h2 turns the stored scale into fp16 once: an fp16 scale is used bit for bit, an fp32 or bf16 one goes through
    `_Float16(float)`, round to nearest even (a bf16's 8 significant bits always fit, so only fp32 scales round here);
  * dq4_core / dq8_core with Fold (woq_device.h) and dequant2_fold build the integer q - zp exactly in fp16 --
    magic-number mantissa tricks whose additions, and the fused multiply-adds by 1/16, 1/4 ..., all stay on integers
    below 2048 -- and multiply it once by that fp16 scale with a packed fp16 multiply: one rounding to nearest even.

So w16 = fp16(fp32(q - zp) * fp32(fp16(s))): the fp32 product of an integer of at most 9 bits and an 11-bit significand
is exact, and its conversion to fp16 is the one rounding of the kernel's multiply.  Every |q - zp| >= 1 times a scale in
[0.001, 0.01] is an fp16 normal, so no subnormal handling enters.  A product of fp16 activations with these weights,
summed in float64, is what the kernel computes up to its fp32 MFMA accumulation: the bar of an exact-input launch
(test_gemm2_gpu TOL["fp16"] = 2e-5 of max|ref|), not FOLD_TOL, which mostly pays for the fold's own rounding.

make() draws the fields so that a misaddressed scale or zero point shows: codes over the whole range (both extremes
included), scales over a decade, zero points over the whole range.
"""
import numpy as np

from tests.oracle_lib import BF16, F16, F32, S2, S4, S8  # noqa: F401  (re-exported for the tests)

BITS = {S4: 4, S2: 2, S8: 8}
S_LO, S_HI = 0.001, 0.01  # within DeviceWeight::fold_ok's range for every |q - zp| <= 255: 2^-14 <= s, 255 s <= 65504


def make(oracle, n, k, bs, qt, st, asym, seed):
    """-> (blob, (Q int8 [k][n], S fp32 [groups][n] as stored, Z int8 [groups][n])): the fields drawn here, packed by
    the oracle for the core orc_select_core(4, ...) gives, and read back from the blob (bf16 / fp16 scale storage
    applied)."""
    bits = BITS[qt]
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1))
    rng = np.random.default_rng(seed)
    ng = -(-k // bs)
    q = rng.integers(lo, hi, size=(k, n)).astype(np.int8)
    q[0, 0], q[-1, -1] = lo, hi - 1  # both extreme codes whatever the draw
    s = rng.uniform(S_LO, S_HI, size=(ng, n)).astype(np.float32)
    z = rng.integers(lo, hi, size=(ng, n)).astype(np.int8) if asym else None
    if asym:  # the largest |q - zp| of the format, both signs
        z[0, 0], z[-1, -1] = hi - 1, lo
    core = oracle.lib.orc_select_core(4, qt, bs, int(asym), 0)
    blob = oracle.pack_q(q, s, z, n, k, bs, qt, st, asym, core)
    Q, S, Z, shf = oracle.unpack_q(blob)
    assert shf is None and np.array_equal(Q, q)
    if asym:
        assert np.array_equal(Z, z)
    else:
        Z = np.zeros_like(Z)
    return blob, (Q, S, Z)


def folded_weights(Q, S, Z, bs):
    """the fp16 [K][N] weights of the folded launch: fp16(q - zp) * fp16(s), one rounding"""
    k = Q.shape[0]
    g = np.arange(k) // bs
    s16 = S.astype(np.float16)  # round to nearest even
    d = Q.astype(np.int32) - Z.astype(np.int32)[g]
    return (d.astype(np.float32) * s16[g].astype(np.float32)).astype(np.float16)


def model_product(x16, w16):
    """float64 product of fp16 activation values [M][K] (any float array holding them) with the folded weights"""
    return np.asarray(x16, dtype=np.float64) @ w16.astype(np.float64)
