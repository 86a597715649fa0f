"""The exact host model of what woq_mid_kernel multiplies (the weights come from fold_model.make).

The mid-M kernel does not fold the group scale.  As read from woq_gemm_mid.hip:

  * dq4 / dequant2_step build the integer q - zp exactly in fp16 -- the 0x6400 magic-number steps, their additions and
    the fused multiply-adds by 1/16 all stay on integers below 2048 -- and that integer is the MFMA's weight operand;
  * each group's fp32 partial is multiplied by the stored scale in fp32 (scale4: an fp32 scale bit for bit, a bf16 /
    fp16 one widened exactly) and added to the stripe's fp32 sum;
  * fp16 activations enter bit for bit (a_frag<kActF16>); fp32 / bf16 activations enter as two fp16 rows, hi =
    fp16(a), lo = fp16(a - float(hi)), both conversions round to nearest even and keep fp16 subnormals (lo of an
    activation near 2^-3 already is one), one MFMA each into the same group partial.

So, in float64,

    ref[m][n] = sum_g S[g][n] * sum_{k in g} (hi + lo)[m][k] * (Q - Z[g])[k][n]

with S as stored (read back from the blob); float64 holds every activation-times-integer product and every (q - zp) * s
exactly and rounds the sums at 2^-53.  What separates the kernel from it is fp32 accumulation only (the MFMA's
sums within a group, the scaled partials across groups, waves and K runs): the bar of an exact-input launch,
test_mid_gpu TOL = 2e-5 of max|ref|.  numpy's float16 conversion rounds to nearest even and keeps subnormals, as the
kernel's does.
"""
import numpy as np


def round_act(A, act):
    """fp32 values -> the values an activation tensor of type `act` holds, as fp32 (round to nearest even)"""
    A = np.ascontiguousarray(A, dtype=np.float32)
    if act == "fp32":
        return A
    if act == "fp16":
        return A.astype(np.float16).astype(np.float32)
    assert act == "bf16", act
    u = A.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000  # finite values only
    return u.astype(np.uint32).view(np.float32)


def hi_lo(x32):
    """the two fp16 rows the kernel makes of fp32 / bf16 activations (a_frag): hi = fp16(a), lo = fp16(a - hi)"""
    x32 = np.asarray(x32, dtype=np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)  # the fp32 difference is exact
    return hi, lo


def split_hi_lo(x32):
    """-> hi + lo as float64 [M][K]: the activation values that reach the MFMAs (fp16 values come back unchanged)"""
    hi, lo = hi_lo(x32)
    return hi.astype(np.float64) + lo.astype(np.float64)


def group_index(k, bs):
    return np.arange(k) // bs


def product(x_eff, Q, S, Z, bs):
    """the model: float64 [M][N] = sum over groups of S[g] * (x_eff[:, g] @ (Q - Z[g])[g]); Z all zero when sym"""
    g = group_index(Q.shape[0], bs)
    d = (Q.astype(np.int32) - Z.astype(np.int32)[g]).astype(np.float64)
    return np.asarray(x_eff, dtype=np.float64) @ (d * S.astype(np.float64)[g])  # d * S is exact in float64


def product_f32(x32, Q, S, Z, bs):
    """The same operands in the kernel's precision, float32 numpy: per group the hi and the lo product, the partial
    times the scale, the groups summed in order.  (Not the kernel's summation order -- that of a plain float32
    restatement: what fp32 accumulation costs against the float64 model.)"""
    k = Q.shape[0]
    hi, lo = hi_lo(x32)
    hi, lo = hi.astype(np.float32), lo.astype(np.float32)
    acc = np.zeros((hi.shape[0], Q.shape[1]), np.float32)
    for gi, k0 in enumerate(range(0, k, bs)):
        k1 = min(k, k0 + bs)
        d = (Q[k0:k1].astype(np.int32) - Z[gi].astype(np.int32)).astype(np.float32)
        part = hi[:, k0:k1] @ d + lo[:, k0:k1] @ d
        acc += part * S[gi].astype(np.float32)
    assert acc.dtype == np.float32
    return acc
