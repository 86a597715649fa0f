"""numpy model of the reference's Q8_K activation rows (block_q8_K, neural_speed/core/data_types.h:140-144;
quantize_row_q8_K_reference, vectors/cpu/quantize.h:1020-1055) and of the Q6_K x Q8_K product contract of
woq_q6k_i8_kernel, written from the format and pinned to the reference's outputs by tests/test_q6_k_q8_k_cpu.py.

A block is 292 bytes for 256 activations: float d, int8 qs[256], int16 bsums[16].  max is the signed value of the first
element with the largest |x|, iscale = -128 / max, q = min(127, nearest_int(iscale * x)) with nearest_int the
`+ 12582912.f` rounding (ties to even), d = 1 / iscale, bsums[j] the sum of the codes of group j; an all-zero
superblock is d = 0, codes 0 (and, here, bsums 0).

The product, for activation row r, weight row c and superblock b:
    isum_b = sum_{g < 16} sc[g] * sum_{i < 16} q[16 g + i] * a[16 g + i]       (int64 here, exact)
    y      = sum_b float64(fp32(fp32(d_w[b]) * d_a[r][b])) * isum_b            (float64 here)
"""
import numpy as np

from tests import q6k_blocks as qb

QK_K = 256
BLOCK_BYTES = 292


def quantize(x):
    """fp32 [m][k] -> uint8 [m][k / 256 * 292]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    m, k = x.shape
    assert k % QK_K == 0
    nb = k // QK_K
    xb = x.reshape(m, nb, QK_K)
    first = np.abs(xb).argmax(axis=2)                     # the first occurrence of the largest |x|
    mx = np.take_along_axis(xb, first[:, :, None], axis=2)[:, :, 0]
    zero = mx == 0
    iscale = np.float32(-128) / np.where(zero, np.float32(1), mx)
    assert iscale.dtype == np.float32
    val = iscale[:, :, None] * xb + np.float32(12582912)  # two fp32 roundings: no contraction in numpy
    assert val.dtype == np.float32
    q = np.minimum(127, (val.view(np.int32) & 0x007FFFFF) - 0x00400000)
    q[zero] = 0
    d = np.where(zero, np.float32(0), np.float32(1) / iscale).astype(np.float32)
    bsums = q.reshape(m, nb, 16, 16).sum(axis=3).astype(np.int16)
    out = np.zeros((m, nb, BLOCK_BYTES), np.uint8)
    out[:, :, 0:4] = np.ascontiguousarray(d).reshape(m, nb, 1).view(np.uint8)
    out[:, :, 4:260] = q.astype(np.int8).view(np.uint8)
    out[:, :, 260:292] = np.ascontiguousarray(bsums).view(np.uint8).reshape(m, nb, 32)
    return out.reshape(m, nb * BLOCK_BYTES)


def fields(blocks, m, k):
    """uint8 block bytes -> (d fp32 [m][nb], q int32 [m][nb][256], bsums int32 [m][nb][16])"""
    nb = k // QK_K
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(m, nb, BLOCK_BYTES)
    d = np.ascontiguousarray(b[:, :, 0:4]).view(np.float32).reshape(m, nb)
    q = np.ascontiguousarray(b[:, :, 4:260]).view(np.int8).astype(np.int32)
    bsums = np.ascontiguousarray(b[:, :, 260:292]).view(np.int16).reshape(m, nb, 16).astype(np.int32)
    return d, q, bsums


def isums(q6_blocks, n, k, q8_blocks, m):
    """int64 [m][n][nb]: sum_g sc[g] * (group dot product)"""
    _, sc, q = qb.fields(q6_blocks, n, k)
    _, a, _ = fields(q8_blocks, m, k)
    nb = k // QK_K
    gd = np.einsum("cbgi,rbgi->rcbg", q.reshape(n, nb, 16, 16).astype(np.int64),
                   a.reshape(m, nb, 16, 16).astype(np.int64))
    return (gd * sc.astype(np.int64)[None]).sum(axis=3)


def dot(q6_blocks, n, k, q8_blocks, m):
    """float64 [m][n]: the contract above"""
    dw, _, _ = qb.fields(q6_blocks, n, k)
    da, _, _ = fields(q8_blocks, m, k)
    f = dw.astype(np.float32)[None, :, :] * da[:, None, :]
    assert f.dtype == np.float32
    return (f.astype(np.float64) * isums(q6_blocks, n, k, q8_blocks, m)).sum(axis=2)
