"""numpy model of the GGUF legacy block types Q4_1 / Q5_0 / Q5_1 / Q8_0 and of the Q8_0 / Q8_1 activation blocks
(neural_speed/core/data_types.h:79-118, vectors/cpu/quantize.h:284-445, 546-579, 706-796, core/layers/vec_dot.h scalar
loops).  tests/test_gguf_types_cpu.py pins every function here to the reference's own outputs (tests/golden/gguf_types),
so the GPU tests may use them at shapes the fixtures do not cover.

Block layouts (little endian), element j < 16 in the low nibble of qs[j], element j + 16 in the high nibble; bit j of
the u32 qh is the fifth bit of element j:
  Q4_1  fp16 d, fp16 m, u8 qs[16]             w = q d + m, q in 0..15
  Q5_0  fp16 d, u8 qh[4], u8 qs[16]           w = (q - 16) d, q in 0..31
  Q5_1  fp16 d, fp16 m, u8 qh[4], u8 qs[16]   w = q d + m, q in 0..31
  Q8_0  fp16 d, i8 qs[32]                     w = q d
  Q8_1  f32 d, f32 s, i8 qs[32]               activations: s = sum(q) d
"""
import numpy as np

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34}
HAS_MIN = {Q4_1: True, Q5_0: False, Q5_1: True, Q8_0: False}
QMAX = {Q4_1: 15, Q5_1: 31}
NAMES = {Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0"}
ACT_BLOCKS = {Q4_1: "y_q8_1", Q5_0: "y_q8_0", Q5_1: "y_q8_1", Q8_0: "y_q8_0"}  # the type's vec_dot_type


def _roundf(v):
    """C roundf (half away from zero) of fp32 values, exact: the + 0.5 is done in fp64"""
    v = v.astype(np.float64)
    return np.trunc(v + np.copysign(0.5, v))


def pack(type, d, q, m=None):
    """blocks from their fields: d (and m) [n][nb] fp16, q [n][nb][32] the STORED integers (Q4_1 0..15, Q5_0 / Q5_1
    0..31, Q8_0 -128..127) -> uint8 [n * nb * block bytes]"""
    d = np.asarray(d, np.float16)
    n, nb = d.shape
    q = np.asarray(q).reshape(n, nb, 32)
    out = np.zeros((n, nb, BLOCK_BYTES[type]), np.uint8)
    out[:, :, 0:2] = d.view(np.uint8).reshape(n, nb, 2)
    o = 2
    if HAS_MIN[type]:
        out[:, :, 2:4] = np.asarray(m, np.float16).view(np.uint8).reshape(n, nb, 2)
        o = 4
    if type == Q8_0:
        out[:, :, 2:34] = q.astype(np.int8).view(np.uint8)
        return out.ravel()
    u = q.astype(np.uint32)
    if type in (Q5_0, Q5_1):
        qh = (((u >> 4) & 1) << np.arange(32, dtype=np.uint32)).sum(axis=2).astype(np.uint32)
        out[:, :, o:o + 4] = qh.astype("<u4").view(np.uint8).reshape(n, nb, 4)
        o += 4
    out[:, :, o:o + 16] = ((u[:, :, :16] & 15) | ((u[:, :, 16:] & 15) << 4)).astype(np.uint8)
    return out.ravel()


def fields(type, blocks, n, k):
    """-> d fp32 [n][nb], m fp32 [n][nb] (zeros without a min), q int32 [n][nb][32] with w = q d + m (Q5_0: q - 16)"""
    nb = k // 32
    b = np.asarray(blocks, np.uint8).reshape(n, nb, BLOCK_BYTES[type])
    d = b[:, :, 0:2].copy().view(np.float16).reshape(n, nb).astype(np.float32)
    m = np.zeros((n, nb), np.float32)
    o = 2
    if HAS_MIN[type]:
        m = b[:, :, 2:4].copy().view(np.float16).reshape(n, nb).astype(np.float32)
        o = 4
    if type == Q8_0:
        return d, m, b[:, :, 2:34].copy().view(np.int8).astype(np.int32)
    hi = np.zeros((n, nb, 32), np.int32)
    if type in (Q5_0, Q5_1):
        qh = b[:, :, o:o + 4].copy().view("<u4").reshape(n, nb, 1)
        hi = ((qh >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int32) << 4
        o += 4
    qs = b[:, :, o:o + 16].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=2) | hi
    if type == Q5_0:
        q = q - 16
    return d, m, q


def dequant(type, blocks, n, k):
    """dequantize_row_*: fp32 [n][k], each value q d + m rounded to fp32 once (q d is exact)"""
    d, m, q = fields(type, blocks, n, k)
    w = q.astype(np.float32) * d[:, :, None]
    if HAS_MIN[type]:  # not otherwise: a zero block of Q5_0 has d = -0 and dequantizes to -0
        w = w + m[:, :, None]
    return w.astype(np.float32).reshape(n, k)


def quantize(type, w):
    """An fp32 [n][k] matrix -> blocks, after the algorithm of quantize_row_*_reference.  NOT pinned to the reference's
    bytes (the fixtures hold no W): it only generates valid blocks for the larger GPU cases, whose expected values
    come from dequant() / forward_int() of these same blocks; the CPU test checks that the blocks track W."""
    w = np.ascontiguousarray(w, np.float32)
    n, k = w.shape
    x = w.reshape(n, k // 32, 32)
    one = np.float32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if type == Q8_0:
            d = (np.abs(x).max(axis=2) / np.float32(127)).astype(np.float32)
            idv = np.where(d != 0, one / d, np.float32(0)).astype(np.float32)
            return pack(type, d.astype(np.float16), _roundf(x * idv[:, :, None]))
        if type == Q5_0:
            i = np.abs(x).argmax(axis=2)  # first largest |v|: the reference replaces on a strict >
            mx = np.take_along_axis(x, i[:, :, None], axis=2)[:, :, 0]
            d = (mx / np.float32(-16)).astype(np.float32)
            idv = np.where(d != 0, one / d, np.float32(0)).astype(np.float32)
            q = np.minimum(31, np.trunc(x * idv[:, :, None] + np.float32(16.5)).astype(np.int32).astype(np.int8))
            return pack(type, d.astype(np.float16), q)
        qm = QMAX[type]
        mn, mx = x.min(axis=2), x.max(axis=2)
        d = ((mx - mn) / np.float32(qm)).astype(np.float32)
        idv = np.where(d != 0, one / d, np.float32(0)).astype(np.float32)
        q = np.trunc((x - mn[:, :, None]) * idv[:, :, None] + np.float32(0.5)).astype(np.int32)
        return pack(type, d.astype(np.float16), np.minimum(qm, q), mn.astype(np.float16))


def quant_q8_0(a):
    """quantize_row_q8_0_reference: fp32 [m][k] -> uint8 [m * k/32 * 34]"""
    a = np.ascontiguousarray(a, np.float32)
    m, k = a.shape
    x = a.reshape(m, k // 32, 32)
    d = (np.abs(x).max(axis=2) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    return pack(Q8_0, d.astype(np.float16), _roundf(x * idv[:, :, None]))


def quant_q8_1(a):
    """quantize_row_q8_1_reference: fp32 [m][k] -> uint8 [m * k/32 * 40] blocks {f32 d, f32 s, i8 qs[32]}"""
    a = np.ascontiguousarray(a, np.float32)
    m, k = a.shape
    nb = k // 32
    x = a.reshape(m, nb, 32)
    d = (np.abs(x).max(axis=2) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    q = _roundf(x * idv[:, :, None]).astype(np.int32)
    s = (q.sum(axis=2).astype(np.float32) * d).astype(np.float32)
    out = np.zeros((m, nb, 40), np.uint8)
    out[:, :, 0:4] = d.astype("<f4").view(np.uint8).reshape(m, nb, 4)
    out[:, :, 4:8] = s.astype("<f4").view(np.uint8).reshape(m, nb, 4)
    out[:, :, 8:40] = q.astype(np.int8).view(np.uint8)
    return out.ravel()


def act_fields(name, blocks, m, k):
    """Q8_0 / Q8_1 activation blocks -> d fp32 [m][nb], s fp32 [m][nb] (zeros for Q8_0), q int32 [m][nb][32]"""
    nb = k // 32
    if name == "y_q8_0":
        d, s, q = fields(Q8_0, blocks, m, k)
        return d, s, q
    b = np.asarray(blocks, np.uint8).reshape(m, nb, 40)
    d = b[:, :, 0:4].copy().view("<f4").reshape(m, nb)
    s = b[:, :, 4:8].copy().view("<f4").reshape(m, nb)
    return d, s, b[:, :, 8:40].copy().view(np.int8).astype(np.int32)


def forward_int(type, blocks, n, k, a):
    """ne_vec_dot_<type>_<q8_0 | q8_1> for every (row of a, row of the matrix): the activations quantized to the
    type's vec_dot_type, integer block dots, the scalar loops' fp32 sums in block order -> fp32 [m][n]"""
    a = np.ascontiguousarray(a, np.float32)
    m = a.shape[0]
    name = ACT_BLOCKS[type]
    da, sa, qa = act_fields(name, quant_q8_0(a) if name == "y_q8_0" else quant_q8_1(a), m, k)
    dw, mw, qw = fields(type, blocks, n, k)
    sumf = np.zeros((m, n), np.float32)
    for b in range(k // 32):
        sumi = (qa[:, b, :].astype(np.int64) @ qw[:, b, :].astype(np.int64).T).astype(np.float32)  # |sumi| < 2^24
        t = (da[:, b, None] * dw[None, :, b]).astype(np.float32) * sumi
        if HAS_MIN[type]:
            t = t.astype(np.float32) + (mw[None, :, b] * sa[:, b, None]).astype(np.float32)
        sumf = (sumf + t.astype(np.float32)).astype(np.float32)
    return sumf
