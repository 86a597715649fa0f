"""numpy model of GGUF Q6_K (block_q6_K, neural_speed/core/data_types.h:133-138; dequantize_row_q6_K,
vectors/cpu/quantize.h:956-999), pinned bit for bit to the reference's outputs by tests/test_q6_k_cpu.py.

A superblock is 210 bytes for 256 weights: ql[128] (low nibbles), qh[64] (high crumbs), scales[16] (int8, one per 16
weights), d (fp16).  Element e: h = e // 128, j = (e % 128) // 32, l = e % 32; nibble = ql[64 h + 32 (j & 1) + l] (low
half for j < 2, high half otherwise), crumb = (qh[32 h + l] >> 2 j) & 3, q = (nibble | crumb << 4) - 32,
w = (d * scales[e // 16]) * q in fp32 with exactly that association.
"""
import numpy as np

QK_K = 256
BLOCK_BYTES = 210

_E = np.arange(QK_K)
_H, _J, _L = _E // 128, (_E % 128) // 32, _E % 32
_QL_IDX = 64 * _H + 32 * (_J & 1) + _L
_QL_HIGH = _J >= 2
_QH_IDX = 32 * _H + _L
_QH_SHIFT = 2 * _J


def fields(blocks, n, k):
    """uint8 block bytes -> (d fp16 [n][nb], sc int8 [n][nb][16], q int32 [n][nb][256] in -32..31)"""
    nb = k // QK_K
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(n, nb, BLOCK_BYTES)
    ql, qh = b[:, :, :128], b[:, :, 128:192]
    sc = b[:, :, 192:208].view(np.int8)
    d = np.ascontiguousarray(b[:, :, 208:210]).view(np.float16).reshape(n, nb)
    byte = ql[:, :, _QL_IDX].astype(np.int32)
    nib = np.where(_QL_HIGH[None, None, :], byte >> 4, byte & 15)
    crumb = (qh[:, :, _QH_IDX].astype(np.int32) >> _QH_SHIFT[None, None, :]) & 3
    return d, sc.copy(), (nib | (crumb << 4)) - 32


def pack(d, sc, q):
    """the inverse of fields(): -> flat uint8 block bytes"""
    d = np.asarray(d, dtype=np.float16)
    n, nb = d.shape
    v = (np.asarray(q).astype(np.int32) + 32).reshape(n, nb, QK_K)
    assert v.min() >= 0 and v.max() <= 63
    out = np.zeros((n, nb, BLOCK_BYTES), np.uint8)
    for e in range(QK_K):
        out[:, :, _QL_IDX[e]] |= ((v[:, :, e] & 15) << (4 if _QL_HIGH[e] else 0)).astype(np.uint8)
        out[:, :, 128 + _QH_IDX[e]] |= ((v[:, :, e] >> 4) << _QH_SHIFT[e]).astype(np.uint8)
    out[:, :, 192:208] = np.asarray(sc, dtype=np.int8).reshape(n, nb, 16).view(np.uint8)
    out[:, :, 208:210] = d.reshape(n, nb, 1).view(np.uint8)
    return out.ravel()


def dequant(blocks, n, k):
    """fp32 [n][k]: (d * sc) * q, each product rounded to fp32 as dequantize_row_q6_K's `d * sc[is] * q` is"""
    d, sc, q = fields(blocks, n, k)
    ds = d.astype(np.float32)[:, :, None] * sc.astype(np.float32)                       # [n][nb][16], fp32
    w = np.repeat(ds, 16, axis=2) * q.astype(np.float32)
    assert w.dtype == np.float32
    return w.reshape(n, k)


def random_blocks(n, k, seed):
    """any bytes are valid Q6_K: ql / qh uniform, sc over the full int8 range, d in 1e-4 .. 1e-2"""
    rng = np.random.default_rng(seed)
    nb = k // QK_K
    out = rng.integers(0, 256, size=(n, nb, BLOCK_BYTES), dtype=np.uint8)
    d = rng.uniform(1e-4, 1e-2, size=(n, nb)).astype(np.float16)
    out[:, :, 208:210] = d.reshape(n, nb, 1).view(np.uint8)
    return out.ravel()
