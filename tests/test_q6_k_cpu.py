"""GGUF Q6_K without a GPU: tests/q6k_blocks.py (the numpy model the GPU tests use at larger shapes) pinned bit for bit
to the reference's own dequantize_row_q6_K outputs in tests/golden/q6_k (tools/q6_k_golden.c), and the size entry of
the C ABI held to the file's byte count."""
import numpy as np
import pytest

from neural_amd import _lib, bestla
from tests import q6k_blocks as qb
from tests.oracle_lib import load_ref_golden

CASES = ["n40_k256", "n16_k768", "ext_n16_k512"]


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("q6_k")


@pytest.mark.parametrize("case", CASES)
def test_dequant_bit_exact(golden, case):
    g = golden[case]
    n, k = (int(v) for v in g["meta"])
    blocks = g["q6_k"]
    assert blocks.size == n * (k // 256) * qb.BLOCK_BYTES
    deq = qb.dequant(blocks, n, k)
    assert deq.dtype == np.float32
    assert np.array_equal(deq.view(np.uint32), g["deq"].reshape(n, k).view(np.uint32))


@pytest.mark.parametrize("case", CASES)
def test_pack_inverts_fields(golden, case):
    g = golden[case]
    n, k = (int(v) for v in g["meta"])
    d, sc, q = qb.fields(g["q6_k"], n, k)
    assert q.min() >= -32 and q.max() <= 31
    assert np.array_equal(qb.pack(d, sc, q), g["q6_k"])


def test_ext_case_covers_the_extremes(golden):
    """what the hand-written case is for: q = -32 and 31 under sc = 127 and -128 (|sc q| past fp16's exact integers),
    sc = 0, a d = 0 block and subnormal fp16 d"""
    g = golden["ext_n16_k512"]
    d, sc, q = qb.fields(g["q6_k"], 16, 512)
    prod = np.abs(np.repeat(sc.astype(np.int32), 16, axis=2) * q)
    assert prod.max() == 4096 and (prod == 31 * 127).any()
    assert sc.min() == -128 and sc.max() == 127 and (sc == 0).any()
    dbits = d.view(np.uint16)
    assert (dbits == 0).any() and (dbits == 1).any() and (dbits == 0x8155).any()


def test_random_blocks_are_full_range():
    blocks = qb.random_blocks(16, 512, seed=3)
    d, sc, q = qb.fields(blocks, 16, 512)
    assert (q.min(), q.max()) == (-32, 31) and (sc.min(), sc.max()) == (-128, 127)
    assert 1e-4 * 0.99 <= float(d.min()) and float(d.max()) <= 1e-2 * 1.01
    assert np.array_equal(qb.pack(d, sc, q), blocks)


@pytest.mark.parametrize("n,k", [(40, 256), (16, 768), (32000, 4096)])
def test_device_size_is_the_files_byte_count(n, k):
    """6 bits per quant, int8 sub-scales, fp16 d: 210 bytes per 256 weights of the stripe-padded matrix, plus alignment"""
    size = _lib.lib().nad_q6_k_device_size(n, k)
    bound = (n + 15) // 16 * 16 * (k // 256) * 210 + 5 * 256
    print(f"n={n} k={k} device bytes {size} bound {bound}")
    assert 0 < size <= bound
    assert size >= (n + 15) // 16 * 16 * (k // 256) * 210


@pytest.mark.parametrize("n,k", [(40, 128), (0, 256), (40, 0), (40, 384)])
def test_device_size_refuses_bad_shapes(n, k):
    L = _lib.lib()
    L.nad_clear_error()
    assert L.nad_q6_k_device_size(n, k) == 0
    assert "Q6_K" in _lib.last_error()
    L.nad_clear_error()


def test_constants_and_the_legacy_entries_still_refuse_14():
    assert bestla.GGUF_Q6_K == 14
    assert bestla.KERNELS[11] == "woq_q6k_gemv_kernel" and bestla.KERNELS[12] == "woq_q6k_gemm_kernel"
    L = _lib.lib()
    L.nad_clear_error()
    assert L.nad_gguf_block_bytes(14) == 0
    assert "14" in _lib.last_error() and "nad_q6_k_device_load" in _lib.last_error()
    L.nad_clear_error()
