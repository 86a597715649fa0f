"""GGUF Q6_K in the reference's Q8_K arithmetic without a GPU: tests/q8k_blocks.py (the numpy model the GPU tests use
at larger shapes) pinned to the reference's own quantize_row_q8_K_reference and ggml_vec_dot_q6_K_q8_K outputs in
tests/golden/q6_k_q8_k (tools/q6_k_q8_k_golden.c), and the argument checks of nad_quant_q8_k."""
import ctypes as C

import numpy as np
import pytest

from neural_amd import _lib, bestla
from tests import q8k_blocks as q8
from tests.oracle_lib import load_ref_golden

QUANT = ["quant_uniform_k256", "quant_uniform_k768", "quant_zero_sb", "quant_plus_first", "quant_minus_first",
         "quant_ties", "quant_amp_1em3", "quant_amp_1e3"]
DOT = ["dot_n40_k256_m5", "dot_n16_k768_m3"]
DOT_TOL = 1e-6  # fp32 summation of at most 3 superblocks; the integer part is exact


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("q6_k_q8_k")


def test_the_fixtures_hold_the_listed_cases(golden):
    assert sorted(golden) == sorted(QUANT + DOT)


@pytest.mark.parametrize("case", QUANT + DOT)
def test_quantizer_model_bit_exact(golden, case):
    g = golden[case]
    m, k = int(g["meta"][-1]) if case in DOT else int(g["meta"][0]), int(g["meta"][1])
    x = g["x"].reshape(m, k)
    assert g["q8_k"].size == m * (k // 256) * q8.BLOCK_BYTES
    assert np.array_equal(q8.quantize(x).ravel(), g["q8_k"])


def test_fixture_cases_cover_what_they_are_for(golden):
    d, q, _ = q8.fields(golden["quant_plus_first"]["q8_k"], 2, 256)
    assert (d < 0).all() and q[0, 0, 17] == -128 and q[0, 0, 101] == 127       # max = +a: iscale < 0, -a clamps
    d, q, _ = q8.fields(golden["quant_minus_first"]["q8_k"], 2, 256)
    assert (d > 0).all() and q[0, 0, 17] == -128 and q[0, 0, 101] == 127
    d, q, bs = q8.fields(golden["quant_zero_sb"]["q8_k"], 2, 768)
    assert d[0, 1] == 0 and not q[0, 1].any() and not bs[0, 1].any() and not d[1].any() and d[0, 0] != 0
    d, q, _ = q8.fields(golden["quant_ties"]["q8_k"], 2, 256)
    x = golden["quant_ties"]["x"].reshape(2, 256)
    assert (d == 1).all() and np.array_equal(q.reshape(2, 256), np.minimum(127, np.rint(x)).astype(np.int32))
    assert (np.abs(x - np.trunc(x)) == 0.5).sum() == 2 * 255
    d, q, bs = q8.fields(golden["dot_n40_k256_m5"]["q8_k"], 5, 256)
    assert set(np.unique(q[0, 0])) == {-128, 127}
    assert np.array_equal(bs, q.reshape(5, 1, 16, 16).sum(axis=3))


@pytest.mark.parametrize("case", DOT)
def test_dot_model_against_the_reference(golden, case):
    g = golden[case]
    n, k, m = (int(v) for v in g["meta"])
    y = g["y"].reshape(m, n).astype(np.float64)
    model = q8.dot(g["q6_k"], n, k, g["q8_k"], m)
    isum = q8.isums(g["q6_k"], n, k, g["q8_k"], m)
    assert np.abs(isum).max() <= 2 ** 27
    err = float(np.abs(model - y).max() / np.abs(y).max())
    print(f"{case}: model vs ggml_vec_dot_q6_K_q8_K rel_err={err:.3e} max|isum|={np.abs(isum).max()}")
    assert err <= DOT_TOL


def test_entry_is_exported_and_constants():
    assert "nad_quant_q8_k" in _lib.header_symbols()
    assert hasattr(_lib.lib(), "nad_quant_q8_k")
    assert bestla.COMPUTE_Q8_K == 2
    assert bestla.KERNELS[13] == "woq_q6k_i8_kernel"


@pytest.mark.parametrize("m,k", [(1, 384), (0, 256)])
def test_quant_q8_k_refuses_bad_arguments_without_a_gpu(m, k):
    L = _lib.lib()
    x = np.zeros((1, 512), np.float32)
    out = np.zeros(2 * q8.BLOCK_BYTES, np.uint8)
    px, po = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    L.nad_clear_error()
    assert L.nad_quant_q8_k(px, 0, m, k, 512, po, None) == -1
    assert "Q8_K" in _lib.last_error()
    L.nad_clear_error()
    assert L.nad_quant_q8_k(None, 0, 1, 256, 512, po, None) == -1
    assert "Q8_K" in _lib.last_error()
    L.nad_clear_error()
    assert not out.any()
