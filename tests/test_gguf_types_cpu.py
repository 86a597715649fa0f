"""GGUF Q4_1 / Q5_0 / Q5_1 / Q8_0 without a GPU: the size / type entries of the C ABI, and tests/gguf_blocks.py (the
numpy model the GPU tests use at larger shapes) pinned to the reference's own outputs in tests/golden/gguf_types
(tools/gguf_types_golden.c: dequantize_row_*, quantize_row_q8_0 / q8_1_reference, ne_vec_dot_*)."""
import numpy as np
import pytest

from neural_amd import _lib, bestla
from tests import gguf_blocks as gb
from tests.oracle_lib import load_ref_golden
from tests.test_gpu_parity import _rel_err

TYPES = [gb.Q4_1, gb.Q5_0, gb.Q5_1, gb.Q8_0]
CASES = ["n40_k256", "n16_k96"]


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("gguf_types")


def _case(golden, type, case):
    g = golden[f"{gb.NAMES[type]}_{case}"]
    n, k, m = (int(v) for v in g["meta"])
    return g, n, k, m


def test_block_bytes_and_constants():
    L = _lib.lib()
    assert [L.nad_gguf_block_bytes(t) for t in (2, 3, 6, 7, 8)] == [18, 20, 22, 24, 34]
    assert (bestla.GGUF_Q4_0, bestla.GGUF_Q4_1, bestla.GGUF_Q5_0, bestla.GGUF_Q5_1, bestla.GGUF_Q8_0) == (2, 3, 6, 7, 8)


@pytest.mark.parametrize("n,k", [(40, 256), (16, 96), (4096, 4096)])
def test_device_sizes(n, k):
    L = _lib.lib()
    assert L.nad_gguf_device_size(2, n, k) == L.nad_q4_0_device_size(n, k) > 0
    s8 = L.nad_synthetic_weight_size(8, n, k, 32, 2, 0)  # 2 = NAD_SCALE_F16
    assert L.nad_gguf_device_size(8, n, k) == s8
    assert L.nad_gguf_device_size(6, n, k) == s8
    ns, ng = (n + 15) // 16, k // 32
    assert L.nad_gguf_device_size(3, n, k) >= L.nad_q4_0_device_size(n, k) + ns * ng * 32
    assert L.nad_gguf_device_size(7, n, k) >= s8 + ns * ng * 32


def test_unsupported_type_and_shape_are_errors():
    L = _lib.lib()
    L.nad_clear_error()
    assert L.nad_gguf_block_bytes(14) == 0
    assert "14" in _lib.last_error()
    L.nad_clear_error()
    assert L.nad_gguf_device_size(14, 64, 64) == 0       # Q6_K
    assert "14" in _lib.last_error()
    for t in (2, 3, 6, 7, 8):
        L.nad_clear_error()
        assert L.nad_gguf_device_size(t, 64, 48) == 0
        assert _lib.last_error()
    L.nad_clear_error()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", TYPES)
def test_dequant_bit_exact(golden, type, case):
    g, n, k, _ = _case(golden, type, case)
    blocks = g[gb.NAMES[type]]
    assert blocks.size == n * (k // 32) * gb.BLOCK_BYTES[type]
    deq = gb.dequant(type, blocks, n, k)
    assert np.array_equal(deq.view(np.uint32), g["deq"].reshape(n, k).view(np.uint32))
    # pack() inverts fields(): the same bytes back
    d, m, q = gb.fields(type, blocks, n, k)
    stored = q + 16 if type == gb.Q5_0 else q
    assert np.array_equal(gb.pack(type, d.astype(np.float16), stored, m.astype(np.float16)), blocks)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", TYPES)
def test_activation_blocks_bit_exact(golden, type, case):
    g, _, k, m = _case(golden, type, case)
    name = gb.ACT_BLOCKS[type]
    quant = gb.quant_q8_0 if name == "y_q8_0" else gb.quant_q8_1
    assert np.array_equal(quant(g["A"].reshape(m, k)), g[name])     # Q8_1: d, s and the codes


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", TYPES)
def test_integer_forward_matches_vec_dot(golden, type, case):
    g, n, k, m = _case(golden, type, case)
    y = gb.forward_int(type, g[gb.NAMES[type]], n, k, g["A"].reshape(m, k))
    assert _rel_err(y, g["C"].reshape(m, n).astype(np.float64)) <= 1e-5


@pytest.mark.parametrize("type", TYPES)
def test_quantize_round_trips_through_dequant(type):
    """quantize() is only the generator of the larger GPU cases; it must give valid blocks whose values track W"""
    rng = np.random.default_rng(type)
    w = (rng.uniform(-1, 1, size=(8, 64)) + (1.5 if gb.HAS_MIN[type] else 0)).astype(np.float32)
    deq = gb.dequant(type, gb.quantize(type, w), 8, 64)
    step = {gb.Q4_1: 2 / 15, gb.Q5_0: 1 / 16, gb.Q5_1: 2 / 31, gb.Q8_0: 1 / 127}[type]
    assert np.abs(deq - w).max() <= step   # half a step of rounding + the fp16 rounding of d and m
