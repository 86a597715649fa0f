"""GPU GGUF Q4_1 / Q5_0 / Q5_1 / Q8_0 (woq_gguf.hip): the repack, the Q8_1 quantizer and the min-term pass against the
reference's own outputs (tests/golden/gguf_types) and, at larger shapes, against tests/gguf_blocks.py, which
tests/test_gguf_types_cpu.py pins to those outputs.

fp mode is checked against the fp64 product with the dequantized matrix at the project's bars: 2e-5 of max|ref| where
nad_plan_weight reports a kernel that keeps the block scale in fp32, FOLD_TOL where it folds the scale into the fp16
weights (q d rounded once to fp16).  int8 mode is checked at 1e-5 against ne_vec_dot_* (float association differs)."""
import numpy as np
import pytest

from tests import gguf_blocks as gb
from tests.conftest import gpu_available
from tests.oracle_lib import load_ref_golden
from tests.test_gemm2_gpu import FOLD_TOL
from tests.test_gpu_parity import _rel_err

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

TYPES = [gb.Q4_1, gb.Q5_0, gb.Q5_1, gb.Q8_0]
CASES = ["n40_k256", "n16_k96"]
EXACT_TOL = 2e-5


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("gguf_types")


@pytest.fixture
def int8_mode():
    prev = bestla.set_compute_mode(bestla.COMPUTE_INT8)
    yield
    bestla.set_compute_mode(prev)


_CACHE = {}


def _weight(type, n, k, seed=0):
    """(blocks, fp64 dequantized [n][k], DeviceWeight) of a quantized random matrix; the min types get mins of the size
    of d * qmax (W in 0.5 .. 2.5), so a dropped or misplaced min term is an error of the size of the result"""
    key = (type, n, k, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * type + n + k + seed)
        w = (rng.uniform(-1, 1, size=(n, k)) + (1.5 if gb.HAS_MIN[type] else 0.0)).astype(np.float32)
        blocks = gb.quantize(type, w)
        _CACHE[key] = (blocks, gb.dequant(type, blocks, n, k).astype(np.float64),
                       bestla.DeviceWeight.from_gguf(type, blocks, n, k))
    return _CACHE[key]


def _tol(m, act, *ws):
    return FOLD_TOL if any(w.plan(m, act)["fold"] for w in ws) else EXACT_TOL


def _x(m, k, dtype=None, seed=0):
    rng = np.random.default_rng(m * 7 + k + seed)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(m, k)).astype(np.float32)).cuda()
    return x.to(dtype or torch.float16)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


_ACT = {"fp16": "float16", "fp32": "float32", "bf16": "bfloat16"}


# ------------------------------------------------------------------------------------------------ load / unpack
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", TYPES)
def test_load_unpacks_bit_exact(golden, type, case):
    g = golden[f"{gb.NAMES[type]}_{case}"]
    n, k, _ = (int(v) for v in g["meta"])
    w = bestla.DeviceWeight.from_gguf(type, g[gb.NAMES[type]], n, k)
    deq = w.unpack()                      # [K][N]
    assert np.array_equal(deq.T.copy().view(np.uint32), g["deq"].reshape(n, k).view(np.uint32))


def test_q4_0_through_from_gguf_is_from_q4_0():
    n, k = 272, 2048
    rng = np.random.default_rng(5)
    d = rng.uniform(0.001, 0.01, size=(n, k // 32)).astype(np.float16)
    blocks = np.concatenate([d.view(np.uint8).reshape(n, k // 32, 2),
                             rng.integers(0, 256, size=(n, k // 32, 16), dtype=np.uint8)], axis=2).ravel()
    a = bestla.DeviceWeight.from_q4_0(blocks, n, k)
    b = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q4_0, blocks, n, k)
    assert (a.bytes, a.bits, a.asym, a.fold_ok, a.ng, a.nt) == (b.bytes, b.bits, b.asym, b.fold_ok, b.ng, b.nt)
    assert np.array_equal(a.unpack().view(np.uint32), b.unpack().view(np.uint32))
    for m in (1, 40):
        x = _x(m, k)
        assert torch.equal(a.forward(x), b.forward(x))
        assert a.plan(m, "fp16") == b.plan(m, "fp16")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", [gb.Q4_1, gb.Q5_1])
def test_q8_1_quant_bit_exact(golden, type, case):
    g = golden[f"{gb.NAMES[type]}_{case}"]
    _, k, m = (int(v) for v in g["meta"])
    x = torch.from_numpy(g["A"].reshape(m, k).copy()).cuda()
    assert np.array_equal(bestla.quant_q8_1(x).cpu().numpy().ravel(), g["y_q8_1"])


# ------------------------------------------------------------------------------------------------ fp mode
@pytest.mark.parametrize("m", [1, 5, 16, 17, 40, 130])
@pytest.mark.parametrize("n,k", [(40, 256), (16, 96), (272, 2048)])
@pytest.mark.parametrize("type", TYPES)
def test_fp_mode(type, n, k, m):
    _, deq, w = _weight(type, n, k)
    x = _x(m, k)
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    tol = _tol(m, "fp16", w)
    print(f"type={type} n={n} k={k} m={m} rel_err={err:.3e} tol={tol}")
    assert err <= tol


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("m", [1, 40])
@pytest.mark.parametrize("type", [gb.Q4_1, gb.Q5_1])
def test_fp_mode_other_activation_dtypes(type, m, act):
    n, k = 272, 2048
    _, deq, w = _weight(type, n, k)
    x = _x(m, k, getattr(torch, _ACT[act]))
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    tol = _tol(m, act, w)
    print(f"type={type} act={act} m={m} rel_err={err:.3e} tol={tol}")
    assert err <= tol


def test_fp_mode_strided_unaligned_rows():
    """rows that are not 16-byte aligned take the scalar activation loads of the block sums"""
    n, k, m = 40, 256, 5
    _, deq, w = _weight(gb.Q4_1, n, k)
    buf = _x(m, k + 3)
    x = buf[:, 1:k + 1]
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    assert err <= _tol(m, "fp16", w)


@pytest.mark.parametrize("m", [1, 16, 40])
@pytest.mark.parametrize("type", [gb.Q4_1, gb.Q5_1])
def test_fp_mode_mins_differ_per_column_and_block(type, m):
    """no constant anywhere: d, m and q drawn per (column, block), so a transposed or shifted mins index fails"""
    n, k = 72, 320                        # 4.5 stripes, 10 blocks: a partial stripe and a partial K tile
    rng = np.random.default_rng(type)
    nb = k // 32
    d = rng.uniform(0.01, 0.1, size=(n, nb)).astype(np.float16)
    mn = (rng.uniform(-2, 2, size=(n, nb)) * (1 + np.arange(nb))[None, :] / nb).astype(np.float16)
    q = rng.integers(0, gb.QMAX[type] + 1, size=(n, nb, 32))
    blocks = gb.pack(type, d, q, mn)
    w = bestla.DeviceWeight.from_gguf(type, blocks, n, k)
    deq = gb.dequant(type, blocks, n, k)
    assert np.array_equal(w.unpack().T.copy().view(np.uint32), deq.view(np.uint32))
    x = _x(m, k)
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.astype(np.float64).T)
    print(f"type={type} m={m} rel_err={err:.3e}")
    assert err <= _tol(m, "fp16", w)


# ------------------------------------------------------------------------------------------------ epilogues
def _gelu(v):
    return 0.5 * v * (1 + np.tanh(0.7978845834732056 * (v + 0.044714998453855515 * v ** 3)))


def _silu(v):
    return v / (1 + np.exp(-v))


@pytest.mark.parametrize("m", [1, 40])
def test_q4_1_epilogues(m):
    n, k = 272, 2048
    _, deq, w = _weight(gb.Q4_1, n, k)
    x = _x(m, k)
    y = _f64(x) @ deq.T
    rng = np.random.default_rng(m)
    bias = torch.from_numpy(rng.uniform(-20, 20, size=n).astype(np.float32)).cuda()
    res = torch.from_numpy(rng.uniform(-20, 20, size=(m, n)).astype(np.float32)).cuda()
    tol = _tol(m, "fp16", w)
    got = w.forward(x, epilogue=bestla.EPI_BIAS, bias=bias).cpu().numpy()
    assert _rel_err(got, y + _f64(bias)[None, :]) <= tol
    got = w.forward(x, epilogue=bestla.EPI_RES_ADD, residual=res).cpu().numpy()
    assert _rel_err(got, y + _f64(res)) <= tol
    got = w.forward(x, epilogue=bestla.EPI_GELU).cpu().numpy()
    assert _rel_err(got, _gelu(y)) <= tol


@pytest.mark.parametrize("m", [1, 40])
def test_q4_1_ffn(m):
    fin, fmid = 256, 288                  # 18 stripes, nine blocks as the down weight's K
    _, d1, w1 = _weight(gb.Q4_1, fmid, fin, seed=1)
    _, d3, w3 = _weight(gb.Q4_1, fmid, fin, seed=3)
    x = _x(m, fin) * 0.125                                 # keeps silu(.) * (.) of the shifted weights moderate
    x64 = _f64(x)
    gate_up = _silu(x64 @ d1.T) * (x64 @ d3.T)
    tol = _tol(m, "fp16", w1, w3)
    got = bestla.ffn_gate_up(x, w1, w3).cpu().numpy()
    assert _rel_err(got, gate_up) <= tol
    # the whole FFN, with a down weight whose K is fmid: a third weight of that shape
    _, dd, wd = _weight(gb.Q4_1, 40, fmid, seed=4)
    got = bestla.ffn_forward(x, w1, wd, w3).cpu().numpy()
    err = _rel_err(got, gate_up @ dd.T)
    print(f"ffn m={m} rel_err={err:.3e}")
    assert err <= max(tol, _tol(m, "fp32", wd))


@pytest.mark.parametrize("m", [1, 16, 40])
@pytest.mark.parametrize("min_first", [True, False])
def test_ffn_gate_up_mixed_min_and_plain_pair(m, min_first):
    """Q5_1 with Q8_0 (one device format, only one of them with mins), either as gate or as up"""
    fin, fmid = 256, 288
    a, b = _weight(gb.Q5_1, fmid, fin, seed=5), _weight(gb.Q8_0, fmid, fin, seed=6)
    (_, d1, w1), (_, d3, w3) = (a, b) if min_first else (b, a)
    x = _x(m, fin) * 0.125
    x64 = _f64(x)
    ref = _silu(x64 @ d1.T) * (x64 @ d3.T)
    err = _rel_err(bestla.ffn_gate_up(x, w1, w3).cpu().numpy(), ref)
    print(f"mixed m={m} min_first={min_first} rel_err={err:.3e}")
    assert err <= _tol(m, "fp16", w1, w3)


def test_batch_refuses_weights_with_mins():
    """the batched M = 1 GEMV has no min-term pass: a Q4_1 / Q5_1 problem is an error, never a silent wrong result"""
    n, k = 272, 2048
    for type in (gb.Q4_1, gb.Q5_1):
        _, _, w = _weight(type, n, k)
        x = torch.zeros(k, dtype=torch.float32, device="cuda")
        y = torch.zeros(n, dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError, match="mins"):
            bestla.Batch([(w, x, y), (w, x, y)])


@pytest.mark.parametrize("m", [1, 40])
def test_q5_1_qkv_unequal_n(m):
    k = 256
    ws = [_weight(gb.Q5_1, n, k, seed=n) for n in (272, 40, 72)]
    x = _x(m, k)
    outs = bestla.qkv_forward(x, ws[0][2], ws[1][2], ws[2][2])
    for (_, deq, w), o in zip(ws, outs):
        assert _rel_err(o.cpu().numpy(), _f64(x) @ deq.T) <= _tol(m, "fp16", w)


# ------------------------------------------------------------------------------------------------ int8 mode
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("type", TYPES)
def test_int8_mode_matches_reference(golden, int8_mode, type, case):
    g = golden[f"{gb.NAMES[type]}_{case}"]
    n, k, m = (int(v) for v in g["meta"])
    w = bestla.DeviceWeight.from_gguf(type, g[gb.NAMES[type]], n, k)
    assert w.compute == bestla.COMPUTE_INT8
    y = w.forward(torch.from_numpy(g["A"].reshape(m, k).copy()).cuda()).cpu().numpy()
    err = _rel_err(y, g["C"].reshape(m, n).astype(np.float64))
    print(f"type={type} case={case} rel_err={err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("m", [1, 16, 40])
@pytest.mark.parametrize("type", TYPES)
def test_int8_mode_matches_block_model(int8_mode, type, m):
    n, k = 200, 1024
    blocks, _, w = _weight(type, n, k)
    a = np.random.default_rng(m).uniform(-1, 1, size=(m, k)).astype(np.float32)
    y = w.forward(torch.from_numpy(a).cuda()).cpu().numpy()
    err = _rel_err(y, gb.forward_int(type, blocks, n, k, a).astype(np.float64))
    print(f"type={type} m={m} rel_err={err:.3e}")
    assert err <= 1e-5


def test_int8_mode_mixed_quantizers_fail(int8_mode):
    """Q4_1 (Q8_1 activations) with Q4_0 (Q8_0) in one gate/up pair: a recorded error, nothing computed"""
    fin, fmid = 256, 288
    blocks, _, w1 = _weight(gb.Q4_1, fmid, fin, seed=1)
    rng = np.random.default_rng(0)
    q40 = np.concatenate([rng.uniform(0.001, 0.01, size=(fmid, fin // 32)).astype(np.float16).view(np.uint8)
                          .reshape(fmid, fin // 32, 2),
                          rng.integers(0, 256, size=(fmid, fin // 32, 16), dtype=np.uint8)], axis=2).ravel()
    w3 = bestla.DeviceWeight.from_q4_0(q40, fmid, fin)
    with pytest.raises(RuntimeError):
        bestla.ffn_gate_up(_x(1, fin), w1, w3)


# ------------------------------------------------------------------------------------------------ graph / plan
def test_q4_1_graph_capture_replays():
    n, k = 272, 2048
    _, deq, w = _weight(gb.Q4_1, n, k)
    x = _x(1, k)
    out = torch.zeros((1, n), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w.forward(x, out=out)               # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        w.forward(x, out=out)
    results = []
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        results.append(out.clone())
    assert torch.equal(results[0], results[1])
    assert torch.equal(results[0], eager)
    assert _rel_err(results[0].cpu().numpy(), _f64(x) @ deq.T) <= _tol(1, "fp16", w)


@pytest.mark.parametrize("m", [1, 16, 40])
def test_plan_counts_the_min_term_launches(m):
    n, k = 272, 2048
    _, _, w41 = _weight(gb.Q4_1, n, k)
    rng = np.random.default_rng(1)
    d = rng.uniform(0.001, 0.01, size=(n, k // 32)).astype(np.float16)
    q40 = np.concatenate([d.view(np.uint8).reshape(n, k // 32, 2),
                          rng.integers(0, 256, size=(n, k // 32, 16), dtype=np.uint8)], axis=2).ravel()
    w40 = bestla.DeviceWeight.from_q4_0(q40, n, k)
    p41, p40 = w41.plan(m, "fp16"), w40.plan(m, "fp16")
    assert p41["kernel"] == p40["kernel"]
    assert p41["launches"] == p40["launches"] + (1 if m <= 16 else 2)
