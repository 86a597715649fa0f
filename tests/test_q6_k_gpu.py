"""GPU GGUF Q6_K (woq_q6k.hip): the repack against the reference's own dequantize_row_q6_K outputs (tests/golden/q6_k),
and the two forward kernels against the fp64 product of the activations' own values with the dequantized matrix of
tests/q6k_blocks.py, which tests/test_q6_k_cpu.py pins to those outputs bit for bit.

Bars: 2e-5 of max|ref| where nad_plan_weight reports fold 0 (woq_q6k_gemv_kernel, M <= 16: the int8 sub-scale is
applied in fp32 to each group's partial, so every product is fp32-accurate), FOLD_TOL where it reports fold 1
(woq_q6k_gemm_kernel, M > 16: sc * q rounded once to fp16).  Random blocks draw the sub-scales over the whole int8 range,
so |sc * q| reaches 4096 -- past fp16's exact integers -- in every case: a decode kernel that folded sc into its fp16
fragment would miss 2e-5 several times over."""
import numpy as np
import pytest

from tests import edges
from tests import q6k_blocks as qb
from tests.conftest import gpu_available
from tests.oracle_lib import load_ref_golden
from tests.test_gemm2_gpu import FOLD_TOL
from tests.test_gpu_parity import _rel_err

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

EXACT_TOL = 2e-5
GOLDEN = ["n40_k256", "n16_k768", "ext_n16_k512"]
# a partial stripe; 1 / 3 / 8 / 17 superblocks (17: more superblocks than the GEMV has waves, and no power of two)
SHAPES = [(40, 256), (16, 768), (272, 2048), (48, 4352)]
MS = [1, 2, 5, 8, 9, 16, 17, 40, 130]
_DT = {"fp16": "float16", "fp32": "float32", "bf16": "bfloat16"}


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("q6_k")


_CACHE = {}


def _weight(n, k, seed=0):
    """(blocks, fp64 dequantized [n][k], DeviceWeight) of random Q6_K blocks, made once"""
    key = (n, k, seed)
    if key not in _CACHE:
        blocks = qb.random_blocks(n, k, seed=1000 * seed + n + k)
        _CACHE[key] = (blocks, qb.dequant(blocks, n, k).astype(np.float64), bestla.DeviceWeight.from_q6_k(blocks, n, k))
    return _CACHE[key]


def _q8_0_weight(n, k, seed):
    from tests import gguf_blocks as gb
    key = ("q8_0", n, k, seed)
    if key not in _CACHE:
        w = np.random.default_rng(seed).uniform(-1, 1, size=(n, k)).astype(np.float32)
        blocks = gb.quantize(gb.Q8_0, w)
        _CACHE[key] = (blocks, gb.dequant(gb.Q8_0, blocks, n, k).astype(np.float64),
                       bestla.DeviceWeight.from_gguf(bestla.GGUF_Q8_0, blocks, n, k))
    return _CACHE[key]


def _x(m, k, act="fp16", seed=0):
    rng = np.random.default_rng(m * 7 + k + seed)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(m, k)).astype(np.float32)).cuda()
    return x.to(getattr(torch, _DT[act]))


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _tol(m, act, w):
    return FOLD_TOL if w.plan(m, act)["fold"] else EXACT_TOL


def _check_plan(w, m, act):
    plan = w.plan(m, act)
    if m <= 16:
        assert plan["kernel"] == "woq_q6k_gemv_kernel" and not plan["fold"] and plan["launches"] == 1, plan
    else:
        assert plan["kernel"] == "woq_q6k_gemm_kernel" and plan["fold"] and plan["launches"] == 1, plan


# ------------------------------------------------------------------------------------------------ load / unpack
@pytest.mark.parametrize("case", GOLDEN)
def test_load_unpacks_bit_exact(golden, case):
    g = golden[case]
    n, k = (int(v) for v in g["meta"])
    w = bestla.DeviceWeight.from_q6_k(g["q6_k"], n, k)
    assert (w.bits, w.blocksize, w.scale_t, w.asym, w.n, w.k) == (6, 16, 2, 0, n, k)
    assert w.bytes <= (n + 15) // 16 * 16 * (k // 256) * 210 + 5 * 256
    deq = w.unpack()                      # [K][N]
    assert np.array_equal(deq.T.copy().view(np.uint32), g["deq"].reshape(n, k).view(np.uint32))


def test_from_gguf_routes_type_14(golden):
    g = golden["n40_k256"]
    a = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q6_K, g["q6_k"], 40, 256)
    b = bestla.DeviceWeight.from_q6_k(g["q6_k"], 40, 256)
    assert (a.bits, a.bytes) == (b.bits, b.bytes) == (6, a.bytes)
    assert np.array_equal(a.unpack().view(np.uint32), b.unpack().view(np.uint32))


def test_random_blocks_unpack_bit_exact():
    """every byte value in ql / qh / scales, at 17 superblocks and three stripes"""
    n, k = 48, 4352
    blocks, _, w = _weight(n, k)
    assert np.array_equal(w.unpack().T.copy().view(np.uint32), qb.dequant(blocks, n, k).view(np.uint32))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n,k", SHAPES)
def test_forward_fp16(n, k, m):
    _, deq, w = _weight(n, k)
    _check_plan(w, m, "fp16")
    x = _x(m, k)
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    tol = _tol(m, "fp16", w)
    print(f"q6_k fp16 n={n} k={k} m={m} rel_err={err:.3e} tol={tol}")
    assert err <= tol


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("m", [1, 9, 40])
@pytest.mark.parametrize("n,k", SHAPES)
def test_forward_other_activation_dtypes(n, k, m, act):
    _, deq, w = _weight(n, k)
    _check_plan(w, m, act)
    x = _x(m, k, act)
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    tol = _tol(m, act, w)
    print(f"q6_k {act} n={n} k={k} m={m} rel_err={err:.3e} tol={tol}")
    assert err <= tol


@pytest.mark.parametrize("m", [1, 16])
def test_forward_extreme_fields_fp32(golden, m):
    """the hand-written blocks (q = -32 / 31 under sc = 127 / -128, sc = 0, d = 0 and subnormal d): the case an fp16
    fold of sc * q fails at decode"""
    g = golden["ext_n16_k512"]
    n, k = (int(v) for v in g["meta"])
    w = bestla.DeviceWeight.from_q6_k(g["q6_k"], n, k)
    _check_plan(w, m, "fp32")
    deq = g["deq"].reshape(n, k).astype(np.float64)
    x = _x(m, k, "fp32", seed=3)
    err = _rel_err(w.forward(x).cpu().numpy(), _f64(x) @ deq.T)
    print(f"q6_k ext m={m} rel_err={err:.3e}")
    assert err <= EXACT_TOL


def test_bestla_device_f32f32_forward_accepts_the_descriptor():
    n, k, m = 40, 256, 5
    _, deq, w = _weight(n, k)
    x = _x(m, k, "fp32")
    out = torch.empty((m, n), dtype=torch.float32, device="cuda")
    bestla.f32f32_forward(x, w, out, m, n, k, k, n)
    assert _rel_err(out.cpu().numpy(), _f64(x) @ deq.T) <= EXACT_TOL


@pytest.mark.parametrize("act", ["fp16", "fp32"])
@pytest.mark.parametrize("m", [1, 16, 40])
def test_forward_edges(m, act):
    """canary windows, NaN padding, unaligned rows, every single-weight epilogue, each call twice"""
    n, k = 40, 256
    _, deq, w = _weight(n, k)
    _check_plan(w, m, act)
    xt, xv = edges.round_to(np.random.default_rng(m).uniform(-1, 1, size=(m, k)), act)
    prod = xv.astype(np.float64) @ deq.T
    edges.check_forward_matrix(w, xt, prod, _tol(m, act, w), f"q6_k m={m} {act}")


# ------------------------------------------------------------------------------------------------ fused entries
@pytest.mark.parametrize("m", [1, 40])
def test_qkv_of_three_q6_k_weights(m):
    k = 768
    ws = [_weight(n, k, seed=n) for n in (272, 40, 48)]
    x = _x(m, k)
    outs = bestla.qkv_forward(x, ws[0][2], ws[1][2], ws[2][2])
    for (_, deq, w), o in zip(ws, outs):
        err = _rel_err(o.cpu().numpy(), _f64(x) @ deq.T)
        print(f"q6_k qkv m={m} n={w.n} rel_err={err:.3e}")
        assert err <= _tol(m, "fp16", w)


def _silu(v):
    return v / (1 + np.exp(-v))


def _gate_up_bound(g, u, t_g, t_u):
    """|d(silu(g) u)| <= SILU_SLOPE t_g max|g| max|u| + t_u max|u| max|silu(g)| + ACT_EVAL_ERR max|g| max|u|: each
    launch's own bar (2e-5 or FOLD_TOL, as its plan reports) carried through the product, worst case; relative to
    max|silu(g) u| of the fp64 reference"""
    gmax, umax = np.abs(g).max(), np.abs(u).max()
    e2 = (edges.SILU_SLOPE * t_g + edges.ACT_EVAL_ERR) * gmax * umax + t_u * umax * np.abs(_silu(g)).max()
    return e2 / np.abs(_silu(g) * u).max()


@pytest.mark.parametrize("m", [1, 40])
def test_ffn_mixed_q6_k_gate_q8_0_up_q6_k_down(m):
    """The fp64 chain link by link: the gate/up intermediate the call leaves in tmp2 against silu(x W1^T) (x W3^T) at
    _gate_up_bound, and the output against the fp64 product of that very tmp2 with the down matrix at the down launch's
    own bar -- so neither link hides behind the other's error."""
    fin, fmid, fout = 256, 512, 40
    _, d1, w1 = _weight(fmid, fin, seed=1)
    _, d3, w3 = _q8_0_weight(fmid, fin, seed=3)
    _, d2, w2 = _weight(fout, fmid, seed=2)
    x = _x(m, fin)
    x64 = _f64(x)
    g, u = x64 @ d1.T, x64 @ d3.T
    t2 = _silu(g) * u
    bound2 = _gate_up_bound(g, u, _tol(m, "fp16", w1), _tol(m, "fp16", w3))
    err2 = _rel_err(bestla.ffn_gate_up(x, w1, w3).cpu().numpy(), t2)
    print(f"q6_k ffn gate_up m={m} rel_err={err2:.3e} bound={bound2:.3e}")
    assert err2 <= bound2
    tmp2 = torch.full((m, fmid), float("nan"), dtype=torch.float32, device="cuda")
    got = bestla.ffn_forward(x, w1, w2, w3, tmp2=tmp2).cpu().numpy()
    err_mid = _rel_err(tmp2.cpu().numpy(), t2)
    err_down, t_d = _rel_err(got, _f64(tmp2) @ d2.T), _tol(m, "fp32", w2)
    print(f"q6_k ffn m={m} tmp2 rel_err={err_mid:.3e} bound={bound2:.3e}; down rel_err={err_down:.3e} bound={t_d}")
    assert err_mid <= bound2
    assert err_down <= t_d


def test_ffn_gate_up_q8_0_gate_q6_k_up():
    """the pair the other way round, M <= 16: the plain weight's kernel applies the activation, the Q6_K pass the multiply"""
    fin, fmid, m = 256, 512, 5
    _, d1, w1 = _q8_0_weight(fmid, fin, seed=3)
    _, d3, w3 = _weight(fmid, fin, seed=1)
    x = _x(m, fin)
    x64 = _f64(x)
    g, u = x64 @ d1.T, x64 @ d3.T
    bound = _gate_up_bound(g, u, _tol(m, "fp16", w1), _tol(m, "fp16", w3))
    err = _rel_err(bestla.ffn_gate_up(x, w1, w3).cpu().numpy(), _silu(g) * u)
    print(f"q6_k ffn gate_up (q8_0 gate) rel_err={err:.3e} bound={bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ refusals / modes
def test_batch_refuses_q6_k():
    n, k = 272, 2048
    _, _, w = _weight(n, k)
    x = torch.zeros(k, dtype=torch.float32, device="cuda")
    y = torch.zeros(n, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="Q6_K"):
        bestla.Batch([(w, x, y), (w, x, y)])


def test_set_compute_int8_leaves_the_weight_in_fp():
    n, k = 272, 2048
    blocks, _, _ = _weight(n, k)
    w = bestla.DeviceWeight.from_q6_k(blocks, n, k)   # a descriptor of its own: the cached one stays untouched
    for m in (1, 40):
        x = _x(m, k, "fp32")
        before = w.forward(x)
        w.set_compute(bestla.COMPUTE_INT8)
        assert w.compute == bestla.COMPUTE_FP
        _check_plan(w, m, "fp32")
        assert torch.equal(w.forward(x), before)
        w.set_compute(None)


# ------------------------------------------------------------------------------------------------ graph
def test_graph_capture_replays_bit_identical():
    n, k = 272, 2048
    _, deq, w = _weight(n, k)
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
    assert _rel_err(results[0].cpu().numpy(), _f64(x) @ deq.T) <= EXACT_TOL
