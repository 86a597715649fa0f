"""GPU GGUF Q6_K in the reference's Q8_K integer arithmetic: nad_quant_q8_k against the reference's own block_q8_K
bytes (tests/golden/q6_k_q8_k) and the numpy model of tests/q8k_blocks.py, which tests/test_q6_k_q8_k_cpu.py pins to
them bit for bit; woq_q6k_i8_kernel (a Q6_K weight in COMPUTE_Q8_K) against ggml_vec_dot_q6_K_q8_K's outputs, against
an exact integer model with no tolerance, and against the model of its contract

    isum_b = sum_g sc[g] * sum_i q[16 g + i] * a[16 g + i]            exact
    y      = sum_b fp32(fp32(d_w[b]) * d_a[r][b]) * float(isum_b)     fp32

at 1e-5 of max|ref|: the bar DESIGN.md section 2 holds the legacy GGUF types' integer modes to, which pays only for
the fp32 summation order (at most 17 superblocks here; float(isum_b) rounds |isum_b| > 2^24 by 6e-8 relative).
"""
import numpy as np
import pytest

from tests import edges
from tests import q6k_blocks as qb
from tests import q8k_blocks as q8
from tests.conftest import gpu_available
from tests.oracle_lib import load_ref_golden
from tests.test_gpu_parity import _rel_err

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla
    from tests import test_q6_k_gpu as t6

TOL = 1e-5
QUANT = ["quant_uniform_k256", "quant_uniform_k768", "quant_zero_sb", "quant_plus_first", "quant_minus_first",
         "quant_ties", "quant_amp_1em3", "quant_amp_1e3"]
DOT = ["dot_n40_k256_m5", "dot_n16_k768_m3"]
# a partial stripe; 1 / 3 / 8 / 17 superblocks (17: more superblocks than the kernel has waves)
SHAPES = [(40, 256), (16, 768), (272, 2048), (48, 4352)]
_DT = {"fp16": "float16", "fp32": "float32", "bf16": "bfloat16"}


@pytest.fixture(scope="module")
def golden():
    return load_ref_golden("q6_k_q8_k")


_CACHE = {}


def _q8k_weight(blocks, n, k):
    return bestla.DeviceWeight.from_q6_k(blocks, n, k).set_compute(bestla.COMPUTE_Q8_K)


def _weight(n, k, seed=0):
    """(blocks, DeviceWeight in COMPUTE_Q8_K) of random Q6_K blocks (d over a decade and more), made once"""
    key = (n, k, seed)
    if key not in _CACHE:
        blocks = qb.random_blocks(n, k, seed=1000 * seed + n + k)
        _CACHE[key] = (blocks, _q8k_weight(blocks, n, k))
    return _CACHE[key]


def _unit_d_weight(n, k):
    """qb.random_blocks(n, k, seed=n + k) with every d replaced by fp16 1.0"""
    key = ("unit", n, k)
    if key not in _CACHE:
        d, sc, q = qb.fields(qb.random_blocks(n, k, seed=n + k), n, k)
        blocks = qb.pack(np.ones_like(d), sc, q)
        _CACHE[key] = (blocks, _q8k_weight(blocks, n, k))
    return _CACHE[key]


def _x(m, k, act="fp16", seed=0):
    rng = np.random.default_rng(m * 7 + k + seed)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(m, k)).astype(np.float32)).cuda()
    return x.to(getattr(torch, _DT[act]))


def _f32(t):
    return t.float().cpu().numpy()


def _model(blocks, n, k, x_values):
    """the contract on the kernel's own input values (fp32 numpy [m][k])"""
    return q8.dot(blocks, n, k, q8.quantize(x_values), x_values.shape[0])


def _strided(x, pad=24):
    """the same values with a row stride larger than K, the padding NaN"""
    m, k = x.shape
    buf = torch.full((m, k + pad), float("nan"), dtype=x.dtype, device="cuda")
    buf[:, :k] = x
    return buf[:, :k]


def _check_plan(w, m, act):
    plan = w.plan(m, act)
    assert plan["kernel"] == "woq_q6k_i8_kernel" and not plan["fold"] and plan["launches"] == 1, plan


# ------------------------------------------------------------------------------------------------ quantizer
@pytest.mark.parametrize("case", QUANT)
def test_quant_q8_k_equals_the_reference_bytes(golden, case):
    g = golden[case]
    m, k = (int(v) for v in g["meta"])
    x = torch.from_numpy(g["x"].reshape(m, k).copy()).cuda()
    got = bestla.quant_q8_k(x).cpu().numpy()
    assert got.shape == (m, k // 256 * q8.BLOCK_BYTES)
    assert np.array_equal(got.ravel(), g["q8_k"])
    assert np.array_equal(bestla.quant_q8_k(_strided(x)).cpu().numpy().ravel(), g["q8_k"])


@pytest.mark.parametrize("act", ["fp16", "bf16"])
def test_quant_q8_k_half_inputs_equal_the_model(golden, act):
    """fp16 / bf16 activations are converted to fp32 first; an all-zero superblock and a clamp among them"""
    for case in ("quant_zero_sb", "quant_plus_first", "quant_amp_1e3"):
        g = golden[case]
        m, k = (int(v) for v in g["meta"])
        x = torch.from_numpy(g["x"].reshape(m, k).copy()).cuda().to(getattr(torch, _DT[act]))
        assert np.array_equal(bestla.quant_q8_k(x).cpu().numpy(), q8.quantize(_f32(x))), case


@pytest.mark.parametrize("k", [256, 4352])
@pytest.mark.parametrize("m", [1, 5, 17])
def test_quant_q8_k_random_rows_with_a_row_stride(m, k):
    for act in ("fp32", "fp16", "bf16"):
        x = _strided(_x(m, k, act, seed=11))
        assert x.stride(0) > k
        assert np.array_equal(bestla.quant_q8_k(x).cpu().numpy(), q8.quantize(_f32(x))), act


# ------------------------------------------------------------------------------------------------ mode plumbing
def test_mode_2_plan_and_back_to_fp():
    n, k = 272, 2048
    blocks = qb.random_blocks(n, k, seed=n + k)
    w = bestla.DeviceWeight.from_q6_k(blocks, n, k)
    xs = {m: _x(m, k, "fp32") for m in (1, 16, 40)}
    before = {m: w.forward(x) for m, x in xs.items()}
    assert w.compute == bestla.COMPUTE_FP
    w.set_compute(bestla.COMPUTE_Q8_K)
    assert w.compute == bestla.COMPUTE_Q8_K == 2
    for m in (1, 16, 40):
        for act in ("fp32", "fp16", "bf16"):
            _check_plan(w, m, act)
    w.set_compute(None)
    assert w.compute == bestla.COMPUTE_FP
    for m, x in xs.items():
        t6._check_plan(w, m, "fp32")
        assert torch.equal(w.forward(x), before[m])


def test_mode_2_is_refused_for_other_weights():
    _, _, w = t6._q8_0_weight(48, 256, seed=5)
    for prev in (None, bestla.COMPUTE_INT8):
        w.set_compute(prev)
        mode = w.compute
        with pytest.raises(RuntimeError, match="Q6_K"):
            w.set_compute(bestla.COMPUTE_Q8_K)
        assert w.compute == mode
    assert mode == bestla.COMPUTE_INT8
    w.set_compute(None)


def test_a_q6_k_weight_does_not_follow_the_process_mode():
    n, k = 40, 256
    blocks, _ = _weight(n, k)
    w = bestla.DeviceWeight.from_q6_k(blocks, n, k)
    prev = bestla.set_compute_mode(1)
    try:
        assert w.compute == bestla.COMPUTE_FP
        t6._check_plan(w, 1, "fp32")
    finally:
        bestla.set_compute_mode(prev)


# ------------------------------------------------------------------------------------------------ reference outputs
@pytest.mark.parametrize("case", DOT)
def test_forward_against_ggml_vec_dot_q6_K_q8_K(golden, case):
    g = golden[case]
    n, k, m = (int(v) for v in g["meta"])
    w = _q8k_weight(g["q6_k"], n, k)
    _check_plan(w, m, "fp32")
    x = torch.from_numpy(g["x"].reshape(m, k).copy()).cuda()
    assert np.array_equal(bestla.quant_q8_k(x).cpu().numpy().ravel(), g["q8_k"])
    y = g["y"].reshape(m, n).astype(np.float64)
    err = _rel_err(w.forward(x).cpu().numpy(), y)
    print(f"q6_k x q8_k {case} rel_err vs the reference={err:.3e}")
    assert err <= TOL


# ------------------------------------------------------------------------------------------------ exact integers
@pytest.mark.parametrize("m", [1, 4, 5, 16, 17])
@pytest.mark.parametrize("n,k", SHAPES)
def test_forward_exact_integers(n, k, m):
    """d_w = 1; integer activations with -128 leading every superblock, so iscale = 1, d_a = 1 and the codes are the
    activations: every output is an integer below 2^24, and the kernel's is that integer.  A sub-scale, group, row
    mask or offset taken from the wrong place fails outright."""
    blocks, w = _unit_d_weight(n, k)
    _check_plan(w, m, "fp32")
    rng = np.random.default_rng(m * 7 + k)
    xv = rng.integers(-15, 16, size=(m, k)).astype(np.float32)
    xv[:, ::256] = -128
    codes = q8.quantize(xv)
    d_a, q, _ = q8.fields(codes, m, k)
    assert (d_a == 1).all() and np.array_equal(q.reshape(m, k), xv.astype(np.int32))
    isum = q8.isums(blocks, n, k, codes, m)
    bound = np.abs(isum).sum(axis=2).max()
    print(f"exact n={n} k={k} m={m}: max sum_b |isum_b| = {bound} ({bound / 2 ** 24:.3f} of 2^24)")
    assert bound < 2 ** 24
    out = w.forward(torch.from_numpy(xv).cuda()).cpu().numpy()
    assert np.array_equal(out, isum.sum(axis=2).astype(np.float32))


# ------------------------------------------------------------------------------------------------ model parity
@pytest.mark.parametrize("m", [1, 2, 4, 5, 8, 16, 17, 40])
@pytest.mark.parametrize("n,k", SHAPES)
def test_forward_fp16(n, k, m):
    blocks, w = _weight(n, k)
    _check_plan(w, m, "fp16")
    x = _x(m, k)
    err = _rel_err(w.forward(x).cpu().numpy(), _model(blocks, n, k, _f32(x)))
    print(f"q6_k x q8_k fp16 n={n} k={k} m={m} rel_err={err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("m", [1, 9, 40])
@pytest.mark.parametrize("n,k", SHAPES)
def test_forward_other_activation_dtypes(n, k, m, act):
    blocks, w = _weight(n, k)
    _check_plan(w, m, act)
    x = _x(m, k, act)
    err = _rel_err(w.forward(x).cpu().numpy(), _model(blocks, n, k, _f32(x)))
    print(f"q6_k x q8_k {act} n={n} k={k} m={m} rel_err={err:.3e}")
    assert err <= TOL


def test_bestla_device_f32f32_forward_takes_the_mode():
    n, k, m = 40, 256, 5
    blocks, w = _weight(n, k)
    x = _x(m, k, "fp32")
    out = torch.empty((m, n), dtype=torch.float32, device="cuda")
    bestla.f32f32_forward(x, w, out, m, n, k, k, n)
    assert torch.equal(out, w.forward(x))
    assert _rel_err(out.cpu().numpy(), _model(blocks, n, k, _f32(x))) <= TOL


@pytest.mark.parametrize("act", ["fp16", "fp32"])
@pytest.mark.parametrize("m", [1, 16, 40])
def test_forward_edges(m, act):
    """canary windows, NaN padding, unaligned rows, every single-weight epilogue, each call twice"""
    n, k = 40, 256
    blocks, w = _weight(n, k)
    _check_plan(w, m, act)
    xt, xv = edges.round_to(np.random.default_rng(m).uniform(-1, 1, size=(m, k)), act)
    edges.check_forward_matrix(w, xt, _model(blocks, n, k, xv), TOL, f"q6_k x q8_k m={m} {act}")


# ------------------------------------------------------------------------------------------------ fused entries
@pytest.mark.parametrize("m", [1, 40])
def test_qkv_of_three_mode_2_weights(m):
    k = 768
    ws = [_weight(n, k, seed=n) for n in (272, 40, 48)]
    x = _x(m, k)
    outs = bestla.qkv_forward(x, ws[0][1], ws[1][1], ws[2][1])
    for (blocks, w), o in zip(ws, outs):
        err = _rel_err(o.cpu().numpy(), _model(blocks, w.n, k, _f32(x)))
        print(f"q6_k x q8_k qkv m={m} n={w.n} rel_err={err:.3e}")
        assert err <= TOL
        assert torch.equal(o, w.forward(x))


@pytest.mark.parametrize("m", [1, 40])
def test_ffn_mode_2_gate_q8_0_up_mode_2_down(m):
    """Link by link, each against its own model: tmp2 against silu(gate model) * (fp64 Q8_0 product) at the bound
    that carries the gate's 1e-5 and the up launch's own bar through the product (test_q6_k_gpu._gate_up_bound), the
    output against the Q8_K model of that very tmp2 with the down matrix at 1e-5."""
    fin, fmid, fout = 256, 512, 40
    b1, w1 = _weight(fmid, fin, seed=1)
    _, d3, w3 = t6._q8_0_weight(fmid, fin, seed=3)
    b2, w2 = _weight(fout, fmid, seed=2)
    assert (w1.compute, w3.compute, w2.compute) == (2, 0, 2)
    x = _x(m, fin)
    g, u = _model(b1, fmid, fin, _f32(x)), _f32(x).astype(np.float64) @ d3.T
    t2 = t6._silu(g) * u
    bound2 = t6._gate_up_bound(g, u, TOL, t6._tol(m, "fp16", w3))
    err2 = _rel_err(bestla.ffn_gate_up(x, w1, w3).cpu().numpy(), t2)
    print(f"q6_k x q8_k ffn gate_up m={m} rel_err={err2:.3e} bound={bound2:.3e}")
    assert err2 <= bound2
    tmp2 = torch.full((m, fmid), float("nan"), dtype=torch.float32, device="cuda")
    got = bestla.ffn_forward(x, w1, w2, w3, tmp2=tmp2).cpu().numpy()
    err_mid = _rel_err(tmp2.cpu().numpy(), t2)
    err_down = _rel_err(got, _model(b2, fout, fmid, tmp2.cpu().numpy()))
    print(f"q6_k x q8_k ffn m={m} tmp2 rel_err={err_mid:.3e} bound={bound2:.3e}; down rel_err={err_down:.3e}")
    assert err_mid <= bound2
    assert err_down <= TOL


def test_batch_still_refuses_q6_k():
    n, k = 272, 2048
    _, w = _weight(n, k)
    x = torch.zeros(k, dtype=torch.float32, device="cuda")
    y = torch.zeros(n, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="Q6_K"):
        bestla.Batch([(w, x, y), (w, x, y)])


# ------------------------------------------------------------------------------------------------ graph
def test_graph_capture_replays_bit_identical():
    n, k = 272, 2048
    blocks, w = _weight(n, k)
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
    assert _rel_err(results[0].cpu().numpy(), _model(blocks, n, k, _f32(x))) <= TOL
