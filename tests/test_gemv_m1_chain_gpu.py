"""The specialised M = 1 decode GEMV after its launch arguments moved into preloaded scalar parameters and its
reduce got the slot count at compile time (woq_gemv_m1s_kernel: 16, 11 and 7 slots per column, 0 = the runtime count).

Every case runs one call into canary-guarded outputs (tests/edges.py) and compares it three ways:
  1. bit for bit against NAD_GEMV_M1_SPEC=0 (woq_gemv_m1_kernel with the full GemvArgs and the runtime reduce): the
     specialised kernel keeps the stream and the summation order;
  2. bit for bit against what the library produced before this kernel changed, recorded once from that build with
     tools/gemv_chain_golden.py (tests/golden/gemv_m1_chain_parent.npz; the inputs are seeded, the weights are packed
     by the oracle on the CPU);
  3. within 2e-5 of max|C| of the oracle (the M = 1 bar of tests/test_gpu_parity.py).
Before it runs, the dry-run plan must name the specialised kernel, so a fallback cannot pass silently.

Shapes: int4 g128 sym with fp16 scales and fp32 activations unless the case says otherwise; N is the smallest that
shows the edge (a ragged last stripe, one stripe for 256 workgroups, three unequal weights).
"""
import os

import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.oracle_lib import BF16, F16, S4

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla
    from tests.edges import Canary

TOL = 2e-5  # tests/test_gpu_parity.py TOL_DECODE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_m1_chain_parent.npz")
GUARD = 24  # canary floats in front of and behind every output row

_CACHE = {}


def _weight(oracle, n, k, bs=128, st=F16, asym=False, seed=0):
    key = (n, k, bs, st, asym, seed)
    if key not in _CACHE:
        W = np.random.default_rng(7000 + seed + n + k).uniform(-0.5, 0.5, size=(n, k)).astype(np.float32)
        core = oracle.lib.orc_select_core(4, S4, bs, int(asym), 0)
        blob = oracle.quant_pack(W, n, k, bs, S4, st, asym, core, is_trans=True)
        _CACHE[key] = (blob, bestla.DeviceWeight(blob))
    return _CACHE[key]


def _act(k, dt="fp32"):
    key = ("A", k, dt)
    if key not in _CACHE:
        A = np.random.default_rng(k).uniform(-0.5, 0.5, size=(1, k)).astype(np.float32)
        t = torch.from_numpy(A).cuda().to({"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dt])
        _CACHE[key] = (t, t.float().cpu().numpy())
    return _CACHE[key]


def _ref(oracle, tag, A, blob, n, k):
    key = ("ref", tag)
    if key not in _CACHE:
        _CACHE[key] = oracle.forward(A, blob, n, k).astype(np.float64)
    return _CACHE[key]


def _silu(x):
    return x / (1 + np.exp(-x))


def _rows(ns):
    """one canary buffer with a guarded row [1][n] per output"""
    can = Canary(sum(GUARD + n for n in ns) + GUARD)
    wins, off = [], GUARD
    for n in ns:
        wins.append(can.window(off, 1, n, n))
        off += n + GUARD
    return can, wins


def _guarded(ns, call):
    """call(windows) once into fresh canary-guarded rows -> their values"""
    can, wins = _rows(ns)
    call(wins)
    torch.cuda.synchronize()
    can.check()
    return [w.cpu().numpy().copy() for w in wins]


# id -> (kind, n or (nq, nk, nv), k, group size, scale type, asym, activation type, threads of the launch)
CASES = {
    "one_n40": ("one", 40, 4096, 128, F16, False, "fp32", 1024),           # ragged last stripe
    "one_n16": ("one", 16, 4096, 128, F16, False, "fp32", 1024),           # one stripe: 255 workgroups without a unit
    "qkv_48_16_32": ("qkv", (48, 16, 32), 4096, 128, F16, False, "fp32", 1024),
    "pair_n40_aux": ("pair_aux", 40, 4096, 128, F16, False, "fp32", 1024),
    "pair_n40": ("pair", 40, 4096, 128, F16, False, "fp32", 1024),
    "slots11_k11008": ("one", 40, 11008, 128, F16, False, "fp32", 11 * 64),
    "slots11_partial_slice": ("one", 24, 10880, 128, F16, False, "fp32", 11 * 64),  # 85 tiles: the last slice has one
    "slots7_g64_k14336": ("one", 24, 14336, 64, F16, False, "fp32", 7 * 64),
    "k5632": ("one", 24, 5632, 128, F16, False, "fp32", 11 * 64),          # 44 tiles: 11 waves of one 4-tile slice
    "runtime_slots_k6144": ("one", 24, 6144, 128, F16, False, "fp32", 12 * 64),    # 12 waves: the runtime count
    "runtime_slots_k3072": ("one", 24, 3072, 128, F16, False, "fp32", 12 * 64),    # 12 waves of one 2-tile slice
    "asym_bf16_scales": ("one", 40, 4096, 128, BF16, True, "fp32", 1024),
    "act_bf16": ("one", 40, 4096, 128, F16, False, "bf16", 1024),
    "act_fp16": ("one", 40, 4096, 128, F16, False, "fp16", 1024),
}


def run_case(name, oracle, check_plan=True):
    """-> (outputs of the default path [list of [1][n]], their oracle references)"""
    kind, n, k, bs, st, asym, dt, threads = CASES[name]
    x, A = _act(k, dt)
    if kind == "one":
        blob, w = _weight(oracle, n, k, bs, st, asym)
        if check_plan:
            p = w.plan(1, dt)
            assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is True and p["threads"] == threads, p
        ys = _guarded([n], lambda o: w.forward(x, out=o[0]))
        return ys, [_ref(oracle, (n, k, bs, st, asym, dt), A, blob, n, k)]
    if kind == "qkv":
        ws = [_weight(oracle, ni, k, bs, st, asym, seed=10 + i) for i, ni in enumerate(n)]
        if check_plan:
            p = bestla.plan_qkv(*[w for _, w in ws], 1, dt)
            assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is True and p["launches"] == 1, p
            assert p["threads"] == threads, p
        ys = _guarded(list(n), lambda o: bestla.qkv_forward(x, *[w for _, w in ws], out=o))
        return ys, [_ref(oracle, ("qkv", i), A, blob, ni, k) for i, ((blob, _), ni) in enumerate(zip(ws, n))]
    (b1, w1), (b3, w3) = _weight(oracle, n, k, seed=21), _weight(oracle, n, k, seed=23)
    if check_plan:  # the pair's launch has one weight's geometry
        p = w1.plan(1, dt)
        assert p["m1_spec"] is True and p["threads"] == threads, p
    h1, h3 = _ref(oracle, ("gate",), A, b1, n, k), _ref(oracle, ("up",), A, b3, n, k)
    if kind == "pair_aux":
        ys = _guarded([n, n], lambda o: bestla.ffn_gate_up(x, w1, w3, act="silu", tmp1=o[1], tmp2=o[0]))
        return ys, [_silu(h1) * h3, _silu(h1)]
    ys = _guarded([n], lambda o: bestla.ffn_gate_up(x, w1, w3, act="silu", tmp1=None, tmp2=o[0]))
    return ys, [_silu(h1) * h3]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(CASES))
def test_case(oracle, knob, golden, name):
    ys, refs = run_case(name, oracle)
    knob("NAD_GEMV_M1_SPEC", "0")
    ys0, _ = run_case(name, oracle, check_plan=False)
    knob("NAD_GEMV_M1_SPEC", None)
    for i, (y, y0, ref) in enumerate(zip(ys, ys0, refs)):
        err = float(np.abs(y.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
        print(f"{name}[{i}]: err {err:.3e} bound {TOL:.1e}")
        assert np.array_equal(y, y0), (name, i, "differs from woq_gemv_m1_kernel")
        assert np.array_equal(y, golden[f"{name}.{i}"]), (name, i, "differs from the recorded earlier build")
        assert err <= TOL, (name, i, err)


def test_graph_replay(oracle):
    """the leading scalar parameters and the remainder struct go through the graph path: one launch captured and
    replayed twice equals the eager result"""
    n, k = 40, 11008
    _, w = _weight(oracle, n, k)
    assert w.plan(1)["m1_spec"] is True
    x, _ = _act(k)
    y0 = w.forward(x).clone()
    out = torch.zeros_like(y0)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w.forward(x, out=out)
        with torch.cuda.graph(g, stream=s):
            w.forward(x, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, y0)
