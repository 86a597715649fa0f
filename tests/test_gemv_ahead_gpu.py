"""The load-ahead order of the specialised M = 1 decode GEMV (woq_gemv_m1s_kernel<..., AHEAD>, NAD_GEMV_AHEAD): a wave
requests its next weight stage when the current one has landed and before it computes it.

Every case runs one call into canary-guarded outputs (tests/edges.py) with NAD_GEMV_AHEAD=1 and with =0 and
  1. compares the two bit for bit: the order of the cursors, the stages, the sums and the reduce is unchanged,
  2. holds the load-ahead result to 2e-5 of max|C| of the oracle (the M = 1 bar of tests/test_gpu_parity.py),
  3. asserts through the dry-run plan that the knob really switches the form for this very call.

Shapes (int4 g128 sym, fp16 scales, fp32 activations unless the case says otherwise) are the smallest at which a
workgroup streams more than one stripe on 256 workgroups, so that a wave has a next stage to request: 517 stripes are
3 for five workgroups and 2 for the rest (an odd and an even stage count, and the u_r remainder); the pair's 259 units
are 4 and 2 stages; three unequal weights put a weight boundary between a stage and the one requested ahead.  The form
for the down projection (K = 11008, 11 waves) was measured and not kept, so there is no case for it.
"""
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
GUARD = 24  # canary floats in front of and behind every output row
N1 = 16 * (2 * 256 + 5)
NPAIR = 16 * (256 + 3)
NQKV = (16 * 300, 16 * 200, 16 * 270)

_CACHE = {}


def _weight(oracle, n, k, st=F16, asym=False, seed=0):
    key = (n, k, st, asym, seed)
    if key not in _CACHE:
        W = np.random.default_rng(9000 + seed + n + k).uniform(-0.5, 0.5, size=(n, k)).astype(np.float32)
        core = oracle.lib.orc_select_core(4, S4, 128, int(asym), 0)
        blob = oracle.quant_pack(W, n, k, 128, S4, st, asym, core, is_trans=True)
        _CACHE[key] = (blob, bestla.DeviceWeight(blob))
    return _CACHE[key]


def _act(k):
    key = ("A", k)
    if key not in _CACHE:
        A = np.random.default_rng(k).uniform(-0.5, 0.5, size=(1, k)).astype(np.float32)
        _CACHE[key] = (torch.from_numpy(A).cuda(), A)
    return _CACHE[key]


def _ref(oracle, A, blob, n, k, key):
    key = ("ref",) + key
    if key not in _CACHE:
        _CACHE[key] = oracle.forward(A, blob, n, k).astype(np.float64)
    return _CACHE[key]


def _silu(x):
    return x / (1 + np.exp(-x))


def _guarded(ns, call):
    """call(windows) once into fresh canary-guarded rows [1][n] -> their values"""
    can = Canary(sum(GUARD + n for n in ns) + GUARD)
    wins, off = [], GUARD
    for n in ns:
        wins.append(can.window(off, 1, n, n))
        off += n + GUARD
    call(wins)
    torch.cuda.synchronize()
    can.check()
    return [w.cpu().numpy().copy() for w in wins]


def _on_off(knob, plan, ns, call):
    """the call with the load-ahead form on and off -> (on, off); the plan must follow the knob"""
    knob("NAD_GEMV_AHEAD", "1")
    p = plan()
    assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is True and p["ahead"] is True and p["launches"] == 1, p
    on = _guarded(ns, call)
    knob("NAD_GEMV_AHEAD", "0")
    p0 = plan()
    assert p0["m1_spec"] is True and p0["ahead"] is False, p0
    assert (p0["grid"], p0["threads"]) == (p["grid"], p["threads"]), (p, p0)
    off = _guarded(ns, call)
    knob("NAD_GEMV_AHEAD", None)
    return on, off


def _compare(name, on, off, refs):
    for i, (y, y0, ref) in enumerate(zip(on, off, refs)):
        err = float(np.abs(y.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
        print(f"{name}[{i}]: err {err:.3e} bound {TOL:.1e}")
        assert np.array_equal(y, y0), (name, i, "differs from the present order")
        assert err <= TOL, (name, i, err)


ONE = [
    # id, n, k, scale type, asym, threads
    ("stripes_3_and_2", N1, 4096, F16, False, 1024),
    ("ragged_last_stripe", N1 - 5, 4096, F16, False, 1024),
    ("asym_bf16_scales", N1, 4096, BF16, True, 1024),
]


@pytest.mark.parametrize("cfg", ONE, ids=[c[0] for c in ONE])
def test_one_weight(oracle, knob, cfg):
    name, n, k, st, asym, threads = cfg
    blob, w = _weight(oracle, n, k, st, asym)
    x, A = _act(k)
    assert w.plan(1)["threads"] == threads, w.plan(1)
    on, off = _on_off(knob, lambda: w.plan(1), [n], lambda o: w.forward(x, out=o[0]))
    _compare(name, on, off, [_ref(oracle, A, blob, n, k, (n, k, st, asym))])


def test_gate_up_pair(oracle, knob):
    """2 and 4 stages per wave; the SiLU * mul output and the SiLU(gate) output"""
    n, k = NPAIR, 4096
    (b1, w1), (b3, w3) = _weight(oracle, n, k, seed=21), _weight(oracle, n, k, seed=23)
    x, A = _act(k)
    h1, h3 = _ref(oracle, A, b1, n, k, ("gate",)), _ref(oracle, A, b3, n, k, ("up",))
    on, off = _on_off(knob, lambda: bestla.plan_gate_up(w1, w3, 1), [n, n],
                      lambda o: bestla.ffn_gate_up(x, w1, w3, act="silu", tmp1=o[1], tmp2=o[0]))
    _compare("pair", on, off, [_silu(h1) * h3, _silu(h1)])


def test_three_unequal_weights(oracle, knob):
    """a wave's next stage crosses from one weight to the next inside the load-ahead"""
    k = 4096
    ws = [_weight(oracle, n, k, seed=10 + i) for i, n in enumerate(NQKV)]
    x, A = _act(k)
    on, off = _on_off(knob, lambda: bestla.plan_qkv(*[w for _, w in ws], 1), list(NQKV),
                      lambda o: bestla.qkv_forward(x, *[w for _, w in ws], out=o))
    _compare("qkv", on, off, [_ref(oracle, A, blob, n, k, ("qkv", i)) for i, ((blob, _), n) in enumerate(zip(ws, NQKV))])


def test_batched_launch_keeps_the_present_order(oracle, knob):
    """the batched launch has no load-ahead form: its plan says so with the knob on, and three problems of a weight
    whose single launch takes the form give that launch's result bit for bit"""
    n, k = N1, 4096
    _, w = _weight(oracle, n, k)
    xs = [torch.from_numpy(np.random.default_rng(50 + i).uniform(-0.5, 0.5, size=(k,)).astype(np.float32)).cuda()
          for i in range(3)]
    ys = [torch.zeros(n, device="cuda") for _ in xs]
    knob("NAD_GEMV_AHEAD", "1")
    assert w.plan(1)["ahead"] is True
    b = bestla.Batch([(w, x, y) for x, y in zip(xs, ys)])
    p = b.plan()
    assert p["kernel"] == "woq_gemv_m1_kernel" and p["ahead"] is False and p["m1_spec"] is False, p
    b.run()
    torch.cuda.synchronize()
    for x, y in zip(xs, ys):
        assert torch.equal(y, w.forward(x.view(1, k))[0])


def test_graph_replay(oracle, knob):
    """one load-ahead launch captured and replayed three times gives the eager result each time"""
    n, k = N1, 4096
    _, w = _weight(oracle, n, k)
    x, _ = _act(k)
    knob("NAD_GEMV_AHEAD", "1")
    assert w.plan(1)["ahead"] is True
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
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, y0)
