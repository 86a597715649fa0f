"""The specialised M = 1 decode GEMV (woq_gemv_m1s_kernel: compact argument block, weight count / reduce / epilogue
class at compile time) against the oracle and against the general M = 1 kernel.

Every case checks
  1. the default path against the oracle at the M = 1 bar of tests/test_gpu_parity.py (2e-5 of max|C|),
  2. the default path against NAD_GEMV_M1_SPEC=0 (every launch on woq_gemv_m1_kernel with the full GemvArgs) bit for bit:
     the specialised kernel keeps the summation order,
  3. where one weight is launched alone, the dry run: which kernel serves the call and whether it is the specialised one.

Shapes are the smallest at which each path can go wrong (M = 1; int4 g128 sym, fp16 scales, fp32 activations unless the
case says otherwise).
"""
import numpy as np
import pytest

from tests.conftest import gpu_available
from tests.oracle_lib import BF16, F16, S2, S4

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

TOL = 2e-5  # tests/test_gpu_parity.py TOL_DECODE

_CACHE = {}


def _weight(oracle, n, k, bs=128, qt=S4, st=F16, asym=False, seed=0):
    """(blob, DeviceWeight) of one geometry, packed once per session"""
    key = (n, k, bs, qt, st, asym, seed)
    if key not in _CACHE:
        W = np.random.default_rng(1000 + seed + n + k).uniform(-0.5, 0.5, size=(n, k)).astype(np.float32)
        core = oracle.lib.orc_select_core(4, qt, bs, int(asym), 0)
        blob = oracle.quant_pack(W, n, k, bs, qt, st, asym, core, is_trans=True)
        _CACHE[key] = (blob, bestla.DeviceWeight(blob))
    return _CACHE[key]


def _act(k, seed=0):
    key = ("A", k, seed)
    if key not in _CACHE:
        _CACHE[key] = np.random.default_rng(seed + k).uniform(-0.5, 0.5, size=(1, k)).astype(np.float32)
    return _CACHE[key]


def _ref(oracle, A, blob, n, k, tag):
    key = ("ref", tag)
    if key not in _CACHE:
        _CACHE[key] = oracle.forward(A, blob, n, k).astype(np.float64)
    return _CACHE[key]


def _check(y, ref):
    err = float(np.abs(y.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))
    assert err <= TOL, (err, TOL)


def _both(knob, run):
    """run() on the default path and with NAD_GEMV_M1_SPEC=0; returns (default, general) as numpy"""
    y = run()
    knob("NAD_GEMV_M1_SPEC", "0")
    y0 = run()
    knob("NAD_GEMV_M1_SPEC", None)
    return y, y0


def _gelu(x):
    return 0.5 * x * (1 + np.tanh(0.7978845834732056 * (x + 0.044714998453855515 * x ** 3)))


def _silu(x):
    return x / (1 + np.exp(-x))


def _plan_is(w, knob, spec, act="fp32"):
    p = w.plan(1, act)
    assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is spec, p
    knob("NAD_GEMV_M1_SPEC", "0")
    p = w.plan(1, act)
    assert p["kernel"] == "woq_gemv_m1_kernel" and p["m1_spec"] is False, p
    knob("NAD_GEMV_M1_SPEC", None)


SINGLE = [
    # id, n, k, bs, qtype, stype, asym, {knobs}, threads of the launch
    ("lean16_3stripes", 48, 4096, 128, S4, F16, False, {}, 1024),
    ("grid2_remainder", 48, 4096, 128, S4, F16, False, {"NAD_GEMV_GRID": "2"}, 1024),
    ("ragged_last_stripe", 40, 4096, 128, S4, F16, False, {}, 1024),
    ("two_one_tile_slices", 32, 256, 128, S4, F16, False, {}, 128),
    ("idle_waves_general_reduce", 32, 256, 128, S4, F16, False, {"NAD_GEMV_WAVES": "16"}, 1024),
    ("down_4tile_22_slices", 32, 11008, 128, S4, F16, False, {}, 11 * 64),
    ("asym_bf16_scales", 48, 4096, 128, S4, BF16, True, {}, 1024),
    ("int2_g64", 32, 4096, 64, S2, F16, False, {}, 1024),
]


@pytest.mark.parametrize("cfg", SINGLE, ids=[c[0] for c in SINGLE])
def test_single_weight(oracle, knob, cfg):
    name, n, k, bs, qt, st, asym, knobs, threads = cfg
    blob, w = _weight(oracle, n, k, bs, qt, st, asym)
    A = _act(k)
    ref = _ref(oracle, A, blob, n, k, (n, k, bs, qt, st, asym))
    for kn, v in knobs.items():
        knob(kn, v)
    assert w.plan(1)["threads"] == threads, w.plan(1)
    _plan_is(w, knob, True)
    x = torch.from_numpy(A).cuda()
    y, y0 = _both(knob, lambda: w.forward(x).cpu().numpy())
    _check(y, ref)
    assert np.array_equal(y, y0)


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_half_activations(oracle, knob, dt):
    n, k = 48, 4096
    blob, w = _weight(oracle, n, k)
    x = torch.from_numpy(_act(k)).cuda().to(torch.float16 if dt == "fp16" else torch.bfloat16)
    ref = _ref(oracle, x.float().cpu().numpy(), blob, n, k, ("half", dt))
    _plan_is(w, knob, True, dt)
    y, y0 = _both(knob, lambda: w.forward(x).cpu().numpy())
    _check(y, ref)
    assert np.array_equal(y, y0)


def test_fused_qkv_unequal_widths(oracle, knob):
    k, ns = 4096, (48, 16, 32)
    ws = [_weight(oracle, n, k, seed=10 + i) for i, n in enumerate(ns)]
    A = _act(k)
    x = torch.from_numpy(A).cuda()
    ys, ys0 = _both(knob, lambda: [t.cpu().numpy() for t in bestla.qkv_forward(x, *[w for _, w in ws])])
    for i, (y, y0, (blob, _), n) in enumerate(zip(ys, ys0, ws, ns)):
        _check(y, _ref(oracle, A, blob, n, k, ("qkv", i)))
        assert np.array_equal(y, y0)


@pytest.mark.parametrize("act,aux", [("silu", True), ("silu", False), ("gelu", True)])
def test_gate_up_pair(oracle, knob, act, aux):
    """SiLU*mul is the specialised kernel's pair form (with and without the act(gate) output); GELU*mul stays on the
    general kernel's runtime switch."""
    n, k = 48, 4096
    (b1, w1), (b3, w3) = _weight(oracle, n, k, seed=21), _weight(oracle, n, k, seed=23)
    A = _act(k)
    x = torch.from_numpy(A).cuda()
    h1, h3 = _ref(oracle, A, b1, n, k, ("gate",)), _ref(oracle, A, b3, n, k, ("up",))
    t1_ref = _silu(h1) if act == "silu" else _gelu(h1)

    def run():
        tmp1 = torch.zeros((1, n), dtype=torch.float32, device="cuda") if aux else None
        y = bestla.ffn_gate_up(x, w1, w3, act=act, tmp1=tmp1)
        return np.concatenate([y.cpu().numpy(), tmp1.cpu().numpy() if aux else np.zeros((1, n), np.float32)])

    y, y0 = _both(knob, run)
    _check(y[:1], t1_ref * h3)
    if aux:
        _check(y[1:], t1_ref)
    assert np.array_equal(y, y0)


@pytest.mark.parametrize("epi", ["bias", "gelu", "bias_gelu", "silu", "residual"])
def test_other_epilogues_stay_general(oracle, knob, epi):
    n, k = 48, 4096
    blob, w = _weight(oracle, n, k)
    A = _act(k)
    ref = _ref(oracle, A, blob, n, k, (n, k, 128, S4, F16, False))
    rng = np.random.default_rng(7)
    b = rng.uniform(-1, 1, size=(n,)).astype(np.float32)
    r = rng.uniform(-1, 1, size=(1, n)).astype(np.float32)
    x, tb, tr = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(r).cuda()
    kw, want = {
        "bias": (dict(epilogue=bestla.EPI_BIAS, bias=tb), ref + b),
        "gelu": (dict(epilogue=bestla.EPI_GELU), _gelu(ref)),
        "bias_gelu": (dict(epilogue=bestla.EPI_ADD_GELU, bias=tb), _gelu(ref + b)),
        "silu": (dict(epilogue=bestla.EPI_SILU), _silu(ref)),
        "residual": (dict(epilogue=bestla.EPI_RES_ADD, residual=tr), ref + r),
    }[epi]
    y, y0 = _both(knob, lambda: w.forward(x, **kw).cpu().numpy())
    _check(y, want)
    assert np.array_equal(y, y0)


def test_batch_of_three(oracle, knob):
    """the batched kernel is unchanged: one launch of 3 problems equals 3 single launches on either path"""
    n, k = 32, 4096
    blob, w = _weight(oracle, n, k)
    xs = [torch.from_numpy(_act(k, seed=i)).cuda().view(k) for i in range(3)]

    def run():
        ys = [torch.zeros(n, device="cuda") for _ in xs]
        bestla.Batch([(w, x, y) for x, y in zip(xs, ys)]).run()
        return np.stack([y.cpu().numpy() for y in ys])

    y, y0 = _both(knob, run)
    assert np.array_equal(y, y0)
    for i, x in enumerate(xs):
        _check(y[i:i + 1], _ref(oracle, _act(k, seed=i), blob, n, k, ("batch", i)))
        assert np.array_equal(y[i], w.forward(x.view(1, k)).cpu().numpy()[0])


def test_graph_replay(oracle):
    """the compact argument block is a kernel argument: it must survive capture, and every replay equals eager"""
    n, k = 48, 4096
    _, w = _weight(oracle, n, k)
    assert w.plan(1)["m1_spec"] is True
    x = torch.from_numpy(_act(k)).cuda()
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
