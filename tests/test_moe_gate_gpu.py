"""nad_moe_gate_route on the GPU: the gate matmul and the router in one launch (moe_gate_route_kernel).

Bars:
  * the logits against tests/gate_model.py (the header's order of sums in numpy float32): BIT-identical, compared as
    uint32 -- and the model itself inside its derived bound of the float64 dot product (printed per case;
    profiles/moe_gate_errors.txt holds the figures);
  * ids and wts against bestla.moe_route on the logits the call wrote: identical (int32 / uint32), since both kernels
    run one device function; ids against the stable argsort of the model's logits;
  * a row's logits, ids and wts do not depend on m or on the row's index; an fp16 / bf16 gate gives the bits of its fp32
    widening.

The shapes are the smallest at which the kernel can go wrong: K = 4 (one live slot), 36 (part of one wave), 4096
(exactly one pass), 4100 (one pass plus one slot), 12292 (three passes plus a tail); n_expert 1, 3, 8 (the 8-expert
instantiation), 64 (the 64-expert one; 16 is covered by the ties and window tests at n_expert = 12).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from neural_amd import bestla  # noqa: E402
from neural_amd._lib import check, lib  # noqa: E402
from tests import edges, gate_model  # noqa: E402

KS = (4, 36, 4096, 4100, 12292)
NES = (1, 3, 8, 64)
M = 5

_DATA = {}


def _data(k, ne, m=M):
    """(x [m][k], gate [ne][k], the model's logits, their float64 reference) for a shape, made once and shared.  The
    draw is repeated until the model's logits of a row are 1e-5 apart: the routing tests compare against an argsort of
    them, which a near-tie inside expf's rounding would not define."""
    key = (k, ne, m)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * k + 10 * ne + m)
        while True:
            x = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
            g = rng.uniform(-0.5, 0.5, size=(ne, k)).astype(np.float32)
            lg = gate_model.logits(x, g)
            if ne == 1 or np.diff(np.sort(lg, axis=1), axis=1).min() > 1e-5:
                break
        for a in (x, g, lg):
            a.setflags(write=False)
        _DATA[key] = (x, g, lg, x.astype(np.float64) @ g.astype(np.float64).T)
    return _DATA[key]


def _padded(values, pad, dtype=torch.float32):
    """numpy [r][c] -> cuda view [r][c] of dtype with row stride c + pad, NaN in the padding"""
    r, c = values.shape
    win = torch.full((r, c + pad), float("nan"), dtype=dtype, device="cuda")[:, :c]
    win.copy_(_cuda(values).to(dtype))
    assert win.stride(0) == c + pad and win.data_ptr() % 16 == 0
    return win


def _call(x, gate, top_k, ids, wts, logits=None, stream=None):
    """the entry on outputs of the caller's (any row strides)"""
    m, k = x.shape
    check(lib().nad_moe_gate_route(bestla._ptr(x), x.stride(0), bestla._ptr(gate), bestla._act_code(gate),
                                   gate.stride(0), m, k, gate.shape[0], top_k, bestla._ptr(ids), ids.stride(0),
                                   bestla._ptr(wts), wts.stride(0), bestla._ptr(logits),
                                   logits.stride(0) if logits is not None else 0, bestla._stream(stream)),
          "nad_moe_gate_route")


def _cuda(a):
    """a copy on the device (the shared arrays are read-only)"""
    return torch.from_numpy(np.array(a)).cuda()


def _u32(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _top_ks(ne):
    return sorted({1, min(2, ne), ne})


# ------------------------------------------------------------------------------------------------ 1. logits, 2. routing
@pytest.mark.parametrize("ne", NES)
@pytest.mark.parametrize("k", KS)
def test_logits_are_the_models_bits_and_routing_is_moe_routes(k, ne):
    x_h, g_h, model, ref64 = _data(k, ne)
    x, gate = _padded(x_h, 8), _padded(g_h, 12)  # lda = k + 8, ldw = k + 12, NaN behind every row
    err = float(np.abs(model.astype(np.float64) - ref64).max())
    bnd = gate_model.bound(x_h, g_h)
    print(f"K={k} n_expert={ne} m={M}: model vs float64 worst err {err:.3e}, bound {bnd.min():.3e} .. {bnd.max():.3e}")
    assert (np.abs(model.astype(np.float64) - ref64) <= bnd).all()
    for top_k in _top_ks(ne):
        ids, wts, logits = bestla.moe_gate_route(x, gate, top_k, return_logits=True)
        assert np.array_equal(_u32(logits), _u32(model)), (k, ne, top_k)
        r_ids, r_wts = bestla.moe_route(logits, top_k)
        assert torch.equal(ids, r_ids) and np.array_equal(_u32(wts), _u32(r_wts)), (k, ne, top_k)
        assert np.array_equal(ids.cpu().numpy(), gate_model.stable_top_k(model, top_k)), (k, ne, top_k)
        # without the logits output: the same routing
        ids2, wts2 = bestla.moe_gate_route(x, gate, top_k)
        assert torch.equal(ids2, ids) and np.array_equal(_u32(wts2), _u32(wts)), (k, ne, top_k)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("k", [36, 4100])
@pytest.mark.parametrize("ne", [8, 64])
def test_narrow_gate_gives_the_bits_of_its_fp32_widening(k, ne, dtype):
    x_h, g_h, _, _ = _data(k, ne)
    x = _padded(x_h, 8)
    g16 = _padded(g_h, 12, edges.torch_dtype(dtype))
    wide_h = g16.float().cpu().numpy()  # exact
    g32 = _padded(wide_h, 4)
    top_k = min(2, ne)
    ids, wts, logits = bestla.moe_gate_route(x, g16, top_k, return_logits=True)
    ids32, wts32, logits32 = bestla.moe_gate_route(x, g32, top_k, return_logits=True)
    assert np.array_equal(_u32(logits), _u32(logits32))
    assert np.array_equal(_u32(logits), _u32(gate_model.logits(x_h, wide_h)))
    assert torch.equal(ids, ids32) and np.array_equal(_u32(wts), _u32(wts32))


# ------------------------------------------------------------------------------------------------ 3. batch invariance
@pytest.mark.parametrize("k,ne,dtype", [(4100, 8, "fp32"), (4096, 64, "fp32"), (4100, 8, "fp16")])
def test_a_row_is_routed_the_same_alone_and_in_a_batch(k, ne, dtype):
    m = 67
    x_h, g_h, model, _ = _data(k, ne, m)
    x = _cuda(x_h)
    gate = _cuda(g_h).to(edges.torch_dtype(dtype))
    ids, wts, logits = bestla.moe_gate_route(x, gate, 2, return_logits=True)
    if dtype == "fp32":
        assert np.array_equal(_u32(logits), _u32(model))
    for r in (0, 33, 66):
        ids1, wts1, logits1 = bestla.moe_gate_route(x[r:r + 1], gate, 2, return_logits=True)
        assert np.array_equal(_u32(logits1), _u32(logits[r:r + 1])), r
        assert torch.equal(ids1, ids[r:r + 1]) and np.array_equal(_u32(wts1), _u32(wts[r:r + 1])), r


# ------------------------------------------------------------------------------------------------ 4. ties
@pytest.mark.parametrize("ne", [8, 12])
def test_identical_gate_rows_tie_to_the_lower_index(ne):
    k = 4100
    x_h, g_h, _, _ = _data(k, ne)
    g_h = g_h.copy()
    g_h[5] = g_h[2]
    ids, wts, logits = bestla.moe_gate_route(_cuda(x_h), _cuda(g_h), ne, return_logits=True)
    lg, ids, wts = _u32(logits), ids.cpu().numpy(), _u32(wts)
    assert np.array_equal(lg[:, 2], lg[:, 5])
    assert np.array_equal(lg, _u32(gate_model.logits(x_h, g_h)))
    for r in range(M):
        at2, at5 = int(np.where(ids[r] == 2)[0][0]), int(np.where(ids[r] == 5)[0][0])
        assert at5 == at2 + 1, (r, ids[r])
        assert wts[r, at2] == wts[r, at5], r


# ------------------------------------------------------------------------------------------------ 5. windows
@pytest.mark.parametrize("k,ne,top_k,logits_out", [(36, 3, 2, True), (4100, 12, 3, True), (4100, 8, 2, False)])
def test_the_call_writes_its_windows_and_nothing_else(k, ne, top_k, logits_out):
    x_h, g_h, model, _ = _data(k, ne)
    x, gate = _padded(x_h, 8), _padded(g_h, 12)
    ids_ld, wts_ld, lg_ld = top_k + 3, top_k + 5, ne + 7
    can = edges.Canary((edges.G + M + edges.G) * (ids_ld + wts_ld + lg_ld))
    at = edges.G * ids_ld
    ids_w = can.window(at, M, top_k, ids_ld)
    at += (M + edges.G) * ids_ld + edges.G * wts_ld
    wts_w = can.window(at, M, top_k, wts_ld)
    at += (M + edges.G) * wts_ld + edges.G * lg_ld
    lg_w = can.window(at, M, ne, lg_ld) if logits_out else None
    ids_i = ids_w.view(torch.int32)  # the same words as int32: an unwritten id stays the canary, a NaN to check()
    assert ids_i.stride(0) == ids_ld

    # garbage in the windows beforehand, the call made twice: the same bits both times, the canary everywhere else
    for w in can.windows:
        w.fill_(float("inf"))
    got = edges.twice(can, lambda: _call(x, gate, top_k, ids_i, wts_w, lg_w), f"moe_gate_route K={k} n_expert={ne}")
    ids, wts = got[0].view(np.int32), got[1]
    p_ids, p_wts, p_lg = bestla.moe_gate_route(x, gate, top_k, return_logits=True)
    assert np.array_equal(ids, p_ids.cpu().numpy()) and np.array_equal(_u32(wts), _u32(p_wts))
    assert np.array_equal(_u32(p_lg), _u32(model))
    if logits_out:
        assert np.array_equal(_u32(got[2]), _u32(model))


# ------------------------------------------------------------------------------------------------ 6. graph
def test_a_replay_follows_x_and_the_gate_as_rewritten_on_the_device():
    k, ne, top_k = 4100, 8, 2
    xa, ga, _, _ = _data(k, ne)
    xb, gb, _, _ = _data(k, ne, m=M + 1)
    sets = [(xa, ga), (xb[:M], gb)]
    eager = []
    for x_h, g_h in sets:
        e = bestla.moe_gate_route(_cuda(x_h), _cuda(g_h), top_k, return_logits=True)
        eager.append([t.cpu().numpy() for t in e])
    assert not np.array_equal(eager[0][2], eager[1][2])
    x, gate = _cuda(xa), _cuda(ga)
    ids = torch.empty((M, top_k), dtype=torch.int32, device="cuda")
    wts = torch.empty((M, top_k), device="cuda")
    logits = torch.empty((M, ne), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(x, gate, top_k, ids, wts, logits, stream=s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            _call(x, gate, top_k, ids, wts, logits, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    for which in (0, 1, 0):
        x.copy_(_cuda(sets[which][0]))
        gate.copy_(_cuda(sets[which][1]))
        ids.fill_(-1)
        wts.fill_(float("nan"))
        logits.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), eager[which][0]), which
        assert np.array_equal(_u32(wts), _u32(eager[which][1])), which
        assert np.array_equal(_u32(logits), _u32(eager[which][2])), which


# ------------------------------------------------------------------------------------------------ 7. chain
def test_gate_route_then_moe_ffn_is_route_of_the_models_logits_then_moe_ffn(oracle):
    from tests.test_moe_gpu import FIN, NE, _ffn_banks

    (_, _, gate_b), (_, _, up_b), (_, _, down_b) = _ffn_banks(oracle, "int4_sym")
    x_h, g_h, model, _ = _data(FIN, NE)
    x, gate = _cuda(x_h), _cuda(g_h)
    ids, wts = bestla.moe_gate_route(x, gate, 2)
    out = bestla.moe_ffn(gate_b, up_b, down_b, x, ids, wts).clone()
    ids_m, wts_m = bestla.moe_route(_cuda(model), 2)
    assert torch.equal(ids, ids_m) and np.array_equal(_u32(wts), _u32(wts_m))
    out_m = bestla.moe_ffn(gate_b, up_b, down_b, x, ids_m, wts_m)
    assert not torch.isnan(out).any()
    assert np.array_equal(_u32(out), _u32(out_m))
