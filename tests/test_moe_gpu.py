"""Routed expert matmuls on the GPU: nad_device_mul_mat_id, nad_device_moe_ffn, nad_moe_route (ne_mul_mat_id /
ne_mul_id_ffn_silu and the router of models/llama/llama.cpp:620-688), routing read on the device.

Parity bars:
  * a routed row against its expert's own one-problem call (DeviceWeight.forward / ffn_gate_up at M = 1): BIT-identical
    -- a stripe is reduced by the same waves, K-slices and wave order whichever launch serves it;
  * mul_mat_id against the oracle: TOL_DECODE = 2e-5 of max|ref|, the bar of tests/test_batch_gpu.py;
  * moe_ffn's combine against numpy float32 on the device's own slot results (tests/test_moe_cpu.py combine_f32): no
    tolerance; against the float64 chain on the oracle: 2 * TOL["fp32"], the bar tests/test_gemm2_gpu.py uses for the
    same gate/up -> down chain;
  * the router's weights: four times the error numpy float32 shows on the same steps against float64 (computed here;
    the factor covers the device expf against numpy's).  The test prints both figures; profiles/moe_errors.txt holds
    them as measured.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from neural_amd import bestla  # noqa: E402
from tests import edges  # noqa: E402
from tests.oracle_lib import BF16, F16, F32, S2, S4  # noqa: E402
from tests.test_gemm2_gpu import TOL  # noqa: E402
from tests.test_gpu_parity import _blob, _rel_err  # noqa: E402
from tests.test_moe_cpu import combine_f32  # noqa: E402

TOL_DECODE = 2e-5
NE = 4
FIN, FMID, FOUT = 1024, 512, 300

FORMATS = {
    "int4_g128_f16_sym": (128, S4, F16, False),
    "int4_g128_bf16_asym": (128, S4, BF16, True),
    "int2_g64_f16": (64, S2, F16, False),
    "int4_perchannel_f32": (None, S4, F32, False),
}

_CACHE = {}


def _experts(oracle, n, k, fmt, tag):
    """NE experts of one shape and format: (blobs, DeviceWeights, ExpertBank), built once and shared"""
    key = (n, k, fmt, tag)
    if key not in _CACHE:
        bs, qt, st, asym = FORMATS[fmt]
        blobs = [_blob(oracle, n, k, bs or k, qt, st, asym, 4, seed=zlib.crc32(repr(key).encode()) % 10000 + 31 * e)
                 for e in range(NE)]
        ws = [bestla.DeviceWeight(b) for b in blobs]
        _CACHE[key] = (blobs, ws, bestla.ExpertBank(ws))
    return _CACHE[key]


def _ids(m, width, rng):
    """ids [m][width] over experts 0, 1, 2 (expert 3 stays unchosen), every row's entries distinct, experts repeated
    across rows"""
    ids = np.stack([rng.permutation(3)[:width] if width <= 3 else rng.integers(0, 3, size=width) for _ in range(m)])
    if m > 1:
        ids[1] = ids[0]
    return ids.astype(np.int32)


# ------------------------------------------------------------------------------------------------ mul_mat_id
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("m,n,k", [(1, 300, 1024), (5, 300, 1024), (3, 1024, 4096), (200, 64, 256)])
def test_mul_mat_id_rows_are_their_experts_forwards(oracle, fmt, m, n, k):
    blobs, ws, bank = _experts(oracle, n, k, fmt, "mmid")
    rng = np.random.default_rng(m * 13 + n)
    A = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    ids = _ids(m, 3, rng)  # ids_ld = 3 > the two slots used
    ids_t = torch.from_numpy(ids).cuda()
    singles = {}
    refs = {e: oracle.forward(A, blobs[e], n, k) for e in range(3)}  # every row on every expert it may be routed to
    for slot in (0, 1):
        out = torch.full((m, n), float("nan"), device="cuda")
        got = bestla.mul_mat_id(bank, x, ids_t, slot, out=out).cpu().numpy()
        assert not np.isnan(got).any()
        for r in range(m):
            e = int(ids[r, slot])
            if (r, e) not in singles:
                singles[(r, e)] = ws[e].forward(x[r:r + 1]).cpu().numpy()[0]
            assert np.array_equal(got[r], singles[(r, e)]), (slot, r, e, float(np.abs(got[r] - singles[(r, e)]).max()))
            err = _rel_err(got[r], refs[e][r])
            assert err <= TOL_DECODE, (slot, r, e, err)


@pytest.mark.parametrize("align", edges.ALIGNS)
def test_mul_mat_id_window(oracle, align):
    n, k, m = 300, 1024, 5
    blobs, ws, bank = _experts(oracle, n, k, "int4_g128_f16_sym", "mmid")
    rng = np.random.default_rng(9)
    A = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    xt = torch.from_numpy(A).cuda()
    # both activation layouts keep rows 16-B aligned (the entry's contract): the NaN padding sits behind each row, and
    # for "odd" the rows are a view into a wider storage at column 8
    if align == "odd":
        store = torch.full((m, k + 24), float("nan"), device="cuda")
        x = store[:, 8:8 + k]
        x.copy_(xt)
    else:
        x = edges.act_window(xt, "aligned")
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
    ids = torch.from_numpy(_ids(m, 2, rng)).cuda()
    can, out = edges.out_window(m, n, align)
    (y,) = edges.twice(can, lambda: bestla.mul_mat_id(bank, x, ids, 1, out=out), f"mul_mat_id {align}")
    for r in range(m):
        e = int(ids[r, 1])
        assert np.array_equal(y[r], ws[e].forward(xt[r:r + 1]).cpu().numpy()[0])


def test_mul_mat_id_refuses_unaligned_rows(oracle):
    n, k = 300, 1024
    _, _, bank = _experts(oracle, n, k, "int4_g128_f16_sym", "mmid")
    flat = torch.zeros(2 * (k + 2) + 1, device="cuda")
    ids = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="16-B aligned base and lda % 4 == 0"):
        bestla.mul_mat_id(bank, flat[:2 * (k + 2)].view(2, k + 2)[:, :k], ids, 0)  # lda = k + 2
    with pytest.raises(RuntimeError, match="16-B aligned base and lda % 4 == 0"):
        bestla.mul_mat_id(bank, flat[1:1 + 2 * k].view(2, k), ids, 0)  # base 4 bytes off


# ------------------------------------------------------------------------------------------------ moe_ffn
POLICIES = {
    "int4_sym": ("int4_g128_f16_sym", "int4_g128_f16_sym"),
    "int4_asym_bf16": ("int4_g128_bf16_asym", "int4_g128_bf16_asym"),
    "int2_g64_gate_up_int4_down": ("int2_g64_f16", "int4_g128_f16_sym"),
}


def _ffn_banks(oracle, policy):
    gu, dn = POLICIES[policy]
    return (_experts(oracle, FMID, FIN, gu, "gate"), _experts(oracle, FMID, FIN, gu, "up"),
            _experts(oracle, FOUT, FMID, dn, "down"))


def _act64(v, act):
    return edges.silu64(v) if act == "silu" else edges.gelu64(v)


def _chain64(oracle, A, ids, wts, banks, act):
    """the float64 chain on the oracle's products, router weights from the same fp32 wts"""
    (gb, _, _), (ub, _, _), (db, _, _) = banks
    m, top_k = ids.shape
    out = np.zeros((m, FOUT), np.float64)
    for r in range(m):
        for i in range(top_k):
            e = int(ids[r, i])
            h1 = oracle.forward(A[r:r + 1], gb[e], FMID, FIN).astype(np.float64)
            h3 = oracle.forward(A[r:r + 1], ub[e], FMID, FIN).astype(np.float64)
            t = (_act64(h1, act) * h3).astype(np.float32)
            out[r] += float(wts[r, i]) * oracle.forward(t, db[e], FOUT, FMID).astype(np.float64)[0]
    return out


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("m,top_k", [(1, 1), (1, 2), (2, 1), (2, 2), (5, 1), (5, 2)])
def test_moe_ffn(oracle, policy, act, m, top_k):
    banks = _ffn_banks(oracle, policy)
    (_, gw, gate), (_, uw, up), (_, dw, down) = banks
    rng = np.random.default_rng(100 * m + top_k)
    A = rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    ids = _ids(m, top_k, rng)
    w = rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    out = torch.full((m, FOUT), float("nan"), device="cuda")
    _, t_ws, y_ws = bestla.moe_workspace(m, top_k, FMID, FOUT, x.device)
    t_ws.fill_(float("nan"))
    y_ws.fill_(float("nan"))
    got = bestla.moe_ffn(gate, up, down, x, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), act=act,
                         out=out).cpu().numpy()
    t, y = t_ws.clone(), y_ws.clone()
    # (i) the workspace rows are the one-problem calls, bit for bit
    for r in range(m):
        for i in range(top_k):
            p, e = r * top_k + i, int(ids[r, i])
            t1 = bestla.ffn_gate_up(x[r:r + 1], gw[e], uw[e], act=act)
            assert torch.equal(t[p:p + 1], t1), (p, e)
            assert torch.equal(y[p:p + 1], dw[e].forward(t[p:p + 1])), (p, e)
    # (ii) the combine is numpy float32 on the device's own y, no tolerance
    assert np.array_equal(got, combine_f32(y.cpu().numpy(), w, top_k))
    # (iii) the float64 chain on the oracle
    ref = _chain64(oracle, A, ids, w, banks, act)
    err = _rel_err(got, ref)
    print(f"moe_ffn {policy} {act} m={m} top_k={top_k}: err {err:.3e} bound {2 * TOL['fp32']:.1e}")
    assert err <= 2 * TOL["fp32"], err


def test_moe_ffn_strided_ids_and_weights_and_own_workspace(oracle):
    """ids and wts as column slices of wider tensors (ids_ld = 5, wts_ld = 7 > top_k = 2), the padding columns holding
    out-of-range ids and NaN weights, and a caller's workspace: the same bits as the contiguous call."""
    (_, _, gate), (_, _, up), (_, _, down) = _ffn_banks(oracle, "int4_sym")
    m, top_k = 5, 2
    rng = np.random.default_rng(33)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    ids = torch.from_numpy(_ids(m, top_k, rng)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)).cuda()
    plain = bestla.moe_ffn(gate, up, down, x, ids, w).cpu().numpy()
    ids_wide = torch.full((m, 5), 1 << 20, dtype=torch.int32, device="cuda")
    w_wide = torch.full((m, 7), float("nan"), device="cuda")
    ids_wide[:, 2:4] = ids
    w_wide[:, 3:5] = w
    ids_v, w_v = ids_wide[:, 2:4], w_wide[:, 3:5]
    assert ids_v.stride(0) == 5 and w_v.stride(0) == 7
    own = bestla.moe_workspace_alloc(m, top_k, FMID, FOUT)
    own.fill_(float("nan"))
    held_t = bestla.moe_workspace(m, top_k, FMID, FOUT, x.device)[1]
    held_t.fill_(float("nan"))
    got = bestla.moe_ffn(gate, up, down, x, ids_v, w_v, workspace=own).cpu().numpy()
    assert np.array_equal(got, plain)
    t, y = bestla.moe_workspace_rows(own, m, top_k, FMID, FOUT)
    assert not torch.isnan(t).any() and not torch.isnan(y).any()
    assert torch.isnan(held_t).all()  # the held workspace was not used
    assert np.array_equal(got, combine_f32(y.cpu().numpy(), w.cpu().numpy(), top_k))


@pytest.mark.parametrize("align", edges.ALIGNS)
def test_moe_ffn_window(oracle, align):
    (_, _, gate), (_, _, up), (_, _, down) = _ffn_banks(oracle, "int4_sym")
    m, top_k = 5, 2
    rng = np.random.default_rng(21)
    A = rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)
    xt = torch.from_numpy(A).cuda()
    if align == "odd":
        store = torch.full((m, FIN + 24), float("nan"), device="cuda")
        x = store[:, 8:8 + FIN]
        x.copy_(xt)
    else:
        x = edges.act_window(xt, "aligned")
    ids = torch.from_numpy(_ids(m, top_k, rng)).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)).cuda()
    can, out = edges.out_window(m, FOUT, align)
    (y,) = edges.twice(can, lambda: bestla.moe_ffn(gate, up, down, x, ids, w, out=out), f"moe_ffn {align}")
    plain = bestla.moe_ffn(gate, up, down, xt, ids, w).cpu().numpy()
    assert np.array_equal(y, plain)


def test_routing_is_read_at_replay(oracle):
    """moe_ffn captured once; ids and wts overwritten on the device between replays: each replay is the eager result
    for the ids it found, bit for bit."""
    (_, _, gate), (_, _, up), (_, _, down) = _ffn_banks(oracle, "int4_sym")
    m, top_k = 2, 2
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    choices = [(np.array([[0, 1], [2, 0]], np.int32), np.array([[0.7, 0.3], [0.4, 0.6]], np.float32)),
               (np.array([[3, 2], [1, 3]], np.int32), np.array([[0.2, 0.8], [0.9, 0.1]], np.float32))]
    eager = []
    for ids_h, w_h in choices:
        eager.append(bestla.moe_ffn(gate, up, down, x, torch.from_numpy(ids_h).cuda(),
                                    torch.from_numpy(w_h).cuda()).cpu().numpy())
    assert not np.array_equal(eager[0], eager[1])
    ids = torch.from_numpy(choices[0][0]).cuda()
    w = torch.from_numpy(choices[0][1]).cuda()
    out = torch.empty((m, FOUT), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bestla.moe_ffn(gate, up, down, x, ids, w, out=out, stream=s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            bestla.moe_ffn(gate, up, down, x, ids, w, out=out, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    for which in (0, 1, 0):
        ids.copy_(torch.from_numpy(choices[which][0]))
        w.copy_(torch.from_numpy(choices[which][1]))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager[which]), which


# ------------------------------------------------------------------------------------------------ out-of-range ids
@pytest.mark.parametrize("bad", [-1, NE])
def test_out_of_range_id_is_a_zero_problem(oracle, bad):
    n, k, m = 300, 1024, 3
    _, ws, bank = _experts(oracle, n, k, "int4_g128_bf16_asym", "mmid")
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)).cuda()
    good = np.array([[0, 1], [2, 0], [1, 2]], np.int32)
    ids = good.copy()
    ids[1, 0] = bad
    base = bestla.mul_mat_id(bank, x, torch.from_numpy(good).cuda(), 0).cpu().numpy()
    out = torch.full((m, n), float("nan"), device="cuda")
    got = bestla.mul_mat_id(bank, x, torch.from_numpy(ids).cuda(), 0, out=out).cpu().numpy()
    assert np.array_equal(got[1], np.zeros(n, np.float32))
    assert np.array_equal(got[[0, 2]], base[[0, 2]])

    (_, _, gate), (_, _, up), (_, _, down) = _ffn_banks(oracle, "int4_sym")
    xf = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    w = rng.uniform(0.1, 1.0, size=(m, 2)).astype(np.float32)
    _, _, y_ws = bestla.moe_workspace(m, 2, FMID, FOUT, xf.device)
    bestla.moe_ffn(gate, up, down, xf, torch.from_numpy(good).cuda(), torch.from_numpy(w).cuda())
    y = y_ws.cpu().numpy().copy()
    y[2] = 0  # problem p = 1 * top_k + 0
    got = bestla.moe_ffn(gate, up, down, xf, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    assert np.array_equal(y_ws.cpu().numpy(), y)
    assert np.array_equal(got, combine_f32(y, w, 2))


# ------------------------------------------------------------------------------------------------ router
def _route_f(logits, top_k, dt):
    """the header's steps in dtype dt: (ids, wts)"""
    x = logits.astype(dt)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True, dtype=dt)
    ids = np.argsort(-p, axis=1, kind="stable")[:, :top_k]
    sel = np.take_along_axis(p, ids, axis=1)
    tot = sel[:, 0].copy()
    for i in range(1, top_k):
        tot = (tot + sel[:, i]).astype(dt)
    return ids.astype(np.int32), (sel / tot[:, None]).astype(dt)


def _logits(m, ne, rng):
    while True:
        x = rng.uniform(-8, 8, size=(m, ne)).astype(np.float32)
        if ne == 1 or np.diff(np.sort(x, axis=1), axis=1).min() > 1e-3:
            return x


@pytest.mark.parametrize("top_k", [1, 2, 4])
@pytest.mark.parametrize("ne", [4, 8, 64])
def test_route(ne, top_k):
    m = 7
    x = _logits(m, ne, np.random.default_rng(ne * 10 + top_k))
    ids, wts = bestla.moe_route(torch.from_numpy(x).cuda(), top_k)
    ids, wts = ids.cpu().numpy(), wts.cpu().numpy()
    ids64, w64 = _route_f(x, top_k, np.float64)
    ids32, w32 = _route_f(x, top_k, np.float32)
    assert w32.dtype == np.float32
    assert np.array_equal(ids, np.argsort(-x, axis=1, kind="stable")[:, :top_k])
    assert np.array_equal(ids, ids64) and np.array_equal(ids32, ids64)
    np_err = float(np.abs(w32.astype(np.float64) - w64).max())
    bound = 4 * np_err  # top_k = 1: p / p = 1 in every arithmetic, so the bound and both errors are 0
    err = float(np.abs(wts.astype(np.float64) - w64).max())
    sum_err = float(np.abs(wts.astype(np.float64).sum(axis=1) - 1).max())
    print(f"route n_expert={ne} top_k={top_k}: device err {err:.3e} numpy-fp32 err {np_err:.3e} bound {bound:.3e} "
          f"sum err {sum_err:.3e}")
    assert err <= bound, (err, bound)
    assert sum_err <= bound, (sum_err, bound)


def test_route_tie_goes_to_the_lower_index():
    x = np.array([[0.5, 3.0, -1.0, 3.0, 2.0, 0.0, 1.0, -2.0]], np.float32)
    ids, wts = bestla.moe_route(torch.from_numpy(x).cuda(), 2)
    assert ids.cpu().numpy().tolist() == [[1, 3]]
    assert wts.cpu().numpy().tolist() == [[0.5, 0.5]]
