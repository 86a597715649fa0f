"""General expert banks on the GPU (ExpertBank(..., general=True)): int4 groups of 32, int8 and GGUF Q4_0 / Q5_0 / Q8_0
experts routed through woq_gemv_routed_kernel, and through the grouped gemm7 at prefill sizes.

Bars:
  * a routed row against its expert's own M = 1 forward: BIT-identical (compared as uint32) -- the routed stripe stream
    runs the expert's own waves, K-slices, hi / lo fp16 rows and cross-wave reduce;
  * mul_mat_id against the oracle: TOL_DECODE = 2e-5 of max|ref| (tests/test_moe_gpu.py); a GGUF bank against the fp64
    product with the dequantized blocks at the bar tests/test_gguf_types_gpu.py holds that weight's M = 1 forward to;
  * moe_ffn's combine against numpy float32 on the device's own slot results: no tolerance; the chain against float64:
    2 * TOL["fp32"];
  * a grouped row against the exact fp16 fold model: 2e-5 of max|ref|; against the expert's own gemm7 forward of the
    fp16 rows: bit-identical at every tile height; the grouped FFN against the float64 chain: TOL["fp32"] = 1e-3.
Every case prints one line starting "moe_general" with its worst error; profiles/moe_general_errors.txt keeps them.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from neural_amd import bestla  # noqa: E402
from tests import edges  # noqa: E402
from tests import fold_model as fm  # noqa: E402
from tests import gguf_blocks as gb  # noqa: E402
from tests.oracle_lib import BF16, F16, F32, S4, S8  # noqa: E402
from tests.test_gemm2_gpu import TOL  # noqa: E402
from tests.test_gguf_types_gpu import _tol as gguf_tol  # noqa: E402
from tests.test_gpu_parity import _blob, _rel_err  # noqa: E402
from tests.test_moe_cpu import combine_f32  # noqa: E402
from tests.test_moe_grouped_cpu import combine_sorted_f32, sort_ref  # noqa: E402

TOL_DECODE = 2e-5
NE = 4
FIN, FMID, FOUT = 1024, 512, 300

# blob formats: (group size (None: per channel), quant type, scale type, asym)
BLOBS = {
    "int4_g32_f32_sym": (32, S4, F32, False),
    "int4_g32_f16_sym": (32, S4, F16, False),
    "int8_g32_f16_sym": (32, S8, F16, False),
    "int8_g128_bf16_asym": (128, S8, BF16, True),
    "int8_perchannel_f32_sym": (None, S8, F32, False),
    "int4_g128_f16_sym": (128, S4, F16, False),  # the M = 1 stream's: the down bank of the mixed FFN
}
GGUF = {"q4_0": gb.Q4_0, "q5_0": gb.Q5_0, "q8_0": gb.Q8_0}
GENERAL = [f for f in BLOBS if f != "int4_g128_f16_sym"] + list(GGUF)
INT4 = ("int4_g32_f32_sym", "int4_g32_f16_sym", "q4_0")


def _q4_0(w):
    """quantize_row_q4_0_reference's blocks of an fp32 [n][k] matrix and their dequantization [n][k]"""
    n, k = w.shape
    x = w.reshape(n, k // 32, 32)
    i = np.abs(x).argmax(axis=2)
    mx = np.take_along_axis(x, i[:, :, None], axis=2)[:, :, 0]
    d = (mx / np.float32(-8)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    q = np.minimum(15, np.trunc(x * idv[:, :, None] + np.float32(8.5)).astype(np.int32)).astype(np.uint8)
    d16 = d.astype(np.float16)
    blocks = np.concatenate([d16.view(np.uint8).reshape(n, k // 32, 2), q[:, :, :16] | (q[:, :, 16:] << 4)], axis=2)
    deq = (q.astype(np.float32) - 8) * d16.astype(np.float32)[:, :, None]
    return blocks.ravel(), deq.reshape(n, k)


class Experts:
    """NE experts of one shape and format: the DeviceWeights, their bank, and a reference product per expert"""

    def __init__(self, oracle, n, k, fmt, tag):
        key = zlib.crc32(repr((n, k, fmt, tag)).encode()) % 10000
        self.n, self.k, self.fmt = n, k, fmt
        if fmt in GGUF:
            self.ws, self.deq = [], []
            for e in range(NE):
                w = np.random.default_rng(key + 31 * e).uniform(-1, 1, size=(n, k)).astype(np.float32)
                if fmt == "q4_0":
                    blocks, deq = _q4_0(w)
                    self.ws.append(bestla.DeviceWeight.from_gguf(bestla.GGUF_Q4_0, blocks, n, k))
                else:
                    blocks = gb.quantize(GGUF[fmt], w)
                    deq = gb.dequant(GGUF[fmt], blocks, n, k)
                    self.ws.append(bestla.DeviceWeight.from_gguf(GGUF[fmt], blocks, n, k))
                self.deq.append(deq.astype(np.float64))
            self.ref = lambda A, e: np.asarray(A, np.float64) @ self.deq[e].T
            self.tol = gguf_tol(1, "fp32", self.ws[0])
        else:
            bs, qt, st, asym = BLOBS[fmt]
            self.blobs = [_blob(oracle, n, k, bs or k, qt, st, asym, 4, seed=key + 31 * e) for e in range(NE)]
            self.ws = [bestla.DeviceWeight(b) for b in self.blobs]
            self.ref = lambda A, e: oracle.forward(A, self.blobs[e], n, k)
            self.tol = TOL_DECODE
        self.bank = bestla.ExpertBank(self.ws, general=True)


_CACHE = {}


def _experts(oracle, n, k, fmt, tag):
    key = (n, k, fmt, tag)
    if key not in _CACHE:
        _CACHE[key] = Experts(oracle, n, k, fmt, tag)
    return _CACHE[key]


def _ids(m, width, rng):
    """ids [m][width] over experts 0, 1, 2, every row's entries distinct, experts repeated across rows"""
    ids = np.stack([rng.permutation(3)[:width] for _ in range(m)])
    if m > 1:
        ids[1] = ids[0]
    return ids.astype(np.int32)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ mul_mat_id
# (1, 72, 768): a half-filled last stripe, a short second K-slice for int4; (5, 300, 992): K ends inside a tile; 33 K
# tiles (4224 int4, 2112 int8): nine slices on eight waves, one wave owns two and the last slice is one tile;
# (200, 64, 256): more problems than CUs, one workgroup per problem
def _shapes(fmt):
    return [(1, 72, 768), (5, 300, 992), (3, 48, 4224 if fmt in INT4 else 2112), (200, 64, 256)]


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("fmt", GENERAL)
def test_mul_mat_id_rows_are_their_experts_forwards(oracle, fmt, shape):
    m, n, k = _shapes(fmt)[shape]
    ex = _experts(oracle, n, k, fmt, "mmid")
    assert ex.bank.route == 1 and ex.bank.has_weights == 1
    with pytest.raises(RuntimeError):  # the M = 1 stream's entry still refuses these weights
        bestla.ExpertBank(ex.ws)
    plan = ex.ws[0].plan(1, "fp32")
    assert plan["kernel"] == "woq_gemv_kernel", plan  # the expert's own forward is the stripe stream
    rng = np.random.default_rng(m * 13 + n)
    A = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    ids = _ids(m, 3, rng)  # ids_ld = 3 > the two slots used
    ids_t = torch.from_numpy(ids).cuda()
    refs = {e: ex.ref(A, e) for e in range(3)}
    singles, worst = {}, 0.0
    for slot in (0, 1):
        out = torch.full((m, n), float("nan"), device="cuda")
        got = bestla.mul_mat_id(ex.bank, x, ids_t, slot, out=out).cpu().numpy()
        assert not np.isnan(got).any()
        for r in range(m):
            e = int(ids[r, slot])
            if (r, e) not in singles:
                singles[(r, e)] = ex.ws[e].forward(x[r:r + 1]).cpu().numpy()[0]
            assert np.array_equal(_u32(got[r]), _u32(singles[(r, e)])), (slot, r, e)
            worst = max(worst, _rel_err(got[r], refs[e][r]))
    print(f"moe_general mul_mat_id {fmt} m={m} n={n} k={k}: bit-identical to forward; worst row vs reference "
          f"{worst:.3e} (bar {ex.tol:.1e})")
    assert worst <= ex.tol, worst


@pytest.mark.parametrize("align", edges.ALIGNS)
@pytest.mark.parametrize("fmt", ["int4_g32_f16_sym", "int8_g128_bf16_asym", "q8_0"])
def test_mul_mat_id_window(oracle, fmt, align):
    m, n, k = 5, 300, 992
    ex = _experts(oracle, n, k, fmt, "mmid")
    rng = np.random.default_rng(9)
    xt = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)).cuda()
    if align == "odd":  # rows stay 16-B aligned (the entry's contract): a view at column 8 of a wider NaN storage
        store = torch.full((m, k + 24), float("nan"), device="cuda")
        x = store[:, 8:8 + k]
        x.copy_(xt)
    else:
        x = edges.act_window(xt, "aligned")
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
    ids = torch.from_numpy(_ids(m, 2, rng)).cuda()
    can, out = edges.out_window(m, n, align)
    (y,) = edges.twice(can, lambda: bestla.mul_mat_id(ex.bank, x, ids, 1, out=out), f"general mul_mat_id {fmt} {align}")
    for r in range(m):
        e = int(ids[r, 1])
        assert np.array_equal(_u32(y[r]), _u32(ex.ws[e].forward(xt[r:r + 1]).cpu().numpy()[0]))


@pytest.mark.parametrize("bad", [-1, NE, 1 << 30])
@pytest.mark.parametrize("fmt", ["int4_g32_f32_sym", "int8_g32_f16_sym", "int8_g128_bf16_asym", "q5_0"])
def test_out_of_range_id_is_a_row_of_plus_zero(oracle, fmt, bad):
    m, n, k = 5, 300, 992
    ex = _experts(oracle, n, k, fmt, "mmid")
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)).cuda()
    good = _ids(m, 2, rng)
    ids = good.copy()
    ids[1, 0] = bad
    ids[4, 0] = bad
    base = bestla.mul_mat_id(ex.bank, x, torch.from_numpy(good).cuda(), 0).cpu().numpy()
    out = torch.full((m, n), float("nan"), device="cuda")
    got = bestla.mul_mat_id(ex.bank, x, torch.from_numpy(ids).cuda(), 0, out=out).cpu().numpy()
    assert (_u32(got[[1, 4]]) == 0).all()  # +0.0, not -0.0
    assert np.array_equal(_u32(got[[0, 2, 3]]), _u32(base[[0, 2, 3]]))


# ------------------------------------------------------------------------------------------------ moe_ffn
POLICIES = {
    "int4_g32_f16": ("int4_g32_f16_sym", "int4_g32_f16_sym"),
    "int8_g32_f16": ("int8_g32_f16_sym", "int8_g32_f16_sym"),
    "int8_g128_bf16_asym": ("int8_g128_bf16_asym", "int8_g128_bf16_asym"),
    "q4_0_gate_up_int4_g128_down": ("q4_0", "int4_g128_f16_sym"),
    "int4_g128_gate_up_q8_0_down": ("int4_g128_f16_sym", "q8_0"),
}


def _ffn_banks(oracle, policy):
    gu, dn = POLICIES[policy]
    return (_experts(oracle, FMID, FIN, gu, "gate"), _experts(oracle, FMID, FIN, gu, "up"),
            _experts(oracle, FOUT, FMID, dn, "down"))


def _act64(v, act):
    return edges.silu64(v) if act == "silu" else edges.gelu64(v)


def _chain64(A, ids, wts, banks, act):
    g, u, d = banks
    m, top_k = ids.shape
    out = np.zeros((m, FOUT), np.float64)
    for r in range(m):
        for i in range(top_k):
            e = int(ids[r, i])
            if not 0 <= e < NE:
                continue
            h1 = np.asarray(g.ref(A[r:r + 1], e), np.float64)
            h3 = np.asarray(u.ref(A[r:r + 1], e), np.float64)
            t = (_act64(h1, act) * h3).astype(np.float32)
            out[r] += float(wts[r, i]) * np.asarray(d.ref(t, e), np.float64)[0]
    return out


@pytest.mark.parametrize("m,top_k,act", [(1, 2, "silu"), (5, 2, "silu"), (2, 1, "gelu")])
@pytest.mark.parametrize("policy", list(POLICIES))
def test_moe_ffn(oracle, policy, m, top_k, act):
    banks = _ffn_banks(oracle, policy)
    g, u, d = banks
    kinds = (g.bank.route, d.bank.route)
    assert kinds == {"q4_0_gate_up_int4_g128_down": (1, 0), "int4_g128_gate_up_q8_0_down": (0, 1)}.get(policy, (1, 1))
    plan = bestla.plan_moe(g.bank, u.bank, d.bank, m, top_k)
    names = {0: "woq_gemv_m1_routed_kernel", 1: "woq_gemv_routed_kernel"}
    assert [p["kernel"] for p in plan[:2]] == [names[kinds[0]], names[kinds[1]]]
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
    got = bestla.moe_ffn(g.bank, u.bank, d.bank, x, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda(), act=act,
                         out=out).cpu().numpy()
    t, y = t_ws.clone(), y_ws.clone()
    for r in range(m):  # the workspace rows are the one-problem calls, bit for bit
        for i in range(top_k):
            p, e = r * top_k + i, int(ids[r, i])
            t1 = bestla.ffn_gate_up(x[r:r + 1], g.ws[e], u.ws[e], act=act)
            assert np.array_equal(_u32(t[p:p + 1].cpu().numpy()), _u32(t1.cpu().numpy())), (p, e)
            y1 = d.ws[e].forward(t[p:p + 1])
            assert np.array_equal(_u32(y[p:p + 1].cpu().numpy()), _u32(y1.cpu().numpy())), (p, e)
    assert np.array_equal(_u32(got), _u32(combine_f32(y.cpu().numpy(), w, top_k)))
    err = _rel_err(got, _chain64(A, ids, w, banks, act))
    print(f"moe_general moe_ffn {policy} {act} m={m} top_k={top_k}: workspace rows bit-identical; chain err {err:.3e} "
          f"(bar {2 * TOL['fp32']:.1e})")
    assert err <= 2 * TOL["fp32"], err


def test_moe_ffn_out_of_range_slot(oracle):
    g, u, d = _ffn_banks(oracle, "q4_0_gate_up_int4_g128_down")
    m = 3
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    good = np.array([[0, 1], [2, 0], [1, 2]], np.int32)
    ids = good.copy()
    ids[1, 0] = NE
    w = rng.uniform(0.1, 1.0, size=(m, 2)).astype(np.float32)
    _, t_ws, y_ws = bestla.moe_workspace(m, 2, FMID, FOUT, x.device)
    bestla.moe_ffn(g.bank, u.bank, d.bank, x, torch.from_numpy(good).cuda(), torch.from_numpy(w).cuda())
    y = y_ws.cpu().numpy().copy()
    y[2] = 0  # problem p = 1 * top_k + 0
    got = bestla.moe_ffn(g.bank, u.bank, d.bank, x, torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda())
    assert (_u32(t_ws[2].cpu().numpy()) == 0).all()
    assert np.array_equal(_u32(y_ws.cpu().numpy()), _u32(y))
    assert np.array_equal(_u32(got.cpu().numpy()), _u32(combine_f32(y, w, 2)))


def test_routing_and_weights_are_read_at_replay(oracle):
    """moe_ffn on a mixed pair of banks captured once; ids and wts overwritten on the device between replays, then an
    expert's weight bytes: every replay is the eager result for what it found, bit for bit."""
    g, u, d = _ffn_banks(oracle, "q4_0_gate_up_int4_g128_down")
    m, top_k = 2, 2
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    choices = [(np.array([[0, 1], [2, 0]], np.int32), np.array([[0.7, 0.3], [0.4, 0.6]], np.float32)),
               (np.array([[3, 2], [1, 3]], np.int32), np.array([[0.2, 0.8], [0.9, 0.1]], np.float32))]

    def eager(which):
        return bestla.moe_ffn(g.bank, u.bank, d.bank, x, torch.from_numpy(choices[which][0]).cuda(),
                              torch.from_numpy(choices[which][1]).cuda()).cpu().numpy()

    want = [eager(0), eager(1)]
    assert not np.array_equal(want[0], want[1])
    ids = torch.from_numpy(choices[0][0]).cuda()
    w = torch.from_numpy(choices[0][1]).cuda()
    out = torch.empty((m, FOUT), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bestla.moe_ffn(g.bank, u.bank, d.bank, x, ids, w, out=out, stream=s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            bestla.moe_ffn(g.bank, u.bank, d.bank, x, ids, w, out=out, stream=s)
    torch.cuda.current_stream().wait_stream(s)

    def replay(which):
        ids.copy_(torch.from_numpy(choices[which][0]))
        w.copy_(torch.from_numpy(choices[which][1]))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        return out.cpu().numpy()

    for which in (0, 1, 0):
        assert np.array_equal(_u32(replay(which)), _u32(want[which])), which
    # gate expert 0's weight becomes gate expert 1's, in place: the bank's table points at the same memory
    w0, w1 = g.ws[0], g.ws[1]
    assert w0.mem.numel() == w1.mem.numel()
    keep = w0.mem.clone()
    w0.mem.copy_(w1.mem)
    torch.cuda.synchronize()
    changed = eager(0)
    assert not np.array_equal(changed, want[0])
    assert np.array_equal(_u32(replay(0)), _u32(changed))
    w0.mem.copy_(keep)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(replay(0)), _u32(want[0]))


# ------------------------------------------------------------------------------------------------ grouped
GROUPED = {
    "int4_g32_f16_sym": (32, S4, F16, False),
    "int8_g32_f16_sym": (32, S8, F16, False),
    "int8_g128_bf16_asym": (128, S8, BF16, True),
}
HEIGHTS = (None, 32, 64)
M = 70
_GCACHE = {}


def _gexperts(oracle, n, k, fmt, tag):
    """-> (blobs, fold-model fp16 weights [k][n], DeviceWeights, general ExpertBank), fields over their whole ranges"""
    key = (n, k, fmt, tag)
    if key not in _GCACHE:
        bs, qt, st, asym = GROUPED[fmt]
        made = [fm.make(oracle, n, k, bs, qt, st, asym, zlib.crc32(repr(key).encode()) % 10000 + 31 * e)
                for e in range(NE)]
        ws = [bestla.DeviceWeight(b) for b, _ in made]
        assert all(w.fold_ok == 1 for w in ws)
        _GCACHE[key] = ([b for b, _ in made], [fm.folded_weights(Q, S, Z, bs) for _, (Q, S, Z) in made], ws,
                        bestla.ExpertBank(ws, general=True))
    return _GCACHE[key]


def _row_err(y_row, ref, r):
    return float(np.abs(y_row.astype(np.float64) - ref[r]).max() / np.abs(ref).max())


@pytest.mark.parametrize("m", [M, 9])
@pytest.mark.parametrize("fmt", list(GROUPED))
def test_mul_mat_id_grouped(oracle, knob, fmt, m):
    n, k = FOUT, FIN
    blobs, w16, ws, bank = _gexperts(oracle, n, k, fmt, "mmid")
    assert bank.route == 1
    A = np.random.default_rng(7).uniform(-0.5, 0.5, size=(m, k)).astype(np.float16).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    ids = np.random.default_rng(3).permutation(np.resize(np.array([0, 0, 0, 1, 1, 3], np.int32), m))  # expert 2 empty
    ids[1], ids[m - 2] = -1, NE
    ids_t = torch.from_numpy(ids[:, None].copy()).cuda()
    model = [fm.model_product(A, w16[e]) for e in range(NE)]
    outs = []
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        can, out = edges.out_window(m, n, "aligned")
        (y,) = edges.twice(can, lambda: bestla.mul_mat_id_grouped(bank, x, ids_t, 0, out=out),
                           f"general mul_mat_id_grouped {fmt} bm={bm}")
        outs.append(y)
    y = outs[0]
    for h, other in zip(HEIGHTS[1:], outs[1:]):
        assert np.array_equal(_u32(y), _u32(other)), f"tile height {h} changes the bits"
    worst = 0.0
    for r in range(m):
        e = int(ids[r])
        if not 0 <= e < NE:
            assert (_u32(y[r]) == 0).all(), r
            continue
        worst = max(worst, _row_err(y[r], model[e], r))
    print(f"moe_general mul_mat_id_grouped {fmt} m={m}: worst row vs fold model {worst:.3e} (bar {TOL['fp16']:.1e})")
    assert worst <= TOL["fp16"], worst
    # each expert's own forward of the same rows as fp16, on gemm7 over the whole K, at each tile height
    knob("NAD_MID_MAX_M", 0)
    knob("NAD_SPLITK_DISABLE", 1)
    x16 = x.half()
    if m > 16:  # below 17 rows an expert's own forward is the decode GEMV, not gemm7
        for bm in HEIGHTS:
            knob("NAD_GEMM7_BM", bm)
            for e in (0, 1, 3):
                plan = ws[e].plan(m, "fp16")
                assert plan["kernel"] == "woq_gemm7_kernel" and plan["ksplit"] == 1, plan
                own = ws[e].forward(x16).cpu().numpy()
                rows = np.nonzero(ids == e)[0]
                assert np.array_equal(_u32(y[rows]), _u32(own[rows])), (bm, e)


def _gchain64(oracle, A, ids, wts, banks, act="silu"):
    (gb_, _, _, _), (ub, _, _, _), (db, _, _, _) = banks
    m, top_k = ids.shape
    out = np.zeros((m, FOUT), np.float64)
    for e in range(NE):
        rows, slots = np.nonzero(ids == e)
        if len(rows) == 0:
            continue
        h1 = oracle.forward(A[rows], gb_[e], FMID, FIN).astype(np.float64)
        h3 = oracle.forward(A[rows], ub[e], FMID, FIN).astype(np.float64)
        t = (_act64(h1, act) * h3).astype(np.float32)
        np.add.at(out, rows, wts[rows, slots].astype(np.float64)[:, None] *
                  oracle.forward(t, db[e], FOUT, FMID).astype(np.float64))
    return out


@pytest.mark.parametrize("m", [M, 9])
@pytest.mark.parametrize("fmt", list(GROUPED))
def test_moe_ffn_grouped(oracle, knob, fmt, m):
    top_k = 2
    banks = (_gexperts(oracle, FMID, FIN, fmt, "gate"), _gexperts(oracle, FMID, FIN, fmt, "up"),
             _gexperts(oracle, FOUT, FMID, fmt, "down"))
    gate, up, down = (b[3] for b in banks)
    A = np.random.default_rng(100 + m).uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    rng = np.random.default_rng(17 + m)
    ids = np.stack([rng.choice(NE, size=top_k, replace=False, p=[0.4, 0.35, 0.2, 0.05]) for _ in range(m)])
    ids = ids.astype(np.int32)
    ids[5, 1] = NE
    w = rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    ids_t, w_t = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()
    ws = bestla.moe_grouped_workspace_alloc(gate, up, down, m, top_k)
    res = []
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        ws.fill_(0xFF)
        out = torch.full((m, FOUT), float("nan"), device="cuda")
        got = bestla.moe_ffn_grouped(gate, up, down, x, ids_t, w_t, out=out, workspace=ws).cpu().numpy()
        v = bestla.moe_grouped_workspace_rows(ws, gate, up, down, m, top_k)
        inv, y = v["inv"].cpu().numpy(), v["y"].cpu().numpy()
        assert np.array_equal(inv, sort_ref(ids, NE)[2])
        nv = int(v["offs"][NE])
        assert nv == m * top_k - 1 and not np.isnan(y[:nv]).any()
        assert np.array_equal(_u32(got), _u32(combine_sorted_f32(y[:nv], inv, w, top_k)))
        res.append(got)
    for h, other in zip(HEIGHTS[1:], res[1:]):
        assert np.array_equal(_u32(res[0]), _u32(other)), f"tile height {h} changes the bits"
    err = _rel_err(res[0], _gchain64(oracle, A, ids, w, banks))
    print(f"moe_general moe_ffn_grouped {fmt} m={m} top_k={top_k}: err {err:.3e} (bar {TOL['fp32']:.1e})")
    assert err <= TOL["fp32"], err


def test_a_bank_whose_scales_do_not_fold_is_refused_grouped_and_runs_row_routed(oracle):
    """weights near 1e6: q * s leaves the fp16 range, so gemm7 cannot fold the scale (fold_ok 0)"""
    n, k, m = 64, 256, 5
    core = oracle.lib.orc_select_core(4, S4, 32, 0, 0)
    ws = []
    for e in range(NE):
        W = (np.random.default_rng(50 + e).uniform(-0.5, 0.5, size=(n, k)) * 2e6).astype(np.float32)
        ws.append(bestla.DeviceWeight(oracle.quant_pack(W, n, k, 32, S4, F32, False, core, is_trans=True)))
    assert all(w.fold_ok == 0 for w in ws)
    bank = bestla.ExpertBank(ws, general=True)
    assert bank.route == 1
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)).cuda()
    ids = torch.from_numpy(_ids(m, 1, rng)).cuda()
    with pytest.raises(RuntimeError, match=r"the given bank \(int4, groups of 32\) does not take the grouped gemm7"):
        bestla.mul_mat_id_grouped(bank, x, ids, 0, workspace=torch.empty(1 << 16, dtype=torch.uint8, device="cuda"))
    got = bestla.mul_mat_id(bank, x, ids, 0).cpu().numpy()
    for r in range(m):
        own = ws[int(ids[r, 0])].forward(x[r:r + 1]).cpu().numpy()[0]
        assert np.array_equal(_u32(got[r]), _u32(own)), r
