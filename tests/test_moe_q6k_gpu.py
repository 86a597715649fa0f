"""Banks of GGUF Q6_K experts on the GPU (ExpertBank(..., general=True), route kind 2): row-routed through
woq_q6k_gemv_routed_kernel, sorted and grouped through woq_q6k_gemm_grouped_kernel.

Bars:
  * a routed row against its expert's own M = 1 forward: BIT-identical (compared as uint32) -- the routed kernel is the
    dense GEMV's body, and a stripe's bits do not depend on how the stripes are dealt over workgroups;
  * a routed row against the float64 product with the dequantized blocks: TOL_DECODE = 2e-5 of the row's max|ref| (the
    bar tests/test_q6_k_gpu.py holds the dense GEMV to);
  * moe_ffn's workspace rows against ffn_gate_up / forward of the expert: bit-identical; the combine against numpy
    float32: no tolerance; the chain against float64: 1e-3;
  * a grouped row against the same row in another batch, and against the expert's dense forward of the fp16 rows at
    M >= 17: bit-identical; against the float64 product: FOLD_TOL (tests/test_gemm2_gpu.py), the dense Q6_K GEMM's bar;
    the grouped FFN against the float64 chain: 1e-3, its last launch against numpy float32: no tolerance.
Every case prints one line starting "moe_q6k" with its worst error; profiles/moe_q6k_errors.txt keeps them.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from neural_amd import bestla  # noqa: E402
from tests import edges  # noqa: E402
from tests import q6k_blocks as qb  # noqa: E402
from tests.test_gemm2_gpu import FOLD_TOL  # noqa: E402
from tests.test_gpu_parity import _rel_err  # noqa: E402
from tests.test_moe_cpu import combine_f32  # noqa: E402
from tests.test_moe_grouped_cpu import combine_sorted_f32, sort_ref  # noqa: E402

TOL_DECODE = 2e-5
TOL_CHAIN = 1e-3
NE = 4
FIN, FMID, FOUT = 512, 768, 72


class Q6kExperts:
    """NE Q6_K experts of one shape: blocks, float64 dequantized weights, DeviceWeights and their bank"""

    def __init__(self, n, k, tag):
        seed = sum(map(ord, tag)) * 100
        self.n, self.k = n, k
        self.blocks = [qb.random_blocks(n, k, seed=seed + e) for e in range(NE)]
        self.deq = [qb.dequant(b, n, k).astype(np.float64) for b in self.blocks]
        self.ws = [bestla.DeviceWeight.from_q6_k(b, n, k) for b in self.blocks]
        self.bank = bestla.ExpertBank(self.ws, general=True)

    def ref(self, A, e):
        return np.asarray(A, np.float64) @ self.deq[e].T


_CACHE = {}


def _experts(n, k, tag):
    key = (n, k, tag)
    if key not in _CACHE:
        _CACHE[key] = Q6kExperts(n, k, tag)
    return _CACHE[key]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_bank_of_loaded_weights_and_its_refusals():
    ex = _experts(40, 256, "mmid")
    assert (ex.bank.route, ex.bank.bits, ex.bank.blocksize, ex.bank.has_weights) == (2, 6, 16, 1)
    with pytest.raises(RuntimeError, match="expert 0's weight is GGUF Q6_K"):
        bestla.ExpertBank(ex.ws)
    w = bestla.DeviceWeight.from_q6_k(ex.blocks[1], 40, 256)
    w.set_compute(bestla.COMPUTE_Q8_K)
    with pytest.raises(RuntimeError, match=r"expert 1's weight is set to integer \(int8 / Q8_K\) arithmetic"):
        bestla.ExpertBank([ex.ws[0], w, ex.ws[2]], general=True)
    w.set_compute(None)
    assert bestla.ExpertBank([ex.ws[0], w, ex.ws[2]], general=True).route == 2


def test_the_refusals_that_stay_under_general(oracle):
    """block mins, NFloat codes and act-order are no banks under NAD_BANK_GENERAL either, alone or beside Q6_K experts
    (a geometry-only bank cannot express the three, so they are loaded weights here)"""
    from tests import gguf_blocks as gb
    from tests.oracle_lib import F32, F4_NF4, S4
    from tests.test_gpu_parity import _blob
    n, k = 40, 256
    ex = _experts(n, k, "mmid")
    w = np.random.default_rng(3).uniform(-1, 1, size=(n, k)).astype(np.float32)
    q4_1 = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q4_1, gb.quantize(gb.Q4_1, w), n, k)
    q8_0 = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q8_0, gb.quantize(gb.Q8_0, w), n, k)
    nf4 = bestla.DeviceWeight(_blob(oracle, n, k, 32, F4_NF4, F32, False, 1, seed=4))
    desc_act = bestla.DeviceWeight(_blob(oracle, n, k, 128, S4, F32, True, 4, seed=5, gidx=True))
    for bad, msg in ((q4_1, r"expert 0's weight carries block mins \(GGUF Q4_1 / Q5_1\), which are not routed"),
                     (nf4, r"expert 0's weight is not in the int4 / int2 / int8 tile layout \(bits 4, NFloat codes\)"),
                     (desc_act, r"expert 0's weight is act-order \(desc_act\), which is not routed")):
        with pytest.raises(RuntimeError, match=msg):
            bestla.ExpertBank([bad], general=True)
    # beside Q6_K experts: expert 0 decides the bank's format
    for bad in (q4_1, desc_act):
        with pytest.raises(RuntimeError, match="expert 2's weight differs in shape or format from expert 0's"):
            bestla.ExpertBank([ex.ws[0], ex.ws[1], bad, ex.ws[3]], general=True)
    with pytest.raises(RuntimeError, match=r"expert 1's weight is not in the int4 / int2 / int8 tile layout \(bits 4, "
                                           r"NFloat codes\)"):
        bestla.ExpertBank([ex.ws[0], nf4], general=True)
    # ... and a Q6_K expert beside another format keeps its message, without the hint that the flag would help
    with pytest.raises(RuntimeError, match="expert 1's weight is GGUF Q6_K, which the routed GEMV does not stream "
                                           "beside other formats"):
        bestla.ExpertBank([q8_0, ex.ws[0]], general=True)


# ------------------------------------------------------------------------------------------------ mul_mat_id
# (40, 256): one superblock, 15 waves idle, a half-filled last stripe; (16, 768): one stripe; (200, 4352): 17
# superblocks (wave 0 takes two), 13 stripes of which the last is half filled -- 13 workgroups per problem at m = 1 and
# 5, uneven shares (6: three stripes for the first, two for the rest) at 40, and one workgroup walking all 13 stripes
# through both partial-sum sets at 300
SHAPES = [(40, 256), (16, 768), (200, 4352)]


def _route_ids(m, rng):
    """ids [m][NE]: column c of row r is (r + c) % NE at the top, so that every expert is hit even at m = 1 (over the
    slots); random below, the last row repeating row 0's"""
    ids = (np.arange(m)[:, None] + np.arange(NE)[None, :]) % NE
    if m > NE:
        ids[NE:] = rng.integers(0, NE, size=(m - NE, NE))
        ids[m - 1] = ids[0]
    return ids.astype(np.int32)


@pytest.mark.parametrize("m", [1, 5, 40, 300])
@pytest.mark.parametrize("shape", SHAPES)
def test_mul_mat_id_rows_are_their_experts_forwards(shape, m):
    n, k = shape
    ex = _experts(n, k, "mmid")
    plan = ex.ws[0].plan(1, "fp32")
    assert plan["kernel"] == "woq_q6k_gemv_kernel", plan
    rng = np.random.default_rng(m * 13 + n)
    A = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    x = _cuda(A)
    ids = _route_ids(m, rng)
    ids_t = _cuda(ids)
    refs = [ex.ref(A, e) for e in range(NE)]
    worst = 0.0
    for slot in (range(NE) if m < NE else (1,)):
        out = torch.full((m, n), float("nan"), device="cuda")
        got_t = bestla.mul_mat_id(ex.bank, x, ids_t, slot, out=out)
        own = torch.cat([ex.ws[int(ids[r, slot])].forward(x[r:r + 1]) for r in range(m)])
        got = got_t.cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(_u32(got), _u32(own.cpu().numpy())), (slot, np.nonzero((got != own.cpu().numpy()).any(1)))
        for r in range(m):
            worst = max(worst, _rel_err(got[r], refs[int(ids[r, slot])][r]))
    assert m < NE or set(ids[:, 1]) == set(range(NE))
    print(f"moe_q6k mul_mat_id n={n} k={k} m={m}: bit-identical to forward; worst row vs float64 {worst:.3e} "
          f"(bar {TOL_DECODE:.1e})")
    assert worst <= TOL_DECODE, worst


@pytest.mark.parametrize("bad", [-1, NE, 1 << 30])
def test_out_of_range_id_is_a_row_of_plus_zero(bad):
    m, n, k = 5, 200, 4352
    ex = _experts(n, k, "mmid")
    rng = np.random.default_rng(77)
    A = rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    good = _route_ids(m, rng)
    ids = good.copy()
    ids[1, 0] = bad
    ids[4, 0] = bad
    base = bestla.mul_mat_id(ex.bank, _cuda(A), _cuda(good), 0).cpu().numpy()
    A[4, 100] = np.inf  # no weight and no activation of an invalid row is read
    out = torch.full((m, n), float("nan"), device="cuda")
    got = bestla.mul_mat_id(ex.bank, _cuda(A), _cuda(ids), 0, out=out).cpu().numpy()
    assert (_u32(got[[1, 4]]) == 0).all()  # +0.0, not -0.0
    assert np.array_equal(_u32(got[[0, 2, 3]]), _u32(base[[0, 2, 3]]))


@pytest.mark.parametrize("align", edges.ALIGNS)
def test_mul_mat_id_window(align):
    m, n, k = 5, 40, 256
    ex = _experts(n, k, "mmid")
    rng = np.random.default_rng(9)
    xt = _cuda(rng.uniform(-0.5, 0.5, size=(m, k)).astype(np.float32))
    if align == "odd":  # rows stay 16-B aligned (the entry's contract): a view at column 8 of a wider NaN storage
        store = torch.full((m, k + 24), float("nan"), device="cuda")
        x = store[:, 8:8 + k]
        x.copy_(xt)
    else:
        x = edges.act_window(xt, "aligned")
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
    ids = _route_ids(m, rng)
    ids[3, 1] = NE  # a zero row is written inside the window too
    ids_t = _cuda(ids)
    can, out = edges.out_window(m, n, align)
    (y,) = edges.twice(can, lambda: bestla.mul_mat_id(ex.bank, x, ids_t, 1, out=out), f"q6k mul_mat_id {align}")
    for r in range(m):
        e = int(ids[r, 1])
        want = ex.ws[e].forward(xt[r:r + 1]).cpu().numpy()[0] if e < NE else np.zeros(n, np.float32)
        assert np.array_equal(_u32(y[r]), _u32(want)), r


# ------------------------------------------------------------------------------------------------ moe_ffn
POLICIES = ("q6k", "q6k_gate_up_q8_0_down", "int4_g128_gate_up_q6k_down")


def _ffn_banks(oracle, policy):
    from tests.test_moe_general_gpu import Experts
    if policy == "int4_g128_gate_up_q6k_down":
        g, u = (Experts(oracle, FMID, FIN, "int4_g128_f16_sym", "q6k_" + t) for t in ("gate", "up"))
    else:
        g, u = _experts(FMID, FIN, "gate"), _experts(FMID, FIN, "up")
    d = Experts(oracle, FOUT, FMID, "q8_0", "q6k_down") if policy == "q6k_gate_up_q8_0_down" \
        else _experts(FOUT, FMID, "down")
    return g, u, d


_FFN = {}


def _banks(oracle, policy):
    if policy not in _FFN:
        _FFN[policy] = _ffn_banks(oracle, policy)
    return _FFN[policy]


def _act64(v, act):
    return edges.silu64(v) if act == "silu" else edges.gelu64(v)


def _chain64(A, ids, wts, banks, act):
    g, u, d = banks
    m, top_k = ids.shape
    out = np.zeros((m, FOUT), np.float64)
    for e in range(NE):
        rows, slots = np.nonzero(ids == e)
        if len(rows) == 0:
            continue
        h1 = np.asarray(g.ref(A[rows], e), np.float64)
        h3 = np.asarray(u.ref(A[rows], e), np.float64)
        t = (_act64(h1, act) * h3).astype(np.float32)
        np.add.at(out, rows, wts[rows, slots].astype(np.float64)[:, None] * np.asarray(d.ref(t, e), np.float64))
    return out


def _ffn_inputs(m, top_k, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)
    ids = np.stack([rng.permutation(NE)[:top_k] for _ in range(m)]).astype(np.int32)
    w = rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    return A, ids, w


@pytest.mark.parametrize("m,top_k,act", [(1, 2, "silu"), (5, 2, "silu"), (2, 1, "gelu")])
@pytest.mark.parametrize("policy", POLICIES)
def test_moe_ffn(oracle, policy, m, top_k, act):
    banks = _banks(oracle, policy)
    g, u, d = banks
    kinds = (g.bank.route, d.bank.route)
    assert kinds == {"q6k": (2, 2), "q6k_gate_up_q8_0_down": (2, 1), "int4_g128_gate_up_q6k_down": (0, 2)}[policy]
    plan = bestla.plan_moe(g.bank, u.bank, d.bank, m, top_k)
    names = {0: ["woq_gemv_m1_routed_kernel"], 1: ["woq_gemv_routed_kernel"], 2: ["woq_q6k_gemv_routed_kernel"]}
    assert [p["kernel"] for p in plan] == names[kinds[0]] * (2 if kinds[0] == 2 else 1) + names[kinds[1]] + \
        ["moe_combine_kernel"]
    A, ids, w = _ffn_inputs(m, top_k, 100 * m + top_k)
    x = _cuda(A)
    out = torch.full((m, FOUT), float("nan"), device="cuda")
    _, t_ws, y_ws = bestla.moe_workspace(m, top_k, FMID, FOUT, x.device)
    t_ws.fill_(float("nan"))
    y_ws.fill_(float("nan"))
    got = bestla.moe_ffn(g.bank, u.bank, d.bank, x, _cuda(ids), _cuda(w), act=act, out=out).cpu().numpy()
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
    print(f"moe_q6k moe_ffn {policy} {act} m={m} top_k={top_k}: workspace rows bit-identical; chain err {err:.3e} "
          f"(bar {TOL_CHAIN:.1e})")
    assert err <= TOL_CHAIN, err


def test_moe_ffn_out_of_range_slot(oracle):
    g, u, d = _banks(oracle, "q6k")
    m = 3
    A, _, w = _ffn_inputs(m, 2, 3)
    x = _cuda(A)
    good = np.array([[0, 1], [2, 0], [1, 3]], np.int32)
    ids = good.copy()
    ids[1, 0] = NE
    _, t_ws, y_ws = bestla.moe_workspace(m, 2, FMID, FOUT, x.device)
    bestla.moe_ffn(g.bank, u.bank, d.bank, x, _cuda(good), _cuda(w))
    y = y_ws.cpu().numpy().copy()
    y[2] = 0  # problem p = 1 * top_k + 0
    t_ws.fill_(float("nan"))
    got = bestla.moe_ffn(g.bank, u.bank, d.bank, x, _cuda(ids), _cuda(w))
    assert (_u32(t_ws[2].cpu().numpy()) == 0).all()
    assert np.array_equal(_u32(y_ws.cpu().numpy()), _u32(y))
    assert np.array_equal(_u32(got.cpu().numpy()), _u32(combine_f32(y, w, 2)))


# ------------------------------------------------------------------------------------------------ grouped
GN, GK = 200, 512


def _skewed_ids(m, rng):
    """expert 0 owns more than 128 rows (two tiles, the second partial), expert 2 none, some ids invalid"""
    ids = np.resize(np.array([0, 0, 0, 1, 0, 3, 0, 1], np.int32), m)
    ids = rng.permutation(ids)
    ids[[1, m // 2, m - 2]] = (-1, NE, 1 << 30)
    return ids


def _grouped_ids(m, rng):
    if m >= 300:
        return _skewed_ids(m, rng)
    ids = rng.permutation(np.resize(np.array([0, 0, 0, 1, 1, 3], np.int32), m))  # expert 2 empty
    ids[1], ids[m - 2] = -1, NE
    return ids


def _own_rows(w, x16_rows, **kw):
    """the expert's dense forward of fp16 rows on woq_q6k_gemm_kernel: at least 17 rows, the last repeated"""
    r = x16_rows.shape[0]
    if r < 17:
        x16_rows = torch.cat([x16_rows, x16_rows[-1:].expand(17 - r, -1)])
    assert w.plan(x16_rows.shape[0], "fp16")["kernel"] == "woq_q6k_gemm_kernel"
    return w.forward(x16_rows.contiguous(), **kw)[:r]


@pytest.mark.parametrize("m", [9, 70, 300])
def test_mul_mat_id_grouped(m):
    ex = _experts(GN, GK, "gmmid")
    rng = np.random.default_rng(7 + m)
    A = rng.uniform(-0.5, 0.5, size=(m, GK)).astype(np.float16).astype(np.float32)
    x = _cuda(A)
    ids = _grouped_ids(m, rng)
    if m >= 300:
        assert (ids == 0).sum() > 128 and (ids == 2).sum() == 0
    plan = bestla.plan_moe_grouped(ex.bank, None, None, m, 1)
    assert plan["bm"] == 128 and plan["launches"][2]["kernel"] == "woq_q6k_gemm_grouped_kernel"
    ids_t = _cuda(ids[:, None].copy())
    can, out = edges.out_window(m, GN, "aligned")
    (y,) = edges.twice(can, lambda: bestla.mul_mat_id_grouped(ex.bank, x, ids_t, 0, out=out), f"q6k grouped m={m}")
    # another batch: the rows in reverse order, every second one dropped -- other tiles, other tile rows
    keep = np.arange(m)[::-1][::2].copy()
    y2 = bestla.mul_mat_id_grouped(ex.bank, _cuda(A[keep]), _cuda(ids[keep][:, None].copy()), 0).cpu().numpy()
    assert np.array_equal(_u32(y2), _u32(y[keep])), "a row's bits depend on its batch"
    x16 = x.half()
    worst = 0.0
    for e in range(NE):
        rows = np.nonzero(ids == e)[0]
        if len(rows) == 0:
            continue
        own = _own_rows(ex.ws[e], x16[torch.from_numpy(rows).cuda()]).cpu().numpy()
        assert np.array_equal(_u32(y[rows]), _u32(own)), e
        worst = max(worst, _rel_err(y[rows], ex.ref(A[rows], e)))
    bad = np.nonzero((ids < 0) | (ids >= NE))[0]
    assert len(bad) >= 2 and (_u32(y[bad]) == 0).all()
    print(f"moe_q6k mul_mat_id_grouped m={m}: bit-identical to the dense GEMM and across batches; worst vs float64 "
          f"{worst:.3e} (bar {FOLD_TOL:.1e})")
    assert worst <= FOLD_TOL, worst


@pytest.mark.parametrize("m,top_k", [(9, 2), (70, 2), (300, 1)])
@pytest.mark.parametrize("policy", POLICIES)
def test_moe_ffn_grouped(oracle, policy, m, top_k):
    banks = _banks(oracle, policy)
    g, u, d = banks
    rng = np.random.default_rng(17 + m)
    A = rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)
    if top_k == 1:
        ids = _skewed_ids(m, rng)[:, None].copy()
    else:
        ids = np.stack([rng.choice(NE, size=top_k, replace=False, p=[0.4, 0.35, 0.2, 0.05]) for _ in range(m)])
        ids = ids.astype(np.int32)
        ids[5, 1] = NE
    w = rng.uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    x = _cuda(A)
    ws = bestla.moe_grouped_workspace_alloc(g.bank, u.bank, d.bank, m, top_k)
    ws.fill_(0xFF)
    can, out = edges.out_window(m, FOUT, "odd")
    (got,) = edges.twice(can, lambda: bestla.moe_ffn_grouped(g.bank, u.bank, d.bank, x, _cuda(ids), _cuda(w), out=out,
                                                             workspace=ws), f"q6k grouped ffn {policy} m={m}")
    v = bestla.moe_grouped_workspace_rows(ws, g.bank, u.bank, d.bank, m, top_k)
    perm, offs, inv, src = sort_ref(ids, NE)
    assert np.array_equal(v["inv"].cpu().numpy(), inv) and np.array_equal(v["offs"].cpu().numpy(), offs)
    nv = int(offs[NE])
    y = v["y"].cpu().numpy()[:nv]
    assert not np.isnan(y).any()
    assert np.array_equal(_u32(got), _u32(combine_sorted_f32(y, inv, w, top_k)))  # the last launch, no tolerance
    if g.bank.route == 2:  # the gate launch: each sorted row is the expert's dense GEMM of the fp16 row, then fp16
        x16, t16 = x.half(), v["t16"][:nv]
        for e in range(NE):
            q0, q1 = int(offs[e]), int(offs[e + 1])
            if q1 > q0:
                own = _own_rows(g.ws[e], x16[torch.from_numpy(src[q0:q1].astype(np.int64)).cuda()],
                                epilogue=bestla.EPI_SILU).half()
                assert torch.equal(t16[q0:q1].view(torch.int16), own.view(torch.int16)), e
    if d.bank.route == 2:  # the down launch: the dense GEMM of the sorted u16 rows as they lie
        u16 = v["u16"][:nv]
        for e in range(NE):
            q0, q1 = int(offs[e]), int(offs[e + 1])
            if q1 > q0:
                assert np.array_equal(_u32(y[q0:q1]), _u32(_own_rows(d.ws[e], u16[q0:q1]).cpu().numpy())), e
    err = _rel_err(got, _chain64(A, ids, w, banks, "silu"))
    print(f"moe_q6k moe_ffn_grouped {policy} m={m} top_k={top_k}: sorted rows bit-identical to the dense GEMM; chain err "
          f"{err:.3e} (bar {TOL_CHAIN:.1e})")
    assert err <= TOL_CHAIN, err


# ------------------------------------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("form", ["routed", "grouped"])
def test_routing_and_weights_are_read_at_replay(oracle, form):
    """one FFN on Q6_K banks captured once; ids and wts overwritten on the device between replays, then an expert's
    weight bytes: every replay is the eager result for what it found, bit for bit"""
    g, u, d = _banks(oracle, "q6k")
    m, top_k = (2, 2) if form == "routed" else (40, 2)
    rng = np.random.default_rng(5)
    x = _cuda(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32))
    choices = []
    for c in range(2):
        ids = np.stack([rng.permutation(NE)[:top_k] for _ in range(m)]).astype(np.int32)
        ids[0] = (0, 1) if c == 0 else (3, 2)
        choices.append((ids, rng.uniform(0.1, 0.9, size=(m, top_k)).astype(np.float32)))
    if form == "routed":
        ws = bestla.moe_workspace_alloc(m, top_k, FMID, FOUT)
        call = bestla.moe_ffn
    else:
        ws = bestla.moe_grouped_workspace_alloc(g.bank, u.bank, d.bank, m, top_k)
        call = bestla.moe_ffn_grouped

    def eager(which):
        return call(g.bank, u.bank, d.bank, x, _cuda(choices[which][0]), _cuda(choices[which][1]),
                    workspace=ws).cpu().numpy()

    want = [eager(0), eager(1)]
    assert not np.array_equal(want[0], want[1])
    ids, w = _cuda(choices[0][0]), _cuda(choices[0][1])
    out = torch.empty((m, FOUT), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(g.bank, u.bank, d.bank, x, ids, w, out=out, stream=s, workspace=ws)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            call(g.bank, u.bank, d.bank, x, ids, w, out=out, stream=s, workspace=ws)
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
    try:
        changed = eager(0)
        assert not np.array_equal(changed, want[0])
        assert np.array_equal(_u32(replay(0)), _u32(changed))
    finally:
        w0.mem.copy_(keep)
        torch.cuda.synchronize()
    assert np.array_equal(_u32(replay(0)), _u32(want[0]))
