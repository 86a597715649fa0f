"""The sorted, grouped routed FFN on the GPU: nad_device_mul_mat_id_grouped, nad_device_moe_ffn_grouped
(moe_sort_kernel, woq_gemm7_grouped_kernel, moe_gather_kernel).

Bars:
  * the sort against numpy's stable argsort with the invalid ids removed (tests/test_moe_grouped_cpu.py sort_ref): no
    tolerance, tile table included;
  * a grouped product row against the exact fp16 fold model of its expert (tests/fold_model.py): 2e-5 of max|ref|, the bar
    of tests/test_gemm7_matrix_gpu.py; against the oracle: FOLD_TOL (tests/test_gemm2_gpu.py);
  * the result for (x_r, e) is BIT-identical whatever else the batch holds, whatever the tile height, and to the expert's
    own DeviceWeight.forward of the fp16 rows where that runs gemm7 without split K: an output element's MFMA sequence
    and its (k-half 0) + (k-half 1) sum do not depend on the tile's other rows;
  * the FFN's last launch against numpy float32 on the device's own y rows and inv: no tolerance; the whole FFN against
    the float64 chain on the oracle: TOL["fp32"] = 1e-3, the bar test_ffn_prefill_fp16_intermediates sets for this
    chain with fp16 intermediates.
Weights come from fold_model.make (codes, scales and zero points over their whole ranges).  The formats are the four an
expert bank of tests/test_moe_gpu.py holds; int4 groups of 32 have no bank (nad_expert_bank_create refuses them,
tests/test_moe_cpu.py test_bank_errors_name_the_expert), so the grouped form cannot be reached with them.
"""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from neural_amd import bestla  # noqa: E402
from tests import edges  # noqa: E402
from tests import fold_model as fm  # noqa: E402
from tests.test_gemm2_gpu import FOLD_TOL, TOL  # noqa: E402
from tests.test_gpu_parity import _rel_err  # noqa: E402
from tests.test_moe_gpu import FIN, FMID, FORMATS, FOUT, NE, POLICIES  # noqa: E402
from tests.test_moe_grouped_cpu import combine_sorted_f32, sort_ref  # noqa: E402

BAR = TOL["fp16"]
HEIGHTS = (None, 32, 64)  # gemm7's own choice, and the two short tiles forced
M = 70
COUNTS = (32, 33, 0, 5)  # at 32-row tiles: a full tile, a tile plus one row, an empty expert, a short tile

_CACHE = {}


def _experts(oracle, n, k, fmt, tag):
    """NE experts of one shape and format -> (blobs, fold-model fp16 weights [k][n], DeviceWeights, ExpertBank)"""
    key = (n, k, fmt, tag)
    if key not in _CACHE:
        bs, qt, st, asym = FORMATS[fmt]
        made = [fm.make(oracle, n, k, bs or k, qt, st, asym, zlib.crc32(repr(key).encode()) % 10000 + 31 * e)
                for e in range(NE)]
        ws = [bestla.DeviceWeight(b) for b, _ in made]
        assert all(w.fold_ok == 1 for w in ws)
        _CACHE[key] = ([b for b, _ in made], [fm.folded_weights(Q, S, Z, bs or k) for _, (Q, S, Z) in made], ws,
                       bestla.ExpertBank(ws))
    return _CACHE[key]


def _ffn_banks(oracle, policy):
    gu, dn = POLICIES[policy]
    return (_experts(oracle, FMID, FIN, gu, "gate"), _experts(oracle, FMID, FIN, gu, "up"),
            _experts(oracle, FOUT, FMID, dn, "down"))


def _fp16_values(m, k, seed):
    A = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    return A.astype(np.float16).astype(np.float32)


def _counted_ids(counts, seed):
    ids = np.concatenate([np.full(c, e, np.int32) for e, c in enumerate(counts)])
    return np.random.default_rng(seed).permutation(ids)


def _weights(m, top_k, seed):
    w = np.random.default_rng(seed).uniform(0.1, 1.0, size=(m, top_k)).astype(np.float32)
    return (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the sort
SORT_CASES = {
    "counts_32_33_0_5": lambda rng: _counted_ids(COUNTS, 1)[:, None],
    "m40_top2_random": lambda rng: rng.integers(0, NE, size=(40, 2)).astype(np.int32),
    "all_65_rows_on_one_expert": lambda rng: np.full((65, 1), 2, np.int32),
    "m1_top2": lambda rng: np.array([[3, 1]], np.int32),
    "m3_each_row_another_expert": lambda rng: np.array([[2], [0], [3]], np.int32),
    "invalid_ids_mixed_in": lambda rng: rng.integers(-1, NE + 1, size=(40, 2)).astype(np.int32),
    "every_id_invalid": lambda rng: np.array([[-1, NE], [NE, -7]], np.int32),
    "more_problems_than_one_pass": lambda rng: rng.integers(-1, NE + 1, size=(1100, 2)).astype(np.int32),
}


@pytest.mark.parametrize("bm", HEIGHTS)
@pytest.mark.parametrize("case", list(SORT_CASES))
def test_sort_is_numpys_stable_argsort(oracle, knob, case, bm):
    knob("NAD_GEMM7_BM", bm)
    ids = SORT_CASES[case](np.random.default_rng(zlib.crc32(case.encode())))
    m, top_k = ids.shape
    if top_k == 1:  # the one-matmul form, the ids a column of a wider tensor
        _, _, _, bank = _experts(oracle, 64, 256, "int4_g128_f16_sym", "sort")
        banks = (bank, None, None)
        wide = torch.full((m, 3), 1, dtype=torch.int32, device="cuda")
        wide[:, 2] = torch.from_numpy(ids[:, 0]).cuda()
        x = torch.zeros((m, 256), device="cuda")

        def call(ws):
            bestla.mul_mat_id_grouped(bank, x, wide, 2, workspace=ws)
    else:
        banks = tuple(b[3] for b in _ffn_banks(oracle, "int4_sym"))
        ids_t = torch.from_numpy(ids).cuda()
        x = torch.zeros((m, FIN), device="cuda")
        wts = torch.ones((m, top_k), device="cuda")

        def call(ws):
            bestla.moe_ffn_grouped(*banks, x, ids_t, wts, workspace=ws)
    plan = bestla.plan_moe_grouped(*banks, m, top_k)
    assert bm is None or plan["bm"] == bm
    perm, offs, inv, src, tiles = sort_ref(ids, NE, plan["bm"])
    assert len(tiles) <= plan["bound"]
    nv = len(perm)
    ws = bestla.moe_grouped_workspace_alloc(*banks, m, top_k)
    got = []
    for fill in (0xFF, 0x00):  # whatever the workspace held: every word a launch reads is rewritten
        ws.fill_(fill)
        call(ws)
        v = bestla.moe_grouped_workspace_rows(ws, *banks, m, top_k)
        got.append({k: v[k].cpu().numpy().copy() for k in ("perm", "offs", "inv", "src", "ntiles", "tiles")})
    g = got[0]
    assert np.array_equal(g["offs"], offs)
    assert np.array_equal(g["perm"][:nv], perm) and (g["perm"][nv:] == -1).all()
    assert np.array_equal(g["src"][:nv], src) and (g["src"][nv:] == 0).all()
    assert np.array_equal(g["inv"], inv)
    assert int(g["ntiles"][0]) == len(tiles) and np.array_equal(g["tiles"][:len(tiles)], tiles)
    for k in ("perm", "offs", "inv", "src", "ntiles"):
        assert np.array_equal(got[0][k], got[1][k]), k
    assert np.array_equal(got[0]["tiles"][:len(tiles)], got[1]["tiles"][:len(tiles)])


# ------------------------------------------------------------------------------------------------ mul_mat_id_grouped
def _row_err(y_row, ref, r):
    """row r's error against the expert's product ref [M][n], relative to max|ref| -- the measure both bars are defined
    by (tests/test_gemm7_matrix_gpu.py edges.rel_err, tests/test_gemm2_gpu.py _rel_err: the largest error over the
    largest reference value of the product), taken row by row.  Relative to the row's own largest value the fp16 fold
    cannot hold FOLD_TOL: an fp32 scale rounds to fp16 with up to 2^-11 = 4.9e-4, a per-channel weight has one scale per
    column, and a column that carries a row's maximum passes that on whole (measured 5.07e-4 on int4 per-channel f32)."""
    return float(np.abs(y_row.astype(np.float64) - ref[r]).max() / np.abs(ref).max())


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_mul_mat_id_grouped(oracle, knob, fmt):
    n, k = FOUT, FIN
    blobs, w16, ws, bank = _experts(oracle, n, k, fmt, "mmid")
    A = _fp16_values(M, k, 7)
    x = torch.from_numpy(A).cuda()
    ids = _counted_ids(COUNTS, 3)
    ids[11] = -1
    ids[40] = NE
    model = [fm.model_product(A, w16[e]) for e in range(NE)]
    orc = [oracle.forward(A, blobs[e], n, k) for e in range(NE)]
    outs = []
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        can, out = edges.out_window(M, n, "aligned")
        (y,) = edges.twice(can, lambda: bestla.mul_mat_id_grouped(bank, x, torch.from_numpy(ids[:, None]).cuda(), 0,
                                                                  out=out), f"mul_mat_id_grouped {fmt} bm={bm}")
        outs.append(y)
    y = outs[0]
    for h, other in zip(HEIGHTS[1:], outs[1:]):
        assert np.array_equal(y.view(np.uint32), other.view(np.uint32)), f"tile height {h} changes the bits"
    worst_model = worst_orc = 0.0
    for r in range(M):
        e = int(ids[r])
        if not 0 <= e < NE:
            assert np.array_equal(y[r], np.zeros(n, np.float32)), r
            continue
        worst_model = max(worst_model, _row_err(y[r], model[e], r))
        worst_orc = max(worst_orc, _row_err(y[r], orc[e], r))
    print(f"mul_mat_id_grouped {fmt}: worst row vs fold model {worst_model:.3e} (bar {BAR:.1e}), vs oracle "
          f"{worst_orc:.3e} (bar {FOLD_TOL:.1e})")
    assert worst_model <= BAR, worst_model
    assert worst_orc <= FOLD_TOL, worst_orc

    # another batch: the rows reversed, every other row sent elsewhere -- a kept (x_r, e) keeps its bits
    knob("NAD_GEMM7_BM", None)
    back = np.arange(M)[::-1].copy()
    ids2 = ids[back].copy()
    ids2[::2] = (ids2[::2] + 1) % NE
    y2 = bestla.mul_mat_id_grouped(bank, x[torch.from_numpy(back).cuda()].contiguous(),
                                   torch.from_numpy(ids2[:, None]).cuda(), 0).cpu().numpy()
    kept = 0
    for j in range(M):
        r, e = int(back[j]), int(ids2[j])
        if e == int(ids[r]) and 0 <= e < NE:
            assert np.array_equal(y2[j], y[r]), (j, r, e)
            kept += 1
        elif 0 <= e < NE:
            assert _row_err(y2[j], model[e], r) <= BAR
    assert kept >= M // 4

    # each expert's own forward of the same rows as fp16, on gemm7 over the whole K
    knob("NAD_MID_MAX_M", 0)
    knob("NAD_SPLITK_DISABLE", 1)
    x16 = x.half()
    for e in range(NE):
        plan = ws[e].plan(M, "fp16")
        assert plan["kernel"] == "woq_gemm7_kernel" and plan["ksplit"] == 1, plan
        own = ws[e].forward(x16).cpu().numpy()
        rows = np.nonzero(ids == e)[0]
        assert np.array_equal(y[rows].view(np.uint32), own[rows].view(np.uint32)), e


# ------------------------------------------------------------------------------------------------ moe_ffn_grouped
def _act64(v, act):
    return edges.silu64(v) if act == "silu" else edges.gelu64(v)


def _chain64(oracle, A, ids, wts, banks, act):
    """the float64 chain on the oracle's products, each expert's rows in one call; an invalid id contributes nothing"""
    (gb, _, _, _), (ub, _, _, _), (db, _, _, _) = banks
    m, top_k = ids.shape
    out = np.zeros((m, FOUT), np.float64)
    for e in range(NE):
        rows, slots = np.nonzero(ids == e)
        if len(rows) == 0:
            continue
        h1 = oracle.forward(A[rows], gb[e], FMID, FIN).astype(np.float64)
        h3 = oracle.forward(A[rows], ub[e], FMID, FIN).astype(np.float64)
        t = (_act64(h1, act) * h3).astype(np.float32)
        d = oracle.forward(t, db[e], FOUT, FMID).astype(np.float64)
        np.add.at(out, rows, wts[rows, slots].astype(np.float64)[:, None] * d)
    return out


def _route(m, top_k, seed):
    """every row's experts distinct, expert 3 rare, one invalid slot"""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.choice(NE, size=top_k, replace=False, p=[0.4, 0.35, 0.2, 0.05]) for _ in range(m)])
    ids = ids.astype(np.int32)
    ids[5, top_k - 1] = NE
    return ids


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("top_k", [1, 2])
def test_moe_ffn_grouped(oracle, knob, policy, act, top_k):
    banks = _ffn_banks(oracle, policy)
    gate, up, down = (b[3] for b in banks)
    A = np.random.default_rng(100 + top_k).uniform(-0.5, 0.5, size=(M, FIN)).astype(np.float32)
    x = torch.from_numpy(A).cuda()
    ids = _route(M, top_k, 17 + top_k)
    w = _weights(M, top_k, 5)
    ids_t, w_t = torch.from_numpy(ids).cuda(), torch.from_numpy(w).cuda()
    ws = bestla.moe_grouped_workspace_alloc(gate, up, down, M, top_k)
    res = []
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        ws.fill_(0xFF)  # NaN in every fp16 / fp32 row, -1 in every index
        out = torch.full((M, FOUT), float("nan"), device="cuda")
        got = bestla.moe_ffn_grouped(gate, up, down, x, ids_t, w_t, act=act, out=out, workspace=ws).cpu().numpy()
        v = bestla.moe_grouped_workspace_rows(ws, gate, up, down, M, top_k)
        inv, y = v["inv"].cpu().numpy(), v["y"].cpu().numpy()
        assert np.array_equal(inv, sort_ref(ids, NE)[2])
        nv = int(v["offs"][NE])
        assert not np.isnan(y[:nv]).any() and not torch.isnan(v["u16"][:nv]).any()
        # (i) the last launch is numpy float32 on the device's own y rows and inv, no tolerance
        assert np.array_equal(got.view(np.uint32), combine_sorted_f32(y[:max(nv, 1)], inv, w, top_k).view(np.uint32))
        res.append((got, y, inv))
    got, y, inv = res[0]
    for h, (g2, y2, inv2) in zip(HEIGHTS[1:], res[1:]):
        assert np.array_equal(got.view(np.uint32), g2.view(np.uint32)), f"tile height {h} changes the bits"
        assert np.array_equal(y[:nv].view(np.uint32), y2[:nv].view(np.uint32))
    # (ii) the float64 chain on the oracle
    err = _rel_err(got, _chain64(oracle, A, ids, w, banks, act))
    print(f"moe_ffn_grouped {policy} {act} top_k={top_k}: err {err:.3e} bound {TOL['fp32']:.1e}")
    assert err <= TOL["fp32"], err
    # (iii) another batch: the rows reversed, the slots swapped, every third row's first expert moved on
    knob("NAD_GEMM7_BM", None)
    back = np.arange(M)[::-1].copy()
    ids2 = ids[back][:, ::-1].copy()
    ids2[::3, 0] = (ids2[::3, 0] + 1) % NE
    ws2 = bestla.moe_grouped_workspace_alloc(gate, up, down, M, top_k)
    bestla.moe_ffn_grouped(gate, up, down, x[torch.from_numpy(back).cuda()].contiguous(),
                           torch.from_numpy(ids2).cuda(), w_t, act=act, workspace=ws2)
    v2 = bestla.moe_grouped_workspace_rows(ws2, gate, up, down, M, top_k)
    inv2, y2 = v2["inv"].cpu().numpy(), v2["y"].cpu().numpy()
    where = {(r, int(ids[r, i])): int(inv[r * top_k + i]) for r in range(M) for i in range(top_k)}
    kept = 0
    for j in range(M):
        for i in range(top_k):
            q1, q2 = where.get((int(back[j]), int(ids2[j, i])), -1), int(inv2[j * top_k + i])
            if q1 >= 0 and q2 >= 0:
                assert np.array_equal(y2[q2].view(np.uint32), y[q1].view(np.uint32)), (j, i)
                kept += 1
    assert kept >= M // 2


# ------------------------------------------------------------------------------------------------ window
def _act_rows(xt, align):
    """16-B aligned rows either way (the entry's contract), NaN behind every row; "odd": a view at column 8"""
    m, k = xt.shape
    if align == "odd":
        store = torch.full((m, k + 24), float("nan"), device="cuda")
        x = store[:, 8:8 + k]
        x.copy_(xt)
    else:
        x = edges.act_window(xt, "aligned")
    assert x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0
    return x


@pytest.mark.parametrize("align", edges.ALIGNS)
def test_grouped_window(oracle, align):
    (_, _, _, gate), (_, _, _, up), (_, _, _, down) = _ffn_banks(oracle, "int4_sym")
    m, top_k = 37, 2
    rng = np.random.default_rng(21)
    xt = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    x = _act_rows(xt, align)
    ids = torch.from_numpy(_route(m, top_k, 2)).cuda()
    w = torch.from_numpy(_weights(m, top_k, 3)).cuda()
    can, out = edges.out_window(m, FOUT, align)
    (y,) = edges.twice(can, lambda: bestla.moe_ffn_grouped(gate, up, down, x, ids, w, out=out),
                       f"moe_ffn_grouped {align}")
    assert np.array_equal(y, bestla.moe_ffn_grouped(gate, up, down, xt, ids, w).cpu().numpy())
    can, out = edges.out_window(m, FMID, align)
    (y,) = edges.twice(can, lambda: bestla.mul_mat_id_grouped(gate, x, ids, 1, out=out),
                       f"mul_mat_id_grouped {align}")
    assert np.array_equal(y, bestla.mul_mat_id_grouped(gate, xt, ids, 1).cpu().numpy())


def test_grouped_refuses_unaligned_rows(oracle):
    _, _, _, bank = _experts(oracle, FMID, FIN, "int4_g128_f16_sym", "gate")
    flat = torch.zeros(2 * (FIN + 2) + 1, device="cuda")
    ids = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="16-B aligned base and lda % 4 == 0"):
        bestla.mul_mat_id_grouped(bank, flat[:2 * (FIN + 2)].view(2, FIN + 2)[:, :FIN], ids, 0)
    with pytest.raises(RuntimeError, match="16-B aligned base and lda % 4 == 0"):
        bestla.mul_mat_id_grouped(bank, flat[1:1 + 2 * FIN].view(2, FIN), ids, 0)


# ------------------------------------------------------------------------------------------------ graph
def test_grouped_routing_is_read_at_replay(oracle):
    """moe_ffn_grouped captured once; ids and wts overwritten on the device between replays -- a balanced routing, all
    rows on expert 0, a routing with invalid ids: each replay is the eager result for the ids it found, bit for bit
    (the tile counts shrink and grow between replays)."""
    (_, _, _, gate), (_, _, _, up), (_, _, _, down) = _ffn_banks(oracle, "int4_sym")
    m, top_k = M, 2
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(m, FIN)).astype(np.float32)).cuda()
    balanced = np.stack([(np.arange(m) * 2) % NE, (np.arange(m) * 2 + 1) % NE], axis=1).astype(np.int32)
    on_zero = np.zeros((m, top_k), np.int32)  # 140 problems, five 32-row tiles, on expert 0; none elsewhere
    invalid = _route(m, top_k, 9)
    invalid[::4, 0] = -1
    invalid[1::7, 1] = NE
    choices = [(balanced, _weights(m, top_k, 1)), (on_zero, _weights(m, top_k, 2)), (invalid, _weights(m, top_k, 3))]
    eager = [bestla.moe_ffn_grouped(gate, up, down, x, torch.from_numpy(i).cuda(), torch.from_numpy(w).cuda(),
                                    workspace=bestla.moe_grouped_workspace_alloc(gate, up, down, m, top_k))
             .cpu().numpy() for i, w in choices]
    assert not np.array_equal(eager[0], eager[1]) and not np.array_equal(eager[1], eager[2])
    ids = torch.from_numpy(choices[0][0]).cuda()
    w = torch.from_numpy(choices[0][1]).cuda()
    out = torch.empty((m, FOUT), device="cuda")
    ws = bestla.moe_grouped_workspace_alloc(gate, up, down, m, top_k)
    x_new = torch.zeros((m + 1, FIN), device="cuda")  # a shape no workspace is held for
    ids_new = torch.zeros((m + 1, top_k), dtype=torch.int32, device="cuda")
    w_new = torch.zeros((m + 1, top_k), device="cuda")
    out_new = torch.empty((m + 1, FOUT), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bestla.moe_ffn_grouped(gate, up, down, x, ids, w, out=out, stream=s, workspace=ws)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            bestla.moe_ffn_grouped(gate, up, down, x, ids, w, out=out, stream=s, workspace=ws)
            with pytest.raises(RuntimeError, match="outside graph capture or pass workspace="):
                bestla.moe_ffn_grouped(gate, up, down, x_new, ids_new, w_new, out=out_new, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    for which in (0, 1, 2, 0):
        ids.copy_(torch.from_numpy(choices[which][0]))
        w.copy_(torch.from_numpy(choices[which][1]))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), eager[which].view(np.uint32)), which
