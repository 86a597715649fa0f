"""The sorted, grouped routed FFN (nad_plan_moe_grouped, nad_moe_grouped_workspace_size), the host side: no GPU needed.

Geometry-only banks serve the dry run.  sort_ref below is the numpy restatement of moe_sort_kernel (a stable argsort
with the invalid ids removed) and combine_sorted_f32 that of the last launch; the GPU tests import both.
"""
import numpy as np
import pytest

from neural_amd import bestla
from neural_amd._lib import lib

FIN, FMID, FOUT, NE = 1024, 512, 300, 4
G128 = (128, "fp16", False)
HEIGHTS = (32, 64, 128, 256)
FFN_KERNELS = ["moe_sort_kernel", "nad_cvt_act_kernel", "woq_gemm7_grouped_kernel", "woq_gemm7_grouped_kernel",
               "woq_gemm7_grouped_kernel", "moe_gather_kernel"]


def sort_ref(ids, n_expert, bm=None):
    """ids [m][top_k] -> (perm, offs, inv, src[, tiles]) as the header defines them: the valid problems p = r * top_k +
    i by (expert, p); offs the experts' row ranges; inv the sorted position of p or -1; tiles (e, q0, q1, 0)."""
    ids = np.asarray(ids)
    m, top_k = ids.shape
    e = ids.reshape(-1).astype(np.int64)
    valid = (e >= 0) & (e < n_expert)
    order = np.argsort(np.where(valid, e, n_expert), kind="stable")
    perm = order[:int(valid.sum())].astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(e[valid], minlength=n_expert))]).astype(np.int32)
    inv = np.full(m * top_k, -1, np.int32)
    inv[perm] = np.arange(len(perm), dtype=np.int32)
    out = (perm, offs, inv, (perm // top_k).astype(np.int32))
    if bm is None:
        return out
    tiles = [(x, q0, min(q0 + bm, int(offs[x + 1])), 0) for x in range(n_expert)
             for q0 in range(int(offs[x]), int(offs[x + 1]), bm)]
    return out + (np.array(tiles, np.int32).reshape(-1, 4),)


def combine_sorted_f32(y, inv, wts, top_k):
    """tests/test_moe_cpu.py combine_f32 on y[inv[p]], an invalid slot (inv < 0) reading 0.0f"""
    from tests.test_moe_cpu import combine_f32
    y = np.asarray(y, np.float32)
    inv = np.asarray(inv)
    rows = np.where(inv[:, None] >= 0, y[np.maximum(inv, 0)], np.float32(0))
    return combine_f32(rows.astype(np.float32), wts, top_k)


def bound(np_, ne, bm):
    return np_ // bm + min(ne, np_)


def _banks(bits=4, group=G128, fin=FIN, fmid=FMID, fout=FOUT, ne=NE, down=G128):
    gate = bestla.ExpertBank.plan_only([(bits, fmid, fin) + group] * ne)
    up = bestla.ExpertBank.plan_only([(bits, fmid, fin) + group] * ne)
    return gate, up, bestla.ExpertBank.plan_only([(4, fout, fmid) + down] * ne)


def _check_plan(plan, banks, m, top_k, bm=None):
    gate, up, down = banks
    ls = plan["launches"]
    assert [p["kernel"] for p in ls] == FFN_KERNELS
    assert plan["bm"] in HEIGHTS and (bm is None or plan["bm"] == bm), plan
    np_ = m * top_k
    assert plan["bound"] == bound(np_, gate.n_expert, plan["bm"]), plan
    assert (ls[0]["grid"], ls[0]["threads"], ls[0]["lds"]) == (1, 1024, 0)
    for p, n in ((ls[2], gate.n), (ls[3], up.n), (ls[4], down.n)):
        assert p["grid"] == plan["bound"] * -(-n // 128), (p, plan)
        assert p["threads"] == 512 and 0 < p["lds"] <= 160 * 1024
    assert ls[5]["threads"] == 256 and ls[5]["grid"] == m * -(-down.n // 256)


@pytest.mark.parametrize("m,top_k", [(1, 2), (3, 1), (70, 2), (200, 1), (2048, 2)])
def test_plan_launches_codes_and_grids(m, top_k):
    banks = _banks()
    _check_plan(bestla.plan_moe_grouped(*banks, m, top_k), banks, m, top_k)


@pytest.mark.parametrize("bm", HEIGHTS)
def test_tile_height_follows_the_knob_and_the_bound_its_formula(knob, bm):
    knob("NAD_GEMM7_BM", bm)
    banks = _banks()
    # np < n_expert, np = BM, np = BM + 1, and a few tiles per expert
    for m, top_k in ((3, 1), (1, 2), (bm, 1), (bm // 2, 2), (bm + 1, 1), (5 * bm + 3, 2)):
        plan = bestla.plan_moe_grouped(*banks, m, top_k)
        _check_plan(plan, banks, m, top_k, bm)
    assert bestla.plan_moe_grouped(*banks, 3, 1)["bound"] == 3          # 0 full tiles + min(4, 3)
    assert bestla.plan_moe_grouped(*banks, bm, 1)["bound"] == 1 + NE
    assert bestla.plan_moe_grouped(*banks, bm + 1, 1)["bound"] == 1 + NE
    assert bestla.plan_moe_grouped(*banks, 2 * bm, 1)["bound"] == 2 + NE


def test_default_tile_height_is_gemm7s_choice_for_the_mean_rows_per_expert(knob):
    knob("NAD_GEMM7_BM", None)
    banks = _banks()
    assert bestla.plan_moe_grouped(*banks, 64, 2)["bm"] == 32   # 128 problems over 4 experts: 32 rows each
    assert bestla.plan_moe_grouped(*banks, 66, 2)["bm"] >= 64   # 33 rows each: past the 32-row tile


@pytest.mark.parametrize("policy", ["int4", "int2_gate_up"])
def test_plan_mixtral_sizes(knob, policy):
    knob("NAD_GEMM7_BM", None)
    fin, fmid, ne = 4096, 14336, 8
    banks = (_banks(fin=fin, fmid=fmid, fout=fin, ne=ne) if policy == "int4" else
             _banks(bits=2, group=(64, "fp16", False), fin=fin, fmid=fmid, fout=fin, ne=ne))
    for m in (16, 64, 256, 2048):
        plan = bestla.plan_moe_grouped(*banks, m, 2)
        _check_plan(plan, banks, m, 2)
        assert plan["launches"][2]["grid"] == bound(2 * m, ne, plan["bm"]) * (fmid // 128)
        assert plan["launches"][4]["grid"] == bound(2 * m, ne, plan["bm"]) * (fin // 128)
        if 2 * m <= 32 * ne:  # at most 32 rows per expert on average: gemm7's 32-row tile
            assert plan["bm"] == 32


def test_plan_one_matmul_form():
    bank = bestla.ExpertBank.plan_only([(4, FOUT, FIN) + G128] * NE)
    plan = bestla.plan_moe_grouped(bank, None, None, 70, 1)
    assert [p["kernel"] for p in plan["launches"]] == ["moe_sort_kernel", "nad_cvt_act_kernel",
                                                       "woq_gemm7_grouped_kernel", "moe_gather_kernel"]
    assert plan["bound"] == bound(70, NE, plan["bm"])
    assert plan["launches"][2]["grid"] == plan["bound"] * -(-FOUT // 128)
    with pytest.raises(RuntimeError, match="one-matmul form has top_k = 1"):
        bestla.plan_moe_grouped(bank, None, None, 70, 2)


def _r256(v):
    return -(-v // 256) * 256


@pytest.mark.parametrize("m,top_k", [(1, 2), (5, 2), (70, 1), (7, 3)])
@pytest.mark.parametrize("bits,group,ktile", [(4, G128, 128), (2, (64, "fp16", False), 256)])
def test_workspace_size_is_the_documented_layout(m, top_k, bits, group, ktile):
    fin = 1000  # not a whole number of K tiles: x16 is padded
    gate, up, down = _banks(bits=bits, group=group, fin=fin)
    np_ = m * top_k
    kp = -(-fin // ktile) * ktile
    head = (_r256((NE + 1) * 4) + 3 * _r256(np_ * 4) + _r256(16 + 16 * (np_ // 32 + min(NE, np_))) +
            _r256(m * kp * 2))
    assert bestla.moe_grouped_workspace_size(gate, up, down, m, top_k) == \
        head + 2 * _r256(np_ * FMID * 2) + _r256(np_ * FOUT * 4)
    if top_k == 1:  # the one-matmul form: no fp16 intermediates, y has the bank's own N
        assert bestla.moe_grouped_workspace_size(gate, None, None, m, 1) == head + _r256(np_ * FMID * 4)


def test_refusals_name_their_cause():
    gate, up, down = _banks()
    # a group gemm7 does not fold: per-channel over K = 384 is one group of 3 K tiles (not 128 * 2^j); the bank itself
    # exists, because the M = 1 GEMV takes it
    odd = bestla.ExpertBank.plan_only([(4, FMID, 384, -1, "fp16", False)] * NE)
    with pytest.raises(RuntimeError, match=r"the gate bank \(int4, groups of 384\) does not take the grouped gemm7"):
        bestla.plan_moe_grouped(odd, odd, down, 40, 2)
    with pytest.raises(RuntimeError, match=r"the given bank \(int4, groups of 384\) does not take the grouped gemm7"):
        bestla.plan_moe_grouped(odd, None, None, 40, 1)
    odd_down = bestla.ExpertBank.plan_only([(4, FOUT, FMID, -1, "fp16", False)] * NE)  # one group of 512: fine
    bestla.plan_moe_grouped(gate, up, odd_down, 40, 2)
    # fmid = 448 = 7 groups of 64, but 3.5 K tiles of the down bank
    g448, u448, d448 = _banks(fmid=448, down=(64, "fp16", False))
    with pytest.raises(RuntimeError, match=r"fmid \(448\) is not a whole number of the down bank's K tiles \(128 deep\)"):
        bestla.plan_moe_grouped(g448, u448, d448, 40, 2)
    # mismatched banks, as nad_plan_moe names them
    up64 = bestla.ExpertBank.plan_only([(4, FMID, FIN, 64, "fp16", False)] * NE)
    with pytest.raises(RuntimeError, match=r"gate and up banks differ in group size \(128 vs 64\)"):
        bestla.plan_moe_grouped(gate, up64, down, 40, 2)
    wrong_k = bestla.ExpertBank.plan_only([(4, FOUT, FMID * 2) + G128] * NE)
    with pytest.raises(RuntimeError, match="down bank's K"):
        bestla.plan_moe_grouped(gate, up, wrong_k, 40, 2)
    fewer = bestla.ExpertBank.plan_only([(4, FOUT, FMID) + G128] * (NE - 1))
    with pytest.raises(RuntimeError, match="the banks hold 4 / 4 / 3 experts"):
        bestla.plan_moe_grouped(gate, up, fewer, 40, 2)
    assert lib().nad_plan_moe_grouped(gate.handle, None, down.handle, 40, 2, None, 0) == -1
    assert "the up bank is not an expert bank" in bestla.last_error()


def test_plan_only_banks_do_not_launch_and_nothing_falls_back():
    gate, up, down = _banks()
    vp = bestla._ptr
    x = np.zeros((2, FIN), np.float32)
    ids = np.zeros((2, 2), np.int32)
    w = np.zeros((2, 2), np.float32)
    out = np.zeros((2, FOUT), np.float32)
    ws = np.zeros(bestla.moe_grouped_workspace_size(gate, up, down, 2, 2) + 16, np.uint8)
    wp = ws[(-ws.ctypes.data) % 16:]
    rc = lib().nad_device_moe_ffn_grouped(gate.handle, up.handle, down.handle, vp(x), vp(ids), 2, vp(w), 2, 2,
                                          bestla.EPI_SILU_MUL, vp(wp), vp(out), 2, FIN, FOUT, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()
    rc = lib().nad_device_moe_ffn_grouped(gate.handle, up.handle, down.handle, vp(x), vp(ids), 2, vp(w), 2, 2,
                                          bestla.EPI_SILU_MUL, vp(wp), vp(out), 2, FIN + 2, FOUT, None)
    assert rc == -1 and "lda % 4 == 0" in bestla.last_error()
    rc = lib().nad_device_mul_mat_id_grouped(gate.handle, vp(x), vp(ids), 2, 0, None, vp(out), 2, FIN, FMID, None)
    assert rc == -1 and "bad arguments" in bestla.last_error()
    # a bank the grouped form does not take is an error there, whatever the row-routed form would do with it
    odd = bestla.ExpertBank.plan_only([(4, FMID, 384, -1, "fp16", False)] * NE)
    x3 = np.zeros((2, 384), np.float32)
    rc = lib().nad_device_mul_mat_id_grouped(odd.handle, vp(x3), vp(ids), 2, 0, vp(wp), vp(out), 2, 384, FMID, None)
    assert rc == -1 and "does not take the grouped gemm7" in bestla.last_error()


def test_sort_restatement():
    ids = np.array([[2, 0], [0, 7], [-1, 2], [2, 2]], np.int32)
    perm, offs, inv, src, tiles = sort_ref(ids, 4, bm=2)
    assert perm.tolist() == [1, 2, 0, 5, 6, 7] and src.tolist() == [0, 1, 0, 2, 3, 3]
    assert offs.tolist() == [0, 2, 2, 6, 6]
    assert inv.tolist() == [2, 0, 1, -1, -1, 3, 4, 5]
    assert tiles.tolist() == [[0, 0, 2, 0], [2, 2, 4, 0], [2, 4, 6, 0]]
    y = np.arange(12, dtype=np.float32).reshape(6, 2)
    w = np.full((4, 2), 0.5, np.float32)
    assert combine_sorted_f32(y, inv, w, 2).tolist() == [[2.0, 3.0], [1.0, 1.5], [3.0, 3.5], [9.0, 10.0]]
