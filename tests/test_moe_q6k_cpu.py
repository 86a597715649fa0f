"""Banks of GGUF Q6_K experts (route kind 2, NAD_BANK_GENERAL), the host side: no GPU needed.

The launch shapes are restated here from woq_q6k.hip, never read back from the library: the row-routed kernel runs 16
waves, max(1, min(stripes, CUs / problems)) workgroups per problem, and stages one fp32 row as its hi and lo fp16 rows
beside the 32 KiB of per-wave partial sums (4 K + 32768 bytes of LDS); the grouped kernel is the dense Q6_K GEMM's
128 x 128 tile on 512 threads with static LDS.
"""
import numpy as np
import pytest

from neural_amd import bestla
from neural_amd._lib import lib
from tests.test_moe_grouped_cpu import bound

NE = 4
FIN, FMID, FOUT = 512, 768, 72
CUS = 256  # without a device, and on the MI355X
Q6K_ROUTED, Q6K_GROUPED = "woq_q6k_gemv_routed_kernel", "woq_q6k_gemm_grouped_kernel"
GENERAL, LEAN, G7 = "woq_gemv_routed_kernel", "woq_gemv_m1_routed_kernel", "woq_gemm7_grouped_kernel"


def q6k(n, k, ne=NE, general=True):
    return bestla.ExpertBank.plan_only([(6, n, k, 16, "fp16", False)] * ne, general=general)


def other(bits, n, k, group, ne=NE):
    return bestla.ExpertBank.plan_only([(bits, n, k, group, "fp16", False)] * ne, general=True)


def routed_launch(n, k, nprob):
    ns = -(-n // 16)
    return dict(kernel=Q6K_ROUTED, grid=nprob * max(1, min(ns, CUS // nprob)), threads=1024, lds=4 * k + 32768)


def test_a_q6k_bank_is_accepted_and_reports_kind_2():
    bank = q6k(FMID, FIN)
    assert (bank.route, bank.bits, bank.blocksize, bank.n, bank.k, bank.n_expert) == (2, 6, 16, FMID, FIN, NE)
    assert bank.has_weights == 0 and bank.asym == 0
    o = np.full(9, -7, np.int64)
    assert lib().nad_expert_bank_info(bank.handle, bestla._ptr(o), 9) == 9 and o[8] == 2 and o[1] == 6 and o[4] == 16
    o8 = np.full(9, -7, np.int64)
    assert lib().nad_expert_bank_info(bank.handle, bestla._ptr(o8), 8) == 8 and o8[8] == -7 and (o8[:8] == o[:8]).all()
    assert q6k(40, 256, ne=1).route == 2  # any N, one superblock, one expert


def test_refusals_by_name():
    one = (6, FMID, FIN, 16, "fp16", False)
    ok4 = (4, FMID, FIN, 128, "fp16", False)
    # an all-Q6_K bank without the flag: the old entries' message, and what to do about it
    with pytest.raises(RuntimeError, match="expert 0's weight is GGUF Q6_K.*NAD_BANK_GENERAL"):
        q6k(FMID, FIN, general=False)
    g = np.array([[6, FMID, FIN, 16, 2, 0]] * NE, np.int32)
    assert not lib().nad_expert_bank_plan_only(bestla._ptr(g), NE)
    assert "nad_expert_bank_plan_only: expert 0's weight is GGUF Q6_K" in bestla.last_error()
    assert not lib().nad_expert_bank_plan_only_ex(bestla._ptr(g), NE, 0)
    assert "nad_expert_bank_plan_only_ex: expert 0's weight is GGUF Q6_K" in bestla.last_error()
    # a Q6_K expert in a bank whose expert 0 is not Q6_K, under either flag value
    for general in (False, True):
        with pytest.raises(RuntimeError, match="expert 2's weight is GGUF Q6_K") as err:
            bestla.ExpertBank.plan_only([ok4, ok4, one, ok4], general=general)
        assert "NAD_BANK_GENERAL" not in str(err.value)  # the flag would not help this bank
    # ... and the other way round: expert 0 decides the bank's format
    with pytest.raises(RuntimeError, match="expert 1's weight differs in shape or format from expert 0's"):
        bestla.ExpertBank.plan_only([one, ok4], general=True)
    with pytest.raises(RuntimeError, match="expert 3's weight differs in shape or format from expert 0's"):
        bestla.ExpertBank.plan_only([one, one, one, (6, FMID, 2 * FIN, 16, "fp16", False)], general=True)
    assert not lib().nad_expert_bank_plan_only_ex(bestla._ptr(g), NE, 2)
    assert "unknown flags" in bestla.last_error()
    with pytest.raises(RuntimeError, match="bad geometry"):  # K is whole superblocks
        q6k(FMID, 300)
    # gate and up of one FFN must both be Q6_K
    gate, down = q6k(FMID, FIN), q6k(FOUT, FMID)
    with pytest.raises(RuntimeError, match=r"gate and up banks differ in group size \(16 vs 128\)"):
        bestla.plan_moe(gate, other(4, FMID, FIN, 128), down, 3, 2)
    # the two fp16 rows of K = 36864 and the partials are 176 KiB
    long_k = q6k(64, 36864)
    with pytest.raises(RuntimeError, match="K = 36864 is too long for the routed Q6_K kernel's LDS staging"):
        bestla.plan_moe(q6k(36864, FIN), q6k(36864, FIN), long_k, 1, 2)
    assert bestla.plan_moe(q6k(32768, FIN), q6k(32768, FIN), q6k(64, 32768), 1, 2)[2]["lds"] == 160 * 1024


@pytest.mark.parametrize("m,top_k", [(1, 2), (40, 1), (300, 1)])
def test_plan_moe_of_an_all_q6k_ffn(m, top_k):
    gate, up, down = q6k(FMID, FIN), q6k(FMID, FIN), q6k(FOUT, FMID)
    plan = bestla.plan_moe(gate, up, down, m, top_k)
    nprob = m * top_k
    assert plan == [routed_launch(FMID, FIN, nprob), routed_launch(FMID, FIN, nprob), routed_launch(FOUT, FMID, nprob),
                    dict(kernel="moe_combine_kernel", grid=m * -(-FOUT // 256), threads=256, lds=0)]
    o = np.full(20, -7, np.int64)
    assert lib().nad_plan_moe(gate.handle, up.handle, down.handle, m, top_k, bestla._ptr(o), 20) == 17
    assert o[16] == 4 and o[17] == -7 and [int(o[4 * i]) for i in range(4)] == [22, 22, 22, 15]
    o5 = np.full(20, -7, np.int64)
    assert lib().nad_plan_moe(gate.handle, up.handle, down.handle, m, top_k, bestla._ptr(o5), 5) == 5
    assert (o5[:5] == o[:5]).all() and o5[5] == -7


def test_plan_moe_of_mixed_ffns():
    """Q6_K gate / up with a Q8_0-layout down (int8 g32, the stripe stream), and int4 g128 gate / up (the M = 1
    stream) with a Q6_K down: each launch is its own bank's"""
    gate, q80_down = q6k(FMID, FIN), other(8, FOUT, FMID, 32)
    assert q80_down.route == 1
    plan = bestla.plan_moe(gate, gate, q80_down, 3, 2)
    assert [p["kernel"] for p in plan] == [Q6K_ROUTED, Q6K_ROUTED, GENERAL, "moe_combine_kernel"]
    assert plan[:2] == [routed_launch(FMID, FIN, 6)] * 2
    alone = bestla.plan_moe(other(8, FMID, FIN, 32), other(8, FMID, FIN, 32), q80_down, 3, 2)
    assert plan[2] == alone[1]
    g4 = other(4, FMID, FIN, 128)
    assert g4.route == 0
    plan = bestla.plan_moe(g4, g4, q6k(FOUT, FMID), 3, 2)
    assert [p["kernel"] for p in plan] == [LEAN, Q6K_ROUTED, "moe_combine_kernel"]
    assert plan[1] == routed_launch(FOUT, FMID, 6)


def test_the_13_value_form_is_unchanged_for_other_ffns():
    g4, d4 = other(4, FMID, FIN, 128), other(4, FOUT, FMID, 128)
    o = np.full(20, -7, np.int64)
    assert lib().nad_plan_moe(g4.handle, g4.handle, d4.handle, 3, 2, bestla._ptr(o), 20) == 13
    assert o[12] == 3 and o[13] == -7 and [int(o[4 * i]) for i in range(3)] == [14, 14, 15]
    plan = bestla.plan_moe(g4, g4, d4, 3, 2)
    assert len(plan) == 3 and [p["kernel"] for p in plan] == [LEAN, LEAN, "moe_combine_kernel"]
    assert [(p["grid"], p["threads"], p["lds"]) for p in plan] == [(int(o[4 * i + 1]), int(o[4 * i + 2]),
                                                                    int(o[4 * i + 3])) for i in range(3)]


def _r256(v):
    return -(-v // 256) * 256


@pytest.mark.parametrize("m,top_k", [(9, 2), (70, 2), (300, 1)])
def test_plan_moe_grouped(knob, m, top_k):
    gate, up, down = q6k(FMID, FIN), q6k(FMID, FIN), q6k(FOUT, FMID)
    np_ = m * top_k
    for bm in (None, 32):  # the knob does not apply: the Q6_K kernel has one tile height
        knob("NAD_GEMM7_BM", bm)
        plan = bestla.plan_moe_grouped(gate, up, down, m, top_k)
        assert plan["bm"] == 128 and plan["bound"] == np_ // 128 + min(NE, np_) == bound(np_, NE, 128)
        ls = plan["launches"]
        assert [p["kernel"] for p in ls] == ["moe_sort_kernel", "nad_cvt_act_kernel", Q6K_GROUPED, Q6K_GROUPED,
                                             Q6K_GROUPED, "moe_gather_kernel"]
        for p, n in ((ls[2], FMID), (ls[3], FMID), (ls[4], FOUT)):
            assert (p["grid"], p["threads"], p["lds"]) == (plan["bound"] * -(-(-(-n // 16)) // 8), 512, 0), p
        one = bestla.plan_moe_grouped(gate, None, None, m, 1)
        assert one["bm"] == 128 and [p["kernel"] for p in one["launches"]] == [
            "moe_sort_kernel", "nad_cvt_act_kernel", Q6K_GROUPED, "moe_gather_kernel"]
    # the documented layout with kp = K; the tile table is sized for 32-row tiles whatever the call's height
    head = _r256((NE + 1) * 4) + 3 * _r256(np_ * 4) + _r256(16 + 16 * (np_ // 32 + min(NE, np_))) + _r256(m * FIN * 2)
    assert bestla.moe_grouped_workspace_size(gate, up, down, m, top_k) == \
        head + 2 * _r256(np_ * FMID * 2) + _r256(np_ * FOUT * 4)
    assert bestla.moe_grouped_workspace_size(gate, None, None, m, 1) == \
        _r256((NE + 1) * 4) + 3 * _r256(m * 4) + _r256(16 + 16 * (m // 32 + min(NE, m))) + _r256(m * FIN * 2) + \
        _r256(m * FMID * 4)


def test_plan_moe_grouped_of_mixed_ffns(knob):
    """one Q6_K bank makes the whole call 128 rows high; gemm7's grouped kernel serves the other banks at 128"""
    knob("NAD_GEMM7_BM", 32)
    g4, d4 = other(4, FMID, FIN, 128), other(4, FOUT, FMID, 128)
    assert bestla.plan_moe_grouped(g4, g4, d4, 70, 2)["bm"] == 32
    plan = bestla.plan_moe_grouped(g4, g4, q6k(FOUT, FMID), 70, 2)
    assert plan["bm"] == 128 and [p["kernel"] for p in plan["launches"]][2:5] == [G7, G7, Q6K_GROUPED]
    plan = bestla.plan_moe_grouped(q6k(FMID, FIN), q6k(FMID, FIN), d4, 70, 2)
    assert plan["bm"] == 128 and [p["kernel"] for p in plan["launches"]][2:5] == [Q6K_GROUPED, Q6K_GROUPED, G7]
    assert plan["launches"][4]["grid"] == plan["bound"] * -(-FOUT // 128) and plan["launches"][4]["lds"] > 0


def test_grouped_refuses_an_fmid_that_is_not_whole_superblocks():
    gate = other(4, 640, FIN, 128)  # fmid = 640 = 2.5 superblocks; the down bank's own K is whole ones by construction
    with pytest.raises(RuntimeError, match=r"fmid \(640\) is not a whole number of the Q6_K down bank's superblocks"):
        bestla.plan_moe_grouped(gate, gate, q6k(FOUT, 768), 40, 2)


def test_a_plan_only_bank_launches_nothing():
    bank = q6k(FMID, FIN)
    x = np.zeros((1, FIN), np.float32)
    ids = np.zeros((1, 2), np.int32)
    out = np.zeros((1, FMID), np.float32)
    vp = bestla._ptr
    rc = lib().nad_device_mul_mat_id(bank.handle, vp(x), vp(ids), 2, 0, vp(out), 1, FIN, FMID, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()
    ws = np.zeros(1 << 16, np.uint8)
    rc = lib().nad_device_mul_mat_id_grouped(bank.handle, vp(x), vp(ids), 2, 0, vp(ws), vp(out), 1, FIN, FMID, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()
    down = q6k(FOUT, FMID)
    w = np.ones((1, 2), np.float32)
    o = np.zeros((1, FOUT), np.float32)
    rc = lib().nad_device_moe_ffn(bank.handle, bank.handle, down.handle, vp(x), vp(ids), 2, vp(w), 2, 2,
                                  bestla.EPI_SILU_MUL, vp(ws), vp(o), 1, FIN, FOUT, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()
    assert not out.any() and not o.any()
