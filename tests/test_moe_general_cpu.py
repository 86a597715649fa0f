"""General expert banks (nad_expert_bank_create_ex / _plan_only_ex with NAD_BANK_GENERAL), the host side: no GPU needed.

A general bank also takes the weights the stripe-stream GEMV runs at M = 1 where the M = 1 stream does not -- int4
groups of 32 sym, int8 -- and routes them through woq_gemv_routed_kernel.  The waves and the LDS image of a launch are
restated here from woq_gemv.hip (gemv_waves, gemv_lds_layout's stripe-stream branch), never read back from the library.
"""
import numpy as np
import pytest

from neural_amd import bestla
from neural_amd._lib import lib
from tests.test_moe_grouped_cpu import FFN_KERNELS, HEIGHTS, bound

FIN, FMID, FOUT, NE = 1024, 512, 300, 4
G128 = (128, "fp16", False)
CUS = 256  # without a device, and on the MI355X
GENERAL, LEAN = "woq_gemv_routed_kernel", "woq_gemv_m1_routed_kernel"

# (bits, group, scale type, asym) of every format a general bank adds
FORMATS = [(4, 32, st, False) for st in ("fp32", "fp16", "bf16")] + \
          [(8, g, "fp16", asym) for g in (32, 64, 128, -1) for asym in (False, True)]


def ktile(bits):
    return {4: 128, 2: 256, 8: 64}[bits]


def waves_of(bits, k, group):
    """gemv_waves: balanced 4-tile K-slices per wave, at most 16 waves, 8 where a K tile holds several groups"""
    nt = -(-k // ktile(bits))
    several = group > 0 and group < ktile(bits) and -(-k // group) > 1
    maxw = 8 if several else 16
    nsl = -(-nt // 4)
    spw = -(-nsl // maxw)
    return -(-nsl // spw)


def lds_of(bits, k, group, units, wpp, dual):
    """gemv_lds_layout for one fp32 row: hi, lo and zero fp16 rows of the padded K, then [stripes][waves][16] floats"""
    kp = -(-k // ktile(bits)) * ktile(bits)
    part_off = (3 * kp * 2 + 15) // 16 * 16
    return part_off + -(-units // wpp) * (2 if dual else 1) * waves_of(bits, k, group) * 16 * 4


def general(geom, ne=NE):
    return bestla.ExpertBank.plan_only([geom] * ne, general=True)


def _ffn(bits, group, st, asym, fin=FIN, fmid=FMID, fout=FOUT):
    g = general((bits, fmid, fin, group, st, asym))
    u = general((bits, fmid, fin, group, st, asym))
    d = general((bits, fout, fmid, group, st, asym))
    return g, u, d


def test_the_entries_exist_and_flags_zero_is_the_old_entry():
    L = lib()
    g = np.array([[4, FMID, FIN, 128, 2, 0]] * NE, np.int32)
    h = L.nad_expert_bank_plan_only_ex(bestla._ptr(g), NE, 0)
    assert h
    o = np.zeros(9, np.int64)
    assert L.nad_expert_bank_info(h, bestla._ptr(o), 9) == 9 and o[8] == 0
    o8 = np.full(9, -7, np.int64)
    assert L.nad_expert_bank_info(h, bestla._ptr(o8), 8) == 8 and o8[8] == -7 and (o8[:8] == o[:8]).all()
    L.nad_expert_bank_destroy(h)
    g32 = np.array([[4, FMID, FIN, 32, 2, 0]] * NE, np.int32)
    assert not L.nad_expert_bank_plan_only_ex(bestla._ptr(g32), NE, 0)
    assert "does not take the M = 1 GEMV" in bestla.last_error()
    assert not L.nad_expert_bank_plan_only_ex(bestla._ptr(g32), NE, 2)
    assert "unknown flags" in bestla.last_error()
    import ctypes as C
    desc = (C.c_uint8 * L.bestla_device_storage_size())()  # zeros: no magic
    arr = (C.c_void_p * 1)(C.cast(desc, C.c_void_p))
    assert not L.nad_expert_bank_create_ex(arr, 1, bestla.BANK_GENERAL)
    assert "expert 0's descriptor is not a loaded neural_amd device weight" in bestla.last_error()


@pytest.mark.parametrize("bits,group,st,asym", FORMATS)
@pytest.mark.parametrize("m,top_k", [(1, 2), (5, 2), (200, 1)])
def test_general_banks_plan_on_the_routed_stripe_stream(bits, group, st, asym, m, top_k):
    with pytest.raises(RuntimeError):  # without the flag the bank does not exist
        bestla.ExpertBank.plan_only([(bits, FMID, FIN, group, st, asym)] * NE)
    gate, up, down = _ffn(bits, group, st, asym)
    assert (gate.route, gate.bits, gate.has_weights, gate.asym) == (1, bits, 0, int(asym))
    plan = bestla.plan_moe(gate, up, down, m, top_k)
    assert [p["kernel"] for p in plan] == [GENERAL, GENERAL, "moe_combine_kernel"]
    nprob = m * top_k
    for p, n, k, dual in ((plan[0], FMID, FIN, True), (plan[1], FOUT, FMID, False)):
        units = -(-n // 16)
        assert p["threads"] == 64 * waves_of(bits, k, group), p
        assert p["grid"] % nprob == 0 and 0 < p["lds"] <= 160 * 1024, p
        wpp = p["grid"] // nprob
        assert wpp == max(1, min(units, CUS // nprob)), p  # these shapes fit LDS at the first count
        assert p["lds"] == lds_of(bits, k, group, units, wpp, dual), p


def test_long_k_lds_forces_more_workgroups_per_problem():
    """300 problems on 256 CUs start at one workgroup each; K = 14336 stages 84 KiB of activation rows, and the 256
    stripes of N = 4096 at 7 waves need 112 KiB of partial sums: two workgroups per problem fit"""
    gate = general((4, 14336, 256, 32, "fp32", False))
    down = general((4, 4096, 14336, 32, "fp32", False))
    plan = bestla.plan_moe(gate, gate, down, 300, 1)
    assert plan[1]["kernel"] == GENERAL and plan[1]["threads"] == 64 * 7
    assert lds_of(4, 14336, 32, 256, 1, False) > 160 * 1024 >= lds_of(4, 14336, 32, 256, 2, False)
    assert plan[1]["grid"] == 2 * 300 and plan[1]["lds"] == lds_of(4, 14336, 32, 256, 2, False)
    assert plan[0]["grid"] == 300 and plan[0]["lds"] == lds_of(4, 256, 32, 896, 1, True) <= 160 * 1024


@pytest.mark.parametrize("m,top_k", [(1, 2), (5, 2), (200, 1)])
def test_a_lean_geometry_plans_the_same_under_either_entry(m, top_k):
    geoms = [[(4, FMID, FIN) + G128] * NE, [(4, FMID, FIN) + G128] * NE, [(4, FOUT, FMID) + G128] * NE]
    lean = [bestla.ExpertBank.plan_only(g) for g in geoms]
    gen = [bestla.ExpertBank.plan_only(g, general=True) for g in geoms]
    assert [b.route for b in gen] == [0, 0, 0]
    assert bestla.plan_moe(*gen, m, top_k) == bestla.plan_moe(*lean, m, top_k)
    assert bestla.plan_moe(gen[0], lean[1], gen[2], m, top_k) == bestla.plan_moe(*lean, m, top_k)
    assert bestla.plan_moe_grouped(*gen, 70, 2) == bestla.plan_moe_grouped(*lean, 70, 2)
    int2 = [(2, FMID, FIN, 64, "fp16", False)] * NE
    assert bestla.ExpertBank.plan_only(int2, general=True).route == 0


def test_a_mixed_ffn_plans():
    """Q4_0's layout (int4 g32, fp16 scales) for gate / up, int4 g128 for down -- and the other way round"""
    q40 = general((4, FMID, FIN, 32, "fp16", False))
    down = general((4, FOUT, FMID) + G128)
    assert (q40.route, down.route) == (1, 0)
    plan = bestla.plan_moe(q40, q40, down, 3, 2)
    assert [p["kernel"] for p in plan] == [GENERAL, LEAN, "moe_combine_kernel"]
    lean_down = bestla.ExpertBank.plan_only([(4, FOUT, FMID) + G128] * NE)
    assert bestla.plan_moe(q40, q40, lean_down, 3, 2) == plan
    gate = general((4, FMID, FIN) + G128)
    q80_down = general((8, FOUT, FMID, 32, "fp16", False))
    plan = bestla.plan_moe(gate, gate, q80_down, 3, 2)
    assert [p["kernel"] for p in plan] == [LEAN, GENERAL, "moe_combine_kernel"]
    with pytest.raises(RuntimeError, match=r"gate and up banks differ in group size \(32 vs 128\)"):
        bestla.plan_moe(q40, gate, down, 3, 2)


def test_refusals_by_name_under_general():
    ok = (4, FMID, FIN, 32, "fp16", False)
    with pytest.raises(RuntimeError, match="int4 groups of 32 with zero points run on the skinny kernel"):
        general((4, FMID, FIN, 32, "fp16", True))
    with pytest.raises(RuntimeError, match="expert 1's weight is GGUF Q6_K"):
        bestla.ExpertBank.plan_only([ok, (6, FMID, FIN, 16, "fp16", False)], general=True)
    with pytest.raises(RuntimeError, match="expert 2's weight differs in shape or format from expert 0's"):
        bestla.ExpertBank.plan_only([ok, ok, (8, FMID, FIN, 32, "fp16", False), ok], general=True)
    with pytest.raises(RuntimeError, match="expert 1's weight differs in shape or format from expert 0's"):
        bestla.ExpertBank.plan_only([ok, (4, FMID, FIN, 32, "fp32", False)], general=True)
    with pytest.raises(RuntimeError, match=r"need 1\.\.256 experts"):
        bestla.ExpertBank.plan_only([ok] * 257, general=True)
    # int8 groups that tile neither a 64-deep K tile nor whole tiles: neither stream takes them
    with pytest.raises(RuntimeError, match="takes neither the M = 1 GEMV nor the routed stripe stream"):
        general((8, FMID, FIN, 192, "fp16", False))
    # a plan-only bank of either kind launches nothing
    bank = general(ok)
    x = np.zeros((1, FIN), np.float32)
    ids = np.zeros((1, 2), np.int32)
    out = np.zeros((1, FMID), np.float32)
    vp = bestla._ptr
    rc = lib().nad_device_mul_mat_id(bank.handle, vp(x), vp(ids), 2, 0, vp(out), 1, FIN, FMID, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()


def _r256(v):
    return -(-v // 256) * 256


@pytest.mark.parametrize("bits,group,asym", [(4, 32, False), (8, 32, False), (8, 32, True), (8, 128, True)])
@pytest.mark.parametrize("m,top_k", [(5, 2), (70, 2), (200, 1)])
def test_grouped_plans_on_general_banks(knob, bits, group, asym, m, top_k):
    knob("NAD_GEMM7_BM", None)
    fin = 1000  # not a whole number of K tiles: x16 is padded
    banks = _ffn(bits, group, "fp16", asym, fin=fin)
    plan = bestla.plan_moe_grouped(*banks, m, top_k)
    ls = plan["launches"]
    assert [p["kernel"] for p in ls] == FFN_KERNELS
    np_ = m * top_k
    assert plan["bm"] in HEIGHTS and plan["bound"] == bound(np_, NE, plan["bm"]), plan
    if np_ <= 32 * NE:
        assert plan["bm"] == 32
    for p, n in ((ls[2], FMID), (ls[3], FMID), (ls[4], FOUT)):
        assert p["grid"] == plan["bound"] * -(-n // 128) and p["threads"] == 512 and 0 < p["lds"] <= 160 * 1024, p
    kp = -(-fin // ktile(bits)) * ktile(bits)  # int8: a 64-deep K tile
    head = (_r256((NE + 1) * 4) + 3 * _r256(np_ * 4) + _r256(16 + 16 * (np_ // 32 + min(NE, np_))) + _r256(m * kp * 2))
    assert bestla.moe_grouped_workspace_size(*banks, m, top_k) == head + 2 * _r256(np_ * FMID * 2) + _r256(np_ * FOUT * 4)
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        p2 = bestla.plan_moe_grouped(*banks, m, top_k)
        assert p2["bm"] == bm and p2["bound"] == bound(np_, NE, bm)


def test_grouped_refusals_on_general_banks():
    # one group per channel over K = 1000 is no 64 * 2^j: the bank exists (the stripe stream takes it), gemm7 does not
    pc = general((8, FMID, 1000, -1, "fp16", False))
    assert pc.route == 1
    with pytest.raises(RuntimeError, match=r"the given bank \(int8, groups of 1000\) does not take the grouped gemm7: it "
                                           r"needs int4 groups of 32, 64 or 128 \* 2\^j, or int2 / int8 groups of 32"):
        bestla.plan_moe_grouped(pc, None, None, 40, 1)
    # fmid = 96 is 1.5 of an int8 down bank's 64-deep K tiles
    g, u, d = _ffn(8, 32, "fp16", False, fmid=96)
    with pytest.raises(RuntimeError, match=r"fmid \(96\) is not a whole number of the down bank's K tiles \(64 deep\)"):
        bestla.plan_moe_grouped(g, u, d, 40, 2)
