"""Routed expert matmuls (nad_expert_bank_*, nad_plan_moe, nad_moe_workspace_size), the host side: no GPU needed.

Geometry-only banks (nad_expert_bank_plan_only) go through the same checks as banks of loaded weights and serve the
dry run.  combine_f32 below is the numpy float32 restatement of launch 3 of nad_device_moe_ffn; the GPU tests import
it.
"""
import numpy as np
import pytest

from neural_amd import bestla
from neural_amd._lib import lib

FIN, FMID, FOUT, NE = 1024, 512, 300, 4
G128 = (128, "fp16", False)


def combine_f32(y, wts, top_k):
    """out[r][n] = ((w[r][0] * y[r * top_k][n]) + w[r][1] * y[r * top_k + 1][n]) + ...: every product and every sum
    rounded to float32 on its own, in slot order.  y [m * top_k][n] and wts [m][top_k] float32."""
    y = np.asarray(y, dtype=np.float32)
    wts = np.asarray(wts, dtype=np.float32)
    m = wts.shape[0]
    yy = y.reshape(m, top_k, y.shape[1])
    out = (wts[:, 0:1] * yy[:, 0, :]).astype(np.float32)
    for i in range(1, top_k):
        out = (out + (wts[:, i:i + 1] * yy[:, i, :]).astype(np.float32)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def _banks(bits=4, group=G128):
    gate = bestla.ExpertBank.plan_only([(bits, FMID, FIN) + group] * NE)
    up = bestla.ExpertBank.plan_only([(bits, FMID, FIN) + group] * NE)
    down = bestla.ExpertBank.plan_only([(4, FOUT, FMID) + G128] * NE)
    return gate, up, down


@pytest.mark.parametrize("m,top_k", [(1, 2), (5, 2), (200, 1)])
def test_plan_moe_launches_and_grids(m, top_k):
    gate, up, down = _banks()
    assert (gate.n_expert, gate.n, gate.k, gate.has_weights) == (NE, FMID, FIN, 0)
    plan = bestla.plan_moe(gate, up, down, m, top_k)
    assert len(plan) == 3
    assert [p["kernel"] for p in plan] == ["woq_gemv_m1_routed_kernel", "woq_gemv_m1_routed_kernel",
                                           "moe_combine_kernel"]
    nprob = m * top_k
    # workgroups per problem as nad_batch_create deals them: the CUs over the problems, at most one per unit (a stripe;
    # for gate + up a stripe pair), at least one.  256 CUs without a device (and on the MI355X).
    cus = 256
    for p, units in ((plan[0], FMID // 16), (plan[1], -(-FOUT // 16))):
        wpp = max(1, min(units, cus // nprob))
        assert p["grid"] == nprob * wpp, (p, wpp)
        assert p["threads"] % 64 == 0 and 0 < p["lds"] <= 160 * 1024
    if nprob > cus // 2:  # more problems than half the CUs: one workgroup each
        assert plan[0]["grid"] == nprob and plan[1]["grid"] == nprob
    assert plan[2]["threads"] == 256 and plan[2]["grid"] == m * -(-FOUT // 256)


def test_plan_moe_int2_policy():
    """int2 g64 gate / up with an int4 down (llama_utils.cpp:269-287): the down bank may differ in format"""
    gate, up, down = _banks(bits=2, group=(64, "fp16", False))
    plan = bestla.plan_moe(gate, up, down, 2, 2)
    assert [p["kernel"] for p in plan[:2]] == ["woq_gemv_m1_routed_kernel"] * 2


def test_bank_errors_name_the_expert():
    ok = (4, FMID, FIN) + G128
    with pytest.raises(RuntimeError, match="expert 2's weight differs in shape or format from expert 0's"):
        bestla.ExpertBank.plan_only([ok, ok, (4, FMID // 2, FIN) + G128, ok])
    with pytest.raises(RuntimeError, match="expert 1's weight is GGUF Q6_K"):
        bestla.ExpertBank.plan_only([ok, (6, FMID, FIN, 16, "fp16", False)])
    with pytest.raises(RuntimeError, match="expert 0's weight is not in the int4 / int2 tile layout"):
        bestla.ExpertBank.plan_only([(8, FMID, FIN) + G128])
    with pytest.raises(RuntimeError, match="expert 0's weight geometry .* does not take the M = 1 GEMV"):
        bestla.ExpertBank.plan_only([(4, FMID, FIN, 32, "fp16", False)])  # 4 groups per K tile
    with pytest.raises(RuntimeError, match=r"need 1\.\.256 experts"):
        bestla.ExpertBank.plan_only([ok] * 257)


def test_bank_create_names_the_expert_whose_descriptor_is_not_a_weight():
    import ctypes as C

    L = lib()
    desc = (C.c_uint8 * L.bestla_device_storage_size())()  # zeros: no magic
    arr = (C.c_void_p * 1)(C.cast(desc, C.c_void_p))
    assert not L.nad_expert_bank_create(arr, 1)
    assert "expert 0's descriptor is not a loaded neural_amd device weight" in bestla.last_error()


def test_gate_and_up_must_share_the_group_size():
    gate, _, down = _banks()
    up64 = bestla.ExpertBank.plan_only([(4, FMID, FIN, 64, "fp16", False)] * NE)
    with pytest.raises(RuntimeError, match=r"gate and up banks differ in group size \(128 vs 64\)"):
        bestla.plan_moe(gate, up64, down, 1, 2)
    wrong_k = bestla.ExpertBank.plan_only([(4, FOUT, FMID * 2) + G128] * NE)
    with pytest.raises(RuntimeError, match="down bank's K"):
        bestla.plan_moe(gate, gate, wrong_k, 1, 2)


def test_plan_only_bank_does_not_launch():
    gate, up, down = _banks()
    x = np.zeros((1, FIN), np.float32)
    ids = np.zeros((1, 2), np.int32)
    out = np.zeros((1, FMID), np.float32)
    vp = bestla._ptr
    rc = lib().nad_device_mul_mat_id(gate.handle, vp(x), vp(ids), 2, 0, vp(out), 1, FIN, FMID, None)
    assert rc == -1 and "holds no weights" in bestla.last_error()
    # misaligned rows: refused before anything else is looked at
    rc = lib().nad_device_mul_mat_id(gate.handle, vp(x), vp(ids), 2, 0, vp(out), 1, FIN + 2, FMID, None)
    assert rc == -1 and "lda % 4 == 0" in bestla.last_error()


@pytest.mark.parametrize("m,top_k", [(1, 2), (5, 2), (7, 3)])
def test_workspace_size(m, top_k):
    def r256(v):
        return -(-v // 256) * 256

    p = m * top_k
    size = lib().nad_moe_workspace_size(m, top_k, FMID, FOUT)
    # the header: round256(m * top_k * fmid * 4) + round256(m * top_k * fout * 4)
    assert size == r256(p * FMID * 4) + r256(p * FOUT * 4)
    assert p * (FMID + FOUT) * 4 <= size < p * (FMID + FOUT) * 4 + 512


def test_combine_restatement_is_separate_float32_ops():
    rng = np.random.default_rng(0)
    y = rng.uniform(-1, 1, size=(6, 33)).astype(np.float32)
    w = rng.uniform(0, 1, size=(3, 2)).astype(np.float32)
    out = combine_f32(y, w, 2)
    for r in range(3):
        for n in range(33):
            a = np.float32(w[r, 0] * y[2 * r, n])
            b = np.float32(w[r, 1] * y[2 * r + 1, n])
            assert out[r, n] == np.float32(a + b)
