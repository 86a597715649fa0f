"""Every woq_gemm7_kernel instantiation against the exact fp16 fold model (tests/fold_model.py).

launch_gemm7_b{4,2,8} dispatches over bits x groups per B buffer x scale type x asym x tile height: 72 + 48 + 48 = 168
kernels, and 18 more in the fused-QKV form.  Here each is run by name -- NAD_GEMM7_BM forces the tile height, and the
plan's grid (row tiles x column tiles x K runs) proves which one ran -- on weights whose codes, scales and zero points
span their whole ranges, so a scale or zero point read from the neighbouring group, stripe or column is an error of
order one, and is held to TOL["fp16"] = 2e-5 of max|ref|: the kernel's fp16 weights are modelled bit for bit on the
host, so what is left is fp32 MFMA accumulation (measured 4e-7 to 8e-7 in float32 numpy, test_fold_model_cpu).

Geometry: M = 130 (5 / 3 / 2 / 1 row tiles at 32 / 64 / 128 / 256 rows, the last holding 2 rows, or 130 of 256),
N = 203 (two column tiles, the second with a partial stripe, N % 4 = 3).  Whole K: K = 300 with split K off (a tail
inside a 32-deep step, a group and a K tile; five int8 tiles, so the odd half step's padding runs).  Split K: seven K
tiles of the format, which splitk_plan cuts into runs of 3, 3, 1 tiles (4, 3 where a group is two tiles).

Each case prints one line per instantiation; profiles/gemm7_matrix_errors.txt keeps them.
"""
import numpy as np
import pytest

from tests import edges
from tests import fold_model as fm
from tests.conftest import gpu_available
from tests.fold_model import BF16, F16, F32, S2, S4, S8
from tests.test_forward_edges_gpu import _qkv_windows
from tests.test_gemm2_gpu import TOL

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

M, N = 130, 203
HEIGHTS = (32, 64, 128, 256)
BAR = TOL["fp16"]
FORMATS = [(S4, 32), (S4, 64), (S4, 128), (S4, 256), (S2, 32), (S2, 64), (S2, 128), (S8, 32), (S8, 64), (S8, 128)]
ST_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
K_TILE = {S4: 128, S2: 256, S8: 64}
WHOLE_K = 300


def variant_k(qt, variant):
    return WHOLE_K if variant == "whole" else 7 * K_TILE[qt]


def expected_ksplit(qt, bs, variant):
    """splitk_plan on 7 K tiles and at most 10 output tiles: runs of at least two tiles and of whole groups"""
    if variant == "whole":
        return 1
    return 2 if bs == 2 * K_TILE[qt] else 3


def inst(qt, bs, st, asym, bm, mw=False):
    """the template arguments launch_gemm7_b* resolves this launch to"""
    bits = fm.BITS[qt]
    gpt = {32: 4, 64: 2}.get(bs, 1) if bits == 4 else (2 if bs == 32 else 1)
    return (f"woq_gemm7_kernel<int{bits}, {bm} rows, {'asym' if asym else 'sym'}, {ST_NAME[st]}, gpt {gpt}"
            f"{', MW' if mw else ''}> g{bs}")


_MADE = {}


def weight(oracle, n, k, bs, qt, st, asym):
    """-> (the model's fp16 weights [k][n], the loaded DeviceWeight); each weight is made once and shared"""
    key = (n, k, bs, qt, st, asym)
    if key not in _MADE:
        seed = n * 7 + k * 3 + bs + fm.BITS[qt] * 1000 + (st % 97) * 11 + int(asym)
        blob, (Q, S, Z) = fm.make(oracle, n, k, bs, qt, st, asym, seed)
        w = bestla.DeviceWeight(blob)
        assert w.fold_ok == 1, "the scale range must leave every q * s an fp16 normal"
        _MADE[key] = (fm.folded_weights(Q, S, Z, bs), w)
    return _MADE[key]


def activations(m, k, act="fp16", seed=0):
    """-> (contiguous cuda tensor of the activation type, the fp16 values the kernel multiplies, as fp32 numpy)"""
    A = np.random.default_rng(m * 7 + k + seed).uniform(-0.5, 0.5, size=(m, k)).astype(np.float32)
    xt = torch.from_numpy(A).cuda().to(edges.torch_dtype(act))
    return xt, xt.half().float().cpu().numpy()  # torch's rounding to fp16 is the model of nad_cvt_act_kernel's


def check_plan(w, qt, bs, variant, bm, n=N):
    plan = w.plan(M, "fp16")
    ks = expected_ksplit(qt, bs, variant)
    assert plan["kernel"] == "woq_gemm7_kernel" and plan["fold"], plan
    assert plan["ksplit"] == ks, (plan, ks)
    assert plan["grid"] == -(-M // bm) * -(-n // 128) * ks, (plan, bm)
    return plan


def set_variant(knob, variant):
    knob("NAD_MID_MAX_M", 0)
    knob("NAD_SPLITK_DISABLE", 1 if variant == "whole" else None)


CASES = [(qt, bs, st, asym, variant) for qt, bs in FORMATS for st in (F32, BF16, F16) for asym in (False, True)
         for variant in ("whole", "splitk")]


def _id(c):
    qt, bs, st, asym, variant = c
    return f"int{fm.BITS[qt]}_g{bs}_{ST_NAME[st]}_{'asym' if asym else 'sym'}_{variant}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gemm7_instantiation(oracle, knob, case):
    qt, bs, st, asym, variant = case
    k = variant_k(qt, variant)
    w16, w = weight(oracle, N, k, bs, qt, st, asym)
    set_variant(knob, variant)
    xt, xv = activations(M, k)
    prod = fm.model_product(xv, w16)
    x = edges.act_window(xt, "aligned")
    ys = []
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        plan = check_plan(w, qt, bs, variant, bm)
        can, out = edges.out_window(M, N, "aligned")
        what = f"{inst(qt, bs, st, asym, bm)} {variant} K={k} grid={plan['grid']} ksplit={plan['ksplit']}"
        (y,) = edges.twice(can, lambda: w.forward(x, out=out), what)
        err = edges.rel_err(y, prod, prod)
        print(f"{what}: err {err:.3e} bound {BAR:.1e}")
        assert err <= BAR, (what, err)
        ys.append(y)
    same = all(np.array_equal(ys[0].view(np.uint32), y.view(np.uint32)) for y in ys[1:])
    print(f"{_id(case)}: the four tile heights' results are bit-identical: {same}")  # recorded, not asserted


# int4 g128 F16 sym and int8 g32 F32 asym: other activation types, unaligned rows, every epilogue
WIDE = [(S4, 128, F16, False), (S8, 32, F32, True)]
WIDE_CASES = [(qt, bs, st, asym, variant, bm) for qt, bs, st, asym in WIDE for variant in ("whole", "splitk")
              for bm in HEIGHTS]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: f"{_id(c[:5])}_bm{c[5]}")
def test_gemm7_activation_types_alignments_epilogues(oracle, knob, case):
    qt, bs, st, asym, variant, bm = case
    k = variant_k(qt, variant)
    w16, w = weight(oracle, N, k, bs, qt, st, asym)
    set_variant(knob, variant)
    knob("NAD_GEMM7_BM", bm)
    check_plan(w, qt, bs, variant, bm)
    label = f"{inst(qt, bs, st, asym, bm)} {variant} K={k}"
    for act in ("fp32", "bf16"):  # rounded to fp16 once by nad_cvt_act_kernel: torch's .half() is the model
        xt, xv = activations(M, k, act, seed=1)
        prod = fm.model_product(xv, w16)
        plan = w.plan(M, act)
        assert plan["kernel"] == "woq_gemm7_kernel" and plan["ksplit"] == expected_ksplit(qt, bs, variant), plan
        can, out = edges.out_window(M, N, "aligned")
        x = edges.act_window(xt, "aligned")
        (y,) = edges.twice(can, lambda: w.forward(x, out=out), f"{label} {act}")
        err = edges.rel_err(y, prod, prod)
        print(f"{label} {act}: err {err:.3e} bound {BAR:.1e}")
        assert err <= BAR, (label, act, err)
    xt, xv = activations(M, k)
    edges.check_forward_matrix(w, xt, fm.model_product(xv, w16), BAR, f"{label} fp16")


@pytest.mark.parametrize("bm", HEIGHTS)
def test_gemm7_xcd_placement(oracle, knob, bm):
    """Split K with every run of a tile on one XCD (GemmArgs::xcd_tile: the tile count a multiple of 8, here 8 column
    tiles): the model bar, and bit for bit the results of the plain placement (NAD_GEMM_XCD=0)."""
    qt, bs, st, asym, n, k = S4, 128, F16, False, 1000, 896
    w16, w = weight(oracle, n, k, bs, qt, st, asym)
    knob("NAD_MID_MAX_M", 0)
    knob("NAD_GEMM7_BM", bm)
    plan = check_plan(w, qt, bs, "splitk", bm, n=n)
    assert plan["ksplit"] > 1 and (plan["grid"] // plan["ksplit"]) % 8 == 0, plan
    xt, xv = activations(M, k, seed=2)
    prod = fm.model_product(xv, w16)
    x = edges.act_window(xt, "aligned")
    ys = []
    for xcd in (None, 0):
        knob("NAD_GEMM_XCD", xcd)
        assert w.plan(M, "fp16") == plan
        can, out = edges.out_window(M, n, "aligned")
        what = f"{inst(qt, bs, st, asym, bm)} N={n} K={k} xcd={'on' if xcd is None else 'off'}"
        (y,) = edges.twice(can, lambda: w.forward(x, out=out), what)
        err = edges.rel_err(y, prod, prod)
        print(f"{what}: err {err:.3e} bound {BAR:.1e}")
        assert err <= BAR, (what, err)
        ys.append(y)
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ fused QKV (MW)
QKV_NS = (203, 75, 40)  # column tiles 2 + 1 + 1: both nbn_cut boundaries
QKV_CASES = [(128, 300, st, asym) for st in (F32, BF16, F16) for asym in (False, True)] + \
            [(256, 640, F16, False), (256, 640, F16, True)]


@pytest.mark.parametrize("case", QKV_CASES,
                         ids=lambda c: f"int4_g{c[0]}_K{c[1]}_{ST_NAME[c[2]]}_{'asym' if c[3] else 'sym'}")
def test_gemm7_fused_qkv_instantiation(oracle, knob, case):
    """The 18 MW kernels (int4, one group per K tile or more, 64 / 128 / 256 rows): plan_qkv shows ONE gemm7 main launch
    over the four column tiles of the three weights; each output at the model bar and bit for bit the separate
    launches' (NAD_GEMM7_FUSE=0).  At 32 rows there is no fused kernel: the plan shows the separate launches."""
    bs, k, st, asym = case
    made = [weight(oracle, n, k, bs, S4, st, asym) for n in QKV_NS]
    ws = [w for _, w in made]
    knob("NAD_MID_MAX_M", 0)
    knob("NAD_SPLITK_DISABLE", 1)
    xt, xv = activations(M, k, seed=3)
    prods = [fm.model_product(xv, w16) for w16, _ in made]
    x = edges.act_window(xt, "aligned")
    for bm in HEIGHTS:
        knob("NAD_GEMM7_BM", bm)
        rt = -(-M // bm)
        results = {}
        for fuse in (None, 0):
            knob("NAD_GEMM7_FUSE", fuse)
            plan = bestla.plan_qkv(*ws, M, "fp16")
            assert plan["kernel"] == "woq_gemm7_kernel" and plan["fold"] and plan["ksplit"] == 1, plan
            fused = fuse is None and bm != 32
            # fused: the one main launch covers 2 + 1 + 1 column tiles; separate: the last is the 40-column weight's
            assert plan["grid"] == rt * (4 if fused else 1), (bm, fuse, plan)
            results[fuse] = plan
            can, wins = _qkv_windows(M, QKV_NS)
            what = f"{inst(S4, bs, st, asym, bm, mw=fused)} qkv K={k} grid={plan['grid']} launches={plan['launches']}"
            ys = edges.twice(can, lambda: bestla.qkv_forward(x, *ws, out=wins), what)
            for i, (y, prod) in enumerate(zip(ys, prods)):
                err = edges.rel_err(y, prod, prod)
                print(f"{what} output {i}: err {err:.3e} bound {BAR:.1e}")
                assert err <= BAR, (what, i, err)
            results[fuse, "y"] = ys
        pre = results[0]["launches"] - 3  # the activation conversion, where the rows are not a whole fp16 K tile copy
        assert pre in (0, 1), results[0]
        assert results[None]["launches"] == pre + (3 if bm == 32 else 1), (bm, results[None], results[0])
        for a, b in zip(results[None, "y"], results[0, "y"]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
