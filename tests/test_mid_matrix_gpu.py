"""Every reachable woq_mid_kernel instantiation against the exact hi / lo model (tests/mid_model.py).

launch_gemm_mid -> mid_at -> mid_rf -> mid_try resolves a launch over bits x groups per K tile x sym / asym x activation
type x (row fragments RF, stripes S, waves NW, stages SPW) x fp32 / 16-bit scales (bf16 or fp16 at run time).  Here
each reachable one is run by name -- M sets RF, NAD_MID_WIDE the stripes, and the plan's threads (NW x 64) and grid
(stripe groups x K runs) prove which one ran -- on weights whose codes, scales and zero points span their whole ranges
(fold_model.make), so a scale or zero point read from the neighbouring group, stripe or column is an error of order
one, and is held to 2e-5 of max|model| (test_mid_gpu TOL): the operands are modelled exactly, what is left is fp32
accumulation (measured in float32 numpy by test_mid_model_cpu).

Shapes: N = 203 (13 stripes: four 4-stripe groups, the last one stripe of 11 columns; two 8-stripe groups, the last
of 5), M = 13 / 29 / 45 / 61 (RF = 1 .. 4, the last fragment ragged), K = 9 K tiles + 40 (10 tiles; the tail ends
inside a 32-deep step, a group and a tile).  Two K variants on the same weight: "one" (NAD_MID_KS=1: the chunk loop
runs twice at 8-tile chunks, three times at 4-tile ones, the second stage live in the first chunk and dead in the
second) and "runs" (NAD_MID_KS=3: runs of 4, 4, 2 tiles, slabs and launch_splitk_reduce).

The 60 reachable (bits, gpt, activation type, RF, S, NW, SPW), from mid_geometry and run_mid's gates (GEOMETRY below):

  int4 gpt 1: RF 1, 2, 3 (4, 8, 1) every type; RF 4 (4, 8, 1) fp16 rows, (4, 4, 2) fp32 / bf16 rows;
              8-stripe RF 1, 2 (8, 8, 1) every type                                                     -> 18
  int4 gpt 2: RF 1, 2 (4, 8, 1); RF 3, 4 (4, 4, 1); 8-stripe RF 1 (8, 8, 1), RF 2 (8, 4, 1); every type -> 18
  int4 gpt 4: RF 1, 2 (4, 4, 2) every type (M <= 32)                                                    ->  6
  int2 gpt 1, 2, 4: RF 1, 2 (4, 4, 1) every type (M <= 32)                                              -> 18

times sym / asym and fp32 / 16-bit scales: 240 kernels, 360 launches with bf16 and fp16 scales apart.

The compiled set equals this reachable set: mid_rf instantiates the shapes mid_geometry's rule (mid_shape) can return
and no others, and tests/test_mid_instances_cpu.py holds the built library's woq_mid_kernel symbols to these 240.

Each launch prints one line; profiles/mid_matrix_errors.txt keeps them.
"""
import numpy as np
import pytest

from tests import edges
from tests import fold_model as fm
from tests import mid_model as mm
from tests.conftest import gpu_available
from tests.fold_model import BF16, F16, F32, S2, S4
from tests.test_mid_gpu import TOL

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

N = 203
NS = 13                                 # stripes of 16 columns
M_OF_RF = {1: 13, 2: 29, 3: 45, 4: 61}  # the last row fragment ragged each time
M_MAX = 61
K_TILE = {S4: 128, S2: 256}
BAR = TOL["fp32"]
assert BAR == TOL["fp16"] == TOL["bf16"] == 2e-5
ACTS = ("fp32", "fp16", "bf16")
ST_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
VARIANTS = {"one": 1, "runs": 3}        # NAD_MID_KS
# one group size per (bits, groups per K tile)
FORMATS = [(S4, 32), (S4, 64), (S4, 128), (S2, 64), (S2, 128), (S2, 256)]

# Transcribed from mid_shape (woq_gemm_mid.hip: mid_geometry and mid_rf both come from it) and run_mid's M gates -- not
# computed by the library: a change to the geometry is a conscious edit here.
# (bits, gpt, activation types, NAD_MID_WIDE, RFs, S, NW, SPW)
GEOMETRY = [
    (4, 1, ACTS,             0, (1, 2, 3), 4, 8, 1),
    (4, 1, ("fp16",),        0, (4,),      4, 8, 1),
    (4, 1, ("fp32", "bf16"), 0, (4,),      4, 4, 2),
    (4, 1, ACTS,             1, (1, 2),    8, 8, 1),
    (4, 2, ACTS,             0, (1, 2),    4, 8, 1),
    (4, 2, ACTS,             0, (3, 4),    4, 4, 1),
    (4, 2, ACTS,             1, (1,),      8, 8, 1),
    (4, 2, ACTS,             1, (2,),      8, 4, 1),
    (4, 4, ACTS,             0, (1, 2),    4, 4, 2),
    (2, 1, ACTS,             0, (1, 2),    4, 4, 1),
    (2, 2, ACTS,             0, (1, 2),    4, 4, 1),
    (2, 4, ACTS,             0, (1, 2),    4, 4, 1),
]


def variant_k(qt):
    return 9 * K_TILE[qt] + 40  # 1192 / 2344: K % 8 == 0 as run_mid requires


def gpt_of(qt, bs):
    return max(1, K_TILE[qt] // bs)


def geometries(qt, bs, act):
    """-> [(wide, rf, s, nw, spw)] this format and activation type reaches"""
    bits, gpt = fm.BITS[qt], gpt_of(qt, bs)
    return [(wide, rf, s, nw, spw) for b, g, acts, wide, rfs, s, nw, spw in GEOMETRY if (b, g) == (bits, gpt)
            and act in acts for rf in rfs]


TUPLES = {(fm.BITS[qt], gpt_of(qt, bs), act, rf, s, nw, spw) for qt, bs in FORMATS for act in ACTS
          for _, rf, s, nw, spw in geometries(qt, bs, act)}
assert len(TUPLES) == 60, len(TUPLES)
assert len({(fm.BITS[qt], gpt_of(qt, bs)) for qt, bs in FORMATS}) == len(FORMATS)


def inst(qt, bs, st, asym, act, rf, s, nw, spw):
    """the template arguments launch_gemm_mid resolves this launch to"""
    return (f"woq_mid_kernel<int{fm.BITS[qt]}, gpt {gpt_of(qt, bs)}, {'asym' if asym else 'sym'}, {act} rows, RF {rf}, "
            f"S {s}, NW {nw}, SPW {spw}, {ST_NAME[st]}> g{bs}")


_MADE = {}
_PROD = {}
RAN = set()  # (the 7-tuple, asym, scale type, variant) of every matrix launch that passed


def weight(oracle, n, k, bs, qt, st, asym):
    """-> (key, (Q, S, Z), the loaded DeviceWeight); each weight is made once and shared"""
    key = (n, k, bs, qt, st, asym)
    if key not in _MADE:
        seed = n * 7 + k * 3 + bs + fm.BITS[qt] * 1000 + (st % 97) * 11 + int(asym)
        blob, fields = fm.make(oracle, n, k, bs, qt, st, asym, seed)
        _MADE[key] = (fields, bestla.DeviceWeight(blob))
    return (key,) + _MADE[key]


def act_values(k, act):
    """the M_MAX rows every launch of this K and type takes its first M of: fp32 numpy holding the type's values"""
    A = np.random.default_rng(k * 3 + ACTS.index(act)).uniform(-0.5, 0.5, size=(M_MAX, k)).astype(np.float32)
    return mm.round_act(A, act)


def model(key, fields, bs, act):
    """-> (activation values [M_MAX][K], the model's float64 product of them [M_MAX][N]), computed once per weight and
    activation type and never written to"""
    if (key, act) not in _PROD:
        xv = act_values(key[1], act)
        prod = mm.product(mm.split_hi_lo(xv), *fields, bs)
        xv.setflags(write=False)
        prod.setflags(write=False)
        _PROD[key, act] = (xv, prod)
    return _PROD[key, act]


def upload(xv, m, act):
    xt = torch.from_numpy(np.array(xv[:m])).cuda().to(edges.torch_dtype(act))
    assert np.array_equal(xt.float().cpu().numpy(), xv[:m])  # the type holds the model's values bit for bit
    return xt


def check_plan(w, m, act, s, nw, ks, ns=NS):
    plan = w.plan(m, act)
    assert plan["kernel"] == "woq_mid_kernel" and plan["fold"] == 0, plan
    assert plan["threads"] == nw * 64, (plan, nw)
    assert plan["grid"] == -(-ns // s) * ks, (plan, s, ks)
    assert plan["ksplit"] == ks, (plan, ks)
    assert plan["launches"] == (1 if ks == 1 else 2), plan
    return plan


def run_launch(w, xt, prod, what):
    """one forward into a canary-guarded window from NaN-padded rows, twice: -> (error against the model, result)"""
    m, n = prod.shape
    x = edges.act_window(xt, "aligned")
    can, out = edges.out_window(m, n, "aligned")
    (y,) = edges.twice(can, lambda: w.forward(x, out=out), what)
    return edges.rel_err(y, prod, prod), y


CASES = [(qt, bs, asym, st, act) for qt, bs in FORMATS for asym in (False, True) for st in (F32, BF16, F16)
         for act in ACTS]
assert len(CASES) == 108


def _id(c):
    qt, bs, asym, st, act = c
    return f"int{fm.BITS[qt]}_g{bs}_{'asym' if asym else 'sym'}_{ST_NAME[st]}_{act}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mid_instantiation(oracle, knob, case):
    qt, bs, asym, st, act = case
    k = variant_k(qt)
    key, fields, w = weight(oracle, N, k, bs, qt, st, asym)
    xv, prod = model(key, fields, bs, act)
    knob("NAD_MID_XCD", None)
    for wide, rf, s, nw, spw in geometries(qt, bs, act):
        m = M_OF_RF[rf]
        xt = upload(xv, m, act)
        knob("NAD_MID_WIDE", wide)
        for variant, ks in VARIANTS.items():
            knob("NAD_MID_KS", ks)
            plan = check_plan(w, m, act, s, nw, ks)
            what = f"{inst(qt, bs, st, asym, act, rf, s, nw, spw)} {variant} K={k} grid={plan['grid']}"
            err, _ = run_launch(w, xt, prod[:m], what)
            print(f"{what}: err {err:.3e} bound {BAR:.1e}")
            assert err <= BAR, (what, err)
            RAN.add(((fm.BITS[qt], gpt_of(qt, bs), act, rf, s, nw, spw), asym, st, variant))


def test_mid_matrix_is_complete():
    """Every one of the 60 geometry tuples x sym / asym x three scale types ran and passed in both K variants: 720
    launches, counted from what test_mid_instantiation recorded (so this test needs the whole file run, in order)."""
    want = {(t, asym, st, v) for t in TUPLES for asym in (False, True) for st in (F32, BF16, F16) for v in VARIANTS}
    assert len(want) == 720
    missing = sorted(want - RAN, key=str)
    print(f"mid-M matrix: {len(RAN & want)} of {len(want)} launches recorded, "
          f"{len({(t, a, s == F32) for t, a, s, _ in RAN})} of 240 kernels")
    assert not missing, (len(missing), missing[:4])
    assert RAN == want, sorted(RAN - want, key=str)[:4]


# ------------------------------------------------------------------------------------------- run-time forms of gpt 1
# groups of two K tiles (tpg_shift 1) and one group (bs = K, tpg_shift 31); asym, fp16 scales, RF 2
COARSE = [(S4, 256), (S2, 512), (S4, None), (S2, None)]


@pytest.mark.parametrize("qt,bs", COARSE, ids=[f"int{fm.BITS[q]}_{'per_channel' if b is None else f'g{b}'}"
                                               for q, b in COARSE])
def test_mid_groups_of_whole_tiles(oracle, knob, qt, bs):
    k = variant_k(qt)
    bs = bs or k
    assert gpt_of(qt, bs) == 1
    key, fields, w = weight(oracle, N, k, bs, qt, F16, True)
    assert fields[1].shape[0] == (-(-k // bs)) and fields[1].shape[0] in (1, 5)
    rf, s, nw, spw = (2, 4, 8, 1) if qt == S4 else (2, 4, 4, 1)
    m = M_OF_RF[rf]
    knob("NAD_MID_WIDE", 0)
    for act in ACTS:
        xv, prod = model(key, fields, bs, act)
        xt = upload(xv, m, act)
        for variant, ks in VARIANTS.items():
            knob("NAD_MID_KS", ks)
            plan = check_plan(w, m, act, s, nw, ks)
            what = f"{inst(qt, bs, F16, True, act, rf, s, nw, spw)} {variant} K={k} grid={plan['grid']}"
            err, _ = run_launch(w, xt, prod[:m], what)
            print(f"{what}: err {err:.3e} bound {BAR:.1e}")
            assert err <= BAR, (what, err)


# ------------------------------------------------------------------------------- epilogues and the slab reduce
# (qt, bs, asym, scale type, activation type, NAD_MID_WIDE, (RF, S, NW, SPW), variant)
EPI_CASES = [
    (S4, 64, True, BF16, "fp16", 1, (2, 8, 4, 1), "runs"),   # 8-stripe workgroups through the reduce's epilogue
    (S2, 64, False, F32, "bf16", 0, (2, 4, 4, 1), "runs"),
    (S4, 128, True, F16, "fp32", 0, (4, 4, 4, 2), "one"),    # 4 waves x 2 stages, the kernel's own epilogue
]


@pytest.mark.parametrize("case", EPI_CASES, ids=lambda c: f"{_id(c[:5])}_rf{c[6][0]}_s{c[6][1]}_{c[7]}")
def test_mid_epilogues(oracle, knob, case):
    qt, bs, asym, st, act, wide, (rf, s, nw, spw), variant = case
    k = variant_k(qt)
    key, fields, w = weight(oracle, N, k, bs, qt, st, asym)
    xv, prod = model(key, fields, bs, act)
    m = M_OF_RF[rf]
    knob("NAD_MID_WIDE", wide)
    knob("NAD_MID_KS", VARIANTS[variant])
    check_plan(w, m, act, s, nw, VARIANTS[variant])
    label = f"{inst(qt, bs, st, asym, act, rf, s, nw, spw)} {variant} K={k}"
    edges.check_forward_matrix(w, upload(xv, m, act), prod[:m], BAR, label, aligns=("aligned",))


# ------------------------------------------------------------------------------------------------ XCD placement
@pytest.mark.parametrize("wide", [0, 1])
def test_mid_xcd_placement_both_branches(oracle, knob, wide):
    """N = 1099: 69 stripes, N % 4 = 3 -- 18 groups of 4 stripes (16 placed by rounds of 8, 2 left over) or 9 groups of
    8 (8 + 1), so the kernel's and the reduce's `bid < full` / else split takes both branches in one launch.  Each
    placement at the model bar, and NAD_MID_XCD=0 bit for bit the same result."""
    qt, bs, st, asym, act, n, rf = S4, 128, F16, False, "fp16", 1099, 2
    k, m, ks = variant_k(qt), M_OF_RF[rf], 3
    s = 8 if wide else 4
    assert -(-n // 16) == 69 and -(-69 // s) == (9 if wide else 18) and -(-69 // s) % 8 != 0
    key, fields, w = weight(oracle, n, k, bs, qt, st, asym)
    xv, prod = model(key, fields, bs, act)
    xt = upload(xv, m, act)
    knob("NAD_MID_WIDE", wide)
    knob("NAD_MID_KS", ks)
    ys = []
    for xcd in (None, 0):
        knob("NAD_MID_XCD", xcd)
        plan = check_plan(w, m, act, s, 8, ks, ns=69)
        what = (f"{inst(qt, bs, st, asym, act, rf, s, 8, 1)} N={n} K={k} grid={plan['grid']} "
                f"xcd={'on' if xcd is None else 'off'}")
        err, y = run_launch(w, xt, prod[:m], what)
        print(f"{what}: err {err:.3e} bound {BAR:.1e}")
        assert err <= BAR, (what, err)
        ys.append(y)
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ gate boundaries
@pytest.mark.parametrize("qt,bs", [(S2, 64), (S2, 128), (S2, 256), (S4, 32)],
                         ids=["int2_g64", "int2_g128", "int2_g256", "int4_g32"])
def test_mid_gates(oracle, knob, qt, bs):
    """int2 and int4 g32 take the mid-M kernel to M = 32 only (run_mid): planned at M = 29, another kernel at M = 45"""
    _, _, w = weight(oracle, N, variant_k(qt), bs, qt, F16, True)
    knob("NAD_MID_WIDE", 0)
    for act in ACTS:
        assert w.plan(M_OF_RF[2], act)["kernel"] == "woq_mid_kernel", (act, w.plan(M_OF_RF[2], act))
        assert w.plan(M_OF_RF[3], act)["kernel"] != "woq_mid_kernel", (act, w.plan(M_OF_RF[3], act))
