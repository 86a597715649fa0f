"""Every reachable decode GEMV instantiation, run by name against the exact hi / lo model (tests/mid_model.py).

woq_gemv.h is compiled into woq_gemv_kernel, woq_gemv_m1_kernel and woq_gemv_m1s_kernel 1169 times over bits x groups per K
tile x sym / asym x activation type x K-slice width and slices per wave x register stages x scale type x weight count
x reduce form x load-ahead order.  The dry run names the instantiation its launch statement selects (plan["instance"]);
here every launch first holds that name to a literal table -- transcribed from gemv_waves, gemv_lean_slices, lean_ok,
m1_nst, m1s_launch3, m1s_ahead_form and prepare_gemv, never computed by the library -- and then runs on weights whose
codes, scales and zero points span their whole ranges (fold_model.make), so a scale or zero point read from the
neighbouring group, tile, stripe or column is an error of order one.  stage_mac builds q - zp exactly in fp16, runs the
MFMA over the fp16 hi and lo activation rows, scales each group's fp32 partial and adds it to the stripe's fp32 sum:
mid_model.product to the letter, so the bar is the decode bar, 2e-5 of max|model| (test_gpu_parity TOL_DECODE,
test_mid_gpu TOL), with the output pre-filled with NaN.  Where the code promises one summation order -- NAD_GEMV_M1_SPEC
1 / 0, NAD_GEMV_AHEAD 1 / 0, the register ring's depth, a batch problem against its single launch -- the outputs of
one (format, activation type, K, waves, grid) are equal as uint32.

Shapes.  N = 40: 3 stripes, the last 8 columns wide; by default one workgroup each, with NAD_GEMV_GRID=2 workgroup 0
streams two (the cursor re-derived at a stripe boundary, u_r = 1).  K = (tiles - 1) K tiles + 40: K % 8 == 0 and the
tail ends inside a 32-deep MFMA step, a group and a tile.  GEOMS below lists the tile counts and knobs that select each
slice form; register stages are always forced (NAD_GEMV_NST), never left to the heuristic.  Fused QKV: widths
(40, 24, 16); the gate / up pair: two weights of N = 40 with and without the tmp1 output; a batch: 3 problems over two
weights.  woq_gemv_kernel: 10 tiles under NAD_GEMV_WAVES=2 and NAD_GEMV_GRID=2, M = 5 and 13 (the last fragment ragged
against 16; NAD_MID_MAX_M=0 keeps 13 rows off the mid-M kernel, as the fused entries do), and M = 1 at K = 9 tiles + 37,
where the activations take the element-wise staging path.

Each launch prints one line; profiles/gemv_matrix_errors.txt keeps a digest of them, one line per case.
tests/test_gemv_matrix_cpu.py holds the table to the dry run without a GPU and caps it by a reachability sweep;
tests/test_gemv_instances_cpu.py holds the built library's symbols to TABLE, ELSEWHERE and UNREACHED.
"""
import itertools
from collections import namedtuple

import numpy as np
import pytest

from tests import edges
from tests import fold_model as fm
from tests import mid_model as mm
from tests.conftest import gpu_available
from tests.fold_model import BF16, F16, F32, S2, S4, S8
from tests.test_mid_gpu import TOL

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla

N = 40
QKV_N = (40, 24, 16)
M_ROWS = 13
BAR = TOL["fp32"]
assert BAR == TOL["fp16"] == TOL["bf16"] == 2e-5
K_TILE = {S4: 128, S2: 256, S8: 64}
ACTS = ("fp32", "fp16", "bf16")
ACT_T = {"fp32": 0, "fp16": 1, "bf16": 2}   # kActF32 / kActF16 / kActBF16 (woq_kernels.h)
ST_CODE = {F32: 0, BF16: 1, F16: 2}         # kScaleF32 / kScaleBF16 / kScaleF16 (woq_layout.h)
ST_NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
KNOBS = ("NAD_GEMV_GRID", "NAD_GEMV_WAVES", "NAD_GEMV_NST", "NAD_GEMV_M1_SPEC", "NAD_GEMV_AHEAD", "NAD_MID_MAX_M")

# ------------------------------------------------------------------------------------------------ formats
# (qtype, group size or None = one group (bs = K), groups per K tile, asym allowed, fp32 activations only)
# one group size per (bits, groups per K tile); on the fp32 launches also groups of two K tiles (tpg_shift 1: a group
# boundary inside a stage) and one group (ng == 1: none at all)
M1_FORMATS = [
    (S4, 128, 1, True, False), (S4, 64, 2, True, False),
    (S2, 256, 1, True, False), (S2, 128, 2, True, False), (S2, 64, 4, False, False),  # prepare_gemv: gpt 4 sym only
    (S4, 256, 1, True, True), (S4, None, 1, True, True), (S2, 512, 1, True, True), (S2, None, 1, True, True),
]
# woq_gemv_kernel also has four groups per tile at int4, and int8
GEMV_FORMATS = M1_FORMATS + [(S4, 32, 4, False, False), (S8, 64, 1, True, False), (S8, 32, 2, True, False)]


def weight_sets(formats):
    return [(qt, bs, gpt, asym, st, f32) for qt, bs, gpt, ok, f32 in formats
            for asym in ((False, True) if ok else (False,)) for st in (F32, BF16, F16)]


def k_of(qt, tiles, tail=40):
    return (tiles - 1) * K_TILE[qt] + tail


# ------------------------------------------------------------------------------------------------ the M = 1 table
# woq_gemv_m1s_kernel is instantiated for (m1s_launch_b4 / _b2): int4 one group per tile, every activation type; int4
# two per tile, fp32 rows; int2 sym, fp32 rows.  Anything else runs woq_gemv_m1_kernel.
def has_m1s(bits, gpt, asym, act):
    if bits == 4:
        return gpt == 1 or (gpt == 2 and act == "fp32")
    return bits == 2 and not asym and act == "fp32"


# m1s_launch3: {(weights NWT, register stages NST): fixed reduce count NSC} per slice form; a pair missing here is
# served by woq_gemv_m1_kernel
NARROW = {(1, 1): 0, (2, 1): 0, (3, 1): 0, (1, 2): 0}          # one 1- or 2-tile slice per wave, runtime count
NARROW16 = {(1, 1): 16, (2, 1): 16, (3, 1): 16, (1, 2): 16}    # ... all 16 slots
WIDE2 = {(1, 1): 0, (2, 1): 0, (3, 1): 0, (1, 2): 0}           # two 4-tile slices per wave
WIDE2_11 = {(1, 1): 11, (2, 1): 0, (3, 1): 0, (1, 2): 0}       # ... 11 waves (one group per tile or coarser only)
WIDE4 = {(1, 1): 0}                                            # four 4-tile slices per wave
WIDE4_7 = {(1, 1): 7}                                          # ... 7 waves

Geom = namedtuple("Geom", "id tiles knobs waves waves_fine ksn spw forms forms_fine bits", defaults=((4, 2),))
# waves / forms: one group per tile or coarser; waves_fine / forms_fine: two or four groups per tile (at most 8 waves
# on 4-tile slices)
GEOMS = [
    Geom("ks1",      5,  {},                       5,  5,  1, 1, NARROW,   NARROW),     # 5 waves: count % 4 != 0
    Geom("ks1_16",   16, {},                       16, 16, 1, 1, NARROW16, NARROW16),
    Geom("ks2",      19, {},                       10, 10, 2, 1, NARROW,   NARROW),
    Geom("ks2_16",   31, {},                       16, 16, 2, 1, NARROW16, NARROW16),   # the load-ahead forms
    Geom("ks4_spw2", 19, {"NAD_GEMV_WAVES": 4},    4,  4,  4, 2, WIDE2,    WIDE2),
    Geom("ks4_spw4", 19, {"NAD_GEMV_WAVES": 2},    2,  2,  4, 4, WIDE4,    WIDE4),
    Geom("idle",     10, {"NAD_GEMV_WAVES": 16},   16, 8,  4, 2, WIDE2,    WIDE2, (4,)),    # 3 slices: idle waves
    # ... int2: 16 waves' activation rows of two 4-tile slices (10 KiB each) do not fit the 160 KiB of LDS
    Geom("idle12",   10, {"NAD_GEMV_WAVES": 12},   12, 8,  4, 2, WIDE2,    WIDE2, (2,)),
    Geom("nsc11",    41, {"NAD_GEMV_WAVES": 11},   11, 8,  4, 2, WIDE2_11, WIDE2),
    Geom("nsc7",     57, {"NAD_GEMV_WAVES": 7},    7,  7,  4, 4, WIDE4_7,  WIDE4_7),
]
GEOM = {g.id: g for g in GEOMS}
FUSED_GEOMS = ("ks1", "ks1_16", "ks2", "ks2_16", "ks4_spw2", "ks4_spw4")
BATCH_GEOMS = ("ks1", "ks2", "ks4_spw2", "ks4_spw4")
# m1s_ahead_form: int4, one group per tile, fp32 rows, one register stage, 16 waves of one 2-tile slice each and two or
# more stages per wave: (call, NAD_GEMV_GRID) of the ks2_16 launches that stream them -- one weight's 3 stripes and the
# QKV's 6 over 2 workgroups; the pair streams two weights per stripe at any grid
AHEAD_AT = {("single", 2), ("qkv", 2), ("pair", None), ("pair", 2)}
NWT = {"single": 1, "pair": 2, "qkv": 3}


def tf(v):
    return "true" if v else "false"


def m1_name(bits, gpt, act, asym, ksn, spw, batch, nst, st):
    return f"woq_gemv_m1_kernel<{bits}, {gpt}, {ACT_T[act]}, {tf(asym)}, {ksn}, {spw}, {tf(batch)}, {nst}, {st}>"


def m1s_name(bits, gpt, act, asym, ksn, spw, nst, st, nwt, nsc, ahead):
    return (f"woq_gemv_m1s_kernel<{bits}, {gpt}, {ACT_T[act]}, {tf(asym)}, {ksn}, {spw}, {nst}, {st}, {nwt}, {nsc}, "
            f"{tf(ahead)}>")


def gemv_name(bits, hilo, gpt, asym, nst):
    return f"woq_gemv_kernel<{bits}, {hilo}, {gpt}, {tf(asym)}, {nst}>"


def m1_expected(ws, act, geom, call, grid, nst, spec, ahead):
    """the instantiation an M = 1 launch of this weight set must resolve to"""
    qt, _, gpt, asym, st, _ = ws
    bits = fm.BITS[qt]
    stc = -1 if bits == 4 else ST_CODE[st]  # int2: the scale type at compile time (NAD_INT2_ST)
    if call == "batch":
        return m1_name(bits, gpt, act, asym, geom.ksn, geom.spw, True, 3, stc)  # NAD_M1_BATCH_NST
    forms = geom.forms if gpt == 1 else geom.forms_fine
    if spec and has_m1s(bits, gpt, asym, act) and (NWT[call], nst) in forms:
        ah = bool(ahead and bits == 4 and gpt == 1 and act == "fp32" and geom.id == "ks2_16" and nst == 1 and
                  (call, grid) in AHEAD_AT)
        return m1s_name(bits, gpt, act, asym, geom.ksn, geom.spw, nst, stc, NWT[call], forms[NWT[call], nst], ah)
    return m1_name(bits, gpt, act, asym, geom.ksn, geom.spw, False, nst, stc)


# one launch: call single / qkv / pair / pair_aux / batch / rows; group: launches of one group give the same bits
Launch = namedtuple("Launch", "call geom tiles tail m act knobs inst group")


def _knobs(geom, grid, nst, spec=1, ahead=1, mid_off=False):
    k = dict.fromkeys(KNOBS)
    k.update(geom.knobs if geom else {})
    k.update({"NAD_GEMV_GRID": grid, "NAD_GEMV_NST": nst, "NAD_GEMV_M1_SPEC": spec, "NAD_GEMV_AHEAD": ahead})
    if mid_off:
        k["NAD_MID_MAX_M"] = 0
    return k


def _variants(ws, act, geom):
    """(grid, nst, spec, ahead): NAD_GEMV_GRID=2 where the table resolves it differently (ks2_16); NAD_GEMV_M1_SPEC=0
    where it can make a difference"""
    specs = (1, 0) if has_m1s(fm.BITS[ws[0]], ws[2], ws[3], act) else (1,)
    for grid in ((None, 2) if geom.id == "ks2_16" else (None,)):
        for nst, spec in itertools.product((1, 2), specs):
            for ahead in ((1, 0) if geom.id == "ks2_16" and spec and nst == 1 else (1,)):
                yield grid, nst, spec, ahead


def acts_of(ws):
    return ("fp32",) if ws[5] else ACTS


def m1_launches(ws):
    for act in acts_of(ws):
        for g in GEOMS:
            if fm.BITS[ws[0]] not in g.bits:
                continue
            for grid, nst, spec, ahead in _variants(ws, act, g):
                yield Launch("single", g.id, g.tiles, 40, 1, act, _knobs(g, grid, nst, spec, ahead),
                             m1_expected(ws, act, g, "single", grid, nst, spec, ahead), ("single", g.id, grid, act))


def fused_launches(ws):
    bits, gpt = fm.BITS[ws[0]], ws[2]
    # 16-bit rows where the stripe stream is instantiated for them; elsewhere they run the single launches' kernels
    for act in (acts_of(ws) if bits == 4 and gpt == 1 else ("fp32",)):
        for gid in FUSED_GEOMS:
            g = GEOM[gid]
            for grid, nst, spec, ahead in _variants(ws, act, g):
                yield Launch("qkv", gid, g.tiles, 40, 1, act, _knobs(g, grid, nst, spec, ahead),
                             m1_expected(ws, act, g, "qkv", grid, nst, spec, ahead), ("qkv", gid, grid, act))
                for call in ("pair_aux",) + (("pair",) if nst == 1 and spec else ()):
                    yield Launch(call, gid, g.tiles, 40, 1, act, _knobs(g, grid, nst, spec, ahead),
                                 m1_expected(ws, act, g, "pair", grid, nst, spec, ahead), (call, gid, grid, act))
    for gid in BATCH_GEOMS:
        g = GEOM[gid]
        yield Launch("batch", gid, g.tiles, 40, 1, "fp32", _knobs(g, None, None),
                     m1_expected(ws, "fp32", g, "batch", None, 3, 1, 1), ("batch", gid))


GEMV_KNOBS = Geom("rows", 10, {"NAD_GEMV_WAVES": 2}, 2, 2, 4, 0, None, None)
# (rows, activation type, HILO of launch_gemv: fp16 rows 0, up to 8 rows 1, more 2)
GEMV_ROWS = [(5, "fp32", 1), (5, "bf16", 1), (13, "fp32", 2), (13, "bf16", 2), (13, "fp16", 0)]


def gemv_launches(ws):
    qt, _, gpt, asym, _, f32 = ws
    bits = fm.BITS[qt]
    for m, act, hilo in GEMV_ROWS:
        if f32 and act != "fp32":
            continue
        for nst in (1, 3):
            yield Launch("rows", "rows", 10, 40, m, act, _knobs(GEMV_KNOBS, 2, nst, mid_off=True),
                         gemv_name(bits, hilo, gpt, asym, nst), ("rows", m, act))
    for nst in (1, 3):  # K % 8 != 0: a_fast off, so M = 1 leaves the M = 1 kernels too
        yield Launch("rows", "tail37", 10, 37, 1, "fp32", _knobs(GEMV_KNOBS, 2, nst, mid_off=True),
                     gemv_name(bits, 1, gpt, asym, nst), ("rows37",))


FAMILIES = {"m1": (M1_FORMATS, m1_launches), "fused": (M1_FORMATS, fused_launches),
            "gemv": (GEMV_FORMATS, gemv_launches)}
CASES = [(fam, ws) for fam, (formats, _) in FAMILIES.items() for ws in weight_sets(formats)]
TABLE = {l.inst for fam, ws in CASES for l in FAMILIES[fam][1](ws)}


def case_id(c):
    fam, (qt, bs, _, asym, st, _) = c
    group = "per_channel" if bs is None else f"g{bs}"
    return f"{fam}_int{fm.BITS[qt]}_{group}_{'asym' if asym else 'sym'}_{ST_NAME[st]}"


# ------------------------------------------------------------------------------------------------ weights, model
_MADE = {}
_PROD = {}
RAN = set()  # the instantiation of every matrix launch that passed


def weight(oracle, ws, n, k, which=0):
    """-> (key, (Q, S, Z), group size, the loaded DeviceWeight); made once and shared"""
    qt, bs, _, asym, st, _ = ws
    bs = bs or k
    key = (n, k, bs, qt, st, asym, which)
    if key not in _MADE:
        seed = n * 7 + k * 3 + bs + fm.BITS[qt] * 1000 + (st % 97) * 11 + int(asym) + which * 101
        blob, fields = fm.make(oracle, n, k, bs, qt, st, asym, seed)
        _MADE[key] = (fields, bestla.DeviceWeight(blob))
    return (key,) + _MADE[key][:1] + (bs,) + _MADE[key][1:]


def act_values(k, act):
    """the M_ROWS rows every launch of this K and type takes its first M of, drawn from uniform(-0.5, 0.5) and rounded
    to the type: fp32 numpy holding the type's values"""
    A = np.random.default_rng(k * 3 + ACTS.index(act)).uniform(-0.5, 0.5, size=(M_ROWS, k)).astype(np.float32)
    return mm.round_act(A, act)


def model(key, fields, bs, act):
    """-> (activation values, the model's float64 product [M_ROWS][n]), computed once and never written to"""
    if (key, act) not in _PROD:
        xv = act_values(key[1], act)
        prod = mm.product(mm.split_hi_lo(xv), *fields, bs)
        xv.setflags(write=False)
        prod.setflags(write=False)
        _PROD[key, act] = (xv, prod)
    return _PROD[key, act]


def upload(xv, act):
    xt = torch.from_numpy(np.array(xv)).cuda().to(edges.torch_dtype(act))
    assert np.array_equal(xt.float().cpu().numpy(), xv)  # the type holds the model's values bit for bit
    return xt


def nan(m, n):
    return torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")


def set_knobs(knob, state, want):
    for name in KNOBS:
        if state.get(name, "unset") != want[name]:
            knob(name, want[name])
            state[name] = want[name]


def run(oracle, ws, l):
    """-> (plan, the launch's outputs as fp32 numpy, the model's value of each)"""
    k = k_of(ws[0], l.tiles, l.tail)
    if l.call in ("single", "rows"):
        key, fields, bs, w = weight(oracle, ws, N, k)
        xv, prod = model(key, fields, bs, l.act)
        out = nan(l.m, N)
        plan = w.plan(l.m, l.act)
        w.forward(upload(xv[:l.m], l.act), out=out)
        return plan, [out.cpu().numpy()], [prod[:l.m]]
    if l.call == "qkv":
        made = [weight(oracle, ws, n, k, i) for i, n in enumerate(QKV_N)]
        outs = [nan(1, n) for n in QKV_N]
        xv = act_values(k, l.act)
        plan = bestla.plan_qkv(*[w for *_, w in made], 1, l.act)
        bestla.qkv_forward(upload(xv[:1], l.act), *[w for *_, w in made], out=outs)
        return plan, [o.cpu().numpy() for o in outs], [model(key, f, bs, l.act)[1][:1] for key, f, bs, _ in made]
    (k1, f1, bs, w1), (k3, f3, _, w3) = weight(oracle, ws, N, k, 0), weight(oracle, ws, N, k, 1)
    xv, gate = model(k1, f1, bs, l.act)
    up = model(k3, f3, bs, l.act)[1]
    if l.call in ("pair", "pair_aux"):  # SiLU(gate) * up of the two float64 products; tmp1 = SiLU(gate)
        aux = l.call == "pair_aux"
        tmp1, tmp2 = (nan(1, N) if aux else None), nan(1, N)
        plan = bestla.plan_gate_up(w1, w3, 1, l.act)
        bestla.ffn_gate_up(upload(xv[:1], l.act), w1, w3, act="silu", tmp1=tmp1, tmp2=tmp2)
        t1 = edges.silu64(gate[:1])
        return plan, [tmp2.cpu().numpy()] + ([tmp1.cpu().numpy()] if aux else []), [t1 * up[:1]] + ([t1] if aux else [])
    assert l.call == "batch"  # 3 problems over two weights of one shape
    xs = [upload(xv[i:i + 1], "fp32") for i in range(3)]
    ys = [nan(1, N) for _ in xs]
    batch = bestla.Batch([(w, x, y) for w, x, y in zip((w1, w3, w1), xs, ys)])
    plan = batch.plan()
    batch.run()
    got = [y.cpu().numpy() for y in ys]
    for w, x, y in zip((w1, w3, w1), xs, got):  # (c): each problem against its single launch
        assert np.array_equal(y.view(np.uint32), w.forward(x).cpu().numpy().view(np.uint32)), (l, "batch != single")
    return plan, got, [gate[0:1], up[1:2], gate[2:3]]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gemv_instantiation(oracle, knob, case):
    fam, ws = case
    state, first = {}, {}
    for l in FAMILIES[fam][1](ws):
        set_knobs(knob, state, l.knobs)
        plan, ys, refs = run(oracle, ws, l)
        want_kernel = "woq_gemv_kernel" if l.call == "rows" else "woq_gemv_m1_kernel"
        assert plan["kernel"] == want_kernel and plan["instance"] == l.inst, (l, plan)   # (a)
        assert plan["m1_spec"] == l.inst.startswith("woq_gemv_m1s_kernel") and plan["ahead"] == l.inst.endswith(
            "true>") and plan["launches"] == 1, (l, plan)
        what = (f"{l.call}/{l.geom}{'/grid2' if l.call != 'rows' and l.knobs['NAD_GEMV_GRID'] else ''} "
                f"K={k_of(ws[0], l.tiles, l.tail)}{f' M={l.m}' if l.m > 1 else ''} {l.act} "
                f"{case_id(case).split('_', 1)[1]}")
        err = max(edges.rel_err(y, ref, ref) for y, ref in zip(ys, refs))  # each output against its own max|model|
        y = np.concatenate(ys, axis=1)
        print(f"{l.inst} {what}: err {err:.2e} bar {BAR:.0e}")
        assert np.isfinite(y).all() and err <= BAR, (l.inst, what, err)                   # (b)
        if l.group in first:                                                              # (c)
            assert np.array_equal(y.view(np.uint32), first[l.group][1].view(np.uint32)), (
                l.inst, first[l.group][0], what)
        else:
            first[l.group] = (l.inst, y)
        RAN.add(l.inst)


def test_gemv_matrix_is_complete():
    """Every instantiation of the table ran and passed, counted from what test_gemv_instantiation recorded (so this
    test needs the whole file run, in order)."""
    print(f"decode GEMV matrix: {len(RAN & TABLE)} of {len(TABLE)} instantiations recorded")
    missing = sorted(TABLE - RAN)
    assert not missing, (len(missing), missing[:4])
    assert RAN == TABLE, sorted(RAN - TABLE)[:4]
