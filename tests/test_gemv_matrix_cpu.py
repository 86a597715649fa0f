"""The decode GEMV matrix (tests/test_gemv_matrix_gpu.py) pinned without a GPU, on its own formats and K:

  (a) the model (mid_model.product) against the oracle on the same values sits inside the bar the GPU matrix holds the
      kernels to, 2e-5 of max|ref|;
  (b) what that bar has to cover: the float32-numpy restatement of the model's operands (mid_model.product_f32) against
      the float64 model at every K used, the 57-tile ones included -- the condition that the bar can be met at all;
  (c) the drawn fields do their job at M = 1, N = 40: a scale or a zero point rolled by one group or one column moves
      the product by more than 1000 bars;
  (d) every launch of the GPU matrix resolves, in the dry run of the same call, to the instantiation its table names,
      so a stale table shows on a machine without a GPU;
  (e) a sweep of dry runs over bits, group sizes, scale and activation types, M, N, K and the GEMV's knobs reports no
      instantiation outside the table: the cap that keeps the matrix from leaving out something reachable.

The worst figures printed by (a) - (c) are recorded at the end of profiles/gemv_matrix_errors.txt."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import fold_model as fm
from tests import mid_model as mm
from tests.fold_model import S8
from tests.test_gemv_matrix_gpu import (BAR, CASES, FAMILIES, GEMV_FORMATS, GEOMS, K_TILE, KNOBS, M_ROWS, N,
                                        QKV_N, ST_NAME, TABLE, act_values, case_id, k_of, set_knobs, weight_sets)

# every (tiles, tail) the matrix makes a weight of
SHAPES = sorted({(g.tiles, 40) for g in GEOMS} | {(10, 40), (10, 37)})
MODEL_SETS = weight_sets(GEMV_FORMATS)


def rel(y, ref):
    return float(np.abs(np.asarray(y, np.float64) - ref).max() / np.abs(ref).max())


def _set_id(ws):
    return case_id(("x", ws))[2:]


@pytest.mark.parametrize("ws", MODEL_SETS, ids=_set_id)
def test_gemv_model_against_the_oracle(oracle, ws):
    qt, bs0, gpt, asym, st, f32 = ws
    bits = fm.BITS[qt]
    # the M = 1 kernels' shapes for the formats they take; woq_gemv_kernel's two for all
    shapes = [s for s in SHAPES if (qt != S8 and not (bits == 4 and gpt == 4)) or s[0] == 10]
    for tiles, tail in shapes:
        k = k_of(qt, tiles, tail)
        bs = bs0 or k
        blob, (Q, S, Z) = fm.make(oracle, N, k, bs, qt, st, asym, seed=k + bs)
        ng = -(-k // bs)
        assert Q.shape == (k, N) and S.shape == Z.shape == (ng, N) and -(-k // K_TILE[qt]) == tiles
        assert Q.min() == -(1 << (bits - 1)) and Q.max() == (1 << (bits - 1)) - 1
        assert fm.S_LO * 0.99 <= S.min() and S.max() <= fm.S_HI * 1.01 and S.max() / S.min() > 3
        name = f"int{bits} {_set_id(ws)} K={k}"
        for act in (("fp32",) if f32 else ("fp32", "fp16", "bf16")):
            xv = act_values(k, act)
            assert xv.shape == (M_ROWS, k)
            ref = oracle.forward(xv, blob, N, k).astype(np.float64)
            prod = mm.product(mm.split_hi_lo(xv), Q, S, Z, bs)
            dist = max(rel(prod[m:m + 1], ref[m:m + 1]) for m in range(M_ROWS))                        # (a), row by row
            acc = max(rel(mm.product_f32(xv[m:m + 1], Q, S, Z, bs), prod[m:m + 1]) for m in (0, 1, 2))  # (b), M = 1
            acc = max(acc, rel(mm.product_f32(xv, Q, S, Z, bs), prod))
            print(f"{name} {act} rows: model vs oracle {dist:.3e}, float32 vs float64 product of the model {acc:.3e} "
                  f"(bar {BAR:.0e})")
            assert dist <= BAR, (name, act, dist)
            assert acc <= BAR, (name, act, acc)
        # (c) at M = 1: the scale of the neighbouring column / group, the zero point of the neighbouring group / column
        x_eff = mm.split_hi_lo(act_values(k, "fp32")[:1])
        prod = mm.product(x_eff, Q, S, Z, bs)
        wrong = {"S column": mm.product(x_eff, Q, np.roll(S, 1, axis=1), Z, bs)}
        if ng > 1:
            wrong["S group"] = mm.product(x_eff, Q, np.roll(S, 1, axis=0), Z, bs)
        if asym:
            wrong["Z column"] = mm.product(x_eff, Q, S, np.roll(Z, 1, axis=1), bs)
            if ng > 1:
                wrong["Z group"] = mm.product(x_eff, Q, S, np.roll(Z, 1, axis=0), bs)
        moved = {what: rel(p, prod) for what, p in wrong.items()}
        print(f"    {name}: misaddressed by one: " + ", ".join(f"{what} {v:.2e}" for what, v in moved.items()))
        assert min(moved.values()) > 1000 * BAR, (name, moved)


# ---------------------------------------------------------------------------------------------- (d) table against plan
def plan_of(bestla, ws, l):
    qt, bs, _, asym, st, _ = ws
    bits, k = fm.BITS[qt], k_of(qt, l.tiles, l.tail)
    bs = bs or k
    if l.call in ("single", "rows"):
        return bestla.plan_forward(bits, N, k, bs, ST_NAME[st], asym, l.m, l.act)
    if l.call == "qkv":
        return bestla.plan_qkv_forward(bits, *QKV_N, k, bs, ST_NAME[st], asym, 1, l.act)
    if l.call in ("pair", "pair_aux"):
        return bestla.plan_gate_up_forward(bits, N, k, bs, ST_NAME[st], asym, 1, l.act)
    assert l.call == "batch"
    return bestla.Batch.plan_only(bestla.plan_only_weight(bits, N, k, bs, ST_NAME[st], asym), 3)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_gemv_table_matches_the_plan(knob, family):
    from neural_amd import bestla
    state, seen = {}, set()
    for fam, ws in CASES:
        if fam != family:
            continue
        for l in FAMILIES[fam][1](ws):
            set_knobs(knob, state, l.knobs)
            plan = plan_of(bestla, ws, l)
            kernel = "woq_gemv_kernel" if l.call == "rows" else "woq_gemv_m1_kernel"
            assert plan["kernel"] == kernel and plan["instance"] == l.inst and plan["launches"] == 1, (ws, l, plan)
            if l.call != "rows":
                g = next(g for g in GEOMS if g.id == l.geom)
                assert plan["threads"] == 64 * (g.waves if ws[2] == 1 else g.waves_fine), (ws, l, plan)
            seen.add(l.inst)
    print(f"{family}: {len(seen)} instantiations named by the dry run")
    assert seen <= TABLE


# ------------------------------------------------------------------------------------------------ (e) reachability
def _knob_grid():
    """knob settings of the sweep: the grid, waves and register-stage knobs in full product on the default path, the
    A/B switches each over the settings they interact with"""
    for grid in (None, 2):
        for waves in (None, 2, 4, 7, 8, 11, 16):
            for nst in (None, 1, 2, 3):
                yield dict(NAD_GEMV_GRID=grid, NAD_GEMV_WAVES=waves, NAD_GEMV_NST=nst)
    for waves in (None, 2, 4, 7, 8, 11, 16):
        for nst in (None, 1, 2):
            yield dict(NAD_GEMV_WAVES=waves, NAD_GEMV_NST=nst, NAD_GEMV_M1_SPEC=0)
    for grid in (None, 2):
        for nst in (None, 1):
            yield dict(NAD_GEMV_GRID=grid, NAD_GEMV_NST=nst, NAD_GEMV_AHEAD=0)
    for nst in (None, 1, 3):
        yield dict(NAD_GEMV_NST=nst, NAD_GEMV_LEAN=0)
    for waves in (None, 2, 7):
        for nst in (1, 2):
            yield dict(NAD_GEMV_WAVES=waves, NAD_GEMV_NST=nst, NAD_GEMV_SPW=2)


SWEEP_KNOBS = KNOBS + ("NAD_GEMV_LEAN", "NAD_GEMV_SPW")
SWEEP_N = (16, 40, 4096)
SWEEP_TILES = range(1, 113)


def sweep(knob):
    """-> the set of instance names any dry run of the grid reports.  The grid is walked in full over the knobs,
    formats, symmetry, K (1 .. 112 tiles, tail 40 and whole) and the calls; N, the scale type, the activation type and
    M rotate along K so that every value meets every format and knob setting many times (the instantiation depends on
    N only through the stripes per workgroup, on M only through M == 1 and M <= 8)."""
    from neural_amd import bestla
    from neural_amd._lib import lib
    L = lib()
    o = np.zeros(6, np.int64)
    po = o.ctypes.data_as(C.c_void_p)
    raw = set()
    formats = [(4, b) for b in (32, 64, 128, 256, 512, 0)] + [(2, b) for b in (32, 64, 128, 256, 512, 1024, 0)] + \
              [(8, b) for b in (32, 64, 128, 0)]
    ms = (1, 1, 2, 1, 5, 1, 8, 1, 9, 1, 13, 1, 16, 1, 3, 1, 4, 6, 7, 10, 11, 12, 14, 15)
    i = 0
    for kn in _knob_grid():
        for name in SWEEP_KNOBS:
            knob(name, kn.get(name))
        knob("NAD_MID_MAX_M", 0 if kn.get("NAD_GEMV_WAVES") == 2 else None)  # rows above 8 on the GEMV too
        for bits, bs in formats:
            kt = {4: 128, 2: 256, 8: 64}[bits]
            for asym in (0, 1):
                for tiles in SWEEP_TILES:
                    i += 1
                    k = tiles * kt if i % 5 == 0 else (tiles - 1) * kt + 40
                    n, st, at, m = SWEEP_N[i % 3], (i // 3) % 3, (i // 9) % 3, ms[(i // 7) % len(ms)]
                    if L.nad_plan_forward(bits, n, k, bs, st, asym, m, at, po, 6) == 6 and o[0] in (1, 2):
                        raw.add(int(o[4]) >> 4)
                    if i % 4 == 0 and L.nad_plan_qkv_forward(bits, 40, 24, n, k, bs, st, asym, 1, at, po, 6) == 6 \
                            and o[0] in (1, 2):
                        raw.add(int(o[4]) >> 4)
                    if i % 4 == 1 and L.nad_plan_gate_up_forward(bits, n, k, bs, st, asym, 1, at, po, 6) == 6 \
                            and o[0] in (1, 2):
                        raw.add(int(o[4]) >> 4)
        for bits, bs in formats:  # tile counts at a threshold of the slice forms: every type and call, no rotation
            kt = {4: 128, 2: 256, 8: 64}[bits]
            for asym, tiles, st, at in itertools.product((0, 1), (5, 16, 17, 19, 31, 32, 41, 57), (0, 1, 2), (0, 1, 2)):
                i += 1
                k, n = (tiles - 1) * kt + 40, SWEEP_N[1 + i % 2]
                if L.nad_plan_forward(bits, n, k, bs, st, asym, 1, at, po, 6) == 6 and o[0] in (1, 2):
                    raw.add(int(o[4]) >> 4)
                if L.nad_plan_qkv_forward(bits, 40, 24, n, k, bs, st, asym, 1, at, po, 6) == 6 and o[0] in (1, 2):
                    raw.add(int(o[4]) >> 4)
                if L.nad_plan_gate_up_forward(bits, n, k, bs, st, asym, 1, at, po, 6) == 6 and o[0] in (1, 2):
                    raw.add(int(o[4]) >> 4)
        for bits, bs in formats:  # the batched launch: fp32 rows, a thinner K grid
            if bits == 8:
                continue
            kt = {4: 128, 2: 256}[bits]
            for asym in (0, 1):
                for tiles in (1, 2, 5, 8, 16, 17, 19, 31, 33, 41, 57, 64, 65, 100, 112):
                    for st in ("fp32", "bf16", "fp16"):
                        try:
                            k = (tiles - 1) * kt + 40
                            d = bestla.plan_only_weight(bits, 40, k, bs or k, st, bool(asym))
                            if L.nad_plan_batch_only(d, 3, po, 6) == 6 and o[0] == 1:
                                raw.add(int(o[4]) >> 4)
                        except RuntimeError:
                            pass
    L.nad_clear_error()
    return {bestla._gemv_instance(v) for v in raw} - {None}, i


_SWEPT = {}


def swept(knob):
    if not _SWEPT:
        _SWEPT["names"], _SWEPT["calls"] = sweep(knob)
    return _SWEPT["names"]


def test_reachability_sweep_stays_inside_the_table(knob):
    names = swept(knob)
    print(f"reachability sweep: {_SWEPT['calls']} geometries, {len(names)} instantiations reported, table {len(TABLE)}")
    assert len(names) > 900  # the sweep is wide enough to mean something
    assert sorted(names - TABLE) == [], "reachable but not in the matrix"
