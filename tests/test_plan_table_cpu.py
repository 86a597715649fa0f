"""What the ten dense dry-run entries return, held to a recorded table: no GPU needed.

tests/golden/plan_dense_table.json was written by the library as it stood before the dense dry runs were put on the
shared recorder scope, stand-in map and geometry-only weight builder (capi_plan.hip), and is never regenerated from
the tree under test: a change to a kernel choice, a launch geometry, the truncation rule or an error text shows here as
a changed record.  It was made with that library by

    from tests import test_plan_table_cpu as t
    open(t.TABLE_PATH, "w").write(t.dump())

(t.record sets the case's NAD_* switch and re-reads the knobs itself when it is called without the knob fixture).  The
file has sorted keys and one record per line.  A value is the raw int64 record taken through lib() into a buffer
pre-filled with -7 -- kernel, grid, block, ksplit, fold (the flag word, the GEMV instantiation's name included),
launches -- or, for a call the library refuses, its whole error text.  nad_weight_plan_only writes a descriptor, not a
record: its value is nad_weight_info2's 14 values of that descriptor.

Cases.  FORMATS below, as (bits, group, scale type, asym).
  nad_plan_forward          FWD_SHAPES x ALL_M x fp32, fp16 activations; bf16 at N = K = 4096 only
  nad_plan_qkv_forward      QKV_SHAPES x FUSED_M x fp32, fp16
  nad_plan_gate_up_forward  GATE_UP_SHAPES x FUSED_M x fp32, fp16
  the descriptor entries, on plan_only_weight descriptors: nad_plan_qkv on (int2, int2, int4) g128 (the dual launch),
    three Q6_K, an act-order trio, int4 g128 with asym differing in V; nad_plan_gate_up on a Q6_K pair and on Q6_K +
    int4; nad_plan_batch_only with 1, 3, 8, 300 problems on int4 g128 and int2 g64 at 4096 x 4096; nad_plan_get_rows
    at the shapes of tests/test_get_rows_cpu.py; nad_weight_plan_only on every format, Q6_K and act-order
  knobs (KNOBS), at (4096, 4096) and (11008, 4096), int4 g128 and int8 g32, ALL_M, fp32 and fp16: nad_plan_forward
    under each but NAD_GEMM7_FUSE, which is the fused QKV's -- nad_plan_qkv_forward at the two QKV shapes of K = 4096
  refusals: one row per message these entries reach on geometry-only descriptors
  nout 0, 3, 6, 9 on one case per entry: min(nout, 6) values are written, nothing past them

What no row can show without a GPU: nad_plan_batch takes a created batch and nad_plan_weight a loaded weight, so both
appear with their refusals only (nad_plan_weight refuses a geometry-only descriptor: it looks the weight up before the
recording starts); a geometry-only descriptor carries no block mins, so nad_batch_create's refusal of them has no row.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from neural_amd import _lib, bestla
from neural_amd._lib import lib

TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_dense_table.json")

SCALE = {"fp32": 0, "bf16": 1, "fp16": 2}
ACT = {"fp32": 0, "fp16": 1, "bf16": 2}
FORMATS = ((4, 128, "fp16", False), (4, 128, "bf16", True), (4, 32, "fp32", False), (4, 64, "fp16", False),
           (4, -1, "fp16", False), (2, 64, "fp16", False), (2, 128, "fp16", True), (8, 32, "fp16", False),
           (8, 128, "fp16", False), (8, -1, "fp16", False))
Q6K = (6, 16, "fp16", False)
FWD_SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008), (32000, 4096), (300, 1024))
# the edges of every M rule in forward_one, run_mid, pipelined_gemm, splitk_plan and gemm7_pick_bm
ALL_M = (1, 2, 5, 8, 9, 12, 16, 17, 32, 33, 64, 65, 130, 256, 640, 2048, 4096)
QKV_SHAPES = ((4096, 4096, 4096, 4096), (4096, 1024, 1024, 4096), (40, 24, 300, 1024))
GATE_UP_SHAPES = ((11008, 4096), (14336, 4096), (512, 1024))
FUSED_M = (1, 5, 16, 40, 130, 2048)
KNOBS = (None, ("NAD_GEMM_KERNEL", 3), ("NAD_GEMM7_FUSE", 0), ("NAD_MID_WIDE", 0), ("NAD_GEMM7_BM", 32),
         ("NAD_GEMM7_BM", 256))
KNOB_FORMATS = ((4, 128, "fp16", False), (8, 32, "fp16", False))
GET_ROWS = ((4, 4096, 128), (4, 384, 128), (2, 4096, 64), (2, 4352, 64), (8, 4096, 32), (8, 96, 32), (6, 4096, 16),
            (6, 4352, 16))
NOUT = 12  # the buffer's length, and what a case passes as nout unless it says otherwise


def fname(f):
    return "%d,%d,%s,%s" % (f[0], f[1], f[2], "T" if f[3] else "F")


@functools.lru_cache(maxsize=None)
def desc(fmt, n, k, act_order=False):
    bits, group, st, asym = fmt
    return bestla.plan_only_weight(bits, n, k, group, st, asym, act_order)


def scalar(fmt, *shape):
    """the leading arguments of a scalar entry: bits, the shape, group, scale type, asym"""
    bits, group, st, asym = fmt
    return (bits,) + shape + (group, SCALE[st], int(asym))


def refusals():
    """(key, entry, the arguments before (out, nout), out given): one row per message"""
    g4 = FORMATS[0]
    w, w1k = desc(g4, 4096, 4096), desc(g4, 4096, 1024)
    zero = (C.c_uint8 * lib().bestla_device_storage_size())()
    for what, bits, n, k, m in (("bits 3", 3, 64, 256, 1), ("n 0", 4, 0, 256, 1), ("k 0", 4, 64, 0, 1),
                                ("m 0", 4, 64, 256, 0)):
        yield "forward/" + what, "nad_plan_forward", (bits, n, k, 128, 2, 0, m, 0), True
        yield "qkv_forward/" + what, "nad_plan_qkv_forward", (bits, n, n, n, k, 128, 2, 0, m, 0), True
        yield "gate_up_forward/" + what, "nad_plan_gate_up_forward", (bits, n, k, 128, 2, 0, m, 0), True
    yield "qkv_forward/nv 0", "nad_plan_qkv_forward", (4, 64, 64, 0, 256, 128, 2, 0, 1, 0), True
    yield "forward/out null", "nad_plan_forward", (4, 64, 256, 128, 2, 0, 1, 0), False
    yield "qkv_forward/out null", "nad_plan_qkv_forward", (4, 64, 64, 64, 256, 128, 2, 0, 1, 0), False
    yield "gate_up_forward/out null", "nad_plan_gate_up_forward", (4, 64, 256, 128, 2, 0, 1, 0), False
    yield "qkv/out null", "nad_plan_qkv", (w, w, w, 1, 0), False
    yield "gate_up/out null", "nad_plan_gate_up", (w, w, 1, 0), False
    yield "batch_only/out null", "nad_plan_batch_only", (w, 1), False
    yield "get_rows/out null", "nad_plan_get_rows", (w, 1, 0), False
    yield "weight/out null", "nad_plan_weight", (w, 1, 0), False
    yield "batch/out null", "nad_plan_batch", (w,), False
    yield "qkv/m 0", "nad_plan_qkv", (w, w, w, 0, 0), True
    yield "qkv/K mismatch", "nad_plan_qkv", (w, w1k, w, 1, 0), True
    yield "qkv/no descriptor", "nad_plan_qkv", (w, zero, w, 1, 0), True
    yield "qkv/null descriptor", "nad_plan_qkv", (w, w, None, 1, 0), True
    yield "qkv/q6k K too long", "nad_plan_qkv", (desc(Q6K, 64, 65536),) * 3 + (1, 0), True
    yield "gate_up/m 0", "nad_plan_gate_up", (w, w, 0, 0), True
    yield "gate_up/shape mismatch", "nad_plan_gate_up", (w, desc(g4, 11008, 4096), 1, 0), True
    yield "gate_up/K mismatch", "nad_plan_gate_up", (w, w1k, 1, 0), True
    yield "gate_up/format mismatch", "nad_plan_gate_up", (w, desc(FORMATS[3], 4096, 4096), 1, 0), True
    yield "gate_up/scale mismatch", "nad_plan_gate_up", (w, desc((4, 128, "fp32", False), 4096, 4096), 1, 0), True
    yield "gate_up/no descriptor", "nad_plan_gate_up", (zero, w, 1, 0), True
    yield "gate_up/q6k K too long", "nad_plan_gate_up", (desc(Q6K, 64, 65536),) * 2 + (1, 0), True
    yield "batch_only/null descriptor", "nad_plan_batch_only", (None, 1), True
    yield "batch_only/n 0", "nad_plan_batch_only", (w, 0), True
    yield "batch_only/no descriptor", "nad_plan_batch_only", (zero, 1), True
    yield "batch_only/q6k", "nad_plan_batch_only", (desc(Q6K, 4096, 4096), 3), True
    yield "batch_only/int4 g32", "nad_plan_batch_only", (desc(FORMATS[2], 4096, 4096), 3), True
    yield "batch_only/int8 g32", "nad_plan_batch_only", (desc(FORMATS[7], 4096, 4096), 3), True
    yield "batch_only/K 65536", "nad_plan_batch_only", (desc(g4, 64, 65536), 3), True
    yield "batch/null batch", "nad_plan_batch", (None,), True
    yield "weight/geometry-only", "nad_plan_weight", (w, 1, 0), True
    yield "weight/no descriptor", "nad_plan_weight", (zero, 1, 0), True
    yield "weight/null descriptor", "nad_plan_weight", (None, 1, 0), True
    yield "get_rows/no descriptor", "nad_plan_get_rows", (zero, 1, 0), True
    yield "get_rows/null descriptor", "nad_plan_get_rows", (None, 1, 0), True
    yield "get_rows/act-order", "nad_plan_get_rows", (desc(g4, 64, 256, True), 1, 0), True
    yield "get_rows/out_dtype 3", "nad_plan_get_rows", (w, 1, 3), True
    yield "get_rows/m -1", "nad_plan_get_rows", (w, -1, 0), True
    yield "get_rows/m 2^31-1", "nad_plan_get_rows", (w, (1 << 31) - 1, 0), True
    store = (C.c_uint8 * lib().bestla_device_storage_size())()
    for what, a in (("bits 3", (3, 64, 256, 128, 2, 0, 0)), ("n 0", (4, 0, 256, 128, 2, 0, 0)),
                    ("k 0", (4, 64, 0, 128, 2, 0, 0)), ("q6k k 384", (6, 64, 384, 16, 2, 0, 0)),
                    ("scale 3", (4, 64, 256, 128, 3, 0, 0)), ("scale -1", (4, 64, 256, 128, -1, 0, 0)),
                    ("group 48", (4, 64, 256, 48, 2, 0, 0))):
        yield "weight_plan_only/" + what, "nad_weight_plan_only", a + (store,), None
    yield "weight_plan_only/no storage", "nad_weight_plan_only", (4, 64, 256, 128, 2, 0, 0, None), None


def cases():
    """(key, knob as (name, value) or None, entry, the arguments before (out, nout), nout; nout None: the entry takes
    no record buffer and out False: it is given a null one)"""
    for f in FORMATS:
        for n, k in FWD_SHAPES:
            for act in ("fp32", "fp16", "bf16"):
                if act == "bf16" and (n, k) != (4096, 4096):
                    continue
                for m in ALL_M:
                    yield ("forward/%s/%dx%d/%s/%d" % (fname(f), n, k, act, m), None, "nad_plan_forward",
                           scalar(f, n, k) + (m, ACT[act]), NOUT)
        for act in ("fp32", "fp16"):
            for m in FUSED_M:
                for nq, nk, nv, k in QKV_SHAPES:
                    yield ("qkv_forward/%s/%d,%d,%dx%d/%s/%d" % (fname(f), nq, nk, nv, k, act, m), None,
                           "nad_plan_qkv_forward", scalar(f, nq, nk, nv, k) + (m, ACT[act]), NOUT)
                for n, k in GATE_UP_SHAPES:
                    yield ("gate_up_forward/%s/%dx%d/%s/%d" % (fname(f), n, k, act, m), None,
                           "nad_plan_gate_up_forward", scalar(f, n, k) + (m, ACT[act]), NOUT)
    # the descriptor entries
    store = (C.c_uint8 * lib().bestla_device_storage_size())()  # what nad_weight_plan_only writes
    g4, i2 = FORMATS[0], (2, 128, "fp16", False)
    trios = {"dual": (desc(i2, 4096, 4096), desc(i2, 1024, 4096), desc(g4, 1024, 4096)),
             "q6k": (desc(Q6K, 4096, 4096), desc(Q6K, 1024, 4096), desc(Q6K, 1024, 4096)),
             "act-order": (desc(g4, 4096, 4096, True), desc(g4, 1024, 4096, True), desc(g4, 1024, 4096, True)),
             "asym V": (desc(g4, 4096, 4096), desc(g4, 1024, 4096), desc((4, 128, "fp16", True), 1024, 4096))}
    pairs = {"q6k": (desc(Q6K, 11008, 4096), desc(Q6K, 11008, 4096)),
             "q6k+int4": (desc(Q6K, 11008, 4096), desc(g4, 11008, 4096)),
             "int4+q6k": (desc(g4, 11008, 4096), desc(Q6K, 11008, 4096))}
    for act in ("fp32", "fp16"):
        for m in FUSED_M:
            for name, ws in trios.items():
                yield "qkv/%s/%s/%d" % (name, act, m), None, "nad_plan_qkv", ws + (m, ACT[act]), NOUT
            for name, ws in pairs.items():
                yield "gate_up/%s/%s/%d" % (name, act, m), None, "nad_plan_gate_up", ws + (m, ACT[act]), NOUT
    for f in (g4, FORMATS[5]):
        for n in (1, 3, 8, 300):
            yield ("batch_only/%s/%d" % (fname(f), n), None, "nad_plan_batch_only", (desc(f, 4096, 4096), n), NOUT)
    for bits, k, group in GET_ROWS:
        d = desc((bits, group, "fp16", bits == 2), 32000, k)
        for m in (0, 1, 2, 5, 16, 2048):
            for dtype in ("fp32", "fp16", "bf16"):
                yield ("get_rows/%d,%d,%d/%s/%d" % (bits, k, group, dtype, m), None, "nad_plan_get_rows",
                       (d, m, ACT[dtype]), NOUT)
    for f in FORMATS + (Q6K,):
        for act_order in (False, True):
            yield ("weight_plan_only/%s/%d" % (fname(f), act_order), None, "nad_weight_plan_only",
                   scalar(f, 300, 1024) + (int(act_order), store), None)
    # the knobs
    for knob in KNOBS[1:]:
        for f in KNOB_FORMATS:
            for act in ("fp32", "fp16"):
                for m in ALL_M:
                    if knob[0] == "NAD_GEMM7_FUSE":
                        for nq, nk, nv, k in QKV_SHAPES[:2]:
                            key = "%s=%d/qkv_forward/%s/%d,%d,%dx%d/%s/%d" % (knob + (fname(f), nq, nk, nv, k, act, m))
                            yield (key, knob, "nad_plan_qkv_forward", scalar(f, nq, nk, nv, k) + (m, ACT[act]), NOUT)
                        continue
                    for n, k in FWD_SHAPES[:2]:
                        yield ("%s=%d/forward/%s/%dx%d/%s/%d" % (knob + (fname(f), n, k, act, m)), knob,
                               "nad_plan_forward", scalar(f, n, k) + (m, ACT[act]), NOUT)
    # the truncation rule, one case per entry
    w = desc(g4, 4096, 4096)
    for nout in (0, 3, 6, 9):
        for entry, a in (("nad_plan_forward", scalar(g4, 4096, 4096) + (2048, 0)),
                         ("nad_plan_qkv_forward", scalar(g4, 4096, 1024, 1024, 4096) + (1, 0)),
                         ("nad_plan_gate_up_forward", scalar(g4, 11008, 4096) + (1, 0)),
                         ("nad_plan_qkv", trios["dual"] + (1, 0)), ("nad_plan_gate_up", pairs["q6k"] + (40, 0)),
                         ("nad_plan_batch_only", (w, 8)), ("nad_plan_get_rows", (w, 5, 1)),
                         ("nad_plan_weight", (w, 1, 0)), ("nad_plan_batch", (None,))):
            yield "nout %d/%s" % (nout, entry), None, entry, a, nout
    for key, entry, a, out in refusals():
        yield "refused/" + key, None, entry, a, None if out is None else (NOUT if out else False)


def call(entry, args, nout):
    """-> (the return value, the NOUT int64 the call was given, pre-filled with -7)"""
    o = np.full(NOUT, -7, np.int64)
    if nout is None:
        return getattr(lib(), entry)(*args), o
    return getattr(lib(), entry)(*args, bestla._ptr(o) if nout is not False else None, nout or 0), o


def record(case, knob=None):
    key, setting, entry, args, nout = case
    if knob is None and setting != record.setting:  # the generator (the module docstring)
        for name, _ in KNOBS[1:]:
            os.environ.pop(name, None)
        if setting is not None:
            os.environ[setting[0]] = str(setting[1])
        _lib.reload_knobs()
        record.setting = setting
    c, o = call(entry, args, nout)
    if c < 0:
        return bestla.last_error()
    if entry == "nad_weight_plan_only":
        info = np.full(14, -7, np.int64)
        assert c == 0 and lib().nad_weight_info2(args[-1], bestla._ptr(info), 14) == 14
        return tuple(int(v) for v in info)
    assert (o[c:] == -7).all(), o
    return tuple(int(v) for v in o[:c])


record.setting = None


def dump():
    rows = {c[0]: record(c) for c in CASES}
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(rows[k])) for k in sorted(rows)) + "\n}\n"


CASES = list(cases())


@functools.lru_cache(maxsize=None)
def table():
    with open(TABLE_PATH) as f:
        return {k: v if isinstance(v, str) else tuple(v) for k, v in json.load(f).items()}


def test_the_case_list_and_the_table_name_the_same_cases():
    keys = [c[0] for c in CASES]
    assert len(keys) == len(set(keys)) and set(keys) == set(table())
    for k, v in table().items():
        refused = k.startswith("refused/") or k.endswith(("/nad_plan_weight", "/nad_plan_batch"))
        assert isinstance(v, str) == refused, k
        if k.startswith("nout "):
            assert refused or len(v) == min(int(k.split("/")[0][5:]), 6), k
        elif not refused:
            assert len(v) == (14 if k.startswith("weight_plan_only/") else 6), k
    # every entry has records, and every knob its cases
    assert {c[2] for c in CASES} == {"nad_plan_forward", "nad_plan_weight", "nad_plan_qkv_forward", "nad_plan_qkv",
                                     "nad_plan_gate_up_forward", "nad_plan_gate_up", "nad_plan_batch",
                                     "nad_plan_batch_only", "nad_plan_get_rows", "nad_weight_plan_only"}
    assert {c[1] for c in CASES} == set(KNOBS)


@pytest.mark.parametrize("setting", KNOBS, ids=lambda s: "default" if s is None else "%s=%d" % s)
def test_every_record_is_the_tables(knob, setting):
    if setting is not None:
        knob(*setting)
    n = 0
    for case in CASES:
        if case[1] != setting:
            continue
        assert record(case, knob) == table()[case[0]], case[0]
        n += 1
    assert n > 100
