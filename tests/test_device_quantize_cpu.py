"""The device quantizer's host side (nad_device_quantize_size, the refusals, the exports) and the promises of
tests/quant_cases.py, checked on the host packer alone: the matrices the GPU test compares on do reach every branch of
the sNauto quantizer.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from neural_amd import _lib, bestla
from tests import quant_cases as qc

BITS = [("S4", 4), ("S2", 2), ("S8", 8)]


def _absmax(w, gs):
    n, k = w.shape
    nblk = -(-k // gs)
    pad = np.zeros((n, nblk * gs), np.float32)
    pad[:, :k] = np.abs(w)
    return pad.reshape(n, nblk, gs).max(axis=2).T  # [nblk][n]


@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
@pytest.mark.parametrize("qname,bits", BITS)
def test_generator_reaches_every_branch(shape, qname, bits):
    n, k, group = shape
    gs = qc.group_size(k, group)
    full, sym = 1 << (bits - 1), (1 << (bits - 1)) - 1
    w, ties, cols = qc.matrix(n, k, group, bits)
    assert set(cols) == set(qc.KINDS)
    blob = bestla.quant_pack(w, gs, qc.QTYPES[qname], bestla.F32, False, bestla.COMP_INT8)
    s = qc.sections(blob)["scales"]
    am = _absmax(w, gs)
    live = am > 0
    with np.errstate(over="ignore"):
        for nval in (np.float32(sym + 0.5), np.float32(-full), np.float32(full)):
            assert (live & (s == am / nval)).any(), f"no group with nval = {nval}"
        # the ties: x * (1 / scale) is exactly half an integer, and there are at least N of them
        assert ties.sum() >= n
        sfull = np.repeat(s.T, gs, axis=1)[:, :k]
        v = w[ties] * (np.float32(1) / sfull[ties])
    assert (v - np.floor(v) == 0.5).all()
    # asym: an all-zero group has scale 0, zero point full - 1 (the INT_MIN of the NaN cast, wrapped and clipped)
    za = qc.sections(bestla.quant_pack(w, gs, qc.QTYPES[qname], bestla.F32, True, bestla.COMP_INT8))
    zero_cols = [i for i, c in enumerate(cols) if c == "zeros"]
    assert zero_cols and (za["zps"][:, zero_cols] == sym).all() and (za["scales"][:, zero_cols] == 0).all()
    # subnormal, huge and large columns are what they say
    for kind, lo, hi in (("subnormal", 0, 1.2e-38), ("huge", 2.5e38, 3.4e38), ("large", 0, 1e6)):
        c = [i for i, x in enumerate(cols) if x == kind]
        a = np.abs(w[c])
        assert c and (a >= lo).all() and (a <= hi).all()
    assert (np.abs(w[[i for i, x in enumerate(cols) if x == "subnormal"]]) > 0).all()


@pytest.mark.parametrize("shape", qc.SHAPES, ids=str)
@pytest.mark.parametrize("qname,bits", BITS)
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("comp", [bestla.COMP_F32, bestla.COMP_INT8, bestla.COMP_BF16])
@pytest.mark.parametrize("isa", [None, "avx512_vnni", "avx2"])
def test_sizes_match_the_host_blob(shape, qname, bits, asym, comp, isa, monkeypatch):
    if isa:
        monkeypatch.setenv("NAD_HOST_ISA", isa)
    else:
        monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    n, k, group = shape
    gs = qc.group_size(k, group)
    L = _lib.lib()
    w = np.ones((n, k), np.float32)
    for st in qc.SCALES.values():
        blob = bestla.quant_pack(w, gs, qc.QTYPES[qname], st, asym, comp)
        bsz = C.c_size_t(0)
        need = L.nad_device_quantize_size(n, k, gs, qc.QTYPES[qname], st, int(asym), comp, C.byref(bsz))
        assert need and need == L.nad_device_weight_size(bestla._ptr(blob)), _lib.last_error()
        assert bsz.value == blob.size == bestla.pack_size(n, k, gs, qc.QTYPES[qname], st, asym, comp)
        assert L.nad_device_quantize_size(n, k, gs, qc.QTYPES[qname], st, int(asym), comp, None) == need
    if group == -1:  # blocksize <= 0 is per-channel too
        assert L.nad_device_quantize_size(n, k, -1, qc.QTYPES[qname], bestla.F32, int(asym), comp, None) == \
            L.nad_device_quantize_size(n, k, k, qc.QTYPES[qname], bestla.F32, int(asym), comp, None)


REFUSED_WEIGHTS = {"S1_CLIP": bestla.S1, "S3_CLIP": bestla.S3, "S5_CLIP": bestla.S5, "S6_CLIP": bestla.S6,
                   "S7_CLIP": bestla.S7, "F4_E2M1": bestla.F4_E2M1, "F4_BNB": bestla.F4_BNB, "F4_NF4": bestla.F4_NF4,
                   "F8_E4M3": bestla.F8_E4M3, "F8_E5M2": bestla.F8_E5M2}
REFUSED_SCALES = {"DQ8_BNB": bestla.DQ8_BNB, "F8_E8M0": bestla.F8_E8M0}


def _quantize_args(w=1, devstor=1, devptr=1, n=32, k=64, ldw=64, bs=32, qt=bestla.S4, st=bestla.F16, cap=1 << 20,
                   blob=None, blob_cap=0, w_dtype=0):
    """placeholder pointers: every refusal comes before the device is touched"""
    buf = (C.c_uint8 * 512)()
    p = lambda x: C.cast(buf, C.c_void_p) if x else None
    return (p(w), w_dtype, n, k, ldw, bs, qt, st, 0, bestla.COMP_INT8, p(devstor), p(devptr), cap, blob, blob_cap, None)


@pytest.mark.parametrize("name", sorted(REFUSED_WEIGHTS))
def test_refused_weight_dtypes_are_named(name):
    L = _lib.lib()
    assert L.nad_device_quantize_size(32, 64, 32, REFUSED_WEIGHTS[name], bestla.F32, 0, bestla.COMP_INT8, None) == 0
    assert f"weight dtype {name} " in _lib.last_error() and "host path" in _lib.last_error()
    assert L.nad_device_quantize(*_quantize_args(qt=REFUSED_WEIGHTS[name])) == -1
    assert f"weight dtype {name} " in _lib.last_error()


@pytest.mark.parametrize("name", sorted(REFUSED_SCALES))
def test_refused_scale_dtypes_are_named(name):
    L = _lib.lib()
    assert L.nad_device_quantize_size(32, 64, 32, bestla.S4, REFUSED_SCALES[name], 0, bestla.COMP_INT8, None) == 0
    assert f"scale dtype {name} " in _lib.last_error() and "host path" in _lib.last_error()
    assert L.nad_device_quantize(*_quantize_args(st=REFUSED_SCALES[name])) == -1
    assert f"scale dtype {name} " in _lib.last_error()


def test_argument_errors_come_before_device_work():
    L = _lib.lib()
    need = L.nad_device_quantize_size(32, 64, 32, bestla.S4, bestla.F16, 0, bestla.COMP_INT8, None)
    bsz = bestla.pack_size(32, 64, 32, bestla.S4, bestla.F16, False, bestla.COMP_INT8)
    for kw, msg in ((dict(w=0), "null weight matrix"), (dict(devstor=0), "null devstor"),
                    (dict(devptr=0), "null deviceptr"), (dict(ldw=63), "ldw 63 < k 64"),
                    (dict(cap=need - 1), f"need {need} bytes, have {need - 1}"),
                    (dict(blob=C.cast((C.c_uint8 * 8)(), C.c_void_p), blob_cap=8), f"need {bsz} bytes, have 8"),
                    (dict(w_dtype=3), "w_dtype=3"), (dict(bs=48), "multiple of 32"), (dict(n=0), "n=0")):
        assert L.nad_device_quantize(*_quantize_args(**kw)) == -1, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert L.nad_device_quantize_size(32, 64, 32, bestla.S4, bestla.F16, 0, 9, None) == 0
    assert "CompType 9" in _lib.last_error()


def test_symbols_are_declared_and_exported():
    names = {"nad_device_quantize_size", "nad_device_quantize"}
    assert names <= set(_lib.header_symbols()) and names <= set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert names <= exported
    assert hasattr(bestla.DeviceWeight, "quantize")
