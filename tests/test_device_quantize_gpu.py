"""nad_device_quantize (woq_quant.hip): a weight quantized and packed on the GPU equals the host packer byte for byte --
the blob (BTLAGemmQuantPackB), the device layout (nad_device_load of that blob) and the descriptor -- on the matrices
of tests/quant_cases.py, which tests/test_device_quantize_cpu.py shows to reach every branch of the quantizer.  No
tolerance anywhere: every comparison is of bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import quant_cases as qc
from tests.conftest import gpu_available

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import bestla
    from neural_amd._lib import check, lib

CANARY = 0xA5
SLACK = 512
BITS = {"S4": 4, "S2": 2, "S8": 8}
COMPS = {"fp32": 1, "int8": 4}
FOLD_SEEN = set()


def _padded(w_t, pad=8):
    """the matrix on the device with ldw = k + pad, its padding NaN -> the [n][k] view"""
    n, k = w_t.shape
    buf = torch.full((n, k + pad), float("nan"), dtype=w_t.dtype, device="cuda")
    buf[:, :k] = w_t.cuda()
    return buf[:, :k]


def _info(desc):
    o = np.zeros(13, np.int64)
    assert lib().nad_weight_info2(desc, bestla._ptr(o), 13) == 13
    return [int(v) for v in o]


def _host_path(w32, gs, qt, st, asym, comp):
    """-> (blob, descriptor info, device bytes) of BTLAGemmQuantPackB + nad_device_load into a canary-filled buffer"""
    L = lib()
    blob = bestla.quant_pack(w32, gs, qt, st, asym, comp)
    need = L.nad_device_weight_size(bestla._ptr(blob))
    mem = torch.full((need + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    desc = (C.c_uint8 * L.bestla_device_storage_size())()
    check(L.nad_device_load(bestla._ptr(blob), desc, bestla._ptr(mem), need, bestla._stream()), "nad_device_load")
    return blob, _info(desc), mem, desc


def _device_path(w_dev, gs, qt, st, asym, comp, mem=None):
    L = lib()
    n, k = w_dev.shape
    bsz = C.c_size_t(0)
    need = L.nad_device_quantize_size(n, k, gs, qt, st, int(asym), comp, C.byref(bsz))
    assert need, bestla.last_error()
    if mem is None:
        mem = torch.full((need + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    blob = bestla._aligned_buffer(bsz.value)
    desc = (C.c_uint8 * L.bestla_device_storage_size())()
    check(L.nad_device_quantize(bestla._ptr(w_dev), bestla._act_code(w_dev), n, k, w_dev.stride(0), gs, qt, st,
                                int(asym), comp, desc, bestla._ptr(mem), need, bestla._ptr(blob), bsz.value,
                                bestla._stream()), "nad_device_quantize")
    return blob, _info(desc), mem, desc, need


def _compare(w32, w_dev, gs, qt, st, asym, comp):
    hblob, hinfo, hmem, _ = _host_path(w32, gs, qt, st, asym, comp)
    dblob, dinfo, dmem, _, need = _device_path(w_dev, gs, qt, st, asym, comp)
    assert dblob.size == hblob.size and np.array_equal(dblob, hblob), "blob differs from BTLAGemmQuantPackB's"
    assert dinfo == hinfo, (dinfo, hinfo)
    assert need == hinfo[11]
    assert torch.equal(dmem[:need], hmem[:need]), "device layout differs from nad_device_load's"
    assert bool((dmem[need:] == CANARY).all()), "bytes at or after `bytes` were written"
    # a second call into the same buffer: the same result
    first = dmem.clone()
    dblob2, dinfo2, _, _, _ = _device_path(w_dev, gs, qt, st, asym, comp, mem=dmem)
    assert torch.equal(dmem, first) and np.array_equal(dblob2, hblob) and dinfo2 == hinfo
    FOLD_SEEN.add(hinfo[12])
    return hinfo


def _case(shape, qname, asym, sname, comp, tame=False):
    n, k, group = shape
    w, _, _ = qc.matrix(n, k, group, BITS[qname], tame=tame)
    return _compare(w, _padded(torch.from_numpy(w)), qc.group_size(k, group), qc.QTYPES[qname], qc.SCALES[sname], asym,
                    COMPS[comp])


CROSS = list(itertools.product(sorted(qc.QTYPES), [False, True], sorted(qc.SCALES), sorted(COMPS)))


@pytest.mark.parametrize("isa", [None, "avx512_vnni", "avx2"])
@pytest.mark.parametrize("qname,asym,sname,comp", CROSS)
def test_cross_on_the_tail_shape(qname, asym, sname, comp, isa, monkeypatch):
    """(50, 200, 64): N tails, a partial last group, kpad > k; the three profiles cover the 48/4/64, 48/2/32, 48/4/4,
    48/1/1 and 24/1/1 cores"""
    if isa:
        monkeypatch.setenv("NAD_HOST_ISA", isa)
    else:
        monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    _case(qc.CROSS_SHAPE, qname, asym, sname, comp)


@pytest.mark.parametrize("shape", [s for s in qc.SHAPES if s != qc.CROSS_SHAPE], ids=str)
@pytest.mark.parametrize("qname,asym,sname,comp", CROSS)
def test_other_shapes(shape, qname, asym, sname, comp, monkeypatch):
    monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    _case(shape, qname, asym, sname, comp)


@pytest.mark.parametrize("qname", sorted(qc.QTYPES))
@pytest.mark.parametrize("asym", [False, True])
def test_fold_ok_takes_both_values(qname, asym, monkeypatch):
    """the full matrices carry scales no fp16 fold takes (fold_ok 0); the tame ones fold (fold_ok 1)"""
    monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    assert _case((48, 256, 128), qname, asym, "F16", "int8")[12] == 0
    assert _case((48, 256, 128), qname, asym, "F16", "int8", tame=True)[12] == 1
    assert FOLD_SEEN >= {0, 1}


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("qname,asym", itertools.product(sorted(qc.QTYPES), [False, True]))
def test_half_inputs_are_widened_exactly(dtype, qname, asym, monkeypatch):
    """fp16 / bf16 inputs give the bytes of the host path on the widened fp32 matrix"""
    monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    n, k, group = qc.CROSS_SHAPE
    w, _, _ = qc.matrix(n, k, group, BITS[qname])
    if dtype == "float16":
        w = np.clip(w, -60000.0, 60000.0)  # finite in fp16 (the subnormal columns become zeros and fp16 subnormals)
    wh = torch.from_numpy(w).to(getattr(torch, dtype))
    wide = wh.float().numpy()
    assert np.isfinite(wide).all()
    _compare(wide, _padded(wh), qc.group_size(k, group), qc.QTYPES[qname], bestla.F16, asym, COMPS["int8"])


@pytest.mark.parametrize("isa", [None, "avx2"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("qname,asym", itertools.product(sorted(qc.QTYPES), [False, True]))
def test_odd_k_and_unaligned_rows(qname, asym, dtype, isa, monkeypatch):
    """k = 97 and ldw = 100: rows that no vector load may take, a last group of one element, and (fp32 compute: the
    KTILE 1 cores) an odd kpad, which puts a stripe boundary inside a dword of packed int2 / int4 codes"""
    if isa:
        monkeypatch.setenv("NAD_HOST_ISA", isa)
    else:
        monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    w, _, _ = qc.matrix(17, 97, 32, BITS[qname])
    if dtype == "float16":
        w = np.clip(w, -60000.0, 60000.0)
    wh = torch.from_numpy(w).to(getattr(torch, dtype))
    _compare(wh.float().numpy(), _padded(wh, pad=3), 32, qc.QTYPES[qname], bestla.BF16, asym, COMPS["fp32"])


def test_forward_of_the_device_quantized_weight(monkeypatch):
    """one smoke: forward at M = 1 and M = 32 equals the host-loaded weight's bit for bit"""
    monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    n, k, group = 512, 1024, 128
    w, _, _ = qc.matrix(n, k, group, 4, tame=True)
    _, _, hmem, hdesc = _host_path(w, group, bestla.S4, bestla.F16, False, COMPS["int8"])
    _, _, dmem, ddesc, _ = _device_path(_padded(torch.from_numpy(w)), group, bestla.S4, bestla.F16, False, COMPS["int8"])
    hw, dw = bestla.DeviceWeight(_desc=hdesc, _mem=hmem), bestla.DeviceWeight(_desc=ddesc, _mem=dmem)
    rng = np.random.default_rng(3)
    for m in (1, 32):
        x = torch.from_numpy(rng.uniform(-1, 1, (m, k)).astype(np.float32)).cuda()
        yh, yd = hw.forward(x), dw.forward(x)
        assert bool(torch.isfinite(yh).all()) and torch.equal(yh, yd)


@pytest.mark.parametrize("kw", [dict(), dict(group_size=-1, weight_dtype="int8", scale_dtype="bf16", alg="asym"),
                                dict(group_size=64, weight_dtype="int2", scale_dtype="fp16", compute_dtype="fp32"),
                                dict(group_size=128, scale_dtype="fp8")], ids=str)
def test_python_entry_round_trips(kw, monkeypatch):
    """DeviceWeight.quantize(..., return_blob=True) unpacks to the integers and scales of bestla.quantize"""
    monkeypatch.delenv("NAD_HOST_ISA", raising=False)
    bits = {"int8": 8, "int2": 2}.get(kw.get("weight_dtype"), 4)
    w, _, _ = qc.matrix(48, 256, 128, bits, tame=True)
    wd = _padded(torch.from_numpy(w))
    ref = bestla.quantize(w, **kw)
    dw, blob = bestla.DeviceWeight.quantize(wd, return_blob=True, **kw)
    assert np.array_equal(blob, ref)
    assert np.array_equal(bestla.unpack(blob), bestla.unpack(ref))
    rs, ds = qc.sections(ref), qc.sections(blob)
    assert np.array_equal(rs["scales"], ds["scales"])
    assert (rs["zps"] is None) == (ds["zps"] is None) and (rs["zps"] is None or np.array_equal(rs["zps"], ds["zps"]))
    hw = bestla.DeviceWeight(ref)
    assert (dw.n, dw.k, dw.bits, dw.blocksize, dw.fold_ok, dw.bytes) == (hw.n, hw.k, hw.bits, hw.blocksize, hw.fold_ok,
                                                                        hw.bytes)
    assert np.array_equal(dw.unpack(), hw.unpack())
    only = bestla.DeviceWeight.quantize(wd, **kw)
    assert isinstance(only, bestla.DeviceWeight) and np.array_equal(only.unpack(), dw.unpack())


def test_python_entry_refuses_by_name():
    w = torch.zeros((32, 64), device="cuda")
    with pytest.raises(RuntimeError, match="weight dtype F4_NF4"):
        bestla.DeviceWeight.quantize(w, weight_dtype="nf4")
    with pytest.raises(ValueError, match="K contiguous"):
        bestla.DeviceWeight.quantize(torch.zeros((64, 32), device="cuda").t())
