"""ne_get_rows on a device weight, the part that needs no GPU: the two entries are declared, exported and have Python
signatures; the dry run (nad_plan_get_rows) on geometry-only descriptors; every refusal of nad_device_get_rows by name;
and the lane map woq_rows.hip decodes with -- restated here in numpy and checked against a brute-force inverse of the
layout description (woq_layout.h), so that the GPU test is not the first place it is exercised.
"""
import ctypes as C

import numpy as np
import pytest

from neural_amd import _lib, bestla

F32O, F16O, BF16O = 0, 1, 2


def test_symbols_declared_exported_and_signed():
    L = _lib.lib()
    names = _lib.header_symbols()
    for name in ("nad_device_get_rows", "nad_plan_get_rows"):
        assert name in names, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert "NAD_KERNEL_GET_ROWS 20" in open(_lib.HEADER).read()
    assert bestla.KERNELS[20] == "woq_get_rows_kernel"


@pytest.mark.parametrize("bits,k,group,runs", [(4, 4096, 128, 2), (4, 384, 128, 1), (2, 4096, 64, 1), (2, 4352, 64, 2),
                                               (8, 4096, 32, 4), (8, 96, 32, 1), (6, 4096, 16, 4), (6, 4352, 16, 5)])
def test_plan_on_geometry_only_weights(bits, k, group, runs):
    """a unit is (row, 16 K tiles) -- Q6_K: (row, 4 superblocks) --, a workgroup takes four: grid = ceil(m * runs / 4), and
    grows with m"""
    desc = bestla.plan_only_weight(bits, 32000, k, group, "fp16", asym=(bits == 2))
    prev = 0
    for m in (1, 2, 5, 16, 2048):
        for dtype in ("fp32", "fp16", "bf16"):
            p = bestla.plan_get_rows(desc, m, dtype)
            assert p["kernel"] == "woq_get_rows_kernel" and p["threads"] == 256 and p["launches"] == 1, p
            assert p["grid"] == -(-m * runs // 4), (m, p)
        assert p["grid"] >= prev and (m < 16 or p["grid"] > prev)
        prev = p["grid"]
    assert bestla.plan_get_rows(desc, 0)["launches"] == 0  # m = 0 launches nothing


def _call(desc, m=4, out=1 << 20, dtype=F32O, ldo=None, k=256, ids=1 << 21, stride=1):
    L = _lib.lib()
    L.nad_clear_error()
    rc = L.nad_device_get_rows(desc, C.c_void_p(ids), stride, m, C.c_void_p(out), dtype, k if ldo is None else ldo,
                               None)
    return rc, _lib.last_error()


def test_every_refusal_is_named():
    """nothing here launches: the pointers are never dereferenced on the host, and the descriptor holds no weights"""
    L = _lib.lib()
    k = 256
    desc = bestla.plan_only_weight(4, 64, k, 128, "fp16")
    zero = (C.c_uint8 * L.bestla_device_storage_size())()
    rc, err = _call(zero)
    assert rc == -1 and "not a loaded neural_amd device weight" in err, err
    rc, err = _call(desc, m=-1)
    assert rc == -1 and "m must not be negative" in err, err
    rc, err = _call(desc, ldo=k - 4)
    assert rc == -1 and "ldo must be at least k" in err, err
    for bad in (-1, 3, 7):
        rc, err = _call(desc, dtype=bad)
        assert rc == -1 and "out_dtype must be fp32" in err, err
    # the 16-byte stores: base and row stride
    for out in ((1 << 20) + 4, (1 << 20) + 8, (1 << 20) + 2):
        rc, err = _call(desc, out=out)
        assert rc == -1 and "16-byte" in err, err
    for dtype, ldo in ((F32O, k + 1), (F32O, k + 2), (F32O, k + 3), (F16O, k + 4), (BF16O, k + 4), (F16O, k + 1)):
        rc, err = _call(desc, dtype=dtype, ldo=ldo)
        assert rc == -1 and "16-byte" in err, (dtype, ldo, err)
    rc, err = _call(desc, stride=0)
    assert rc == -1 and "ids_stride" in err, err
    act_order = bestla.plan_only_weight(4, 64, k, 128, "fp16", act_order=True)
    rc, err = _call(act_order)
    assert rc == -1 and "is act-order (desc_act): rows are not gathered from it" in err, err
    with pytest.raises(RuntimeError, match="act-order"):
        bestla.plan_get_rows(act_order, 1)
    # with every argument in order the call gets as far as the launch, which a geometry-only weight refuses
    for dtype, ldo in ((F32O, k), (F32O, k + 4), (F16O, k + 8), (BF16O, k)):
        rc, err = _call(desc, dtype=dtype, ldo=ldo)
        assert rc == -1 and "geometry-only" in err, err
    assert _call(desc, m=0) == (0, "")
    # ... and so does every entry that would launch on it
    y = np.zeros((1, 64), np.float32)
    x = np.zeros((1, k), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    L.nad_clear_error()
    assert L.nad_device_forward(vp(x), 0, desc, vp(y), 1, 64, k, k, 64, 0, None, 0, None, 0, None) == -1
    assert "geometry-only" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ the lane map
KT = {4: 128, 2: 256, 8: 64}
WIDTH = {4: 4, 2: 2, 8: 8}


def lane_map(bits, n, kk):
    """What woq_get_rows_kernel computes for element (n, kk): (stripe, tile, lane slot of the 16-byte piece, dword of
    the piece, shift of the field inside the dword)"""
    s, c = n >> 4, n & 15
    t, kin = kk // KT[bits], kk % KT[bits]
    d, kq, j = kin // 32, (kin % 32) // 8, kin % 8
    slot = kq * 16 + c
    if bits == 4:
        return s, t, slot, d, 4 * ((j >> 1) + 4 * (j & 1))
    if bits == 2:
        return s, t, slot, d >> 1, 2 * ((j >> 1) + 4 * (d & 1) + 8 * (j & 1))
    return s, t, slot, 2 * d + (j >> 2), 8 * (j & 3)


def layout_inverse(bits, ns, nt):
    """{(stripe, tile, lane, dword, shift): (n, k)} by walking the layout description field by field: lane l of a tile
    owns column 16 s + (l & 15) and k-quarter l >> 4; step d covers k = t KT + 32 d + 8 kq + j;
      int4 dword (one step):  nibble position p holds element j = 2 p (p < 4) / 2 (p - 4) + 1 (p >= 4)
      int2 dword (two steps): crumb position p: step h = (p & 7) >> 2, j = 2 (p & 3) + (p >> 3)
      int8 dword pair (step): byte b of dword w holds element j = 4 w + b"""
    inv = {}
    for s in range(ns):
        for t in range(nt):
            for lane in range(64):
                n, kq = 16 * s + (lane & 15), lane >> 4
                for dword in range(4):
                    for p in range(32 // WIDTH[bits]):
                        if bits == 4:
                            d, j = dword, (2 * p if p < 4 else 2 * (p - 4) + 1)
                        elif bits == 2:
                            d, j = 2 * dword + ((p & 7) >> 2), 2 * (p & 3) + (p >> 3)
                        else:
                            d, j = dword >> 1, 4 * (dword & 1) + p
                        inv[(s, t, lane, dword, WIDTH[bits] * p)] = (n, t * KT[bits] + 32 * d + 8 * kq + j)
    return inv


@pytest.mark.parametrize("bits", [4, 2, 8])
def test_lane_map_inverts_the_layout(bits):
    ns, nt = 2, 2
    inv = layout_inverse(bits, ns, nt)
    assert len(inv) == ns * nt * 64 * 128 // WIDTH[bits]           # every field of every tile, once
    assert len(set(inv.values())) == len(inv) == ns * 16 * nt * KT[bits]
    for n in range(ns * 16):
        for kk in range(nt * KT[bits]):
            assert inv[lane_map(bits, n, kk)] == (n, kk), (bits, n, kk)
    # the lane's 8 k of a step are consecutive in the output row, and the four k-quarters of a step adjoin
    for kq in range(4):
        ks = sorted(k for (s, t, lane, dword, sh), (n, k) in inv.items() if (s, t, lane) == (0, 0, kq * 16 + 3))
        runs = np.array(ks).reshape(-1, 8)
        assert (np.diff(runs, axis=1) == 1).all() and (runs[:, 0] % 32 == 8 * kq).all()
