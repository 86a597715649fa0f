"""GPU ne_get_rows (woq_rows.hip, nad_device_get_rows): bit for bit against references that are never the code under
test -- the oracle's unpack_fp32 for blobs, the reference's own dequantize_row_* outputs (tests/golden) and the numpy
block models (tests/gguf_blocks.py, tests/q6k_blocks.py) for the GGUF types.  Every comparison is on uint32 words, no
tolerance; the one figure with a bar is the tied-use case, which ties the op's row index to the forward's column index
at the decode bar (2e-5 of max|y|).  Each comparison prints its count of differing words (pytest -s shows them).
"""
import ctypes as C

import numpy as np
import pytest

from tests import edges
from tests import gguf_blocks as gb
from tests import q6k_blocks as qb
from tests.conftest import gpu_available
from tests.oracle_lib import (BF16, DQ8_BNB, F16, F32, F4_BNB, F4_E2M1, F4_NF4, F8_E4M3, F8_E5M2, F8_E8M0, S1, S2, S3, S4,
                              S5, S7, S8, load_ref_golden)
from tests.test_gpu_parity import _blob

pytestmark = pytest.mark.gpu

if gpu_available():
    import torch
    from neural_amd import _lib, bestla

TOL_DECODE = 2e-5
N, K = 300, 1024                      # the last stripe has 12 columns
ROWS = [0, 15, 16, 287, 288, 299]

BLOBS = {
    # name: n, k, bs, qtype, stype, asym, comp
    "s4_g128_f16_sym": (N, K, 128, S4, F16, False, 1),
    "s4_g32_bf16_asym": (N, K, 32, S4, BF16, True, 4),
    "s4_perchannel_f32": (N, K, K, S4, F32, False, 1),
    "s2_g64_f32_asym": (N, K, 64, S2, F32, True, 1),
    "s8_g32": (N, K, 32, S8, F32, False, 1),
    "s1": (N, K, 64, S1, F16, False, 1),
    "s3": (N, K, 128, S3, F16, False, 1),
    "s5": (N, K, 64, S5, F32, True, 1),
    "s7": (N, K, 128, S7, F32, False, 1),
    "nf4": (N, K, 32, F4_NF4, F32, False, 1),
    "e2m1": (N, K, 64, F4_E2M1, BF16, False, 2),
    "bnb_fp4": (N, K, 32, F4_BNB, F16, False, 1),
    "f8_e4m3_e8m0": (N, K, 32, F8_E4M3, F8_E8M0, False, 1),
    "f8_e5m2_f32": (N, K, 128, F8_E5M2, F32, False, 1),
    "s4_dq8_bnb": (N, K, 128, S4, DQ8_BNB, False, 1),
    # K that is not a whole number of the K tile (128 / 256 / 64 deep), and K = 300: no multiple of 8
    "s4_g128_k384": (44, 384, 128, S4, F16, False, 1),
    "s4_g32_k320": (44, 320, 32, S4, BF16, True, 1),
    "s2_g64_k320": (44, 320, 64, S2, F32, True, 1),
    "s8_g32_k96": (44, 96, 32, S8, F32, False, 1),
    "s4_perchannel_k300": (44, 300, 1024, S4, F32, False, 1),
    "f8_e5m2_g128_k300": (44, 300, 128, F8_E5M2, F32, False, 1),
}
GGUF = {"q4_1": gb.Q4_1, "q5_0": gb.Q5_0, "q5_1": gb.Q5_1, "q8_0": gb.Q8_0}
GGUF_GOLDEN = [f"{t}_{c}" for t in GGUF for c in ("n40_k256", "n16_k96")]   # k96: 0.75 / 1.5 K tiles
Q6K_GOLDEN = ["n40_k256", "n16_k768"]
NAMES = (list(BLOBS) + ["q4_0", "q4_0_golden_n40_k256"] + list(GGUF) + ["golden_" + c for c in GGUF_GOLDEN] +
         ["q6_k", "q6_k_k768"] + ["q6_k_golden_" + c for c in Q6K_GOLDEN] + ["device_quantize"])

_CACHE = {}


def q4_0_dequant(blocks, n, k):
    """dequantize_row_q4_0: w = (nibble - 8) * d, elements 0..15 the low nibbles, 16..31 the high ones"""
    b = np.asarray(blocks, np.uint8).reshape(n, k // 32, 18)
    d = b[:, :, 0:2].copy().view(np.float16).reshape(n, k // 32).astype(np.float32)
    qs = b[:, :, 2:].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=2) - 8
    return (q.astype(np.float32) * d[:, :, None]).reshape(n, k)


def _weight(oracle, name):
    """(DeviceWeight, reference fp32 [n][k]) by name, made once and never written to"""
    if name in _CACHE:
        return _CACHE[name]
    rng = np.random.default_rng(len(name) + 7)
    if name in BLOBS:
        n, k, bs, qt, st, asym, comp = BLOBS[name]
        blob = _blob(oracle, n, k, bs, qt, st, asym, comp, seed=n + k + len(name))
        w, ref = bestla.DeviceWeight(blob), oracle.unpack_fp32(blob).T
    elif name == "q4_0":
        d = rng.uniform(0.001, 0.01, size=(N, K // 32)).astype(np.float16)
        blocks = np.concatenate([d.view(np.uint8).reshape(N, K // 32, 2),
                                 rng.integers(0, 256, size=(N, K // 32, 16), dtype=np.uint8)], axis=2).ravel()
        w, ref = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q4_0, blocks, N, K), q4_0_dequant(blocks, N, K)
    elif name == "q4_0_golden_n40_k256":
        g = load_ref_golden("gguf")["q4_0_n40_k256"]
        ref = g["deq"].reshape(40, 256)
        assert np.array_equal(q4_0_dequant(g["q4_0"], 40, 256).view(np.uint32), ref.view(np.uint32))  # pins the model
        w = bestla.DeviceWeight.from_q4_0(g["q4_0"], 40, 256)
    elif name in GGUF:
        t = GGUF[name]
        wm = (rng.uniform(-1, 1, size=(N, K)) + (1.5 if gb.HAS_MIN[t] else 0.0)).astype(np.float32)
        blocks = gb.quantize(t, wm)
        w, ref = bestla.DeviceWeight.from_gguf(t, blocks, N, K), gb.dequant(t, blocks, N, K)
    elif name.startswith("golden_"):
        case = name[len("golden_"):]
        g = load_ref_golden("gguf_types")[case]
        n, k, _ = (int(v) for v in g["meta"])
        tname = case[:4]
        w, ref = bestla.DeviceWeight.from_gguf(GGUF[tname], g[tname], n, k), g["deq"].reshape(n, k)
    elif name in ("q6_k", "q6_k_k768"):
        n, k = (N, K) if name == "q6_k" else (44, 768)
        blocks = qb.random_blocks(n, k, seed=n + k)
        w, ref = bestla.DeviceWeight.from_q6_k(blocks, n, k), qb.dequant(blocks, n, k)
    elif name.startswith("q6_k_golden_"):
        g = load_ref_golden("q6_k")[name[len("q6_k_golden_"):]]
        n, k = (int(v) for v in g["meta"])
        w, ref = bestla.DeviceWeight.from_gguf(bestla.GGUF_Q6_K, g["q6_k"], n, k), g["deq"].reshape(n, k)
    else:
        assert name == "device_quantize"
        wm = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(N, K)).astype(np.float32)).cuda()
        w, blob = bestla.DeviceWeight.quantize(wm, group_size=32, weight_dtype="int4", scale_dtype="fp16", alg="asym",
                                               return_blob=True)
        ref = oracle.unpack_fp32(blob).T
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    ref.setflags(write=False)
    assert ref.shape == (w.n, w.k)
    _CACHE[name] = (w, ref)
    return _CACHE[name]


def _ids(values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def _expected(ref, ids):
    """rows of ref, +0.0 where the id is no row"""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < ref.shape[0])
    out = np.zeros((len(ids), ref.shape[1]), np.float32)
    out[ok] = ref[ids[ok]]
    return out


def _same_bits(got, want, label):
    got = np.ascontiguousarray(got.detach().cpu().numpy() if hasattr(got, "detach") else got)
    diff = int((got.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).sum())
    print(f"get_rows {label}: {diff} differing words of {want.size}")
    assert got.shape == want.shape and diff == 0, (label, diff)


# ------------------------------------------------------------------------------------------------ 1. every layout
@pytest.mark.parametrize("name", NAMES)
def test_every_layout(oracle, name):
    w, ref = _weight(oracle, name)
    rows = [r for r in ROWS if r < w.n] + [w.n - 1] + list(np.random.default_rng(1).permutation(w.n))
    out = w.get_rows(_ids(rows))
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(rows), w.k)
    _same_bits(out, ref[rows], name)


# ------------------------------------------------------------------------------------------------ 2. ids
IDS_WEIGHTS = ["s4_g128_f16_sym", "q6_k", "s8_g32_k96"]


@pytest.mark.parametrize("name", IDS_WEIGHTS)
@pytest.mark.parametrize("m", [1, 5, 200])
def test_row_counts_and_duplicates(oracle, name, m):
    w, ref = _weight(oracle, name)
    ids = np.random.default_rng(m).integers(0, w.n, size=m)
    if m >= 5:
        ids[1] = ids[3] = ids[0]                      # duplicates
    _same_bits(w.get_rows(_ids(ids)), ref[ids], f"{name} m={m}")


@pytest.mark.parametrize("name", IDS_WEIGHTS)
def test_strided_id_table(oracle, name):
    w, ref = _weight(oracle, name)
    table = np.random.default_rng(3).integers(0, w.n, size=(37, 3)).astype(np.int32)
    tt = torch.from_numpy(table).cuda()
    for col in range(3):
        view = tt[:, col]
        assert view.stride(0) == 3
        _same_bits(w.get_rows(view), ref[table[:, col]], f"{name} ids_stride=3 column {col}")


@pytest.mark.parametrize("name", IDS_WEIGHTS)
def test_ids_out_of_range_give_plus_zero(oracle, name):
    w, ref = _weight(oracle, name)
    ids = [w.n - 1, -1, 0, w.n, 1, 2 ** 31 - 1, w.n - 2, -2 ** 31, 17 % w.n]
    out = w.get_rows(_ids(ids))
    _same_bits(out, _expected(ref, ids), f"{name} out-of-range ids")
    bits = out.cpu().numpy().view(np.uint32)
    for r in (1, 3, 5, 7):
        assert not bits[r].any()                      # +0.0, not -0.0


# ------------------------------------------------------------------------------------------------ 3. window
@pytest.mark.parametrize("name", ["s4_g32_bf16_asym", "q6_k", "s4_perchannel_k300", "s2_g64_k320"])
@pytest.mark.parametrize("pad", [24, 8])
def test_writes_exactly_its_window(oracle, name, pad):
    w, ref = _weight(oracle, name)
    ids = [r for r in ROWS if r < w.n] + [w.n, w.n - 1]
    m, ldo = len(ids), w.k + pad
    assert ldo % 4 == 0
    can = edges.Canary((edges.G + m + edges.G) * ldo)
    win = can.window(edges.G * ldo, m, w.k, ldo)
    assert win.data_ptr() % 16 == 0
    idt = _ids(ids)
    got, = edges.twice(can, lambda: w.get_rows(idt, out=win), f"{name} ldo=k+{pad}")
    _same_bits(got, _expected(ref, ids), f"{name} window ldo=k+{pad}")


# ------------------------------------------------------------------------------------------------ 4. output types
@pytest.mark.parametrize("name", ["s4_g128_f16_sym", "f8_e4m3_e8m0", "q5_1", "q6_k", "s4_perchannel_k300"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_half_outputs_are_the_fp32_result_rounded_once(oracle, name, dtype):
    w, ref = _weight(oracle, name)
    dt = getattr(torch, dtype)
    ids = [r for r in ROWS if r < w.n] + [w.n, 3, w.n - 1]
    out = w.get_rows(_ids(ids), dtype=dt)
    assert out.dtype == dt
    want = torch.from_numpy(_expected(ref, ids)).to(dt)     # round to nearest even, on the host
    diff = int((out.cpu().view(torch.int16) != want.view(torch.int16)).sum())
    print(f"get_rows {name} {dtype}: {diff} differing halfwords of {want.numel()}")
    assert diff == 0
    # into a padded buffer: a row stride of whole 16-byte runs (8 halves), at least 8 halves of padding
    buf = torch.full((len(ids), -(-w.k // 8) * 8 + 8), float("nan"), dtype=dt, device="cuda")
    w.get_rows(_ids(ids), out=buf[:, :w.k])
    assert torch.equal(buf[:, :w.k].cpu().view(torch.int16), want.view(torch.int16))
    assert bool(torch.isnan(buf[:, w.k:]).all())


# ------------------------------------------------------------------------------------------------ 5. graph
@pytest.mark.parametrize("name", ["s4_g128_f16_sym", "q6_k"])
def test_captured_call_follows_ids_rewritten_on_the_device(oracle, name):
    w, ref = _weight(oracle, name)
    m = 5
    ids = _ids([0] * m)
    out = torch.empty((m, w.k), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w.get_rows(ids, out=out)
        with torch.cuda.graph(g, stream=s):
            w.get_rows(ids, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for step, cur in enumerate(([3, 1, 4, 1, 5], [w.n - 1, w.n, -1, 16, 15], [287 % w.n, 16, 2, 299 % w.n, 0])):
        ids.copy_(_ids(cur))                                # rewritten on the device, no new capture
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _same_bits(out, _expected(ref, cur), f"{name} graph replay {step}")


# ------------------------------------------------------------------------------------------------ 6. tied use
@pytest.mark.parametrize("name", ["q6_k", "s4_g128_f16_sym"])
def test_tied_embedding_and_lm_head(oracle, name):
    """the row get_rows returns is the row the forward multiplies by: row . x in float64 against y[0][id]"""
    w, _ = _weight(oracle, name)
    x = torch.from_numpy(np.random.default_rng(11).uniform(-1, 1, size=(1, w.k)).astype(np.float32)).cuda()
    y0 = w.forward(x).clone()
    ids = ROWS + [7, 100, 201]
    rows = w.get_rows(_ids(ids))
    y1 = w.forward(x)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    y = y0.cpu().numpy().astype(np.float64)[0]
    dots = rows.cpu().numpy().astype(np.float64) @ x.cpu().numpy().astype(np.float64)[0]
    err = float(np.abs(dots - y[ids]).max() / np.abs(y).max())
    print(f"get_rows {name} tied use: max|row . x - y[id]| / max|y| = {err:.3e} (bar {TOL_DECODE:.0e})")
    assert err <= TOL_DECODE, err
    # and a wrong row would show: the neighbouring column is far outside the bar
    assert float(np.abs(dots - y[[i + 1 if i + 1 < w.n else i - 1 for i in ids]]).max() / np.abs(y).max()) > 100 * TOL_DECODE


# ------------------------------------------------------------------------------------------------ 7. both tile orders
KMAJOR_FIELD = 11 * 4   # DeviceWeight::kmajor: the twelfth 32-bit field of the descriptor (woq_layout.h)


def _info(w):
    o = np.zeros(14, np.int64)
    assert _lib.lib().nad_weight_info2(w.desc, bestla._ptr(o), 14) == 14
    return o


def test_both_tile_orders(oracle):
    """No loader selects the K-major order today (nad_device_load, the GGUF loaders, nad_device_quantize and
    nad_synthetic_weight all pass kmajor = 0 to layout_geometry), so the K-major weight is made here: the tiles, scale
    rows and zero-point rows of a loaded stripe-major weight transposed on the device from [ns][nt] to [nt][ns] (the
    sections keep their sizes and places) under a copy of the descriptor with kmajor = 1.  nad_weight_info2 value 13
    shows which order each descriptor has, and the library's own unpack reads the transposed weight back unchanged."""
    w, ref = _weight(oracle, "s4_g32_bf16_asym")
    a = lambda v: (v + 255) // 256 * 256  # noqa: E731
    ns, nt, ng = w.ns, w.nt, w.ng
    tb, sb, zb = ns * nt * 1024, ns * ng * 16 * 2, ns * ng * 16
    assert nt > 1 and ng > 1 and ns > 1 and w.asym and w.bytes >= a(tb) + a(sb) + a(zb)
    mem = w.mem.clone()
    mem[:tb] = w.mem[:tb].view(ns, nt, 1024).transpose(0, 1).reshape(-1)
    mem[a(tb):a(tb) + sb] = w.mem[a(tb):a(tb) + sb].view(ns, ng, 32).transpose(0, 1).reshape(-1)
    z0 = a(tb) + a(sb)
    mem[z0:z0 + zb] = w.mem[z0:z0 + zb].view(ns, ng, 16).transpose(0, 1).reshape(-1)
    desc = (C.c_uint8 * len(w.desc))()
    C.memmove(desc, w.desc, len(w.desc))
    assert int.from_bytes(bytes(desc[KMAJOR_FIELD:KMAJOR_FIELD + 4]), "little") == 0
    desc[KMAJOR_FIELD] = 1
    # the sections' addresses follow the copy
    base_old, base_new = w.mem.data_ptr(), mem.data_ptr()
    raw = bytearray(bytes(desc))
    for off in range(0, len(raw) - 7, 8):
        v = int.from_bytes(raw[off:off + 8], "little")
        if base_old <= v < base_old + w.bytes:
            raw[off:off + 8] = (v - base_old + base_new).to_bytes(8, "little")
    C.memmove(desc, bytes(raw), len(raw))
    wk = bestla.DeviceWeight(_desc=desc, _mem=mem)
    assert _info(w)[13] == 0 and _info(wk)[13] == 1
    assert (wk.n, wk.k, wk.ns, wk.nt, wk.ng) == (w.n, w.k, ns, nt, ng)
    assert np.array_equal(wk.unpack().view(np.uint32), ref.T.view(np.uint32))
    rows = ROWS + list(range(w.n))
    for order, weight in (("stripe-major", w), ("K-major", wk)):
        _same_bits(weight.get_rows(_ids(rows)), ref[rows], f"s4_g32_bf16_asym {order}")
