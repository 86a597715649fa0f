"""Seeded [N][K] weight matrices whose quantization groups hit every branch of quantize_kblock's integer (sNauto)
quantizer, and a reader of a blob's scale / zero-point / reduce sections.  Shared by tests/test_device_quantize_cpu.py
(which checks that the generator delivers what it promises, on the host packer alone) and
tests/test_device_quantize_gpu.py.

Column n carries groups of kind KINDS[n % len(KINDS)], repeated across its groups:
  zeros      all 0: the scale is 0, 0 * inf = NaN, and the float -> int cast's INT_MIN decides the codes
  one        one nonzero value
  positive   all positive: max + min > 0 beyond the threshold, nval = -full
  negative   negative-dominant: max + min < 0 beyond the threshold, nval = +full
  balanced   max = -min: nval = sym + 0.5
  ties       balanced at absmax (sym + 0.5) / 8, so the scale is 1 / 8 (sym and asym) and every other value
             (j + 0.5) / 8 sits on an exact rounding tie
  subnormal  all fp32 subnormals (the scale is subnormal, 1 / scale overflows)
  huge       magnitudes near 3e38 (max + min and max - min overflow)
  large      magnitudes near 1e6 (no fp16 fold: fold_ok = 0)
  random     plain normal
tame=True keeps the kinds whose scales an fp16 fold takes (fold_ok = 1)."""
import numpy as np

from neural_amd import bestla

KINDS = ["zeros", "one", "positive", "negative", "balanced", "ties", "subnormal", "huge", "large", "random"]
TAME = ["zeros", "one", "positive", "negative", "balanced", "ties", "random"]

# (n, k, group): the smallest shapes at which each thing can go wrong (group -1: per-channel)
SHAPES = [(48, 256, 128), (50, 200, 64), (17, 96, 32), (33, 320, -1), (512, 1024, 128)]
CROSS_SHAPE = (50, 200, 64)
QTYPES = {"S4": bestla.S4, "S2": bestla.S2, "S8": bestla.S8}
SCALES = {"F32": bestla.F32, "BF16": bestla.BF16, "F16": bestla.F16}


def group_size(k, group):
    return k if group == -1 else group


def _group(kind, length, bits, rng):
    """-> (values float32 [length], tie mask)"""
    full = 1 << (bits - 1)
    sym = full - 1
    ties = np.zeros(length, bool)
    if kind == "zeros":
        v = np.zeros(length, np.float32)
    elif kind == "one":
        v = np.zeros(length, np.float32)
        v[rng.integers(length)] = rng.choice([-1.0, 1.0]) * rng.uniform(0.25, 2.0)
    elif kind == "positive":
        v = rng.uniform(0.1, 1.0, length)
    elif kind == "negative":
        v = rng.uniform(-0.9, 0.3, length)
        v[:1], v[1:2] = -1.0, 0.3  # (a group of one element keeps what fits)
    elif kind == "balanced":
        v = rng.uniform(-1.0, 1.0, length)
        v[:1], v[1:2] = 1.0, -1.0
    elif kind == "ties":
        v = (rng.integers(-sym, sym, length) + 0.5) / 8.0
        ties[:] = True
        v[:1], v[1:2] = (sym + 0.5) / 8.0, -(sym + 0.5) / 8.0
        ties[:2] = False
    elif kind == "subnormal":
        m = rng.integers(1, 1 << 20, length).astype(np.uint32) | (rng.integers(0, 2, length).astype(np.uint32) << 31)
        v = m.view(np.float32)
    elif kind == "huge":
        v = rng.uniform(2.5e38, 3.3e38, length) * rng.choice([-1.0, 1.0], length)
    elif kind == "large":
        v = rng.uniform(-1e6, 1e6, length)
    else:
        v = rng.normal(0.0, 1.0, length)
    return np.asarray(v, np.float32), ties


def matrix(n, k, group, bits, seed=0, tame=False):
    """-> (W float32 [n][k], tie mask [n][k], kind name per column)"""
    rng = np.random.default_rng([seed, n, k, bits, group & 0xffff])
    kinds = TAME if tame else KINDS
    gs = group_size(k, group)
    w = np.zeros((n, k), np.float32)
    ties = np.zeros((n, k), bool)
    cols = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        cols.append(kind)
        for j in range(0, k, gs):
            ln = min(gs, k - j)
            w[i, j:j + ln], ties[i, j:j + ln] = _group(kind, ln, bits, rng)
    assert np.isfinite(w).all()
    return w, ties, cols


def sections(blob):
    """The blob's correction sections over the real groups and columns: dict(scales fp32 [nblk][n], zps int8 [nblk][n] or
    None, reduce uint16 [nblk][n] or None)."""
    inf = bestla.blob_info(blob)
    n, k, bs, cstep = inf["n"], inf["k"], inf["bs"], inf["cstep"]
    nblk = -(-k // bs)
    raw = np.asarray(blob)[inf["s_off"]:inf["s_off"] + inf["s_size"]]
    if inf["scat"] == bestla.F32:
        s = raw.view(np.float32)
    elif inf["scat"] == bestla.BF16:
        s = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    else:
        s = raw.view(np.float16).astype(np.float32)
    out = dict(scales=s.reshape(-1, cstep)[:nblk, :n], zps=None, reduce=None)
    if inf["asym"]:
        out["zps"] = np.asarray(blob)[inf["z_off"]:inf["z_off"] + inf["z_size"]].view(np.int8).reshape(-1, cstep)[:nblk, :n]
    if inf["has_reduce"]:
        out["reduce"] = np.asarray(blob)[inf["r_off"]:inf["r_off"] + inf["r_size"]].view(np.uint16).reshape(
            -1, cstep)[:nblk, :n]
    return out
