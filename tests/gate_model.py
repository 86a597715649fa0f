"""numpy float32 restatement of nad_moe_gate_route's logits (include/neural_amd.h, "the router from the hidden state").

For row r and expert e, x = act[r], w = gate[e] (an fp16 / bf16 gate widened exactly to float32 first).  Every product
and every sum is a float32 operation rounded on its own:

  slots   1024 slots t, each starting at +0.0.  For pass i = 0, 1, ... and j = 0..3 in that order slot t adds
          x[k] * w[k], k = 4 (t + 1024 i) + j; elements with k >= K are skipped.  Here K is padded with zeros to whole
          passes instead: the skipped elements then add +0.0, which leaves a sum that started at +0.0 as it is (it is
          never -0.0), bit for bit.
  waves   the 64 slots of wave t >> 6 by the xor butterfly s = s + s[lane ^ o], o = 32, 16, ..., 1.
  row     the 16 waves' sums in wave order: ((s0 + s1) + s2) + ... + s15.

The kernel is held to these bits (tests/test_moe_gate_gpu.py); the model is held to the exact dot product under
bound() (tests/test_moe_gate_cpu.py).
"""
import numpy as np

SLOTS, WAVES, PASS = 1024, 16, 4096


def passes(k):
    return -(-k // PASS)


def logits(x, gate):
    """x float32 [m][K], gate float32 [n_expert][K] -> float32 [m][n_expert]"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    gate = np.ascontiguousarray(gate, dtype=np.float32)
    m, k = x.shape
    ne = gate.shape[0]
    assert gate.shape[1] == k
    npass = passes(k)
    xp = np.zeros((m, npass * PASS), np.float32)
    wp = np.zeros((ne, npass * PASS), np.float32)
    xp[:, :k] = x
    wp[:, :k] = gate
    xp = xp.reshape(m, 1, npass, SLOTS, 4)
    wp = wp.reshape(1, ne, npass, SLOTS, 4)
    s = np.zeros((m, ne, SLOTS), np.float32)
    for i in range(npass):
        for j in range(4):
            s = s + xp[:, :, i, :, j] * wp[:, :, i, :, j]  # the product rounded to float32, then the sum
            assert s.dtype == np.float32
    s = s.reshape(m, ne, WAVES, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    assert (s == s[..., :1]).all()  # addition commutes: every lane of a wave holds the same value
    out = s[:, :, 0, 0]
    for w in range(1, WAVES):
        out = out + s[:, :, w, 0]
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def bound(x, gate):
    """depth * 2^-24 * sum |x_k w_k| per (row, expert), in float64: every partial sum of a chain of `depth` roundings
    is bounded by the sum of the magnitudes, and each rounding is relative 2^-24 at most.  depth: 4 adds per pass in the
    slot, 6 butterfly steps, 15 adds across the waves, 1 for the product's own rounding."""
    depth = 4 * passes(x.shape[1]) + 6 + 15 + 1
    mag = np.abs(x.astype(np.float64)) @ np.abs(gate.astype(np.float64)).T
    return depth * 2.0 ** -24 * mag


def stable_top_k(lg, top_k):
    """the indices of the top_k largest logits per row in descending order, a tie going to the lower index"""
    return np.argsort(-lg.astype(np.float64), axis=1, kind="stable")[:, :top_k].astype(np.int32)
