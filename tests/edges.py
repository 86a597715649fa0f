"""Edge harness for the forward entries: one call with poisoned surroundings, checked against a float64 reference.

What a forward may touch is exactly its windows: it writes out[0:m, 0:n] and nothing else, reads the activations only
inside [0:m, 0:k], the bias and the residual only inside [0:m, 0:n], and its result does not depend on what out held
before.  The harness builds the operands so that breaking any of these shows:

  * output: a buffer [G + m + G][ldo] filled with one quiet-NaN bit pattern (CANARY), the window inside it.  After the
    call the window holds no NaN and every other element still is the canary, compared bit for bit as int32.
    "odd":     ldo = n + 5, window at column 0 (rows at every alignment: the scalar stores);
    "aligned": ldo = n + 8, window at the first column that makes its start 16-byte aligned (the float4 stores).
  * activations: "odd" -- storage [m][k + 24], window at column 8, the storage itself one element into its allocation
    (so no row is 16-byte aligned); "aligned" -- window at column 0, lda = roundup(k, 8) + 32 (every row 16-byte
    aligned: the a_fast / vec_ok loads).  All padding is NaN.
  * bias: 1-D broadcast, or a [m][n + 3] NaN-padded storage passed as a view (bias_ld = n + 3).
  * residual: [m][n + 7] NaN-padded storage passed as a view (ld_res = n + 7).
  * every call runs twice into the same window (the canary re-poisoned, the first result left in place): the second
    result equals the first bit for bit.

Error metric: max|y - epi(ref)| / max|ref| with ref the un-epilogued float64 product, so a large bias or residual cannot
loosen the bound; bias and residual are drawn at the product's own scale.  The tolerance is the path's own (the
caller's), times the activation's largest slope for the GELU / SiLU epilogues (1.13 for tanh-GELU, 1.10 for SiLU:
max |d/dx| of either), plus ACT_EVAL_ERR, the error of evaluating the activation in fp32 at all: measured on the CPU
as float32 numpy against float64 over a reference product and twice that product (the ADD_GELU argument), by

    python -c "from tests import edges; print(edges.measure_act_eval_error())"

which printed {'gelu': 4.38e-08, 'silu': 1.13e-07} (relative to max|product|); ACT_EVAL_ERR is the larger, rounded up
to 2e-7 (a hundredth of the tightest path tolerance, 1e-5).
"""
import numpy as np

from tests.conftest import gpu_available

if gpu_available():
    import torch
    from neural_amd import bestla

CANARY = 0x7FC0BEEF  # a quiet NaN with a payload no arithmetic produces
G = 2                # guard rows above and below an output window
ALIGNS = ("odd", "aligned")
GELU_SLOPE, SILU_SLOPE = 1.13, 1.10
ACT_EVAL_ERR = 2e-7

# name -> (EPI_* name, bias form, residual?, activation)
EPILOGUES = {
    "none": ("EPI_NONE", None, False, None),
    "bias_bcast": ("EPI_BIAS", "bcast", False, None),
    "bias_row": ("EPI_BIAS", "row", False, None),
    "add_gelu_row": ("EPI_ADD_GELU", "row", False, "gelu"),
    "gelu": ("EPI_GELU", None, False, "gelu"),
    "silu": ("EPI_SILU", None, False, "silu"),
    "res_add": ("EPI_RES_ADD", None, True, None),
}


def gelu64(v):
    return 0.5 * v * (1 + np.tanh(0.7978845834732056 * (v + 0.044714998453855515 * v ** 3)))


def silu64(v):
    return v / (1 + np.exp(-v))


def measure_act_eval_error(seed=0):
    """fp32 evaluation error of the two activations, relative to max|product|: float32 numpy against float64 on a
    reference product (uniform activations and weights, K = 1024) and on twice it.  No GPU, no kernel output."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, size=(64, 1024)) @ rng.uniform(-0.5, 0.5, size=(1024, 256))
    out = {}
    for name in ("gelu", "silu"):
        worst = 0.0
        for v in (p, 2 * p):
            x = v.astype(np.float32)
            if name == "gelu":
                one, half = np.float32(1), np.float32(0.5)
                y = half * x * (one + np.tanh(np.float32(0.7978845834732056) *
                                              (x + np.float32(0.044714998453855515) * x * x * x)))
                ref = gelu64(x.astype(np.float64))
            else:
                y = x / (np.float32(1) + np.exp(-x))
                ref = silu64(x.astype(np.float64))
            assert y.dtype == np.float32
            worst = max(worst, float(np.abs(y - ref).max() / np.abs(p).max()))
        out[name] = worst
    return out


# ------------------------------------------------------------------------------------------------ poisoned operands
def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def torch_dtype(act):
    return {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[act]


def round_to(A, act):
    """fp32 numpy values -> (cuda tensor of the activation type, its values as fp32 numpy)"""
    t = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).cuda().to(torch_dtype(act))
    return t, t.float().cpu().numpy()


def act_window(xt, align):
    """xt: contiguous cuda [m][k] of the activation type -> a view of the same values inside NaN padding"""
    m, k = xt.shape
    if align == "odd":
        ld = k + 24
        flat = _nan((1 + m * ld,), xt.dtype)
        win = flat[1:].view(m, ld)[:, 8:8 + k]
    else:
        ld = (k + 7) // 8 * 8 + 32
        win = _nan((m, ld), xt.dtype)[:, :k]
        assert win.data_ptr() % 16 == 0 and (ld * xt.element_size()) % 16 == 0
    win.copy_(xt)
    assert win.stride(0) == ld and win.stride(1) == 1
    return win


def padded(values, pad):
    """fp32 numpy [m][n] -> cuda view [m][n] with row stride n + pad, the padding NaN"""
    m, n = values.shape
    win = _nan((m, n + pad), torch.float32)[:, :n]
    win.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
    return win


class Canary:
    """A canary-filled fp32 buffer and the windows carved from it."""

    def __init__(self, numel):
        self.bits = torch.full((numel,), CANARY, dtype=torch.int32, device="cuda")
        self.f32 = self.bits.view(torch.float32)
        self.windows = []

    def window(self, offset, m, n, ld):
        assert offset >= 0 and offset + (m - 1) * ld + n <= self.f32.numel()
        w = self.f32.as_strided((m, n), (ld, 1), offset)
        self.windows.append(w)
        return w

    def repoison(self):
        """the canary again everywhere but in the windows, which keep what they hold"""
        keep = [w.clone() for w in self.windows]
        self.bits.fill_(CANARY)
        for w, kept in zip(self.windows, keep):
            w.copy_(kept)

    def check(self, what=""):
        """no NaN inside the windows, the canary bit for bit everywhere else"""
        for i, w in enumerate(self.windows):
            bad = int(torch.isnan(w).sum())
            assert bad == 0, f"{what}: {bad} NaN element(s) in output window {i} (unwritten, or NaN read from padding)"
        outside = self.bits.clone()
        ov = outside.view(torch.float32)
        for w in self.windows:
            ov.as_strided(w.shape, w.stride(), w.storage_offset()).view(torch.int32).fill_(CANARY)
        wrong = (outside != CANARY).nonzero().flatten()
        assert wrong.numel() == 0, (f"{what}: {wrong.numel()} element(s) outside the output window overwritten, "
                                    f"first flat indices {wrong[:8].tolist()}")


def out_window(m, n, align):
    """-> (Canary, window [m][n]) with G guard rows above and below and padding columns"""
    if align == "odd":
        ldo, c0 = n + 5, 0
    else:
        ldo = n + 8
        c0 = next(c for c in range(4) if ((G * ldo + c) * 4) % 16 == 0)
    can = Canary((G + m + G) * ldo)
    win = can.window(G * ldo + c0, m, n, ldo)
    if align == "aligned":
        assert win.data_ptr() % 16 == 0
    return can, win


def rel_err(y, ref_epi, prod):
    return float(np.abs(y.astype(np.float64) - ref_epi).max() / max(np.abs(prod).max(), 1e-30))


def epi_tol(tol, activation):
    if activation == "gelu":
        return tol * GELU_SLOPE + ACT_EVAL_ERR
    if activation == "silu":
        return tol * SILU_SLOPE + ACT_EVAL_ERR
    return tol


def twice(can, call, what):
    """run `call` twice into the canary's windows; checks the canary after each and that the second results equal the
    first bit for bit (nothing accumulates into, or depends on, what the windows held).  Returns the windows' values."""
    call()
    torch.cuda.synchronize()
    can.check(what)
    first = [w.clone() for w in can.windows]
    can.repoison()
    call()
    torch.cuda.synchronize()
    can.check(what + " (second call)")
    for i, (w, f) in enumerate(zip(can.windows, first)):
        assert torch.equal(w.view(torch.int32), f.view(torch.int32)), \
            f"{what}: window {i} differs on a second call into its own previous result"
    return [f.cpu().numpy() for f in first]


def check_forward_matrix(w, xt, prod, tol, label, aligns=ALIGNS, epilogues=tuple(EPILOGUES)):
    """Every epilogue x alignment variant of w.forward on the activations xt (contiguous cuda [m][k]) against prod, the
    float64 product of xt's values with the weight; tol is the path's tolerance for the un-epilogued product (a dict by
    alignment variant where the two take different kernels).  Prints each figure before it asserts."""
    m, n = prod.shape
    scale = float(np.abs(prod).max())
    rng = np.random.default_rng(m * 1000 + n)
    b1 = (rng.uniform(-1, 1, size=(n,)) * scale).astype(np.float32)
    b2 = (rng.uniform(-1, 1, size=(m, n)) * scale).astype(np.float32)
    r = (rng.uniform(-1, 1, size=(m, n)) * scale).astype(np.float32)
    b1_t = torch.from_numpy(b1).cuda()
    for align in aligns:
        x = act_window(xt, align)
        b2_t, r_t = padded(b2, 3), padded(r, 7)
        assert b2_t.stride(0) == n + 3 and r_t.stride(0) == n + 7
        for name in epilogues:
            epi, bias_form, has_res, activation = EPILOGUES[name]
            bias = {None: None, "bcast": b1_t, "row": b2_t}[bias_form]
            ref = prod
            if bias_form:
                ref = ref + (b1.astype(np.float64)[None, :] if bias_form == "bcast" else b2.astype(np.float64))
            if has_res:
                ref = ref + r.astype(np.float64)
            if activation:
                ref = gelu64(ref) if activation == "gelu" else silu64(ref)
            can, out = out_window(m, n, align)
            what = f"{label} {align} {name}"
            (y,) = twice(can, lambda: w.forward(x, out=out, epilogue=getattr(bestla, epi), bias=bias,
                                                residual=r_t if has_res else None), what)
            err = rel_err(y, ref, prod)
            bound = epi_tol(tol[align] if isinstance(tol, dict) else tol, activation)
            print(f"{what}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (what, err, bound)
