"""Python mirror of Neural Speed's BesTLA operator surface, backed by the MI355X C-ABI (libneural_amd.so).

Reference entry points mirrored (paths relative to the reference repo root):
  quantize()        <- bestla_quantize          neural_speed/models/model_utils/quant_utils.cpp:269-354
  qpack()           <- bestla_qpack / Model.np_bestla_qpack
                                                quant_utils.cpp:226-266, application/main_pybind.cpp:378-402
  pack_size()       <- BTLAGemmPackBSize        neural_speed/core/layers/bestla_gemm.h:38-39
  unpack()          <- BTLAGemmUnPackB / bestla_unpackweight_fp32
  DeviceWeight      <- bestla_device_load_storage (ne_bestla.h:96; SYCL impl ne_bestla_sycl.cpp:94-144)
  DeviceWeight.forward / f32f32_forward
                    <- bestla_device_f32f32_forward (ne_bestla.h:97-98) / bestla_f32f32_forward (inner_product.cpp:28-36)
  DeviceWeight.get_rows
                    <- ne_get_rows on a quantized tensor (ne_compute_forward_get_rows_q, core/ne_layers.c:8385-8433)
  qkv_forward()     <- bestla_fusion_QKV_f32f32_forward (ip_fusion_qkv.cpp)
  ffn_forward()     <- bestla_fusion_FFN_SiLu_f32f32_forward / _Gelu_Mul_ (ip_fusion_ffn.cpp:734-755)
  ExpertBank / mul_mat_id() / moe_ffn() / moe_route() / moe_gate_route()
                    <- ne_mul_mat_id / ne_mul_id_ffn_silu and the router of models/llama/llama.cpp:620-688
  split()           <- TP weight split of model_files.h:1538-1660 (here exact: no re-quantization)

Device buffers are torch tensors (plumbing only); every arithmetic op on the path runs in the HIP kernels.
"""
import ctypes as C

import numpy as np

from ._lib import check, last_error, lib

# BTLA_DTYPE (bestla/bestla/bestla.h:38-87)
F32, F16, BF16 = 32, 16, 16 | (1 << 16)
S8, S4, S2 = 8 | 0x100, 4 | 0x100, 2 | 0x100
# ne_comp_type (neural_speed/core/data_types.h:57-63)
COMP_UNDEF, COMP_F32, COMP_BF16, COMP_F16, COMP_INT8 = 0, 1, 2, 3, 4
# activation dtypes / epilogues of the native API
ACT_F32, ACT_F16, ACT_BF16 = 0, 1, 2
EPI_NONE, EPI_BIAS, EPI_SILU_MUL, EPI_GELU_MUL, EPI_GELU, EPI_ADD_GELU, EPI_SILU, EPI_RES_ADD = range(8)

S1, S3, S5, S6, S7 = 1 | 0x100, 3 | 0x100, 5 | 0x100, 6 | 0x100, 7 | 0x100
F4_E2M1, F4_BNB, F4_NF4 = 4, 4 | (1 << 16), 4 | (2 << 16)
F8_E4M3, F8_E5M2, F8_E8M0 = 8, 8 | (1 << 16), 8 | (3 << 16)
DQ8_BNB = 8 | (4 << 16)  # double-quantized u8 scale codes + fp32 block absmax / offset (bestla_storage.h:223-231)
# quant_config.h:22-57 parse_bits ("int1" is not supported here); "fp4_bnb" names the F4_BNB type the reference packs
# but has no command-line name for
_WEIGHT_DTYPES = {"int4": S4, "int8": S8, "int2": S2, "int1": S1, "int3": S3, "int5": S5, "int6": S6, "int7": S7,
                  "fp4_e2m1": F4_E2M1, "fp4": F4_E2M1, "nf4": F4_NF4, "fp4_bnb": F4_BNB,
                  "fp8_e4m3": F8_E4M3, "fp8": F8_E4M3, "fp8_e5m2": F8_E5M2}
_SCALE_DTYPES = {"fp32": F32, "bf16": BF16, "fp16": F16, "fp8": F8_E8M0}
_COMP = {"int8": COMP_INT8, "bf16": COMP_BF16, "fp16": COMP_F16, "fp32": COMP_F32, "auto": COMP_UNDEF}
BITS = {S4: 4, S2: 2, S8: 8, S1: 1, S3: 3, S5: 5, S6: 6, S7: 7, F4_E2M1: 4, F4_BNB: 4, F4_NF4: 4, F8_E4M3: 8, F8_E5M2: 8}


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(a.data_ptr())


def _aligned_buffer(size):
    """64-byte aligned, zero-filled uint8 numpy buffer (the blob serializer aligns relative to the base)."""
    raw = np.zeros(size + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + size]


def parse_weight_dtype(s):
    if s not in _WEIGHT_DTYPES:
        raise ValueError(f"unsupported weight_dtype {s!r} (supported: {sorted(_WEIGHT_DTYPES)})")
    return _WEIGHT_DTYPES[s]


def pack_size(n, k, block_size, weight_dtype=S4, scale_dtype=F32, asym=False, comp=COMP_INT8, shuffle=False):
    L = lib()
    dummy = C.c_int(0)
    return L.BTLAGemmPackBSize(n, k, block_size, weight_dtype, scale_dtype, bool(asym), comp,
                               C.byref(dummy) if shuffle else None)


def _quantize_types(weight_dtype, scale_dtype):
    """The BTLA_DTYPE codes bestla_quantize packs with for these names (weight, scale)."""
    qt = parse_weight_dtype(weight_dtype)
    if scale_dtype not in _SCALE_DTYPES:
        raise ValueError(f"unsupported scale_dtype {scale_dtype!r} (supported: {sorted(_SCALE_DTYPES)})")
    st = _SCALE_DTYPES[scale_dtype]
    if qt in (F8_E4M3, F8_E5M2):
        st = F8_E8M0  # quant_utils.cpp:336-341: fp8 weights always get F8_E8M0 shared-exponent scales
    elif st == F8_E8M0:
        st = BF16  # quant_utils.cpp:329-335: anything but fp32 / fp16 is stored as bf16
    return qt, st


def quantize(w_nk, group_size=32, weight_dtype="int4", scale_dtype="fp32", alg="sym", compute_dtype="int8"):
    """bestla_quantize (quant_utils.cpp:269-354): fp32 torch-layout weight [N][K] -> packed BTLA blob (uint8)."""
    w = np.ascontiguousarray(w_nk, dtype=np.float32)
    qt, st = _quantize_types(weight_dtype, scale_dtype)
    gsize = w.shape[1] if group_size == -1 else group_size
    return quant_pack(w, gsize, qt, st, alg == "asym", _COMP[compute_dtype])


def quant_pack(w_nk, block_size, qtype, scale_type, asym, comp):
    """BTLAGemmPackBSize + BTLAGemmQuantPackB on a torch-layout [N][K] weight with BTLA_DTYPE codes (bestla_gemm.cpp);
    unlike quantize() any scale dtype the pack API accepts may be named (e.g. F32 scales for fp8 weights)."""
    w = np.ascontiguousarray(w_nk, dtype=np.float32)
    n, k = w.shape
    gsize, qt, st = block_size, qtype, scale_type
    size = pack_size(n, k, gsize, qt, st, asym, comp)
    if not size:
        raise RuntimeError(f"no packing core for this configuration: {last_error()}")
    blob = _aligned_buffer(size)
    if not lib().BTLAGemmQuantPackB(_ptr(blob), _ptr(w), n, k, k, gsize, qt, st, asym, comp, True, None):
        raise RuntimeError(f"BTLAGemmQuantPackB failed: {last_error()}")
    return blob


def qpack(int_weight, scales, zeros=None, g_idx=None, weight_dtype="int4", group_size=128, alg="sym",
          scale_dtype="fp32", compute_dtype="int8"):
    """bestla_qpack / np_bestla_qpack: pre-quantized int8 [K][N] (+ scales [K/g][N], zeros, g_idx) -> blob.
    As in the reference (quant_utils.cpp:248-254) fp16 scale requests are stored as bf16."""
    q = np.ascontiguousarray(int_weight, dtype=np.int8)
    k, n = q.shape
    s = np.ascontiguousarray(scales, dtype=np.float32)
    asym = alg == "asym"
    z = np.ascontiguousarray(zeros, dtype=np.int8) if (asym and zeros is not None and np.size(zeros)) else None
    gi = np.ascontiguousarray(g_idx, dtype=np.int32) if (g_idx is not None and np.size(g_idx)) else None
    qt = parse_weight_dtype(weight_dtype)
    # "dq8_bnb" (no quant_utils name; the pack API's DQ8_BNB) double-quantizes the given scales at pack time
    st = F32 if scale_dtype == "fp32" else (DQ8_BNB if scale_dtype == "dq8_bnb" else BF16)
    gsize = k if group_size == -1 else group_size
    comp = _COMP[compute_dtype]
    size = pack_size(n, k, gsize, qt, st, asym, comp, gi is not None)
    if not size:
        raise RuntimeError(f"no packing core for this configuration: {last_error()}")
    blob = _aligned_buffer(size)
    if not lib().BTLAGemmPackB(_ptr(blob), _ptr(q), _ptr(s), _ptr(z), n, k, n, gsize, qt, st, asym, comp,
                               _ptr(gi), None):
        raise RuntimeError(f"BTLAGemmPackB failed: {last_error()}")
    return blob


BLOB_FIELDS = ["size", "prologue", "coreid", "npad", "kpad", "n", "k", "dtype", "bs", "scat", "zpt", "redt",
               "cstep", "csize", "asym", "has_reduce", "has_shuffle", "q_off", "q_size", "s_off", "s_size",
               "z_off", "z_size", "r_off", "r_size", "shf_off", "shf_size"]


def blob_info(blob):
    o = np.zeros(27, np.int64)
    check(lib().nad_blob_info(_ptr(blob), _ptr(o)), "nad_blob_info")
    return dict(zip(BLOB_FIELDS, (int(v) for v in o)))


def unpack(blob):
    """BTLAGemmUnPackB: dequantized fp32 [K][N]."""
    inf = blob_info(blob)
    out = np.zeros((inf["k"], inf["n"]), np.float32)
    if not lib().BTLAGemmUnPackB(_ptr(out), _ptr(blob), inf["n"], inf["k"], inf["n"], None):
        raise RuntimeError(f"BTLAGemmUnPackB failed: {last_error()}")
    return out


def split(blob, axis, rank, world, unit=1):
    """Exact TP shard of a blob: axis 0 splits N (TP_1D_ROW) in chunks of `unit` columns, axis 1 splits K by whole
    quantization groups (TP_1D_COLUMN)."""
    L = lib()
    size = L.nad_blob_split(_ptr(blob), axis, rank, world, unit, None, 0)
    if not size:
        raise RuntimeError(f"nad_blob_split failed: {last_error()}")
    out = _aligned_buffer(size)
    if L.nad_blob_split(_ptr(blob), axis, rank, world, unit, _ptr(out), size) != size:
        raise RuntimeError(f"nad_blob_split failed: {last_error()}")
    return out


def split_range(blob, axis, rank, world, unit=1):
    b, e = C.c_int(0), C.c_int(0)
    check(lib().nad_split_range(_ptr(blob), axis, rank, world, unit, C.byref(b), C.byref(e)), "nad_split_range")
    return b.value, e.value


# ---------------------------------------------------------------------------------------------------- device
KERNELS = {1: "woq_gemv_m1_kernel", 2: "woq_gemv_kernel", 3: "woq_skinny_kernel", 4: "woq_i8_kernel",
           5: "woq_gemm3_kernel", 6: "woq_gemm4_kernel", 7: "woq_gemm2_kernel", 8: "woq_gemm_kernel",
           9: "woq_gemm7_kernel", 10: "woq_mid_kernel", 11: "woq_q6k_gemv_kernel", 12: "woq_q6k_gemm_kernel",
           13: "woq_q6k_i8_kernel", 14: "woq_gemv_m1_routed_kernel", 15: "moe_combine_kernel", 16: "moe_sort_kernel",
           17: "nad_cvt_act_kernel", 18: "woq_gemm7_grouped_kernel", 19: "moe_gather_kernel",
           20: "woq_get_rows_kernel", 21: "woq_gemv_routed_kernel", 22: "woq_q6k_gemv_routed_kernel",
           23: "woq_q6k_gemm_grouped_kernel", 24: "moe_gate_route_kernel"}


_SCALE_CODE = {"fp32": 0, "bf16": 1, "fp16": 2}  # ScaleType (woq_layout.h)
_ACT_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}    # ActType: activations, and the rows get_rows writes


def _plan6(entry, *args):
    """One six-value dry-run entry by name, as _plan_dict."""
    o = np.zeros(6, np.int64)
    if getattr(lib(), entry)(*args, _ptr(o), 6) != 6:
        raise RuntimeError(f"{entry} failed: {last_error()}")
    return _plan_dict(o)


def plan_forward(bits, n, k, group_size=128, scale_dtype="fp16", asym=False, m=1, act="fp32"):
    """Which kernel a forward of this geometry launches, with what grid (nad_plan_forward: the host side of the call
    with every launch recorded instead of issued -- no GPU needed)."""
    return _plan6("nad_plan_forward", bits, n, k, group_size, _SCALE_CODE[scale_dtype], int(asym), m, _ACT_CODE[act])


def _gemv_instance(v):
    """The decode GEMV instantiation a dry run's launch statement named (woq_kernels.h: gemv_inst), written as the
    kernel's demangled template-id; None where the call's last main launch was no GEMV."""
    f = lambda at, bits: (v >> at) & ((1 << bits) - 1)
    b = lambda at: "true" if (v >> at) & 1 else "false"
    family, bits, gpt, at = f(0, 2), 1 << f(2, 2), 1 << f(4, 2), f(7, 2)
    ksn, spw, nst, st, nwt, nsc = f(9, 3), f(12, 3), f(15, 2), f(17, 2) - 1, f(20, 2), (0, 7, 11, 16)[f(22, 2)]
    if family == 1:
        return f"woq_gemv_kernel<{bits}, {at}, {gpt}, {b(6)}, {nst}>"
    if family == 2:
        return f"woq_gemv_m1_kernel<{bits}, {gpt}, {at}, {b(6)}, {ksn}, {spw}, {b(19)}, {nst}, {st}>"
    if family == 3:
        return f"woq_gemv_m1s_kernel<{bits}, {gpt}, {at}, {b(6)}, {ksn}, {spw}, {nst}, {st}, {nwt}, {nsc}, {b(24)}>"
    return None


def _plan_dict(o):
    return dict(kernel=KERNELS.get(int(o[0]), str(int(o[0]))), grid=int(o[1]), threads=int(o[2]), ksplit=int(o[3]),
                fold=bool(o[4] & 1), ksw=bool(o[4] & 2), m1_spec=bool(o[4] & 4), ahead=bool(o[4] & 8),
                instance=_gemv_instance(int(o[4]) >> 4), launches=int(o[5]))


def plan_qkv_forward(bits, nq, nk, nv, k, group_size=128, scale_dtype="fp16", asym=False, m=1, act="fp32"):
    """What a fused Q/K/V forward of three weights of this format launches (nad_plan_qkv_forward: no GPU needed): the
    last main launch's kernel, grid, threads, ksplit and flags; `launches` counts every launch of the call."""
    return _plan6("nad_plan_qkv_forward", bits, nq, nk, nv, k, group_size, _SCALE_CODE[scale_dtype], int(asym), m,
                  _ACT_CODE[act])


def plan_qkv(wq, wk, wv, m, act="fp32"):
    """The same dry run for three DeviceWeights or plan_only_weight descriptors (nad_plan_qkv)."""
    return _plan6("nad_plan_qkv", *(getattr(w, "desc", w) for w in (wq, wk, wv)), m, _ACT_CODE[act])


def plan_gate_up_forward(bits, n, k, group_size=128, scale_dtype="fp16", asym=False, m=1, act="fp32"):
    """What the FFN's fused gate/up (SiLU * mul) of two weights of this format launches (nad_plan_gate_up_forward: no
    GPU needed); the record is plan_qkv_forward's."""
    return _plan6("nad_plan_gate_up_forward", bits, n, k, group_size, _SCALE_CODE[scale_dtype], int(asym), m,
                  _ACT_CODE[act])


def plan_gate_up(w1, w3, m, act="fp32"):
    """The same dry run for two loaded DeviceWeights (nad_plan_gate_up)."""
    return _plan6("nad_plan_gate_up", w1.desc, w3.desc, m, _ACT_CODE[act])


def plan_only_weight(bits, n, k, group_size=128, scale_dtype="fp16", asym=False, act_order=False):
    """A geometry-only weight descriptor for the dry runs (nad_weight_plan_only: no GPU needed, holds no weights);
    bits 6 is GGUF Q6_K."""
    L = lib()
    desc = (C.c_uint8 * L.bestla_device_storage_size())()
    check(L.nad_weight_plan_only(bits, n, k, group_size, _SCALE_CODE[scale_dtype], int(asym), int(act_order), desc),
          "nad_weight_plan_only")
    return desc


def _plan_get_rows(desc, m, dtype="fp32"):
    return _plan6("nad_plan_get_rows", desc, m, _ACT_CODE[dtype])


def plan_get_rows(desc, m, dtype="fp32"):
    """What get_rows of m ids on this descriptor (plan_only_weight's, or a DeviceWeight's .desc) launches: kernel, grid
    and threads (nad_plan_get_rows -- no GPU needed)."""
    return _plan_get_rows(desc, m, dtype)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("neural_amd device ops need a ROCm GPU (torch.cuda.is_available() is False)")
    return torch


def _stream(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


_ACT = {}


def _act_code(t):
    torch = _torch()
    if not _ACT:
        _ACT.update({torch.float32: ACT_F32, torch.float16: ACT_F16, torch.bfloat16: ACT_BF16})
    if t.dtype not in _ACT:
        raise TypeError(f"activation dtype {t.dtype} not supported (float32/float16/bfloat16)")
    return _ACT[t.dtype]


class DeviceWeight:
    """A WOQ weight resident in HBM in the MFMA tile layout (woq_layout.h); the reference's ne_tensor device
    storage: `desc` plays the role of the embedded descriptor (devstor), `mem` of the device buffer."""

    def __init__(self, blob=None, device=None, stream=None, _desc=None, _mem=None):
        torch = _torch()
        L = lib()
        self.desc = (C.c_uint8 * L.bestla_device_storage_size())()
        if blob is not None:
            blob = np.ascontiguousarray(blob)
            need = L.nad_device_weight_size(_ptr(blob))
            if not need:
                raise RuntimeError(f"unsupported blob: {last_error()}")
            self.mem = torch.empty(need, dtype=torch.uint8, device=device or "cuda")
            check(L.nad_device_load(_ptr(blob), self.desc, _ptr(self.mem), need, _stream(stream)),
                  "nad_device_load")
        else:
            self.mem = _mem
            C.memmove(self.desc, _desc, len(self.desc))
        o = np.zeros(13, np.int64)
        if L.nad_weight_info2(self.desc, _ptr(o), 13) != 13:
            raise RuntimeError(f"nad_weight_info2 failed: {last_error()}")
        (_, self.bits, self.n, self.k, self.blocksize, self.ns, self.nt, self.ng, self.scale_t, self.asym,
         self.has_shuffle, self.bytes, self.fold_ok) = (int(v) for v in o)

    @classmethod
    def synthetic(cls, bits, n, k, group_size=128, scale_dtype="fp16", asym=False, seed=0, device=None, stream=None):
        torch = _torch()
        L = lib()
        st = _SCALE_CODE[scale_dtype]
        need = L.nad_synthetic_weight_size(bits, n, k, group_size, st, int(asym))
        mem = torch.empty(need, dtype=torch.uint8, device=device or "cuda")
        desc = (C.c_uint8 * L.bestla_device_storage_size())()
        check(L.nad_synthetic_weight(desc, _ptr(mem), need, bits, n, k, group_size, st, int(asym), seed,
                                     _stream(stream)), "nad_synthetic_weight")
        return cls(_desc=desc, _mem=mem)

    @classmethod
    def _from_blocks(cls, size_fn, load_fn, load_name, block_bytes, block_elems, blocks, n, k, device, stream):
        """n rows of k / block_elems GGUF blocks through one pair of C entries: size_fn(n, k) and load_fn(blocks, n, k,
        desc, mem, capacity, queue)"""
        torch = _torch()
        need = size_fn(n, k)
        if not need:
            raise RuntimeError(last_error())
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        assert blocks.size == n * (k // block_elems) * block_bytes, (blocks.size, n, k, block_bytes)
        mem = torch.empty(need, dtype=torch.uint8, device=device or "cuda")
        desc = (C.c_uint8 * lib().bestla_device_storage_size())()
        check(load_fn(_ptr(blocks), n, k, desc, _ptr(mem), need, _stream(stream)), load_name)
        return cls(_desc=desc, _mem=mem)

    @classmethod
    def from_q4_0(cls, blocks, n, k, device=None, stream=None):
        """A GGUF Q4_0 matrix (n rows of k/32 block_q4_0, as an NE_TYPE_Q4_0 ne_tensor holds it) in the device tile
        layout (nad_q4_0_device_load)."""
        L = lib()
        return cls._from_blocks(L.nad_q4_0_device_size, L.nad_q4_0_device_load, "nad_q4_0_device_load", 18, 32, blocks,
                                n, k, device, stream)

    @classmethod
    def from_gguf(cls, type, blocks, n, k, device=None, stream=None):
        """A GGUF matrix of one of the legacy block types (GGUF_Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0: n rows of k/32 blocks,
        as an ne_tensor of that NE_TYPE holds it) in the device tile layout (nad_gguf_device_load); GGUF_Q6_K goes to
        from_q6_k."""
        type = int(type)
        if type == GGUF_Q6_K:  # superblocks of 256: entries of its own
            return cls.from_q6_k(blocks, n, k, device=device, stream=stream)
        L = lib()
        bb = L.nad_gguf_block_bytes(type)
        if not bb:
            raise RuntimeError(last_error())
        return cls._from_blocks(lambda n, k: L.nad_gguf_device_size(type, n, k),
                                lambda *a: L.nad_gguf_device_load(type, *a), "nad_gguf_device_load", bb, 32, blocks, n,
                                k, device, stream)

    @classmethod
    def from_q6_k(cls, blocks, n, k, device=None, stream=None):
        """A GGUF Q6_K matrix (n rows of k/256 block_q6_K of 210 bytes, as an NE_TYPE_Q6_K ne_tensor holds it) in its
        own device layout at 6.5625 bits per weight (nad_q6_k_device_load)."""
        L = lib()
        return cls._from_blocks(L.nad_q6_k_device_size, L.nad_q6_k_device_load, "nad_q6_k_device_load", 210, 256, blocks,
                                n, k, device, stream)

    @classmethod
    def quantize(cls, w, group_size=32, weight_dtype="int4", scale_dtype="fp32", alg="sym", compute_dtype="int8",
                 return_blob=False, stream=None):
        """bestla.quantize + DeviceWeight for a weight that already sits in HBM (nad_device_quantize): w is a cuda
        tensor [N][K] fp32 / fp16 / bf16 with K contiguous (a row stride is honoured), quantized, packed and laid out by
        HIP kernels, byte-identical to the host path.  int4 / int2 / int8 weights with fp32 / bf16 / fp16 scales;
        anything else raises and stays on the host path.  Returns the DeviceWeight, or (DeviceWeight, blob) with the
        blob bestla.quantize would return when return_blob is true."""
        torch = _torch()
        L = lib()
        if w.dim() != 2 or not w.is_cuda or w.stride(1) != 1:
            raise ValueError("DeviceWeight.quantize takes a cuda tensor [N][K] with K contiguous")
        n, k = w.shape
        qt, st = _quantize_types(weight_dtype, scale_dtype)
        gsize = k if group_size == -1 else group_size
        asym, comp = int(alg == "asym"), _COMP[compute_dtype]
        bsz = C.c_size_t(0)
        need = L.nad_device_quantize_size(n, k, gsize, qt, st, asym, comp, C.byref(bsz))
        if not need:
            raise RuntimeError(f"nad_device_quantize_size failed: {last_error()}")
        blob = _aligned_buffer(bsz.value) if return_blob else None
        mem = torch.empty(need, dtype=torch.uint8, device=w.device)
        desc = (C.c_uint8 * L.bestla_device_storage_size())()
        with torch.cuda.device(w.device):
            check(L.nad_device_quantize(_ptr(w), _act_code(w), n, k, w.stride(0), gsize, qt, st, asym, comp, desc,
                                        _ptr(mem), need, _ptr(blob), bsz.value if return_blob else 0, _stream(stream)),
                  "nad_device_quantize")
        dw = cls(_desc=desc, _mem=mem)
        return (dw, blob) if return_blob else dw

    def forward(self, x, out=None, epilogue=EPI_NONE, bias=None, residual=None, stream=None):
        """out[m][n] = epi(sum_k x[m][k] * W[n][k]); x: cuda [M][K] fp32/fp16/bf16 (row stride honoured)."""
        torch = _torch()
        m, k = x.shape
        assert k == self.k, (k, self.k)
        if out is None:
            out = torch.empty((m, self.n), dtype=torch.float32, device=x.device)
        bias_ld = 0 if bias is None or bias.dim() == 1 else bias.stride(0)
        check(lib().nad_device_forward(_ptr(x), _act_code(x), self.desc, _ptr(out), m, self.n, k, x.stride(0),
                                       out.stride(0), epilogue, _ptr(bias), bias_ld, _ptr(residual),
                                       residual.stride(0) if residual is not None else 0, _stream(stream)),
              "nad_device_forward")
        return out

    __call__ = forward

    def plan(self, m, act="fp32"):
        """which kernel a forward of m rows launches (nad_plan_weight: a dry run, nothing is launched)"""
        return _plan6("nad_plan_weight", self.desc, m, _ACT_CODE[act])

    def get_rows(self, ids, out=None, dtype=None, stream=None):
        """ne_get_rows (nad_device_get_rows): out[r][0:k] = the dequantized weight row ids[r], bit for bit the columns
        of unpack().  ids: an int32 cuda tensor, contiguous or a strided 1-D view (one column of an [m][top_k] table);
        read on the device, so a captured call follows ids as it is rewritten.  An id outside [0, n) gives a row of
        +0.0.  out: [m][>= k] fp32 / fp16 / bf16 with 16-byte aligned rows (default: a new [m][k] tensor of dtype,
        fp32 when not given).  One launch, no synchronisation."""
        torch = _torch()
        if ids.dim() != 1 or ids.dtype != torch.int32 or not ids.is_cuda:
            raise ValueError("get_rows takes a 1-D int32 cuda tensor of row ids")
        m = ids.shape[0]
        if out is None:
            ld = -(-self.k // 8) * 8  # whole 16-byte stores for every output type
            out = torch.empty((m, ld), dtype=dtype or torch.float32, device=ids.device)[:, :self.k]
        elif dtype is not None and out.dtype != dtype:
            raise TypeError(f"out is {out.dtype}, dtype asks for {dtype}")
        if out.dim() != 2 or out.shape[0] != m or out.shape[1] != self.k or out.stride(1) != 1:
            raise ValueError(f"out must be [{m}][{self.k}] with contiguous rows")
        # the strides of a single row are never applied
        stride = ids.stride(0) if m > 1 else 1
        ldo = out.stride(0) if m > 1 else -(-self.k // 8) * 8
        check(lib().nad_device_get_rows(self.desc, _ptr(ids), stride, m, _ptr(out), _act_code(out), ldo,
                                        _stream(stream)), "nad_device_get_rows")
        return out

    def plan_get_rows(self, m, dtype="fp32"):
        """what get_rows of m ids launches (nad_plan_get_rows: a dry run, nothing is launched, no GPU needed)"""
        return _plan_get_rows(self.desc, m, dtype)

    def set_compute(self, mode):
        """Per-weight arithmetic (nad_device_set_compute): None / -1 follow the thread / process mode, COMPUTE_FP,
        COMPUTE_INT8 (integer-core blobs and the legacy GGUF block types only; other weights stay fp) or COMPUTE_Q8_K
        (a GGUF Q6_K weight only -- any other weight raises and keeps its mode: the reference's Q8_K activation rows
        and integer dot product, woq_q6k_i8_kernel at every M)."""
        check(lib().nad_device_set_compute(self.desc, -1 if mode is None else int(mode)), "nad_device_set_compute")
        return self

    @property
    def compute(self):
        """the arithmetic a forward takes now: COMPUTE_FP, COMPUTE_INT8 or COMPUTE_Q8_K"""
        return lib().nad_device_get_compute(self.desc)

    def unpack(self, stream=None):
        """dequantized fp32 [K][N] read back from the device tile layout (repack exactness check)."""
        out = np.zeros((self.k, self.n), np.float32)
        check(lib().nad_device_unpack_fp32(self.desc, _ptr(out), _stream(stream)), "nad_device_unpack_fp32")
        return out


COMPUTE_FP, COMPUTE_INT8 = 0, 1
COMPUTE_Q8_K = 2  # a GGUF Q6_K weight's own mode (DeviceWeight.set_compute): the reference's Q8_K integer arithmetic
# GGUF block types (the reference's ne_type values, neural_speed/core/data_types.h)
GGUF_Q4_0, GGUF_Q4_1, GGUF_Q5_0, GGUF_Q5_1, GGUF_Q8_0 = 2, 3, 6, 7, 8
GGUF_Q6_K = 14  # superblocks of 256 (DeviceWeight.from_q6_k; from_gguf routes it there)


def set_compute_mode(mode):
    """0 (fp16 MFMA on exact weights, default) or 1: the reference's comp_int8 arithmetic for weights packed for an
    integer core (u8 activations per (row, block), s32 block dots, kblock fp32 combine).  Returns the previous mode."""
    L = lib()
    prev = L.nad_get_compute_mode()
    check(L.nad_set_compute_mode(int(mode)), "nad_set_compute_mode")
    return prev


def get_compute_mode():
    return lib().nad_get_compute_mode()


def set_thread_compute_mode(mode):
    """Per-thread override of the process mode (None / -1 clears it)."""
    check(lib().nad_set_thread_compute_mode(-1 if mode is None else int(mode)), "nad_set_thread_compute_mode")


def quant_u8_colblock(x, blocksize, stream=None):
    """kernel::wrapper::QuantizeU8ColBlock (kernel_wrapper.h:571-590) on the GPU: x cuda [M][K] fp32/fp16/bf16 ->
    (q u8 [M][K], scales f32 [M][nblk], zero points u8 [M][nblk], block reduce f32 [M][nblk])."""
    torch = _torch()
    m, k = x.shape
    nblk = -(-k // blocksize)
    q = torch.empty((m, k), dtype=torch.uint8, device=x.device)
    s = torch.empty((m, nblk), dtype=torch.float32, device=x.device)
    z = torch.empty((m, nblk), dtype=torch.uint8, device=x.device)
    red = torch.empty((m, nblk), dtype=torch.float32, device=x.device)
    check(lib().nad_quant_u8_colblock(_ptr(x), _act_code(x), m, k, x.stride(0), blocksize, _ptr(q), k, _ptr(s),
                                      _ptr(z), nblk, _ptr(red), _stream(stream)), "nad_quant_u8_colblock")
    return q, s, z, red


def quant_q8_0(x, stream=None):
    """quantize_row_q8_0 (vectors/cpu/quantize.h:422-445) on the GPU: x cuda [M][K] -> uint8 [M][K/32 * 34] blocks"""
    torch = _torch()
    m, k = x.shape
    out = torch.empty((m, k // 32 * 34), dtype=torch.uint8, device=x.device)
    check(lib().nad_quant_q8_0(_ptr(x), _act_code(x), m, k, x.stride(0), _ptr(out), _stream(stream)), "nad_quant_q8_0")
    return out


def quant_q8_1(x, stream=None):
    """quantize_row_q8_1_reference (vectors/cpu/quantize.h:546-579) on the GPU: x cuda [M][K] -> uint8 [M][K/32 * 40]
    blocks {float d; float s; int8 qs[32]}"""
    torch = _torch()
    m, k = x.shape
    out = torch.empty((m, k // 32 * 40), dtype=torch.uint8, device=x.device)
    check(lib().nad_quant_q8_1(_ptr(x), _act_code(x), m, k, x.stride(0), _ptr(out), _stream(stream)), "nad_quant_q8_1")
    return out


def quant_q8_k(x, stream=None):
    """quantize_row_q8_K_reference (vectors/cpu/quantize.h:1020-1055) on the GPU: x cuda [M][K], K % 256 == 0 -> uint8
    [M][K/256 * 292] blocks {float d; int8 qs[256]; int16 bsums[16]}"""
    torch = _torch()
    m, k = x.shape
    out = torch.empty((m, k // 256 * 292), dtype=torch.uint8, device=x.device)
    check(lib().nad_quant_q8_k(_ptr(x), _act_code(x), m, k, x.stride(0), _ptr(out), _stream(stream)), "nad_quant_q8_k")
    return out


def f32f32_forward(activation, weight, output, m, n, k, lda, ldo, stream=None):
    """bestla_device_f32f32_forward with raw device tensors (void result; errors via last_error)."""
    L = lib()
    L.nad_clear_error()
    L.bestla_device_f32f32_forward(_ptr(activation), weight.desc, _ptr(output), m, n, k, lda, ldo, None,
                                   _stream(stream))
    err = last_error()
    if err:
        raise RuntimeError(err)
    return output


def qkv_forward(x, wq, wk, wv, out=None, stream=None):
    """Fused Q/K/V: returns (q, k, v) fp32, written into out[3][M][N] when given (reference layout)."""
    torch = _torch()
    m = x.shape[0]
    if out is None:
        oq = torch.empty((m, wq.n), dtype=torch.float32, device=x.device)
        ok = torch.empty((m, wk.n), dtype=torch.float32, device=x.device)
        ov = torch.empty((m, wv.n), dtype=torch.float32, device=x.device)
    else:
        oq, ok, ov = out[0], out[1], out[2]
    check(lib().nad_device_qkv_forward(_ptr(x), _act_code(x), wq.desc, wk.desc, wv.desc, _ptr(oq), _ptr(ok),
                                       _ptr(ov), m, x.shape[1], x.stride(0), oq.stride(0), ok.stride(0),
                                       ov.stride(0), _stream(stream)), "nad_device_qkv_forward")
    return oq, ok, ov


def ffn_gate_up(x, w1, w3, act="silu", tmp1=None, tmp2=None, stream=None):
    """Gate/up half of the fused FFN: tmp2 = act(x.W1^T) * (x.W3^T), tmp1 = act(x.W1^T) (ip_fusion_ffn.cpp:407-433).
    tmp1 may be None at M <= 16 (decode: one dual-weight launch); the prefill path needs it."""
    torch = _torch()
    m, fin = x.shape
    fmid = w1.n
    if tmp1 is None and m > 16:
        tmp1 = torch.empty((m, fmid), dtype=torch.float32, device=x.device)
    tmp2 = torch.empty((m, fmid), dtype=torch.float32, device=x.device) if tmp2 is None else tmp2
    epi = EPI_SILU_MUL if act == "silu" else EPI_GELU_MUL
    check(lib().nad_device_ffn_gate_up(_ptr(x), _act_code(x), w1.desc, w3.desc, _ptr(tmp1), _ptr(tmp2), m, fin, fmid,
                                       x.stride(0), epi, _stream(stream)), "nad_device_ffn_gate_up")
    return tmp2


def ffn_forward(x, w1, w2, w3, act="silu", tmp1=None, tmp2=None, out=None, stream=None):
    """Fused FFN: out = (act(x.W1^T) * (x.W3^T)) . W2^T  (ip_fusion_ffn.cpp:407-457)."""
    torch = _torch()
    m, fin = x.shape
    fmid, fout = w1.n, w2.n
    dev = x.device
    tmp1 = torch.empty((m, fmid), dtype=torch.float32, device=dev) if tmp1 is None else tmp1
    tmp2 = torch.empty((m, fmid), dtype=torch.float32, device=dev) if tmp2 is None else tmp2
    out = torch.empty((m, fout), dtype=torch.float32, device=dev) if out is None else out
    epi = EPI_SILU_MUL if act == "silu" else EPI_GELU_MUL
    check(lib().nad_device_ffn_forward(_ptr(x), _act_code(x), w1.desc, w2.desc, w3.desc, _ptr(tmp1), _ptr(tmp2),
                                       _ptr(out), m, fin, fmid, fout, x.stride(0), epi, _stream(stream)),
          "nad_device_ffn_forward")
    return out


class Batch:
    """Independent M = 1 problems y_i = x_i W_i of one weight shape as ONE launch (include/neural_amd.h nad_batch_*:
    BTLAGemmBatchDriver, bestla_gemm.cpp:508-624, for device tensors).  problems: list of (DeviceWeight, x [K] or [1][K]
    fp32 cuda tensor, y [N] or [1][N] fp32 cuda tensor); the tensors are bound at creation (keep them alive)."""

    class _P(C.Structure):
        _fields_ = [("weight", C.c_void_p), ("act", C.c_void_p), ("out", C.c_void_p)]

    def __init__(self, problems):
        arr = (Batch._P * len(problems))()
        self._keep = []
        for i, (w, x, y) in enumerate(problems):
            arr[i].weight = C.cast(w.desc, C.c_void_p)
            arr[i].act = x.data_ptr()
            arr[i].out = y.data_ptr()
            self._keep.extend((w, x, y))
        self._arr = arr
        h = lib().nad_batch_create(C.cast(arr, C.c_void_p), len(problems))
        if not h:
            raise RuntimeError(f"nad_batch_create failed: {last_error()}")
        self.handle = h

    def run(self, stream=None):
        check(lib().nad_batch_run(self.handle, _stream(stream)), "nad_batch_run")

    def plan(self):
        """what run() launches (nad_plan_batch: a dry run, nothing is launched)"""
        return _plan6("nad_plan_batch", self.handle)

    @staticmethod
    def plan_only(desc, n):
        """what a batch of n problems on this weight launches; desc: plan_only_weight's descriptor or a DeviceWeight
        (nad_plan_batch_only -- no GPU needed)"""
        return _plan6("nad_plan_batch_only", getattr(desc, "desc", desc), n)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().nad_batch_destroy(h)
            except Exception:
                pass
            self.handle = None


# ---------------------------------------------------------------------------------------------------- routed experts
BANK_GENERAL = 1  # NAD_BANK_GENERAL


class ExpertBank:
    """The expert weights of one matmul of a Mixtral-style FFN layer (include/neural_amd.h nad_expert_bank_*): a list of
    DeviceWeights of one shape and format, held as one device table the routed kernel indexes with ids it reads on the
    device.  The weights are kept alive with the bank.  general=True (NAD_BANK_GENERAL) also takes the weights the
    stripe-stream GEMV runs at M = 1 and the M = 1 stream does not -- int4 groups of 32 sym, int8 (GGUF Q4_0, Q5_0,
    Q8_0) -- served by woq_gemv_routed_kernel, and a list whose weights are all GGUF Q6_K, served by
    woq_q6k_gemv_routed_kernel (grouped: woq_q6k_gemm_grouped_kernel); route is 0 for the M = 1 stream, 1 for the
    stripe stream, 2 for Q6_K (bits 6, blocksize 16)."""

    def __init__(self, weights, general=False, _handle=None):
        self._keep = list(weights)
        if _handle is None:
            arr = (C.c_void_p * len(self._keep))(*[C.cast(w.desc, C.c_void_p) for w in self._keep])
            if general:
                _handle = lib().nad_expert_bank_create_ex(arr, len(self._keep), BANK_GENERAL)
            else:
                _handle = lib().nad_expert_bank_create(arr, len(self._keep))
            if not _handle:
                raise RuntimeError(f"nad_expert_bank_create{'_ex' if general else ''} failed: {last_error()}")
        self.handle = _handle
        o = np.zeros(9, np.int64)
        if lib().nad_expert_bank_info(self.handle, _ptr(o), 9) != 9:
            raise RuntimeError(f"nad_expert_bank_info failed: {last_error()}")
        (self.n_expert, self.bits, self.n, self.k, self.blocksize, self.scale_t, self.asym, self.has_weights,
         self.route) = (int(v) for v in o)

    @classmethod
    def plan_only(cls, geometries, general=False):
        """A geometry-only bank for plan_moe (no GPU needed, the same checks as a real bank): geometries is a list of
        (bits, n, k, group_size, scale_dtype, asym) per expert; bits 6 names GGUF Q6_K."""
        g = np.array([[b, n, k, gs, _SCALE_CODE[st], int(asym)] for b, n, k, gs, st, asym in geometries], np.int32)
        if general:
            h = lib().nad_expert_bank_plan_only_ex(_ptr(g), len(g), BANK_GENERAL)
        else:
            h = lib().nad_expert_bank_plan_only(_ptr(g), len(g))
        if not h:
            raise RuntimeError(f"nad_expert_bank_plan_only{'_ex' if general else ''} failed: {last_error()}")
        return cls([], _handle=h)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().nad_expert_bank_destroy(h)
            except Exception:
                pass
            self.handle = None


def mul_mat_id(bank, x, ids, slot, out=None, stream=None):
    """ne_mul_mat_id: out[r] = x[r] . W[ids[r][slot]]^T in one launch; x cuda fp32 [M][K], ids cuda int32 [M][>slot],
    read on the device (an id outside the bank gives a zero row)."""
    torch = _torch()
    m, k = x.shape
    assert k == bank.k, (k, bank.k)
    assert ids.dtype == torch.int32 and ids.shape[0] == m, (ids.dtype, ids.shape)
    if out is None:
        out = torch.empty((m, bank.n), dtype=torch.float32, device=x.device)
    check(lib().nad_device_mul_mat_id(bank.handle, _ptr(x), _ptr(ids), ids.stride(0), slot, _ptr(out), m, x.stride(0),
                                      out.stride(0), _stream(stream)), "nad_device_mul_mat_id")
    return out


_MOE_WS = {}


def moe_workspace(m, top_k, fmid, fout, device, stream=None):
    """The fp32 workspace moe_ffn uses when the caller gives none, with its two row blocks: (buffer, t [m * top_k][fmid],
    y [m * top_k][fout]).  One buffer per (shape, device, stream), kept for the life of the process: calls on one stream
    are ordered and may share it, calls on different streams get their own.  It is allocated at the first call of its
    key, so make that call outside graph capture (a buffer first allocated inside a capture would come from the
    graph's private pool and outlive it here), or pass moe_ffn a workspace of your own."""
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    key = (m, top_k, fmid, fout, str(device), int(s.cuda_stream))
    if key not in _MOE_WS:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("moe_ffn: the first call of a shape on a stream allocates its workspace; make it outside "
                               "graph capture or pass workspace=")
        _MOE_WS[key] = moe_workspace_alloc(m, top_k, fmid, fout, device)
    return (_MOE_WS[key],) + moe_workspace_rows(_MOE_WS[key], m, top_k, fmid, fout)


def moe_workspace_alloc(m, top_k, fmid, fout, device="cuda"):
    """A workspace of nad_moe_workspace_size(m, top_k, fmid, fout) bytes for moe_ffn(..., workspace=)."""
    torch = _torch()
    return torch.empty(lib().nad_moe_workspace_size(m, top_k, fmid, fout) // 4, dtype=torch.float32, device=device)


def moe_workspace_rows(ws, m, top_k, fmid, fout):
    """The two row blocks of a moe_ffn workspace: (t [m * top_k][fmid], y [m * top_k][fout]) as views."""
    p = m * top_k
    off = (p * fmid * 4 + 255) // 256 * 64
    return ws[:p * fmid].view(p, fmid), ws[off:off + p * fout].view(p, fout)


def moe_ffn(gate, up, down, x, ids, wts, act="silu", out=None, stream=None, workspace=None):
    """The routed FFN of llama.cpp:641-679 in three launches, four with Q6_K gate / up banks (nad_device_moe_ffn): out[r] = sum_i wts[r][i] *
    ((act(x_r . G_e^T) * (x_r . U_e^T)) . D_e^T), e = ids[r][i], slots summed in order.  gate / up / down: ExpertBanks;
    ids int32 [M][top_k] and wts fp32 [M][top_k] cuda tensors (row strides honoured), read on the device.  workspace: an
    fp32 cuda tensor of at least nad_moe_workspace_size bytes (moe_workspace_alloc) that no concurrent call uses; None
    takes the one moe_workspace holds for this shape and stream."""
    torch = _torch()
    m, fin = x.shape
    top_k = ids.shape[1]
    assert fin == gate.k and ids.dtype == torch.int32 and wts.dtype == torch.float32
    assert ids.shape[0] == m and tuple(wts.shape) == (m, top_k), (ids.shape, wts.shape)
    if out is None:
        out = torch.empty((m, down.n), dtype=torch.float32, device=x.device)
    if workspace is None:
        workspace = moe_workspace(m, top_k, gate.n, down.n, x.device, stream)[0]
    need = lib().nad_moe_workspace_size(m, top_k, gate.n, down.n)
    assert workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() * 4 >= need, need
    ws = workspace
    epi = EPI_SILU_MUL if act == "silu" else EPI_GELU_MUL
    check(lib().nad_device_moe_ffn(gate.handle, up.handle, down.handle, _ptr(x), _ptr(ids), ids.stride(0), _ptr(wts),
                                   wts.stride(0), top_k, epi, _ptr(ws), _ptr(out), m, x.stride(0), out.stride(0),
                                   _stream(stream)), "nad_device_moe_ffn")
    return out


def moe_route(logits, top_k, stream=None):
    """The router (nad_moe_route): softmax of each row of logits (cuda fp32 [M][n_expert <= 64]), the top_k experts
    in descending order (a tie to the lower index) and their weights renormalised to sum 1 -> (ids int32, wts fp32)."""
    torch = _torch()
    m, ne = logits.shape
    ids = torch.empty((m, top_k), dtype=torch.int32, device=logits.device)
    wts = torch.empty((m, top_k), dtype=torch.float32, device=logits.device)
    check(lib().nad_moe_route(_ptr(logits), logits.stride(0), m, ne, top_k, _ptr(ids), top_k, _ptr(wts), top_k,
                              _stream(stream)), "nad_moe_route")
    return ids, wts


def moe_gate_route(x, gate, top_k, *, return_logits=False, stream=None):
    """The router from the hidden state in one launch (nad_moe_gate_route): logits = x . gate^T in the order the header
    defines -- a function of the row, the gate and K alone, whatever M -- then moe_route's arithmetic on them.  x cuda
    fp32 [M][K]; gate cuda [n_expert <= 64][K], float32, float16 or bfloat16 (the unquantized ffn_gate_inp.weight); row
    strides honoured (multiples of 4, 16-byte aligned bases) -> (ids int32 [M][top_k], wts fp32 [M][top_k]), and the
    logits fp32 [M][n_expert] with return_logits."""
    torch = _torch()
    m, k = x.shape
    ne, kw = gate.shape
    if x.dtype != torch.float32 or kw != k or x.stride(1) != 1 or gate.stride(1) != 1:
        raise TypeError(f"moe_gate_route: x must be float32 [M][K] and gate [n_expert][K], rows contiguous "
                        f"(x {x.dtype} {tuple(x.shape)}, gate {tuple(gate.shape)})")
    ids = torch.empty((m, top_k), dtype=torch.int32, device=x.device)
    wts = torch.empty((m, top_k), dtype=torch.float32, device=x.device)
    logits = torch.empty((m, ne), dtype=torch.float32, device=x.device) if return_logits else None
    check(lib().nad_moe_gate_route(_ptr(x), x.stride(0), _ptr(gate), _act_code(gate), gate.stride(0), m, k, ne, top_k,
                                   _ptr(ids), top_k, _ptr(wts), top_k, _ptr(logits), ne, _stream(stream)),
          "nad_moe_gate_route")
    return (ids, wts, logits) if return_logits else (ids, wts)


def plan_moe_gate_route(m, k, n_expert, top_k, gate_dtype="fp32"):
    """What moe_gate_route launches for m rows (nad_plan_moe_gate_route: no launch, no GPU needed):
    dict(kernel, grid, threads, lds, launches)."""
    o = np.zeros(5, np.int64)
    if lib().nad_plan_moe_gate_route(m, k, n_expert, top_k, _ACT_CODE[gate_dtype], _ptr(o), 5) != 5:
        raise RuntimeError(f"nad_plan_moe_gate_route failed: {last_error()}")
    return dict(kernel=KERNELS.get(int(o[0]), str(int(o[0]))), grid=int(o[1]), threads=int(o[2]), lds=int(o[3]),
                launches=int(o[4]))


def plan_moe(gate, up, down, m, top_k):
    """What moe_ffn launches for m rows (nad_plan_moe: no launch, no GPU needed; plan-only banks qualify): a list of
    dict(kernel, grid, threads, lds), one per launch."""
    o = np.zeros(17, np.int64)
    c = lib().nad_plan_moe(gate.handle, up.handle, down.handle, m, top_k, _ptr(o), 17)
    if c not in (13, 17):  # three launches, or four with Q6_K gate / up banks (gate and up apart)
        raise RuntimeError(f"nad_plan_moe failed: {last_error()}")
    n = int(o[c - 1])
    assert c == 4 * n + 1, (c, n)
    return [dict(kernel=KERNELS.get(int(o[4 * i]), str(int(o[4 * i]))), grid=int(o[4 * i + 1]),
                 threads=int(o[4 * i + 2]), lds=int(o[4 * i + 3])) for i in range(n)]


# ------------------------------------------------------------------------------------- routed experts, sorted and grouped
def _h(bank):
    return bank.handle if bank is not None else None


def moe_grouped_workspace_size(gate, up, down, m, top_k):
    """nad_moe_grouped_workspace_size: bytes; up = down = None sizes the one-matmul form (top_k = 1)."""
    return int(lib().nad_moe_grouped_workspace_size(_h(gate), _h(up), _h(down), m, top_k))


def moe_grouped_workspace_alloc(gate, up, down, m, top_k, device="cuda"):
    """A workspace (uint8 cuda tensor) for moe_ffn_grouped(..., workspace=), or with up = down = None for
    mul_mat_id_grouped.  torch's allocations are 256-byte aligned, which the entries' 16 bytes need."""
    torch = _torch()
    size = moe_grouped_workspace_size(gate, up, down, m, top_k)
    if size == 0:
        raise RuntimeError(f"nad_moe_grouped_workspace_size failed: {last_error()}")
    return torch.empty(size, dtype=torch.uint8, device=device)


def moe_grouped_workspace_rows(ws, gate, up, down, m, top_k):
    """Views into a grouped workspace by the layout of include/neural_amd.h: dict(perm int32 [np], offs int32
    [n_expert + 1], inv int32 [np], src int32 [np], ntiles int32 [1], tiles int32 [bound][4], x16 fp16 [m][kp], y fp32
    [np][fout], and for the FFN t16 / u16 fp16 [np][fmid])."""
    torch = _torch()
    np_, ne = m * top_k, gate.n_expert
    ktile = {4: 128, 2: 256, 8: 64, 6: 256}[gate.bits]  # Q6_K: K is whole superblocks, kp = K
    kp = (gate.k + ktile - 1) // ktile * ktile
    fout = down.n if down is not None else gate.n
    o = [0]

    def part(nbytes, dtype, shape, skip=0):
        at = o[0]
        o[0] += (nbytes + 255) // 256 * 256
        return ws[at + skip:at + nbytes].view(dtype).view(*shape)

    bound = np_ // 32 + min(ne, np_)
    r = dict(offs=part((ne + 1) * 4, torch.int32, (ne + 1,)), perm=part(np_ * 4, torch.int32, (np_,)),
             src=part(np_ * 4, torch.int32, (np_,)), inv=part(np_ * 4, torch.int32, (np_,)))
    at = o[0]
    r["tiles"] = part(16 + bound * 16, torch.int32, (bound, 4), skip=16)
    r["ntiles"] = ws[at:at + 4].view(torch.int32)
    r["x16"] = part(m * kp * 2, torch.float16, (m, kp))
    if down is not None:
        r["t16"] = part(np_ * gate.n * 2, torch.float16, (np_, gate.n))
        r["u16"] = part(np_ * gate.n * 2, torch.float16, (np_, gate.n))
    r["y"] = part(np_ * fout * 4, torch.float32, (np_, fout))
    assert o[0] == moe_grouped_workspace_size(gate, up, down, m, top_k), o[0]
    return r


_MOE_GWS = {}


def _grouped_workspace(gate, up, down, m, top_k, device, stream, who):
    """The workspace the grouped calls use when the caller gives none: one per (banks, shape, device, stream), kept for
    the life of the process and first allocated outside graph capture (as moe_workspace)."""
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    key = (gate.handle, _h(up), _h(down), m, top_k, str(device), int(s.cuda_stream))
    if key not in _MOE_GWS:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: the first call of a shape on a stream allocates its workspace; make it outside "
                               "graph capture or pass workspace=")
        _MOE_GWS[key] = moe_grouped_workspace_alloc(gate, up, down, m, top_k, device)
    return _MOE_GWS[key]


def _check_ws(ws, need):
    torch = _torch()
    assert ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= need and ws.data_ptr() % 16 == 0, need


def moe_ffn_grouped(gate, up, down, x, ids, wts, act="silu", out=None, stream=None, workspace=None):
    """moe_ffn for prefill-size M (nad_device_moe_ffn_grouped): the problems sorted by expert on the device, each
    expert's rows through the grouped gemm7 (a Q6_K bank's: woq_q6k_gemm_grouped_kernel), six launches.  Same arguments as moe_ffn; workspace: a uint8 cuda tensor
    of moe_grouped_workspace_size bytes (moe_grouped_workspace_alloc), None takes the one held for this shape and
    stream.  Banks gemm7 does not take raise (there is no fallback to moe_ffn)."""
    torch = _torch()
    m, fin = x.shape
    top_k = ids.shape[1]
    assert fin == gate.k and ids.dtype == torch.int32 and wts.dtype == torch.float32
    assert ids.shape[0] == m and tuple(wts.shape) == (m, top_k), (ids.shape, wts.shape)
    if workspace is None:
        workspace = _grouped_workspace(gate, up, down, m, top_k, x.device, stream, "moe_ffn_grouped")
    if out is None:
        out = torch.empty((m, down.n), dtype=torch.float32, device=x.device)
    _check_ws(workspace, moe_grouped_workspace_size(gate, up, down, m, top_k))
    epi = EPI_SILU_MUL if act == "silu" else EPI_GELU_MUL
    check(lib().nad_device_moe_ffn_grouped(gate.handle, up.handle, down.handle, _ptr(x), _ptr(ids), ids.stride(0),
                                           _ptr(wts), wts.stride(0), top_k, epi, _ptr(workspace), _ptr(out), m,
                                           x.stride(0), out.stride(0), _stream(stream)), "nad_device_moe_ffn_grouped")
    return out


def mul_mat_id_grouped(bank, x, ids, slot, out=None, stream=None, workspace=None):
    """mul_mat_id for prefill-size M (nad_device_mul_mat_id_grouped): sort, fp16 conversion, one grouped gemm7,
    un-permute; an id outside the bank gives a zero row."""
    torch = _torch()
    m, k = x.shape
    assert k == bank.k, (k, bank.k)
    assert ids.dtype == torch.int32 and ids.shape[0] == m, (ids.dtype, ids.shape)
    if workspace is None:
        workspace = _grouped_workspace(bank, None, None, m, 1, x.device, stream, "mul_mat_id_grouped")
    if out is None:
        out = torch.empty((m, bank.n), dtype=torch.float32, device=x.device)
    _check_ws(workspace, moe_grouped_workspace_size(bank, None, None, m, 1))
    check(lib().nad_device_mul_mat_id_grouped(bank.handle, _ptr(x), _ptr(ids), ids.stride(0), slot, _ptr(workspace),
                                              _ptr(out), m, x.stride(0), out.stride(0), _stream(stream)),
          "nad_device_mul_mat_id_grouped")
    return out


def plan_moe_grouped(gate, up, down, m, top_k):
    """What moe_ffn_grouped (up = down = None: mul_mat_id_grouped) launches for m rows (nad_plan_moe_grouped: no launch,
    no GPU needed; plan-only banks qualify): dict(launches=[dict(kernel, grid, threads, lds), ...], bm, bound)."""
    o = np.zeros(27, np.int64)
    c = lib().nad_plan_moe_grouped(_h(gate), _h(up), _h(down), m, top_k, _ptr(o), 27)
    if c < 3:
        raise RuntimeError(f"nad_plan_moe_grouped failed: {last_error()}")
    n = int(o[c - 1])
    assert c == 4 * n + 3, (c, n)
    return dict(launches=[dict(kernel=KERNELS.get(int(o[4 * i]), str(int(o[4 * i]))), grid=int(o[4 * i + 1]),
                               threads=int(o[4 * i + 2]), lds=int(o[4 * i + 3])) for i in range(n)],
                bm=int(o[4 * n]), bound=int(o[4 * n + 1]))
