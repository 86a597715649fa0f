// capi_quant.hip -- a weight quantized, packed and laid out on the device (include/neural_amd.h nad_device_quantize*):
// what BTLAGemmQuantPackB + nad_device_load do through the host, for a matrix that already sits in HBM.
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "woq_quant.h"

using namespace nad;

namespace {

const char* dtype_name(uint32_t t) {
  switch (t) {
    case kF32: return "F32";
    case kF16: return "F16";
    case kBF16: return "BF16";
    case kS8: return "S8";
    case kS4: return "S4_CLIP";
    case kS2: return "S2_CLIP";
    case 1 | 0x100: return "S1_CLIP";
    case kS3: return "S3_CLIP";
    case kS5: return "S5_CLIP";
    case kS6: return "S6_CLIP";
    case kS7: return "S7_CLIP";
    case kF4E2M1: return "F4_E2M1";
    case kF4BNB: return "F4_BNB";
    case kF4NF4: return "F4_NF4";
    case kF8E4M3: return "F8_E4M3";
    case kF8E5M2: return "F8_E5M2";
    case kF8E8M0: return "F8_E8M0";
    case kDQ8_BNB: return "DQ8_BNB";
    default: return nullptr;
  }
}

struct QuantPlan {
  Blob b;          // the blob BTLAGemmQuantPackB would write (offsets unset)
  DeviceWeight w;  // the geometry nad_device_load would give it
  uint64_t need;
};

// the refusals of both entries, by name; blocksize <= 0 or >= k is per-channel
bool plan_quantize(const char* who, int n, int k, int blocksize, uint32_t qtype, uint32_t scale_dtype, int asym, int comp,
                   QuantPlan* p) {
  if (n <= 0 || k <= 0) {
    set_err("%s: n and k must be positive (n=%d k=%d)", who, n, k);
    return false;
  }
  if (qtype != kS4 && qtype != kS2 && qtype != kS8) {
    const char* nm = dtype_name(qtype);
    if (nm)
      set_err("%s: weight dtype %s is not quantized on the device (S4_CLIP, S2_CLIP and S8 are); it stays on the host "
              "path, BTLAGemmQuantPackB + nad_device_load", who, nm);
    else
      set_err("%s: unknown weight dtype 0x%x (S4_CLIP, S2_CLIP and S8 are quantized on the device)", who, qtype);
    return false;
  }
  if (scale_dtype != kF32 && scale_dtype != kBF16 && scale_dtype != kF16) {
    const char* nm = dtype_name(scale_dtype);
    if (nm)
      set_err("%s: scale dtype %s is not written on the device (F32, BF16 and F16 are); it stays on the host path, "
              "BTLAGemmQuantPackB + nad_device_load", who, nm);
    else
      set_err("%s: unknown scale dtype 0x%x (F32, BF16 and F16 are written on the device)", who, scale_dtype);
    return false;
  }
  if (blocksize <= 0) blocksize = k;
  const uint64_t core = select_core(comp, qtype, blocksize, asym != 0, host_isa_profile());
  if (!core) {
    set_err("%s: no packing core for CompType %d", who, comp);
    return false;
  }
  p->b = Blob::describe(n, k, blocksize, qtype, scale_dtype, asym != 0, core, false);
  std::string err;
  if (!blob_supported(p->b, &err)) {
    set_err("%s: %s", who, err.c_str());
    return false;
  }
  const Blob& b = p->b;
  const int bs = b.blocksize >= b.k ? b.kpad : b.blocksize;  // as nad_device_load: per-channel is one group
  p->w = DeviceWeight{};
  p->need = layout_geometry(p->w, device_bits(b.qtype), b.n, b.k, bs, scale_code(b.scale_t), b.asym, false, 0,
                            b.has_reduce);
  return true;
}

}  // namespace

extern "C" size_t nad_device_quantize_size(int n, int k, int blocksize, uint32_t qtype, uint32_t scale_dtype, int asym,
                                           int comp, size_t* blob_size) {
  QuantPlan p;
  if (!plan_quantize("nad_device_quantize_size", n, k, blocksize, qtype, scale_dtype, asym, comp, &p)) return 0;
  if (blob_size) *blob_size = p.b.size;
  return p.need;
}

extern "C" int nad_device_quantize(const void* wsrc, int w_dtype, int n, int k, int ldw, int blocksize, uint32_t qtype,
                                   uint32_t scale_dtype, int asym, int comp, void* devstor, void* deviceptr,
                                   size_t capacity, void* blob_out, size_t blob_capacity, void* queue) {
  // every refusal comes before any device work
  if (!wsrc || !devstor || !deviceptr) {
    set_err("nad_device_quantize: null %s", !wsrc ? "weight matrix" : (!devstor ? "devstor" : "deviceptr"));
    return -1;
  }
  if (w_dtype != kActF32 && w_dtype != kActF16 && w_dtype != kActBF16) {
    set_err("nad_device_quantize: the matrix must be fp32 (0), fp16 (1) or bf16 (2) (w_dtype=%d)", w_dtype);
    return -1;
  }
  QuantPlan p;
  if (!plan_quantize("nad_device_quantize", n, k, blocksize, qtype, scale_dtype, asym, comp, &p)) return -1;
  if (ldw < k) {
    set_err("nad_device_quantize: ldw %d < k %d", ldw, k);
    return -1;
  }
  if (p.need > capacity) {
    set_err("nad_device_quantize: device buffer too small for the tile layout: need %llu bytes, have %zu (see "
            "nad_device_quantize_size)", (unsigned long long)p.need, capacity);
    return -1;
  }
  Blob& b = p.b;
  if (blob_out && b.size > blob_capacity) {
    set_err("nad_device_quantize: blob buffer too small: need %llu bytes, have %zu (see nad_device_quantize_size)",
            (unsigned long long)b.size, blob_capacity);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  DeviceWeight& w = p.w;
  layout_assign(w, deviceptr);
  w.src_core_id = b.core_id;
  w.owner = nullptr;
  w.blob_bs = b.blocksize;
  w.f4kind = -1;

  // staging: the signed codes [n][ldq], then the blob's own sections q | scales | zps | reduce
  const CoreInfo ci = core_info(b.core_id);
  const int bits = dtype_bits(b.qtype);
  const uint64_t ldq = (uint64_t(k) + 15) & ~uint64_t(15);
  const uint64_t cz = align256(uint64_t(n) * ldq), qz = align256(b.q_size), sz = align256(b.s_size),
                 zz = b.asym ? align256(b.z_size) : 0, rz = b.has_reduce ? align256(b.r_size) : 0;
  std::vector<uint8_t> hs(b.s_size);  // the scales copied back for fold_ok (outlives the staging)
  Staging stage(st);                  // every return below synchronises, then frees
  if (!stage.alloc(cz + qz + sz + zz + rz)) return staging_finish("nad_device_quantize", stage);
  int8_t* dcodes = reinterpret_cast<int8_t*>(stage.ptr());
  uint8_t* dq = stage.ptr() + cz;
  uint8_t* ds = dq + qz;
  int8_t* dz = b.asym ? reinterpret_cast<int8_t*>(ds + sz) : nullptr;
  uint16_t* dr = b.has_reduce ? reinterpret_cast<uint16_t*>(ds + sz + zz) : nullptr;
  HIP_OK(hipMemsetAsync(ds, 0, sz + zz + rz, st));  // the padding rows and columns: scale 0, zp 0, reduce 0

  WoqQuantArgs qa{};
  qa.w = wsrc;
  qa.w_dtype = w_dtype;
  qa.n = n;
  qa.k = k;
  qa.ldw = ldw;
  qa.bs = b.blocksize;
  qa.nblk = b.ngroups_k();
  qa.bits = bits;
  qa.asym = b.asym ? 1 : 0;
  qa.scale_t = w.scale_t;
  qa.npad = b.cstep;
  qa.codes = dcodes;
  qa.ldq = int64_t(ldq);
  qa.scales = ds;
  qa.zps = dz;
  HIP_OK(launch_woq_quantize(qa, st));
  WoqPackArgs pa{};
  pa.codes = dcodes;
  pa.ldq = int64_t(ldq);
  pa.n = n;
  pa.k = k;
  pa.npad = b.npad;
  pa.kpad = b.kpad;
  pa.ntile = ci.ntile;
  pa.packrow = ci.packrow;
  pa.bits = bits;
  pa.q = dq;
  pa.q_size = b.q_size;
  HIP_OK(launch_woq_pack(pa, st));
  if (dr) {
    WoqReduceArgs ra{};
    ra.codes = dcodes;
    ra.ldq = int64_t(ldq);
    ra.n = n;
    ra.k = k;
    ra.bs = b.blocksize;
    ra.nblk = b.ngroups_k();
    ra.npad = b.cstep;
    ra.scale_t = w.scale_t;
    ra.scales = ds;
    ra.zps = dz;
    ra.red = dr;
    HIP_OK(launch_woq_reduce(ra, st));
  }

  // the device layout, as nad_device_load builds it from the uploaded sections
  if (w.reduce) {
    HIP_OK(hipMemsetAsync(w.reduce, 0, size_t(w.ng) * w.red_ld * 2, st));
    HIP_OK(hipMemcpy2DAsync(w.reduce, size_t(w.red_ld) * 2, dr, size_t(b.cstep) * 2, size_t(b.n) * 2, size_t(w.ng),
                            hipMemcpyDeviceToDevice, st));
  }
  if (repack_sections(b, w, dq, ds, dz, st)) return -1;

  // fold_ok by the rule of the load, over the small scale buffer copied back
  HIP_OK(hipMemcpyAsync(hs.data(), ds, b.s_size, hipMemcpyDeviceToHost, st));
  if (blob_out) {
    nad_host_cache_evict(blob_out);  // a pack entry is about to rewrite this blob
    int8_t* hb = static_cast<int8_t*>(blob_out);
    b.write_header(hb);
    HIP_OK(hipMemcpyAsync(hb + b.q_off, dq, b.q_size, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hb + b.s_off, ds, b.s_size, hipMemcpyDeviceToHost, st));
    if (b.asym) HIP_OK(hipMemcpyAsync(hb + b.z_off, dz, b.z_size, hipMemcpyDeviceToHost, st));
    if (b.has_reduce) HIP_OK(hipMemcpyAsync(hb + b.r_off, dr, b.r_size, hipMemcpyDeviceToHost, st));
  }
  if (staging_finish("nad_device_quantize", stage)) return -1;
  Blob sb = b;  // the scales alone: Blob::scale_at reads base + s_off
  sb.s_off = 0;
  w.fold_ok = blob_fold_ok(sb, hs.data(), w.bits) ? 1 : 0;
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}
