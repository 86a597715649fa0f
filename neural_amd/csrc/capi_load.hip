// capi_load.hip -- weights onto the device: blob load / repack, descriptor summaries, the GGUF block types, the
// activation quantizer entries, synthetic weights and the unpack check (include/neural_amd.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "woq_device.h"

using namespace nad;

// ------------------------------------------------------------------------------------------------ load / repack
// F8_E8M0 shared exponents become exact fp32 scales 2^e on the device; DQ8_BNB codes are decoded on the host at load
// (dq8_get_fp_scale, kernel_ref.h:1981-1991) into the fp32 scales the reference computes
int scale_code(uint32_t t) {
  return (t == kF32 || t == kF8E8M0 || t == kDQ8_BNB) ? kScaleF32 : (t == kBF16 ? kScaleBF16 : kScaleF16);
}
// NFloat kind of the device weight: 0..2 the F4 LUTs (int4 layout), 3 F8_E4M3 / 4 F8_E5M2 (int8 layout, raw codes)
static int nfloat_kind(uint32_t qtype) {
  return is_f8(qtype) ? (qtype == kF8E4M3 ? 3 : 4) : f4_kind(qtype);
}

bool blob_supported(const Blob& b, const void* base, std::string* err) {
  if (b.blocksize % 32 != 0 && b.blocksize < b.k) {
    *err = "quantization group size must be a multiple of 32 (or per-channel)";
    return false;
  }
  if (base && b.qtype == kF8E5M2) {  // exponent field 31 (2^16 and up) has no fp16 B operand; the quantizer never writes it
    const uint8_t* q = static_cast<const uint8_t*>(base) + b.q_off;
    for (uint64_t i = 0; i < b.q_size; i++)
      if ((q[i] & 0x7c) == 0x7c) {
        *err = "F8_E5M2 code with exponent field 31 (|w| >= 65536 * scale) is not supported";
        return false;
      }
  }
  return true;
}


extern "C" size_t nad_device_weight_size(const void* hostblob) {
  Blob b;
  std::string err;
  if (!b.parse(hostblob, &err)) {
    set_err("%s", err.c_str());
    return 0;
  }
  DeviceWeight w{};
  int bs = b.blocksize >= b.k ? b.kpad : b.blocksize;
  return layout_geometry(w, device_bits(b.qtype), b.n, b.k, bs, scale_code(b.scale_t), b.asym, b.has_shuffle, 0,
                         b.has_reduce);
}

// largest |q - zp| of the device layout (int4 / int2 / int8 codes, sym or asym)
static float fold_qmax(int bits, bool asym) {
  if (bits == 4) return asym ? 15.f : 8.f;
  if (bits == 2) return asym ? 3.f : 2.f;
  return asym ? 255.f : 128.f;
}
// every scale s: s == 0, or s >= 2^-14 (the smallest nonzero |q| s is an fp16 normal) and qmax |s| <= 65504
static bool scale_in_fold_range(float s, float qmax) {
  const float a = std::fabs(s);
  return a == 0.f || (a >= 6.103515625e-05f && a * qmax <= 65504.f);
}
bool blob_fold_ok(const Blob& b, const uint8_t* base, int dev_bits) {
  if (b.scale_t == kF8E8M0 || nfloat_kind(b.qtype) >= 0) return false;  // F4 / F8 weights never take gemm3 / gemm4
  const float qmax = fold_qmax(dev_bits, b.asym);
  for (int g = 0; g < b.ngroups_k(); g++)  // the padding rows and columns hold zeros
    for (int n = 0; n < b.n; n++)
      if (!scale_in_fold_range(b.scale_at(reinterpret_cast<const int8_t*>(base), g, n), qmax)) return false;
  return true;
}

// the blob's q / scale / zero-point sections, already on the device, into w's tile layout (dz null: symmetric)
int repack_sections(const Blob& b, const DeviceWeight& w, const uint8_t* dq, const void* ds, const int8_t* dz,
                    hipStream_t st) {
  CoreInfo ci = core_info(b.core_id);
  RepackArgs ra{};
  ra.src_q = dq;
  ra.src_s = ds;
  ra.src_z = dz;
  ra.ntile = ci.ntile;
  ra.packrow = ci.packrow;
  ra.kpad = b.kpad;
  ra.cstep = b.cstep;
  ra.src_bits = dtype_bits(b.qtype);
  ra.raw = is_f8(b.qtype) ? 1 : 0;
  ra.src_e8m0 = b.scale_t == kF8E8M0 ? 1 : 0;
  ra.nel = uint64_t(b.npad) * b.kpad;
  ra.bits = w.bits;
  ra.n = w.n;
  ra.k = w.k;
  ra.ns = w.ns;
  ra.nt = w.nt;
  ra.ng = w.ng;
  ra.scale_t = w.scale_t;
  ra.kmajor = w.kmajor;
  ra.dst_tiles = static_cast<uint32_t*>(w.tiles);
  ra.dst_scales = w.scales;
  ra.dst_zps = w.zps;
  HIP_OK(launch_repack(ra, st));
  return 0;
}

extern "C" int nad_device_load(const void* hostblob, void* devstor, void* deviceptr, size_t capacity, void* queue) {
  Blob b;
  std::string err;
  if (!devstor || !deviceptr) {
    set_err("null devstor/deviceptr");
    return -1;
  }
  if (!b.parse(hostblob, &err) || !blob_supported(b, hostblob, &err)) {
    set_err("%s", err.c_str());
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  DeviceWeight w{};
  // per-channel (group >= K) is one group covering all tiles
  const int bs = b.blocksize >= b.k ? b.kpad : b.blocksize;
  const uint64_t need = layout_geometry(w, device_bits(b.qtype), b.n, b.k, bs, scale_code(b.scale_t), b.asym,
                                        b.has_shuffle, false, b.has_reduce);
  if (need > capacity) {
    set_err("device buffer too small for the tile layout: need %llu bytes, have %zu (see nad_device_weight_size)",
            (unsigned long long)need, capacity);
    return -1;
  }
  layout_assign(w, deviceptr);
  w.src_core_id = b.core_id;
  w.owner = nullptr;
  w.blob_bs = b.blocksize;
  // F4 codes go through the int4 repack unchanged (blob_q returns code - 8, + 8 back); F8 codes are stored raw
  w.f4kind = nfloat_kind(b.qtype);
  w.fold_ok = blob_fold_ok(b, static_cast<const uint8_t*>(hostblob), w.bits) ? 1 : 0;
  // stage the raw blob buffers on the device, repack there
  const uint8_t* base = static_cast<const uint8_t*>(hostblob);
  std::vector<float> dqs;  // DQ8_BNB: the decoded fp32 scales [ngroups][cstep], zero padding (outlives the staging)
  if (b.has_dq) {
    dqs.assign(size_t(b.ngroups()) * b.cstep, 0.f);
    for (int g = 0; g < b.ngroups_k(); g++)
      for (int n = 0; n < b.n; n++) dqs[size_t(g) * b.cstep + n] = b.scale_at(static_cast<const int8_t*>(hostblob), g, n);
  }
  const uint8_t* shost = b.has_dq ? reinterpret_cast<const uint8_t*>(dqs.data()) : base + b.s_off;
  const uint64_t qz = b.q_size, sz = b.has_dq ? dqs.size() * 4 : b.s_size, zz = b.asym ? b.z_size : 0;
  Staging stage(st);  // every return below synchronises, then frees
  if (!stage.alloc(align256(qz) + align256(sz) + align256(zz) + 256)) return staging_finish("nad_device_load", stage);
  uint8_t* dq = stage.ptr();
  uint8_t* ds = dq + align256(qz);
  uint8_t* dz = ds + align256(sz);
  HIP_OK(hipMemcpyAsync(dq, base + b.q_off, qz, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(ds, shost, sz, hipMemcpyHostToDevice, st));
  if (zz) HIP_OK(hipMemcpyAsync(dz, base + b.z_off, zz, hipMemcpyHostToDevice, st));
  if (b.has_shuffle) HIP_OK(hipMemcpyAsync(w.shuffle, base + b.shf_off, size_t(b.k) * 4, hipMemcpyHostToDevice, st));
  if (w.reduce) {  // bf16 rows [block][cstep] -> [block][red_ld], zero padded columns
    HIP_OK(hipMemsetAsync(w.reduce, 0, size_t(w.ng) * w.red_ld * 2, st));
    HIP_OK(hipMemcpy2DAsync(w.reduce, size_t(w.red_ld) * 2, base + b.r_off, size_t(b.cstep) * 2, size_t(b.n) * 2,
                            size_t(w.ng), hipMemcpyHostToDevice, st));
  }
  if (repack_sections(b, w, dq, ds, zz ? reinterpret_cast<const int8_t*>(dz) : nullptr, st)) return -1;
  if (staging_finish("nad_device_load", stage)) return -1;
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}

extern "C" void bestla_device_load_storage(void* hoststor, void* devstor, void* deviceptr, void* queue) {
  Blob b;
  std::string err;
  if (!b.parse(hoststor, &err)) {
    set_err("%s", err.c_str());
    report("bestla_device_load_storage");
    return;
  }
  // the caller sized deviceptr with the blob size (ne_layers.c:935-945, model_files.h:1515-1525)
  if (nad_device_load(hoststor, devstor, deviceptr, b.size, queue) != 0) report("bestla_device_load_storage");
}

// descriptor summary, versioned by the caller's buffer length: writes min(n, 14) values, returns the count written
extern "C" int nad_weight_info2(const void* devstor, int64_t* o, int n) {
  const auto* w = static_cast<const DeviceWeight*>(devstor);
  if (!w || w->magic != kWeightMagic || !o || n < 0) {
    set_err("not a neural_amd device weight descriptor (or no output buffer)");
    return -1;
  }
  const int64_t v[14] = {w->magic, w->bits, w->n, w->k, w->blocksize, w->ns, w->nt, w->ng, w->scale_t, w->asym,
                         w->has_shuffle, int64_t(w->bytes), w->fold_ok, w->kmajor};
  const int c = n < 14 ? n : 14;
  std::memcpy(o, v, sizeof(int64_t) * size_t(c));
  return c;
}
// the original 12-value form (callers built against the round-1 header)
extern "C" int nad_weight_info(const void* devstor, int64_t* o) { return nad_weight_info2(devstor, o, 12) == 12 ? 0 : -1; }

extern "C" int nad_blob_info(const void* hostblob, int64_t* o) {
  Blob b;
  std::string err;
  if (!b.parse(hostblob, &err)) {
    set_err("%s", err.c_str());
    return -1;
  }
  int64_t v[27] = {int64_t(b.size), b.prologue, int64_t(b.core_id), b.npad, b.kpad, b.n, b.k, b.qtype, b.blocksize,
                   b.scale_t, b.zp_t, b.red_t, b.cstep, int64_t(b.csize), b.asym, b.has_reduce, b.has_shuffle,
                   int64_t(b.q_off), int64_t(b.q_size), int64_t(b.s_off), int64_t(b.s_size), int64_t(b.z_off),
                   int64_t(b.z_size), int64_t(b.r_off), int64_t(b.r_size), int64_t(b.shf_off), int64_t(b.shf_size)};
  std::memcpy(o, v, sizeof(v));
  return 0;
}

extern "C" int nad_quant_u8_colblock(const void* act, int act_dtype, int m, int k, int lda, int blocksize,
                                     uint8_t* q, int ldq, float* scales, uint8_t* zps, int ld_scale, float* blkreduce,
                                     void* queue) {
  if (m <= 0 || k <= 0 || blocksize <= 0 || lda < k || ldq < k || !q || !scales || !zps ||
      ld_scale < (k + blocksize - 1) / blocksize) {
    set_err("nad_quant_u8_colblock: bad arguments (m=%d k=%d lda=%d ldq=%d blocksize=%d ld_scale=%d)", m, k, lda, ldq,
            blocksize, ld_scale);
    return -1;
  }
  QuantU8Args a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.bs = blocksize;
  a.ng = (k + blocksize - 1) / blocksize;
  a.q_u8 = q;
  a.ldu = ldq;
  a.s_out = scales;
  a.z_out = zps;
  a.red_out = blkreduce;
  a.ld_scale = ld_scale;
  hipError_t e = launch_quant_u8(a, act_dtype, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("activation quantization launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ GGUF block types
// One load path for every row of kGgufTypes (woq_gguf.h); the exported entries below name themselves in `who`.
extern "C" size_t nad_gguf_block_bytes(int type) {
  const GgufType* t = gguf_type_by_id(type);
  if (t && t->block_elems == 32) return size_t(t->block_bytes);
  if (t)  // superblocks of 256, not blocks of 32: entries of its own
    set_err("GGUF type %d (%s) has no 32-element block: it loads through nad_q6_k_device_size / nad_q6_k_device_load",
            t->id, t->name);
  else
    set_err("GGUF type %d is not supported (Q4_0 = 2, Q4_1 = 3, Q5_0 = 6, Q5_1 = 7, Q8_0 = 8; Q6_K = 14 through "
            "nad_q6_k_device_load)", type);
  return 0;
}

// geometry of an n x k matrix of type t and its device bytes (0, with the error set, for a bad shape): the type's
// layout, and behind it the fp16 mins of Q4_1 / Q5_1 at *mins_off
static uint64_t gguf_geometry(const char* who, const GgufType& t, int n, int k, DeviceWeight& w, uint64_t* mins_off) {
  if (n <= 0 || k <= 0 || k % t.block_elems) {
    set_err("%s: %s needs n > 0 and k a positive multiple of %d (n=%d k=%d)", who, t.name, t.block_elems, n, k);
    return 0;
  }
  if (t.bits == 6) return q6k_geometry(w, n, k);
  const uint64_t base = layout_geometry(w, t.bits, n, k, 32, kScaleF16, false, false);
  *mins_off = base;
  return base + (t.has_min ? align256(uint64_t(w.ns) * w.ng * 16 * 2) : 0);
}

static size_t gguf_size(const char* who, const GgufType& t, int n, int k) {
  DeviceWeight w{};
  uint64_t mins_off;
  return gguf_geometry(who, t, n, k, w, &mins_off);
}

// every block starts with its fp16 d: each inside the fold range for the type's largest |decoded value|
static bool blocks_fold_ok(const void* blocks, size_t block_bytes, size_t count, float qmax) {
  const uint8_t* bp = static_cast<const uint8_t*>(blocks);
  for (size_t i = 0; i < count; i++) {
    uint16_t h;
    std::memcpy(&h, bp + block_bytes * i, 2);
    if (!scale_in_fold_range(float(__builtin_bit_cast(_Float16, h)), qmax)) return false;
  }
  return true;
}

static int gguf_load(const char* who, const GgufType& t, const void* blocks, int n, int k, void* devstor,
                     void* deviceptr, size_t capacity, void* queue) {
  DeviceWeight w{};
  uint64_t mins_off = 0;
  const size_t need = gguf_geometry(who, t, n, k, w, &mins_off);
  if (!need) return -1;
  if (!blocks || !devstor || !deviceptr || capacity < need) {
    set_err("%s: null pointer or device buffer too small (need %zu, have %zu)", who, need, capacity);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  if (is_q6k(w)) {
    q6k_assign(w, deviceptr);
  } else {
    layout_assign(w, deviceptr);
    if (t.has_min) {
      w.mins = static_cast<char*>(deviceptr) + mins_off;
      w.bytes = need;
      w.min_bias = t.min_bias;
    }
  }
  w.owner = nullptr;
  w.src_core_id = t.tag;
  const size_t count = size_t(n) * (k / t.block_elems), bytes = count * t.block_bytes;
  // qmax 0 (Q6_K): sc * q is folded by the Q6_K GEMM itself (|sc * q| <= 4096 always fits fp16), d never
  w.fold_ok = t.qmax > 0.f && blocks_fold_ok(blocks, t.block_bytes, count, t.qmax) ? 1 : 0;
  Staging stage(st);
  if (!is_q6k(w)) {  // padding columns / K tiles decode to 0: int8 byte 128, nibble 8; scale 0, min 0 (the Q6_K repack
                     // writes every byte of its layout itself)
    const size_t entries = size_t(w.ns) * w.ng * 16;
    stage.run("hipMemsetAsync of the padding", [&] {
      hipError_t e = hipMemsetAsync(w.tiles, w.bits == 4 ? 0x88 : 0x80, size_t(w.ns) * w.nt * 1024, st);
      if (e == hipSuccess) e = hipMemsetAsync(w.scales, 0, entries * 2, st);
      if (e == hipSuccess && w.mins) e = hipMemsetAsync(w.mins, 0, entries * 2, st);
      return e;
    });
  }
  stage.alloc(bytes);
  stage.run("hipMemcpyAsync of the blocks",
            [&] { return hipMemcpyAsync(stage.ptr(), blocks, bytes, hipMemcpyHostToDevice, st); });
  stage.run("repack launch", [&] {
    return is_q6k(w) ? launch_q6k_repack(stage.ptr(), n, k, w, st) : launch_gguf_repack(t.id, stage.ptr(), n, k, w, st);
  });
  if (staging_finish(who, stage)) return -1;
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}

extern "C" size_t nad_gguf_device_size(int type, int n, int k) {
  return nad_gguf_block_bytes(type) ? gguf_size("nad_gguf_device_size", *gguf_type_by_id(type), n, k) : 0;
}
extern "C" int nad_gguf_device_load(int type, const void* blocks, int n, int k, void* devstor, void* deviceptr,
                                    size_t capacity, void* queue) {
  if (!nad_gguf_block_bytes(type)) return -1;  // the 32-element types; Q6_K keeps to its own entries
  return gguf_load("nad_gguf_device_load", *gguf_type_by_id(type), blocks, n, k, devstor, deviceptr, capacity, queue);
}
extern "C" size_t nad_q4_0_device_size(int n, int k) {
  return gguf_size("nad_q4_0_device_size", *gguf_type_by_id(NAD_GGUF_Q4_0), n, k);
}
extern "C" int nad_q4_0_device_load(const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity,
                                    void* queue) {
  return gguf_load("nad_q4_0_device_load", *gguf_type_by_id(NAD_GGUF_Q4_0), blocks, n, k, devstor, deviceptr, capacity,
                   queue);
}
extern "C" size_t nad_q6_k_device_size(int n, int k) {
  return gguf_size("nad_q6_k_device_size", *gguf_type_by_id(NAD_GGUF_Q6_K), n, k);
}
extern "C" int nad_q6_k_device_load(const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity,
                                    void* queue) {
  return gguf_load("nad_q6_k_device_load", *gguf_type_by_id(NAD_GGUF_Q6_K), blocks, n, k, devstor, deviceptr, capacity,
                   queue);
}

// ------------------------------------------------------------------------------------------------ activation rows
// Q8_0 (q8_1 false) / Q8_1 blocks of the activation rows, as the reference's vec_dot reads them
static int quant_q8(const char* who, bool q8_1, const void* act, int act_dtype, int m, int k, int lda, void* blocks,
                    void* queue) {
  if (m <= 0 || k <= 0 || k % 32 || lda < k || !blocks) {
    set_err("%s: bad arguments (m=%d k=%d lda=%d)", who, m, k, lda);
    return -1;
  }
  Q8Args a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.blocks = static_cast<int8_t*>(blocks);
  const hipError_t e = launch_q8_quant(a, q8_1, act_dtype, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("%s: quantization launch failed: %s", who, hipGetErrorString(e));
    return -1;
  }
  return 0;
}
extern "C" int nad_quant_q8_0(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue) {
  return quant_q8("nad_quant_q8_0", false, act, act_dtype, m, k, lda, blocks, queue);
}
extern "C" int nad_quant_q8_1(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue) {
  return quant_q8("nad_quant_q8_1", true, act, act_dtype, m, k, lda, blocks, queue);
}

extern "C" int nad_quant_q8_k(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue) {
  if (!act || !blocks || m <= 0 || k <= 0 || k % 256 || lda < k) {  // before anything on the device is touched
    set_err("nad_quant_q8_k: Q8_K needs non-null pointers, m > 0, k a positive multiple of 256 and lda >= k "
            "(m=%d k=%d lda=%d)", m, k, lda);
    return -1;
  }
  if (act_dtype != kActF32 && act_dtype != kActF16 && act_dtype != kActBF16) {
    set_err("nad_quant_q8_k: Q8_K activations must be fp32, fp16 or bf16 (act_dtype=%d)", act_dtype);
    return -1;
  }
  hipError_t e = launch_q8_k_quant(act, act_dtype, lda, m, k, blocks, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("Q8_K quantization launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ synthetic weights
__global__ void nad_fill_u32_kernel(uint32_t* p, uint64_t n, uint64_t seed) {
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
    uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    p[i] = uint32_t(x ^ (x >> 32));
  }
}
__global__ void nad_fill_scales_kernel(void* p, int st, uint64_t n, uint64_t seed) {
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
    uint64_t x = (i + 7) * 0xD6E8FEB86659FD93ull ^ seed;
    x ^= x >> 32;
    float v = 0.001f + 0.009f * float(x & 0xFFFFFF) / 16777216.f;
    if (st == kScaleF32)
      static_cast<float*>(p)[i] = v;
    else if (st == kScaleBF16)
      static_cast<uint16_t*>(p)[i] = uint16_t(__float_as_uint(v) >> 16);
    else
      static_cast<_Float16*>(p)[i] = _Float16(v);
  }
}

extern "C" size_t nad_synthetic_weight_size(int bits, int n, int k, int blocksize, int scale_t, int asym) {
  DeviceWeight w{};
  return layout_geometry(w, bits, n, k, blocksize > 0 ? blocksize : k, scale_t, asym != 0, false);
}

extern "C" int nad_synthetic_weight(void* devstor, void* deviceptr, size_t capacity, int bits, int n, int k,
                                    int blocksize, int scale_t, int asym, uint64_t seed, void* queue) {
  if (bits != 2 && bits != 4 && bits != 8) {
    set_err("bits must be 2, 4 or 8");
    return -1;
  }
  if (blocksize <= 0) blocksize = k;
  if (blocksize % 32 && blocksize < k) {
    set_err("group size must be a multiple of 32");
    return -1;
  }
  DeviceWeight w{};
  uint64_t need = layout_geometry(w, bits, n, k, blocksize, scale_t, asym != 0, false, false);
  if (need > capacity) {
    set_err("capacity %zu < needed %llu", capacity, (unsigned long long)need);
    return -1;
  }
  layout_assign(w, deviceptr);
  w.src_core_id = 0;
  w.fold_ok = 1;  // scales U[0.001, 0.01] (nad_fill_scales_kernel): every q * s is an fp16 normal
  hipStream_t st = static_cast<hipStream_t>(queue);
  uint64_t nd = uint64_t(w.ns) * w.nt * 256;
  hipLaunchKernelGGL(nad_fill_u32_kernel, dim3(4096), dim3(256), 0, st, static_cast<uint32_t*>(w.tiles), nd, seed);
  uint64_t nsc = uint64_t(w.ns) * w.ng * 16;
  hipLaunchKernelGGL(nad_fill_scales_kernel, dim3(1024), dim3(256), 0, st, w.scales, scale_t, nsc, seed * 3 + 1);
  if (w.zps)
    hipLaunchKernelGGL(nad_fill_u32_kernel, dim3(1024), dim3(256), 0, st, reinterpret_cast<uint32_t*>(w.zps),
                       (nsc + 3) / 4, seed * 5 + 2);
  HIP_OK(hipGetLastError());
  if (w.zps) {
    // zero points must stay in the signed range of the bit width: squash with a tiny kernel-free trick on host
    // (synthetic data only): reuse the fill but mask in place
    std::vector<int8_t> z(nsc);
    HIP_OK(hipMemcpyAsync(z.data(), w.zps, nsc, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const int half = bits == 8 ? 128 : (1 << (bits - 1));
    for (auto& v : z) v = int8_t((int(uint8_t(v)) % (2 * half)) - half);
    HIP_OK(hipMemcpyAsync(w.zps, z.data(), nsc, hipMemcpyHostToDevice, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}

// dequantize the device tile layout back to fp32 [K][N] (exactness check of the repack)
__global__ void nad_unrepack_kernel(DeviceWeight w, float* out) {
  const int KT = tile_k(w.bits);
  const uint64_t total = uint64_t(w.n) * w.k;
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < total; i += uint64_t(gridDim.x) * blockDim.x) {
    const int kk = int(i / w.n), n = int(i % w.n);
    const int s = n / 16, c = n % 16, t = kk / KT, kin = kk % KT;
    const int d = kin / 32, kq = (kin % 32) / 8, j = kin % 8;
    const int lane = kq * 16 + c;
    const uint32_t* tile = static_cast<const uint32_t*>(w.tiles) + tile_index(w.kmajor, w.ns, w.nt, s, t) * 256 + lane * 4;
    uint32_t v;
    int bias;
    if (w.bits == 4) {
      int p = (j >> 1) + 4 * (j & 1);
      v = (tile[d] >> (4 * p)) & 0xF;
      bias = 8;
    } else if (w.bits == 2) {
      int h = d & 1, p = (j >> 1) + 4 * h + 8 * (j & 1);
      v = (tile[d >> 1] >> (2 * p)) & 0x3;
      bias = 2;
    } else {
      v = (tile[2 * d + (j >> 2)] >> (8 * (j & 3))) & 0xFF;
      bias = 128;
    }
    const int g = kk / w.blocksize;
    const uint64_t si = scale_row(w.kmajor, w.ns, w.ng, s, g) * 16 + c;
    const float sc = load_scale(w.scales, si, w.scale_t);
    const int zp = w.zps ? int(w.zps[si]) : 0;
    float q;
    if (w.f4kind >= 3) {  // F8 raw code (f8_to_fp32, kernel_ref.h:984-1001)
      const int eb = w.f4kind == 3 ? 4 : 5, mb = 7 - eb;
      const uint32_t e = ((v & 0x7f) >> mb) - (1u << (eb - 1)) + 128;
      q = __uint_as_float(((v & 0x80) << 24) | (e << 23) | ((v << (23 - mb)) & 0x7fffffu));
    } else {
      q = w.f4kind >= 0 ? kF4LutF[w.f4kind][v & 15] : float(int(v) - bias - zp);
    }
    if (w.mins) q = q + float(w.min_bias);  // Q4_1 / Q5_1: the true q, q d exact, + m rounded once
    float r = q * sc;
    if (w.mins) r = r + float(static_cast<const _Float16*>(w.mins)[si]);
    out[i] = r;
  }
}

extern "C" int nad_device_unpack_fp32(const void* devstor, float* host_out, void* queue) {
  const DeviceWeight* w = as_weight(devstor);
  if (!w) return -1;
  hipStream_t st = static_cast<hipStream_t>(queue);
  const size_t bytes = size_t(w->n) * w->k * 4;
  Staging stage(st);  // host_out is the caller's: every return waits for the copy into it
  if (!stage.alloc(bytes)) return staging_finish("nad_device_unpack_fp32", stage);
  float* d = reinterpret_cast<float*>(stage.ptr());
  if (is_q6k(*w)) {
    HIP_OK(launch_q6k_unpack(*w, d, st));
  } else {
    hipLaunchKernelGGL(nad_unrepack_kernel, dim3(2048), dim3(256), 0, st, *w, d);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipMemcpyAsync(host_out, d, bytes, hipMemcpyDeviceToHost, st));
  return staging_finish("nad_device_unpack_fp32", stage);
}
