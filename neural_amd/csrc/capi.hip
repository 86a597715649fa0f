// capi.hip -- the extern "C" boundary (include/neural_amd.h): Neural Speed's BesTLA device/host/pack ABI re-hosted on
// MI355X.  Host-side orchestration only; all arithmetic on the hot path runs in woq_kernels.hip.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/neural_amd.h"
#include "btla_format.h"
#include "woq_kernels.h"

using namespace nad;

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
static void set_err(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}
static void report(const char* where) { fprintf(stderr, "neural_amd: %s: %s\n", where, g_err.c_str()); }
#define HIP_OK(expr)                                                           \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      set_err("%s failed: %s", #expr, hipGetErrorString(e_));                  \
      return -1;                                                               \
    }                                                                          \
  } while (0)

extern "C" const char* nad_last_error(void) { return g_err.c_str(); }
extern "C" void nad_clear_error(void) { g_err.clear(); }

// ------------------------------------------------------------------------------------------------ knobs
static int env_int(const char* name, int def) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : def;
}

// Tuning / A-B switches.  Read from the environment ONCE (at the first forward, or by nad_reload_knobs), never per
// launch: the eager path an NE graph takes (one bestla_device_f32f32_forward per node) must not scan the environment.
struct Knobs {
  int gemv_grid, gemv_waves, gemv_lean, gemv_spw, gemv_disable, gemv_dual, gemv_nst, gemv_m1_spec;
  int compute_int8;
  int gemm2_disable, gemm4_all, gemm4_disable, ffn_f32, gemm_kernel, gemm7_bm, splitk_disable;
  int gemm3_stagger, gemm4_fold_all, gemm4_fold, gemm4_ksw;
  int mid_min_m, mid_max_m, mid_ks, mid_xcd, mid_wide, gemm_xcd, gemm7_model, gemm7_fuse;
  int host_cache_mb;
};
static Knobs read_knobs() {
  Knobs k{};
  k.gemv_grid = env_int("NAD_GEMV_GRID", 0);    // tests / tuning: cap the workgroups of a stripe-stream launch
  k.gemv_waves = env_int("NAD_GEMV_WAVES", 0);  // tests / tuning: waves of a stripe-stream launch
  k.gemv_nst = env_int("NAD_GEMV_NST", 0);  // register stages per wave: 0 auto; 1 or 2 (M = 1 kernel), 1 or 3 (M <= 16)
  k.gemv_lean = env_int("NAD_GEMV_LEAN", 1);
  // M = 1 launches on woq_gemv_m1s_kernel (compact arguments, weight count / reduce / epilogue at compile time) where
  // one is instantiated; 0: every launch on woq_gemv_m1_kernel with the full GemvArgs (A/B, bit-identity tests)
  k.gemv_m1_spec = env_int("NAD_GEMV_M1_SPEC", 1);
  k.gemv_dual = env_int("NAD_GEMV_DUAL", 1);  // decode QKV of two formats (int2 Q, K + int4 V) as one launch
  k.gemv_spw = env_int("NAD_GEMV_SPW", 4);
  k.gemv_disable = env_int("NAD_GEMV_DISABLE", 0);
  k.compute_int8 = env_int("NAD_COMPUTE_INT8", 0);
  k.gemm2_disable = env_int("NAD_GEMM2_DISABLE", 0);
  k.gemm4_all = env_int("NAD_GEMM4_ALL", 0);
  k.gemm4_disable = env_int("NAD_GEMM4_DISABLE", 0);
  k.ffn_f32 = env_int("NAD_FFN_F32", 0);
  k.gemm_kernel = env_int("NAD_GEMM_KERNEL", 7);  // int4 g128 * 2^j prefill: 7 = gemm7, 3 = gemm3 (exact), 2 = gemm2
  k.gemm7_bm = env_int("NAD_GEMM7_BM", 0);        // gemm7 tile height (A/B): 0 auto, 32, 64, 128, 256
  k.splitk_disable = env_int("NAD_SPLITK_DISABLE", 0);
  k.gemm3_stagger = env_int("NAD_GEMM3_STAGGER", 1);  // measured +3-7 % (profiles/r02_gemm3_stagger.txt)
  k.gemm4_fold_all = env_int("NAD_GEMM4_FOLD_ALL", 1);
  k.gemm4_fold = env_int("NAD_GEMM4_FOLD", 1);
  k.gemm4_ksw = env_int("NAD_GEMM4_KSW", 2);  // folded gemm4 launches with the waves split over K: 0 off, 1 on, 2 auto
  k.mid_max_m = env_int("NAD_MID_MAX_M", 64);  // mid-M kernel (woq_gemm_mid.hip) up to this M (0: off)
  k.mid_ks = env_int("NAD_MID_KS", 0);         // tests / tuning: its K runs (0 auto)
  k.mid_xcd = env_int("NAD_MID_XCD", 1);       // the runs of a stripe group and their reduce on one XCD (0: off)
  k.mid_wide = env_int("NAD_MID_WIDE", 2);     // mid-M 8-stripe workgroups (M <= 32): 0 never, 1 always, 2 auto
  k.gemm_xcd = env_int("NAD_GEMM_XCD", 1);        // gemm7 split-K: the runs of a tile and their reduce on one XCD (0: off)
  k.gemm7_fuse = env_int("NAD_GEMM7_FUSE", 1);    // fused QKV prefill as one gemm7 launch (0: one per weight)
  k.gemm7_model = env_int("NAD_GEMM7_MODEL", 2);  // gemm7 tile-height model: 2 (round 6 refit), 1 (round 5)
  // mid-M from this M (0 auto: fp16 rows from 9 where its grid fits the CUs in one round, else 12; fp32 / bf16 from 8)
  k.mid_min_m = env_int("NAD_MID_MIN_M", 0);
  k.host_cache_mb = env_int("NAD_HOST_CACHE_MB", 64 * 1024);
  return k;
}
static Knobs g_knobs = read_knobs();  // library load
static const Knobs& knobs() { return g_knobs; }
// re-read the NAD_* switches (tests and A/B tools that change the environment at run time; not thread-safe against
// concurrent forwards)
extern "C" void nad_reload_knobs(void) { g_knobs = read_knobs(); }

// ------------------------------------------------------------------------------------------------ dry runs
// nad_plan_forward runs the whole host side of a forward (validation, kernel choice, geometry, workspace sizing) with
// every launch replaced by a record of it: which kernel would serve the call, and what the host path costs per call.
struct NadPlan {
  int kernel = 0, grid = 0, block = 0, ksplit = 1, fold = 0, launches = 0;
};
static thread_local NadPlan* t_plan = nullptr;
// true (and the launch recorded) in a dry run; main = false for pre-passes (conversions, activation quantizers)
static bool planned(int kernel, int grid, int block, int ksplit = 1, int fold = 0, bool main = true) {
  if (!t_plan) return false;
  t_plan->launches++;
  if (main) {
    t_plan->kernel = kernel;
    t_plan->grid = grid;
    t_plan->block = block;
    t_plan->ksplit = ksplit;
    t_plan->fold = fold;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ device context
struct NadDevice {
  int device;
  hipStream_t stream;
  bool profile;
};

extern "C" void* bestla_create_device(bool profile) {
  auto* d = new NadDevice();
  if (hipGetDevice(&d->device) != hipSuccess || hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
    set_err("no HIP device available");
    report("bestla_create_device");
    delete d;
    return nullptr;
  }
  d->profile = profile;
  return d;
}
extern "C" void* bestla_get_device_queue(void* device) {
  return device ? static_cast<void*>(static_cast<NadDevice*>(device)->stream) : nullptr;
}
extern "C" void bestla_release_device(void* device) {
  if (!device) return;
  auto* d = static_cast<NadDevice*>(device);
  (void)hipStreamSynchronize(d->stream);
  (void)hipStreamDestroy(d->stream);
  delete d;
}
extern "C" size_t bestla_device_gmem_size(void* device) {
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 0;
  return tot;
}
extern "C" void* bestla_device_malloc(size_t size, void* queue) {
  void* p = nullptr;
  if (hipMalloc(&p, size) != hipSuccess) {
    set_err("hipMalloc(%zu) failed", size);
    report("bestla_device_malloc");
    return nullptr;
  }
  return p;
}
extern "C" void bestla_device_free(void* ptr, void* queue) {
  if (!ptr) return;
  if (queue) (void)hipStreamSynchronize(static_cast<hipStream_t>(queue));
  (void)hipFree(ptr);
}
extern "C" void bestla_device_memcpy(void* dst, const void* src, size_t size, void* queue) {
  if (!dst || !src || !size) return;
  if (hipMemcpyAsync(dst, src, size, hipMemcpyDefault, static_cast<hipStream_t>(queue)) != hipSuccess) {
    set_err("hipMemcpyAsync failed");
    report("bestla_device_memcpy");
  }
}
extern "C" void bestla_device_memcpy_sync(void* dst, const void* src, size_t size, void* queue) {
  bestla_device_memcpy(dst, src, size, queue);
  (void)hipStreamSynchronize(static_cast<hipStream_t>(queue));
}
extern "C" void bestla_device_sync(void* queue) { (void)hipStreamSynchronize(static_cast<hipStream_t>(queue)); }
extern "C" size_t bestla_device_storage_size(void) { return sizeof(DeviceWeight); }

// ------------------------------------------------------------------------------------------------ load / repack
// F8_E8M0 shared exponents become exact fp32 scales 2^e on the device; DQ8_BNB codes are decoded on the host at load
// (dq8_get_fp_scale, kernel_ref.h:1981-1991) into the fp32 scales the reference computes
static int scale_code(uint32_t t) {
  return (t == kF32 || t == kF8E8M0 || t == kDQ8_BNB) ? kScaleF32 : (t == kBF16 ? kScaleBF16 : kScaleF16);
}
// NFloat kind of the device weight: 0..2 the F4 LUTs (int4 layout), 3 F8_E4M3 / 4 F8_E5M2 (int8 layout, raw codes)
static int nfloat_kind(uint32_t qtype) {
  return is_f8(qtype) ? (qtype == kF8E4M3 ? 3 : 4) : f4_kind(qtype);
}

// base: the host blob, scanned for codes the device cannot hold (load time only; null skips the scan)
static bool blob_supported(const Blob& b, const void* base, std::string* err) {
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
static bool blob_supported(const Blob& b, std::string* err) { return blob_supported(b, nullptr, err); }

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
static bool blob_fold_ok(const Blob& b, const uint8_t* base, int dev_bits) {
  if (b.scale_t == kF8E8M0 || nfloat_kind(b.qtype) >= 0) return false;  // F4 / F8 weights never take gemm3 / gemm4
  const float qmax = fold_qmax(dev_bits, b.asym);
  for (int g = 0; g < b.ngroups_k(); g++)  // the padding rows and columns hold zeros
    for (int n = 0; n < b.n; n++)
      if (!scale_in_fold_range(b.scale_at(reinterpret_cast<const int8_t*>(base), g, n), qmax)) return false;
  return true;
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
  uint8_t* stage = nullptr;
  std::vector<float> dqs;  // DQ8_BNB: the decoded fp32 scales [ngroups][cstep], zero padding
  if (b.has_dq) {
    dqs.assign(size_t(b.ngroups()) * b.cstep, 0.f);
    for (int g = 0; g < b.ngroups_k(); g++)
      for (int n = 0; n < b.n; n++) dqs[size_t(g) * b.cstep + n] = b.scale_at(static_cast<const int8_t*>(hostblob), g, n);
  }
  const uint8_t* shost = b.has_dq ? reinterpret_cast<const uint8_t*>(dqs.data()) : base + b.s_off;
  const uint64_t qz = b.q_size, sz = b.has_dq ? dqs.size() * 4 : b.s_size, zz = b.asym ? b.z_size : 0;
  HIP_OK(hipMalloc(&stage, align256(qz) + align256(sz) + align256(zz) + 256));
  uint8_t* dq = stage;
  uint8_t* ds = stage + align256(qz);
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
  CoreInfo ci = core_info(b.core_id);
  RepackArgs ra{};
  ra.src_q = dq;
  ra.src_s = ds;
  ra.src_z = zz ? reinterpret_cast<const int8_t*>(dz) : nullptr;
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
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipFree(stage));
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

// descriptor summary, versioned by the caller's buffer length: writes min(n, 13) values, returns the count written
extern "C" int nad_weight_info2(const void* devstor, int64_t* o, int n) {
  const auto* w = static_cast<const DeviceWeight*>(devstor);
  if (!w || w->magic != kWeightMagic || !o || n < 0) {
    set_err("not a neural_amd device weight descriptor (or no output buffer)");
    return -1;
  }
  const int64_t v[13] = {w->magic, w->bits, w->n, w->k, w->blocksize, w->ns, w->nt, w->ng, w->scale_t, w->asym,
                         w->has_shuffle, int64_t(w->bytes), w->fold_ok};
  const int c = n < 13 ? n : 13;
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

// ------------------------------------------------------------------------------------------------ forward
static const DeviceWeight* as_weight(const void* p) {
  const auto* w = static_cast<const DeviceWeight*>(p);
  if (!w || w->magic != kWeightMagic) {
    set_err("weight descriptor is not a loaded neural_amd device weight");
    return nullptr;
  }
  return w;
}

static SkinnyWeight view(const DeviceWeight& w, float* out, int ldo, const float* bias, int bias_ld) {
  SkinnyWeight v{};
  v.tiles = w.tiles;
  v.scales = w.scales;
  v.zps = w.zps;
  v.shuffle = w.shuffle;
  v.n = w.n;
  v.ns = w.ns;
  v.nt = w.nt;
  v.ng = w.ng;
  v.bs = w.blocksize;
  v.kmajor = w.kmajor;
  v.ldo = ldo;
  v.out = out;
  v.bias = bias;
  v.bias_ld = bias_ld;
  v.f4 = w.f4kind;
  return v;
}

static bool vec_aligned(const void* A, int lda, int act_t) {
  const int esz = act_t == kActF32 ? 4 : 2;
  return (reinterpret_cast<uintptr_t>(A) % 16 == 0) && ((size_t(lda) * esz) % 16 == 0);
}

// geometry of a skinny launch: K slices per stripe so the chip holds ~4K waves, capped by the 1024-thread WG
static void skinny_geometry(int total_stripes, int nt, int nwi, int* ks, int* tpw, int* ch) {
  const int target_waves = 4096;
  int k = (target_waves + total_stripes - 1) / total_stripes;
  k = std::max(k, (nt + 7) / 8);  // one chunk of <= 8 tiles per wave when possible
  k = std::max(1, std::min({k, 16 / nwi, nt}));
  int t = (nt + k - 1) / k;
  k = (nt + t - 1) / t;
  *ks = k;
  *tpw = t;
  *ch = t <= 4 ? 4 : 8;
}


static int device_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// The persistent stripe-stream GEMV (woq_gemv.hip) when the launch fits it: M <= 16, the staged activations fit LDS,
// the group size tiles the K tile, and all weights share one act-order LUT.  Returns 1 if launched, 0 if not eligible,
// -1 on a launch error.
// Fill the GemvArgs of one decode op; returns 1 when the stripe-stream GEMV handles it, 0 when not eligible.
static int prepare_gemv(GemvArgs& a, int& waves, int& grid, int& gpt_out, const void* act, int act_t, int lda, int m,
                        int k, int nw, const DeviceWeight* const* ws, float* const* outs, const int* ldos, int epi,
                        const float* bias, int bias_ld, const float* res, int ld_res, float* aux, int ld_aux,
                        bool single_op = true) {
  const DeviceWeight& w0 = *ws[0];
  for (int i = 1; i < nw; i++)
    if (ws[i]->shuffle != w0.shuffle || ws[i]->nt != w0.nt || ws[i]->ng != w0.ng || ws[i]->bits != w0.bits ||
        ws[i]->asym != w0.asym || ws[i]->scale_t != w0.scale_t || ws[i]->blocksize != w0.blocksize ||
        ws[i]->kmajor)
      return 0;
  if (w0.kmajor) return 0;  // the stream stages each stripe's scale block: stripe-major layout only
  for (int i = 0; i < nw; i++)
    if (ws[i]->f4kind >= 0) return 0;  // NFloat weights: LUT dequant lives in the skinny kernel
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(w0.bits, w0.nt, w0.ng, w0.blocksize, &tpg);
  if (gpt == 0 || (gpt >= 4 && w0.asym)) return 0;
  a = GemvArgs{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.act_t = act_t;
  a.dual = (epi == kEpiSiluMul || epi == kEpiGeluMul) ? 1 : 0;
  a.nt = w0.nt;
  a.ng = w0.ng;
  a.bs = w0.blocksize;
  a.tpg_mask = tpg == 0 ? 0x7fffffff : tpg - 1;
  a.tpg_shift = tpg == 0 ? 31 : __builtin_ctz(unsigned(tpg));
  a.scale_t = w0.scale_t;
  a.asym = w0.asym;
  a.epi = epi;
  a.shuffle = w0.shuffle;
  a.a_fast = (vec_aligned(act, lda, act_t) && w0.shuffle == nullptr && k % 8 == 0) ? 1 : 0;
  a.res = res;
  a.ld_res = ld_res;
  a.aux = aux;
  a.ld_aux = ld_aux;
  int stripes = 0;
  for (int i = 0; i < 4; i++) a.stripe_base[i] = INT_MAX;
  for (int i = 0; i < nw; i++) {
    a.w[i] = view(*ws[i], outs[i], ldos[i], bias, bias_ld);
    a.stripe_base[i] = stripes;
    stripes += ws[i]->ns;
  }
  for (int i = nw; i < 3; i++) a.w[i] = a.w[0];
  a.units = a.dual ? ws[0]->ns : stripes;
  const Knobs& kn = knobs();
  grid = std::max(1, std::min(a.units, device_cus()));
  if (kn.gemv_grid > 0) grid = std::min(a.units, kn.gemv_grid);  // tests / tuning
  waves = gemv_waves(w0.bits, w0.nt, w0.ng, w0.blocksize);
  if (kn.gemv_waves > 0) waves = std::min(gpt > 1 ? 8 : 16, kn.gemv_waves);
  a.dq_mask = 0x000F000Fu;
  a.dq_magic = 0x64006400u;
  a.m1_nst = kn.gemv_nst;
  a.m1_spec = kn.gemv_m1_spec;
  a.u_q = a.units / grid;
  a.u_r = a.units % grid;
  a.lean = kn.gemv_lean;
  // M = 1 single-op launches may stream 2-tile K-slices, one per wave (up to 16 waves); fused launches keep 4-tile ones
  if (single_op)
    gemv_lean_slices(a, w0.bits, &waves, kn.gemv_waves > 0 ? 4 : 2);
  if (kn.gemv_spw != 4 && a.lean_spw == 4) a.lean_spw = 2;  // A/B: long K back on the general stream kernel
  const size_t lds = gemv_lds_layout(a, w0.bits, waves, grid);
  if (lds > 160 * 1024) return 0;
  // buffer-resource offsets are 32-bit: every tile array, scale array and the activations must stay below 2 GiB
  const int esz = act_t == kActF32 ? 4 : 2;
  if (uint64_t(m) * lda * esz >= (1ull << 30)) return 0;
  for (int i = 0; i < nw; i++)
    if (uint64_t(ws[i]->ns) * ws[i]->nt * 1024 >= (1ull << 30)) return 0;
  gpt_out = gpt;
  (void)lds;
  return 1;
}

static int try_gemv(const void* act, int act_t, int lda, int m, int k, int nw, const DeviceWeight* const* ws,
                    float* const* outs, const int* ldos, int epi, const float* bias, int bias_ld, const float* res,
                    int ld_res, float* aux, int ld_aux, hipStream_t st) {
  if (knobs().gemv_disable) return 0;
  GemvArgs a{};
  int waves = 0, grid = 0, gpt = 0;
  if (!prepare_gemv(a, waves, grid, gpt, act, act_t, lda, m, k, nw, ws, outs, ldos, epi, bias, bias_ld, res, ld_res,
                    aux, ld_aux))
    return 0;
  const size_t lds = gemv_lds_layout(a, ws[0]->bits, waves, grid);
  hipError_t e = planned(gemv_uses_m1(a, ws[0]->bits, waves) ? NAD_KERNEL_GEMV_M1 : NAD_KERNEL_GEMV, grid, waves * 64, 1,
                         t_plan && gemv_uses_m1s(a, ws[0]->bits, waves) ? 4 : 0)
                     ? hipSuccess
                     : launch_gemv(a, ws[0]->bits, waves, grid, lds, st);
  if (e != hipSuccess) {
    set_err("gemv kernel launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 1;
}

static bool int8_compute(const DeviceWeight& w);
static int gguf_act_quant(const DeviceWeight& w);
static int run_i8(const void* act, int act_t, int lda, int m, int k, int nw, const DeviceWeight* const* ws,
                  float* const* outs, const int* ldos, bool dual, int epi, const float* bias, int bias_ld,
                  const float* res, int ld_res, const float* aux, int ld_aux, hipStream_t st);

static int run_skinny(const void* act, int act_t, int lda, int m, int k, int nw, const DeviceWeight* const* ws,
                      float* const* outs, const int* ldos, int epi, const float* bias, int bias_ld, const float* res,
                      int ld_res, float* aux, int ld_aux, hipStream_t st) {
  if (nw > 1) {  // weights of one fused call whose arithmetic differs (per-weight compute modes) run one by one
    bool mixed = false;
    for (int i = 1; i < nw; i++)
      mixed |= int8_compute(*ws[i]) != int8_compute(*ws[0]) || gguf_act_quant(*ws[i]) != gguf_act_quant(*ws[0]);
    if (mixed) {
      if (epi == kEpiSiluMul || epi == kEpiGeluMul) {
        set_err("gate/up weights of one FFN must resolve to the same arithmetic (nad_device_set_compute)");
        return -1;
      }
      for (int i = 0; i < nw; i++)
        if (run_skinny(act, act_t, lda, m, k, 1, ws + i, outs + i, ldos + i, epi, bias, bias_ld, res, ld_res, aux,
                       ld_aux, st))
          return -1;
      return 0;
    }
  }
  if (int8_compute(*ws[0]))
    return run_i8(act, act_t, lda, m, k, nw, ws, outs, ldos, nw == 2 && (epi == kEpiSiluMul || epi == kEpiGeluMul),
                  epi, bias, bias_ld, res, ld_res, aux, ld_aux, st);
  const int g = try_gemv(act, act_t, lda, m, k, nw, ws, outs, ldos, epi, bias, bias_ld, res, ld_res, aux, ld_aux, st);
  if (g != 0) return g < 0 ? -1 : 0;
  SkinnyArgs a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.nw = nw;
  a.scale_t = ws[0]->scale_t;
  a.epi = epi;
  a.vec_ok = vec_aligned(act, lda, act_t) ? 1 : 0;
  a.res = res;
  a.ld_res = ld_res;
  a.aux = aux;
  a.ld_aux = ld_aux;
  const bool dual = epi == kEpiSiluMul || epi == kEpiGeluMul;
  int stripes = 0;
  for (int i = 0; i < nw; i++) {
    a.w[i] = view(*ws[i], outs[i], ldos[i], bias, bias_ld);
    a.stripe_base[i] = stripes;
    stripes += ws[i]->ns;
  }
  a.stripe_base[nw] = stripes;
  if (dual) stripes = ws[0]->ns;
  int ks, tpw, ch;
  skinny_geometry(stripes, ws[0]->nt, dual ? 2 : 1, &ks, &tpw, &ch);
  a.tiles_per_wave = tpw;
  a.steps_per_group = ws[0]->blocksize / 32;
  a.a_fast = (a.vec_ok && ws[0]->shuffle == nullptr && k % (act_t == kActF32 ? 4 : 8) == 0) ? 1 : 0;
  hipError_t e = planned(NAD_KERNEL_SKINNY, stripes, ks * (dual ? 2 : 1) * 64)
                     ? hipSuccess
                     : launch_skinny(a, ws[0]->bits, act_t, ks * (dual ? 2 : 1), stripes, ch, st);
  if (e != hipSuccess) {
    set_err("skinny kernel launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// Device workspace for the prefill GEMM's fp16 copy of the activations, in order of preference:
//   1. the caller's workspace of a reference entry point (bestla_device_f32f32_forward(..., workspace, queue): the
//      graph's dev_work, sized by bestla_support -> nad_device_workspace_size, ne_layers.c:11947-11967);
//   2. a workspace the caller bound to the stream (nad_bind_workspace; the nad_device_* entries take no argument);
//   3. a per-stream grow-only scratch owned by the library.  It grows only outside graph capture and a buffer is never
//      freed (a captured graph may reference it); a capture that would need growth fails loudly instead of switching
//      kernels.
namespace {
struct WsRef {
  void* ptr = nullptr;
  size_t bytes = 0;
};
thread_local WsRef t_call_ws;  // set by the reference entry points for the duration of one call
std::mutex g_ws_mu;
std::unordered_map<hipStream_t, WsRef> g_bound_ws;
std::unordered_map<hipStream_t, WsRef> g_scratch;
std::vector<void*> g_scratch_all;  // every scratch buffer ever handed out (kept for captured graphs)

struct CallWorkspace {  // RAII binding of a reference call's workspace argument
  CallWorkspace(void* p, size_t b) { t_call_ws = WsRef{p, p ? b : 0}; }
  ~CallWorkspace() { t_call_ws = WsRef{}; }
};
}  // namespace

extern "C" size_t nad_device_workspace_size(int m, int k);

extern "C" int nad_bind_workspace(void* queue, void* ptr, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  hipStream_t st = static_cast<hipStream_t>(queue);
  if (!ptr || !bytes)
    g_bound_ws.erase(st);
  else
    g_bound_ws[st] = WsRef{ptr, bytes};
  return 0;
}

static void* workspace_for(size_t bytes, hipStream_t st) {
  if (t_plan) return reinterpret_cast<void*>(uintptr_t(1) << 40);  // dry run: sized, never touched
  if (t_call_ws.ptr && t_call_ws.bytes >= bytes) return t_call_ws.ptr;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  auto b = g_bound_ws.find(st);
  if (b != g_bound_ws.end() && b->second.bytes >= bytes) return b->second.ptr;
  WsRef& sc = g_scratch[st];
  if (sc.bytes >= bytes) return sc.ptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
    set_err("prefill under graph capture needs %zu bytes of device workspace: bind one with nad_bind_workspace (or run "
            "the same shape once before capturing)", bytes);
    return nullptr;
  }
  void* p = nullptr;
  const size_t want = std::max(bytes, sc.bytes * 2);
  if (hipMalloc(&p, want) != hipSuccess) {
    set_err("workspace allocation of %zu bytes failed", want);
    return nullptr;
  }
  g_scratch_all.push_back(p);
  sc = WsRef{p, want};
  return p;
}

// ------------------------------------------------------------------------------------------------ int8 compute
// The reference's comp_int8 arithmetic (woq_i8.hip) for weights packed for an integer core (the blob carries the bf16
// reduce).  Off by default: the fp16-MFMA path on exact weights is the more accurate one.  Mode 1 (nad_set_compute_mode
// or NAD_COMPUTE_INT8=1) reproduces the reference: u8 activations per (row, block), s32 block dots, the kblock core's
// fp32 combine.
// The arithmetic is chosen per call, in order: the weight's own setting (nad_device_set_compute: the reference picks
// it per blob core, bestla_gemm.cpp:516-616), else the calling thread's (nad_set_thread_compute_mode), else the
// process default (nad_set_compute_mode, initialised from NAD_COMPUTE_INT8).  Mode 1 applies to blobs packed for an
// integer core only -- exactly those that carry the reduce -- and to the GGUF block types (Q4_0, Q4_1, Q5_0, Q5_1,
// Q8_0: the reference's Q8_0 / Q8_1 vec_dot arithmetic); every other weight stays fp.
static std::atomic<int> g_compute_mode{-1};
static thread_local int t_compute_mode = -1;
static int compute_mode() {
  if (t_compute_mode >= 0) return t_compute_mode;
  int m = g_compute_mode.load(std::memory_order_relaxed);
  if (m < 0) {
    int init = knobs().compute_int8 ? 1 : 0, expect = -1;
    g_compute_mode.compare_exchange_strong(expect, init);
    m = g_compute_mode.load(std::memory_order_relaxed);
  }
  return m;
}
// a GGUF Q4_0 matrix (nad_q4_0_device_load) carries this in src_core_id: its int8 arithmetic is Q8_0 x Q4_0
constexpr uint64_t kGgufQ4_0 = 0x3054344655474700ull;  // "\0GGUF4Q0"
static bool is_q4_0(const DeviceWeight& w) { return w.src_core_id == kGgufQ4_0; }
// the other GGUF block types (nad_gguf_device_load): the same tag with the type's two characters
constexpr uint64_t kGgufQ4_1 = 0x3154344655474700ull;  // "\0GGUF4Q1"
constexpr uint64_t kGgufQ5_0 = 0x3054354655474700ull;  // "\0GGUF5Q0"
constexpr uint64_t kGgufQ5_1 = 0x3154354655474700ull;  // "\0GGUF5Q1"
constexpr uint64_t kGgufQ8_0 = 0x3054384655474700ull;  // "\0GGUF8Q0"
// NAD_GGUF_* of a loaded weight, 0 for a weight that is no GGUF matrix
static int gguf_type(const DeviceWeight& w) {
  if (is_q4_0(w)) return NAD_GGUF_Q4_0;
  switch (w.src_core_id) {
    case kGgufQ4_1: return NAD_GGUF_Q4_1;
    case kGgufQ5_0: return NAD_GGUF_Q5_0;
    case kGgufQ5_1: return NAD_GGUF_Q5_1;
    case kGgufQ8_0: return NAD_GGUF_Q8_0;
    default: return 0;
  }
}
// the activation quantizer of the weight's int8 arithmetic (its vec_dot_type, ne_layers.c:266-318): 0 the kblock
// core's u8, 1 Q8_0 (Q4_0, Q5_0, Q8_0), 2 Q8_1 (Q4_1, Q5_1)
static int gguf_act_quant(const DeviceWeight& w) {
  const int t = gguf_type(w);
  return t == 0 ? 0 : ((t == NAD_GGUF_Q4_1 || t == NAD_GGUF_Q5_1) ? 2 : 1);
}
static int effective_mode(const DeviceWeight& w) { return w.compute > 0 ? w.compute - 1 : compute_mode(); }
static bool int8_compute(const DeviceWeight& w) {
  return effective_mode(w) == 1 && (w.reduce != nullptr || gguf_type(w) != 0);
}

extern "C" int nad_set_compute_mode(int mode) {
  if (mode != 0 && mode != 1) {
    set_err("compute mode must be 0 (fp) or 1 (int8 for integer-core weights), got %d", mode);
    return -1;
  }
  g_compute_mode.store(mode, std::memory_order_relaxed);
  return 0;
}
extern "C" int nad_get_compute_mode(void) { return compute_mode(); }
extern "C" int nad_set_thread_compute_mode(int mode) {
  if (mode < -1 || mode > 1) {
    set_err("thread compute mode must be -1 (follow the process default), 0 or 1, got %d", mode);
    return -1;
  }
  t_compute_mode = mode;
  return 0;
}
extern "C" int nad_device_set_compute(void* devstor, int mode) {
  DeviceWeight* w = static_cast<DeviceWeight*>(devstor);
  if (!w || w->magic != kWeightMagic) {
    set_err("nad_device_set_compute: not a device weight");
    return -1;
  }
  if (mode < -1 || mode > 1) {
    set_err("weight compute mode must be -1 (follow the thread/process setting), 0 (fp) or 1 (int8), got %d", mode);
    return -1;
  }
  w->compute = mode + 1;
  return 0;
}
// the arithmetic a forward of this weight takes right now: 0 fp, 1 int8
extern "C" int nad_device_get_compute(const void* devstor) {
  const DeviceWeight* w = static_cast<const DeviceWeight*>(devstor);
  if (!w || w->magic != kWeightMagic) {
    set_err("nad_device_get_compute: not a device weight");
    return -1;
  }
  return int8_compute(*w) ? 1 : 0;
}

struct I8Act {
  const int8_t* aq = nullptr;
  int ldq = 0;
  const float2* sa = nullptr;
};

static size_t i8_act_bytes(int m, const DeviceWeight& w) {
  return align256(size_t(m) * w.nt * tile_k(w.bits)) + align256(size_t(m) * w.ng * sizeof(float2));
}

static int i8_quantize(I8Act& r, char* ws, const void* act, int act_t, int lda, int m, int k, const DeviceWeight& w,
                       hipStream_t st) {
  const int kp = w.nt * tile_k(w.bits);
  if (gguf_act_quant(w)) {  // Q8_0 / Q8_1 rows (quantize_row_q8_0_reference / quantize_row_q8_1_reference)
    Q80Args q{};
    q.A = act;
    q.lda = lda;
    q.M = m;
    q.K = k;
    q.aq = reinterpret_cast<int8_t*>(ws);
    q.ldq = kp;
    q.kp = kp;
    q.sa = reinterpret_cast<float2*>(ws + align256(size_t(m) * kp));
    hipError_t e = planned(0, 0, 0, 1, 0, false)
                       ? hipSuccess
                       : (gguf_act_quant(w) == 2 ? launch_q8_1_quant(q, act_t, st) : launch_q8_0_quant(q, act_t, st));
    if (e != hipSuccess) {
      set_err("Q8_0 / Q8_1 activation quantization launch failed: %s", hipGetErrorString(e));
      return -1;
    }
    r.aq = q.aq;
    r.ldq = kp;
    r.sa = q.sa;
    return 0;
  }
  QuantU8Args q{};
  q.A = act;
  q.lda = lda;
  q.M = m;
  q.K = k;
  q.bs = w.blob_bs;
  q.ng = w.ng;
  q.shuffle = w.shuffle;
  q.aq = reinterpret_cast<int8_t*>(ws);
  q.ldq = kp;
  q.kp = kp;
  q.sa = reinterpret_cast<float2*>(ws + align256(size_t(m) * kp));
  hipError_t e = planned(0, 0, 0, 1, 0, false) ? hipSuccess : launch_quant_u8(q, act_t, st);
  if (e != hipSuccess) {
    set_err("activation quantization launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  r.aq = q.aq;
  r.ldq = kp;
  r.sa = q.sa;
  return 0;
}

static int min_term(const void* act, int act_t, int lda, const float* S, int s_ld, int s_st, int m, int k,
                    const DeviceWeight& w, float* out, int ldo, int epi, const float* bias, int bias_ld,
                    const float* res, int ld_res, const float* aux, int ld_aux, hipStream_t st);

static int i8_gemm_main(const I8Act& x, int m, int k, const DeviceWeight& w, float* out, int ldo, int epi,
                        const float* bias, int bias_ld, const float* res, int ld_res, const float* aux, int ld_aux,
                        hipStream_t st) {
  I8Args a{};
  a.aq = x.aq;
  a.ldq = x.ldq;
  a.a_signed = gguf_act_quant(w) ? 1 : 0;
  a.sa = x.sa;
  a.M = m;
  a.K = k;
  a.red = static_cast<const uint16_t*>(w.reduce);
  a.red_ld = w.red_ld;
  a.scale_t = w.scale_t;
  a.epi = epi;
  a.res = res;
  a.ld_res = ld_res;
  a.aux = aux;
  a.ld_aux = ld_aux;
  a.w = view(w, out, ldo, bias, bias_ld);
  hipError_t e = planned(NAD_KERNEL_I8, 0, 0) ? hipSuccess : launch_i8(a, w.bits, st);
  if (e != hipSuccess) {
    set_err("int8-compute kernel launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

static int i8_gemm(const I8Act& x, int m, int k, const DeviceWeight& w, float* out, int ldo, int epi,
                   const float* bias, int bias_ld, const float* res, int ld_res, const float* aux, int ld_aux,
                   hipStream_t st) {
  if (!w.mins) return i8_gemm_main(x, m, k, w, out, ldo, epi, bias, bias_ld, res, ld_res, aux, ld_aux, st);
  // Q4_1 / Q5_1 x Q8_1 (vec_dot.h:385-400, 569-590): the block dots on the true q, then + sum_b m * s with the Q8_1
  // block sums s = sa[].y, and the caller's epilogue
  if (i8_gemm_main(x, m, k, w, out, ldo, kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0, st)) return -1;
  return min_term(nullptr, kActF32, 0, &x.sa[0].y, 2 * w.ng, 2, m, k, w, out, ldo, epi, bias, bias_ld, res, ld_res, aux,
                  ld_aux, st);
}

// nw weights on one activation.  dual: the FFN gate/up pair (outs[1] = act(x.w0) * (x.w1); aux, if given, receives
// act(x.w0)), run as the prefill FFN does: two passes, the second multiplying by the first's output.
static int run_i8(const void* act, int act_t, int lda, int m, int k, int nw, const DeviceWeight* const* ws,
                  float* const* outs, const int* ldos, bool dual, int epi, const float* bias, int bias_ld,
                  const float* res, int ld_res, const float* aux, int ld_aux, hipStream_t st) {
  for (int i = 0; i < nw; i++)
    if (!int8_compute(*ws[i]) || gguf_act_quant(*ws[i]) != gguf_act_quant(*ws[0])) {
      set_err("int8 compute: the weights of a fused call must all be integer-core blobs (with reduce) or all GGUF types "
              "of one activation quantizer (Q8_0: Q4_0, Q5_0, Q8_0; Q8_1: Q4_1, Q5_1)");
      return -1;
    }
  const size_t abytes = i8_act_bytes(m, *ws[0]);
  const bool own_t1 = dual && !aux;
  const size_t t1bytes = own_t1 ? size_t(m) * ws[0]->n * sizeof(float) : 0;
  char* wsp = static_cast<char*>(workspace_for(abytes + t1bytes, st));
  if (!wsp) return -1;
  I8Act x;
  if (i8_quantize(x, wsp, act, act_t, lda, m, k, *ws[0], st)) return -1;
  if (dual) {
    float* t1 = own_t1 ? reinterpret_cast<float*>(wsp + abytes) : const_cast<float*>(aux);
    const int ld1 = own_t1 ? ws[0]->n : ld_aux;
    const int e1 = epi == kEpiSiluMul ? kEpiSilu : kEpiGelu;
    if (i8_gemm(x, m, k, *ws[0], t1, ld1, e1, nullptr, 0, nullptr, 0, nullptr, 0, st)) return -1;
    return i8_gemm(x, m, k, *ws[1], outs[1], ldos[1], kEpiSiluMul, nullptr, 0, nullptr, 0, t1, ld1, st);
  }
  for (int i = 0; i < nw; i++)
    if (i8_gemm(x, m, k, *ws[i], outs[i], ldos[i], epi, bias, bias_ld, res, ld_res, aux, ld_aux, st)) return -1;
  return 0;
}

// The minimum term of a GGUF Q4_1 / Q5_1 weight and the caller's epilogue, on an `out` that holds X (q d)^T
// (woq_gguf.hip): out = epi(out + S mins^T).  S null: the exact block sums of the activations -- summed inside the
// M <= 16 kernel, else by a pre-pass into the workspace (the main kernel's use of it is over by stream order).  A
// weight without mins gets the epilogue alone (the mixed FFN pairs).
static int min_term(const void* act, int act_t, int lda, const float* S, int s_ld, int s_st, int m, int k,
                    const DeviceWeight& w, float* out, int ldo, int epi, const float* bias, int bias_ld,
                    const float* res, int ld_res, const float* aux, int ld_aux, hipStream_t st) {
  MinTermArgs a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.S = S;
  a.s_ld = s_ld;
  a.s_st = s_st;
  a.mins = static_cast<const uint16_t*>(w.mins);
  a.scales = static_cast<const uint16_t*>(w.scales);  // GGUF: fp16
  a.qbias = float(w.min_bias);
  a.ns = w.ns;
  a.ng = w.ng;
  a.kmajor = w.kmajor;
  a.g.M = m;
  a.g.K = k;
  a.g.epi = epi == kEpiGeluMul ? kEpiSiluMul : epi;  // the multiply by aux (the activation is in aux already)
  a.g.res = res;
  a.g.ld_res = ld_res;
  a.g.aux = aux;
  a.g.ld_aux = ld_aux;
  a.g.w = view(w, out, ldo, bias, bias_ld);
  const bool small = m <= kMinTermSmallM && size_t(m) * w.ng * sizeof(float) <= kMinTermSmallLds;
  if (!small && a.mins && !S) {
    float* sums = static_cast<float*>(workspace_for(size_t(m) * w.ng * sizeof(float), st));
    if (!sums) return -1;
    const hipError_t e = planned(0, 0, 0, 1, 0, false) ? hipSuccess : launch_block_sums(act, act_t, lda, m, k, sums, st);
    if (e != hipSuccess) {
      set_err("activation block-sum launch failed: %s", hipGetErrorString(e));
      return -1;
    }
    a.S = sums;
    a.s_ld = w.ng;
    a.s_st = 1;
  }
  const hipError_t e = planned(0, 0, 0, 1, 0, false)
                           ? hipSuccess
                           : (small ? launch_min_term(a, act_t, st) : launch_min_term_tiled(a, st));
  if (e != hipSuccess) {
    set_err("min-term kernel launch failed: %s", hipGetErrorString(e));
    return -1;
  }
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

// ------------------------------------------------------------------------------------------------ GGUF Q4_0
extern "C" size_t nad_q4_0_device_size(int n, int k) {
  if (n <= 0 || k <= 0 || k % 32) {
    set_err("Q4_0 needs n > 0 and k a positive multiple of 32 (n=%d k=%d)", n, k);
    return 0;
  }
  DeviceWeight w{};
  return layout_geometry(w, 4, n, k, 32, kScaleF16, false, false);
}

extern "C" int nad_q4_0_device_load(const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity,
                                    void* queue) {
  const size_t need = nad_q4_0_device_size(n, k);
  if (!need) return -1;
  if (!blocks || !devstor || !deviceptr || capacity < need) {
    set_err("nad_q4_0_device_load: null pointer or device buffer too small (need %zu, have %zu)", need, capacity);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  DeviceWeight w{};
  layout_geometry(w, 4, n, k, 32, kScaleF16, false, false);
  layout_assign(w, deviceptr);
  w.src_core_id = kGgufQ4_0;
  w.owner = nullptr;
  {  // block_q4_0: fp16 d, then 16 bytes of nibbles; q in [-8, 7]
    const uint8_t* bp = static_cast<const uint8_t*>(blocks);
    bool ok = true;
    for (size_t i = 0; ok && i < size_t(n) * (k / 32); i++) {
      uint16_t h;
      std::memcpy(&h, bp + 18 * i, 2);
      ok = scale_in_fold_range(float(__builtin_bit_cast(_Float16, h)), 8.f);
    }
    w.fold_ok = ok ? 1 : 0;
  }
  // padding columns / K tiles: nibble 8 = q 0, scale 0
  HIP_OK(hipMemsetAsync(w.tiles, 0x88, size_t(w.ns) * w.nt * 1024, st));
  HIP_OK(hipMemsetAsync(w.scales, 0, size_t(w.ns) * w.ng * 16 * 2, st));
  const size_t bytes = size_t(n) * (k / 32) * 18;
  uint8_t* stage = nullptr;
  HIP_OK(hipMalloc(&stage, bytes));
  HIP_OK(hipMemcpyAsync(stage, blocks, bytes, hipMemcpyHostToDevice, st));
  hipError_t e = launch_q4_0_repack(stage, n, k, w, st);
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipFree(stage));
  if (e != hipSuccess) {
    set_err("Q4_0 repack launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}

extern "C" int nad_quant_q8_0(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue) {
  if (m <= 0 || k <= 0 || k % 32 || lda < k || !blocks) {
    set_err("nad_quant_q8_0: bad arguments (m=%d k=%d lda=%d)", m, k, lda);
    return -1;
  }
  Q80Args a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.blocks = static_cast<int8_t*>(blocks);
  hipError_t e = launch_q8_0_quant(a, act_dtype, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("Q8_0 quantization launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// ------------------------------------------------------------------------------- GGUF Q4_1 / Q5_0 / Q5_1 / Q8_0
extern "C" size_t nad_gguf_block_bytes(int type) {
  switch (type) {
    case NAD_GGUF_Q4_0: return 18;
    case NAD_GGUF_Q4_1: return 20;
    case NAD_GGUF_Q5_0: return 22;
    case NAD_GGUF_Q5_1: return 24;
    case NAD_GGUF_Q8_0: return 34;
    default:
      set_err("GGUF type %d is not supported (Q4_0 = 2, Q4_1 = 3, Q5_0 = 6, Q5_1 = 7, Q8_0 = 8)", type);
      return 0;
  }
}

// geometry of a GGUF matrix of the four new types: Q4_1 in the symmetric int4 layout, the others in the symmetric int8
// layout; the fp16 mins of Q4_1 / Q5_1 follow the layout's own regions
static uint64_t gguf_geometry(DeviceWeight& w, int type, int n, int k, uint64_t* mins_off) {
  const bool q41 = type == NAD_GGUF_Q4_1;
  const uint64_t base = layout_geometry(w, q41 ? 4 : 8, n, k, 32, kScaleF16, false, false);
  const bool has_m = q41 || type == NAD_GGUF_Q5_1;
  if (mins_off) *mins_off = base;
  return base + (has_m ? align256(uint64_t(w.ns) * w.ng * 16 * 2) : 0);
}

extern "C" size_t nad_gguf_device_size(int type, int n, int k) {
  if (!nad_gguf_block_bytes(type)) return 0;
  if (type == NAD_GGUF_Q4_0) return nad_q4_0_device_size(n, k);
  if (n <= 0 || k <= 0 || k % 32) {
    set_err("a GGUF matrix needs n > 0 and k a positive multiple of 32 (type=%d n=%d k=%d)", type, n, k);
    return 0;
  }
  DeviceWeight w{};
  return gguf_geometry(w, type, n, k, nullptr);
}

extern "C" int nad_gguf_device_load(int type, const void* blocks, int n, int k, void* devstor, void* deviceptr,
                                    size_t capacity, void* queue) {
  const size_t bb = nad_gguf_block_bytes(type);
  if (!bb) return -1;
  if (type == NAD_GGUF_Q4_0) return nad_q4_0_device_load(blocks, n, k, devstor, deviceptr, capacity, queue);
  const size_t need = nad_gguf_device_size(type, n, k);
  if (!need) return -1;
  if (!blocks || !devstor || !deviceptr || capacity < need) {
    set_err("nad_gguf_device_load: null pointer or device buffer too small (need %zu, have %zu)", need, capacity);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  DeviceWeight w{};
  uint64_t mins_off = 0;
  const uint64_t total = gguf_geometry(w, type, n, k, &mins_off);
  layout_assign(w, deviceptr);
  const bool has_m = total > mins_off;
  if (has_m) {
    w.mins = static_cast<char*>(deviceptr) + mins_off;
    w.bytes = total;
    w.min_bias = type == NAD_GGUF_Q4_1 ? 8 : 0;  // the nibble holds q, the layout decodes q - 8
  }
  w.owner = nullptr;
  w.src_core_id = type == NAD_GGUF_Q4_1 ? kGgufQ4_1
                  : type == NAD_GGUF_Q5_0 ? kGgufQ5_0
                  : type == NAD_GGUF_Q5_1 ? kGgufQ5_1
                                          : kGgufQ8_0;
  {  // every block starts with the fp16 d; the largest |decoded value| of the type
    const float qmax = type == NAD_GGUF_Q4_1 ? 8.f : (type == NAD_GGUF_Q5_0 ? 16.f : (type == NAD_GGUF_Q5_1 ? 31.f : 128.f));
    const uint8_t* bp = static_cast<const uint8_t*>(blocks);
    bool ok = true;
    for (size_t i = 0; ok && i < size_t(n) * (k / 32); i++) {
      uint16_t h;
      std::memcpy(&h, bp + bb * i, 2);
      ok = scale_in_fold_range(float(__builtin_bit_cast(_Float16, h)), qmax);
    }
    w.fold_ok = ok ? 1 : 0;
  }
  // padding columns / K tiles decode to 0: int8 byte 128, nibble 8; scale 0, min 0
  const size_t entries = size_t(w.ns) * w.ng * 16;
  HIP_OK(hipMemsetAsync(w.tiles, w.bits == 4 ? 0x88 : 0x80, size_t(w.ns) * w.nt * 1024, st));
  HIP_OK(hipMemsetAsync(w.scales, 0, entries * 2, st));
  if (w.mins) HIP_OK(hipMemsetAsync(w.mins, 0, entries * 2, st));
  const size_t bytes = size_t(n) * (k / 32) * bb;
  uint8_t* stage = nullptr;
  HIP_OK(hipMalloc(&stage, bytes));
  // copy, repack, wait; the staging buffer is freed on every way out
  const char* what = "hipMemcpyAsync of the blocks";
  hipError_t e = hipMemcpyAsync(stage, blocks, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    what = "GGUF repack launch";
    e = launch_gguf_repack(type, stage, n, k, w, st);
  }
  const hipError_t es = hipStreamSynchronize(st);  // also after a failure: the copy may still read `blocks`
  if (e == hipSuccess && es != hipSuccess) {
    what = "hipStreamSynchronize";
    e = es;
  }
  const hipError_t ef = hipFree(stage);
  if (e == hipSuccess && ef != hipSuccess) {
    what = "hipFree of the staging buffer";
    e = ef;
  }
  if (e != hipSuccess) {
    set_err("nad_gguf_device_load: %s failed: %s", what, hipGetErrorString(e));
    return -1;
  }
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}

extern "C" int nad_quant_q8_1(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue) {
  if (m <= 0 || k <= 0 || k % 32 || lda < k || !blocks) {
    set_err("nad_quant_q8_1: bad arguments (m=%d k=%d lda=%d)", m, k, lda);
    return -1;
  }
  Q81Args a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.blocks = static_cast<int8_t*>(blocks);
  hipError_t e = launch_q8_1_quant(a, act_dtype, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("Q8_1 quantization launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

// fp16 activations for the pipelined prefill GEMM (woq_gemm2.hip): the caller's rows when they already are fp16,
// aligned, unshuffled and tile-padded, else one conversion pass into the workspace.  One conversion serves every GEMM
// that reads the same activations (the QKV and gate/up fusions).
struct A16 {
  const _Float16* p = nullptr;
  int ld = 0;
  int kp = 0;
};

// 3: gemm3 (int4, groups of 128 * 2^j); 4: gemm4 (int4 g32 / g64, int2 groups >= 64); 0: register-staged fallback
static int pipelined_gemm(const DeviceWeight& w, int m) {
  const Knobs& kn = knobs();
  if (kn.gemm2_disable || w.kmajor || w.f4kind >= 0 || m <= 16 ||
      uint64_t(m) * uint64_t(w.nt) * 512 >= (1ull << 32))
    return 0;
  const int tpg = w.blocksize / 128;
  if (w.bits == 4 && w.blocksize % 128 == 0 && (tpg & (tpg - 1)) == 0 && !kn.gemm4_all) return 3;
  // int4 groups of 32 / 64 and int2 / int8 with a foldable q * s: gemm7 with the group scale per 32-deep step or per
  // half step (profiles/r05_gemm7_g32*, r05_gemm7_int2_int8*; NAD_GEMM4_FOLD=0, the exact fp32 group scales, or
  // NAD_GEMM_KERNEL=3 keep gemm4)
  if ((w.bits == 4 || w.bits == 2 || w.bits == 8) && gemm7_ok(w.bits, w.blocksize, w.fold_ok) &&
      kn.gemm_kernel == 7 && kn.gemm4_fold && !kn.gemm4_all)
    return 3;
  if (!kn.gemm4_disable && gemm4_mode(w.bits, w.blocksize, w.ng, w.nt * tile_k(w.bits), w.asym)) return 4;
  return 0;
}
static bool gemm2_ok(const DeviceWeight& w, int m) { return pipelined_gemm(w, m) != 0; }
static int k_tile(const DeviceWeight& w) { return w.bits == 4 ? 128 : (w.bits == 2 ? 256 : 64); }
// The FFN's prefill keeps its intermediates in fp16 when all three GEMMs are the pipelined ones reading the unshuffled
// fp16 operand and fmid is a whole number of w2's K tiles (NAD_FFN_F32=1: the fp32 intermediates, A/B)
static bool ffn16_ok(const DeviceWeight& w1, const DeviceWeight& w2, const DeviceWeight& w3, int m, int fmid) {
  auto ok = [&](const DeviceWeight& w) {
    return pipelined_gemm(w, m) && !w.shuffle && !int8_compute(w);
  };
  return !knobs().ffn_f32 && knobs().gemm_kernel != 2 && ok(w1) && ok(w2) && ok(w3) &&
         w2.nt * k_tile(w2) == fmid && fmid % 8 == 0;
}

// 1 ready, -1 error (no workspace under capture, launch error)
static int prepare_a16(A16& r, const void* act, int act_t, int lda, int m, int k, const DeviceWeight& w,
                       hipStream_t st) {
  const int kp = w.nt * k_tile(w);
  r.kp = kp;
  if (act_t == kActF16 && !w.shuffle && k == kp && reinterpret_cast<uintptr_t>(act) % 16 == 0 &&
      (size_t(lda) * 2) % 16 == 0) {
    r.p = static_cast<const _Float16*>(act);
    r.ld = lda;
    return 1;
  }
  _Float16* buf = static_cast<_Float16*>(workspace_for(size_t(m) * kp * 2, st));
  if (!buf) return -1;
  hipError_t e = planned(0, 0, 0, 1, 0, false) ? hipSuccess : launch_cvt_act(act, act_t, lda, m, k, kp, w.shuffle, buf, st);
  if (e != hipSuccess) {
    set_err("activation conversion launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  r.p = buf;
  r.ld = kp;
  return 1;
}

// Split-K plan of a pipelined GEMM whose 256 x 128 output tiles alone leave most CUs idle (M up to a few hundred, or
// narrow N): runs of whole groups, at least two K tiles each, at most one workgroup per CU in total.  Returns the run
// count (1 = no split) and the K tiles per run.
static int splitk_plan(const DeviceWeight& w, int m, int* ktiles, int bm = 256) {
  *ktiles = w.nt;
  if (knobs().splitk_disable) return 1;
  const int tiles = ((m + bm - 1) / bm) * ((w.ns + 7) / 8);
  if (tiles > 128) return 1;
  const int tpg = std::max(1, w.blocksize / k_tile(w));
  const int unit = tpg >= 2 ? tpg : 2;  // K tiles per run at least: one whole group and two tiles
  int s = std::min(256 / tiles, w.nt / unit);
  if (s < 2) return 1;
  int kt = (w.nt + s - 1) / s;
  kt = (kt + tpg - 1) / tpg * tpg;
  s = (w.nt + kt - 1) / kt;
  if (s < 2) return 1;
  *ktiles = kt;
  return s;
}
// fp16 result / SiLU*mul operand of a pipelined GEMM (the FFN's intermediates, ffn16_ok)
struct Half16 {
  _Float16* out = nullptr;
  int ldo = 0;
  const _Float16* aux = nullptr;
};

// The mid-M GEMM (woq_gemm_mid.hip) for 17 <= M <= 64 (NAD_MID_MIN_M / NAD_MID_MAX_M): integer int4 / int2 weights,
// stripe-major, no act-order gather, 16-B aligned activation rows with K % 8 == 0 (int2 and int4 g32: M <= 32).
// Stripe groups of 4 x K runs of one chunk (8 K tiles int4, 4 int2: mid_geometry) each, so K = 4096 splits 4 ways and
// the 256 / 688 / 768 stripes of the Llama shapes give 256 / 688 / 768 workgroups; the runs' fp32 slabs are summed by
// the split-K reduce launch.  Returns 1 if launched, 0 if not eligible, -1 on error.
static int run_mid(const void* act, int act_t, int lda, int m, int k, const DeviceWeight& w, float* out, int ldo,
                   int epi, const float* bias, int bias_ld, const float* res, int ld_res, const float* aux, int ld_aux,
                   hipStream_t st, const A16* pre, const Half16* h16) {
  const Knobs& kn = knobs();
  if (m > kn.mid_max_m || m < (kn.mid_min_m > 0 ? kn.mid_min_m : 8)) return 0;
  if ((w.bits != 4 && w.bits != 2) || w.kmajor || w.f4kind >= 0 || w.shuffle) return 0;
  if (w.bits == 2 && m > 32) return 0;  // a 256-deep int2 stage's activation fragments: 32 rows fit the registers
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(w.bits, w.nt, w.ng, w.blocksize, &tpg);
  if (gpt != 1 && gpt != 2 && gpt != 4) return 0;
  if (gpt == 4 && m > 32) return 0;  // 4 groups per tile x 4 stripes of scales beside 64 rows: out of registers
  // a fused caller's shared fp16 copy of A (pre) is not read: the kernel converts the caller's activations itself, so a
  // fused QKV / FFN launch is bit-identical to the same weights' single launches; its split-K slabs go past where such a
  // copy sits in the workspace (the weights after this one may still read it)
  (void)pre;
  if (!vec_aligned(act, lda, act_t) || k % 8 != 0) return 0;
  const int esz = act_t == kActF32 ? 4 : 2;
  if (uint64_t(m) * lda * esz >= (1ull << 31) || uint64_t(w.ns) * w.nt * 1024 >= (1ull << 31)) return 0;
  const int rf = (m + 15) / 16;
  int sps = 0, nw = 0, spw = 0, nsg = 0, ks = 0;
  // runs per stripe group: one chunk each, the slabs within nad_device_workspace_size's N-independent bound (m x 128 KiB
  // past the fp16 copy): ks x N <= 32768, so wide weights split K less (N = 11008: 2 runs; N = 32000: none)
  auto plan = [&](int wide) {
    mid_geometry(w.bits, gpt, act_t, rf, wide, &sps, &nw, &spw);
    const int chunk = nw * spw;
    nsg = (w.ns + sps - 1) / sps;
    ks = std::max(1, std::min((w.nt + chunk - 1) / chunk, 32768 / ((w.n + 3) / 4 * 4)));
    if (kn.mid_ks > 0) ks = std::max(1, std::min({kn.mid_ks, w.nt, 32768 / ((w.n + 3) / 4 * 4)}));
  };
  plan(kn.mid_wide == 1);
  // from 8 rows of fp32 / bf16 activations (the GEMV stages them as two fp16 rows each) the mid-M kernel beats the
  // stripe-stream GEMV: K = N = 4096 M = 16 8.3 vs 10.1 us (fp16), 9.0 vs 12.7 (fp32); N = 11008 fp32 M = 16 17.7 vs
  // 36.7 (profiles/r05_mid_small_m.txt).  fp16 rows: from 9 where the stripe groups x K runs fit the CUs in one round
  // (K = N = 4096 M = 10: 7.7 vs 8.7 us), else from 12 (N = 11008 M = 8: GEMV 12.1 vs 14.2; profiles/r06_mid_min_m_ab.txt)
  if (kn.mid_min_m <= 0 && act_t == kActF16 && m < (nsg * ks <= device_cus() ? 9 : 12)) return 0;
  // 8-stripe workgroups (where mid_geometry has them) when the 4-stripe grid takes more than one workgroup per CU and
  // theirs does not: N = 11008, M = 16 / 32: 344 -> 172 workgroups, 16.3 -> 14.3-14.9 us, 21.1 -> 18.8
  // (profiles/r06_mid_wide_ab.txt); at N = 4096 (256 either way) the 8-stripe form's doubled slabs cost 0.7-1 us
  if (kn.mid_wide == 2 && sps == 4 && nsg * ks > device_cus()) {
    const int s4 = sps, n4 = nsg, k4 = ks, w4 = spw;
    plan(1);
    if (sps == 4 || nsg * ks > device_cus()) {
      sps = s4;
      nsg = n4;
      ks = k4;
      spw = w4;
    }
  }
  const int ktiles = (w.nt + ks - 1) / ks;
  ks = (w.nt + ktiles - 1) / ktiles;
  GemmArgs a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.scale_t = w.scale_t;
  a.epi = epi;
  a.res = res;
  a.ld_res = ld_res;
  a.aux = aux;
  a.ld_aux = ld_aux;
  a.tpg_shift = tpg == 0 ? 31 : __builtin_ctz(unsigned(tpg));
  a.w = view(w, out, ldo, bias, bias_ld);
  if (h16) {
    a.out16 = h16->out;
    a.ldo16 = h16->ldo;
    a.aux16 = h16->aux;
  }
  if (ks > 1) {
    a.ksplit = ks;
    a.ktiles = ktiles;
    a.ldp = (w.n + 3) / 4 * 4;
    if (uint64_t(ks) * m * a.ldp * 4 >= (1ull << 31)) return 0;
    const size_t a16 = (size_t(m) * ((size_t(k) + 255) / 256 * 256) * 2 + 255) / 256 * 256;  // an fp16 copy's room
    char* base = static_cast<char*>(workspace_for(a16 + size_t(ks) * m * a.ldp * 4, st));
    if (!base) return -1;
    a.part = reinterpret_cast<float*>(base + a16);
  } else {
    a.ktiles = w.nt;
  }
  // a stripe group's runs and the reduce of their slabs on one XCD: the reduce reads the slabs from that XCD's L2
  // instead of memory (K = N = 4096: M = 64 14.3 -> 12.7 us, M = 32 10.3 -> 9.5; profiles/r06_mid_xcd_ab.txt)
  if (ks > 1 && kn.mid_xcd) {
    a.xcd_sg = nsg;
    a.xcd_w = sps * 4;
  }
  const int grid = nsg * ks;
  if (planned(NAD_KERNEL_MID, grid, nw * 64, ks, 0)) {
    if (ks > 1) planned(0, 0, 0, 1, 0, false);  // the split-K reduce
    return 1;
  }
  hipError_t e = launch_gemm_mid(a, w.bits, gpt, act_t, rf, sps, grid, st);
  if (e == hipSuccess && ks > 1) e = launch_splitk_reduce(a, st);
  if (e != hipSuccess) {
    set_err("mid-M GEMM launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 1;
}

// gemm7's tile height (32 rows up to M = 32, else 64 / 128 / 256) by a cost model fitted to the K = 4096, N = 4096 /
// 11008 sweeps (profiles/r05_gemm7_tile_height_sweep.txt): a launch takes the rounds of workgroups over the CUs, each
// a fixed P (prologue, epilogue, output stores) plus its K run's half steps at h per half step (h grows with the tile
// height: 0.35 / 0.55 / 0.95 us at 64 / 128 / 256 rows), plus, with split K, the reduce launch and the fp32 slabs
// (written and read once, ~5 TB/s).  Picks within ~10 % of the best measured height at every swept M (the fixed
// M-thresholds it replaces were up to 35 % off: N = 4096, M = 256 31.1 us against 22.7 with 64-row tiles).
static int gemm7_pick_bm(const DeviceWeight& w, int m) {
  if (m <= 32) return 32;
  static const int bms[3] = {64, 128, 256};
  static const double hs_us[3] = {0.35, 0.55, 0.95}, fixed_us[3] = {5.5, 5.0, 8.0};
  const int cus = device_cus();
  const int hpt = k_tile(w) / 64;
  int best = 256;
  double best_t = 1e30;
  for (int i = 0; i < 3; i++) {
    int kt = w.nt;
    const int ks = splitk_plan(w, m, &kt, bms[i]);
    const long tiles = long((m + bms[i] - 1) / bms[i]) * ((w.ns + 7) / 8);
    const long rounds = (tiles * ks + cus - 1) / cus;
    // 64-row tiles over the whole K (no split): 7.9 us fixed, refitted on the split-K XCD placement's sweep (K = N =
    // 4096, M = 320 / 384: 64-row tiles 30.0 / 30.3 us, 128-row tiles with 2 runs 27.3 / 28.2;
    // profiles/r06_gemm7_tile_height_xcd.txt)
    const double fx = bms[i] == 64 && ks == 1 && knobs().gemm7_model != 1 ? 7.9 : fixed_us[i];
    double t = double(rounds) * (fx + double(kt) * hpt * hs_us[i]);
    if (ks > 1) t += 2.0 + double(m) * w.n * ks * 8.0 / 5e6;
    if (t < best_t) {
      best_t = t;
      best = bms[i];
    }
  }
  return best;
}

static int run_gemm(const void* act, int act_t, int lda, int m, int k, const DeviceWeight& w, float* out, int ldo,
                    int epi, const float* bias, int bias_ld, const float* res, int ld_res, const float* aux,
                    int ld_aux, hipStream_t st, const A16* pre = nullptr, const Half16* h16 = nullptr) {
  if (int8_compute(w)) {
    const DeviceWeight* ws[1] = {&w};
    float* outs[1] = {out};
    const int ldos[1] = {ldo};
    return run_i8(act, act_t, lda, m, k, 1, ws, outs, ldos, false, epi, bias, bias_ld, res, ld_res, aux, ld_aux, st);
  }
  {
    const int r = run_mid(act, act_t, lda, m, k, w, out, ldo, epi, bias, bias_ld, res, ld_res, aux, ld_aux, st, pre, h16);
    if (r != 0) return r < 0 ? -1 : 0;
  }
  GemmArgs a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.scale_t = w.scale_t;
  a.epi = epi;
  a.vec_ok = vec_aligned(act, lda, act_t) ? 1 : 0;
  a.res = res;
  a.ld_res = ld_res;
  a.aux = aux;
  a.ld_aux = ld_aux;
  const Knobs& kn = knobs();
  a.stagger = kn.gemm3_stagger;  // measured +3-7 % (profiles/r02_gemm3_stagger.txt)
  // scale folding measured 1-5 % SLOWER on gemm3 (profiles/r03_gemm3_fold.txt): gemm3 keeps the exact fp32 group scale
  a.fold = 0;
  a.w = view(w, out, ldo, bias, bias_ld);
  const int pg = pipelined_gemm(w, m);
  // gemm4 at groups of 32 / 64 scales the products into the result every 32 / 64 k (4 / 2 FMAs per MFMA): there the
  // fold pays, +14-23 %; at groups of 128 (int2 / int8: int4 g128 runs gemm3) it measured +6-21 % with the int2 stagger
  // it enables (profiles/r03_gemm4_g128_fold.txt), the default since the full GPU suite ran green with it
  // (profiles/r04_pytest_gpu_foldall.log; NAD_GEMM4_FOLD_ALL=0 keeps g128 unfolded); NAD_GEMM4_FOLD=0 restores the exact
  // fp32 per-group path everywhere (gemm4 scale folding)
  if (pg == 4 && (w.blocksize == 32 || w.blocksize == 64 || kn.gemm4_fold_all))
    a.fold = w.fold_ok && kn.gemm4_fold ? 1 : 0;
  // KSW (waves split over K, each B fragment dequantized once per workgroup): measured +8-18 % on launches of more than
  // one round of output tiles or long K (gate 11008 x 4096, down 4096 x 11008 at M = 2048) and 0-7 % slower on a single
  // round at K = 4096 (4096 x 4096, 256 tiles; profiles/r04_gemm4_ksw_ab.txt): auto picks it for the former
  if (pg == 4 && a.fold) {
    const int tiles = ((m + 255) / 256) * ((w.n + 127) / 128);
    const bool win = tiles > device_cus() || w.nt * k_tile(w) >= 8192;
    a.ksw = kn.gemm4_ksw == 1 || (kn.gemm4_ksw == 2 && win) ? 1 : 0;
  }
  if (h16) {
    if (!pg) {
      set_err("fp16 GEMM output needs the pipelined GEMM");
      return -1;
    }
    a.out16 = h16->out;
    a.ldo16 = h16->ldo;
    a.aux16 = h16->aux;
  }
  if (pg) {
    A16 own;
    if (!pre || pre->kp != w.nt * k_tile(w) || w.shuffle) {
      if (prepare_a16(own, act, act_t, lda, m, k, w, st) < 0) return -1;
      pre = &own;
    }
    const bool g2 = pg == 3 && kn.gemm_kernel == 2;
    // gemm7 (group scale folded, waves split over K) is the default for int4 groups of 128 * 2^j: +5-10 % over gemm3
    // (profiles/r05_gemm7_*); a weight whose q * s leaves the fp16 normal range, or NAD_GEMM_KERNEL=3, runs gemm3
    // (as for gemm4, NAD_GEMM4_FOLD=0 turns the fold off: int4 g128 then runs gemm3's exact fp32 group scale)
    const bool g7 = pg == 3 && kn.gemm_kernel == 7 && kn.gemm4_fold && gemm7_ok(w.bits, w.blocksize, w.fold_ok);
    if (g7) a.fold = 1;
    int bm = 256;
    if (g7) {
      bm = kn.gemm7_bm > 0 ? kn.gemm7_bm : gemm7_pick_bm(w, m);
      if (bm != 32 && bm != 64 && bm != 128) bm = 256;
    }
    int ktiles = w.nt;
    const int ks = !g2 ? splitk_plan(w, m, &ktiles, bm) : 1;
    if (ks > 1 && kn.gemm4_ksw == 2) a.ksw = 0;  // auto KSW was measured on whole-K launches only
    if (ks > 1) {  // partials after the fp16 activations in the same workspace (stream-ordered reuse)
      a.ksplit = ks;
      a.ktiles = ktiles;
      a.ldp = (w.n + 3) / 4 * 4;
      const size_t a16 = (size_t(m) * w.nt * k_tile(w) * 2 + 255) / 256 * 256;
      char* base = static_cast<char*>(workspace_for(a16 + size_t(ks) * m * a.ldp * 4, st));
      if (!base) return -1;
      a.part = reinterpret_cast<float*>(base + a16);
    }
    const int tiles = ((m + bm - 1) / bm) * ((w.n + 127) / 128);
    // split K: every run of a tile and the reduce of its slabs on one XCD (slabs read back from that XCD's L2): K = N =
    // 4096 M = 128 18.6 -> 15.9 us, M = 96 17.2 -> 14.8 (profiles/r06_gemm7_xcd_splitk_ab.txt)
    if (g7 && ks > 1 && kn.gemm_xcd && (((m + bm - 1) / bm) * ((w.ns + 7) / 8)) % 8 == 0) a.xcd_tile = bm;
    if (planned(pg == 4 ? NAD_KERNEL_GEMM4 : (g2 ? NAD_KERNEL_GEMM2 : (g7 ? NAD_KERNEL_GEMM7 : NAD_KERNEL_GEMM3)),
                tiles * ks, 512, ks, a.fold | (a.ksw << 1))) {
      if (ks > 1) planned(0, 0, 0, 1, 0, false);  // the split-K reduce
      return 0;
    }
    hipError_t e = pg == 4 ? launch_gemm4(a, w.bits, pre->p, pre->ld, st)
                   : g2    ? launch_gemm2(a, pre->p, pre->ld, st)
                   : g7    ? launch_gemm7(a, w.bits, bm, pre->p, pre->ld, st)
                           : launch_gemm3(a, pre->p, pre->ld, st);
    if (e == hipSuccess && ks > 1) e = launch_splitk_reduce(a, st);
    if (e != hipSuccess) {
      set_err("gemm2 kernel launch failed: %s", hipGetErrorString(e));
      return -1;
    }
    return 0;
  }
  hipError_t e = planned(NAD_KERNEL_GEMM, 0, 0) ? hipSuccess : launch_gemm(a, w.bits, act_t, st);
  if (e != hipSuccess) {
    set_err("gemm kernel launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

static constexpr int kSkinnyMaxM = 16;

static bool check_shape(const DeviceWeight& w, int m, int n, int k, int lda, int ldo) {
  if (m <= 0 || n != w.n || k != w.k) {
    set_err("shape mismatch: call (m=%d, n=%d, k=%d) vs weight (n=%d, k=%d)", m, n, k, w.n, w.k);
    return false;
  }
  if (lda < k || ldo < n) {
    set_err("lda (%d) < k (%d) or ldo (%d) < n (%d)", lda, k, ldo, n);
    return false;
  }
  return true;
}

static int forward_one(const void* act, int act_dtype, int lda, int m, int k, const DeviceWeight& w, float* out,
                       int ldo, int epi, const float* bias, int bias_ld, const float* res, int ld_res, hipStream_t st);
static int forward_min(const void* act, int act_dtype, int lda, int m, int k, const DeviceWeight& w, float* out,
                       int ldo, int epi, const float* bias, int bias_ld, const float* res, int ld_res,
                       const float* aux, int ld_aux, hipStream_t st);

extern "C" int nad_device_forward(const void* act, int act_dtype, const void* devstor, float* out, int m, int n, int k,
                                  int lda, int ldo, int epi, const float* bias, int bias_ld, const float* res,
                                  int ld_res, void* queue) {
  const DeviceWeight* w = as_weight(devstor);
  if (!w || !check_shape(*w, m, n, k, lda, ldo)) return -1;
  if (epi == kEpiSiluMul || epi == kEpiGeluMul) {
    set_err("dual epilogues go through nad_device_ffn_forward");
    return -1;
  }
  if ((epi == kEpiBias || epi == kEpiAddGelu) && !bias) {
    set_err("bias epilogue without bias");
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  if (w->mins)
    return forward_min(act, act_dtype, lda, m, k, *w, out, ldo, epi, bias, bias_ld, res, ld_res, nullptr, 0, st);
  return forward_one(act, act_dtype, lda, m, k, *w, out, ldo, epi, bias, bias_ld, res, ld_res, st);
}

// one weight, one launch chain: the body of nad_device_forward
static int forward_one(const void* act, int act_dtype, int lda, int m, int k, const DeviceWeight& wr, float* out,
                       int ldo, int epi, const float* bias, int bias_ld, const float* res, int ld_res,
                       hipStream_t st) {
  const DeviceWeight* w = &wr;
  if (m <= kSkinnyMaxM) {
    // the mid-M kernel from 9 rows of fp16 activations where its grid fits the CUs in one round, else from 12, and from 8
    // rows of fp32 / bf16 (run_mid; NAD_MID_MIN_M overrides); below that, and for the
    // fused QKV / FFN entries at any M <= 16, the skinny GEMV.  Its split-K slabs fit nad_device_workspace_size(m, k).
    if (!int8_compute(*w)) {
      const int r = run_mid(act, act_dtype, lda, m, k, *w, out, ldo, epi, bias, bias_ld, res, ld_res, nullptr, 0, st,
                            nullptr, nullptr);
      if (r != 0) return r < 0 ? -1 : 0;
    }
    float* outs[1] = {out};
    int ldos[1] = {ldo};
    const DeviceWeight* ws[1] = {w};
    return run_skinny(act, act_dtype, lda, m, k, 1, ws, outs, ldos, epi, bias, bias_ld, res, ld_res, nullptr, 0, st);
  }
  return run_gemm(act, act_dtype, lda, m, k, *w, out, ldo, epi, bias, bias_ld, res, ld_res, nullptr, 0, st);
}

// A weight with block mins (GGUF Q4_1 / Q5_1), or the partner of one in a fused FFN: the unchanged kernels compute
// X (q d)^T into out, the min-term pass adds S mins^T and applies the epilogue (aux: the SILU_MUL / GELU_MUL operand).
// In the int8 mode the Q8_1 sums replace S and run_i8 appends the pass itself.
static int forward_min(const void* act, int act_dtype, int lda, int m, int k, const DeviceWeight& w, float* out,
                       int ldo, int epi, const float* bias, int bias_ld, const float* res, int ld_res,
                       const float* aux, int ld_aux, hipStream_t st) {
  if (int8_compute(w)) {
    const DeviceWeight* ws[1] = {&w};
    float* outs[1] = {out};
    const int ldos[1] = {ldo};
    const int e = epi == kEpiGeluMul ? kEpiSiluMul : epi;
    return run_i8(act, act_dtype, lda, m, k, 1, ws, outs, ldos, false, e, bias, bias_ld, res, ld_res, aux, ld_aux, st);
  }
  if (forward_one(act, act_dtype, lda, m, k, w, out, ldo, kEpiNone, nullptr, 0, nullptr, 0, st)) return -1;
  return min_term(act, act_dtype, lda, nullptr, 0, 0, m, k, w, out, ldo, epi, bias, bias_ld, res, ld_res, aux, ld_aux,
                  st);
}

extern "C" void bestla_device_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k,
                                             int lda, int ldo, void* workspace, void* queue) {
  CallWorkspace cw(workspace, nad_device_workspace_size(_m, _k));
  if (nad_device_forward(activation, kActF32, weiptr, output, _m, _n, _k, lda, ldo, kEpiNone, nullptr, 0, nullptr, 0,
                         queue) != 0)
    report("bestla_device_f32f32_forward");
}

static int plan_for(const DeviceWeight& w, int m, int act_dtype, int64_t* out, int nout) {
  if (!out || nout < 0 || m <= 0) {
    set_err("nad_plan_*: bad arguments (m=%d)", m);
    return -1;
  }
  NadPlan plan;
  t_plan = &plan;
  const void* act = reinterpret_cast<const void*>(uintptr_t(1) << 42);  // aligned, never dereferenced on the host
  float* y = reinterpret_cast<float*>(uintptr_t(1) << 43);
  const int rc = nad_device_forward(act, act_dtype, &w, y, m, w.n, w.k, w.k, w.n, kEpiNone, nullptr, 0, nullptr, 0,
                                    nullptr);
  t_plan = nullptr;
  if (rc) return -1;
  const int64_t v[6] = {plan.kernel, plan.grid, plan.block, plan.ksplit, plan.fold, plan.launches};
  const int c = nout < 6 ? nout : 6;
  std::memcpy(out, v, sizeof(int64_t) * size_t(c));
  return c;
}

extern "C" int nad_plan_forward(int bits, int n, int k, int blocksize, int scale_t, int asym, int m, int act_dtype,
                                int64_t* out, int nout) {
  if ((bits != 2 && bits != 4 && bits != 8) || n <= 0 || k <= 0) {
    set_err("nad_plan_forward: bad arguments (bits=%d n=%d k=%d)", bits, n, k);
    return -1;
  }
  if (blocksize <= 0) blocksize = k;
  DeviceWeight w{};
  layout_geometry(w, bits, n, k, blocksize, scale_t, asym != 0, false, false);
  layout_assign(w, reinterpret_cast<void*>(uintptr_t(1) << 41));  // never dereferenced on the host
  w.f4kind = -1;
  w.fold_ok = 1;
  w.owner = nullptr;
  return plan_for(w, m, act_dtype, out, nout);
}

extern "C" int nad_plan_weight(const void* devstor, int m, int act_dtype, int64_t* out, int nout) {
  const DeviceWeight* w = as_weight(devstor);
  return w ? plan_for(*w, m, act_dtype, out, nout) : -1;
}

static bool same_kind(const DeviceWeight& a, const DeviceWeight& b) {
  return a.bits == b.bits && a.f4kind == b.f4kind && a.k == b.k && a.blocksize == b.blocksize &&
         a.scale_t == b.scale_t && a.nt == b.nt &&
         a.ng == b.ng && (a.shuffle == nullptr) == (b.shuffle == nullptr);
}

// Fused QKV prefill on gemm7: the weights' column tiles in ONE launch where each weight would run whole-K gemm7 at the
// same tile height on its own -- the same tiles and arithmetic as the separate launches (bit-identical outputs), one
// kernel boundary and one tail of output stores instead of n: Llama-2-7B at M = 2048 runs 3 x 256 tiles as 3 rounds of
// one launch (profiles/r06_gemm7_fused_qkv_ab.txt).  Returns 1 if launched, 0 if not eligible, -1 on error.
static int run_gemm7_fused(const void* act, int act_t, int lda, int m, int k, const DeviceWeight* const* ws, int n,
                           float* const* outs, const int* ldos, hipStream_t st, const A16* pre) {
  const Knobs& kn = knobs();
  if (n < 2 || n > 3 || !kn.gemm7_fuse || m <= kn.mid_max_m) return 0;
  // the fused instantiation (woq_gemm7_kernel<..., MW>): int4, one group per K tile or more
  if (ws[0]->bits != 4 || ws[0]->blocksize % 128 != 0) return 0;
  int bm0 = 0;
  for (int i = 0; i < n; i++) {
    const DeviceWeight& w = *ws[i];
    if (int8_compute(w) || w.shuffle || pipelined_gemm(w, m) != 3) return 0;
    if (kn.gemm_kernel != 7 || !kn.gemm4_fold || !gemm7_ok(w.bits, w.blocksize, w.fold_ok)) return 0;
    if (i > 0 && (!same_kind(w, *ws[0]) || (w.zps == nullptr) != (ws[0]->zps == nullptr))) return 0;
    int bm = kn.gemm7_bm > 0 ? kn.gemm7_bm : gemm7_pick_bm(w, m);
    if (bm != 32 && bm != 64 && bm != 128) bm = 256;
    int kt = w.nt;
    if (splitk_plan(w, m, &kt, bm) != 1) return 0;  // that weight's own launch splits K: other sums
    if (bm == 32 || (i > 0 && bm != bm0)) return 0;
    bm0 = bm;
  }
  GemmArgs a{};
  a.A = act;
  a.lda = lda;
  a.M = m;
  a.K = k;
  a.scale_t = ws[0]->scale_t;
  a.epi = kEpiNone;
  a.vec_ok = vec_aligned(act, lda, act_t) ? 1 : 0;
  a.fold = 1;
  a.w = view(*ws[0], outs[0], ldos[0], nullptr, 0);
  int cut = (ws[0]->ns + 7) / 8;
  a.nbn_cut[0] = a.nbn_cut[1] = cut;
  for (int i = 1; i < n; i++) {
    a.wf[i - 1] = view(*ws[i], outs[i], ldos[i], nullptr, 0);
    cut += (ws[i]->ns + 7) / 8;
    if (i == 1) a.nbn_cut[1] = cut;
  }
  a.nbn_all = cut;
  a.nwt = n;
  if (planned(NAD_KERNEL_GEMM7, ((m + bm0 - 1) / bm0) * cut, 512, 1, 1)) return 1;
  A16 own;
  if (!pre || pre->kp != ws[0]->nt * k_tile(*ws[0])) {
    if (prepare_a16(own, act, act_t, lda, m, k, *ws[0], st) < 0) return -1;
    pre = &own;
  }
  const hipError_t e = launch_gemm7(a, ws[0]->bits, bm0, pre->p, pre->ld, st);
  if (e != hipSuccess) {
    set_err("fused gemm7 launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 1;
}

extern "C" int nad_device_qkv_forward(const void* act, int act_dtype, const void* wq, const void* wk, const void* wv,
                                      float* oq, float* okk, float* ov, int m, int k, int lda, int ldo_q, int ldo_k,
                                      int ldo_v, void* queue) {
  const DeviceWeight* ws[3] = {as_weight(wq), as_weight(wk), as_weight(wv)};
  if (!ws[0] || !ws[1] || !ws[2]) return -1;
  if (ws[0]->k != k || ws[1]->k != k || ws[2]->k != k) {
    set_err("QKV fusion needs three weights with K = %d", k);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  float* outs[3] = {oq, okk, ov};
  int ldos[3] = {ldo_q, ldo_k, ldo_v};
  if (ws[0]->mins || ws[1]->mins || ws[2]->mins) {  // block mins: the three weights one after another
    for (int i = 0; i < 3; i++) {
      const DeviceWeight& w = *ws[i];
      const int rc = w.mins ? forward_min(act, act_dtype, lda, m, k, w, outs[i], ldos[i], kEpiNone, nullptr, 0, nullptr,
                                          0, nullptr, 0, st)
                            : forward_one(act, act_dtype, lda, m, k, w, outs[i], ldos[i], kEpiNone, nullptr, 0, nullptr,
                                          0, st);
      if (rc) return -1;
    }
    return 0;
  }
  if (m <= kSkinnyMaxM) {
    // one stream launch over every run of consecutive weights of one kind (Q, K and V may differ in N; a mixed-format
    // model such as the int2 policy's int4 wv gets {Q, K} + {V}), each output computed exactly as on its own
    auto kin = [&](int i, int j) { return same_kind(*ws[i], *ws[j]) && ws[i]->asym == ws[j]->asym; };
    if (m == 1 && kin(0, 1) && !kin(1, 2) && knobs().gemv_dual && !knobs().gemv_disable) {
      // {Q, K} int2 + {V} int4 at M = 1: ONE launch whose workgroups are split between the two formats by bytes
      GemvArgs a1, a2;
      int w1 = 0, w2 = 0, g1 = 0, g2 = 0, p1 = 0, p2 = 0;
      if (prepare_gemv(a1, w1, g1, p1, act, act_dtype, lda, 1, k, 2, ws, outs, ldos, kEpiNone, nullptr, 0, nullptr, 0,
                       nullptr, 0) &&
          prepare_gemv(a2, w2, g2, p2, act, act_dtype, lda, 1, k, 1, ws + 2, outs + 2, ldos + 2, kEpiNone, nullptr, 0,
                       nullptr, 0, nullptr, 0) &&
          w1 == 16 && w2 == 16 && gemv_dual_ok(a1, ws[0]->bits, a2, ws[2]->bits, 16)) {
        const double b1 = double(a1.units) * a1.nt, b2 = double(a2.units) * a2.nt;  // 1 KiB tiles of each part
        const int cus = device_cus();
        int n1 = int(cus * b1 / (b1 + b2) + 0.5);
        n1 = std::max(1, std::min(std::min(n1, cus - 1), a1.units));
        const int n2 = std::max(1, std::min(cus - n1, a2.units));
        a1.u_q = a1.units / n1;
        a1.u_r = a1.units % n1;
        a2.u_q = a2.units / n2;
        a2.u_r = a2.units % n2;
        const size_t lds = std::max(gemv_lds_layout(a1, ws[0]->bits, 16, n1), gemv_lds_layout(a2, ws[2]->bits, 16, n2));
        if (lds <= 160 * 1024) {
          if (planned(NAD_KERNEL_GEMV_M1, n1 + n2, 16 * 64)) return 0;
          hipError_t e = launch_gemv_dual(a1, a2, n1, n2, 16, lds, st);
          if (e != hipSuccess) {
            set_err("gemv dual launch failed: %s", hipGetErrorString(e));
            return -1;
          }
          return 0;
        }
      }
    }
    for (int i = 0; i < 3;) {
      int n = 1;
      while (i + n < 3 && kin(i, i + n)) n++;
      if (run_skinny(act, act_dtype, lda, m, k, n, ws + i, outs + i, ldos + i, kEpiNone, nullptr, 0, nullptr, 0, nullptr,
                     0, st))
        return -1;
      i += n;
    }
    return 0;
  }
  A16 pre;
  const A16* pp = nullptr;
  if (gemm2_ok(*ws[0], m) && !ws[0]->shuffle && !int8_compute(*ws[0])) {
    if (prepare_a16(pre, act, act_dtype, lda, m, k, *ws[0], st) < 0) return -1;
    pp = &pre;
  }
  {
    const int r = run_gemm7_fused(act, act_dtype, lda, m, k, ws, 3, outs, ldos, st, pp);
    if (r != 0) return r < 0 ? -1 : 0;
  }
  for (int i = 0; i < 3; i++) {
    const DeviceWeight& w = *ws[i];
    // a weight that cannot reuse the shared fp16 copy (other K tile, act-order, int8 arithmetic) writes its own
    // conversion / u8 codes at the start of the same workspace: the copy is gone for the weights after it
    const bool reuses = pp && !int8_compute(w) && pipelined_gemm(w, m) && !w.shuffle && pp->kp == w.nt * k_tile(w);
    const bool clobbers = !reuses && (int8_compute(w) || pipelined_gemm(w, m));
    if (run_gemm(act, act_dtype, lda, m, k, w, outs[i], ldos[i], kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0, st,
                 reuses ? pp : nullptr))
      return -1;
    if (clobbers && pp && pp->p != act) pp = nullptr;
  }
  return 0;
}

// The gate/up half of the fused FFN (ip_fusion_ffn.cpp:407-433): tmp2 = act(X.W1^T) * (X.W3^T), tmp1 = act(X.W1^T)
// (optional at M <= 16, required above).  Decode: one dual-weight stream launch; prefill: two GEMM launches.
extern "C" int nad_device_ffn_gate_up(const void* act, int act_dtype, const void* w1p, const void* w3p, float* tmp1,
                                      float* tmp2, int m, int fin, int fmid, int lda, int epi, void* queue) {
  const DeviceWeight* w1 = as_weight(w1p);
  const DeviceWeight* w3 = as_weight(w3p);
  if (!w1 || !w3) return -1;
  if (epi != kEpiSiluMul && epi != kEpiGeluMul) {
    set_err("ffn epilogue must be SILU_MUL or GELU_MUL");
    return -1;
  }
  if (w1->n != fmid || w3->n != fmid || w1->k != fin || w3->k != fin || !same_kind(*w1, *w3)) {
    set_err("FFN gate/up shapes do not match (fin=%d fmid=%d)", fin, fmid);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  if (w1->mins || w3->mins) {
    // block mins: two passes as run_i8's -- t1 = act(x.w1), tmp2 = t1 * (x.w3) -- each a main launch and the min-term
    // pass, which applies the activation / the multiply.  Without tmp1, t1 lies in the workspace behind the part the
    // passes' own kernels use (nad_device_workspace_size).
    if (int8_compute(*w1) != int8_compute(*w3) ||
        (int8_compute(*w1) && gguf_act_quant(*w1) != gguf_act_quant(*w3))) {
      set_err("gate/up weights of one FFN must resolve to the same arithmetic (nad_device_set_compute) and, in the "
              "int8 mode, to one activation quantizer");
      return -1;
    }
    float* t1 = tmp1;
    if (!t1) {
      const size_t head = align256(nad_device_workspace_size(m, fin));
      char* wsp = static_cast<char*>(workspace_for(head + size_t(m) * fmid * sizeof(float), st));
      if (!wsp) return -1;
      t1 = reinterpret_cast<float*>(wsp + head);
    }
    const int e1 = epi == kEpiSiluMul ? kEpiSilu : kEpiGelu;
    // the partner without mins of a mixed pair applies the epilogue in its own kernel where that kernel can: the
    // activation always, the multiply by t1 in the prefill GEMMs and the int8 kernel (the M <= 16 fp kernels take the
    // multiply only as a fused pair, so there the min-term kernel runs as the epilogue alone)
    const int r1 = w1->mins ? forward_min(act, act_dtype, lda, m, fin, *w1, t1, fmid, e1, nullptr, 0, nullptr, 0, nullptr,
                                          0, st)
                            : forward_one(act, act_dtype, lda, m, fin, *w1, t1, fmid, e1, nullptr, 0, nullptr, 0, st);
    if (r1) return -1;
    if (!w3->mins && m > kSkinnyMaxM)
      return run_gemm(act, act_dtype, lda, m, fin, *w3, tmp2, fmid, kEpiSiluMul, nullptr, 0, nullptr, 0, t1, fmid, st);
    return forward_min(act, act_dtype, lda, m, fin, *w3, tmp2, fmid, kEpiSiluMul, nullptr, 0, nullptr, 0, t1, fmid, st);
  }
  if (m <= kSkinnyMaxM) {
    const DeviceWeight* ws[2] = {w1, w3};
    float* outs[2] = {tmp2, tmp2};
    int ldos[2] = {fmid, fmid};
    return run_skinny(act, act_dtype, lda, m, fin, 2, ws, outs, ldos, epi, nullptr, 0, nullptr, 0, tmp1, fmid, st);
  }
  if (!tmp1) {
    set_err("prefill FFN needs the tmp1 buffer");
    return -1;
  }
  const int e1 = epi == kEpiSiluMul ? kEpiSilu : kEpiGelu;
  A16 pre;
  const A16* pp = nullptr;
  if (gemm2_ok(*w1, m) && !w1->shuffle && !int8_compute(*w1)) {
    if (prepare_a16(pre, act, act_dtype, lda, m, fin, *w1, st) < 0) return -1;
    pp = &pre;
  }
  if (run_gemm(act, act_dtype, lda, m, fin, *w1, tmp1, fmid, e1, nullptr, 0, nullptr, 0, nullptr, 0, st, pp))
    return -1;
  return run_gemm(act, act_dtype, lda, m, fin, *w3, tmp2, fmid, kEpiSiluMul, nullptr, 0, nullptr, 0, tmp1, fmid, st,
                  pp);
}

// f16_tmp: the prefill may keep tmp1 / tmp2 as fp16 scratch (ffn16_ok); the reference-named host entries, whose
// tmp2 the caller reads back as the fp32 intermediate (ip_fusion_ffn.cpp), pass false
static int ffn_forward(const void* act, int act_dtype, const void* w1p, const void* w2p, const void* w3p, float* tmp1,
                       float* tmp2, float* out, int m, int fin, int fmid, int fout, int lda, int epi, void* queue,
                       bool f16_tmp) {
  const DeviceWeight* w1 = as_weight(w1p);
  const DeviceWeight* w2 = as_weight(w2p);
  const DeviceWeight* w3 = as_weight(w3p);
  if (!w1 || !w2 || !w3) return -1;
  if (epi != kEpiSiluMul && epi != kEpiGeluMul) {
    set_err("ffn epilogue must be SILU_MUL or GELU_MUL");
    return -1;
  }
  if (w1->n != fmid || w3->n != fmid || w1->k != fin || w3->k != fin || w2->k != fmid || w2->n != fout ||
      !same_kind(*w1, *w3)) {
    set_err("FFN shapes do not match (fin=%d fmid=%d fout=%d)", fin, fmid, fout);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  const bool any_mins = w1->mins || w2->mins || w3->mins;
  if (!any_mins && f16_tmp && m > kSkinnyMaxM && tmp1 && ffn16_ok(*w1, *w2, *w3, m, fmid)) {
    // prefill with fp16 intermediates: gate -> act(x.w1) as fp16 in tmp1, up -> act(x.w1) * (x.w3) as fp16 in tmp2,
    // which IS down's fp16 A operand (fmid = whole K tiles): no fp32 round trip, no conversion pass before down
    A16 pre;
    if (prepare_a16(pre, act, act_dtype, lda, m, fin, *w1, st) < 0) return -1;
    _Float16* h1 = reinterpret_cast<_Float16*>(tmp1);
    _Float16* h2 = reinterpret_cast<_Float16*>(tmp2);
    const Half16 g{h1, fmid, nullptr}, u{h2, fmid, h1};
    const int e1 = epi == kEpiSiluMul ? kEpiSilu : kEpiGelu;
    if (run_gemm(act, act_dtype, lda, m, fin, *w1, nullptr, fmid, e1, nullptr, 0, nullptr, 0, nullptr, 0, st, &pre,
                 &g) ||
        run_gemm(act, act_dtype, lda, m, fin, *w3, nullptr, fmid, kEpiSiluMul, nullptr, 0, nullptr, 0, nullptr, fmid,
                 st, &pre, &u))
      return -1;
    A16 d;
    d.p = h2;
    d.ld = fmid;
    d.kp = fmid;
    return run_gemm(h2, kActF16, fmid, m, fmid, *w2, out, fout, kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0, st, &d);
  }
  if (nad_device_ffn_gate_up(act, act_dtype, w1p, w3p, tmp1, tmp2, m, fin, fmid, lda, epi, queue)) return -1;
  if (w2->mins)
    return forward_min(tmp2, kActF32, fmid, m, fmid, *w2, out, fout, kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0, st);
  if (m <= kSkinnyMaxM) {
    const DeviceWeight* ws[1] = {w2};
    float* outs[1] = {out};
    int ldos[1] = {fout};
    return run_skinny(tmp2, kActF32, fmid, m, fmid, 1, ws, outs, ldos, kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0,
                      st);
  }
  return run_gemm(tmp2, kActF32, fmid, m, fmid, *w2, out, fout, kEpiNone, nullptr, 0, nullptr, 0, nullptr, 0, st);
}

extern "C" int nad_device_ffn_forward(const void* act, int act_dtype, const void* w1p, const void* w2p,
                                      const void* w3p, float* tmp1, float* tmp2, float* out, int m, int fin, int fmid,
                                      int fout, int lda, int epi, void* queue) {
  return ffn_forward(act, act_dtype, w1p, w2p, w3p, tmp1, tmp2, out, m, fin, fmid, fout, lda, epi, queue, true);
}

// ------------------------------------------------------------------------------------------------ batched problems
struct NadBatch {
  GemvArgs a;
  int bits = 0, waves = 0, grid = 0;
  size_t lds = 0;
  GemvBatchEnt* dev = nullptr;
};

extern "C" void* nad_batch_create(const nad_batch_problem* p, int n) {
  if (!p || n <= 0) {
    set_err("nad_batch_create: need at least one problem");
    return nullptr;
  }
  const DeviceWeight* w0 = as_weight(p[0].weight);
  if (!w0) return nullptr;
  for (int i = 0; i < n; i++) {
    const DeviceWeight* w = as_weight(p[i].weight);
    if (!w) return nullptr;
    if (w->n != w0->n || w->k != w0->k || w->bits != w0->bits || w->blocksize != w0->blocksize ||
        w->asym != w0->asym || w->scale_t != w0->scale_t || w->nt != w0->nt || w->ng != w0->ng ||
        w->kmajor != w0->kmajor || w->f4kind != w0->f4kind) {
      set_err("nad_batch_create: problem %d's weight differs in shape or format from problem 0's", i);
      return nullptr;
    }
    if (w->shuffle || int8_compute(*w)) {
      set_err("nad_batch_create: act-order and int8-compute weights are not batched");
      return nullptr;
    }
    if (w->mins) {  // the batched GEMV has no min-term pass: it would drop S (m + bias d)^T
      set_err("nad_batch_create: problem %d's weight carries block mins (GGUF Q4_1 / Q5_1), which are not batched", i);
      return nullptr;
    }
    if (!p[i].act || !p[i].out || reinterpret_cast<uintptr_t>(p[i].act) % 16 != 0) {
      set_err("nad_batch_create: problem %d needs a 16-B aligned activation vector and an output", i);
      return nullptr;
    }
  }
  auto* b = new NadBatch();
  int gpt = 0;
  float* out0 = p[0].out;
  const int ldo = w0->n;
  if (!prepare_gemv(b->a, b->waves, b->grid, gpt, p[0].act, kActF32, w0->k, 1, w0->k, 1, &w0, &out0, &ldo, kEpiNone,
                    nullptr, 0, nullptr, 0, nullptr, 0) ||
      !gemv_uses_m1(b->a, w0->bits, b->waves)) {
    set_err("nad_batch_create: this weight geometry does not take the M = 1 GEMV");
    delete b;
    return nullptr;
  }
  // workgroups per problem: the chip's CUs dealt out evenly, more where one problem's stripes would not fit one
  // workgroup's partial-sum slots
  const int ns = w0->ns;
  int wpp = std::max(1, std::min(ns, device_cus() / n));
  for (;; wpp++) {
    b->a.u_q = ns / wpp;
    b->a.u_r = ns % wpp;
    b->lds = gemv_lds_layout(b->a, w0->bits, b->waves, wpp);
    if (b->lds <= 160 * 1024 || wpp >= ns) break;
  }
  if (b->lds > 160 * 1024) {
    set_err("nad_batch_create: LDS layout does not fit");
    delete b;
    return nullptr;
  }
  b->a.batch_wpp = wpp;
  b->grid = n * wpp;
  b->bits = w0->bits;
  std::vector<GemvBatchEnt> host(static_cast<size_t>(n));
  for (int i = 0; i < n; i++) {
    const DeviceWeight* w = as_weight(p[i].weight);
    host[i] = GemvBatchEnt{p[i].act, w->tiles, w->scales, w->zps, p[i].out, {nullptr, nullptr, nullptr}};
  }
  if (hipMalloc(&b->dev, sizeof(GemvBatchEnt) * size_t(n)) != hipSuccess ||
      hipMemcpy(b->dev, host.data(), sizeof(GemvBatchEnt) * size_t(n), hipMemcpyHostToDevice) != hipSuccess) {
    set_err("nad_batch_create: device table allocation failed");
    if (b->dev) (void)hipFree(b->dev);
    delete b;
    return nullptr;
  }
  b->a.batch = b->dev;
  return b;
}

extern "C" int nad_batch_run(void* batch, void* queue) {
  NadBatch* b = static_cast<NadBatch*>(batch);
  if (!b) return -1;
  if (planned(NAD_KERNEL_GEMV_M1, b->grid, b->waves * 64)) return 0;
  hipError_t e = launch_gemv_batch(b->a, b->bits, b->waves, b->grid, b->lds, static_cast<hipStream_t>(queue));
  if (e != hipSuccess) {
    set_err("nad_batch_run: launch failed: %s", hipGetErrorString(e));
    return -1;
  }
  return 0;
}

extern "C" void nad_batch_destroy(void* batch) {
  NadBatch* b = static_cast<NadBatch*>(batch);
  if (!b) return;
  if (b->dev) (void)hipFree(b->dev);
  delete b;
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

static __constant__ float kF4LutF[3][16] = {
    {0.00000000f, 5.208333333e-03f, 0.66666667f, 1.00000000f, 0.33333333f, 0.50000000f, 0.16666667f, 0.25000000f,
     -1.f * 0.00000000f, -1.f * 5.208333333e-03f, -1.f * 0.66666667f, -1.f * 1.00000000f, -1.f * 0.33333333f,
     -1.f * 0.50000000f, -1.f * 0.16666667f, -1.f * 0.25000000f},
    {0.f, 0.010416666666666666f, 0.16666666666666666f, 0.25f, 0.333333333333333f, 0.5f, 0.6666666666666f, 1.f,
     -1.f * 0.f, -1.f * 0.010416666666666666f, -1.f * 0.16666666666666666f, -1.f * 0.25f, -1.f * 0.333333333333333f,
     -1.f * 0.5f, -1.f * 0.6666666666666f, -1.f * 1.f},
    {0.f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
     -0.18477343022823334f, -0.09105003625154495f, -1.f, 0.07958029955625534f, 0.16093020141124725f,
     0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f,
     1.0f}};

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
    float sc;
    if (w.scale_t == kScaleF32)
      sc = static_cast<const float*>(w.scales)[si];
    else if (w.scale_t == kScaleBF16)
      sc = __uint_as_float(uint32_t(static_cast<const uint16_t*>(w.scales)[si]) << 16);
    else
      sc = float(static_cast<const _Float16*>(w.scales)[si]);
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
  float* d = nullptr;
  size_t bytes = size_t(w->n) * w->k * 4;
  HIP_OK(hipMalloc(&d, bytes));
  hipLaunchKernelGGL(nad_unrepack_kernel, dim3(2048), dim3(256), 0, st, *w, d);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(host_out, d, bytes, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipFree(d));
  return 0;
}

// ------------------------------------------------------------------------------------------------ host half
// Default device context + per-blob weight cache for the host-pointer ABI (ne_bestla.h:21-83).
namespace {
struct CachedWeight {
  DeviceWeight w;
  void* mem;
  uint64_t size;
  uint64_t key;
  uint64_t bytes;     // device bytes held
  uint64_t last_use;  // LRU tick
};
struct HostCtx {
  std::mutex mu;
  NadDevice* dev = nullptr;
  std::unordered_map<const void*, CachedWeight> cache;
  uint64_t cached_bytes = 0;
  uint64_t limit = 0;       // 0: NAD_HOST_CACHE_MB or the default
  uint64_t tick = 0;
  uint64_t call_start = 0;  // entries used since this tick belong to the running call: never evicted by it
  void* stage = nullptr;
  size_t stage_bytes = 0;
  int threads = 0;
};
HostCtx& hctx() {
  static HostCtx c;
  return c;
}
NadDevice* host_device() {
  HostCtx& c = hctx();
  if (!c.dev) c.dev = static_cast<NadDevice*>(bestla_create_device(false));
  return c.dev;
}
uint64_t cache_limit() {
  HostCtx& c = hctx();
  if (c.limit) return c.limit;
  const uint64_t mb = uint64_t(knobs().host_cache_mb);
  return (mb ? mb : 1) << 20;
}
// one host-ABI call (holds the context lock): the weights it fetches stay cached until it returns
struct HostCall {
  std::lock_guard<std::mutex> lk;
  HostCall() : lk(hctx().mu) { hctx().call_start = hctx().tick + 1; }
};
// O(1) per-call key: FNV-1a over the 64-byte header, the blob size and 64 dwords at fixed positions spread over the
// whole blob (codes and scales).  Rewrites through this library's pack entries are caught exactly (they drop the
// entry, invalidate_host_weight); the samples catch a re-pack of another matrix into the same buffer.
uint64_t blob_key(const Blob& b, const uint8_t* base) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
  };
  mix(base, 64);
  mix(reinterpret_cast<const uint8_t*>(&b.size), sizeof(b.size));
  if (b.size >= 8) {
    const uint64_t span = (b.size - 4) & ~uint64_t(3);
    for (uint64_t i = 0; i < 64; i++) mix(base + (span * i / 63 & ~uint64_t(3)), 4);
  }
  return h;
}
void drop_cached(const void* blob) {
  HostCtx& c = hctx();
  auto it = c.cache.find(blob);
  if (it == c.cache.end()) return;
  if (c.dev) (void)hipStreamSynchronize(c.dev->stream);
  (void)hipFree(it->second.mem);
  c.cached_bytes -= it->second.bytes;
  c.cache.erase(it);
}
// least recently used entries out until the cache fits its cap (not those of the running call)
void evict_to_limit() {
  HostCtx& c = hctx();
  const uint64_t lim = cache_limit();
  while (c.cached_bytes > lim) {
    const void* victim = nullptr;
    uint64_t oldest = UINT64_MAX;
    for (auto& kv : c.cache)
      if (kv.second.last_use < c.call_start && kv.second.last_use < oldest) {
        oldest = kv.second.last_use;
        victim = kv.first;
      }
    if (!victim) break;
    drop_cached(victim);
  }
}
// device copy of a host blob, created on first use and refreshed when the blob's key changes
const DeviceWeight* cached_weight(void* blob) {
  HostCtx& c = hctx();
  Blob b;
  std::string err;
  if (!b.parse(blob, &err)) {
    set_err("%s", err.c_str());
    return nullptr;
  }
  const uint64_t key = blob_key(b, static_cast<const uint8_t*>(blob));
  auto it = c.cache.find(blob);
  if (it != c.cache.end() && it->second.size == b.size && it->second.key == key) {
    it->second.last_use = ++c.tick;
    return &it->second.w;
  }
  drop_cached(blob);
  NadDevice* d = host_device();
  if (!d) return nullptr;
  size_t need = nad_device_weight_size(blob);
  if (!need) return nullptr;
  void* mem = nullptr;
  if (hipMalloc(&mem, need) != hipSuccess) {
    set_err("hipMalloc(%zu) failed for a weight", need);
    return nullptr;
  }
  CachedWeight cw{};
  if (nad_device_load(blob, &cw.w, mem, need, d->stream) != 0) {
    (void)hipFree(mem);
    return nullptr;
  }
  cw.mem = mem;
  cw.size = b.size;
  cw.key = key;
  cw.bytes = need;
  cw.last_use = ++c.tick;
  c.cached_bytes += need;
  auto res = c.cache.emplace(blob, cw);
  evict_to_limit();
  return &res.first->second.w;
}
bool is_device_ptr(const void* p) {
  hipPointerAttribute_t at;
  if (!p) return false;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeDevice;
}
// staging arena for host activations/outputs
void* stage(size_t bytes) {
  HostCtx& c = hctx();
  if (c.stage_bytes < bytes) {
    if (c.stage) (void)hipFree(c.stage);
    c.stage = nullptr;
    c.stage_bytes = 0;
    if (hipMalloc(&c.stage, bytes) != hipSuccess) return nullptr;
    c.stage_bytes = bytes;
  }
  return c.stage;
}

// run `fn(dev_in_ptrs..., dev_out_ptrs...)` with host buffers staged to the device
struct HostBuf {
  const void* host;
  size_t bytes;
  bool out;
  void* dev;
};
int with_staged(std::vector<HostBuf>& bufs, hipStream_t st) {
  size_t total = 0;
  for (auto& b : bufs)
    if (b.host && !is_device_ptr(b.host)) total += align256(b.bytes);
  char* arena = total ? static_cast<char*>(stage(total)) : nullptr;
  if (total && !arena) {
    set_err("staging allocation failed");
    return -1;
  }
  size_t off = 0;
  for (auto& b : bufs) {
    if (!b.host) {
      b.dev = nullptr;
    } else if (is_device_ptr(b.host)) {
      b.dev = const_cast<void*>(b.host);
    } else {
      b.dev = arena + off;
      off += align256(b.bytes);
      if (!b.out) HIP_OK(hipMemcpyAsync(b.dev, b.host, b.bytes, hipMemcpyHostToDevice, st));
    }
  }
  return 0;
}
int finish_staged(std::vector<HostBuf>& bufs, hipStream_t st) {
  for (auto& b : bufs)
    if (b.out && b.host && b.dev != b.host)
      HIP_OK(hipMemcpyAsync(const_cast<void*>(b.host), b.dev, b.bytes, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
}  // namespace

extern "C" void bestla_init(void) { host_device(); }
extern "C" int bestla_set_threads(int nth) {
  hctx().threads = nth;
  if (nth > 0) {
    static char buf[32];
    snprintf(buf, sizeof(buf), "%d", nth);
    setenv("NAD_HOST_THREADS", buf, 1);
  }
  return nth;
}
extern "C" void* bestla_get_thread_handle(void) { return &hctx(); }

extern "C" unsigned long long bestla_f32f32_get_workspace_size(int _m, int _n, int _k, void* wptr) {
  return (unsigned long long)_m * ((size_t(_k) + 127) / 128 * 128) * 4;  // inner_product.cpp:20-25
}
extern "C" unsigned long long bestla_fusion_QKV_f32f32_get_workspace_size(int _m, int _n, int _k, void* w1ptr) {
  return (unsigned long long)_m * ((size_t(_k) + 127) / 128 * 128) * 4;  // ip_fusion_qkv.cpp:159-165
}
extern "C" unsigned long long bestla_fusion_FFN_f32f32_get_workspace_size(int seq, int fin, int fmid, int fout,
                                                                         void* w1ptr, void* w2ptr) {
  return (unsigned long long)seq * ((size_t(fin) + 127) / 128 * 128) * 4 +
         (unsigned long long)seq * ((size_t(fmid) + 127) / 128 * 128) * 4;  // ip_fusion_ffn.cpp:20-27
}

static int host_forward(float* act, void* wblob, float* out, int m, int n, int k, int lda, int ldo, int epi,
                        const float* bias, int bias_ld) {
  HostCall call;
  const DeviceWeight* w = cached_weight(wblob);
  if (!w) return -1;
  NadDevice* d = host_device();
  std::vector<HostBuf> bufs = {{act, size_t(m - 1) * lda * 4 + size_t(k) * 4, false, nullptr},
                               {out, size_t(m - 1) * ldo * 4 + size_t(n) * 4, true, nullptr},
                               {bias, bias ? (bias_ld ? size_t(m - 1) * bias_ld * 4 + size_t(n) * 4 : size_t(n) * 4) : 0,
                                false, nullptr}};
  if (with_staged(bufs, d->stream)) return -1;
  if (nad_device_forward(bufs[0].dev, kActF32, w, static_cast<float*>(bufs[1].dev), m, n, k, lda, ldo, epi,
                         static_cast<const float*>(bufs[2].dev), bias_ld, nullptr, 0, d->stream))
    return -1;
  return finish_staged(bufs, d->stream);
}

extern "C" void bestla_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k, int lda,
                                      int ldo, void* workspace) {
  if (host_forward(activation, weiptr, output, _m, _n, _k, lda, ldo, kEpiNone, nullptr, 0))
    report("bestla_f32f32_forward");
}

extern "C" bool bestla_fusion_add_f32f32_support(void* weiptr, int _m, int _n, int _k) {
  Blob b;
  std::string err;
  return b.parse(weiptr, &err) && blob_supported(b, &err) && b.n == _n && b.k == _k;
}
extern "C" void bestla_fusion_add_f32f32_forward(float* activation, void* weiptr, float* bias, float* output, int _m,
                                                 int _n, int _k, int lda, int ldo, bool boardcast_bias,
                                                 void* workspace) {
  // inner_product.cpp:132-244: + bias[n] (broadcast) or + bias[m][n] with row stride ldo
  if (host_forward(activation, weiptr, output, _m, _n, _k, lda, ldo, kEpiBias, bias, boardcast_bias ? 0 : ldo))
    report("bestla_fusion_add_f32f32_forward");
}

static bool same_blob_kind(void* const* ws, int nw) {
  Blob b0;
  std::string err;
  if (!b0.parse(ws[0], &err) || !blob_supported(b0, &err)) return false;
  for (int i = 1; i < nw; i++) {
    Blob b;
    if (!b.parse(ws[i], &err)) return false;
    if (b.core_id != b0.core_id || b.qtype != b0.qtype || b.blocksize != b0.blocksize || b.scale_t != b0.scale_t ||
        b.asym != b0.asym || b.k != b0.k)
      return false;
  }
  return true;
}

extern "C" bool bestla_fusion_QKV_f32f32_support(void* wqptr, void* wkptr, void* wvptr, int _m, int _n, int _k) {
  void* ws[3] = {wqptr, wkptr, wvptr};
  if (!same_blob_kind(ws, 3)) return false;
  Blob b;
  std::string err;
  b.parse(wqptr, &err);
  return !b.has_shuffle && b.k == _k;  // ip_fusion_qkv.cpp:175-180: no act-order shuffle
}

extern "C" void bestla_fusion_QKV_f32f32_forward(float* activation, void* wqptr, void* wkptr, void* wvptr,
                                                 float* output, int _m, int _n, int _k, int lda, int ldo,
                                                 void* workspace) {
  // ip_fusion_qkv.cpp:22-40: Q, K, V written to output, output + M*ldo, output + 2*M*ldo
  HostCall call;
  const DeviceWeight* w[3] = {cached_weight(wqptr), cached_weight(wkptr), cached_weight(wvptr)};
  if (!w[0] || !w[1] || !w[2]) {
    report("bestla_fusion_QKV_f32f32_forward");
    return;
  }
  NadDevice* d = host_device();
  const size_t obytes = size_t(3) * _m * ldo * 4;
  std::vector<HostBuf> bufs = {{activation, size_t(_m - 1) * lda * 4 + size_t(_k) * 4, false, nullptr},
                               {output, obytes, true, nullptr}};
  if (with_staged(bufs, d->stream)) {
    report("bestla_fusion_QKV_f32f32_forward");
    return;
  }
  float* o = static_cast<float*>(bufs[1].dev);
  if (nad_device_qkv_forward(bufs[0].dev, kActF32, w[0], w[1], w[2], o, o + size_t(_m) * ldo,
                             o + size_t(2) * _m * ldo, _m, _k, lda, ldo, ldo, ldo, d->stream) ||
      finish_staged(bufs, d->stream))
    report("bestla_fusion_QKV_f32f32_forward");
}

static bool ffn_support3(void* w1, void* w2, void* w3, int fin, int fmid, int fout) {
  void* ws[2] = {w1, w3};
  if (!same_blob_kind(ws, 2)) return false;
  Blob b1, b2;
  std::string err;
  if (!b1.parse(w1, &err) || !b2.parse(w2, &err) || !blob_supported(b2, &err)) return false;
  return !b1.has_shuffle && !b2.has_shuffle && b1.k == fin && b1.n == fmid && b2.k == fmid && b2.n == fout &&
         b2.qtype == b1.qtype;
}

extern "C" bool bestla_fusion_FFN_SiLu_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin,
                                                      int fmid, int fout) {
  return ffn_support3(w1ptr, w2ptr, w3ptr, fin, fmid, fout);
}
extern "C" bool bestla_fusion_FFN_Gelu_Mul_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin,
                                                          int fmid, int fout) {
  return ffn_support3(w1ptr, w2ptr, w3ptr, fin, fmid, fout);
}

static void host_ffn3(float* act, void* w1p, void* w2p, void* w3p, float* tmp1, float* tmp2, float* out, int seq,
                      int fin, int fmid, int fout, int epi, const char* name) {
  HostCall call;
  const DeviceWeight* w1 = cached_weight(w1p);
  const DeviceWeight* w2 = cached_weight(w2p);
  const DeviceWeight* w3 = cached_weight(w3p);
  if (!w1 || !w2 || !w3) {
    report(name);
    return;
  }
  NadDevice* d = host_device();
  std::vector<HostBuf> bufs = {{act, size_t(seq) * fin * 4, false, nullptr},
                               {tmp1, size_t(seq) * fmid * 4, true, nullptr},
                               {tmp2, size_t(seq) * fmid * 4, true, nullptr},
                               {out, size_t(seq) * fout * 4, true, nullptr}};
  if (with_staged(bufs, d->stream) ||
      ffn_forward(bufs[0].dev, kActF32, w1, w2, w3, static_cast<float*>(bufs[1].dev), static_cast<float*>(bufs[2].dev),
                  static_cast<float*>(bufs[3].dev), seq, fin, fmid, fout, fin, epi, d->stream, false) ||
      finish_staged(bufs, d->stream))
    report(name);
}

extern "C" void bestla_fusion_FFN_SiLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr,
                                                      float* tmp1, float* tmp2, float* output, int seq, int fin,
                                                      int fmid, int fout, void* workspace) {
  host_ffn3(activation, w1ptr, w2ptr, w3ptr, tmp1, tmp2, output, seq, fin, fmid, fout, kEpiSiluMul,
            "bestla_fusion_FFN_SiLu_f32f32_forward");
}
extern "C" void bestla_fusion_FFN_Gelu_Mul_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr,
                                                          float* tmp1, float* tmp2, float* output, int seq, int fin,
                                                          int fmid, int fout, void* workspace) {
  host_ffn3(activation, w1ptr, w2ptr, w3ptr, tmp1, tmp2, output, seq, fin, fmid, fout, kEpiGeluMul,
            "bestla_fusion_FFN_Gelu_Mul_f32f32_forward");
}

static bool ffn_support2(void* w1, void* w2, int fin, int fmid, int fout) {
  void* ws[2] = {w1, w2};
  Blob b1, b2;
  std::string err;
  if (!b1.parse(w1, &err) || !b2.parse(w2, &err) || !blob_supported(b1, &err) || !blob_supported(b2, &err))
    return false;
  (void)ws;
  return b1.k == fin && b1.n == fmid && b2.k == fmid && b2.n == fout;
}
extern "C" bool bestla_fusion_FFN_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid, int fout) {
  return ffn_support2(w1ptr, w2ptr, fin, fmid, fout);
}
extern "C" bool bestla_fusion_FFN_Add_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid,
                                                          int fout) {
  return ffn_support2(w1ptr, w2ptr, fin, fmid, fout);
}

static void host_ffn2(float* act, void* w1p, void* w2p, const float* b1, const float* b2, float* tmp1, float* out,
                      int seq, int fin, int fmid, int fout, bool add, bool bcast, const char* name) {
  HostCall call;
  const DeviceWeight* w1 = cached_weight(w1p);
  const DeviceWeight* w2 = cached_weight(w2p);
  if (!w1 || !w2) {
    report(name);
    return;
  }
  NadDevice* d = host_device();
  const size_t b1b = b1 ? (bcast ? size_t(fmid) : size_t(seq) * fmid) * 4 : 0;
  const size_t b2b = b2 ? (bcast ? size_t(fout) : size_t(seq) * fout) * 4 : 0;
  std::vector<HostBuf> bufs = {{act, size_t(seq) * fin * 4, false, nullptr},
                               {tmp1, size_t(seq) * fmid * 4, true, nullptr},
                               {out, size_t(seq) * fout * 4, true, nullptr},
                               {b1, b1b, false, nullptr},
                               {b2, b2b, false, nullptr}};
  int rc = with_staged(bufs, d->stream);
  float* t1 = static_cast<float*>(bufs[1].dev);
  if (!rc)
    rc = nad_device_forward(bufs[0].dev, kActF32, w1, t1, seq, fmid, fin, fin, fmid, add ? kEpiAddGelu : kEpiGelu,
                            static_cast<const float*>(bufs[3].dev), bcast ? 0 : fmid, nullptr, 0, d->stream);
  if (!rc)
    rc = nad_device_forward(t1, kActF32, w2, static_cast<float*>(bufs[2].dev), seq, fout, fmid, fmid, fout,
                            add ? kEpiBias : kEpiNone, static_cast<const float*>(bufs[4].dev), bcast ? 0 : fout,
                            nullptr, 0, d->stream);
  if (!rc) rc = finish_staged(bufs, d->stream);
  if (rc) report(name);
}

extern "C" void bestla_fusion_FFN_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* tmp1,
                                                      float* output, int seq, int fin, int fmid, int fout,
                                                      void* workspace) {
  host_ffn2(activation, w1ptr, w2ptr, nullptr, nullptr, tmp1, output, seq, fin, fmid, fout, false, true,
            "bestla_fusion_FFN_GeLu_f32f32_forward");
}
extern "C" void bestla_fusion_FFN_Add_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* b1ptr,
                                                          float* b2ptr, float* tmp1, float* output, int seq, int fin,
                                                          int fmid, int fout, bool boardcast_bias, void* workspace) {
  host_ffn2(activation, w1ptr, w2ptr, b1ptr, b2ptr, tmp1, output, seq, fin, fmid, fout, true, boardcast_bias,
            "bestla_fusion_FFN_Add_GeLu_f32f32_forward");
}

// a pack entry is about to (re)write `blob`: forget its device copy
static void invalidate_host_weight(const void* blob) {
  std::lock_guard<std::mutex> lk(hctx().mu);
  drop_cached(blob);
}

// release every cached device weight of the host-pointer ABI (e.g. before freeing host blobs)
extern "C" void nad_host_cache_clear(void) {
  HostCtx& c = hctx();
  std::lock_guard<std::mutex> lk(c.mu);
  if (c.dev) (void)hipStreamSynchronize(c.dev->stream);
  for (auto& kv : c.cache) (void)hipFree(kv.second.mem);
  c.cache.clear();
  c.cached_bytes = 0;
}

extern "C" void nad_host_cache_evict(const void* blob) { invalidate_host_weight(blob); }

extern "C" size_t nad_host_cache_set_limit(size_t bytes) {
  HostCtx& c = hctx();
  std::lock_guard<std::mutex> lk(c.mu);
  const size_t prev = cache_limit();
  c.limit = bytes;
  c.call_start = c.tick + 1;
  evict_to_limit();
  return prev;
}

extern "C" int nad_host_cache_stats(size_t* entries, size_t* bytes) {
  HostCtx& c = hctx();
  std::lock_guard<std::mutex> lk(c.mu);
  if (entries) *entries = c.cache.size();
  if (bytes) *bytes = c.cached_bytes;
  return 0;
}

extern "C" unsigned long long nad_host_blob_key(const void* blob) {
  Blob b;
  std::string err;
  if (!blob || !b.parse(blob, &err)) {
    set_err("%s", err.c_str());
    return 0;
  }
  return blob_key(b, static_cast<const uint8_t*>(blob));
}

// ------------------------------------------------------------------------------------------------ pack API
// scale dtype against weight dtype: F8_E8M0 with F8 weights (bestla_prologue_b.h:1198-1208); DQ8_BNB sym with integer
// or NF4 weights and a group of a multiple of 8 (initDoubleQuantBlkSize asserts, bestla_storage.h:755-759)
static bool pack_scale_ok(uint32_t qt, uint32_t st, bool asym, size_t bs, size_t K) {
  if (st == kF8E8M0 && !is_f8(qt)) {
    set_err("F8_E8M0 scales go with F8 weights only");
    return false;
  }
  if (st == kDQ8_BNB) {
    const size_t g = bs >= K || bs == 0 ? K : bs;
    if (asym || (!dtype_is_int(qt) && qt != kF4NF4) || g % 8) {
      set_err("DQ8_BNB scales need symmetric integer or F4_NF4 weights and a group size that is a multiple of 8");
      return false;
    }
    return true;
  }
  if (st != kF32 && st != kBF16 && st != kF16 && st != kF8E8M0) {
    set_err("scale dtype must be F32, BF16, F16, F8_E8M0 or DQ8_BNB");
    return false;
  }
  return true;
}
extern "C" size_t BTLAGemmPackBSize(size_t N, size_t K, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype,
                                    bool isAsym, int CompType, int* shuffle_indice) {
  if (!dtype_is_int(QuantType) && f4_kind(QuantType) < 0 && !is_f8(QuantType)) {
    set_err("weight dtype must be an integer, F4_BNB / F4_E2M1 / F4_NF4 or F8_E4M3 / F8_E5M2");
    return 0;
  }
  if (!pack_scale_ok(QuantType, ScaleDtype, isAsym, BlkSize, K)) return 0;
  uint64_t core = select_core(CompType, QuantType, int(BlkSize), isAsym, host_isa_profile());
  if (!core) return 0;
  return Blob::describe(int(N), int(K), int(BlkSize), QuantType, ScaleDtype, isAsym, core, shuffle_indice != nullptr)
      .size;
}

extern "C" bool BTLAGemmQuantPackB(void* PackedBuf, const float* FpData, size_t N, size_t K, size_t ldb,
                                   size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType,
                                   bool isTrans, void* ThreadPool) {
  if ((!dtype_is_int(QuantType) && f4_kind(QuantType) < 0 && !is_f8(QuantType)) || !PackedBuf || !FpData) return false;
  if (!pack_scale_ok(QuantType, ScaleDtype, isAsym, BlkSize, K)) return false;
  uint64_t core = select_core(CompType, QuantType, int(BlkSize), isAsym, host_isa_profile());
  if (!core) return false;
  Blob b = Blob::describe(int(N), int(K), int(BlkSize), QuantType, ScaleDtype, isAsym, core, false);
  invalidate_host_weight(PackedBuf);
  b.write_header(static_cast<int8_t*>(PackedBuf));
  // quantizeWeight works on [K][N]; packTransposeWeight first transposes a torch-layout [N][ldb] matrix
  std::vector<float> kn;
  const float* src = FpData;
  int ld = int(ldb);
  if (isTrans) {
    kn.resize(K * N);
    for (size_t kk = 0; kk < K; kk++)
      for (size_t nn = 0; nn < N; nn++) kn[kk * N + nn] = FpData[nn * ldb + kk];
    src = kn.data();
    ld = int(N);
  }
  const int nblk = b.ngroups_k();
  std::vector<int8_t> q(K * N), z(isAsym ? size_t(nblk) * N : 0);
  std::vector<float> s(size_t(nblk) * N);
  quantize_kblock(src, int(K), int(N), ld, b.blocksize, uint32_t(QuantType), q.data(), s.data(),
                  b.asym ? z.data() : nullptr, ScaleDtype == kF8E8M0);
  std::string err;
  if (!pack_quantized(b, static_cast<int8_t*>(PackedBuf), q.data(), int(N), s.data(), isAsym ? z.data() : nullptr,
                      nullptr, &err)) {
    set_err("%s", err.c_str());
    return false;
  }
  return true;
}

extern "C" bool BTLAGemmPackB(void* PackedBuf, const int8_t* QData, const float* Scales, const int8_t* Zp, size_t N,
                              size_t K, size_t ldb, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype,
                              bool isAsym, int CompType, int* shuffle_indice, void* ThreadPool) {
  if (!dtype_is_int(QuantType) || !PackedBuf || !QData || !Scales) return false;
  if (!pack_scale_ok(QuantType, ScaleDtype, isAsym, BlkSize, K)) return false;
  uint64_t core = select_core(CompType, QuantType, int(BlkSize), isAsym, host_isa_profile());
  if (!core) return false;
  Blob b = Blob::describe(int(N), int(K), int(BlkSize), QuantType, ScaleDtype, isAsym, core,
                          shuffle_indice != nullptr);
  invalidate_host_weight(PackedBuf);
  b.write_header(static_cast<int8_t*>(PackedBuf));
  std::string err;
  if (!pack_quantized(b, static_cast<int8_t*>(PackedBuf), QData, int(ldb), Scales, isAsym ? Zp : nullptr,
                      shuffle_indice, &err)) {
    set_err("%s", err.c_str());
    return false;
  }
  return true;
}

extern "C" bool BTLAGemmUnPackB(float* FpData, const void* PackedBuf, size_t N, size_t K, size_t ldb,
                                void* ThreadPool) {
  Blob b;
  std::string err;
  if (!b.parse(PackedBuf, &err)) {
    set_err("%s", err.c_str());
    return false;
  }
  if (size_t(b.n) != N || size_t(b.k) != K) {
    set_err("unpack shape mismatch");
    return false;
  }
  unpack_fp32(b, static_cast<const int8_t*>(PackedBuf), FpData, int(ldb));
  return true;
}

extern "C" bool BTLAGemmBatchDriver(const size_t M, const size_t N, const size_t K, const size_t BatchN,
                                    const BTLA_GEMM_DATA_PACKED_PARAMS* DataParams, int8_t* WorkSpace,
                                    void* ThreadPool) {
  for (size_t i = 0; i < BatchN; i++) {
    const auto& p = DataParams[i];
    // the reference ignores lda/ldc (bestla_gemm.cpp:44,71-73); honour them when set, default to contiguous
    int lda = p.lda > 0 ? p.lda : int(K), ldc = p.ldc > 0 ? p.ldc : int(N);
    if (host_forward(const_cast<float*>(p.A), const_cast<void*>(p.B), p.C, int(M), int(N), int(K), lda, ldc, kEpiNone,
                     nullptr, 0))
      return false;
  }
  return true;
}

extern "C" void bestla_unpackweight_fp32(void* wptr, int n, int k, float* fp32data, int ld) {
  if (!BTLAGemmUnPackB(fp32data, wptr, size_t(n), size_t(k), size_t(ld), nullptr)) report("bestla_unpackweight_fp32");
}

extern "C" void bestla_packweight_copyattr(const float* f32ptr, void* dstpr, int n, int k, int ld, void* srcptr) {
  // ne_bestla.cpp:79-111: quantize f32 [N][ld] with the source blob's attributes (core, bits, group, scale, asym)
  Blob s;
  std::string err;
  if (!s.parse(srcptr, &err)) {
    set_err("%s", err.c_str());
    report("bestla_packweight_copyattr");
    return;
  }
  Blob b = Blob::describe(n, k, s.blocksize >= s.kpad ? -1 : s.blocksize, s.qtype, s.scale_t, s.asym, s.core_id, false);
  invalidate_host_weight(dstpr);
  b.write_header(static_cast<int8_t*>(dstpr));
  std::vector<float> kn(size_t(k) * n);
  for (int kk = 0; kk < k; kk++)
    for (int nn = 0; nn < n; nn++) kn[size_t(kk) * n + nn] = f32ptr[size_t(nn) * ld + kk];
  const int nblk = b.ngroups_k();
  std::vector<int8_t> q(size_t(k) * n), z(s.asym ? size_t(nblk) * n : 0);
  std::vector<float> sc(size_t(nblk) * n);
  quantize_kblock(kn.data(), k, n, n, b.blocksize, b.qtype, q.data(), sc.data(),
                  s.asym ? z.data() : nullptr);
  if (!pack_quantized(b, static_cast<int8_t*>(dstpr), q.data(), n, sc.data(), s.asym ? z.data() : nullptr, nullptr,
                      &err)) {
    set_err("%s", err.c_str());
    report("bestla_packweight_copyattr");
  }
}

// ------------------------------------------------------------------------------------------------ TP split
extern "C" int nad_split_range(const void* src, int axis, int rank, int world, int unit, int* begin, int* end) {
  Blob b;
  std::string err;
  if (!b.parse(src, &err)) {
    set_err("%s", err.c_str());
    return -1;
  }
  if (world <= 0 || rank < 0 || rank >= world) {
    set_err("bad rank/world");
    return -1;
  }
  if (axis == 0) {  // N: near-equal chunks of `unit` columns (the reference requires N % world == 0,
                    // model_files.h:193-235, which unit = 1 reproduces)
    const int u = std::max(1, unit);
    const int units = (b.n + u - 1) / u;
    const int base = units / world, rem = units % world;
    const int u0 = rank * base + std::min(rank, rem), u1 = u0 + base + (rank < rem ? 1 : 0);
    *begin = std::min(b.n, u0 * u);
    *end = std::min(b.n, u1 * u);
  } else {  // K: whole quantization groups, near-equal (e.g. Llama down K=11008 = 86 g128 -> 11x6, 10x2)
    const int bs = b.blocksize >= b.k ? b.k : b.blocksize;
    const int groups = (b.k + bs - 1) / bs;
    if (b.blocksize >= b.k) {
      set_err("per-channel quantization cannot be split along K without re-quantization");
      return -1;
    }
    const int base = groups / world, rem = groups % world;
    const int g0 = rank * base + std::min(rank, rem), g1 = g0 + base + (rank < rem ? 1 : 0);
    *begin = std::min(b.k, g0 * bs);
    *end = std::min(b.k, g1 * bs);
  }
  return 0;
}

extern "C" size_t nad_blob_split(const void* src, int axis, int rank, int world, int unit, void* dst,
                                  size_t dst_capacity) {
  Blob b;
  std::string err;
  if (!b.parse(src, &err)) {
    set_err("%s", err.c_str());
    return 0;
  }
  if (b.has_shuffle && axis == 1) {
    set_err("act-order (g_idx) weights cannot be split along K");
    return 0;
  }
  if (b.has_dq) {  // a slice would double-quantize its scales again around a new mean: not the same numbers
    set_err("DQ8_BNB double-quantized weights cannot be split exactly");
    return 0;
  }
  int lo, hi;
  if (nad_split_range(src, axis, rank, world, unit, &lo, &hi)) return 0;
  const int n2 = axis == 0 ? hi - lo : b.n;
  const int k2 = axis == 1 ? hi - lo : b.k;
  const int bs = b.blocksize >= b.kpad ? -1 : b.blocksize;
  Blob o = Blob::describe(n2, k2, bs, b.qtype, b.scale_t, b.asym, b.core_id, b.has_shuffle);
  if (!dst) return o.size;
  if (dst_capacity < o.size) {
    set_err("destination too small");
    return 0;
  }
  // exact: unpack the integers and stored scales, slice, pack again with identical attributes
  std::vector<int8_t> Q(size_t(b.k) * b.n), Z(size_t(b.ngroups_k()) * b.n);
  std::vector<float> S(size_t(b.ngroups_k()) * b.n);
  std::vector<int> shf(b.has_shuffle ? b.k : 0);
  unpack_quantized(b, static_cast<const int8_t*>(src), Q.data(), S.data(), Z.data(),
                   b.has_shuffle ? shf.data() : nullptr);
  const int gb = b.blocksize >= b.k ? b.k : b.blocksize;
  const int g0 = axis == 1 ? lo / gb : 0;
  const int ng2 = (k2 + gb - 1) / gb;
  std::vector<int8_t> Q2(size_t(k2) * n2), Z2(size_t(ng2) * n2);
  std::vector<float> S2(size_t(ng2) * n2);
  const int n0 = axis == 0 ? lo : 0, k0 = axis == 1 ? lo : 0;
  for (int kk = 0; kk < k2; kk++)
    std::memcpy(&Q2[size_t(kk) * n2], &Q[size_t(k0 + kk) * b.n + n0], size_t(n2));
  for (int g = 0; g < ng2; g++)
    for (int nn = 0; nn < n2; nn++) {
      S2[size_t(g) * n2 + nn] = S[size_t(g0 + g) * b.n + n0 + nn];
      Z2[size_t(g) * n2 + nn] = Z[size_t(g0 + g) * b.n + n0 + nn];
    }
  // g_idx for the shard (N split keeps K, so the LUT is unchanged): rebuild group ids from the LUT
  std::vector<int> gidx;
  if (b.has_shuffle) {
    gidx.resize(b.k);
    for (int p = 0; p < b.k; p++) gidx[shf[p]] = p / b.blocksize;
  }
  invalidate_host_weight(dst);
  o.write_header(static_cast<int8_t*>(dst));
  if (!pack_quantized(o, static_cast<int8_t*>(dst), Q2.data(), n2, S2.data(), b.asym ? Z2.data() : nullptr,
                      b.has_shuffle ? gidx.data() : nullptr, &err)) {
    set_err("%s", err.c_str());
    return 0;
  }
  return o.size;
}
