// capi_internal.h -- what the units behind the extern "C" boundary share: capi.hip (errors, knobs, dry runs, device
// context, workspace, compute mode), capi_load.hip, capi_forward.hip, capi_host.hip, capi_moe.hip.  Nothing here is
// exported.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/neural_amd.h"
#include "btla_format.h"
#include "staging.h"
#include "woq_kernels.h"

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------------------------ errors (capi.hip)
void set_err(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void report(const char* where);
#define HIP_OK(expr)                                                           \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) {                                                    \
      set_err("%s failed: %s", #expr, hipGetErrorString(e_));                  \
      return -1;                                                               \
    }                                                                          \
  } while (0)

// ------------------------------------------------------------------------------------------------ knobs (capi.hip)
// Tuning / A-B switches.  Read from the environment ONCE (at the first forward, or by nad_reload_knobs), never per
// launch: the eager path an NE graph takes (one bestla_device_f32f32_forward per node) must not scan the environment.
struct Knobs {
  int gemv_grid, gemv_waves, gemv_lean, gemv_spw, gemv_disable, gemv_dual, gemv_nst, gemv_m1_spec, gemv_ahead;
  int compute_int8;
  int gemm2_disable, gemm4_all, gemm4_disable, ffn_f32, gemm_kernel, gemm7_bm, splitk_disable;
  int gemm3_stagger, gemm4_fold_all, gemm4_fold, gemm4_ksw;
  int mid_min_m, mid_max_m, mid_ks, mid_xcd, mid_wide, gemm_xcd, gemm7_model, gemm7_fuse;
  int host_cache_mb;
};
const Knobs& knobs();

// ------------------------------------------------------------------------------------------------ dry runs (capi.hip)
// nad_plan_forward runs the whole host side of a forward (validation, kernel choice, geometry, workspace sizing) with
// every launch replaced by a record of it: which kernel would serve the call, and what the host path costs per call.
struct NadPlan {
  int kernel = 0, grid = 0, block = 0, ksplit = 1, fold = 0, launches = 0;  // the last main launch; every launch counted
  // the first kListMax launches in call order, pre-passes included: kernel code, grid, threads per workgroup, dynamic
  // LDS bytes (the routed-expert dry runs write the list out; their longest call has 6 launches)
  static constexpr int kListMax = 8;
  int64_t list[kListMax][4] = {};
  int listed() const { return launches < kListMax ? launches : kListMax; }
};
void set_plan(NadPlan* p);  // the calling thread's forwards record into *p until set_plan(nullptr)
bool planning();
// true (and the launch recorded) in a dry run; main = false for pre-passes (conversions, activation quantizers)
bool planned(int kernel, int grid, int block, int ksplit = 1, int fold = 0, bool main = true, size_t lds = 0);
inline bool planned_pass() { return planned(0, 0, 0, 1, 0, false); }
// ... of a launcher's own shape (woq_kernels.h) and its dynamic LDS
inline bool planned(int kernel, nad::LaunchShape s, size_t lds = 0) {
  return planned(kernel, s.grid, s.block, 1, 0, true, lds);
}

// One launch: recorded in a dry run (`recorded`, the result of planned()), else issued by fn; false, with the error
// "<what> launch failed: ..." set, when it fails.
template <class F>
static inline bool launch(bool recorded, const char* what, F&& fn) {
  if (recorded) return true;
  const hipError_t e = fn();
  if (e == hipSuccess) return true;
  set_err("%s launch failed: %s", what, hipGetErrorString(e));
  return false;
}

// The launch of a decode GEMV (launch_gemv, launch_gemv_batch).  In a dry run fn runs too, and the launch statement it
// reaches names its kernel instead of launching (woq_kernels.h: gemv_name_begin); the name joins the record's flag word.
void plan_gemv_instance(uint32_t inst);
template <class F>
static inline bool launch_gemv_named(bool recorded, const char* what, F&& fn) {
  if (recorded) nad::gemv_name_begin();
  const bool ok = launch(false, what, fn);
  if (recorded) plan_gemv_instance(nad::gemv_name_end());
  return ok;
}

// ------------------------------------------------------------------------------------------------ device context
struct NadDevice {
  int device;
  hipStream_t stream;
  bool profile;
};

const nad::DeviceWeight* as_weight(const void* p);  // null, with the error set, for anything but a loaded weight

// ------------------------------------------------------------------------------------------------ workspace (capi.hip)
void* workspace_for(size_t bytes, hipStream_t st);
struct CallWorkspace {  // RAII binding of a reference call's workspace argument
  CallWorkspace(void* p, size_t b);
  ~CallWorkspace();
};

// ------------------------------------------------------------------------------------------------ compute mode (capi.hip)
// a GGUF matrix carries its type's tag in src_core_id (woq_gguf.h: kGgufTypes).  The 32-element types run the
// reference's Q8_0 / Q8_1 arithmetic in int8 mode; Q6_K (bits = 6, a layout and forward kernels of its own, woq_q6k.hip)
// runs fp arithmetic, or the reference's Q8_K integer arithmetic as the weight's own mode 2
inline bool is_q6k(const nad::DeviceWeight& w) { return w.bits == 6; }
// the activation quantizer of the weight's int8 arithmetic (its vec_dot_type, ne_layers.c:266-318): 0 the kblock
// core's u8, 1 Q8_0 (Q4_0, Q5_0, Q8_0), 2 Q8_1 (Q4_1, Q5_1)
int gguf_act_quant(const nad::DeviceWeight& w);
bool int8_compute(const nad::DeviceWeight& w);  // a forward of this weight takes the int8 arithmetic right now
bool q8k_compute(const nad::DeviceWeight& w);   // a Q6_K weight set to NAD_COMPUTE_Q8_K: forward_q6k takes woq_q6k_i8_kernel

// ------------------------------------------------------------------------------------------------ staging (capi.hip)
struct HipStagingApi {
  using Error = hipError_t;
  using Stream = hipStream_t;
  static constexpr Error kOk = hipSuccess;
  static Error malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static Error sync(Stream st) { return hipStreamSynchronize(st); }
  static Error free(void* p) { return hipFree(p); }
};
using Staging = nad::StagingBuffer<HipStagingApi>;
// s.finish(); 0, or -1 with "<who>: <first failing step> failed: <HIP error>" set
int staging_finish(const char* who, Staging& s);

// ------------------------------------------------------------------------------------------------ load (capi_load.hip)
// base: the host blob, scanned for codes the device cannot hold (load time only; null skips the scan)
bool blob_supported(const nad::Blob& b, const void* base, std::string* err);
inline bool blob_supported(const nad::Blob& b, std::string* err) { return blob_supported(b, nullptr, err); }
// for capi_quant.hip, which fills a descriptor the way nad_device_load does: the ScaleType of a blob scale dtype, the
// fold_ok rule over the scales at base + b.s_off, and the repack of the blob's sections once they are on the device
// (dz null: symmetric)
int scale_code(uint32_t scale_dtype);
bool blob_fold_ok(const nad::Blob& b, const uint8_t* base, int dev_bits);
int repack_sections(const nad::Blob& b, const nad::DeviceWeight& w, const uint8_t* dq, const void* ds, const int8_t* dz,
                    hipStream_t st);

// ------------------------------------------------------------------------------------------------ forward calls
// One forward as three values (capi_forward.hip): the activations, what happens to the product, where it goes.
struct Act {
  const void* p;
  int t;  // ActType
  int ld, m, k;
};

struct Epi {  // the default value: no epilogue
  int kind = nad::kEpiNone;
  const float* bias = nullptr;  // bias[m * bias_ld + n] (bias_ld = 0 broadcasts one row)
  int bias_ld = 0;
  const float* res = nullptr;
  int ld_res = 0;
  float* aux = nullptr;  // dual kinds: optional output of the gate activation; SILU_MUL of one weight: the multiplier
  int ld_aux = 0;

  bool is_dual() const { return kind == nad::kEpiSiluMul || kind == nad::kEpiGeluMul; }
  // the gate activation alone of a dual kind (the first pass of a two-pass gate/up)
  static Epi gate_of(int dual_kind) {
    Epi e;
    e.kind = dual_kind == nad::kEpiSiluMul ? nad::kEpiSilu : nad::kEpiGelu;
    return e;
  }
  // the product times aux (the second pass; the activation is in aux already)
  static Epi mul(float* aux, int ld_aux) {
    Epi e;
    e.kind = nad::kEpiSiluMul;
    e.aux = aux;
    e.ld_aux = ld_aux;
    return e;
  }
};

// fp16 result / SiLU*mul operand of a pipelined GEMM (the FFN's intermediates, ffn16_ok)
struct Half16 {
  _Float16* out = nullptr;
  int ldo = 0;
  const _Float16* aux = nullptr;
};

struct Out {
  float* p;
  int ld;
  const Half16* h16 = nullptr;  // set: the result goes there as fp16 instead (p is not written)
};

// f16_tmp: the prefill may keep tmp1 / tmp2 as fp16 scratch (ffn16_ok); the reference-named host entries, whose
// tmp2 the caller reads back as the fp32 intermediate (ip_fusion_ffn.cpp), pass false
int ffn_forward(const void* act, int act_dtype, const void* w1p, const void* w2p, const void* w3p, float* tmp1,
                float* tmp2, float* out, int m, int fin, int fmid, int fout, int lda, int epi, void* queue,
                bool f16_tmp);

// capi_forward.hip, for capi_moe.hip: the chip's compute units (256 without a device), and the GemvArgs / waves of one
// M = 1 fp32 problem on ws[0] or on the {gate, up} pair with a dual epilogue, exactly as that problem's own decode
// launch prepares them; false where the M = 1 GEMV does not take the geometry
int device_cus();
bool prepare_m1_problem(nad::GemvArgs& a, int& waves, const nad::DeviceWeight* const* ws, int nw, int epi);
// ... the same problem where the stripe-stream GEMV (woq_gemv_kernel, hi / lo fp16 rows) serves it and the M = 1 stream
// does not: false where prepare_gemv refuses the geometry or the M = 1 stream takes it
bool prepare_general_problem(nad::GemvArgs& a, int& waves, const nad::DeviceWeight* const* ws, int nw, int epi);
// ... and the tile height a gemm7 launch of m rows on w takes (NAD_GEMM7_BM, else the cost model), and w's K tile
int gemm7_tile_height(const nad::DeviceWeight& w, int m);
int gemm7_k_tile(const nad::DeviceWeight& w);

#pragma GCC visibility pop

extern "C" size_t nad_device_workspace_size(int m, int k);  // ne_ops.hip (include/neural_amd_ne.h)
