// capi_internal.h -- what the units behind the extern "C" boundary share: capi.hip (errors, knobs, the dry-run
// recorder, device context, workspace, compute mode), capi_load.hip, capi_forward.hip, capi_plan.hip (the dense dry
// runs), capi_host.hip, capi_moe.hip, capi_quant.hip, capi_rows.hip.  Nothing here is exported.
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
// The calling thread's forwards record into `plan` for as long as the scope lives, however it is left.
struct PlanScope {
  NadPlan plan;
  PlanScope();
  ~PlanScope();
  PlanScope(const PlanScope&) = delete;
  PlanScope& operator=(const PlanScope&) = delete;
};
// A dry run: body (an entry's own, on stand-in arguments) with its launches recorded; -1 if it fails, else what
// write(plan) returns.  write_plan6 is the dense entries' writer: kernel, grid, block, ksplit, fold, launches, the
// first min(nout, 6) of them, and that count returned.
template <class F, class W>
static inline int dry_run(F&& body, W&& write) {
  PlanScope s;
  return body() ? -1 : write(s.plan);
}
int write_plan6(const NadPlan& p, int64_t* out, int nout);
template <class F>
static inline int dry_run6(int64_t* out, int nout, F&& body) {
  return dry_run(body, [&](const NadPlan& p) { return write_plan6(p, out, nout); });
}
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

// null, with the error set, for anything but a loaded weight -- or, inside a dry run, a geometry-only one
const nad::DeviceWeight* as_weight(const void* p);
// a loaded or a geometry-only weight, outside a dry run too ("<who>: weight descriptor is not a loaded ...")
const nad::DeviceWeight* any_weight(const char* who, const void* p);

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

// ------------------------------------------------------------------------------------------------ dry-run stand-ins
// The addresses a dry run passes where a call takes device memory: aligned, distinct, never dereferenced on the host.
// Role r starts at 2^(42 + r) and holds one 2^38-byte slot per object -- at most 4, where the workspace's range ends
// and the weights' begins -- so no two overlap:
//   2^40  the workspace of the dense forwards (workspace_for)
//   2^41  weight sections, slot i the call's i-th weight (plan_weight_assign)
//   2^42  activations
//   2^43  outputs, slot i the call's i-th (QKV, gate / up); a routed call's expert ids
//   2^44  the batch table (nad_batch_create); a routed call's combine weights
//   2^45, 2^46  a routed call's workspace and output (capi_moe.hip takes both from its caller)
// The 16-byte alignment of the activation address feeds vec_aligned and a_fast, and so the kernel choice.
enum StandIn {
  kStandWorkspace = -2, kStandWeight = -1, kStandAct = 0, kStandOut = 1, kStandTable = 2,
  kStandMoeIds = 1, kStandMoeWts = 2, kStandMoeWorkspace = 3, kStandMoeOut = 4
};
template <class T>
static inline T* stand_in(int role, int slot = 0) {
  return reinterpret_cast<T*>((uintptr_t(1) << (42 + role)) + (uintptr_t(slot) << 38));
}

// A weight made from scalars for the dry runs, in two steps: the geometry (bits = 6: GGUF Q6_K; blocksize is the
// caller's, already resolved) with every pointer null -- which is what marks a descriptor as geometry-only
// (nad_weight_plan_only stops here) -- then stand-in section pointers for the call's i-th weight.  An integer weight
// may fold its scales (fold_ok, which a load checks over the scales); the Q6_K kernels do not read the flag.
inline bool plan_geometry_ok(int bits, int n, int k, int scale_t) {
  return n > 0 && k > 0 && (bits == 2 || bits == 4 || bits == 6 || bits == 8) && (bits != 6 || k % 256 == 0) &&
         scale_t >= nad::kScaleF32 && scale_t <= nad::kScaleF16;
}
inline void plan_weight_geometry(nad::DeviceWeight& w, int bits, int n, int k, int blocksize, int scale_t, int asym,
                                 int act_order) {
  if (bits == 6) {
    nad::q6k_geometry(w, n, k);
    return;
  }
  w = nad::DeviceWeight{};
  nad::layout_geometry(w, bits, n, k, blocksize, scale_t, asym != 0, act_order != 0, false);
  w.fold_ok = 1;
}
inline void plan_weight_assign(nad::DeviceWeight& w, int i) {
  void* base = stand_in<void>(kStandWeight, i);
  if (is_q6k(w))
    nad::q6k_assign(w, base);
  else
    nad::layout_assign(w, base);
}

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

// capi_rows.hip, for its dry run in capi_plan.hip: nad_device_get_rows under the name `who` in its error texts
int get_rows(const char* who, const void* devstor, const int32_t* ids, int ids_stride, int m, void* out, int out_dtype,
             int ldo, hipStream_t st);

#pragma GCC visibility pop

extern "C" size_t nad_device_workspace_size(int m, int k);  // ne_ops.hip (include/neural_amd_ne.h)
