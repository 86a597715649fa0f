// capi.hip -- the extern "C" boundary (include/neural_amd.h): Neural Speed's BesTLA device/host/pack ABI re-hosted on
// MI355X.  Host-side orchestration only; all arithmetic on the hot path runs in woq_kernels.hip.  This unit holds the
// state the others share (capi_internal.h): errors, knobs, the dry-run recorder, the device context, the workspace and
// the compute mode.  Loading is in capi_load.hip, the forwards in capi_forward.hip, their dry runs in capi_plan.hip,
// the host-pointer half in capi_host.hip.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "capi_internal.h"

using namespace nad;

// ------------------------------------------------------------------------------------------------ errors
static thread_local std::string g_err;
void set_err(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}
void report(const char* where) { fprintf(stderr, "neural_amd: %s: %s\n", where, g_err.c_str()); }

extern "C" const char* nad_last_error(void) { return g_err.c_str(); }
extern "C" void nad_clear_error(void) { g_err.clear(); }

// ------------------------------------------------------------------------------------------------ knobs
static int env_int(const char* name, int def) {
  const char* v = getenv(name);
  return (v && *v) ? atoi(v) : def;
}

static Knobs read_knobs() {
  Knobs k{};
  k.gemv_grid = env_int("NAD_GEMV_GRID", 0);    // tests / tuning: cap the workgroups of a stripe-stream launch
  k.gemv_waves = env_int("NAD_GEMV_WAVES", 0);  // tests / tuning: waves of a stripe-stream launch
  k.gemv_nst = env_int("NAD_GEMV_NST", 0);  // register stages per wave: 0 auto; 1 or 2 (M = 1 kernel), 1 or 3 (M <= 16)
  k.gemv_lean = env_int("NAD_GEMV_LEAN", 1);
  // M = 1 launches on woq_gemv_m1s_kernel (compact arguments, weight count / reduce / epilogue at compile time) where
  // one is instantiated; 0: every launch on woq_gemv_m1_kernel with the full GemvArgs (A/B, bit-identity tests)
  k.gemv_m1_spec = env_int("NAD_GEMV_M1_SPEC", 1);
  // woq_gemv_m1s_kernel's load-ahead order wherever a form is instantiated (QKV, gate/up, one weight of two or more
  // stages per wave: all measured on, so unset = 1); 0: the present order everywhere (A/B, bit-identity tests)
  k.gemv_ahead = env_int("NAD_GEMV_AHEAD", 1) != 0;
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
const Knobs& knobs() { return g_knobs; }
// re-read the NAD_* switches (tests and A/B tools that change the environment at run time; not thread-safe against
// concurrent forwards)
extern "C" void nad_reload_knobs(void) { g_knobs = read_knobs(); }

// ------------------------------------------------------------------------------------------------ dry runs
static thread_local NadPlan* t_plan = nullptr;
static void set_plan(NadPlan* p) { t_plan = p; }
PlanScope::PlanScope() { set_plan(&plan); }
PlanScope::~PlanScope() { set_plan(nullptr); }
int write_plan6(const NadPlan& p, int64_t* out, int nout) {
  const int64_t v[6] = {p.kernel, p.grid, p.block, p.ksplit, p.fold, p.launches};
  const int c = nout < 6 ? nout : 6;
  std::memcpy(out, v, sizeof(int64_t) * size_t(c));
  return c;
}
bool planning() { return t_plan != nullptr; }
bool planned(int kernel, int grid, int block, int ksplit, int fold, bool main, size_t lds) {
  if (!t_plan) return false;
  if (t_plan->launches < NadPlan::kListMax) {
    int64_t* l = t_plan->list[t_plan->launches];
    l[0] = kernel;
    l[1] = grid;
    l[2] = block;
    l[3] = int64_t(lds);
  }
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
// the name, and from it flag bit 4 (woq_gemv_m1s_kernel: family 3) and bit 8 (its load-ahead order)
void plan_gemv_instance(uint32_t inst) {
  if (!t_plan) return;
  const int m1s = (inst & 3u) == 3u ? 4 : 0, ahead = (inst >> 24 & 1u) ? 8 : 0;
  t_plan->fold |= m1s | ahead | int(inst) << nad::kPlanGemvInstShift;
}

// ------------------------------------------------------------------------------------------------ device context
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

const DeviceWeight* as_weight(const void* p) {
  const auto* w = static_cast<const DeviceWeight*>(p);
  if (!w || w->magic != kWeightMagic) {
    set_err("weight descriptor is not a loaded neural_amd device weight");
    return nullptr;
  }
  if (!w->tiles && !planning()) {  // nad_weight_plan_only: dry runs only, nothing may be launched on it
    set_err("weight descriptor is geometry-only (nad_weight_plan_only): it holds no weights");
    return nullptr;
  }
  return w;
}
const DeviceWeight* any_weight(const char* who, const void* p) {
  const auto* w = static_cast<const DeviceWeight*>(p);
  if (w && w->magic == kWeightMagic) return w;
  set_err("%s: weight descriptor is not a loaded neural_amd device weight", who);
  return nullptr;
}

// ------------------------------------------------------------------------------------------------ staging
int staging_finish(const char* who, Staging& s) {
  if (s.finish() == hipSuccess) return 0;
  set_err("%s: %s failed: %s", who, s.what(), hipGetErrorString(s.error()));
  return -1;
}

// ------------------------------------------------------------------------------------------------ workspace
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
}  // namespace

CallWorkspace::CallWorkspace(void* p, size_t b) { t_call_ws = WsRef{p, p ? b : 0}; }
CallWorkspace::~CallWorkspace() { t_call_ws = WsRef{}; }

extern "C" int nad_bind_workspace(void* queue, void* ptr, size_t bytes) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  hipStream_t st = static_cast<hipStream_t>(queue);
  if (!ptr || !bytes)
    g_bound_ws.erase(st);
  else
    g_bound_ws[st] = WsRef{ptr, bytes};
  return 0;
}

void* workspace_for(size_t bytes, hipStream_t st) {
  if (t_plan) return stand_in<void>(kStandWorkspace);  // dry run: sized, never touched
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

// ------------------------------------------------------------------------------------------------ compute mode
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
int gguf_act_quant(const DeviceWeight& w) {
  const GgufType* t = gguf_type_by_tag(w.src_core_id);  // null: no GGUF matrix
  return t ? t->act_quant : 0;
}
static int effective_mode(const DeviceWeight& w) { return w.compute > 0 ? w.compute - 1 : compute_mode(); }
bool int8_compute(const DeviceWeight& w) {
  return effective_mode(w) == 1 && (w.reduce != nullptr || gguf_act_quant(w) != 0);
}
// Mode 2 (NAD_COMPUTE_Q8_K) is a GGUF Q6_K weight's own setting only: the reference's Q8_K activation rows and
// ggml_vec_dot_q6_K_q8_K integer dot product (woq_q6k_i8_kernel).  The thread and process modes keep their two values,
// so a Q6_K weight never follows them into integer arithmetic.
bool q8k_compute(const DeviceWeight& w) { return is_q6k(w) && w.compute == NAD_COMPUTE_Q8_K + 1; }

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
  if (mode < -1 || mode > NAD_COMPUTE_Q8_K) {
    set_err("weight compute mode must be -1 (follow the thread/process setting), 0 (fp), 1 (int8) or 2 (Q8_K, GGUF "
            "Q6_K weights only), got %d", mode);
    return -1;
  }
  if (mode == NAD_COMPUTE_Q8_K && !is_q6k(*w)) {
    set_err("weight compute mode 2 (Q8_K integer arithmetic) is for GGUF Q6_K weights only; this weight has bits = %d",
            w->bits);
    return -1;
  }
  w->compute = mode + 1;
  return 0;
}
// the arithmetic a forward of this weight takes right now: 0 fp, 1 int8, 2 Q8_K (a Q6_K weight set to it)
extern "C" int nad_device_get_compute(const void* devstor) {
  const DeviceWeight* w = static_cast<const DeviceWeight*>(devstor);
  if (!w || w->magic != kWeightMagic) {
    set_err("nad_device_get_compute: not a device weight");
    return -1;
  }
  if (q8k_compute(*w)) return NAD_COMPUTE_Q8_K;
  return int8_compute(*w) ? 1 : 0;
}
