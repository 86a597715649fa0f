// capi_host.hip -- the host-pointer half of the ABI (ne_bestla.h:21-83): a default device context and a per-blob
// weight cache in front of the device entries, the pack API and the tensor-parallel blob split.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "capi_internal.h"

using namespace nad;

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
  // an output of `rows` rows of `width` bytes, `pitch` bytes apart (pitch > width): only those come back, the
  // caller's bytes between the rows stay as they are.  rows = 0: one flat span of `bytes`.
  size_t rows = 0, width = 0, pitch = 0;
};
// the staged form of an output matrix [rows][n] fp32 with row stride ld: flat when contiguous
HostBuf out_buf(float* p, size_t rows, int n, int ld) {
  HostBuf b{p, (rows - 1) * size_t(ld) * 4 + size_t(n) * 4, true, nullptr};
  if (ld > n) {
    b.rows = rows;
    b.width = size_t(n) * 4;
    b.pitch = size_t(ld) * 4;
  }
  return b;
}
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
    if (b.out && b.host && b.dev != b.host) {
      if (b.rows)
        HIP_OK(hipMemcpy2DAsync(const_cast<void*>(b.host), b.pitch, b.dev, b.pitch, b.width, b.rows,
                                hipMemcpyDeviceToHost, st));
      else
        HIP_OK(hipMemcpyAsync(const_cast<void*>(b.host), b.dev, b.bytes, hipMemcpyDeviceToHost, st));
    }
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
                               out_buf(out, size_t(m), n, ldo),
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
  // the three matrices lie m * ldo floats apart: 3 m rows of one pitch
  std::vector<HostBuf> bufs = {{activation, size_t(_m - 1) * lda * 4 + size_t(_k) * 4, false, nullptr},
                               out_buf(output, size_t(3) * _m, _n, ldo)};
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
