// capi_moe.hip -- Mixtral-style expert FFNs with the routing read on the device (include/neural_amd.h, "routed expert
// matmuls"): the expert bank, nad_device_mul_mat_id (ne_mul_mat_id, ne_layers.c:2384-2462, 7783-7916),
// nad_device_moe_ffn (models/llama/llama.cpp:641-679), the router (llama.cpp:624-638) and the dry run.  The hot path is
// woq_gemv_m1_routed_kernel (woq_gemv.hip); the bank's device table is the feature's only allocation.
#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace nad;

namespace {
constexpr uint32_t kBankMagic = 0x4b424e41u;  // "ANBK"
constexpr int kMaxExperts = 256;

struct NadExpertBank {
  uint32_t magic = kBankMagic;
  int n_expert = 0;
  DeviceWeight w0{};             // the shape and format every expert shares (its pointers are expert 0's)
  GemvExpertEnt* dev = nullptr;  // [n_expert]; null for a geometry-only bank (nad_expert_bank_plan_only)
};

const NadExpertBank* as_bank(const void* p, const char* who, const char* role) {
  const auto* b = static_cast<const NadExpertBank*>(p);
  if (!b || b->magic != kBankMagic) {
    set_err("%s: the %s bank is not an expert bank (nad_expert_bank_create)", who, role);
    return nullptr;
  }
  return b;
}

// nad_batch_create's conditions, per expert (the callers have checked 1 <= n <= kMaxExperts)
bool bank_check(const DeviceWeight* const* ws, int n, const char* who) {
  const DeviceWeight& w0 = *ws[0];
  for (int i = 0; i < n; i++) {
    const DeviceWeight& w = *ws[i];
    if (is_q6k(w)) {  // the routed GEMV streams the int4 / int2 tile layouts only
      set_err("%s: expert %d's weight is GGUF Q6_K, which the routed GEMV does not stream", who, i);
      return false;
    }
    if ((w.bits != 4 && w.bits != 2) || w.f4kind >= 0) {
      set_err("%s: expert %d's weight is not in the int4 / int2 tile layout (bits %d%s)", who, i, w.bits,
              w.f4kind >= 0 ? ", NFloat codes" : "");
      return false;
    }
    if (w.n != w0.n || w.k != w0.k || w.bits != w0.bits || w.blocksize != w0.blocksize || w.asym != w0.asym ||
        w.scale_t != w0.scale_t || w.nt != w0.nt || w.ng != w0.ng || w.kmajor != w0.kmajor) {
      set_err("%s: expert %d's weight differs in shape or format from expert 0's", who, i);
      return false;
    }
    if (w.shuffle || w.has_shuffle) {
      set_err("%s: expert %d's weight is act-order (desc_act), which is not routed", who, i);
      return false;
    }
    if (int8_compute(w) || q8k_compute(w)) {
      set_err("%s: expert %d's weight is set to integer (int8 / Q8_K) arithmetic, which is not routed", who, i);
      return false;
    }
    if (w.mins) {  // the routed GEMV has no min-term pass: it would drop S (m + bias d)^T
      set_err("%s: expert %d's weight carries block mins (GGUF Q4_1 / Q5_1), which are not routed", who, i);
      return false;
    }
  }
  GemvArgs a{};
  int waves = 0;
  if (!prepare_m1_problem(a, waves, ws, 1, kEpiNone)) {
    set_err("%s: expert 0's weight geometry (n %d, k %d, group %d) does not take the M = 1 GEMV", who, w0.n, w0.k,
            w0.blocksize);
    return false;
  }
  return true;
}

// One routed launch: the GemvArgs of one problem, the workgroups per problem and the grid
struct RoutedGeom {
  GemvArgs a{};
  int bits = 0, waves = 0, wpp = 0, grid = 0;
  size_t lds = 0;
};

// up == nullptr: one weight per problem; else the {gate, up} pair under the dual epilogue epi.  Workgroups per
// problem as nad_batch_create deals them: the chip's CUs over the problems, at least one, more where one problem's
// share of the stripes would not fit a workgroup's partial-sum slots.
bool routed_geometry(RoutedGeom& g, const NadExpertBank& w, const NadExpertBank* up, int epi, int64_t nprob,
                     const char* who) {
  const DeviceWeight* ws[2] = {&w.w0, up ? &up->w0 : nullptr};
  if (!prepare_m1_problem(g.a, g.waves, ws, up ? 2 : 1, epi)) {
    set_err("%s: this weight geometry does not take the M = 1 GEMV", who);
    return false;
  }
  g.bits = w.w0.bits;
  const int units = g.a.units;
  int wpp = int(std::max<int64_t>(1, std::min<int64_t>(units, device_cus() / nprob)));
  for (;; wpp++) {
    g.a.u_q = units / wpp;
    g.a.u_r = units % wpp;
    g.lds = gemv_lds_layout(g.a, g.bits, g.waves, wpp);
    if (g.lds <= 160 * 1024 || wpp >= units) break;
  }
  if (g.lds > 160 * 1024) {
    set_err("%s: LDS layout does not fit", who);
    return false;
  }
  if (nprob * wpp >= (int64_t(1) << 31)) {
    set_err("%s: %lld problems are more than one launch takes", who, static_cast<long long>(nprob));
    return false;
  }
  g.wpp = wpp;
  g.grid = int(nprob * wpp);
  return true;
}

int run_routed(const RoutedGeom& g, GemvRouted r, hipStream_t st) {
  r.wpp = g.wpp;
  return launch(planned(NAD_KERNEL_GEMV_ROUTED, g.grid, g.waves * 64), "routed gemv kernel",
                [&] { return launch_gemv_routed(g.a, r, g.bits, g.waves, g.grid, g.lds, st); })
             ? 0
             : -1;
}

bool rows_ok(const float* act, int lda, int k, const char* who) {
  if (lda % 4 != 0 || lda < k || reinterpret_cast<uintptr_t>(act) % 16 != 0) {
    set_err("%s: the activation rows need a 16-B aligned base and lda %% 4 == 0, lda >= k (lda %d, k %d)", who, lda, k);
    return false;
  }
  return true;
}

bool launchable(const NadExpertBank& b, const char* who) {
  if (b.dev) return true;
  set_err("%s: a geometry-only bank (nad_expert_bank_plan_only) holds no weights", who);
  return false;
}

// gate and up must agree in everything the dual launch shares
bool pair_ok(const NadExpertBank& g, const NadExpertBank& u, const NadExpertBank& d, const char* who) {
  const DeviceWeight &a = g.w0, &b = u.w0;
  if (a.blocksize != b.blocksize) {
    set_err("%s: the gate and up banks differ in group size (%d vs %d)", who, a.blocksize, b.blocksize);
    return false;
  }
  if (a.k != b.k || a.n != b.n || a.bits != b.bits || a.scale_t != b.scale_t || a.asym != b.asym || a.nt != b.nt ||
      a.ng != b.ng) {
    set_err("%s: the gate and up banks differ in shape or format (K, N, bits, scale type and symmetry must agree)", who);
    return false;
  }
  if (d.w0.k != a.n) {
    set_err("%s: the down bank's K (%d) is not the gate bank's N (%d)", who, d.w0.k, a.n);
    return false;
  }
  if (g.n_expert != u.n_expert || g.n_expert != d.n_expert) {
    set_err("%s: the banks hold %d / %d / %d experts", who, g.n_expert, u.n_expert, d.n_expert);
    return false;
  }
  return true;
}

size_t ws_part(int64_t rows, int cols) { return size_t(align256(uint64_t(rows) * uint64_t(cols) * sizeof(float))); }

NadExpertBank* bank_new(const DeviceWeight* const* ws, int n, const char* who) {
  if (!bank_check(ws, n, who)) return nullptr;
  auto* b = new NadExpertBank();
  b->n_expert = n;
  b->w0 = *ws[0];
  return b;
}
}  // namespace

extern "C" void* nad_expert_bank_create(const void* const* weights, int n_expert) {
  const char* who = "nad_expert_bank_create";
  if (!weights || n_expert < 1 || n_expert > kMaxExperts) {
    set_err("%s: need 1..%d experts (got %d)", who, kMaxExperts, n_expert);
    return nullptr;
  }
  std::vector<const DeviceWeight*> ws(static_cast<size_t>(n_expert));
  for (int i = 0; i < n_expert; i++)
    if (!(ws[size_t(i)] = as_weight(weights[i]))) {
      set_err("%s: expert %d's descriptor is not a loaded neural_amd device weight", who, i);
      return nullptr;
    }
  NadExpertBank* b = bank_new(ws.data(), n_expert, who);
  if (!b) return nullptr;
  std::vector<GemvExpertEnt> host(static_cast<size_t>(n_expert));
  for (int i = 0; i < n_expert; i++) {
    const DeviceWeight* w = ws[size_t(i)];
    host[size_t(i)] = GemvExpertEnt{w->tiles, w->scales, w->zps, {nullptr, nullptr, nullptr, nullptr, nullptr}};
  }
  const size_t bytes = sizeof(GemvExpertEnt) * size_t(n_expert);
  if (hipMalloc(&b->dev, bytes) != hipSuccess || hipMemcpy(b->dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    set_err("%s: device table allocation failed", who);
    if (b->dev) (void)hipFree(b->dev);
    delete b;
    return nullptr;
  }
  return b;
}

extern "C" void* nad_expert_bank_plan_only(const int32_t* geom, int n_expert) {
  const char* who = "nad_expert_bank_plan_only";
  if (!geom || n_expert < 1 || n_expert > kMaxExperts) {
    set_err("%s: need 1..%d experts (got %d)", who, kMaxExperts, n_expert);
    return nullptr;
  }
  std::vector<DeviceWeight> store(static_cast<size_t>(n_expert));
  std::vector<const DeviceWeight*> ws(static_cast<size_t>(n_expert));
  for (int i = 0; i < n_expert; i++) {
    const int32_t* g = geom + 6 * i;
    const int bits = g[0], n = g[1], k = g[2], asym = g[5];
    DeviceWeight& w = store[size_t(i)];
    if (n <= 0 || k <= 0 || (bits != 2 && bits != 4 && bits != 6 && bits != 8) || (bits == 6 && k % 256 != 0) ||
        g[4] < kScaleF32 || g[4] > kScaleF16) {
      set_err("%s: expert %d: bad geometry (bits=%d n=%d k=%d scale=%d)", who, i, bits, n, k, g[4]);
      return nullptr;
    }
    void* fake = reinterpret_cast<void*>(uintptr_t(1) << 41);  // never dereferenced on the host
    if (bits == 6) {
      q6k_geometry(w, n, k);
      q6k_assign(w, fake);
    } else {
      w = DeviceWeight{};
      layout_geometry(w, bits, n, k, g[3] <= 0 ? k : g[3], g[4], asym != 0, false, false);
      layout_assign(w, fake);
      w.fold_ok = 1;
    }
    ws[size_t(i)] = &w;
  }
  return bank_new(ws.data(), n_expert, who);
}

extern "C" void nad_expert_bank_destroy(void* bank) {
  auto* b = static_cast<NadExpertBank*>(bank);
  if (!b || b->magic != kBankMagic) return;
  if (b->dev) (void)hipFree(b->dev);
  b->magic = 0;
  delete b;
}

extern "C" int nad_expert_bank_info(const void* bank, int64_t* out, int nout) {
  const NadExpertBank* b = as_bank(bank, "nad_expert_bank_info", "given");
  if (!b || !out || nout < 0) return -1;
  const DeviceWeight& w = b->w0;
  const int64_t v[8] = {b->n_expert, w.bits, w.n, w.k, w.blocksize, w.scale_t, w.asym, b->dev ? 1 : 0};
  const int c = std::min(nout, 8);
  std::memcpy(out, v, sizeof(int64_t) * size_t(c));
  return c;
}

extern "C" int nad_device_mul_mat_id(const void* bank, const float* act, const int32_t* ids, int ids_ld, int slot,
                                     float* out, int m, int lda, int ldo, void* queue) {
  const char* who = "nad_device_mul_mat_id";
  const NadExpertBank* b = as_bank(bank, who, "given");
  if (!b) return -1;
  if (!act || !ids || !out || m < 0 || slot < 0 || slot >= ids_ld || ldo < b->w0.n) {
    set_err("%s: bad arguments (m=%d slot=%d ids_ld=%d ldo=%d n=%d)", who, m, slot, ids_ld, ldo, b->w0.n);
    return -1;
  }
  if (!rows_ok(act, lda, b->w0.k, who) || !launchable(*b, who)) return -1;
  if (m == 0) return 0;
  RoutedGeom g;
  if (!routed_geometry(g, *b, nullptr, kEpiNone, m, who)) return -1;
  GemvRouted r{};
  r.bank[0] = b->dev;
  r.n_expert = b->n_expert;
  r.ids = ids;
  r.ids_ld = ids_ld;
  r.ids_col = slot;
  r.slots = 1;
  r.act = act;
  r.act_ld = lda;
  r.out = out;
  r.out_ld = ldo;
  return run_routed(g, r, static_cast<hipStream_t>(queue));
}

extern "C" size_t nad_moe_workspace_size(int m, int top_k, int fmid, int fout) {
  if (m <= 0 || top_k <= 0 || fmid <= 0 || fout <= 0) return 0;
  const int64_t p = int64_t(m) * top_k;
  return ws_part(p, fmid) + ws_part(p, fout);
}

extern "C" int nad_device_moe_ffn(const void* gate_bank, const void* up_bank, const void* down_bank, const float* act,
                                  const int32_t* ids, int ids_ld, const float* wts, int wts_ld, int top_k, int epi,
                                  void* workspace, float* out, int m, int lda, int ldo, void* queue) {
  const char* who = "nad_device_moe_ffn";
  const NadExpertBank* gb = as_bank(gate_bank, who, "gate");
  const NadExpertBank* ub = gb ? as_bank(up_bank, who, "up") : nullptr;
  const NadExpertBank* db = ub ? as_bank(down_bank, who, "down") : nullptr;
  if (!db) return -1;
  if (epi != kEpiSiluMul && epi != kEpiGeluMul) {
    set_err("%s: the epilogue must be SILU_MUL or GELU_MUL", who);
    return -1;
  }
  if (!pair_ok(*gb, *ub, *db, who)) return -1;
  const int fin = gb->w0.k, fmid = gb->w0.n, fout = db->w0.n;
  if (!act || !ids || !wts || !workspace || !out || m < 0 || top_k < 1 || top_k > ids_ld || top_k > wts_ld ||
      ldo < fout || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
    set_err("%s: bad arguments (m=%d top_k=%d ids_ld=%d wts_ld=%d ldo=%d fout=%d; the workspace 16-B aligned)", who, m,
            top_k, ids_ld, wts_ld, ldo, fout);
    return -1;
  }
  if (!rows_ok(act, lda, fin, who) || !launchable(*gb, who) || !launchable(*ub, who) || !launchable(*db, who)) return -1;
  if (m == 0) return 0;
  const int64_t np = int64_t(m) * top_k;
  RoutedGeom g1, g2;
  if (!routed_geometry(g1, *gb, ub, epi, np, who) || !routed_geometry(g2, *db, nullptr, kEpiNone, np, who)) return -1;
  hipStream_t st = static_cast<hipStream_t>(queue);
  float* t = static_cast<float*>(workspace);                                         // [np][fmid]
  float* y = reinterpret_cast<float*>(static_cast<char*>(workspace) + ws_part(np, fmid));  // [np][fout]
  GemvRouted r{};
  r.n_expert = gb->n_expert;
  r.ids = ids;
  r.ids_ld = ids_ld;
  r.ids_col = 0;
  r.slots = top_k;
  // launch 1: t[p] = act1(x_r . G_e^T) * (x_r . U_e^T)
  r.bank[0] = gb->dev;
  r.bank[1] = ub->dev;
  r.act = act;
  r.act_ld = lda;
  r.act_per_slot = 0;
  r.out = t;
  r.out_ld = fmid;
  if (run_routed(g1, r, st)) return -1;
  // launch 2: y[p] = t[p] . D_e^T
  r.bank[0] = db->dev;
  r.bank[1] = nullptr;
  r.act = t;
  r.act_ld = fmid;
  r.act_per_slot = 1;
  r.out = y;
  r.out_ld = fout;
  if (run_routed(g2, r, st)) return -1;
  // launch 3: out[r] = sum_i w[r][i] * y[r * top_k + i], in slot order
  MoeCombineArgs c{y, fout, wts, wts_ld, top_k, out, ldo, m, fout};
  return launch(planned(NAD_KERNEL_MOE_COMBINE, ((fout + 255) / 256) * m, 256), "moe combine kernel",
                [&] { return launch_moe_combine(c, st); })
             ? 0
             : -1;
}

extern "C" int nad_plan_moe(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k,
                            int64_t* out, int nout) {
  const char* who = "nad_plan_moe";
  const NadExpertBank* gb = as_bank(gate_bank, who, "gate");
  const NadExpertBank* ub = gb ? as_bank(up_bank, who, "up") : nullptr;
  const NadExpertBank* db = ub ? as_bank(down_bank, who, "down") : nullptr;
  if (!db) return -1;
  if (!out || nout < 0 || m <= 0 || top_k <= 0) {
    set_err("%s: bad arguments (m=%d top_k=%d)", who, m, top_k);
    return -1;
  }
  if (!pair_ok(*gb, *ub, *db, who)) return -1;
  const int64_t np = int64_t(m) * top_k;
  RoutedGeom g1, g2;
  if (!routed_geometry(g1, *gb, ub, kEpiSiluMul, np, who) || !routed_geometry(g2, *db, nullptr, kEpiNone, np, who))
    return -1;
  const int fout = db->w0.n;
  const int64_t v[13] = {NAD_KERNEL_GEMV_ROUTED, g1.grid, g1.waves * 64, int64_t(g1.lds),
                         NAD_KERNEL_GEMV_ROUTED, g2.grid, g2.waves * 64, int64_t(g2.lds),
                         NAD_KERNEL_MOE_COMBINE, int64_t((fout + 255) / 256) * m, 256, 0,
                         3};
  const int c = std::min(nout, 13);
  std::memcpy(out, v, sizeof(int64_t) * size_t(c));
  return c;
}

extern "C" int nad_moe_route(const float* logits, int ld, int m, int n_expert, int top_k, int32_t* ids, int ids_ld,
                             float* wts, int wts_ld, void* queue) {
  if (!logits || !ids || !wts || m < 0 || n_expert < 1 || n_expert > 64 || top_k < 1 || top_k > n_expert ||
      ld < n_expert || ids_ld < top_k || wts_ld < top_k) {
    set_err("nad_moe_route: bad arguments (m=%d n_expert=%d (1..64) top_k=%d ld=%d ids_ld=%d wts_ld=%d)", m, n_expert,
            top_k, ld, ids_ld, wts_ld);
    return -1;
  }
  if (m == 0) return 0;
  const MoeRouteArgs a{logits, ld, m, n_expert, top_k, ids, ids_ld, wts, wts_ld};
  return launch(planned_pass(), "moe route kernel", [&] { return launch_moe_route(a, static_cast<hipStream_t>(queue)); })
             ? 0
             : -1;
}
