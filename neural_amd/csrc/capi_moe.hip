// capi_moe.hip -- Mixtral-style expert FFNs with the routing read on the device (include/neural_amd.h, "routed expert
// matmuls"): the expert bank, nad_device_mul_mat_id (ne_mul_mat_id, ne_layers.c:2384-2462, 7783-7916),
// nad_device_moe_ffn (models/llama/llama.cpp:641-679), the router (llama.cpp:624-638) and the dry run.  The hot path is
// woq_gemv_m1_routed_kernel, or woq_gemv_routed_kernel for a general bank's int4 g32 / int8 weights (woq_gemv.hip), or
// woq_q6k_gemv_routed_kernel for a bank of GGUF Q6_K experts (woq_q6k.hip); the bank's device table is the feature's
// only allocation.  For prefill
// sizes the sorted, grouped entries (nad_device_moe_ffn_grouped, nad_device_mul_mat_id_grouped): moe_sort_kernel
// (woq_moe.hip), then woq_gemm7_grouped_kernel (woq_gemm7.hip) -- a Q6_K bank: woq_q6k_gemm_grouped_kernel -- over
// every expert's sorted rows.
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
  bool g7_ok = false;            // every expert takes gemm7 (gemm7_ok, stripe-major): the grouped entries serve the bank
  int kind = 0;                  // the routed launch that serves it: 0 the M = 1 stream, 1 the stripe stream, 2 the Q6_K
                                 // GEMV (1 and 2: NAD_BANK_GENERAL)
};
constexpr int kBankLean = 0, kBankStripe = 1, kBankQ6k = 2;

const NadExpertBank* as_bank(const void* p, const char* who, const char* role) {
  const auto* b = static_cast<const NadExpertBank*>(p);
  if (!b || b->magic != kBankMagic) {
    set_err("%s: the %s bank is not an expert bank (nad_expert_bank_create)", who, role);
    return nullptr;
  }
  return b;
}

// nad_batch_create's conditions, per expert (the callers have checked 1 <= n <= kMaxExperts)
// general (NAD_BANK_GENERAL): also the weights the stripe-stream GEMV runs at M = 1 where the M = 1 stream does not --
// int4 groups of 32 sym, int8 -- and a bank whose experts are all GGUF Q6_K (woq_q6k_gemv_routed_kernel), with kind set
// to the launch that serves the bank
bool bank_check(const DeviceWeight* const* ws, int n, const char* who, bool general, int& kind) {
  const DeviceWeight& w0 = *ws[0];
  kind = kBankLean;
  const bool q6k = general && is_q6k(w0);  // a Q6_K bank: every expert must be one (expert 0's shape and format)
  for (int i = 0; i < n; i++) {
    const DeviceWeight& w = *ws[i];
    if (is_q6k(w) && !q6k) {  // the routed GEMV streams the int4 / int2 (/ int8) tile layouts only
      set_err("%s: expert %d's weight is GGUF Q6_K, which the routed GEMV does not stream%s", who, i,
              is_q6k(w0) ? " (a bank whose experts are all Q6_K needs NAD_BANK_GENERAL)"
                         : " beside other formats (a bank of Q6_K experts holds nothing else)");
      return false;
    }
    if (!is_q6k(w) && ((w.bits != 4 && w.bits != 2 && !(general && w.bits == 8)) || w.f4kind >= 0)) {
      set_err("%s: expert %d's weight is not in the int4 / int2%s tile layout (bits %d%s)", who, i,
              general ? " / int8" : "", w.bits, w.f4kind >= 0 ? ", NFloat codes" : "");
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
  if (q6k) {  // any n, any k % 256 == 0 (the loader's condition); the routed launch checks its LDS staging of K itself
    kind = kBankQ6k;
    return true;
  }
  GemvArgs a{};
  int waves = 0;
  if (prepare_m1_problem(a, waves, ws, 1, kEpiNone)) return true;
  if (!general) {
    set_err("%s: expert 0's weight geometry (n %d, k %d, group %d) does not take the M = 1 GEMV", who, w0.n, w0.k,
            w0.blocksize);
    return false;
  }
  if (w0.bits == 4 && w0.blocksize == 32 && w0.asym) {
    set_err("%s: int4 groups of 32 with zero points run on the skinny kernel, which is not routed", who);
    return false;
  }
  if (!((w0.bits == 4 && w0.blocksize == 32) || w0.bits == 8) || !prepare_general_problem(a, waves, ws, 1, kEpiNone)) {
    set_err("%s: expert 0's weight geometry (int%d, n %d, k %d, group %d) takes neither the M = 1 GEMV nor the routed "
            "stripe stream (int4 groups of 32 sym; int8 groups of 32, 64 * 2^j or one per channel)", who, w0.bits, w0.n,
            w0.k, w0.blocksize);
    return false;
  }
  kind = kBankStripe;
  return true;
}

// One routed launch: the GemvArgs of one problem, the workgroups per problem and the grid
struct RoutedGeom {
  GemvArgs a{};
  int bits = 0, waves = 0, wpp = 0, grid = 0, kind = kBankLean;
  size_t lds = 0;
  // a Q6_K bank (kBankQ6k; a unused): the bank, and the single-weight epilogue of the launch -- none, the gate
  // activation, or kEpiSiluMul with the problem's own output row as the multiplier (q6k_aux_out)
  const NadExpertBank* q6k = nullptr;
  int q6k_epi = kEpiNone;
  bool q6k_aux_out = false;
  int kernel() const {
    return kind == kBankQ6k ? NAD_KERNEL_Q6K_GEMV_ROUTED
                            : (kind == kBankStripe ? NAD_KERNEL_GEMV_ROUTED_GENERAL : NAD_KERNEL_GEMV_ROUTED);
  }
};

// A Q6_K bank's launch: one weight per problem (the FFN runs gate and up as two launches, as the dense Q6_K FFN does)
bool routed_geometry_q6k(RoutedGeom& g, const NadExpertBank& w, int epi, bool aux_out, int64_t nprob, const char* who) {
  Q6kRoutedGeom q{};
  g.kind = kBankQ6k;
  g.bits = 6;
  g.q6k = &w;
  g.q6k_epi = epi;
  g.q6k_aux_out = aux_out;
  if (!q6k_routed_geometry(w.w0.k, w.w0.ns, nprob, device_cus(), &q)) {
    if (q.lds > 160 * 1024)
      set_err("%s: K = %d is too long for the routed Q6_K kernel's LDS staging of one activation row (its hi and lo "
              "fp16 rows beside the 32 KiB of partial sums exceed 160 KiB)", who, w.w0.k);
    else
      set_err("%s: %lld problems are more than one launch takes", who, static_cast<long long>(nprob));
    return false;
  }
  g.waves = q.waves;
  g.wpp = q.wpp;
  g.grid = q.grid;
  g.lds = q.lds;
  return true;
}

// up == nullptr: one weight per problem; else the {gate, up} pair under the dual epilogue epi.  Workgroups per
// problem as nad_batch_create deals them: the chip's CUs over the problems, at least one, more where one problem's
// share of the stripes would not fit a workgroup's partial-sum slots.
bool routed_geometry(RoutedGeom& g, const NadExpertBank& w, const NadExpertBank* up, int epi, int64_t nprob,
                     const char* who) {
  if (w.kind == kBankQ6k) {
    if (!up) return routed_geometry_q6k(g, w, epi, false, nprob, who);
    set_err("%s: a Q6_K pair runs as two launches", who);  // the callers do; not reached
    return false;
  }
  const DeviceWeight* ws[2] = {&w.w0, up ? &up->w0 : nullptr};
  g.kind = w.kind;
  if (!(g.kind == kBankStripe ? prepare_general_problem : prepare_m1_problem)(g.a, g.waves, ws, up ? 2 : 1, epi)) {
    set_err("%s: this weight geometry does not take the %s", who,
            g.kind == kBankStripe ? "routed stripe stream" : "M = 1 GEMV");
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

SkinnyWeight bank_view(const NadExpertBank& b, float* out, int ldo);

int run_routed(const RoutedGeom& g, GemvRouted r, hipStream_t st) {
  r.wpp = g.wpp;
  if (g.kind == kBankQ6k) {
    const DeviceWeight& w = g.q6k->w0;
    GemmArgs a{};  // one problem: M = 1; the kernel fills A, the weight's pointers, the output row and aux
    a.M = 1;
    a.K = w.k;
    a.lda = r.act_ld;
    a.scale_t = w.scale_t;
    a.epi = g.q6k_epi;
    a.vec_ok = 1;  // rows_ok: a 16-B base and lda % 4 == 0 (the FFN's t rows: K = fmid, a multiple of 256)
    a.w = bank_view(*g.q6k, nullptr, w.n);
    const Q6kRoutedGeom q{g.wpp, g.grid, g.waves, g.lds};
    return launch(planned(g.kernel(), g.grid, g.waves * 64), "routed Q6_K gemv kernel",
                  [&] { return launch_q6k_gemv_routed(a, r, g.q6k_aux_out, q, st); })
               ? 0
               : -1;
  }
  return launch(planned(g.kernel(), g.grid, g.waves * 64), "routed gemv kernel",
                [&] {
                  return g.kind == kBankStripe
                             ? launch_gemv_routed_general(g.a, r, g.bits, g.waves, g.grid, g.lds, st)
                             : launch_gemv_routed(g.a, r, g.bits, g.waves, g.grid, g.lds, st);
                })
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

int gate_epi(int dual);

// The routed launches of one FFN: g1 the {gate, up} pair under the dual epilogue -- or, for a Q6_K pair, the gate under
// its activation alone and g1u the up weight times the gate's result in place -- and g2 the down weight.  Each launch
// is served by its own bank's kernel.
bool ffn_geometry(RoutedGeom& g1, RoutedGeom& g1u, RoutedGeom& g2, const NadExpertBank& gb, const NadExpertBank& ub,
                  const NadExpertBank& db, int epi, int64_t np, const char* who) {
  if (gb.kind == kBankQ6k) {
    if (!routed_geometry_q6k(g1, gb, gate_epi(epi), false, np, who) ||
        !routed_geometry_q6k(g1u, ub, kEpiSiluMul, true, np, who))
      return false;
  } else if (!routed_geometry(g1, gb, &ub, epi, np, who)) {
    return false;
  }
  return routed_geometry(g2, db, nullptr, kEpiNone, np, who);
}

size_t ws_part(int64_t rows, int cols) { return size_t(align256(uint64_t(rows) * uint64_t(cols) * sizeof(float))); }

NadExpertBank* bank_new(const DeviceWeight* const* ws, int n, const char* who, bool general) {
  int kind = kBankLean;
  if (!bank_check(ws, n, who, general, kind)) return nullptr;
  auto* b = new NadExpertBank();
  b->n_expert = n;
  b->w0 = *ws[0];
  b->kind = kind;
  b->g7_ok = true;
  // groups of 32 (a stripe-stream bank's) have grouped gemm7 instantiations too; a lean bank never holds them
  for (int i = 0; i < n; i++)
    b->g7_ok = b->g7_ok && !ws[i]->kmajor && (kind == kBankStripe || ws[i]->blocksize >= 64) &&
               gemm7_ok(ws[i]->bits, ws[i]->blocksize, ws[i]->fold_ok);
  return b;
}

bool flags_ok(unsigned flags, const char* who) {
  if ((flags & ~NAD_BANK_GENERAL) == 0) return true;
  set_err("%s: unknown flags 0x%x (NAD_BANK_GENERAL is the only one)", who, flags);
  return false;
}

void* bank_create(const void* const* weights, int n_expert, unsigned flags, const char* who) {
  if (!flags_ok(flags, who)) return nullptr;
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
  NadExpertBank* b = bank_new(ws.data(), n_expert, who, (flags & NAD_BANK_GENERAL) != 0);
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

void* bank_plan_only(const int32_t* geom, int n_expert, unsigned flags, const char* who) {
  if (!flags_ok(flags, who)) return nullptr;
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
  return bank_new(ws.data(), n_expert, who, (flags & NAD_BANK_GENERAL) != 0);
}
}  // namespace

extern "C" void* nad_expert_bank_create(const void* const* weights, int n_expert) {
  return bank_create(weights, n_expert, 0, "nad_expert_bank_create");
}
extern "C" void* nad_expert_bank_create_ex(const void* const* weights, int n_expert, unsigned flags) {
  return bank_create(weights, n_expert, flags, "nad_expert_bank_create_ex");
}
extern "C" void* nad_expert_bank_plan_only(const int32_t* geom, int n_expert) {
  return bank_plan_only(geom, n_expert, 0, "nad_expert_bank_plan_only");
}
extern "C" void* nad_expert_bank_plan_only_ex(const int32_t* geom, int n_expert, unsigned flags) {
  return bank_plan_only(geom, n_expert, flags, "nad_expert_bank_plan_only_ex");
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
  const int64_t v[9] = {b->n_expert, w.bits, w.n, w.k, w.blocksize, w.scale_t, w.asym, b->dev ? 1 : 0, b->kind};
  const int c = std::min(nout, 9);
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
  RoutedGeom g1, g1u, g2;
  if (!ffn_geometry(g1, g1u, g2, *gb, *ub, *db, epi, np, who)) return -1;
  hipStream_t st = static_cast<hipStream_t>(queue);
  float* t = static_cast<float*>(workspace);                                         // [np][fmid]
  float* y = reinterpret_cast<float*>(static_cast<char*>(workspace) + ws_part(np, fmid));  // [np][fout]
  GemvRouted r{};
  r.n_expert = gb->n_expert;
  r.ids = ids;
  r.ids_ld = ids_ld;
  r.ids_col = 0;
  r.slots = top_k;
  // launch 1: t[p] = act1(x_r . G_e^T) * (x_r . U_e^T); a Q6_K pair: t[p] = act1(x_r . G_e^T) alone
  r.bank[0] = gb->dev;
  r.bank[1] = ub->dev;
  r.act = act;
  r.act_ld = lda;
  r.act_per_slot = 0;
  r.out = t;
  r.out_ld = fmid;
  if (run_routed(g1, r, st)) return -1;
  if (g1.kind == kBankQ6k) {  // a Q6_K pair only, launch 1b: t[p] = t[p] * (x_r . U_e^T), in place
    r.bank[0] = ub->dev;
    r.bank[1] = nullptr;
    if (run_routed(g1u, r, st)) return -1;
  }
  // the down launch (2; 3 after a Q6_K pair): y[p] = t[p] . D_e^T
  r.bank[0] = db->dev;
  r.bank[1] = nullptr;
  r.act = t;
  r.act_ld = fmid;
  r.act_per_slot = 1;
  r.out = y;
  r.out_ld = fout;
  if (run_routed(g2, r, st)) return -1;
  // the combine (3; 4 after a Q6_K pair): out[r] = sum_i w[r][i] * y[r * top_k + i], in slot order
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
  RoutedGeom g1, g1u, g2;
  if (!ffn_geometry(g1, g1u, g2, *gb, *ub, *db, kEpiSiluMul, np, who)) return -1;
  const int fout = db->w0.n;
  int64_t v[17];
  int n = 0;
  auto rec = [&](int64_t k, int64_t grid, int64_t threads, int64_t lds) {
    v[n] = k;
    v[n + 1] = grid;
    v[n + 2] = threads;
    v[n + 3] = lds;
    n += 4;
  };
  rec(g1.kernel(), g1.grid, g1.waves * 64, int64_t(g1.lds));
  if (g1.kind == kBankQ6k) rec(g1u.kernel(), g1u.grid, g1u.waves * 64, int64_t(g1u.lds));
  rec(g2.kernel(), g2.grid, g2.waves * 64, int64_t(g2.lds));
  rec(NAD_KERNEL_MOE_COMBINE, int64_t((fout + 255) / 256) * m, 256, 0);
  v[n] = n / 4;
  n++;
  const int c = std::min(nout, n);
  std::memcpy(out, v, sizeof(int64_t) * size_t(c));
  return c;
}

// ------------------------------------------------------------------------------------------------ sorted, grouped
namespace {
// The workspace of the grouped entries (include/neural_amd.h), every part at a multiple of 256 bytes
struct GroupedWs {
  int64_t np = 0;
  int bound32 = 0, kp = 0, fmid = 0, fout = 0;
  size_t offs = 0, perm = 0, src = 0, inv = 0, tiles = 0, x16 = 0, t16 = 0, u16 = 0, y = 0, total = 0;
};
int tile_bound(int64_t np, int n_expert, int bm) { return int(np / bm + std::min<int64_t>(n_expert, np)); }

// up == down == nullptr: the one-matmul form (x16 and y only)
GroupedWs grouped_ws(const NadExpertBank& g, const NadExpertBank* down, int m, int top_k) {
  GroupedWs w;
  w.np = int64_t(m) * top_k;
  w.bound32 = tile_bound(w.np, g.n_expert, 32);
  w.kp = g.kind == kBankQ6k ? g.w0.k : g.w0.nt * gemm7_k_tile(g.w0);  // Q6_K: K is whole superblocks, no padding
  w.fmid = down ? g.w0.n : 0;
  w.fout = down ? down->w0.n : g.w0.n;
  size_t o = 0;
  auto part = [&](uint64_t bytes) {
    const size_t at = o;
    o += size_t(align256(bytes));
    return at;
  };
  const uint64_t np = uint64_t(w.np);
  w.offs = part(uint64_t(g.n_expert + 1) * 4);
  w.perm = part(np * 4);
  w.src = part(np * 4);
  w.inv = part(np * 4);
  w.tiles = part(16 + uint64_t(w.bound32) * 16);
  w.x16 = part(uint64_t(m) * w.kp * 2);
  if (down) {
    w.t16 = part(np * w.fmid * 2);
    w.u16 = part(np * w.fmid * 2);
  }
  w.y = part(np * w.fout * 4);
  w.total = o;
  return w;
}

bool grouped_bank_ok(const NadExpertBank& b, const char* who, const char* role) {
  if (b.g7_ok || b.kind == kBankQ6k) return true;  // a Q6_K bank: woq_q6k_gemm_grouped_kernel, any shape
  if (b.kind == kBankStripe) {
    set_err("%s: the %s bank (int%d, groups of %d%s) does not take the grouped gemm7: it needs int4 groups of 32, 64 or "
            "128 * 2^j, or int2 / int8 groups of 32 or 64 * 2^j, stripe-major, with every q * s in fp16 range",
            who, role, b.w0.bits, b.w0.blocksize, b.w0.kmajor ? ", K-major" : "");
    return false;
  }
  set_err("%s: the %s bank (int%d, groups of %d%s) does not take the grouped gemm7: it needs int4 groups of 64 or 128 * 2^j, or "
          "int2 groups of 64 * 2^j, stripe-major, with every q * s in fp16 range",
          who, role, b.w0.bits, b.w0.blocksize, b.w0.kmajor ? ", K-major" : "");
  return false;
}

// One grouped launch's shape: the tile height is one for the whole call (the sort writes one tile table)
struct GroupedGeom {
  int bm = 0, bound = 0;
};
bool grouped_geometry(GroupedGeom& g, const NadExpertBank& first, const NadExpertBank* const* banks, int nb, int m,
                      int top_k, const GroupedWs& ws, const char* who) {
  const int64_t np = ws.np;
  if (np >= (int64_t(1) << 30) || uint64_t(m) * ws.kp * 2 >= (1ull << 32) ||
      uint64_t(np) * std::max(ws.fmid, 1) * 2 >= (1ull << 32)) {
    set_err("%s: %lld problems of these shapes are more than one launch addresses", who, static_cast<long long>(np));
    return false;
  }
  // the height gemm7 picks for an expert's mean share of the rows; 128, the Q6_K kernel's one height, as soon as a
  // bank of the call is Q6_K (NAD_GEMM7_BM does not apply: gemm7's grouped kernel has a 128 form for the other banks)
  bool any_q6k = false;
  for (int i = 0; i < nb; i++) any_q6k = any_q6k || banks[i]->kind == kBankQ6k;
  g.bm = any_q6k ? 128 : gemm7_tile_height(first.w0, int((np + first.n_expert - 1) / first.n_expert));
  g.bound = tile_bound(np, first.n_expert, g.bm);
  for (int i = 0; i < nb; i++)
    if (int64_t(g.bound) * ((banks[i]->w0.ns + 7) / 8) >= (int64_t(1) << 31)) {
      set_err("%s: %lld problems are more than one launch takes", who, static_cast<long long>(np));
      return false;
    }
  return true;
}

SkinnyWeight bank_view(const NadExpertBank& b, float* out, int ldo) {
  const DeviceWeight& w = b.w0;
  SkinnyWeight v{};
  v.tiles = w.tiles;  // expert 0's; the kernel takes every tile's own from the bank's table
  v.scales = w.scales;
  v.zps = w.zps;
  v.n = w.n;
  v.ns = w.ns;
  v.nt = w.nt;
  v.ng = w.ng;
  v.bs = w.blocksize;
  v.ldo = ldo;
  v.out = out;
  v.f4 = -1;
  return v;
}

struct GroupedPtrs {
  int32_t *offs, *perm, *src, *inv, *ntiles;
  int4* tiles;
  _Float16 *x16, *t16, *u16;
  float* y;
};
GroupedPtrs grouped_ptrs(void* workspace, const GroupedWs& w) {
  char* b = static_cast<char*>(workspace);
  auto i32 = [&](size_t o) { return reinterpret_cast<int32_t*>(b + o); };
  auto h16 = [&](size_t o) { return reinterpret_cast<_Float16*>(b + o); };
  return GroupedPtrs{i32(w.offs), i32(w.perm), i32(w.src), i32(w.inv), i32(w.tiles),
                     reinterpret_cast<int4*>(b + w.tiles + 16), h16(w.x16), h16(w.t16), h16(w.u16),
                     reinterpret_cast<float*>(b + w.y)};
}

// One grouped GEMM of the call.  lds: the dry run's record of the instantiation's dynamic LDS.
struct GroupedOp {
  const NadExpertBank* bank;
  const _Float16* A16;
  int lda16;
  const int32_t* rows;
  int epi;
  _Float16* out16;
  const _Float16* aux16;
  float* out;
};
int run_grouped(const GroupedOp& op, const GroupedGeom& g, const GroupedPtrs& p, hipStream_t st, int64_t* plan4) {
  const DeviceWeight& w = op.bank->w0;
  GemmArgs a{};
  a.K = w.k;
  a.scale_t = w.scale_t;
  a.epi = op.epi;
  a.fold = 1;
  a.ld_aux = w.n;
  a.out16 = op.out16;
  a.ldo16 = w.n;
  a.aux16 = op.aux16;
  a.w = bank_view(*op.bank, op.out, w.n);
  const GemmGrouped gg{op.bank->dev, p.tiles, p.ntiles, op.rows};
  const int grid = g.bound * ((w.ns + 7) / 8);
  if (op.bank->kind == kBankQ6k) {  // 128-row tiles (grouped_geometry), static LDS
    if (plan4) {
      plan4[0] = NAD_KERNEL_Q6K_GEMM_GROUPED;
      plan4[1] = grid;
      plan4[2] = 512;
      plan4[3] = 0;
      return 0;
    }
    a.A = op.A16;
    a.lda = op.lda16;
    a.vec_ok = 1;  // x16 / u16: 256-byte aligned parts of the workspace, rows of K (a multiple of 256) fp16
    return launch(false, "grouped Q6_K gemm kernel", [&] { return launch_q6k_gemm_grouped(a, gg, grid, st); }) ? 0 : -1;
  }
  if (plan4) {
    int lds = 0;
    (void)launch_gemm7_grouped(a, gg, w.bits, g.bm, grid, nullptr, 0, nullptr, &lds);
    plan4[0] = NAD_KERNEL_GEMM7_GROUPED;
    plan4[1] = grid;
    plan4[2] = 512;
    plan4[3] = lds;
    return 0;
  }
  return launch(false, "grouped gemm7 kernel",
                [&] { return launch_gemm7_grouped(a, gg, w.bits, g.bm, grid, op.A16, op.lda16, st, nullptr); })
             ? 0
             : -1;
}

int gate_epi(int dual) { return dual == kEpiSiluMul ? kEpiSilu : kEpiGelu; }

// what the FFN entry and its dry run check alike; fills ws and g
bool grouped_ffn_ok(const NadExpertBank& gb, const NadExpertBank& ub, const NadExpertBank& db, int m, int top_k,
                    GroupedWs& ws, GroupedGeom& g, const char* who) {
  const int fmid = gb.w0.n;
  // ahead of pair_ok, whose "K is not N" would otherwise name the same mismatch less usefully: a Q6_K bank's K is
  // whole superblocks, so the u16 rows it reads as they lie must be
  if (db.kind == kBankQ6k && fmid % 256 != 0) {
    set_err("%s: fmid (%d) is not a whole number of the Q6_K down bank's superblocks (256 deep): the fp16 "
            "intermediate cannot be its operand as it lies", who, fmid);
    return false;
  }
  if (!pair_ok(gb, ub, db, who)) return false;
  if (!grouped_bank_ok(gb, who, "gate") || !grouped_bank_ok(ub, who, "up") || !grouped_bank_ok(db, who, "down"))
    return false;
  const int kt = db.kind == kBankQ6k ? 256 : gemm7_k_tile(db.w0);
  if (db.w0.nt * kt != fmid || fmid % 8 != 0) {
    set_err("%s: fmid (%d) is not a whole number of the down bank's K tiles (%d deep): the fp16 intermediate cannot be "
            "its operand as it lies", who, fmid, kt);
    return false;
  }
  ws = grouped_ws(gb, &db, m, top_k);
  const NadExpertBank* banks[3] = {&gb, &ub, &db};
  return grouped_geometry(g, gb, banks, 3, m, top_k, ws, who);
}
}  // namespace

extern "C" size_t nad_moe_grouped_workspace_size(const void* gate_bank, const void* up_bank, const void* down_bank,
                                                 int m, int top_k) {
  const char* who = "nad_moe_grouped_workspace_size";
  const NadExpertBank* gb = as_bank(gate_bank, who, "gate");
  if (!gb || m <= 0 || top_k <= 0) return 0;
  const NadExpertBank* db = nullptr;
  if (up_bank || down_bank) {
    if (!as_bank(up_bank, who, "up") || !(db = as_bank(down_bank, who, "down"))) return 0;
  }
  return grouped_ws(*gb, db, m, top_k).total;
}

extern "C" int nad_device_moe_ffn_grouped(const void* gate_bank, const void* up_bank, const void* down_bank,
                                          const float* act, const int32_t* ids, int ids_ld, const float* wts,
                                          int wts_ld, int top_k, int epi, void* workspace, float* out, int m, int lda,
                                          int ldo, void* queue) {
  const char* who = "nad_device_moe_ffn_grouped";
  const NadExpertBank* gb = as_bank(gate_bank, who, "gate");
  const NadExpertBank* ub = gb ? as_bank(up_bank, who, "up") : nullptr;
  const NadExpertBank* db = ub ? as_bank(down_bank, who, "down") : nullptr;
  if (!db) return -1;
  if (epi != kEpiSiluMul && epi != kEpiGeluMul) {
    set_err("%s: the epilogue must be SILU_MUL or GELU_MUL", who);
    return -1;
  }
  const int fin = gb->w0.k, fmid = gb->w0.n, fout = db->w0.n;
  if (!act || !ids || !wts || !workspace || !out || m < 0 || top_k < 1 || top_k > ids_ld || top_k > wts_ld ||
      ldo < fout || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
    set_err("%s: bad arguments (m=%d top_k=%d ids_ld=%d wts_ld=%d ldo=%d fout=%d; the workspace 16-B aligned)", who, m,
            top_k, ids_ld, wts_ld, ldo, fout);
    return -1;
  }
  GroupedWs ws;
  GroupedGeom g;
  if (!grouped_ffn_ok(*gb, *ub, *db, std::max(m, 1), top_k, ws, g, who)) return -1;
  if (!rows_ok(act, lda, fin, who) || !launchable(*gb, who) || !launchable(*ub, who) || !launchable(*db, who)) return -1;
  if (m == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(queue);
  const GroupedPtrs p = grouped_ptrs(workspace, ws);
  // launch 1: the sort
  const MoeSortArgs sa{ids, ids_ld, m, top_k, gb->n_expert, g.bm, p.offs, p.perm, p.src, p.inv, p.tiles, p.ntiles};
  if (!launch(false, "moe sort kernel", [&] { return launch_moe_sort(sa, st); })) return -1;
  // launch 2: x -> fp16 [m][kp], zeros past fin
  if (!launch(false, "activation conversion",
              [&] { return launch_cvt_act(act, kActF32, lda, m, fin, ws.kp, nullptr, p.x16, st); }))
    return -1;
  // launches 3-5: t16[q] = act1(x_src[q] . G_e^T); u16[q] = t16[q] * (x_src[q] . U_e^T); y[q] = u16[q] . D_e^T
  if (run_grouped(GroupedOp{gb, p.x16, ws.kp, p.src, gate_epi(epi), p.t16, nullptr, nullptr}, g, p, st, nullptr) ||
      run_grouped(GroupedOp{ub, p.x16, ws.kp, p.src, kEpiSiluMul, p.u16, p.t16, nullptr}, g, p, st, nullptr) ||
      run_grouped(GroupedOp{db, p.u16, fmid, nullptr, kEpiNone, nullptr, nullptr, p.y}, g, p, st, nullptr))
    return -1;
  // launch 6: out[r] = sum_i w[r][i] * y[inv[r * top_k + i]], in slot order
  const MoeGatherArgs c{p.y, fout, p.inv, wts, wts_ld, top_k, out, ldo, m, fout};
  return launch(false, "moe gather kernel", [&] { return launch_moe_gather(c, st); }) ? 0 : -1;
}

extern "C" int nad_device_mul_mat_id_grouped(const void* bank, const float* act, const int32_t* ids, int ids_ld,
                                             int slot, void* workspace, float* out, int m, int lda, int ldo,
                                             void* queue) {
  const char* who = "nad_device_mul_mat_id_grouped";
  const NadExpertBank* b = as_bank(bank, who, "given");
  if (!b) return -1;
  if (!act || !ids || !out || !workspace || m < 0 || slot < 0 || slot >= ids_ld || ldo < b->w0.n ||
      reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
    set_err("%s: bad arguments (m=%d slot=%d ids_ld=%d ldo=%d n=%d; the workspace 16-B aligned)", who, m, slot, ids_ld,
            ldo, b->w0.n);
    return -1;
  }
  if (!grouped_bank_ok(*b, who, "given")) return -1;
  const GroupedWs ws = grouped_ws(*b, nullptr, std::max(m, 1), 1);
  GroupedGeom g;
  if (!grouped_geometry(g, *b, &b, 1, std::max(m, 1), 1, ws, who)) return -1;
  if (!rows_ok(act, lda, b->w0.k, who) || !launchable(*b, who)) return -1;
  if (m == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(queue);
  const GroupedPtrs p = grouped_ptrs(workspace, ws);
  const MoeSortArgs sa{ids + slot, ids_ld, m, 1, b->n_expert, g.bm, p.offs, p.perm, p.src, p.inv, p.tiles, p.ntiles};
  if (!launch(false, "moe sort kernel", [&] { return launch_moe_sort(sa, st); })) return -1;
  if (!launch(false, "activation conversion",
              [&] { return launch_cvt_act(act, kActF32, lda, m, b->w0.k, ws.kp, nullptr, p.x16, st); }))
    return -1;
  if (run_grouped(GroupedOp{b, p.x16, ws.kp, p.src, kEpiNone, nullptr, nullptr, p.y}, g, p, st, nullptr)) return -1;
  const MoeGatherArgs c{p.y, b->w0.n, p.inv, nullptr, 0, 1, out, ldo, m, b->w0.n};
  return launch(false, "moe gather kernel", [&] { return launch_moe_gather(c, st); }) ? 0 : -1;
}

extern "C" int nad_plan_moe_grouped(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k,
                                    int64_t* out, int nout) {
  const char* who = "nad_plan_moe_grouped";
  const NadExpertBank* gb = as_bank(gate_bank, who, "gate");
  if (!gb) return -1;
  const bool ffn = up_bank || down_bank;
  const NadExpertBank* ub = ffn ? as_bank(up_bank, who, "up") : nullptr;
  const NadExpertBank* db = ub ? as_bank(down_bank, who, "down") : nullptr;
  if (ffn && !db) return -1;
  if (!out || nout < 0 || m <= 0 || top_k <= 0 || (!ffn && top_k != 1)) {
    set_err("%s: bad arguments (m=%d top_k=%d; the one-matmul form has top_k = 1)", who, m, top_k);
    return -1;
  }
  GroupedWs ws;
  GroupedGeom g;
  if (ffn) {
    if (!grouped_ffn_ok(*gb, *ub, *db, m, top_k, ws, g, who)) return -1;
  } else {
    if (!grouped_bank_ok(*gb, who, "given")) return -1;
    ws = grouped_ws(*gb, nullptr, m, 1);
    if (!grouped_geometry(g, *gb, &gb, 1, m, 1, ws, who)) return -1;
  }
  const GroupedPtrs p{};
  int64_t v[27] = {};
  int n = 0;
  auto rec = [&](int64_t k, int64_t grid, int64_t threads) {
    v[n] = k;
    v[n + 1] = grid;
    v[n + 2] = threads;
    v[n + 3] = 0;
    n += 4;
  };
  const int fout = ffn ? db->w0.n : gb->w0.n;
  rec(NAD_KERNEL_MOE_SORT, 1, 1024);
  rec(NAD_KERNEL_CVT_ACT, std::min<int64_t>((int64_t(m) * (ws.kp / 8) + 255) / 256, 4096), 256);
  if (ffn) {
    run_grouped(GroupedOp{gb, nullptr, 0, nullptr, kEpiSilu, nullptr, nullptr, nullptr}, g, p, nullptr, v + n);
    n += 4;
    run_grouped(GroupedOp{ub, nullptr, 0, nullptr, kEpiSiluMul, nullptr, nullptr, nullptr}, g, p, nullptr, v + n);
    n += 4;
    run_grouped(GroupedOp{db, nullptr, 0, nullptr, kEpiNone, nullptr, nullptr, nullptr}, g, p, nullptr, v + n);
    n += 4;
  } else {
    run_grouped(GroupedOp{gb, nullptr, 0, nullptr, kEpiNone, nullptr, nullptr, nullptr}, g, p, nullptr, v + n);
    n += 4;
  }
  rec(NAD_KERNEL_MOE_GATHER, int64_t((fout + 255) / 256) * m, 256);
  const int launches = n / 4;
  v[n++] = g.bm;
  v[n++] = g.bound;
  v[n++] = launches;
  const int c = std::min(nout, n);
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
