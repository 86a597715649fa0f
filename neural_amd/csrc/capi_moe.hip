// capi_moe.hip -- Mixtral-style expert FFNs with the routing read on the device (include/neural_amd.h, "routed expert
// matmuls"): the expert bank, nad_device_mul_mat_id (ne_mul_mat_id, ne_layers.c:2384-2462, 7783-7916),
// nad_device_moe_ffn (models/llama/llama.cpp:641-679), the router (llama.cpp:624-638), alone (nad_moe_route) or behind
// the unquantized gate's matmul in the same launch (nad_moe_gate_route, llama.cpp:631), and the dry runs.  A dry run
// (nad_plan_moe, nad_plan_moe_grouped) is the entry's own body run on stand-in arguments under the launch recorder
// (capi_internal.h: dry_run): every launch statement records itself instead of launching (planned), and the record is
// written out.
// The hot path is woq_gemv_m1_routed_kernel, or woq_gemv_routed_kernel for a general bank's int4 g32 / int8 weights
// (woq_gemv.h), or woq_q6k_gemv_routed_kernel for a bank of GGUF Q6_K experts (woq_q6k.hip); the bank's device table
// is the feature's only allocation.  For prefill sizes the sorted, grouped entries (nad_device_moe_ffn_grouped,
// nad_device_mul_mat_id_grouped): moe_sort_kernel (woq_moe.hip), then woq_gemm7_grouped_kernel (woq_gemm7.hip) -- a
// Q6_K bank: woq_q6k_gemm_grouped_kernel -- over every expert's sorted rows.
#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace nad;

namespace {
constexpr uint32_t kBankMagic = 0x4b424e41u;  // "ANBK"
constexpr int kMaxExperts = 256;
constexpr size_t kLdsMax = 160 << 10;  // a workgroup's LDS: 160 KiB

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

// One routed launch.  What a bank kind takes is here and nowhere else: its row of kRouted, its case of routed_geometry
// and its case of run_routed.
constexpr struct {
  int kernel;
  const char* what;
} kRouted[3] = {{NAD_KERNEL_GEMV_ROUTED, "routed gemv kernel"},  // by kBank*
                {NAD_KERNEL_GEMV_ROUTED_GENERAL, "routed gemv kernel"},
                {NAD_KERNEL_Q6K_GEMV_ROUTED, "routed Q6_K gemv kernel"}};

struct RoutedGeom {
  const NadExpertBank* bank = nullptr;  // the kernel of its kind serves the launch
  int waves = 0, wpp = 0, grid = 0;     // wpp: the workgroups per problem
  size_t lds = 0;
  GemvArgs a{};          // kBankLean, kBankStripe: one problem as its own decode launch prepares it, epilogue included
  int epi = kEpiNone;    // kBankQ6k: the single-weight epilogue of the launch -- none, the gate activation, or
  bool aux_out = false;  //   kEpiSiluMul with the problem's own output row as the multiplier (aux_out)
};

// up == nullptr: one weight per problem; else the {gate, up} pair under the dual epilogue epi (a Q6_K pair runs as two
// launches of one weight, as the dense Q6_K FFN does).  Workgroups per problem as nad_batch_create deals them: the
// chip's CUs over the problems, at least one, more where one problem's share of the stripes would not fit a
// workgroup's partial-sum slots.
bool routed_geometry(RoutedGeom& g, const NadExpertBank& w, const NadExpertBank* up, int epi, int64_t nprob,
                     const char* who, bool aux_out = false) {
  g.bank = &w;
  switch (w.kind) {
    case kBankQ6k: {
      if (up) {
        set_err("%s: a Q6_K pair runs as two launches", who);  // the callers do; not reached
        return false;
      }
      Q6kRoutedGeom q{};
      g.epi = epi;
      g.aux_out = aux_out;
      if (!q6k_routed_geometry(w.w0.k, w.w0.ns, nprob, device_cus(), &q)) {
        if (q.lds > kLdsMax)
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
    default: {  // kBankLean, kBankStripe
      const bool stripe = w.kind == kBankStripe;
      const DeviceWeight* ws[2] = {&w.w0, up ? &up->w0 : nullptr};
      if (!(stripe ? prepare_general_problem : prepare_m1_problem)(g.a, g.waves, ws, up ? 2 : 1, epi)) {
        set_err("%s: this weight geometry does not take the %s", who, stripe ? "routed stripe stream" : "M = 1 GEMV");
        return false;
      }
      const int units = g.a.units;
      int wpp = int(std::max<int64_t>(1, std::min<int64_t>(units, device_cus() / nprob)));
      for (;; wpp++) {
        g.a.u_q = units / wpp;
        g.a.u_r = units % wpp;
        g.lds = gemv_lds_layout(g.a, w.w0.bits, g.waves, wpp);
        if (g.lds <= kLdsMax || wpp >= units) break;
      }
      if (g.lds > kLdsMax) {
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
  }
}

bool run_routed(const RoutedGeom& g, GemvRouted r, hipStream_t st) {
  r.wpp = g.wpp;
  const DeviceWeight& w = g.bank->w0;
  const auto& kind = kRouted[g.bank->kind];
  return launch(planned(kind.kernel, {g.grid, g.waves * 64}, g.lds), kind.what,
                [&] {
                  switch (g.bank->kind) {
                    case kBankQ6k: {
                      GemmArgs a{};  // one problem: M = 1; the kernel fills A, the weight's pointers, the output row and aux
                      a.M = 1;
                      a.K = w.k;
                      a.lda = r.act_ld;
                      a.scale_t = w.scale_t;
                      a.epi = g.epi;
                      a.vec_ok = 1;  // rows_ok: a 16-B base and lda % 4 == 0 (the FFN's t rows: K = fmid, a multiple of 256)
                      a.w = bank_view(*g.bank, nullptr, w.n);
                      return launch_q6k_gemv_routed(a, r, g.aux_out, Q6kRoutedGeom{g.wpp, g.grid, g.waves, g.lds}, st);
                    }
                    case kBankStripe:
                      return launch_gemv_routed_general(g.a, r, w.bits, g.waves, g.grid, g.lds, st);
                    default:
                      return launch_gemv_routed(g.a, r, w.bits, g.waves, g.grid, g.lds, st);
                  }
                });
}

bool rows_ok(const float* act, int lda, int k, const char* who) {
  if (lda % 4 != 0 || lda < k || reinterpret_cast<uintptr_t>(act) % 16 != 0) {
    set_err("%s: the activation rows need a 16-B aligned base and lda %% 4 == 0, lda >= k (lda %d, k %d)", who, lda, k);
    return false;
  }
  return true;
}

bool launchable(const NadExpertBank& b, const char* who) {
  if (b.dev || planning()) return true;  // a dry run launches nothing (as_weight, capi.hip)
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

// The routed launches of one FFN: g1 the {gate, up} pair under the dual epilogue -- or, for a Q6_K pair, the gate under
// its activation alone and g1u the up weight times the gate's result in place -- and g2 the down weight.  Each launch
// is served by its own bank's kernel.
bool ffn_geometry(RoutedGeom& g1, RoutedGeom& g1u, RoutedGeom& g2, const NadExpertBank& gb, const NadExpertBank& ub,
                  const NadExpertBank& db, int epi, int64_t np, const char* who) {
  if (gb.kind == kBankQ6k) {
    if (!routed_geometry(g1, gb, nullptr, Epi::gate_of(epi).kind, np, who) ||
        !routed_geometry(g1u, ub, nullptr, kEpiSiluMul, np, who, true))
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

// what both ways to make a bank check first: the flags, then the list (weights or geometries) and its length
bool bank_args_ok(const void* list, int n_expert, unsigned flags, const char* who) {
  if ((flags & ~NAD_BANK_GENERAL) != 0)
    set_err("%s: unknown flags 0x%x (NAD_BANK_GENERAL is the only one)", who, flags);
  else if (!list || n_expert < 1 || n_expert > kMaxExperts)
    set_err("%s: need 1..%d experts (got %d)", who, kMaxExperts, n_expert);
  else
    return true;
  return false;
}

void* bank_create(const void* const* weights, int n_expert, unsigned flags, const char* who) {
  if (!bank_args_ok(weights, n_expert, flags, who)) return nullptr;
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
  if (!bank_args_ok(geom, n_expert, flags, who)) return nullptr;
  std::vector<DeviceWeight> store(static_cast<size_t>(n_expert));
  std::vector<const DeviceWeight*> ws(static_cast<size_t>(n_expert));
  for (int i = 0; i < n_expert; i++) {
    const int32_t* g = geom + 6 * i;
    const int bits = g[0], n = g[1], k = g[2], asym = g[5];
    DeviceWeight& w = store[size_t(i)];
    if (!plan_geometry_ok(bits, n, k, g[4])) {
      set_err("%s: expert %d: bad geometry (bits=%d n=%d k=%d scale=%d)", who, i, bits, n, k, g[4]);
      return nullptr;
    }
    plan_weight_geometry(w, bits, n, k, g[3] <= 0 ? k : g[3], g[4], asym, 0);
    plan_weight_assign(w, 0);  // every expert on slot 0: only the bank's geometry is read
    ws[size_t(i)] = &w;
  }
  return bank_new(ws.data(), n_expert, who, (flags & NAD_BANK_GENERAL) != 0);
}

// ------------------------------------------------------------------------------------------------ the FFN entries
// What nad_device_moe_ffn and nad_device_moe_ffn_grouped take, and the checks they share
struct FfnCall {
  const void *gate_bank, *up_bank, *down_bank;
  const float* act;
  const int32_t* ids;
  int ids_ld;
  const float* wts;
  int wts_ld, top_k, epi;
  void* workspace;
  float* out;
  int m, lda, ldo;
  void* queue;
};
struct FfnBanks {
  const NadExpertBank *g = nullptr, *u = nullptr, *d = nullptr;
};
bool ffn_banks(FfnBanks& b, const void* gate, const void* up, const void* down, const char* who) {
  b.g = as_bank(gate, who, "gate");
  b.u = b.g ? as_bank(up, who, "up") : nullptr;
  b.d = b.u ? as_bank(down, who, "down") : nullptr;
  return b.d != nullptr;
}
bool ffn_banks_epi(FfnBanks& b, const FfnCall& c, const char* who) {
  if (!ffn_banks(b, c.gate_bank, c.up_bank, c.down_bank, who)) return false;
  if (c.epi == kEpiSiluMul || c.epi == kEpiGeluMul) return true;
  set_err("%s: the epilogue must be SILU_MUL or GELU_MUL", who);
  return false;
}
bool ffn_args_ok(const FfnCall& c, int fout, const char* who) {
  if (c.act && c.ids && c.wts && c.workspace && c.out && c.m >= 0 && c.top_k >= 1 && c.top_k <= c.ids_ld &&
      c.top_k <= c.wts_ld && c.ldo >= fout && reinterpret_cast<uintptr_t>(c.workspace) % 16 == 0)
    return true;
  set_err("%s: bad arguments (m=%d top_k=%d ids_ld=%d wts_ld=%d ldo=%d fout=%d; the workspace 16-B aligned)", who, c.m,
          c.top_k, c.ids_ld, c.wts_ld, c.ldo, fout);
  return false;
}

int moe_ffn(const FfnCall& c, const char* who) {
  FfnBanks b;
  if (!ffn_banks_epi(b, c, who) || !pair_ok(*b.g, *b.u, *b.d, who)) return -1;
  const int fin = b.g->w0.k, fmid = b.g->w0.n, fout = b.d->w0.n, m = c.m, top_k = c.top_k;
  if (!ffn_args_ok(c, fout, who)) return -1;
  if (!rows_ok(c.act, c.lda, fin, who) || !launchable(*b.g, who) || !launchable(*b.u, who) || !launchable(*b.d, who))
    return -1;
  if (m == 0) return 0;
  const int64_t np = int64_t(m) * top_k;
  RoutedGeom g1, g1u, g2;
  if (!ffn_geometry(g1, g1u, g2, *b.g, *b.u, *b.d, c.epi, np, who)) return -1;
  hipStream_t st = static_cast<hipStream_t>(c.queue);
  float* t = static_cast<float*>(c.workspace);                                         // [np][fmid]
  float* y = reinterpret_cast<float*>(static_cast<char*>(c.workspace) + ws_part(np, fmid));  // [np][fout]
  // launch 1: t[p] = act1(x_r . G_e^T) * (x_r . U_e^T); a Q6_K pair: t[p] = act1(x_r . G_e^T) alone.  wpp (0 here) is
  // the launch's own; ids from column 0, top_k slots per row, one activation row per row
  GemvRouted r{{b.g->dev, b.u->dev}, b.g->n_expert, 0, c.ids, c.ids_ld, 0, top_k, 0, c.act, c.lda, t, fmid};
  if (!run_routed(g1, r, st)) return -1;
  if (b.g->kind == kBankQ6k) {  // a Q6_K pair only, launch 1b: t[p] = t[p] * (x_r . U_e^T), in place
    r.bank[0] = b.u->dev;
    r.bank[1] = nullptr;
    if (!run_routed(g1u, r, st)) return -1;
  }
  // the down launch (2; 3 after a Q6_K pair): y[p] = t[p] . D_e^T, one activation row per problem
  r = GemvRouted{{b.d->dev, nullptr}, b.g->n_expert, 0, c.ids, c.ids_ld, 0, top_k, 1, t, fmid, y, fout};
  if (!run_routed(g2, r, st)) return -1;
  // the combine (3; 4 after a Q6_K pair): out[r] = sum_i w[r][i] * y[r * top_k + i], in slot order
  const MoeCombineArgs ca{y, fout, c.wts, c.wts_ld, top_k, c.out, c.ldo, m, fout};
  return launch(planned(NAD_KERNEL_MOE_COMBINE, moe_combine_shape(m, fout)), "moe combine kernel",
                [&] { return launch_moe_combine(ca, st); })
             ? 0
             : -1;
}

// ------------------------------------------------------------------------------------------------ sorted, grouped
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
  set_err("%s: the %s bank (int%d, groups of %d%s) does not take the grouped gemm7: it needs %s, stripe-major, with every "
          "q * s in fp16 range", who, role, b.w0.bits, b.w0.blocksize, b.w0.kmajor ? ", K-major" : "",
          b.kind == kBankStripe ? "int4 groups of 32, 64 or 128 * 2^j, or int2 / int8 groups of 32 or 64 * 2^j"
                                : "int4 groups of 64 or 128 * 2^j, or int2 groups of 64 * 2^j");
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

// One grouped GEMM of the call
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
bool run_grouped(const GroupedOp& op, const GroupedGeom& g, const GroupedPtrs& p, hipStream_t st) {
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
  const LaunchShape shape{g.bound * ((w.ns + 7) / 8), 512};
  if (op.bank->kind == kBankQ6k) {  // 128-row tiles (grouped_geometry), static LDS
    a.A = op.A16;
    a.lda = op.lda16;
    a.vec_ok = 1;  // x16 / u16: 256-byte aligned parts of the workspace, rows of K (a multiple of 256) fp16
    return launch(planned(NAD_KERNEL_Q6K_GEMM_GROUPED, shape), "grouped Q6_K gemm kernel",
                  [&] { return launch_q6k_gemm_grouped(a, gg, shape.grid, st); });
  }
  // a dry run records the dynamic LDS of the instantiation the launcher's own ladder picks
  auto lds = [&] {
    int v = 0;
    (void)launch_gemm7_grouped(a, gg, w.bits, g.bm, shape.grid, nullptr, 0, nullptr, &v);
    return size_t(v);
  };
  return launch(planning() && planned(NAD_KERNEL_GEMM7_GROUPED, shape, lds()), "grouped gemm7 kernel",
                [&] { return launch_gemm7_grouped(a, gg, w.bits, g.bm, shape.grid, op.A16, op.lda16, st, nullptr); });
}

// The first two launches of a grouped call: the sort of the m * top_k problems at ids, then x -> fp16 [m][kp], zeros
// past the bank's K
bool grouped_begin(const NadExpertBank& b, const int32_t* ids, int ids_ld, int top_k, const float* act, int lda, int m,
                   const GroupedWs& ws, const GroupedGeom& g, const GroupedPtrs& p, hipStream_t st) {
  const MoeSortArgs sa{ids, ids_ld, m, top_k, b.n_expert, g.bm, p.offs, p.perm, p.src, p.inv, p.tiles, p.ntiles};
  return launch(planned(NAD_KERNEL_MOE_SORT, moe_sort_shape()), "moe sort kernel",
                [&] { return launch_moe_sort(sa, st); }) &&
         launch(planned(NAD_KERNEL_CVT_ACT, cvt_act_shape(m, ws.kp)), "activation conversion",
                [&] { return launch_cvt_act(act, kActF32, lda, m, b.w0.k, ws.kp, nullptr, p.x16, st); });
}
// ... and the last: out[r] = sum_i w[r][i] * y[inv[r * top_k + i]], in slot order (wts null, top_k = 1: out[r] = y[inv[r]])
bool grouped_end(const GroupedPtrs& p, const float* wts, int wts_ld, int top_k, float* out, int ldo, int m, int fout,
                hipStream_t st) {
  const MoeGatherArgs c{p.y, fout, p.inv, wts, wts_ld, top_k, out, ldo, m, fout};
  return launch(planned(NAD_KERNEL_MOE_GATHER, moe_combine_shape(m, fout)), "moe gather kernel",
                [&] { return launch_moe_gather(c, st); });
}

// what the FFN entry checks of its banks; fills ws and g
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

int moe_ffn_grouped(const FfnCall& c, GroupedGeom& g, const char* who) {
  FfnBanks b;
  if (!ffn_banks_epi(b, c, who)) return -1;
  const int fin = b.g->w0.k, fmid = b.g->w0.n, fout = b.d->w0.n, m = c.m, top_k = c.top_k;
  if (!ffn_args_ok(c, fout, who)) return -1;
  GroupedWs ws;
  if (!grouped_ffn_ok(*b.g, *b.u, *b.d, std::max(m, 1), top_k, ws, g, who)) return -1;
  if (!rows_ok(c.act, c.lda, fin, who) || !launchable(*b.g, who) || !launchable(*b.u, who) || !launchable(*b.d, who))
    return -1;
  if (m == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(c.queue);
  const GroupedPtrs p = grouped_ptrs(c.workspace, ws);
  // launches 1 and 2: the sort; x -> fp16
  if (!grouped_begin(*b.g, c.ids, c.ids_ld, top_k, c.act, c.lda, m, ws, g, p, st)) return -1;
  // launches 3-5: t16[q] = act1(x_src[q] . G_e^T); u16[q] = t16[q] * (x_src[q] . U_e^T); y[q] = u16[q] . D_e^T
  if (!run_grouped(GroupedOp{b.g, p.x16, ws.kp, p.src, Epi::gate_of(c.epi).kind, p.t16, nullptr, nullptr}, g, p, st) ||
      !run_grouped(GroupedOp{b.u, p.x16, ws.kp, p.src, kEpiSiluMul, p.u16, p.t16, nullptr}, g, p, st) ||
      !run_grouped(GroupedOp{b.d, p.u16, fmid, nullptr, kEpiNone, nullptr, nullptr, p.y}, g, p, st))
    return -1;
  // launch 6: the slot sum over the sorted rows
  return grouped_end(p, c.wts, c.wts_ld, top_k, c.out, c.ldo, m, fout, st) ? 0 : -1;
}

int mul_mat_id_grouped(const void* bank, const float* act, const int32_t* ids, int ids_ld, int slot, void* workspace,
                       float* out, int m, int lda, int ldo, void* queue, GroupedGeom& g, const char* who) {
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
  if (!grouped_geometry(g, *b, &b, 1, std::max(m, 1), 1, ws, who)) return -1;
  if (!rows_ok(act, lda, b->w0.k, who) || !launchable(*b, who)) return -1;
  if (m == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(queue);
  const GroupedPtrs p = grouped_ptrs(workspace, ws);
  if (!grouped_begin(*b, ids + slot, ids_ld, 1, act, lda, m, ws, g, p, st)) return -1;
  if (!run_grouped(GroupedOp{b, p.x16, ws.kp, p.src, kEpiNone, nullptr, nullptr, p.y}, g, p, st)) return -1;
  return grouped_end(p, nullptr, 0, 1, out, ldo, m, b->w0.n, st) ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------ the dry runs
// Stand-in arguments (capi_internal.h: stand_in): rows of K rounded up to a multiple of 4 floats, ids and weights of
// top_k columns, the output of the down bank's N
int padded4(int k) { return (k + 3) / 4 * 4; }
FfnCall stand_in_call(const FfnBanks& b, int m, int top_k) {
  return FfnCall{b.g, b.u, b.d, stand_in<const float>(kStandAct), stand_in<const int32_t>(kStandMoeIds), top_k,
                 stand_in<const float>(kStandMoeWts), top_k, top_k, kEpiSiluMul, stand_in<void>(kStandMoeWorkspace),
                 stand_in<float>(kStandMoeOut), m, padded4(b.g->w0.k), b.d->w0.n, nullptr};
}

// The routed dry runs' writer (capi_internal.h: dry_run): four values per launch (kernel code, grid, threads, dynamic
// LDS bytes), the ntail values body left in tail, the launch count
template <class F>
int dry_run_list(int64_t* out, int nout, const int64_t* tail, int ntail, F&& body) {
  return dry_run(body, [&](const NadPlan& plan) {
    int64_t v[4 * NadPlan::kListMax + 3];
    int n = 4 * plan.listed();
    std::memcpy(v, plan.list, sizeof(int64_t) * size_t(n));
    for (int i = 0; i < ntail; i++) v[n++] = tail[i];
    v[n++] = plan.listed();
    const int c = std::min(nout, n);
    std::memcpy(out, v, sizeof(int64_t) * size_t(c));
    return c;
  });
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
  const GemvRouted r{{b->dev, nullptr}, b->n_expert, 0, ids, ids_ld, slot, 1, 0, act, lda, out, ldo};  // wpp: the launch's
  return run_routed(g, r, static_cast<hipStream_t>(queue)) ? 0 : -1;
}

extern "C" size_t nad_moe_workspace_size(int m, int top_k, int fmid, int fout) {
  if (m <= 0 || top_k <= 0 || fmid <= 0 || fout <= 0) return 0;
  const int64_t p = int64_t(m) * top_k;
  return ws_part(p, fmid) + ws_part(p, fout);
}

extern "C" int nad_device_moe_ffn(const void* gate_bank, const void* up_bank, const void* down_bank, const float* act,
                                  const int32_t* ids, int ids_ld, const float* wts, int wts_ld, int top_k, int epi,
                                  void* workspace, float* out, int m, int lda, int ldo, void* queue) {
  return moe_ffn(FfnCall{gate_bank, up_bank, down_bank, act, ids, ids_ld, wts, wts_ld, top_k, epi, workspace, out, m,
                         lda, ldo, queue},
                 "nad_device_moe_ffn");
}

extern "C" int nad_plan_moe(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k,
                            int64_t* out, int nout) {
  const char* who = "nad_plan_moe";
  FfnBanks b;
  if (!ffn_banks(b, gate_bank, up_bank, down_bank, who)) return -1;
  if (!out || nout < 0 || m <= 0 || top_k <= 0) {
    set_err("%s: bad arguments (m=%d top_k=%d)", who, m, top_k);
    return -1;
  }
  return dry_run_list(out, nout, nullptr, 0, [&] { return moe_ffn(stand_in_call(b, m, top_k), who); });
}

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
  GroupedGeom g;
  return moe_ffn_grouped(FfnCall{gate_bank, up_bank, down_bank, act, ids, ids_ld, wts, wts_ld, top_k, epi, workspace,
                                 out, m, lda, ldo, queue},
                         g, "nad_device_moe_ffn_grouped");
}

extern "C" int nad_device_mul_mat_id_grouped(const void* bank, const float* act, const int32_t* ids, int ids_ld,
                                             int slot, void* workspace, float* out, int m, int lda, int ldo,
                                             void* queue) {
  GroupedGeom g;
  return mul_mat_id_grouped(bank, act, ids, ids_ld, slot, workspace, out, m, lda, ldo, queue, g,
                            "nad_device_mul_mat_id_grouped");
}

extern "C" int nad_plan_moe_grouped(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k,
                                    int64_t* out, int nout) {
  const char* who = "nad_plan_moe_grouped";
  const bool ffn = up_bank || down_bank;
  FfnBanks b;
  if (ffn ? !ffn_banks(b, gate_bank, up_bank, down_bank, who) : !(b.g = as_bank(gate_bank, who, "gate"))) return -1;
  if (!out || nout < 0 || m <= 0 || top_k <= 0 || (!ffn && top_k != 1)) {
    set_err("%s: bad arguments (m=%d top_k=%d; the one-matmul form has top_k = 1)", who, m, top_k);
    return -1;
  }
  int64_t geom[2] = {0, 0};  // the tile height and the tile bound, from the body's own GroupedGeom
  return dry_run_list(out, nout, geom, 2, [&] {
    GroupedGeom g;
    const int rc = ffn ? moe_ffn_grouped(stand_in_call(b, m, top_k), g, who)
                       : mul_mat_id_grouped(b.g, stand_in<const float>(kStandAct), stand_in<const int32_t>(kStandMoeIds),
                                            1, 0, stand_in<void>(kStandMoeWorkspace), stand_in<float>(kStandMoeOut), m,
                                            padded4(b.g->w0.k), b.g->w0.n, nullptr, g, who);
    geom[0] = g.bm;
    geom[1] = g.bound;
    return rc;
  });
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

// ------------------------------------------------------------------------------------------------ gate matmul + route
namespace {
// nad_moe_gate_route's refusals, each naming its argument, then the one launch (recorded in a dry run)
int moe_gate_route(const MoeGateRouteArgs& a, hipStream_t st, const char* who) {
  const auto misaligned = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 != 0; };
  if (!a.act || !a.gate || !a.ids || !a.wts)
    set_err("%s: %s is null", who, !a.act ? "act" : !a.gate ? "gate" : !a.ids ? "ids" : "wts");
  else if (a.m < 0)
    set_err("%s: m (%d) is negative", who, a.m);
  else if (a.k < 4 || a.k % 4 != 0)
    set_err("%s: k (%d) must be a multiple of 4, at least 4", who, a.k);
  else if (a.n_expert < 1 || a.n_expert > 64)
    set_err("%s: n_expert (%d) is outside 1..64", who, a.n_expert);
  else if (a.top_k < 1 || a.top_k > a.n_expert)
    set_err("%s: top_k (%d) is outside 1..n_expert (%d)", who, a.top_k, a.n_expert);
  else if (a.gate_t != kActF32 && a.gate_t != kActF16 && a.gate_t != kActBF16)
    set_err("%s: gate_dtype (%d) is none of NAD_ACT_F32, NAD_ACT_F16, NAD_ACT_BF16", who, a.gate_t);
  else if (a.lda < a.k || a.lda % 4 != 0)
    set_err("%s: lda (%d) must be a multiple of 4, at least k (%d)", who, a.lda, a.k);
  else if (a.ldw < a.k || a.ldw % 4 != 0)
    set_err("%s: ldw (%d) must be a multiple of 4, at least k (%d)", who, a.ldw, a.k);
  else if (a.ids_ld < a.top_k)
    set_err("%s: ids_ld (%d) is below top_k (%d)", who, a.ids_ld, a.top_k);
  else if (a.wts_ld < a.top_k)
    set_err("%s: wts_ld (%d) is below top_k (%d)", who, a.wts_ld, a.top_k);
  else if (a.logits && a.logits_ld < a.n_expert)
    set_err("%s: logits_ld (%d) is below n_expert (%d)", who, a.logits_ld, a.n_expert);
  else if (misaligned(a.act) || misaligned(a.gate))
    set_err("%s: %s is not 16-byte aligned", who, misaligned(a.act) ? "act" : "gate");
  else if (a.m == 0)
    return 0;
  else
    return launch(planned(NAD_KERNEL_MOE_GATE_ROUTE, moe_gate_route_shape(a.m), moe_gate_route_lds(a.n_expert)),
                  "moe gate route kernel", [&] { return launch_moe_gate_route(a, st); })
               ? 0
               : -1;
  return -1;
}
}  // namespace

extern "C" int nad_moe_gate_route(const float* act, int lda, const void* gate, int gate_dtype, int ldw, int m, int k,
                                  int n_expert, int top_k, int32_t* ids, int ids_ld, float* wts, int wts_ld,
                                  float* logits, int logits_ld, void* queue) {
  return moe_gate_route(MoeGateRouteArgs{act, lda, gate, gate_dtype, ldw, m, k, n_expert, top_k, ids, ids_ld, wts,
                                         wts_ld, logits, logits_ld},
                        static_cast<hipStream_t>(queue), "nad_moe_gate_route");
}

extern "C" int nad_plan_moe_gate_route(int m, int k, int n_expert, int top_k, int gate_dtype, int64_t* out, int nout) {
  const char* who = "nad_plan_moe_gate_route";
  if (!out || nout < 0 || m <= 0) {
    set_err("%s: bad arguments (m=%d: a dry run needs m >= 1)", who, m);
    return -1;
  }
  // stand-ins: contiguous rows of k, no logits output (it changes nothing about the launch)
  const MoeGateRouteArgs a{stand_in<const float>(kStandAct), k, stand_in<const void>(kStandWeight), gate_dtype, k, m, k,
                           n_expert, top_k, stand_in<int32_t>(kStandMoeIds), top_k, stand_in<float>(kStandMoeWts), top_k,
                           nullptr, 0};
  return dry_run_list(out, nout, nullptr, 0, [&] { return moe_gate_route(a, nullptr, who); });
}
