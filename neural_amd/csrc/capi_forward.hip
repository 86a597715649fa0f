// capi_forward.hip -- the device forwards (include/neural_amd.h): kernel choice and launch geometry for decode
// (stripe-stream GEMV, skinny), mid-M and prefill (gemm2/3/4/7), the int8 arithmetic and the GGUF min-term pass; then
// nad_device_forward, the fused QKV / FFN entries and the batch API (their dry runs: capi_plan.hip).  A call travels
// through the internals as an Act, an Epi and an Out (capi_internal.h).
#include <algorithm>
#include <climits>
#include <vector>

#include "capi_internal.h"

using namespace nad;

// ------------------------------------------------------------------------------------------------ call plumbing
// nw weights on one activation, each with its output
struct Weights {
  int nw;
  const DeviceWeight* const* ws;
  float* const* outs;
  const int* ldos;
  const DeviceWeight& operator[](int i) const { return *ws[i]; }
  Weights sub(int i, int n) const { return Weights{n, ws + i, outs + i, ldos + i}; }
};
// a single weight and output in the nw = 1 form
struct One {
  const DeviceWeight* w;
  float* out;
  int ldo;
  One(const DeviceWeight& w_, const Out& o) : w(&w_), out(o.p), ldo(o.ld) {}
  operator Weights() const { return Weights{1, &w, &out, &ldo}; }
};

static SkinnyWeight view(const DeviceWeight& w, float* out, int ldo, const Epi& e = Epi{}) {
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
  v.bias = e.bias;
  v.bias_ld = e.bias_ld;
  v.f4 = w.f4kind;
  return v;
}

// the fields every kernel-argument family shares (SkinnyArgs, GemmArgs, GemvArgs, I8Args, MinTermArgs::g)
template <class Args>
static void fill_act(Args& a, const Act& x) {
  a.A = x.p;
  a.lda = x.ld;
  a.M = x.m;
  a.K = x.k;
}
template <class Args>
static void fill_epi(Args& a, const Epi& e) {
  a.epi = e.kind;
  a.res = e.res;
  a.ld_res = e.ld_res;
  a.aux = e.aux;
  a.ld_aux = e.ld_aux;
}
static void fill_h16(GemmArgs& a, const Half16* h16) {
  if (!h16) return;
  a.out16 = h16->out;
  a.ldo16 = h16->ldo;
  a.aux16 = h16->aux;
}

static bool vec_aligned(const Act& x) {
  const int esz = x.t == kActF32 ? 4 : 2;
  return (reinterpret_cast<uintptr_t>(x.p) % 16 == 0) && ((size_t(x.ld) * esz) % 16 == 0);
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

int device_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

// ------------------------------------------------------------------------------------------------ decode: GEMV, skinny
// Fill the GemvArgs, waves and grid of one decode op on the persistent stripe-stream GEMV (woq_gemv.h); returns 1
// when that kernel handles it, 0 when not eligible: M <= 16, the staged activations fit LDS, the group size tiles the K
// tile, and all weights share one act-order LUT.
static int prepare_gemv(GemvArgs& a, int& waves, int& grid, const Act& x, const Weights& W, const Epi& e,
                        bool single_op = true) {
  const DeviceWeight& w0 = W[0];
  for (int i = 1; i < W.nw; i++)
    if (W[i].shuffle != w0.shuffle || W[i].nt != w0.nt || W[i].ng != w0.ng || W[i].bits != w0.bits ||
        W[i].asym != w0.asym || W[i].scale_t != w0.scale_t || W[i].blocksize != w0.blocksize || W[i].kmajor)
      return 0;
  if (w0.kmajor) return 0;  // the stream stages each stripe's scale block: stripe-major layout only
  for (int i = 0; i < W.nw; i++)
    if (is_q6k(W[i])) return 0;  // a layout of its own (forward_q6k); run_skinny refuses it by name
  for (int i = 0; i < W.nw; i++)
    if (W[i].f4kind >= 0) return 0;  // NFloat weights: LUT dequant lives in the skinny kernel
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(w0.bits, w0.nt, w0.ng, w0.blocksize, &tpg);
  if (gpt == 0 || (gpt >= 4 && w0.asym)) return 0;
  a = GemvArgs{};
  fill_act(a, x);
  fill_epi(a, e);
  a.act_t = x.t;
  a.dual = e.is_dual() ? 1 : 0;
  a.nt = w0.nt;
  a.ng = w0.ng;
  a.bs = w0.blocksize;
  a.tpg_shift = tpg == 0 ? 31 : __builtin_ctz(unsigned(tpg));
  a.scale_t = w0.scale_t;
  a.asym = w0.asym;
  a.shuffle = w0.shuffle;
  a.a_fast = (vec_aligned(x) && w0.shuffle == nullptr && x.k % 8 == 0) ? 1 : 0;
  int stripes = 0;
  for (int i = 0; i < 3; i++) a.stripe_base[i] = INT_MAX;
  for (int i = 0; i < W.nw; i++) {
    a.w[i] = view(W[i], W.outs[i], W.ldos[i], e);
    a.stripe_base[i] = stripes;
    stripes += W[i].ns;
  }
  for (int i = W.nw; i < 3; i++) a.w[i] = a.w[0];
  a.units = a.dual ? w0.ns : stripes;
  const Knobs& kn = knobs();
  grid = std::max(1, std::min(a.units, device_cus()));
  if (kn.gemv_grid > 0) grid = std::min(a.units, kn.gemv_grid);  // tests / tuning
  waves = gemv_waves(w0.bits, w0.nt, w0.ng, w0.blocksize);
  if (kn.gemv_waves > 0) waves = std::min(gpt > 1 ? 8 : 16, kn.gemv_waves);
  a.dq_mask = 0x000F000Fu;
  a.dq_magic = 0x64006400u;
  a.m1_nst = kn.gemv_nst;
  a.m1_spec = kn.gemv_m1_spec ? 1 | (kn.gemv_ahead ? kM1SpecAhead : 0) : 0;
  a.u_q = a.units / grid;
  a.u_r = a.units % grid;
  a.lean = kn.gemv_lean;
  // M = 1 single-op launches may stream 2-tile K-slices, one per wave (up to 16 waves); fused launches keep 4-tile ones
  if (single_op)
    gemv_lean_slices(a, w0.bits, &waves, kn.gemv_waves > 0 ? 4 : 2);
  if (kn.gemv_spw != 4 && a.lean_spw == 4) a.lean_spw = 2;  // A/B: long K back on the general stream kernel
  if (gemv_lds_layout(a, w0.bits, waves, grid) > 160 * 1024) return 0;
  // buffer-resource offsets are 32-bit: every tile array, scale array and the activations must stay below 2 GiB
  const int esz = x.t == kActF32 ? 4 : 2;
  if (uint64_t(x.m) * x.ld * esz >= (1ull << 30)) return 0;
  for (int i = 0; i < W.nw; i++)
    if (uint64_t(W[i].ns) * W[i].nt * 1024 >= (1ull << 30)) return 0;
  return 1;
}

// One M = 1 fp32 problem on ws[0] (nw = 1), or on the {gate, up} pair ws[0], ws[1] with a dual epilogue (nw = 2), as
// its own decode launch prepares it (capi_moe.hip: the routed launch runs every problem at exactly this geometry).  The
// pointers in `a` are placeholders.
static bool prepare_one_problem(GemvArgs& a, int& waves, const DeviceWeight* const* ws, int nw, int epi) {
  const float* act = stand_in<const float>(kStandAct);
  float* y = stand_in<float>(kStandOut);
  float* outs[2] = {y, y};
  const int ldos[2] = {ws[0]->n, ws[0]->n};
  Epi e;
  e.kind = epi;
  int grid = 0;
  return prepare_gemv(a, waves, grid, Act{act, kActF32, ws[0]->k, 1, ws[0]->k}, Weights{nw, ws, outs, ldos}, e);
}
bool prepare_m1_problem(GemvArgs& a, int& waves, const DeviceWeight* const* ws, int nw, int epi) {
  return prepare_one_problem(a, waves, ws, nw, epi) && gemv_uses_m1(a, ws[0]->bits, waves);
}
// ... the same problem on the stripe-stream kernel: what try_gemv launches where gemv_uses_m1 is false
bool prepare_general_problem(GemvArgs& a, int& waves, const DeviceWeight* const* ws, int nw, int epi) {
  return prepare_one_problem(a, waves, ws, nw, epi) && !gemv_uses_m1(a, ws[0]->bits, waves);
}

// 1 launched, 0 not eligible, -1 launch error
static int try_gemv(const Act& x, const Weights& W, const Epi& e, hipStream_t st) {
  if (knobs().gemv_disable) return 0;
  GemvArgs a{};
  int waves = 0, grid = 0;
  if (!prepare_gemv(a, waves, grid, x, W, e)) return 0;
  const int bits = W[0].bits;
  const size_t lds = gemv_lds_layout(a, bits, waves, grid);
  const bool dry = planned(gemv_uses_m1(a, bits, waves) ? NAD_KERNEL_GEMV_M1 : NAD_KERNEL_GEMV, grid, waves * 64, 1, 0);
  return launch_gemv_named(dry, "gemv kernel", [&] { return launch_gemv(a, bits, waves, grid, lds, st); }) ? 1 : -1;
}

static int run_i8(const Act& x, const Weights& W, bool dual, const Epi& e, hipStream_t st);

static bool refuse_q6k(const DeviceWeight& w, const char* path) {
  if (!is_q6k(w)) return false;
  set_err("a GGUF Q6_K weight reached the %s path, which cannot read its layout (Q6_K runs on woq_q6k_gemv_kernel / "
          "woq_q6k_gemm_kernel only)", path);
  return true;
}

static int run_skinny(const Act& x, const Weights& W, const Epi& e, hipStream_t st) {
  const int nw = W.nw;
  for (int i = 0; i < nw; i++)
    if (refuse_q6k(W[i], "stripe-stream / skinny decode")) return -1;
  if (nw > 1) {  // weights of one fused call whose arithmetic differs (per-weight compute modes) run one by one
    bool mixed = false;
    for (int i = 1; i < nw; i++)
      mixed |= int8_compute(W[i]) != int8_compute(W[0]) || gguf_act_quant(W[i]) != gguf_act_quant(W[0]);
    if (mixed) {
      if (e.is_dual()) {
        set_err("gate/up weights of one FFN must resolve to the same arithmetic (nad_device_set_compute)");
        return -1;
      }
      for (int i = 0; i < nw; i++)
        if (run_skinny(x, W.sub(i, 1), e, st)) return -1;
      return 0;
    }
  }
  if (int8_compute(W[0])) return run_i8(x, W, nw == 2 && e.is_dual(), e, st);
  const int g = try_gemv(x, W, e, st);
  if (g != 0) return g < 0 ? -1 : 0;
  SkinnyArgs a{};
  fill_act(a, x);
  fill_epi(a, e);
  a.nw = nw;
  a.scale_t = W[0].scale_t;
  a.vec_ok = vec_aligned(x) ? 1 : 0;
  const bool dual = e.is_dual();
  int stripes = 0;
  for (int i = 0; i < nw; i++) {
    a.w[i] = view(W[i], W.outs[i], W.ldos[i], e);
    a.stripe_base[i] = stripes;
    stripes += W[i].ns;
  }
  a.stripe_base[nw] = stripes;
  if (dual) stripes = W[0].ns;
  int ks, tpw, ch;
  skinny_geometry(stripes, W[0].nt, dual ? 2 : 1, &ks, &tpw, &ch);
  a.tiles_per_wave = tpw;
  a.steps_per_group = W[0].blocksize / 32;
  a.a_fast = (a.vec_ok && W[0].shuffle == nullptr && x.k % (x.t == kActF32 ? 4 : 8) == 0) ? 1 : 0;
  const int waves = ks * (dual ? 2 : 1);
  return launch(planned(NAD_KERNEL_SKINNY, stripes, waves * 64), "skinny kernel",
                [&] { return launch_skinny(a, W[0].bits, x.t, waves, stripes, ch, st); })
             ? 0
             : -1;
}

// ------------------------------------------------------------------------------------------------ int8 compute
struct I8Act {  // the quantized activations of one call
  const int8_t* aq = nullptr;
  int ldq = 0;
  const float2* sa = nullptr;
  int m = 0, k = 0;
};

static size_t i8_act_bytes(int m, const DeviceWeight& w) {
  return align256(size_t(m) * w.nt * tile_k(w.bits)) + align256(size_t(m) * w.ng * sizeof(float2));
}

static int i8_quantize(I8Act& r, char* ws, const Act& x, const DeviceWeight& w, hipStream_t st) {
  const int kp = w.nt * tile_k(w.bits);
  r.aq = reinterpret_cast<int8_t*>(ws);
  r.ldq = kp;
  r.sa = reinterpret_cast<float2*>(ws + align256(size_t(x.m) * kp));
  r.m = x.m;
  r.k = x.k;
  if (const int aq = gguf_act_quant(w)) {  // Q8_0 / Q8_1 rows (quantize_row_q8_0_reference / quantize_row_q8_1_reference)
    Q8Args q{};
    fill_act(q, x);
    q.aq = const_cast<int8_t*>(r.aq);
    q.ldq = kp;
    q.kp = kp;
    q.sa = const_cast<float2*>(r.sa);
    return launch(planned_pass(), "Q8_0 / Q8_1 activation quantization",
                  [&] { return launch_q8_quant(q, aq == 2, x.t, st); })
               ? 0
               : -1;
  }
  QuantU8Args q{};
  fill_act(q, x);
  q.bs = w.blob_bs;
  q.ng = w.ng;
  q.shuffle = w.shuffle;
  q.aq = const_cast<int8_t*>(r.aq);
  q.ldq = kp;
  q.kp = kp;
  q.sa = const_cast<float2*>(r.sa);
  return launch(planned_pass(), "activation quantization", [&] { return launch_quant_u8(q, x.t, st); }) ? 0 : -1;
}

struct Sums {  // block sums of the activation rows: p[m * ld + b * st] (p null: the min-term pass sums them itself)
  const float* p = nullptr;
  int ld = 0, st = 0;
};
static int min_term(const Act& x, Sums s, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st);

static int i8_gemm_main(const I8Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  I8Args a{};
  a.aq = x.aq;
  a.ldq = x.ldq;
  a.a_signed = gguf_act_quant(w) ? 1 : 0;
  a.sa = x.sa;
  a.M = x.m;
  a.K = x.k;
  a.red = static_cast<const uint16_t*>(w.reduce);
  a.red_ld = w.red_ld;
  a.scale_t = w.scale_t;
  fill_epi(a, e);
  a.w = view(w, o.p, o.ld, e);
  return launch(planned(NAD_KERNEL_I8, 0, 0), "int8-compute kernel", [&] { return launch_i8(a, w.bits, st); }) ? 0 : -1;
}

static int i8_gemm(const I8Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  if (!w.mins) return i8_gemm_main(x, w, o, e, st);
  // Q4_1 / Q5_1 x Q8_1 (vec_dot.h:385-400, 569-590): the block dots on the true q, then + sum_b m * s with the Q8_1
  // block sums s = sa[].y, and the caller's epilogue
  if (i8_gemm_main(x, w, o, Epi{}, st)) return -1;
  return min_term(Act{nullptr, kActF32, 0, x.m, x.k}, Sums{&x.sa[0].y, 2 * w.ng, 2}, w, o, e, st);
}

// nw weights on one activation.  dual: the FFN gate/up pair (outs[1] = act(x.w0) * (x.w1); aux, if given, receives
// act(x.w0)), run as the prefill FFN does: two passes, the second multiplying by the first's output.
static int run_i8(const Act& x, const Weights& W, bool dual, const Epi& e, hipStream_t st) {
  for (int i = 0; i < W.nw; i++)
    if (!int8_compute(W[i]) || gguf_act_quant(W[i]) != gguf_act_quant(W[0])) {
      set_err("int8 compute: the weights of a fused call must all be integer-core blobs (with reduce) or all GGUF types "
              "of one activation quantizer (Q8_0: Q4_0, Q5_0, Q8_0; Q8_1: Q4_1, Q5_1)");
      return -1;
    }
  const size_t abytes = i8_act_bytes(x.m, W[0]);
  const bool own_t1 = dual && !e.aux;
  const size_t t1bytes = own_t1 ? size_t(x.m) * W[0].n * sizeof(float) : 0;
  char* wsp = static_cast<char*>(workspace_for(abytes + t1bytes, st));
  if (!wsp) return -1;
  I8Act xq;
  if (i8_quantize(xq, wsp, x, W[0], st)) return -1;
  if (dual) {
    float* t1 = own_t1 ? reinterpret_cast<float*>(wsp + abytes) : e.aux;
    const int ld1 = own_t1 ? W[0].n : e.ld_aux;
    if (i8_gemm(xq, W[0], Out{t1, ld1}, Epi::gate_of(e.kind), st)) return -1;
    return i8_gemm(xq, W[1], Out{W.outs[1], W.ldos[1]}, Epi::mul(t1, ld1), st);
  }
  for (int i = 0; i < W.nw; i++)
    if (i8_gemm(xq, W[i], Out{W.outs[i], W.ldos[i]}, e, st)) return -1;
  return 0;
}

// ------------------------------------------------------------------------------------------------ min-term pass
// The minimum term of a GGUF Q4_1 / Q5_1 weight and the caller's epilogue, on an `out` that holds X (q d)^T
// (woq_gguf.hip): out = epi(out + S mins^T).  s.p null: the exact block sums of the activations -- summed inside the
// M <= 16 kernel, else by a pre-pass into the workspace (the main kernel's use of it is over by stream order).  A
// weight without mins gets the epilogue alone (the mixed FFN pairs).
static int min_term(const Act& x, Sums s, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  MinTermArgs a{};
  fill_act(a, x);
  a.mins = static_cast<const uint16_t*>(w.mins);
  a.scales = static_cast<const uint16_t*>(w.scales);  // GGUF: fp16
  a.qbias = float(w.min_bias);
  a.ns = w.ns;
  a.ng = w.ng;
  a.kmajor = w.kmajor;
  a.g.M = x.m;
  a.g.K = x.k;
  fill_epi(a.g, e);
  if (e.kind == kEpiGeluMul) a.g.epi = kEpiSiluMul;  // the multiply by aux (the activation is in aux already)
  a.g.w = view(w, o.p, o.ld, e);
  const bool small = x.m <= kMinTermSmallM && size_t(x.m) * w.ng * sizeof(float) <= kMinTermSmallLds;
  if (!small && a.mins && !s.p) {
    float* sums = static_cast<float*>(workspace_for(size_t(x.m) * w.ng * sizeof(float), st));
    if (!sums) return -1;
    if (!launch(planned_pass(), "activation block-sum",
                [&] { return launch_block_sums(x.p, x.t, x.ld, x.m, x.k, sums, st); }))
      return -1;
    s = Sums{sums, w.ng, 1};
  }
  a.S = s.p;
  a.s_ld = s.ld;
  a.s_st = s.st;
  return launch(planned_pass(), "min-term kernel",
                [&] { return small ? launch_min_term(a, x.t, st) : launch_min_term_tiled(a, st); })
             ? 0
             : -1;
}

// ------------------------------------------------------------------------------------------------ prefill GEMMs
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
  if (kn.gemm2_disable || w.kmajor || w.f4kind >= 0 || m <= 16 || is_q6k(w) ||
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
// The FFN's prefill keeps its intermediates in fp16 when all three GEMMs are the pipelined ones reading the unshuffled
// fp16 operand and fmid is a whole number of w2's K tiles (NAD_FFN_F32=1: the fp32 intermediates, A/B)
static bool ffn16_ok(const DeviceWeight& w1, const DeviceWeight& w2, const DeviceWeight& w3, int m, int fmid) {
  auto ok = [&](const DeviceWeight& w) {
    return pipelined_gemm(w, m) && !w.shuffle && !int8_compute(w);
  };
  return !knobs().ffn_f32 && knobs().gemm_kernel != 2 && ok(w1) && ok(w2) && ok(w3) &&
         w2.nt * tile_k(w2.bits) == fmid && fmid % 8 == 0;
}

// 1 ready, -1 error (no workspace under capture, launch error)
static int prepare_a16(A16& r, const Act& x, const DeviceWeight& w, hipStream_t st) {
  const int kp = w.nt * tile_k(w.bits);
  r.kp = kp;
  if (x.t == kActF16 && !w.shuffle && x.k == kp && reinterpret_cast<uintptr_t>(x.p) % 16 == 0 &&
      (size_t(x.ld) * 2) % 16 == 0) {
    r.p = static_cast<const _Float16*>(x.p);
    r.ld = x.ld;
    return 1;
  }
  _Float16* buf = static_cast<_Float16*>(workspace_for(size_t(x.m) * kp * 2, st));
  if (!buf) return -1;
  if (!launch(planned_pass(), "activation conversion",
              [&] { return launch_cvt_act(x.p, x.t, x.ld, x.m, x.k, kp, w.shuffle, buf, st); }))
    return -1;
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
  const int tpg = std::max(1, w.blocksize / tile_k(w.bits));
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

// The slabs of a split-K launch (ks runs of ktiles K tiles; launch_splitk_reduce sums them): ks x m fp32 rows in the
// stream's workspace (stream-ordered reuse) after the caller's a16 bytes, the fp16 activations' room; false: none
static bool splitk_slabs(GemmArgs& a, const DeviceWeight& w, int m, int ks, int ktiles, size_t a16, hipStream_t st) {
  a.ksplit = ks;
  a.ktiles = ktiles;
  a.ldp = (w.n + 3) / 4 * 4;
  char* base = static_cast<char*>(workspace_for(a16 + size_t(ks) * m * a.ldp * 4, st));
  if (base) a.part = reinterpret_cast<float*>(base + a16);
  return base != nullptr;
}

// Geometry of a mid-M launch: stripes per workgroup, its waves, stages per wave (mid_geometry), stripe groups, K runs
struct MidGeom {
  int sps, nw, spw, nsg, ks;
  int grid() const { return nsg * ks; }
};
// runs per stripe group: one chunk each, the slabs within nad_device_workspace_size's N-independent bound (m x 128 KiB
// past the fp16 copy): ks x N <= 32768, so wide weights split K less (N = 11008: 2 runs; N = 32000: none)
static MidGeom mid_plan(const DeviceWeight& w, int gpt, int act_t, int rf, int wide) {
  MidGeom g{};
  mid_geometry(w.bits, gpt, act_t, rf, wide, &g.sps, &g.nw, &g.spw);
  const int chunk = g.nw * g.spw, ks_max = 32768 / ((w.n + 3) / 4 * 4), mid_ks = knobs().mid_ks;
  g.nsg = (w.ns + g.sps - 1) / g.sps;
  g.ks = std::max(1, std::min((w.nt + chunk - 1) / chunk, ks_max));
  if (mid_ks > 0) g.ks = std::max(1, std::min({mid_ks, w.nt, ks_max}));
  return g;
}

// The mid-M GEMM (woq_gemm_mid.hip) for 17 <= M <= 64 (NAD_MID_MIN_M / NAD_MID_MAX_M): integer int4 / int2 weights,
// stripe-major, no act-order gather, 16-B aligned activation rows with K % 8 == 0 (int2 and int4 g32: M <= 32).
// Stripe groups of 4 x K runs of one chunk (8 K tiles int4, 4 int2: mid_geometry) each, so K = 4096 splits 4 ways and
// the 256 / 688 / 768 stripes of the Llama shapes give 256 / 688 / 768 workgroups; the runs' fp32 slabs are summed by
// the split-K reduce launch.  Returns 1 if launched, 0 if not eligible, -1 on error.
// A fused caller's shared fp16 copy of A is not read: the kernel converts the caller's activations itself, so a fused
// QKV / FFN launch is bit-identical to the same weights' single launches; its split-K slabs go past where such a copy
// sits in the workspace (the weights after this one may still read it).
static int run_mid(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  const Knobs& kn = knobs();
  const int m = x.m;
  if (m > kn.mid_max_m || m < (kn.mid_min_m > 0 ? kn.mid_min_m : 8)) return 0;
  if ((w.bits != 4 && w.bits != 2) || w.kmajor || w.f4kind >= 0 || w.shuffle) return 0;
  if (w.bits == 2 && m > 32) return 0;  // a 256-deep int2 stage's activation fragments: 32 rows fit the registers
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(w.bits, w.nt, w.ng, w.blocksize, &tpg);
  if (gpt != 1 && gpt != 2 && gpt != 4) return 0;
  if (gpt == 4 && m > 32) return 0;  // 4 groups per tile x 4 stripes of scales beside 64 rows: out of registers
  if (!vec_aligned(x) || x.k % 8 != 0) return 0;
  const int esz = x.t == kActF32 ? 4 : 2;
  if (uint64_t(m) * x.ld * esz >= (1ull << 31) || uint64_t(w.ns) * w.nt * 1024 >= (1ull << 31)) return 0;
  const int rf = (m + 15) / 16;
  if (rf > 4) return 0;  // NAD_MID_MAX_M above 64: mid_geometry has no shape for more than 4 row fragments
  MidGeom g = mid_plan(w, gpt, x.t, rf, kn.mid_wide == 1);
  // from 8 rows of fp32 / bf16 activations (the GEMV stages them as two fp16 rows each) the mid-M kernel beats the
  // stripe-stream GEMV: K = N = 4096 M = 16 8.3 vs 10.1 us (fp16), 9.0 vs 12.7 (fp32); N = 11008 fp32 M = 16 17.7 vs
  // 36.7 (profiles/r05_mid_small_m.txt).  fp16 rows: from 9 where the stripe groups x K runs fit the CUs in one round
  // (K = N = 4096 M = 10: 7.7 vs 8.7 us), else from 12 (N = 11008 M = 8: GEMV 12.1 vs 14.2; profiles/r06_mid_min_m_ab.txt)
  if (kn.mid_min_m <= 0 && x.t == kActF16 && m < (g.grid() <= device_cus() ? 9 : 12)) return 0;
  // 8-stripe workgroups (where mid_geometry has them) when the 4-stripe grid takes more than one workgroup per CU and
  // theirs does not: N = 11008, M = 16 / 32: 344 -> 172 workgroups, 16.3 -> 14.3-14.9 us, 21.1 -> 18.8
  // (profiles/r06_mid_wide_ab.txt); at N = 4096 (256 either way) the 8-stripe form's doubled slabs cost 0.7-1 us
  if (kn.mid_wide == 2 && g.sps == 4 && g.grid() > device_cus()) {
    const MidGeom wide = mid_plan(w, gpt, x.t, rf, 1);
    if (wide.sps != 4 && wide.grid() <= device_cus()) g = wide;
  }
  const int ktiles = (w.nt + g.ks - 1) / g.ks;
  const int ks = (w.nt + ktiles - 1) / ktiles;
  GemmArgs a{};
  fill_act(a, x);
  fill_epi(a, e);
  fill_h16(a, o.h16);
  a.scale_t = w.scale_t;
  a.tpg_shift = tpg == 0 ? 31 : __builtin_ctz(unsigned(tpg));
  a.w = view(w, o.p, o.ld, e);
  if (ks > 1) {
    if (uint64_t(ks) * m * ((w.n + 3) / 4 * 4) * 4 >= (1ull << 31)) return 0;
    const size_t a16 = (size_t(m) * ((size_t(x.k) + 255) / 256 * 256) * 2 + 255) / 256 * 256;  // an fp16 copy's room
    if (!splitk_slabs(a, w, m, ks, ktiles, a16, st)) return -1;
  } else {
    a.ktiles = w.nt;
  }
  // a stripe group's runs and the reduce of their slabs on one XCD: the reduce reads the slabs from that XCD's L2
  // instead of memory (K = N = 4096: M = 64 14.3 -> 12.7 us, M = 32 10.3 -> 9.5; profiles/r06_mid_xcd_ab.txt)
  if (ks > 1 && kn.mid_xcd) {
    a.xcd_sg = g.nsg;
    a.xcd_w = g.sps * 4;
  }
  const int grid = g.nsg * ks;
  const bool dry = planned(NAD_KERNEL_MID, grid, g.nw * 64, ks, 0);
  if (dry && ks > 1) planned_pass();  // the split-K reduce
  return launch(dry, "mid-M GEMM",
                [&] {
                  hipError_t err = launch_gemm_mid(a, w.bits, gpt, x.t, rf, g.sps, grid, st);
                  if (err == hipSuccess && ks > 1) err = launch_splitk_reduce(a, st);
                  return err;
                })
             ? 1
             : -1;
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
  const int hpt = tile_k(w.bits) / 64;
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
// the tile height a gemm7 launch of this weight takes: NAD_GEMM7_BM or the model's
static int gemm7_bm(const DeviceWeight& w, int m) {
  const int bm = knobs().gemm7_bm > 0 ? knobs().gemm7_bm : gemm7_pick_bm(w, m);
  return (bm != 32 && bm != 64 && bm != 128) ? 256 : bm;
}
int gemm7_tile_height(const DeviceWeight& w, int m) { return gemm7_bm(w, m); }
int gemm7_k_tile(const DeviceWeight& w) { return tile_k(w.bits); }

// M > 16, one weight: the int8 arithmetic, the mid-M kernel, a pipelined GEMM on the fp16 activations (pre: a copy the
// caller shares among weights) or the register-staged fallback
static int run_gemm(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st,
                    const A16* pre = nullptr) {
  if (refuse_q6k(w, "mid-M / prefill GEMM")) return -1;
  if (int8_compute(w)) return run_i8(x, One(w, o), false, e, st);
  {
    const int r = run_mid(x, w, o, e, st);
    if (r != 0) return r < 0 ? -1 : 0;
  }
  const int m = x.m;
  GemmArgs a{};
  fill_act(a, x);
  fill_epi(a, e);
  a.scale_t = w.scale_t;
  a.vec_ok = vec_aligned(x) ? 1 : 0;
  const Knobs& kn = knobs();
  a.stagger = kn.gemm3_stagger;  // measured +3-7 % (profiles/r02_gemm3_stagger.txt)
  // scale folding measured 1-5 % SLOWER on gemm3 (profiles/r03_gemm3_fold.txt): gemm3 keeps the exact fp32 group scale
  a.fold = 0;
  a.w = view(w, o.p, o.ld, e);
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
    const bool win = tiles > device_cus() || w.nt * tile_k(w.bits) >= 8192;
    a.ksw = kn.gemm4_ksw == 1 || (kn.gemm4_ksw == 2 && win) ? 1 : 0;
  }
  if (o.h16 && !pg) {
    set_err("fp16 GEMM output needs the pipelined GEMM");
    return -1;
  }
  fill_h16(a, o.h16);
  if (!pg)
    return launch(planned(NAD_KERNEL_GEMM, 0, 0), "gemm kernel", [&] { return launch_gemm(a, w.bits, x.t, st); }) ? 0
                                                                                                                 : -1;
  A16 own;
  if (!pre || pre->kp != w.nt * tile_k(w.bits) || w.shuffle) {
    if (prepare_a16(own, x, w, st) < 0) return -1;
    pre = &own;
  }
  const bool g2 = pg == 3 && kn.gemm_kernel == 2;
  // gemm7 (group scale folded, waves split over K) is the default for int4 groups of 128 * 2^j: +5-10 % over gemm3
  // (profiles/r05_gemm7_*); a weight whose q * s leaves the fp16 normal range, or NAD_GEMM_KERNEL=3, runs gemm3
  // (as for gemm4, NAD_GEMM4_FOLD=0 turns the fold off: int4 g128 then runs gemm3's exact fp32 group scale)
  const bool g7 = pg == 3 && kn.gemm_kernel == 7 && kn.gemm4_fold && gemm7_ok(w.bits, w.blocksize, w.fold_ok);
  if (g7) a.fold = 1;
  const int bm = g7 ? gemm7_bm(w, m) : 256;
  int ktiles = w.nt;
  const int ks = !g2 ? splitk_plan(w, m, &ktiles, bm) : 1;
  if (ks > 1 && kn.gemm4_ksw == 2) a.ksw = 0;  // auto KSW was measured on whole-K launches only
  // partials after the fp16 activations
  if (ks > 1 && !splitk_slabs(a, w, m, ks, ktiles, (size_t(m) * w.nt * tile_k(w.bits) * 2 + 255) / 256 * 256, st)) return -1;
  const int tiles = ((m + bm - 1) / bm) * ((w.n + 127) / 128);
  // split K: every run of a tile and the reduce of its slabs on one XCD (slabs read back from that XCD's L2): K = N =
  // 4096 M = 128 18.6 -> 15.9 us, M = 96 17.2 -> 14.8 (profiles/r06_gemm7_xcd_splitk_ab.txt)
  if (g7 && ks > 1 && kn.gemm_xcd && (((m + bm - 1) / bm) * ((w.ns + 7) / 8)) % 8 == 0) a.xcd_tile = bm;
  const bool dry =
      planned(pg == 4 ? NAD_KERNEL_GEMM4 : (g2 ? NAD_KERNEL_GEMM2 : (g7 ? NAD_KERNEL_GEMM7 : NAD_KERNEL_GEMM3)),
              tiles * ks, 512, ks, a.fold | (a.ksw << 1));
  if (dry && ks > 1) planned_pass();  // the split-K reduce
  return launch(dry, "gemm2 kernel",
                [&] {
                  hipError_t err = pg == 4 ? launch_gemm4(a, w.bits, pre->p, pre->ld, st)
                                   : g2    ? launch_gemm2(a, pre->p, pre->ld, st)
                                   : g7    ? launch_gemm7(a, w.bits, bm, pre->p, pre->ld, st)
                                           : launch_gemm3(a, pre->p, pre->ld, st);
                  if (err == hipSuccess && ks > 1) err = launch_splitk_reduce(a, st);
                  return err;
                })
             ? 0
             : -1;
}

// ------------------------------------------------------------------------------------------------ forward
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

// one weight, one launch chain: the body of nad_device_forward
static int forward_one(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  if (x.m > kSkinnyMaxM) return run_gemm(x, w, o, e, st);
  // M <= 16: the mid-M kernel from 8 rows of fp32 / bf16 activations, and of fp16 rows from 9 where its grid fits the
  // CUs in one round, else from 12 (run_mid; NAD_MID_MIN_M overrides); below that, and for the fused QKV / FFN entries
  // at any M <= 16, the skinny GEMV.  Its split-K slabs fit nad_device_workspace_size(m, k).
  if (!int8_compute(w)) {
    const int r = run_mid(x, w, o, e, st);
    if (r != 0) return r < 0 ? -1 : 0;
  }
  return run_skinny(x, One(w, o), e, st);
}

// A weight with block mins (GGUF Q4_1 / Q5_1), or the partner of one in a fused FFN: the unchanged kernels compute
// X (q d)^T into out, the min-term pass adds S mins^T and applies the epilogue (aux: the SILU_MUL / GELU_MUL operand).
// In the int8 mode the Q8_1 sums replace S and run_i8 appends the pass itself.
static int forward_min(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  if (int8_compute(w)) {
    Epi e8 = e;
    if (e.kind == kEpiGeluMul) e8.kind = kEpiSiluMul;
    return run_i8(x, One(w, o), false, e8, st);
  }
  if (forward_one(x, w, o, Epi{}, st)) return -1;
  return min_term(x, Sums{}, w, o, e, st);
}
// A GGUF Q6_K weight (woq_q6k.hip): the decode GEMV up to 16 rows -- sub-scales applied in fp32, plan fold 0 -- and the
// register-staged GEMM above, which folds sc * q into its fp16 fragments (plan fold 1).  Both apply the epilogue
// themselves (gemm_epilogue4: every single-weight kind and the multiply by aux of the FFN's second pass).  A weight
// in mode 2 (q8k_compute) takes woq_q6k_i8_kernel at every M instead: Q8_K activation rows quantized in the kernel's own
// staging (no pre-pass, one launch), integer group dot products, plan fold 0.
static int forward_q6k(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  if (o.h16 || e.kind == kEpiGeluMul) {
    set_err("Q6_K: fp16 GEMM output and the fused dual epilogues are not available (the FFN entries run two passes)");
    return -1;
  }
  GemmArgs a{};
  fill_act(a, x);
  fill_epi(a, e);
  a.scale_t = w.scale_t;
  a.vec_ok = vec_aligned(x) ? 1 : 0;
  a.w = view(w, o.p, o.ld, e);
  if (q8k_compute(w)) {
    Q6kI8Geom g{};
    if (!q6k_i8_geometry(x.m, x.k, w.ns, device_cus(), &g)) {
      set_err("Q6_K in Q8_K arithmetic: K = %d is too long for the kernel's LDS staging of one activation row", x.k);
      return -1;
    }
    return launch(planned(NAD_KERNEL_Q6K_I8, g.grid * g.passes, g.waves * 64, 1, 0), "Q6_K Q8_K-arithmetic kernel",
                  [&] { return launch_q6k_i8(a, x.t, g, st); })
               ? 0
               : -1;
  }
  if (x.m <= kSkinnyMaxM) {
    Q6kGemvGeom g{};
    if (!q6k_gemv_geometry(x.m, x.k, w.ns, x.t, device_cus(), &g)) {
      set_err("Q6_K decode: K = %d is too long for the kernel's LDS staging of one activation row", x.k);
      return -1;
    }
    return launch(planned(NAD_KERNEL_Q6K_GEMV, g.grid * g.passes, g.waves * 64, 1, 0), "Q6_K gemv kernel",
                  [&] { return launch_q6k_gemv(a, x.t, g, st); })
               ? 0
               : -1;
  }
  a.fold = 1;
  const int tiles = ((x.m + 127) / 128) * ((w.ns + 7) / 8);
  return launch(planned(NAD_KERNEL_Q6K_GEMM, tiles, 512, 1, 1), "Q6_K gemm kernel",
                [&] { return launch_q6k_gemm(a, x.t, st); })
             ? 0
             : -1;
}
static int forward_any(const Act& x, const DeviceWeight& w, const Out& o, const Epi& e, hipStream_t st) {
  if (is_q6k(w)) return forward_q6k(x, w, o, e, st);
  return w.mins ? forward_min(x, w, o, e, st) : forward_one(x, w, o, e, st);
}

extern "C" int nad_device_forward(const void* act, int act_dtype, const void* devstor, float* out, int m, int n, int k,
                                  int lda, int ldo, int epi, const float* bias, int bias_ld, const float* res,
                                  int ld_res, void* queue) {
  Epi e;
  e.kind = epi;
  e.bias = bias;
  e.bias_ld = bias_ld;
  e.res = res;
  e.ld_res = ld_res;
  if (e.is_dual()) {
    set_err("dual epilogues go through nad_device_ffn_forward");
    return -1;
  }
  if ((epi == kEpiBias || epi == kEpiAddGelu) && !bias) {
    set_err("bias epilogue without bias");
    return -1;
  }
  if (epi == kEpiResAdd && !res) {
    set_err("residual epilogue without residual");
    return -1;
  }
  const DeviceWeight* w = as_weight(devstor);
  if (!w || !check_shape(*w, m, n, k, lda, ldo)) return -1;
  return forward_any(Act{act, act_dtype, lda, m, k}, *w, Out{out, ldo}, e, static_cast<hipStream_t>(queue));
}

extern "C" void bestla_device_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k,
                                             int lda, int ldo, void* workspace, void* queue) {
  CallWorkspace cw(workspace, nad_device_workspace_size(_m, _k));
  if (nad_device_forward(activation, kActF32, weiptr, output, _m, _n, _k, lda, ldo, kEpiNone, nullptr, 0, nullptr, 0,
                         queue) != 0)
    report("bestla_device_f32f32_forward");
}

// ------------------------------------------------------------------------------------------------ fused QKV
static bool same_kind(const DeviceWeight& a, const DeviceWeight& b) {
  return a.bits == b.bits && a.f4kind == b.f4kind && a.k == b.k && a.blocksize == b.blocksize &&
         a.scale_t == b.scale_t && a.nt == b.nt &&
         a.ng == b.ng && (a.shuffle == nullptr) == (b.shuffle == nullptr);
}

// Fused QKV prefill on gemm7: the weights' column tiles in ONE launch where each weight would run whole-K gemm7 at the
// same tile height on its own -- the same tiles and arithmetic as the separate launches (bit-identical outputs), one
// kernel boundary and one tail of output stores instead of n: Llama-2-7B at M = 2048 runs 3 x 256 tiles as 3 rounds of
// one launch (profiles/r06_gemm7_fused_qkv_ab.txt).  Returns 1 if launched, 0 if not eligible, -1 on error.
static int run_gemm7_fused(const Act& x, const Weights& W, hipStream_t st, const A16* pre) {
  const Knobs& kn = knobs();
  const int n = W.nw, m = x.m;
  if (n < 2 || n > 3 || !kn.gemm7_fuse || m <= kn.mid_max_m) return 0;
  // the fused instantiation (woq_gemm7_kernel<..., MW>): int4, one group per K tile or more
  if (W[0].bits != 4 || W[0].blocksize % 128 != 0) return 0;
  int bm0 = 0;
  for (int i = 0; i < n; i++) {
    const DeviceWeight& w = W[i];
    if (int8_compute(w) || w.shuffle || pipelined_gemm(w, m) != 3) return 0;
    if (kn.gemm_kernel != 7 || !kn.gemm4_fold || !gemm7_ok(w.bits, w.blocksize, w.fold_ok)) return 0;
    if (i > 0 && (!same_kind(w, W[0]) || (w.zps == nullptr) != (W[0].zps == nullptr))) return 0;
    const int bm = gemm7_bm(w, m);
    int kt = w.nt;
    if (splitk_plan(w, m, &kt, bm) != 1) return 0;  // that weight's own launch splits K: other sums
    if (bm == 32 || (i > 0 && bm != bm0)) return 0;
    bm0 = bm;
  }
  GemmArgs a{};
  fill_act(a, x);
  a.scale_t = W[0].scale_t;
  a.epi = kEpiNone;
  a.vec_ok = vec_aligned(x) ? 1 : 0;
  a.fold = 1;
  a.w = view(W[0], W.outs[0], W.ldos[0]);
  int cut = (W[0].ns + 7) / 8;
  a.nbn_cut[0] = a.nbn_cut[1] = cut;
  for (int i = 1; i < n; i++) {
    a.wf[i - 1] = view(W[i], W.outs[i], W.ldos[i]);
    cut += (W[i].ns + 7) / 8;
    if (i == 1) a.nbn_cut[1] = cut;
  }
  a.nbn_all = cut;
  a.nwt = n;
  if (planned(NAD_KERNEL_GEMM7, ((m + bm0 - 1) / bm0) * cut, 512, 1, 1)) return 1;
  A16 own;
  if (!pre || pre->kp != W[0].nt * tile_k(W[0].bits)) {
    if (prepare_a16(own, x, W[0], st) < 0) return -1;
    pre = &own;
  }
  return launch(false, "fused gemm7", [&] { return launch_gemm7(a, W[0].bits, bm0, pre->p, pre->ld, st); }) ? 1 : -1;
}

// {Q, K} int2 + {V} int4 at M = 1: ONE launch whose workgroups are split between the two formats by bytes.  1 launched,
// 0 not eligible, -1 launch error
static int try_gemv_dual(const Act& x, const Weights& qk, const Weights& v, hipStream_t st) {
  GemvArgs a1, a2;
  int w1 = 0, w2 = 0, g1 = 0, g2 = 0;
  if (!prepare_gemv(a1, w1, g1, x, qk, Epi{}) || !prepare_gemv(a2, w2, g2, x, v, Epi{}) || w1 != 16 || w2 != 16 ||
      !gemv_dual_ok(a1, qk[0].bits, a2, v[0].bits, 16))
    return 0;
  const double b1 = double(a1.units) * a1.nt, b2 = double(a2.units) * a2.nt;  // 1 KiB tiles of each part
  const int cus = device_cus();
  int n1 = int(cus * b1 / (b1 + b2) + 0.5);
  n1 = std::max(1, std::min(std::min(n1, cus - 1), a1.units));
  const int n2 = std::max(1, std::min(cus - n1, a2.units));
  a1.u_q = a1.units / n1;
  a1.u_r = a1.units % n1;
  a2.u_q = a2.units / n2;
  a2.u_r = a2.units % n2;
  const size_t lds = std::max(gemv_lds_layout(a1, qk[0].bits, 16, n1), gemv_lds_layout(a2, v[0].bits, 16, n2));
  if (lds > 160 * 1024) return 0;
  return launch(planned(NAD_KERNEL_GEMV_M1, n1 + n2, 16 * 64), "gemv dual",
                [&] { return launch_gemv_dual(a1, a2, n1, n2, 16, lds, st); })
             ? 1
             : -1;
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
  const Weights W{3, ws, outs, ldos};
  const Act x{act, act_dtype, lda, m, k};
  // block mins or a Q6_K weight: the three weights one after another
  if (ws[0]->mins || ws[1]->mins || ws[2]->mins || is_q6k(*ws[0]) || is_q6k(*ws[1]) || is_q6k(*ws[2])) {
    for (int i = 0; i < 3; i++)
      if (forward_any(x, W[i], Out{outs[i], ldos[i]}, Epi{}, st)) return -1;
    return 0;
  }
  if (m <= kSkinnyMaxM) {
    // one stream launch over every run of consecutive weights of one kind (Q, K and V may differ in N; a mixed-format
    // model such as the int2 policy's int4 wv gets {Q, K} + {V}), each output computed exactly as on its own
    auto kin = [&](int i, int j) { return same_kind(W[i], W[j]) && W[i].asym == W[j].asym; };
    if (m == 1 && kin(0, 1) && !kin(1, 2) && knobs().gemv_dual && !knobs().gemv_disable) {
      const int r = try_gemv_dual(x, W.sub(0, 2), W.sub(2, 1), st);
      if (r != 0) return r < 0 ? -1 : 0;
    }
    for (int i = 0; i < 3;) {
      int n = 1;
      while (i + n < 3 && kin(i, i + n)) n++;
      if (run_skinny(x, W.sub(i, n), Epi{}, st)) return -1;
      i += n;
    }
    return 0;
  }
  A16 pre;
  const A16* pp = nullptr;
  if (gemm2_ok(W[0], m) && !W[0].shuffle && !int8_compute(W[0])) {
    if (prepare_a16(pre, x, W[0], st) < 0) return -1;
    pp = &pre;
  }
  {
    const int r = run_gemm7_fused(x, W, st, pp);
    if (r != 0) return r < 0 ? -1 : 0;
  }
  for (int i = 0; i < 3; i++) {
    const DeviceWeight& w = W[i];
    // a weight that cannot reuse the shared fp16 copy (other K tile, act-order, int8 arithmetic) writes its own
    // conversion / u8 codes at the start of the same workspace: the copy is gone for the weights after it
    const bool reuses = pp && !int8_compute(w) && pipelined_gemm(w, m) && !w.shuffle && pp->kp == w.nt * tile_k(w.bits);
    const bool clobbers = !reuses && (int8_compute(w) || pipelined_gemm(w, m));
    if (run_gemm(x, w, Out{outs[i], ldos[i]}, Epi{}, st, reuses ? pp : nullptr)) return -1;
    if (clobbers && pp && pp->p != act) pp = nullptr;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ fused FFN
// The gate/up half of the fused FFN (ip_fusion_ffn.cpp:407-433): tmp2 = act(X.W1^T) * (X.W3^T), tmp1 = act(X.W1^T)
// (optional at M <= 16, required above).  Decode: one dual-weight stream launch; prefill: two GEMM launches.
extern "C" int nad_device_ffn_gate_up(const void* act, int act_dtype, const void* w1p, const void* w3p, float* tmp1,
                                      float* tmp2, int m, int fin, int fmid, int lda, int epi, void* queue) {
  const DeviceWeight* w1 = as_weight(w1p);
  const DeviceWeight* w3 = as_weight(w3p);
  if (!w1 || !w3) return -1;
  Epi e;
  e.kind = epi;
  if (!e.is_dual()) {
    set_err("ffn epilogue must be SILU_MUL or GELU_MUL");
    return -1;
  }
  // a pair with a Q6_K weight runs as two single-weight passes: the two need not share a format
  const bool q6k = is_q6k(*w1) || is_q6k(*w3);
  if (w1->n != fmid || w3->n != fmid || w1->k != fin || w3->k != fin || (!q6k && !same_kind(*w1, *w3))) {
    set_err("FFN gate/up shapes do not match (fin=%d fmid=%d)", fin, fmid);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  const Act x{act, act_dtype, lda, m, fin};
  const Out up{tmp2, fmid};
  if (w1->mins || w3->mins || q6k) {
    // block mins: two passes as run_i8's -- t1 = act(x.w1), tmp2 = t1 * (x.w3) -- each a main launch and the min-term
    // pass, which applies the activation / the multiply.  Without tmp1, t1 lies in the workspace behind the part the
    // passes' own kernels use (nad_device_workspace_size).
    if (!q6k && (int8_compute(*w1) != int8_compute(*w3) ||
                 (int8_compute(*w1) && gguf_act_quant(*w1) != gguf_act_quant(*w3)))) {
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
    // the partner without mins of a mixed pair applies the epilogue in its own kernel where that kernel can: the
    // activation always, the multiply by t1 in the prefill GEMMs and the int8 kernel (the M <= 16 fp kernels take the
    // multiply only as a fused pair, so there the min-term kernel runs as the epilogue alone)
    if (forward_any(x, *w1, Out{t1, fmid}, Epi::gate_of(epi), st)) return -1;
    if (is_q6k(*w3)) return forward_q6k(x, *w3, up, Epi::mul(t1, fmid), st);
    if (!w3->mins && m > kSkinnyMaxM) return run_gemm(x, *w3, up, Epi::mul(t1, fmid), st);
    return forward_min(x, *w3, up, Epi::mul(t1, fmid), st);
  }
  if (m <= kSkinnyMaxM) {
    const DeviceWeight* ws[2] = {w1, w3};
    float* outs[2] = {tmp2, tmp2};
    int ldos[2] = {fmid, fmid};
    e.aux = tmp1;
    e.ld_aux = fmid;
    return run_skinny(x, Weights{2, ws, outs, ldos}, e, st);
  }
  if (!tmp1) {
    set_err("prefill FFN needs the tmp1 buffer");
    return -1;
  }
  A16 pre;
  const A16* pp = nullptr;
  if (gemm2_ok(*w1, m) && !w1->shuffle && !int8_compute(*w1)) {
    if (prepare_a16(pre, x, *w1, st) < 0) return -1;
    pp = &pre;
  }
  if (run_gemm(x, *w1, Out{tmp1, fmid}, Epi::gate_of(epi), st, pp)) return -1;
  return run_gemm(x, *w3, up, Epi::mul(tmp1, fmid), st, pp);
}

int ffn_forward(const void* act, int act_dtype, const void* w1p, const void* w2p, const void* w3p, float* tmp1,
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
      (!is_q6k(*w1) && !is_q6k(*w3) && !same_kind(*w1, *w3))) {
    set_err("FFN shapes do not match (fin=%d fmid=%d fout=%d)", fin, fmid, fout);
    return -1;
  }
  hipStream_t st = static_cast<hipStream_t>(queue);
  const Out down{out, fout};
  const bool any_mins = w1->mins || w2->mins || w3->mins;
  const bool any_q6k = is_q6k(*w1) || is_q6k(*w2) || is_q6k(*w3);
  if (!any_mins && !any_q6k && f16_tmp && m > kSkinnyMaxM && tmp1 && ffn16_ok(*w1, *w2, *w3, m, fmid)) {
    // prefill with fp16 intermediates: gate -> act(x.w1) as fp16 in tmp1, up -> act(x.w1) * (x.w3) as fp16 in tmp2,
    // which IS down's fp16 A operand (fmid = whole K tiles): no fp32 round trip, no conversion pass before down
    const Act x{act, act_dtype, lda, m, fin};
    A16 pre;
    if (prepare_a16(pre, x, *w1, st) < 0) return -1;
    _Float16* h1 = reinterpret_cast<_Float16*>(tmp1);
    _Float16* h2 = reinterpret_cast<_Float16*>(tmp2);
    const Half16 g{h1, fmid, nullptr}, u{h2, fmid, h1};
    if (run_gemm(x, *w1, Out{nullptr, fmid, &g}, Epi::gate_of(epi), st, &pre) ||
        run_gemm(x, *w3, Out{nullptr, fmid, &u}, Epi::mul(nullptr, fmid), st, &pre))  // the multiplier: u.aux, fp16
      return -1;
    A16 d;
    d.p = h2;
    d.ld = fmid;
    d.kp = fmid;
    return run_gemm(Act{h2, kActF16, fmid, m, fmid}, *w2, down, Epi{}, st, &d);
  }
  if (nad_device_ffn_gate_up(act, act_dtype, w1p, w3p, tmp1, tmp2, m, fin, fmid, lda, epi, queue)) return -1;
  const Act t{tmp2, kActF32, fmid, m, fmid};
  if (is_q6k(*w2)) return forward_q6k(t, *w2, down, Epi{}, st);
  if (w2->mins) return forward_min(t, *w2, down, Epi{}, st);
  if (m <= kSkinnyMaxM) return run_skinny(t, One(*w2, down), Epi{}, st);
  return run_gemm(t, *w2, down, Epi{}, st);
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
    if (is_q6k(*w)) {  // the batched GEMV streams the int4 / int2 tile layouts only
      set_err("nad_batch_create: problem %d's weight is GGUF Q6_K, which is not batched", i);
      return nullptr;
    }
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
  if (!prepare_gemv(b->a, b->waves, b->grid, Act{p[0].act, kActF32, w0->k, 1, w0->k}, One(*w0, Out{p[0].out, w0->n}),
                    Epi{}) ||
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
  if (planning()) {  // nad_plan_batch_only: geometry-only weights, no table; nad_batch_run only records
    b->a.batch = stand_in<const GemvBatchEnt>(kStandTable);
    return b;
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
  return launch_gemv_named(planned(NAD_KERNEL_GEMV_M1, b->grid, b->waves * 64), "nad_batch_run:", [&] {
           return launch_gemv_batch(b->a, b->bits, b->waves, b->grid, b->lds, static_cast<hipStream_t>(queue));
         })
             ? 0
             : -1;
}

extern "C" void nad_batch_destroy(void* batch) {
  NadBatch* b = static_cast<NadBatch*>(batch);
  if (!b) return;
  if (b->dev) (void)hipFree(b->dev);
  delete b;
}
