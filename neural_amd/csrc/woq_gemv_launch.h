// woq_gemv_launch.h -- host side of the decode GEMV (woq_gemv.h): the launch's slice geometry, the register-stage
// depth, and the ladders that turn a launch's runtime arguments into the template arguments of one instantiation.
// Everything here is static or a template: each woq_gemv*.hip object instantiates, through the launchers it defines,
// only its own kernels (woq_kernels.h lists the launchers and their objects).
#pragma once
#include <climits>
#include <type_traits>

#include "woq_gemv.h"
#include "woq_launch.h"

namespace nad {

// ------------------------------------------------------------------------------------------------ M = 1 geometry
static int lean_ks(const GemvArgs& a) { return a.lean_ks == 1 || a.lean_ks == 2 ? a.lean_ks : KS; }
// K-slices per wave staged: 1 for the narrow-slice launches (exactly one slice per wave: a second would only be a
// dead out-of-range activation load in front of the weights), 4 for long K, else 2
static int lean_spw(const GemvArgs& a) { return a.lean_spw == 4 ? 4 : (a.lean_spw == 1 ? 1 : 2); }

static bool lean_ok(const GemvArgs& a, int bits, int waves) {
  int tpg = 0;
  const int ks = lean_ks(a);
  const int nsl = (a.nt + ks - 1) / ks;
  const int gpt = gemv_groups_per_tile(bits, a.nt, a.ng, a.bs, &tpg);
  const bool inst = bits == 4 ? (gpt == 1 || gpt == 2) : (bits == 2 && (gpt == 1 || gpt == 2 || (gpt == 4 && !a.asym)));
  return a.lean && a.M == 1 && inst && a.a_fast && nsl <= waves * lean_spw(a);
}

// the most (stripe, K-slice) stages any wave of a single-problem launch streams
static int m1_stages_per_wave(const GemvArgs& a, int ksn, int waves) {
  const int nsl = (a.nt + ksn - 1) / ksn;
  return (a.u_q + (a.u_r ? 1 : 0)) * (a.dual ? 2 : 1) * ((nsl + waves - 1) / waves);
}
// register stages per wave of an M = 1 launch (NST of m1_body: the measurements are there); NAD_GEMV_NST overrides
static int m1_nst(const GemvArgs& a, int ksn, int waves) {
  if (a.m1_nst == 1 || a.m1_nst == 2) return a.m1_nst;
  const int spw = m1_stages_per_wave(a, ksn, waves);
  return spw >= 7 || (ksn == 1 && spw >= 4) ? 2 : 1;
}

// ------------------------------------------------------------------------------------------------ launch statements
// the launch's runtime activation type / symmetry as the compile-time argument of f
template <int V>
using IntC = std::integral_constant<int, V>;
template <class F>
static auto by_act(const GemvArgs& a, F f) {
  if (a.act_t == kActF32) return f(IntC<kActF32>{});
  if (a.act_t == kActF16) return f(IntC<kActF16>{});
  return f(IntC<kActBF16>{});
}
template <class F>
static auto by_asym(const GemvArgs& a, F f) {
  return a.asym ? f(std::true_type{}) : f(std::false_type{});
}

// Every launch of the three forward kernels goes through here with its template arguments packed (gemv_inst): in a dry
// run the statement that would have launched names its kernel instead (gemv_named).
template <auto K, class... Args>
static hipError_t gemv_issue(uint32_t inst, dim3 g, dim3 b, size_t lds, hipStream_t st, const Args&... args) {
  return gemv_named(inst) ? hipSuccess : launch_big_lds<K>(g, b, lds, st, args...);
}

// ------------------------------------------------------------------------------------------------ woq_gemv_kernel
template <int BITS, int HILO, int GPT, bool ASYM>
static hipError_t gemv_launch4(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  const int spw = m1_stages_per_wave(a, KS, int(b.x / 64));
  const int nst = a.m1_nst == 1 ? 1 : (a.m1_nst == 3 ? 3 : (spw <= 2 ? 1 : 3));
  constexpr auto inst = [](int n) { return gemv_inst(1, BITS, GPT, ASYM, HILO, 0, 0, n, -1, false, 0, 0, false); };
  return nst == 1 ? gemv_issue<woq_gemv_kernel<BITS, HILO, GPT, ASYM, 1>>(inst(1), g, b, lds, st, a)
                  : gemv_issue<woq_gemv_kernel<BITS, HILO, GPT, ASYM, 3>>(inst(3), g, b, lds, st, a);
}

// ------------------------------------------------------------------------------------------------ woq_gemv_m1_kernel
template <int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, int ST>
static hipError_t gemv_m1_launch5(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  constexpr auto inst = [](bool batch, int n) {
    return gemv_inst(2, BITS, GPT, ASYM, AT, KSN, SPW, n, ST, batch, 0, 0, false);
  };
  if (a.batch)
    return gemv_issue<woq_gemv_m1_kernel<BITS, GPT, AT, ASYM, KSN, SPW, true, NAD_M1_BATCH_NST, ST>>(
        inst(true, NAD_M1_BATCH_NST), g, b, lds, st, a);
  return m1_nst(a, KSN, int(b.x / 64)) == 1
             ? gemv_issue<woq_gemv_m1_kernel<BITS, GPT, AT, ASYM, KSN, SPW, false, 1, ST>>(inst(false, 1), g, b, lds, st, a)
             : gemv_issue<woq_gemv_m1_kernel<BITS, GPT, AT, ASYM, KSN, SPW, false, 2, ST>>(inst(false, 2), g, b, lds, st, a);
}
// int2: the scale type as a template parameter (3 x the int2 instantiations; int4 keeps the runtime form)
#ifndef NAD_INT2_ST
#define NAD_INT2_ST 1
#endif
template <int BITS, int GPT, int AT, bool ASYM, int ST = -1>
static hipError_t gemv_m1_launch4(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if constexpr (BITS == 2 && ST < 0 && NAD_INT2_ST) {
    if (a.scale_t == kScaleF32) return gemv_m1_launch4<BITS, GPT, AT, ASYM, kScaleF32>(a, g, b, lds, st);
    if (a.scale_t == kScaleBF16) return gemv_m1_launch4<BITS, GPT, AT, ASYM, kScaleBF16>(a, g, b, lds, st);
    return gemv_m1_launch4<BITS, GPT, AT, ASYM, kScaleF16>(a, g, b, lds, st);
  } else {
    if (a.lean_ks == 1) return gemv_m1_launch5<BITS, GPT, AT, ASYM, 1, 1, ST>(a, g, b, lds, st);
    if (a.lean_ks == 2) return gemv_m1_launch5<BITS, GPT, AT, ASYM, 2, 1, ST>(a, g, b, lds, st);
    return a.lean_spw == 4 ? gemv_m1_launch5<BITS, GPT, AT, ASYM, KS, 4, ST>(a, g, b, lds, st)
                           : gemv_m1_launch5<BITS, GPT, AT, ASYM, KS, 2, ST>(a, g, b, lds, st);
  }
}
// int4 / int2 with one group per tile or 2 per tile; int2 also 4 per tile (sym only, as the general kernel).  The
// int4 instantiations are woq_gemv.hip's (gemv_m1_launch), the int2 ones (3 scale types each) woq_gemv_b2.hip's
// (gemv_m1_launch_b2), so that the two compile in parallel.
template <int BITS, int GPT>
static hipError_t gemv_m1_launch2(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  return by_act(a, [&](auto at) {
    return by_asym(a, [&](auto as) { return gemv_m1_launch4<BITS, GPT, at.value, as.value>(a, g, b, lds, st); });
  });
}

// ------------------------------------------------------------------------------------------------ woq_gemv_m1s_kernel
// Its instantiations are their own objects (woq_gemv_s2.hip: int4, woq_gemv_s3.hip: int2) next to the general ones;
// gemv_m1s_launch_b{4,2} return false where no instantiation serves the launch -- any epilogue but {none, SiLU*mul},
// two weights, a batch, and the geometries left out below -- and woq_gemv_m1_kernel takes it.  Where they return true
// the launch was issued (or, in a dry run, named) and e is its status.
template <int NWT>
static GemvM1Rest<NWT> m1s_rest(const GemvArgs& a) {
  GemvM1Rest<NWT> c{};
  c.part_off = a.part_off;
  c.dq_mask = a.dq_mask;
  c.dq_magic = a.dq_magic;
  c.sb1 = a.stripe_base[1];
  c.sb2 = a.stripe_base[2];
  for (int i = 0; i < NWT; i++) {
    const SkinnyWeight& w = a.w[i];
    c.ns[i] = w.ns;
    c.zps[i] = w.zps;
    c.n[i] = w.n;
    c.out[i] = w.out;
  }
  c.tiles2 = NWT > 2 ? a.w[2].tiles : nullptr;
  c.scales2 = NWT > 2 ? a.w[2].scales : nullptr;
  c.aux = a.aux;
  return c;
}
// whether the launch fits the packed leading parameters (field widths of uqr / geom, one stripe count for the pair)
static bool m1s_packable(const GemvArgs& a, int nwt, int waves) {
  if (a.u_q < 0 || a.u_q > 0xFFFF || a.u_r < 0 || a.u_r > 0xFFFF) return false;
  if (a.nt >= (1 << kM1GeomNgShift) || a.ng >= (1 << (kM1GeomTpgShift - kM1GeomNgShift))) return false;
  if (a.tpg_shift < 0 || a.tpg_shift > 31 || a.scale_t < 0 || a.scale_t > 3 || waves > 16) return false;
  return nwt != 2 || a.w[0].ns == a.w[1].ns;
}
template <int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, int NST, int ST, int NWT, int NSC, bool AHEAD = false>
static hipError_t m1s_go(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  const int esz = a.act_t == kActF32 ? 4 : 2;
  const uint32_t uqr = uint32_t(a.u_q) | uint32_t(a.u_r) << 16;
  const uint32_t geom = uint32_t(a.nt) | uint32_t(a.ng) << kM1GeomNgShift | uint32_t(a.tpg_shift) << kM1GeomTpgShift |
                        uint32_t(a.scale_t) << kM1GeomScaleShift | uint32_t(b.x / 64) << kM1GeomWavesShift;
  return gemv_issue<woq_gemv_m1s_kernel<BITS, GPT, AT, ASYM, KSN, SPW, NST, ST, NWT, NSC, AHEAD>>(
      gemv_inst(3, BITS, GPT, ASYM, AT, KSN, SPW, NST, ST, false, NWT, NSC, AHEAD), g, b, lds, st, a.A, a.w[0].tiles,
      a.w[0].scales, NWT > 1 ? a.w[1].tiles : nullptr, NWT > 1 ? a.w[1].scales : nullptr, a.K * esz, uqr, geom,
      a.w[0].ns, m1s_rest<NWT>(a));
}
// weights of the launch as woq_gemv_m1s_kernel's NWT (0: not served)
static int m1s_nwt(const GemvArgs& a, int waves) {
  if (a.batch || !a.m1_spec) return 0;
  int nwt = 0;
  if (a.dual) {
    nwt = a.epi == kEpiSiluMul ? 2 : 0;
  } else if (a.epi == kEpiNone) {
    const int nw = 1 + (a.stripe_base[1] != INT_MAX ? 1 : 0) + (a.stripe_base[2] != INT_MAX ? 1 : 0);
    nwt = nw == 1 || nw == 3 ? nw : 0;
  }
  return nwt != 0 && m1s_packable(a, nwt, waves) ? nwt : 0;
}
// The load-ahead order of m1_stream (AHEAD) exists for the launches of a decode token that run one register stage and
// stream two or more stages per wave -- int4, one group per tile, fp32 activations, sym and asym:
//   form 1 / 2 / 3   16 waves of one 2-tile slice each, 1 weight / the {gate, up} pair / 3 weights (fused QKV)
// in an object of their own (woq_gemv_s6.hip).  The form for Llama's down projection (11 waves of two 4-tile slices)
// was built and measured and did not gain inside the token: down keeps the present order.
// m1s_ahead_form: the form that serves the launch, 0 = none, or switched off (NAD_GEMV_AHEAD=0: kM1SpecAhead clear).
static int m1s_ahead_form(const GemvArgs& a, int bits, int gpt, int waves) {
  if (bits != 4 || gpt != 1 || a.act_t != kActF32 || !(a.m1_spec & kM1SpecAhead)) return 0;
  const int ks = lean_ks(a), nwt = m1s_nwt(a, waves);
  if (nwt == 0 || m1_nst(a, ks, waves) != 1 || m1_stages_per_wave(a, ks, waves) < 2) return 0;
  const int nsl = (a.nt + ks - 1) / ks;
  return ks == 2 && waves == 16 && nsl >= 16 ? nwt : 0;
}
// Instantiated: slices of 1 or 2 tiles, one per wave: every weight count, 16 slots per column or the runtime count,
// two register stages for one weight only (lm_head); 4-tile slices with fewer than 16 slots per column: two per wave
// for every weight count (two stages: one weight), four per wave for one weight (the long K of a down projection) --
// the runtime count, and for one weight the two counts the down projections of the token run at: 11 (Llama, K = 11008:
// two slices per wave) and 7 (Mistral, K = 14336: four).
template <int BITS, int GPT, int AT, bool ASYM, int ST>
static bool m1s_launch3(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e) {
  const int waves = int(b.x / 64), ks = lean_ks(a), nwt = m1s_nwt(a, waves);
  if (nwt == 0) return false;
  const int nsl = (a.nt + ks - 1) / ks;
  const bool l16 = waves == 16 && nsl >= 16;
  const int nst = m1_nst(a, ks, waves);
  if (const int form = m1s_ahead_form(a, BITS, GPT, waves)) {
    e = gemv_m1s_ahead_launch(a, form, g, b, lds, st);
    return true;
  }
#define NAD_M1S(KSN, SPW, NST, NWT, NSC)                                                  \
  do {                                                                                    \
    e = m1s_go<BITS, GPT, AT, ASYM, KSN, SPW, NST, ST, NWT, NSC>(a, g, b, lds, st);       \
    return true;                                                                          \
  } while (0)
#define NAD_M1S_NARROW(KSN)                               \
  do {                                                    \
    if (nst == 1) {                                       \
      if (nwt == 1 && l16) NAD_M1S(KSN, 1, 1, 1, 16);     \
      if (nwt == 1) NAD_M1S(KSN, 1, 1, 1, 0);             \
      if (nwt == 2 && l16) NAD_M1S(KSN, 1, 1, 2, 16);     \
      if (nwt == 2) NAD_M1S(KSN, 1, 1, 2, 0);             \
      if (nwt == 3 && l16) NAD_M1S(KSN, 1, 1, 3, 16);     \
      if (nwt == 3) NAD_M1S(KSN, 1, 1, 3, 0);             \
    } else if (nwt == 1) {                                \
      if (l16) NAD_M1S(KSN, 1, 2, 1, 16);                 \
      NAD_M1S(KSN, 1, 2, 1, 0);                           \
    }                                                     \
    return false;                                         \
  } while (0)
  if (ks == 1) NAD_M1S_NARROW(1);
  if (ks == 2) NAD_M1S_NARROW(2);
  if (l16 || (GPT != 1 && waves > 8)) return false;
  if (lean_spw(a) == 4) {
    if (nwt == 1 && nst == 1 && waves == 7 && nsl >= 7) NAD_M1S(KS, 4, 1, 1, 7);
    if (nwt == 1 && nst == 1) NAD_M1S(KS, 4, 1, 1, 0);
    return false;
  }
  if (nst == 1) {
    if constexpr (GPT == 1) {  // 11 waves: groups of a whole tile or coarser only
      if (nwt == 1 && waves == 11 && nsl >= 11) NAD_M1S(KS, 2, 1, 1, 11);
    }
    if (nwt == 1) NAD_M1S(KS, 2, 1, 1, 0);
    if (nwt == 2) NAD_M1S(KS, 2, 1, 2, 0);
    NAD_M1S(KS, 2, 1, 3, 0);
  }
  if (nwt == 1) NAD_M1S(KS, 2, 2, 1, 0);
  return false;
#undef NAD_M1S_NARROW
#undef NAD_M1S
}

// ------------------------------------------------------------------------------------------------ routed M = 1
// woq_gemv_m1_routed_kernel.  fp32 activations only; the K-slice geometry is that of the expert's own one-problem
// launch (a.lean_ks / a.lean_spw as prepared for it), so a stripe's sums are the same whichever launch serves it.  Two
// register stages per wave throughout: a routed problem's workgroups stream from a few stages per wave (one token,
// the chip's workgroups dealt out over top_k problems) to dozens (several rows), where m1_nst would take two and the
// batched launch three; one depth keeps the instantiations (their own objects: woq_gemv_r4.hip int4, woq_gemv_r5.hip
// int2) at a quarter of woq_gemv_m1_kernel's.
constexpr int kRoutedNst = 2;
template <int BITS, int GPT, bool ASYM, int ST>
static hipError_t routed_launch2(const GemvArgs& a, const GemvRouted& r, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (a.lean_ks == 1)
    return launch_big_lds<woq_gemv_m1_routed_kernel<BITS, GPT, ASYM, 1, 1, kRoutedNst, ST>>(g, b, lds, st, a, r);
  if (a.lean_ks == 2)
    return launch_big_lds<woq_gemv_m1_routed_kernel<BITS, GPT, ASYM, 2, 1, kRoutedNst, ST>>(g, b, lds, st, a, r);
  return a.lean_spw == 4
             ? launch_big_lds<woq_gemv_m1_routed_kernel<BITS, GPT, ASYM, KS, 4, kRoutedNst, ST>>(g, b, lds, st, a, r)
             : launch_big_lds<woq_gemv_m1_routed_kernel<BITS, GPT, ASYM, KS, 2, kRoutedNst, ST>>(g, b, lds, st, a, r);
}

}  // namespace nad
