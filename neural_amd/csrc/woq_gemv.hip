// woq_gemv.hip -- the decode GEMV's entry points (launch_gemv, launch_gemv_batch, launch_gemv_dual), its launch
// geometry, the dry runs' naming, and the instantiations of woq_gemv_kernel, the int4 woq_gemv_m1_kernel and
// woq_gemv_m1_dual_kernel.  The other instantiations are woq_gemv_{b2,s2,s3,s6,r4,r5,r7}.hip's, compiled in parallel.
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

static thread_local uint32_t t_named = 0;
static thread_local bool t_naming = false;
void gemv_name_begin() {
  t_naming = true;
  t_named = 0;
}
uint32_t gemv_name_end() {
  t_naming = false;
  return t_named;
}
bool gemv_named(uint32_t inst) {
  if (t_naming) t_named = inst;
  return t_naming;
}

static hipError_t gemv_m1_launch(const GemvArgs& a, int bits, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (bits == 4) {
    if (gpt == 1) return gemv_m1_launch2<4, 1>(a, g, b, lds, st);
    if (gpt == 2) return gemv_m1_launch2<4, 2>(a, g, b, lds, st);
    return hipErrorInvalidValue;
  }
  return gemv_m1_launch_b2(a, gpt, g, b, lds, st);
}

// Instantiated: groups of >= KT (GPT 1), KT/2 (GPT 2) and KT/4 (GPT 4), sym and asym.  Finer groups fall back to
// woq_skinny_kernel.
template <int BITS, int HILO>
static hipError_t gemv_launch2(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  constexpr int SPT = k_tile(BITS) / 32;
  return by_asym(a, [&](auto as) {
    if (gpt == 1) return gemv_launch4<BITS, HILO, 1, as.value>(a, g, b, lds, st);
    if (gpt == 2) return gemv_launch4<BITS, HILO, 2, as.value>(a, g, b, lds, st);
    if constexpr (SPT % 4 == 0) {
      if (gpt == 4) return gemv_launch4<BITS, HILO, 4, as.value>(a, g, b, lds, st);
    }
    return hipError_t(hipErrorInvalidValue);
  });
}

template <int BITS>
static hipError_t gemv_launch1(const GemvArgs& a, int hilo, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (hilo == 0) return gemv_launch2<BITS, 0>(a, gpt, g, b, lds, st);
  if (hilo == 1) return gemv_launch2<BITS, 1>(a, gpt, g, b, lds, st);
  return gemv_launch2<BITS, 2>(a, gpt, g, b, lds, st);
}

// LDS layout (and its size) of one launch: activation rows, then the partial-sum slots [nv][waves][M][16]
size_t gemv_lds_layout(GemvArgs& a, int bits, int waves, int grid) {
  if (lean_ok(a, bits, waves)) {  // the M = 1 kernels: per-wave rows, then the partial slots [nv][16 columns][waves]
    const int upw = (a.units + grid - 1) / grid;
    a.part_off = waves * lean_wave_lds(bits, lean_ks(a), lean_spw(a));
    // ... with room for the slot stride of woq_gemv_m1s_kernel's fixed counts: the waves rounded up to 4
    return size_t(a.part_off) + size_t(upw) * (a.dual ? 2 : 1) * ((waves + 3) & ~3) * 16 * 4;
  }
  const int R = a.act_t == kActF16 ? a.M : 2 * a.M;
  const size_t kp = size_t(a.nt) * tile_k(bits);
  const size_t abytes = (size_t(R) + 1) * kp * 2;
  const int upw = (a.units + grid - 1) / grid;  // max units per workgroup
  const size_t nv = size_t(upw) * (a.dual ? 2 : 1);
  a.part_off = int((abytes + 15) & ~size_t(15));
  return size_t(a.part_off) + nv * waves * a.M * 16 * 4;
}

// waves per workgroup: balanced K-slices per wave, at most 16 (8 for groups finer than a K tile)
int gemv_waves(int bits, int nt, int ng, int bs) {
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(bits, nt, ng, bs, &tpg);
  const int maxw = gpt > 1 ? 8 : 16;
  const int nsl = (nt + KS - 1) / KS;
  const int spw = (nsl + maxw - 1) / maxw;  // slices per wave
  return (nsl + spw - 1) / spw;
}

void gemv_lean_slices(GemvArgs& a, int bits, int* waves, int ks_pref) {
  a.lean_ks = KS;
  a.lean_spw = 2;
  if (a.M == 1 && a.lean && (a.nt + KS - 1) / KS > 2 * *waves) {  // long K: up to 4 slices per wave
    a.lean_spw = 4;
    if (!lean_ok(a, bits, *waves)) a.lean_spw = 2;
    return;
  }
  // Slices of 1 or 2 tiles, one per wave, up to 16 waves (the narrowest width that fits).  bench (graph-replayed
  // token): 2-tile slices took Llama int4 g128 837 -> 853 tok/s and the Mistral int2 policy 586 -> 633 (its int2
  // K = 4096 launches from 4 waves to 8).  NAD_GEMV_KS: 2 = 1- or 2-tile, 3 = 2-tile only, 4 = 4-tile everywhere.
  if ((ks_pref != 2 && ks_pref != 3) || a.M != 1 || !a.lean) return;
  const int ks = a.nt <= 16 && ks_pref == 2 ? 1 : 2;
  const int nsl = (a.nt + ks - 1) / ks;
  if (nsl > 16 || nsl <= *waves) return;  // narrow slices only where each wave gets one and there are more waves
  if (!lean_ok(a, bits, *waves)) return;  // the 4-tile launch would not take the M = 1 kernel either
  a.lean_ks = ks;
  a.lean_spw = 1;  // one slice per wave
  if (!lean_ok(a, bits, nsl)) {
    a.lean_ks = KS;
    a.lean_spw = 2;
    return;
  }
  *waves = nsl;
}

int gemv_groups_per_tile(int bits, int nt, int ng, int bs, int* tpg) {
  const int KT = tile_k(bits);
  if (ng == 1) {
    *tpg = 0;  // one group: ends only at the last tile
    return 1;
  }
  if (bs % KT == 0) {
    *tpg = bs / KT;
    return (*tpg & (*tpg - 1)) == 0 ? 1 : 0;  // power-of-two tiles per group
  }
  if (KT % bs == 0 && bs % 32 == 0) {
    *tpg = 1;
    const int g = KT / bs;
    return (g == 2 || g == 4) ? g : 0;
  }
  return 0;
}

bool gemv_uses_m1(const GemvArgs& a, int bits, int waves) { return lean_ok(a, bits, waves); }

bool gemv_dual_ok(const GemvArgs& a, int bits_a, const GemvArgs& b, int bits_b, int waves) {
  int tpg = 0;
  const int ga = gemv_groups_per_tile(bits_a, a.nt, a.ng, a.bs, &tpg), gb = gemv_groups_per_tile(bits_b, b.nt, b.ng, b.bs, &tpg);
  const bool pair = bits_a == 2 && bits_b == 4 && ((ga == 4 && gb == 2) || (ga == 2 && gb == 1));
  return pair && !a.asym && !b.asym && a.lean_ks == 1 && b.lean_ks == 2 && a.act_t == kActF32 && b.act_t == kActF32 &&
         waves == 16 && lean_ok(a, bits_a, waves) && lean_ok(b, bits_b, waves);
}

hipError_t launch_gemv_dual(const GemvArgs& a, const GemvArgs& b, int ga, int gb, int waves, size_t lds,
                            hipStream_t stream) {
  int tpg = 0;
  const int g1 = gemv_groups_per_tile(2, a.nt, a.ng, a.bs, &tpg);
  const dim3 g(ga + gb), blk(waves * 64);
  if (g1 == 4)  // groups of 64
    return launch_big_lds<woq_gemv_m1_dual_kernel<2, 4, 1, 4, 2, 2, kActF32>>(g, blk, lds, stream, a, b, ga);
  return launch_big_lds<woq_gemv_m1_dual_kernel<2, 2, 1, 4, 1, 2, kActF32>>(g, blk, lds, stream, a, b, ga);  // of 128
}

hipError_t launch_gemv_batch(const GemvArgs& a, int bits, int waves, int grid, size_t lds, hipStream_t stream) {
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(bits, a.nt, a.ng, a.bs, &tpg);
  if (gpt == 0 || !a.batch || a.batch_wpp <= 0 || !lean_ok(a, bits, waves)) return hipErrorInvalidValue;
  return gemv_m1_launch(a, bits, gpt, dim3(grid), dim3(waves * 64), lds, stream);
}

hipError_t launch_gemv(const GemvArgs& a, int bits, int waves, int grid, size_t lds, hipStream_t stream) {
  const int hilo = a.act_t == kActF16 ? 0 : (a.M <= 8 ? 1 : 2);
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(bits, a.nt, a.ng, a.bs, &tpg);
  if (gpt == 0) return hipErrorInvalidValue;
  dim3 g(grid), b(waves * 64);
  if (lean_ok(a, bits, waves)) {
    hipError_t e = hipSuccess;
    if (bits == 4 ? gemv_m1s_launch_b4(a, gpt, g, b, lds, stream, e) : gemv_m1s_launch_b2(a, gpt, g, b, lds, stream, e))
      return e;
    return gemv_m1_launch(a, bits, gpt, g, b, lds, stream);
  }
  if (bits == 4) return gemv_launch1<4>(a, hilo, gpt, g, b, lds, stream);
  if (bits == 2) return gemv_launch1<2>(a, hilo, gpt, g, b, lds, stream);
  return gemv_launch1<8>(a, hilo, gpt, g, b, lds, stream);
}

}  // namespace nad

#ifdef NAD_PHASE_TRACE
extern "C" int nad_trace_clock_khz() {
  int dev = 0, khz = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return -1;
  return khz;
}

extern "C" int nad_trace_fetch(void* host, size_t bytes, int clear, int grid_filter) {
  (void)grid_filter;
  const size_t n = sizeof(nad::nad_trace_buf) < bytes ? sizeof(nad::nad_trace_buf) : bytes;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (host && hipMemcpyFromSymbol(host, HIP_SYMBOL(nad::nad_trace_buf), n) != hipSuccess) return -1;
  if (clear) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(nad::nad_trace_buf)) != hipSuccess) return -1;
    if (hipMemset(p, 0, sizeof(nad::nad_trace_buf)) != hipSuccess) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
  }
  return 0;
}
#endif
