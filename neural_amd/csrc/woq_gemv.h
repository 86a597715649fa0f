// woq_gemv.h -- the decode (M <= 16) weight-only-quantized GEMV for gfx950: a persistent stripe stream.  The device
// code: every kernel template and what they are made of.  woq_gemv_launch.h holds the host helpers that pick an
// instantiation, and one woq_gemv*.hip per object instantiates its share (woq_kernels.h lists which).
//
// Replaces GEMVWrapper::gemv_kblock -> gemv_{4,2}bit_fp32_fp32 (bestla/bestla/bestla_wrapper.h:364-468,
// bestla/bestla/kernel_ref.h:2489-2531,2712-2760) and the fused QKV / FFN-gate-up decode launches
// (neural_speed/core/layers/ip_fusion_qkv.cpp:22-93, ip_fusion_ffn.cpp:407-457).
//
// Shape of the work.  A launch streams `units` stripes (16 output columns x all of K; for the dual SiLU*mul / GELU*mul
// epilogue a unit is the pair {gate stripe s, up stripe s}).  The grid is sized to the chip (one workgroup per CU),
// each workgroup owns a contiguous, balanced run of whole units, and its waves split the run's concatenated 1 KiB tiles
// evenly -- a wave's range may cross stripe boundaries.
//
// What the measurements on MI355X (tools/gemv_sweep.py, tools/hbm_probe.hip) shaped:
//   * a launch of this size is dominated by fixed costs, not arithmetic: everything before the first weight load and
//     every instruction executed once per launch shows up directly in the time.  So the prologue issues the
//     activation, scale and weight loads back to back with no waits in between, all bookkeeping is wave-uniform SALU
//     work (a cursor advanced per tile, the weight / stripe re-derived only at stripe boundaries), and the weight loads
//     are raw buffer loads that are never predicated -- tiles past a wave's range get an out-of-range offset, which
//     returns zeros without touching memory -- so every pipeline stage has the same vmcnt footprint and hipcc waits for
//     exactly one stage instead of draining the queue at control-flow joins;
//   * the activations are staged into LDS once per workgroup as MFMA-ready fp16 rows (fp32/bf16 inputs split
//     hi = fp16(a), lo = fp16(a - hi) so the products are fp32-accurate; the act-order gather of
//     ShuffleActivationKBlock, bestla_prologue_a.h:407-422, is applied while staging), and the workgroup's group scales
//     loads of each stage are issued with it (one dword per tile: L2-merged 32 B rows);
//   * wave w owns K-slices w, w + NW, ... (KS = 4 tiles) of every stripe in the run: a pipeline stage is one
//     (stripe, slice) -- four loads at immediate offsets from one base -- and NST stages are in flight per wave
//     (register ring, 1 or 3 chosen per launch: see NST below), the stage being computed the oldest;
//   * int4 dequantization takes 1 shift + 4 v_and_or + 4 packed fp16 ops per 8 weights (the 0x6400 magic makes
//     1024 + q and 1024 + 16 q exact fp16 without per-nibble shifts), then one
//     v_mfma_f32_16x16x32_f16 with the activation rows in the A operand; the group scale multiplies an fp32 group
//     accumulator once per group, so the weights are dequantized exactly;
//   * a wave's partial sum per stripe goes to an LDS slot; after ONE barrier the workgroup sums the slots of each
//     stripe in wave order (deterministic, no atomics) and applies the fused epilogue.
// HBM-bound by design: weights + scales are read exactly once; the only other traffic is A (L2-resident) once per WG.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "woq_device.h"
#include "woq_kernels.h"

namespace nad {

// ------------------------------------------------------------------------------------------------ phase trace
// Development instrumentation (make trace -> libneural_amd_trace.so): per-workgroup wall-clock stamps of the
// GEMV kernel's phases, read back with nad_trace_fetch().  Compiled out of the product library.
#ifdef NAD_PHASE_TRACE
constexpr int kTraceSlots = 8, kTraceMaxWg = 16384;
__device__ unsigned long long nad_trace_buf[kTraceSlots][kTraceMaxWg];
#define NAD_TRACE(slot)                                                                       \
  do {                                                                                        \
    if (threadIdx.x == 0 && blockIdx.x < kTraceMaxWg) nad_trace_buf[slot][blockIdx.x] = wall_clock64(); \
  } while (0)
#define NAD_TRACE_MAX(slot)                                                                               \
  do {                                                                                                    \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < kTraceMaxWg)                                              \
      atomicMax(&nad_trace_buf[slot][blockIdx.x], (unsigned long long)wall_clock64());                    \
  } while (0)
#else
#define NAD_TRACE(slot) \
  do {                  \
  } while (0)
#define NAD_TRACE_MAX(slot) \
  do {                      \
  } while (0)
#endif

// virtual stripe -> (weight index, stripe within that weight); all wave-uniform
__device__ __forceinline__ void vstripe(const GemvArgs& a, int v, int& w, int& s) {
  if (a.dual) {
    w = v & 1;
    s = v >> 1;
  } else {
    w = (v >= a.stripe_base[1] ? 1 : 0) + (v >= a.stripe_base[2] ? 1 : 0);
    s = v - (w == 0 ? 0 : (w == 1 ? a.stripe_base[1] : a.stripe_base[2]));
  }
}

template <class T>
__device__ __forceinline__ T sel3(int w, T x0, T x1, T x2) {
  return w == 0 ? x0 : (w == 1 ? x1 : x2);
}

// ------------------------------------------------------------------------------------------------ weight stream
// Wave w owns the K-slices q = w, w + NW, w + 2 NW, ... (KS consecutive tiles each) of EVERY stripe of the workgroup's
// run, visited stripe-major.  One pipeline stage is one (stripe, slice): KS tile loads at immediate offsets from one
// stripe base, plus the slice's group scales / zero points -- a few SALU ops per stage, nothing per tile.
constexpr int KS = 4;

struct StageCursor {
  int j, q;                      // local virtual stripe, K-slice
  int s;                         // stripe within its weight
  __amdgpu_buffer_rsrc_t rt, rs, rz;
};

__device__ __forceinline__ void cursor_stripe(const GemvArgs& a, StageCursor& c, int v0) {
  int w, s;
  vstripe(a, v0 + c.j, w, s);
  const int ns = sel3(w, a.w[0].ns, a.w[1].ns, a.w[2].ns);
  const int ssz = a.scale_t == kScaleF32 ? 4 : 2;
  c.s = s;
  c.rt = rsrc(sel3(w, a.w[0].tiles, a.w[1].tiles, a.w[2].tiles), ns * a.nt * 1024);
  c.rs = rsrc(sel3(w, a.w[0].scales, a.w[1].scales, a.w[2].scales), ns * a.ng * 16 * ssz);
  c.rz = rsrc(sel3(w, a.w[0].zps, a.w[1].zps, a.w[2].zps), ns * a.ng * 16);
}

template <int GPT, int KSN = KS>
struct StageRegs {
  u4_t b[KSN];
  uint32_t sc[KSN][GPT];  // raw scale bits (the dword holding this lane's 16-bit scale, or the f32)
  int zp[KSN][GPT];
};

#ifndef NAD_TILE_AUX
#define NAD_TILE_AUX 2  // non-temporal: the weights are read once per token
#endif
// The loads of the stage at the cursor: KSN tiles at immediate offsets from one stripe base, each with its GPT group
// scales (+ zero points).  Never predicated: tiles and groups past the end of K -- and, with `on` false, the whole
// stage -- take the out-of-range offset.  Shared by both stage loaders below.
template <bool ASYM, int GPT, int KSN, class Args>
__device__ __forceinline__ void stage_loads(const Args& a, StageRegs<GPT, KSN>& S, const StageCursor& c, bool on,
                                            int lane, int vs) {
  const int nt = a.nt, ng = a.ng;
  const int t0 = c.q * KSN;
  const int tb = (c.s * nt + t0) * 1024;
  const int rowb = a.scale_t == kScaleF32 ? 64 : 32;  // bytes per scale row of 16
#pragma unroll
  for (int i = 0; i < KSN; i++) {
    const bool live = on && t0 + i < nt;
    S.b[i] = __builtin_bit_cast(u4_t, __builtin_amdgcn_raw_buffer_load_b128(c.rt, (live ? tb + i * 1024 : kOOB) + lane * 16, 0, NAD_TILE_AUX));
#pragma unroll
    for (int g = 0; g < GPT; g++) {
      const int grp = GPT == 1 ? ((t0 + i) >> a.tpg_shift) : (t0 + i) * GPT + g;
      const bool gl = live && (GPT == 1 || grp < ng);
      const int row = c.s * ng + grp;
      S.sc[i][g] = __builtin_amdgcn_raw_buffer_load_b32(c.rs, (gl ? row * rowb : kOOB) + vs, 0, 0);
      if constexpr (ASYM)
        S.zp[i][g] = int(int8_t(__builtin_amdgcn_raw_buffer_load_b8(c.rz, (gl ? row * 16 : kOOB) + (lane & 15), 0, 0)));
      else
        S.zp[i][g] = 0;
    }
  }
}

// Issue one stage's loads, then advance.  Two-armed: a past-the-end stage issues the same loads, all out of range.
template <int GPT, bool ASYM, int KSN = KS>
__device__ __forceinline__ void load_stage(const GemvArgs& a, StageRegs<GPT, KSN>& S, StageCursor& c, int nv, int nsl,
                                           int wave, int NW, int v0, int lane, int vs) {
  if (c.j >= nv) {  // past this wave's last stage: the same loads, all out of range, no bookkeeping
#pragma unroll
    for (int i = 0; i < KSN; i++) {
      S.b[i] = __builtin_bit_cast(u4_t, __builtin_amdgcn_raw_buffer_load_b128(c.rt, kOOB, 0, NAD_TILE_AUX));
#pragma unroll
      for (int g = 0; g < GPT; g++) {
        S.sc[i][g] = __builtin_amdgcn_raw_buffer_load_b32(c.rs, kOOB, 0, 0);
        S.zp[i][g] = ASYM ? int(int8_t(__builtin_amdgcn_raw_buffer_load_b8(c.rz, kOOB, 0, 0))) : 0;
      }
    }
    return;
  }
  stage_loads<ASYM>(a, S, c, true, lane, vs);
  c.q += NW;
  if (c.q >= nsl) {
    c.q = wave;
    c.j++;
    if (c.j < nv)
      cursor_stripe(a, c, v0);
    else
      c.rt = c.rs = c.rz = rsrc(a.w[0].tiles, 0);
  }
}

// ------------------------------------------------------------------------------------------------ dequantization
// int4: the four nibble pairs of one MFMA step's dword as exact integer fp16 (q - zp).  The 0x6400 magic leaves the
// ten mantissa bits free, so a nibble can sit at bits 0-3 (value 1024 + q) or bits 4-7 (value 1024 + 16 q):
//   pair 0 = (w & 0x000F000F) | M          = 1024 + q     -> x - (1024 + 8 + zp)
//   pair 1 = (w & 0x00F000F0) | M          = 1024 + 16 q  -> x / 16 - (64 + 8 + zp)
//   pair 2 = ((w >> 8) & 0x000F000F) | M   = 1024 + q
//   pair 3 = ((w >> 8) & 0x00F000F0) | M   = 1024 + 16 q
// = 1 shift + 4 v_and_or + 2 v_pk_add_f16 + 2 v_pk_fma_f16 per 8 weights; each pk op rounds an exact value once.
struct Dq4 {
  uint32_t m0, m1, mag;  // masks and magic, kept in registers (VOP3 takes no literals on gfx9)
  h2_t s16;
  h2_t c0, c1;           // -(1024 + bias) and -(64 + bias): the symmetric weights' zero point folded into the magic's
};

__device__ __forceinline__ h8_t dequant4(uint32_t w, const Dq4& q, h2_t c0, h2_t c1) {
  return dq4_core(w, q.m0, q.m1, q.mag, q.s16, c0, c1);
}

// a group scale from the dword load_stage fetched: f32 as is, 16-bit types from the half selected by `sh`
// (branch-free: the scale type is launch-uniform, selects are cheaper than branches here)
__device__ __forceinline__ float scale_bits_to_f32(uint32_t x, int st, int sh) {
  const uint32_t h = (x >> sh) & 0xFFFFu;
  const float fb = __uint_as_float(h << 16);
  const float fh = f16_bits_to_f32(uint16_t(h));
  const float f16or = st == kScaleBF16 ? fb : fh;
  return st == kScaleF32 ? __uint_as_float(x) : f16or;
}

// ... with the scale type known at compile time (ST >= 0: the int2 M = 1 instantiations, whose body applies a scale
// every 64 k at g64 -- VERDICT r5 item 4), else from the launch-uniform runtime value as above
template <int ST>
__device__ __forceinline__ float scale_to_f32(uint32_t x, int st, int sh) {
  if constexpr (ST < 0) return scale_bits_to_f32(x, st, sh);
  else if constexpr (ST == kScaleF32) return __uint_as_float(x);
  else if constexpr (ST == kScaleBF16) return __uint_as_float((x >> sh) << 16);
  else return f16_bits_to_f32(uint16_t(x >> sh));
}

constexpr int k_tile(int bits) { return bits == 4 ? 128 : (bits == 2 ? 256 : 64); }  // k per 1 KiB tile
constexpr int zp_bias(int bits) { return bits == 4 ? 8 : (bits == 2 ? 2 : 128); }

// the launch's int4 constants; mask and magic arrive as kernel arguments so that they stay in scalar registers
template <int BITS>
__device__ __forceinline__ Dq4 dq4_consts(uint32_t mask, uint32_t magic) {
  Dq4 q;
  q.m0 = __builtin_amdgcn_readfirstlane(mask);
  q.m1 = q.m0 << 4;
  q.mag = __builtin_amdgcn_readfirstlane(magic);
  q.s16 = splat(1.f / 16.f);
  q.c0 = splat(-(1024.f + zp_bias(BITS)));
  q.c1 = splat(-(64.f + zp_bias(BITS)));
  return q;
}

// the 8 weights (q - zero point, exact fp16) a lane feeds MFMA step d of a tile
template <int BITS, bool ASYM>
__device__ __forceinline__ h8_t dequant_tile_step(const u4_t& b, int d, int zp, const Dq4& dq) {
  if constexpr (BITS == 4) {
    if constexpr (ASYM) {
      const float z = float(zp);
      return dequant4(b[d], dq, dq.c0 - splat(z), dq.c1 - splat(z));
    } else {
      return dequant4(b[d], dq, dq.c0, dq.c1);
    }
  } else {
    return BITS == 2 ? dequant2_step(b, d, zp_bias(BITS) + zp) : dequant_step<BITS>(b, d, zp_const(zp_bias(BITS) + zp));
  }
}

// One stage's arithmetic, shared by every kernel of this file: KSN independent MFMA chains (one per tile, step-major)
// so the scheduler can interleave them; at each group end the tiles' group partials are scaled into the stripe sum
// `acc`, in tile order.  ab + tile_off(i): this lane's activation row at tile i of the stage; LO adds the second MFMA
// over the fp16 lo row at abl (woq_gemv_kernel with more than 8 fp32 / bf16 rows).
template <int BITS, int GPT, bool ASYM, int KSN, int ST, bool LO, class TileOff>
__device__ __forceinline__ void stage_mac(const StageRegs<GPT, KSN>& S, const Dq4& dq, const char* ab, const char* abl,
                                          TileOff tile_off, int scale_t, int ssh, f4_t& acc) {
  constexpr int SPT = k_tile(BITS) / 32, SPG = SPT / GPT;  // MFMA steps per tile, per group
  f4_t accg[KSN];
#pragma unroll
  for (int d = 0; d < SPT; d++) {
    const int g = GPT == 1 ? 0 : d / SPG;
#pragma unroll
    for (int i = 0; i < KSN; i++) {
      const h8_t bf = dequant_tile_step<BITS, ASYM>(S.b[i], d, S.zp[i][g], dq);
      const h8_t af = *reinterpret_cast<const h8_t*>(ab + tile_off(i) + d * 64);
      accg[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, d % SPG == 0 ? f4_t{0.f, 0.f, 0.f, 0.f} : accg[i], 0, 0, 0);
      if constexpr (LO) {
        const h8_t afl = *reinterpret_cast<const h8_t*>(abl + tile_off(i) + d * 64);
        accg[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afl, bf, accg[i], 0, 0, 0);
      }
    }
    if ((d + 1) % SPG == 0) {
#pragma unroll
      for (int i = 0; i < KSN; i++) acc += accg[i] * scale_to_f32<ST>(S.sc[i][g], scale_t, ssh);
    }
  }
}

// ------------------------------------------------------------------------------------------------ slot reduction
// A wave's partial sum of a stripe goes to an LDS slot; after the barrier each output sums its slots in wave order:
// s_i sums slots i, i + 4, ... of the whole groups of four, s_0 takes the rest, then (s0 + s1) + (s2 + s3).
// The M = 1 kernels' form: at most 16 adjacent slots, all read at once (one LDS round trip) at offsets clamped to the
// last slot.  woq_gemv_kernel keeps the same order as a loop of its own (step 4 there says why).
__device__ __forceinline__ float reduce_slots(const float* ps, int nwl) {
  float t[16];
#pragma unroll
  for (int w = 0; w < 16; w++) t[w] = ps[min(w, nwl - 1)];
  const int full = nwl & ~3;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int w = 0; w < 16; w += 4)
    if (w < full) {
      s0 += t[w];
      s1 += t[w + 1];
      s2 += t[w + 2];
      s3 += t[w + 3];
    }
#pragma unroll
  for (int w = 0; w < 16; w++)
    if (w >= full && w < nwl) s0 += t[w];
  return (s0 + s1) + (s2 + s3);
}

// The M = 1 kernels lay their slots out per column, [nv][16 columns][slot stride], so that a launch whose slot count N
// is known at compile time (the stride is then N rounded up to 4) reduces with N / 4 rounded up 16-B LDS reads per
// output and no per-slot clamps: the same order as reduce_slots at N, whose 16 clamped offsets + masks are ~100 scalar
// instructions executed once per launch, cold in the instruction cache (~0.4 us per KB).  Measured at N = 16
// (profiles/r06_gemv_tail_ab.txt, same box, alternating): O 4.80 -> 4.55 us, decode 946-951 -> 969-972 tok/s;
// bit-identical sums.
template <int N>
__device__ __forceinline__ float reduce_fixed(const float* col) {
  static_assert(N >= 4 && N <= 16, "at least one whole group of four");
  constexpr int NV = (N + 3) / 4, FULL = N / 4;
  const float4* ps = reinterpret_cast<const float4*>(col);
  float4 t[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) t[i] = ps[i];
  float s0 = t[0].x, s1 = t[0].y, s2 = t[0].z, s3 = t[0].w;
#pragma unroll
  for (int i = 1; i < FULL; i++) {
    s0 += t[i].x;
    s1 += t[i].y;
    s2 += t[i].z;
    s3 += t[i].w;
  }
  if constexpr (N % 4 > 0) s0 += t[FULL].x;
  if constexpr (N % 4 > 1) s0 += t[FULL].y;
  if constexpr (N % 4 > 2) s0 += t[FULL].z;
  return (s0 + s1) + (s2 + s3);
}

// ------------------------------------------------------------------------------------------------ activation staging
// activation bits -> 8 floats of one staging unit (runtime type: staging runs once per workgroup)
__device__ __forceinline__ void unit_to_f32(int act_t, uint4 x0, uint4 x1, float (&f)[8]) {
  const uint32_t w[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  if (act_t == kActF32) {
#pragma unroll
    for (int j = 0; j < 8; j++) f[j] = __uint_as_float(w[j]);
  } else if (act_t == kActBF16) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f[2 * j] = __uint_as_float(w[j] << 16);
      f[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const h2_t h = as_h2(w[j]);
      f[2 * j] = float(h[0]);
      f[2 * j + 1] = float(h[1]);
    }
  }
}

// write one staging unit (8 k of one row) as fp16 hi (+ lo) rows
template <int HILO>
__device__ __forceinline__ void unit_store(char* smem, const float (&f)[8], int row, int k, int M, int Kp) {
  h8_t hi, lo;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    hi[j] = _Float16(f[j]);
    lo[j] = _Float16(f[j] - float(hi[j]));
  }
  *reinterpret_cast<h8_t*>(smem + (size_t(row) * Kp + k) * 2) = hi;
  if constexpr (HILO != 0) *reinterpret_cast<h8_t*>(smem + (size_t(M + row) * Kp + k) * 2) = lo;
}

// element-wise staging (act-order gather, unaligned rows, K % 8 != 0)
template <int HILO>
__device__ __forceinline__ void stage_a_slow(const GemvArgs& a, char* smem, int units, int Kp) {
  for (int u = threadIdx.x; u < units; u += blockDim.x) {
    const int row = u / (Kp >> 3), k = (u - row * (Kp >> 3)) * 8;
    float f[8];
    for (int j = 0; j < 8; j++) {
      const int kk = k + j;
      f[j] = 0.f;
      if (kk < a.K) {
        const size_t src = size_t(row) * a.lda + (a.shuffle ? a.shuffle[kk] : kk);
        if (a.act_t == kActF32)
          f[j] = static_cast<const float*>(a.A)[src];
        else if (a.act_t == kActBF16)
          f[j] = bf16_bits_to_f32(static_cast<const uint16_t*>(a.A)[src]);
        else
          f[j] = float(static_cast<const _Float16*>(a.A)[src]);
      }
    }
    unit_store<HILO>(smem, f, row, k, a.M, Kp);
  }
}

// ------------------------------------------------------------------------------------------------ the kernel
// finer groups carry GPT scale (+ zero-point) registers per tile: those variants run at most 8 waves per workgroup
template <int GPT>
constexpr int gemv_max_threads() {
  return GPT == 1 ? 1024 : 512;
}

// NST: register stages in flight per wave (3, or 1 where no wave streams more than two stages: the ring's extra slots
// would only carry dead out-of-range loads, see m1_body).
// The body (steps 1-4) is woq_gemv_body.inc, which says why it is text: woq_gemv_kernel runs it as workgroup blockIdx.x
// of gridDim.x, woq_gemv_routed_kernel as workgroup b % wpp of the wpp that share one problem.
template <int BITS, int HILO, int GPT, bool ASYM, int NST>
__global__ __launch_bounds__(gemv_max_threads<GPT>()) void woq_gemv_kernel(GemvArgs a) {
#define GEMV_WG_INDEX blockIdx.x
#define GEMV_WG_COUNT gridDim.x
#include "woq_gemv_body.inc"
#undef GEMV_WG_INDEX
#undef GEMV_WG_COUNT
}

// Routed, for the formats the M = 1 stream below does not instantiate (int4 groups of 32; int8): to
// woq_gemv_kernel<BITS, HILO = 1, GPT, ASYM, NST> what woq_gemv_m1_routed_kernel is to m1_body: the same body, once
// more.  Workgroup b serves problem p = b / wpp -- row r = p / slots, slot i = p % slots -- reads that problem's
// expert id from device memory (one wave-uniform load), clamps it before the table is touched, takes the expert's tiles / scales / zero points (and
// the up weight's, for the {gate, up} pair) from the bank entry, derives its one activation row (fp32: hi / lo fp16
// rows) and its output row from r, p and the strides, and runs the body on share b % wpp of the problem's units.  The
// waves, the K-slices and the cross-wave reduce are those of the expert's own one-problem launch, and how the units are
// dealt over workgroups changes no sum: every routed row has the bits of the expert's own M = 1 forward.
// An id outside [0, n_expert) leaves the weight views with zero stripes: cursor_stripe builds zero-record resources,
// nothing of any weight is read, every partial is 0 * 0-scale = +0.0, and step 4 -- which takes the column count from
// SkinnyWeight::n, not from the stripe count -- still writes the row: +0.0.
// NST = 3: the ring gemv_launch4 takes once a wave streams more than two stages, which a routed workgroup does as soon
// as the chip's workgroups are dealt over several problems (one Mixtral token: 896 gate / up stripe pairs over 128
// workgroups per problem, 14 stripes each); a depth of 1 serves only launches of one or two stages per wave, where the
// ring's extra slots issue out-of-range loads that touch no memory.  One depth for all five instantiations (their own
// object: woq_gemv_r7.hip); the depth orders loads only and changes no sum.
constexpr int kRoutedGeneralNst = 3;
template <int BITS, int GPT, bool ASYM>
__global__ __launch_bounds__(gemv_max_threads<GPT>()) void woq_gemv_routed_kernel(GemvArgs a, GemvRouted r) {
  const int p = int(blockIdx.x) / r.wpp;
  const int wg_index = int(blockIdx.x) - p * r.wpp, wg_count = r.wpp;
  const int row = p / r.slots;
  const int id = __builtin_amdgcn_readfirstlane(r.ids[size_t(row) * r.ids_ld + r.ids_col + (p - row * r.slots)]);
  const bool valid = unsigned(id) < unsigned(r.n_expert);
  const int e = min(max(id, 0), r.n_expert - 1);
  const GemvExpertEnt g = r.bank[0][e];
  a.A = r.act + size_t(r.act_per_slot ? p : row) * r.act_ld;
  a.w[0].tiles = g.tiles;
  a.w[0].scales = g.scales;
  a.w[0].zps = g.zps;
  a.w[0].out = r.out + size_t(p) * r.out_ld;
  if (a.dual) {
    const GemvExpertEnt u = r.bank[1][e];
    a.w[1].tiles = u.tiles;
    a.w[1].scales = u.scales;
    a.w[1].zps = u.zps;
    a.w[1].out = a.w[0].out;
  }
  if (!valid) a.w[0].ns = a.w[1].ns = 0;
  constexpr int HILO = 1, NST = kRoutedGeneralNst;
#define GEMV_WG_INDEX wg_index
#define GEMV_WG_COUNT wg_count
#include "woq_gemv_body.inc"
#undef GEMV_WG_INDEX
#undef GEMV_WG_COUNT
}

// ------------------------------------------------------------------------------------------------ M = 1 variant
// Every launch pays its executed code again (the instruction cache starts cold per dispatch: ~0.45 us per KB at 8
// waves per CU, tools/ifetch_probe.hip), and a decode matmul at K = 4096 streams one stripe per workgroup -- so the
// executed instruction bytes ARE the fixed cost.  This variant of the stream for M = 1 (int4 / int2, groups of a whole
// tile or a power-of-two part of one) keeps that path short: the activation type is a template parameter, the workgroup's unit range comes from host-divided
// counts (no integer division), and each wave stages only ITS K-slices of the activations into its own LDS rows
// (hi / lo fp16, plus a zero row for the MFMA rows M = 1 leaves empty), so nothing waits on a block-wide barrier before
// the stream; the one barrier is the final cross-wave reduction.
// K-slices per wave it stages: 2 (K <= waves * 2 * ks * KT), or 4 for long K (Mistral's down, K = 14336 at 7 waves)
// per wave: a zero row, then per slice {hi, lo} rows of ks * KT fp16 each
constexpr int lean_row_bytes(int bits, int ks) { return ks * (bits == 4 ? 128 : 256) * 2; }
constexpr int lean_wave_lds(int bits, int ks, int spw) { return lean_row_bytes(bits, ks) * (1 + 2 * spw); }
// narrow slices carry few stage registers: those launches may run 16 waves whatever the groups per tile
template <int GPT, int KSN>
constexpr int m1_max_threads() {
  return GPT == 1 || KSN <= 2 ? 1024 : 512;
}

// BATCH: independent problems of one shape in one launch (BTLAGemmBatchDriver, bestla_gemm.cpp:508-624): workgroup
// b serves problem b / batch_wpp -- its activations, weight and output pointers come from the problem table (one
// scalar-cache line) -- and that problem's share b % batch_wpp of the stripes, so a batch of decode-size problems
// streams like one large launch instead of paying each launch's fixed chain.
// The kernel body takes its workgroup index as an argument: woq_gemv_m1_dual_kernel runs two instantiations side by
// side in one launch.
// NST: register stages in flight per wave.  Every stage slot is loaded again right after it is computed -- with
// out-of-range offsets once the wave's run is done -- so a ring deeper than the wave's own stages only adds dead
// loads to the CU's memory queue, in front of the live ones.  Measured (profiles/r04_gemv_ring_depth_ab.txt,
// r04_gemv_nst_ab.txt): one stage (1-2 KiB per wave) is fastest until a wave streams about seven, two beyond that
// or for 1 KiB int2 stages from four (O 5.78 -> 4.83 us, down K = 11008 9.6 -> 7.8, gate/up 13.2 -> 12.2, QKV 8.6 ->
// 8.1); deeper rings are slower everywhere except the batched launch's long streams (3: 1.43 vs 1.46 us per problem).
#ifndef NAD_M1_BATCH_NST
#define NAD_M1_BATCH_NST 3
#endif
#ifndef NAD_M1_DUAL_NST
#define NAD_M1_DUAL_NST 2
#endif

// Steps 1-3 of both M = 1 kernels -- this wave's activation loads, its first weight stage, the staging into its LDS
// rows, the remaining ring stages, and the compute loop up to the published partial sums and the one barrier -- exist
// once, here.  What differs between woq_gemv_m1_kernel and woq_gemv_m1s_kernel comes in as the policy P:
//   P::Args                       the argument block (GemvArgs / GemvM1Args<NWT>)
//   P::act_rsrc, P::act_live      the activations' buffer resource and which of a wave's loads are in range
//   P::cursor_start, P::load      the stage loader (two-armed load_stage / select-based m1s_load_stage: both were
//                                 measured separately and both stay)
// and the wave count NW and the slot stride PS of a column's partial sums as values (blockDim, the argument block's,
// or literals).
struct M1General {
  using Args = GemvArgs;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t act_rsrc(const Args& a, int esz) { return rsrc(a.A, a.K * esz); }
  static __device__ __forceinline__ bool act_live(const Args& a, int q, int nsl, int k) { return q < nsl && k < a.K; }
  template <bool ASYM>
  static __device__ __forceinline__ void cursor_start(const Args& a, StageCursor& c, int v0, int nv, bool idle) {
    c.s = 0;
    c.rt = rsrc(a.w[0].tiles, 0);  // zero records: every access out of range (idle waves, past-the-end stages)
    c.rs = c.rt;
    c.rz = c.rt;
    if (!idle && nv > 0) cursor_stripe(a, c, v0);
  }
  template <int GPT, bool ASYM, int KSN>
  static __device__ __forceinline__ void load(const Args& a, StageRegs<GPT, KSN>& S, StageCursor& c, int nv, int nsl,
                                              int wave, int NW, int v0, int lane, int vs) {
    load_stage<GPT, ASYM, KSN>(a, S, c, nv, nsl, wave, NW, v0, lane, vs);
  }
};

template <class P, int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, int NST, int ST, bool AHEAD = false>
__device__ __forceinline__ void m1_stream(const typename P::Args& a, int lane, int wave, int NW, int nsl, int v0,
                                          int nv, bool idle, float* part, int PS) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KT = k_tile(BITS);
  constexpr int RB = lean_row_bytes(BITS, KSN);  // one fp16 row of a slice
  constexpr int UNITS = KSN * KT / 8;             // 8-element staging units per slice
  constexpr int UPL = UNITS >= 64 ? UNITS / 64 : 1;  // ... per lane (2-tile int4 slices: lanes < 32 hold one)
  constexpr bool PART = UNITS < 64;
  constexpr int ESZ = AT == kActF32 ? 4 : 2;
  constexpr bool HL = AT != kActF16;  // fp32 / bf16 rows split into fp16 hi + lo (MFMA rows 0 and 8)
  const bool ulane = !PART || lane < UNITS;  // this lane holds a staging unit of each slice

  // 1) this wave's activation slices (q = wave + j NW; past the end of K the buffer returns zeros), then the first
  //    weight stage
  const auto ra = P::act_rsrc(a, ESZ);
  uint4 x[SPW * UPL][2];
#pragma unroll
  for (int j = 0; j < SPW * UPL; j++) {
    const int q = wave + (j / UPL) * NW, k = q * (KSN * KT) + ((j % UPL) * 64 + lane) * 8;
    const int off = (ulane && P::act_live(a, q, nsl, k)) ? k * ESZ : kOOB;
    x[j][0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
    if constexpr (ESZ == 4) x[j][1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
  }
  const int vs = a.scale_t == kScaleF32 ? (lane & 15) * 4 : (lane & 14) * 2;
  StageCursor lc;
  lc.j = idle ? nv : 0;
  lc.q = wave;
  P::template cursor_start<ASYM>(a, lc, v0, nv, idle);
  StageRegs<GPT, KSN> S[NST];
  P::template load<GPT, ASYM, KSN>(a, S[0], lc, nv, nsl, wave, NW, v0, lane, vs);
  NAD_TRACE(4);

  // 2) stage the slices into this wave's rows (LDS ops of one wave complete in order: no barrier)
  char* wrow = smem + wave * lean_wave_lds(BITS, KSN, SPW);
#pragma unroll
  for (int u = 0; u < UPL; u++)
    if (ulane) *reinterpret_cast<uint4*>(wrow + (u * 64 + lane) * 16) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int j = 0; j < SPW * UPL; j++) {
    if (!ulane) break;
    h8_t hi, lo;
    if constexpr (AT == kActF16) {
      hi = __builtin_bit_cast(h8_t, x[j][0]);
    } else {
      float f[8];
      unit_to_f32(AT, x[j][0], x[j][1], f);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        hi[e] = _Float16(f[e]);
        lo[e] = _Float16(f[e] - float(hi[e]));
      }
    }
    char* row = wrow + RB + (j / UPL) * 2 * RB + ((j % UPL) * 64 + lane) * 16;
    *reinterpret_cast<h8_t*>(row) = hi;
    if constexpr (HL) *reinterpret_cast<h8_t*>(row + RB) = lo;
  }
#pragma unroll
  for (int i = 1; i < NST; i++) P::template load<GPT, ASYM, KSN>(a, S[i], lc, nv, nsl, wave, NW, v0, lane, vs);
  NAD_TRACE(1);

  // 3) the stream: MFMA row 0 = hi (lane m 0), row 8 = lo (lane m 8), every other row reads the zero row
  const int m = lane & 15, kq = lane >> 4;
  const bool isrow = m == 0 || (HL && m == 8);
  const char* abase = wrow + (isrow ? (m == 0 ? RB : 2 * RB) : 0) + kq * 16;
  const int slice_step = isrow ? 2 * RB : 0;
  const int ssh = a.scale_t == kScaleF32 ? 0 : (lane & 1) * 16;
  const Dq4 dq = dq4_consts<BITS>(a.dq_mask, a.dq_magic);

  f4_t acc = {0.f, 0.f, 0.f, 0.f};
  int cj = idle ? nv : 0, cq = wave, cs = 0;  // compute cursor: local stripe, K-slice, slice ordinal of this wave

#ifdef NAD_PHASE_TRACE
  // slots 5-7: wave 0's arithmetic time of its first stage, of all later stages, and the stage count -- each stage
  // timed from an explicit wait for its loads to its last MFMA result (is the stream body's code, first executed when
  // nothing else is pending, fetched late?)
  unsigned long long tr_first = 0, tr_later = 0, tr_k = 0;
#endif
  auto compute_stage = [&](const StageRegs<GPT, KSN>& S) {
    if (cj >= nv) return;
    const char* ab = abase + cs * slice_step;
#ifdef NAD_PHASE_TRACE
    if constexpr (!AHEAD) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // AHEAD: waited before the next stage went out
    const unsigned long long tr0 = wall_clock64();
#endif
    stage_mac<BITS, GPT, ASYM, KSN, ST, false>(S, dq, ab, ab, [](int i) { return i * KT * 2; }, a.scale_t, ssh, acc);
#ifdef NAD_PHASE_TRACE
    {
      const int sink = __builtin_amdgcn_readfirstlane(__float_as_int(acc[0]));  // the last MFMA's result has landed
      asm volatile("" ::"s"(sink));
      const unsigned long long d = wall_clock64() - tr0;
      if (tr_k == 0) tr_first = d;
      else tr_later += d;
      tr_k++;
    }
#endif
    cq += NW;
    cs++;
    if (cq >= nsl) {  // this wave's last slice of stripe cj: publish its partial (row 0 + row 8 = hi + lo)
      float r = acc[0];
      if constexpr (HL) {
        r += __shfl_down(r, 32, 64);
      }
      if (lane < 16) part[(size_t(cj) * 16 + lane) * PS + wave] = r;  // [nv][16 columns][PS]: a column's slots together
      acc = f4_t{0.f, 0.f, 0.f, 0.f};
      cq = wave;
      cs = 0;
      cj++;
    }
  };

  if constexpr (AHEAD) {
    // Load-ahead order (one register stage, two sets): once the current set has landed, the wave's next live stage is
    // requested into the other set, and only then is the current one computed -- one live stage outstanding per wave
    // at any time, nothing requested past the wave's last stage, so the waits are plain vmcnt(0).  The loads sit under
    // a wave-uniform branch; the scheduling barrier keeps them in front of the stage's first MFMA.
    static_assert(NST == 1, "the load-ahead order replaces the one-stage loop");
    StageRegs<GPT, KSN> T;
    auto ahead = [&](StageRegs<GPT, KSN>& next) {
      // vmcnt(0) as the builtin, not inline assembly: hipcc then knows that nothing is outstanding here and puts no
      // wait of its own (which, merged over the branch below, would wait for the loads just issued) before the MFMAs
      __builtin_amdgcn_s_waitcnt(0x0F70);
      if (lc.j < nv) P::template load<GPT, ASYM, KSN>(a, next, lc, nv, nsl, wave, NW, v0, lane, vs);
      __builtin_amdgcn_sched_barrier(0);
    };
    while (cj < nv) {
      ahead(T);
      compute_stage(S[0]);
      if (cj >= nv) break;
      ahead(S[0]);
      compute_stage(T);
    }
  } else {
    while (cj < nv) {
#pragma unroll
      for (int i = 0; i < NST; i++) {
        compute_stage(S[i]);
        P::template load<GPT, ASYM, KSN>(a, S[i], lc, nv, nsl, wave, NW, v0, lane, vs);
      }
    }
  }
#ifdef NAD_PHASE_TRACE
  if (threadIdx.x == 0 && blockIdx.x < kTraceMaxWg) {
    nad_trace_buf[5][blockIdx.x] = tr_first;
    nad_trace_buf[6][blockIdx.x] = tr_later;
    nad_trace_buf[7][blockIdx.x] = tr_k;
  }
#endif
  NAD_TRACE_MAX(2);
  __syncthreads();
}

// woq_gemv_m1_kernel's body: the stream over the full GemvArgs, then the runtime epilogue switch.  A branch-free first
// weight stage (the two-armed load_stage makes hipcc wait vmcnt(0) for the activation loads before the first weight
// load) measured neutral (943-947 tok/s) on this kernel and was not kept here; woq_gemv_m1s_kernel below, which serves
// the decode token's launches, has no control flow around any stage's loads.
template <int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, bool BATCH, int NST, int ST = -1>
__device__ __forceinline__ void m1_body(GemvArgs& a, int bid) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int NW = __builtin_amdgcn_readfirstlane(int(blockDim.x >> 6));
  const int nsl = (a.nt + KSN - 1) / KSN;
  NAD_TRACE(0);
  if constexpr (BATCH) {
    const int p = bid / a.batch_wpp;
    bid -= p * a.batch_wpp;
    const GemvBatchEnt e = a.batch[p];
    a.A = e.act;
    a.w[0].tiles = e.tiles;
    a.w[0].scales = e.scales;
    a.w[0].zps = e.zps;
    a.w[0].out = e.out;
  }
  const int u0 = bid * a.u_q + min(bid, a.u_r);
  const int u1 = u0 + a.u_q + (bid < a.u_r ? 1 : 0);
  const int vpu = a.dual ? 2 : 1;
  const int v0 = u0 * vpu, nv = (u1 - u0) * vpu;
  float* part = reinterpret_cast<float*>(smem + a.part_off);  // [nv][16 columns][NW]
  m1_stream<M1General, BITS, GPT, AT, ASYM, KSN, SPW, NST, ST>(a, lane, wave, NW, nsl, v0, nv, wave >= nsl, part, NW);

  // 4) sum each stripe's wave slots in wave order and apply the epilogue
  const int nout = (u1 - u0) * 16;
  const int nwl = min(NW, nsl);
  // the fused epilogue of output o = (local stripe p, column nn) from its stripe sum(s) y
  auto emit = [&](int p, int nn, const float (&y)[2]) {
    int wsel, s;
    vstripe(a, v0 + p * vpu, wsel, s);
    if (a.dual) wsel = 0;
    const int n = s * 16 + nn;
    if (n >= sel3(wsel, a.w[0].n, a.w[1].n, a.w[2].n)) return;
    float* out = sel3(wsel, a.w[0].out, a.w[1].out, a.w[2].out);
    float v = y[0];
    switch (a.epi) {
      case kEpiBias:
        v += a.w[0].bias[n];
        break;
      case kEpiAddGelu:
        v = gelu_f(v + a.w[0].bias[n]);
        break;
      case kEpiGelu:
        v = gelu_f(v);
        break;
      case kEpiSilu:
        v = silu_f(v);
        break;
      case kEpiResAdd:
        v += a.res[n];
        break;
      case kEpiSiluMul: {
        const float t1 = silu_f(y[0]);
        if (a.aux) a.aux[n] = t1;
        v = t1 * y[1];
        break;
      }
      case kEpiGeluMul: {
        const float t1 = gelu_f(y[0]);
        if (a.aux) a.aux[n] = t1;
        v = t1 * y[1];
        break;
      }
      default:
        break;
    }
    out[n] = v;
  };
  if (nwl == 16 && NW == 16) {  // 16 waves with a slice each
    for (int o = threadIdx.x; o < nout; o += blockDim.x) {
      const int p = o >> 4, nn = o & 15;
      float y[2] = {0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 2; h++)
        if (h < vpu) y[h] = reduce_fixed<16>(part + (size_t(p * vpu + h) * 16 + nn) * 16);
      emit(p, nn, y);
    }
    NAD_TRACE(3);
    return;
  }
  for (int o = threadIdx.x; o < nout; o += blockDim.x) {
    const int p = o >> 4, nn = o & 15;
    float y[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; h++)
      if (h < vpu) y[h] = reduce_slots(part + (size_t(p * vpu + h) * 16 + nn) * NW, nwl);
    emit(p, nn, y);
  }
  NAD_TRACE(3);
}

template <int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, bool BATCH, int NST, int ST>
__global__ __launch_bounds__((m1_max_threads<GPT, KSN>())) void woq_gemv_m1_kernel(GemvArgs a) {
  m1_body<BITS, GPT, AT, ASYM, KSN, SPW, BATCH, NST, ST>(a, int(blockIdx.x));
}

// Two weight formats in one decode launch: workgroups [0, ga) run format 1's body over a, the rest format 2's over b
// (each exactly its own one-format launch's arithmetic).  The int2 policies' QKV (llama_utils.cpp:269-287: int2 Q, K
// with an int4 V of the same group size) then costs one launch instead of two.  Both bodies take 16 waves at K = 4096
// (int2: 1-tile slices of 256 k, int4: 2-tile slices of 256 k); the launch takes the larger LDS image.
template <int B1, int G1, int K1, int B2, int G2, int K2, int AT>
__global__ __launch_bounds__(1024) void woq_gemv_m1_dual_kernel(GemvArgs a, GemvArgs b, int ga) {
  if (int(blockIdx.x) < ga)
    m1_body<B1, G1, AT, false, K1, 1, false, NAD_M1_DUAL_NST>(a, int(blockIdx.x));
  else
    m1_body<B2, G2, AT, false, K2, 1, false, NAD_M1_DUAL_NST>(b, int(blockIdx.x) - ga);
}

// Routed: the batched launch with the problem table replaced by a lookup the kernel does itself (ne_mul_mat_id,
// ne_layers.c:7783-7916: per row an int32 id picks one of n_as expert weights).  Workgroup b serves problem
// p = b / wpp of one shape -- row r = p / slots, slot i = p % slots -- reads that problem's expert id from device
// memory, takes the expert's tiles / scales / zero points (and the up weight's, for the {gate, up} pair) from the bank
// entry, derives its activation and output vectors from r, p and the strides, and runs m1_body on its share b % wpp of
// the stripes: each stripe exactly the arithmetic of the expert's own one-problem launch.  The routing is data of the
// launch, not of the host call, so a captured graph follows ids that change between replays.
// An id outside [0, n_expert) is clamped before the table is touched and the problem runs with zero stripes in its
// weight views: cursor_stripe then builds zero-record resources (the rsrc(ptr, 0) of idle waves), every weight, scale
// and zero-point load returns zero without touching memory, and the problem writes zeros.
template <int BITS, int GPT, bool ASYM, int KSN, int SPW, int NST, int ST>
__global__ __launch_bounds__((m1_max_threads<GPT, KSN>())) void woq_gemv_m1_routed_kernel(GemvArgs a, GemvRouted r) {
  int bid = int(blockIdx.x);
  const int p = bid / r.wpp;
  bid -= p * r.wpp;
  const int row = p / r.slots;
  const int id = __builtin_amdgcn_readfirstlane(r.ids[size_t(row) * r.ids_ld + r.ids_col + (p - row * r.slots)]);
  const bool valid = unsigned(id) < unsigned(r.n_expert);
  const int e = min(max(id, 0), r.n_expert - 1);
  const GemvExpertEnt g = r.bank[0][e];
  a.A = r.act + size_t(r.act_per_slot ? p : row) * r.act_ld;
  a.w[0].tiles = g.tiles;
  a.w[0].scales = g.scales;
  a.w[0].zps = g.zps;
  a.w[0].out = r.out + size_t(p) * r.out_ld;
  if (a.dual) {
    const GemvExpertEnt u = r.bank[1][e];
    a.w[1].tiles = u.tiles;
    a.w[1].scales = u.scales;
    a.w[1].zps = u.zps;
    a.w[1].out = a.w[0].out;
  }
  if (!valid) a.w[0].ns = a.w[1].ns = 0;
  m1_body<BITS, GPT, kActF32, ASYM, KSN, SPW, false, NST, ST>(a, bid);
}

// ------------------------------------------------------------------------------------------------ M = 1, specialised
// The same stream and the same sums as m1_body for the launches a decode token is made of, with the code a launch runs
// where no memory latency hides it cut down (tools/gemv_path_bytes.py prints it per instantiation):
//   * its own arguments instead of GemvArgs, every per-launch constant worked out by the host: 14 dwords of leading
//     scalar parameters that arrive in SGPRs at dispatch (kernarg preload, -mllvm -amdgpu-kernarg-preload-count=14 on
//     this kernel's objects), so the path to the first loads waits for no scalar load, and a remainder struct read by
//     one batch of scalar loads behind them;
//   * NWT, the weights of the launch, at compile time: 1 (no stripe -> weight lookup at all), 3 (fused QKV) or
//     2 = the {gate, up} pair, which also fixes the epilogue: a plain store for 1 and 3, SiLU(gate) * up for 2.  Every
//     other epilogue stays on woq_gemv_m1_kernel with its runtime switch;
//   * NSC, the slots per column the launch reduces (= its waves, each with a K-slice of every stripe), at compile
//     time for the counts the token runs at -- 16, and the down projections' 11 and 7 -- so the wave count is a literal
//     and the reduce is reduce_fixed; 0 = the runtime count (reduce_slots).  One reduce per instantiation, straight
//     after the stream;
//   * a stage's loads are never under control flow (past-the-end stages select the out-of-range offset), so nothing
//     makes hipcc wait for the activation loads before it issues the first weight stage.
template <int NWT>
struct M1Sel {  // the wave-uniform (weight, stripe within it) of virtual stripe v
  int w, s;
  __device__ __forceinline__ M1Sel(const GemvM1Args<NWT>& a, int v) {
    if constexpr (NWT == 1) {
      w = 0;
      s = v;
    } else if constexpr (NWT == 2) {
      w = v & 1;
      s = v >> 1;
    } else {
      w = (v >= a.sb1 ? 1 : 0) + (v >= a.sb2 ? 1 : 0);
      s = v - (w == 0 ? 0 : (w == 1 ? a.sb1 : a.sb2));
    }
  }
};
template <int NWT, class T>
__device__ __forceinline__ T m1_pick(int w, const T (&x)[3]) {
  if constexpr (NWT == 1) return x[0];
  else if constexpr (NWT == 2) return w == 0 ? x[0] : x[1];
  else return sel3(w, x[0], x[1], x[2]);
}
#define NAD_M1_FIELD(args, wi, f) \
  m1_pick<NWT>(wi, {args.w[0].f, args.w[NWT > 1 ? 1 : 0].f, args.w[NWT > 2 ? 2 : 0].f})

template <int NWT, bool ASYM>
__device__ __forceinline__ void m1s_cursor_stripe(const GemvM1Args<NWT>& a, StageCursor& c, int v, bool on) {
  const M1Sel<NWT> vs(a, v);
  c.s = vs.s;
  const void* const tp[3] = {a.w[0].tiles, a.w[NWT > 1 ? 1 : 0].tiles, a.w[NWT > 2 ? 2 : 0].tiles};
  const void* const sp[3] = {a.w[0].scales, a.w[NWT > 1 ? 1 : 0].scales, a.w[NWT > 2 ? 2 : 0].scales};
  const int tb[3] = {a.w[0].tiles_bytes, a.w[NWT > 1 ? 1 : 0].tiles_bytes, a.w[NWT > 2 ? 2 : 0].tiles_bytes};
  const int sb[3] = {a.w[0].scales_bytes, a.w[NWT > 1 ? 1 : 0].scales_bytes, a.w[NWT > 2 ? 2 : 0].scales_bytes};
  // off: zero records, every access out of range (idle waves, past-the-end stages)
  c.rt = rsrc(m1_pick<NWT>(vs.w, tp), on ? m1_pick<NWT>(vs.w, tb) : 0);
  c.rs = rsrc(m1_pick<NWT>(vs.w, sp), on ? m1_pick<NWT>(vs.w, sb) : 0);
  if constexpr (ASYM) {
    const void* const zp[3] = {a.w[0].zps, a.w[NWT > 1 ? 1 : 0].zps, a.w[NWT > 2 ? 2 : 0].zps};
    const int zb[3] = {a.w[0].zps_bytes, a.w[NWT > 1 ? 1 : 0].zps_bytes, a.w[NWT > 2 ? 2 : 0].zps_bytes};
    c.rz = rsrc(m1_pick<NWT>(vs.w, zp), on ? m1_pick<NWT>(vs.w, zb) : 0);
  } else {
    c.rz = c.rs;
  }
}

// load_stage without control flow around the loads: a past-the-end stage (c.j >= nv) issues the same loads at the
// out-of-range offset -- same vmcnt footprint, no memory touched -- and leaves the cursor alone
template <int GPT, bool ASYM, int KSN, int NWT>
__device__ __forceinline__ void m1s_load_stage(const GemvM1Args<NWT>& a, StageRegs<GPT, KSN>& S, StageCursor& c, int nv,
                                               int nsl, int wave, int NW, int v0, int lane, int vs) {
  const bool on = c.j < nv;
  stage_loads<ASYM>(a, S, c, on, lane, vs);
  if (on) {
    c.q += NW;
    if (c.q >= nsl) {
      c.q = wave;
      c.j++;
      m1s_cursor_stripe<NWT, ASYM>(a, c, v0 + c.j, c.j < nv);
    }
  }
}

template <int NWT>
struct M1Spec {  // m1_stream's policy for woq_gemv_m1s_kernel
  using Args = GemvM1Args<NWT>;
  static __device__ __forceinline__ __amdgpu_buffer_rsrc_t act_rsrc(const Args& a, int) { return rsrc(a.A, a.a_bytes); }
  static __device__ __forceinline__ bool act_live(const Args&, int, int, int) { return true; }
  template <bool ASYM>
  static __device__ __forceinline__ void cursor_start(const Args& a, StageCursor& c, int v0, int nv, bool) {
    m1s_cursor_stripe<NWT, ASYM>(a, c, v0, c.j < nv);
  }
  template <int GPT, bool ASYM, int KSN>
  static __device__ __forceinline__ void load(const Args& a, StageRegs<GPT, KSN>& S, StageCursor& c, int nv, int nsl,
                                              int wave, int NW, int v0, int lane, int vs) {
    m1s_load_stage<GPT, ASYM, KSN, NWT>(a, S, c, nv, nsl, wave, NW, v0, lane, vs);
  }
};

// The leading scalar parameters are the preloaded ones (woq_kernels.h has the layout); a, the view the stream and the
// tail work on, is put together from them and from the remainder r.  Nothing on the way to the first loads of a
// one-weight or pair launch reads r (the pair's first stage is a gate stripe: weight 0); the 3-weight form's stripe ->
// weight select does, behind the activation loads.
template <int BITS, int GPT, int AT, bool ASYM, int KSN, int SPW, int NST, int ST, int NWT, int NSC, bool AHEAD = false>
__global__ __launch_bounds__((m1_max_threads<GPT, KSN>())) void woq_gemv_m1s_kernel(
    const void* A, const void* tiles0, const void* scales0, const void* tiles1, const void* scales1, int a_bytes,
    uint32_t uqr, uint32_t geom, int ns0, GemvM1Rest<NWT> r) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(NWT >= 1 && NWT <= 3, "1 weight, the {gate, up} pair, or 3 weights");
  static_assert(NSC == 0 || (NSC >= 4 && NSC <= 16), "slots per column: 0 = by the launch");
  constexpr int VPU = NWT == 2 ? 2 : 1;
  GemvM1Args<NWT> a;
  a.A = A;
  a.a_bytes = a_bytes;
  a.u_q = int(uqr & 0xFFFFu);
  a.u_r = int(uqr >> 16);
  a.nt = int(geom & ((1u << kM1GeomNgShift) - 1));
  a.ng = int((geom >> kM1GeomNgShift) & ((1u << (kM1GeomTpgShift - kM1GeomNgShift)) - 1));
  a.tpg_shift = int((geom >> kM1GeomTpgShift) & 31u);
  a.scale_t = int((geom >> kM1GeomScaleShift) & 3u);
  a.nw = int(geom >> kM1GeomWavesShift);
  a.nsl = (a.nt + KSN - 1) / KSN;
  a.part_off = r.part_off;
  a.dq_mask = r.dq_mask;
  a.dq_magic = r.dq_magic;
  a.sb1 = r.sb1;
  a.sb2 = r.sb2;
  a.aux = r.aux;
#pragma unroll
  for (int i = 0; i < NWT; i++) {
    const int ns = i == 0 || NWT == 2 ? ns0 : r.ns[i];
    a.w[i].tiles = i == 0 ? tiles0 : (i == 1 ? tiles1 : r.tiles2);
    a.w[i].scales = i == 0 ? scales0 : (i == 1 ? scales1 : r.scales2);
    a.w[i].zps = r.zps[i];
    a.w[i].tiles_bytes = (ns * a.nt) << 10;
    a.w[i].scales_bytes = (ns * a.ng) << (a.scale_t == kScaleF32 ? 6 : 5);
    a.w[i].zps_bytes = (ns * a.ng) << 4;
    a.w[i].n = r.n[i];
    a.w[i].out = r.out[i];
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  // NSC: the launch has NSC waves and every one of them owns a K-slice of every stripe, so a column has NSC slots
  const int NW = NSC ? NSC : a.nw;
  const int PS = NSC ? (NSC + 3) & ~3 : NW;  // whole 16-B LDS reads per column
  const int nsl = a.nsl;
  NAD_TRACE(0);
  const int bid = int(blockIdx.x);
  const int u0 = bid * a.u_q + min(bid, a.u_r);
  const int nu = a.u_q + (bid < a.u_r ? 1 : 0);
  const int v0 = u0 * VPU, nv = nu * VPU;
  const bool idle = NSC == 0 && wave >= nsl;
  float* part = reinterpret_cast<float*>(smem + a.part_off);  // [nv][16 columns][PS]
  m1_stream<M1Spec<NWT>, BITS, GPT, AT, ASYM, KSN, SPW, NST, ST, AHEAD>(a, lane, wave, NW, nsl, v0, nv, idle, part, PS);

  // 4) sum each stripe's wave slots in wave order (m1_body's order exactly), then the store
  const int nout = nu * 16;
  for (int o = threadIdx.x; o < nout; o += NW * 64) {
    const int p = o >> 4, nn = o & 15;
    float y[VPU];
#pragma unroll
    for (int h = 0; h < VPU; h++) {
      if constexpr (NSC != 0)
        y[h] = reduce_fixed<NSC>(part + (size_t(p * VPU + h) * 16 + nn) * PS);
      else
        y[h] = reduce_slots(part + (size_t(p * VPU + h) * 16 + nn) * NW, min(NW, nsl));
    }
    const M1Sel<NWT> vsel(a, v0 + p * VPU);
    const int wsel = NWT == 2 ? 0 : vsel.w;
    const int n = vsel.s * 16 + nn;
    if (n >= NAD_M1_FIELD(a, wsel, n)) continue;
    float* out = NAD_M1_FIELD(a, wsel, out);
    if constexpr (NWT == 2) {  // SiLU(gate) * up
      const float t1 = silu_f(y[0]);
      if (a.aux) a.aux[n] = t1;
      out[n] = t1 * y[VPU - 1];
    } else {
      out[n] = y[0];
    }
  }
  NAD_TRACE(3);
}

}  // namespace nad
