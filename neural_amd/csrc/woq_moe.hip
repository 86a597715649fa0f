// woq_moe.hip -- the small kernels around the routed expert matmuls (woq_gemv_m1_routed_kernel, woq_gemv.h) of a
// Mixtral-style FFN (models/llama/llama.cpp:620-688): the router (softmax -> top_k -> renormalise, :624-638), alone or
// behind the ffn_gate_inp matmul of an unquantized gate in the same launch (:631), and the weighted sum of the slot
// results (ne_mul then ne_add per slot, :676-679); and around the sorted, grouped form (woq_gemm7_grouped_kernel,
// woq_gemm7.hip): the sort of the problems by expert and the same sum over sorted rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "woq_kernels.h"

// Both kernels here are defined by separately rounded fp32 operations.  hipcc contracts a * b + c into an fma by
// default, and HIP's __fmul_rn / __fadd_rn are plain * and + compiled under that default in its headers (they fused
// here: v_fmac_f32), so the operations are written as * + / under this pragma instead.
#pragma clang fp contract(off)

namespace nad {

// out[r][n] = ((w[r][0] * y[r * top_k][n]) + w[r][1] * y[r * top_k + 1][n]) + ...  Every product and every sum is
// rounded on its own (no fma), in slot order: numpy float32 reproduces it bit for bit.
__global__ __launch_bounds__(256) void moe_combine_kernel(MoeCombineArgs a) {
  // workgroup r * nb + j: columns [256 j, 256 j + 256) of row r
  const int nb = (a.n + 255) / 256, r = int(blockIdx.x) / nb;
  const int n = (int(blockIdx.x) - r * nb) * 256 + int(threadIdx.x);
  if (n >= a.n) return;
  const float* y = a.y + size_t(r) * a.top_k * a.ldy + n;
  const float* w = a.wts + size_t(r) * a.wts_ld;
  float s = w[0] * y[0];
  for (int i = 1; i < a.top_k; i++) s = s + w[i] * y[size_t(i) * a.ldy];
  a.out[size_t(r) * a.ldo + n] = s;
}

LaunchShape moe_combine_shape(int m, int n) { return {int(unsigned((n + 255) / 256) * unsigned(m)), 256}; }
hipError_t launch_moe_combine(const MoeCombineArgs& a, hipStream_t stream) {
  const LaunchShape s = moe_combine_shape(a.m, a.n);
  hipLaunchKernelGGL(moe_combine_kernel, dim3(unsigned(s.grid)), dim3(s.block), 0, stream, a);
  return hipGetLastError();
}

// The router of one row on one wave; lane l holds expert l's logit x (n_expert <= 64; a lane past n_expert: -inf).
// All in fp32:
//   p = exp(x - max x) / sum exp(x - max x)      (the sum over the lanes as a butterfly: the same value in every lane)
//   top_k rounds of arg max over the experts not yet taken, a tie going to the lower index
//   wts[i] = p[ids[i]] / (p[ids[0]] + p[ids[1]] + ...), the sum added in slot order
// ids and wts are the row's own.  moe_route_kernel and moe_gate_route_kernel both route through it.
__device__ __forceinline__ void moe_route_wave(float x, int lane, int n_expert, int top_k, int32_t* ids, float* wts) {
  const bool live = lane < n_expert;
  float mx = x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float e = live ? expf(x - mx) : 0.f;
  float sum = e;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_xor(sum, o, 64);
  const float p = e / sum;
  float v = live ? p : -1.f;  // -1: not a candidate (a lane past n_expert, or an expert already taken)
  float mine = 0.f, tot = 0.f;  // lane i < top_k: p of slot i; the slots' sum
  for (int i = 0; i < top_k; i++) {
    float bv = v;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    bi = __builtin_amdgcn_readfirstlane(bi);
    const float ps = __shfl(p, bi, 64);
    if (lane == bi) v = -1.f;
    if (lane == i) mine = ps;
    tot = i == 0 ? ps : tot + ps;
    if (lane == 0) ids[i] = bi;
  }
  if (lane < top_k) wts[lane] = mine / tot;
}

// One wave per row (nad_moe_route)
__global__ __launch_bounds__(64) void moe_route_kernel(MoeRouteArgs a) {
  const int r = int(blockIdx.x), lane = int(threadIdx.x);
  const float x = lane < a.n_expert ? a.logits[size_t(r) * a.ld + lane] : -INFINITY;
  moe_route_wave(x, lane, a.n_expert, a.top_k, a.ids + size_t(r) * a.ids_ld, a.wts + size_t(r) * a.wts_ld);
}

hipError_t launch_moe_route(const MoeRouteArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(moe_route_kernel, dim3(a.m), dim3(64), 0, stream, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ gate matmul + route
// logits[r][e] = act[r] . gate[e] and the router on them, one workgroup of 16 waves per row (MoeGateRouteArgs,
// woq_kernels.h; the order of the sums is the contract of nad_moe_gate_route, include/neural_amd.h):
//   1. thread t is slot t: per pass of 4096 elements one 16-byte load of x at k = 4 (t + 1024 pass), and per expert one
//      16-byte (fp32) or 8-byte (fp16, bf16) load of the gate at the same k.  The loads of kGateBatch experts are issued
//      before their multiply-adds; acc[e] carries across the passes.  K % 4 == 0, so a slot's four elements are all
//      inside K or all outside.
//   2. per expert the xor butterfly over the wave; lane e keeps expert e's sum and writes it to part[wave][e] (LDS).
//   3. after the one barrier lane e of wave 0 adds the 16 partials in wave order: logit e, the lane layout
//      moe_route_wave starts from.
// NEB bounds n_expert at compile time: acc[] is indexed by unrolled constants only and stays in registers.
constexpr int kGateWaves = 16, kGateSlots = kGateWaves * 64, kGateBatch = 8;

template <class W>
struct GateLoad;
template <>
struct GateLoad<float> {
  using Raw = float4;
  static __device__ __forceinline__ float4 widen(const float4& v) { return v; }
};
template <>
struct GateLoad<_Float16> {
  using Raw = uint2;  // four fp16
  static __device__ __forceinline__ float4 widen(const uint2& v) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 a = __builtin_bit_cast(h2, v.x), b = __builtin_bit_cast(h2, v.y);
    return make_float4(float(a.x), float(a.y), float(b.x), float(b.y));
  }
};
struct GateBf16 {};
template <>
struct GateLoad<GateBf16> {
  using Raw = uint2;  // four bf16: the upper halves of their fp32 values
  static __device__ __forceinline__ float4 widen(const uint2& v) {
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xffff0000u));
  }
};

template <int NEB, class W>
__global__ __launch_bounds__(kGateSlots) void moe_gate_route_kernel(MoeGateRouteArgs a) {
  using Raw = typename GateLoad<W>::Raw;
  extern __shared__ float gate_part[];  // [kGateWaves][n_expert]
  const int r = int(blockIdx.x), t = int(threadIdx.x), lane = t & 63, wave = t >> 6;
  const int ne = a.n_expert;
  const float* x = a.act + size_t(r) * a.lda;
  const Raw* g = static_cast<const Raw*>(a.gate);  // a Raw holds four elements; ldw % 4 == 0
  const size_t ldw4 = size_t(a.ldw >> 2);
  float acc[NEB];
#pragma unroll
  for (int e = 0; e < NEB; e++) acc[e] = 0.0f;
  for (int k = 4 * t; k < a.k; k += 4 * kGateSlots) {
    const float4 xv = *reinterpret_cast<const float4*>(x + k);
    const Raw* gk = g + (k >> 2);
#pragma unroll
    for (int e0 = 0; e0 < NEB; e0 += kGateBatch) {
      if (e0 >= ne) continue;  // uniform; no break: the loops unroll fully, so acc[] is indexed by constants
      Raw raw[kGateBatch];
#pragma unroll
      for (int j = 0; j < kGateBatch; j++)
        if (e0 + j < ne) raw[j] = gk[size_t(e0 + j) * ldw4];
#pragma unroll
      for (int j = 0; j < kGateBatch; j++)
        if (e0 + j < ne) {
          const float4 w = GateLoad<W>::widen(raw[j]);
          float s = acc[e0 + j];
          s = s + xv.x * w.x;
          s = s + xv.y * w.y;
          s = s + xv.z * w.z;
          s = s + xv.w * w.w;
          acc[e0 + j] = s;
        }
    }
  }
  float mine = 0.0f;  // lane e: the wave's sum of expert e
#pragma unroll
  for (int e = 0; e < NEB; e++) {
    if (e >= ne) continue;
    float s = acc[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    if (lane == e) mine = s;
  }
  if (lane < ne) gate_part[wave * ne + lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  float logit = -INFINITY;
  if (lane < ne) {
    logit = gate_part[lane];
    for (int w = 1; w < kGateWaves; w++) logit = logit + gate_part[w * ne + lane];
    if (a.logits) a.logits[size_t(r) * a.logits_ld + lane] = logit;
  }
  moe_route_wave(logit, lane, ne, a.top_k, a.ids + size_t(r) * a.ids_ld, a.wts + size_t(r) * a.wts_ld);
}

LaunchShape moe_gate_route_shape(int m) { return {m, kGateSlots}; }
size_t moe_gate_route_lds(int n_expert) { return size_t(kGateWaves) * size_t(n_expert) * sizeof(float); }

template <class W>
static hipError_t launch_gate_route_as(const MoeGateRouteArgs& a, hipStream_t stream) {
  const LaunchShape s = moe_gate_route_shape(a.m);
  const size_t lds = moe_gate_route_lds(a.n_expert);
  const dim3 grid(unsigned(s.grid)), block(s.block);
  if (a.n_expert <= 8)
    hipLaunchKernelGGL((moe_gate_route_kernel<8, W>), grid, block, lds, stream, a);
  else if (a.n_expert <= 16)
    hipLaunchKernelGGL((moe_gate_route_kernel<16, W>), grid, block, lds, stream, a);
  else
    hipLaunchKernelGGL((moe_gate_route_kernel<64, W>), grid, block, lds, stream, a);
  return hipGetLastError();
}

hipError_t launch_moe_gate_route(const MoeGateRouteArgs& a, hipStream_t stream) {
  if (a.n_expert < 1 || a.n_expert > 64 || a.m < 1) return hipErrorInvalidValue;
  switch (a.gate_t) {
    case kActF32: return launch_gate_route_as<float>(a, stream);
    case kActF16: return launch_gate_route_as<_Float16>(a, stream);
    case kActBF16: return launch_gate_route_as<GateBf16>(a, stream);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------------------------------------ grouped: the sort
// The stable counting sort of the problems by expert (MoeSortArgs, woq_kernels.h), one workgroup of 16 waves.  Wave w
// owns the contiguous problems [w * seg, (w + 1) * seg) and walks them 64 at a time, twice:
//   1. cnt[w][e] = its problems of expert e.  The lanes of one expert in a block of 64 are found by ballot, one expert
//      per round (as many rounds as the block has experts), and counted by popcount.
//   2. wave 0 scans the totals: offs[] and the first tile of every expert; cnt[w][e] becomes the exclusive sum over the
//      waves, i.e. how many problems of e lie before wave w's.
//   3. the same walk again: problem p of expert e in lane l goes to offs[e] + cnt[w][e] + (lanes of e below l), then
//      cnt[w][e] moves on by the block's count.
// Every position is a sum of counts of problems before p: no atomic decides anything, two runs write the same bytes.
constexpr int kSortWaves = 16, kSortMaxE = 256;

__global__ __launch_bounds__(kSortWaves * 64) void moe_sort_kernel(MoeSortArgs a) {
  __shared__ int cnt[kSortWaves][kSortMaxE];
  __shared__ int tot[kSortMaxE], offs_s[kSortMaxE + 1], tb[kSortMaxE + 1];
  const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int ne = a.n_expert, np = a.m * a.top_k;
  const int seg = (np + kSortWaves * 64 - 1) / (kSortWaves * 64) * 64;
  const int p0 = min(np, wave * seg), p1 = min(np, p0 + seg);
  for (int i = tid; i < kSortWaves * kSortMaxE; i += kSortWaves * 64) (&cnt[0][0])[i] = 0;
  __syncthreads();

  // one block of 64 problems: fn(expert, the lanes of that expert) once per expert present, in lane order of the
  // expert's first problem; returns this lane's id
  auto block = [&](int b, auto&& fn) {
    const int p = b + lane;
    int e = -1;
    if (p < p1) {
      const int r = p / a.top_k;
      e = a.ids[size_t(r) * a.ids_ld + (p - r * a.top_k)];
    }
    const bool valid = unsigned(e) < unsigned(ne);
    unsigned long long todo = __ballot(valid);
    while (todo) {
      const int ef = __builtin_amdgcn_readfirstlane(__shfl(e, __ffsll(todo) - 1, 64));
      const unsigned long long mk = __ballot(valid && e == ef);
      fn(ef, mk, valid && e == ef, p);
      todo &= ~mk;
    }
    return valid;
  };

  for (int b = p0; b < p1; b += 64)
    block(b, [&](int ef, unsigned long long mk, bool, int) {
      if (lane == 0) cnt[wave][ef] += __popcll(mk);
    });
  __syncthreads();

  if (tid < ne) {
    int s = 0;
    for (int w = 0; w < kSortWaves; w++) {
      const int c = cnt[w][tid];
      cnt[w][tid] = s;
      s += c;
    }
    tot[tid] = s;
  }
  __syncthreads();
  if (wave == 0) {  // lane l: experts 4 l .. 4 l + 3
    int c[4], sc = 0, st = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      c[j] = lane * 4 + j < ne ? tot[lane * 4 + j] : 0;
      sc += c[j];
      st += (c[j] + a.bm - 1) / a.bm;
    }
    int ic = sc, it = st;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int uc = __shfl_up(ic, o, 64), ut = __shfl_up(it, o, 64);
      if (lane >= o) {
        ic += uc;
        it += ut;
      }
    }
    int rc = ic - sc, rt = it - st;
    if (lane == 0) offs_s[0] = tb[0] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rc += c[j];
      rt += (c[j] + a.bm - 1) / a.bm;
      if (lane * 4 + j < ne) {
        offs_s[lane * 4 + j + 1] = rc;
        tb[lane * 4 + j + 1] = rt;
      }
    }
  }
  __syncthreads();

  const int nvalid = offs_s[ne], ntiles = tb[ne];
  if (tid <= ne) a.offs[tid] = offs_s[tid];
  if (tid == 0) a.ntiles[0] = ntiles;
  for (int t = tid; t < ntiles; t += kSortWaves * 64) {
    int lo = 0, hi = ne;  // the expert with tb[e] <= t < tb[e + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tb[mid] <= t) lo = mid; else hi = mid;
    }
    const int q0 = offs_s[lo] + (t - tb[lo]) * a.bm;
    a.tiles[t] = make_int4(lo, q0, min(q0 + a.bm, offs_s[lo + 1]), 0);
  }
  for (int q = nvalid + tid; q < np; q += kSortWaves * 64) {
    a.perm[q] = -1;
    a.src[q] = 0;
  }

  for (int b = p0; b < p1; b += 64) {
    const bool valid = block(b, [&](int ef, unsigned long long mk, bool mine, int p) {
      const int base = offs_s[ef] + cnt[wave][ef];
      if (mine) {
        const int q = base + __popcll(mk & ((1ull << lane) - 1ull));
        a.perm[q] = p;
        a.src[q] = p / a.top_k;
        a.inv[p] = q;
      }
      if (lane == 0) cnt[wave][ef] = base - offs_s[ef] + __popcll(mk);
    });
    if (!valid && b + lane < p1) a.inv[b + lane] = -1;
  }
}

LaunchShape moe_sort_shape() { return {1, kSortWaves * 64}; }
hipError_t launch_moe_sort(const MoeSortArgs& a, hipStream_t stream) {
  if (a.n_expert < 1 || a.n_expert > kSortMaxE || a.bm < 1) return hipErrorInvalidValue;
  const LaunchShape s = moe_sort_shape();
  hipLaunchKernelGGL(moe_sort_kernel, dim3(s.grid), dim3(s.block), 0, stream, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ grouped: the way back
// moe_combine_kernel's sum over the sorted rows (MoeGatherArgs): slot i of row r lies at y[inv[r * top_k + i]], an
// invalid slot reads 0.0f
__global__ __launch_bounds__(256) void moe_gather_kernel(MoeGatherArgs a) {
  const int nb = (a.n + 255) / 256, r = int(blockIdx.x) / nb;
  const int n = (int(blockIdx.x) - r * nb) * 256 + int(threadIdx.x);
  if (n >= a.n) return;
  const int32_t* inv = a.inv + size_t(r) * a.top_k;
  auto y = [&](int i) {
    const int q = inv[i];
    return q >= 0 ? a.y[size_t(q) * a.ldy + n] : 0.0f;
  };
  float s;
  if (a.wts) {
    const float* w = a.wts + size_t(r) * a.wts_ld;
    s = w[0] * y(0);
    for (int i = 1; i < a.top_k; i++) s = s + w[i] * y(i);
  } else {
    s = y(0);
  }
  a.out[size_t(r) * a.ldo + n] = s;
}

hipError_t launch_moe_gather(const MoeGatherArgs& a, hipStream_t stream) {
  const LaunchShape s = moe_combine_shape(a.m, a.n);  // moe_combine_kernel's indexing
  hipLaunchKernelGGL(moe_gather_kernel, dim3(unsigned(s.grid)), dim3(s.block), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nad
