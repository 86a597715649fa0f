// woq_moe.hip -- the two small kernels around the routed expert matmuls (woq_gemv_m1_routed_kernel, woq_gemv.hip) of a
// Mixtral-style FFN (models/llama/llama.cpp:620-688): the router (softmax -> top_k -> renormalise, :624-638) and the
// weighted sum of the slot results (ne_mul then ne_add per slot, :676-679).
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

hipError_t launch_moe_combine(const MoeCombineArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3(unsigned((a.n + 255) / 256) * unsigned(a.m)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// One wave per row; lane l holds expert l (n_expert <= 64).  All in fp32:
//   p = exp(x - max x) / sum exp(x - max x)      (the sum over the lanes as a butterfly: the same value in every lane)
//   top_k rounds of arg max over the experts not yet taken, a tie going to the lower index
//   wts[i] = p[ids[i]] / (p[ids[0]] + p[ids[1]] + ...), the sum added in slot order
__global__ __launch_bounds__(64) void moe_route_kernel(MoeRouteArgs a) {
  const int r = int(blockIdx.x), lane = int(threadIdx.x);
  const bool live = lane < a.n_expert;
  const float x = live ? a.logits[size_t(r) * a.ld + lane] : -INFINITY;
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
  for (int i = 0; i < a.top_k; i++) {
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
    if (lane == 0) a.ids[size_t(r) * a.ids_ld + i] = bi;
  }
  if (lane < a.top_k) a.wts[size_t(r) * a.wts_ld + lane] = mine / tot;
}

hipError_t launch_moe_route(const MoeRouteArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(moe_route_kernel, dim3(a.m), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nad
