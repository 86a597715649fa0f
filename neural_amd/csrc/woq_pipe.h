// woq_pipe.h -- the LDS-DMA pipeline layer of the prefill GEMMs (gemm3 in woq_gemm2.hip, woq_gemm4.hip, woq_gemm7.hip):
// global / buffer -> LDS DMAs, counted waits and the inline-asm LDS reads that go with them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "woq_device.h"

namespace nad {

// LDS-DMA from a flat global address: 16 or 4 bytes per lane, the LDS image is lane-linear from `l`
__device__ __forceinline__ void glds16(const void* g, char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* g, char* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 4, 0, 0);
}
// LDS-DMA as raw buffer loads: 32-bit per-lane offsets fixed for the whole K loop, the moving part in an SGPR
__device__ __forceinline__ void blds16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, char* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)l, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void blds4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, char* l) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)l, 4, voff, soff, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS reads in inline asm: hipcc puts a vmcnt(0) in front of every LDS read it can see while an LDS-DMA is in flight
// (it cannot tell the buffers of one __shared__ array apart), which would drain the whole prefetch each half step.
// Results are consumed only after an explicit lgkmcnt wait that names them (wait_lgk below).
template <int OFF>
__device__ __forceinline__ h8_t lds_b128(uint32_t addr) {
  h8_t r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ u4_t lds_u128(uint32_t addr) {
  u4_t r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ uint2 lds_b64(uint32_t addr) {
  uint2 r;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
template <int OFF>
__device__ __forceinline__ uint32_t lds_b32(uint32_t addr) {
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
__device__ __forceinline__ uint32_t lds_b32v(uint32_t addr) {  // runtime offset folded into the address
  uint32_t r;
  asm volatile("ds_read_b32 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
// A fragments B + I (I = 0 ..) of rows 16 apart, ROWB bytes a row, into f[B + I]
template <int ROWB, int B, size_t... I>
__device__ __forceinline__ void read_frags(h8_t* f, uint32_t addr, std::index_sequence<I...>) {
  ((f[B + I] = lds_b128<int(B + I) * 16 * ROWB>(addr)), ...);
}
template <class T>
__device__ __forceinline__ void tie(T& r) {
  asm volatile("" : "+v"(r));
}
template <int B, size_t... I>
__device__ __forceinline__ void tie_frags(h8_t* f, std::index_sequence<I...>) {
  (tie(f[B + I]), ...);
}
template <int N, class... T>
__device__ __forceinline__ void wait_lgk(T&... regs) {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N));
  (tie(regs), ...);  // each result is redefined after the wait: no use can be scheduled above it
}
__device__ __forceinline__ uint32_t lds_addr(const char* p) {
  return uint32_t(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) char*)p));
}

}  // namespace nad
