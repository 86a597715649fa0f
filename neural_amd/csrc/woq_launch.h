// woq_launch.h -- host side: launching a kernel that may need more than the default 64 KiB of dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>

namespace nad {

// Launch kernel K with `lds` bytes of dynamic LDS.  A launch above 64 KiB first opts K in to the CU's whole 160 KiB,
// once: the flag is K's own (one instance of this template per kernel instantiation).  Not for a kernel with static
// __shared__ as it stands: 160 KiB of dynamic LDS plus the static part would exceed the CU.
template <auto K, class... Args>
static hipError_t launch_big_lds(dim3 g, dim3 b, size_t lds, hipStream_t st, const Args&... args) {
  static bool attr_set = false;
  if (!attr_set && lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(K, g, b, lds, st, args...);
  return hipGetLastError();
}

}  // namespace nad
