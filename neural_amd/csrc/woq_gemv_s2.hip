// woq_gemv_s2.hip -- the int4 instantiations of woq_gemv_m1s_kernel (compiled with the kernarg-preload flag).
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

// int4: every activation type at one group per tile, fp32 activations at two
bool gemv_m1s_launch_b4(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e) {
  if (gpt == 1)
    return by_act(a, [&](auto at) {
      return by_asym(a, [&](auto as) { return m1s_launch3<4, 1, at.value, as.value, -1>(a, g, b, lds, st, e); });
    });
  if (gpt == 2 && a.act_t == kActF32)
    return by_asym(a, [&](auto as) { return m1s_launch3<4, 2, kActF32, as.value, -1>(a, g, b, lds, st, e); });
  return false;
}

}  // namespace nad
