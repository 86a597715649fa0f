// woq_gemv_b2.hip -- the int2 instantiations of woq_gemv_m1_kernel (3 scale types each), with its batched form.
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

hipError_t gemv_m1_launch_b2(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (gpt == 1) return gemv_m1_launch2<2, 1>(a, g, b, lds, st);
  if (gpt == 2) return gemv_m1_launch2<2, 2>(a, g, b, lds, st);
  if (gpt == 4 && !a.asym)
    return by_act(a, [&](auto at) { return gemv_m1_launch4<2, 4, at.value, false>(a, g, b, lds, st); });
  return hipErrorInvalidValue;
}

}  // namespace nad
