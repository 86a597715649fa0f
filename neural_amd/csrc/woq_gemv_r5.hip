// woq_gemv_r5.hip -- the int2 instantiations of woq_gemv_m1_routed_kernel.
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

// int2: the scale type at compile time, as woq_gemv_m1_kernel's int2 instantiations
template <int GPT, bool ASYM>
static hipError_t routed_launch_b2g(const GemvArgs& a, const GemvRouted& r, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (a.scale_t == kScaleF32) return routed_launch2<2, GPT, ASYM, NAD_INT2_ST ? kScaleF32 : -1>(a, r, g, b, lds, st);
  if (a.scale_t == kScaleBF16) return routed_launch2<2, GPT, ASYM, NAD_INT2_ST ? kScaleBF16 : -1>(a, r, g, b, lds, st);
  return routed_launch2<2, GPT, ASYM, NAD_INT2_ST ? kScaleF16 : -1>(a, r, g, b, lds, st);
}
hipError_t gemv_routed_launch_b2(const GemvArgs& a, const GemvRouted& r, int gpt, dim3 g, dim3 b, size_t lds,
                                 hipStream_t st) {
  if (gpt == 4 && !a.asym) return routed_launch_b2g<4, false>(a, r, g, b, lds, st);
  if (gpt != 1 && gpt != 2) return hipErrorInvalidValue;
  return by_asym(a, [&](auto as) {
    return gpt == 1 ? routed_launch_b2g<1, as.value>(a, r, g, b, lds, st) : routed_launch_b2g<2, as.value>(a, r, g, b, lds, st);
  });
}

}  // namespace nad
