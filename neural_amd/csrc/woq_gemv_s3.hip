// woq_gemv_s3.hip -- the int2 instantiations of woq_gemv_m1s_kernel (compiled with the kernarg-preload flag).
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

// int2: symmetric weights with fp32 activations, each scale type (as woq_gemv_m1_kernel's int2 instantiations)
template <int GPT>
static bool m1s_launch_b2g(const GemvArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e) {
  if (a.scale_t == kScaleF32) return m1s_launch3<2, GPT, kActF32, false, NAD_INT2_ST ? kScaleF32 : -1>(a, g, b, lds, st, e);
  if (a.scale_t == kScaleBF16) return m1s_launch3<2, GPT, kActF32, false, NAD_INT2_ST ? kScaleBF16 : -1>(a, g, b, lds, st, e);
  return m1s_launch3<2, GPT, kActF32, false, NAD_INT2_ST ? kScaleF16 : -1>(a, g, b, lds, st, e);
}
bool gemv_m1s_launch_b2(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e) {
  if (a.asym || a.act_t != kActF32) return false;
  if (gpt == 1) return m1s_launch_b2g<1>(a, g, b, lds, st, e);
  if (gpt == 2) return m1s_launch_b2g<2>(a, g, b, lds, st, e);
  if (gpt == 4) return m1s_launch_b2g<4>(a, g, b, lds, st, e);
  return false;
}

}  // namespace nad
