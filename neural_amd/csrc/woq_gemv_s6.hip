// woq_gemv_s6.hip -- the load-ahead forms of woq_gemv_m1s_kernel (m1s_ahead_form says which launches they serve;
// compiled with the kernarg-preload flag).
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

hipError_t gemv_m1s_ahead_launch(const GemvArgs& a, int form, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  return by_asym(a, [&](auto as) {
    constexpr bool AS = as.value;
    if (form == 1) return m1s_go<4, 1, kActF32, AS, 2, 1, 1, -1, 1, 16, true>(a, g, b, lds, st);
    if (form == 2) return m1s_go<4, 1, kActF32, AS, 2, 1, 1, -1, 2, 16, true>(a, g, b, lds, st);
    return m1s_go<4, 1, kActF32, AS, 2, 1, 1, -1, 3, 16, true>(a, g, b, lds, st);
  });
}

}  // namespace nad
