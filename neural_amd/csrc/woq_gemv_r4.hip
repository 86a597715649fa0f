// woq_gemv_r4.hip -- launch_gemv_routed and the int4 instantiations of woq_gemv_m1_routed_kernel.
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

hipError_t launch_gemv_routed(const GemvArgs& a, const GemvRouted& r, int bits, int waves, int grid, size_t lds,
                              hipStream_t stream) {
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(bits, a.nt, a.ng, a.bs, &tpg);
  if (gpt == 0 || a.batch || a.act_t != kActF32 || r.wpp <= 0 || r.slots <= 0 || r.n_expert <= 0 ||
      !lean_ok(a, bits, waves))
    return hipErrorInvalidValue;
  const dim3 g(grid), b(waves * 64);
  if (bits == 2) return gemv_routed_launch_b2(a, r, gpt, g, b, lds, stream);
  if (bits != 4 || (gpt != 1 && gpt != 2)) return hipErrorInvalidValue;
  return by_asym(a, [&](auto as) {
    return gpt == 1 ? routed_launch2<4, 1, as.value, -1>(a, r, g, b, lds, stream)
                    : routed_launch2<4, 2, as.value, -1>(a, r, g, b, lds, stream);
  });
}

}  // namespace nad
