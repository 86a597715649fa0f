// woq_gemv_r7.hip -- launch_gemv_routed_general and the instantiations of woq_gemv_routed_kernel.
#include "woq_gemv.h"
#include "woq_gemv_launch.h"

namespace nad {

// woq_gemv_routed_kernel: the launches of launch_gemv at M = 1 with fp32 rows that lean_ok does not take, in the
// formats an expert bank holds -- int4 groups of 32 (four per K tile, sym), int8 groups of 32 (two per 64-deep tile)
// and of 64 * 2^j or one per channel (one per tile), sym and asym
hipError_t launch_gemv_routed_general(const GemvArgs& a, const GemvRouted& r, int bits, int waves, int grid, size_t lds,
                                      hipStream_t stream) {
  int tpg = 0;
  const int gpt = gemv_groups_per_tile(bits, a.nt, a.ng, a.bs, &tpg);
  if (a.batch || a.act_t != kActF32 || a.M != 1 || r.wpp <= 0 || r.slots <= 0 || r.n_expert <= 0 ||
      waves * 64 > (gpt == 1 ? 1024 : 512) || lean_ok(a, bits, waves))
    return hipErrorInvalidValue;
  const dim3 g(grid), b(waves * 64);
  if (bits == 4 && gpt == 4 && !a.asym) return launch_big_lds<woq_gemv_routed_kernel<4, 4, false>>(g, b, lds, stream, a, r);
  if (bits != 8 || (gpt != 1 && gpt != 2)) return hipErrorInvalidValue;
  return by_asym(a, [&](auto as) {
    return gpt == 1 ? launch_big_lds<woq_gemv_routed_kernel<8, 1, as.value>>(g, b, lds, stream, a, r)
                    : launch_big_lds<woq_gemv_routed_kernel<8, 2, as.value>>(g, b, lds, stream, a, r);
  });
}

}  // namespace nad
