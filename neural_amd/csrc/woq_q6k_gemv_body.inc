// The body of woq_q6k_gemv_kernel and woq_q6k_gemv_routed_kernel (woq_q6k.hip), included into each.  The including
// kernel defines:
//   Q6K_ROWS_PP    activation rows per pass (the LDS rows reserved)
//   Q6K_WG_ROW0    the first activation row of this workgroup's pass
//   Q6K_WG_INDEX   the workgroup's first stripe; it takes every Q6K_WG_COUNT-th from there
// and q6k_lds (the dynamic LDS), AT and HILO (the activation type; fp16 hi / lo rows) and a (the GemmArgs).
  const SkinnyWeight& W = a.w;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar
  const int nl = lane & 15, kq = lane >> 4;
  const int nsb = W.nt, ns = W.ns, K = a.K;
  const int row0 = Q6K_WG_ROW0;
  const int mloc = min(Q6K_ROWS_PP, a.M - row0);
  const int rows = HILO ? 2 * mloc : mloc;                         // fp16 rows in LDS
  const size_t row_bytes = size_t(K) * 2;
  float* part = reinterpret_cast<float*>(q6k_lds + size_t(HILO ? 2 * Q6K_ROWS_PP : Q6K_ROWS_PP) * row_bytes);

  const u4_t* qp = static_cast<const u4_t*>(W.tiles);
  const u4_t* scp = reinterpret_cast<const u4_t*>(W.zps);
  const u4_t* dp = static_cast<const u4_t*>(W.scales);
  const bool has = wave < nsb;
  u4_t c0{}, c1{}, c2{}, csc{}, cd{};
  auto fetch = [&](int s, int b, u4_t& l0, u4_t& l1, u4_t& h, u4_t& sc, u4_t& d) {
    const size_t sb = size_t(s) * nsb + b;
    const u4_t* t = qp + sb * 192 + lane;
    l0 = __builtin_nontemporal_load(t);
    l1 = __builtin_nontemporal_load(t + 64);
    h = __builtin_nontemporal_load(t + 128);
    sc = __builtin_nontemporal_load(scp + sb * 16 + nl);
    d = __builtin_nontemporal_load(dp + sb * 2 + (nl >> 3));
  };
  int s = Q6K_WG_INDEX;
  if (has && s < ns) fetch(s, wave, c0, c1, c2, csc, cd);

  // stage the activations: one 8-element chunk per thread and step
  {
    const int chunks = K / 8;
    const bool vec_ok = a.vec_ok != 0;
    for (int i = threadIdx.x; i < mloc * chunks; i += kQ6kWaves * 64) {
      const int r = i / chunks, c = i % chunks;
      float v[8];
      load_a8<AT>(a.A, a.lda, row0 + r, c * 8, K, nullptr, vec_ok, v);
      h8_t hi;
#pragma unroll
      for (int j = 0; j < 8; j++) hi[j] = _Float16(v[j]);
      if constexpr (HILO) {
        h8_t lo;
#pragma unroll
        for (int j = 0; j < 8; j++) lo[j] = _Float16(v[j] - float(hi[j]));
        *reinterpret_cast<h8_t*>(q6k_lds + size_t(2 * r) * row_bytes + size_t(c ^ ((2 * r) & 15)) * 16) = hi;
        *reinterpret_cast<h8_t*>(q6k_lds + size_t(2 * r + 1) * row_bytes + size_t(c ^ ((2 * r + 1) & 15)) * 16) = lo;
      } else {
        *reinterpret_cast<h8_t*>(q6k_lds + size_t(r) * row_bytes + size_t(c ^ (r & 15)) * 16) = hi;
      }
    }
  }
  __syncthreads();

  const h2_t m1056 = splat(-1056.f);
  const f4_t zero4{0.f, 0.f, 0.f, 0.f};
  // this lane's A fragments: row nl of LDS, four fp16 at k = 256 b + 16 g + 4 kq.  A lane past the staged rows reads
  // row 0 instead (in bounds, finite): its row of the product is one nobody reads
  const bool arow = nl < rows;
  const char* abase = q6k_lds + size_t(arow ? nl : 0) * row_bytes + (kq & 1) * 8;
  for (int it = 0; s < ns; s += Q6K_WG_COUNT, it++) {
    f4_t acc = zero4;
    if (has) {
      for (int b = wave; b < nsb; b += kQ6kWaves) {
        int s2 = s, b2 = b + kQ6kWaves;
        if (b2 >= nsb) {
          s2 = s + Q6K_WG_COUNT;
          b2 = wave;
        }
        u4_t n0 = c0, n1 = c1, n2 = c2, nsc = csc, nd = cd;
        if (s2 < ns) fetch(s2, b2, n0, n1, n2, nsc, nd);
        f4_t sbacc = zero4;
        auto group = [&](auto gc) {
          constexpr int G = decltype(gc)::value;
          const h4_t af = *reinterpret_cast<const h4_t*>(abase + size_t((32 * b + 2 * G + (kq >> 1)) ^ nl) * 16);
          const f4_t p = __builtin_amdgcn_mfma_f32_16x16x16f16(af, q6k_group<G>(c0, c1, c2, m1056), zero4, 0, 0, 0);
          const float scf = float(q6k_sc(csc, G));
#pragma unroll
          for (int r = 0; r < 4; r++) sbacc[r] = __builtin_fmaf(scf, p[r], sbacc[r]);
        };
        group(std::integral_constant<int, 0>{});
        group(std::integral_constant<int, 1>{});
        group(std::integral_constant<int, 2>{});
        group(std::integral_constant<int, 3>{});
        group(std::integral_constant<int, 4>{});
        group(std::integral_constant<int, 5>{});
        group(std::integral_constant<int, 6>{});
        group(std::integral_constant<int, 7>{});
        group(std::integral_constant<int, 8>{});
        group(std::integral_constant<int, 9>{});
        group(std::integral_constant<int, 10>{});
        group(std::integral_constant<int, 11>{});
        group(std::integral_constant<int, 12>{});
        group(std::integral_constant<int, 13>{});
        group(std::integral_constant<int, 14>{});
        group(std::integral_constant<int, 15>{});
        const float df = q6k_d(cd, nl);
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = __builtin_fmaf(df, sbacc[r], acc[r]);
        c0 = n0;
        c1 = n1;
        c2 = n2;
        csc = nsc;
        cd = nd;
      }
    }
    // partial of this wave: C layout row = 4 kq + r, column nl
    float* slot = part + size_t(it & 1) * (kQ6kWaves * 256);
#pragma unroll
    for (int r = 0; r < 4; r++) slot[wave * 256 + (4 * kq + r) * 16 + nl] = acc[r];
    __syncthreads();
    if (wave == (it & (kQ6kWaves - 1))) {
      const int row = lane >> 2, n0 = 4 * (lane & 3);
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int w = 0; w < kQ6kWaves; w++) {  // wave order; four reads in flight (sixteen would spill)
        const float4 pv = *reinterpret_cast<const float4*>(slot + w * 256 + row * 16 + n0);
        v[0] += pv.x;
        v[1] += pv.y;
        v[2] += pv.z;
        v[3] += pv.w;
      }
      int orow = row;
      bool valid = row < mloc;
      if constexpr (HILO) {  // rows 2 i (hi) and 2 i + 1 (lo) sit four lanes apart
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float other = __shfl_xor(v[e], 4);
          v[e] = (row & 1) ? other + v[e] : v[e] + other;
        }
        orow = row >> 1;
        valid = (row & 1) == 0 && orow < mloc;
      }
      if (valid && s * 16 + n0 < W.n) gemm_epilogue4(a, row0 + orow, s * 16 + n0, v);
    }
  }
