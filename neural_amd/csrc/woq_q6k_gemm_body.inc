// The body of woq_q6k_gemm_kernel and woq_q6k_gemm_grouped_kernel (woq_q6k.hip), included into each.  The including
// kernel defines:
//   Q6K_GEMM_TILE          declarations of W (the weight read), bn (the column tile) and m0 (the tile's first output row)
//   Q6K_GEMM_M             one past the tile's last output row is min(m0 + 128, Q6K_GEMM_M)
//   Q6K_GEMM_A_ROWS        declarations ahead of the K loop that Q6K_GEMM_A_ROW may use (r0: the thread's first tile row)
//   Q6K_GEMM_A_ROW(p, row) the A row of output row row = m0 + r0 + 32 p
// and AT (the activation type) and a (the GemmArgs; the epilogue writes through a.w).
  constexpr int KT = 128, BM = 128, ROWB = KT * 2, CHUNKS = ROWB / 16;
  __shared__ __attribute__((aligned(16))) char lds_a[BM * ROWB];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar
  const int wm = wave >> 1, wn = wave & 1;
  const int nl = lane & 15, kq = lane >> 4;
  Q6K_GEMM_TILE
  const int s0 = bn * 8 + wn * 4;
  const int nsb = W.nt;

  f4_t acc[2][4], accsb[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = accsb[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};

  const int ch = threadIdx.x % CHUNKS;  // 16 chunks of 8 k; 32 rows per pass, 4 passes
  const int r0 = threadIdx.x / CHUNKS;
  const bool vec_ok = a.vec_ok != 0;
  const u4_t* qp = static_cast<const u4_t*>(W.tiles);
  const u4_t* scp = reinterpret_cast<const u4_t*>(W.zps);
  const _Float16* dp = static_cast<const _Float16*>(W.scales);
  const h2_t m1056 = splat(-1056.f);

  size_t sbi[4];  // (stripe, superblock 0) index of the wave's stripes, clamped to the last stripe
#pragma unroll
  for (int j = 0; j < 4; j++) sbi[j] = size_t(min(s0 + j, W.ns - 1)) * nsb;
  u4_t lo[4], hi[4], sc[4], lo_n[4];
#pragma unroll
  for (int j = 0; j < 4; j++) lo[j] = qp[sbi[j] * 192 + lane];

  Q6K_GEMM_A_ROWS
  const int nsteps = nsb * 2;
  for (int t = 0; t < nsteps; t++) {
    const int b = t >> 1, half = t & 1;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int r = r0 + p * 32;
      const int row = m0 + r;
      float v[8];
      if (row < Q6K_GEMM_M) {
        load_a8<AT>(a.A, a.lda, Q6K_GEMM_A_ROW(p, row), t * KT + ch * 8, a.K, nullptr, vec_ok, v);
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = 0.f;
      }
      h8_t hv;
#pragma unroll
      for (int j = 0; j < 8; j++) hv[j] = _Float16(v[j]);
      *reinterpret_cast<h8_t*>(lds_a + r * ROWB + (ch ^ (r & 15)) * 16) = hv;
    }
    if (half == 0) {  // the superblock's crumbs and sub-scales
#pragma unroll
      for (int j = 0; j < 4; j++) {
        hi[j] = qp[(sbi[j] + b) * 192 + 128 + lane];
        sc[j] = scp[(sbi[j] + b) * 16 + nl];
      }
    }
    if (t + 1 < nsteps) {
#pragma unroll
      for (int j = 0; j < 4; j++) lo_n[j] = qp[(sbi[j] + ((t + 1) >> 1)) * 192 + ((t + 1) & 1) * 64 + lane];
    }
    __syncthreads();
#pragma unroll
    for (int dd = 0; dd < 4; dd++) {
      // groups g0 = 8 half + 2 dd and g0 + 1 of the superblock: pairs 0, 1 / 2, 3 of the dword
      h8_t bf[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t lw = lo[j][dd];
        const uint32_t hw = (half ? (dd < 2 ? hi[j][2] : hi[j][3]) : (dd < 2 ? hi[j][0] : hi[j][1])) >> (8 * (dd & 1));
        const int g0 = 8 * half + 2 * dd;
        const h2_t s0h = splat(float(q6k_sc(sc[j], g0))), s1h = splat(float(q6k_sc(sc[j], g0 + 1)));
        const h2_t p0 = q6k_pair(lw, q6k_hi_at4<0>(hw), m1056) * s0h;
        const h2_t p1 = q6k_pair(lw >> 4, q6k_hi_at4<1>(hw), m1056) * s0h;
        const h2_t p2 = q6k_pair(lw >> 8, q6k_hi_at4<2>(hw), m1056) * s1h;
        const h2_t p3 = q6k_pair(lw >> 12, q6k_hi_at4<3>(hw), m1056) * s1h;
        bf[j] = h8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
      }
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int r = wm * 32 + i * 16 + nl;
        // k (local) = 32 dd + 4 kq + e and + 16: chunks 4 dd + (kq >> 1) and + 2, byte (kq & 1) * 8 inside
        const char* rp = lds_a + r * ROWB + (kq & 1) * 8;
        const h4_t a0 = *reinterpret_cast<const h4_t*>(rp + ((4 * dd + (kq >> 1)) ^ (r & 15)) * 16);
        const h4_t a1 = *reinterpret_cast<const h4_t*>(rp + ((4 * dd + 2 + (kq >> 1)) ^ (r & 15)) * 16);
        const h8_t af{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
        for (int j = 0; j < 4; j++)
          accsb[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[j], accsb[i][j], 0, 0, 0);
      }
    }
    if (half == 1) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = float(dp[(sbi[j] + b) * 16 + nl]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
          for (int r = 0; r < 4; r++) acc[i][j][r] = __builtin_fmaf(d, accsb[i][j][r], acc[i][j][r]);
          accsb[i][j] = f4_t{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) lo[j] = lo_n[j];
  }

  // C layout: column nl, rows 4 kq + r.  gemm_epilogue4 takes four consecutive columns of a row, so the 16 x 16 tile
  // is turned through LDS (the A tile is free after the last barrier): wave-private 1 KiB per tile
  float* tbuf = reinterpret_cast<float*>(lds_a) + wave * 256;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (s0 + j >= W.ns) continue;
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
      for (int r = 0; r < 4; r++) tbuf[(4 * kq + r) * 16 + nl] = acc[i][j][r];
      __builtin_amdgcn_wave_barrier();
      const int trow = lane >> 2, n0 = (s0 + j) * 16 + 4 * (lane & 3);
      const float4 pv = *reinterpret_cast<const float4*>(tbuf + trow * 16 + 4 * (lane & 3));
      float v[4] = {pv.x, pv.y, pv.z, pv.w};
      const int row = m0 + wm * 32 + i * 16 + trow;
      if (row < Q6K_GEMM_M && n0 < W.n) gemm_epilogue4(a, row, n0, v);
      __builtin_amdgcn_wave_barrier();
    }
  }
