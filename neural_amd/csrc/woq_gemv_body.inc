// woq_gemv_body.inc -- the body of the stripe-stream GEMV (woq_gemv.h: steps 1-4 of woq_gemv_kernel), included once
// by each kernel that runs it, inside the kernel function, with
//   GEMV_WG_INDEX, GEMV_WG_COUNT   this workgroup's index among the workgroups that share the launch's units, and how
//                                  many they are (woq_gemv_kernel: blockIdx.x, gridDim.x; woq_gemv_routed_kernel: b % wpp,
//                                  wpp)
// defined, and `a` (GemvArgs) and the template parameters BITS, HILO, GPT, ASYM, NST in scope.
// Text and not a __device__ __forceinline__ function: hipcc simplifies a function on its own before it inlines it, and
// every form of a lifted function that was tried (const reference, reference or value arguments; the index and count as
// values or read through a policy object; lane, wave, wave count and blockDim.x read by the kernel and passed in) left
// woq_gemv_kernel with other code than it had -- blockDim.x no longer folded to the one load of a uniform-work-group
// launch, 64-bit index arithmetic narrowed elsewhere, another register allocation.  Included as text the kernel sees
// the tokens it always did and its 96 instantiations compile to the bytes they had.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KT = k_tile(BITS);
  static_assert(KT / 32 % GPT == 0, "groups must tile the K tile");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int NW = __builtin_amdgcn_readfirstlane(int(blockDim.x >> 6));
  const int M = a.M, nt = a.nt, Kp = nt * KT;
  const int R = HILO == 0 ? M : 2 * M;
  const int nsl = (nt + KS - 1) / KS;  // K-slices per stripe
  NAD_TRACE(0);

  // this workgroup's units (wave-uniform)
  const int G = GEMV_WG_COUNT, bid = GEMV_WG_INDEX;
  const int u0 = int(unsigned(bid) * unsigned(a.units) / unsigned(G));
  const int u1 = int(unsigned(bid + 1) * unsigned(a.units) / unsigned(G));
  const int vpu = a.dual ? 2 : 1;
  const int v0 = u0 * vpu, nv = (u1 - u0) * vpu;
  const bool idle = wave >= nsl;  // more waves than K-slices: this wave only joins the barriers
  float* part = reinterpret_cast<float*>(smem + a.part_off);  // [nv][NW][M][16]
  const int bd = blockDim.x;

  // 1) activation loads, then the first three weight stages, back to back
  const int a_units = M * (Kp >> 3);
  constexpr int AR = 2;  // activation units per thread issued ahead of the weights
  const int esz = a.act_t == kActF32 ? 4 : 2;
  const auto ra = rsrc(a.A, (M - 1) * a.lda * esz + a.K * esz);
  uint4 x[AR][2];
  if (a.a_fast) {
#pragma unroll
    for (int q = 0; q < AR; q++) {
      const int u = q * bd + int(threadIdx.x);
      const int row = u / (Kp >> 3), k = (u - row * (Kp >> 3)) * 8;
      const int off = (u < a_units && k < a.K) ? (row * a.lda + k) * esz : kOOB;
      x[q][0] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
      x[q][1] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
    }
  }
  const int vs = a.scale_t == kScaleF32 ? (lane & 15) * 4 : (lane & 14) * 2;
  StageCursor lc;
  lc.j = idle ? nv : 0;
  lc.q = wave;
  lc.s = 0;
  lc.rt = rsrc(a.w[0].tiles, 0);  // zero records: every access out of range (idle waves, past-the-end stages)
  lc.rs = lc.rt;
  lc.rz = lc.rt;
  if (!idle && nv > 0) cursor_stripe(a, lc, v0);
  StageRegs<GPT> S[NST];
  // Only the first stage goes out before the activations are published: issuing all three first stalled the wave on
  // memory back-pressure and delayed the (already landed) activation staging by ~1-2 us (phase trace; the pre-issue
  // A/B of round 4, profiles/r04_gemv_preissue_ab.txt).
  load_stage<GPT, ASYM>(a, S[0], lc, nv, nsl, wave, NW, v0, lane, vs);
  NAD_TRACE(4);

  // 2) publish the activations (waits only for the loads issued before the weights)
  if (a.a_fast) {
#pragma unroll
    for (int q = 0; q < AR; q++) {
      const int u = q * bd + int(threadIdx.x);
      if (u < a_units) {
        const int row = u / (Kp >> 3), k = (u - row * (Kp >> 3)) * 8;
        float f[8];
        unit_to_f32(a.act_t, x[q][0], x[q][1], f);
        unit_store<HILO>(smem, f, row, k, M, Kp);
      }
    }
    for (int u = AR * bd + int(threadIdx.x); u < a_units; u += bd) {  // large M * K only
      const int row = u / (Kp >> 3), k = (u - row * (Kp >> 3)) * 8;
      const int off = k < a.K ? (row * a.lda + k) * esz : kOOB;
      const uint4 y0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off, 0, 0));
      const uint4 y1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(ra, off + 16, 0, 0));
      float f[8];
      unit_to_f32(a.act_t, y0, y1, f);
      unit_store<HILO>(smem, f, row, k, M, Kp);
    }
  } else {
    stage_a_slow<HILO>(a, smem, a_units, Kp);
  }
  {
    uint4* zr = reinterpret_cast<uint4*>(smem + size_t(R) * Kp * 2);
    for (int i = threadIdx.x; i < (Kp >> 3); i += bd) zr[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
#pragma unroll
  for (int i = 1; i < NST; i++) load_stage<GPT, ASYM>(a, S[i], lc, nv, nsl, wave, NW, v0, lane, vs);
  NAD_TRACE(1);

  // 3) the stream
  const int m = lane & 15;   // MFMA A row fed by this lane (and C column n)
  const int kq = lane >> 4;  // k-quarter of a 32-k step
  const int arow = HILO == 1 ? (m & 7) : m;
  const bool is_lo = HILO == 1 && m >= 8;
  const int row_hi = arow < M ? (is_lo ? M + arow : arow) : R;  // inactive rows read the zero row
  const int row_lo = arow < M ? M + arow : R;
  const char* a_hi = smem + size_t(row_hi) * Kp * 2 + kq * 16;
  const char* a_lo = smem + size_t(row_lo) * Kp * 2 + kq * 16;
  const int ssh = a.scale_t == kScaleF32 ? 0 : (lane & 1) * 16;  // this lane's half of a 16-bit scale pair
  const Dq4 dq = dq4_consts<BITS>(a.dq_mask, a.dq_magic);

  f4_t acc = {0.f, 0.f, 0.f, 0.f};
  int cj = idle ? nv : 0, cq = wave;  // compute cursor (wave-uniform)

  auto compute_stage = [&](const StageRegs<GPT>& S) {
    if (cj >= nv) return;
    const int t0 = cq * KS;
    // tiles past the end of K carry out-of-range (zero) weights and a zero scale, and read a valid activation row (no
    // NaN from LDS)
    stage_mac<BITS, GPT, ASYM, KS, -1, HILO == 2>(
        S, dq, a_hi + t0 * KT * 2, a_lo + t0 * KT * 2, [&](int i) { return (min(t0 + i, nt - 1) - t0) * KT * 2; },
        a.scale_t, ssh, acc);
    cq += NW;
    if (cq >= nsl) {  // this wave's last slice of stripe cj: publish its partial
      f4_t r = acc;
      if constexpr (HILO == 1) {
#pragma unroll
        for (int xx = 0; xx < 4; xx++) r[xx] += __shfl_down(r[xx], 32, 64);
      }
      float* ps = part + (size_t(cj) * NW + wave) * M * 16 + m;
#pragma unroll
      for (int xx = 0; xx < 4; xx++) {
        const int row = (lane >> 4) * 4 + xx;
        if (row < M && (HILO != 1 || lane < 32)) ps[row * 16] = r[xx];
      }
      acc = f4_t{0.f, 0.f, 0.f, 0.f};
      cq = wave;
      cj++;
    }
  };

  while (cj < nv) {
#pragma unroll
    for (int i = 0; i < NST; i++) {
      compute_stage(S[i]);
      load_stage<GPT, ASYM>(a, S[i], lc, nv, nsl, wave, NW, v0, lane, vs);
    }
  }
  NAD_TRACE_MAX(2);
  __syncthreads();

  // 4) sum each stripe's wave slots in wave order and apply the epilogue
  const int nout = (u1 - u0) * M * 16;
  const int nwl = min(NW, nsl);  // waves that own slices
  for (int o = threadIdx.x; o < nout; o += bd) {
    const int p = o / (M * 16), mm = (o >> 4) % M, nn = o & 15;
    float y[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (h < vpu) {
        // reduce_slots' order as a loop over the live slots (slots M * 16 floats apart).  Kept as this kernel's own
        // copy: reading 16 clamped slots per output, as reduce_slots does, measured 1-2.5 % slower here, where a
        // thread reduces M outputs per stripe (N = 11008 M = 8 fp16: 12.1 -> 12.4 us; DESIGN.md section 4).
        const float* ps = part + (size_t(p * vpu + h) * NW * M + mm) * 16 + nn;
        const size_t wst = size_t(M) * 16;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int w = 0;
        for (; w + 3 < nwl; w += 4) {
          s0 += ps[size_t(w) * wst];
          s1 += ps[size_t(w + 1) * wst];
          s2 += ps[size_t(w + 2) * wst];
          s3 += ps[size_t(w + 3) * wst];
        }
        for (; w < nwl; w++) s0 += ps[size_t(w) * wst];
        y[h] = (s0 + s1) + (s2 + s3);
      }
    }
    int wsel, s;
    vstripe(a, v0 + p * vpu, wsel, s);
    if (a.dual) wsel = 0;
    const int n = s * 16 + nn;
    const int nmax = sel3(wsel, a.w[0].n, a.w[1].n, a.w[2].n);
    if (n >= nmax) continue;
    float* out = sel3(wsel, a.w[0].out, a.w[1].out, a.w[2].out);
    const int ldo = sel3(wsel, a.w[0].ldo, a.w[1].ldo, a.w[2].ldo);
    float v = y[0];
    switch (a.epi) {
      case kEpiBias:
        v += a.w[0].bias[size_t(mm) * a.w[0].bias_ld + n];
        break;
      case kEpiAddGelu:
        v = gelu_f(v + a.w[0].bias[size_t(mm) * a.w[0].bias_ld + n]);
        break;
      case kEpiGelu:
        v = gelu_f(v);
        break;
      case kEpiSilu:
        v = silu_f(v);
        break;
      case kEpiResAdd:
        v += a.res[size_t(mm) * a.ld_res + n];
        break;
      case kEpiSiluMul: {
        const float t1 = silu_f(y[0]);
        if (a.aux) a.aux[size_t(mm) * a.ld_aux + n] = t1;
        v = t1 * y[1];
        break;
      }
      case kEpiGeluMul: {
        const float t1 = gelu_f(y[0]);
        if (a.aux) a.aux[size_t(mm) * a.ld_aux + n] = t1;
        v = t1 * y[1];
        break;
      }
      default:
        break;
    }
    out[size_t(mm) * ldo + n] = v;
  }
  NAD_TRACE(3);
