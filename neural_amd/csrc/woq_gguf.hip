// woq_gguf.hip -- GGUF Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 weights, Q8_0 / Q8_1 activations.
//
// A Q4_0 row is K/32 blocks {fp16 d; u8 qs[16]} (neural_speed/core/data_types.h:79-83), value = (nibble - 8) * d with
// element j < 16 in the low nibble of qs[j] and j >= 16 in the high nibble of qs[j - 16] (vectors/cpu/quantize.h:
// 686-704).  That is exactly a symmetric int4, group-32, fp16-scale weight, so nad_gguf_repack_kernel<2> writes it into
// the same MFMA tile layout as a BTLA blob (woq_layout.h) and every forward kernel serves it unchanged.
//
// The reference multiplies a Q4_0 matrix by quantizing the activation rows to Q8_0 (vec_dot_type, ne_layers.c:266-273;
// quantize_row_q8_0_reference, quantize.h:422-445) and summing per block sumi * d_w * d_a (vec_dot.h:187-204).
// nad_q8_quant_kernel<AT, false> is that quantizer (<AT, true>: the Q8_1 rows of Q4_1 / Q5_1); woq_i8.hip's GEMM runs
// the block dot products in its signed-activation mode.
//
// The other four legacy block types (data_types.h:85-118, dequantize_row_*: quantize.h:706-796) land in the same
// layouts through the same kernel template, each described by its row of kGgufTypes (woq_gguf.h): Q8_0 and Q5_0 as
// symmetric int8 (q + 128), Q5_1 as int8 with the true q in 0..31 (q + 128), Q4_1 as symmetric int4.  The symmetric nibble decodes as nibble - 8, and Q4_1's q in 0..15 plus 8 does not fit a nibble: the
// nibble holds q itself, the kernels see q - 8, and w = (q - 8) d + (8 d + m).  (An asymmetric layout with zero point
// -8 would decode q, but the stripe-stream GEMV does not take asymmetric groups of 32.)  The fp16 block minimum of
// Q4_1 / Q5_1 goes into the descriptor's mins region untouched: m / d is no integer, so it cannot ride in a zero point.
// Y = X ((q - bias) d)^T comes from the unchanged forward kernels; the minimum term sum_b S[m][b] (mins[n][b] + bias
// d[n][b]) (S = the block sums of X) is added by woq_min_term_kernel / woq_min_term_tiled_kernel, which also apply
// the caller's epilogue.  8 d is exact in fp32 and m + 8 d is not, so the two products are accumulated separately.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "woq_device.h"
#include "woq_kernels.h"
#include "woq_layout.h"

#pragma clang fp contract(off)

namespace nad {

// ---------------------------------------------------------------------------------------- the 32-element block types
// one thread per (row n, block b) of a GGUF matrix: the 32 stored values into the tile, the fp16 scale (and min) as is.
// TYPE's row of kGgufTypes (woq_gguf.h) gives the block's shape and what a code means
template <int TYPE>
__global__ void nad_gguf_repack_kernel(const uint8_t* __restrict__ src, int n, int k, DeviceWeight w) {
  constexpr GgufType T = *gguf_type_by_id(TYPE);
  constexpr int BB = T.block_bytes;
  constexpr bool HAS_M = T.has_min;
  constexpr int QS = HAS_M ? 4 : 2;                 // offset of qh (5-bit types) or qs
  constexpr int CODE_BITS = (BB - QS) * 8 / 32;     // 4, 5 (16 bytes of nibbles behind the 32 high bits) or 8
  // stored value = code + ADD: the layout decodes stored - (8 | 128), the type code - code_zero (Q4_0: nibble; Q4_1:
  // (q - 8) + 8; Q5_0: (q - 16) + 128; Q5_1: q + 128)
  constexpr uint32_t ADD = (T.bits == 4 ? 8 : 128) - T.min_bias - T.code_zero;
  static_assert(T.block_elems == 32 && (T.bits == 4 || T.bits == 8), "a 32-element type in the int4 / int8 layout");
  const int nb = k / 32;
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= int64_t(n) * nb) return;
  const int row = int(idx / nb), b = int(idx % nb);
  const uint8_t* blk = src + (size_t(row) * nb + b) * BB;
  uint32_t v[32];  // the stored value of element j
  if constexpr (CODE_BITS == 8) {
#pragma unroll
    for (int j = 0; j < 32; j++) v[j] = uint32_t(blk[2 + j]) ^ 0x80u;  // s8 q -> q + 128
  } else {
    uint32_t qh = 0;
    const uint8_t* qs = blk + QS;
    if constexpr (CODE_BITS == 5) {
      qh = uint32_t(qs[0]) | (uint32_t(qs[1]) << 8) | (uint32_t(qs[2]) << 16) | (uint32_t(qs[3]) << 24);
      qs += 4;
    }
#pragma unroll
    for (int j = 0; j < 32; j++) {
      const uint32_t q = (j < 16 ? (qs[j] & 15u) : (qs[j - 16] >> 4)) | (((qh >> j) & 1u) << 4);
      v[j] = q + ADD;
    }
  }
  const int s = row >> 4, nl = row & 15;
  uint32_t* tiles = static_cast<uint32_t*>(w.tiles);
  if constexpr (T.bits == 4) {  // int4 layout: four blocks per tile, one dword per k-quarter
    const int t = b >> 2, d = b & 3;
#pragma unroll
    for (int kq = 0; kq < 4; kq++) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int p = (e & 1) ? 4 + (e >> 1) : (e >> 1);  // woq_layout.h int4 element order
        word |= v[kq * 8 + e] << (4 * p);
      }
      tiles[(tile_index(w.kmajor, w.ns, w.nt, s, t) * 64 + kq * 16 + nl) * 4 + d] = word;
    }
  } else {  // int8 layout: two blocks per tile, a dword pair per k-quarter (byte b of dword w: element 4w + b)
    const int t = b >> 1, d = b & 1;
#pragma unroll
    for (int kq = 0; kq < 4; kq++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int j = kq * 8 + h * 4;
        tiles[(tile_index(w.kmajor, w.ns, w.nt, s, t) * 64 + kq * 16 + nl) * 4 + 2 * d + h] =
            v[j] | (v[j + 1] << 8) | (v[j + 2] << 16) | (v[j + 3] << 24);
      }
  }
  const size_t si = scale_row(w.kmajor, w.ns, w.ng, s, b) * 16 + nl;
  static_cast<uint16_t*>(w.scales)[si] = uint16_t(blk[0]) | (uint16_t(blk[1]) << 8);
  if constexpr (HAS_M) static_cast<uint16_t*>(w.mins)[si] = uint16_t(blk[2]) | (uint16_t(blk[3]) << 8);
}

// ---------------------------------------------------------------------------------------- Q8_0 / Q8_1 activation rows
// per (row, 32-block): amax, d = amax / 127, q = roundf(x * (1 / d)).  Q8_0 (quantize_row_q8_0_reference, quantize.h:
// 422-445) keeps d as fp16 in blocks of 34 bytes; Q8_1 (quantize_row_q8_1_reference, quantize.h:546-579) keeps d fp32
// and adds s = sum(q) * d, blocks of 40 bytes
template <int AT, bool Q81>
__global__ __launch_bounds__(256) void nad_q8_quant_kernel(Q8Args a) {
  const int nb = a.K / 32;
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= int64_t(a.M) * nb) return;
  const int row = int(idx / nb), b = int(idx % nb);
  const size_t rb = size_t(row) * a.lda + size_t(b) * 32;
  float x[32];
  float amax = 0.0f;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    x[j] = a_elem<AT>(a.A, rb + j);
    const float v = fabsf(x[j]);
    amax = amax > v ? amax : v;  // MAX(amax, fabsf(v))
  }
  const float d = amax / 127.f;
  const float id = d != 0.f ? 1.0f / d : 0.0f;
  constexpr int BB = Q81 ? 40 : 34, QS = BB - 32;  // block bytes, offset of the codes
  const __half dh = __float2half_rn(d);
  const float dk = Q81 ? d : __half2float(dh);  // the d the block keeps
  int8_t* out = a.blocks ? a.blocks + (size_t(row) * nb + b) * BB : nullptr;
  if constexpr (!Q81) {
    if (out) {
      const uint16_t bits = __half_as_ushort(dh);
      out[0] = int8_t(bits & 0xff);
      out[1] = int8_t(bits >> 8);
    }
  }
  int sum = 0;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    const int8_t q = int8_t(int(roundf(x[j] * id)));
    sum += q;
    if (a.aq) a.aq[size_t(row) * a.ldq + b * 32 + j] = q;
    if (out) out[QS + j] = q;
  }
  const float sd = Q81 ? float(sum) * d : 0.f;
  if constexpr (Q81) {
    if (out) {
      reinterpret_cast<float*>(out)[0] = d;  // blocks are 40 bytes: 4-byte aligned with the buffer
      reinterpret_cast<float*>(out)[1] = sd;
    }
  }
  if (a.aq && b == nb - 1)
    for (int k = a.K; k < a.kp; k++) a.aq[size_t(row) * a.ldq + k] = 0;
  if (a.sa) a.sa[size_t(row) * nb + b] = make_float2(dk, sd);
}

// ---------------------------------------------------------------------------------------- the minimum term
// the 32 activations of block b of a row, summed in element order
template <int AT>
__device__ __forceinline__ float block_sum(const void* A, int lda, int row, int b, int K, bool vec_ok) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    float v[8];
    load_a8<AT>(A, lda, row, b * 32 + q * 8, K, nullptr, vec_ok, v);
#pragma unroll
    for (int j = 0; j < 8; j++) s += v[j];
  }
  return s;
}

template <int AT>
__global__ __launch_bounds__(256) void woq_block_sum_kernel(const void* A, int lda, int M, int K, int vec_ok, float* S) {
  const int ng = K / 32;
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= int64_t(M) * ng) return;
  S[idx] = block_sum<AT>(A, lda, int(idx / ng), int(idx % ng), K, vec_ok != 0);
}

// out (holding X (q d)^T) -> epi(out + S mins^T), M <= 16.  A workgroup takes four stripes, one per wave.  It first
// builds S [M][K/32] in LDS (from A, or from a.S: the Q8_1 sums of the int8 mode).  A wave then streams its stripe's
// mins with 16-byte loads -- lane l reads columns 8 (l & 1) .. + 7 of block (l >> 1) + 32 i, 1 KiB contiguous per wave
// in the stripe-major order -- and accumulates four rows at a time in fp32; the 32 block slices are summed by a
// butterfly whose order is fixed, so a result never depends on the launch.
template <int AT>
__global__ __launch_bounds__(256) void woq_min_term_kernel(MinTermArgs a) {
  extern __shared__ float s_lds[];
  const int ng = a.ng, M = a.M;
  if (a.mins) {
    for (int i = threadIdx.x; i < M * ng; i += 256) {
      const int row = i / ng, b = i % ng;
      s_lds[i] = a.S ? a.S[size_t(row) * a.s_ld + size_t(b) * a.s_st]
                     : block_sum<AT>(a.A, a.lda, row, b, a.K, a.a_vec != 0);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= a.ns) return;
  const int half = lane & 1, bl = lane >> 1;
  for (int r0 = 0; r0 < M; r0 += 4) {
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 8; c++) acc[r][c] = 0.f;
    // pass 0: the mins; pass 1 (Q4_1): qbias * d
    for (int pass = 0; pass < (a.mins ? (a.qbias != 0.f ? 2 : 1) : 0); pass++) {
      const uint16_t* src = pass ? a.scales : a.mins;
      const float mul = pass ? a.qbias : 1.f;
      for (int b = bl; b < ng; b += 32) {
        const uint4 mv = *reinterpret_cast<const uint4*>(src + scale_row(a.kmajor, a.ns, ng, s, b) * 16 + 8 * half);
        const uint32_t mw[4] = {mv.x, mv.y, mv.z, mv.w};
        float m[8];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          m[2 * c] = f16_bits_to_f32(uint16_t(mw[c] & 0xffffu)) * mul;
          m[2 * c + 1] = f16_bits_to_f32(uint16_t(mw[c] >> 16)) * mul;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float sv = s_lds[min(r0 + r, M - 1) * ng + b];
#pragma unroll
          for (int c = 0; c < 8; c++) acc[r][c] = __builtin_fmaf(sv, m[c], acc[r][c]);
        }
      }
    }
    if (a.mins) {
#pragma unroll
      for (int off = 2; off < 64; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
          for (int c = 0; c < 8; c++) acc[r][c] += __shfl_xor(acc[r][c], off);
    }
    // every lane of a half now holds that half's 4 x 8 sums: lane group bl < 8 finishes row r0 + (bl >> 1), four columns
    if (bl >= 8) continue;
    const int row = r0 + (bl >> 1), q = bl & 1;
    if (row >= M) continue;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (r == (bl >> 1)) v[e] = q ? acc[r][4 + e] : acc[r][e];
    const int n0 = s * 16 + 8 * half + 4 * q;
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (n0 + e < a.g.w.n) v[e] = a.g.w.out[size_t(row) * a.g.w.ldo + n0 + e] + v[e];
    if (n0 < a.g.w.n) gemm_epilogue4(a.g, row, n0, v);
  }
}

// The same for any M, S given: a 64 x 64 output tile per workgroup, 4 x 4 outputs per thread, panels of 32 blocks of S
// (rows padded to 33 floats: the four row groups of a wave read distinct banks) and of the mins (fp32, [block][64
// columns], rows of 80 floats) in LDS; fp32 FMAs in block order.
__global__ __launch_bounds__(256) void woq_min_term_tiled_kernel(MinTermArgs a) {
  __shared__ float sp[64 * 33];
  __shared__ __attribute__((aligned(16))) float mp[32 * 80];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int e = 0; e < 4; e++) acc[i][e] = 0.f;
  for (int pass = 0; pass < (a.mins ? (a.qbias != 0.f ? 2 : 1) : 0); pass++) {  // the mins, then (Q4_1) qbias * d
    const uint16_t* src = pass ? a.scales : a.mins;
    const float mul = pass ? a.qbias : 1.f;
    for (int b0 = 0; b0 < a.ng; b0 += 32) {
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int idx = tid + 256 * i, bb = idx & 31, r = idx >> 5;
        const int row = min(m0 + r, a.M - 1), b = b0 + bb;
        sp[r * 33 + bb] = b < a.ng ? a.S[size_t(row) * a.s_ld + size_t(b) * a.s_st] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int idx = tid + 256 * i, c = idx & 15, bb = (idx >> 4) & 31, sl = idx >> 9;
        const int s = (n0 >> 4) + sl, b = b0 + bb;
        mp[bb * 80 + sl * 16 + c] =
            (s < a.ns && b < a.ng) ? f16_bits_to_f32(src[scale_row(a.kmajor, a.ns, a.ng, s, b) * 16 + c]) * mul : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int bb = 0; bb < 32; bb++) {
        const float4 mv = *reinterpret_cast<const float4*>(&mp[bb * 80 + 4 * tx]);
        const float m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const float sv = sp[(4 * ty + i) * 33 + bb];
#pragma unroll
          for (int e = 0; e < 4; e++) acc[i][e] = __builtin_fmaf(sv, m[e], acc[i][e]);
        }
      }
      __syncthreads();
    }
  }
  const int nn = n0 + 4 * tx;
  if (nn >= a.g.w.n) return;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int row = m0 + 4 * ty + i;
    if (row >= a.M) continue;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; e++)
      v[e] = nn + e < a.g.w.n ? a.g.w.out[size_t(row) * a.g.w.ldo + nn + e] + acc[i][e] : 0.f;
    gemm_epilogue4(a.g, row, nn, v);
  }
}

hipError_t launch_gguf_repack(int type, const uint8_t* src, int n, int k, const DeviceWeight& w, hipStream_t st) {
  const int64_t total = int64_t(n) * (k / 32);
  const dim3 grid(int((total + 255) / 256));
  switch (type) {
#define NAD_REPACK(T) \
  case T: hipLaunchKernelGGL(nad_gguf_repack_kernel<T>, grid, dim3(256), 0, st, src, n, k, w); break
    NAD_REPACK(2);
    NAD_REPACK(3);
    NAD_REPACK(6);
    NAD_REPACK(7);
    NAD_REPACK(8);
#undef NAD_REPACK
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <bool Q81>
static void launch_q8_quant_t(const Q8Args& a, int act_t, dim3 grid, hipStream_t st) {
  if (act_t == kActF32)
    hipLaunchKernelGGL((nad_q8_quant_kernel<kActF32, Q81>), grid, dim3(256), 0, st, a);
  else if (act_t == kActF16)
    hipLaunchKernelGGL((nad_q8_quant_kernel<kActF16, Q81>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((nad_q8_quant_kernel<kActBF16, Q81>), grid, dim3(256), 0, st, a);
}
hipError_t launch_q8_quant(const Q8Args& a, bool q8_1, int act_t, hipStream_t st) {
  const int64_t total = int64_t(a.M) * (a.K / 32);
  const dim3 grid(int((total + 255) / 256));
  if (q8_1)
    launch_q8_quant_t<true>(a, act_t, grid, st);
  else
    launch_q8_quant_t<false>(a, act_t, grid, st);
  return hipGetLastError();
}

static bool rows_vec_ok(const void* A, int lda, int act_t) {
  const size_t es = act_t == kActF32 ? 4 : 2;
  return reinterpret_cast<uintptr_t>(A) % 16 == 0 && (size_t(lda) * es) % 16 == 0;
}

hipError_t launch_block_sums(const void* A, int act_t, int lda, int M, int K, float* S, hipStream_t st) {
  const int64_t total = int64_t(M) * (K / 32);
  const dim3 grid(int((total + 255) / 256));
  const int vec = rows_vec_ok(A, lda, act_t) ? 1 : 0;
  if (act_t == kActF32)
    hipLaunchKernelGGL(woq_block_sum_kernel<kActF32>, grid, dim3(256), 0, st, A, lda, M, K, vec, S);
  else if (act_t == kActF16)
    hipLaunchKernelGGL(woq_block_sum_kernel<kActF16>, grid, dim3(256), 0, st, A, lda, M, K, vec, S);
  else
    hipLaunchKernelGGL(woq_block_sum_kernel<kActBF16>, grid, dim3(256), 0, st, A, lda, M, K, vec, S);
  return hipGetLastError();
}

hipError_t launch_min_term(const MinTermArgs& a0, int act_t, hipStream_t st) {
  MinTermArgs a = a0;
  a.a_vec = (!a.S && a.A && rows_vec_ok(a.A, a.lda, act_t)) ? 1 : 0;
  const size_t lds = a.mins ? size_t(a.M) * a.ng * sizeof(float) : 0;
  if (a.M > kMinTermSmallM || lds > kMinTermSmallLds) return hipErrorInvalidValue;
  const dim3 grid((a.ns + 3) / 4);
  if (act_t == kActF32)
    hipLaunchKernelGGL(woq_min_term_kernel<kActF32>, grid, dim3(256), lds, st, a);
  else if (act_t == kActF16)
    hipLaunchKernelGGL(woq_min_term_kernel<kActF16>, grid, dim3(256), lds, st, a);
  else
    hipLaunchKernelGGL(woq_min_term_kernel<kActBF16>, grid, dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_min_term_tiled(const MinTermArgs& a, hipStream_t st) {
  if (a.mins && !a.S) return hipErrorInvalidValue;
  const dim3 grid((a.g.w.n + 63) / 64, (a.M + 63) / 64);
  hipLaunchKernelGGL(woq_min_term_tiled_kernel, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace nad
