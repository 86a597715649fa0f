// woq_quant.hip -- weights quantized and packed on the device, byte-identical to the host packer (btla_format.cpp
// quantize_kblock's integer branch and pack_quantized): the blob's q / scale / zero-point / reduce sections are produced
// in HBM from a matrix that already sits there, and launch_repack then builds the tile layout from them as it does after
// nad_device_load's upload.
#include "woq_quant.h"

#include <cfloat>
#include <climits>

#include "woq_kernels.h"

// Every value here is defined by separately rounded fp32 operations (the host file is built with -ffp-contract=off):
// x * rscale then roundf, float(q - z) * s then +.  hipcc contracts a * b + c into an fma by default, so contraction is
// switched off for the whole file.  No fast-math; the divides are hipcc's default correctly rounded fp32 divide, and
// the default kernel mode keeps fp32 subnormals.
#pragma clang fp contract(off)

namespace nad {

namespace {

// std::max / std::min argument order, as the host's smax / smin
__device__ inline float smax(float a, float b) { return (a < b) ? b : a; }
__device__ inline float smin(float a, float b) { return (b < a) ? b : a; }
// the x86 cast of the host's f2i: NaN and out-of-range give INT_MIN (the hardware convert gives 0 for NaN and saturates)
__device__ inline int32_t f2i(float x) {
  if (x != x || x >= 2147483648.0f || x < -2147483648.0f) return INT_MIN;
  return int32_t(x);
}
__device__ inline int32_t wrap_add(int32_t a, int32_t b) { return int32_t(uint32_t(a) + uint32_t(b)); }

__device__ inline uint16_t f32_to_bf16_rne(float v) {
  uint32_t u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return uint16_t(u >> 16);
}
__device__ inline uint16_t f32_to_f16_rne(float v) {
  const uint32_t x = __float_as_uint(v);
  const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7FFFFFFFu;
  if (ax > 0x7F800000u) return uint16_t(sign | 0x7E00u | ((ax >> 13) & 0x3FFu));
  if (ax >= 0x477FF000u) return uint16_t(sign | 0x7C00u);
  if (ax < 0x38800000u) {
    if (ax < 0x33000000u) return uint16_t(sign);
    const uint32_t e = ax >> 23, mant = (ax & 0x7FFFFFu) | 0x800000u, sh = 126 - e;
    uint32_t q = mant >> sh;
    const uint32_t rem = mant & ((1u << sh) - 1), half = 1u << (sh - 1);
    if (rem > half || (rem == half && (q & 1u))) q++;
    return uint16_t(sign | q);
  }
  uint32_t q = (((ax >> 23) - 112) << 10) | ((ax & 0x7FFFFFu) >> 13);
  const uint32_t rem = ax & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (q & 1u))) q++;
  return uint16_t(sign | q);
}

__device__ inline void store_scale(void* sp, uint64_t i, int t, float v) {
  if (t == kScaleF32)
    static_cast<float*>(sp)[i] = v;
  else
    static_cast<uint16_t*>(sp)[i] = t == kScaleBF16 ? f32_to_bf16_rne(v) : f32_to_f16_rne(v);
}
__device__ inline float load_scale(const void* sp, uint64_t i, int t) {
  if (t == kScaleF32) return static_cast<const float*>(sp)[i];
  const uint16_t h = static_cast<const uint16_t*>(sp)[i];
  return t == kScaleBF16 ? __uint_as_float(uint32_t(h) << 16) : float(__builtin_bit_cast(_Float16, h));
}

// fp16 / bf16 widen exactly
__device__ inline float load_w(const void* w, int t, uint64_t i) {
  if (t == kActF32) return static_cast<const float*>(w)[i];
  if (t == kActF16) return float(static_cast<const _Float16*>(w)[i]);
  return __uint_as_float(uint32_t(static_cast<const uint16_t*>(w)[i]) << 16);
}

}  // namespace

// One wave per (n, g): the lanes stride over the group's elements, max / min / absmax go through a butterfly (order-free
// for finite inputs; the two signs of zero cannot reach a result: sym adds minval to a maxval >= FLT_MIN, asym starts
// both from + 0 and replaces them on a strict compare only), then every lane derives the same scale and quantizes its
// elements from the matrix again.
template <int ASYM>
__global__ __launch_bounds__(256) void woq_quantize_kernel(WoqQuantArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t items = uint64_t(a.n) * a.nblk;
  const int full = 1 << (a.bits - 1), sym = full - 1;
  for (uint64_t it = blockIdx.x * 4ull + (threadIdx.x >> 6); it < items; it += gridDim.x * 4ull) {
    const int n = int(it / a.nblk), g = int(it % a.nblk);
    const int j = g * a.bs, len = min(a.bs, a.k - j);
    const uint64_t row = uint64_t(n) * a.ldw + j;
    int8_t* qrow = a.codes + uint64_t(n) * a.ldq + j;
    const uint64_t ci = uint64_t(g) * a.npad + n;
    if (!ASYM) {  // sNauto sym
      float maxval = FLT_MIN, minval = FLT_MAX, absmax = 0.f;
      for (int t = lane; t < len; t += 64) {
        const float x = load_w(a.w, a.w_dtype, row + t);
        maxval = smax(maxval, x);
        minval = smin(minval, x);
        absmax = smax(absmax, fabsf(x));
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        maxval = smax(maxval, __shfl_xor(maxval, o, 64));
        minval = smin(minval, __shfl_xor(minval, o, 64));
        absmax = smax(absmax, __shfl_xor(absmax, o, 64));
      }
      float nval = float(sym) + 0.5f;
      const float sum = maxval + minval;
      if (fabsf(sum) >= absmax / float(full)) nval = sum > 0.f ? float(-full) : float(full);
      const float scale = absmax / nval, rscale = 1.f / scale;
      if (lane == 0) store_scale(a.scales, ci, a.scale_t, scale);
      for (int t = lane; t < len; t += 64) {
        float v = roundf(load_w(a.w, a.w_dtype, row + t) * rscale);
        v = smax(smin(v, 127.f), -128.f);
        const int32_t s = int8_t(f2i(v));
        qrow[t] = int8_t(s < -full ? -full : (s > sym ? sym : s));
      }
    } else {  // sNauto asym
      float maxval = 0.f, minval = 0.f;
      for (int t = lane; t < len; t += 64) {
        const float x = load_w(a.w, a.w_dtype, row + t);
        maxval = smax(maxval, x);
        minval = smin(minval, x);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        maxval = smax(maxval, __shfl_xor(maxval, o, 64));
        minval = smin(minval, __shfl_xor(minval, o, 64));
      }
      const float scale = (maxval - minval) / float((1 << a.bits) - 1), rscale = 1.f / scale;
      int32_t z = wrap_add(f2i(roundf((0 - minval) * rscale)), -full);
      z = z < -full ? -full : (z > sym ? sym : z);
      if (lane == 0) {
        store_scale(a.scales, ci, a.scale_t, scale);
        a.zps[ci] = int8_t(z);
      }
      for (int t = lane; t < len; t += 64) {
        const int32_t s = wrap_add(f2i(roundf(load_w(a.w, a.w_dtype, row + t) * rscale)), z);
        qrow[t] = int8_t(s < -full ? -full : (s > sym ? sym : s));
      }
    }
  }
}

// The same arithmetic for groups of 8 * 2^j elements, j = 0 .. 6: 8 consecutive elements per lane (one 16-byte load of
// fp16 / bf16, an 8-byte store of codes), 2^j lanes per group and 64 / 2^j groups per wave, so the butterfly is j steps
// and one pass of the scale arithmetic serves every group of the wave.  Elements past a partial last group (cnt < 8)
// are neither read nor written and take no part in the statistics.
template <int ASYM>
__global__ __launch_bounds__(256) void woq_quantize8_kernel(WoqQuantArgs a, int lpg_shift, int vec_ok) {
  const int lane = threadIdx.x & 63;
  const int lpg = 1 << lpg_shift, gpw = 64 >> lpg_shift;
  const int sub = lane & (lpg - 1);
  const uint64_t items = uint64_t(a.n) * a.nblk;
  const uint64_t tasks = (items + gpw - 1) / gpw;
  const int full = 1 << (a.bits - 1), sym = full - 1;
  for (uint64_t wt = blockIdx.x * 4ull + (threadIdx.x >> 6); wt < tasks; wt += gridDim.x * 4ull) {
    const uint64_t it = wt * gpw + (lane >> lpg_shift);
    const bool live = it < items;
    const uint64_t itc = live ? it : items - 1;
    const int n = int(itc / a.nblk), g = int(itc % a.nblk);
    const int j = g * a.bs + sub * 8;
    const int cnt = live ? max(0, min(8, min(a.k, g * a.bs + a.bs) - j)) : 0;
    const uint64_t base = uint64_t(n) * a.ldw + j;
    float x[8];
    if (vec_ok && cnt == 8) {
      if (a.w_dtype == kActF32) {
        const float4 v0 = *reinterpret_cast<const float4*>(static_cast<const float*>(a.w) + base);
        const float4 v1 = *reinterpret_cast<const float4*>(static_cast<const float*>(a.w) + base + 4);
        x[0] = v0.x, x[1] = v0.y, x[2] = v0.z, x[3] = v0.w, x[4] = v1.x, x[5] = v1.y, x[6] = v1.z, x[7] = v1.w;
      } else {
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.w) + base);
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const uint16_t h = uint16_t(u[e >> 1] >> (16 * (e & 1)));
          x[e] = a.w_dtype == kActF16 ? float(__builtin_bit_cast(_Float16, h)) : __uint_as_float(uint32_t(h) << 16);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) x[e] = e < cnt ? load_w(a.w, a.w_dtype, base + e) : 0.f;
    }
    const uint64_t ci = uint64_t(g) * a.npad + n;
    int32_t q[8];
    if (!ASYM) {
      float maxval = FLT_MIN, minval = FLT_MAX, absmax = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (e < cnt) {
          maxval = smax(maxval, x[e]);
          minval = smin(minval, x[e]);
          absmax = smax(absmax, fabsf(x[e]));
        }
      for (int o = lpg >> 1; o > 0; o >>= 1) {
        maxval = smax(maxval, __shfl_xor(maxval, o, 64));
        minval = smin(minval, __shfl_xor(minval, o, 64));
        absmax = smax(absmax, __shfl_xor(absmax, o, 64));
      }
      float nval = float(sym) + 0.5f;
      const float sum = maxval + minval;
      if (fabsf(sum) >= absmax / float(full)) nval = sum > 0.f ? float(-full) : float(full);
      const float scale = absmax / nval, rscale = 1.f / scale;
      if (live && sub == 0) store_scale(a.scales, ci, a.scale_t, scale);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float v = roundf(x[e] * rscale);
        v = smax(smin(v, 127.f), -128.f);
        const int32_t s = int8_t(f2i(v));
        q[e] = s < -full ? -full : (s > sym ? sym : s);
      }
    } else {
      float maxval = 0.f, minval = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (e < cnt) {
          maxval = smax(maxval, x[e]);
          minval = smin(minval, x[e]);
        }
      for (int o = lpg >> 1; o > 0; o >>= 1) {
        maxval = smax(maxval, __shfl_xor(maxval, o, 64));
        minval = smin(minval, __shfl_xor(minval, o, 64));
      }
      const float scale = (maxval - minval) / float((1 << a.bits) - 1), rscale = 1.f / scale;
      int32_t z = wrap_add(f2i(roundf((0 - minval) * rscale)), -full);
      z = z < -full ? -full : (z > sym ? sym : z);
      if (live && sub == 0) {
        store_scale(a.scales, ci, a.scale_t, scale);
        a.zps[ci] = int8_t(z);
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int32_t s = wrap_add(f2i(roundf(x[e] * rscale)), z);
        q[e] = s < -full ? -full : (s > sym ? sym : s);
      }
    }
    int8_t* qrow = a.codes + uint64_t(n) * a.ldq + j;  // ldq is a multiple of 16, j of 8
    if (cnt == 8) {
      uint2 o;
      o.x = (q[0] & 0xff) | ((q[1] & 0xff) << 8) | ((q[2] & 0xff) << 16) | (uint32_t(q[3] & 0xff) << 24);
      o.y = (q[4] & 0xff) | ((q[5] & 0xff) << 8) | ((q[6] & 0xff) << 16) | (uint32_t(q[7] & 0xff) << 24);
      *reinterpret_cast<uint2*>(qrow) = o;
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (e < cnt) qrow[e] = int8_t(q[e]);
    }
  }
}

// One thread per dword of the q section: byte B holds the elements B * (8 / bits) + t of the flat interleaved order;
// element e lies in stripe e / (ntile * kpad) at [k / packrow][ntile][packrow].  A dword's elements are consecutive and
// the position is divided out once and then stepped.
__global__ __launch_bounds__(256) void woq_pack_kernel(WoqPackArgs a, int pr_shift) {
  const uint64_t ndw = (a.q_size + 3) / 4;
  const int per = 8 / a.bits, nel = 4 * per;  // elements per byte / per dword: 4, 8 or 16
  const uint32_t mask = (1u << a.bits) - 1;
  const int bias = a.bits == 8 ? 0 : 1 << (a.bits - 1);
  const uint64_t stripe = uint64_t(a.ntile) * a.kpad, total = uint64_t(a.npad) * a.kpad;
  const uint32_t tp = uint32_t(a.ntile) << pr_shift;
  for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < ndw; d += gridDim.x * 256ull) {
    const uint64_t e0 = d * nel;
    const int st = int(e0 / stripe);
    const uint32_t el = uint32_t(e0 - uint64_t(st) * stripe);
    uint32_t kb = el / tp, r = el - kb * tp;  // r: position in [ntile][packrow]
    int n0 = st * a.ntile;
    uint32_t word = 0;
    for (int i = 0; i < nel; i++) {
      if (e0 + i < total) {
        const int kk = int(kb << pr_shift) + int(r & ((1u << pr_shift) - 1));
        const int nn = n0 + int(r >> pr_shift);
        const int v = (kk < a.k && nn < a.n) ? int(a.codes[uint64_t(nn) * a.ldq + kk]) : 0;
        word |= (uint32_t(v + bias) & mask) << (a.bits * i);
      }
      if (++r == tp) {
        r = 0;
        if (int(++kb << pr_shift) >= a.kpad) {  // the next stripe (an odd kpad puts the boundary inside a dword)
          kb = 0;
          n0 += a.ntile;
        }
      }
    }
    if (d * 4 + 4 <= a.q_size) {
      reinterpret_cast<uint32_t*>(a.q)[d] = word;
    } else {
      for (uint64_t byte = d * 4; byte < a.q_size; byte++) a.q[byte] = uint8_t(word >> (8 * (byte - d * 4)));
    }
  }
}

// One thread per (g, n), n fastest: the sequential fp32 sum of the host's reduceWeight
__global__ __launch_bounds__(256) void woq_reduce_kernel(WoqReduceArgs a) {
  const uint64_t items = uint64_t(a.nblk) * a.n;
  for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < items; i += gridDim.x * 256ull) {
    const int g = int(i / a.n), n = int(i % a.n);
    const uint64_t ci = uint64_t(g) * a.npad + n;
    const float s = load_scale(a.scales, ci, a.scale_t);
    const int z = a.zps ? int(a.zps[ci]) : 0;
    const int k0 = g * a.bs, k1 = min(a.k, k0 + a.bs);
    const int8_t* q = a.codes + uint64_t(n) * a.ldq;
    float t = 0.f;
    int kk = k0;
    if (((k0 | int(a.ldq)) & 15) == 0)  // the codes buffer is 256-byte aligned: 16 codes per load
      for (; kk + 16 <= k1; kk += 16) {
        const uint4 v4 = *reinterpret_cast<const uint4*>(q + kk);
        const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int b = 0; b < 16; b++) t += float(int(int8_t(v[b >> 2] >> (8 * (b & 3)))) - z) * s;
      }
    for (; kk < k1; kk++) t += float(int(q[kk]) - z) * s;
    // finite inputs can still overflow a stored scale to inf (fp16 scales of large weights, asym max - min): 0 * inf
    // and inf - inf then make the sum NaN.  No operand is ever NaN, so on the host it is always the x86 default NaN
    // (sign set); the GPU's default NaN has the sign clear
    if (t != t) t = __uint_as_float(0xFFC00000u);
    a.red[ci] = f32_to_bf16_rne(t);
  }
}

static int grid_for(uint64_t work_items, uint64_t per_block) {
  const uint64_t g = (work_items + per_block - 1) / per_block;
  return int(g < 1 ? 1 : (g > (1u << 20) ? (1u << 20) : g));
}

hipError_t launch_woq_quantize(const WoqQuantArgs& a, hipStream_t stream) {
  const uint64_t items = uint64_t(a.n) * a.nblk;
  if (a.bs >= 8 && a.bs <= 512 && (a.bs & (a.bs - 1)) == 0) {  // 8 * 2^j: woq_quantize8_kernel
    int sh = 0;
    while ((8 << sh) < a.bs) sh++;
    const int esz = a.w_dtype == kActF32 ? 4 : 2;
    const int vec_ok = (reinterpret_cast<uintptr_t>(a.w) % 16 == 0 && (uint64_t(a.ldw) * esz) % 16 == 0) ? 1 : 0;
    const int grid = grid_for((items + (64 >> sh) - 1) / (64 >> sh), 4);
    if (a.asym)
      hipLaunchKernelGGL(woq_quantize8_kernel<1>, dim3(grid), dim3(256), 0, stream, a, sh, vec_ok);
    else
      hipLaunchKernelGGL(woq_quantize8_kernel<0>, dim3(grid), dim3(256), 0, stream, a, sh, vec_ok);
    return hipGetLastError();
  }
  const int grid = grid_for(items, 4);
  if (a.asym)
    hipLaunchKernelGGL(woq_quantize_kernel<1>, dim3(grid), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(woq_quantize_kernel<0>, dim3(grid), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_woq_pack(const WoqPackArgs& a, hipStream_t stream) {
  const int pr_shift = a.packrow == 4 ? 2 : (a.packrow == 2 ? 1 : 0);
  hipLaunchKernelGGL(woq_pack_kernel, dim3(grid_for((a.q_size + 3) / 4, 256)), dim3(256), 0, stream, a, pr_shift);
  return hipGetLastError();
}

hipError_t launch_woq_reduce(const WoqReduceArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(woq_reduce_kernel, dim3(grid_for(uint64_t(a.nblk) * a.n, 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace nad
