// woq_quant.h -- launch-argument structs and launchers of the device weight quantizer (woq_quant.hip): the sNauto
// quantizer and the blob packer of btla_format.cpp, byte for byte, on a matrix that already sits in HBM.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nad {

// quantize_kblock's integer branch.  w is the torch-layout [n][ldw] matrix (K contiguous) of ActType w_dtype; groups of
// 8 * 2^j <= 512 take 8 elements per lane and 2^j lanes per group, any other group one wave per (column n, group g).
// Writes the signed codes [n][ldq] and, at [g][npad], the scale in the blob's dtype
// (store_scale's RNE conversions; the codes come from the unrounded fp32 scale) and the zero point (asym).  The padding
// of scales / zps (rows >= nblk, columns >= n) is not written: the caller zero-fills them.
struct WoqQuantArgs {
  const void* w;
  int w_dtype;
  int n, k;
  int64_t ldw;
  int bs, nblk;  // group along K (>= k: per channel), ceil(k / bs)
  int bits, asym;
  int scale_t;   // ScaleType
  int npad;
  int8_t* codes;
  int64_t ldq;
  void* scales;
  int8_t* zps;
};
hipError_t launch_woq_quantize(const WoqQuantArgs& a, hipStream_t stream);

// pack_quantized's q section: codes [n][ldq] -> the [npad / ntile][kpad / packrow][ntile][packrow] interleave,
// compressed with the + 2^(bits - 1) bias (raw for 8 bits); padding rows and columns hold code 0.  Writes all q_size bytes.
struct WoqPackArgs {
  const int8_t* codes;
  int64_t ldq;
  int n, k, npad, kpad, ntile, packrow, bits;
  uint8_t* q;
  uint64_t q_size;
};
hipError_t launch_woq_pack(const WoqPackArgs& a, hipStream_t stream);

// pack_quantized's reduce: red[g][n] = bf16(t), t += float(q - z) * s in ascending k, s the stored (rounded) scale; one
// thread per (g, n).  The padding of red is not written.
struct WoqReduceArgs {
  const int8_t* codes;
  int64_t ldq;
  int n, k, bs, nblk, npad, scale_t;
  const void* scales;
  const int8_t* zps;  // null: symmetric
  uint16_t* red;
};
hipError_t launch_woq_reduce(const WoqReduceArgs& a, hipStream_t stream);

}  // namespace nad
