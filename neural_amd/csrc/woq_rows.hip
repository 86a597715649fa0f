// woq_rows.hip -- ne_get_rows on a device weight (ne_compute_forward_get_rows_q, core/ne_layers.c:8385-8433): the
// requested rows of the [N][K] matrix a weight was quantized from, dequantized straight out of the tile layouts of
// woq_layout.h.  The values are those of the unpack kernels (nad_unrepack_kernel, nad_q6k_unpack_kernel), operation for
// operation and with no contraction, so an fp32 row has the bits of that column of nad_device_unpack_fp32.
//
// Work: a unit is (requested row r, run of 16 K tiles); a wave takes one unit, a workgroup four.  The wave reads ids[r]
// with a wave-uniform load, clamps it -- an id outside [0, n) becomes row 0 for every address and the lanes write
// +0.0 without reading the weight -- and forms stripe s = id >> 4, column c = id & 15.  Lane L takes tile
// t0 + (L >> 2) and k-quarter kq = L & 3: its one 16-byte load is lane slot kq * 16 + c of the tile, which holds, for
// every 32-k step d of the tile, the 8 consecutive k = t KT + 32 d + 8 kq + j of column c.  The four lanes of a tile
// therefore write 128 contiguous bytes of fp32 per step, each with 16-byte stores.  The group's scale, zero point and
// min are loaded when the lane's step enters a new group, never per element; the divisions are one 32-bit one per wave
// (unit -> row, run) and one per lane (the group of the tile's first step).
// K that is not a whole number of tiles ends in a step that is skipped (k0 >= k) or, for a K that is no multiple of 8,
// stored element by element below k.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "woq_device.h"
#include "woq_kernels.h"
#include "woq_layout.h"
#include "woq_rows.h"

#pragma clang fp contract(off)

namespace nad {

// fp32 -> the 16 bits of the output type, round to nearest even (NaN: the quiet NaN torch writes)
template <int OT>
__device__ __forceinline__ uint32_t rows_cvt16(float x) {
  if constexpr (OT == kActF16) return __builtin_bit_cast(uint16_t, _Float16(x));
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// N (8 or 4) consecutive values to row[k0 .. k0 + N - 1], clipped at k.  k0 is a multiple of N and the row base is
// 16-byte aligned, so a whole run is one or two 16-byte stores (fp32), one 16-byte store (8 halves) or one 8-byte store
// (4 halves, Q6_K)
template <int OT, int N>
__device__ __forceinline__ void rows_store(void* row, int k0, int k, const float (&v)[N]) {
  if constexpr (OT == kActF32) {
    float* o = static_cast<float*>(row) + k0;
    if (k0 + N <= k) {
#pragma unroll
      for (int i = 0; i < N; i += 4) *reinterpret_cast<f4_t*>(o + i) = f4_t{v[i], v[i + 1], v[i + 2], v[i + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < N; j++)
        if (k0 + j < k) o[j] = v[j];
    }
  } else {
    uint16_t* o = static_cast<uint16_t*>(row) + k0;
    if (k0 + N <= k) {
      uint32_t p[N / 2];
#pragma unroll
      for (int i = 0; i < N / 2; i++) p[i] = rows_cvt16<OT>(v[2 * i]) | (rows_cvt16<OT>(v[2 * i + 1]) << 16);
      if constexpr (N == 8)
        *reinterpret_cast<u4_t*>(o) = u4_t{p[0], p[1], p[2], p[3]};
      else
        *reinterpret_cast<uint2*>(o) = make_uint2(p[0], p[1]);
    } else {
#pragma unroll
      for (int j = 0; j < N; j++)
        if (k0 + j < k) o[j] = uint16_t(rows_cvt16<OT>(v[j]));
    }
  }
}

// the unit of this wave: false past the last one.  r: the output row, run: its run of tiles, valid: the id is a row
// of the weight, id: the clamped row
struct RowsUnit {
  int r, run, id;
  bool valid;
};
__device__ __forceinline__ bool rows_unit(const GetRowsArgs& a, RowsUnit& u) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: the id load is scalar
  const uint32_t unit = blockIdx.x * uint32_t(kRowsWaves) + uint32_t(wave);  // units < 2^32 (get_rows_geometry)
  if (unit >= uint32_t(a.m) * uint32_t(a.runs)) return false;
  u.r = int(unit / uint32_t(a.runs));
  u.run = int(unit - uint32_t(u.r) * uint32_t(a.runs));
  const int id = a.ids[int64_t(u.r) * a.ids_stride];
  u.valid = uint32_t(id) < uint32_t(a.w.n);
  u.id = u.valid ? id : 0;  // clamped before any address is formed
  return true;
}

// KIND: 0 integer codes, 1 the F4 LUTs (int4 layout), 2 raw F8 codes (int8 layout)
template <int BITS, int KIND, int OT>
__global__ __launch_bounds__(kRowsWaves * 64) void woq_get_rows_kernel(GetRowsArgs a) {
  constexpr int KT = BITS == 4 ? 128 : (BITS == 2 ? 256 : 64), SPT = KT / 32;
  constexpr int BIAS = BITS == 4 ? 8 : (BITS == 2 ? 2 : 128);
  constexpr int ESZ = OT == kActF32 ? 4 : 2;
  const DeviceWeight& w = a.w;
  RowsUnit u;
  if (!rows_unit(a, u)) return;
  const int lane = threadIdx.x & 63;
  const int s = u.id >> 4, c = u.id & 15;
  const int t = u.run * kRowsTilesPerUnit + (lane >> 2), kq = lane & 3;
  if (t >= w.nt) return;
  char* row = static_cast<char*>(a.out) + size_t(u.r) * size_t(a.ldo) * ESZ;
  const int kb = t * KT + 8 * kq;
  const bool has_min = w.mins != nullptr;
  const float min_bias = float(w.min_bias);

  u4_t piece{0u, 0u, 0u, 0u};
  if (u.valid)
    piece = static_cast<const u4_t*>(w.tiles)[tile_index(w.kmajor, w.ns, w.nt, s, t) * 64 + uint64_t(kq * 16 + c)];
  // the group of the tile's first step; the steps after it count up
  int g = (t * SPT) / a.bs32, rem = t * SPT - g * a.bs32;
  bool fetch = true;
  float sc = 0.f, mn = 0.f;
  int zp = 0;
#pragma unroll
  for (int d = 0; d < SPT; d++) {
    const int k0 = kb + 32 * d;
    if (k0 < w.k) {
      float v[8];
      if (u.valid) {
        if (fetch) {
          const uint64_t si = scale_row(w.kmajor, w.ns, w.ng, s, g) * 16 + uint64_t(c);
          sc = load_scale(w.scales, si, w.scale_t);
          if (KIND == 0 && w.zps) zp = int(w.zps[si]);
          if (has_min) mn = float(static_cast<const _Float16*>(w.mins)[si]);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
          uint32_t code;
          if constexpr (BITS == 4)
            code = (piece[d] >> (4 * ((j >> 1) + 4 * (j & 1)))) & 0xFu;
          else if constexpr (BITS == 2)
            code = (piece[d >> 1] >> (2 * ((j >> 1) + 4 * (d & 1) + 8 * (j & 1)))) & 0x3u;
          else
            code = (piece[2 * d + (j >> 2)] >> (8 * (j & 3))) & 0xFFu;
          float q;
          if constexpr (KIND == 2) {  // f8_to_fp32's bit construction (kernel_ref.h:984-1001)
            const int eb = w.f4kind == 3 ? 4 : 5, mb = 7 - eb;
            const uint32_t e = ((code & 0x7f) >> mb) - (1u << (eb - 1)) + 128;
            q = __uint_as_float(((code & 0x80) << 24) | (e << 23) | ((code << (23 - mb)) & 0x7fffffu));
          } else if constexpr (KIND == 1) {
            q = kF4LutF[w.f4kind][code & 15];
          } else {
            q = float(int(code) - BIAS - zp);
          }
          if (has_min) q = q + min_bias;  // Q4_1 / Q5_1: the true q, q d exact, + m rounded once
          float x = q * sc;
          if (has_min) x = x + mn;
          v[j] = x;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = 0.f;
      }
      rows_store<OT, 8>(row, k0, w.k, v);
    }
    fetch = false;
    if (++rem == a.bs32) {
      rem = 0;
      g++;
      fetch = true;
    }
  }
}

// GGUF Q6_K: a unit is (row, run of 4 superblocks); 16 lanes share a superblock.  Lane L takes superblock
// b0 + (L >> 4), k-quarter kq = L & 3 and the groups g = 4 i + gq, gq = (L >> 2) & 3, i = 0..3: the 16 bytes of lane
// slot kq * 16 + c in each of the three pieces, the column's 16 sub-scales (one 16-byte load) and d -- the four gq
// lanes of a slot ask for the same bytes, one request each.  Group g of the lane is the four
// k = 256 b + 16 g + 4 kq + j, so in step i the 16 lanes of a superblock write 256 contiguous bytes of fp32;
// (d * sc) * q as nad_q6k_unpack_kernel has it.
template <int OT>
__global__ __launch_bounds__(kRowsWaves * 64) void woq_get_rows_q6k_kernel(GetRowsArgs a) {
  constexpr int ESZ = OT == kActF32 ? 4 : 2;
  const DeviceWeight& w = a.w;
  RowsUnit u;
  if (!rows_unit(a, u)) return;
  const int lane = threadIdx.x & 63;
  const int s = u.id >> 4, c = u.id & 15;
  const int b = u.run * kRowsQ6kPerUnit + (lane >> 4), kq = lane & 3, gq = (lane >> 2) & 3;
  if (b >= w.nt) return;
  char* row = static_cast<char*>(a.out) + size_t(u.r) * size_t(a.ldo) * ESZ;
  const size_t sb = size_t(s) * w.nt + b;
  u4_t lo0{0u, 0u, 0u, 0u}, lo1 = lo0, hi = lo0, scv = lo0;
  float d = 0.f;
  if (u.valid) {
    const u4_t* tl = static_cast<const u4_t*>(w.tiles) + sb * 192 + size_t(kq * 16 + c);
    lo0 = tl[0];
    lo1 = tl[64];
    hi = tl[128];
    scv = reinterpret_cast<const u4_t*>(w.zps)[sb * 16 + c];
    d = float(static_cast<const _Float16*>(w.scales)[sb * 16 + c]);
  }
  const bool odd_dword = (gq >> 1) != 0;
  const int nsh = 8 * (gq & 1), csh = 4 * gq;  // 4 pl = nsh + ..., 2 ph = csh + ... below
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // group g = 4 i + gq: nibbles in dword (g & 7) >> 1 = 2 (i & 1) + (gq >> 1) of piece g >> 3 = i >> 1, crumbs in
    // dword g >> 2 = i of piece 2, sub-scale byte gq of dword i
    float v[4];
    if (u.valid) {
      const float ds = d * float(int(__builtin_amdgcn_sbfe(int(scv[i]), 8 * gq, 8)));  // the builtin's type is unsigned
      const u4_t& lo = i < 2 ? lo0 : lo1;
      const uint32_t lw = odd_dword ? lo[2 * (i & 1) + 1] : lo[2 * (i & 1)], hw = hi[i];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        // nibble position pl = 2 (g & 1) + (j >> 1) + 4 (j & 1), crumb position ph = 2 (g & 3) + (j >> 1) + 8 (j & 1)
        const uint32_t nib = (lw >> (nsh + 4 * (j >> 1) + 16 * (j & 1))) & 15u;
        const uint32_t crumb = (hw >> (csh + 2 * (j >> 1) + 16 * (j & 1))) & 3u;
        const int q = int(nib | (crumb << 4)) - 32;
        v[j] = ds * float(q);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = 0.f;
    }
    rows_store<OT, 4>(row, 256 * b + 16 * (4 * i + gq) + 4 * kq, w.k, v);
  }
}

bool get_rows_geometry(const DeviceWeight& w, int m, int* runs, int* grid) {
  const int per = w.bits == 6 ? kRowsQ6kPerUnit : kRowsTilesPerUnit;
  *runs = (w.nt + per - 1) / per;
  const int64_t blocks = (int64_t(m) * *runs + kRowsWaves - 1) / kRowsWaves;
  if (m < 0 || *runs < 1 || blocks >= (int64_t(1) << 30)) return false;  // the kernels count units in 32 bits
  *grid = int(blocks);
  return true;
}

template <int BITS, int KIND>
static hipError_t launch_rows_t(const GetRowsArgs& a, int grid, hipStream_t st) {
  const dim3 g(grid), b(kRowsWaves * 64);
  if (a.out_t == kActF32)
    hipLaunchKernelGGL((woq_get_rows_kernel<BITS, KIND, kActF32>), g, b, 0, st, a);
  else if (a.out_t == kActF16)
    hipLaunchKernelGGL((woq_get_rows_kernel<BITS, KIND, kActF16>), g, b, 0, st, a);
  else
    hipLaunchKernelGGL((woq_get_rows_kernel<BITS, KIND, kActBF16>), g, b, 0, st, a);
  return hipGetLastError();
}

hipError_t launch_get_rows(const GetRowsArgs& a, int grid, hipStream_t st) {
  const DeviceWeight& w = a.w;
  const int esz = a.out_t == kActF32 ? 4 : 2;
  if (grid < 1 || a.m < 1 || a.runs < 1 || a.bs32 < 1 || !a.ids || !a.out || !w.tiles || !w.scales || a.ldo < w.k ||
      reinterpret_cast<uintptr_t>(a.out) % 16 != 0 || (uint64_t(a.ldo) * esz) % 16 != 0 ||
      (a.out_t != kActF32 && a.out_t != kActF16 && a.out_t != kActBF16))
    return hipErrorInvalidValue;
  int runs = 0, blocks = 0;
  if (!get_rows_geometry(w, a.m, &runs, &blocks) || runs != a.runs || blocks != grid) return hipErrorInvalidValue;
  if (w.bits == 6) {
    if (!w.zps || w.k % 256 != 0) return hipErrorInvalidValue;
    const dim3 g(grid), b(kRowsWaves * 64);
    if (a.out_t == kActF32)
      hipLaunchKernelGGL(woq_get_rows_q6k_kernel<kActF32>, g, b, 0, st, a);
    else if (a.out_t == kActF16)
      hipLaunchKernelGGL(woq_get_rows_q6k_kernel<kActF16>, g, b, 0, st, a);
    else
      hipLaunchKernelGGL(woq_get_rows_q6k_kernel<kActBF16>, g, b, 0, st, a);
    return hipGetLastError();
  }
  if (w.bits == 4) {
    if (w.f4kind >= 3) return hipErrorInvalidValue;
    return w.f4kind >= 0 ? launch_rows_t<4, 1>(a, grid, st) : launch_rows_t<4, 0>(a, grid, st);
  }
  if (w.bits == 8) {
    if (w.f4kind >= 0 && w.f4kind < 3) return hipErrorInvalidValue;
    return w.f4kind >= 3 ? launch_rows_t<8, 2>(a, grid, st) : launch_rows_t<8, 0>(a, grid, st);
  }
  if (w.bits == 2 && w.f4kind < 0) return launch_rows_t<2, 0>(a, grid, st);
  return hipErrorInvalidValue;
}

}  // namespace nad
