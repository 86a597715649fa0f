// woq_q6k.hip -- GGUF Q6_K weights (neural_speed/core/data_types.h:133-138; dequantize_row_q6_K,
// vectors/cpu/quantize.h:956-999) at the file's own 6.5625 bits per weight: the repack into the layout of woq_layout.h,
// the unpack check, the two fp forward kernels, and -- the weight's own mode NAD_COMPUTE_Q8_K -- the reference's Q8_K
// activation quantizer and integer forward (woq_q6k_i8_kernel, below).
//
// A superblock is 256 weights w = d * sc * q: q in -32..31 (low nibbles in ql, high crumbs in qh), an int8 sc per 16
// weights, one fp16 d.  The quantizer writes sc up to +-127, so |sc * q| reaches 4096 and an fp16 B fragment holding
// sc * q is rounded (fp16 is exact only to 2048): at decode that costs 1.4e-4 .. 2.4e-4 of max|y|, seven to twelve
// times the 2e-5 bar.  So woq_q6k_gemv_kernel keeps q alone in the fp16 fragment (exact), multiplies one group of 16
// per v_mfma_f32_16x16x16_f16 -- whose K is exactly one group -- into a fresh accumulator, and applies float(sc) and
// then d in fp32.  woq_q6k_gemm_kernel (M > 16) folds sc * q into the fragment, rounded once (<= 2^-11 relative, the
// project's FOLD_TOL class), runs v_mfma_f32_16x16x32_f16 over two groups at a time and applies d per superblock.
// Banks of Q6_K experts (capi_moe.hip, route kind 2) run the same two bodies with the weight taken from the bank's
// device table: woq_q6k_gemv_routed_kernel, a problem per fp32 row, and woq_q6k_gemm_grouped_kernel over sorted rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "woq_device.h"
#include "woq_kernels.h"
#include "woq_launch.h"
#include "woq_layout.h"

namespace nad {

typedef _Float16 h4_t __attribute__((ext_vector_type(4)));

constexpr int kQ6kBlockBytes = 210;  // ql[128] qh[64] scales[16] d
constexpr int kQ8kBlockBytes = 292;  // block_q8_K: float d, int8 qs[256], int16 bsums[16]
constexpr int kQ6kWaves = 16;        // waves of a GEMV workgroup = K-slices of a stripe
constexpr size_t kQ6kLdsMax = 160 * 1024;
constexpr size_t kQ6kPartBytes = 2 * kQ6kWaves * 1024;  // two sets of per-wave 16 x 16 fp32 partials

// ------------------------------------------------------------------------------------------------ repack / unpack
// the stored 6-bit value v = q + 32 of element e of a block_q6_K: h = e / 128, j = (e % 128) / 32, l = e % 32; nibble
// ql[64 h + 32 (j & 1) + l] (low half for j < 2), crumb (qh[32 h + l] >> 2 j) & 3
__device__ __forceinline__ uint32_t q6k_value(const uint8_t* blk, int e) {
  const int h = e >> 7, j = (e & 127) >> 5, l = e & 31;
  const uint32_t ql = blk[64 * h + 32 * (j & 1) + l];
  const uint32_t nib = j < 2 ? (ql & 15u) : (ql >> 4);
  const uint32_t crumb = (uint32_t(blk[128 + 32 * h + l]) >> (2 * j)) & 3u;
  return nib | (crumb << 4);
}

// one thread per (row of the padded ns * 16, superblock): 210 bytes in; 48 dwords of the three pieces, 16 sub-scales
// and d out.  Rows past n write v = 32, sc = 0, d = 0, so nothing of the layout is left unwritten.
__global__ void nad_q6k_repack_kernel(const uint8_t* __restrict__ src, int n, int k, DeviceWeight w) {
  const int nsb = k / 256;
  const int64_t idx = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= int64_t(w.ns) * 16 * nsb) return;
  const int row = int(idx / nsb), b = int(idx % nsb);
  const bool real = row < n;
  const uint8_t* blk = src + (size_t(real ? row : 0) * nsb + b) * kQ6kBlockBytes;
  const int s = row >> 4, nl = row & 15;
  const size_t sb = size_t(s) * nsb + b;
  uint32_t* tiles = static_cast<uint32_t*>(w.tiles) + sb * 768;
  for (int kq = 0; kq < 4; kq++) {
    uint32_t* lane = tiles + (kq * 16 + nl) * 4;
    for (int pc = 0; pc < 2; pc++)
      for (int dd = 0; dd < 4; dd++) {
        uint32_t word = 0;
        for (int p = 0; p < 8; p++) {
          const int g = 8 * pc + 2 * dd + ((p & 3) >> 1), j = 2 * (p & 1) + (p >> 2);
          const uint32_t v = real ? q6k_value(blk, 16 * g + 4 * kq + j) : 32u;
          word |= (v & 15u) << (4 * p);
        }
        lane[pc * 256 + dd] = word;
      }
    for (int wd = 0; wd < 4; wd++) {
      uint32_t word = 0;
      for (int p = 0; p < 16; p++) {
        const int g = 4 * wd + ((p & 7) >> 1), j = 2 * (p & 1) + (p >> 3);
        const uint32_t v = real ? q6k_value(blk, 16 * g + 4 * kq + j) : 32u;
        word |= (v >> 4) << (2 * p);
      }
      lane[512 + wd] = word;
    }
  }
  int8_t* sc = w.zps + (sb * 16 + nl) * 16;
  for (int g = 0; g < 16; g++) sc[g] = real ? int8_t(blk[192 + g]) : int8_t(0);
  static_cast<uint16_t*>(w.scales)[sb * 16 + nl] = real ? uint16_t(blk[208] | (uint16_t(blk[209]) << 8)) : uint16_t(0);
}

// the layout back to fp32 [K][N]: (d * sc) * q with dequantize_row_q6_K's association, no contraction
__global__ void nad_q6k_unpack_kernel(DeviceWeight w, float* out) {
#pragma clang fp contract(off)
  const int nsb = w.nt;
  const uint64_t total = uint64_t(w.n) * w.k;
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < total; i += uint64_t(gridDim.x) * blockDim.x) {
    const int kk = int(i / w.n), n = int(i % w.n);
    const int s = n >> 4, nl = n & 15, b = kk >> 8, g = (kk & 255) >> 4, kq = (kk & 15) >> 2, j = kk & 3;
    const size_t sb = size_t(s) * nsb + b;
    const uint32_t* lane = static_cast<const uint32_t*>(w.tiles) + sb * 768 + (kq * 16 + nl) * 4;
    const int pl = 2 * (g & 1) + (j >> 1) + 4 * (j & 1);          // nibble position in dword (g & 7) >> 1 of piece g >> 3
    const int ph = 2 * (g & 3) + (j >> 1) + 8 * (j & 1);          // crumb position in dword g >> 2 of piece 2
    const uint32_t nib = (lane[(g >> 3) * 256 + ((g & 7) >> 1)] >> (4 * pl)) & 15u;
    const uint32_t crumb = (lane[512 + (g >> 2)] >> (2 * ph)) & 3u;
    const int q = int(nib | (crumb << 4)) - 32;
    const float d = float(static_cast<const _Float16*>(w.scales)[sb * 16 + nl]);
    const float ds = d * float(int(w.zps[(sb * 16 + nl) * 16 + g]));
    out[i] = ds * float(q);
  }
}

hipError_t launch_q6k_repack(const uint8_t* src, int n, int k, const DeviceWeight& w, hipStream_t st) {
  const int64_t total = int64_t(w.ns) * 16 * (k / 256);
  hipLaunchKernelGGL(nad_q6k_repack_kernel, dim3(int((total + 127) / 128)), dim3(128), 0, st, src, n, k, w);
  return hipGetLastError();
}

hipError_t launch_q6k_unpack(const DeviceWeight& w, float* out, hipStream_t st) {
  hipLaunchKernelGGL(nad_q6k_unpack_kernel, dim3(2048), dim3(256), 0, st, w, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ shared pieces
// The fp16 pair (q_j, q_j+1) of pair i of a group: lo already shifted right by 4 i, hi shifted so that its crumb pair
// sits at bits 4..5 / 20..21 (q6k_hi_at4)
__device__ __forceinline__ h2_t q6k_pair(uint32_t lo_sh, uint32_t hi_at4, h2_t m1056) {
  const uint32_t t = and_or(lo_sh, 0x000F000Fu, 0x64006400u);
  return as_h2(and_or(hi_at4, 0x00300030u, t)) + m1056;
}
// the crumb pair at position i (bits 2 i, 2 i + 16) of hi moved to bits 4 / 20
template <int I>
__device__ __forceinline__ uint32_t q6k_hi_at4(uint32_t hi) {
  if constexpr (2 * I >= 4) return hi >> (2 * I - 4);
  return hi << (4 - 2 * I);
}
// the four q of group G (0..15) of a superblock this lane holds, as an MFMA 16x16x16 B fragment
template <int G>
__device__ __forceinline__ h4_t q6k_group(const u4_t& lo0, const u4_t& lo1, const u4_t& hi, h2_t m1056) {
  const uint32_t lo = (G < 8 ? lo0 : lo1)[(G & 7) >> 1];
  const uint32_t hw = hi[G >> 2];
  constexpr int IL = 2 * (G & 1), IH = 2 * (G & 3);
  const h2_t p0 = q6k_pair(lo >> (4 * IL), q6k_hi_at4<IH>(hw), m1056);
  const h2_t p1 = q6k_pair(lo >> (4 * IL + 4), q6k_hi_at4<IH + 1>(hw), m1056);
  return h4_t{p0[0], p0[1], p1[0], p1[1]};
}
__device__ __forceinline__ int q6k_sc(const u4_t& sc, int g) {  // sub-scale g of the lane's 16
  return __builtin_amdgcn_sbfe(int(sc[g >> 2]), 8 * (g & 3), 8);
}
// d of column nl from the 16 bytes holding columns 8 (nl >> 3) .. + 7
__device__ __forceinline__ float q6k_d(const u4_t& dv, int nl) {
  const uint32_t lo2 = (nl & 2) ? dv[1] : dv[0], hi2 = (nl & 2) ? dv[3] : dv[2];
  const uint32_t wsel = (nl & 4) ? hi2 : lo2;
  return f16_bits_to_f32(uint16_t((nl & 1) ? (wsel >> 16) : (wsel & 0xffffu)));
}

// ------------------------------------------------------------------------------------------------ GEMV, M <= 16
// Workgroups own whole stripes (blockIdx.x, + gridDim.x, ...); the 16 waves of a workgroup own the superblocks
// b = wave, wave + 16, ... of each (any superblock count; a wave without one adds zeros).  blockIdx.y selects a pass of
// rows_pp activation rows (q6k_gemv_geometry).  A wave sends the three 16-B-per-lane nontemporal loads of its first
// superblock, its sub-scales and d before anything else, then the workgroup stages the pass's activations into LDS as
// fp16 rows -- the rows themselves for fp16 activations, a hi and a lo row per activation row (x = hi + lo to 2^-22)
// for fp32 / bf16 -- with the 16-byte chunks of row r XORed by r (the fragment reads are then conflict-free).  While a
// superblock is multiplied the next one (of the next stripe at the end) is in flight.  Per group: q (exact fp16)
// through one 16x16x16 MFMA onto C = 0, then acc_sb += float(sc) * p; per superblock acc += d * acc_sb.  The waves'
// 16 x 16 partials meet in LDS (two sets, by stripe parity: one barrier per stripe) and one wave, taking turns, sums
// them in wave order, adds lo to hi rows and runs gemm_epilogue4.  No atomics, no workspace: the same inputs give the
// same bits on every launch.
struct Q6kGemvArgs {
  GemmArgs g;
  int rows_pp;
};

template <int AT>
__global__ __launch_bounds__(kQ6kWaves * 64) void woq_q6k_gemv_kernel(Q6kGemvArgs qa) {
  extern __shared__ __attribute__((aligned(16))) char q6k_lds[];
  constexpr bool HILO = AT != kActF16;
  const GemmArgs& a = qa.g;
#define Q6K_ROWS_PP (qa.rows_pp)
#define Q6K_WG_ROW0 (blockIdx.y * qa.rows_pp)
#define Q6K_WG_INDEX (blockIdx.x)
#define Q6K_WG_COUNT (gridDim.x)
#include "woq_q6k_gemv_body.inc"
#undef Q6K_ROWS_PP
#undef Q6K_WG_ROW0
#undef Q6K_WG_INDEX
#undef Q6K_WG_COUNT
}

// Routed (nad_device_mul_mat_id / nad_device_moe_ffn on a bank of Q6_K experts): the same body once more, a problem
// being one fp32 row (M = 1: its hi and its lo fp16 row).  Workgroup b serves problem p = b / wpp -- row r = p / slots,
// slot p % slots -- and that problem's stripes b % wpp, + wpp, ...; the 16 waves own the superblocks as above and the
// partials are summed in wave order, so a stripe's bits do not depend on wpp: a routed row has the bits of the
// expert's own M = 1 forward.  The expert id is one wave-uniform load, clamped before the table is touched; the three
// weight pointers come from the bank's 64-byte entry.  An id outside [0, n_expert) loads no weight and applies no
// epilogue: the workgroup writes +0.0 to its stripes of the problem's output row and leaves before any barrier.
// aux_out: the multiplier of the kEpiSiluMul epilogue is the problem's own output row (t = t * (x . U^T) in place: the
// lane that reads an element is the one that writes it).
struct Q6kRoutedArgs {
  GemmArgs g;  // M = 1, K, the epilogue kind; w: the bank's shape (the pointers are the kernel's to fill)
  GemvRouted r;
  int aux_out;
};
__global__ __launch_bounds__(kQ6kWaves * 64) void woq_q6k_gemv_routed_kernel(Q6kRoutedArgs qa) {
  extern __shared__ __attribute__((aligned(16))) char q6k_lds[];
  constexpr int AT = kActF32;
  constexpr bool HILO = true;
  const GemvRouted& r = qa.r;
  const int p = int(blockIdx.x) / r.wpp;
  const int wg_index = int(blockIdx.x) - p * r.wpp, wg_count = r.wpp;
  const int row = p / r.slots;
  const int id = __builtin_amdgcn_readfirstlane(r.ids[size_t(row) * r.ids_ld + r.ids_col + (p - row * r.slots)]);
  const bool valid = unsigned(id) < unsigned(r.n_expert);
  const int e = min(max(id, 0), r.n_expert - 1);
  float* out = r.out + size_t(p) * r.out_ld;
  if (!valid) {
    const int n = int(threadIdx.x);
    for (int s = wg_index; s < qa.g.w.ns; s += r.wpp)
      if (n < 16 && s * 16 + n < qa.g.w.n) out[s * 16 + n] = 0.f;
    return;
  }
  const GemvExpertEnt g = r.bank[0][e];
  GemmArgs a = qa.g;
  a.A = r.act + size_t(r.act_per_slot ? p : row) * r.act_ld;
  a.w.tiles = g.tiles;
  a.w.scales = g.scales;
  a.w.zps = g.zps;
  a.w.out = out;
  if (qa.aux_out) a.aux = out;
#define Q6K_ROWS_PP 1
#define Q6K_WG_ROW0 0
#define Q6K_WG_INDEX (wg_index)
#define Q6K_WG_COUNT (wg_count)
#include "woq_q6k_gemv_body.inc"
#undef Q6K_ROWS_PP
#undef Q6K_WG_ROW0
#undef Q6K_WG_INDEX
#undef Q6K_WG_COUNT
}

bool q6k_gemv_geometry(int m, int k, int ns, int act_t, int cus, Q6kGemvGeom* g) {
  const size_t row_bytes = size_t(k) * 2;
  const int per = act_t == kActF16 ? 1 : 2;  // fp16 rows in LDS per activation row
  int cap = int(std::min<size_t>((kQ6kLdsMax - kQ6kPartBytes) / row_bytes, 16)) / per;
  if (cap < 1) return false;
  g->rows_pp = std::min(m, cap);
  g->passes = (m + g->rows_pp - 1) / g->rows_pp;
  g->grid = std::max(1, std::min(ns, cus));
  g->waves = kQ6kWaves;
  g->lds = size_t(g->rows_pp) * per * row_bytes + kQ6kPartBytes;
  return true;
}

hipError_t launch_q6k_gemv(const GemmArgs& a, int act_t, const Q6kGemvGeom& g, hipStream_t st) {
  if (a.M < 1 || a.M > 16 || a.K % 256 != 0 || g.lds > kQ6kLdsMax || g.rows_pp < 1) return hipErrorInvalidValue;
  Q6kGemvArgs qa{a, g.rows_pp};
  const dim3 grid(g.grid, g.passes), block(kQ6kWaves * 64);
  if (act_t == kActF32) return launch_big_lds<woq_q6k_gemv_kernel<kActF32>>(grid, block, g.lds, st, qa);
  if (act_t == kActF16) return launch_big_lds<woq_q6k_gemv_kernel<kActF16>>(grid, block, g.lds, st, qa);
  return launch_big_lds<woq_q6k_gemv_kernel<kActBF16>>(grid, block, g.lds, st, qa);
}

bool q6k_routed_geometry(int k, int ns, int64_t nprob, int cus, Q6kRoutedGeom* g) {
  g->lds = size_t(k) * 4 + kQ6kPartBytes;  // the hi and the lo fp16 row, then the partials
  g->waves = kQ6kWaves;
  g->wpp = g->grid = 0;
  if (k < 256 || k % 256 != 0 || g->lds > kQ6kLdsMax || nprob < 1 || ns < 1) return false;
  g->wpp = int(std::max<int64_t>(1, std::min<int64_t>(ns, cus / nprob)));
  if (nprob * g->wpp >= (int64_t(1) << 31)) return false;
  g->grid = int(nprob * g->wpp);
  return true;
}

hipError_t launch_q6k_gemv_routed(const GemmArgs& a, const GemvRouted& r, bool aux_out, const Q6kRoutedGeom& g,
                                  hipStream_t st) {
  if (a.M != 1 || a.K < 256 || a.K % 256 != 0 || g.lds != size_t(a.K) * 4 + kQ6kPartBytes || g.lds > kQ6kLdsMax ||
      r.wpp < 1 || r.wpp != g.wpp || g.grid < 1 || g.grid % r.wpp != 0 || r.n_expert < 1 || r.slots < 1)
    return hipErrorInvalidValue;
  Q6kRoutedArgs qa{a, r, aux_out ? 1 : 0};
  return launch_big_lds<woq_q6k_gemv_routed_kernel>(dim3(g.grid), dim3(kQ6kWaves * 64), g.lds, st, qa);
}

// ------------------------------------------------------------------------------------------------ GEMM, M > 16
// Register-staged MFMA tile kernel in the manner of woq_gemm_kernel (woq_kernels.hip): a 128 x 128 output tile per
// workgroup, 8 waves as 4 (M) x 2 (N), a wave 32 rows x 4 stripes; the K step is half a superblock (128).  A goes
// through LDS as fp16 (16-B chunks XOR-swizzled by the row); the quants of the wave's four stripes are loaded a step
// ahead.  A lane's low-nibble dword holds two groups (woq_layout.h), which is one v_mfma_f32_16x16x32_f16: the B
// fragment is fp16(sc * q) -- q exact, sc an fp16 integer, the product rounded once -- and the lane's A fragment the
// matching two runs of four k.  acc_sb collects a superblock, acc += d * acc_sb in fp32.
template <int AT>
__global__ __launch_bounds__(512) void woq_q6k_gemm_kernel(GemmArgs a) {
#define Q6K_GEMM_TILE                                      \
  const SkinnyWeight& W = a.w;                             \
  const int nbm = (a.M + BM - 1) / BM;                     \
  const int bn = blockIdx.x / nbm, bm = blockIdx.x % nbm;  \
  const int m0 = bm * BM;
#define Q6K_GEMM_M (a.M)
#define Q6K_GEMM_A_ROWS
#define Q6K_GEMM_A_ROW(p, row) (row)
#include "woq_q6k_gemm_body.inc"
#undef Q6K_GEMM_TILE
#undef Q6K_GEMM_M
#undef Q6K_GEMM_A_ROWS
#undef Q6K_GEMM_A_ROW
}

// Grouped (nad_device_moe_ffn_grouped / nad_device_mul_mat_id_grouped on a bank of Q6_K experts): the body above over
// each expert's sorted rows.  Workgroup -> (tile, column tile), the column tiles of one tile in consecutive workgroups
// as in woq_gemm7_grouped_kernel; the tile's expert and sorted rows [q0, q1), q1 - q0 <= 128, come from the table the
// sort wrote, the weight pointers from the bank's entry of that expert.  A is fp16: rows gathered through gg.rows (the
// activation row of a sorted row) or the sorted rows as they lie; the result goes to the sorted row.  A workgroup past
// the device tile count leaves before any barrier.  An MFMA row depends on its own A row alone, so a sorted row's
// bits depend neither on its tile nor on the batch: they are those of woq_q6k_gemm_kernel on that fp16 row.
__global__ __launch_bounds__(512) void woq_q6k_gemm_grouped_kernel(GemmArgs a, GemmGrouped gg) {
  constexpr int AT = kActF16;
  const int nbn = (a.w.ns + 7) / 8;
  const int tile = int(blockIdx.x) / nbn, bn = int(blockIdx.x) - tile * nbn;
  if (tile >= __builtin_amdgcn_readfirstlane(*gg.ntiles)) return;
  const int4 te = gg.tiles[tile];  // (expert, q0, q1, 0): q0 < q1 <= q0 + 128, expert < n_expert (the sort's contract)
  const int m0 = __builtin_amdgcn_readfirstlane(te.y), q1 = __builtin_amdgcn_readfirstlane(te.z);
  const GemvExpertEnt ge = gg.bank[__builtin_amdgcn_readfirstlane(te.x)];
  SkinnyWeight Wg = a.w;
  Wg.tiles = ge.tiles;
  Wg.scales = ge.scales;
  Wg.zps = ge.zps;
#define Q6K_GEMM_TILE const SkinnyWeight& W = Wg;
#define Q6K_GEMM_M (q1)
  // the A rows of the thread's four tile rows, read once (a row past q1 is never loaded: it takes the last row's)
#define Q6K_GEMM_A_ROWS                                      \
  int asrc[4];                                               \
  _Pragma("unroll") for (int p = 0; p < 4; p++) {            \
    const int q = min(m0 + r0 + p * 32, q1 - 1);             \
    asrc[p] = gg.rows ? gg.rows[q] : q;                      \
  }
#define Q6K_GEMM_A_ROW(p, row) (asrc[p])
#include "woq_q6k_gemm_body.inc"
#undef Q6K_GEMM_TILE
#undef Q6K_GEMM_M
#undef Q6K_GEMM_A_ROWS
#undef Q6K_GEMM_A_ROW
}

hipError_t launch_q6k_gemm(const GemmArgs& a, int act_t, hipStream_t st) {
  if (a.K % 256 != 0) return hipErrorInvalidValue;
  const dim3 grid(((a.M + 127) / 128) * ((a.w.ns + 7) / 8));
  if (act_t == kActF32)
    hipLaunchKernelGGL(woq_q6k_gemm_kernel<kActF32>, grid, dim3(512), 0, st, a);
  else if (act_t == kActF16)
    hipLaunchKernelGGL(woq_q6k_gemm_kernel<kActF16>, grid, dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL(woq_q6k_gemm_kernel<kActBF16>, grid, dim3(512), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_q6k_gemm_grouped(const GemmArgs& a, const GemmGrouped& gg, int grid, hipStream_t st) {
  // the fp16 rows are read in 16-byte chunks: a 16-byte base and a row pitch of whole chunks
  if (a.K < 256 || a.K % 256 != 0 || grid < 1 || !a.A || a.lda < a.K || a.lda % 8 != 0 ||
      reinterpret_cast<uintptr_t>(a.A) % 16 != 0 || !gg.bank || !gg.tiles || !gg.ntiles)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(woq_q6k_gemm_grouped_kernel, dim3(grid), dim3(512), 0, st, a, gg);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ Q8_K activations
// quantize_row_q8_K_reference (vectors/cpu/quantize.h:1020-1055) for one superblock of one row, by one wave: lane l
// holds x[4 l .. 4 l + 3].  max is the signed value of the first element with the strictly largest |x|: the lane's own
// first one, then the one of the lowest lane whose largest |x| equals the wave's (lane order is element order).  The
// wave's largest |x| is reduced on the bit patterns (non-negative floats order as unsigned integers) with DPP inside
// the rows of 16 lanes and four v_readlane across them: no LDS round trip;
// iscale = -128 / max, q = min(127, nearest_int(iscale * x))
// with the reference's magic-number rounding and no contraction of the product into the add, d = 1 / iscale.  Returns
// the lane's four codes (byte j = element 4 l + j), d, and the sum of the 16 codes of group l >> 2.  An all-zero
// superblock gives d = 0, codes 0 and sums 0.  Every lane of the wave must call it.
template <int CTRL>
__device__ __forceinline__ int q8k_dpp(int v) {  // v of the lane the DPP control selects (all lanes active)
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, true);
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E;              // quad_perm [1,0,3,2] / [2,3,0,1]
constexpr int kDppHalfMirror = 0x141, kDppRowMirror = 0x140;  // lane i <-> 7 - i of its 8 / 15 - i of its 16
struct Q8kLane {
  uint32_t codes;
  float d;
  int bsum;
};
__device__ __forceinline__ Q8kLane q8k_quant_wave(const float (&x)[4], int lane) {
#pragma clang fp contract(off)
  float lmax = 0.f, lmx = 0.f;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float ax = fabsf(x[j]);
    if (ax > lmax) {
      lmax = ax;
      lmx = x[j];
    }
  }
  const uint32_t lbits = __float_as_uint(lmax);
  uint32_t rmax = lbits;
  rmax = max(rmax, uint32_t(q8k_dpp<kDppXor1>(int(rmax))));
  rmax = max(rmax, uint32_t(q8k_dpp<kDppXor2>(int(rmax))));
  rmax = max(rmax, uint32_t(q8k_dpp<kDppHalfMirror>(int(rmax))));
  rmax = max(rmax, uint32_t(q8k_dpp<kDppRowMirror>(int(rmax))));
  const uint32_t amax = max(max(uint32_t(__builtin_amdgcn_readlane(int(rmax), 0)),
                                uint32_t(__builtin_amdgcn_readlane(int(rmax), 16))),
                            max(uint32_t(__builtin_amdgcn_readlane(int(rmax), 32)),
                                uint32_t(__builtin_amdgcn_readlane(int(rmax), 48))));
  Q8kLane r{0u, 0.f, 0};
  const int first = __builtin_ctzll(__ballot(lbits == amax));  // wave-uniform; some lane holds amax, so the mask is not 0
  const float mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lmx), first));
  // an all-zero superblock takes iscale = 0 (every code 0) and d = 0 with no branch, so that the quantizations a wave
  // runs side by side interleave
  const float iscale = mx != 0.f ? -128.f / mx : 0.f;
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float p = iscale * x[j];
    const float val = p + 12582912.f;
    int q = (__float_as_int(val) & 0x007fffff) - 0x00400000;
    q = min(127, q);
    s += q;
    r.codes |= uint32_t(q & 0xff) << (8 * j);
  }
  s += q8k_dpp<kDppXor1>(s);
  s += q8k_dpp<kDppXor2>(s);
  r.bsum = s;
  r.d = mx != 0.f ? 1.f / iscale : 0.f;
  return r;
}

// The four activations A[row][k0 .. k0 + 3]: the loads (load_a4_raw: one 16- or 8-byte load where the rows are 16-byte
// aligned, VEC, else four element loads) apart from the conversion to fp32 (cvt_a4), so that a wave can send the loads
// of several superblocks before it waits for the first
template <int AT, bool VEC>
__device__ __forceinline__ u4_t load_a4_raw(const void* A, int lda, int row, int k0) {
  const size_t base = size_t(row) * lda + k0;
  if constexpr (AT == kActF32) {
    const uint32_t* p = static_cast<const uint32_t*>(A) + base;
    if constexpr (VEC) return *reinterpret_cast<const u4_t*>(p);
    return u4_t{p[0], p[1], p[2], p[3]};
  } else {
    const uint16_t* p = static_cast<const uint16_t*>(A) + base;
    if constexpr (VEC) {
      const uint2 x = *reinterpret_cast<const uint2*>(p);
      return u4_t{x.x, x.y, 0u, 0u};
    }
    return u4_t{p[0], p[1], p[2], p[3]};
  }
}
template <int AT, bool VEC>
__device__ __forceinline__ void cvt_a4(const u4_t& raw, float (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if constexpr (AT == kActF32) {
      v[j] = __uint_as_float(raw[j]);
    } else {
      const uint16_t h = VEC ? uint16_t(raw[j >> 1] >> (16 * (j & 1))) : uint16_t(raw[j]);
      v[j] = AT == kActF16 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h);
    }
  }
}

// block_q8_K rows {float d; int8 qs[256]; int16 bsums[16]}: one wave per (row, superblock)
struct Q8kArgs {
  const void* A;
  int lda, M, K, vec_ok;
  char* blocks;
};
template <int AT>
__global__ __launch_bounds__(256) void nad_q8_k_quant_kernel(Q8kArgs a) {
  const int nsb = a.K / 256;
  const int lane = threadIdx.x & 63;
  const int64_t idx = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (idx >= int64_t(a.M) * nsb) return;
  const int row = int(idx / nsb), b = int(idx % nsb);
  float x[4];
  if (a.vec_ok)
    cvt_a4<AT, true>(load_a4_raw<AT, true>(a.A, a.lda, row, 256 * b + 4 * lane), x);
  else
    cvt_a4<AT, false>(load_a4_raw<AT, false>(a.A, a.lda, row, 256 * b + 4 * lane), x);
  const Q8kLane q = q8k_quant_wave(x, lane);
  char* blk = a.blocks + size_t(idx) * kQ8kBlockBytes;  // 292 = 4 * 73: every field keeps its alignment
  if (lane == 0) *reinterpret_cast<float*>(blk) = q.d;
  *reinterpret_cast<uint32_t*>(blk + 4 + 4 * lane) = q.codes;
  if ((lane & 3) == 0) *reinterpret_cast<int16_t*>(blk + 260 + 2 * (lane >> 2)) = int16_t(q.bsum);
}

hipError_t launch_q8_k_quant(const void* A, int act_t, int lda, int m, int k, void* blocks, hipStream_t st) {
  if (m < 1 || k < 256 || k % 256 != 0 || !A || !blocks) return hipErrorInvalidValue;
  const int esz = act_t == kActF32 ? 4 : 2;
  const bool vec_ok = reinterpret_cast<uintptr_t>(A) % 16 == 0 && (size_t(lda) * esz) % 16 == 0;
  const Q8kArgs a{A, lda, m, k, vec_ok ? 1 : 0, static_cast<char*>(blocks)};
  const int64_t total = int64_t(m) * (k / 256);
  const dim3 grid(unsigned((total + 3) / 4)), block(256);
  if (act_t == kActF32)
    hipLaunchKernelGGL(nad_q8_k_quant_kernel<kActF32>, grid, block, 0, st, a);
  else if (act_t == kActF16)
    hipLaunchKernelGGL(nad_q8_k_quant_kernel<kActF16>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(nad_q8_k_quant_kernel<kActBF16>, grid, block, 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ Q8_K integer forward
// ggml_vec_dot_q6_K_q8_K's arithmetic (core/layers/vec_dot.h:1190-1231) on v_mfma_i32_16x16x64_i8.  Per output row r,
// column c and superblock b:
//   isum_b = sum_{g < 16} sc[g] * sum_{i < 16} q[16 g + i] * a[16 g + i]        exact in int32 (|isum_b| <= 2^27)
//   y      = sum_b fp32(fp32(d_w[b]) * d_a[r][b]) * float(isum_b)              fp32
// in this order: a wave adds its superblocks b = wave, wave + 16, ... in ascending order with one fma each onto 0, and
// one wave adds the 16 waves' partials in wave order (the reference's eight interleaved fp32 partials are not
// reproduced).
//
// The workgroup structure is woq_q6k_gemv_kernel's.  Staging quantizes the pass's rows with q8k_quant_wave, a wave per
// (row, superblock), and leaves in LDS: the codes (row stride K + 64 bytes: the four rows a fragment read touches fall
// in different banks; inside every run of four k the bytes are in the order 0, 2, 1, 3, the order the weight bytes
// come out of the nibble / crumb dwords with the fewest operations), d_a as [superblock][16 rows], and -32 times the
// block sums as int32 [superblock][row set][4 rows][group].
//
// One MFMA issue spans four groups (64 k).  The lane's B operand is the four dwords of stored values v = q + 32
// (0 .. 63) of groups 4 t .. 4 t + 3: B[k slot (kq, i, j)][n = nl] = v[16 (4 t + i) + 4 kq + j].  A row 4 m + i holds
// the codes of activation row m (of the row set) in dword i alone, zeros elsewhere, so C row 4 m + i is the dot
// product of group 4 t + i for row m -- and by the C/D map (row = 4 (lane >> 4) + reg) lane (nl, kq) holds in register
// i the dot product of group 4 t + i for row kq, whose sub-scale is byte i of dword t of the 16 the lane already has.
// The C input is -32 * bsum of that (row, group): sum (v - 32) a = sum v a - 32 bsum, exact.  isum += sc * C is one
// v_mad_i32_i24 per group (|C| <= 2^16), so after the four issues of a superblock the lane holds the whole isum of
// its (row, column) with no exchange between lanes.  Four issues per superblock and row set of four rows.
typedef int i4_t __attribute__((ext_vector_type(4)));

struct Q6kI8Args {
  GemmArgs g;
  int rows_pp, rs_pp;  // activation rows per pass; row sets of four the pass works on (the kernel's RS)
};

// the bytes v of group G (elements 4 kq + 0, 2, 1, 3 in bytes 0 .. 3) from the lane's nibble and crumb dwords
template <int S>
__device__ __forceinline__ uint32_t q6k_shl(uint32_t x) {  // x << S, S < 0: x >> -S
  if constexpr (S >= 0) return x << S;
  return x >> (-S);
}
template <int G>
__device__ __forceinline__ uint32_t q6k_bytes(const u4_t& lo0, const u4_t& lo1, const u4_t& hi) {
  const uint32_t lo = (G < 8 ? lo0 : lo1)[(G & 7) >> 1];
  const uint32_t hw = hi[G >> 2];
  constexpr int GP = G & 1, G4 = G & 3;
  const uint32_t x = GP ? lo >> 8 : lo;
  uint32_t t = x & 0x000F000Fu;
  t = and_or(x << 4, 0x0F000F00u, t);
  t = and_or(q6k_shl<4 - 4 * G4>(hw), 0x00300030u, t);
  return and_or(q6k_shl<10 - 4 * G4>(hw), 0x30003000u, t);
}

// RS: the row sets of four rows a pass works on (1: the decode case; 2; 4) = Q6kI8Geom::rs_pp.  All RS of them are
// staged and multiplied with no test on the row count, so that the LDS reads and the MFMAs of the row sets of one
// issue go out together; rows past mloc are zeros (d_a = 0) and are not written out.
template <int AT, int RS>
__global__ __launch_bounds__(kQ6kWaves * 64) void woq_q6k_i8_kernel(Q6kI8Args qa) {
  extern __shared__ __attribute__((aligned(16))) char q6k_lds[];
  const GemmArgs& a = qa.g;
  const SkinnyWeight& W = a.w;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar
  const int nl = lane & 15, kq = lane >> 4;
  const int nsb = W.nt, ns = W.ns, K = a.K;
  const int row0 = blockIdx.y * qa.rows_pp;
  const int mloc = min(qa.rows_pp, a.M - row0);
  constexpr int rs_pp = RS;
  const int rstride = K + 64;
  char* codes = q6k_lds;
  float* da = reinterpret_cast<float*>(q6k_lds + size_t(qa.rows_pp) * rstride);
  int* nb = reinterpret_cast<int*>(da + size_t(nsb) * 16);
  float* part = reinterpret_cast<float*>(nb + size_t(nsb) * rs_pp * 64);

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
  int s = blockIdx.x;
  if (has && s < ns) fetch(s, wave, c0, c1, c2, csc, cd);

  // stage: a wave per (row, superblock) over the 4 RS rows of the pass's row sets, U at a time with their loads sent
  // together.  Rows past mloc get d_a = 0 and zero sums (their codes are never read: the fragment reads below take
  // row 0 instead)
  auto stage = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    constexpr int U = RS == 1 ? 4 : 8;
    constexpr int rows = 4 * RS;
    // the wave's tasks are wave, wave + 16, ... of the rows * nsb in (row, superblock) order; (tr, tb) is its next one
    const int q16 = kQ6kWaves / nsb, r16 = kQ6kWaves - q16 * nsb;
    int tr = wave / nsb, tb = wave - tr * nsb;
    u4_t raw[U];
    int rr[U], bb[U];
    // no branch in here (the loads stay back to back, and the first batch goes out right behind the weight loads
    // above): a task of a row past mloc loads what the last real row's does and the value is dropped below
    auto load = [&]() {
#pragma unroll
      for (int u = 0; u < U; u++) {
        rr[u] = tr;
        bb[u] = tb;
        raw[u] = load_a4_raw<AT, VEC>(a.A, a.lda, row0 + min(tr, mloc - 1), 256 * tb + 4 * lane);
        tr += q16;
        tb += r16;
        if (tb >= nsb) {
          tb -= nsb;
          tr++;
        }
      }
    };
    load();
    while (rr[0] < rows) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int r = rr[u], b = bb[u];
        if (r < rows) {
          Q8kLane q{0u, 0.f, 0};
          if (r < mloc) {
            float x[4];
            cvt_a4<AT, VEC>(raw[u], x);
            q = q8k_quant_wave(x, lane);
            *reinterpret_cast<uint32_t*>(codes + size_t(r) * rstride + 256 * b + 4 * lane) =
                __builtin_amdgcn_perm(0u, q.codes, 0x03010200u);
          }
          if (lane == 0) da[b * 16 + r] = q.d;
          if ((lane & 3) == 0) nb[((b * rs_pp + (r >> 2)) * 4 + (r & 3)) * 16 + (lane >> 2)] = -32 * q.bsum;
        }
      }
      if (tr >= rows) break;
      load();
    }
  };
  if (a.vec_ok)
    stage(std::true_type{});
  else
    stage(std::false_type{});
  __syncthreads();

  // A row nl = 4 m + i: dword i of the fragment, activation row m of the row set
  const int ai = nl & 3, am = nl >> 2;
  const uint32_t am0 = ai == 0 ? ~0u : 0u, am1 = ai == 1 ? ~0u : 0u, am2 = ai == 2 ? ~0u : 0u, am3 = ai == 3 ? ~0u : 0u;
  const char* abase[RS];
#pragma unroll
  for (int rs = 0; rs < RS; rs++) {
    const int r = 4 * rs + am;
    abase[rs] = codes + size_t(r < mloc ? r : 0) * rstride + 16 * ai + 4 * kq;
  }
  for (int it = 0; s < ns; s += gridDim.x, it++) {
    float acc[RS];  // row 4 rs + kq, column nl
#pragma unroll
    for (int rs = 0; rs < RS; rs++) acc[rs] = 0.f;
    if (has) {
      for (int b = wave; b < nsb; b += kQ6kWaves) {
        int s2 = s, b2 = b + kQ6kWaves;
        if (b2 >= nsb) {
          s2 = s + gridDim.x;
          b2 = wave;
        }
        u4_t n0 = c0, n1 = c1, n2 = c2, nsc = csc, nd = cd;
        if (s2 < ns) fetch(s2, b2, n0, n1, n2, nsc, nd);
        int isum[RS];
#pragma unroll
        for (int rs = 0; rs < RS; rs++) isum[rs] = 0;
        auto issue = [&](auto tc) {
          constexpr int T = decltype(tc)::value;
          const i4_t bf{int(q6k_bytes<4 * T>(c0, c1, c2)), int(q6k_bytes<4 * T + 1>(c0, c1, c2)),
                        int(q6k_bytes<4 * T + 2>(c0, c1, c2)), int(q6k_bytes<4 * T + 3>(c0, c1, c2))};
          const int scw = int(csc[T]);
#pragma unroll
          for (int rs = 0; rs < RS; rs++) {
            {
              const uint32_t av = *reinterpret_cast<const uint32_t*>(abase[rs] + 256 * b + 64 * T);
              const i4_t af{int(av & am0), int(av & am1), int(av & am2), int(av & am3)};
              const i4_t cin = *reinterpret_cast<const i4_t*>(nb + ((b * rs_pp + rs) * 4 + kq) * 16 + 4 * T);
              const i4_t c = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, cin, 0, 0, 0);
#pragma unroll
              for (int i = 0; i < 4; i++) isum[rs] += __mul24(__builtin_amdgcn_sbfe(scw, 8 * i, 8), c[i]);
            }
          }
        };
        issue(std::integral_constant<int, 0>{});
        issue(std::integral_constant<int, 1>{});
        issue(std::integral_constant<int, 2>{});
        issue(std::integral_constant<int, 3>{});
        const float df = q6k_d(cd, nl);
#pragma unroll
        for (int rs = 0; rs < RS; rs++) {
          {
            const float f = df * da[b * 16 + 4 * rs + kq];
            acc[rs] = __builtin_fmaf(f, float(isum[rs]), acc[rs]);
          }
        }
        c0 = n0;
        c1 = n1;
        c2 = n2;
        csc = nsc;
        cd = nd;
      }
    }
    // partial of this wave: rows 4 rs + kq, column nl (the rows of an RS = 1 launch are 0 .. 3: the reduce below
    // writes out rows below mloc <= 4 only)
    float* slot = part + size_t(it & 1) * (kQ6kWaves * 256);
#pragma unroll
    for (int rs = 0; rs < RS; rs++) slot[wave * 256 + (4 * rs + kq) * 16 + nl] = acc[rs];
    __syncthreads();
    if (wave == (it & (kQ6kWaves - 1))) {
      const int row = lane >> 2, n0 = 4 * (lane & 3);
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int w = 0; w < kQ6kWaves; w++) {  // wave order
        const float4 pv = *reinterpret_cast<const float4*>(slot + w * 256 + row * 16 + n0);
        v[0] += pv.x;
        v[1] += pv.y;
        v[2] += pv.z;
        v[3] += pv.w;
      }
      if (row < mloc && s * 16 + n0 < W.n) gemm_epilogue4(a, row0 + row, s * 16 + n0, v);
    }
  }
}

bool q6k_i8_geometry(int m, int k, int ns, int cus, Q6kI8Geom* g) {
  // per row: K + 64 code bytes; per row set: 256 bytes of sums per superblock; d_a: 64 bytes per superblock
  const size_t nsb = size_t(k) / 256, budget = kQ6kLdsMax - kQ6kPartBytes;
  auto need = [&](int rows) {
    return size_t(rows) * (size_t(k) + 64) + nsb * 64 + nsb * size_t(rows <= 4 ? 1 : (rows <= 8 ? 2 : 4)) * 256;
  };
  int rows = std::min(m, 16);
  while (rows >= 1 && need(rows) > budget) rows--;
  if (rows < 1) return false;
  g->rows_pp = rows;
  g->rs_pp = rows <= 4 ? 1 : (rows <= 8 ? 2 : 4);
  g->passes = (m + rows - 1) / rows;
  g->grid = std::max(1, std::min(ns, cus));
  g->waves = kQ6kWaves;
  g->lds = need(rows) + kQ6kPartBytes;
  return true;
}

hipError_t launch_q6k_i8(const GemmArgs& a, int act_t, const Q6kI8Geom& g, hipStream_t st) {
  if (a.M < 1 || a.K < 256 || a.K % 256 != 0 || g.lds > kQ6kLdsMax || g.rows_pp < 1 || g.rows_pp > 16 ||
      g.passes != (a.M + g.rows_pp - 1) / g.rows_pp || g.passes > 65535)
    return hipErrorInvalidValue;
  Q6kI8Args qa{a, g.rows_pp, g.rs_pp};
  const dim3 grid(g.grid, g.passes), block(kQ6kWaves * 64);
  if (g.rs_pp != (g.rows_pp <= 4 ? 1 : (g.rows_pp <= 8 ? 2 : 4))) return hipErrorInvalidValue;
  if (g.rs_pp == 1) {
    if (act_t == kActF32) return launch_big_lds<woq_q6k_i8_kernel<kActF32, 1>>(grid, block, g.lds, st, qa);
    if (act_t == kActF16) return launch_big_lds<woq_q6k_i8_kernel<kActF16, 1>>(grid, block, g.lds, st, qa);
    return launch_big_lds<woq_q6k_i8_kernel<kActBF16, 1>>(grid, block, g.lds, st, qa);
  }
  if (g.rs_pp == 2) {
    if (act_t == kActF32) return launch_big_lds<woq_q6k_i8_kernel<kActF32, 2>>(grid, block, g.lds, st, qa);
    if (act_t == kActF16) return launch_big_lds<woq_q6k_i8_kernel<kActF16, 2>>(grid, block, g.lds, st, qa);
    return launch_big_lds<woq_q6k_i8_kernel<kActBF16, 2>>(grid, block, g.lds, st, qa);
  }
  if (act_t == kActF32) return launch_big_lds<woq_q6k_i8_kernel<kActF32, 4>>(grid, block, g.lds, st, qa);
  if (act_t == kActF16) return launch_big_lds<woq_q6k_i8_kernel<kActF16, 4>>(grid, block, g.lds, st, qa);
  return launch_big_lds<woq_q6k_i8_kernel<kActBF16, 4>>(grid, block, g.lds, st, qa);
}

}  // namespace nad
