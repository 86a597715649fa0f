// woq_kernels.h -- launch-argument structs and launchers of the gfx950 WOQ kernels (woq_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "woq_gguf.h"
#include "woq_layout.h"

namespace nad {

enum ActType : int { kActF32 = 0, kActF16 = 1, kActBF16 = 2 };

struct RepackArgs {
  // source blob (already on the device): interleaved [NPad/NTILE][KPad/PR][NTILE][PR] packed values
  const uint8_t* src_q;
  const void* src_s;
  const int8_t* src_z;
  int ntile, packrow, kpad, cstep;
  int src_bits;         // blob element bits: 2, 3, 4, 5, 6, 7, 8 (3/5/6/7 in bit planes, bestla_prologue_b.h:512-546)
  uint64_t nel;         // NPad * KPad: plane size of the multi-plane formats
  int raw;              // F8 weights: store the 8-bit code as it is (no + 128 bias)
  int src_e8m0;         // source scales are F8_E8M0 exponents (one byte each) -> fp32 2^e
  // destination geometry (bits: the device layout's 2 / 4 / 8 -- S3 lands in the int4 layout, S5-S7 in int8)
  int bits, n, k, ns, nt, ng, scale_t, kmajor;
  uint32_t* dst_tiles;
  void* dst_scales;
  int8_t* dst_zps;
};

struct SkinnyWeight {
  const void* tiles;
  const void* scales;
  const int8_t* zps;
  const int32_t* shuffle;
  int n, ns, nt, ng, bs;
  int kmajor;         // tile / scale order (woq_layout.h tile_index, scale_row)
  int ldo;
  float* out;
  const float* bias;  // bias[m * bias_ld + n] (bias_ld = 0 broadcasts one row)
  int bias_ld;
  int f4;             // NFloat weight: 0 = F4_BNB, 1 = F4_E2M1, 2 = F4_NF4 (int4 layout, LUT), 3 = F8_E4M3,
                      // 4 = F8_E5M2 (int8 layout, raw codes); -1 = integer weight
};

struct SkinnyArgs {
  const void* A;
  int lda, M, K;
  int nw;               // weights in this launch (1..3); for dual epilogues w[0], w[1] pair up
  int stripe_base[4];   // prefix sums of ns over the weights (non-dual)
  int tiles_per_wave;
  int steps_per_group;  // blocksize / 32
  int scale_t;
  int epi;
  int vec_ok;           // A rows 16-B aligned (vector loads allowed)
  int a_fast;           // vec_ok && no act-order shuffle && K % (16 B / elem) == 0
  const float* res;
  int ld_res;
  float* aux;           // dual epilogue: optional silu/gelu(W0.a) output (tmp1 of the reference FFN)
  int ld_aux;
  SkinnyWeight w[3];
};

struct GemmArgs {
  const void* A;
  int lda, M, K;
  int scale_t;
  int epi;
  int vec_ok;
  const float* res;
  int ld_res;
  const float* aux;
  int ld_aux;
  int stagger;          // gemm3: waves 4-7 half a step behind waves 0-3 (NAD_GEMM3_STAGGER)
  int fold;             // gemm3 / gemm4: group scale folded into the fp16 B fragment (DeviceWeight::fold_ok)
  int ksw;              // gemm4 (folded): waves split over K, 1 (M) x 4 (N) x 2 (K) -- each B fragment dequantized once
  // split-K (gemm3 / gemm4 when the output tiles alone cannot fill the chip): the K tiles are cut into ksplit runs of
  // ktiles (a multiple of the tiles per group); run r of tile b writes its raw fp32 partial to
  // part[(r * M + row) * ldp + n] and launch_splitk_reduce sums the runs in order and applies the epilogue.
  int ksplit;           // 0 / 1: no split
  int ktiles;
  float* part;
  int ldp;
  // FFN prefill with fp16 intermediates: out16 set = the result goes to out16[row * ldo16 + n] as fp16 (RNE) instead of
  // w.out; aux16 set = the SiLU*mul operand is read as fp16 from aux16[row * ld_aux + n]
  _Float16* out16;
  int ldo16;
  const _Float16* aux16;
  int tpg_shift;        // mid-M kernel, one group per K tile or more: log2(K tiles per group) (31: one group)
  int xcd_sg;           // mid-M kernel + its reduce: > 0 = the stripe-group count; the runs of stripe group sg on XCD
                        // sg % 8 (whole rounds of 8 groups), and the reduce workgroups that sum them there too
  int xcd_w;            // ... the stripe group's width in float4 (S stripes x 4)
  // gemm7 without split K: nwt = 2 / 3 weights of one format and K in one launch (fused QKV prefill); the column tiles
  // of weight i follow those of weight i - 1 (nbn_cut: running tile-column counts, nbn_all their total); a.w is weight 0
  int nwt;
  int nbn_cut[2];
  int nbn_all;
  SkinnyWeight wf[2];
  int xcd_tile;         // gemm7 split-K: > 0 = its tile height; XCD x runs every K run of tiles [x T/8, (x+1) T/8) (T tiles,
                        // a multiple of 8), and the reduce workgroups of those tiles run there too
  SkinnyWeight w;
};

// One problem of a batched M = 1 launch (nad_batch_*: BTLAGemmBatchDriver's independent problems, bestla_gemm.cpp:508-624)
struct GemvBatchEnt {
  const void* act;
  const void* tiles;
  const void* scales;
  const int8_t* zps;
  float* out;
  const void* pad[3];  // 64 B per entry (one scalar-cache line)
};

// Persistent stripe-stream decode GEMV (woq_gemv.h).  All weights of one launch share K, group size, scale type and
// symmetry; for the dual epilogues w[0] = gate, w[1] = up.
struct GemvArgs {
  const void* A;
  int lda, M, K;
  int act_t;            // ActType
  int dual;             // units are {w[0] stripe s, w[1] stripe s} pairs (SiLU*mul / GELU*mul)
  int units;            // stripes (non-dual, summed over the weights) or stripe pairs (dual)
  int stripe_base[3];   // non-dual: first virtual stripe of each weight (unused entries = INT_MAX)
  int nt, ng, bs;       // tiles along K, groups along K, group size
  int tpg_shift;        // GPT == 1: log2(tiles per group) (a power of two; 31 for one group), group = t >> shift
  int scale_t;
  int asym;
  int epi;
  int a_fast;           // 16-B aligned rows, K % 8 == 0, no act-order shuffle: vector staging
  const int32_t* shuffle;
  const float* res;
  int ld_res;
  float* aux;
  int ld_aux;
  int part_off;         // LDS byte offset of the partial-sum slots
  uint32_t dq_mask;     // 0x000F000F and 0x64006400: int4 dequant constants, passed in so they stay in registers
  uint32_t dq_magic;
  int u_q, u_r;         // units per workgroup: u_q, one more for the first u_r workgroups (host-divided)
  int lean;             // M = 1 int4 single-group-per-tile launches may take woq_gemv_m1_kernel (NAD_GEMV_LEAN)
  int lean_ks;          // woq_gemv_m1_kernel: K tiles per K-slice (4, or 1 / 2 where that gives each of up to 16 waves one)
  int lean_spw;         // woq_gemv_m1_kernel: K-slices per wave at most (2; 4 for long K; 1 for narrow slices)
  SkinnyWeight w[3];
  const GemvBatchEnt* batch;  // batched M = 1 launch (woq_gemv_m1_kernel<..., BATCH>): problem p = blockIdx / batch_wpp
  int batch_wpp;              //   reads its activations / weight / output from batch[p]; u_q / u_r split one problem
  int m1_nst;                 // woq_gemv_m1_kernel: register stages in flight per wave (0 = by the stages per wave)
  int m1_spec;                // M = 1 launches may take woq_gemv_m1s_kernel (NAD_GEMV_M1_SPEC; 0: always the kernel above)
                              //   + kM1SpecAhead: ... in its load-ahead order where a form exists (NAD_GEMV_AHEAD).
                              //   A host-only bit of this field and not a field of its own: GemvArgs is passed by value
                              //   to woq_gemv_m1_kernel / woq_gemv_kernel / the dual kernel, whose code must not change
};
constexpr int kM1SpecAhead = 2;

// Routed M = 1 launch (woq_gemv_m1_routed_kernel; nad_device_mul_mat_id / nad_device_moe_ffn: ne_mul_mat_id,
// ne_layers.c:7783-7916).  One expert of a bank: 64 B per entry (one scalar-cache line).
struct GemvExpertEnt {
  const void* tiles;
  const void* scales;
  const int8_t* zps;
  const void* pad[5];
};
// What the routed kernel takes beside the GemvArgs of ONE problem of the bank's shape.  Workgroup b serves problem
// p = b / wpp (row r = p / slots, slot i = p % slots) and that problem's share b % wpp of the stripes; the expert is
// ids[r * ids_ld + ids_col + i], read on the device.
struct GemvRouted {
  const GemvExpertEnt* bank[2];  // [0] the weight (gate of a pair), [1] the pair's up weight (dual launches only)
  int n_expert;
  int wpp;               // workgroups per problem; GemvArgs::u_q / u_r split one problem's units over them
  const int32_t* ids;
  int ids_ld, ids_col;
  int slots;             // problems per row (1: nad_device_mul_mat_id, top_k: nad_device_moe_ffn)
  int act_per_slot;      // activation vector of problem p: act + (act_per_slot ? p : r) * act_ld
  const float* act;
  int act_ld;
  float* out;            // output vector of problem p: out + p * out_ld
  int out_ld;
};
// The grid and the threads per workgroup of a launch whose launcher owns them: the launcher takes its dim3s from the
// *_shape function beside it, and a dry run records the same values (capi_internal.h: planned)
struct LaunchShape {
  int grid, block;
};
#pragma GCC visibility push(hidden)  // host helpers: no dynamic symbols
LaunchShape moe_combine_shape(int m, int n);  // one workgroup per 256 columns of a row; launch_moe_gather's too
LaunchShape moe_sort_shape();
LaunchShape cvt_act_shape(int M, int Kp);
#pragma GCC visibility pop
// out[r][n] = ((w[r][0] * y[r * top_k][n]) + w[r][1] * y[r * top_k + 1][n]) + ...: separate fp32 multiplies and adds
// in slot order (ne_mul then ne_add, llama.cpp:676-679)
struct MoeCombineArgs {
  const float* y;   // [m * top_k][ldy]
  int ldy;
  const float* wts;
  int wts_ld;
  int top_k;
  float* out;
  int ldo, m, n;
};
hipError_t launch_moe_combine(const MoeCombineArgs& a, hipStream_t stream);
// softmax -> top_k -> renormalise, one wave per row, n_expert <= 64 (nad_moe_route)
struct MoeRouteArgs {
  const float* logits;
  int ld, m, n_expert, top_k;
  int32_t* ids;
  int ids_ld;
  float* wts;
  int wts_ld;
};
hipError_t launch_moe_route(const MoeRouteArgs& a, hipStream_t stream);
// The gate matmul and the router in one launch (nad_moe_gate_route): logits[r][e] = act[r] . gate[e] in the order the
// header defines, then MoeRouteArgs' arithmetic on them.  One workgroup of 1024 threads per row, dynamic LDS
// [16][n_expert] floats.  k % 4 == 0, lda % 4 == 0, ldw % 4 == 0, act and gate 16-byte aligned (the entry checks).
struct MoeGateRouteArgs {
  const float* act;  // [m][lda]
  int lda;
  const void* gate;  // [n_expert][ldw] of gate_t (ActType)
  int gate_t, ldw;
  int m, k, n_expert, top_k;
  int32_t* ids;
  int ids_ld;
  float* wts;
  int wts_ld;
  float* logits;  // [m][logits_ld], or null
  int logits_ld;
};
#pragma GCC visibility push(hidden)
LaunchShape moe_gate_route_shape(int m);
size_t moe_gate_route_lds(int n_expert);
#pragma GCC visibility pop
hipError_t launch_moe_gate_route(const MoeGateRouteArgs& a, hipStream_t stream);

// Sorted, grouped expert GEMMs (nad_device_moe_ffn_grouped / nad_device_mul_mat_id_grouped).  Problem p = r * top_k + i
// has expert ids[r * ids_ld + i] and is valid when that lies in [0, n_expert).  moe_sort_kernel, one workgroup, writes
// from ids alone (a stable counting sort: ballots and prefix sums, no atomics, so the bytes are a function of ids):
//   offs[0 .. n_expert]  expert e owns the sorted rows offs[e] .. offs[e + 1] - 1; offs[n_expert] = the valid problems
//   perm[q]              the valid problems ordered by (expert, p); -1 from offs[n_expert] on
//   src[q]               perm[q] / top_k, the activation row of sorted row q; 0 from offs[n_expert] on
//   inv[p]               the sorted position of p, -1 for an invalid id
//   tiles[t]             (expert, q0, q1, 0) in expert order, ceil(count_e / bm) per expert, q1 - q0 <= bm
//   ntiles[0]            the tile count, at most np / bm + min(n_expert, np)
struct MoeSortArgs {
  const int32_t* ids;
  int ids_ld, m, top_k, n_expert, bm;
  int32_t *offs, *perm, *src, *inv;
  int4* tiles;
  int32_t* ntiles;
};
hipError_t launch_moe_sort(const MoeSortArgs& a, hipStream_t stream);
// What woq_gemm7_grouped_kernel takes beside the GemmArgs of one expert's GEMM (a.w: the bank's shape and format, its
// pointers unused; a.M unused; whole K)
struct GemmGrouped {
  const GemvExpertEnt* bank;  // [n_expert]
  const int4* tiles;          // MoeSortArgs::tiles
  const int32_t* ntiles;
  const int32_t* rows;        // A row of sorted row q (MoeSortArgs::src), or null: A holds the sorted rows themselves
};
// bits 4 / 2 / 8, bm 32 / 64 / 128 / 256 (anything else: 256), grid = tile bound * ceil(ns / 8).  lds_out set: no launch,
// *lds_out = the dynamic LDS bytes of the instantiation that would serve it (what a dry run records of the launch).
hipError_t launch_gemm7_grouped(const GemmArgs& a, const GemmGrouped& g, int bits, int bm, int grid, const _Float16* A16,
                                int lda16, hipStream_t stream, int* lds_out);
// out[r][n] = ((w[r][0] * y[inv[r * top_k]][n]) + w[r][1] * y[inv[r * top_k + 1]][n]) + ... with moe_combine_kernel's
// arithmetic; a slot with inv < 0 contributes w * 0.0f.  wts null (top_k = 1): out[r] = y[inv[r]], or zeros.
struct MoeGatherArgs {
  const float* y;  // [valid problems][ldy], sorted rows
  int ldy;
  const int32_t* inv;
  const float* wts;
  int wts_ld;
  int top_k;
  float* out;
  int ldo, m, n;
};
hipError_t launch_moe_gather(const MoeGatherArgs& a, hipStream_t stream);

// The arguments of woq_gemv_m1s_kernel: only what that kernel reads, with everything that is constant per launch
// worked out by launch_gemv (K-slices per stripe, units per workgroup).  NWS: weights in the launch (1; 3 = fused QKV;
// 2 = the {gate, up} pair of the SiLU*mul epilogue).
//
// The kernel takes them in two parts.  What the path to the first loads needs comes first, as plain scalar parameters
// of 14 dwords in all, which gfx950 delivers in SGPRs at dispatch (kernarg preload: the wave starts with them instead
// of waiting for a scalar load): A, the tiles / scales pointers of weights 0 and 1, and four dwords
//   a_bytes
//   uqr    u_q | u_r << 16
//   geom   nt | ng << 9 | tpg_shift << 20 | scale_t << 25 | waves << 27
//   ns0    stripes of weight 0 (the pair: of both); the buffer-resource sizes follow from it
// (m1s_packable() in woq_gemv_launch.h holds the field widths).  Everything else is the by-value GemvM1Rest that comes last
// and is read by scalar loads behind the first loads, as before.  GemvM1Args is what the kernel puts the two together
// into: the view its stream and tail work on, never a kernel argument itself.
constexpr int kM1GeomNgShift = 9, kM1GeomTpgShift = 20, kM1GeomScaleShift = 25, kM1GeomWavesShift = 27;
template <int NWS>
struct GemvM1Rest {
  int part_off;         // LDS byte offset of the partial-sum slots
  uint32_t dq_mask, dq_magic;
  int sb1, sb2;         // NWS == 3: first virtual stripe of weights 1 and 2
  int ns[3];            // NWS == 3: stripes of each weight (weights 1 and 2's resource sizes)
  const void* tiles2;   // NWS == 3: weight 2
  const void* scales2;
  const int8_t* zps[NWS];
  int n[NWS];           // output columns (tail)
  float* out[NWS];      // (tail)
  float* aux;           // NWS == 2: optional silu(gate) output (tail)
};
struct GemvM1Weight {
  const void* tiles;
  const void* scales;
  const int8_t* zps;
  int tiles_bytes, scales_bytes, zps_bytes;  // buffer-resource sizes: ns * nt * 1024, ns * ng * 16 * scale size, ns * ng * 16
  int n;                                     // output columns (tail)
  float* out;                                // (tail)
};
template <int NWS>
struct GemvM1Args {
  const void* A;
  int a_bytes;          // K * element size
  int nsl;              // K-slices per stripe
  int u_q, u_r;         // units per workgroup: u_q, one more for the first u_r workgroups
  int nt, ng;
  int tpg_shift;        // one group per tile or coarser: log2(tiles per group)
  int scale_t;
  int nw;               // waves per workgroup
  int part_off;         // LDS byte offset of the partial-sum slots
  uint32_t dq_mask, dq_magic;
  int sb1, sb2;         // NWS == 3: first virtual stripe of weights 1 and 2
  GemvM1Weight w[NWS];
  float* aux;           // NWS == 2: optional silu(gate) output (tail)
};

hipError_t launch_repack(const RepackArgs& a, hipStream_t stream);
hipError_t launch_skinny(const SkinnyArgs& a, int bits, int act_t, int waves_per_wg, int stripes, int ch,
                         hipStream_t stream);
hipError_t launch_gemm(const GemmArgs& a, int bits, int act_t, hipStream_t stream);
// prefill GEMM v2 (woq_gemm2.hip): int4, group = 128 * 2^j, stripe-major; A as fp16 [M][lda16] with K padded to the
// 128-deep tile (zeros), e.g. from launch_cvt_act
hipError_t launch_gemm2(const GemmArgs& a, const _Float16* A16, int lda16, hipStream_t stream);
// prefill GEMM v3 (woq_gemm2.hip): same contract as launch_gemm2; every operand staged by LDS-DMA three 64-deep half
// steps ahead with counted vmcnt (no drain at the barriers)
hipError_t launch_gemm3(const GemmArgs& a, const _Float16* A16, int lda16, hipStream_t stream);
// prefill GEMM v4 (woq_gemm4.hip): gemm3's pipeline for int4 groups of 32 / 64 and int2 groups >= 64.
// gemm4_mode: 0 = not taken, else the group mode; A as for gemm3 with K padded to the weight's K tile (128 / 256)
int gemm4_mode(int bits, int blocksize, int ng, int kpad, bool asym);

// int8-compute mode (woq_i8.hip).  Activation quantizer: one thread per (row, block); any output may be null.
struct QuantU8Args {
  const void* A;
  int lda, M, K, bs, ng;
  const int32_t* shuffle;
  int8_t* aq;           // [M][ldq] s8 = u8 - 128, zero in [K, kp)
  int ldq, kp;
  float2* sa;           // [M][ng] {scale, float(zp) * scale}
  uint8_t* q_u8;        // [M][ldu] the reference's u8 codes
  int ldu;
  float* s_out;         // [M][ld_scale]
  uint8_t* z_out;
  float* red_out;       // sum(q - zp... as kernel_ref: sum of round(x / s)) * s
  int ld_scale;
};
struct I8Args {
  const int8_t* aq;
  int ldq;
  int a_signed;         // 1: Q8_0 activations (s8, sa = {d, 0}; C += float(s32) * d_w * d_a); 0: u8 kblock mode
  const float2* sa;     // [M][ng]
  int M, K;
  const uint16_t* red;  // bf16 reduce [ng][red_ld]
  int red_ld;
  int scale_t;
  int epi;
  const float* res;
  int ld_res;
  const float* aux;
  int ld_aux;
  SkinnyWeight w;
};
// GGUF Q8_0 / Q8_1 activation rows (woq_gguf.hip).  Q8_0: sa = {float(fp16 d), 0}, raw blocks {fp16 d; int8 qs[32]}
// (34 bytes); Q8_1: d kept fp32, sa = {d, float(sum q) * d}, raw blocks {float d; float s; int8 qs[32]} (40 bytes)
struct Q8Args {
  const void* A;
  int lda, M, K;        // K % 32 == 0
  int8_t* aq;           // [M][ldq] s8 codes, zero in [K, kp)
  int ldq, kp;
  float2* sa;           // [M][K/32]
  int8_t* blocks;       // optional raw block rows [M][K/32][34 | 40]
};
// The minimum term of GGUF Q4_1 / Q5_1 (woq_gguf.hip): out[m][n] = epi(out[m][n] + sum_b S[m][b] * mins[n][b]), S the
// block sums of the activations (S null: woq_min_term_kernel sums A itself).  g carries the epilogue operands and the
// output (g.w.out / ldo / n / bias, g.epi, g.res, g.aux) for gemm_epilogue4; mins null = the epilogue alone.
struct MinTermArgs {
  const void* A;
  int lda, M, K;
  int a_vec;            // the rows of A are 16-byte aligned: the block sums may use vector loads (set by the launcher)
  const float* S;       // [M] rows of K/32 sums: S[m * s_ld + b * s_st]
  int s_ld, s_st;
  const uint16_t* mins; // fp16, scale_row() order
  const uint16_t* scales;  // fp16 block scales d, same order: with qbias != 0 the term is S (mins + qbias d)^T, the two
  float qbias;             //   products accumulated one after the other (qbias d is exact in fp32, mins + qbias d is not)
  int ns, ng, kmajor;
  GemmArgs g;
};
constexpr int kMinTermSmallM = 16;          // woq_min_term_kernel: rows it takes ...
constexpr size_t kMinTermSmallLds = 65536;  // ... while M * K/32 floats fit this much LDS
// type: a 32-element GGUF type of woq_gguf.h (2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0); src: n rows of k/32 blocks on
// the device
hipError_t launch_gguf_repack(int type, const uint8_t* src, int n, int k, const DeviceWeight& w, hipStream_t stream);
hipError_t launch_q8_quant(const Q8Args& a, bool q8_1, int act_t, hipStream_t stream);
// block sums of the activation rows into S[m * ng + b] (the pre-pass of launch_min_term_tiled)
hipError_t launch_block_sums(const void* A, int act_t, int lda, int M, int K, float* S, hipStream_t stream);
hipError_t launch_min_term(const MinTermArgs& a, int act_t, hipStream_t stream);        // M <= kMinTermSmallM
hipError_t launch_min_term_tiled(const MinTermArgs& a, hipStream_t stream);            // any M, S given
// GGUF Q6_K (woq_q6k.hip; the layout: woq_layout.h).  src: n rows of k/256 block_q6_K on the device
hipError_t launch_q6k_repack(const uint8_t* src, int n, int k, const DeviceWeight& w, hipStream_t stream);
// (d * sc) * q in fp32, [K][N]
hipError_t launch_q6k_unpack(const DeviceWeight& w, float* out, hipStream_t stream);
// Geometry of a woq_q6k_gemv_kernel launch of m <= 16 rows: activation rows per pass (a pass streams the whole weight
// for the rows whose fp16 staging fits LDS beside the partial-sum slots), passes and LDS bytes; false when not even one
// row fits (K > 65536 / 2 for fp32 / bf16 rows)
struct Q6kGemvGeom {
  int rows_pp, passes, grid, waves;
  size_t lds;
};
bool q6k_gemv_geometry(int m, int k, int ns, int act_t, int cus, Q6kGemvGeom* g);
// a: A / lda / M / K, the epilogue operands and a.w (tiles = quants, zps = sub-scales, scales = d, nt = superblocks)
hipError_t launch_q6k_gemv(const GemmArgs& a, int act_t, const Q6kGemvGeom& g, hipStream_t stream);
hipError_t launch_q6k_gemm(const GemmArgs& a, int act_t, hipStream_t stream);  // grid: ceil(M / 128) * ceil(ns / 8)
// Geometry of a woq_q6k_gemv_routed_kernel launch of nprob one-row problems: wpp = max(1, min(ns, cus / nprob))
// workgroups per problem, grid = nprob * wpp, lds = 4 K (the hi and lo fp16 rows) + the 32 KiB of partials; false when
// the two rows do not fit LDS (K > 32768) or the grid reaches 2^31
struct Q6kRoutedGeom {
  int wpp, grid, waves;
  size_t lds;
};
bool q6k_routed_geometry(int k, int ns, int64_t nprob, int cus, Q6kRoutedGeom* g);
// a: M = 1, K, the epilogue kind (none, SiLU / GELU, or kEpiSiluMul with aux_out: times the problem's own output row,
// in place) and a.w -- the bank's shape; the kernel takes each problem's pointers from r (r.wpp = g.wpp)
hipError_t launch_q6k_gemv_routed(const GemmArgs& a, const GemvRouted& r, bool aux_out, const Q6kRoutedGeom& g,
                                  hipStream_t stream);
// woq_q6k_gemm_grouped_kernel: a.A / a.lda the fp16 rows (gathered through gg.rows, or the sorted rows themselves), the
// outputs by sorted row (a.out16 / a.aux16 / a.w.out); 128-row tiles, grid = tile bound * ceil(ns / 8), 512 threads
hipError_t launch_q6k_gemm_grouped(const GemmArgs& a, const GemmGrouped& gg, int grid, hipStream_t stream);
// quantize_row_q8_K_reference: act [m][lda] -> m rows of k/256 block_q8_K (292 bytes); k % 256 == 0
hipError_t launch_q8_k_quant(const void* A, int act_t, int lda, int m, int k, void* blocks, hipStream_t stream);
// Geometry of a woq_q6k_i8_kernel launch (the Q8_K integer arithmetic, any m): rows per pass (at most 16, fewer where
// their codes and block sums do not fit LDS), the row sets of four a pass works on (1, 2 or 4), passes (grid.y) and LDS
// bytes; false
// when not even one row fits
struct Q6kI8Geom {
  int rows_pp, rs_pp, passes, grid, waves;
  size_t lds;
};
bool q6k_i8_geometry(int m, int k, int ns, int cus, Q6kI8Geom* g);
hipError_t launch_q6k_i8(const GemmArgs& a, int act_t, const Q6kI8Geom& g, hipStream_t stream);
hipError_t launch_quant_u8(const QuantU8Args& a, int act_t, hipStream_t stream);
hipError_t launch_i8(const I8Args& a, int bits, hipStream_t stream);
hipError_t launch_gemm4(const GemmArgs& a, int bits, const _Float16* A16, int lda16, hipStream_t stream);
// prefill GEMM v7 (woq_gemm7.hip, the default for int4 groups of 128 * 2^j): gemm3's contract (256 x 128 tiles,
// split-K partials, fp16 A padded to the 128-deep tile) with the group scale folded (needs DeviceWeight::fold_ok)
bool gemm7_ok(int bits, int blocksize, int fold_ok);
hipError_t launch_gemm7(const GemmArgs& a, int bits, int bm, const _Float16* A16, int lda16, hipStream_t stream);
// mid-M GEMM (woq_gemm_mid.hip, 17 <= M <= 64): int4 / int2, gpt groups per K tile (1, 2, 4), rf = ceil(M / 16) row
// fragments; grid = ceil(ns / S) * a.ksplit for the S of mid_geometry; a.ksplit > 1: launch_splitk_reduce follows
void mid_geometry(int bits, int gpt, int act_t, int rf, int wide, int* s, int* nw, int* spw);
int mid_lds_bytes(int rf, int s, int nw);
hipError_t launch_gemm_mid(const GemmArgs& a, int bits, int gpt, int act_t, int rf, int s, int grid, hipStream_t stream);
// sum a.ksplit partials of a split-K gemm3 / gemm4 launch in run order and apply a.epi into a.w.out (woq_gemm2.hip)
hipError_t launch_splitk_reduce(const GemmArgs& a, hipStream_t stream);
hipError_t launch_cvt_act(const void* A, int act_t, int lda, int M, int K, int Kp, const int32_t* shuffle,
                          _Float16* out, hipStream_t stream);
// groups per K tile the GEMV handles (1, 2, 4, 8) for this geometry, 0 if unsupported; *tpg = tiles per group
int gemv_groups_per_tile(int bits, int nt, int ng, int bs, int* tpg);
size_t gemv_lds_layout(GemvArgs& a, int bits, int waves, int grid);
int gemv_waves(int bits, int nt, int ng, int bs);
// M = 1: K-slices of 2 tiles for woq_gemv_m1_kernel when that gives more waves (one slice each); sets a.lean_ks and
// *waves when taken (ks_pref = NAD_GEMV_KS: 2 = 1- or 2-tile slices wherever that gives more waves, 3 = 2-tile only,
// 4 = never)
void gemv_lean_slices(GemvArgs& a, int bits, int* waves, int ks_pref);
hipError_t launch_gemv(const GemvArgs& a, int bits, int waves, int grid, size_t lds, hipStream_t stream);
// What launch_gemv, launch_gemv_batch and launch_gemv_routed hand on to, each defined in the object that holds the
// instantiations it reaches (woq_gemv.o itself: woq_gemv_kernel, the int4 woq_gemv_m1_kernel, woq_gemv_m1_dual_kernel):
//   woq_gemv_b2.o   the int2 woq_gemv_m1_kernel
hipError_t gemv_m1_launch_b2(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st);
//   woq_gemv_s2.o / _s3.o   the int4 / int2 woq_gemv_m1s_kernel.  false: no instantiation serves the launch, nothing
//   was issued and e is untouched; true: the launch was issued (in a dry run: named), e is its status
bool gemv_m1s_launch_b4(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e);
bool gemv_m1s_launch_b2(const GemvArgs& a, int gpt, dim3 g, dim3 b, size_t lds, hipStream_t st, hipError_t& e);
//   woq_gemv_s6.o   woq_gemv_m1s_kernel's load-ahead forms (form 1 / 2 / 3: m1s_ahead_form, woq_gemv_launch.h)
hipError_t gemv_m1s_ahead_launch(const GemvArgs& a, int form, dim3 g, dim3 b, size_t lds, hipStream_t st);
//   woq_gemv_r5.o   the int2 woq_gemv_m1_routed_kernel (woq_gemv_r4.o: launch_gemv_routed with the int4 ones;
//   woq_gemv_r7.o: launch_gemv_routed_general with woq_gemv_routed_kernel)
hipError_t gemv_routed_launch_b2(const GemvArgs& a, const GemvRouted& r, int gpt, dim3 g, dim3 b, size_t lds,
                                 hipStream_t st);
// Dry runs (nad_plan_*): between gemv_name_begin() and gemv_name_end() on the calling thread launch_gemv and
// launch_gemv_batch run as always up to the launch itself, which records its kernel's template arguments instead of
// being issued -- the name comes from the statement that would have launched.  gemv_name_end() returns the record of the
// last such launch (gemv_inst below), 0 if there was none.
void gemv_name_begin();
uint32_t gemv_name_end();
bool gemv_named(uint32_t inst);  // the launch statements of woq_gemv_launch.h: true (and inst recorded) while naming
// family 1 woq_gemv_kernel (at = HILO; ksn, spw, st, nwt, nsc: 0 / -1), 2 woq_gemv_m1_kernel, 3 woq_gemv_m1s_kernel;
// bits, gpt in {1, 2, 4, 8}; st -1..2; nsc in {0, 7, 11, 16}
constexpr uint32_t gemv_inst(int family, int bits, int gpt, bool asym, int at, int ksn, int spw, int nst, int st,
                             bool batch, int nwt, int nsc, bool ahead) {
  const auto lg = [](int v) { return uint32_t(v >= 8 ? 3 : (v >= 4 ? 2 : (v >= 2 ? 1 : 0))); };
  return uint32_t(family) | lg(bits) << 2 | lg(gpt) << 4 | uint32_t(asym) << 6 | uint32_t(at) << 7 |
         uint32_t(ksn) << 9 | uint32_t(spw) << 12 | uint32_t(nst) << 15 | uint32_t(st + 1) << 17 |
         uint32_t(batch) << 19 | uint32_t(nwt) << 20 | uint32_t(nsc == 16 ? 3 : (nsc == 11 ? 2 : nsc == 7)) << 22 |
         uint32_t(ahead) << 24;
}
constexpr int kPlanGemvInstShift = 4;  // the record's place in the plan's flag word (o[4] of nad_plan_*)
// whether launch_gemv would take woq_gemv_m1_kernel for these arguments
bool gemv_uses_m1(const GemvArgs& a, int bits, int waves);
// two M = 1 launches of different formats as one (int2 a + int4 b at groups of 64 or 128, fp32 activations, sym,
// 16 waves each; a on workgroups [0, ga), b on [ga, ga + gb))
bool gemv_dual_ok(const GemvArgs& a, int bits_a, const GemvArgs& b, int bits_b, int waves);
hipError_t launch_gemv_dual(const GemvArgs& a, const GemvArgs& b, int ga, int gb, int waves, size_t lds,
                            hipStream_t stream);
// the batched M = 1 launch (requires gemv_uses_m1; grid = problems * a.batch_wpp)
hipError_t launch_gemv_batch(const GemvArgs& a, int bits, int waves, int grid, size_t lds, hipStream_t stream);
// the routed M = 1 launch (requires gemv_uses_m1 and fp32 activations; grid = problems * r.wpp)
hipError_t launch_gemv_routed(const GemvArgs& a, const GemvRouted& r, int bits, int waves, int grid, size_t lds,
                              hipStream_t stream);
// the routed stripe-stream launch (woq_gemv_routed_kernel: M = 1, fp32 activations, gemv_uses_m1 false; int4 groups of
// 32 sym, int8 groups of 32 / 64 * 2^j / one per channel; grid = problems * r.wpp)
hipError_t launch_gemv_routed_general(const GemvArgs& a, const GemvRouted& r, int bits, int waves, int grid, size_t lds,
                                      hipStream_t stream);

}  // namespace nad
