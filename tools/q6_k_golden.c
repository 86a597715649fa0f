// Golden vectors for GGUF Q6_K from the reference's own code: it includes Neural Speed's core/data_types.h and
// vectors/cpu/quantize.h by path and holds none of their text.  Not built by make or build(): run once, its DATA is
// committed under tests/golden/q6_k (manifest.txt + .bin, read by tests.oracle_lib.load_ref_golden("q6_k")).
//
//   gcc -std=gnu11 -O2 -ffp-contract=off -DNDEBUG -I <reference>/neural_speed -o q6_k_golden tools/q6_k_golden.c -lm \
//       && ./q6_k_golden tests/golden/q6_k
//
// Cases (each stores the block bytes "q6_k", dequantize_row_q6_K's output "deq" and meta = {n, k}):
//   n40_k256      quantize_row_q6_K_reference of uniform +-1 weights; row 1 all zero, one outlier in row 2
//   n16_k768      the same at three superblocks, amplitude 0.05
//   ext_n16_k512  block fields written by hand: q = -32 and 31, sc = -128, 127 and 0, a d = 0 block, a subnormal fp16
//                 d, random bytes elsewhere
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "core/data_types.h"
#include "vectors/cpu/quantize.h"

static const char* g_dir;
static FILE* g_man;

static void dump(const char* cs, const char* name, const char* dt, const void* p, size_t esz, size_t n) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s.%s.bin", g_dir, cs, name);
  FILE* f = fopen(path, "wb");
  fwrite(p, esz, n, f);
  fclose(f);
  fprintf(g_man, "%s %s %s %zu\n", cs, name, dt, n);
}

static uint32_t g_state = 20261019u;
static uint32_t rnd(void) {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return g_state;
}
static float urand(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xFFFFFF) / 16777216.f; }

static void finish(const char* cs, int n, int k, const block_q6_K* Q) {
  const int nb = k / QK_K;
  float* D = malloc(sizeof(float) * n * k);
  for (int r = 0; r < n; r++) dequantize_row_q6_K(Q + (size_t)r * nb, D + (size_t)r * k, k);
  int meta[2] = {n, k};
  dump(cs, "meta", "i4", meta, 4, 2);
  dump(cs, "q6_k", "u1", Q, 1, sizeof(block_q6_K) * n * nb);
  dump(cs, "deq", "f4", D, 4, (size_t)n * k);
  free(D);
}

static void quantized_case(const char* cs, int n, int k, float amp) {
  float* W = malloc(sizeof(float) * n * k);
  for (int i = 0; i < n * k; i++) W[i] = urand(-amp, amp);
  for (int j = 0; j < k && n > 1; j++) W[k + j] = 0.f;  // row 1: all zero (d = 0, the memset branch)
  if (n > 2) W[2 * k + 5] = 40.f * amp;                 // row 2: one outlier
  const int nb = k / QK_K;
  block_q6_K* Q = malloc(sizeof(block_q6_K) * n * nb);
  for (int r = 0; r < n; r++) quantize_row_q6_K_reference(W + (size_t)r * k, Q + (size_t)r * nb, k);
  finish(cs, n, k, Q);
  free(W);
  free(Q);
}

// element e of a superblock takes the 6-bit value v (q + 32): the inverse of dequantize_row_q6_K's reads
static void set_v(block_q6_K* b, int e, int v) {
  const int h = e / 128, j = (e % 128) / 32, l = e % 32;
  uint8_t* ql = &b->ql[64 * h + 32 * (j & 1) + l];
  *ql = j < 2 ? (uint8_t)((*ql & 0xF0) | (v & 15)) : (uint8_t)((*ql & 0x0F) | ((v & 15) << 4));
  uint8_t* qh = &b->qh[32 * h + l];
  *qh = (uint8_t)((*qh & ~(3 << (2 * j))) | ((v >> 4) << (2 * j)));
}

static void ext_case(const char* cs, int n, int k) {
  const int nb = k / QK_K;
  block_q6_K* Q = malloc(sizeof(block_q6_K) * n * nb);
  for (int i = 0; i < n * nb; i++) {
    uint8_t* p = (uint8_t*)&Q[i];
    for (size_t j = 0; j < sizeof(block_q6_K) - 2; j++) p[j] = (uint8_t)rnd();  // any bytes are valid quants / scales
    Q[i].d = NE_FP32_TO_FP16(urand(1e-4f, 1e-2f));
  }
  // row 0, block 0: sc = 127 over q = 31 and -32 (|sc q| = 4064 / 4096: past fp16's exact integers), sc = -128, sc = 0
  for (int e = 0; e < 16; e++) set_v(&Q[0], e, e & 1 ? 63 : 0);
  Q[0].scales[0] = 127;
  for (int e = 16; e < 32; e++) set_v(&Q[0], e, e & 1 ? 0 : 63);
  Q[0].scales[1] = -128;
  Q[0].scales[2] = 0;
  for (int e = 240; e < 256; e++) set_v(&Q[0], e, 63);  // the last group, all q = 31, sc = 127
  Q[0].scales[15] = 127;
  // row 1: every sub-scale at an extreme, alternating
  for (int b = 0; b < nb; b++)
    for (int g = 0; g < 16; g++) Q[1 * nb + b].scales[g] = (g + b) & 1 ? 127 : -128;
  // row 2, block 1: d = 0; row 3, block 0: the smallest fp16 subnormal; row 3, block 1: a larger subnormal, negative
  Q[2 * nb + 1].d = NE_FP32_TO_FP16(0.f);
  {
    const uint16_t sub1 = 0x0001, sub2 = 0x8155;
    memcpy(&Q[3 * nb + 0].d, &sub1, 2);
    memcpy(&Q[3 * nb + 1].d, &sub2, 2);
  }
  // row 4: all q = -32 with sc = -128 in block 0, all q = 31 with sc = 127 in block 1
  for (int e = 0; e < 256; e++) {
    set_v(&Q[4 * nb + 0], e, 0);
    set_v(&Q[4 * nb + 1], e, 63);
  }
  for (int g = 0; g < 16; g++) {
    Q[4 * nb + 0].scales[g] = -128;
    Q[4 * nb + 1].scales[g] = 127;
  }
  finish(cs, n, k, Q);
  free(Q);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 0; i < (1 << 16); ++i) {  // ne_init's fp16 -> fp32 table: without it every d reads 0
    uint16_t ui = (uint16_t)i;
    ne_fp16_t ii;
    memcpy(&ii, &ui, sizeof(ii));
    table_f32_f16[i] = NE_COMPUTE_FP16_TO_FP32(ii);
  }
  g_dir = argv[1];
  char path[1024];
  snprintf(path, sizeof(path), "%s/manifest.txt", g_dir);
  g_man = fopen(path, "w");
  if (!g_man) return 3;
  quantized_case("n40_k256", 40, 256, 1.f);
  quantized_case("n16_k768", 16, 768, 0.05f);
  ext_case("ext_n16_k512", 16, 512);
  fclose(g_man);
  return 0;
}
