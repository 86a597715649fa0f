// Golden vectors for GGUF Q6_K in the reference's Q8_K integer arithmetic, from the reference's own code: it includes
// Neural Speed's core/data_types.h, vectors/cpu/quantize.h and core/layers/vec_dot.h by path and holds none of their
// text.  Not built by make or build(): run once, its DATA is committed under tests/golden/q6_k_q8_k (manifest.txt +
// .bin, read by tests.oracle_lib.load_ref_golden("q6_k_q8_k")).  Compiled at the baseline ISA, so quantize_row_q8_K
// and ggml_vec_dot_q6_K_q8_K take their scalar branches:
//
//   gcc -std=gnu11 -O2 -ffp-contract=off -DNDEBUG -I <reference>/neural_speed -o q6_k_q8_k_golden \
//       tools/q6_k_q8_k_golden.c -lm && ./q6_k_q8_k_golden tests/golden/q6_k_q8_k
//
// quant_* cases store meta = {m, k}, the fp32 rows "x" and quantize_row_q8_K_reference's block_q8_K bytes "q8_k"
// (the output buffer zero-initialised: the reference leaves the bsums of an all-zero superblock unwritten):
//   quant_uniform_k256 / _k768   uniform +-1 rows
//   quant_zero_sb                k = 768, the middle superblock of row 0 and all of row 1 zero
//   quant_plus_first             +a precedes -a at the same largest magnitude (max = +a; -a clamps at 127)
//   quant_minus_first            -a precedes +a (max = -a; +a clamps at 127)
//   quant_ties                   max = -128, so iscale = 1, and every other element at n + 0.5: ties to even
//   quant_amp_1em3 / _1e3        uniform rows of amplitude 1e-3 and 1e3
// dot_* cases store meta = {n, k, m}, the Q6_K blocks "q6_k" (quantize_row_q6_K_reference of uniform weights, some
// rows overwritten with extreme fields written by hand as in tools/q6_k_golden.c's ext case), the fp32 activations
// "x", their block_q8_K bytes "q8_k" and y[m][n] from ggml_vec_dot_q6_K_q8_K:
//   dot_n40_k256_m5, dot_n16_k768_m3
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "core/data_types.h"
#include "vectors/cpu/quantize.h"
#include "core/layers/vec_dot.h"

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

static block_q8_K* quant_rows(const float* X, int m, int k) {
  const int nb = k / QK_K;
  block_q8_K* Y = calloc((size_t)m * nb, sizeof(block_q8_K));
  for (int r = 0; r < m; r++) quantize_row_q8_K_reference(X + (size_t)r * k, Y + (size_t)r * nb, k);
  return Y;
}

static void quant_case(const char* cs, const float* X, int m, int k) {
  block_q8_K* Y = quant_rows(X, m, k);
  int meta[2] = {m, k};
  dump(cs, "meta", "i4", meta, 4, 2);
  dump(cs, "x", "f4", X, 4, (size_t)m * k);
  dump(cs, "q8_k", "u1", Y, 1, sizeof(block_q8_K) * m * (k / QK_K));
  free(Y);
}

static float* uniform(int m, int k, float amp) {
  float* X = malloc(sizeof(float) * m * k);
  for (int i = 0; i < m * k; i++) X[i] = urand(-amp, amp);
  return X;
}

// element e of a superblock takes the 6-bit value v (q + 32): the inverse of dequantize_row_q6_K's reads
static void set_v(block_q6_K* b, int e, int v) {
  const int h = e / 128, j = (e % 128) / 32, l = e % 32;
  uint8_t* ql = &b->ql[64 * h + 32 * (j & 1) + l];
  *ql = j < 2 ? (uint8_t)((*ql & 0xF0) | (v & 15)) : (uint8_t)((*ql & 0x0F) | ((v & 15) << 4));
  uint8_t* qh = &b->qh[32 * h + l];
  *qh = (uint8_t)((*qh & ~(3 << (2 * j))) | ((v >> 4) << (2 * j)));
}

static void dot_case(const char* cs, int n, int k, int m) {
  const int nb = k / QK_K;
  float* W = uniform(n, k, 1.f);
  block_q6_K* Q = malloc(sizeof(block_q6_K) * n * nb);
  for (int r = 0; r < n; r++) quantize_row_q6_K_reference(W + (size_t)r * k, Q + (size_t)r * nb, k);
  // row 0, block 0: sc = 127 over q = 31 and -32, sc = -128, sc = 0, the last group all q = 31 under sc = 127
  for (int e = 0; e < 16; e++) set_v(&Q[0], e, e & 1 ? 63 : 0);
  Q[0].scales[0] = 127;
  for (int e = 16; e < 32; e++) set_v(&Q[0], e, e & 1 ? 0 : 63);
  Q[0].scales[1] = -128;
  Q[0].scales[2] = 0;
  for (int e = 240; e < 256; e++) set_v(&Q[0], e, 63);
  Q[0].scales[15] = 127;
  // row 1: every sub-scale at an extreme, alternating
  for (int b = 0; b < nb; b++)
    for (int g = 0; g < 16; g++) Q[1 * nb + b].scales[g] = (g + b) & 1 ? 127 : -128;
  // row 4: all q = -32 with sc = -128 in block 0, all q = 31 with sc = 127 in the last block
  for (int e = 0; e < 256; e++) set_v(&Q[4 * nb + 0], e, 0);
  for (int g = 0; g < 16; g++) Q[4 * nb + 0].scales[g] = -128;
  if (nb > 1) {
    for (int e = 0; e < 256; e++) set_v(&Q[4 * nb + nb - 1], e, 63);
    for (int g = 0; g < 16; g++) Q[4 * nb + nb - 1].scales[g] = 127;
    Q[2 * nb + 1].d = NE_FP32_TO_FP16(0.f);  // row 2, block 1: d = 0
  }
  float* X = uniform(m, k, 1.f);
  for (int j = 0; j < QK_K; j++) X[j] = X[j] < 0 ? -1.f : 1.f;  // row 0, block 0: every code -128 or 127
  block_q8_K* Y = quant_rows(X, m, k);
  float* out = malloc(sizeof(float) * m * n);
  for (int r = 0; r < m; r++)
    for (int c = 0; c < n; c++)
      ggml_vec_dot_q6_K_q8_K(k, &out[(size_t)r * n + c], Q + (size_t)c * nb, Y + (size_t)r * nb);
  int meta[3] = {n, k, m};
  dump(cs, "meta", "i4", meta, 4, 3);
  dump(cs, "q6_k", "u1", Q, 1, sizeof(block_q6_K) * n * nb);
  dump(cs, "x", "f4", X, 4, (size_t)m * k);
  dump(cs, "q8_k", "u1", Y, 1, sizeof(block_q8_K) * m * nb);
  dump(cs, "y", "f4", out, 4, (size_t)m * n);
  free(W);
  free(Q);
  free(X);
  free(Y);
  free(out);
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

  float* X = uniform(3, 256, 1.f);
  quant_case("quant_uniform_k256", X, 3, 256);
  free(X);
  X = uniform(2, 768, 1.f);
  quant_case("quant_uniform_k768", X, 2, 768);
  free(X);

  X = uniform(2, 768, 1.f);
  for (int j = 256; j < 512; j++) X[j] = 0.f;
  for (int j = 0; j < 768; j++) X[768 + j] = 0.f;
  quant_case("quant_zero_sb", X, 2, 768);
  free(X);

  X = uniform(2, 256, 0.9f * 0.37f);
  X[17] = 0.37f, X[101] = -0.37f;
  X[256 + 200] = 0.37f, X[256 + 255] = -0.37f;
  quant_case("quant_plus_first", X, 2, 256);
  X[17] = -0.37f, X[101] = 0.37f;
  X[256 + 200] = -0.37f, X[256 + 255] = 0.37f;
  quant_case("quant_minus_first", X, 2, 256);
  free(X);

  X = malloc(sizeof(float) * 2 * 256);
  for (int j = 0; j < 256; j++) {
    X[j] = (float)(j % 127) + 0.5f;             // 0.5 .. 126.5: every tie of the positive range
    X[256 + j] = -((float)(j % 128) + 0.5f);    // -0.5 .. -127.5
  }
  X[3] = -128.f;       // max = -128: iscale = 1
  X[256 + 250] = -128.f;
  quant_case("quant_ties", X, 2, 256);
  free(X);

  X = uniform(2, 512, 1e-3f);
  quant_case("quant_amp_1em3", X, 2, 512);
  free(X);
  X = uniform(2, 512, 1e3f);
  quant_case("quant_amp_1e3", X, 2, 512);
  free(X);

  dot_case("dot_n40_k256_m5", 40, 256, 5);
  dot_case("dot_n16_k768_m3", 16, 768, 3);
  fclose(g_man);
  return 0;
}
