// Golden vectors for the GGUF Q4_1 / Q5_0 / Q5_1 / Q8_0 paths from the reference's own code: it includes Neural Speed's
// core/data_types.h, vectors/cpu/quantize.h and core/layers/vec_dot.h by path (their scalar paths, host baseline ISA)
// and holds none of their text.  Not built by make or build(): run once, its DATA is committed under
// tests/golden/gguf_types (manifest.txt + .bin, read by tests.oracle_lib.load_ref_golden("gguf_types")).
//
//   gcc -std=gnu11 -O2 -ffp-contract=off -DNDEBUG -I <reference>/neural_speed -o gguf_types_golden \
//       tools/gguf_types_golden.c -lm && ./gguf_types_golden tests/golden/gguf_types
//
// -DNDEBUG: the vec_dot functions assert an even block count for their two-block SIMD loops; the scalar loops compiled
// here take any count, and the k = 96 cases have three blocks.
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

typedef void (*quant_fn)(const float*, void*, int);
typedef void (*dequant_fn)(const void*, float*, int);
typedef void (*dot_fn)(const int, float*, const void*, const void*);

static void dq4_1(const void* x, float* y, int k) { dequantize_row_q4_1((const block_q4_1*)x, y, k); }
static void dq5_0(const void* x, float* y, int k) { dequantize_row_q5_0((const block_q5_0*)x, y, k); }
static void dq5_1(const void* x, float* y, int k) { dequantize_row_q5_1((const block_q5_1*)x, y, k); }
static void dq8_0(const void* x, float* y, int k) { dequantize_row_q8_0(x, y, k); }
static void qa8_0(const float* x, void* y, int k) { quantize_row_q8_0_reference(x, (block_q8_0*)y, k); }
static void qa8_1(const float* x, void* y, int k) { quantize_row_q8_1_reference(x, (block_q8_1*)y, k); }

// wname / aname: the manifest names of the weight and activation blocks; off: every weight shifted by it, so that the
// min formats get mins of the size of d * qmax
static void one_case(const char* cs, int n, int k, int m, float amp, float off, const char* wname, size_t wblk,
                     quant_fn qw, dequant_fn dqw, const char* aname, size_t ablk, quant_fn qa, dot_fn dot) {
  float* W = malloc(sizeof(float) * n * k);
  for (int i = 0; i < n * k; i++) W[i] = off + urand(-amp, amp);
  for (int j = 0; j < k && n > 1; j++) W[k + j] = 0.f;  // row 1: all zero (d = 0)
  if (n > 2) W[2 * k + 5] = 40.f * amp;                 // row 2: one outlier
  const int nb = k / 32;
  char* Q = malloc(wblk * n * nb);
  float* D = malloc(sizeof(float) * n * k);
  for (int r = 0; r < n; r++) {
    qw(W + (size_t)r * k, Q + wblk * r * nb, k);
    dqw(Q + wblk * r * nb, D + (size_t)r * k, k);
  }
  float* A = malloc(sizeof(float) * m * k);
  for (int i = 0; i < m * k; i++) A[i] = urand(-1.f, 1.f);
  char* Y = malloc(ablk * m * nb);
  float* C = malloc(sizeof(float) * m * n);
  for (int i = 0; i < m; i++) {
    qa(A + (size_t)i * k, Y + ablk * i * nb, k);
    for (int r = 0; r < n; r++) dot(k, C + (size_t)i * n + r, Q + wblk * r * nb, Y + ablk * i * nb);
  }
  int meta[3] = {n, k, m};
  dump(cs, "meta", "i4", meta, 4, 3);
  dump(cs, wname, "u1", Q, 1, wblk * n * nb);
  dump(cs, "deq", "f4", D, 4, (size_t)n * k);
  dump(cs, "A", "f4", A, 4, (size_t)m * k);
  dump(cs, aname, "u1", Y, 1, ablk * m * nb);
  dump(cs, "C", "f4", C, 4, (size_t)m * n);
  free(W);
  free(Q);
  free(D);
  free(A);
  free(Y);
  free(C);
}

static void both(const char* type, float off, size_t wblk, quant_fn qw, dequant_fn dqw, const char* aname, size_t ablk,
                 quant_fn qa, dot_fn dot) {
  char cs[64];
  snprintf(cs, sizeof(cs), "%s_n40_k256", type);
  one_case(cs, 40, 256, 3, 1.f, off, type, wblk, qw, dqw, aname, ablk, qa, dot);
  snprintf(cs, sizeof(cs), "%s_n16_k96", type);
  one_case(cs, 16, 96, 2, 0.05f, off * 0.05f, type, wblk, qw, dqw, aname, ablk, qa, dot);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 0; i < (1 << 16); ++i) {  // ne_init's fp16 -> fp32 table
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
  both("q4_1", 1.5f, sizeof(block_q4_1), quantize_row_q4_1, dq4_1, "y_q8_1", sizeof(block_q8_1), qa8_1,
       ne_vec_dot_q4_1_q8_1);
  both("q5_0", 0.f, sizeof(block_q5_0), quantize_row_q5_0, dq5_0, "y_q8_0", sizeof(block_q8_0), qa8_0,
       ne_vec_dot_q5_0_q8_0);
  both("q5_1", 1.5f, sizeof(block_q5_1), quantize_row_q5_1, dq5_1, "y_q8_1", sizeof(block_q8_1), qa8_1,
       ne_vec_dot_q5_1_q8_1);
  both("q8_0", 0.f, sizeof(block_q8_0), qa8_0, dq8_0, "y_q8_0", sizeof(block_q8_0), qa8_0,
       ne_vec_dot_q8_0_q8_0);
  fclose(g_man);
  return 0;
}
