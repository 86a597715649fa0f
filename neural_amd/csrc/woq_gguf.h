// woq_gguf.h -- what each GGUF block type is, one row per type.  Host and device code read the same rows: the loaders
// (capi_load.hip), the compute mode (capi.hip) and the repack kernel (woq_gguf.hip) derive everything from them, so a
// new type is a new row (and, for a new layout, a kernel).
#pragma once
#include <cstdint>

namespace nad {

// DeviceWeight::src_core_id of a GGUF matrix: "\0GGUF" and the type's three characters
constexpr uint64_t kGgufQ4_0 = 0x3054344655474700ull;  // "\0GGUF4Q0"
constexpr uint64_t kGgufQ4_1 = 0x3154344655474700ull;  // "\0GGUF4Q1"
constexpr uint64_t kGgufQ5_0 = 0x3054354655474700ull;  // "\0GGUF5Q0"
constexpr uint64_t kGgufQ5_1 = 0x3154354655474700ull;  // "\0GGUF5Q1"
constexpr uint64_t kGgufQ8_0 = 0x3054384655474700ull;  // "\0GGUF8Q0"
constexpr uint64_t kGgufQ6_K = 0x4b51364655474700ull;  // "\0GGUF6QK"

struct GgufType {
  int id;  // the file's type number (NAD_GGUF_*)
  const char* name;
  int block_elems, block_bytes;
  int bits;         // device layout: 4 / 8 the symmetric tile layouts of woq_layout.h, 6 Q6_K's own
  int code_zero;    // the stored code that decodes to 0 (Q4_0: 8, Q5_0: 16; Q8_0's codes are signed)
  float qmax;       // largest |decoded value| before the scale: the bound of the fold rule (0: the type never folds)
  bool has_min;     // blocks carry an fp16 minimum behind d (the descriptor's mins region)
  int min_bias;     // with a minimum: the layout decodes q - min_bias (DeviceWeight::min_bias)
  uint64_t tag;     // DeviceWeight::src_core_id
  int act_quant;    // activation rows of the int8 arithmetic (vec_dot_type, ne_layers.c:266-318): 0 none (Q6_K has its
                    // own Q8_K mode), 1 Q8_0, 2 Q8_1
};

constexpr GgufType kGgufTypes[] = {
    {2, "Q4_0", 32, 18, 4, 8, 8.f, false, 0, kGgufQ4_0, 1},     // (nibble - 8) d
    {3, "Q4_1", 32, 20, 4, 0, 8.f, true, 8, kGgufQ4_1, 2},      // q d + m: the nibble holds q, the layout decodes q - 8
    {6, "Q5_0", 32, 22, 8, 16, 16.f, false, 0, kGgufQ5_0, 1},   // (q - 16) d
    {7, "Q5_1", 32, 24, 8, 0, 31.f, true, 0, kGgufQ5_1, 2},     // q d + m
    {8, "Q8_0", 32, 34, 8, 0, 128.f, false, 0, kGgufQ8_0, 1},   // q d, q signed
    {14, "Q6_K", 256, 210, 6, 32, 0.f, false, 0, kGgufQ6_K, 0},  // superblocks: d sc (q - 32), folded by its own GEMM
};

// the row of a GGUF type number / of a loaded weight's src_core_id; null for anything else
constexpr const GgufType* gguf_type_by_id(int id) {
  for (const GgufType& t : kGgufTypes)
    if (t.id == id) return &t;
  return nullptr;
}
constexpr const GgufType* gguf_type_by_tag(uint64_t tag) {
  for (const GgufType& t : kGgufTypes)
    if (t.tag == tag) return &t;
  return nullptr;
}

}  // namespace nad
