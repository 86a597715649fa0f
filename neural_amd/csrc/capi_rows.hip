// capi_rows.hip -- ne_get_rows on a device weight (include/neural_amd.h): nad_device_get_rows (its dry run,
// nad_plan_get_rows, is in capi_plan.hip).
#include <climits>

#include "capi_internal.h"
#include "woq_rows.h"

using namespace nad;

// the checks in the order the header states them, the geometry, then the launch or its record.  The weight may be
// geometry-only (any_weight: as_weight refuses that outside a dry run; here the argument checks come first and the
// launch is refused below)
int get_rows(const char* who, const void* devstor, const int32_t* ids, int ids_stride, int m, void* out, int out_dtype,
             int ldo, hipStream_t st) {
  const DeviceWeight* w = any_weight(who, devstor);
  if (!w) return -1;
  if (w->has_shuffle || w->shuffle) {
    set_err("%s: the weight is act-order (desc_act): rows are not gathered from it", who);
    return -1;
  }
  if (out_dtype != kActF32 && out_dtype != kActF16 && out_dtype != kActBF16) {
    set_err("%s: out_dtype must be fp32 (0), fp16 (1) or bf16 (2) (out_dtype=%d)", who, out_dtype);
    return -1;
  }
  if (m < 0) {
    set_err("%s: m must not be negative (m=%d)", who, m);
    return -1;
  }
  if (ldo < w->k) {
    set_err("%s: ldo must be at least k (ldo=%d k=%d)", who, ldo, w->k);
    return -1;
  }
  const int esz = out_dtype == kActF32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0 || (uint64_t(ldo) * esz) % 16 != 0) {
    set_err("%s: the rows are written with 16-byte stores: out needs a 16-byte aligned base and ldo a multiple of %d "
            "elements (ldo=%d)", who, 16 / esz, ldo);
    return -1;
  }
  if (ids_stride < 1) {
    set_err("%s: ids_stride must be at least 1 (ids_stride=%d)", who, ids_stride);
    return -1;
  }
  const bool q6k = is_q6k(*w);
  if (!q6k && w->ng > 1 && w->blocksize % 32 != 0) {
    set_err("%s: the group size must be a multiple of 32 (blocksize=%d)", who, w->blocksize);
    return -1;
  }
  if ((q6k && (w->k % 256 != 0 || w->f4kind >= 0)) || (!q6k && w->bits != 2 && w->bits != 4 && w->bits != 8) ||
      (w->f4kind >= 0 && (w->f4kind > 4 || (w->f4kind < 3) != (w->bits == 4)))) {
    set_err("%s: no row kernel for this weight (bits=%d kind=%d)", who, w->bits, w->f4kind);
    return -1;
  }
  int runs = 0, grid = 0;
  if (!get_rows_geometry(*w, m, &runs, &grid)) {
    set_err("%s: %d rows are more than one launch takes", who, m);
    return -1;
  }
  if (m == 0) return 0;
  const bool rec = planned(NAD_KERNEL_GET_ROWS, grid, kRowsWaves * 64);
  if (!rec) {
    if (!ids || !out) {
      set_err("%s: null ids / out", who);
      return -1;
    }
    if (!w->tiles || !w->scales || (q6k && !w->zps)) {
      set_err("%s: a geometry-only weight (nad_weight_plan_only) holds no weights", who);
      return -1;
    }
  }
  GetRowsArgs a{};
  a.w = *w;
  a.ids = ids;
  a.ids_stride = ids_stride;
  a.m = m;
  a.out = out;
  a.ldo = ldo;
  a.out_t = out_dtype;
  a.runs = runs;
  a.bs32 = (q6k || w->ng <= 1) ? INT_MAX : w->blocksize / 32;
  return launch(rec, "row gather kernel", [&] { return launch_get_rows(a, grid, st); }) ? 0 : -1;
}

extern "C" int nad_device_get_rows(const void* devstor, const int32_t* ids, int ids_stride, int m, void* out,
                                   int out_dtype, int ldo, void* queue) {
  return get_rows("nad_device_get_rows", devstor, ids, ids_stride, m, out, out_dtype, ldo,
                  static_cast<hipStream_t>(queue));
}
