// woq_rows.h -- launch arguments and launcher of the row gather (woq_rows.hip): ne_get_rows on a device weight, the
// requested rows of the [N][K] matrix dequantized with the unpack kernels' operations.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "woq_layout.h"

namespace nad {

constexpr int kRowsWaves = 4;      // waves of a workgroup, one unit each
constexpr int kRowsTilesPerUnit = 16;  // K tiles of a unit: 64 lanes = 16 tiles x 4 k-quarters
constexpr int kRowsQ6kPerUnit = 4;     // Q6_K superblocks of a unit: 64 lanes = 4 superblocks x 4 group sets x 4 k-quarters

struct GetRowsArgs {
  DeviceWeight w;
  const int32_t* ids;  // device, m entries ids_stride int32s apart
  int64_t ids_stride;
  int m;
  void* out;           // device [m][ldo] of out_t (ActType codes), 16-byte aligned rows
  int64_t ldo;
  int out_t;
  int runs;            // units per row: ceil(nt / kRowsTilesPerUnit), Q6_K ceil(nt / kRowsQ6kPerUnit)
  int bs32;            // 32-k steps per group (one group: INT_MAX)
};

// units per row and workgroups of a launch of m rows (0 for m = 0); false where one launch does not take them
bool get_rows_geometry(const DeviceWeight& w, int m, int* runs, int* grid);
// one launch on the stream, nothing else; hipErrorInvalidValue for arguments the kernels do not take
hipError_t launch_get_rows(const GetRowsArgs& a, int grid, hipStream_t stream);

}  // namespace nad
