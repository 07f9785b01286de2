// Launcher of segment_sum.hip (fixed-order per-structure sums of a batch).
#pragma once
#include <hip/hip_runtime.h>

namespace e3gnn {

// out[s][c] = sum of in[r][c] over r in [ptr[s], ptr[s+1]), s < B, c < width
// (1 or 6; anything else: hipErrorInvalidValue).  ptr is device memory; a range
// is clamped to [0, n_rows].
hipError_t launch_segment_sum(int B, const int* ptr, int n_rows, int width, const float* in,
                              float* out, hipStream_t s);

}  // namespace e3gnn
