// The error recorder's device sums (error_sums.hip): e3gnn_error_sums.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {
// sums[E3GNN_ERR_SUMS] (f64, layout in include/e3gnn.h) += this batch's terms
struct ErrSumArgs {
  int criterion;  // 0 MSE, 1 Huber(delta)
  float delta;
  int64_t nb, n;
  const float *e_pred, *e_ref;
  const int64_t* natoms;
  const float *f_pred, *f_ref, *s_pred, *s_ref;  // f_* / s_* null: that quantity is skipped
  float s_scale;
  double* sums;
};
hipError_t launch_error_sums(const ErrSumArgs& a, hipStream_t s);
}  // namespace e3gnn
