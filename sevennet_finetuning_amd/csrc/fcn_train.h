// The FCN readout (readout_as_fcn) in the fine-tune step's hand-scheduled
// derivatives (fcn_train.hip; train_explicit.py _Fcn).  Dims and the packed
// weights are the inference kernel's (node.h FcnDims).  Per hidden layer
// k = 1 .. nh of width w[k], with pre_k = w[1] + .. + w[k - 1]:
//   z, zd  [n, w[k]] at n pre_k      pre-activations z_k and their tangents z'_k
//   a, zb  [2n, w[k]] at 2n pre_k    rows [0, n): a_k / z-bar_k, rows [n, 2n):
//                                    a'_k / z'-bar_k (the stacked operands of
//                                    the weight-gradient products)
#pragma once
#include <hip/hip_runtime.h>

#include "node.h"

namespace e3gnn {
// x [n, D] -> z, a (primal rows), s [n] and, when dx is not null,
// dx [n, D] = seed[i] ds/dx (seed null: 1)
hipError_t launch_fcn_train_fwd(int n, const FcnDims& d, const float* W, const float* x, const float* seed,
                                float* z, float* a, float* s, float* dx, hipStream_t st);
// xd [n, D] (the tangent of x), z -> zd, a (tangent rows), sd [n]
hipError_t launch_fcn_train_tangent(int n, const FcnDims& d, const float* W, const float* xd, const float* z,
                                    float* zd, float* a, float* sd, hipStream_t st);
// the reverse of (s, s') seeded with (sb, sbd) [n]: zb and xb [2n, D]
hipError_t launch_fcn_train_dual(int n, const FcnDims& d, const float* W, const float* sb, const float* sbd,
                                 const float* z, const float* zd, float* zb, float* xb, hipStream_t st);
}  // namespace e3gnn
