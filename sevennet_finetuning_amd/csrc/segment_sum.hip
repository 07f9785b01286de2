// Per-structure sums of a concatenated batch, gfx950: the energies (row width
// 1, from the atomic energies) and virials (row width 6, from the per-atom
// virials) of e3gnn_energy_forces_batch.
//
// One workgroup per structure, no atomics.  Thread t adds the rows t, t + 256,
// ... of its structure in that order, then a binary tree over the 256 partial
// sums in LDS: the order of the additions is a function of (rows in the
// structure, width) alone -- not of the structure's place in the batch, of the
// other structures or of timing -- so the sums are bitwise reproducible.
#include "segment_sum.h"

namespace e3gnn {
namespace {

constexpr int TPB = 256;

template <int W>
__global__ __launch_bounds__(TPB) void k_segment_sum(int n_rows, const int* __restrict__ ptr,
                                                     const float* __restrict__ in,
                                                     float* __restrict__ out) {
  __shared__ float part[W][TPB];
  const int s = blockIdx.x, t = threadIdx.x;
  const int b = min(max(ptr[s], 0), n_rows), e = min(max(ptr[s + 1], b), n_rows);
  float acc[W];
#pragma unroll
  for (int c = 0; c < W; ++c) acc[c] = 0.f;
  for (int r = b + t; r < e; r += TPB) {
    const float* x = in + (int64_t)W * r;
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] += x[c];
  }
#pragma unroll
  for (int c = 0; c < W; ++c) part[c][t] = acc[c];
  __syncthreads();
  for (int o = TPB / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int c = 0; c < W; ++c) part[c][t] += part[c][t + o];
    }
    __syncthreads();
  }
  if (t < W) out[(int64_t)W * s + t] = part[t][0];
}

}  // namespace

hipError_t launch_segment_sum(int B, const int* ptr, int n_rows, int width, const float* in,
                              float* out, hipStream_t s) {
  if (width != 1 && width != 6) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  if (width == 1)
    hipLaunchKernelGGL(k_segment_sum<1>, dim3(B), dim3(TPB), 0, s, n_rows, ptr, in, out);
  else
    hipLaunchKernelGGL(k_segment_sum<6>, dim3(B), dim3(TPB), 0, s, n_rows, ptr, in, out);
  return hipGetLastError();
}

}  // namespace e3gnn
