// Launcher of scan.hip: the exclusive scan of int counts every graph build
// uses (CSR offsets of the neighbour lists, the rank graph, the list filter and
// the transposed graph of node.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace e3gnn {

// out[0..n) = exclusive prefix sums of cnt[0..n), out[n] = the total (n = 0:
// out[0] = 0).  bsum is a workspace of scan_blocks(n) ints for the scan over
// many workgroups; bsum == nullptr, or a short array, runs one workgroup.
// The sums are formed in unsigned arithmetic: a total beyond int32 wraps
// (defined), for the caller's total < 0 check to see.
int scan_blocks(int n);
hipError_t launch_exclusive_scan(int n, const int* cnt, int* out, int* bsum, hipStream_t s);

#ifdef __HIP__
// inclusive scan across the wave's lanes
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}
#endif

}  // namespace e3gnn
