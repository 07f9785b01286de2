// Exclusive scan of int counts, gfx950: the one scan of the graph builds.
//
// Three launches over many workgroups: k_scan_blocks (1,024 counts per
// workgroup, 4 consecutive per thread: local exclusive prefixes to out, the
// block total to bsum), k_scan_top (one workgroup scans the block totals in
// place, out[n] = the grand total), k_scan_add (adds each block's offset).
// k_scan_top alone is the scan in one workgroup.  The single-workgroup scans
// this replaces (strided per-thread chunks) took 164 us for 97k nodes and 2 ms
// at 778k entries.
#include "scan.h"

namespace e3gnn {
namespace {

constexpr int SCAN_B = 1024;
// Up to this many entries k_scan_top's loop is no slower than three launches
// (the bins and rows of a batch of small structures; figures in DESIGN.md 4b).
constexpr int SCAN_ONE_WG = 4 * SCAN_B;

__global__ __launch_bounds__(256) void k_scan_blocks(int n, const int* __restrict__ cnt,
                                                     int* __restrict__ out, int* __restrict__ bsum) {
  __shared__ unsigned wsum[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int i0 = blockIdx.x * SCAN_B + 4 * t;
  unsigned c[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) c[q] = i0 + q < n ? (unsigned)cnt[i0 + q] : 0u;
  const unsigned ts = c[0] + c[1] + c[2] + c[3];
  const unsigned incl = wave_incl_scan(ts, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned base = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) base += q < w ? wsum[q] : 0u;
  unsigned run = base + incl - ts;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (i0 + q < n) out[i0 + q] = (int)run;
    run += c[q];
  }
  if (t == 255) bsum[blockIdx.x] = (int)(base + incl);
}
// one workgroup: out[0..m) = exclusive prefix sums of in[0..m) (out == in: in
// place), *tot = the total; 1,024 entries at a time with a carry
__global__ __launch_bounds__(1024) void k_scan_top(int m, const int* in, int* out,
                                                   int* __restrict__ tot) {
  __shared__ unsigned wsum[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned carry = 0;
  for (int c0 = 0; c0 < m; c0 += 1024) {
    const unsigned v = c0 + t < m ? (unsigned)in[c0 + t] : 0u;
    const unsigned incl = wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned base = carry;
    for (int q = 0; q < w; ++q) base += wsum[q];
    unsigned total = carry;
    for (int q = 0; q < 16; ++q) total += wsum[q];
    if (c0 + t < m) out[c0 + t] = (int)(base + incl - v);
    carry = total;
    __syncthreads();
  }
  if (t == 0) *tot = (int)carry;
}
__global__ __launch_bounds__(256) void k_scan_add(int n, const int* __restrict__ bsum,
                                                  int* __restrict__ out) {
  const int i0 = blockIdx.x * SCAN_B + 4 * threadIdx.x;
  const unsigned add = (unsigned)bsum[blockIdx.x];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (i0 + q < n) out[i0 + q] = (int)((unsigned)out[i0 + q] + add);
}

}  // namespace

int scan_blocks(int n) { return n > 0 ? (n + SCAN_B - 1) / SCAN_B : 1; }
hipError_t launch_exclusive_scan(int n, const int* cnt, int* out, int* bsum, hipStream_t s) {
  if (n < 0) return hipErrorInvalidValue;
  const int nb = scan_blocks(n);
  if (!bsum || n <= SCAN_ONE_WG) {
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, n, cnt, out, out + n);
  } else {
    hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(256), 0, s, n, cnt, out, bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, nb, bsum, bsum, out + n);
    hipLaunchKernelGGL(k_scan_add, dim3(nb), dim3(256), 0, s, n, bsum, out);
  }
  return hipGetLastError();
}

}  // namespace e3gnn
