// Cutoff filter over a host code's neighbour list -> CSR edge list, gfx950.
//
// The serial LAMMPS pair style (native/pair_e3gnn_core.cpp, SerialStep) takes
// its edges from LAMMPS' full list, built at cutoff + skin: every candidate j
// of centre i with |x_j - x_i|^2 < rc^2 is an edge (pair_e3gnn.cpp:156-182).
// This is that loop on the device, over the list as LAMMPS built it: atoms are
// LAMMPS indices (owned rows, then ghost rows that already carry their image
// shift in x), candidates keep LAMMPS' order, and nothing is sorted, so the
// edges are the host loop's edges bit for bit.
//
// One wave per graph row t (centre atom row_atom[t]).  The wave walks the row's
// candidates 64 at a time; each lane masks its entry (special bits), gathers
// x[j] and evaluates d = x[j] - x[i] and ((d0 d0) + (d1 d1)) + (d2 d2) < rc2 in
// f64 with contraction off -- the host loop's arithmetic.  A hit's slot is the
// row's running count plus the lane's rank in the ballot, so a row's edges keep
// the list's order.  The count pass (FILL = false) writes the row's degree, a
// scan gives the CSR offsets, the fill pass (FILL = true) recomputes the test
// and writes edge_center = t, edge_nbr = atom_row[j], edge_vec = (float)d.
// No LDS, no atomics: the output is a function of the inputs alone, and a row
// may hold any number of edges.
//
// The kernel indexes x, cand and atom_row without guards: e3gnn_plist_set
// (api_plist.cpp) has checked every index of the list on the host.
#include "pairlist.h"

#pragma clang fp contract(off)

namespace e3gnn {
namespace {

template <bool FILL>
__global__ __launch_bounds__(256) void k_pl_filter(
    int n, const double* __restrict__ x, const int* __restrict__ row_atom,
    const long long* __restrict__ cand_ptr, const int* __restrict__ cand, int neighmask,
    const int* __restrict__ atom_row, double rc2, int* __restrict__ deg,
    const int* __restrict__ row_ptr, int* __restrict__ center, int* __restrict__ nbr,
    float* __restrict__ vec) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wid);
  if (t >= n) return;
  const int i = __builtin_amdgcn_readfirstlane(row_atom[t]);
  const long long b = cand_ptr[t], e = cand_ptr[t + 1];
  const double xi0 = x[3 * (size_t)i], xi1 = x[3 * (size_t)i + 1], xi2 = x[3 * (size_t)i + 2];
  const long long base = FILL ? (long long)row_ptr[t] : 0;
  int count = 0;  // uniform
  for (long long c0 = b; c0 < e; c0 += 64) {
    const long long c = c0 + lane;
    bool hit = false;
    int j = 0;
    double d0 = 0, d1 = 0, d2 = 0;
    if (c < e) {
      j = cand[c] & neighmask;
      d0 = x[3 * (size_t)j] - xi0;
      d1 = x[3 * (size_t)j + 1] - xi1;
      d2 = x[3 * (size_t)j + 2] - xi2;
      const double r2 = ((d0 * d0) + (d1 * d1)) + (d2 * d2);
      hit = r2 < rc2;
    }
    const unsigned long long m = __ballot(hit);
    if (FILL && hit) {
      const long long q = base + count + __popcll(m & ((1ull << lane) - 1));
      center[q] = t;
      nbr[q] = atom_row[j];
      vec[3 * q] = (float)d0;
      vec[3 * q + 1] = (float)d1;
      vec[3 * q + 2] = (float)d2;
    }
    count += __popcll(m);
  }
  if constexpr (!FILL) {
    if (lane == 0) deg[t] = count;
  }
}

}  // namespace

hipError_t launch_pl_filter(bool fill, int n, const double* x, const int* row_atom,
                            const int64_t* cand_ptr, const int* cand, int neighmask,
                            const int* atom_row, double rc2, int* deg, const int* row_ptr,
                            int* center, int* nbr, float* vec, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 3) / 4), block(256);
  if (fill)
    hipLaunchKernelGGL(k_pl_filter<true>, grid, block, 0, s, n, x, row_atom,
                       (const long long*)cand_ptr, cand, neighmask, atom_row, rc2, deg, row_ptr,
                       center, nbr, vec);
  else
    hipLaunchKernelGGL(k_pl_filter<false>, grid, block, 0, s, n, x, row_atom,
                       (const long long*)cand_ptr, cand, neighmask, atom_row, rc2, deg, row_ptr,
                       center, nbr, vec);
  return hipGetLastError();
}

}  // namespace e3gnn
