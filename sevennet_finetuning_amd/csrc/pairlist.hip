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
//
// k_pl_rank further down is the same walk for the parallel pair style
// (ParallelStep): ghost atoms get graph rows in first-seen order.
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

// ---- the parallel pair style's rank graph (ParallelStep::build) ----
// The same walk with atom_class in place of atom_row: a class below n is an
// owned row (the atom itself, or a periodic self-image of it), a class n + k is
// the k-th tag this rank does not own.  The host loop gives such a tag the row
// n + r, r counting the tags in the order their first edge appears, and keeps
// the atom index of that first edge.  An edge's place in that order is (row t,
// position p in the row), packed as the key t << 32 | p, which sorts like the
// edge index without needing the row offsets:
//   COUNT  deg[t], and atomicMin(first_key[k], key) for every hit of class
//          n + k.  An integer minimum is the same in any order, so first_key
//          is a function of the inputs alone; it costs no pass of its own
//          (a per-row minimum and a second-level pass would cost two).
//   (k_pl_first_rows: row_first[t] = number of classes whose first edge is in
//    row t; integer adds, any order.  Scanned into first_ptr.)
//   RANK   a hit whose key is its class's first_key is a first edge: its rank
//          is first_ptr[t] + the first edges before it in the row (ballot), so
//          class_row[k] = n + rank.  Rows without a first edge leave at once.
//   FILL   the edges, edge_nbr = the class (owned) or class_row (ghost), and
//          ghost_atom[rank] = j at every first edge.
enum { PL_COUNT = 0, PL_RANK = 1, PL_FILL = 2 };
constexpr unsigned long long kNoEdge = ~0ull;   // first_key of a class without an edge

template <int MODE>
__global__ __launch_bounds__(256) void k_pl_rank(
    int n, const double* __restrict__ x, const int* __restrict__ row_atom,
    const long long* __restrict__ cand_ptr, const int* __restrict__ cand, int neighmask,
    const int* __restrict__ atom_class, double rc2, int* __restrict__ deg,
    unsigned long long* first_key, const int* __restrict__ first_ptr, int* class_row,
    const int* __restrict__ row_ptr, int* __restrict__ center, int* __restrict__ nbr,
    float* __restrict__ vec, int* __restrict__ ghost_atom) {
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wid);
  if (t >= n) return;
  int first_base = 0;
  if constexpr (MODE == PL_RANK) {
    first_base = first_ptr[t];
    if (first_ptr[t + 1] == first_base) return;
  }
  const int i = __builtin_amdgcn_readfirstlane(row_atom[t]);
  const long long b = cand_ptr[t], e = cand_ptr[t + 1];
  const double xi0 = x[3 * (size_t)i], xi1 = x[3 * (size_t)i + 1], xi2 = x[3 * (size_t)i + 2];
  const long long base = MODE == PL_FILL ? (long long)row_ptr[t] : 0;
  const unsigned long long below = (1ull << lane) - 1;
  int count = 0, nfirst = 0;  // uniform
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
    const int p = count + __popcll(m & below);
    const int cls = hit ? atom_class[j] : 0;
    const bool ghost = cls >= n;
    const unsigned long long key = ((unsigned long long)(unsigned)t << 32) | (unsigned)p;
    if constexpr (MODE == PL_COUNT) {
      if (ghost) atomicMin(&first_key[cls - n], key);
    } else if constexpr (MODE == PL_RANK) {
      const bool first = ghost && first_key[cls - n] == key;
      const unsigned long long mf = __ballot(first);
      if (first) class_row[cls - n] = n + first_base + nfirst + __popcll(mf & below);
      nfirst += __popcll(mf);
    } else if (hit) {
      const long long q = base + p;
      const int row = ghost ? class_row[cls - n] : cls;
      center[q] = t;
      nbr[q] = row;
      vec[3 * q] = (float)d0;
      vec[3 * q + 1] = (float)d1;
      vec[3 * q + 2] = (float)d2;
      if (ghost && first_key[cls - n] == key) ghost_atom[row - n] = j;
    }
    count += __popcll(m);
  }
  if constexpr (MODE == PL_COUNT) {
    if (lane == 0) deg[t] = count;
  }
}

__global__ __launch_bounds__(256) void k_pl_first_rows(int n_class,
                                                       const unsigned long long* __restrict__ first_key,
                                                       int* __restrict__ row_first) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_class) return;
  const unsigned long long key = first_key[k];
  if (key != kNoEdge) atomicAdd(&row_first[(int)(key >> 32)], 1);
}

}  // namespace

hipError_t launch_pl_rank_count(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                                const int* cand, int neighmask, const int* atom_class, double rc2,
                                int n_class, int* deg, unsigned long long* first_key, int* row_first,
                                hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipError_t err = hipMemsetAsync(row_first, 0, (size_t)n * 4, s);
  if (err != hipSuccess) return err;
  if (n_class > 0) {
    err = hipMemsetAsync(first_key, 0xff, (size_t)n_class * 8, s);   // kNoEdge
    if (err != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_pl_rank<PL_COUNT>, dim3((n + 3) / 4), dim3(256), 0, s, n, x, row_atom,
                     (const long long*)cand_ptr, cand, neighmask, atom_class, rc2, deg, first_key,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (n_class > 0)
    hipLaunchKernelGGL(k_pl_first_rows, dim3((n_class + 255) / 256), dim3(256), 0, s, n_class,
                       first_key, row_first);
  return hipGetLastError();
}

hipError_t launch_pl_rank_rows(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                               const int* cand, int neighmask, const int* atom_class, double rc2,
                               const unsigned long long* first_key, const int* first_ptr,
                               int* class_row, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pl_rank<PL_RANK>, dim3((n + 3) / 4), dim3(256), 0, s, n, x, row_atom,
                     (const long long*)cand_ptr, cand, neighmask, atom_class, rc2, nullptr,
                     const_cast<unsigned long long*>(first_key), first_ptr, class_row, nullptr,
                     nullptr, nullptr, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t launch_pl_rank_fill(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                               const int* cand, int neighmask, const int* atom_class, double rc2,
                               const unsigned long long* first_key, const int* class_row,
                               const int* row_ptr, int* center, int* nbr, float* vec, int* ghost_atom,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pl_rank<PL_FILL>, dim3((n + 3) / 4), dim3(256), 0, s, n, x, row_atom,
                     (const long long*)cand_ptr, cand, neighmask, atom_class, rc2, nullptr,
                     const_cast<unsigned long long*>(first_key), nullptr,
                     const_cast<int*>(class_row), row_ptr, center, nbr, vec, ghost_atom);
  return hipGetLastError();
}

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
