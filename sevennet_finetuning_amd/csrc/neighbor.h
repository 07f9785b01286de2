// Launchers of neighbor.hip (device cell-list neighbour list; its scans: scan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {

constexpr int NL_MAXD = 512;  // max edges per centre (LDS sort buffer per wave)

struct NlGeom {
  double cell[9];    // rows a, b, c (periodic) or the virtual box of a cluster
  double inv[9];     // frac = (pos - origin) @ inv
  double origin[3];
  int nb[3];         // bins per dimension (bin width >= rc)
  int R[3];          // bin-image stencil half-width per dimension
  int periodic;      // 1: all three dimensions periodic; 0: isolated cluster
  double rc2;
};

constexpr int NL_MAX_WORLD = 256;  // ranks of a decomposition (LDS owner counters)

// Rank-graph form of the search (one rank of a spatial decomposition).
struct NlRank {
  const int* centers;  // atom id of each centre: count pass by id, fill pass by local row
  const int* owner;    // [n] owner rank of every atom
  int rank;
  int* boundary_flag;  // count pass, [centres]: 1 if any neighbour is not owned
  int* ghost_flag;     // count pass, [n]: 1 for every non-owned neighbour
  const int* lid;      // fill pass, [n]: atom id -> local row
};

hipError_t launch_nl_bin(int n, const double* pos, const NlGeom& G, int* f0, int* bin,
                         int* bin_count, int* err, hipStream_t s);
hipError_t launch_nl_place(int n, const int* bin, const int* bin_start, int* cursor,
                           int* bin_atoms, hipStream_t s);
hipError_t launch_nl_search(bool fill, int n, const double* pos, const NlGeom& G, const int* f0,
                            const int* bin, const int* bin_start, const int* bin_atoms, int* deg,
                            const int* row_ptr, int* center, int* nbr, int* shift, float* vec,
                            int* err, hipStream_t s);
// the same search over a centre list, flags (count) or local rows (fill) per NlRank
hipError_t launch_nl_rank_search(bool fill, int nc, const double* pos, const NlGeom& G,
                                 const int* f0, const int* bin, const int* bin_start,
                                 const int* bin_atoms, int* deg, const int* row_ptr, int* center,
                                 int* nbr, int* shift, float* vec, int* err, const NlRank& rk,
                                 hipStream_t s);
// mine[a] = (owner[a] == rank); err |= 8 for an owner outside [0, world)
hipError_t launch_rk_mark(int n, const int* owner, int rank, int world, int* mine, int* err,
                          hipStream_t s);
// out[pos[a]] = a where flag[a] (pos = exclusive scan of flag)
hipError_t launch_rk_compact(int n, const int* flag, const int* pos, int* out, hipStream_t s);
// interior-then-boundary rows of the id-ordered centres: owned, deg_row, lid[owned]
hipError_t launch_rk_rows(int nc, const int* centers, const int* bflag, const int* bpos,
                          const int* deg, int* owned, int* deg_row, int* lid, hipStream_t s);
// stable counting sort of gid[ng] by owner over nblk = ceil(ng / 256) (>= 1) blocks:
// scatter = false fills hist[world * nblk], true places ghosts / lid from its scan off
hipError_t launch_rk_ghost_sort(bool scatter, int ng, int world, int nblk, const int* gid,
                                const int* owner, int* hist, const int* off, int n_local,
                                int* ghosts, int* lid, hipStream_t s);
hipError_t launch_rk_recv(int world, int nblk, const int* off, int64_t* recv_counts,
                          hipStream_t s);

// Batched form (B structures concatenated, one set of launches): structure s
// owns the rows [atom_ptr[s], atom_ptr[s+1]) and the bins [bin_base, bin_base +
// nb[0] nb[1] nb[2]) of one concatenated bin array, so candidates never cross
// structures.  err is int[4]: the flags of the single build (1, 2, 4) and, for
// each, 1 + the largest offending structure index (err[1], err[2], err[3]).
struct NlGeomB {
  NlGeom G;
  int bin_base;
};
// batch[a] = s for a in [atom_ptr[s], atom_ptr[s+1])
hipError_t launch_nlb_batch(int B, const int* atom_ptr, int* batch, hipStream_t s);
hipError_t launch_nlb_bin(int n, const double* pos, const NlGeomB* geoms, const int* batch, int* f0,
                          int* bin, int* bin_count, int* err, hipStream_t s);
hipError_t launch_nlb_search(bool fill, int n, const double* pos, const NlGeomB* geoms,
                             const int* batch, const int* f0, const int* bin,
                             const int* bin_start, const int* bin_atoms, int* deg,
                             const int* row_ptr, int* center, int* nbr, int* shift, float* vec,
                             int* err, hipStream_t s);
// edge_ptr[s] = row_ptr[atom_ptr[s]], s in [0, B]
hipError_t launch_nlb_edge_ptr(int B, const int* atom_ptr, const int* row_ptr, int64_t* edge_ptr,
                               hipStream_t s);

}  // namespace e3gnn
