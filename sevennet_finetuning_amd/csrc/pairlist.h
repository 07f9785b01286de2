// Launcher of pairlist.hip (cutoff filter over a host code's neighbour list).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {

// One wave per graph row t < n: the candidates cand[cand_ptr[t] .. cand_ptr[t+1])
// (masked with neighmask) of centre row_atom[t] within rc2 of it.  fill = false
// writes deg[t]; fill = true writes the edges of row t from row_ptr[t] on
// (row_ptr: exclusive scan of deg), in the list's order.  x: f64 [n_total][3].
// Unguarded: every index must have been validated (e3gnn_plist_set).
hipError_t launch_pl_filter(bool fill, int n, const double* x, const int* row_atom,
                            const int64_t* cand_ptr, const int* cand, int neighmask,
                            const int* atom_row, double rc2, int* deg, const int* row_ptr,
                            int* center, int* nbr, float* vec, hipStream_t s);

// The rank graph of the parallel pair style: the same walk with atom_class
// [n_total] in place of atom_row -- below n an owned row, n + k the k-th tag
// (k < n_class) the rank does not own.  Such a class gets the row n + r, r its
// rank among the classes with an edge by the place of their first edge.  Three
// launches around two scans (api_plist.cpp, e3gnn_plist_rank_build / _fetch):
//  _count: deg[t]; first_key[k] = (row << 32 | place in the row) of class k's
//          first edge, all-ones without one; row_first[t] = classes first seen
//          in row t.  Then row_ptr = scan(deg), first_ptr = scan(row_first),
//          first_ptr[n] = n_ghost.
//  _rows:  class_row[k] = n + r for every class with an edge.
//  _fill:  the edges from row_ptr[t] on, edge_nbr = the class or its class_row,
//          and ghost_atom[r] = the atom index of class r's first edge.
// Integer atomics only (a minimum, a count): every output is a function of the
// inputs alone.  Unguarded like launch_pl_filter (e3gnn_plist_set_rank).
hipError_t launch_pl_rank_count(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                                const int* cand, int neighmask, const int* atom_class, double rc2,
                                int n_class, int* deg, unsigned long long* first_key, int* row_first,
                                hipStream_t s);
hipError_t launch_pl_rank_rows(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                               const int* cand, int neighmask, const int* atom_class, double rc2,
                               const unsigned long long* first_key, const int* first_ptr,
                               int* class_row, hipStream_t s);
hipError_t launch_pl_rank_fill(int n, const double* x, const int* row_atom, const int64_t* cand_ptr,
                               const int* cand, int neighmask, const int* atom_class, double rc2,
                               const unsigned long long* first_key, const int* class_row,
                               const int* row_ptr, int* center, int* nbr, float* vec, int* ghost_atom,
                               hipStream_t s);

}  // namespace e3gnn
