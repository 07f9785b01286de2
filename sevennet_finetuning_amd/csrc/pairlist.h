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

}  // namespace e3gnn
