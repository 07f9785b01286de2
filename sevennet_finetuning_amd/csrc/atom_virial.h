// Launcher of atom_virial.hip (the per-atom virial of the edge-gradient partition).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {
// W[n_nodes, 6] (xx, yy, zz, xy, yz, zx): each edge's virial term -voigt(r_e, f_e)
// in halves to its centre and its neighbour.  Rows >= n_centers (ghosts) have
// the neighbour side only; no launch for n_nodes == 0.
hipError_t launch_atom_virial(int n_nodes, int n_centers, const int* row_ptr, const int* src_ptr,
                              const int* src_perm, const float* vec, const float* fe, float* W,
                              hipStream_t s);
}  // namespace e3gnn
