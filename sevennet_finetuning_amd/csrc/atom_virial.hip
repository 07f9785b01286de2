// Per-atom virial of the energy+force path, gfx950: the edge-gradient
// partition ("Per-atom virial").  A translation unit of its own, so
// the code objects of node.hip and fused.hip do not change with it.
//
// Deterministic like every reduction of node.hip: one thread walks an atom's
// centre-side edges in CSR order, then its neighbour-side edges in src_perm
// order (no float atomics), so two evaluations give equal bits.
#include "atom_virial.h"

namespace e3gnn {
namespace {

constexpr int TPB = 256;

// half of edge e's virial term v_e = -voigt(r_e, f_e) (k_edge_force, node.hip)
// added to w: the diagonal entries -1/2 r_a f_a, the others -1/4 (r_a f_b + r_b f_a)
__device__ __forceinline__ void add_half(const float* __restrict__ vec, const float* __restrict__ fe,
                                         int e, float (&w)[6]) {
  const int64_t o = 3 * (int64_t)e;
  const float rx = vec[o], ry = vec[o + 1], rz = vec[o + 2];
  const float gx = fe[o], gy = fe[o + 1], gz = fe[o + 2];
  w[0] -= 0.5f * (rx * gx);
  w[1] -= 0.5f * (ry * gy);
  w[2] -= 0.5f * (rz * gz);
  w[3] -= 0.25f * (rx * gy + ry * gx);
  w[4] -= 0.25f * (ry * gz + rz * gy);
  w[5] -= 0.25f * (rx * gz + rz * gx);
}

// W_a = 1/2 sum_{e: center=a} v_e + 1/2 sum_{e: nbr=a} v_e; an edge from an
// atom to its own image gives both halves to that atom, so sum_a W_a = virial6
__global__ void k_atom_virial(int n_nodes, int n_centers, const int* __restrict__ row_ptr,
                              const int* __restrict__ src_ptr, const int* __restrict__ src_perm,
                              const float* __restrict__ vec, const float* __restrict__ fe,
                              float* __restrict__ W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  float w[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < n_centers)
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; ++e) add_half(vec, fe, e, w);
  for (int q = src_ptr[i]; q < src_ptr[i + 1]; ++q) add_half(vec, fe, src_perm[q], w);
  float* o = W + 6 * (int64_t)i;
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = w[k];
}

}  // namespace

hipError_t launch_atom_virial(int n_nodes, int n_centers, const int* row_ptr, const int* src_ptr,
                              const int* src_perm, const float* vec, const float* fe, float* W,
                              hipStream_t s) {
  if (n_nodes <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_atom_virial, dim3((n_nodes + TPB - 1) / TPB), dim3(TPB), 0, s, n_nodes,
                     n_centers, row_ptr, src_ptr, src_perm, vec, fe, W);
  return hipGetLastError();
}

}  // namespace e3gnn
