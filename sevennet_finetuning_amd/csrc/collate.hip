// Batch assembly for training from a device-resident dataset, gfx950: one
// padded batch gathered in one launch.
//
// Thread r serves batch atom row r, batch edge r and slot r, each where it
// exists.  A row finds its slot by a scan of the slot table, which arrives by
// value in the kernel arguments (<= 64 slots, uniform loads).  Real rows copy
// from the dataset; rows past the real ones are the dummy atoms (type 0, NaN
// force label) and edges past the real ones the padded self edges
// (r_pad, 0, 0) of the dummy atoms, dealt out in blocks of pad_block so the
// centres stay non-decreasing.  A gather: no atomics, no order dependence.
#include "collate.h"

#include <algorithm>
#include <cmath>

namespace e3gnn {
namespace {

constexpr int TPB = 256;

__device__ __forceinline__ int slot_of(const int32_t* __restrict__ first, int n, int row) {
  // the last s < n with first[s] <= row (first is non-decreasing, first[0] = 0)
  int s = 0;
  for (int k = 1; k < n; ++k) s += first[k] <= row ? 1 : 0;
  return s;
}

__global__ __launch_bounds__(TPB) void k_collate(const CollateData d, const CollateOut o,
                                                 const CollateSlots t) {
  const int r = blockIdx.x * TPB + threadIdx.x;
  const float qnan = __int_as_float(0x7fc00000);
  const int n_real_atoms = t.dst_atom[t.n_real];
  const int n_real_edges = t.dst_edge[t.n_real];
  if (r < t.atom_cap) {
    const int s = slot_of(t.dst_atom, t.slots, r);
    o.batch[r] = s;
    if (s < t.n_real) {
      const int64_t a = t.src_atom[s] + (r - t.dst_atom[s]);
      o.x[r] = d.type[a];
      o.force[3 * (int64_t)r] = d.force[3 * a];
      o.force[3 * (int64_t)r + 1] = d.force[3 * a + 1];
      o.force[3 * (int64_t)r + 2] = d.force[3 * a + 2];
    } else {
      o.x[r] = 0;
      o.force[3 * (int64_t)r] = qnan;
      o.force[3 * (int64_t)r + 1] = qnan;
      o.force[3 * (int64_t)r + 2] = qnan;
    }
  }
  if (r < t.edge_cap) {
    const int64_t e = r;
    if (r < n_real_edges) {
      const int s = slot_of(t.dst_edge, t.n_real, r);
      const int64_t q = t.src_edge[s] + (r - t.dst_edge[s]);
      const int base = t.dst_atom[s];
      o.edge_index[e] = base + d.edge_center[q];
      o.edge_index[(int64_t)t.edge_cap + e] = base + d.edge_nbr[q];
      o.edge_vec[3 * e] = d.edge_vec[3 * q];
      o.edge_vec[3 * e + 1] = d.edge_vec[3 * q + 1];
      o.edge_vec[3 * e + 2] = d.edge_vec[3 * q + 2];
      if (o.shift) {
        o.shift[3 * e] = d.shift[3 * q];
        o.shift[3 * e + 1] = d.shift[3 * q + 1];
        o.shift[3 * e + 2] = d.shift[3 * q + 2];
      }
    } else {
      const int row = n_real_atoms + (r - n_real_edges) / t.pad_block;
      o.edge_index[e] = row;
      o.edge_index[(int64_t)t.edge_cap + e] = row;
      o.edge_vec[3 * e] = t.r_pad;
      o.edge_vec[3 * e + 1] = 0.f;
      o.edge_vec[3 * e + 2] = 0.f;
      if (o.shift) {
        o.shift[3 * e] = 0.f;
        o.shift[3 * e + 1] = 0.f;
        o.shift[3 * e + 2] = 0.f;
      }
    }
  }
  if (r < t.slots) {
    o.num_atoms[r] = t.dst_atom[r + 1] - t.dst_atom[r];
    if (r < t.n_real) {
      const int k = t.src[r];
      o.volume[r] = d.volume[k];
      o.energy[r] = d.energy[k];
      for (int c = 0; c < 6; ++c) o.stress[6 * r + c] = d.stress[6 * (int64_t)k + c];
    } else {
      o.volume[r] = 1.f;
      o.energy[r] = qnan;
      for (int c = 0; c < 6; ++c) o.stress[6 * r + c] = qnan;
    }
  }
}

}  // namespace

hipError_t launch_collate(const CollateData& d, const CollateOut& o, const CollateSlots& t,
                          hipStream_t s) {
  if (t.slots < 1 || t.slots > COLLATE_MAX_SLOTS || t.n_real < 0 || t.n_real > t.slots ||
      t.atom_cap < 0 || t.edge_cap < 0 || t.pad_block < 1)
    return hipErrorInvalidValue;
  const int rows = std::max(std::max(t.atom_cap, t.edge_cap), t.slots);
  hipLaunchKernelGGL(k_collate, dim3((rows + TPB - 1) / TPB), dim3(TPB), 0, s, d, o, t);
  return hipGetLastError();
}

}  // namespace e3gnn
