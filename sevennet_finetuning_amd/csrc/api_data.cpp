// The device-resident training dataset and its batch assembly behind the C
// ABI (include/e3gnn.h; kernel in collate.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "collate.h"

using namespace e3gnn;

struct e3gnn_dataset {
  int device = 0;
  int64_t S = 0;
  std::vector<int64_t> atom_ptr, edge_ptr;  // host copies, [S+1]
  CollateData d{};
};

namespace {
// Argument rules of e3gnn_dataset_create (host only).  Returns the refusal or "".
std::string dataset_args(int64_t S, const int64_t* atom_ptr, const int64_t* edge_ptr,
                         const e3gnn_dataset_arrays* a) {
  if (S < 1 || S >= (int64_t)1 << 30) return "dataset: the number of structures must be in [1, 2^30)";
  if (!atom_ptr) return "dataset: null atom_ptr";
  if (!edge_ptr) return "dataset: null edge_ptr";
  if (!a) return "dataset: null arrays";
  if (atom_ptr[0] != 0) return "dataset: atom_ptr[0] must be 0";
  if (edge_ptr[0] != 0) return "dataset: edge_ptr[0] must be 0";
  for (int64_t s = 0; s < S; ++s) {
    if (atom_ptr[s + 1] <= atom_ptr[s])
      return "dataset: structure " + std::to_string(s) +
             " is empty or atom_ptr decreases (every structure needs at least one atom)";
    if (edge_ptr[s + 1] < edge_ptr[s])
      return "dataset: edge_ptr decreases at structure " + std::to_string(s);
    if (atom_ptr[s + 1] - atom_ptr[s] >= (int64_t)1 << 30 ||
        edge_ptr[s + 1] - edge_ptr[s] >= (int64_t)1 << 31)
      return "dataset: structure " + std::to_string(s) + " is out of range (2^30 atoms, 2^31 edges)";
  }
  if (!a->type || !a->force) return "dataset: null atom array (type, force)";
  if (edge_ptr[S] > 0 && (!a->edge_center || !a->edge_nbr || !a->edge_vec))
    return "dataset: null edge array (edge_center, edge_nbr, edge_vec)";
  if (!a->energy || !a->stress || !a->volume)
    return "dataset: null per-structure array (energy, stress, volume)";
  return "";
}

// Argument rules of e3gnn_dataset_collate and the slot table of the batch,
// before any HIP call (host only).  Returns the refusal or "".
std::string collate_args(const e3gnn_dataset* h, int64_t n_real, const int64_t* index, int slots,
                         int64_t atom_cap, int64_t edge_cap, int64_t max_degree, float r_pad,
                         const e3gnn_batch_arrays* out, CollateSlots& t) {
  if (!h) return "collate: null dataset handle";
  if (!out) return "collate: null batch arrays";
  if (!out->x || !out->force_of_atoms || !out->batch || !out->num_atoms || !out->cell_volume ||
      !out->total_energy || !out->stress)
    return "collate: null batch buffer";
  if (edge_cap > 0 && (!out->edge_index || !out->edge_vec))
    return "collate: null batch buffer (edge_index, edge_vec)";
  if (edge_cap > 0 && h->d.shift && !out->pbc_shift)
    return "collate: null batch buffer (pbc_shift: the dataset holds shifts)";
  if (slots < 2 || slots > COLLATE_MAX_SLOTS)
    return "collate: the slot count must be in [2, " + std::to_string(COLLATE_MAX_SLOTS) +
           "] (the real structures plus at least one dummy)";
  if (n_real < 0 || n_real > slots - 1)
    return "collate: " + std::to_string(n_real) + " real structures in " + std::to_string(slots) +
           " slots (at most slots - 1: the last slot is a dummy)";
  if (n_real > 0 && !index) return "collate: null index list";
  if (!(r_pad > 0) || !std::isfinite(r_pad)) return "collate: r_pad must be finite and positive";
  if (atom_cap < 1 || atom_cap >= (int64_t)1 << 31 || edge_cap < 0 || edge_cap >= (int64_t)1 << 31)
    return "collate: capacities out of range (2^31)";
  int64_t atoms = 0, edges = 0;
  for (int64_t k = 0; k < n_real; ++k) {
    const int64_t s = index[k];
    if (s < 0 || s >= h->S)
      return "collate: index " + std::to_string(s) + " (entry " + std::to_string(k) +
             ") outside [0, " + std::to_string(h->S) + ")";
    t.dst_atom[k] = (int32_t)std::min<int64_t>(atoms, INT32_MAX);
    t.dst_edge[k] = (int32_t)std::min<int64_t>(edges, INT32_MAX);
    t.src[k] = (int32_t)s;
    t.src_atom[k] = h->atom_ptr[s];
    t.src_edge[k] = h->edge_ptr[s];
    atoms += h->atom_ptr[s + 1] - h->atom_ptr[s];
    edges += h->edge_ptr[s + 1] - h->edge_ptr[s];
  }
  const int64_t n_dummy = slots - n_real;
  if (atoms + n_dummy > atom_cap)
    return "collate: " + std::to_string(atoms) + " real atoms plus one atom for each of the " +
           std::to_string(n_dummy) + " dummy slots exceed the atom capacity " +
           std::to_string(atom_cap);
  if (edges > edge_cap)
    return "collate: " + std::to_string(edges) + " real edges exceed the edge capacity " +
           std::to_string(edge_cap);
  const int64_t n_dummy_atoms = atom_cap - atoms, pad = edge_cap - edges;
  const int64_t block = pad ? (pad + n_dummy_atoms - 1) / n_dummy_atoms : 1;
  if (pad && (max_degree < 1 || block > max_degree))
    return "collate: " + std::to_string(pad) + " padded edges over " +
           std::to_string(n_dummy_atoms) + " dummy atoms give a dummy atom " +
           std::to_string(block) + " edges, above the degree cap " + std::to_string(max_degree);
  // the dummy slots: one atom each, the last takes the rest
  for (int64_t k = n_real; k < slots; ++k) {
    t.dst_atom[k] = (int32_t)(atoms + (k - n_real));
    t.dst_edge[k] = (int32_t)edges;
  }
  t.dst_atom[slots] = (int32_t)atom_cap;
  t.dst_edge[slots] = (int32_t)edges;
  t.slots = slots;
  t.n_real = (int32_t)n_real;
  t.atom_cap = (int32_t)atom_cap;
  t.edge_cap = (int32_t)edge_cap;
  t.pad_block = (int32_t)block;
  t.r_pad = r_pad;
  return "";
}
}  // namespace

extern "C" {

e3gnn_dataset* e3gnn_dataset_create(int device, int64_t n_structures, const int64_t* atom_ptr,
                                    const int64_t* edge_ptr, const e3gnn_dataset_arrays* a) {
  const std::string why = dataset_args(n_structures, atom_ptr, edge_ptr, a);
  if (!why.empty()) {
    fail(E3GNN_ERR_ARG, why);
    return nullptr;
  }
  auto* h = new e3gnn_dataset;
  h->device = device;
  h->S = n_structures;
  h->atom_ptr.assign(atom_ptr, atom_ptr + n_structures + 1);
  h->edge_ptr.assign(edge_ptr, edge_ptr + n_structures + 1);
  h->d = CollateData{a->type,     a->force,  a->edge_center, a->edge_nbr, a->edge_vec,
                     a->shift,    a->energy, a->stress,      a->volume};
  return h;
}

void e3gnn_dataset_free(e3gnn_dataset* h) { delete h; }

int e3gnn_dataset_collate(const e3gnn_dataset* h, int64_t n_real, const int64_t* index, int slots,
                          int64_t atom_cap, int64_t edge_cap, int64_t max_degree, float r_pad,
                          const e3gnn_batch_arrays* out, void* stream) {
  CollateSlots t{};
  {
    const std::string why =
        collate_args(h, n_real, index, slots, atom_cap, edge_cap, max_degree, r_pad, out, t);
    if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  }
  HIPCHK(hipSetDevice(h->device));
  const CollateOut o{out->x,     out->edge_index, out->edge_vec,    h->d.shift ? out->pbc_shift : nullptr,
                     out->force_of_atoms, out->batch,      out->num_atoms,   out->cell_volume,
                     out->total_energy,   out->stress};
  HIPCHK(launch_collate(h->d, o, t, (hipStream_t)stream));
  return E3GNN_OK;
}

}  // extern "C"
