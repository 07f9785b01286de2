// Launcher of collate.hip (one padded training batch gathered from a
// device-resident dataset; the contract is DESIGN.md §4i).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace e3gnn {

constexpr int COLLATE_MAX_SLOTS = 64;

// The concatenated dataset (device arrays the caller owns).
struct CollateData {
  const int32_t* type;         // [Na]
  const float* force;          // [Na][3]
  const int32_t* edge_center;  // [Ea], rows relative to the structure's first atom
  const int32_t* edge_nbr;     // [Ea]
  const float* edge_vec;       // [Ea][3]
  const float* shift;          // [Ea][3] or nullptr
  const float* energy;         // [S]
  const float* stress;         // [S][6]
  const float* volume;         // [S]
};

// The batch outputs (device arrays the caller owns; layouts of train.collate).
struct CollateOut {
  int64_t* x;           // [atom_cap]
  int64_t* edge_index;  // [2][edge_cap]
  float* edge_vec;      // [edge_cap][3]
  float* shift;         // [edge_cap][3] or nullptr
  float* force;         // [atom_cap][3]
  int64_t* batch;       // [atom_cap]
  int64_t* num_atoms;   // [slots]
  float* volume;        // [slots]
  float* energy;        // [slots]
  float* stress;        // [slots][6]
};

// The slot table of ONE batch, passed to the kernel by value: a later call
// cannot overwrite it before the kernel has read it.  Slots [0, n_real) are
// real structures, [n_real, slots) dummies.
struct CollateSlots {
  int32_t slots, n_real;
  int32_t atom_cap, edge_cap;
  int32_t pad_block;  // padded edges per dummy atom (the last block may be short)
  float r_pad;
  int32_t dst_atom[COLLATE_MAX_SLOTS + 1];  // first batch row of every slot; [slots] = atom_cap
  int32_t dst_edge[COLLATE_MAX_SLOTS + 1];  // first batch edge of a real slot; [n_real..] = real edges
  int32_t src[COLLATE_MAX_SLOTS];           // structure of a real slot
  int64_t src_atom[COLLATE_MAX_SLOTS];      // its first dataset atom row
  int64_t src_edge[COLLATE_MAX_SLOTS];      // its first dataset edge
};

// One launch over max(atom_cap, edge_cap, slots) rows: a gather, no atomics,
// bitwise reproducible.  Enqueues on `s` and returns.
hipError_t launch_collate(const CollateData& d, const CollateOut& o, const CollateSlots& t,
                          hipStream_t s);

}  // namespace e3gnn
