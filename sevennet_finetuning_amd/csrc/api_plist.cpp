// The cutoff filter over a host code's neighbour list behind the C ABI
// (include/e3gnn.h, e3gnn_plist_*; kernel in pairlist.hip, scan in scan.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "dbuf.h"
#include "pairlist.h"
#include "scan.h"

using namespace e3gnn;

extern "C" {

struct e3gnn_plist {
  int device = 0;
  int64_t n = 0, n_total = 0, ncand = 0, E = 0;
  int32_t neighmask = 0;
  bool is_set = false, built = false;
  const double* x = nullptr;   // of the last build (the fill pass reads it again)
  double rc2 = 0.0;
  DBuf row_atom, cand_ptr, cand, atom_row, deg, row_ptr, bsum;
  void* stage = nullptr;       // pinned host image of the four uploads
  size_t stage_cap = 0;
  ~e3gnn_plist() {
    if (stage) (void)hipHostFree(stage);
  }
};

// no HIP call: the device is first touched by e3gnn_plist_set
e3gnn_plist* e3gnn_plist_create(int device) {
  if (device < 0) {
    fail(E3GNN_ERR_ARG, "list filter: negative device");
    return nullptr;
  }
  auto* h = new e3gnn_plist;
  h->device = device;
  return h;
}
void e3gnn_plist_free(e3gnn_plist* h) { delete h; }

namespace {
// Argument rules of e3gnn_plist_set (host only: no handle state, no HIP call).
// Returns the refusal or nullptr.
const char* pl_set_args(bool have_handle, int64_t n, int64_t n_total, const int32_t* row_atom,
                        const int64_t* cand_ptr, const int32_t* cand, const int32_t* atom_row) {
  if (!have_handle) return "null list-filter handle";
  if (n <= 0 || n >= (int64_t)1 << 30) return "list filter: n must be in [1, 2^30)";
  if (n_total < n || n_total >= (int64_t)1 << 30) return "list filter: n_total must be in [n, 2^30)";
  if (!row_atom) return "list filter: null row_atom";
  if (!cand_ptr) return "list filter: null cand_ptr";
  if (!atom_row) return "list filter: null atom_row";
  if (!cand && cand_ptr[n] != 0) return "list filter: null cand";
  return nullptr;
}

// The list itself, one pass over the host arrays; `staged` (nullable) receives
// the raw candidates on the way.  Returns the refusal or "".
std::string pl_check_list(int64_t n, int64_t n_total, const int32_t* row_atom,
                          const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                          const int32_t* atom_row, int32_t* staged) {
  // cand_ptr first, whole: the candidate loop below then stays inside
  // [0, cand_ptr[n]), the length the caller vouches for
  if (cand_ptr[0] != 0) return "list filter: cand_ptr[0] must be 0";
  for (int64_t t = 0; t < n; ++t)
    if (cand_ptr[t + 1] < cand_ptr[t])
      return "list filter: row " + std::to_string(t) + ": cand_ptr decreases";
  for (int64_t a = 0; a < n_total; ++a)
    if (atom_row[a] < 0 || atom_row[a] >= n)
      return "list filter: atom " + std::to_string(a) + ": atom_row " + std::to_string(atom_row[a]) +
             " outside [0, n)";
  for (int64_t t = 0; t < n; ++t) {
    const std::string row = "list filter: row " + std::to_string(t);
    const int64_t b = cand_ptr[t], e = cand_ptr[t + 1];
    if (row_atom[t] < 0 || row_atom[t] >= n_total)
      return row + ": row_atom " + std::to_string(row_atom[t]) + " outside [0, n_total)";
    if (atom_row[row_atom[t]] != t)
      return row + ": atom_row[row_atom] is " + std::to_string(atom_row[row_atom[t]]) +
             " (the two maps must agree on the n nodes)";
    for (int64_t c = b; c < e; ++c) {
      const int32_t v = cand[c], j = v & neighmask;
      if (j < 0 || j >= n_total)
        return row + ": candidate " + std::to_string(j) + " outside [0, n_total)";
      if (staged) staged[c] = v;
    }
  }
  return "";
}
}  // namespace

int e3gnn_plist_check_list(int64_t n, int64_t n_total, const int32_t* row_atom,
                           const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                           const int32_t* atom_row) {
  if (const char* why = pl_set_args(true, n, n_total, row_atom, cand_ptr, cand, atom_row))
    return fail(E3GNN_ERR_ARG, why);
  const std::string why = pl_check_list(n, n_total, row_atom, cand_ptr, cand, neighmask, atom_row,
                                        nullptr);
  if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  return E3GNN_OK;
}

int e3gnn_plist_set(e3gnn_plist* h, int64_t n, int64_t n_total, const int32_t* row_atom,
                    const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                    const int32_t* atom_row, void* stream) {
  if (const char* why = pl_set_args(h != nullptr, n, n_total, row_atom, cand_ptr, cand, atom_row))
    return fail(E3GNN_ERR_ARG, why);
  h->is_set = false;
  h->built = false;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  // pinned image: cand_ptr [n+1] i64 | cand [ncand] | row_atom [n] | atom_row [n_total]
  // (a garbage cand_ptr[n] only sizes the request: the check below refuses it)
  const int64_t ncand = cand_ptr[n] > 0 ? cand_ptr[n] : 0;
  const size_t b_ptr = (size_t)(n + 1) * 8, b_cand = (size_t)ncand * 4, b_row = (size_t)n * 4,
               b_atom = (size_t)n_total * 4;
  const size_t need = b_ptr + b_cand + b_row + b_atom;
  if (need > h->stage_cap) {
    if (h->stage) HIPCHK(hipHostFree(h->stage));
    h->stage = nullptr;
    h->stage_cap = 0;
    const size_t cap = need + need / 5 + 4096;
    HIPCHK(hipHostMalloc(&h->stage, cap, hipHostMallocDefault));
    h->stage_cap = cap;
  }
  char* st = (char*)h->stage;
  int32_t* st_cand = (int32_t*)(st + b_ptr);
  const std::string why =
      pl_check_list(n, n_total, row_atom, cand_ptr, cand, neighmask, atom_row, st_cand);
  if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  std::memcpy(st, cand_ptr, b_ptr);
  std::memcpy(st + b_ptr + b_cand, row_atom, b_row);
  std::memcpy(st + b_ptr + b_cand + b_row, atom_row, b_atom);
  if (h->cand_ptr.ensure(b_ptr) != hipSuccess || h->cand.ensure(b_cand) != hipSuccess ||
      h->row_atom.ensure(b_row) != hipSuccess || h->atom_row.ensure(b_atom) != hipSuccess ||
      h->deg.ensure(b_row) != hipSuccess || h->row_ptr.ensure((size_t)(n + 1) * 4) != hipSuccess ||
      h->bsum.ensure((size_t)scan_blocks((int)n) * 4) != hipSuccess)
    return fail(E3GNN_ERR_HIP, "list-filter workspace allocation failed");
  HIPCHK(hipMemcpyAsync(h->cand_ptr.p, st, b_ptr, hipMemcpyHostToDevice, s));
  if (b_cand) HIPCHK(hipMemcpyAsync(h->cand.p, st_cand, b_cand, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->row_atom.p, st + b_ptr + b_cand, b_row, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->atom_row.p, st + b_ptr + b_cand + b_row, b_atom, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // the staging buffer is free for the next set
  h->n = n;
  h->n_total = n_total;
  h->ncand = ncand;
  h->neighmask = neighmask;
  h->is_set = true;
  return E3GNN_OK;
}

int e3gnn_plist_build(e3gnn_plist* h, const double* x, double cutoff, int64_t* n_edges,
                      void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null list-filter handle");
  if (!x) return fail(E3GNN_ERR_ARG, "list filter: null positions");
  if (!std::isfinite(cutoff) || !(cutoff > 0))
    return fail(E3GNN_ERR_ARG, "list filter: cutoff must be positive and finite");
  if (!h->is_set) return fail(E3GNN_ERR_ARG, "list filter: build before set");
  h->built = false;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)h->n;
  h->x = x;
  h->rc2 = cutoff * cutoff;
  HIPCHK(launch_pl_filter(false, n, x, h->row_atom.i(), (const int64_t*)h->cand_ptr.p, h->cand.i(),
                          h->neighmask, h->atom_row.i(), h->rc2, h->deg.i(), nullptr, nullptr,
                          nullptr, nullptr, s));
  HIPCHK(launch_exclusive_scan(n, h->deg.i(), h->row_ptr.i(), h->bsum.i(), s));
  int total = 0;
  HIPCHK(hipMemcpyAsync(&total, h->row_ptr.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int64_t E = total;
  if (h->ncand >= (int64_t)1 << 31) {
    // only then can the int32 scan have wrapped: the degrees summed in 64 bits
    std::vector<int32_t> deg((size_t)n);
    HIPCHK(hipMemcpy(deg.data(), h->deg.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    E = 0;
    for (int32_t d : deg) E += d;
  }
  if (E >= (int64_t)1 << 31) return fail(E3GNN_ERR_GRAPH, "edge count exceeds int32");
  h->E = E;
  h->built = true;
  if (n_edges) *n_edges = E;
  return E3GNN_OK;
}

int e3gnn_plist_fetch(e3gnn_plist* h, int32_t* edge_center, int32_t* edge_nbr, float* edge_vec,
                      void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null list-filter handle");
  if (!h->built) return fail(E3GNN_ERR_ARG, "list filter: fetch before build");
  if (h->E > 0 && (!edge_center || !edge_nbr || !edge_vec))
    return fail(E3GNN_ERR_ARG, "list filter: null edge output");
  if (h->E == 0) return E3GNN_OK;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(launch_pl_filter(true, (int)h->n, h->x, h->row_atom.i(), (const int64_t*)h->cand_ptr.p,
                          h->cand.i(), h->neighmask, h->atom_row.i(), h->rc2, nullptr,
                          h->row_ptr.i(), edge_center, edge_nbr, edge_vec, (hipStream_t)stream));
  return E3GNN_OK;
}

}  // extern "C"
