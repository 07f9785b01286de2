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
  // the rank graph (e3gnn_plist_set_rank / _rank_build / _rank_fetch): the same
  // list buffers, atom_row holding atom_class.  One list at a time: a set of
  // either kind replaces the other's, a build of either kind ends the other's fetch
  bool rank_set = false, rank_built = false;
  int64_t n_class = 0, n_ghost = 0;
  const double* x = nullptr;   // of the last build (the fill pass reads it again)
  double rc2 = 0.0;
  DBuf row_atom, cand_ptr, cand, atom_row, deg, row_ptr, bsum;
  DBuf first_key, row_first, first_ptr, class_row;   // rank graph only
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
// n_class < 0: the plain list (atom_row); else the rank list (atom_class).
const char* pl_set_args(bool have_handle, int64_t n, int64_t n_total, const int32_t* row_atom,
                        const int64_t* cand_ptr, const int32_t* cand, const int32_t* atom_row,
                        int64_t n_class = -1) {
  if (!have_handle) return "null list-filter handle";
  if (n <= 0 || n >= (int64_t)1 << 30) return "list filter: n must be in [1, 2^30)";
  if (n_total < n || n_total >= (int64_t)1 << 30) return "list filter: n_total must be in [n, 2^30)";
  if (!row_atom) return "list filter: null row_atom";
  if (!cand_ptr) return "list filter: null cand_ptr";
  if (!atom_row) return n_class < 0 ? "list filter: null atom_row" : "list filter: null atom_class";
  if (!cand && cand_ptr[n] != 0) return "list filter: null cand";
  return nullptr;
}

// ... and of the rank list on top: a class needs an atom of its own, so there
// are at most n_total - n; the first-edge keys hold an edge's place in its row
// in 32 bits and the offsets are int32, so the list stays below 2^31 entries
const char* pl_rank_args(int64_t n, int64_t n_total, const int64_t* cand_ptr, int64_t n_class) {
  if (n_class < 0 || n_class > n_total - n) return "list filter: n_class must be in [0, n_total - n]";
  if (cand_ptr[n] >= (int64_t)1 << 31) return "list filter: a rank list holds fewer than 2^31 candidates";
  return nullptr;
}

// The list itself, one pass over the host arrays; `staged` (nullable) receives
// the raw candidates on the way.  Returns the refusal or "".
// n_class >= 0: atom_row is atom_class, in [0, n + n_class), every class of
// [n, n + n_class) named by an atom.
std::string pl_check_list(int64_t n, int64_t n_total, const int32_t* row_atom,
                          const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                          const int32_t* atom_row, int32_t* staged, int64_t n_class = -1) {
  const bool rank = n_class >= 0;
  const char* map = rank ? "atom_class" : "atom_row";
  const int64_t rows = rank ? n + n_class : n;
  // cand_ptr first, whole: the candidate loop below then stays inside
  // [0, cand_ptr[n]), the length the caller vouches for
  if (cand_ptr[0] != 0) return "list filter: cand_ptr[0] must be 0";
  for (int64_t t = 0; t < n; ++t)
    if (cand_ptr[t + 1] < cand_ptr[t])
      return "list filter: row " + std::to_string(t) + ": cand_ptr decreases";
  for (int64_t a = 0; a < n_total; ++a)
    if (atom_row[a] < 0 || atom_row[a] >= rows)
      return "list filter: atom " + std::to_string(a) + ": " + map + " " + std::to_string(atom_row[a]) +
             (rank ? " outside [0, n + n_class)" : " outside [0, n)");
  if (rank && n_class > 0) {
    std::vector<char> named((size_t)n_class, 0);
    for (int64_t a = 0; a < n_total; ++a)
      if (atom_row[a] >= n) named[(size_t)(atom_row[a] - n)] = 1;
    for (int64_t k = 0; k < n_class; ++k)
      if (!named[(size_t)k])
        return "list filter: class " + std::to_string(n + k) + " is named by no atom";
  }
  for (int64_t t = 0; t < n; ++t) {
    const std::string row = "list filter: row " + std::to_string(t);
    const int64_t b = cand_ptr[t], e = cand_ptr[t + 1];
    if (row_atom[t] < 0 || row_atom[t] >= n_total)
      return row + ": row_atom " + std::to_string(row_atom[t]) + " outside [0, n_total)";
    if (atom_row[row_atom[t]] != t)
      return row + ": " + map + "[row_atom] is " + std::to_string(atom_row[row_atom[t]]) +
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

int e3gnn_plist_check_rank_list(int64_t n, int64_t n_total, const int32_t* row_atom,
                                const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                                const int32_t* atom_class, int64_t n_class) {
  const char* args = pl_set_args(true, n, n_total, row_atom, cand_ptr, cand, atom_class, n_class);
  if (!args) args = pl_rank_args(n, n_total, cand_ptr, n_class);
  if (args) return fail(E3GNN_ERR_ARG, args);
  const std::string why = pl_check_list(n, n_total, row_atom, cand_ptr, cand, neighmask, atom_class,
                                        nullptr, n_class);
  if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  return E3GNN_OK;
}

namespace {
// The body of e3gnn_plist_set and e3gnn_plist_set_rank (n_class < 0: the plain
// list) after the argument rules: checks the list on its way into the pinned
// image, sizes the workspace, uploads.
int pl_upload(e3gnn_plist* h, int64_t n, int64_t n_total, const int32_t* row_atom,
              const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
              const int32_t* atom_row, int64_t n_class, void* stream) {
  h->is_set = h->built = h->rank_set = h->rank_built = false;
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
      pl_check_list(n, n_total, row_atom, cand_ptr, cand, neighmask, atom_row, st_cand, n_class);
  if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  std::memcpy(st, cand_ptr, b_ptr);
  std::memcpy(st + b_ptr + b_cand, row_atom, b_row);
  std::memcpy(st + b_ptr + b_cand + b_row, atom_row, b_atom);
  if (h->cand_ptr.ensure(b_ptr) != hipSuccess || h->cand.ensure(b_cand) != hipSuccess ||
      h->row_atom.ensure(b_row) != hipSuccess || h->atom_row.ensure(b_atom) != hipSuccess ||
      h->deg.ensure(b_row) != hipSuccess || h->row_ptr.ensure((size_t)(n + 1) * 4) != hipSuccess ||
      h->bsum.ensure((size_t)scan_blocks((int)n) * 4) != hipSuccess)
    return fail(E3GNN_ERR_HIP, "list-filter workspace allocation failed");
  if (n_class >= 0 &&
      (h->first_key.ensure((size_t)(n_class + 1) * 8) != hipSuccess ||
       h->class_row.ensure((size_t)(n_class + 1) * 4) != hipSuccess ||
       h->row_first.ensure(b_row) != hipSuccess || h->first_ptr.ensure((size_t)(n + 1) * 4) != hipSuccess))
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
  h->n_class = n_class < 0 ? 0 : n_class;
  (n_class < 0 ? h->is_set : h->rank_set) = true;
  return E3GNN_OK;
}
}  // namespace

int e3gnn_plist_set(e3gnn_plist* h, int64_t n, int64_t n_total, const int32_t* row_atom,
                    const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                    const int32_t* atom_row, void* stream) {
  if (const char* why = pl_set_args(h != nullptr, n, n_total, row_atom, cand_ptr, cand, atom_row))
    return fail(E3GNN_ERR_ARG, why);
  return pl_upload(h, n, n_total, row_atom, cand_ptr, cand, neighmask, atom_row, -1, stream);
}

int e3gnn_plist_set_rank(e3gnn_plist* h, int64_t n, int64_t n_total, const int32_t* row_atom,
                         const int64_t* cand_ptr, const int32_t* cand, int32_t neighmask,
                         const int32_t* atom_class, int64_t n_class, void* stream) {
  const char* args = pl_set_args(h != nullptr, n, n_total, row_atom, cand_ptr, cand, atom_class, n_class);
  if (!args) args = pl_rank_args(n, n_total, cand_ptr, n_class);
  if (args) return fail(E3GNN_ERR_ARG, args);
  return pl_upload(h, n, n_total, row_atom, cand_ptr, cand, neighmask, atom_class, n_class, stream);
}

int e3gnn_plist_build(e3gnn_plist* h, const double* x, double cutoff, int64_t* n_edges,
                      void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null list-filter handle");
  if (!x) return fail(E3GNN_ERR_ARG, "list filter: null positions");
  if (!std::isfinite(cutoff) || !(cutoff > 0))
    return fail(E3GNN_ERR_ARG, "list filter: cutoff must be positive and finite");
  h->rank_built = false;   // a build of one kind ends the other kind's fetch
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

int e3gnn_plist_rank_build(e3gnn_plist* h, const double* x, double cutoff, int64_t* n_edges,
                           int64_t* n_ghost, void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null list-filter handle");
  if (!x) return fail(E3GNN_ERR_ARG, "list filter: null positions");
  if (!std::isfinite(cutoff) || !(cutoff > 0))
    return fail(E3GNN_ERR_ARG, "list filter: cutoff must be positive and finite");
  h->built = false;   // a build of one kind ends the other kind's fetch
  if (!h->rank_set) return fail(E3GNN_ERR_ARG, "list filter: rank_build before set_rank");
  h->rank_built = false;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)h->n;
  const int64_t* cand_ptr = (const int64_t*)h->cand_ptr.p;
  auto* first_key = (unsigned long long*)h->first_key.p;
  h->x = x;
  h->rc2 = cutoff * cutoff;
  HIPCHK(launch_pl_rank_count(n, x, h->row_atom.i(), cand_ptr, h->cand.i(), h->neighmask,
                              h->atom_row.i(), h->rc2, (int)h->n_class, h->deg.i(), first_key,
                              h->row_first.i(), s));
  HIPCHK(launch_exclusive_scan(n, h->deg.i(), h->row_ptr.i(), h->bsum.i(), s));
  HIPCHK(launch_exclusive_scan(n, h->row_first.i(), h->first_ptr.i(), h->bsum.i(), s));
  HIPCHK(launch_pl_rank_rows(n, x, h->row_atom.i(), cand_ptr, h->cand.i(), h->neighmask,
                             h->atom_row.i(), h->rc2, first_key, h->first_ptr.i(), h->class_row.i(), s));
  int total[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&total[0], h->row_ptr.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&total[1], h->first_ptr.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // fewer than 2^31 candidates (set_rank): neither scan can have wrapped
  h->E = total[0];
  h->n_ghost = total[1];
  h->rank_built = true;
  if (n_edges) *n_edges = h->E;
  if (n_ghost) *n_ghost = h->n_ghost;
  return E3GNN_OK;
}

int e3gnn_plist_rank_fetch(e3gnn_plist* h, int32_t* edge_center, int32_t* edge_nbr, float* edge_vec,
                           int32_t* ghost_atom, void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null list-filter handle");
  if (!h->rank_built) return fail(E3GNN_ERR_ARG, "list filter: rank_fetch before rank_build");
  if (h->E > 0 && (!edge_center || !edge_nbr || !edge_vec))
    return fail(E3GNN_ERR_ARG, "list filter: null edge output");
  if (h->n_ghost > 0 && !ghost_atom) return fail(E3GNN_ERR_ARG, "list filter: null ghost_atom");
  if (h->E == 0) return E3GNN_OK;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(launch_pl_rank_fill((int)h->n, h->x, h->row_atom.i(), (const int64_t*)h->cand_ptr.p,
                             h->cand.i(), h->neighmask, h->atom_row.i(), h->rc2,
                             (const unsigned long long*)h->first_key.p, h->class_row.i(),
                             h->row_ptr.i(), edge_center, edge_nbr, edge_vec, ghost_atom,
                             (hipStream_t)stream));
  return E3GNN_OK;
}

}  // extern "C"
