// The device neighbour list, its batched form and the rank graph behind the C
// ABI (include/e3gnn.h; kernels in neighbor.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "dbuf.h"
#include "neighbor.h"
#include "scan.h"

using namespace e3gnn;

extern "C" {

// ------------------------------------------------------------ neighbour list
struct e3gnn_nlist {
  int device = 0;
  int64_t n = 0, E = 0;
  const double* pos = nullptr;
  bool built = false;
  DBuf f0, bin, bin_count, bin_start, cursor, bin_atoms, deg, row_ptr, err;
  DBuf bsum;  // the scans' block totals: scan_blocks(the longest array scanned) ints
  // rank graph (e3gnn_nlist_rank_build): counts and the row maps it keeps
  bool rank_built = false;
  int64_t n_local = 0, n_ghost = 0;
  int world = 0;
  DBuf flag, fpos, centers, bflag, degrow, owned, gid, ghosts, lid, hist, hoff, recv;
  // the structures of the last build (one, or the B of e3gnn_nlist_batch_build):
  // geometries and row ranges, uploaded for a batch
  bool batch_built = false;
  int64_t B = 0;
  DBuf geoms, batch, aptr;
  std::vector<NlGeomB> hgeoms;  // host images of the uploads: alive until the next build
  std::vector<int32_t> haptr;
};

e3gnn_nlist* e3gnn_nlist_create(int device) {
  if (hipSetDevice(device) != hipSuccess) {
    fail(E3GNN_ERR_HIP, "hipSetDevice failed");
    return nullptr;
  }
  auto* h = new e3gnn_nlist;
  h->device = device;
  return h;
}
void e3gnn_nlist_free(e3gnn_nlist* h) { delete h; }

namespace {
// bins of width >= rc per dimension (heights h), at most ~4 per atom
void nl_bins(NlGeom& G, const double h[3], double rc, int64_t n) {
  for (int k = 0; k < 3; ++k) G.nb[k] = std::max(1, (int)std::floor(h[k] / rc));
  while ((int64_t)G.nb[0] * G.nb[1] * G.nb[2] > 4 * n + 64) {
    int k = 0;
    for (int q = 1; q < 3; ++q)
      if (G.nb[q] > G.nb[k]) k = q;
    G.nb[k] = std::max(1, G.nb[k] / 2);
  }
  for (int k = 0; k < 3; ++k) G.R[k] = std::max(1, (int)std::ceil(rc * G.nb[k] / h[k]));
}

// Periodic cell (rows a, b, c): G.cell, G.inv and the heights.  Returns the
// refusal or nullptr.
const char* nl_cell_geom(NlGeom& G, const double* cell, double hgt[3]) {
  for (int k = 0; k < 9; ++k) G.cell[k] = cell[k];
  const double* a = cell;
  const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
                     a[2] * (a[3] * a[7] - a[4] * a[6]);
  if (!(std::fabs(det) > 1e-12)) return "singular cell";
  // inverse (rows of cell = lattice vectors): frac = pos @ inv
  G.inv[0] = (a[4] * a[8] - a[5] * a[7]) / det;
  G.inv[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  G.inv[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  G.inv[3] = (a[5] * a[6] - a[3] * a[8]) / det;
  G.inv[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  G.inv[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  G.inv[6] = (a[3] * a[7] - a[4] * a[6]) / det;
  G.inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  G.inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  for (int k = 0; k < 3; ++k) {  // height along k = |det| / |a_{k+1} x a_{k+2}|
    const double* u = a + 3 * ((k + 1) % 3);
    const double* v = a + 3 * ((k + 2) % 3);
    const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2],
                 cz = u[0] * v[1] - u[1] * v[0];
    hgt[k] = std::fabs(det) / std::sqrt(cx * cx + cy * cy + cz * cz);
  }
  return nullptr;
}

// Isolated cluster (hp: its n positions on the host): a virtual orthorhombic
// box 1 A beyond the atoms on every side, so no image is ever within the
// cutoff (S = 0 throughout).  Returns the refusal or nullptr.
const char* nl_cluster_geom(NlGeom& G, const double* hp, int64_t n, double hgt[3]) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int64_t a = 0; a < n; ++a)
    for (int k = 0; k < 3; ++k) {
      const double v = hp[3 * a + k];
      if (!std::isfinite(v)) return "non-finite position";
      lo[k] = a ? std::min(lo[k], v) : v;
      hi[k] = a ? std::max(hi[k], v) : v;
    }
  for (int k = 0; k < 3; ++k) {
    G.origin[k] = lo[k] - 1.0;
    hgt[k] = (hi[k] - lo[k]) + 2.0;
    G.cell[4 * k] = hgt[k];
    G.inv[4 * k] = 1.0 / hgt[k];
  }
  return nullptr;
}

// What every build starts with: the handle reset, the geometry and the bins of
// each of the B structures (rows [atom_ptr[k], atom_ptr[k + 1]); periodic[k]:
// all three dimensions periodic with the cell at cells + 9 k, else an isolated
// cluster), the workspace, and the atoms binned (bin, scan, place).  The single
// and the rank build are B = 1, not `batched`: their kernels take the one
// geometry by value, and nothing is uploaded.
int nl_bin_atoms(e3gnn_nlist* h, bool batched, int64_t B, const int64_t* atom_ptr,
                 const double* pos, const double* cells, const int32_t* periodic, double cutoff,
                 hipStream_t s) {
  HIPCHK(hipSetDevice(h->device));
  h->built = false;
  h->rank_built = false;
  h->batch_built = false;
  const int64_t n = atom_ptr[B];
  h->n = n;
  h->B = B;
  h->pos = pos;
  // isolated members need their extent: one copy of the positions per build
  std::vector<double> hp;
  bool any_isolated = false;
  for (int64_t k = 0; k < B; ++k) any_isolated |= periodic[k] == 0;
  if (any_isolated) {
    hp.resize((size_t)n * 3);
    if (n) HIPCHK(hipMemcpy(hp.data(), pos, hp.size() * 8, hipMemcpyDefault));
  }
  h->hgeoms.assign((size_t)B, NlGeomB{});
  h->haptr.resize((size_t)B + 1);
  int64_t nbins = 0;
  for (int64_t k = 0; k < B; ++k) {
    NlGeom& G = h->hgeoms[k].G;
    const int64_t n_k = atom_ptr[k + 1] - atom_ptr[k];
    G.rc2 = cutoff * cutoff;
    G.periodic = periodic[k] ? 1 : 0;
    double hgt[3];
    const char* why = !periodic[k] ? nl_cluster_geom(G, hp.data() + 3 * atom_ptr[k], n_k, hgt)
                      : !cells     ? "null cell"
                                   : nl_cell_geom(G, cells + 9 * k, hgt);
    if (why)
      return fail(E3GNN_ERR_ARG,
                  (batched ? "batch: structure " + std::to_string(k) + ": " : std::string()) + why);
    nl_bins(G, hgt, cutoff, n_k);
    h->hgeoms[k].bin_base = (int)nbins;
    h->haptr[k] = (int32_t)atom_ptr[k];
    nbins += (int64_t)G.nb[0] * G.nb[1] * G.nb[2];
    if (nbins >= (int64_t)1 << 31) return fail(E3GNN_ERR_ARG, "batch: bin count exceeds int32");
  }
  h->haptr[B] = (int32_t)n;
  const size_t n1 = (size_t)std::max<int64_t>(n, 1);
  if (h->f0.ensure(n1 * 12) != hipSuccess || h->bin.ensure(n1 * 4) != hipSuccess ||
      h->bin_atoms.ensure(n1 * 4) != hipSuccess || h->deg.ensure(n1 * 4) != hipSuccess ||
      h->row_ptr.ensure((size_t)(n + 1) * 4) != hipSuccess ||
      h->bin_count.ensure((size_t)nbins * 4) != hipSuccess ||
      h->bin_start.ensure((size_t)(nbins + 1) * 4) != hipSuccess ||
      h->cursor.ensure((size_t)nbins * 4) != hipSuccess || h->err.ensure(16) != hipSuccess ||
      h->bsum.ensure((size_t)scan_blocks((int)std::max(n, nbins)) * 4) != hipSuccess ||
      (batched && (h->geoms.ensure((size_t)B * sizeof(NlGeomB)) != hipSuccess ||
                   h->batch.ensure(n1 * 4) != hipSuccess ||
                   h->aptr.ensure((size_t)(B + 1) * 4) != hipSuccess)))
    return fail(E3GNN_ERR_HIP, "neighbour-list workspace allocation failed");
  int* err = h->err.i();
  HIPCHK(hipMemsetAsync(err, 0, 16, s));
  HIPCHK(hipMemsetAsync(h->bin_count.p, 0, (size_t)nbins * 4, s));
  HIPCHK(hipMemsetAsync(h->cursor.p, 0, (size_t)nbins * 4, s));
  if (batched) {
    HIPCHK(hipMemcpyAsync(h->geoms.p, h->hgeoms.data(), (size_t)B * sizeof(NlGeomB),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->aptr.p, h->haptr.data(), (size_t)(B + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(launch_nlb_batch((int)B, h->aptr.i(), h->batch.i(), s));
    HIPCHK(launch_nlb_bin((int)n, pos, (const NlGeomB*)h->geoms.p, h->batch.i(), h->f0.i(),
                          h->bin.i(), h->bin_count.i(), err, s));
  } else {
    HIPCHK(launch_nl_bin((int)n, pos, h->hgeoms[0].G, h->f0.i(), h->bin.i(), h->bin_count.i(), err,
                         s));
  }
  HIPCHK(launch_exclusive_scan((int)nbins, h->bin_count.i(), h->bin_start.i(), h->bsum.i(), s));
  HIPCHK(launch_nl_place((int)n, h->bin.i(), h->bin_start.i(), h->cursor.i(), h->bin_atoms.i(), s));
  return E3GNN_OK;
}

// The fetched err words of a build or a fetch (neighbor.h: int[1], of a batch
// int[4]) as its refusal, or E3GNN_OK.
int nl_refusal(const int* herr, bool batched) {
  auto where = [&](int slot) {
    return batched ? "batch: structure " + std::to_string(herr[slot] - 1) + ": " : std::string();
  };
  if (herr[0] & 1)
    return fail(E3GNN_ERR_ARG, where(1) + "non-finite or out-of-box atom position");
  if (herr[0] & 8)
    return fail(E3GNN_ERR_GRAPH, "rank graph: an owner value is outside [0, world)");
  if (herr[0] & 4)
    return fail(E3GNN_ERR_GRAPH, where(3) + "a centre has more than " + std::to_string(NL_MAXD) +
                                     " neighbours (device neighbour-list limit)");
  if (herr[0] & 2)
    return fail(E3GNN_ERR_GRAPH, where(2) + "periodic image shift beyond +-1024 cells");
  return E3GNN_OK;
}

// The single and the batched build after the binning: the count pass, the
// degrees scanned into row_ptr, the device's refusals, the edge count.
int nl_count_edges(e3gnn_nlist* h, bool batched, int64_t* n_edges, hipStream_t s) {
  const int n = (int)h->n;
  int* err = h->err.i();
  if (batched)
    HIPCHK(launch_nlb_search(false, n, h->pos, (const NlGeomB*)h->geoms.p, h->batch.i(),
                             h->f0.i(), h->bin.i(), h->bin_start.i(), h->bin_atoms.i(), h->deg.i(),
                             nullptr, nullptr, nullptr, nullptr, nullptr, err, s));
  else
    HIPCHK(launch_nl_search(false, n, h->pos, h->hgeoms[0].G, h->f0.i(), h->bin.i(),
                            h->bin_start.i(), h->bin_atoms.i(), h->deg.i(), nullptr, nullptr,
                            nullptr, nullptr, nullptr, err, s));
  HIPCHK(launch_exclusive_scan(n, h->deg.i(), h->row_ptr.i(), h->bsum.i(), s));
  int herr[4] = {0, 0, 0, 0}, total = 0;
  HIPCHK(hipMemcpyAsync(herr, err, batched ? 16 : 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&total, h->row_ptr.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (const int rc = nl_refusal(herr, batched)) return rc;
  if (total < 0) return fail(E3GNN_ERR_GRAPH, "edge count exceeds int32");
  h->E = total;
  (batched ? h->batch_built : h->built) = true;
  if (n_edges) *n_edges = total;
  return E3GNN_OK;
}

// The refusal of a fill pass (a shift beyond the key's range), once it has run.
int nl_fill_refusal(e3gnn_nlist* h, bool batched, hipStream_t s) {
  int herr[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(herr, h->err.i(), batched ? 16 : 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return nl_refusal(herr, batched);
}
}  // namespace

int e3gnn_nlist_build(e3gnn_nlist* h, int64_t n, const double* pos, const double* cell,
                      const int* pbc, double cutoff, int64_t* n_edges, void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null neighbour-list handle");
  if (n < 0 || n >= (int64_t)1 << 30) return fail(E3GNN_ERR_ARG, "atom count out of range");
  if (!(cutoff > 0)) return fail(E3GNN_ERR_ARG, "cutoff must be positive");
  if (n > 0 && !pos) return fail(E3GNN_ERR_ARG, "null positions");
  if (!pbc) return fail(E3GNN_ERR_ARG, "null pbc flags");
  const bool all = pbc[0] && pbc[1] && pbc[2], none = !pbc[0] && !pbc[1] && !pbc[2];
  if (!all && !none)
    return fail(E3GNN_ERR_ARG, "device neighbour list: pbc must be all true or all false");
  hipStream_t s = (hipStream_t)stream;
  const int64_t atom_ptr[2] = {0, n};
  const int32_t periodic = all ? 7 : 0;
  if (const int rc = nl_bin_atoms(h, false, 1, atom_ptr, pos, cell, &periodic, cutoff, s)) return rc;
  return nl_count_edges(h, false, n_edges, s);
}

int e3gnn_nlist_fetch(e3gnn_nlist* h, int32_t* center, int32_t* nbr, int32_t* shift, float* vec,
                      void* stream) {
  if (!h || !h->built) return fail(E3GNN_ERR_ARG, "neighbour list not built");
  if (h->E > 0 && (!center || !nbr)) return fail(E3GNN_ERR_ARG, "null edge output");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int* err = h->err.i();
  HIPCHK(hipMemsetAsync(err, 0, 4, s));
  HIPCHK(launch_nl_search(true, (int)h->n, h->pos, h->hgeoms[0].G, h->f0.i(), h->bin.i(),
                          h->bin_start.i(), h->bin_atoms.i(), nullptr, h->row_ptr.i(), center, nbr,
                          shift, vec, err, s));
  return nl_fill_refusal(h, false, s);
}

namespace {
// Argument rules of e3gnn_nlist_rank_build, checked before any device work
// (host only: no handle state, no HIP call).  Returns the refusal or nullptr.
const char* nl_rank_args(bool have_handle, int64_t n, const double* pos, const double* cell,
                         double cutoff, const int32_t* owner, int rank, int world) {
  if (world < 1 || world > NL_MAX_WORLD) return "rank graph: world must be in [1, 256]";
  if (rank < 0 || rank >= world) return "rank graph: rank outside [0, world)";
  if (!have_handle) return "null neighbour-list handle";
  if (n < 0 || n >= (int64_t)1 << 30) return "atom count out of range";
  if (!(cutoff > 0)) return "cutoff must be positive";
  if (n > 0 && !pos) return "null positions";
  if (n > 0 && !owner) return "rank graph: null owner array";
  if (!cell) return "rank graph: null cell (all three dimensions must be periodic)";
  return nullptr;
}
}  // namespace

int e3gnn_nlist_rank_build(e3gnn_nlist* h, int64_t n, const double* pos, const double* cell,
                           double cutoff, const int32_t* owner, int rank, int world,
                           int64_t* n_local, int64_t* n_interior, int64_t* n_ghost,
                           int64_t* n_edges, void* stream) {
  static_assert(NL_MAX_WORLD == 256, "message of nl_rank_args");
  if (const char* why = nl_rank_args(h != nullptr, n, pos, cell, cutoff, owner, rank, world))
    return fail(E3GNN_ERR_ARG, why);
  hipStream_t s = (hipStream_t)stream;
  const int64_t atom_ptr[2] = {0, n};
  const int32_t periodic = 7;
  if (const int rc = nl_bin_atoms(h, false, 1, atom_ptr, pos, cell, &periodic, cutoff, s)) return rc;
  const NlGeom& G = h->hgeoms[0].G;
  int* err = h->err.i();
  const size_t n1 = (size_t)std::max<int64_t>(n, 1);
  if (h->flag.ensure(n1 * 4) != hipSuccess || h->fpos.ensure((n1 + 1) * 4) != hipSuccess ||
      h->lid.ensure(n1 * 4) != hipSuccess || h->recv.ensure((size_t)world * 8) != hipSuccess)
    return fail(E3GNN_ERR_HIP, "rank-graph workspace allocation failed");
  // bsum: sized for n entries by nl_bin_atoms, and for the ghost histogram below
  auto scan = [&](int m, const int* cnt, int* out) {
    return launch_exclusive_scan(m, cnt, out, h->bsum.i(), s);
  };
  // the rank's atoms in id order
  HIPCHK(launch_rk_mark((int)n, owner, rank, world, h->flag.i(), err, s));
  HIPCHK(scan((int)n, h->flag.i(), h->fpos.i()));
  int herr = 0, nc = 0;
  HIPCHK(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&nc, h->fpos.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (const int rc = nl_refusal(&herr, false)) return rc;
  const size_t nc1 = (size_t)std::max(nc, 1);
  if (h->centers.ensure(nc1 * 4) != hipSuccess || h->bflag.ensure(nc1 * 4) != hipSuccess ||
      h->degrow.ensure(nc1 * 4) != hipSuccess || h->owned.ensure(nc1 * 4) != hipSuccess ||
      h->gid.ensure(n1 * 4) != hipSuccess)
    return fail(E3GNN_ERR_HIP, "rank-graph workspace allocation failed");
  HIPCHK(launch_rk_compact((int)n, h->flag.i(), h->fpos.i(), h->centers.i(), s));
  // count pass: degrees, boundary flags, ghost flags (h->flag from here on)
  HIPCHK(hipMemsetAsync(h->flag.p, 0, n1 * 4, s));
  HIPCHK(hipMemsetAsync(h->lid.p, 0xff, n1 * 4, s));
  NlRank rk{};
  rk.centers = h->centers.i();
  rk.owner = owner;
  rk.rank = rank;
  rk.boundary_flag = h->bflag.i();
  rk.ghost_flag = h->flag.i();
  HIPCHK(launch_nl_rank_search(false, nc, pos, G, h->f0.i(), h->bin.i(), h->bin_start.i(),
                               h->bin_atoms.i(), h->deg.i(), nullptr, nullptr, nullptr, nullptr,
                               nullptr, err, rk, s));
  // rows: interior then boundary; degrees in row order -> row_ptr
  int nbnd = 0, total = 0, ng = 0;
  HIPCHK(scan(nc, h->bflag.i(), h->fpos.i()));
  HIPCHK(hipMemcpyAsync(&nbnd, h->fpos.i() + nc, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(launch_rk_rows(nc, h->centers.i(), h->bflag.i(), h->fpos.i(), h->deg.i(), h->owned.i(),
                        h->degrow.i(), h->lid.i(), s));
  HIPCHK(scan(nc, h->degrow.i(), h->row_ptr.i()));
  HIPCHK(hipMemcpyAsync(&total, h->row_ptr.i() + nc, 4, hipMemcpyDeviceToHost, s));
  // ghosts in id order
  HIPCHK(scan((int)n, h->flag.i(), h->fpos.i()));
  HIPCHK(launch_rk_compact((int)n, h->flag.i(), h->fpos.i(), h->gid.i(), s));
  HIPCHK(hipMemcpyAsync(&ng, h->fpos.i() + n, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (const int rc = nl_refusal(&herr, false)) return rc;
  if (total < 0) return fail(E3GNN_ERR_GRAPH, "edge count exceeds int32");
  // ghosts by (owner, id): stable counting sort over blocks of 256
  const int nblk = std::max(1, (ng + 255) / 256);
  const size_t nh = (size_t)world * nblk;
  if (h->ghosts.ensure((size_t)std::max(ng, 1) * 4) != hipSuccess ||
      h->hist.ensure(nh * 4) != hipSuccess || h->hoff.ensure((nh + 1) * 4) != hipSuccess ||
      h->bsum.ensure((size_t)scan_blocks((int)nh) * 4) != hipSuccess)
    return fail(E3GNN_ERR_HIP, "rank-graph workspace allocation failed");
  HIPCHK(launch_rk_ghost_sort(false, ng, world, nblk, h->gid.i(), owner, h->hist.i(), nullptr, nc,
                              nullptr, nullptr, s));
  HIPCHK(scan((int)nh, h->hist.i(), h->hoff.i()));
  HIPCHK(launch_rk_ghost_sort(true, ng, world, nblk, h->gid.i(), owner, nullptr, h->hoff.i(), nc,
                              h->ghosts.i(), h->lid.i(), s));
  HIPCHK(launch_rk_recv(world, nblk, h->hoff.i(), (int64_t*)h->recv.p, s));
  HIPCHK(hipStreamSynchronize(s));
  h->n_local = nc;
  h->n_ghost = ng;
  h->world = world;
  h->E = total;
  h->rank_built = true;
  if (n_local) *n_local = nc;
  if (n_interior) *n_interior = nc - nbnd;
  if (n_ghost) *n_ghost = ng;
  if (n_edges) *n_edges = total;
  return E3GNN_OK;
}

int e3gnn_nlist_rank_fetch(e3gnn_nlist* h, int32_t* owned, int32_t* ghosts, int64_t* recv_counts,
                           int32_t* edge_center, int32_t* edge_nbr, int32_t* shift,
                           float* edge_vec, void* stream) {
  if (!h || !h->rank_built) return fail(E3GNN_ERR_ARG, "rank graph not built");
  if ((h->n_local > 0 && !owned) || (h->n_ghost > 0 && !ghosts) || !recv_counts ||
      (h->E > 0 && (!edge_center || !edge_nbr)))
    return fail(E3GNN_ERR_ARG, "null rank-graph output");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int* err = h->err.i();
  HIPCHK(hipMemsetAsync(err, 0, 4, s));
  if (h->n_local)
    HIPCHK(hipMemcpyAsync(owned, h->owned.p, (size_t)h->n_local * 4, hipMemcpyDeviceToDevice, s));
  if (h->n_ghost)
    HIPCHK(hipMemcpyAsync(ghosts, h->ghosts.p, (size_t)h->n_ghost * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(recv_counts, h->recv.p, (size_t)h->world * 8, hipMemcpyDeviceToDevice, s));
  // fill pass: one wave per local row (the centres in row order)
  NlRank rk{};
  rk.centers = h->owned.i();
  rk.lid = h->lid.i();
  HIPCHK(launch_nl_rank_search(true, (int)h->n_local, h->pos, h->hgeoms[0].G, h->f0.i(), h->bin.i(),
                               h->bin_start.i(), h->bin_atoms.i(), nullptr, h->row_ptr.i(),
                               edge_center, edge_nbr, shift, edge_vec, err, rk, s));
  return nl_fill_refusal(h, false, s);
}

// ------------------------------------------------------------------- batch
namespace {
// Argument rules of e3gnn_nlist_batch_build, checked before any device work
// (host only: no handle state, no HIP call).  Returns the refusal or "".
std::string nl_batch_args(bool have_handle, int64_t B, const int64_t* atom_ptr, const double* pos,
                          const double* cells, const int32_t* periodic, double cutoff) {
  if (B < 1 || B >= (int64_t)1 << 30) return "batch: the number of structures must be in [1, 2^30)";
  if (!atom_ptr) return "batch: null atom_ptr";
  if (!(cutoff > 0)) return "cutoff must be positive";
  if (!periodic) return "batch: null periodic flags";
  if (atom_ptr[0] != 0) return "batch: atom_ptr[0] must be 0";
  for (int64_t s = 0; s < B; ++s) {
    if (atom_ptr[s + 1] <= atom_ptr[s])
      return "batch: structure " + std::to_string(s) +
             " is empty or atom_ptr decreases (every structure needs at least one atom)";
    if (atom_ptr[s + 1] >= (int64_t)1 << 30) return "batch: atom count out of range (2^30)";
    if (periodic[s] != 0 && periodic[s] != 7)
      return "batch: structure " + std::to_string(s) +
             ": device neighbour list: pbc must be all true or all false";
    if (periodic[s] && !cells) return "batch: null cells";
  }
  if (!pos) return "null positions";
  if (!have_handle) return "null neighbour-list handle";
  return "";
}
}  // namespace

int e3gnn_nlist_batch_build(e3gnn_nlist* h, int64_t B, const int64_t* atom_ptr, const double* pos,
                            const double* cells, const int32_t* periodic, double cutoff,
                            int64_t* n_edges, void* stream) {
  {
    const std::string why = nl_batch_args(h != nullptr, B, atom_ptr, pos, cells, periodic, cutoff);
    if (!why.empty()) return fail(E3GNN_ERR_ARG, why);
  }
  hipStream_t s = (hipStream_t)stream;
  if (const int rc = nl_bin_atoms(h, true, B, atom_ptr, pos, cells, periodic, cutoff, s)) return rc;
  return nl_count_edges(h, true, n_edges, s);
}

int e3gnn_nlist_batch_fetch(e3gnn_nlist* h, int32_t* edge_center, int32_t* edge_nbr, int32_t* shift,
                            float* edge_vec, int64_t* edge_ptr, void* stream) {
  if (!h || !h->batch_built) return fail(E3GNN_ERR_ARG, "batched neighbour list not built");
  if (h->E > 0 && (!edge_center || !edge_nbr)) return fail(E3GNN_ERR_ARG, "null edge output");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  int* err = h->err.i();
  HIPCHK(hipMemsetAsync(err, 0, 16, s));
  HIPCHK(launch_nlb_search(true, (int)h->n, h->pos, (const NlGeomB*)h->geoms.p, h->batch.i(),
                           h->f0.i(), h->bin.i(), h->bin_start.i(), h->bin_atoms.i(), nullptr,
                           h->row_ptr.i(), edge_center, edge_nbr, shift, edge_vec, err, s));
  if (edge_ptr) HIPCHK(launch_nlb_edge_ptr((int)h->B, h->aptr.i(), h->row_ptr.i(), edge_ptr, s));
  return nl_fill_refusal(h, true, s);
}

}  // extern "C"
