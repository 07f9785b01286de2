// DFT-D3 behind the C ABI (include/e3gnn.h; kernels in d3.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "d3.h"
#include "dbuf.h"

using namespace e3gnn;

// ------------------------------------------------------------ DFT-D3
// PairD3 (sevenn/pair_e3gnn/pair_d3.cu) over host arrays, as LAMMPS hands
// them to PairD3::compute: settings/coeff -> e3gnn_d3_create, compute ->
// e3gnn_d3_compute (wrap into the cell :1182-1224, image lists :1026-1045 and
// :1230-1266, the four kernels of d3.hip, update :2003-2024).
struct e3gnn_d3 {
  int device = 0;
  D3Params p{};
  DBuf rcov, r2r4, r0ab, mxc, c6ab, cnref, x, type, bin_of, bin_start, off_v, off_c, cn, gw,
      c6tab, rows, forces, totals;
};

e3gnn_d3* e3gnn_d3_create(int device, int damping, const float* func, float rthr, float cn_thr,
                          int ntypes, const float* rcov, const float* r2r4, const float* r0ab,
                          const int32_t* mxc, const float* c6ab) {
  if (damping != 1 && damping != 2 && damping != 4) {
    fail(E3GNN_ERR_ARG, damping == 3 ? "damp_zerom is not implemented (nor by the reference, "
                                       "pair_d3.cu:1550-1553)"
                                     : "damping must be 1 (zero), 2 (bj) or 4 (bjm)");
    return nullptr;
  }
  if (ntypes <= 0 || !func || !rcov || !r2r4 || !r0ab || !mxc || !c6ab || !(rthr > 0) ||
      !(cn_thr > 0)) {
    fail(E3GNN_ERR_ARG, "d3: bad parameters");
    return nullptr;
  }
  for (int t = 0; t < ntypes; ++t)
    if (mxc[t] < 0 || mxc[t] > 5) {
      fail(E3GNN_ERR_ARG, "d3: mxc out of [0, 5]");
      return nullptr;
    }
  if (hipSetDevice(device) != hipSuccess) {
    fail(E3GNN_ERR_HIP, "hipSetDevice failed");
    return nullptr;
  }
  auto* h = new e3gnn_d3;
  h->device = device;
  const size_t nt = (size_t)ntypes;
  auto up = [](DBuf& b, const void* src, size_t bytes) {
    if (b.ensure(bytes) != hipSuccess) return false;
    return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(h->rcov, rcov, nt * 4) || !up(h->r2r4, r2r4, nt * 4) || !up(h->r0ab, r0ab, nt * nt * 4) ||
      !up(h->mxc, mxc, nt * 4) || !up(h->c6ab, c6ab, nt * nt * 75 * 4)) {
    delete h;
    fail(E3GNN_ERR_HIP, "d3: table upload failed");
    return nullptr;
  }
  D3Params& p = h->p;
  p.damping = damping == 1 ? 1 : 2;
  p.ntypes = ntypes;
  p.s6 = func[0];
  p.s8 = func[1];
  p.a1 = func[2];
  p.a2 = func[3];
  p.alp6 = func[4];
  p.alp8 = func[5];
  p.rthr = rthr;
  p.cn_thr = cn_thr;
  p.rcov = h->rcov.f();
  p.r2r4 = h->r2r4.f();
  p.r0ab = h->r0ab.f();
  p.mxc = h->mxc.i();
  p.c6ab = h->c6ab.f();
  // reference CN per (type, grid index), if the table is separable that way
  // (Grimme's data is: a reference CN belongs to an element's reference)
  std::vector<float> cr((size_t)ntypes * 5, 0.0f);
  std::vector<int> seen((size_t)ntypes * 5, 0);
  bool separable = true;
  for (int a = 0; a < ntypes; ++a)
    for (int b = 0; b < ntypes; ++b)
      for (int ia = 0; ia < 5; ++ia)
        for (int ib = 0; ib < 5; ++ib) {
          const float* e = c6ab + ((((size_t)a * ntypes + b) * 5 + ia) * 5 + ib) * 3;
          if (!(e[0] > 0.0f)) continue;
          const int ka = a * 5 + ia, kb = b * 5 + ib;
          if (seen[ka] && cr[ka] != e[1]) separable = false;
          if (seen[kb] && cr[kb] != e[2]) separable = false;
          cr[ka] = e[1];
          cr[kb] = e[2];
          seen[ka] = seen[kb] = 1;
        }
  p.cnref = nullptr;
  if (separable) {
    if (!up(h->cnref, cr.data(), cr.size() * 4)) {
      delete h;
      fail(E3GNN_ERR_HIP, "d3: table upload failed");
      return nullptr;
    }
    p.cnref = h->cnref.f();
  }
  return h;
}

void e3gnn_d3_free(e3gnn_d3* h) { delete h; }

namespace {
constexpr double D3_BIN_BOHR = 30.0;     // bin edge: swept 12-40 bohr on 8k-atom Si, 30 best
constexpr int64_t D3_C6TAB_MAX = 32768;  // n^2 C6 table up to 8.6 GB; beyond: C6 per item

// stencil of bin offsets covering a sphere of radius sqrt(thr): R = floor(rc /
// bin height) + 1 bins along each periodic axis (every (bin, image) pair once)
std::vector<int> d3_stencil(float thr, const double binh[3], const int* pbc,
                            const double lat[3][3], const int nb[3], double hd, bool prune) {
  const double rc = std::sqrt((double)thr);
  int R[3];
  for (int k = 0; k < 3; ++k) R[k] = pbc[k] ? (int)std::floor(rc / binh[k]) + 1 : 0;
  std::vector<int> off;
  for (int a = -R[0]; a <= R[0]; ++a)
    for (int b = -R[1]; b <= R[1]; ++b)
      for (int c = -R[2]; c <= R[2]; ++c) {
        if (prune) {
          // a cell whose centre is farther than rc + one full bin diagonal from
          // the home cell's centre cannot hold a partner of any atom of it
          double d[3];
          for (int k = 0; k < 3; ++k)
            d[k] = a * lat[0][k] / nb[0] + b * lat[1][k] / nb[1] + c * lat[2][k] / nb[2];
          if (std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > rc + 2.0 * hd + 1e-9) continue;
        }
        off.push_back(a);
        off.push_back(b);
        off.push_back(c);
      }
  return off;
}
}  // namespace

int e3gnn_d3_compute(e3gnn_d3* h, int64_t n, const double* pos, const double* cell,
                     const int32_t* pbc, const int32_t* type, double* energy, double* forces,
                     double* virial6, void* stream) {
  if (!h) return fail(E3GNN_ERR_ARG, "null d3 handle");
  if (n < 0 || n >= (int64_t)1 << 31) return fail(E3GNN_ERR_ARG, "d3: atom count out of range");
  if (n > 0 && (!pos || !type || !forces)) return fail(E3GNN_ERR_ARG, "d3: null input");
  if (!cell || !pbc || !energy || !virial6) return fail(E3GNN_ERR_ARG, "d3: null input");
  for (int64_t i = 0; i < n; ++i)
    if (type[i] < 0 || type[i] >= h->p.ntypes) return fail(E3GNN_ERR_ARG, "d3: type out of range");
  // lattice in bohr, rows a, b, c
  double lat[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) lat[r][c] = cell[3 * r + c] / D3_AU_TO_ANG;
  const double det = lat[0][0] * (lat[1][1] * lat[2][2] - lat[1][2] * lat[2][1]) -
                     lat[0][1] * (lat[1][0] * lat[2][2] - lat[1][2] * lat[2][0]) +
                     lat[0][2] * (lat[1][0] * lat[2][1] - lat[1][1] * lat[2][0]);
  if (!(std::fabs(det) > 1e-12)) return fail(E3GNN_ERR_ARG, "d3: singular cell");
  // inverse (columns of inv = reciprocal rows / det); frac = pos . inv
  double inv[3][3];
  inv[0][0] = (lat[1][1] * lat[2][2] - lat[1][2] * lat[2][1]) / det;
  inv[0][1] = (lat[0][2] * lat[2][1] - lat[0][1] * lat[2][2]) / det;
  inv[0][2] = (lat[0][1] * lat[1][2] - lat[0][2] * lat[1][1]) / det;
  inv[1][0] = (lat[1][2] * lat[2][0] - lat[1][0] * lat[2][2]) / det;
  inv[1][1] = (lat[0][0] * lat[2][2] - lat[0][2] * lat[2][0]) / det;
  inv[1][2] = (lat[0][2] * lat[1][0] - lat[0][0] * lat[1][2]) / det;
  inv[2][0] = (lat[1][0] * lat[2][1] - lat[1][1] * lat[2][0]) / det;
  inv[2][1] = (lat[0][1] * lat[2][0] - lat[0][0] * lat[2][1]) / det;
  inv[2][2] = (lat[0][0] * lat[1][1] - lat[0][1] * lat[1][0]) / det;
  // wrap (load_atom_info :1182-1224) and bin along the lattice vectors
  // (E3GNN_D3_BIN: bin edge in bohr, for tuning)
  const char* bin_env = std::getenv("E3GNN_D3_BIN");
  const double bin_w = bin_env ? std::max(2.0, std::atof(bin_env)) : D3_BIN_BOHR;
  double hgt[3], binh[3];
  int nb[3];
  bool all_pbc = true;
  for (int k = 0; k < 3; ++k) {
    const double* u = lat[(k + 1) % 3];
    const double* v = lat[(k + 2) % 3];
    const double c[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                         u[0] * v[1] - u[1] * v[0]};
    hgt[k] = std::fabs(c[0] * lat[k][0] + c[1] * lat[k][1] + c[2] * lat[k][2]) /
           std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    nb[k] = pbc[k] ? std::max(1, (int)(hgt[k] / bin_w)) : 1;
    binh[k] = hgt[k] / nb[k];
    all_pbc = all_pbc && pbc[k];
  }
  const int nbins = nb[0] * nb[1] * nb[2];
  std::vector<float> xw((size_t)n * 3);
  std::vector<int> bin((size_t)n), cnt(nbins + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    double p[3], a[3];
    int b[3];
    for (int d = 0; d < 3; ++d) p[d] = pos[3 * i + d] / D3_AU_TO_ANG;
    for (int k = 0; k < 3; ++k) {
      // row vector p = a . lat  ->  a = p . inv
      a[k] = p[0] * inv[0][k] + p[1] * inv[1][k] + p[2] * inv[2][k];
      if (pbc[k]) a[k] -= std::floor(a[k]);
      b[k] = pbc[k] ? std::min(nb[k] - 1, std::max(0, (int)(a[k] * nb[k]))) : 0;
    }
    for (int d = 0; d < 3; ++d)
      xw[3 * i + d] = (float)(a[0] * lat[0][d] + a[1] * lat[1][d] + a[2] * lat[2][d]);
    bin[i] = (b[0] * nb[1] + b[1]) * nb[2] + b[2];
    ++cnt[bin[i] + 1];
  }
  for (int b = 0; b < nbins; ++b) cnt[b + 1] += cnt[b];
  // counting sort by bin (stable: ascending atom id inside a bin)
  std::vector<int> perm((size_t)n), fill(cnt.begin(), cnt.end() - 1);
  for (int64_t i = 0; i < n; ++i) perm[fill[bin[i]]++] = (int)i;
  std::vector<float> xs((size_t)n * 4);
  std::vector<int> ts((size_t)n), bs((size_t)n);
  for (int64_t s2 = 0; s2 < n; ++s2) {
    const int i = perm[s2];
    for (int d = 0; d < 3; ++d) xs[4 * s2 + d] = xw[3 * i + d];
    std::memcpy(&xs[4 * s2 + 3], &type[i], 4);   // type bits in .w
    ts[s2] = type[i];
    bs[s2] = bin[i];
  }
  // half of the longest bin diagonal
  double hd = 0.0;
  for (int sa = -1; sa <= 1; sa += 2)
    for (int sb = -1; sb <= 1; sb += 2) {
      double d[3];
      for (int c = 0; c < 3; ++c)
        d[c] = lat[0][c] / nb[0] + sa * lat[1][c] / nb[1] + sb * lat[2][c] / nb[2];
      hd = std::max(hd, 0.5 * std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
    }
  const std::vector<int> ov = d3_stencil(h->p.rthr, binh, pbc, lat, nb, hd, all_pbc);
  const std::vector<int> oc = d3_stencil(h->p.cn_thr, binh, pbc, lat, nb, hd, all_pbc);
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t nn = (size_t)std::max<int64_t>(n, 1);
  // E3GNN_D3_NO_C6TAB=1: the per-item C6 path of large systems (tests)
  const char* no_tab = std::getenv("E3GNN_D3_NO_C6TAB");
  const bool use_tab = n <= D3_C6TAB_MAX && !(no_tab && no_tab[0] == '1');
  HIPCHK(h->x.ensure(nn * 16));
  HIPCHK(h->type.ensure(nn * 4));
  HIPCHK(h->bin_of.ensure(nn * 4));
  HIPCHK(h->bin_start.ensure((nbins + 1) * 4));
  HIPCHK(h->off_v.ensure(ov.size() * 4));
  HIPCHK(h->off_c.ensure(oc.size() * 4));
  HIPCHK(h->cn.ensure(nn * 8));
  if (use_tab) HIPCHK(h->c6tab.ensure(nn * nn * 8));
  HIPCHK(h->gw.ensure(nn * 80));
  HIPCHK(h->rows.ensure(nn * 64));
  HIPCHK(h->forces.ensure(nn * 24));
  HIPCHK(h->totals.ensure(7 * 8));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(h->x.p, xs.data(), n * 16, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->type.p, ts.data(), n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->bin_of.p, bs.data(), n * 4, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(h->bin_start.p, cnt.data(), (nbins + 1) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->off_v.p, ov.data(), ov.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->off_c.p, oc.data(), oc.size() * 4, hipMemcpyHostToDevice, s));
  D3Grid g{};
  for (int k = 0; k < 3; ++k) {
    g.nb[k] = nb[k];
    g.inv_nb[k] = (float)(1.0 / nb[k]);
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) g.lat[3 * r + c] = (float)lat[r][c];
  g.cull = all_pbc ? 1 : 0;
  const double rv = std::sqrt((double)h->p.rthr) + hd, rcn = std::sqrt((double)h->p.cn_thr) + hd;
  g.cull2_vdw = (float)(rv * rv * (1.0 + 1e-5));
  g.cull2_cn = (float)(rcn * rcn * (1.0 + 1e-5));
  g.bin_of = h->bin_of.i();
  g.bin_start = h->bin_start.i();
  g.off_vdw = h->off_v.i();
  g.off_cn = h->off_c.i();
  g.n_off_vdw = (int)(ov.size() / 3);
  g.n_off_cn = (int)(oc.size() / 3);
  HIPCHK(launch_d3(h->p, g, (int)n, (const float4*)h->x.p, h->type.i(), (double*)h->cn.p,
                   (double*)h->gw.p, use_tab ? (float2*)h->c6tab.p : nullptr, (double*)h->rows.p,
                   (double*)h->forces.p, (double*)h->totals.p, s));
  double tot[7];
  std::vector<double> fs((size_t)n * 3);
  HIPCHK(hipMemcpyAsync(tot, h->totals.p, 7 * 8, hipMemcpyDeviceToHost, s));
  if (n > 0) HIPCHK(hipMemcpyAsync(fs.data(), h->forces.p, n * 24, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t s2 = 0; s2 < n; ++s2)
    for (int d = 0; d < 3; ++d) forces[3 * perm[s2] + d] = fs[3 * s2 + d];
  *energy = tot[0];
  for (int k = 0; k < 6; ++k) virial6[k] = tot[1 + k];
  return E3GNN_OK;
}
