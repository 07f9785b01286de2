// e3gnn_batch_check -- the batched entry points of the C ABI from a native host
// (C++, no Python, no tensors in between): two displaced Si diamond cells
// (2x2x1 = 32 atoms and 2x2x2 = 64 atoms) evaluated
//   (1) one at a time: e3gnn_nlist_build / _fetch + e3gnn_energy_forces;
//   (2) as one batch:  e3gnn_nlist_batch_build / _fetch + e3gnn_energy_forces_batch.
// Prints one JSON line: whether the batch's graph is the two single graphs with
// the row offset (integer for integer), the largest differences of the
// energies (relative), forces (eV/A) and stresses (eV/A^3), and whether a
// second batched call reproduced the first bit for bit.  Exit status 0 when
// the graph is equal, the repeat bitwise and the differences are within
// 2e-6 / 1e-5 / 2e-6.
//
//   e3gnn_batch_check <weights.bin> <manifest.json> [seed]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "e3gnn.h"

namespace {

void die(const char* what) {
  std::fprintf(stderr, "e3gnn_batch_check: %s: %s\n", what, e3gnn_last_error());
  std::exit(1);
}

#define HIPOK(x)                                                                      \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                           \
      std::fprintf(stderr, "e3gnn_batch_check: %s: %s\n", #x, hipGetErrorString(e_)); \
      std::exit(1);                                                                   \
    }                                                                                 \
  } while (0)

// species index of `sym` in the manifest's chemical_symbols
int species_index(const std::string& manifest, const std::string& sym) {
  std::ifstream f(manifest);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string s = ss.str();
  const size_t k = s.find("\"chemical_symbols\"");
  if (k == std::string::npos) return -1;
  const size_t a = s.find('[', k), b = s.find(']', a);
  int idx = 0;
  for (size_t p = a; p < b;) {
    const size_t q0 = s.find('"', p);
    if (q0 == std::string::npos || q0 > b) break;
    const size_t q1 = s.find('"', q0 + 1);
    if (s.compare(q0 + 1, q1 - q0 - 1, sym) == 0) return idx;
    ++idx;
    p = q1 + 1;
  }
  return -1;
}

template <class T>
T* to_device(const std::vector<T>& v) {
  T* d = nullptr;
  HIPOK(hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIPOK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
template <class T>
std::vector<T> to_host(const T* d, size_t n) {
  std::vector<T> v(n);
  if (n) HIPOK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return v;
}
template <class T>
T* device_array(size_t n) {
  T* d = nullptr;
  HIPOK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  return d;
}

struct Cell {
  int n = 0;
  double cell[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<double> pos;
};

// Si diamond, cx x cy x cz conventional cells, N(0, 0.05 A) displacements
Cell si_cell(int cx, int cy, int cz, std::mt19937& rng) {
  const double a0 = 5.43;
  const double basis[8][3] = {{0, 0, 0},       {0, .5, .5},     {.5, 0, .5},     {.5, .5, 0},
                              {.25, .25, .25}, {.25, .75, .75}, {.75, .25, .75}, {.75, .75, .25}};
  std::normal_distribution<double> gauss(0.0, 0.05);
  Cell c;
  c.n = 8 * cx * cy * cz;
  c.cell[0] = cx * a0;
  c.cell[4] = cy * a0;
  c.cell[8] = cz * a0;
  for (int i = 0; i < cx; ++i)
    for (int j = 0; j < cy; ++j)
      for (int k = 0; k < cz; ++k)
        for (int b = 0; b < 8; ++b) {
          const double f[3] = {i + basis[b][0], j + basis[b][1], k + basis[b][2]};
          for (int d = 0; d < 3; ++d) c.pos.push_back(f[d] * a0 + gauss(rng));
        }
  return c;
}

struct Result {
  std::vector<int32_t> center, nbr, shift;
  std::vector<float> energy, forces, virial;
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s weights.bin manifest.json [seed]\n", argv[0]);
    return 2;
  }
  const unsigned seed = argc > 3 ? (unsigned)std::atoi(argv[3]) : 0u;
  const int si = species_index(argv[2], "Si");
  if (si < 0) {
    std::fprintf(stderr, "e3gnn_batch_check: Si not in the manifest\n");
    return 1;
  }
  e3gnn_model* model = e3gnn_load(argv[1], argv[2], 0);
  if (!model) die("e3gnn_load");
  int nspecies = 0, nlayers = 0, comm = 0;
  float cutoff = 0.f;
  if (e3gnn_model_info(model, &nspecies, &cutoff, &nlayers, &comm)) die("e3gnn_model_info");
  e3gnn_ctx* ctx = e3gnn_ctx_create(model);
  if (!ctx) die("e3gnn_ctx_create");
  e3gnn_nlist* nl = e3gnn_nlist_create(0);
  if (!nl) die("e3gnn_nlist_create");

  std::mt19937 rng(seed);
  const Cell cells[2] = {si_cell(2, 2, 1, rng), si_cell(2, 2, 2, rng)};
  const int pbc[3] = {1, 1, 1};

  // (1) one structure at a time
  Result one[2];
  for (int k = 0; k < 2; ++k) {
    const Cell& c = cells[k];
    double* pos = to_device(c.pos);
    int32_t* type = to_device(std::vector<int32_t>(c.n, si));
    int64_t E = 0;
    if (e3gnn_nlist_build(nl, c.n, pos, c.cell, pbc, cutoff, &E, nullptr)) die("e3gnn_nlist_build");
    int32_t* center = device_array<int32_t>(E);
    int32_t* nbr = device_array<int32_t>(E);
    int32_t* shift = device_array<int32_t>(3 * E);
    float* vec = device_array<float>(3 * E);
    if (e3gnn_nlist_fetch(nl, center, nbr, shift, vec, nullptr)) die("e3gnn_nlist_fetch");
    float* energy = device_array<float>(1);
    float* forces = device_array<float>(3 * (size_t)c.n);
    float* virial = device_array<float>(6);
    if (e3gnn_energy_forces(ctx, c.n, E, type, center, nbr, vec, energy, nullptr, forces, virial,
                            nullptr, nullptr))
      die("e3gnn_energy_forces");
    HIPOK(hipDeviceSynchronize());
    one[k] = {to_host(center, E),  to_host(nbr, E),       to_host(shift, 3 * E),
              to_host(energy, 1), to_host(forces, 3 * (size_t)c.n), to_host(virial, 6)};
    for (void* p : {(void*)pos, (void*)type, (void*)center, (void*)nbr, (void*)shift, (void*)vec,
                    (void*)energy, (void*)forces, (void*)virial})
      HIPOK(hipFree(p));
  }

  // (2) the two as one batch
  const int n = cells[0].n + cells[1].n;
  const int64_t atom_ptr[3] = {0, cells[0].n, n};
  std::vector<double> hpos(cells[0].pos);
  hpos.insert(hpos.end(), cells[1].pos.begin(), cells[1].pos.end());
  double hcells[18];
  std::memcpy(hcells, cells[0].cell, sizeof(cells[0].cell));
  std::memcpy(hcells + 9, cells[1].cell, sizeof(cells[1].cell));
  const int32_t periodic[2] = {7, 7};
  double* pos = to_device(hpos);
  int32_t* type = to_device(std::vector<int32_t>(n, si));
  int32_t* aptr = to_device(std::vector<int32_t>{0, cells[0].n, n});
  int64_t E = 0;
  if (e3gnn_nlist_batch_build(nl, 2, atom_ptr, pos, hcells, periodic, cutoff, &E, nullptr))
    die("e3gnn_nlist_batch_build");
  int32_t* center = device_array<int32_t>(E);
  int32_t* nbr = device_array<int32_t>(E);
  int32_t* shift = device_array<int32_t>(3 * E);
  float* vec = device_array<float>(3 * E);
  int64_t* edge_ptr = device_array<int64_t>(3);
  if (e3gnn_nlist_batch_fetch(nl, center, nbr, shift, vec, edge_ptr, nullptr))
    die("e3gnn_nlist_batch_fetch");
  Result got[2];
  for (int rep = 0; rep < 2; ++rep) {
    float* energy = device_array<float>(2);
    float* forces = device_array<float>(3 * (size_t)n);
    float* virial = device_array<float>(12);
    if (e3gnn_energy_forces_batch(ctx, n, E, 2, aptr, type, center, nbr, vec, energy, nullptr,
                                  forces, virial, nullptr, nullptr))
      die("e3gnn_energy_forces_batch");
    HIPOK(hipDeviceSynchronize());
    got[rep] = {to_host(center, E),  to_host(nbr, E),       to_host(shift, 3 * E),
                to_host(energy, 2), to_host(forces, 3 * (size_t)n), to_host(virial, 12)};
    for (void* p : {(void*)energy, (void*)forces, (void*)virial}) HIPOK(hipFree(p));
  }
  const std::vector<int64_t> eptr = to_host(edge_ptr, 3);

  // compare
  const Result& b = got[0];
  const int64_t E0 = (int64_t)one[0].center.size(), E1 = (int64_t)one[1].center.size();
  bool graph_equal = E == E0 + E1 && eptr[0] == 0 && eptr[1] == E0 && eptr[2] == E;
  for (int k = 0; graph_equal && k < 2; ++k) {
    const int64_t e0 = k ? E0 : 0, a0 = k ? cells[0].n : 0;
    for (size_t e = 0; e < one[k].center.size(); ++e) {
      graph_equal &= b.center[e0 + e] == one[k].center[e] + a0 && b.nbr[e0 + e] == one[k].nbr[e] + a0;
      for (int d = 0; d < 3; ++d) graph_equal &= b.shift[3 * (e0 + e) + d] == one[k].shift[3 * e + d];
    }
  }
  double de = 0, df = 0, ds = 0;
  for (int k = 0; k < 2; ++k) {
    const int a0 = k ? cells[0].n : 0;
    const double vol = cells[k].cell[0] * cells[k].cell[4] * cells[k].cell[8];
    de = std::max(de, std::fabs((double)b.energy[k] - one[k].energy[0]) / std::fabs(one[k].energy[0]));
    for (int q = 0; q < 3 * cells[k].n; ++q)
      df = std::max(df, std::fabs((double)b.forces[3 * a0 + q] - one[k].forces[q]));
    for (int q = 0; q < 6; ++q)
      ds = std::max(ds, std::fabs((double)b.virial[6 * k + q] - one[k].virial[q]) / vol);
  }
  const bool repeat_bitwise =
      got[0].energy.size() == got[1].energy.size() &&
      !std::memcmp(got[0].energy.data(), got[1].energy.data(), got[0].energy.size() * 4) &&
      !std::memcmp(got[0].forces.data(), got[1].forces.data(), got[0].forces.size() * 4) &&
      !std::memcmp(got[0].virial.data(), got[1].virial.data(), got[0].virial.size() * 4);
  std::printf(
      "{\"n_atoms\": [%d, %d], \"n_edges\": [%lld, %lld], \"graph_equal\": %s, "
      "\"energy\": [%.9g, %.9g], \"energy_single\": [%.9g, %.9g], \"max_energy_rel_diff\": %.3e, "
      "\"max_force_diff\": %.3e, \"max_stress_diff\": %.3e, \"repeat_bitwise\": %s}\n",
      cells[0].n, cells[1].n, (long long)E0, (long long)E1, graph_equal ? "true" : "false",
      b.energy[0], b.energy[1], one[0].energy[0], one[1].energy[0], de, df, ds,
      repeat_bitwise ? "true" : "false");
  for (void* p : {(void*)pos, (void*)type, (void*)aptr, (void*)center, (void*)nbr, (void*)shift,
                  (void*)vec, (void*)edge_ptr})
    HIPOK(hipFree(p));
  e3gnn_nlist_free(nl);
  e3gnn_ctx_free(ctx);
  e3gnn_free(model);
  return graph_equal && repeat_bitwise && de <= 2e-6 && df <= 1e-5 && ds <= 2e-6 ? 0 : 1;
}
