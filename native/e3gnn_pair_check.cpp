// e3gnn_pair_check -- the LAMMPS pair styles of native/lammps/ (the ADAPTOR
// sources themselves: pair_e3gnn_hip.cpp, pair_e3gnn_parallel_hip.cpp) run
// inside a mini-LAMMPS scaffold (native/lammps_mock/: Atom, NeighList, Pair and
// a CommBrick emulation whose ranks are threads of this process).
//
//   (0) reference: the library's device neighbour list + e3gnn_energy_forces
//       on the whole periodic box (atoms in tag order);
//   (1) pair_style e3gnn (PairE3GNN, pair_e3gnn.cpp:72-275) on one rank whose
//       ghosts come from CommBrick's six self swaps;
//   (2) pair_style e3gnn/parallel (PairE3GNNParallel, pair_e3gnn_parallel.cpp:
//       207-933) on px x py x pz bricks: CommBrick::borders() builds each
//       rank's ghosts swap by swap (corner atoms relayed through the ranks of
//       earlier dimensions), the pair's comm_preprocess runs the "false"
//       forward_comm through the *_init hooks, every layer's features go out
//       through forward_comm(pair) and the gradients come back through
//       reverse_comm(pair) (the reference's comm_brick.cpp:1057-1120), and the
//       ghost forces reach their owners through LAMMPS' own newton-on reverse
//       communication.
// Prints one JSON line: energies, largest force / virial differences, the comm
// counters (extra rows, relays, zero returns, trash rows) and whether a second
// compute() reproduced the first bit for bit.  With --vatom both styles also
// run with VIRIAL_ATOM set, the scaffold reverse-communicates Pair::vatom as
// compute stress/atom does, and each style's object gains vatom_max_diff
// (against the library's e3gnn_atom_virial on the whole box, matched by tag),
// vatom_sum_max_diff (sum over atoms against the style's global virial),
// vatom_max_ends (most edge ends on one atom) and vatom_repeat_bitwise.
// With --graph-device style (1) then runs again on one rank in both graph
// modes (pair_style e3gnn graph host|device) on the same atoms and list, and
// the line gains the object graph_device: edges / edges_host, energy_, forces_
// and virial_bits_equal (memcmp against the host mode), repeat_bitwise, and a
// reuse leg -- every atom and image moved by up to 0.4 A per component keyed
// by its tag, neighbor->ago = 1, the list left alone -- as reuse_edges,
// reuse_edges_changed and reuse_bits_equal.  --time K runs style (1) only and
// prints, per mode (host; device with the list re-uploaded; device with the
// list reused), the median and range of K alternating compute() times in ms.
// With --parallel-graph-device style (2) runs again on the requested grid in
// both graph modes (pair_style e3gnn/parallel graph host|device) on the same
// atoms and lists, and the line gains the object parallel_graph_device: per
// rank edges / edges_host, ghost_rows / ghost_rows_host and reuse_edges;
// graph_bits_equal (memcmp of center, nbr, vec, type and the row -> atom map,
// rank by rank), energy_, forces_ and virial_bits_equal, comm_equal (the comm
// counters of both modes), repeat_bitwise, and the reuse leg of --graph-device
// as reuse_edges_changed and reuse_bits_equal.  With --time K it runs style
// (2) only, the ranks as threads sharing one GPU, and prints rank 0's times of
// build() + comm_preprocess + compute() per mode in the same alternation.
//
//   e3gnn_pair_check <model dir> <structure> <px> <py> <pz> [seed] [--gpu-aware] [--vatom]
//                    [--graph-device] [--parallel-graph-device] [--time K]
//   structure: si:<cells> (displaced Si diamond) or a file
//              "n \n 9 cell values (rows = lattice vectors) \n symbol x y z ..."
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "atom.h"
#include "comm_brick.h"
#include "domain.h"
#include "e3gnn.h"
#include "error.h"
#include "force.h"
#include "memory.h"
#include "neigh_list.h"
#include "neighbor.h"
#include "pair_e3gnn_core.h"
#include "pair_e3gnn_hip.h"
#include "pair_e3gnn_parallel.h"

using namespace LAMMPS_NS;

namespace {

constexpr double SKIN = 1.0;

struct Structure {
  int n = 0;
  double cell[9];
  std::vector<double> pos;            // n x 3
  std::vector<std::string> symbol;    // per atom
  std::vector<std::string> elements;  // LAMMPS type k + 1 = elements[k]
  std::vector<int> type;              // 1-based
  std::vector<tagint> tag;            // atom a carries tag[a]
};

Structure load_structure(const std::string& spec, std::mt19937& rng) {
  Structure s;
  if (spec.rfind("si:", 0) == 0) {
    const int cells = std::atoi(spec.c_str() + 3);
    const double a0 = 5.43, L = cells * a0;
    const double basis[8][3] = {{0, 0, 0},       {0, .5, .5},     {.5, 0, .5},     {.5, .5, 0},
                                {.25, .25, .25}, {.25, .75, .75}, {.75, .25, .75}, {.75, .75, .25}};
    std::normal_distribution<double> disp(0.0, 0.1);
    for (int i = 0; i < cells; ++i)
      for (int j = 0; j < cells; ++j)
        for (int k = 0; k < cells; ++k)
          for (int b = 0; b < 8; ++b) {
            s.pos.push_back((i + basis[b][0]) * a0 + disp(rng));
            s.pos.push_back((j + basis[b][1]) * a0 + disp(rng));
            s.pos.push_back((k + basis[b][2]) * a0 + disp(rng));
            s.symbol.push_back("Si");
          }
    s.n = 8 * cells * cells * cells;
    const double c[9] = {L, 0, 0, 0, L, 0, 0, 0, L};
    std::copy(c, c + 9, s.cell);
  } else {
    std::ifstream f(spec);
    if (!f) throw std::runtime_error("cannot open " + spec);
    f >> s.n;
    for (double& v : s.cell) f >> v;
    s.pos.resize(3 * (size_t)s.n);
    s.symbol.resize(s.n);
    for (int a = 0; a < s.n; ++a) f >> s.symbol[a] >> s.pos[3 * a] >> s.pos[3 * a + 1] >> s.pos[3 * a + 2];
    if (!f) throw std::runtime_error("malformed structure file " + spec);
  }
  for (int a = 0; a < s.n; ++a) {
    auto it = std::find(s.elements.begin(), s.elements.end(), s.symbol[a]);
    if (it == s.elements.end()) {
      s.elements.push_back(s.symbol[a]);
      it = s.elements.end() - 1;
    }
    s.type.push_back((int)(it - s.elements.begin()) + 1);
  }
  s.tag.resize(s.n);
  for (int a = 0; a < s.n; ++a) s.tag[a] = a + 1;
  std::shuffle(s.tag.begin(), s.tag.end(), rng);   // LAMMPS tags != file order
  return s;
}

struct RankOut {
  double energy = 0, virial[6] = {0, 0, 0, 0, 0, 0}, eatom = 0;
  std::vector<std::pair<tagint, std::array<double, 3>>> f;   // owned atoms
  std::vector<std::pair<tagint, std::array<double, 6>>> vatom;   // owned atoms (--vatom)
  e3gnn_pair::CommMaps::Stats st;
  int nghost = 0, graph = 0;
  bool same_again = true, vatom_same_again = true;
  std::string err;
};

// one emulated MPI rank: LAMMPS-style setup, pair_style / pair_coeff, then
// `repeat` force evaluations (each: borders, neighbour list, compute, reverse comm)
void run_rank(const Structure& S, const std::string& model_dir, const int grid[3], int me, World* world,
              bool parallel, int repeat, bool want_vatom, std::mutex* load_mutex, RankOut* out) {
  LAMMPS lmp;
  Memory mem;
  Error err;
  Atom atom;
  Neighbor neigh;
  Force force;
  Domain dom;
  lmp.memory = &mem;
  lmp.error = &err;
  lmp.atom = &atom;
  lmp.neighbor = &neigh;
  lmp.force = &force;
  lmp.domain = &dom;
  CommBrick comm(&lmp, world, me, grid);
  lmp.comm = &comm;
  dom.set_cell(S.cell);
  neigh.skin = SKIN;
  // owned atoms: wrapped lamda inside this brick
  for (int a = 0; a < S.n; ++a) {
    double s[3], x[3];
    dom.x2lamda(&S.pos[3 * a], s);
    bool mine = true;
    for (int d = 0; d < 3; ++d) {
      s[d] -= std::floor(s[d]);
      if (s[d] >= 1.0) s[d] -= 1.0;
      const int c = std::min(grid[d] - 1, (int)(s[d] * grid[d]));
      mine = mine && c == comm.myloc[d];
    }
    if (!mine) continue;
    dom.lamda2x(s, x);
    atom.add(x, s, S.tag[a], S.type[a]);
  }
  atom.nlocal = (int)atom.tags.size();
  atom.natoms = S.n;
  atom.ntypes = (int)S.elements.size();
  atom.sync();

  std::unique_ptr<Pair> pair;
  std::vector<std::string> args = {"*", "*"};
  if (parallel) args.push_back("4");   // segment count (ignored)
  args.push_back(model_dir);
  for (const auto& e : S.elements) args.push_back(e);
  std::vector<char*> argv;
  for (auto& a : args) argv.push_back(&a[0]);
  {
    std::lock_guard<std::mutex> lk(*load_mutex);
    if (parallel) pair.reset(new PairE3GNNParallel(&lmp));
    else pair.reset(new PairE3GNN(&lmp));
    pair->settings(0, nullptr);
    pair->coeff((int)argv.size(), argv.data());
  }
  pair->init_style();
  if (!neigh.requested_full) throw std::runtime_error("pair style did not request a full list");
  const double cut = pair->init_one(1, 1);
  comm.setup(cut + SKIN);
  NeighList list;
  std::vector<std::vector<double>> first;
  std::vector<double> first_vatom;
  for (int it = 0; it < repeat; ++it) {
    comm.borders();
    neigh.build_full(&atom, cut, &list);
    pair->init_list(0, &list);
    std::fill(atom.fs.begin(), atom.fs.end(), 0.0);
    pair->compute(1 | 2, want_vatom ? 1 | 4 : 1);   // VIRIAL_PAIR (| VIRIAL_ATOM)
    comm.reverse_comm();   // ghost forces onto their owners (newton on)
    std::vector<double> f(atom.fs.begin(), atom.fs.begin() + 3 * (size_t)atom.nlocal);
    std::vector<double> va;
    if (want_vatom) {
      // what compute stress/atom does before it reads vatom (newton on)
      comm.reverse_comm_peratom(pair->vatom, 6);
      for (int i = 0; i < atom.nlocal; ++i) va.insert(va.end(), pair->vatom[i], pair->vatom[i] + 6);
    }
    if (it == 0) {
      out->energy = pair->eng_vdwl;
      for (int k = 0; k < 6; ++k) out->virial[k] = pair->virial[k];
      for (int i = 0; i < atom.nlocal; ++i) {
        out->eatom += pair->eatom[i];
        out->f.push_back({atom.tag[i], {f[3 * i], f[3 * i + 1], f[3 * i + 2]}});
      }
      for (int i = 0; want_vatom && i < atom.nlocal; ++i) {
        std::array<double, 6> w;
        std::copy(va.begin() + 6 * (size_t)i, va.begin() + 6 * (size_t)i + 6, w.begin());
        out->vatom.push_back({atom.tag[i], w});
      }
      first_vatom = va;
      out->nghost = atom.nghost;
      if (parallel) {
        auto* pp = static_cast<PairE3GNNParallel*>(pair.get());
        out->st = pp->comm_maps()->stats();
      }
      first.push_back(f);
    } else {
      out->same_again = out->same_again && f == first[0] && pair->eng_vdwl == out->energy;
      out->vatom_same_again = out->vatom_same_again && va == first_vatom;
    }
  }
}

struct RunOut {
  double energy = 0, virial[6] = {0, 0, 0, 0, 0, 0}, eatom = 0;
  std::vector<double> f_tag;   // by tag - 1
  std::vector<double> vatom_tag;   // by tag - 1, LAMMPS order (--vatom)
  e3gnn_pair::CommMaps::Stats st;
  int64_t ghosts = 0;
  bool same_again = true, vatom_same_again = true;
};

RunOut run(const Structure& S, const std::string& dir, const int grid[3], bool parallel, int repeat,
           bool want_vatom) {
  const int P = grid[0] * grid[1] * grid[2];
  World world(P);
  std::mutex load_mutex;
  std::vector<RankOut> outs(P);
  std::vector<std::thread> th;
  for (int r = 0; r < P; ++r)
    th.emplace_back([&, r] {
      try {
        if (hipSetDevice(0) != hipSuccess) throw std::runtime_error("hipSetDevice");
        run_rank(S, dir, grid, r, &world, parallel, repeat, want_vatom, &load_mutex, &outs[r]);
      } catch (const std::exception& e) {
        outs[r].err = e.what();
        world.abort();
      }
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < P; ++r)
    if (!outs[r].err.empty() && outs[r].err != "world aborted")
      throw std::runtime_error("rank " + std::to_string(r) + ": " + outs[r].err);
  RunOut R;
  R.f_tag.assign(3 * (size_t)S.n, 0.0);
  if (want_vatom) R.vatom_tag.assign(6 * (size_t)S.n, 0.0);
  std::vector<int> seen(S.n, 0);
  for (auto& o : outs) {
    R.energy += o.energy;
    R.eatom += o.eatom;
    for (int k = 0; k < 6; ++k) R.virial[k] += o.virial[k];
    for (auto& [t, f] : o.f) {
      seen[t - 1]++;
      for (int k = 0; k < 3; ++k) R.f_tag[3 * (t - 1) + k] = f[k];
    }
    for (auto& [t, w] : o.vatom)
      for (int k = 0; k < 6; ++k) R.vatom_tag[6 * (t - 1) + k] = w[k];
    R.ghosts += o.nghost;
    R.same_again = R.same_again && o.same_again;
    R.vatom_same_again = R.vatom_same_again && o.vatom_same_again;
    R.st.swaps += o.st.swaps;
    R.st.sent += o.st.sent;
    R.st.relayed += o.st.relayed;
    R.st.extra_rows += o.st.extra_rows;
    R.st.zero_sends += o.st.zero_sends;
    R.st.trash_forward += o.st.trash_forward;
    R.st.trash_reverse += o.st.trash_reverse;
  }
  for (int a = 0; a < S.n; ++a)
    if (seen[a] != 1) throw std::runtime_error("the bricks do not partition the atoms");
  return R;
}

// Style (1) on one rank, kept alive between force evaluations (--graph-device,
// --time): the setup of run_rank, one list build, then compute() as often as
// the caller likes, in either graph mode, with neighbor->ago in its hands.
struct SerialRig {
  LAMMPS lmp;
  Memory mem;
  Error err;
  Atom atom;
  Neighbor neigh;
  Force force;
  Domain dom;
  World world{1};
  std::unique_ptr<CommBrick> comm;
  std::unique_ptr<PairE3GNN> pair;
  NeighList list;
  struct Result {
    double energy = 0, virial[6] = {0, 0, 0, 0, 0, 0};
    std::vector<double> f;   // owned atoms
    long long edges = 0;
    bool same_bits(const Result& o) const {
      return !std::memcmp(&energy, &o.energy, 8) && !std::memcmp(virial, o.virial, 48) &&
             f.size() == o.f.size() && !std::memcmp(f.data(), o.f.data(), f.size() * 8);
    }
  };

  SerialRig(const Structure& S, const std::string& model_dir) {
    const int one[3] = {1, 1, 1};
    lmp.memory = &mem;
    lmp.error = &err;
    lmp.atom = &atom;
    lmp.neighbor = &neigh;
    lmp.force = &force;
    lmp.domain = &dom;
    comm.reset(new CommBrick(&lmp, &world, 0, one));
    lmp.comm = comm.get();
    dom.set_cell(S.cell);
    neigh.skin = SKIN;
    for (int a = 0; a < S.n; ++a) {
      double s[3], x[3];
      dom.x2lamda(&S.pos[3 * a], s);
      for (int d = 0; d < 3; ++d) {
        s[d] -= std::floor(s[d]);
        if (s[d] >= 1.0) s[d] -= 1.0;
      }
      dom.lamda2x(s, x);
      atom.add(x, s, S.tag[a], S.type[a]);
    }
    atom.nlocal = (int)atom.tags.size();
    atom.natoms = S.n;
    atom.ntypes = (int)S.elements.size();
    atom.sync();
    std::vector<std::string> args = {"*", "*", model_dir};
    for (const auto& e : S.elements) args.push_back(e);
    std::vector<char*> argv;
    for (auto& a : args) argv.push_back(&a[0]);
    pair.reset(new PairE3GNN(&lmp));
    pair->settings(0, nullptr);
    pair->coeff((int)argv.size(), argv.data());
    pair->init_style();
    const double cut = pair->init_one(1, 1);
    comm->setup(cut + SKIN);
    comm->borders();
    neigh.build_full(&atom, cut, &list);
    pair->init_list(0, &list);
  }
  void graph(const char* where) {
    std::string a = "graph", b = where;
    char* argv[2] = {&a[0], &b[0]};
    pair->settings(2, argv);
  }
  void zero_forces() { std::fill(atom.fs.begin(), atom.fs.end(), 0.0); }
  Result compute(int ago) {
    neigh.ago = ago;
    zero_forces();
    pair->compute(1 | 2, 1);
    Result r;
    r.energy = pair->eng_vdwl;
    std::copy(pair->virial, pair->virial + 6, r.virial);
    r.f.assign(atom.fs.begin(), atom.fs.begin() + 3 * (size_t)atom.nlocal);
    r.edges = pair->last_edges();
    return r;
  }
  // every atom, owned or ghost, moved by a displacement keyed by its tag
  // (|d| <= amp per component): every image of an atom moves alike
  void displace(unsigned seed, double amp) {
    const int nt = atom.nlocal + atom.nghost;
    for (int a = 0; a < nt; ++a) {
      std::mt19937 r(seed * 7919u + (unsigned)atom.tag[a]);
      std::uniform_real_distribution<double> u(-amp, amp);
      for (int k = 0; k < 3; ++k) atom.x[a][k] += u(r);
    }
  }
};

// --graph-device: the keys of the "graph_device" object
std::string graph_device_keys(const Structure& S, const std::string& dir, unsigned seed) {
  SerialRig rig(S, dir);
  const auto host = rig.compute(0);
  rig.graph("device");
  const auto dev = rig.compute(0), dev2 = rig.compute(0);
  // reuse leg: the atoms move, the list stays (ago = 1); device first, so that
  // the step really reuses the list uploaded above
  rig.displace(seed, 0.4);
  const auto rdev = rig.compute(1);
  rig.graph("host");
  const auto rhost = rig.compute(1);
  auto tf = [](bool b) { return b ? "true" : "false"; };
  char buf[512];
  std::snprintf(buf, sizeof(buf),
                ", \"graph_device\": {\"edges\": %lld, \"edges_host\": %lld, \"energy_bits_equal\": %s, "
                "\"forces_bits_equal\": %s, \"virial_bits_equal\": %s, \"repeat_bitwise\": %s, "
                "\"reuse_edges\": %lld, \"reuse_edges_changed\": %s, \"reuse_bits_equal\": %s}",
                dev.edges, host.edges, tf(!std::memcmp(&dev.energy, &host.energy, 8)),
                tf(dev.f.size() == host.f.size() && !std::memcmp(dev.f.data(), host.f.data(), dev.f.size() * 8)),
                tf(!std::memcmp(dev.virial, host.virial, 48)), tf(dev.same_bits(dev2)), rdev.edges,
                tf(rdev.edges != dev.edges), tf(rdev.same_bits(rhost) && rdev.edges == rhost.edges));
  return buf;
}

// median and range, and the rounds themselves, of a --time series as JSON
std::string stats(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  const size_t m = v.size();
  const double med = m % 2 ? v[m / 2] : 0.5 * (v[m / 2 - 1] + v[m / 2]);
  char buf[96];
  std::snprintf(buf, sizeof(buf), "{\"median\": %.3f, \"min\": %.3f, \"max\": %.3f}", med, v.front(), v.back());
  return std::string(buf);
}
std::string rounds(const std::vector<double>& v) {
  std::string s = "[";
  char buf[32];
  for (size_t k = 0; k < v.size(); ++k) {
    std::snprintf(buf, sizeof(buf), "%s%.3f", k ? ", " : "", v[k]);
    s += buf;
  }
  return s + "]";
}

// --time K: style (1) only; per round host mode, device mode with the list
// re-uploaded (ago = 0), device mode with the list reused (ago = 1)
int time_graph_modes(const Structure& S, const std::string& dir, int K) {
  using clk = std::chrono::steady_clock;
  SerialRig rig(S, dir);
  auto timed = [&](int ago) {
    rig.neigh.ago = ago;
    rig.zero_forces();
    const auto t0 = clk::now();
    rig.pair->compute(1, 1);   // ends in a stream synchronise
    return std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  };
  for (int w = 0; w < 2; ++w) timed(0);
  rig.graph("device");
  for (int w = 0; w < 2; ++w) timed(0);
  for (int w = 0; w < 2; ++w) timed(1);
  std::vector<double> t[3];
  int wins = 0;
  for (int k = 0; k < K; ++k) {
    rig.graph("host");
    t[0].push_back(timed(0));
    rig.graph("device");
    t[1].push_back(timed(0));
    t[2].push_back(timed(1));
    wins += t[2].back() < t[0].back();
  }
  std::printf("{\"n_atoms\": %d, \"ghosts\": %d, \"edges\": %lld, \"rounds\": %d, \"host_ms\": %s, "
              "\"device_new_list_ms\": %s, \"device_reused_list_ms\": %s, \"reused_beats_host_rounds\": %d, "
              "\"host_rounds_ms\": %s, \"device_new_list_rounds_ms\": %s, \"device_reused_list_rounds_ms\": %s}\n",
              S.n, rig.atom.nghost, rig.pair->last_edges(), K, stats(t[0]).c_str(), stats(t[1]).c_str(),
              stats(t[2]).c_str(), wins, rounds(t[0]).c_str(), rounds(t[1]).c_str(), rounds(t[2]).c_str());
  return 0;
}

// Style (2) on one emulated rank, kept alive between force evaluations
// (--parallel-graph-device): the setup of run_rank, one borders() and one list
// build, then compute() as often as the caller likes, in either graph mode.
// Every rank of the grid runs the same sequence (the exchanges meet in World).
struct ParallelRig {
  LAMMPS lmp;
  Memory mem;
  Error err;
  Atom atom;
  Neighbor neigh;
  Force force;
  Domain dom;
  std::unique_ptr<CommBrick> comm;
  std::unique_ptr<PairE3GNNParallel> pair;
  NeighList list;
  struct Result {
    double energy = 0, virial[6] = {0, 0, 0, 0, 0, 0};
    std::vector<double> f;   // owned atoms, after the reverse communication
    long long edges = 0, ghost_rows = 0;
    std::vector<int32_t> center, nbr, type;
    std::vector<float> vec;
    std::vector<int> row_atom;
    e3gnn_pair::CommMaps::Stats st;
    bool same_bits(const Result& o) const {
      return !std::memcmp(&energy, &o.energy, 8) && !std::memcmp(virial, o.virial, 48) &&
             f.size() == o.f.size() && !std::memcmp(f.data(), o.f.data(), f.size() * 8);
    }
    bool same_graph(const Result& o) const {
      auto eq = [](const auto& a, const auto& b) {
        return a.size() == b.size() && !std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0]));
      };
      return eq(center, o.center) && eq(nbr, o.nbr) && eq(vec, o.vec) && eq(type, o.type) &&
             eq(row_atom, o.row_atom);
    }
    bool same_comm(const Result& o) const {
      return st.swaps == o.st.swaps && st.sent == o.st.sent && st.relayed == o.st.relayed &&
             st.extra_rows == o.st.extra_rows && st.zero_sends == o.st.zero_sends &&
             st.trash_forward == o.st.trash_forward && st.trash_reverse == o.st.trash_reverse;
    }
  };

  ParallelRig(const Structure& S, const std::string& model_dir, const int grid[3], int me, World* world,
              std::mutex* load_mutex) {
    lmp.memory = &mem;
    lmp.error = &err;
    lmp.atom = &atom;
    lmp.neighbor = &neigh;
    lmp.force = &force;
    lmp.domain = &dom;
    comm.reset(new CommBrick(&lmp, world, me, grid));
    lmp.comm = comm.get();
    dom.set_cell(S.cell);
    neigh.skin = SKIN;
    for (int a = 0; a < S.n; ++a) {
      double s[3], x[3];
      dom.x2lamda(&S.pos[3 * a], s);
      bool mine = true;
      for (int d = 0; d < 3; ++d) {
        s[d] -= std::floor(s[d]);
        if (s[d] >= 1.0) s[d] -= 1.0;
        const int c = std::min(grid[d] - 1, (int)(s[d] * grid[d]));
        mine = mine && c == comm->myloc[d];
      }
      if (!mine) continue;
      dom.lamda2x(s, x);
      atom.add(x, s, S.tag[a], S.type[a]);
    }
    atom.nlocal = (int)atom.tags.size();
    atom.natoms = S.n;
    atom.ntypes = (int)S.elements.size();
    atom.sync();
    std::vector<std::string> args = {"*", "*", "4", model_dir};
    for (const auto& e : S.elements) args.push_back(e);
    std::vector<char*> argv;
    for (auto& a : args) argv.push_back(&a[0]);
    {
      std::lock_guard<std::mutex> lk(*load_mutex);
      pair.reset(new PairE3GNNParallel(&lmp));
      pair->settings(0, nullptr);
      pair->coeff((int)argv.size(), argv.data());
    }
    pair->init_style();
    const double cut = pair->init_one(1, 1);
    comm->setup(cut + SKIN);
    comm->borders();
    neigh.build_full(&atom, cut, &list);
    pair->init_list(0, &list);
  }
  void graph(const char* where) {
    std::string a = "graph", b = where;
    char* argv[2] = {&a[0], &b[0]};
    pair->settings(2, argv);
  }
  // build() + comm_preprocess + compute(), without the ghost forces' way home
  void step(int ago) {
    neigh.ago = ago;
    std::fill(atom.fs.begin(), atom.fs.end(), 0.0);
    pair->compute(1 | 2, 1);
  }
  Result compute(int ago) {
    step(ago);
    comm->reverse_comm();   // ghost forces onto their owners (newton on)
    Result r;
    r.energy = pair->eng_vdwl;
    std::copy(pair->virial, pair->virial + 6, r.virial);
    r.f.assign(atom.fs.begin(), atom.fs.begin() + 3 * (size_t)atom.nlocal);
    e3gnn_pair::ParallelStep* core = pair->core();
    r.edges = core->nedges();
    r.ghost_rows = core->graph_size() - core->nlocal();
    if (core->graph_copy(r.center, r.nbr, r.vec, r.type, r.row_atom)) throw std::runtime_error(core->error());
    r.st = pair->comm_maps()->stats();
    return r;
  }
  void displace(unsigned seed, double amp) {
    const int nt = atom.nlocal + atom.nghost;
    for (int a = 0; a < nt; ++a) {
      std::mt19937 r(seed * 7919u + (unsigned)atom.tag[a]);
      std::uniform_real_distribution<double> u(-amp, amp);
      for (int k = 0; k < 3; ++k) atom.x[a][k] += u(r);
    }
  }
};

// one thread per rank of the grid, each with a rig of its own; `body(rig, rank)`
template <class Body>
void on_ranks(const Structure& S, const std::string& dir, const int grid[3], Body body) {
  const int P = grid[0] * grid[1] * grid[2];
  World world(P);
  std::mutex load_mutex;
  std::vector<std::string> errs(P);
  std::vector<std::thread> th;
  for (int r = 0; r < P; ++r)
    th.emplace_back([&, r] {
      try {
        if (hipSetDevice(0) != hipSuccess) throw std::runtime_error("hipSetDevice");
        ParallelRig rig(S, dir, grid, r, &world, &load_mutex);
        body(rig, r);
      } catch (const std::exception& e) {
        errs[r] = e.what();
        world.abort();
      }
    });
  for (auto& t : th) t.join();
  for (int r = 0; r < P; ++r)
    if (!errs[r].empty() && errs[r] != "world aborted")
      throw std::runtime_error("rank " + std::to_string(r) + ": " + errs[r]);
}

// --parallel-graph-device: the keys of the "parallel_graph_device" object
std::string parallel_graph_device_keys(const Structure& S, const std::string& dir, const int grid[3],
                                       unsigned seed) {
  const int P = grid[0] * grid[1] * grid[2];
  struct Out {
    long long edges = 0, edges_host = 0, ghost_rows = 0, ghost_rows_host = 0, reuse_edges = 0;
    bool graph = false, energy = false, forces = false, virial = false, comm = false, repeat = false,
         reuse_changed = false, reuse = false;
  };
  std::vector<Out> outs(P);
  on_ranks(S, dir, grid, [&](ParallelRig& rig, int r) {
    const auto host = rig.compute(0);
    rig.graph("device");
    const auto dev = rig.compute(0), dev2 = rig.compute(0);
    // reuse leg: the atoms move, the list stays (ago = 1); device first, so
    // that the step really reuses the list uploaded above
    rig.displace(seed, 0.4);
    const auto rdev = rig.compute(1);
    rig.graph("host");
    const auto rhost = rig.compute(1);
    Out& o = outs[r];
    o.edges = dev.edges;
    o.edges_host = host.edges;
    o.ghost_rows = dev.ghost_rows;
    o.ghost_rows_host = host.ghost_rows;
    o.reuse_edges = rdev.edges;
    o.graph = dev.same_graph(host);
    o.energy = !std::memcmp(&dev.energy, &host.energy, 8);
    o.forces = dev.f.size() == host.f.size() && !std::memcmp(dev.f.data(), host.f.data(), dev.f.size() * 8);
    o.virial = !std::memcmp(dev.virial, host.virial, 48);
    o.comm = dev.same_comm(host) && rdev.same_comm(rhost);
    o.repeat = dev.same_bits(dev2) && dev.same_graph(dev2);
    o.reuse_changed = rdev.edges != dev.edges || !rdev.same_graph(dev);
    o.reuse = rdev.same_bits(rhost) && rdev.same_graph(rhost);
  });
  auto tf = [](bool b) { return b ? "true" : "false"; };
  auto all = [&](bool Out::*m) {
    bool b = true;
    for (const Out& o : outs) b = b && o.*m;
    return b;
  };
  auto list = [&](long long Out::*m) {
    std::string s = "[";
    for (int r = 0; r < P; ++r) s += (r ? ", " : "") + std::to_string(outs[r].*m);
    return s + "]";
  };
  bool reuse_changed = false;   // on any rank: a small brick may keep its count
  for (const Out& o : outs) reuse_changed = reuse_changed || o.reuse_changed;
  return ", \"parallel_graph_device\": {\"edges\": " + list(&Out::edges) + ", \"edges_host\": " +
         list(&Out::edges_host) + ", \"ghost_rows\": " + list(&Out::ghost_rows) +
         ", \"ghost_rows_host\": " + list(&Out::ghost_rows_host) + ", \"graph_bits_equal\": " +
         tf(all(&Out::graph)) + ", \"energy_bits_equal\": " + tf(all(&Out::energy)) +
         ", \"forces_bits_equal\": " + tf(all(&Out::forces)) + ", \"virial_bits_equal\": " +
         tf(all(&Out::virial)) + ", \"comm_equal\": " + tf(all(&Out::comm)) + ", \"repeat_bitwise\": " +
         tf(all(&Out::repeat)) + ", \"reuse_edges\": " + list(&Out::reuse_edges) +
         ", \"reuse_edges_changed\": " + tf(reuse_changed) + ", \"reuse_bits_equal\": " +
         tf(all(&Out::reuse)) + "}";
}

// --parallel-graph-device --time K: style (2) on the grid, the ranks threads
// of this process sharing one GPU; rank 0's wall time of build() +
// comm_preprocess + compute() per round in host mode, device mode with the
// list re-uploaded (ago = 0) and device mode with the list reused (ago = 1)
int time_parallel_graph_modes(const Structure& S, const std::string& dir, const int grid[3], int K) {
  using clk = std::chrono::steady_clock;
  std::vector<double> t[3];
  int wins = 0, nghost = 0, nlocal = 0;
  long long edges = 0, ghost_rows = 0;
  on_ranks(S, dir, grid, [&](ParallelRig& rig, int r) {
    auto timed = [&](int ago) {
      const auto t0 = clk::now();
      rig.step(ago);   // ends in a stream synchronise
      return std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    };
    for (int w = 0; w < 2; ++w) timed(0);
    rig.graph("device");
    for (int w = 0; w < 2; ++w) timed(0);
    for (int w = 0; w < 2; ++w) timed(1);
    for (int k = 0; k < K; ++k) {
      rig.graph("host");
      const double a = timed(0);
      rig.graph("device");
      const double b = timed(0), c = timed(1);
      if (r == 0) {
        t[0].push_back(a);
        t[1].push_back(b);
        t[2].push_back(c);
        wins += c < a;
      }
    }
    if (r == 0) {
      nlocal = rig.atom.nlocal;
      nghost = rig.atom.nghost;
      edges = rig.pair->core()->nedges();
      ghost_rows = rig.pair->core()->graph_size() - rig.pair->core()->nlocal();
    }
  });
  std::printf("{\"style\": \"e3gnn/parallel\", \"n_atoms\": %d, \"ranks_as_threads_on_one_gpu\": %d, "
              "\"rank0_owned\": %d, \"rank0_ghosts\": %d, \"rank0_edges\": %lld, \"rank0_ghost_rows\": %lld, "
              "\"rounds\": %d, \"host_ms\": %s, \"device_new_list_ms\": %s, \"device_reused_list_ms\": %s, "
              "\"reused_beats_host_rounds\": %d, \"host_rounds_ms\": %s, \"device_new_list_rounds_ms\": %s, "
              "\"device_reused_list_rounds_ms\": %s}\n",
              S.n, grid[0] * grid[1] * grid[2], nlocal, nghost, edges, ghost_rows, K, stats(t[0]).c_str(),
              stats(t[1]).c_str(), stats(t[2]).c_str(), wins, rounds(t[0]).c_str(), rounds(t[1]).c_str(),
              rounds(t[2]).c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s model_dir structure px py pz [seed] [--gpu-aware] [--vatom] "
                         "[--graph-device] [--parallel-graph-device] [--time K]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int grid[3] = {std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5])};
  unsigned seed = 0;
  bool want_vatom = false, want_graph_device = false, want_parallel_graph_device = false;
  int time_rounds = 0;
  for (int k = 6; k < argc; ++k) {
    if (!std::strcmp(argv[k], "--gpu-aware")) setenv("E3GNN_GPU_AWARE_MPI", "1", 1);
    else if (!std::strcmp(argv[k], "--vatom")) want_vatom = true;
    else if (!std::strcmp(argv[k], "--graph-device")) want_graph_device = true;
    else if (!std::strcmp(argv[k], "--parallel-graph-device")) want_parallel_graph_device = true;
    else if (!std::strcmp(argv[k], "--time") && k + 1 < argc) time_rounds = std::max(1, std::atoi(argv[++k]));
    else seed = (unsigned)std::atoi(argv[k]);
  }
  try {
    std::mt19937 rng(seed);
    const Structure S = load_structure(argv[2], rng);
    if (time_rounds) {
      if (hipSetDevice(0) != hipSuccess) throw std::runtime_error("hipSetDevice");
      if (want_parallel_graph_device) return time_parallel_graph_modes(S, dir, grid, time_rounds);
      return time_graph_modes(S, dir, time_rounds);
    }
    e3gnn_pair::Model model(dir, 0);
    const std::vector<int> map = model.type_map(S.elements);
    const double rc = model.cutoff();
    const int n = S.n;

    // ---- (0) the library's own neighbour list + evaluation, atoms in tag order
    std::vector<double> pos_t(3 * (size_t)n), f_ref(3 * (size_t)n);
    std::vector<int32_t> ty(n);
    for (int a = 0; a < n; ++a) {
      for (int k = 0; k < 3; ++k) pos_t[3 * (S.tag[a] - 1) + k] = S.pos[3 * a + k];
      ty[S.tag[a] - 1] = map[S.type[a]];
    }
    double e_ref = 0, v_ref[6];
    std::vector<double> w_ref;   // --vatom: e3gnn_atom_virial by tag - 1, LAMMPS order
    int max_ends = 0;            // ... and the most edge ends (centre + neighbour side) on one atom
    {
      e3gnn_ctx* ctx = e3gnn_ctx_create(model.handle());
      e3gnn_nlist* nl = e3gnn_nlist_create(0);
      double* dp;
      int32_t *dt, *dc, *dn;
      float *dv, *df, *ds;
      (void)hipMalloc(&dp, 3 * n * 8);
      (void)hipMemcpy(dp, pos_t.data(), 3 * n * 8, hipMemcpyHostToDevice);
      const int pbc[3] = {1, 1, 1};
      int64_t E = 0;
      if (e3gnn_nlist_build(nl, n, dp, S.cell, pbc, rc, &E, nullptr)) throw std::runtime_error(e3gnn_last_error());
      (void)hipMalloc(&dc, E * 4);
      (void)hipMalloc(&dn, E * 4);
      (void)hipMalloc(&dv, E * 12);
      (void)hipMalloc(&dt, n * 4);
      (void)hipMalloc(&df, n * 12);
      (void)hipMalloc(&ds, 8 * 4);
      (void)hipMemcpy(dt, ty.data(), n * 4, hipMemcpyHostToDevice);
      if (e3gnn_nlist_fetch(nl, dc, dn, nullptr, dv, nullptr)) throw std::runtime_error(e3gnn_last_error());
      if (e3gnn_energy_forces(ctx, n, E, dt, dc, dn, dv, ds, nullptr, df, ds + 1, nullptr, nullptr))
        throw std::runtime_error(e3gnn_last_error());
      std::vector<float> hf(3 * (size_t)n);
      float sc[7];
      (void)hipMemcpy(hf.data(), df, n * 12, hipMemcpyDeviceToHost);
      (void)hipMemcpy(sc, ds, 28, hipMemcpyDeviceToHost);
      for (int i = 0; i < 3 * n; ++i) f_ref[i] = hf[i];
      e_ref = sc[0];
      const float* v6 = sc + 1;   // (xx, yy, zz, xy, yz, zx) -> LAMMPS (xx, yy, zz, xy, xz, yz)
      const double vl[6] = {v6[0], v6[1], v6[2], v6[3], v6[5], v6[4]};
      for (int k = 0; k < 6; ++k) v_ref[k] = vl[k];
      if (want_vatom) {
        float* dw;
        (void)hipMalloc(&dw, (size_t)n * 24);
        if (e3gnn_atom_virial(ctx, dw, nullptr)) throw std::runtime_error(e3gnn_last_error());
        std::vector<float> hw(6 * (size_t)n);
        std::vector<int32_t> hc(E), hn(E);
        (void)hipMemcpy(hw.data(), dw, (size_t)n * 24, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hc.data(), dc, E * 4, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hn.data(), dn, E * 4, hipMemcpyDeviceToHost);
        (void)hipFree(dw);
        const int lmp_of[6] = {0, 1, 2, 3, 5, 4};
        w_ref.resize(6 * (size_t)n);
        for (int a = 0; a < n; ++a)
          for (int k = 0; k < 6; ++k) w_ref[6 * (size_t)a + k] = hw[6 * (size_t)a + lmp_of[k]];
        std::vector<int> ends(n, 0);
        for (int64_t e = 0; e < E; ++e) {
          ends[hc[e]]++;
          ends[hn[e]]++;
        }
        max_ends = n ? *std::max_element(ends.begin(), ends.end()) : 0;
      }
      for (void* p : {(void*)dp, (void*)dc, (void*)dn, (void*)dv, (void*)dt, (void*)df, (void*)ds})
        (void)hipFree(p);
      e3gnn_nlist_free(nl);
      e3gnn_ctx_free(ctx);
    }
    auto max_diff = [](const std::vector<double>& a, const std::vector<double>& b) {
      double m = 0;
      for (size_t i = 0; i < a.size(); ++i) m = std::max(m, std::fabs(a[i] - b[i]));
      return m;
    };
    auto max_vdiff = [](const double* a, const double* b) {
      double m = 0;
      for (int k = 0; k < 6; ++k) m = std::max(m, std::fabs(a[k] - b[k]));
      return m;
    };

    const int one[3] = {1, 1, 1};
    const RunOut ser = run(S, dir, one, false, 2, want_vatom);
    const RunOut par = run(S, dir, grid, true, 2, want_vatom);
    const double scale = std::fabs(e_ref);
    // --vatom: the extra keys of a style's object (empty without the flag)
    auto vatom_keys = [&](const RunOut& R) -> std::string {
      if (!want_vatom) return "";
      double sum[6] = {0, 0, 0, 0, 0, 0};
      for (int a = 0; a < n; ++a)
        for (int k = 0; k < 6; ++k) sum[k] += R.vatom_tag[6 * (size_t)a + k];
      char buf[256];
      std::snprintf(buf, sizeof(buf),
                    ", \"vatom_max_diff\": %.3e, \"vatom_sum_max_diff\": %.3e, \"vatom_max_ends\": %d, "
                    "\"vatom_repeat_bitwise\": %s",
                    max_diff(R.vatom_tag, w_ref), max_vdiff(sum, R.virial), max_ends,
                    R.vatom_same_again ? "true" : "false");
      return buf;
    };
    const std::string vs = vatom_keys(ser), vp = vatom_keys(par);
    std::string gd = want_graph_device ? graph_device_keys(S, dir, seed) : "";
    if (want_parallel_graph_device) gd += parallel_graph_device_keys(S, dir, grid, seed);
    std::printf(
        "{\"n_atoms\": %d, \"ranks\": %d, \"energy_ref\": %.8f, \"max_virial_ref\": %.6e, "
        "\"serial\": {\"energy\": %.8f, \"energy_rel\": %.3e, \"max_force\": %.3e, \"max_virial\": %.3e, "
        "\"eatom_sum_rel\": %.3e, \"repeat_bitwise\": %s%s}, "
        "\"parallel\": {\"energy\": %.8f, \"energy_rel\": %.3e, \"max_force\": %.3e, \"max_virial\": %.3e, "
        "\"eatom_sum_rel\": %.3e, \"repeat_bitwise\": %s, \"vs_serial_energy_rel\": %.3e, "
        "\"vs_serial_max_force\": %.3e%s}, "
        "\"comm\": {\"ghosts\": %lld, \"swaps\": %lld, \"sent\": %lld, \"relayed\": %lld, \"extra_rows\": %lld, "
        "\"zero_sends\": %lld, \"trash_forward\": %lld, \"trash_reverse\": %lld}%s}\n",
        n, grid[0] * grid[1] * grid[2], e_ref, std::max(std::fabs(*std::max_element(v_ref, v_ref + 6)),
                                                       std::fabs(*std::min_element(v_ref, v_ref + 6))),
        ser.energy, std::fabs(ser.energy - e_ref) / scale, max_diff(ser.f_tag, f_ref), max_vdiff(ser.virial, v_ref),
        std::fabs(ser.eatom - e_ref) / scale, ser.same_again ? "true" : "false", vs.c_str(), par.energy,
        std::fabs(par.energy - e_ref) / scale, max_diff(par.f_tag, f_ref), max_vdiff(par.virial, v_ref),
        std::fabs(par.eatom - e_ref) / scale, par.same_again ? "true" : "false",
        std::fabs(par.energy - ser.energy) / scale, max_diff(par.f_tag, ser.f_tag), vp.c_str(),
        (long long)par.ghosts,
        (long long)par.st.swaps, (long long)par.st.sent, (long long)par.st.relayed, (long long)par.st.extra_rows,
        (long long)par.st.zero_sends, (long long)par.st.trash_forward, (long long)par.st.trash_reverse,
        gd.c_str());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "e3gnn_pair_check: %s\n", e.what());
    return 1;
  }
  return 0;
}
