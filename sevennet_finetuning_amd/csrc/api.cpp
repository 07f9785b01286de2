// Host side of libe3gnn_hip.so: the evaluation context -- workspace management
// and the per-layer orchestration of the SevenNet-0 energy + force evaluation,
// behind the C ABI of include/e3gnn.h.  The model it evaluates is built by
// model_load.cpp (model.h); the stateless entry points are in api_train.cpp
// (training ops), api_nlist.cpp (neighbour list) and api_d3.cpp (DFT-D3).
//
// Pipeline (sevenn/model_build.py:186-445; deploy.py:20-32 for the serial
// deployment, model_build.py:103-182 for the parallel segments):
//   edge embedding -> onehot embed -> 5 x [self_connection_intro,
//   self_interaction_1, IrrepsConvolution, self_interaction_2,
//   self_connection_outro, gate] -> readout -> SpeciesWiseRescale -> sum
// and the reverse-mode pass that ForceStressOutput gets from autograd
// (force_output.py:74-130), written out explicitly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "atom_virial.h"
#include "cg_tables.h"
#include "common.h"
#include "dbuf.h"
#include "fused.h"
#include "generic.h"
#include "model.h"
#include "node.h"
#include "segment_sum.h"
#include "tp.h"

using namespace e3gnn;

namespace {
thread_local std::string g_err;

bool trace_errors() {
  static int on = [] {
    const char* v = std::getenv("E3GNN_TRACE_ERRORS");
    return v && v[0] == '1';
  }();
  return on;
}
}  // namespace

namespace e3gnn {
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
void trace_point(const char* where) {
  if (!trace_errors()) return;
  hipError_t e = hipPeekAtLastError();
  if (e != hipSuccess) std::fprintf(stderr, "[e3gnn] sticky HIP error %d (%s) at %s\n", (int)e,
                                    hipGetErrorString(e), where);
}
}  // namespace e3gnn

namespace {

struct Stat {
  double ms = 0, flops = 0, bytes = 0;
  int64_t launches = 0;
};
struct Pending {
  int cls;
  hipEvent_t a, b;
  double flops, bytes;
};
const char* kClassNames[] = {"graph_build", "edge_embed",  "node_linear", "radial_mlp_fwd",
                             "tp_fwd",      "gate_fwd",    "readout",     "gate_bwd",
                             "tp_bwd",      "radial_mlp_bwd", "gather_src", "edge_force",
                             "atom_force",  "atom_virial", "embed",
                             // fused kernels, one class per kernel and block kind
                             "conv_fwd.first", "conv_fwd.mid", "conv_fwd.last",
                             "conv_bwd_x.first", "conv_bwd_x.mid", "conv_bwd_x.last"};
enum Cls {
  C_GRAPH,
  C_EMBED_EDGE,
  C_LINEAR,
  C_MLP_FWD,
  C_TP_FWD,
  C_GATE_FWD,
  C_READOUT,
  C_GATE_BWD,
  C_TP_BWD,
  C_MLP_BWD,
  C_GATHER,
  C_EDGE_FORCE,
  C_ATOM_FORCE,
  C_ATOM_VIRIAL,
  C_EMBED_NODE,
  C_CONV_FWD,             // + kind (0 first, 1 mid, 2 last)
  C_CONV_BWD_X = C_CONV_FWD + 3,
  C_NCLS = C_CONV_BWD_X + 3
};
static_assert(sizeof(kClassNames) / sizeof(kClassNames[0]) == C_NCLS, "class names");

// algorithmic per-edge FLOP of one TP forward (SevenNet-0:
// 3,456 / 16,832 / 1,184 for the first / middle / last block)
double tp_flops_per_edge(int code) { return fused_kind_tp_flops(code); }

}  // namespace

struct e3gnn_ctx {
  e3gnn_model* m;
  GenCtx* gen = nullptr;  // the generic engine's buffers (m->gen)
  int64_t n = 0, nl = 0, E = 0;
  // halo overlap: owned centres [0, n_int) have no ghost neighbour; their
  // edges are [0, e_int) (e3gnn_set_interior, effective at graph_set)
  int64_t n_interior_req = 0, n_int = 0, e_int = 0;
  // graph
  DBuf type, center, nbr, vec, row_ptr, src_ptr, src_perm, cnt, err;
  DBuf Y, emb, dY, dgu, demb, fe;
  // the fused kernels take the radial MLP's share of dE/dr in forward mode:
  // embd = d emb / dr [E, 8] in, drad [E] accumulated over the blocks (demb,
  // dE/demb, is the v1 kernels')
  DBuf embd, drad;
  // node linears on k_nodelin (node-aligned tiles, si2 + sc in one problem,
  // gate in the epilogue; 1, default) or the grouped k_gemm + k_gate kernels
  // (0; E3GNN_NODELIN=0)
  int nodelin = [] {
    const char* v = std::getenv("E3GNN_NODELIN");
    return (v && std::string(v) == "0") ? 0 : 1;
  }();
  // 0: fused radial-MLP + TP kernels (fused.hip); 1: the unfused v1 kernels
  // (materialised per-edge weights; kept as an independent cross-check,
  // e3gnn_set_impl)
  int impl = 0;
  int graph_impl = 0;  // impl in force since the last e3gnn_graph_set (buffers sized for it)
  // per layer
  std::vector<DBuf> x, grad, h, y, w, a1, a2;
  DBuf H1, H2, agg, dw, dxc, dy, dh, eat, part, vpart, scratch6;
  // e3gnn_energy_forces_batch: atomic energies (when the caller takes none) and
  // per-atom virials, the inputs of the per-structure sums
  DBuf beat, bw;
  bool timing = false;
  bool stream_ordered = false;  // e3gnn_set_stream_ordered
  // stream-ordered mode: the end of the last evaluation on `done_stream`; a
  // call on another stream waits for it before touching the shared
  // workspaces (inputs are copied into them at graph_set)
  hipEvent_t done_ev = nullptr;
  hipStream_t done_stream = nullptr;
  bool done_pending = false;
  Stat stats[C_NCLS];
  std::vector<Pending> pending;
  std::vector<hipEvent_t> evpool;
  int readout_done = 0;
  // e3gnn_forces has written the per-edge dE/dr of the current graph (what
  // e3gnn_atom_virial reads); cleared by e3gnn_graph_set
  int forces_done = 0;

  hipEvent_t ev() {
    if (!evpool.empty()) {
      hipEvent_t e = evpool.back();
      evpool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
  void flush() {
    for (auto& p : pending) {
      (void)hipEventSynchronize(p.b);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, p.a, p.b);
      stats[p.cls].ms += ms;
      stats[p.cls].launches += 1;
      stats[p.cls].flops += p.flops;
      stats[p.cls].bytes += p.bytes;
      evpool.push_back(p.a);
      evpool.push_back(p.b);
    }
    pending.clear();
  }
  ~e3gnn_ctx() {
    if (gen) gen_ctx_free(gen);
    flush();
    if (done_ev) {
      (void)hipEventSynchronize(done_ev);
      (void)hipEventDestroy(done_ev);
    }
    for (auto e : evpool) (void)hipEventDestroy(e);
  }
};

namespace {

// Timed region helper: brackets the enclosed launches with events when timing.
struct Region {
  e3gnn_ctx* c;
  hipStream_t s;
  int cls;
  double flops, bytes;
  hipEvent_t a = nullptr;
  Region(e3gnn_ctx* c_, hipStream_t s_, int cls_, double f = 0, double b = 0)
      : c(c_), s(s_), cls(cls_), flops(f), bytes(b) {
    if (c->timing) {
      a = c->ev();
      (void)hipEventRecord(a, s);
    }
  }
  ~Region() {
    if (c->timing) {
      hipEvent_t b = c->ev();
      (void)hipEventRecord(b, s);
      c->pending.push_back({cls, a, b, flops, bytes});
    }
  }
};

// ------------------------------------------------------------ linear → GEMM problems
void add_prob(GemmBatch& b, const GemmProb& p) {
  GemmProb q = p;
  const int tm = (q.M + 63) / 64, tn = (q.N + 63) / 64;
  if (tm == 0 || tn == 0) return;
  q.tiles_n = tn;
  q.tile_begin = b.total_tiles;
  b.p[b.nprob++] = q;
  b.total_tiles += tm * tn;
}

GemmProb base_prob() {
  GemmProb p;
  std::memset(&p, 0, sizeof(p));
  p.R = 1;
  return p;
}

// y[rows, dout] (+)= x[rows, din] @ lin    (row strides lda/ldc)
GemmBatch lin_fwd(const Linear& L, const float* x, int64_t lda, float* y, int64_t ldc, int64_t rows,
                  int beta) {
  GemmBatch b;
  std::memset(&b, 0, sizeof(b));
  for (auto& k : L.blocks) {
    GemmProb p = base_prob();
    p.A = x;
    p.B = L.W.f() + k.w_off;
    p.C = y;
    p.lda = lda;
    p.ldc = ldc;
    p.R = 2 * k.l + 1;
    p.M = (int)(rows * p.R);
    p.K = k.K;
    p.N = k.N;
    p.a_off = k.in_off;
    p.c_off = k.out_off;
    p.ldb = k.N;
    p.beta = beta;
    add_prob(b, p);
  }
  return b;
}
// dx[rows, din] (+)= dy[rows, dout] @ lin^T
GemmBatch lin_bwd(const Linear& L, const float* dy, int64_t ldy, float* dx, int64_t ldx,
                  int64_t rows, int beta) {
  GemmBatch b;
  std::memset(&b, 0, sizeof(b));
  for (auto& k : L.blocks) {
    GemmProb p = base_prob();
    p.A = dy;
    p.B = L.WT.f() + k.wt_off;
    p.C = dx;
    p.lda = ldy;
    p.ldc = ldx;
    p.R = 2 * k.l + 1;
    p.M = (int)(rows * p.R);
    p.K = k.N;
    p.N = k.K;
    p.a_off = k.out_off;
    p.c_off = k.in_off;
    p.ldb = k.K;
    p.beta = beta;
    add_prob(b, p);
  }
  return b;
}
double lin_flops(const Linear& L, int64_t rows) {
  double f = 0;
  for (auto& k : L.blocks) f += 2.0 * rows * (2 * k.l + 1) * k.K * k.N;
  return f;
}

// k_nodelin batch over rows [0, rows) of A (+ A2) -> C for the blocks of P
// selected by `sel` (0 all, 1 the l = 0 block, 2 the l > 0 blocks); `fix`
// fills the epilogue fields per block.  false: not expressible (the caller
// takes the k_gemm path).
struct NoFix {
  void operator()(NlProb&, const PairBlock&) const {}
};
template <class Fix = NoFix>
bool nl_batch(NlBatch& b, LinPair& P, const float* A, int64_t lda, const float* A2, int64_t lda2,
              float* C, int64_t ldc, int64_t rows, int epi, int sel = 0, Fix fix = Fix()) {
  std::memset(&b, 0, sizeof(b));
  if (!P.ok) return false;
  for (auto& k : P.blocks) {
    if ((sel == 1 && k.l != 0) || (sel == 2 && k.l == 0)) continue;
    NlProb q;
    std::memset(&q, 0, sizeof(q));
    q.A = A;
    q.lda = lda;
    q.a_off = k.off1;
    q.A2 = k.K2 ? A2 : nullptr;
    q.lda2 = lda2;
    q.a_off2 = k.off2;
    q.K1 = k.K1;
    q.K = k.K1 + k.K2;
    q.B = P.W.f() + k.w_off;
    q.Bb = P.Wb.p ? static_cast<const char*>(P.Wb.p) + k.wb_off : nullptr;
    q.C = C;
    q.ldc = ldc;
    q.c_off = k.out_off;
    q.N = k.N;
    q.R = 2 * k.l + 1;
    q.nodes = (int)rows;
    q.epi = epi;
    fix(q, k);
    if (!add_nl(b, q)) return false;
  }
  return true;
}
double pair_flops(const LinPair& P, int64_t rows) {
  double f = 0;
  for (auto& k : P.blocks) f += 2.0 * rows * (2 * k.l + 1) * (k.K1 + k.K2) * k.N;
  return f;
}

template <int A, int B, int C>
void dense_cg(float* out) {
  using T = CG<A, B, C>;
  std::memset(out, 0, sizeof(float) * (2 * A + 1) * (2 * B + 1) * (2 * C + 1));
  for (int q = 0; q < T::n; ++q)
    out[(T::e[q].i * (2 * B + 1) + T::e[q].j) * (2 * C + 1) + T::e[q].k] = T::e[q].c;
}
MlpW mlp_ptrs(const e3gnn_model* m, int t) {
  const auto& mm = m->mlp[t];
  MlpW w{};   // (the retired slots stay null)
  w.w0 = mm.w0.f();
  w.w2b = static_cast<const uint16_t*>(mm.w2b.p);
  w.w2v = static_cast<const uint16_t*>(mm.w2v.p);
  w.w2s = static_cast<const uint16_t*>(mm.w2s.p);
  w.w1b = static_cast<const uint16_t*>(mm.w1b.p);
  return w;
}

// What every fused launch of block t shares (fused.h): the graph, the edge
// embedding and SH, the block's h rows and radial MLP, the counts.  The
// forward and backward parts add their outputs and work ranges.
FusedArgs fused_base(const e3gnn_ctx* c, int t) {
  FusedArgs a;
  std::memset(&a, 0, sizeof(a));
  a.row_ptr = c->row_ptr.i();
  a.nbr = c->nbr.i();
  a.emb = c->emb.f();
  a.Y = c->Y.f();
  a.h = c->h[t].f();
  a.W = mlp_ptrs(c->m, t);
  a.n_centers = (int)c->nl;
  a.n_nodes = (int)c->n;
  return a;
}

GenGraph gen_graph(e3gnn_ctx* c) {
  return GenGraph{c->n, c->nl, c->E, c->type.i(), c->nbr.i(), c->vec.f(), c->row_ptr.i(),
                  c->src_ptr.i(), c->src_perm.i(), c->err.i()};
}

}  // namespace

extern "C" {

const char* e3gnn_last_error(void) { return g_err.c_str(); }
int e3gnn_abi_version(void) { return 1; }

e3gnn_ctx* e3gnn_ctx_create(e3gnn_model* m) {
  if (!m) {
    fail(E3GNN_ERR_ARG, "null model");
    return nullptr;
  }
  auto c = new e3gnn_ctx();
  c->m = m;
  if (m->gen) c->gen = gen_ctx_create(m->gen);
  const int L = m->nlayer;
  c->x.resize(L + 1);
  c->grad.resize(L + 1);
  c->h.resize(L);
  c->y.resize(L);
  c->w.resize(L);
  c->a1.resize(L);
  c->a2.resize(L);
  return c;
}
void e3gnn_ctx_free(e3gnn_ctx* c) { delete c; }

int e3gnn_feature_dim(const e3gnn_ctx* c, int layer) {
  if (!c || layer < 0 || layer > c->m->nlayer) return -1;
  if (c->m->gen) return gen_feature_dim(c->m->gen, layer);
  return irreps_dim(c->m->irreps[layer]);
}
float* e3gnn_feature_ptr(e3gnn_ctx* c, int layer) {
  if (!c || layer < 0 || layer > c->m->nlayer) return nullptr;
  if (c->gen) return gen_x(c->gen, layer);
  return c->x[layer].f();
}
float* e3gnn_grad_ptr(e3gnn_ctx* c, int layer) {
  if (!c || layer < 0 || layer > c->m->nlayer) return nullptr;
  if (c->gen) return gen_grad(c->gen, layer);
  return c->grad[layer].f();
}

int e3gnn_graph_set(e3gnn_ctx* c, int64_t n_local, int64_t n_ghost, int64_t n_edges,
                    const int32_t* type, const int32_t* edge_center, const int32_t* edge_nbr,
                    const float* edge_vec, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  c->forces_done = 0;
  if (n_local < 0 || n_ghost < 0 || n_edges < 0) return fail(E3GNN_ERR_ARG, "negative size");
  if (n_local + n_ghost > (1LL << 30) || n_edges > (1LL << 31) - 1)
    return fail(E3GNN_ERR_ARG, "graph too large for int32 indices");
  // the fused kernels gather node-feature rows through one 32-bit buffer
  // descriptor (n x DX fp32 < 2 GiB: 1.1M atoms at SevenNet-0's 480; the last
  // block's dE/dagg rows fit whenever these do)
  if (!c->gen && (n_local + n_ghost) * (int64_t)c->m->max_dx * 4 > 0x7fffffffLL)
    return fail(E3GNN_ERR_ARG, "more than " + std::to_string(0x7fffffffLL / (4LL * c->m->max_dx)) +
                                   " atoms (owned + ghost) per device for this model: shard the system");
  if (!c->gen && c->impl == 1 && c->m->family != 0)
    return fail(E3GNN_ERR_ARG, "the v1 (unfused) kernels serve SevenNet-0's channel family only");
  if ((n_local + n_ghost > 0 && !type) || (n_edges > 0 && (!edge_center || !edge_nbr || !edge_vec)))
    return fail(E3GNN_ERR_ARG, "null input array");
  e3gnn_model* m = c->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  if (c->done_pending && c->done_stream != s) HIPCHK(hipStreamWaitEvent(s, c->done_ev, 0));
  c->done_pending = false;
  const int64_t n = n_local + n_ghost, nl = n_local, E = n_edges;
  c->n = n;
  c->nl = nl;
  c->E = E;
  c->readout_done = 0;
  if (c->n_interior_req > nl) return fail(E3GNN_ERR_ARG, "n_interior exceeds n_local");
  c->n_int = c->n_interior_req;
  c->e_int = 0;
  const size_t F = sizeof(float);
  // workspace (grow-only)
  HIPCHK(c->type.ensure(n * 4));
  HIPCHK(c->center.ensure(E * 4));
  HIPCHK(c->nbr.ensure(E * 4));
  HIPCHK(c->vec.ensure(E * 3 * F));
  HIPCHK(c->row_ptr.ensure((nl + 1) * 4));
  HIPCHK(c->src_ptr.ensure((n + 1) * 4));
  HIPCHK(c->src_perm.ensure(E * 4));
  HIPCHK(c->cnt.ensure(n * 4));
  HIPCHK(c->err.ensure(4));
  if (!c->gen) {
    HIPCHK(c->Y.ensure(E * 9 * F));
    HIPCHK(c->emb.ensure(E * 8 * F));
    HIPCHK(c->dY.ensure(E * 9 * F));
    HIPCHK(c->fe.ensure(E * 3 * F));
    HIPCHK(c->dgu.ensure(E * 3 * F));
    const bool v1 = c->impl == 1;
    c->graph_impl = c->impl;
    if (v1) {
      HIPCHK(c->demb.ensure(E * 8 * F));
      HIPCHK(c->H1.ensure(E * 64 * F));
      HIPCHK(c->H2.ensure(E * 64 * F));
    } else {
      HIPCHK(c->embd.ensure(E * 8 * F));
      HIPCHK(c->drad.ensure(E * F));
    }
    int maxW = 0, maxDM = 0;
    for (int t = 0; t < m->nlayer; ++t) {
      const int dx = irreps_dim(m->irreps[t]), dg = irreps_dim(m->gin[t]);
      maxW = std::max(maxW, m->W[t]);
      maxDM = std::max(maxDM, irreps_dim(m->mid[t]));
      HIPCHK(c->x[t].ensure(std::max<int64_t>(n, 1) * dx * F));
      HIPCHK(c->grad[t].ensure(std::max<int64_t>(n, 1) * dx * F));
      HIPCHK(c->h[t].ensure(n * dx * F));
      HIPCHK(c->y[t].ensure(nl * dg * F));
      if (v1) {
        HIPCHK(c->w[t].ensure(E * m->W[t] * F));
        HIPCHK(c->a1[t].ensure(E * 64 * F));
        HIPCHK(c->a2[t].ensure(E * 64 * F));
      }
    }
    const int dlast = irreps_dim(m->irreps[m->nlayer]);
    HIPCHK(c->x[m->nlayer].ensure(std::max<int64_t>(n, 1) * dlast * F));
    HIPCHK(c->grad[m->nlayer].ensure(std::max<int64_t>(n, 1) * dlast * F));
    HIPCHK(c->agg.ensure(nl * maxDM * F));
    if (v1) HIPCHK(c->dw.ensure(E * maxW * F));
    HIPCHK(c->dxc.ensure(E * m->max_dx * F));
    HIPCHK(c->dy.ensure(nl * m->max_dg * F));
    HIPCHK(c->dh.ensure(n * m->max_dx * F));
    HIPCHK(c->eat.ensure(std::max<int64_t>(nl, 1) * F));
    HIPCHK(c->part.ensure((sum_blocks(nl) + 1) * F));
    HIPCHK(c->vpart.ensure((edge_force_blocks(E) + 1) * 6 * F));
    HIPCHK(c->scratch6.ensure(8 * F));

  }
  if (n > 0) HIPCHK(hipMemcpyAsync(c->type.p, type, n * 4, hipMemcpyDefault, s));
  if (E > 0) {
    HIPCHK(hipMemcpyAsync(c->center.p, edge_center, E * 4, hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(c->nbr.p, edge_nbr, E * 4, hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(c->vec.p, edge_vec, E * 3 * F, hipMemcpyDefault, s));
  }
  HIPCHK(hipMemsetAsync(c->err.p, 0, 4, s));
  {
    Region r(c, s, C_GRAPH, 0, (double)E * 24 + n * 12);
    HIPCHK(launch_build_graph(E, (int)nl, (int)n, c->center.i(), c->nbr.i(), c->row_ptr.i(),
                              c->src_ptr.i(), c->src_perm.i(), c->cnt.i(), c->err.i(), s,
                              (int)c->n_int));
  }
  if (c->gen) {
    HIPCHK(gen_graph_set(c->gen, m->gen, gen_graph(c), s));
  } else {
    const int d0 = irreps_dim(m->irreps[0]);
    Region r(c, s, C_EMBED_NODE, 0, (double)n * d0 * 4);
    HIPCHK(launch_embed((int)n, d0, c->type.i(), m->nsp, m->embed.f(), c->x[0].f(), c->err.i(), s));
  }
  int err = 0, e_int = 0;
  HIPCHK(hipMemcpyAsync(&err, c->err.p, 4, hipMemcpyDeviceToHost, s));
  if (c->n_int > 0)
    HIPCHK(hipMemcpyAsync(&e_int, c->row_ptr.i() + c->n_int, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->e_int = e_int;
  if (err) {
    std::string msg = "invalid graph:";
    if (err & 1) msg += " edge_center not sorted non-decreasing;";
    if (err & 2) msg += " edge_center out of [0, n_local);";
    if (err & 4) msg += " edge_nbr out of [0, n_local+n_ghost);";
    if (err & 8) msg += " species index out of range;";
    if (err & 16) msg += " an interior centre (below n_interior) has a ghost neighbour;";
    return fail(E3GNN_ERR_GRAPH, msg);
  }
  if (c->gen) return E3GNN_OK;  // (edge embedding done by gen_graph_set)
  {
    Region r(c, s, C_EMBED_EDGE, 0, (double)E * (12 + 68 + (c->graph_impl == 1 ? 0 : 32)));
    HIPCHK(launch_edge_embed(E, c->vec.f(), m->coeffs.f(), m->cutoff, m->r_on, m->raw_sh, c->Y.f(),
                             c->emb.f(), c->graph_impl == 1 ? nullptr : c->embd.f(), s));
  }
  if (E > 0) {
    // zero kernels, not hipMemsetAsync: the evaluation stays correct when a
    // host captures it in a HIP graph (launch_zero, node.hip)
    HIPCHK(launch_zero(c->dY.f(), E * 9, s));
    HIPCHK(launch_zero(c->dgu.f(), E * 3, s));
    if (c->graph_impl == 1) HIPCHK(launch_zero(c->demb.f(), E * 8, s));
    else HIPCHK(launch_zero(c->drad.f(), E, s));
  }
  return E3GNN_OK;
}

// The convolution of the v1 cross-check (impl 1), over all edges: the radial
// MLP materialises the per-edge weights w, the tensor-product kernels read them.
static int v1_conv_forward(e3gnn_ctx* c, int t, hipStream_t s) {
  e3gnn_model* m = c->m;
  const int64_t nl = c->nl, E = c->E;
  const int dx = irreps_dim(m->irreps[t]), dm = irreps_dim(m->mid[t]), W = m->W[t];
  const int kind = t == 0 ? 0 : (t == m->nlayer - 1 ? 2 : 1);
  // radial MLP: emb -> 64 -> 64 -> W  (convolution.py:97-106)
  {
    Region r(c, s, C_MLP_FWD, 2.0 * E * (8 * 64 + 64 * 64 + 64 * W),
             (double)E * 4 * (8 + 64 * 4 + 2 * 64 + W));
    auto& mm = m->mlp[t];
    GemmBatch b;
    std::memset(&b, 0, sizeof(b));
    GemmProb p = base_prob();
    p.A = c->emb.f(); p.lda = 8; p.K = 8;
    p.B = mm.w0.f(); p.ldb = 64; p.N = 64;
    p.C = c->H1.f(); p.ldc = 64; p.M = (int)E;
    p.act = 1; p.pre_out = c->a1[t].f();
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
    std::memset(&b, 0, sizeof(b));
    p.A = c->H1.f(); p.lda = 64; p.K = 64;
    p.B = mm.w1.f(); p.C = c->H2.f(); p.pre_out = c->a2[t].f();
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
    std::memset(&b, 0, sizeof(b));
    p.A = c->H2.f(); p.B = mm.w2.f(); p.ldb = W; p.N = W;
    p.C = c->w[t].f(); p.ldc = W; p.act = 0; p.pre_out = nullptr;
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
  }
  // tensor product + segmented neighbour sum
  {
    Region r(c, s, C_TP_FWD, tp_flops_per_edge(m->kcode(t)) * E,
             (double)E * 4 * (W + 9 + dx + 2) + nl * 4.0 * dm);
    TpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.row_ptr = c->row_ptr.i();
    a.nbr = c->nbr.i();
    a.Y = c->Y.f();
    a.w = c->w[t].f();
    a.h = c->h[t].f();
    a.agg = c->agg.f();
    a.n_centers = (int)nl;
    a.denom = m->denom[t];
    HIPCHK(launch_tp_fwd(kind, a, s));
  }
  return E3GNN_OK;
}

// Parts of one interaction block for the halo overlap (e3gnn.h):
// part 0 needs only the owned rows of the block's input features (it runs
// while the ghost rows are in flight): self_interaction_1 of the owned rows and
// the convolution of the interior centres [0, n_int); part 1: the ghost rows'
// self_interaction_1, the boundary centres [n_int, n_local), si2 +
// self-connection + gate.  The v1 kernels run whole in part 1.
int e3gnn_layer_forward_part(e3gnn_ctx* c, int t, int part, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  e3gnn_model* m = c->m;
  if (t < 0 || t >= m->nlayer) return fail(E3GNN_ERR_ARG, "layer out of range");
  if (part != 0 && part != 1) return fail(E3GNN_ERR_ARG, "part must be 0 or 1");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // generic engine: the whole layer after the halo of x[t] (part 1)
  if (c->gen) {
    if (part == 1) HIPCHK(gen_layer_forward(c->gen, m->gen, gen_graph(c), t, s));
    return E3GNN_OK;
  }
  const int64_t n = c->n, nl = c->nl, E = c->E, n_int = c->n_int;
  const int dx = irreps_dim(m->irreps[t]), dg = irreps_dim(m->gin[t]);
  const int dm = irreps_dim(m->mid[t]), W = m->W[t];
  const bool last = t == m->nlayer - 1;
  const int kind = t == 0 ? 0 : (last ? 2 : 1);   // block kind (timing class)
  const int code = m->kcode(t);                    // fused kernel kind code
  // self_interaction_1 of the rows [r0, r1)
  auto si1 = [&](int64_t r0, int64_t r1) -> int {
    Region r(c, s, C_LINEAR, lin_flops(*m->si1[t], r1 - r0));
    if (r1 <= r0) return E3GNN_OK;
    const float* x = c->x[t].f() + r0 * dx;
    float* h = c->h[t].f() + r0 * dx;
    NlBatch nb;
    const float* b1 = m->b_si1[t].f();   // use_bias_in_linear: on the 0e block
    auto bias_fix = [&](NlProb& q, const PairBlock& k) {
      if (b1 && k.l == 0) q.bias = b1 + k.out_off;
    };
    if (c->nodelin && nl_batch(nb, *m->nl_si1[t], x, dx, nullptr, 0, h, dx, r1 - r0, 0, 0, bias_fix)) {
      HIPCHK(launch_nodelin(nb, s));
    } else {
      HIPCHK(launch_gemm(lin_fwd(*m->si1[t], x, dx, h, dx, r1 - r0, 0), s));
      if (b1) HIPCHK(launch_row_bias(r1 - r0, dx, b1, h, s));
    }
    return E3GNN_OK;
  };
  // fused radial MLP + tensor product + segmented sum (fused.hip) of the
  // centres [c0, c1)
  auto conv_fwd = [&](int64_t c0, int64_t c1, double e_share) -> int {
    if (c1 <= c0) return E3GNN_OK;
    Region r(c, s, C_CONV_FWD + kind,
             e_share * (tp_flops_per_edge(code) + 2.0 * (8 * 64 + 64 * 64 + 64 * W)),
             e_share * 4 * (8 + 9 + 2 + dx) + (c1 - c0) * 4.0 * dm);
    FusedArgs a = fused_base(c, t);
    a.agg = c->agg.f();
    a.denom = m->denom[t];
    a.c_begin = (int)c0;
    a.c_end = (int)c1;
    HIPCHK(launch_conv_fwd(code, a, s));
    return E3GNN_OK;
  };
  if (c->graph_impl == 1) {  // the v1 cross-check: all rows and edges, in part 1
    if (part == 0) return E3GNN_OK;
    if (const int rc = si1(0, n)) return rc;
    if (const int rc = v1_conv_forward(c, t, s)) return rc;
  } else if (part == 0) {
    if (const int rc = si1(0, nl)) return rc;
    return conv_fwd(0, n_int, (double)c->e_int);
  } else {
    if (const int rc = si1(nl, n)) return rc;
    if (const int rc = conv_fwd(n_int, nl, (double)(E - c->e_int))) return rc;
  }
  // self_interaction_2 + self_connection (intro/outro) + gate: on k_nodelin
  // one K-concatenated problem per output block, the 0e block first (its
  // epilogue activates the scalars and stores the gate pre-activations), then
  // the gated blocks (epilogue: x = act(gate) * y)
  {
    const Irreps& gin = m->gin[t];
    const Irreps& xo = m->irreps[t + 1];
    int nscal = 0;
    for (auto& i : xo)
      if (i.l == 0) nscal += i.mul;
    const bool gate_ok = !gin.empty() && gin[0].l == 0 && !xo.empty() && xo[0].l == 0;
    auto gate_fix = [&](NlProb& q, const PairBlock& k) {
      q.xo = c->x[t + 1].f();
      q.ldxo = irreps_dim(xo);
      if (k.l == 0) {
        q.n_act = nscal;
        // si2's bias on the scalars and the gates: C keeps the biased
        // pre-activations the backward differentiates at
        if (m->b_si2[t].f()) q.bias = m->b_si2[t].f() + k.out_off;
        return;
      }
      int off = gin[0].mul, gmul = 0, gdim = 0;
      for (size_t i = 1; i < gin.size() && off != k.out_off; ++i) {
        gmul += gin[i].mul;
        gdim += gin[i].mul * (2 * gin[i].l + 1);
        off += gin[i].mul * (2 * gin[i].l + 1);
      }
      q.gate_off = nscal + gmul;
      q.xo_off = nscal + gdim;
    };
    NlBatch b0, b1;
    if (c->nodelin && gate_ok &&
        nl_batch(b0, *m->nl_fwd[t], c->agg.f(), dm, c->x[t].f(), dx, c->y[t].f(), dg, nl, 2, 1, gate_fix) &&
        nl_batch(b1, *m->nl_fwd[t], c->agg.f(), dm, c->x[t].f(), dx, c->y[t].f(), dg, nl, 3, 2, gate_fix)) {
      Region r(c, s, C_LINEAR, pair_flops(*m->nl_fwd[t], nl));
      HIPCHK(launch_nodelin(b0, s));
      HIPCHK(launch_nodelin(b1, s));
      return E3GNN_OK;
    }
  }
  {
    Region r(c, s, C_LINEAR, lin_flops(*m->si2[t], nl) + lin_flops(*m->sc[t], nl));
    HIPCHK(launch_gemm(lin_fwd(*m->si2[t], c->agg.f(), dm, c->y[t].f(), dg, nl, 0), s));
    HIPCHK(launch_gemm(lin_fwd(*m->sc[t], c->x[t].f(), dx, c->y[t].f(), dg, nl, 1), s));
    if (m->b_si2[t].f()) HIPCHK(launch_row_bias(nl, dg, m->b_si2[t].f(), c->y[t].f(), s));
  }
  {
    Region r(c, s, C_GATE_FWD, 0, nl * 4.0 * (dg + irreps_dim(m->irreps[t + 1])));
    HIPCHK(launch_gate_fwd((int)nl, last, m->gdims[t], c->y[t].f(), c->x[t + 1].f(), s));
  }
  return E3GNN_OK;
}

int e3gnn_layer_forward(e3gnn_ctx* c, int t, void* stream) {
  const int rc = e3gnn_layer_forward_part(c, t, 0, stream);
  return rc ? rc : e3gnn_layer_forward_part(c, t, 1, stream);
}

int e3gnn_readout(e3gnn_ctx* c, float* energy, float* atomic_energy, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  e3gnn_model* m = c->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  if (c->gen) {
    HIPCHK(gen_readout(c->gen, m->gen, gen_graph(c), energy, atomic_energy, s));
    c->readout_done = 1;
    return E3GNN_OK;
  }
  const int64_t nl = c->nl;
  const int L = m->nlayer;
  {
    const int dl = irreps_dim(m->irreps[L]);
    const FcnDims& fd = m->fcnd;
    double flops = 2.0 * nl * dl, bytes = nl * 4.0 * (dl + 2);
    if (m->fcn) {   // forward and backward of every layer; x[L] in, dE/dx[L] out
      double mac = fd.w[fd.nh];
      for (int k = 0; k < fd.nh; ++k) mac += (double)fd.w[k] * fd.w[k + 1];
      flops = 4.0 * nl * mac;
      bytes = nl * 4.0 * (2 * dl + 2);
    }
    Region r(c, s, C_READOUT, flops, bytes);
    if (m->fcn)   // the FCN readout with its backward in one launch: eat and dE/dx[L]
      HIPCHK(launch_readout_fcn((int)nl, fd, c->x[L].f(), m->fcn_w.f(), c->type.i(), m->scale.f(),
                                m->shift.f(), c->eat.f(), c->grad[L].f(), s));
    else
      HIPCHK(launch_readout((int)nl, dl, c->x[L].f(), m->readout_v.f(), c->type.i(), m->scale.f(),
                            m->shift.f(), c->eat.f(), s));
    HIPCHK(launch_sum(nl, c->eat.f(), c->part.f(), energy ? energy : c->scratch6.f(), s));
    if (atomic_energy && nl > 0)
      HIPCHK(hipMemcpyAsync(atomic_energy, c->eat.p, nl * 4, hipMemcpyDeviceToDevice, s));
    if (!m->fcn)
      HIPCHK(launch_readout_bwd((int)nl, dl, m->readout_v.f(), c->type.i(), m->scale.f(),
                                c->grad[L].f(), s));
  }
  c->readout_done = 1;
  return E3GNN_OK;
}

// The convolution backward of the v1 cross-check (impl 1), over all edges:
// the tensor-product backward writes dE/dw per edge, the radial MLP's backward
// reads it.
static int v1_conv_backward(e3gnn_ctx* c, int t, hipStream_t s) {
  e3gnn_model* m = c->m;
  const int64_t nl = c->nl, E = c->E;
  const int dx = irreps_dim(m->irreps[t]), dm = irreps_dim(m->mid[t]), W = m->W[t];
  const int kind = t == 0 ? 0 : (t == m->nlayer - 1 ? 2 : 1);
  {
    Region r(c, s, C_TP_BWD, 3.0 * tp_flops_per_edge(m->kcode(t)) * E,
             (double)E * 4 * (2 * W + 2 * 9 + dx + (t > 0 ? dx : 0) + 2) + nl * 4.0 * dm);
    TpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.row_ptr = c->row_ptr.i();
    a.nbr = c->nbr.i();
    a.Y = c->Y.f();
    a.w = c->w[t].f();
    a.h = c->h[t].f();
    a.gagg = c->agg.f();
    a.dw = c->dw.f();
    a.dxc = t > 0 ? c->dxc.f() : nullptr;
    a.dYacc = c->dY.f();
    a.n_centers = (int)nl;
    HIPCHK(launch_tp_bwd(kind, a, s));
  }
  {
    Region r(c, s, C_MLP_BWD, 2.0 * E * (64 * W + 64 * 64 + 64 * 8),
             (double)E * 4 * (W + 64 * 6 + 16));
    auto& mm = m->mlp[t];
    GemmBatch b;
    std::memset(&b, 0, sizeof(b));
    GemmProb p = base_prob();
    p.A = c->dw.f(); p.lda = W; p.K = W;
    p.B = mm.w2t.f(); p.ldb = 64; p.N = 64;
    p.C = c->H2.f(); p.ldc = 64; p.M = (int)E;
    p.act = 2; p.pre_in = c->a2[t].f();
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
    std::memset(&b, 0, sizeof(b));
    p.A = c->H2.f(); p.lda = 64; p.K = 64;
    p.B = mm.w1t.f(); p.C = c->H1.f(); p.pre_in = c->a1[t].f();
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
    std::memset(&b, 0, sizeof(b));
    p.A = c->H1.f(); p.B = mm.w0t.f(); p.ldb = 8; p.N = 8;
    p.C = c->demb.f(); p.ldc = 8; p.act = 0; p.pre_in = nullptr; p.beta = 1;
    add_prob(b, p);
    HIPCHK(launch_gemm(b, s));
  }
  return E3GNN_OK;
}

// Parts of a block's backward for the halo overlap (e3gnn.h): part 0 makes
// everything the GHOST rows of dE/dx need (gate + si2 backward of the owned
// rows, the boundary centres' edges, the ghost rows' gather and
// self_interaction_1 backward), so the reverse exchange can start; part 1 does
// the interior centres and the owned rows.  The v1 kernels run whole in part 0.
int e3gnn_layer_backward_part(e3gnn_ctx* c, int t, int part, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  e3gnn_model* m = c->m;
  if (t < 0 || t >= m->nlayer) return fail(E3GNN_ERR_ARG, "layer out of range");
  if (part != 0 && part != 1) return fail(E3GNN_ERR_ARG, "part must be 0 or 1");
  if (!c->readout_done) return fail(E3GNN_ERR_ARG, "e3gnn_readout must precede the backward");
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  // generic engine: the whole layer before the reverse halo of dE/dx[t] (part 0)
  if (c->gen) {
    if (part == 0) HIPCHK(gen_layer_backward(c->gen, m->gen, gen_graph(c), t, s));
    return E3GNN_OK;
  }
  const int64_t n = c->n, nl = c->nl, E = c->E;
  const int dx = irreps_dim(m->irreps[t]), dg = irreps_dim(m->gin[t]);
  const int dm = irreps_dim(m->mid[t]), W = m->W[t];
  const bool last = t == m->nlayer - 1;
  const int kind = t == 0 ? 0 : (last ? 2 : 1);   // block kind (timing class)
  const int code = m->kcode(t);                    // fused kernel kind code
  const int64_t n_int = c->n_int, e_int = c->e_int;
  // gate + self_interaction_2 backward of the owned rows
  auto out_bwd = [&]() -> int {
    {
      Region r(c, s, C_GATE_BWD, 0, nl * 4.0 * (2 * dg + irreps_dim(m->irreps[t + 1])));
      HIPCHK(launch_gate_bwd((int)nl, last, m->gdims[t], c->y[t].f(), c->grad[t + 1].f(), c->dy.f(), s));
    }
    Region r(c, s, C_LINEAR, lin_flops(*m->si2[t], nl));
    NlBatch nb;
    if (c->nodelin && nl_batch(nb, *m->nl_si2t[t], c->dy.f(), dg, nullptr, 0, c->agg.f(), dm, nl, 0))
      HIPCHK(launch_nodelin(nb, s));
    else
      HIPCHK(launch_gemm(lin_bwd(*m->si2[t], c->dy.f(), dg, c->agg.f(), dm, nl, 0), s));
    return E3GNN_OK;
  };
  // dE/dx of the block's input rows [r0, r1): the transposed-CSR gather of the
  // per-edge dE/dx (dxc) where the convolution wrote that, self_interaction_1
  // backward, and with the owned rows [0, nl) the self-connection's backward
  auto in_bwd = [&](int64_t r0, int64_t r1, bool gather, bool owned) -> int {
    if (t == 0) return E3GNN_OK;
    if (gather && r1 > r0) {
      Region r(c, s, C_GATHER, 0, (double)E * 4 * (dx + 1) * (r1 - r0) / std::max<int64_t>(n, 1) +
                                      (r1 - r0) * 4.0 * dx);
      HIPCHK(launch_gather_rows_range((int)r0, (int)r1, dx, c->src_ptr.i(), c->src_perm.i(),
                                      c->dxc.f(), c->dh.f(), s));
    }
    Region r(c, s, C_LINEAR, lin_flops(*m->si1[t], r1 - r0) + (owned ? lin_flops(*m->sc[t], nl) : 0));
    // k_nodelin: owned rows [0, nl) as one si1^T + sc^T problem per block,
    // the remaining rows (ghosts) si1^T alone
    NlBatch b0, b1;
    const int64_t p1 = owned ? nl : r0;  // first row of the si1^T-only range
    if (c->nodelin && (!owned || r0 == 0) && r1 >= p1 &&
        (!owned || nl_batch(b0, *m->nl_bwd[t], c->dh.f(), dx, c->dy.f(), dg, c->grad[t].f(), dx, nl, 0)) &&
        (r1 == p1 || nl_batch(b1, *m->nl_si1t[t], c->dh.f() + p1 * dx, dx, nullptr, 0,
                              c->grad[t].f() + p1 * dx, dx, r1 - p1, 0))) {
      if (owned) HIPCHK(launch_nodelin(b0, s));
      if (r1 > p1) HIPCHK(launch_nodelin(b1, s));
    } else {
      if (r1 > r0)
        HIPCHK(launch_gemm(lin_bwd(*m->si1[t], c->dh.f() + r0 * dx, dx, c->grad[t].f() + r0 * dx, dx,
                                   r1 - r0, 0), s));
      if (owned) HIPCHK(launch_gemm(lin_bwd(*m->sc[t], c->dy.f(), dg, c->grad[t].f(), dx, nl, 1), s));
    }
    return E3GNN_OK;
  };
  if (c->graph_impl == 1) {  // the v1 cross-check: all rows and edges, in part 0
    if (part == 1) return E3GNN_OK;
    if (const int rc = out_bwd()) return rc;
    if (const int rc = v1_conv_backward(c, t, s)) return rc;
    return in_bwd(0, n, true, true);
  }
  if (part == 0) {
    if (const int rc = out_bwd()) return rc;
  }
  // fused radial-MLP + tensor-product backward (fused.hip).  First / middle
  // blocks: per-edge dE/dx (dxc) + transposed-CSR gather; the last block (224
  // message channels) writes dE/dx per neighbour node
  FusedArgs a = fused_base(c, t);
  a.gagg = c->agg.f();
  a.center = c->center.i();
  a.n_edges = (int)E;
  a.src_ptr = c->src_ptr.i();
  a.src_perm = c->src_perm.i();
  a.dh = c->dh.f();  // the last block writes its dE/dx rows here
  a.dxc = (!last && t > 0) ? c->dxc.f() : nullptr;
  a.dgu = c->dgu.f();
  a.embd = c->embd.f();
  a.drad = c->drad.f();
  // part 0: boundary centres / their edges / ghost neighbour nodes
  a.c_begin = (int)(part == 0 ? n_int : 0);
  a.c_end = (int)(part == 0 ? nl : n_int);
  // (graph_set checked every centre to lie in [0, nl): row_ptr[nl] == E, and
  // e_int is row_ptr[n_int])
  a.e_begin = (int)(part == 0 ? e_int : 0);
  a.e_end = (int)(part == 0 ? E : e_int);
  a.node_begin = (int)(part == 0 ? nl : 0);
  a.node_end = (int)(part == 0 ? n : nl);
  double ef = (double)(part == 0 ? E - e_int : e_int);
  if (last && c->timing && a.node_end > a.node_begin) {
    // the last block's launch covers the edges of its neighbour-node range
    int32_t q[2];
    HIPCHK(hipMemcpyAsync(&q[0], a.src_ptr + a.node_begin, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&q[1], a.src_ptr + a.node_end, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ef = (double)(q[1] - q[0]);
  }
  // empty ranges launch nothing (and are not counted as launches)
  if (last ? a.node_end > a.node_begin : a.c_end > a.c_begin) {
    // algorithmic FLOP (the forward radial MLP the kernel recomputes is not
    // counted): dE/dx + dE/dY = 2 x TP; dE/dw = TP, dH2 = dw W2^T, MLP chain
    const double xf = 3.0 * tp_flops_per_edge(code) + 2.0 * (64 * W + 64 * 64 + 8 * 64);
    Region r(c, s, C_CONV_BWD_X + kind, xf * ef,
             ef * 4 * (8 + 9 + 2 + 3 + 8) + (a.c_end - a.c_begin) * 4.0 * dm);
    HIPCHK(last ? launch_conv_bwd_nbr_last(code, a, s) : launch_conv_bwd_ls(code, a, s));
  }
  // rows of this part: ghosts [nl, n) in part 0, owned [0, nl) in part 1
  return part == 0 ? in_bwd(nl, n, !last, false) : in_bwd(0, nl, !last, true);
}

int e3gnn_layer_backward(e3gnn_ctx* c, int t, void* stream) {
  const int rc = e3gnn_layer_backward_part(c, t, 0, stream);
  return rc ? rc : e3gnn_layer_backward_part(c, t, 1, stream);
}

int e3gnn_forces(e3gnn_ctx* c, float* forces, float* virial6, float* edge_grad, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  e3gnn_model* m = c->m;
  HIPCHK(hipSetDevice(m->device));
  hipStream_t s = (hipStream_t)stream;
  if (c->gen) {
    HIPCHK(gen_forces(c->gen, m->gen, gen_graph(c), forces, virial6, edge_grad, s));
    c->forces_done = 1;
    return E3GNN_OK;
  }
  const int64_t n = c->n, nl = c->nl, E = c->E;
  {
    Region r(c, s, C_EDGE_FORCE, 0, (double)E * 4 * (3 + 9 + (c->graph_impl == 1 ? 8 : 1) + 3));
    HIPCHK(launch_edge_force(E, c->vec.f(), m->coeffs.f(), m->cutoff, m->r_on, m->raw_sh, c->dY.f(),
                             c->dgu.f(), c->graph_impl == 1 ? c->demb.f() : nullptr,
                             c->graph_impl == 1 ? nullptr : c->drad.f(), c->fe.f(), c->vpart.f(), s));
    HIPCHK(launch_final_sum(edge_force_blocks(E), 6, c->vpart.f(),
                            virial6 ? virial6 : c->scratch6.f(), s));
  }
  if (forces) {
    Region r(c, s, C_ATOM_FORCE, 0, (double)E * 4 * 2 * 4 + n * 12.0);
    HIPCHK(launch_atom_force((int)n, (int)nl, c->row_ptr.i(), c->src_ptr.i(), c->src_perm.i(),
                             c->fe.f(), forces, s));
  }
  if (edge_grad && E > 0)
    HIPCHK(hipMemcpyAsync(edge_grad, c->fe.p, E * 12, hipMemcpyDeviceToDevice, s));
  c->forces_done = 1;
  return E3GNN_OK;
}

int e3gnn_atom_virial(e3gnn_ctx* c, float* atom_virial6, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  if (!atom_virial6) return fail(E3GNN_ERR_ARG, "null atom_virial6 output");
  if (!c->forces_done)
    return fail(E3GNN_ERR_ARG, "e3gnn_forces (or e3gnn_energy_forces) on the current graph must "
                               "precede e3gnn_atom_virial");
  HIPCHK(hipSetDevice(c->m->device));
  hipStream_t s = (hipStream_t)stream;
  // stream-ordered mode: the per-edge dE/dr is ready at the end of the last
  // evaluation (done_ev), and a later graph_set on another stream must not
  // overwrite it under this launch (done_ev moves behind it)
  const bool ordered = c->done_pending;
  if (ordered && c->done_stream != s) HIPCHK(hipStreamWaitEvent(s, c->done_ev, 0));
  const float* fe = c->gen ? gen_fe(c->gen) : c->fe.f();
  {
    // both index lists, edge_vec and dE/dr once per edge end; one row out
    Region r(c, s, C_ATOM_VIRIAL, 18.0 * 2 * c->E, (double)c->E * 4 * 2 * 7 + c->n * 24.0);
    HIPCHK(launch_atom_virial((int)c->n, (int)c->nl, c->row_ptr.i(), c->src_ptr.i(),
                              c->src_perm.i(), c->vec.f(), fe, atom_virial6, s));
  }
  if (ordered) {
    HIPCHK(hipEventRecord(c->done_ev, s));
    c->done_stream = s;
  }
  return E3GNN_OK;
}

int e3gnn_energy_forces(e3gnn_ctx* c, int64_t n_atoms, int64_t n_edges, const int32_t* type,
                        const int32_t* edge_center, const int32_t* edge_nbr,
                        const float* edge_vec, float* energy, float* atomic_energy,
                        float* forces, float* virial6, float* edge_grad, void* stream) {
  if (!energy) return fail(E3GNN_ERR_ARG, "energy output is required");
  int rc = e3gnn_graph_set(c, n_atoms, 0, n_edges, type, edge_center, edge_nbr, edge_vec, stream);
  if (rc) return rc;
  const int L = c->m->nlayer;
  for (int t = 0; t < L; ++t)
    if ((rc = e3gnn_layer_forward(c, t, stream))) return rc;
  if ((rc = e3gnn_readout(c, energy, atomic_energy, stream))) return rc;
  for (int t = L - 1; t >= 0; --t)
    if ((rc = e3gnn_layer_backward(c, t, stream))) return rc;
  if ((rc = e3gnn_forces(c, forces, virial6, edge_grad, stream))) return rc;
  if (!c->stream_ordered) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  } else {
    if (!c->done_ev) HIPCHK(hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->done_ev, (hipStream_t)stream));
    c->done_stream = (hipStream_t)stream;
    c->done_pending = true;
  }
  return E3GNN_OK;
}

int e3gnn_segment_sum(int64_t n_segments, const int32_t* ptr, int64_t n_rows, int width,
                      const float* in, float* out, void* stream) {
  if (n_segments < 1 || n_segments >= (1LL << 30))
    return fail(E3GNN_ERR_ARG, "segment sum: the number of segments must be in [1, 2^30)");
  if (n_rows < 0 || n_rows > (1LL << 30)) return fail(E3GNN_ERR_ARG, "segment sum: row count out of range");
  if (width != 1 && width != 6) return fail(E3GNN_ERR_ARG, "segment sum: width must be 1 or 6");
  if (!ptr || !out || (n_rows > 0 && !in)) return fail(E3GNN_ERR_ARG, "segment sum: null array");
  HIPCHK(launch_segment_sum((int)n_segments, ptr, (int)n_rows, width, in, out, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_energy_forces_batch(e3gnn_ctx* c, int64_t n_atoms, int64_t n_edges, int64_t B,
                              const int32_t* atom_ptr, const int32_t* type,
                              const int32_t* edge_center, const int32_t* edge_nbr,
                              const float* edge_vec, float* energy, float* atomic_energy,
                              float* forces, float* virial6, float* edge_grad, void* stream) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  if (B < 1 || B >= (1LL << 30))
    return fail(E3GNN_ERR_ARG, "batch: the number of structures must be in [1, 2^30)");
  if (B > n_atoms) return fail(E3GNN_ERR_ARG, "batch: more structures than atoms");
  if (!atom_ptr) return fail(E3GNN_ERR_ARG, "batch: null atom_ptr");
  if (!energy) return fail(E3GNN_ERR_ARG, "energy output is required");
  // the evaluation of e3gnn_energy_forces on the concatenated graph ...
  int rc = e3gnn_graph_set(c, n_atoms, 0, n_edges, type, edge_center, edge_nbr, edge_vec, stream);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* eat = atomic_energy;
  if (!eat) {
    HIPCHK(c->beat.ensure((size_t)n_atoms * sizeof(float)));
    eat = c->beat.f();
  }
  if (virial6) HIPCHK(c->bw.ensure((size_t)n_atoms * 6 * sizeof(float)));
  const int L = c->m->nlayer;
  for (int t = 0; t < L; ++t)
    if ((rc = e3gnn_layer_forward(c, t, stream))) return rc;
  if ((rc = e3gnn_readout(c, nullptr, eat, stream))) return rc;
  for (int t = L - 1; t >= 0; --t)
    if ((rc = e3gnn_layer_backward(c, t, stream))) return rc;
  if ((rc = e3gnn_forces(c, forces, nullptr, edge_grad, stream))) return rc;
  // ... then the per-structure sums in a fixed order (segment_sum.hip): the
  // energies from the atomic energies, the virials from the per-atom virials
  // (both atoms of every edge lie in one structure, so its rows sum to its virial)
  HIPCHK(launch_segment_sum((int)B, atom_ptr, (int)n_atoms, 1, eat, energy, s));
  if (virial6) {
    if ((rc = e3gnn_atom_virial(c, c->bw.f(), stream))) return rc;
    HIPCHK(launch_segment_sum((int)B, atom_ptr, (int)n_atoms, 6, c->bw.f(), virial6, s));
  }
  if (!c->stream_ordered) {
    HIPCHK(hipStreamSynchronize(s));
  } else {
    if (!c->done_ev) HIPCHK(hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->done_ev, s));
    c->done_stream = s;
    c->done_pending = true;
  }
  return E3GNN_OK;
}

int e3gnn_halo_pack(const int32_t* idx, int64_t n, int dim, const float* src, int64_t src_stride,
                    float* dst, void* stream) {
  if (n < 0 || dim <= 0) return fail(E3GNN_ERR_ARG, "bad halo size");
  HIPCHK(launch_pack(n, dim, idx, src, src_stride, dst, (hipStream_t)stream));
  return E3GNN_OK;
}
int e3gnn_halo_unpack(const int32_t* idx, int64_t n, int dim, const float* src, float* dst,
                      int64_t dst_stride, int accumulate, void* stream) {
  if (n < 0 || dim <= 0) return fail(E3GNN_ERR_ARG, "bad halo size");
  HIPCHK(launch_unpack(n, dim, idx, src, dst, dst_stride, accumulate, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_set_interior(e3gnn_ctx* c, int64_t n_interior) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  if (n_interior < 0) return fail(E3GNN_ERR_ARG, "negative n_interior");
  c->n_interior_req = n_interior;
  return E3GNN_OK;
}

int e3gnn_set_impl(e3gnn_ctx* c, int impl) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  if (impl != 0 && impl != 1) return fail(E3GNN_ERR_ARG, "impl must be 0 (fused) or 1 (v1)");
  c->impl = impl;
  return E3GNN_OK;
}

int e3gnn_set_timing(e3gnn_ctx* c, int enable) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  c->flush();
  c->timing = enable != 0;
  return E3GNN_OK;
}
int e3gnn_set_stream_ordered(e3gnn_ctx* c, int enable) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  c->stream_ordered = enable != 0;
  return E3GNN_OK;
}
int e3gnn_kernel_stats(e3gnn_ctx* c, const char** names, double* ms, int64_t* launches,
                       double* flops, double* bytes, int max) {
  if (!c) return -1;
  c->flush();
  for (int i = 0; i < C_NCLS && i < max; ++i) {
    if (names) names[i] = kClassNames[i];
    if (ms) ms[i] = c->stats[i].ms;
    if (launches) launches[i] = c->stats[i].launches;
    if (flops) flops[i] = c->stats[i].flops;
    if (bytes) bytes[i] = c->stats[i].bytes;
  }
  return C_NCLS;
}
int e3gnn_reset_stats(e3gnn_ctx* c) {
  if (!c) return fail(E3GNN_ERR_ARG, "null context");
  c->flush();
  for (auto& st : c->stats) st = Stat();
  return E3GNN_OK;
}

int e3gnn_cg_table(int l1, int l2, int l3, float* out) {
  if (!out) return fail(E3GNN_ERR_ARG, "null out");
  const int key = l1 * 100 + l2 * 10 + l3;
  switch (key) {
#define CGCASE(a, b, c) \
  case a * 100 + b * 10 + c: dense_cg<a, b, c>(out); return E3GNN_OK;
    CGCASE(0, 0, 0) CGCASE(0, 1, 1) CGCASE(0, 2, 2) CGCASE(1, 0, 1) CGCASE(1, 1, 0)
    CGCASE(1, 1, 1) CGCASE(1, 1, 2) CGCASE(1, 2, 1) CGCASE(1, 2, 2) CGCASE(2, 0, 2)
    CGCASE(2, 1, 1) CGCASE(2, 1, 2) CGCASE(2, 2, 0) CGCASE(2, 2, 1) CGCASE(2, 2, 2)
#undef CGCASE
    default: return fail(E3GNN_ERR_ARG, "no coupling table for this (l1,l2,l3)");
  }
}

float* e3gnn_debug_ptr(e3gnn_ctx* c, const char* name, int layer, int64_t* numel) {
  if (!c || !name) return nullptr;
  const std::string n(name);
  const e3gnn_model* m = c->m;
  const int L = m->nlayer;
  auto ok = [&](int lo, int hi) { return layer >= lo && layer <= hi; };
  float* p = nullptr;
  int64_t k = 0;
  if (n == "x" && ok(0, L)) { p = c->x[layer].f(); k = c->n * irreps_dim(m->irreps[layer]); }
  else if (n == "grad" && ok(0, L)) { p = c->grad[layer].f(); k = c->n * irreps_dim(m->irreps[layer]); }
  else if (n == "h" && ok(0, L - 1)) { p = c->h[layer].f(); k = c->n * irreps_dim(m->irreps[layer]); }
  else if (n == "y" && ok(0, L - 1)) { p = c->y[layer].f(); k = c->nl * irreps_dim(m->gin[layer]); }
  else if (n == "agg" && ok(0, L - 1)) { p = c->agg.f(); k = c->nl * irreps_dim(m->mid[layer]); }
  else if (n == "Y") { p = c->Y.f(); k = c->E * 9; }
  else if (n == "emb") { p = c->emb.f(); k = c->E * 8; }
  else if (n == "dY") { p = c->dY.f(); k = c->E * 9; }
  else if (n == "dgu") { p = c->dgu.f(); k = c->E * 3; }
  else if (n == "demb" && c->graph_impl == 1) { p = c->demb.f(); k = c->E * 8; }
  else if (n == "embd" && c->graph_impl != 1) { p = c->embd.f(); k = c->E * 8; }
  else if (n == "drad" && c->graph_impl != 1) { p = c->drad.f(); k = c->E; }
  else if (n == "dxc") { p = c->dxc.f(); k = c->E * 480; }
  else if (n == "fe") { p = c->fe.f(); k = c->E * 3; }
  if (numel) *numel = p ? k : 0;
  return p;
}

int64_t e3gnn_workspace_bytes(const e3gnn_ctx* c) {
  if (!c) return 0;
  int64_t b = 0;
  const DBuf* fixed[] = {&c->type, &c->center, &c->nbr, &c->vec, &c->row_ptr, &c->src_ptr,
                         &c->src_perm, &c->cnt, &c->err, &c->Y, &c->emb, &c->dY, &c->dgu, &c->demb,
                         &c->embd, &c->drad,
                         &c->fe, &c->H1, &c->H2, &c->agg, &c->dw, &c->dxc, &c->dy, &c->dh,
                         &c->eat, &c->part, &c->vpart, &c->scratch6, &c->beat, &c->bw};
  for (auto* d : fixed) b += (int64_t)d->cap;
  for (auto* v : {&c->x, &c->grad, &c->h, &c->y, &c->w, &c->a1, &c->a2})
    for (auto& d : *v) b += (int64_t)d.cap;
  return b;
}

}  // extern "C"
