// The stateless entry points of the C ABI (include/e3gnn.h) over caller-owned
// device tensors: the grouped GEMM, the loss and EWC terms, and the kernel
// side of the fine-tune step -- convolution, radial MLP, edge geometry,
// generic path tables, activations / gates, column sums, the FCN readout.
// Argument checks and launches only; no model or context is read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "cg_tables.h"
#include "common.h"
#include "dbuf.h"
#include "error_sums.h"
#include "fcn_act.h"
#include "fcn_train.h"
#include "gtp.h"
#include "node.h"
#include "tgemm.h"
#include "tp.h"
#include "train_ops.h"

using namespace e3gnn;

extern "C" {

int64_t e3gnn_gemm_workspace_floats(int n, const e3gnn_gemm_desc* d) {
  if (n < 0 || (n > 0 && !d)) return -1;
  int64_t w = 0;
  for (int i = 0; i < n; ++i) {
    const int sp = tg_splits(d[i].m, d[i].n, (int64_t)d[i].k + d[i].k2);
    if (sp > 1) w += (int64_t)sp * d[i].m * d[i].n;
  }
  return w;
}

static int gemm_prob(const e3gnn_gemm_desc& q, int i, TgProb& p) {
  if (q.m < 0 || q.n < 0 || q.k < 0 || q.k2 < 0 || (q.m > 0 && q.n > 0 && (!q.c || (q.k > 0 && (!q.a || !q.b)) ||
                                                                      (q.k2 > 0 && (!q.a2 || !q.b2)))))
    return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: bad problem " + std::to_string(i));
  if (q.beta != 0 && q.beta != 1) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: beta must be 0 or 1");
  p = TgProb{};
  // op(A)(m, k): X[m][k] (ld, k contiguous) or X[k][m]; op(B)(k, n) as
  // element (n, k): B[k][n] or B[n][k]
  auto lay = [](const float* X, int64_t ld, bool kfast, int K) {
    return TgLay{X, kfast ? (int)ld : 1, kfast ? 1 : (int)ld, 0, 1, 0, K};
  };
  auto glay = [](const float* X, const e3gnn_gemm_layout& g) {
    return TgLay{X, (int)g.ld, (int)g.kst, (int)g.sst, g.rep, g.rs, g.ks};
  };
  if (q.layout) {
    const e3gnn_gemm_layouts& L = *q.layout;
    p.A1 = glay(q.a, L.a); p.B1 = glay(q.b, L.b); p.A2 = glay(q.a2, L.a2); p.B2 = glay(q.b2, L.b2);
    p.ldc = L.ldc; p.crep = L.crep; p.crs = L.crs; p.cns = L.cns;
  } else {
    p.A1 = lay(q.a, q.lda, !q.trans_a, q.k);
    p.B1 = lay(q.b, q.ldb, q.trans_b, q.k);
    p.A2 = lay(q.a2, q.lda2, !q.trans_a2, q.k2);
    p.B2 = lay(q.b2, q.ldb2, q.trans_b2, q.k2);
    p.ldc = q.ldc; p.crep = 1; p.crs = 0; p.cns = 1;
  }
  // the kernel addresses each operand through one buffer descriptor with
  // 32-bit byte offsets (TG_RECORDS, ~2 GB): refuse what would wrap
  {
    auto fits = [](const TgLay& L, int64_t rows, int64_t K, const e3gnn_gemm_layout* g) {
      if (g && (g->ld < 0 || g->kst < 0 || g->sst < 0 || g->rs < 0 || g->ld > INT32_MAX ||
                g->kst > INT32_MAX || g->sst > INT32_MAX))
        return false;
      if (L.ld < 0 || L.kst < 0 || L.sst < 0 || L.rs < 0) return false;
      if (rows <= 0 || K <= 0) return true;
      const int64_t rep = std::max(L.rep, 1), ks = L.ks > 0 ? L.ks : K;
      const int64_t off = (rows - 1) / rep * L.ld + std::min<int64_t>(rows - 1, rep - 1) * L.rs +
                          std::min<int64_t>(K - 1, ks - 1) * L.kst + (K - 1) / ks * L.sst;
      return off >= 0 && (off + 1) * 4 <= (int64_t)0x7fff0000;
    };
    const e3gnn_gemm_layouts* G = q.layout;
    const int64_t lds[4] = {q.lda, q.ldb, q.lda2, q.ldb2};
    for (int64_t v : lds)
      if (v < 0 || v > INT32_MAX) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: leading dimension beyond int32");
    if (!fits(p.A1, q.m, q.k, G ? &G->a : nullptr) || !fits(p.B1, q.n, q.k, G ? &G->b : nullptr) ||
        (q.k2 > 0 && (!fits(p.A2, q.m, q.k2, G ? &G->a2 : nullptr) || !fits(p.B2, q.n, q.k2, G ? &G->b2 : nullptr))))
      return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: problem " + std::to_string(i) +
                                     " addresses an operand beyond 2 GB (32-bit buffer offsets)");
  }
  // krange counts k rows; the kernel turns it into k steps, and with every
  // segment padded to whole steps a step index is k / BK in a one-segment
  // pair only
  if (q.krange && q.layout) {
    const e3gnn_gemm_layouts& L = *q.layout;
    auto segs = [](int K, int ks) { return K > 0 && ks > 0 && ks < K; };
    if (segs(q.k, L.a.ks) || segs(q.k, L.b.ks) || segs(q.k2, L.a2.ks) || segs(q.k2, L.b2.ks))
      return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: problem " + std::to_string(i) +
                                     " has krange with a layout of several K segments");
  }
  p.C = q.c;
  p.M = q.m; p.N = q.n; p.K1 = q.k; p.K2 = q.k2;
  p.alpha = q.alpha; p.beta = q.beta;
  p.kr = q.krange; p.kr_sm = q.krange_stride_m;
  p.splits = tg_splits(q.m, q.n, (int64_t)q.k + q.k2);
  return E3GNN_OK;
}

int e3gnn_gemm_grouped_ex(int n, const e3gnn_gemm_desc* d, float* workspace, int64_t workspace_floats,
                          int flags, void* stream) {
  if (n < 0 || n > TG_MAX_PROBS || (n > 0 && !d))
    return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: 0.." + std::to_string(TG_MAX_PROBS) + " problems");
  TgBatch b;
  int64_t used = 0;
  for (int i = 0; i < n; ++i) {
    TgProb p;
    if (int rc = gemm_prob(d[i], i, p)) return rc;
    if (p.splits > 1) {
      const int64_t need = (int64_t)p.splits * d[i].m * d[i].n;
      if (!workspace || used + need > workspace_floats)
        return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: workspace too small (e3gnn_gemm_workspace_floats)");
      p.ws = workspace + used;
      used += need;
    }
    if (!tg_add(b, p)) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_grouped: problem " + std::to_string(i));
  }
  HIPCHK(launch_tgemm(b, (hipStream_t)stream, !(flags & E3GNN_GEMM_DEFER_REDUCE)));
  return E3GNN_OK;
}

int e3gnn_gemm_grouped(int n, const e3gnn_gemm_desc* d, float* workspace, int64_t workspace_floats,
                       void* stream) {
  return e3gnn_gemm_grouped_ex(n, d, workspace, workspace_floats, 0, stream);
}

int e3gnn_gemm_reduce(int n, const e3gnn_gemm_desc* d, float* const* workspaces, void* stream) {
  if (n < 0 || (n > 0 && (!d || !workspaces))) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_reduce: bad arguments");
  TgRedBatch r;
  for (int i = 0; i < n; ++i) {
    TgProb p;
    if (int rc = gemm_prob(d[i], i, p)) return rc;
    if (p.splits <= 1 || p.M == 0 || p.N == 0) continue;   // reduced (or written) by its own launch
    {   // the split count its launch settled on (tg_add: whole k-step slices per split)
      TgBatch one;
      if (!tg_add(one, p)) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_reduce: problem " + std::to_string(i));
      p = one.p[0];
      if (p.splits <= 1) continue;
    }
    if (!workspaces[i]) return fail(E3GNN_ERR_ARG, "e3gnn_gemm_reduce: problem " + std::to_string(i) + " has no slabs");
    if (r.n == TG_MAX_RED) {   // launches of TG_MAX_RED problems, in order
      HIPCHK(launch_tgemm_reduce(r, (hipStream_t)stream));
      r = TgRedBatch{};
    }
    tg_red_add(r, TgRed{workspaces[i], p.C, p.ldc, p.crep, p.crs, p.cns, p.M, p.N, p.splits, p.alpha, p.beta});
  }
  HIPCHK(launch_tgemm_reduce(r, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_loss_efs(int criterion, float delta, int64_t nb, int64_t n, const float* e_pred,
                   const float* e_ref, const int64_t* natoms, const float* f_pred, const float* f_ref,
                   const float* s_pred, const float* s_ref, float w_e, float w_f, float w_s,
                   float s_scale, float* terms, float* ce, float* cf, float* cs, void* stream) {
  if (criterion != 0 && criterion != 1) return fail(E3GNN_ERR_ARG, "loss criterion must be 0 (mse) or 1 (huber)");
  if (nb < 0 || n < 0 || !terms || (nb > 0 && (!e_pred || !e_ref || !natoms || !ce)) ||
      (n > 0 && (!f_pred || !f_ref || !cf)) || (s_pred && (!s_ref || !cs)))
    return fail(E3GNN_ERR_ARG, "null loss operand");
  LossArgs a{criterion, delta, nb, n, e_pred, e_ref, natoms, f_pred, f_ref, s_pred, s_ref,
             w_e, w_f, w_s, s_scale, terms, ce, cf, cs};
  HIPCHK(launch_loss_efs(a, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_ewc_flat(int64_t n, const float* theta, const float* f, const float* o, const float* f_train,
                   float lam, float* grad, float* part, float* value, void* stream) {
  if (n < 0 || (n > 0 && (!theta || !f || !o || !part || (grad && !f_train))) || !value)
    return fail(E3GNN_ERR_ARG, "null EWC operand");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(launch_ewc_flat(n, theta, f, o, f_train, lam, grad, part, s));
  // fixed-order block sums into part[n ...], then their sum (node.hip launch_sum)
  HIPCHK(launch_sum(n, part, part + n, value, s));
  return E3GNN_OK;
}

int e3gnn_error_sums(int criterion, float delta, int64_t nb, int64_t n, const float* e_pred,
                     const float* e_ref, const int64_t* natoms, const float* f_pred, const float* f_ref,
                     const float* s_pred, const float* s_ref, float s_scale, double* sums, void* stream) {
  // (every rule before any HIP call)
  if (!sums) return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: null sums buffer");
  if (criterion != 0 && criterion != 1)
    return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: criterion must be 0 (mse) or 1 (huber)");
  if (nb < 0 || n < 0 || nb >= (int64_t)1 << 31 || n >= (int64_t)1 << 31)
    return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: nb / n out of range [0, 2^31)");
  if ((e_pred == nullptr) != (e_ref == nullptr) || (f_pred == nullptr) != (f_ref == nullptr) ||
      (s_pred == nullptr) != (s_ref == nullptr))
    return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: a prediction and its reference go together");
  if (nb > 0 && !natoms) return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: null natoms with nb > 0");
  if (nb > 0 && !e_pred) return fail(E3GNN_ERR_ARG, "e3gnn_error_sums: null energies with nb > 0");
  if (nb == 0 && n == 0) return E3GNN_OK;
  ErrSumArgs a{criterion, delta, nb, n, e_pred, e_ref, natoms, f_pred, f_ref, s_pred, s_ref, s_scale, sums};
  HIPCHK(launch_error_sums(a, (hipStream_t)stream));
  return E3GNN_OK;
}

// ------------------------------------------------------------ training ops
// Stateless convolution primitives over caller-owned device tensors, the
// kernel side of the fine-tune step (sevenn/train/trainer.py:155-222): the
// uvu tensor product + segmented sum (convolution.py:104-123) and its
// gradients w.r.t. all three operands.  The product is trilinear in
// (h, Y, w), so every derivative of any order is one of these two launches
// with permuted operands (sevennet_finetuning_amd/conv_ops.py).
namespace {
bool conv_kind_dims(int kind, int* dx, int* w, int* dm) {
  switch (kind) {
    case 0: *dx = LayerFirst::DX; *w = LayerFirst::W; *dm = LayerFirst::DM; return true;
    case 1: *dx = LayerMid::DX; *w = LayerMid::W; *dm = LayerMid::DM; return true;
    case 2: *dx = LayerLast::DX; *w = LayerLast::W; *dm = LayerLast::DM; return true;
    default: return false;
  }
}
}  // namespace

int e3gnn_conv_dims(int kind, int* dx, int* w, int* dm) {
  int a, b, d;
  if (!conv_kind_dims(kind, &a, &b, &d)) return fail(E3GNN_ERR_ARG, "conv kind must be 0, 1 or 2");
  if (dx) *dx = a;
  if (w) *w = b;
  if (dm) *dm = d;
  return E3GNN_OK;
}

static int graph_check(int* err_d, hipStream_t s);   // reads the build's error bits (synchronises)

int e3gnn_conv_graph(int64_t n_nodes, int64_t n_edges, const int32_t* edge_center,
                     const int32_t* edge_nbr, int32_t* row_ptr, int32_t* src_ptr,
                     int32_t* src_perm, int32_t* scratch, void* stream) {
  if (n_nodes < 0 || n_edges < 0 || n_nodes >= (int64_t)1 << 31 || n_edges >= (int64_t)1 << 31)
    return fail(E3GNN_ERR_ARG, "conv graph size out of int32 range");
  if (!row_ptr || !src_ptr || !scratch || (n_edges > 0 && (!edge_center || !edge_nbr || !src_perm)))
    return fail(E3GNN_ERR_ARG, "null conv graph buffer");
  hipStream_t s = (hipStream_t)stream;
  int* err_d = scratch + n_nodes;
  if (n_nodes <= graph_small_max_nodes() && n_edges <= graph_small_max_edges()) {   // one workgroup, one launch
    HIPCHK(launch_build_graph_small(n_edges, (int)n_nodes, edge_center, edge_nbr, nullptr, nullptr, nullptr,
                                    nullptr, row_ptr, src_ptr, src_perm, err_d, s));
  } else {
    HIPCHK(hipMemsetAsync(err_d, 0, 4, s));
    HIPCHK(launch_build_graph(n_edges, (int)n_nodes, (int)n_nodes, edge_center, edge_nbr, row_ptr,
                              src_ptr, src_perm, scratch, err_d, s));
  }
  return graph_check(err_d, s);
}

int e3gnn_conv_graph_i64(int64_t n_nodes, int64_t n_edges, const int64_t* edge_center,
                         const int64_t* edge_nbr, int32_t* center_out, int32_t* nbr_out, int32_t* row_ptr,
                         int32_t* src_ptr, int32_t* src_perm, int32_t* scratch, void* stream) {
  if (n_nodes < 0 || n_edges < 0 || n_nodes >= (int64_t)1 << 31 || n_edges >= (int64_t)1 << 31)
    return fail(E3GNN_ERR_ARG, "conv graph size out of int32 range");
  if (n_nodes > graph_small_max_nodes() || n_edges > graph_small_max_edges())
    return fail(E3GNN_ERR_ARG, "e3gnn_conv_graph_i64: more than " + std::to_string(graph_small_max_nodes()) +
                                   " nodes or " + std::to_string(graph_small_max_edges()) +
                                   " edges (convert the indices and use e3gnn_conv_graph)");
  if (!row_ptr || !src_ptr || !scratch ||
      (n_edges > 0 && (!edge_center || !edge_nbr || !center_out || !nbr_out || !src_perm)))
    return fail(E3GNN_ERR_ARG, "null conv graph buffer");
  hipStream_t s = (hipStream_t)stream;
  int* err_d = scratch + n_nodes;
  HIPCHK(launch_build_graph_small(n_edges, (int)n_nodes, nullptr, nullptr, edge_center, edge_nbr, center_out,
                                  nbr_out, row_ptr, src_ptr, src_perm, err_d, s));
  return graph_check(err_d, s);
}

int e3gnn_conv_graph_small_max_nodes(void) { return graph_small_max_nodes(); }
int e3gnn_conv_graph_small_max_edges(void) { return graph_small_max_edges(); }

static int graph_check(int* err_d, hipStream_t s) {
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, err_d, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (err) {
    std::string msg = "invalid graph:";
    if (err & 1) msg += " edge_center not sorted non-decreasing;";
    if (err & 2) msg += " edge_center out of [0, n_nodes);";
    if (err & 4) msg += " edge_nbr out of [0, n_nodes);";
    return fail(E3GNN_ERR_GRAPH, msg);
  }
  return E3GNN_OK;
}

int e3gnn_conv_forward(int kind, int64_t n_nodes, const int32_t* row_ptr, const int32_t* edge_nbr,
                       const float* h, const float* Y, const float* w, float* agg,
                       void* stream) {
  return e3gnn_conv_forward_acc(kind, n_nodes, row_ptr, edge_nbr, h, Y, w, agg, 0, stream);
}

int e3gnn_conv_forward_acc(int kind, int64_t n_nodes, const int32_t* row_ptr,
                           const int32_t* edge_nbr, const float* h, const float* Y, const float* w,
                           float* agg, int accumulate, void* stream) {
  int dx, W, dm;
  if (!conv_kind_dims(kind, &dx, &W, &dm)) return fail(E3GNN_ERR_ARG, "conv kind must be 0, 1 or 2");
  if (n_nodes <= 0) return E3GNN_OK;
  if (!row_ptr || !h || !Y || !w || !agg) return fail(E3GNN_ERR_ARG, "null conv operand");
  TpArgs a{};
  a.row_ptr = row_ptr;
  a.nbr = edge_nbr;
  a.Y = Y;
  a.w = w;
  a.h = h;
  a.agg = agg;
  a.n_centers = (int)n_nodes;
  a.denom = 1.0f;
  a.acc_out = accumulate & 1;
  HIPCHK(launch_tp_fwd(kind, a, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_conv_backward(int kind, int64_t n_nodes, int64_t n_edges, const int32_t* row_ptr,
                        const int32_t* edge_nbr, const int32_t* src_ptr, const int32_t* src_perm,
                        const float* h, const float* Y, const float* w, const float* gagg,
                        float* dh, float* dY, float* dw, float* dxc, void* stream) {
  return e3gnn_conv_backward_acc(kind, n_nodes, n_edges, row_ptr, edge_nbr, src_ptr, src_perm, h, Y,
                                 w, gagg, dh, dY, dw, dxc, 0, stream);
}

int e3gnn_conv_backward_acc(int kind, int64_t n_nodes, int64_t n_edges, const int32_t* row_ptr,
                            const int32_t* edge_nbr, const int32_t* src_ptr,
                            const int32_t* src_perm, const float* h, const float* Y, const float* w,
                            const float* gagg, float* dh, float* dY, float* dw, float* dxc,
                            int accumulate, void* stream) {
  int dx, W, dm;
  if (!conv_kind_dims(kind, &dx, &W, &dm)) return fail(E3GNN_ERR_ARG, "conv kind must be 0, 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  const int acc_dh = accumulate & 1, acc_dY = accumulate & 2, acc_dw = accumulate & 4;
  if (n_edges <= 0 || n_nodes <= 0) {
    // no edges: zero gradients (the accumulated ones keep their values)
    if (dh && n_nodes > 0 && !acc_dh) HIPCHK(launch_zero(dh, n_nodes * dx, s));
    return E3GNN_OK;
  }
  if (!row_ptr || !edge_nbr || !h || !Y || !w || !gagg || !dY || !dw)
    return fail(E3GNN_ERR_ARG, "null conv operand");
  if (dh && (!dxc || !src_ptr || !src_perm))
    return fail(E3GNN_ERR_ARG, "dh needs dxc scratch and the transposed CSR");
  TpArgs a{};
  a.row_ptr = row_ptr;
  a.nbr = edge_nbr;
  a.Y = Y;
  a.w = w;
  a.h = h;
  a.gagg = gagg;
  a.dw = dw;
  a.dxc = dh ? dxc : nullptr;
  a.dYacc = dY;
  a.n_centers = (int)n_nodes;
  a.denom = 1.0f;
  a.acc_out = acc_dw ? 1 : 0;
  a.dy_assign = acc_dY ? 0 : 1;   // every edge's dY has one writer: no zeroing launch
  HIPCHK(launch_tp_bwd(kind, a, s));
  // the gather writes every row (zero without incoming edges): no zeroing launch
  if (dh) HIPCHK(launch_gather_rows((int)n_nodes, dx, src_ptr, src_perm, dxc, dh, s, acc_dh ? 1 : 0));
  return E3GNN_OK;
}

// ------------------------------------------------------------ fine-tune radial MLP
int e3gnn_radial_mlp_forward(int64_t n_rows, int width, const float* emb, const float* W0,
                             const float* W1, const float* W2, const float* a1_primal,
                             const float* a2_primal, float* a1, float* h1, float* a2, float* h2,
                             float* w, float act_scale, void* stream) {
  if (n_rows <= 0) return E3GNN_OK;
  if (n_rows > INT32_MAX || width <= 0 || width % 16)
    return fail(E3GNN_ERR_ARG, "radial MLP: width must be a positive multiple of 16");
  if (!emb || !W0 || !W1 || !W2 || !a1 || !h1 || !a2 || !h2 || !w ||
      ((a1_primal == nullptr) != (a2_primal == nullptr)))
    return fail(E3GNN_ERR_ARG, "null radial MLP operand");
  HIPCHK(launch_mlp_fwd((int)n_rows, width, emb, W0, W1, W2, a1_primal, a2_primal, a1, h1, a2, h2, w,
                        act_scale, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_radial_mlp_forward_p(int64_t n_rows, int width, const float* emb, const float* W0,
                               const float* W1, const float* W2, const void* w2_pieces,
                               const float* a1_primal, const float* a2_primal, float* a1, float* h1,
                               float* a2, float* h2, float* w, float act_scale, void* stream) {
  if (n_rows <= 0) return E3GNN_OK;
  if (n_rows > INT32_MAX || width <= 0 || width % 16)
    return fail(E3GNN_ERR_ARG, "radial MLP: width must be a positive multiple of 16");
  if (!emb || !W0 || !W1 || !W2 || !a1 || !h1 || !a2 || !h2 || !w ||
      ((a1_primal == nullptr) != (a2_primal == nullptr)))
    return fail(E3GNN_ERR_ARG, "null radial MLP operand");
  if (w2_pieces && reinterpret_cast<uintptr_t>(w2_pieces) % 16)
    return fail(E3GNN_ERR_ARG, "radial MLP: the W2 piece image must be 16-byte aligned");
  HIPCHK(launch_mlp_fwd((int)n_rows, width, emb, W0, W1, W2, a1_primal, a2_primal, a1, h1, a2, h2, w,
                        act_scale, (hipStream_t)stream, w2_pieces));
  return E3GNN_OK;
}

int64_t e3gnn_radial_mlp_w2_piece_bytes(int width) {
  return (width > 0 && width % 16 == 0) ? mlp_w2_piece_bytes(width) : -1;
}

int e3gnn_radial_mlp_w2_pieces(int n, const float* const* W2, const int32_t* widths, void* const* images,
                               void* stream) {
  if (n < 0 || n > 8 || (n > 0 && (!W2 || !widths || !images)))
    return fail(E3GNN_ERR_ARG, "e3gnn_radial_mlp_w2_pieces: 0..8 matrices");
  for (int i = 0; i < n; ++i)
    if (!W2[i] || !images[i] || widths[i] <= 0 || widths[i] % 16 || reinterpret_cast<uintptr_t>(images[i]) % 16)
      return fail(E3GNN_ERR_ARG, "e3gnn_radial_mlp_w2_pieces: matrix " + std::to_string(i));
  HIPCHK(launch_mlp_w2_pieces(n, W2, widths, images, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_radial_mlp_backward(int64_t n_rows, int width, const float* wb, const float* W0,
                              const float* W1, const float* W2, const float* a1, const float* a2,
                              const float* a1_tangent, const float* a2_tangent, float* a2b,
                              float* a1b, float* embb, float act_scale, void* stream) {
  return e3gnn_radial_mlp_backward_p(n_rows, width, wb, W0, W1, W2, nullptr, a1, a2, a1_tangent, a2_tangent,
                                     a2b, a1b, embb, act_scale, stream);
}

int e3gnn_radial_mlp_backward_p(int64_t n_rows, int width, const float* wb, const float* W0,
                                const float* W1, const float* W2, const void* w2_pieces, const float* a1,
                                const float* a2, const float* a1_tangent, const float* a2_tangent,
                                float* a2b, float* a1b, float* embb, float act_scale, void* stream) {
  if (n_rows <= 0) return E3GNN_OK;
  if (w2_pieces && reinterpret_cast<uintptr_t>(w2_pieces) % 16)
    return fail(E3GNN_ERR_ARG, "radial MLP backward: the W2 piece image must be 16-byte aligned");
  if (n_rows > INT32_MAX || width <= 0 || width % 16)
    return fail(E3GNN_ERR_ARG, "radial MLP backward: width must be a multiple of 16");
  if (!wb || !W0 || !W1 || !W2 || !a1 || !a2 || !embb ||
      ((a1_tangent == nullptr) != (a2_tangent == nullptr)))
    return fail(E3GNN_ERR_ARG, "null radial MLP operand");
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (!al(wb) || !al(W0) || !al(W1) || !al(W2))
    return fail(E3GNN_ERR_ARG, "radial MLP backward: wb / W0 / W1 / W2 must be 16-byte aligned");
  HIPCHK(launch_mlp_bwd((int)n_rows, width, wb, W0, W1, W2, a1, a2, a1_tangent, a2_tangent, a2b, a1b,
                        embb, act_scale, (hipStream_t)stream, w2_pieces));
  return E3GNN_OK;
}

// ------------------------------------------------------------ fine-tune edge geometry
int e3gnn_edge_geometry(int64_t n_edges, const float* vec, const float* coeffs, float rc, float ron,
                        int raw_sh, float* Y, float* emb, void* stream) {
  if (n_edges <= 0) return E3GNN_OK;
  if (!vec || !coeffs || !Y || !emb) return fail(E3GNN_ERR_ARG, "null edge geometry operand");
  HIPCHK(launch_edge_embed(n_edges, vec, coeffs, rc, ron, raw_sh, Y, emb, nullptr, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_edge_geometry_jvp(int64_t n_edges, const float* vec, const float* coeffs, float rc,
                            float ron, int raw_sh, const int32_t* center, const int32_t* nbr,
                            const int64_t* batch, const float* cF, const float* cS,
                            const float* vol, float* Yd, float* embd, float* rd, void* stream) {
  if (n_edges <= 0) return E3GNN_OK;
  if (!vec || !coeffs || !center || !nbr || !cF || !Yd || !embd || !rd ||
      (cS && (!batch || !vol)))
    return fail(E3GNN_ERR_ARG, "null edge geometry operand");
  HIPCHK(launch_edge_geom_jvp(n_edges, vec, coeffs, rc, ron, raw_sh, center, nbr, batch, cF, cS, vol,
                              Yd, embd, rd, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_edge_geometry_vjp(int64_t n_edges, const float* vec, const float* coeffs, float rc,
                            float ron, int raw_sh, const float* Yb, const float* embb, float* fij,
                            void* stream) {
  if (n_edges <= 0) return E3GNN_OK;
  if (!vec || !coeffs || !Yb || !embb || !fij) return fail(E3GNN_ERR_ARG, "null edge geometry operand");
  HIPCHK(launch_edge_force(n_edges, vec, coeffs, rc, ron, raw_sh, Yb, nullptr, embb, nullptr, fij, nullptr,
                           (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_edge_geometry_coeff_grad(int64_t n_edges, const float* vec, const float* coeffs, float rc,
                                   float ron, const float* embb, const float* embdb, const float* rd,
                                   float* out, void* stream) {
  if (n_edges <= 0) return E3GNN_OK;
  if (!vec || !coeffs || !embb || !embdb || !rd || !out)
    return fail(E3GNN_ERR_ARG, "null edge geometry operand");
  HIPCHK(launch_edge_geom_coeff(n_edges, vec, coeffs, rc, ron, embb, embdb, rd, out,
                                (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_edge_forces_to_atoms(int64_t n_nodes, const int32_t* row_ptr, const int32_t* src_ptr,
                               const int32_t* src_perm, const float* fij, float* F, void* stream) {
  if (n_nodes <= 0) return E3GNN_OK;
  if (!row_ptr || !src_ptr || !src_perm || !fij || !F) return fail(E3GNN_ERR_ARG, "null force operand");
  HIPCHK(launch_atom_force((int)n_nodes, (int)n_nodes, row_ptr, src_ptr, src_perm, fij, F,
                           (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_conv_tangent_forward(int kind, int64_t n_nodes, const int32_t* row_ptr,
                               const int32_t* edge_nbr, const float* h, const float* hd,
                               const float* Y, const float* Yd, const float* w, const float* wd,
                               float* agg, int accumulate, void* stream) {
  int dx, W, dm;
  if (!conv_kind_dims(kind, &dx, &W, &dm)) return fail(E3GNN_ERR_ARG, "conv kind must be 0, 1 or 2");
  if (n_nodes <= 0) return E3GNN_OK;
  if (!row_ptr || !h || !Y || !Yd || !w || !wd || !agg) return fail(E3GNN_ERR_ARG, "null conv operand");
  TpDualArgs a{};
  a.row_ptr = row_ptr;
  a.nbr = edge_nbr;
  a.Y = Y;
  a.Yd = Yd;
  a.w = w;
  a.wd = wd;
  a.h = h;
  a.hd = hd;
  a.agg = agg;
  a.n_centers = (int)n_nodes;
  a.acc_out = accumulate & 1;
  HIPCHK(launch_tp_fwd_tan(kind, a, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_conv_dual_backward(int kind, int64_t n_nodes, int64_t n_edges, const int32_t* row_ptr,
                             const int32_t* edge_nbr, const int32_t* src_ptr,
                             const int32_t* src_perm, const float* h, const float* hd,
                             const float* Y, const float* Yd, const float* w, const float* wd,
                             const float* g, const float* gd, float* dh, float* dhd, float* dw,
                             float* dwd, float* dxc, void* stream) {
  int dx, W, dm;
  if (!conv_kind_dims(kind, &dx, &W, &dm)) return fail(E3GNN_ERR_ARG, "conv kind must be 0, 1 or 2");
  hipStream_t s = (hipStream_t)stream;
  if (n_nodes <= 0) return E3GNN_OK;
  if ((hd == nullptr) != (dhd == nullptr))
    return fail(E3GNN_ERR_ARG, "dual conv backward: h' and dh' go together");
  if (n_edges <= 0) {
    HIPCHK(launch_zero(dh, n_nodes * dx, s));
    if (dhd) HIPCHK(launch_zero(dhd, n_nodes * dx, s));
    return E3GNN_OK;
  }
  if (!row_ptr || !edge_nbr || !src_ptr || !src_perm || !h || !Y || !Yd || !w || !wd || !g || !gd ||
      !dh || !dw || !dwd || !dxc)
    return fail(E3GNN_ERR_ARG, "null conv operand");
  TpDualArgs a{};
  a.row_ptr = row_ptr;
  a.nbr = edge_nbr;
  a.Y = Y;
  a.Yd = Yd;
  a.w = w;
  a.wd = wd;
  a.h = h;
  a.hd = hd;
  a.g = g;
  a.gd = gd;
  a.dw = dw;
  a.dwd = dwd;
  a.dxc = dxc;
  a.dxcd = dhd ? dxc + n_edges * dx : nullptr;
  a.n_centers = (int)n_nodes;
  HIPCHK(launch_tp_bwd_dual(kind, a, s));
  if (dhd)
    HIPCHK(launch_gather_rows2((int)n_nodes, dx, src_ptr, src_perm, dxc, dh, a.dxcd, dhd, s));
  else
    HIPCHK(launch_gather_rows((int)n_nodes, dx, src_ptr, src_perm, dxc, dh, s, 0));
  return E3GNN_OK;
}

// ------------------------------------------------------------ generic path tables
// (gtp.hip): the convolution of any nequip-family model from its instruction list
namespace {
void cg_entries(int l1, int l2, int l3, std::vector<CGEntry>& out) {
  auto add = [&](const CGEntry* e, int n) { out.assign(e, e + n); };
#define E3GNN_CG_CASE(a, b, c) \
  if (l1 == a && l2 == b && l3 == c) return add(CG<a, b, c>::e, CG<a, b, c>::n);
  E3GNN_CG_CASE(0, 0, 0) E3GNN_CG_CASE(0, 1, 1) E3GNN_CG_CASE(0, 2, 2)
  E3GNN_CG_CASE(1, 0, 1) E3GNN_CG_CASE(1, 1, 0) E3GNN_CG_CASE(1, 1, 1) E3GNN_CG_CASE(1, 1, 2)
  E3GNN_CG_CASE(1, 2, 1) E3GNN_CG_CASE(1, 2, 2) E3GNN_CG_CASE(2, 0, 2) E3GNN_CG_CASE(2, 1, 1)
  E3GNN_CG_CASE(2, 1, 2) E3GNN_CG_CASE(2, 2, 0) E3GNN_CG_CASE(2, 2, 1) E3GNN_CG_CASE(2, 2, 2)
#undef E3GNN_CG_CASE
  out.clear();
}
}  // namespace

struct e3gnn_gtp {
  int device = 0;
  GtpTables T{};
  DBuf by[4], ptr[4];
};

e3gnn_gtp* e3gnn_gtp_create(int n_paths, const int32_t* paths, int dx, int dy, int dw, int dm) {
  if (n_paths <= 0 || !paths || dx <= 0 || dy <= 0 || dw <= 0 || dm <= 0) {
    fail(E3GNN_ERR_ARG, "gtp: empty path table or dimensions");
    return nullptr;
  }
  std::vector<GtpTerm> terms;
  std::vector<CGEntry> cg;
  for (int p = 0; p < n_paths; ++p) {
    const int32_t* q = paths + 8 * p;
    const int l1 = q[0], l2 = q[1], l3 = q[2], mul = q[3], xo = q[4], yo = q[5], wo = q[6], mo = q[7];
    if (l1 < 0 || l2 < 0 || l3 < 0 || l1 > 2 || l2 > 2 || l3 > 2 || l3 < std::abs(l1 - l2) ||
        l3 > l1 + l2 || mul <= 0 || xo < 0 || yo < 0 || wo < 0 || mo < 0 ||
        xo + mul * (2 * l1 + 1) > dx || yo + 2 * l2 + 1 > dy || wo + mul > dw ||
        mo + mul * (2 * l3 + 1) > dm) {
      fail(E3GNN_ERR_ARG, "gtp: path " + std::to_string(p) + " out of range (l <= 2, offsets within dims)");
      return nullptr;
    }
    cg_entries(l1, l2, l3, cg);
    for (int u = 0; u < mul; ++u)
      for (auto& e : cg)
        terms.push_back({xo + u * (2 * l1 + 1) + e.i, yo + e.j, wo + u, mo + u * (2 * l3 + 1) + e.k, e.c});
  }
  auto* g = new e3gnn_gtp;
  if (hipGetDevice(&g->device) != hipSuccess) {
    delete g;
    fail(E3GNN_ERR_HIP, "gtp: no device");
    return nullptr;
  }
  const int dims[4] = {dm, dw, dx, dy};
  const GtpTerm* dev_by[4];
  const int* dev_ptr[4];
  for (int o = 0; o < 4; ++o) {
    // stable order by the output each term feeds (fixed summation order)
    auto key = [o](const GtpTerm& t) { return o == 0 ? t.m : (o == 1 ? t.w : (o == 2 ? t.x : t.y)); };
    std::vector<GtpTerm> s = terms;
    std::stable_sort(s.begin(), s.end(), [&](const GtpTerm& a, const GtpTerm& b) { return key(a) < key(b); });
    std::vector<int> ptr(dims[o] + 1, 0);
    for (auto& t : s) ptr[key(t) + 1]++;
    for (int i = 0; i < dims[o]; ++i) ptr[i + 1] += ptr[i];
    if (g->by[o].ensure(s.size() * sizeof(GtpTerm)) != hipSuccess ||
        g->ptr[o].ensure(ptr.size() * 4) != hipSuccess ||
        hipMemcpy(g->by[o].p, s.data(), s.size() * sizeof(GtpTerm), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->ptr[o].p, ptr.data(), ptr.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      delete g;
      fail(E3GNN_ERR_HIP, "gtp: table upload failed");
      return nullptr;
    }
    dev_by[o] = static_cast<const GtpTerm*>(g->by[o].p);
    dev_ptr[o] = static_cast<const int*>(g->ptr[o].p);
  }
  g->T = GtpTables{dx, dy, dw, dm, dev_by[0], dev_ptr[0], dev_by[1], dev_ptr[1],
                   dev_by[2], dev_ptr[2], dev_by[3], dev_ptr[3]};
  (void)hipGetLastError();
  return g;
}

void e3gnn_gtp_free(e3gnn_gtp* g) { delete g; }

extern "C++" {  // internal accessor for the generic engine (gtp.h; generic.cpp)
namespace e3gnn {
const GtpTables* gtp_tables(const e3gnn_gtp* g) { return &g->T; }
}  // namespace e3gnn
}

int e3gnn_gtp_dims(const e3gnn_gtp* g, int* dx, int* dy, int* dw, int* dm) {
  if (!g) return fail(E3GNN_ERR_ARG, "null gtp");
  if (dx) *dx = g->T.dx;
  if (dy) *dy = g->T.dy;
  if (dw) *dw = g->T.dw;
  if (dm) *dm = g->T.dm;
  return E3GNN_OK;
}

int e3gnn_gtp_forward(const e3gnn_gtp* g, int64_t n_nodes, const int32_t* row_ptr,
                      const int32_t* edge_nbr, const float* h, const float* Y, const float* w,
                      float* agg, void* stream) {
  if (!g) return fail(E3GNN_ERR_ARG, "null gtp");
  if (n_nodes <= 0) return E3GNN_OK;
  if (n_nodes >= (int64_t)1 << 31) return fail(E3GNN_ERR_ARG, "gtp: too many nodes");
  if (!row_ptr || !h || !Y || !w || !agg) return fail(E3GNN_ERR_ARG, "null gtp operand");
  HIPCHK(launch_gtp_fwd((int)n_nodes, row_ptr, edge_nbr, h, Y, w, g->T, agg, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_gtp_backward(const e3gnn_gtp* g, int64_t n_nodes, int64_t n_edges, const int32_t* row_ptr,
                       const int32_t* edge_nbr, const int32_t* src_ptr, const int32_t* src_perm,
                       const float* h, const float* Y, const float* w, const float* gagg,
                       float* dh, float* dY, float* dw, float* dxc, void* stream) {
  if (!g) return fail(E3GNN_ERR_ARG, "null gtp");
  hipStream_t s = (hipStream_t)stream;
  if (dh && n_nodes > 0) HIPCHK(launch_zero(dh, n_nodes * g->T.dx, s));
  if (n_edges <= 0 || n_nodes <= 0) return E3GNN_OK;
  if (n_nodes >= (int64_t)1 << 31 || n_edges >= (int64_t)1 << 31)
    return fail(E3GNN_ERR_ARG, "gtp: graph size out of int32 range");
  if (!row_ptr || !edge_nbr || !h || !Y || !w || !gagg || !dY || !dw)
    return fail(E3GNN_ERR_ARG, "null gtp operand");
  if (dh && (!dxc || !src_ptr || !src_perm))
    return fail(E3GNN_ERR_ARG, "dh needs dxc scratch and the transposed CSR");
  HIPCHK(launch_gtp_bwd((int)n_nodes, row_ptr, edge_nbr, h, Y, w, gagg, g->T, dw, dh ? dxc : nullptr,
                        dY, s));
  if (dh) HIPCHK(launch_gather_rows((int)n_nodes, g->T.dx, src_ptr, src_perm, dxc, dh, s));
  return E3GNN_OK;
}

int e3gnn_act(int op, int64_t n, const float* x, const float* g, const float* gg, float* out0,
              float* out1, float scale, void* stream) {
  if (op < 0 || op > 2) return fail(E3GNN_ERR_ARG, "act op must be 0, 1 or 2");
  if (n < 0) return fail(E3GNN_ERR_ARG, "negative size");
  if (n > 0 && (!x || (op == 0 && !out0) || (op == 1 && (!g || !out0)) ||
                (op == 2 && (!g || !gg || (!out0 && !out1)))))
    return fail(E3GNN_ERR_ARG, "null act operand");
  HIPCHK(launch_act(op, n, x, g, gg, out0, out1, scale, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_gate(int op, int64_t n, const int32_t* dims, const float* y, const float* go,
               const float* q, float* out0, float* out1, float scale, void* stream) {
  if (op < 0 || op > 2) return fail(E3GNN_ERR_ARG, "gate op must be 0, 1 or 2");
  if (n < 0 || !dims) return fail(E3GNN_ERR_ARG, "bad gate arguments");
  if (dims[4] < 0 || dims[4] > 2) return fail(E3GNN_ERR_ARG, "at most two gated irreps");
  if (n > 0 && (!y || (op >= 1 && !go) || (op == 2 && !q) || (op < 2 && !out0)))
    return fail(E3GNN_ERR_ARG, "null gate operand");
  HIPCHK(launch_gate(op, n, dims, y, go, q, out0, out1, scale, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_act_dual(int64_t n, const float* x, const float* xd, const float* g, const float* gd,
                   float* og, float* ogd, float scale, void* stream) {
  if (n < 0) return fail(E3GNN_ERR_ARG, "negative size");
  if (n > 0 && (!x || !xd || !g || !gd || !og || !ogd)) return fail(E3GNN_ERR_ARG, "null act operand");
  HIPCHK(launch_act_dual(n, x, xd, g, gd, og, ogd, scale, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_gate_dual(int op, int64_t n, const int32_t* dims, const float* y, const float* yd,
                    const float* xb, const float* xdb, float* out0, float* out1, float scale,
                    void* stream) {
  if (op < 0 || op > 1) return fail(E3GNN_ERR_ARG, "gate_dual op must be 0 or 1");
  if (n < 0 || !dims) return fail(E3GNN_ERR_ARG, "bad gate arguments");
  if (dims[4] < 0 || dims[4] > 2) return fail(E3GNN_ERR_ARG, "at most two gated irreps");
  if (n > 0 && (!y || !yd || !out0 || (op == 1 && (!xb || !xdb || !out1))))
    return fail(E3GNN_ERR_ARG, "null gate operand");
  HIPCHK(launch_gate_dual(op, n, dims, y, yd, xb, xdb, out0, out1, scale, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_colsum_grouped(int n, const e3gnn_colsum_desc* blocks, void* stream) {
  if (n < 0 || n > COLSUM_MAX || (n > 0 && !blocks))
    return fail(E3GNN_ERR_ARG, "e3gnn_colsum_grouped: 0.." + std::to_string(COLSUM_MAX) + " blocks");
  ColsumBatch b{};
  for (int i = 0; i < n; ++i) {
    const e3gnn_colsum_desc& d = blocks[i];
    if (d.rows < 0 || d.cols < 0 || d.ld < d.cols || (d.rows > 0 && d.cols > 0 && (!d.src || !d.dst)))
      return fail(E3GNN_ERR_ARG, "e3gnn_colsum_grouped: block " + std::to_string(i));
    b.p[i] = ColsumProb{d.src, d.dst, d.ld, d.rows, d.cols};
  }
  b.n = n;
  HIPCHK(launch_colsum(b, (hipStream_t)stream));
  return E3GNN_OK;
}

// the FCN readout of the fine-tune step (fcn_train.hip): the inference
// kernel's limits (node.h FcnDims)
static int fcn_train_dims(int64_t n, int nh, const int32_t* widths, int act, float act_norm, FcnDims& d) {
  if (n < 0 || n > 0x7fffffff) return fail(E3GNN_ERR_ARG, "fcn_train: bad row count");
  if (nh < 1 || nh > FCN_MAX_HIDDEN || !widths)
    return fail(E3GNN_ERR_ARG, "fcn_train: 1.." + std::to_string(FCN_MAX_HIDDEN) + " hidden layers");
  if (act < 0 || act >= FCN_ACT_KINDS) return fail(E3GNN_ERR_ARG, "fcn_train: unknown activation");
  d = FcnDims{};
  d.nh = nh;
  for (int k = 0; k <= nh; ++k) {
    if (widths[k] < 1 || widths[k] > FCN_MAX_WIDTH)
      return fail(E3GNN_ERR_ARG, "fcn_train: widths of 1.." + std::to_string(FCN_MAX_WIDTH));
    d.w[k] = widths[k];
  }
  d.kind = act;
  d.c = act_norm;
  return E3GNN_OK;
}

int64_t e3gnn_fcn_packed_floats(int n_hidden, const int32_t* widths) {
  FcnDims d;
  if (fcn_train_dims(0, n_hidden, widths, 0, 1.f, d)) return -1;
  return d.padded_floats();
}

int e3gnn_fcn_train_forward(int64_t n, int n_hidden, const int32_t* widths, int act, float act_norm,
                            const float* weights, const float* x, const float* seed, float* z, float* a,
                            float* s, float* dx, void* stream) {
  FcnDims d;
  if (int rc = fcn_train_dims(n, n_hidden, widths, act, act_norm, d)) return rc;
  if (n > 0 && (!weights || !x || !z || !a || !s)) return fail(E3GNN_ERR_ARG, "fcn_train_forward: null operand");
  HIPCHK(launch_fcn_train_fwd((int)n, d, weights, x, seed, z, a, s, dx, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_fcn_train_tangent(int64_t n, int n_hidden, const int32_t* widths, int act, float act_norm,
                            const float* weights, const float* xd, const float* z, float* zd, float* a,
                            float* sd, void* stream) {
  FcnDims d;
  if (int rc = fcn_train_dims(n, n_hidden, widths, act, act_norm, d)) return rc;
  if (n > 0 && (!weights || !xd || !z || !zd || !a || !sd))
    return fail(E3GNN_ERR_ARG, "fcn_train_tangent: null operand");
  HIPCHK(launch_fcn_train_tangent((int)n, d, weights, xd, z, zd, a, sd, (hipStream_t)stream));
  return E3GNN_OK;
}

int e3gnn_fcn_train_dual(int64_t n, int n_hidden, const int32_t* widths, int act, float act_norm,
                         const float* weights, const float* sb, const float* sbd, const float* z,
                         const float* zd, float* zb, float* xb, void* stream) {
  FcnDims d;
  if (int rc = fcn_train_dims(n, n_hidden, widths, act, act_norm, d)) return rc;
  if (n > 0 && (!weights || !sb || !sbd || !z || !zd || !zb || !xb))
    return fail(E3GNN_ERR_ARG, "fcn_train_dual: null operand");
  HIPCHK(launch_fcn_train_dual((int)n, d, weights, sb, sbd, z, zd, zb, xb, (hipStream_t)stream));
  return E3GNN_OK;
}

}  // extern "C"
