// The loaded model of the specialised (SevenNet-0-shaped) engine: irreps, the
// node linears and their k_nodelin problem sets, the radial MLP's operand
// images.  Built by model_load.cpp (e3gnn_load), read by api.cpp.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "dbuf.h"
#include "generic.h"
#include "node.h"

namespace e3gnn {

// ------------------------------------------------------------ irreps helpers
struct Irr {
  int mul, l;
};
using Irreps = std::vector<Irr>;

Irreps parse_irreps(const std::string& s);
int irreps_dim(const Irreps& ir);
// merge consecutive equal-l entries (the layouts are identical, see tp.h)
Irreps merged(const Irreps& ir);

// e3nn o3.Linear on merged irreps: one block per l present in both.
struct LinBlock {
  int l, K, N, in_off, out_off, w_off, wt_off;
};
struct Linear {
  std::vector<LinBlock> blocks;
  DBuf W, WT;  // W: per block [K x N] row-major; WT: [N x K]
  std::vector<float> W_h, WT_h;  // host copies (pair construction at load)
  int din = 0, dout = 0;
};

// Node-linear problems for k_nodelin (gemm.hip): each block one output irrep
// block, from one linear (K2 = 0) or two K-concatenated linears writing the
// same block; `W` holds [K1 + K2 x N] per block (16-byte aligned).
struct PairBlock {
  int l, N, out_off, K1, off1, K2, off2, w_off;
  int64_t wb_off;  // byte offset of the block's bf16 pieces in LinPair::Wb
};
struct LinPair {
  std::vector<PairBlock> blocks;
  DBuf W;
  // W as three bf16 pieces (W = p0 + p1 + p2 exactly) in the 16x16x32 MFMA
  // B-operand order of k_nodelin_b (mlp_images.h pack_nodelin_b)
  DBuf Wb;
  bool ok = false;
};

}  // namespace e3gnn

// ------------------------------------------------------------ model
struct e3gnn_model {
  int device = 0;
  int nsp = 0, nlayer = 0;
  // channel family of the fused kernels (tp.h Family<f>): 0 SevenNet-0,
  // 1 uniform 64, 2 uniform 32
  int family = 0;
  // kernel kind code of block t (tp.h: 3 * family + first / middle / last)
  int kcode(int t) const { return 3 * family + (t == 0 ? 0 : (t == nlayer - 1 ? 2 : 1)); }
  std::vector<e3gnn::GateDims> gdims;  // gate layout per block (node.h)
  int max_dx = 0, max_dg = 0;
  float cutoff = 5.f, r_on = 4.5f;
  int raw_sh = 0;   // SH of the raw edge vector (sh_normalize false: checkpoints before sevenn 0.9)
  std::vector<e3gnn::Irreps> irreps;  // irreps_manual per layer boundary (merged)
  std::vector<e3gnn::Irreps> gin, mid;
  std::vector<int> W;          // radial weight numel per layer
  std::vector<float> denom;
  e3gnn::DBuf coeffs, embed, readout_v, scale, shift;
  std::vector<std::unique_ptr<e3gnn::Linear>> sc, si1, si2;
  // use_bias_in_linear: the full-width bias rows of si1 (dim(irreps[t])) and
  // si2 (dim(gin[t]): scalars and gates), nonzero on the 0e columns; null
  // without biases.  The embedding's bias sits in `embed`, the linear
  // readout's constant in `shift`.
  std::vector<e3gnn::DBuf> b_si1, b_si2;
  // readout_as_fcn: the FCN readout's dims and packed weights (node.h
  // FcnDims); readout_v is not built
  bool fcn = false;
  e3gnn::FcnDims fcnd{};
  e3gnn::DBuf fcn_w;
  // k_nodelin problem sets: si1, si1^T, si2^T, si2 + sc (forward, gate
  // epilogue), si1^T + sc^T (backward)
  std::vector<std::unique_ptr<e3gnn::LinPair>> nl_si1, nl_si1t, nl_si2t, nl_fwd, nl_bwd;
  struct Mlp {
    using DBuf = e3gnn::DBuf;
    DBuf w0, w1, w2, w0t, w1t, w2t;  // f32, plain and transposed (w1, w2 and the transposes: the v1 path)
    DBuf w2b;            // 3-way bf16 split of w2 in 16x16x32 operand order (fused.h)
    DBuf w2v;            // w2b's column blocks in visiting order (last block; fused.h)
    DBuf w2s;            // the lock-step backward's pair images (first / middle; w2_image.h)
    DBuf w1b;            // layer 1's operand, w2b order (fused.h)
  };
  std::vector<Mlp> mlp;
  // the manifest the fused-family model was loaded with and the extent of its
  // tensor table: e3gnn_set_weights lays a new flat array out by them
  std::string manifest_json;
  int64_t flat_numel = 0;
  // any other nequip-family deployment: the generic engine (generic.cpp)
  e3gnn::GenModel* gen = nullptr;
  ~e3gnn_model() {
    if (gen) e3gnn::gen_free(gen);
  }
};
