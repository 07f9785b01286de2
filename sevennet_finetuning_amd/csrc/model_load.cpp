// e3gnn_load: this build's deploy format (manifest + flat weights) into an
// e3gnn_model (model.h) -- the irreps, the readout, and per interaction block
// the node linears with their biases and k_nodelin problem sets and the radial
// MLP with its operand images (mlp_images.h, w2_image.h).  Every deployment
// outside the fused kernels' family goes to the generic engine (generic.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/e3gnn.h"
#include "api_util.h"
#include "bias_row.h"
#include "common.h"
#include "fcn_act.h"
#include "fused.h"
#include "generic.h"
#include "minijson.h"
#include "mlp_images.h"
#include "model.h"
#include "node.h"
#include "tp.h"

namespace e3gnn {

Irreps parse_irreps(const std::string& s) {
  Irreps out;
  std::stringstream ss(s);
  std::string term;
  while (std::getline(ss, term, '+')) {
    const auto x = term.find('x');
    out.push_back({std::stoi(term.substr(0, x)), std::stoi(term.substr(x + 1))});
  }
  return out;
}
int irreps_dim(const Irreps& ir) {
  int d = 0;
  for (auto& i : ir) d += i.mul * (2 * i.l + 1);
  return d;
}
Irreps merged(const Irreps& ir) {
  Irreps out;
  for (auto& i : ir) {
    if (!out.empty() && out.back().l == i.l) out.back().mul += i.mul;
    else out.push_back(i);
  }
  return out;
}

}  // namespace e3gnn

using namespace e3gnn;

namespace {

// ------------------------------------------------------------ model loading
int build_linear(Linear& L, const Irreps& in, const Irreps& out, const float* w, size_t numel,
                 double extra_scale_t) {
  std::vector<float> W, WT;
  int in_off = 0;
  size_t woff = 0;
  L.blocks.clear();   // (a refresh rebuilds the same table)
  L.din = irreps_dim(in);
  L.dout = irreps_dim(out);
  for (auto& a : in) {
    int out_off = 0;
    for (auto& b : out) {
      if (a.l == b.l) {
        LinBlock k{a.l, a.mul, b.mul, in_off, out_off, (int)W.size(), (int)WT.size()};
        // e3nn Linear 'element' path normalisation: 1/sqrt(fan_in), fan_in = mul_in
        const double sc = 1.0 / std::sqrt((double)a.mul);
        if (woff + (size_t)a.mul * b.mul > numel) return -1;
        for (int u = 0; u < a.mul; ++u)
          for (int v = 0; v < b.mul; ++v) W.push_back((float)(w[woff + (size_t)u * b.mul + v] * sc));
        for (int v = 0; v < b.mul; ++v)
          for (int u = 0; u < a.mul; ++u)
            WT.push_back((float)(w[woff + (size_t)u * b.mul + v] * sc * extra_scale_t));
        woff += (size_t)a.mul * b.mul;
        L.blocks.push_back(k);
      }
      out_off += b.mul * (2 * b.l + 1);
    }
    in_off += a.mul * (2 * a.l + 1);
  }
  if (woff != numel) return -1;
  if (upload(L.W, W) != hipSuccess || upload(L.WT, WT) != hipSuccess) return -2;
  L.W_h = std::move(W);
  L.WT_h = std::move(WT);
  return 0;
}

// One linear (forward: in -> out with W, or transposed: out -> in with WT) plus
// optionally a second one into the same output blocks (K-concatenated).
// ok = false when a block of the second has no partner in the first.
int build_pair(LinPair& P, const Linear& a, bool ta, const Linear* b, bool tb) {
  std::vector<float> W;
  size_t matched = 0;
  P.blocks.clear();   // (a refresh rebuilds the same table)
  P.ok = false;
  for (auto& k : a.blocks) {
    PairBlock pb;
    pb.l = k.l;
    pb.N = ta ? k.K : k.N;
    pb.out_off = ta ? k.in_off : k.out_off;
    pb.K1 = ta ? k.N : k.K;
    pb.off1 = ta ? k.out_off : k.in_off;
    pb.K2 = 0;
    pb.off2 = 0;
    pb.w_off = (int)W.size();
    const float* w1 = ta ? a.WT_h.data() + k.wt_off : a.W_h.data() + k.w_off;
    W.insert(W.end(), w1, w1 + (size_t)pb.K1 * pb.N);
    if (b) {
      for (auto& q : b->blocks) {
        const int n2 = tb ? q.K : q.N, o2 = tb ? q.in_off : q.out_off;
        if (q.l != k.l || o2 != pb.out_off) continue;
        if (n2 != pb.N || pb.K2) return 0;
        pb.K2 = tb ? q.N : q.K;
        pb.off2 = tb ? q.out_off : q.in_off;
        const float* w2 = tb ? b->WT_h.data() + q.wt_off : b->W_h.data() + q.w_off;
        W.insert(W.end(), w2, w2 + (size_t)pb.K2 * pb.N);
        ++matched;
      }
    }
    while (W.size() % 4) W.push_back(0.f);
    P.blocks.push_back(pb);
  }
  if (b && matched != b->blocks.size()) return 0;
  if (upload(P.W, W) != hipSuccess) return -2;
  // the bf16x6 operand image (k_nodelin_b)
  std::vector<float> Wb;   // bf16 pairs packed in floats
  for (auto& pb : P.blocks) {
    pb.wb_off = (int64_t)Wb.size() * 4;
    const size_t base = Wb.size();
    Wb.resize(base + mlpimg::nodelin_b_floats(pb.K1, pb.K2, pb.N), 0.f);
    mlpimg::pack_nodelin_b(W.data() + pb.w_off, pb.K1, pb.K2, pb.N, Wb.data() + base);
  }
  if (upload(P.Wb, Wb) != hipSuccess) return -2;
  P.ok = true;
  return 0;
}

// the path table of a fused kind code (tp.h)
std::vector<PathDef> kind_paths(int code) {
  std::vector<PathDef> P(16);
  P.resize(fused_kind_paths(code, P.data(), (int)P.size()));
  return P;
}

// Column start of every 16-channel weight block in the order the fused
// kernels visit them (input irrep I, channel block jj, then the paths of I in
// instruction order): pairs of consecutive blocks share one staged image of
// the lock-step backward (MlpW::w2s).
std::vector<int> bwd_w_block_cols(int code) {
  const auto P = kind_paths(code);
  std::vector<int> cols;
  for (int I = 0; I < 3; ++I) {
    int mul = 0;
    for (auto& p : P)
      if (p.l1 == I) mul = p.mul;
    for (int jj = 0; jj < mul / 16; ++jj)
      for (auto& p : P)
        if (p.l1 == I) cols.push_back(p.woff + 16 * jj);
  }
  return cols;
}

// IrrepsConvolution instruction list (convolution.py:72-95) vs the kernel
// tables of kind code `code`
bool check_paths(int code, const Irreps& x, int lmax_out) {
  struct Ins {
    int l1, l2, l3, mul, xoff;
  };
  const auto P = kind_paths(code);
  int DX = 0, W = 0, DM = 0;
  if (P.empty() || !fused_kind_dims(code, &DX, &W, &DM)) return false;
  std::vector<Ins> ins;
  int xoff = 0;
  for (auto& i : x) {
    for (int l2 = 0; l2 <= 2; ++l2)
      for (int l3 = std::abs(i.l - l2); l3 <= i.l + l2; ++l3)
        if (l3 <= lmax_out) ins.push_back({i.l, l2, l3, i.mul, xoff});
    xoff += i.mul * (2 * i.l + 1);
  }
  if (ins.size() != P.size()) return false;
  // mid slots: stable sort by l3
  std::vector<int> moff(ins.size());
  int off = 0;
  for (int l3 = 0; l3 <= 2; ++l3)
    for (size_t k = 0; k < ins.size(); ++k)
      if (ins[k].l3 == l3) {
        moff[k] = off;
        off += ins[k].mul * (2 * l3 + 1);
      }
  if (off != DM) return false;
  int woff = 0;
  for (size_t k = 0; k < ins.size(); ++k) {
    const PathDef& p = P[k];
    if (p.l1 != ins[k].l1 || p.l2 != ins[k].l2 || p.l3 != ins[k].l3 || p.mul != ins[k].mul ||
        p.xoff != ins[k].xoff || p.woff != woff || p.moff != moff[k])
      return false;
    woff += ins[k].mul;
  }
  return woff == W && xoff == DX;
}

// The SevenNet-0-shaped family test: what the specialised engine serves.
// The knobs of nn.sevennet0_kinds (even parity, lmax 2, linear
// self-connection, XPLOR cutoff), what the fused kernels hard-code (8 Bessel
// functions, a 64-64 radial MLP), at least 2 blocks, and the irreps of one
// compiled channel family (tp.h): A x0e -> (L - 1) x C0x0e+C1x1e+C2x2e -> D x0e.
// Returns the family, or -1 (the generic engine serves the deployment).
int fused_family(const minijson::Value& man) {
  // E3GNN_GENERIC=1: every deployment on the generic engine (cross-checks)
  if (const char* g = std::getenv("E3GNN_GENERIC"); g && g[0] == '1') return -1;
  if (man.has("is_parity") && man["is_parity"].boolean()) return -1;
  const int lmax = man.has("lmax_edge") ? (int)man["lmax_edge"].num()
                                        : (man.has("lmax") ? (int)man["lmax"].num() : 2);
  if (lmax != 2) return -1;
  if (man.has("self_connection_type") && man["self_connection_type"].str() != "linear") return -1;
  if (!man.has("cutoff_function") || man["cutoff_function"]["name"].str() != "XPLOR") return -1;
  // linear biases (model_build.py:194-240) ride in the node-linear epilogues
  // and the FCN readout (:396-408) has its own kernel (node.hip
  // k_readout_fcn), within its limits: 1 .. FCN_MAX_HIDDEN hidden layers of
  // 1 .. FCN_MAX_WIDTH units and one of fcn_act.h's activations.  Beyond them
  // the generic engine serves the model.
  if (man.has("readout") && man["readout"].has("type") && man["readout"]["type"].str() != "linear") {
    const auto& ro = man["readout"];
    if (ro["type"].str() != "fcn" || !ro.has("hidden") || !ro.has("act") || !ro.has("act_norm")) return -1;
    const auto& h = ro["hidden"].arr();
    if (h.size() < 1 || h.size() > (size_t)FCN_MAX_HIDDEN) return -1;
    for (auto& w : h)
      if (w.num() < 1 || w.num() > FCN_MAX_WIDTH || w.num() != std::floor(w.num())) return -1;
    bool known = false;
    for (int k = 0; k < FCN_ACT_KINDS; ++k) known = known || ro["act"].str() == fcn_act_names()[k];
    if (!known) return -1;
  }
  const int L = (int)man["num_convolution_layer"].num();
  if (L < 2) return -1;
  if (man.has("weight_nn_hidden_neurons")) {
    const auto& h = man["weight_nn_hidden_neurons"].arr();
    if (h.size() != 2 || (int)h[0].num() != 64 || (int)h[1].num() != 64) return -1;
  }
  if (man.has("radial_basis") && man["radial_basis"].has("num") && (int)man["radial_basis"]["num"].num() != 8)
    return -1;
  const auto& ir = man["irreps_manual"].arr();
  if ((int)ir.size() != L + 1) return -1;
  Irreps first, mid, last;
  try {
    first = merged(parse_irreps(ir[0].str()));
    mid = merged(parse_irreps(ir[1].str()));
    last = merged(parse_irreps(ir[L].str()));
  } catch (...) {
    return -1;
  }
  if (first.size() != 1 || first[0].l != 0 || last.size() != 1 || last[0].l != 0) return -1;
  for (int t = 1; t < L; ++t)
    if (ir[t].str() != ir[1].str()) return -1;
  if (L > 1 && (mid.size() != 3 || mid[0].l != 0 || mid[1].l != 1 || mid[2].l != 2)) return -1;
  for (int f = 0; f < N_FAMILIES; ++f) {
    PathDef P0[16], P1[16];
    fused_kind_paths(3 * f, P0, 16);
    fused_kind_paths(3 * f + 1, P1, 16);
    // first block's input A; middle irreps C0 / C1 / C2 (paths 0, 3, 9 of the middle table)
    if (first[0].mul == P0[0].mul && mid[0].mul == P1[0].mul && mid[1].mul == P1[3].mul &&
        mid[2].mul == P1[9].mul)
      return f;
  }
  return -1;
}

// ------------------------------------------------------------ the steps of e3gnn_load
// The deployment as read from disk or taken from memory: the manifest (and
// its text), the flat weights and the manifest's tensor index, with checked
// access by name.  The steps come in two kinds: those that read the manifest
// alone (load_header, load_block_irreps: run once, they size the model) and
// those that read the weights (load_weights and below: each writes slot t of
// the model's tables and uploads into the buffers already there, so
// e3gnn_set_weights re-runs them over a new flat array and every device
// buffer keeps its address and size).
struct Deploy {
  std::string text;
  minijson::Value man;
  std::vector<float> flat;
  std::map<std::string, std::pair<size_t, size_t>> T;   // name -> (offset, numel)
  size_t total = 0;                                      // the tensor table's extent
  bool has_bias = false;                                 // use_bias_in_linear

  const float* get(const std::string& n, size_t expect = 0) const {
    auto it = T.find(n);
    if (it == T.end()) throw std::runtime_error("missing tensor " + n);
    if (it->second.first + it->second.second > flat.size())
      throw std::runtime_error("tensor out of file range " + n);
    if (expect && it->second.second != expect) throw std::runtime_error("bad size " + n);
    return flat.data() + it->second.first;
  }
  size_t numel(const std::string& n) const { return T.at(n).second; }
  // use_bias_in_linear: a bias tensor's full-width row over `out` (bias_row.h)
  std::vector<float> bias(const std::string& n, const Irreps& out) const {
    const float* b = get(n);   // (present and inside the file)
    return bias_row(out, [](const Irr& i) { return i.l == 0; }, b, numel(n), n);
  }
};

void must_upload(DBuf& d, const std::vector<float>& v, const char* what = "upload") {
  if (upload(d, v) != hipSuccess) throw std::runtime_error(what);
}

// manifest and weights from disk; nonzero (the error is set) when a file is
// missing or the manifest does not parse
int read_deploy(Deploy& D, const char* weights_path, const char* manifest_path) {
  {
    std::ifstream f(manifest_path);
    if (!f) return fail(E3GNN_ERR_IO, std::string("cannot open manifest ") + manifest_path);
    std::stringstream ss;
    ss << f.rdbuf();
    D.text = ss.str();
    std::string err;
    if (!minijson::parse(D.text, D.man, err)) return fail(E3GNN_ERR_IO, "manifest parse error: " + err);
  }
  std::ifstream f(weights_path, std::ios::binary | std::ios::ate);
  if (!f) return fail(E3GNN_ERR_IO, std::string("cannot open weights ") + weights_path);
  const std::streamsize sz = f.tellg();
  f.seekg(0);
  D.flat.resize(sz / 4);
  f.read((char*)D.flat.data(), (std::streamsize)D.flat.size() * 4);
  return E3GNN_OK;
}

// the tensor index of D's manifest
void index_tensors(Deploy& D) {
  for (auto& t : D.man["tensors"].arr()) {
    const size_t off = (size_t)t["offset"].num(), n = (size_t)t["numel"].num();
    D.T[t["name"].str()] = {off, n};
    D.total = std::max(D.total, off + n);
  }
  D.has_bias = D.man.has("use_bias_in_linear") && D.man["use_bias_in_linear"].boolean();
}

// the manifest's scalars and irreps; the per-block tables sized for their slots
void load_header(e3gnn_model* m, const Deploy& D, int family) {
  const minijson::Value& man = D.man;
  // the knobs this engine does not read must hold SevenNet-0's values (the
  // same predicate as nn.sevennet0_kinds)
  // sh_normalize false (checkpoints before sevenn 0.9, util.py:130-146): the
  // same kernels, the SH polynomials of the raw vector (node.hip)
  m->raw_sh = man.has("sh_normalize") && !man["sh_normalize"].boolean() ? 1 : 0;
  m->family = family;
  if (man.has("is_parity") && man["is_parity"].boolean())
    throw std::runtime_error("odd-parity filters are not SevenNet-0's architecture");
  if (man.has("self_connection_type") && man["self_connection_type"].str() != "linear")
    throw std::runtime_error("self_connection_type " + man["self_connection_type"].str() +
                             " is not SevenNet-0's (linear)");
  if (man.has("lmax_edge") && (int)man["lmax_edge"].num() != 2)
    throw std::runtime_error("lmax_edge must be 2 (SevenNet-0)");
  m->nsp = (int)man["num_species"].num();
  m->cutoff = (float)man["cutoff"].num();
  m->r_on = (float)man["cutoff_function"]["cutoff_on"].num();
  if (man["cutoff_function"]["name"].str() != "XPLOR")
    throw std::runtime_error("only the XPLOR cutoff of SevenNet-0 is implemented");
  m->nlayer = (int)man["num_convolution_layer"].num();
  if (std::abs(man["silu_norm"].num() - (double)SILU_NORM) > 1e-6)
    throw std::runtime_error("silu_norm mismatch");
  for (auto& s : man["irreps_manual"].arr()) m->irreps.push_back(merged(parse_irreps(s.str())));
  if ((int)m->irreps.size() != m->nlayer + 1) throw std::runtime_error("irreps_manual length");
  const size_t L = (size_t)m->nlayer;
  m->denom.assign(L, 0.f);
  m->W.assign(L, 0);
  m->mlp.resize(L);
  m->b_si1.resize(L);
  m->b_si2.resize(L);
  for (auto* v : {&m->sc, &m->si1, &m->si2}) v->resize(L);
  for (auto* v : {&m->nl_si1, &m->nl_si1t, &m->nl_si2t, &m->nl_fwd, &m->nl_bwd}) v->resize(L);
}

// radial basis coefficients and the species embedding
void load_embedding(e3gnn_model* m, const Deploy& D) {
  const float* cf = D.get("edge_embedding.basis_function.coeffs", 8);
  must_upload(m->coeffs, std::vector<float>(cf, cf + 8));
  const int d0 = irreps_dim(m->irreps[0]);
  const float* we = D.get("onehot_to_feature_x.linear.weight", (size_t)m->nsp * d0);
  std::vector<float> emb((size_t)m->nsp * d0);
  for (size_t i = 0; i < emb.size(); ++i) emb[i] = (float)(we[i] / std::sqrt((double)m->nsp));
  if (D.has_bias) {
    // the embedding's bias: the same for every species row (k_embed copies rows)
    const auto row = D.bias("onehot_to_feature_x.linear.bias", m->irreps[0]);
    for (int sp = 0; sp < m->nsp; ++sp)
      for (int c = 0; c < d0; ++c) emb[(size_t)sp * d0 + c] += row[c];
  }
  must_upload(m->embed, emb);
}

// FCN_e3nn (nn/linear.py:94-129): e3nn FullyConnectedNet([dl] + hidden +
// [1], act), every layer's weight / sqrt(fan_in); packed in the order
// of node.h FcnDims (the hidden matrices with their odd row strides,
// then the output vector).  (fused_family checked the limits.)
void load_readout_fcn(e3gnn_model* m, const Deploy& D, int dl) {
  const auto& ro = D.man["readout"];
  FcnDims& fd = m->fcnd;
  fd.nh = (int)ro["hidden"].arr().size();
  fd.w[0] = dl;
  for (int k = 0; k < fd.nh; ++k) fd.w[k + 1] = (int)ro["hidden"].arr()[k].num();
  fd.kind = -1;
  for (int k = 0; k < FCN_ACT_KINDS; ++k)
    if (ro["act"].str() == fcn_act_names()[k]) fd.kind = k;
  fd.c = (float)ro["act_norm"].num();
  if (fd.kind < 0 || dl > FCN_MAX_WIDTH) throw std::runtime_error("readout FCN outside the kernel's limits");
  std::vector<float> pk(fd.padded_floats(), 0.f);
  for (int k = 0; k <= fd.nh; ++k) {
    const int a = fd.w[k], b = k < fd.nh ? fd.w[k + 1] : 1;
    const float* w = D.get("readout_FCN.fcn.layer" + std::to_string(k) + ".weight", (size_t)a * b);
    const double sn = 1.0 / std::sqrt((double)a);
    float* M = pk.data() + fd.mat_off(k);
    const int ld = k < fd.nh ? fd.stride(k) : 1;
    for (int i = 0; i < a; ++i)
      for (int j = 0; j < b; ++j) M[(size_t)i * ld + j] = (float)(w[(size_t)i * b + j] * sn);
  }
  must_upload(m->fcn_w, pk);
}

// two linears without activation (D x0e -> H x0e -> 1x0e) folded into one
// vector, e3nn path weights 1 / sqrt(fan_in) each; their biases fold into `shift`
void load_readout_linear(e3gnn_model* m, const Deploy& D, int dl, const float* sc, std::vector<float>& shift) {
  const int hid = (int)D.numel("reduce_hidden_to_energy.linear.weight");
  const float* wh = D.get("reduce_input_to_hidden.linear.weight", (size_t)dl * hid);
  const float* wo = D.get("reduce_hidden_to_energy.linear.weight", hid);
  std::vector<float> v(dl);
  for (int c = 0; c < dl; ++c) {
    double s = 0;
    for (int k = 0; k < hid; ++k) s += (double)wh[c * hid + k] * wo[k];
    v[c] = (float)(s / (std::sqrt((double)dl) * std::sqrt((double)hid)));
  }
  must_upload(m->readout_v, v);
  if (D.has_bias) {
    // e = (x A + bA) B + bB = x . v + c, c = bA . B / sqrt(hid) + bB, per
    // atom before the rescale: shift[t] += scale[t] c (k_readout unchanged)
    const Irreps hir{{hid, 0}}, one{{1, 0}};
    const auto bh = D.bias("reduce_input_to_hidden.linear.bias", hir);
    const auto bo = D.bias("reduce_hidden_to_energy.linear.bias", one);
    double cst = bo[0];
    for (int k = 0; k < hid; ++k) cst += (double)bh[k] * wo[k] / std::sqrt((double)hid);
    for (int t = 0; t < m->nsp; ++t) shift[t] = (float)(shift[t] + cst * sc[t]);
  }
}

// the readout (linear or FCN) and the species-wise rescale
void load_readout(e3gnn_model* m, const Deploy& D) {
  const minijson::Value& man = D.man;
  const int dl = irreps_dim(m->irreps[m->nlayer]);
  const float* sc = D.get("rescale_atomic_energy.scale", m->nsp);
  const float* sh = D.get("rescale_atomic_energy.shift", m->nsp);
  std::vector<float> shift(sh, sh + m->nsp);
  m->fcn = man.has("readout") && man["readout"].has("type") && man["readout"]["type"].str() == "fcn";
  if (m->fcn) load_readout_fcn(m, D, dl);
  else load_readout_linear(m, D, dl, sc, shift);
  trace_point("load:readout");
  must_upload(m->scale, std::vector<float>(sc, sc + m->nsp));
  must_upload(m->shift, shift);
}

// block t's irreps: the gate's input row, the gate layout and the
// convolution's mid irreps; the kernel tables of its kind code must match
void load_block_irreps(e3gnn_model* m, int t) {
  const Irreps& xin = m->irreps[t];
  const Irreps& xout = m->irreps[t + 1];
  const bool last = t == m->nlayer - 1;
  // gate irreps_in: scalars + gates (0e) + gated (equivariant_gate.py:48-55)
  Irreps gin;
  int nscal = 0, ngated = 0;
  for (auto& i : xout) (i.l == 0 ? nscal : ngated) += i.mul;
  gin.push_back({nscal + ngated, 0});
  for (auto& i : xout)
    if (i.l > 0) gin.push_back(i);
  const int lmax_out = last ? 0 : 2;
  if (!check_paths(m->kcode(t), xin, lmax_out))
    throw std::runtime_error("convolution path table mismatch at layer " + std::to_string(t));
  {
    // gate layout (node.h GateDims): scalars, then the gated 1e / 2e blocks
    GateDims gd{0, 0, 0};
    for (auto& i : xout) (i.l == 0 ? gd.ns : (i.l == 1 ? gd.g1 : gd.g2)) += i.mul;
    if (last ? (gd.g1 || gd.g2) : false)
      throw std::runtime_error("the last block's output must be scalars");
    for (size_t k = 1; k < xout.size(); ++k)
      if (xout[k].l < xout[k - 1].l) throw std::runtime_error("output irreps must be sorted by l");
    m->gdims.push_back(gd);
    m->max_dx = std::max(m->max_dx, irreps_dim(xin));
    m->max_dg = std::max(m->max_dg, gd.dy());
  }
  // mid irreps merged by l (sorted), see tp.h
  Irreps mid;
  for (int l3 = 0; l3 <= lmax_out; ++l3) {
    int mul = 0;
    for (auto& i : xin)
      for (int l2 = 0; l2 <= 2; ++l2)
        if (std::abs(i.l - l2) <= l3 && l3 <= i.l + l2) mul += i.mul;
    if (mul) mid.push_back({mul, l3});
  }
  m->gin.push_back(gin);
  m->mid.push_back(mid);
}

// block t's denominator, node linears, their biases and the k_nodelin problem sets
void load_block_linears(e3gnn_model* m, const Deploy& D, int t) {
  const Irreps &xin = m->irreps[t], &gin = m->gin[t], &mid = m->mid[t];
  const std::string p = std::to_string(t);
  const float den = m->denom[t] = *D.get(p + "_convolution.denominator", 1);
  auto mk = [&](std::unique_ptr<Linear>& L, const std::string& name, const Irreps& a, const Irreps& b,
                double extra) {
    if (!L) L = std::make_unique<Linear>();
    if (build_linear(*L, a, b, D.get(name), D.numel(name), extra) != 0)
      throw std::runtime_error("linear " + name);
  };
  trace_point("load:layer-begin");
  mk(m->sc[t], p + "_self_connection_intro.linear.weight", xin, gin, 1.0);
  trace_point("load:sc");
  mk(m->si1[t], p + "_self_interaction_1.linear.weight", xin, xin, 1.0);
  // backward of si2 feeds dE/dagg_raw = dE/dagg / denominator (convolution.py:117-118)
  mk(m->si2[t], p + "_self_interaction_2.linear.weight", mid, gin, 1.0 / den);
  // their biases (the self-connection has none, model_build.py:281-282):
  // si2's covers the scalars and the gate pre-activations, and is not
  // divided by the denominator (only si2's weights carry it)
  if (D.has_bias) {
    must_upload(m->b_si1[t], D.bias(p + "_self_interaction_1.linear.bias", xin));
    must_upload(m->b_si2[t], D.bias(p + "_self_interaction_2.linear.bias", gin));
  }
  auto pair = [&](std::unique_ptr<LinPair>& P, const Linear& a, bool ta, const Linear* b, bool tb) {
    if (!P) P = std::make_unique<LinPair>();
    if (build_pair(*P, a, ta, b, tb) < 0) throw std::runtime_error("upload");
  };
  pair(m->nl_si1[t], *m->si1[t], false, nullptr, false);
  pair(m->nl_si1t[t], *m->si1[t], true, nullptr, false);
  pair(m->nl_si2t[t], *m->si2[t], true, nullptr, false);
  pair(m->nl_fwd[t], *m->si2[t], false, m->sc[t].get(), false);
  pair(m->nl_bwd[t], *m->si1[t], true, m->sc[t].get(), true);
}

// a[r][c] * s, optionally transposed
std::vector<float> scaled(const float* a, int r, int c, double s, bool tr) {
  std::vector<float> o((size_t)r * c);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) {
      const float v = (float)(a[(size_t)i * c + j] * s);
      if (tr) o[(size_t)j * r + i] = v;
      else o[(size_t)i * c + j] = v;
    }
  return o;
}

// block t's radial MLP (e3nn FullyConnectedNet, weights / sqrt(fan_in)): the
// f32 matrices and the operand images of the fused kernels (fused.h MlpW)
void load_block_mlp(e3gnn_model* m, const Deploy& D, int t) {
  const std::string p = std::to_string(t);
  const float* w0 = D.get(p + "_convolution.weight_nn.layer0.weight", 8 * 64);
  const float* w1 = D.get(p + "_convolution.weight_nn.layer1.weight", 64 * 64);
  const size_t n2 = D.numel(p + "_convolution.weight_nn.layer2.weight");
  const float* w2 = D.get(p + "_convolution.weight_nn.layer2.weight");
  const int W = (int)(n2 / 64);
  int kdx = 0, Wexp = 0, kdm = 0;
  fused_kind_dims(m->kcode(t), &kdx, &Wexp, &kdm);
  if (W != Wexp || W % 16) throw std::runtime_error("radial weight width mismatch");
  m->W[t] = W;
  auto& mm = m->mlp[t];
  const double s0 = 1.0 / std::sqrt(8.0), s1 = 1.0 / 8.0, s2 = 1.0 / 8.0;
  const auto a0 = scaled(w0, 8, 64, s0, false), a1 = scaled(w1, 64, 64, s1, false),
             a2 = scaled(w2, 64, W, s2, false);
  const auto a1t = scaled(w1, 64, 64, s1, true);
  must_upload(mm.w0, a0, "upload mlp");
  must_upload(mm.w1, a1, "upload mlp");
  must_upload(mm.w2, a2, "upload mlp");
  must_upload(mm.w0t, scaled(w0, 8, 64, s0, true), "upload mlp");
  must_upload(mm.w1t, a1t, "upload mlp");
  must_upload(mm.w2t, scaled(w2, 64, W, s2, true), "upload mlp");
  // layer 1 in w2b's order: W1 (64 x 64, in x out), the operand of the value
  // and of the backward's tangent alike
  must_upload(mm.w1b, mlpimg::pack_w2b(a1, 64), "upload mlp (w1b)");
  // the kernels' visiting order of the 16-column blocks (input irrep,
  // channel block, path): pairs of consecutive blocks
  const std::vector<int> cols = bwd_w_block_cols(m->kcode(t));
  if ((int)cols.size() * 16 != W || cols.size() % 2)
    throw std::runtime_error("dE/dw block order does not cover the weights");
  const std::vector<float> b2 = mlpimg::pack_w2b(a2, W);
  // the last block's backward (k_conv_bwd_nbr) reads its operand from L2
  // in the lane order w2v; the first and middle blocks' (k_conv_bwd_ls)
  // stage one image per pair (w2s)
  if (m->kcode(t) % 3 == 2) {
    must_upload(mm.w2v, mlpimg::pack_w2v(b2, cols), "upload mlp (w2v)");
  } else {
    // w2s (MlpW::w2s): per pair P and piece, the [hidden unit][channel]
    // matrix of the pair's 2 x 16 columns cols[2P], cols[2P + 1] in the
    // swizzled order of w2_image.h, the same residual chain of bf16
    // pieces: read transposed (ds_read_b64_tr_b16) it gives w2v's lane
    // registers
    const size_t npairs = cols.size() / 2;
    std::vector<float> s2(npairs * w2img::PAIR_BYTES / 4);
    w2img::pack(a2.data(), W, cols.data(), (int)npairs, reinterpret_cast<uint16_t*>(s2.data()));
    must_upload(mm.w2s, s2, "upload mlp (w2s)");
  }
  must_upload(mm.w2b, b2, "upload mlp (packed)");
  trace_point("load:mlp");
}

// every weight-dependent step, over the tables load_header / load_block_irreps sized
void load_weights(e3gnn_model* m, const Deploy& D) {
  load_embedding(m, D);
  load_readout(m, D);
  for (int t = 0; t < m->nlayer; ++t) {
    load_block_linears(m, D, t);
    load_block_mlp(m, D, t);
  }
}

// e3gnn_load / e3gnn_load_memory: `read` fills D's manifest and weights
// (nonzero with the error set when it cannot)
template <class Read>
e3gnn_model* load_model(int device, Read read) {
  auto m = std::make_unique<e3gnn_model>();
  m->device = device;
  trace_point("load:entry");
  if (hipSetDevice(device) != hipSuccess) {
    fail(E3GNN_ERR_HIP, "hipSetDevice failed");
    return nullptr;
  }
  trace_point("load:hipSetDevice");
  Deploy D;
  if (read(D)) return nullptr;
  try {
    if (D.man["model_type"].str() != "E3_equivariant_model")
      throw std::runtime_error("unsupported model_type");
    // SevenNet-0's architecture runs on the specialised kernels; every other
    // member of the family on the generic engine (generic.cpp)
    const int family = fused_family(D.man);
    if (family < 0) {
      m->gen = gen_load(D.man, D.flat);
      m->nsp = gen_num_species(m->gen);
      m->nlayer = gen_num_layers(m->gen);
      m->cutoff = gen_cutoff(m->gen);
      trace_point("load:generic");
      (void)hipGetLastError();
      return m.release();
    }
    index_tensors(D);
    load_header(m.get(), D, family);
    for (int t = 0; t < m->nlayer; ++t) load_block_irreps(m.get(), t);
    load_weights(m.get(), D);
    m->manifest_json = std::move(D.text);
    m->flat_numel = (int64_t)D.total;
  } catch (const std::exception& ex) {
    fail(E3GNN_ERR_IO, std::string("model load: ") + ex.what());
    return nullptr;
  }
  trace_point("load:exit");
  // every HIP call above was checked; do not leave the host application's
  // thread-local HIP error state dirty (torch re-reads it after its own calls)
  (void)hipGetLastError();
  return m.release();
}

}  // namespace

extern "C" {

e3gnn_model* e3gnn_load(const char* weights_path, const char* manifest_path, int device) {
  return load_model(device, [&](Deploy& D) { return read_deploy(D, weights_path, manifest_path); });
}

e3gnn_model* e3gnn_load_memory(const char* manifest_json, const float* weights, int64_t numel, int device) {
  if (!manifest_json || !weights || numel < 0) {
    fail(E3GNN_ERR_ARG, "e3gnn_load_memory: null manifest or weights, or a negative numel");
    return nullptr;
  }
  return load_model(device, [&](Deploy& D) {
    D.text = manifest_json;
    std::string err;
    if (!minijson::parse(D.text, D.man, err)) return fail(E3GNN_ERR_IO, "manifest parse error: " + err);
    D.flat.assign(weights, weights + numel);
    return (int)E3GNN_OK;
  });
}

int e3gnn_set_weights(e3gnn_model* m, const float* weights, int64_t numel, void* stream) {
  if (!m) return fail(E3GNN_ERR_ARG, "e3gnn_set_weights: null model");
  if (!weights) return fail(E3GNN_ERR_ARG, "e3gnn_set_weights: null weights");
  if (m->gen)
    return fail(E3GNN_ERR_ARG, "e3gnn_set_weights: a generic-engine model has no in-place refresh "
                               "(load it again with e3gnn_load_memory)");
  if (numel != m->flat_numel)
    return fail(E3GNN_ERR_ARG, "e3gnn_set_weights: numel " + std::to_string(numel) + ", the manifest's tensors hold " +
                                   std::to_string(m->flat_numel));
  HIPCHK(hipSetDevice(m->device));
  // Stream-ordered evaluations may still read the buffers about to be
  // overwritten, and `weights` may be written by work queued on `stream`: drain
  // the device (the hazard DBuf::ensure documents), then take the weights
  HIPCHK(hipDeviceSynchronize());
  Deploy D;
  D.flat.resize((size_t)numel);
  {
    hipPointerAttribute_t at{};
    const bool dev = hipPointerGetAttributes(&at, weights) == hipSuccess &&
                     (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged);
    (void)hipGetLastError();   // (a plain host pointer is "invalid value" to some runtimes)
    if (dev) {
      HIPCHK(hipMemcpyAsync(D.flat.data(), weights, (size_t)numel * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
      HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    } else {
      std::copy(weights, weights + numel, D.flat.begin());
    }
  }
  try {
    std::string err;
    if (!minijson::parse(m->manifest_json, D.man, err)) throw std::runtime_error("manifest: " + err);
    index_tensors(D);
    // the manifest passed every shape check at load and the packers read
    // nothing else: only a HIP failure can stop the steps below
    load_weights(m, D);
  } catch (const std::exception& ex) {
    return fail(E3GNN_ERR_HIP, std::string("e3gnn_set_weights: ") + ex.what());
  }
  (void)hipGetLastError();
  return E3GNN_OK;
}

void e3gnn_free(e3gnn_model* m) { delete m; }

int e3gnn_model_info(const e3gnn_model* m, int* num_species, float* cutoff, int* num_layers,
                     int* comm_size) {
  if (!m) return fail(E3GNN_ERR_ARG, "null model");
  if (num_species) *num_species = m->nsp;
  if (cutoff) *cutoff = m->cutoff;
  if (num_layers) *num_layers = m->nlayer;
  if (comm_size) {
    if (m->gen) {  // the widest exchanged row (x[t] / dE/dx[t], t >= 1)
      int d = 0;
      for (int t = 1; t <= m->nlayer; ++t) d = std::max(d, gen_feature_dim(m->gen, t));
      *comm_size = d;
    } else {
      *comm_size = irreps_dim(m->irreps[1]);
    }
  }
  return E3GNN_OK;
}

int e3gnn_model_family(const e3gnn_model* m) {
  if (!m) return fail(E3GNN_ERR_ARG, "null model"), -1;
  return m->gen ? -1 : m->family;
}

}  // extern "C"
