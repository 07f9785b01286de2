// Launchers of node.hip (edge geometry, graph indices, node ops, reductions).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {
// embd (nullable): d emb / dr [E, 8], the tangent input of the fused backward
hipError_t launch_edge_embed(int64_t E, const float* vec, const float* coeffs, float rc, float ron,
                             int raw_sh, float* Y, float* emb, float* embd, hipStream_t s);
// the fine-tune step's edge-geometry tangent / coefficient gradient (node.hip)
hipError_t launch_edge_geom_jvp(int64_t E, const float* vec, const float* coeffs, float rc, float ron,
                                int raw_sh, const int* center, const int* nbr, const int64_t* batch,
                                const float* cF, const float* cS, const float* vol, float* Yd,
                                float* embd, float* rd, hipStream_t s);
hipError_t launch_edge_geom_coeff(int64_t E, const float* vec, const float* coeffs, float rc,
                                  float ron, const float* embb, const float* embdb, const float* rd,
                                  float* out, hipStream_t s);
int edge_force_blocks(int64_t E);
// the radial part of dE/dr from demb ([E, 8] dE/demb, through d emb / dr) and
// drad ([E] dE/dr itself, the fused kernels'), either nullable; vir_part nullable
hipError_t launch_edge_force(int64_t E, const float* vec, const float* coeffs, float rc, float ron,
                             int raw_sh, const float* dY, const float* dgu, const float* demb,
                             const float* drad, float* fe, float* vir_part, hipStream_t s);
hipError_t launch_atom_force(int n_nodes, int n_centers, const int* row_ptr, const int* src_ptr,
                             const int* src_perm, const float* fe, float* F, hipStream_t s);
hipError_t launch_build_graph(int64_t E, int n_centers, int n_nodes, const int* center,
                              const int* nbr, int* row_ptr, int* src_ptr, int* src_perm, int* cnt,
                              int* err, hipStream_t s, int n_interior = 0);
// the whole build in one workgroup (n <= graph_small_max_nodes(), E <=
// graph_small_max_edges()); int64
// indices (c64 / j64, converted into cout / jout) or int32 ones (c32 / j32);
// writes *err (no memset needed)
hipError_t launch_build_graph_small(int64_t E, int n, const int* c32, const int* j32, const int64_t* c64,
                                    const int64_t* j64, int* cout, int* jout, int* row_ptr, int* src_ptr,
                                    int* src_perm, int* err, hipStream_t s);
int graph_small_max_nodes();
int graph_small_max_edges();
hipError_t launch_embed(int n, int D, const int* type, int nsp, const float* W, float* x, int* err,
                        hipStream_t s);
// e3nn Gate of the SevenNet-0-shaped family: y = [ns scalars | g1 + g2 gates |
// g1 x 1e | g2 x 2e] -> x = [ns x 0e | g1 x 1e | g2 x 2e]; the last block
// (scalars only) uses ns alone
struct GateDims {
  int ns, g1, g2;
  __host__ __device__ int dx() const { return ns + 3 * g1 + 5 * g2; }
  __host__ __device__ int dy() const { return ns + 4 * g1 + 6 * g2; }
};
hipError_t launch_gate_fwd(int n, bool last, GateDims d, const float* y, float* x, hipStream_t s);
hipError_t launch_gate_bwd(int n, bool last, GateDims d, const float* y, const float* dx, float* dy,
                           hipStream_t s);
hipError_t launch_readout(int n, int D, const float* x, const float* v, const int* type,
                          const float* scale, const float* shift, float* eat, hipStream_t s);
hipError_t launch_readout_bwd(int n, int D, const float* v, const int* type, const float* scale,
                              float* dx, hipStream_t s);
// y[n, d] += b[d] on every row: the linear biases (use_bias_in_linear) after
// the k_gemm fallback of the node linears (api.cpp e3gnn_layer_forward_part); no launch for n == 0
hipError_t launch_row_bias(int64_t n, int d, const float* b, float* y, hipStream_t s);
// The FCN readout (readout_as_fcn, FCN_e3nn nn/linear.py:94-129) of the fused
// engine: a_0 = x, a_k = c f(a_{k-1} M_{k-1}) for the nh hidden layers, s =
// a_nh . v, e = s * scale[t] + shift[t]; one launch writes eat[i] = e and
// dx[i, :] = scale[t] ds/dx (what k_readout_bwd writes for the linear readout).
// The packed weights (every matrix pre-scaled by 1 / sqrt(fan_in)): for k < nh
// M_k [w[k]][stride(k)] row-major with an odd row stride >= w[k + 1] (padding
// zero), then v [w[nh]]; padded to padded_floats().
constexpr int FCN_MAX_HIDDEN = 4, FCN_MAX_WIDTH = 128;
struct FcnDims {
  int nh;                     // hidden layers: 1 .. FCN_MAX_HIDDEN
  int w[FCN_MAX_HIDDEN + 1];  // w[0] = D (the row of x), w[1 .. nh] the hidden widths (1 .. FCN_MAX_WIDTH)
  int kind;                   // activation f (fcn_act.h)
  float c;                    // its normalize2mom constant (manifest readout.act_norm)
  __host__ __device__ int stride(int k) const { return w[k + 1] | 1; }
  __host__ __device__ int mat_off(int k) const {   // M_k (k < nh), v (k == nh)
    int o = 0;
    for (int q = 0; q < k; ++q) o += w[q] * stride(q);
    return o;
  }
  __host__ __device__ int padded_floats() const { return (mat_off(nh) + w[nh] + 3) & ~3; }
};
hipError_t launch_readout_fcn(int n, const FcnDims& d, const float* x, const float* W, const int* type,
                              const float* scale, const float* shift, float* eat, float* dx, hipStream_t s);
int sum_blocks(int64_t n);
hipError_t launch_sum(int64_t n, const float* a, float* part, float* out, hipStream_t s);
hipError_t launch_final_sum(int nb, int k, const float* part, float* out, hipStream_t s);
hipError_t launch_zero(float* p, int64_t n, hipStream_t s);
// acc: dst += the sums instead of dst = (the explicit fine-tune derivatives)
// two gathers over the same transposed CSR in one launch (src -> dst, src2 -> dst2)
hipError_t launch_gather_rows2(int n, int D, const int* ptr, const int* perm, const float* src,
                               float* dst, const float* src2, float* dst2, hipStream_t s);
hipError_t launch_gather_rows(int n, int D, const int* ptr, const int* perm, const float* src,
                              float* dst, hipStream_t s, int acc = 0);
// the same over neighbour nodes [j_begin, j_end) only
hipError_t launch_gather_rows_range(int j_begin, int j_end, int D, const int* ptr, const int* perm,
                                    const float* src, float* dst, hipStream_t s, int acc = 0);
hipError_t launch_pack(int64_t n, int dim, const int* idx, const float* src, int64_t ss, float* dst,
                       hipStream_t s);
hipError_t launch_unpack(int64_t n, int dim, const int* idx, const float* src, float* dst,
                         int64_t ds, int acc, hipStream_t s);
}  // namespace e3gnn
