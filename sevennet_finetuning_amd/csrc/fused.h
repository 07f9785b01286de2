// Launch API of the fused radial-MLP + tensor-product kernels (fused.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace e3gnn {

// The struct is a kernel argument of the forward kernels too: the slots of the
// operands that only the reverse-mode radial backward read (W2 in the dH2
// orders, W1^T, W0^T) are kept, null, so that the forward kernels' argument
// layout -- and with it their code objects and the bits of the energy -- stay
// what they were (DESIGN.md 8 records how a change there once moved atomic
// energies by an ulp).
struct MlpW {
  const float* w0;   // [8][64]   layer0 / sqrt(8)
  const float* retired0;
  // w2 = layer2 / 8 ([64][W]) as three bf16 pieces (w2 = p0 + p1 + p2, exact) in
  // v_mfma_f32_16x16x32_bf16 operand order: [n/16][piece][m][g][c][t] = piece of
  // w2[16(2m + t/4) + 4g + t%4][n]
  const uint16_t* w2b;
  const uint16_t* retired1;
  // w2b's column blocks in the kernels' visiting order (block k at column 16 k;
  // model_load.cpp bwd_w_block_cols): the software-pipelined loops fetch the
  // operand of the block after next (last block only; null elsewhere)
  const uint16_t* w2v;
  // the lock-step backward's one image per PAIR of visited blocks (w2_image.h):
  // [pair][piece][hidden unit][swizzled 8-byte unit of 4 channels of one of the
  // pair's two blocks], staged in LDS by a straight copy; its transposed reads
  // are w2v's lane registers (first / middle blocks only)
  const uint16_t* w2s;
  // layer 1 (W1, 64 columns) in w2b's operand order: the value's and the
  // backward tangent's operand
  const uint16_t* w1b;
  const uint16_t* retired2;
  const uint16_t* retired3;
};

struct FusedArgs {
  const int* row_ptr;
  const int* center;  // [E] edge_index[0] (sorted)
  const int* nbr;
  const float* emb;   // [E, 8]
  const float* Y;     // [E, 9]
  const float* h;     // [n_nodes, DX]
  float* agg;         // fwd out [n_centers, DM]
  const float* gagg;  // bwd in  [n_centers, DM] (dE/dagg / denominator)
  const int* src_ptr;  // [n_nodes + 1] transposed CSR (edges by edge_index[1])
  const int* src_perm; // [E]
  float* dh;           // bwd out [n_nodes, DX]: dE/dx of the gathered features (last block)
  float* dxc;          // [E, DX] per-edge dE/dx (first / middle blocks; null: not stored)
  float* dgu;         // bwd in/out [E, 3]  dE/du accumulated over layers
  // the radial MLP's share of dE/dr in forward mode: sum over the block's
  // weights of dE/dw . dw/dr, the tangent dw/dr run through the MLP from embd
  const float* embd;  // bwd in     [E, 8]  d emb / dr (node.hip k_edge_embed)
  float* drad;        // bwd in/out [E]     dE/dr |radial accumulated over layers
  MlpW W;
  int n_centers;
  int n_edges;
  int n_nodes;
  float denom;
  // work range of one launch (halo overlap splits a layer into parts):
  // centres [c_begin, c_end) (forward, first / middle backward), neighbour
  // nodes [node_begin, node_end) (last backward)
  int c_begin, c_end, node_begin, node_end;
  // the CSR edges of the centre range, [row_ptr[c_begin], row_ptr[c_end]): the
  // first / middle backward partitions its launch by edges
  int e_begin, e_end;
};

// `kind` is a kind code of tp.h (3 * channel family + block kind)
hipError_t launch_conv_fwd(int kind, const FusedArgs& a, hipStream_t s);
// backward of a first / middle block: the lock-step kernel (rounds of four
// consecutive 16-edge tiles of the range [e_begin, e_end) per workgroup, W2
// operands staged per block pair in LDS), per-edge dE/dx to dxc, dE/du,
// dE/dw . dw/dr -> drad
hipError_t launch_conv_bwd_ls(int kind, const FusedArgs& a, hipStream_t s);
// backward of the last block, one wave per neighbour node: dE/dx to dh, dE/du,
// dE/dw . dw/dr -> drad
hipError_t launch_conv_bwd_nbr_last(int kind, const FusedArgs& a, hipStream_t s);

}  // namespace e3gnn
