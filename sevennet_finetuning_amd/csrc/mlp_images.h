// Host packers of the MFMA operand images built at model load
// (model_load.cpp): the radial MLP's weights in the lane orders of the fused
// kernels (fused.h MlpW) and the node linears' in k_nodelin_b's (gemm.hip).
// The bf16 images hold every weight as three pieces, w = p0 + p1 + p2 exactly
// (the same residual chain as w2_image.h's pair image, MlpW::w2s).  Images
// are returned as floats (two bf16 per float), as they are uploaded.
// Host-only: no kernel includes this header; tools/microtests/
// w2_dual_image.hip checks the w2b / w2d / w2v packers against their index
// formulas.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "w2_image.h"

namespace e3gnn {
namespace mlpimg {

using w2img::bf16_rne;
using w2img::bf16_to_f32;

// the residual chain: p[0] = rne(v), p[1] = rne(v - p[0]), p[2] = rne(v - p[0] - p[1])
// (bf16 round to nearest even; the subtractions are exact in f32)
inline void bf16_pieces(float v, uint16_t (&p)[3]) {
  for (int pc = 0; pc < 3; ++pc) {
    p[pc] = bf16_rne(v);
    v -= bf16_to_f32(p[pc]);
  }
}

// w2b (MlpW::w2b): a = p0 + p1 + p2 exactly (bf16 pieces, round to
// nearest even); element t of lane (g, c) in k-half m of column block cb
// is a[16(2m + t/4) + 4g + t%4][16 cb + c].  a: [64][N] (N a multiple of 16);
// also the order of w1b.
inline std::vector<float> pack_w2b(const std::vector<float>& a, int N) {
  std::vector<float> o((size_t)N * 64 * 3 / 2);
  uint16_t* oh = reinterpret_cast<uint16_t*>(o.data());
  for (int cb = 0; cb < N / 16; ++cb)
    for (int m2 = 0; m2 < 2; ++m2)
      for (int g = 0; g < 4; ++g)
        for (int c = 0; c < 16; ++c)
          for (int t = 0; t < 8; ++t) {
            uint16_t p[3];
            bf16_pieces(a[(size_t)(16 * (2 * m2 + t / 4) + 4 * g + t % 4) * N + 16 * cb + c], p);
            for (int pc = 0; pc < 3; ++pc)
              oh[((((size_t)cb * 3 + pc) * 2 + m2) * 64 + g * 16 + c) * 8 + t] = p[pc];
          }
  return o;
}

// w2d, the order the pair image's ROW reads give (w2_image.h row_read; no
// kernel reads it since the fused backward takes the radial derivative in
// forward mode, the microtest still checks the image against it): element t
// of lane (g, c) for hidden block bh is
// w2[16 bh + c][col], col = cols[2P] + 4g + t (t < 4) or cols[2P + 1] + 4g + t - 4.
// a2: [64][W]; cols: the visited 16-column blocks' starts, two per pair P.
inline std::vector<float> pack_w2d(const std::vector<float>& a2, int W, const std::vector<int>& cols) {
  std::vector<float> d2((size_t)W * 64 * 3 / 2);
  uint16_t* d2h = reinterpret_cast<uint16_t*>(d2.data());
  for (size_t P = 0; P < cols.size() / 2; ++P)
    for (int bh = 0; bh < 4; ++bh)
      for (int g = 0; g < 4; ++g)
        for (int c = 0; c < 16; ++c)
          for (int t8 = 0; t8 < 8; ++t8) {
            const int col = t8 < 4 ? cols[2 * P] + 4 * g + t8 : cols[2 * P + 1] + 4 * g + t8 - 4;
            uint16_t p[3];
            bf16_pieces(a2[(size_t)(16 * bh + c) * W + col], p);
            for (int pc = 0; pc < 3; ++pc)
              d2h[(((P * 3 + pc) * 4 + bh) * 64 + g * 16 + c) * 8 + t8] = p[pc];
          }
  return d2;
}

// w2v (MlpW::w2v): w2b's blocks in the visiting order of the kernels.
// b2: pack_w2b's image; block k of the result is b2's block cols[k] / 16.
inline std::vector<float> pack_w2v(const std::vector<float>& b2, const std::vector<int>& cols) {
  std::vector<float> v2(b2.size());
  const size_t blk = (size_t)64 * 16 * 3 / 2;   // floats per column block
  for (size_t k = 0; k < cols.size(); ++k)
    std::memcpy(v2.data() + k * blk, b2.data() + (size_t)(cols[k] / 16) * blk, blk * 4);
  return v2;
}

// The bf16x6 operand image of one k_nodelin_b block (gemm.hip): w = [K1 + K2][N]
// as three bf16 pieces (w = p0 + p1 + p2 exactly) in the 16x16x32 MFMA
// B-operand order: [16-column block cb][32-row chunk kc (K1's chunks, then
// K2's)][piece][lane][8], element t of lane l = w[k][16 cb + l % 16] with
// k = 32 kc' + 8 (l / 16) + t inside its part (0 past the part's rows / the
// block's columns).  1 KB per piece image: nodelin_b_floats floats at `out`.
inline size_t nodelin_b_floats(int K1, int K2, int N) {
  return (size_t)((N + 15) / 16) * ((K1 + 31) / 32 + (K2 + 31) / 32) * 3 * 256;
}
inline void pack_nodelin_b(const float* w, int K1, int K2, int N, float* out) {
  const int ncb = (N + 15) / 16, nk1 = (K1 + 31) / 32, nk2 = (K2 + 31) / 32;
  uint16_t* o = reinterpret_cast<uint16_t*>(out);
  for (int cb = 0; cb < ncb; ++cb)
    for (int kc = 0; kc < nk1 + nk2; ++kc)
      for (int l = 0; l < 64; ++l)
        for (int t = 0; t < 8; ++t) {
          const bool second = kc >= nk1;
          const int kk = 32 * (second ? kc - nk1 : kc) + 8 * (l / 16) + t;
          const int col = 16 * cb + l % 16;
          float v = 0.f;
          if (col < N && kk < (second ? K2 : K1)) v = w[(size_t)(second ? K1 + kk : kk) * N + col];
          uint16_t p[3];
          bf16_pieces(v, p);
          for (int pc = 0; pc < 3; ++pc)
            o[(((size_t)cb * (nk1 + nk2) + kc) * 3 + pc) * 512 + l * 8 + t] = p[pc];
        }
}

}  // namespace mlpimg
}  // namespace e3gnn
