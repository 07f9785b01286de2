// The lock-step backward's one W2 image per block pair (csrc/w2_image.h)
// against the two operand orders it replaces: for every lane, block, piece
// and k-half the transposed read (ds_read_b64_tr_b16) must deliver the
// registers of the w2v order, and for every lane, piece and hidden block the
// row read those of the w2d order -- bit for bit; and the w-recompute and
// dH2 three-product MFMA chains must give the same accumulator bits from
// either source.  W2 is random f32, 64 x 64 columns = two pairs, visited out
// of column order; the image is packed by the header's packer and staged in
// LDS as k_conv_bwd_ls stages it (256 threads, tid-strided b128 copy).
//   w2_dual_image              the whole test (needs a gfx950 device)
//   w2_dual_image --host-only  packers against the index formulas only: the
//                              reads are emulated on the host, and the w2b /
//                              w2v / w2d packers of csrc/mlp_images.h must
//                              equal the restated formulas (no device)
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 w2_dual_image.hip -o w2_dual_image
// (the host part also under -Xarch_host -fsanitize=address,undefined, run --host-only)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../sevennet_finetuning_amd/csrc/mlp_images.h"
#include "../../sevennet_finetuning_amd/csrc/w2_image.h"

namespace wi = e3gnn::w2img;
namespace mi = e3gnn::mlpimg;
constexpr int W = 64, NPAIR = 2, NWAVE = 4;
static const int COLS[2 * NPAIR] = {16, 48, 32, 0};   // visiting order of the 16-column blocks

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// per (pair, wave, lane): registers read from the image and the products
struct Out {
  uint16_t tr[2][3][2][8];    // [block][piece][k-half][t]: w2v order
  uint16_t row[3][4][8];      // [piece][hidden block][t]: w2d order
  float w_img[2][4], w_ref[2][4];      // w recompute of the pair's two blocks
  float dh_img[4][4], dh_ref[4][4];    // dH2 of the four hidden blocks
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// s2: packed images; v2 / d2: the w2v / w2d orders; hq: [wave][piece 2][half 2][lane][8]
// random H2 pieces; dq: [wave][piece 2][lane][8] random dw pieces
__global__ __launch_bounds__(256) void k(const uint16_t* s2, const uint16_t* v2, const uint16_t* d2,
                                         const uint16_t* hq, const uint16_t* dq, Out* out) {
  __shared__ __attribute__((aligned(16))) char img[wi::PAIR_BYTES];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  for (int P = 0; P < NPAIR; ++P) {
    __syncthreads();
    for (int i = 0; i < wi::PAIR_BYTES / 16 / 256; ++i)
      *reinterpret_cast<f32x4*>(img + (tid + 256 * i) * 16) =
          *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(s2) + P * wi::PAIR_BYTES + (tid + 256 * i) * 16);
    __syncthreads();
    Out& o = out[(P * NWAVE + wid) * 64 + lane];
    bf16x8 h[2][2], d[2];
    for (int pc = 0; pc < 2; ++pc) {
      for (int m = 0; m < 2; ++m)
        h[pc][m] = *reinterpret_cast<const bf16x8*>(hq + (((wid * 2 + pc) * 2 + m) * 64 + lane) * 8);
      d[pc] = *reinterpret_cast<const bf16x8*>(dq + ((wid * 2 + pc) * 64 + lane) * 8);
    }
    for (int b = 0; b < 2; ++b) {
      bf16x8 wt[3][2], wr[3][2];
      for (int pc = 0; pc < 3; ++pc)
        for (int m = 0; m < 2; ++m) {
          wt[pc][m] = wi::tr_read(img, lane, b, pc, m);
          wr[pc][m] = *reinterpret_cast<const bf16x8*>(v2 + (((((2 * P + b) * 3 + pc) * 2 + m) * 64) + lane) * 8);
          *reinterpret_cast<bf16x8*>(o.tr[b][pc][m]) = wt[pc][m];
        }
      // fused.hip w2_block3<false>: A = W2^T pieces, B = H2 pieces
      f32x4 ai = {0.f, 0.f, 0.f, 0.f}, ar = ai;
      for (int m = 0; m < 2; ++m) {
        ai = mfma16(wt[0][m], h[1][m], ai), ar = mfma16(wr[0][m], h[1][m], ar);
        ai = mfma16(wt[1][m], h[0][m], ai), ar = mfma16(wr[1][m], h[0][m], ar);
        ai = mfma16(wt[0][m], h[0][m], ai), ar = mfma16(wr[0][m], h[0][m], ar);
      }
      for (int r = 0; r < 4; ++r) o.w_img[b][r] = ai[r], o.w_ref[b][r] = ar[r];
    }
    for (int bh = 0; bh < 4; ++bh) {
      bf16x8 at[3], ar[3];
      for (int pc = 0; pc < 3; ++pc) {
        at[pc] = wi::row_read(img, lane, pc, bh);
        ar[pc] = *reinterpret_cast<const bf16x8*>(d2 + ((((P * 3 + pc) * 4 + bh) * 64) + lane) * 8);
        *reinterpret_cast<bf16x8*>(o.row[pc][bh]) = at[pc];
      }
      // fused.hip dh2_pair, three products
      f32x4 ci = {0.f, 0.f, 0.f, 0.f}, cr = ci;
      ci = mfma16(at[1], d[0], ci), cr = mfma16(ar[1], d[0], cr);
      ci = mfma16(at[0], d[1], ci), cr = mfma16(ar[0], d[1], cr);
      ci = mfma16(at[0], d[0], ci), cr = mfma16(ar[0], d[0], cr);
      for (int r = 0; r < 4; ++r) o.dh_img[bh][r] = ci[r], o.dh_ref[bh][r] = cr[r];
    }
  }
}

static float frand() { return (float)(rand() & 0xffffff) / 8388608.f - 1.f; }

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !strcmp(argv[1], "--host-only");
  srand(7);
  std::vector<float> a2((size_t)64 * W);
  for (auto& x : a2) x = frand() * 0.37f;
  std::vector<uint16_t> s2((size_t)NPAIR * wi::PAIR_BYTES / 2, 0xdead);
  wi::pack(a2.data(), W, COLS, NPAIR, s2.data());

  // the index formulas of mlp_images.h's packers, restated (model_load.cpp
  // builds the library's images with those packers): the pieces are the bf16
  // residual chain
  auto piece = [&](int h, int col, int pc) {
    float v = a2[(size_t)h * W + col];
    uint16_t hb = 0;
    for (int q = 0; q <= pc; ++q) {
      hb = wi::bf16_rne(v);
      v -= wi::bf16_to_f32(hb);
    }
    return hb;
  };
  // w2v: block k in visiting order, element t of lane (g, c) in k-half m =
  // w2[16 (2m + t/4) + 4g + t%4][cols[k] + c]
  std::vector<uint16_t> v2((size_t)2 * NPAIR * 3 * 2 * 64 * 8);
  for (int k = 0; k < 2 * NPAIR; ++k)
    for (int pc = 0; pc < 3; ++pc)
      for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
          for (int c = 0; c < 16; ++c)
            for (int t = 0; t < 8; ++t)
              v2[((((size_t)k * 3 + pc) * 2 + m) * 64 + g * 16 + c) * 8 + t] =
                  piece(16 * (2 * m + t / 4) + 4 * g + t % 4, COLS[k] + c, pc);
  // w2d: element t of lane (g, c) for hidden block bh = w2[16 bh + c][col],
  // col = cols[2P] + 4g + t (t < 4) or cols[2P + 1] + 4g + t - 4
  std::vector<uint16_t> d2((size_t)NPAIR * 3 * 4 * 64 * 8);
  for (int P = 0; P < NPAIR; ++P)
    for (int pc = 0; pc < 3; ++pc)
      for (int bh = 0; bh < 4; ++bh)
        for (int g = 0; g < 4; ++g)
          for (int c = 0; c < 16; ++c)
            for (int t = 0; t < 8; ++t)
              d2[((((size_t)P * 3 + pc) * 4 + bh) * 64 + g * 16 + c) * 8 + t] =
                  piece(16 * bh + c, t < 4 ? COLS[2 * P] + 4 * g + t : COLS[2 * P + 1] + 4 * g + t - 4, pc);

  // host part: the two reads emulated over the packed bytes
  int bad_tr = 0, bad_row = 0, bad_cover = 0;
  for (int P = 0; P < NPAIR; ++P) {
    const char* img = reinterpret_cast<const char*>(s2.data()) + (size_t)P * wi::PAIR_BYTES;
    for (int lane = 0; lane < 64; ++lane) {
      const int g = lane >> 4, c = lane & 15;
      for (int b = 0; b < 2; ++b)
        for (int pc = 0; pc < 3; ++pc)
          for (int m = 0; m < 2; ++m) {
            uint16_t got[8];
            for (int j = 0; j < 2; ++j)
              for (int q = 0; q < 4; ++q) {
                // the address lane 4q + p of the group supplies, p = c / 4;
                // lane c takes element c % 4 of it
                const int row = 32 * m + 16 * j + 4 * g + q;
                memcpy(&got[4 * j + q], img + wi::off(pc, row, 2 * (c >> 2) + b) + 2 * (c & 3), 2);
              }
            if (memcmp(got, &v2[(((((size_t)(2 * P + b)) * 3 + pc) * 2 + m) * 64 + lane) * 8], 16)) ++bad_tr;
          }
      for (int pc = 0; pc < 3; ++pc)
        for (int bh = 0; bh < 4; ++bh) {
          uint16_t got[8];
          memcpy(got, img + wi::off(pc, 16 * bh + c, 2 * g), 8);
          memcpy(got + 4, img + wi::off(pc, 16 * bh + c, 2 * g + 1), 8);
          if (memcmp(got, &d2[((((size_t)P * 3 + pc) * 4 + bh) * 64 + lane) * 8], 16)) ++bad_row;
        }
    }
  }
  // off() is a bijection of (piece, row, unit) onto the pair's 8-byte units
  {
    std::vector<char> seen(wi::PAIR_BYTES / 8, 0);
    for (int pc = 0; pc < wi::PIECES; ++pc)
      for (int h = 0; h < wi::ROWS; ++h)
        for (int u = 0; u < 8; ++u) {
          const int o = wi::off(pc, h, u);
          if (o < 0 || o % 8 || o >= wi::PAIR_BYTES || seen[o / 8]++) ++bad_cover;
        }
  }
  printf("host: transposed-read mismatches %d, row-read mismatches %d, off() collisions %d\n", bad_tr, bad_row,
         bad_cover);
  // the library's packers (mlp_images.h) against the restated formulas, bit
  // for bit: w2v and w2d above, and w2b = block cb at column 16 cb (w2v's
  // formula in column order)
  int bad_pack = 0;
  {
    const std::vector<int> cols(COLS, COLS + 2 * NPAIR);
    auto differs = [](const std::vector<float>& img, const std::vector<uint16_t>& ref) {
      return img.size() * 4 != ref.size() * 2 || memcmp(img.data(), ref.data(), ref.size() * 2) != 0;
    };
    const std::vector<float> b2 = mi::pack_w2b(a2, W);
    std::vector<uint16_t> b2ref(v2.size());
    for (int cb = 0; cb < W / 16; ++cb)
      for (int pc = 0; pc < 3; ++pc)
        for (int m = 0; m < 2; ++m)
          for (int g = 0; g < 4; ++g)
            for (int c = 0; c < 16; ++c)
              for (int t = 0; t < 8; ++t)
                b2ref[((((size_t)cb * 3 + pc) * 2 + m) * 64 + g * 16 + c) * 8 + t] =
                    piece(16 * (2 * m + t / 4) + 4 * g + t % 4, 16 * cb + c, pc);
    bad_pack += differs(b2, b2ref);
    bad_pack += differs(mi::pack_w2v(b2, cols), v2);
    bad_pack += differs(mi::pack_w2d(a2, W, cols), d2);
  }
  printf("host: packer images (w2b, w2v, w2d) differing from the formulas %d\n", bad_pack);
  int bad = bad_tr + bad_row + bad_cover + bad_pack;
  if (host_only) return bad != 0;

  std::vector<uint16_t> hq((size_t)NWAVE * 2 * 2 * 64 * 8), dq((size_t)NWAVE * 2 * 64 * 8);
  for (auto& x : hq) x = wi::bf16_rne(frand());
  for (auto& x : dq) x = wi::bf16_rne(frand() * 0.01f);
  const size_t nout = (size_t)NPAIR * NWAVE * 64;
  std::vector<Out> out(nout);
  uint16_t *ds2, *dv2, *dd2, *dhq, *ddq;
  Out* dout;
  if (hipMalloc(&ds2, s2.size() * 2) || hipMalloc(&dv2, v2.size() * 2) || hipMalloc(&dd2, d2.size() * 2) ||
      hipMalloc(&dhq, hq.size() * 2) || hipMalloc(&ddq, dq.size() * 2) || hipMalloc(&dout, nout * sizeof(Out)))
    return 2;
  if (hipMemcpy(ds2, s2.data(), s2.size() * 2, hipMemcpyHostToDevice) ||
      hipMemcpy(dv2, v2.data(), v2.size() * 2, hipMemcpyHostToDevice) ||
      hipMemcpy(dd2, d2.data(), d2.size() * 2, hipMemcpyHostToDevice) ||
      hipMemcpy(dhq, hq.data(), hq.size() * 2, hipMemcpyHostToDevice) ||
      hipMemcpy(ddq, dq.data(), dq.size() * 2, hipMemcpyHostToDevice) || hipMemset(dout, 0xff, nout * sizeof(Out)))
    return 2;
  hipLaunchKernelGGL(k, dim3(1), dim3(256), 0, 0, ds2, dv2, dd2, dhq, ddq, dout);
  if (hipGetLastError() || hipMemcpy(out.data(), dout, nout * sizeof(Out), hipMemcpyDeviceToHost)) return 2;
  int g_tr = 0, g_row = 0, g_w = 0, g_dh = 0;
  for (int P = 0; P < NPAIR; ++P)
    for (int w = 0; w < NWAVE; ++w)
      for (int lane = 0; lane < 64; ++lane) {
        const Out& o = out[((size_t)P * NWAVE + w) * 64 + lane];
        for (int b = 0; b < 2; ++b)
          for (int pc = 0; pc < 3; ++pc)
            for (int m = 0; m < 2; ++m)
              if (memcmp(o.tr[b][pc][m], &v2[(((((size_t)(2 * P + b)) * 3 + pc) * 2 + m) * 64 + lane) * 8], 16))
                ++g_tr;
        for (int pc = 0; pc < 3; ++pc)
          for (int bh = 0; bh < 4; ++bh)
            if (memcmp(o.row[pc][bh], &d2[((((size_t)P * 3 + pc) * 4 + bh) * 64 + lane) * 8], 16)) ++g_row;
        if (memcmp(o.w_img, o.w_ref, sizeof o.w_img)) ++g_w;
        if (memcmp(o.dh_img, o.dh_ref, sizeof o.dh_img)) ++g_dh;
      }
  // the products are not all zero (a dead kernel would compare equal)
  double s = 0;
  for (auto& o : out)
    for (int r = 0; r < 4; ++r) s += (double)o.w_ref[0][r] * o.w_ref[0][r] + (double)o.dh_ref[0][r] * o.dh_ref[0][r];
  printf("gpu: transposed-read mismatches %d, row-read mismatches %d, w-recompute mismatches %d, "
         "dH2 mismatches %d (sum of squares %.6g)\n", g_tr, g_row, g_w, g_dh, s);
  bad += g_tr + g_row + g_w + g_dh + !(s > 0 && s < 1e30);
  return bad != 0;
}
