// The lock-step backward's W2 image of one block PAIR (MlpW::w2s): one
// [hidden unit][channel] matrix per bf16 piece that serves both of the pair's
// MFMA operands, so a pair is staged in LDS once instead of as a matrix and
// its transpose.
//   * read by rows (ds_read_b64) it is the A operand of dH2 = W2[:, pair] dw^T
//     (rows = hidden units, K = the pair's 32 channels; the former w2d order).
//     No kernel takes this read any more: the fused backward forms the radial
//     derivative in forward mode from the transposed reads alone (fused.hip
//     w2_block_tan); row_read stays for the microtest that pins the layout;
//   * read transposed (ds_read_b64_tr_b16) it is the A operand of the w
//     recompute w^T = W2^T H2^T (rows = channels, K = hidden units; the former
//     w2v order).
// Layout: per piece 64 rows (hidden unit h) of 64 bytes; a row is eight 8-byte
// units, unit u = 2 q + b holding channels 4q .. 4q+3 of the pair's block b
// (b = 0: the 16 columns at cols[2P], b = 1: at cols[2P + 1]), stored at unit
// u ^ swz(h).  The host packer, both device readers and the microtest
// (tools/microtests/w2_dual_image.hip) address the image through off() alone.
//
// The swizzle, from the LDS bank rule (bank = (byte / 4) % 64, so a 256-byte
// bank row is four image rows and h % 4 picks its 64-byte quarter; both reads
// are serviced per 32-lane half, 32 x 8 bytes = one bank row when no two lanes
// share a unit position):
//   * row read, lane (g, c) reads units 2g and 2g + 1 of row 16 bh + c: the
//     half's lanes g = 0, 1 (or 2, 3) x c = 0..15 put four rows (c, c + 4,
//     c + 8, c + 12) x two units in every quarter, so those four rows need
//     four different XOR masks whose effect on {2g, 2g'} is disjoint:
//     swz = 0, 1, 4, 5 for (h >> 2) & 3 = 0..3 maps units {0, 2} to {0, 2},
//     {1, 3}, {4, 6}, {5, 7}: all eight positions of the quarter, once each.
//   * transposed read, lane 4q + p of 16-lane group g addresses unit 2p + b of
//     row R + 4g + q (R a multiple of 16): a half holds rows R .. R + 7 (or
//     R + 8 .. R + 15), rows r and r + 4 share a quarter and ask for the same
//     four units 2p + b -- bit 0 of swz (h >> 2) moves one of them to the
//     units 2p + (b ^ 1): again all eight positions once.
// Without bit 0 the transposed read is 2-way (both rows of a quarter on the
// same 8-byte halves of its four 16-byte chunks), without bit 2 the row read is.
#pragma once
#include <cstdint>
#include <cstring>

namespace e3gnn {
namespace w2img {

constexpr int ROWS = 64;                       // hidden units
constexpr int ROW_BYTES = 64;                  // 32 bf16: the pair's 2 x 16 channels
constexpr int PIECE_BYTES = ROWS * ROW_BYTES;  // one bf16 piece of a pair
constexpr int PIECES = 3;                      // pieces packed per pair (w2 = p0 + p1 + p2)
constexpr int PAIR_BYTES = PIECES * PIECE_BYTES;

constexpr int swz(int h) { return (((h >> 3) & 1) << 2) | ((h >> 2) & 1); }
// byte offset, from the pair's base, of 8-byte unit u (channels 4 (u >> 1) ..
// + 3 of block u & 1) of hidden unit h in piece pc
constexpr int off(int pc, int h, int u) { return pc * PIECE_BYTES + h * ROW_BYTES + 8 * (u ^ swz(h)); }

inline uint16_t bf16_rne(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// Host packer: a2 = W2 [64][W] (f32), cols = the visited blocks' column starts
// (two per pair), out = npairs * PAIR_BYTES bytes.  The pieces are the bf16
// round-to-nearest-even residual chain of w2b / w2d / w2v.
inline void pack(const float* a2, int W, const int* cols, int npairs, uint16_t* out) {
  for (int P = 0; P < npairs; ++P)
    for (int h = 0; h < ROWS; ++h)
      for (int b = 0; b < 2; ++b)
        for (int ch = 0; ch < 16; ++ch) {
          float v = a2[(size_t)h * W + cols[2 * P + b] + ch];
          for (int pc = 0; pc < PIECES; ++pc) {
            const uint16_t hb = bf16_rne(v);
            out[((size_t)P * PAIR_BYTES + off(pc, h, 2 * (ch >> 2) + b)) / 2 + (ch & 3)] = hb;
            v -= bf16_to_f32(hb);
          }
        }
}

#if defined(__HIPCC__)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// dH2 operand of lane (g, c) = lane >> 4, lane & 15 for hidden block bh,
// piece pc: row 16 bh + c, element t = channel 4g + t of block 0 (t < 4) or
// 4g + t - 4 of block 1 (two ds_read_b64; swz(16 bh + c) = swz(c))
__device__ __forceinline__ bf16x8 row_read(const char* img, int lane, int pc, int bh) {
  const int g = lane >> 4, c = lane & 15;
  const int a0 = off(0, c, 2 * g), a1 = a0 ^ 8;   // = off(0, c, 2 g + 1)
  const int k = pc * PIECE_BYTES + 16 * bh * ROW_BYTES;
  // volatile: two plain 8-byte reads off one base are merged into ds_read2_b64
  // / ds_read2st64_b64, which run at half the rate and bank modulo 32, where
  // this image is 2-way
  typedef const volatile __attribute__((address_space(3))) s16x4* lds_vp;
  const s16x4 lo = *(lds_vp)(img + a0 + k);
  const s16x4 hi = *(lds_vp)(img + a1 + k);
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// w-recompute operand of lane (g, c) for block b, piece pc, k-half m: element
// t = W2[16 (2m + t/4) + 4g + t%4][block b, channel c].  Two transposed
// reads of the 4-row x 16-channel blocks at rows 32 m + 16 j + 4g (j = 0, 1):
// lane 4q + p of the 16-lane group addresses row q's channels 4p .. 4p+3 and
// receives channel c of the four rows.  Every lane of the wave must be active
// (the gather crosses lanes), and all 64 addresses are in the image.
__device__ __forceinline__ bf16x8 tr_read(const char* img, int lane, int b, int pc, int m) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  // swz(32 m + 16 j + 4g + q) = swz(4g + q)
  const int a = off(0, 4 * g + q, 2 * p) ^ (8 * b);   // = off(0, 4g + q, 2p + b)
  const int k = pc * PIECE_BYTES + 32 * m * ROW_BYTES;
  typedef __attribute__((address_space(3))) s16x4* lds_p;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + a + k));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(img + a + k + 16 * ROW_BYTES));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
#endif

}  // namespace w2img
}  // namespace e3gnn
