// Fused radial-MLP + tensor-product kernels (forward and force backward), gfx950.
//
// Reference: IrrepsConvolution.forward (sevenn/nn/convolution.py:104-123):
//   w = FCN(edge_embedding)                      (e3nn FullyConnectedNet 8->64->64->W)
//   msg = TP(x[edge_index[1]], Y, w)              (uvu, convolution.py:72-95)
//   agg = scatter_sum(msg, edge_index[0]) / denominator
// and its reverse-mode pass (what ForceStressOutput obtains through autograd,
// force_output.py:74-130).  The per-edge weights w (E x 960 for the middle
// blocks) never touch HBM: f32 MFMA produces them directly in the registers the
// tensor product reads.
//
// Mapping: one wave = one centre (forward, first / middle backward) or one
// neighbour node (last backward), its edges in tiles of 16 edge slots.
//   * v_mfma_f32_16x16x4_f32: A lane l = A[i=l&15][k=l>>4], B lane l =
//     B[k=l>>4][j=l&15], D lane l reg r = D[4(l>>4)+r][l&15].  Lane group
//     g = l>>4, column c = l&15.
//   * The MLP runs transposed (H^T = W^T emb^T: rows = hidden units, columns =
//     edge slots), so every product's accumulator is the k-operand of the next
//     one; the 64 -> W layer (90 % of the MLP FLOPs) on bf16x6 MFMA (below).
//   * Forward: w = H2 W2[:, 16-column block], lane (g, c) holds w[edge 4g+r]
//     [channel c]; two tiles per pass share every W2 operand block; the
//     message is summed over registers and the 4 lane groups into the
//     centre's row in LDS.  Backward (lock-step, four consecutive 16-edge
//     tiles per round whatever their centres, W2 pieces staged per block
//     pair in LDS): w^T recomputed, lane (g, c) =
//     edge c x channels 4g..4g+3; dE/dx per edge, dE/dY -> dE/du, and the
//     radial MLP's share of dE/dr in forward mode: dE/dw . w', the tangent
//     w' = dw/dr formed beside w from the same W2 operand registers.
//   * Weights via buffer descriptors (scalar k offsets, one VGPR of lane offset).
// Deterministic: no atomics; every sum has a fixed order.
#include "cg_tables.h"
#include "common.h"
#include "fused.h"
#include "tp.h"
#include "w2_image.h"

#include <type_traits>


namespace e3gnn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int N, int I = 0, class F>
constexpr void sfor_host(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor_host<N, I + 1>(f);
  }
}
template <int N, int I = 0, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor<N, I + 1>(f);
  }
}

__device__ __forceinline__ constexpr int yoff(int l) { return l == 0 ? 0 : (l == 1 ? 1 : 4); }
// hidden unit of k-step s, lane group 0 (add 4g): 16(s>>2) + (s&3)
__device__ __forceinline__ constexpr int KH(int s) { return 16 * (s >> 2) + (s & 3); }

// Phase fence: keeps the scheduler from interleaving (and hoisting loads across)
// the MFMA chain of one column block and the tensor product of another, which
// otherwise multiplies live registers and halves occupancy.
__device__ __forceinline__ void phase() { __builtin_amdgcn_sched_barrier(0); }

// Diagnostic build only (-DE3GNN_STAMPS, never the shipped library): per-wave
// s_memtime totals of the middle backward's phases, written by lane 0 to a
// buffer of their own (e3gnn_debug_stamps) that no other code reads.
// E3GNN_STAMPS_FWD=1 (with E3GNN_STAMPS): the middle FORWARD's phases instead
#ifndef E3GNN_STAMPS_FWD
#define E3GNN_STAMPS_FWD 0
#endif
#ifdef E3GNN_STAMPS
__device__ unsigned long long* g_stamp_buf = nullptr;
#define STAMP_N 8
#define STAMP_DECL                               \
  unsigned long long st_acc[STAMP_N] = {0, 0, 0, 0, 0, 0, 0, 0}; \
  unsigned long long st_t = __builtin_amdgcn_s_memtime(), st_t0 = st_t;
#define STAMP(k)                                          \
  do {                                                    \
    const unsigned long long st_now = __builtin_amdgcn_s_memtime(); \
    st_acc[k] += st_now - st_t;                           \
    st_t = st_now;                                        \
  } while (0)
#define STAMP_FLUSH(wave)                                                   \
  do {                                                                      \
    if (g_stamp_buf && lane == 0) {                                         \
      st_acc[7] = __builtin_amdgcn_s_memtime() - st_t0;                     \
      for (int k_ = 0; k_ < STAMP_N; ++k_) g_stamp_buf[(int64_t)(wave) * STAMP_N + k_] = st_acc[k_]; \
    }                                                                       \
  } while (0)
#else
#define STAMP_DECL
#define STAMP(k) \
  do {           \
  } while (0)
#define STAMP_FLUSH(wave) \
  do {                    \
  } while (0)
#endif

// materialise a value here: stops the compiler from sinking an accumulation
// chain past later paths (which keeps every partial product live)
template <int N>
__device__ __forceinline__ void pin(float* v) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" : "+v"(v[i]));
}

__device__ __forceinline__ f32x4 zero4() {
  f32x4 z;
  z[0] = z[1] = z[2] = z[3] = 0.f;
  return z;
}
__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------- weight operands
// Weight operands are read through buffer descriptors: the per-lane part of the
// offset is one VGPR and the per-k-step part a scalar (soffset), so the compiler
// does not hoist hundreds of 64-bit addresses out of the centre loop (which it
// did, and spilled).  Offsets outside the descriptor read 0 (padded rows).
struct WRes {
  __amdgpu_buffer_rsrc_t w0, w2b, w2v, w1b;
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const float* p, int nfloats) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, nfloats * 4, 0x00020000);
}
__device__ __forceinline__ WRes make_wres(const MlpW& W, int width) {
  return {rsrc(W.w0, 8 * 64), rsrc((const float*)W.w2b, 64 * width * 3 / 2),
          rsrc((const float*)W.w2v, 64 * width * 3 / 2), rsrc((const float*)W.w1b, 64 * 64 * 3 / 2)};
}
__device__ __forceinline__ float ldw(__amdgpu_buffer_rsrc_t r, int vbytes, int sbytes) {
  // the builtin returns the raw 32 bits (an unsigned int): reinterpret, never convert
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vbytes, sbytes, 0));
}

__device__ __forceinline__ f32x4 ldw4(__amdgpu_buffer_rsrc_t r, int vbytes, int sbytes) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, vbytes, sbytes, 0));
}
// N contiguous floats from one lane offset (b128/b96/b64 pieces; dword alignment)
template <int N>
__device__ __forceinline__ void ldv(__amdgpu_buffer_rsrc_t r, int vbytes, int sbytes, float* o) {
  if constexpr (N >= 4) {
    const f32x4 v = ldw4(r, vbytes, sbytes);
    o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    ldv<N - 4>(r, vbytes, sbytes + 16, o + 4);
  } else if constexpr (N == 3) {
    typedef float f32x3 __attribute__((ext_vector_type(3)));
    const f32x3 v = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(r, vbytes, sbytes, 0));
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
  } else if constexpr (N == 2) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, vbytes, sbytes, 0));
    o[0] = v[0], o[1] = v[1];
  } else if constexpr (N == 1) {
    o[0] = ldw(r, vbytes, sbytes);
  }
}

__device__ __forceinline__ void stw(float v, __amdgpu_buffer_rsrc_t r, int vbytes, int sbytes) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, vbytes, sbytes, 0);
}
// N contiguous floats to one lane offset (b128 pieces; 16-byte aligned);
// offsets outside the descriptor are dropped
template <int N>
__device__ __forceinline__ void stv(__amdgpu_buffer_rsrc_t r, int vbytes, int sbytes, const float* v) {
  static_assert(N % 4 == 0, "b128 pieces");
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    f32x4 t;
    t[0] = v[4 * q], t[1] = v[4 * q + 1], t[2] = v[4 * q + 2], t[3] = v[4 * q + 3];
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, t), r,
                                           vbytes, sbytes + 16 * q, 0);
  }
}
// descriptor over [p, p + nbytes) (nbytes clamped to the 32-bit range)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_bytes(const void* p, int64_t nbytes) {
  const int n = nbytes > 0x7fffffff ? 0x7fffffff : (int)nbytes;
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, n, 0x00020000);
}

// ---------------------------------------------------------------- w = H2 W2 on bf16 MFMA
// The 64 -> W layer of the radial MLP (90 % of its FLOPs) runs on
// v_mfma_f32_16x16x32_bf16 with both operands split into three bf16 pieces
// (x = p0 + p1 + p2 exactly, 24 significant bits) and the six piece products
// with i + j <= 2 accumulated in f32, smallest first: f32-grade accuracy (the
// dropped terms are below 2^-24 relative) at 12 x 16 = 192 MFMA cycles per
// 16 x 16 x 64 block instead of 16 x 32 = 512 on v_mfma_f32_16x16x4_f32.
// k order: element t of lane group g in k-half m is hidden unit
// 16(2m + t/4) + 4g + t%4, which is exactly register (bh = 2m + t/4, r = t%4)
// of the H2 accumulators a lane already holds -- no lane movement.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
struct Op3 {
  bf16x8 v[3][2];  // [piece][k-half]
};
// W2 operand of column block col0 (w2b order, 6 x b128 per lane)
__device__ __forceinline__ void load_w2b(Op3& o, __amdgpu_buffer_rsrc_t w2b, int lane, int col0) {
#pragma unroll
  for (int pc = 0; pc < 3; ++pc)
#pragma unroll
    for (int m = 0; m < 2; ++m)
      o.v[pc][m] = __builtin_bit_cast(
          bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w2b, lane * 16, ((col0 / 16 * 3 + pc) * 2 + m) * 1024, 0));
}
// Eight floats as three bf16 pieces (v = p0 + p1 + p2, each piece the
// round-to-nearest-even bf16 of the remaining residual), two values per
// v_cvt_pk_bf16_f32: the packed pair is both the MFMA operand word and, widened
// by a shift / mask, what the residual subtracts (5.5 VALU per value instead of
// the 7.5 of per-value conversions re-packed afterwards; same bits)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split3x8(const float (&v)[8], bf16x8 (&d)[3]) {
  u32x4 w[3];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x2 r;
    r[0] = v[2 * q];
    r[1] = v[2 * q + 1];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
      const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
      w[pc][q] = u;
      if (pc < 2) {
        r[0] -= __builtin_bit_cast(float, u << 16);
        r[1] -= __builtin_bit_cast(float, u & 0xffff0000u);
      }
    }
  }
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) d[pc] = __builtin_bit_cast(bf16x8, w[pc]);
}

// the lane's 16 H2 values (units 16 bh + 4g + r) as three bf16 pieces
__device__ __forceinline__ void split_h2(const f32x4 (&h2)[4], Op3& o) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = h2[2 * m + (t >> 2)][t & 3];
    bf16x8 d[3];
    split3x8(v, d);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) o.v[pc][m] = d[pc];
  }
}
// HA: H2 is the A operand (rows = edges: forward); else W2^T is (rows = channels)
template <bool HA>
__device__ __forceinline__ f32x4 w2_block(const Op3& h, const Op3& w) {
  constexpr int I[6] = {2, 1, 0, 1, 0, 0}, J[6] = {0, 1, 2, 0, 1, 0};
  f32x4 acc = zero4();
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int m = 0; m < 2; ++m)
      acc = HA ? mfma16(h.v[I[q]][m], w.v[J[q]][m], acc) : mfma16(w.v[J[q]][m], h.v[I[q]][m], acc);
  return acc;
}

// the same block from the first two pieces only (three products): the
// backward kernels' w recompute (default; E3GNN_BWD_W_X3=0: six).  The energy
// keeps the forward's six-product w; the recomputed w differs from it by
// ~2^-16 relative, and the force errors against the reference KATs did not
// move (max 1.91e-5 -> 1.89e-5 eV/A over the five systems; 97k / 778k
// full-size checks green); middle backward -5.5 %, first block -11 %
template <bool HA>
__device__ __forceinline__ f32x4 w2_block3(const Op3& h, const Op3& w) {
  f32x4 acc = zero4();
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    acc = HA ? mfma16(h.v[1][m], w.v[0][m], acc) : mfma16(w.v[0][m], h.v[1][m], acc);
    acc = HA ? mfma16(h.v[0][m], w.v[1][m], acc) : mfma16(w.v[1][m], h.v[0][m], acc);
    acc = HA ? mfma16(h.v[0][m], w.v[0][m], acc) : mfma16(w.v[0][m], h.v[0][m], acc);
  }
  return acc;
}
#ifndef E3GNN_BWD_W_X3
#define E3GNN_BWD_W_X3 1
#endif
template <bool HA>
__device__ __forceinline__ f32x4 w2_block_bwd(const Op3& h, const Op3& w) {
  if constexpr (E3GNN_BWD_W_X3) return w2_block3<HA>(h, w);
  else return w2_block<HA>(h, w);
}
// the backward kernels' tangent product w' = W2^T H2'^T (mlp_chain_jvp): the
// w recompute's W2 operand registers against the pieces of H2'.  It took the
// place of the reverse-mode dH2 = dw W2^T and keeps that product's switch:
// three bf16 products by default (dropped terms ~2^-16 of w'; the dH2 form's
// measurements on the reference KAT systems: force errors 2.9e-6 .. 2.1e-5
// against the six-product build's 3.1e-6 .. 1.9e-5 eV/A, tolerance 1e-4),
// E3GNN_DH2_X3=0: six
#ifndef E3GNN_DH2_X3
#define E3GNN_DH2_X3 1
#endif
template <bool HA>
__device__ __forceinline__ f32x4 w2_block_tan(const Op3& hd, const Op3& w) {
  if constexpr (E3GNN_DH2_X3) return w2_block3<HA>(hd, w);
  else return w2_block<HA>(hd, w);
}

// ---------------------------------------------------------------- radial MLP
// Tile of 16 edge slots [e0, e0+16) (slots >= e1 are zero rows).
// a1/a2: pre-activations of the two hidden layers, transposed (4 blocks of 16 units).
struct MlpT {
  f32x4 a1[4], a2[4];
};

// b[s] = emb[edge of slot (l&15)][4s + (l>>4)]
// Layer 0 (K = 8) on f32 MFMA; layer 1 (64 -> 64) on bf16x6 like w = H2 W2
// (w2_block: act(a1) split in three bf16 pieces in its accumulator layout, W1
// pre-split in the same operand order, MlpW::w1b): 48 MFMAs x 16 cycles
// instead of 64 x 32 on v_mfma_f32_16x16x4_f32, f32-grade.
__device__ __forceinline__ void mlp_layer0(const WRes& R, const float (&b)[2], int lane, f32x4 (&a1)[4]) {
  const int g = lane >> 4, c = lane & 15;
  const int v0 = (g * 64 + c) * 4;  // W0s[4s + g][16 bh + c]
#pragma unroll
  for (int bh = 0; bh < 4; ++bh) {
    f32x4 acc = zero4();
#pragma unroll
    for (int s = 0; s < 2; ++s) acc = mfma(ldw(R.w0, v0, (4 * s * 64 + 16 * bh) * 4), b[s], acc);
    a1[bh] = acc;
  }
}
// The backward kernels' layer-1 products (the recompute and its tangent, see
// mlp_chain_jvp) on three bf16 products like the w recompute (E3GNN_CHAIN_X3,
// default; =0 six); the forward, whose chain gives the energy, keeps six.
// Measured with the reverse-mode chain this replaced: step 39.8 -> 39.2 ms;
// parity, full-size and family tests green; NVE drift over 2,000 steps 1.67e-4
// meV/atom/ps against 1.38e-4 (six-product chains) and 1.19e-4 (exact-gradient
// generic engine), excursions identical (profiles/r06_s18_*)
#ifndef E3GNN_CHAIN_X3
#define E3GNN_CHAIN_X3 1
#endif
constexpr bool CX3 = E3GNN_CHAIN_X3 != 0;
__device__ __forceinline__ void mlp_chain(const WRes& R, const float (&b)[2], int lane, MlpT& m) {
  mlp_layer0(R, b, lane, m.a1);
  Op3 hq;
  {
    f32x4 h1[4];
#pragma unroll
    for (int bh = 0; bh < 4; ++bh)
#pragma unroll
      for (int r = 0; r < 4; ++r) h1[bh][r] = act_fwd(m.a1[bh][r]);
    split_h2(h1, hq);
  }
#pragma unroll
  for (int bo = 0; bo < 4; ++bo) {
    phase();
    Op3 wq;
    load_w2b(wq, R.w1b, lane, 16 * bo);
    m.a2[bo] = w2_block<false>(hq, wq);
  }
}

// The backward kernels' chain: the tile's H2 and its TANGENT H2' = dH2/dr, in
// the w product's operand pieces.  The radial MLP has one scalar input, r, so
// the radial share of dE/dr is taken in forward mode: emb' = d emb / dr
// (k_edge_embed's embd; b / bd = the lane's emb / emb' values, mlp_pre's
// order; padded slots 0) runs through the same layers,
//   a1' = W0^T emb',  H1' = act'(a1) a1',  a2' = W1^T H1',  H2' = act'(a2) a2',
// every W0 fragment and W1 operand block loaded once for value and tangent
// (the products of E3GNN_CHAIN_X3 for both), and the kernels contract
// w' = W2^T H2' with the dE/dw they hold in w's layout.  No W1^T / W0^T
// operands, no dH2 accumulators and no pre-activations kept to the tile end.
__device__ __forceinline__ void mlp_chain_jvp(const WRes& R, const float (&b)[2], const float (&bd)[2], int lane,
                                              Op3& h2q, Op3& h2dq) {
  const int g = lane >> 4, c = lane & 15;
  const int v0 = (g * 64 + c) * 4;  // W0s[4s + g][16 bh + c]
  Op3 hq, hdq;
  {
    f32x4 h1[4], h1d[4];
#pragma unroll
    for (int bh = 0; bh < 4; ++bh) {
      f32x4 acc = zero4(), accd = zero4();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float w = ldw(R.w0, v0, (4 * s * 64 + 16 * bh) * 4);
        acc = mfma(w, b[s], acc);
        accd = mfma(w, bd[s], accd);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        h1[bh][r] = act_fwd(acc[r]);
        h1d[bh][r] = act_grad(acc[r]) * accd[r];
      }
    }
    split_h2(h1, hq);
    split_h2(h1d, hdq);
  }
  f32x4 h2[4], h2d[4];
#pragma unroll
  for (int bo = 0; bo < 4; ++bo) {
    phase();
    Op3 wq;
    load_w2b(wq, R.w1b, lane, 16 * bo);
    const f32x4 a2 = CX3 ? w2_block3<false>(hq, wq) : w2_block<false>(hq, wq);
    const f32x4 a2d = CX3 ? w2_block3<false>(hdq, wq) : w2_block<false>(hdq, wq);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h2[bo][r] = act_fwd(a2[r]);
      h2d[bo][r] = act_grad(a2[r]) * a2d[r];
    }
  }
  split_h2(h2, h2q);
  split_h2(h2d, h2dq);
}

__device__ __forceinline__ void mlp_pre(const WRes& R, const float* __restrict__ emb, int e0,
                                        int e1, int lane, MlpT& m) {
  const int g = lane >> 4, c = lane & 15;
  const int e = e0 + c;
  float b[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) b[s] = e < e1 ? emb[(int64_t)e * 8 + 4 * s + g] : 0.f;
  mlp_chain(R, b, lane, m);
}

// both tiles of a forward pass: layer 1's W1 operand blocks loaded once for
// the two tiles' products (the same six products per tile as mlp_chain, the
// same sums)
__device__ __forceinline__ void mlp_pre2(const WRes& R, const float* __restrict__ emb, int e0, int e1,
                                         bool two, int lane, f32x4 (&a2)[2][4]) {
  const int g = lane >> 4, c = lane & 15;
  Op3 hq[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = e0 + 16 * u + c;
    float b[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) b[s] = (e < e1 && (u == 0 || two)) ? emb[(int64_t)e * 8 + 4 * s + g] : 0.f;
    f32x4 a1[4];
    mlp_layer0(R, b, lane, a1);
    f32x4 h1[4];
#pragma unroll
    for (int bh = 0; bh < 4; ++bh)
#pragma unroll
      for (int r = 0; r < 4; ++r) h1[bh][r] = act_fwd(a1[bh][r]);
    split_h2(h1, hq[u]);
  }
#pragma unroll
  for (int bo = 0; bo < 4; ++bo) {
    phase();
    Op3 wq;
    load_w2b(wq, R.w1b, lane, 16 * bo);
    a2[0][bo] = w2_block<false>(hq[0], wq);
    a2[1][bo] = two ? w2_block<false>(hq[1], wq) : zero4();
  }
}

// ---------------------------------------------------------------- TP pieces
// CG entries grouped by (i, j): each pair's partial sum over k is formed and
// consumed at once (short live ranges, one product per pair)
template <class C, int I, int J>
__device__ __forceinline__ constexpr bool cg_pair() {
  for (int q = 0; q < C::n; ++q)
    if (C::e[q].i == I && C::e[q].j == J) return true;
  return false;
}

// The lane's four edge slots r = 0..3 in lock-step (the dependency chains of
// the contraction run four-wide).  Forward:
//   acc[k] += sum_ij C_ijk s_ij,  s_ij = sum_r w[r] x[r][i] y[r][j]
// (4 per (i, j) pair + 1 per CG entry; forming sum_ij C_ijk x y per slot first
// and weighting at the end costs 4 per CG entry); y[r] = the slot's SH block
// (stride ys between slots).
template <int L1, int L2, int L3>
__device__ __forceinline__ void tp_acc4(const float* x, const float* y, int ys, const f32x4 w,
                                        float* acc) {
  using C = CG<L1, L2, L3>;
  constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1;
  float yv[4][D2];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < D2; ++q) yv[r][q] = y[r * ys + q];
  sfor<D1>([&](auto i) {
    float wx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wx[r] = w[r] * x[r * D1 + i];
    sfor<D2>([&](auto j) {
      if constexpr (cg_pair<C, i, j>()) {
        float sv = wx[0] * yv[0][j];
#pragma unroll
        for (int r = 1; r < 4; ++r) sv += wx[r] * yv[r][j];
        sfor<C::n>([&](auto q) {
          if constexpr (C::e[q].i == i && C::e[q].j == j) acc[C::e[q].k] += C::e[q].c * sv;
        });
      }
    });
  });
}

// Backward, the lane's 4 channels r of one edge:
//   u_ri = sum_jk C_ijk y_j g[r][k],  dx[r][i] += w[r] u_ri,  dw[r] = sum_i x[r][i] u_ri,
//   dy_j += sum_ik C_ijk sum_r w[r] x[r][i] g[r][k]
// Two contraction orders, chosen per path at compile time by VALU count:
//  * by (i, j): t'_rij = sum_k C_ijk g[r][k] (4 per CG entry: g is per channel),
//    u_ri += t'_rij y_j, dy_j += sum_r t'_rij w[r] x[r][i] (4 + 4 per (i, j) pair);
//  * by (i, k): ytilde_ik = sum_j C_ijk y_j (1 per CG entry: y is per edge, the
//    same for the lane's 4 channels), u_ri += ytilde_ik g[r][k] and
//    m_ik = sum_r w[r] x[r][i] g[r][k] (4 + 4 per (i, k) pair), dy_j += C_ijk m_ik
//    (1 per CG entry).  For the paths with many CG entries per output (l >= 1
//    on all three legs) this is ~25 % fewer VALU instructions.
template <class C, int I, int K>
__device__ __forceinline__ constexpr bool cg_ik() {
  for (int q = 0; q < C::n; ++q)
    if (C::e[q].i == I && C::e[q].k == K) return true;
  return false;
}
template <class C>
constexpr int cg_count_pairs(bool by_ik) {
  int n = 0;
  for (int q = 0; q < C::n; ++q) {
    bool first = true;
    for (int p = 0; p < q; ++p)
      if (C::e[p].i == C::e[q].i && (by_ik ? C::e[p].k == C::e[q].k : C::e[p].j == C::e[q].j)) first = false;
    n += first;
  }
  return n;
}
// CG entries that cost an instruction in the (i, j) order (a pair's only entry
// with coefficient 1 is a register alias)
template <class C>
constexpr int cg_cost_ij_entries() {
  int n = 0;
  for (int q = 0; q < C::n; ++q) {
    int cnt = 0;
    for (int p = 0; p < C::n; ++p) cnt += C::e[p].i == C::e[q].i && C::e[p].j == C::e[q].j;
    n += !(cnt == 1 && C::e[q].c == 1.0f);
  }
  return n;
}
template <int L1, int L2, int L3>
constexpr bool tp_bwd_by_ik() {
  using C = CG<L1, L2, L3>;
  const int P = cg_count_pairs<C>(false), Q = cg_count_pairs<C>(true);
  const int ij = 4 * (cg_cost_ij_entries<C>() + P) + (L2 > 0 ? 4 * P : 0);
  const int ik = C::n + 4 * Q + (L2 > 0 ? 4 * Q + C::n : 0);
  return ik < ij;
}

template <int L1, int L2, int L3>
__device__ __forceinline__ void tp_bwd_xw4(const float* x, const float* y, const f32x4 w,
                                           const float* gm, float* dx, float* dy, float* dw) {
  using C = CG<L1, L2, L3>;
  constexpr int D1 = 2 * L1 + 1, D2 = 2 * L2 + 1, D3 = 2 * L3 + 1;
#pragma unroll
  for (int r = 0; r < 4; ++r) dw[r] = -0.f;
  // ytilde depends on the edge only: without this opaque copy LLVM hoists
  // every path's ytilde out of the channel-group loop (74 live values for
  // l1 = 2: spills)
  float yl[D2];
  if constexpr (tp_bwd_by_ik<L1, L2, L3>()) {
#pragma unroll
    for (int q = 0; q < D2; ++q) yl[q] = y[q];
    pin<D2>(yl);
  }
  sfor<D1>([&](auto i) {
    float u[4] = {-0.f, -0.f, -0.f, -0.f}, wx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wx[r] = w[r] * x[r * D1 + i];
    if constexpr (tp_bwd_by_ik<L1, L2, L3>()) {
      sfor<D3>([&](auto k) {
        if constexpr (cg_ik<C, i, k>()) {
          float yt = -0.f;
          sfor<C::n>([&](auto q) {
            if constexpr (C::e[q].i == i && C::e[q].k == k) yt += C::e[q].c * yl[C::e[q].j];
          });
#pragma unroll
          for (int r = 0; r < 4; ++r) u[r] += yt * gm[r * D3 + k];
          if constexpr (L2 > 0) {
            float m = wx[0] * gm[k];
#pragma unroll
            for (int r = 1; r < 4; ++r) m += wx[r] * gm[r * D3 + k];
            sfor<C::n>([&](auto q) {
              if constexpr (C::e[q].i == i && C::e[q].k == k) dy[C::e[q].j] += C::e[q].c * m;
            });
          }
        }
      });
    } else {
      sfor<D2>([&](auto j) {
        if constexpr (cg_pair<C, i, j>()) {
          float tp[4] = {-0.f, -0.f, -0.f, -0.f};
          sfor<C::n>([&](auto q) {
            if constexpr (C::e[q].i == i && C::e[q].j == j) {
#pragma unroll
              for (int r = 0; r < 4; ++r) tp[r] += C::e[q].c * gm[r * D3 + C::e[q].k];
            }
          });
#pragma unroll
          for (int r = 0; r < 4; ++r) u[r] += tp[r] * y[j];
          if constexpr (L2 > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dy[j] += tp[r] * wx[r];
          }
        }
      });
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dx[r * D1 + i] += w[r] * u[r];
      dw[r] += x[r * D1 + i] * u[r];
    }
  });
}

template <class L, int I>
constexpr int iblock_mul() {
  for (int p = 0; p < L::NP; ++p)
    if (L::P[p].l1 == I) return L::P[p].mul;
  return 0;
}
template <class L, int I>
constexpr int iblock_xoff() {
  for (int p = 0; p < L::NP; ++p)
    if (L::P[p].l1 == I) return L::P[p].xoff;
  return 0;
}

// ---- block sequence (input irrep I, channel block jj, path) and operand prefetch
template <class L>
constexpr int first_path_of(int I) {
  for (int p = 0; p < L::NP; ++p)
    if (L::P[p].l1 == I) return p;
  return -1;
}
template <class L>
constexpr int next_path_same_I(int pi) {
  for (int p = pi + 1; p < L::NP; ++p)
    if (L::P[p].l1 == L::P[pi].l1) return p;
  return -1;
}
template <class L>
constexpr int first_path_after_I(int I) {
  for (int i = I + 1; i < 3; ++i)
    if (first_path_of<L>(i) >= 0) return first_path_of<L>(i);
  return -1;
}
// weight column of the block after (I, jj, PI); -1 at the end of the tile
template <class L, int I, int PI>
__device__ __forceinline__ int next_block_col(int jj) {
  constexpr int np = next_path_same_I<L>(PI);
  if constexpr (np >= 0) {
    return L::P[np].woff + 16 * jj;
  } else {
    constexpr int f = first_path_of<L>(I);
    constexpr int fn = first_path_after_I<L>(I);
    if (jj + 1 < L::P[f].mul / 16) return L::P[f].woff + 16 * (jj + 1);
    return fn >= 0 ? L::P[fn].woff : -1;
  }
}
// channel groups (input irrep I, 16-channel block j) in visiting order
template <class L>
constexpr int mul_of(int I) {
  for (int p = 0; p < L::NP; ++p)
    if (L::P[p].l1 == I) return L::P[p].mul;
  return 0;
}
template <class L>
constexpr int next_I(int I) {
  for (int i = I + 1; i < 3; ++i)
    if (mul_of<L>(i) > 0) return i;
  return -1;
}
template <class L>
constexpr int first_I() { return mul_of<L>(0) > 0 ? 0 : next_I<L>(0); }
// paths of input irrep I; rank of path pi among them; blocks visited before I
template <class L>
constexpr int paths_of(int I) {
  int n = 0;
  for (int p = 0; p < L::NP; ++p) n += L::P[p].l1 == I;
  return n;
}
template <class L>
constexpr int path_rank(int pi) {
  int n = 0;
  for (int p = 0; p < pi; ++p) n += L::P[p].l1 == L::P[pi].l1;
  return n;
}
template <class L>
constexpr int blocks_before(int I) {
  int n = 0;
  for (int i = 0; i < I; ++i) n += paths_of<L>(i) * mul_of<L>(i) / 16;
  return n;
}

// per tile: neighbour ids of the lane group's 4 edges, Y of the 16 edges in LDS
__device__ __forceinline__ void load_tile_edges(const int* __restrict__ nbr,
                                                const float* __restrict__ Y, int e0, int end,
                                                int lane, int (&src)[4], float* ybuf) {
  const int g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = e0 + 4 * g + r;
    src[r] = e < end ? nbr[e] : 0;
  }
#pragma unroll
  for (int q0 = 0; q0 < 144; q0 += 64) {
    const int q = q0 + lane;
    if (q < 144) ybuf[q] = (e0 + q / 9 < end) ? Y[(int64_t)e0 * 9 + q] : 0.f;
  }
}

// ---------------------------------------------------------------- forward
// agg[c] = sum_e TP(h[nbr e], Y_e, w_e) / denom.
// Two 16-edge tiles of the centre per pass: every W2 operand block
// (6 KB per lane set, from L2) feeds both tiles' w = H2 W2 products, halving
// the operand stream that dominates the one-tile kernel, and the two tiles'
// messages are summed in registers before the LDS accumulation.
// waves per SIMD the register allocation targets (unified VGPR+AGPR file:
// 3 waves <= 168 registers, 2 <= 256; without the hint the compiler parks
// MFMA accumulators in AGPRs and lands just above a boundary): the first
// block (128 input channels) fits three, the others two
// row sums over the four lane groups as groups of permlane swaps (the
// forward's D3 values per path, the lock-step backward's 8 dE/dY values per
// edge) instead of one hazard-padded pair of swaps per value: middle forward
// 9.21 -> 9.01-9.11 ms for the three launches, same box (profiles/r06_s20_*);
// in the last block's backward it measured neutral to slower and stays per
// value
// the forward's row sums are a reduce-scatter (sum_rows4_scatter): a path's D3
// totals end up one per lane group, 3 swaps + 3 adds per four values instead of
// 8 + 8 + 8 copies, and every group stores its own: middle forward 2.98 -> 2.83
// ms per launch, first 1.04 -> 1.02, same bits (profiles/rowsum_*)
// the middle and last blocks' two tiles go through the radial MLP together,
// each W1 operand block loaded once for both (same products, same bits):
// last-block forward 1.05-1.06 -> 1.00-1.01 ms, middle 9.13 -> 9.02 ms
// averaged over two runs each (noisy box; profiles/r06_s23_*)
template <class L>
struct Fwd2Waves {
  static constexpr int v = L::KIND == 0 ? 3 : 2;
};
template <class L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Fwd2Waves<L>::v, Fwd2Waves<L>::v))) void k_conv_fwd(
    const int* __restrict__ row_ptr, const int* __restrict__ nbr, const float* __restrict__ emb,
    const float* __restrict__ Y, const float* __restrict__ h, float* __restrict__ agg, MlpW W, int c_begin,
    int c_end, int n_nodes, float denom) {
  __shared__ float lds[4][2][160];
  __shared__ __attribute__((aligned(16))) float aggl[4][L::DM];
  const int wid = threadIdx.x >> 6;
  const int c = __builtin_amdgcn_readfirstlane(c_begin + blockIdx.x * 4 + wid);
  if (c >= c_end) return;
  float* acl = aggl[wid];
  const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
  const int beg = row_ptr[c], end = row_ptr[c + 1];
  float* out = agg + (int64_t)c * L::DM;
  const WRes R = make_wres(W, L::W);
  const __amdgpu_buffer_rsrc_t Rh = rsrc_bytes(h, (int64_t)n_nodes * L::DX * 4);
  const float rden = 1.0f / denom;
  constexpr bool STAMPED = std::is_same<L, LayerMid>::value && E3GNN_STAMPS_FWD;
  STAMP_DECL
  for (int e0 = beg; e0 < end || e0 == beg; e0 += 32) {
    if constexpr (STAMPED) STAMP(0);
    const bool first_tile = e0 == beg;
    const bool two = e0 + 16 < end;   // wave-uniform: the second tile has edges
    int src[2][4];
    Op3 wq;
    load_w2b(wq, R.w2b, lane, L::P[0].woff);
#pragma unroll
    for (int u = 0; u < 2; ++u) load_tile_edges(nbr, Y, e0 + 16 * u, end, lane, src[u], lds[wid][u]);
    // tile 0's neighbour rows of the next channel group are prefetched under
    // the current group; tile 1's are loaded at the group start (consumed
    // after tile 0's first product: their latency hides there)
    float xpf[20];
    auto load_rows = [&](auto Iq, int jq, int u, float* dst) {
      constexpr int D1q = 2 * Iq + 1;
      constexpr int XOq = iblock_xoff<L, Iq>();
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ldv<D1q>(Rh, (src[u][r] * L::DX + col * D1q) * 4, (XOq + 16 * jq * D1q) * 4, dst + r * D1q);
    };
    auto load_group = [&](auto Iq, int jq) { load_rows(Iq, jq, 0, xpf); };
    load_group(std::integral_constant<int, first_I<L>()>{}, 0);
    Op3 hq[2];
    if constexpr (L::KIND != 0) {   // (the first block: three waves, no room)
      f32x4 a2[2][4];
      mlp_pre2(R, emb, e0, end, two, lane, a2);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && !two) break;
        f32x4 h2[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) h2[b][r] = act_fwd(a2[u][b][r]);
        split_h2(h2, hq[u]);
      }
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && !two) break;
        MlpT m;
        mlp_pre(R, emb, e0 + 16 * u, end, lane, m);
        f32x4 h2[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) h2[b][r] = act_fwd(m.a2[b][r]);
        split_h2(h2, hq[u]);
      }
    }
    if constexpr (STAMPED) STAMP(1);   // edge loads, MLP chain, H2 split
    sfor<3>([&](auto I) {
      constexpr int MUL = iblock_mul<L, I>();
      if constexpr (MUL > 0) {
        constexpr int D1 = 2 * I + 1;
        for (int j = 0; j < MUL / 16; ++j) {
          float x[2][4 * D1];
          phase();
#pragma unroll
          for (int i = 0; i < 4 * D1; ++i) x[0][i] = xpf[i];
          load_rows(I, j, 1, x[1]);
          if (j + 1 < MUL / 16) {
            load_group(I, j + 1);
          } else {
            constexpr int IN = next_I<L>(I);
            if constexpr (IN >= 0) load_group(std::integral_constant<int, IN>{}, 0);
          }
          sfor<L::NP>([&](auto pi) {
            constexpr PathDef p = L::P[pi];
            if constexpr (p.l1 == I) {
              constexpr int D3 = 2 * p.l3 + 1;
              phase();
              if constexpr (STAMPED) STAMP(4);   // (group start: row copies / loads)
              const f32x4 wv0 = w2_block<true>(hq[0], wq);
              const f32x4 wv1 = two ? w2_block<true>(hq[1], wq) : zero4();
              {  // operands of the next block load under this block's tensor product
                const int nc = next_block_col<L, I, pi>(j);
                if (nc >= 0) load_w2b(wq, R.w2b, lane, nc);
              }
              phase();
              if constexpr (STAMPED) STAMP(2);   // w MFMAs
              float acc[D3];
#pragma unroll
              for (int k = 0; k < D3; ++k) acc[k] = -0.f;
              // the lane's 4 edges of each tile (padded edges have Y = 0)
              tp_acc4<p.l1, p.l2, p.l3>(x[0], lds[wid][0] + 4 * g * 9 + yoff(p.l2), 9, wv0, acc);
              if (two) tp_acc4<p.l1, p.l2, p.l3>(x[1], lds[wid][1] + 4 * g * 9 + yoff(p.l2), 9, wv1, acc);
              if constexpr (STAMPED) STAMP(3);   // tensor product
              // reduce-scatter over the lane groups: group g ends up with the
              // total of component k = g and stores it, all groups at once.
              // Groups left with a second copy of a total (D3 = 3: group 3
              // holds component 1; D3 = 1 and component 4 of D3 = 5: every
              // group) store it too -- the same bits to the same address --
              // so no store needs a lane mask (masking the copies measured
              // the same: 2.79 ms per middle launch either way)
              float tot[(D3 + 3) / 4];
              sum_rows4_scatter<D3>(acc, tot);
              float* a0 = acl + p.moff + (16 * j + col) * D3;
              {
                const float v = tot[0] * rden;
                float* a = a0 + (D3 == 1 ? 0 : D3 == 3 && g == 3 ? 1 : g);
                *a = first_tile ? v : *a + v;
              }
              if constexpr (D3 == 5) {
                const float v = tot[1] * rden;
                a0[4] = first_tile ? v : a0[4] + v;
              }
              if constexpr (STAMPED) STAMP(5);   // row sums + LDS accumulation
            }
          });
        }
      }
    });
    if (end <= beg) break;
  }
  phase();
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  {
    const float4* src = reinterpret_cast<const float4*>(acl);
    float4* dst = reinterpret_cast<float4*>(out);
    for (int t = lane; t < L::DM / 4; t += 64) dst[t] = src[t];
  }
  if constexpr (STAMPED) {
    STAMP(6);   // copy-out
    STAMP_FLUSH(c - c_begin);
  }
}

// ---------------------------------------------------------------- backward
// tp_bwd_x and dE/dw of the same (edge, channel) in one pass: with
// t'_ij = sum_k C_ijk g_k and u_i = sum_j t'_ij y_j,
//   dE/dx_i += w u_i,  dE/dy_j += t'_ij (w x_i),  dE/dw = sum_i x_i u_i
// (no x_i y_j products: those are shared by the paths of an (l1, l2) pair, and
// the compiler kept them live across paths; the fused backward, MODE 3)
template <int L1, int L2, int L3>
__device__ __forceinline__ float tp_bwd_xw(const float* x, const float* y, float w, const float* gm,
                                           float* dx, float* dy) {
  using C = CG<L1, L2, L3>;
  float dwv = -0.f;
  sfor<2 * L1 + 1>([&](auto i) {
    float ui = -0.f;
    const float wx = w * x[i];
    sfor<2 * L2 + 1>([&](auto j) {
      if constexpr (cg_pair<C, i, j>()) {
        float tp = -0.f;
        sfor<C::n>([&](auto q) {
          if constexpr (C::e[q].i == i && C::e[q].j == j) tp += C::e[q].c * gm[C::e[q].k];
        });
        ui += tp * y[j];
        dy[j] += tp * wx;
      }
    });
    dx[i] += w * ui;
    dwv += x[i] * ui;
  });
  return dwv;
}

// dE/dagg operands of path PN at channel block jj for the lane's edge (4 * D3
// floats at the edge centre's row, channels 4g..4g+3)
template <class L, int PN>
__device__ __forceinline__ void load_gm(float* gmN, __amdgpu_buffer_rsrc_t Rg, int vg, int g, int jj) {
  constexpr int D3 = 2 * L::P[PN].l3 + 1;
  ldv<4 * D3>(Rg, vg + 4 * g * D3 * 4, (L::P[PN].moff + 16 * jj * D3) * 4, gmN);
}

// Backward of the last block (224 message channels), one wave per NEIGHBOUR
// node j over its incoming edges (transposed CSR src_ptr / src_perm, ascending
// edge id, tiles of 16): lane (g, c) = edge slot c x channels 4g..4g+3 of a
// 16-channel block (transposed product w^T = W2^T H2^T: D[channel 4g+r][edge
// c]); x = h[j] (one row), the edges' centres' dE/dagg gathered per block
// (DM = 224 floats a row).  dE/dx[j] is summed over the tile's 16 edge lanes
// (DPP) once per block, accumulated in LDS and written once (no per-edge
// buffer, no gather pass); per edge: dE/dY -> dE/du, and dE/dw . w' summed
// over the blocks -> dE/dr |radial (drad; w' = W2^T H2'^T, mlp_chain_jvp).
// Every edge is visited once (by its neighbour's wave): deterministic.  The
// radial weights w and tangents w' of the NEXT visited block are formed (MFMA,
// on the one W2 operand block) before this block's tensor product (VALU).
// Two 16-edge tiles of the node per pass (28 incoming edges on average: one
// pass per node): every W2 operand block feeds both tiles, and dE/dx[j] of
// both tiles is summed in registers before the per-block DPP row sum.  The
// second tile is skipped when it has no edge.
// the pass end's read-modify-writes of dE/du and drad: the old values read at
// the pass start (for dE/du and the former dE/demb 2.13 -> 2.09-2.12 ms, same
// box; profiles/r06_s12_*)
template <class L>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_conv_bwd_nbr(
    const int* __restrict__ src_ptr, const int* __restrict__ src_perm, const int* __restrict__ center,
    const float* __restrict__ emb, const float* __restrict__ Y, const float* __restrict__ h,
    const float* __restrict__ gagg, MlpW W, float* __restrict__ dh, float* __restrict__ dgu, int n_centers,
    int r_begin, int r_end, const float* __restrict__ embd, float* __restrict__ drad) {
  __shared__ __attribute__((aligned(16))) float lds[4][L::DX];
  const int wid = threadIdx.x >> 6;
  const int jn = __builtin_amdgcn_readfirstlane(r_begin + blockIdx.x * 4 + wid);
  if (jn >= r_end) return;
  float* dacc = lds[wid];
  const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
  const int qb = src_ptr[jn], qe = src_ptr[jn + 1];
  const WRes R = make_wres(W, L::W);
  const __amdgpu_buffer_rsrc_t Rx = rsrc_bytes(h + (int64_t)jn * L::DX, L::DX * 4);
  const __amdgpu_buffer_rsrc_t Rg = rsrc_bytes(gagg, (int64_t)n_centers * L::DM * 4);
  for (int t = lane; t < L::DX; t += 64) dacc[t] = 0.f;
  const RowSel rsel = row_scatter_sel(col);
  const int own = row_scatter_own(col);

  for (int q0 = qb; q0 < qe; q0 += 32) {
    const bool two = q0 + 16 < qe;   // wave-uniform
    phase();
    Op3 wq;
    load_w2b(wq, R.w2b, lane, L::P[0].woff);
    int er[2], vg[2];
    float y[2][9];
    // the pass end's dE/du and drad old values, read here
    float gu_old[2][3], dr_old[2];
    Op3 hq[2], hdq[2];   // H2 and its tangent H2'
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int q = q0 + 16 * u + col;
      er[u] = q < qe ? src_perm[q] : -1;   // edge of slot c
      vg[u] = (er[u] >= 0 ? center[er[u]] * L::DM : n_centers * L::DM) * 4;
#pragma unroll
      for (int k = 0; k < 9; ++k) y[u][k] = er[u] >= 0 ? Y[(int64_t)er[u] * 9 + k] : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) gu_old[u][k] = (g == 0 && er[u] >= 0) ? dgu[(int64_t)er[u] * 3 + k] : 0.f;
      dr_old[u] = (g == 0 && er[u] >= 0) ? drad[er[u]] : 0.f;
      if (u == 1 && !two) continue;
      float b[2], bd[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        b[k] = er[u] >= 0 ? emb[(int64_t)er[u] * 8 + 4 * k + g] : 0.f;
        bd[k] = er[u] >= 0 ? embd[(int64_t)er[u] * 8 + 4 * k + g] : 0.f;
      }
      mlp_chain_jvp(R, b, bd, lane, hq[u], hdq[u]);
    }
    float drl[2] = {0.f, 0.f};   // the lane's share of dE/dw . w' (edge c, channels 4g .. 4g+3 of every block)
    int nb = 0;
    constexpr int NBLK = L::W / 16;
    f32x4 wcur[2], wnxt[2] = {zero4(), zero4()};
    f32x4 tcur[2], tnxt[2] = {zero4(), zero4()};   // w' of the same blocks
    wcur[0] = w2_block_bwd<false>(hq[0], wq);
    tcur[0] = w2_block_tan<false>(hdq[0], wq);
    wcur[1] = two ? w2_block_bwd<false>(hq[1], wq) : zero4();
    tcur[1] = two ? w2_block_tan<false>(hdq[1], wq) : zero4();
    if (NBLK > 1) load_w2b(wq, R.w2v, lane, 16);
    float dYa[2][9];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int k = 0; k < 9; ++k) dYa[u][k] = 0.f;

    sfor<3>([&](auto I) {
      constexpr int MUL = iblock_mul<L, I>();
      if constexpr (MUL > 0) {
        constexpr int D1 = 2 * I + 1;
        constexpr int XOFF = iblock_xoff<L, I>();
        for (int jj = 0; jj < MUL / 16; ++jj) {
          float x[4 * D1], dx[4 * D1];
          phase();
          ldv<4 * D1>(Rx, 4 * g * D1 * 4, (XOFF + 16 * jj * D1) * 4, x);
#pragma unroll
          for (int i = 0; i < 4 * D1; ++i) dx[i] = -0.f;
          sfor<L::NP>([&](auto pi) {
            constexpr PathDef p = L::P[pi];
            if constexpr (p.l1 == I) {
              constexpr int D3 = 2 * p.l3 + 1;
              phase();
              float gm[2][4 * D3];
              load_gm<L, pi>(gm[0], Rg, vg[0], g, jj);
              load_gm<L, pi>(gm[1], Rg, vg[1], g, jj);
              f32x4 wv[2] = {wcur[0], wcur[1]}, tv[2] = {tcur[0], tcur[1]};
              if (nb + 1 < NBLK) {
                wnxt[0] = w2_block_bwd<false>(hq[0], wq);
                tnxt[0] = w2_block_tan<false>(hdq[0], wq);
                wnxt[1] = two ? w2_block_bwd<false>(hq[1], wq) : zero4();
                tnxt[1] = two ? w2_block_tan<false>(hdq[1], wq) : zero4();
              }
              if (nb + 2 < NBLK) load_w2b(wq, R.w2v, lane, 16 * (nb + 2));
#pragma unroll
              for (int u = 0; u < 2; ++u) {
                if (u == 1 && !two) break;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  phase();
                  float dy[2 * p.l2 + 1];
#pragma unroll
                  for (int q = 0; q < 2 * p.l2 + 1; ++q) dy[q] = 0.f;
                  // padded slots: w = 0, g = 0 and y = 0 (so dE/dw = 0)
                  const float dwr = tp_bwd_xw<p.l1, p.l2, p.l3>(x + r * D1, y[u] + yoff(p.l2), wv[u][r],
                                                                gm[u] + r * D3, dx + r * D1, dy);
                  drl[u] += dwr * tv[u][r];   // dE/dw . dw/dr
                  if constexpr (p.l2 > 0) {
#pragma unroll
                    for (int q = 0; q < 2 * p.l2 + 1; ++q) dYa[u][yoff(p.l2) + q] += dy[q];
                  }
                  pin<D1>(dx + r * D1);
                  pin<8>(dYa[u] + 1);
                }
              }
              pin<4 * D1>(dx);
              wcur[0] = wnxt[0];
              wcur[1] = wnxt[1];
              tcur[0] = tnxt[0];
              tcur[1] = tnxt[1];
              ++nb;
            }
          });
          phase();
          // both tiles' edges summed per lane already: the lane's 4 * D1
          // values (4, 12 or 20) summed over the 16 edge lanes as a
          // reduce-scatter in batches of 16 / 8 / 4 (row_sum16's pairs, the
          // same bits), every lane accumulating the value it ends up owning
          // (the lanes sharing a value of a short batch read, add and write
          // the same bits); as all-reduces with lane c == 0 accumulating,
          // this kernel ran 1.93 ms, so 1.80 (profiles/rowsum_kernel_stats_*)
          {
            constexpr int NV = 4 * D1;
            static_assert(NV % 8 == 4, "batches of 16, 8, then 4");
            float* da = dacc + XOFF + (16 * jj + 4 * g) * D1;
            if constexpr (NV >= 16) da[own] += row_scatter16<16>(dx, rsel);
            if constexpr (NV % 16 >= 8) da[NV / 16 * 16 + (own & 7)] += row_scatter16<8>(dx + NV / 16 * 16, rsel);
            da[NV / 8 * 8 + (own & 3)] += row_scatter16<4>(dx + NV / 8 * 8, rsel);
          }
        }
      }
    });

#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
      phase();
      // dE/dY of edge c: sum over the 4 lane groups, then dE/du through the SH
      // polynomials (serial_code.py:50-70)
      float d[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) d[q] = sum_rows4(dYa[u][q + 1]);
      if (g == 0 && er[u] >= 0) {
        const float s3 = 1.7320508075688772f, s5 = 2.23606797749979f, c15 = s3 * s5;
        const float is3 = 0.57735026918962576f;  // 1 / sqrt(3)
        const float ux = y[u][1] * is3, uy = y[u][2] * is3, uz = y[u][3] * is3;
        const float gx = s3 * d[0] + c15 * (uz * d[3] + uy * d[4]) - s5 * ux * d[5] - c15 * ux * d[7];
        const float gy = s3 * d[1] + c15 * (ux * d[4] + uz * d[6]) + 2.f * s5 * uy * d[5];
        const float gz = s3 * d[2] + c15 * (ux * d[3] + uy * d[6]) - s5 * uz * d[5] + c15 * uz * d[7];
        float* o = dgu + (int64_t)er[u] * 3;
        o[0] = gu_old[u][0] + gx;
        o[1] = gu_old[u][1] + gy;
        o[2] = gu_old[u][2] + gz;
      }
      // dE/dr |radial of edge c: the same sum over the 4 lane groups
      const float dr = sum_rows4(drl[u]);
      if (g == 0 && er[u] >= 0) drad[er[u]] = dr_old[u] + dr;
    }
  }
  phase();
  __builtin_amdgcn_s_waitcnt(0);
  float* dhj = dh + (int64_t)jn * L::DX;
  for (int t = lane; t < L::DX; t += 64) dhj[t] = dacc[t];
}

// ================================================================ lock-step kernels
// One workgroup = 4 waves over a contiguous range of the launch's CSR edges,
// walked in ROUNDS of four consecutive 16-edge tiles (one per wave, in
// lock-step).  Every output is per edge and no sum crosses edges, so a tile
// need not belong to one centre: it takes its lanes' centres from center[] and
// their dE/dagg rows from a window of four LDS slots (centre c in slot c & 3),
// and a round spans at most four consecutive centres (its edges end at
// row_ptr[cf + 4], cf the centre of its first edge: low-degree graphs).  No
// slot of a tile is padding except at a round's clipped end.
// The waves walk the same sequence of 16-column weight blocks and share the
// W2 operands of each block PAIR: staged once per workgroup in LDS (register
// staging: issued a whole pair ahead, written between two barriers), so each
// operand crosses the L2 -> CU path once per 4 tiles instead of once per tile
// and needs no per-wave prefetch registers.  Middle blocks: two workgroups per
// CU (LDS), 2 waves per SIMD (SevenNet-0's: two pairs per barrier, LsQuads); the
// first block: 3 waves per SIMD.

// The pair's W2 pieces are staged as the [hidden][channel] image of
// w2_image.h (MlpW::w2s) and read transposed (ds_read_b64_tr_b16): the operand
// registers of the w recompute w^T = W2^T H2^T, which the tangent product
// w'^T = W2^T H2'^T shares (the image's row reads were the operand of the
// reverse-mode dH2 = dw W2^T that the tangent replaced).  The image holds only
// the pieces the two products read: with the three-product forms
// (E3GNN_BWD_W_X3, E3GNN_DH2_X3) pieces 0 and 1, 8 KB per pair (12 KB when
// either product runs on six)
constexpr int LS_WPC = E3GNN_BWD_W_X3 ? 2 : 3;   // pieces the w recompute reads
constexpr int LS_DPC = E3GNN_DH2_X3 ? 2 : 3;     // pieces the tangent product reads
constexpr int LS_PCS = LS_WPC > LS_DPC ? LS_WPC : LS_DPC;   // staged, and read into the shared operand
constexpr int LS_IMG = LS_PCS * w2img::PIECE_BYTES;

// the operand of the pair's block b (transposed reads: every lane of the wave
// active)
template <int NPC = 3>
__device__ __forceinline__ void lds_op3(Op3& o, const char* pimg, int b, int lane) {
#pragma unroll
  for (int pc = 0; pc < NPC; ++pc)
#pragma unroll
    for (int m = 0; m < 2; ++m) o.v[pc][m] = w2img::tr_read(pimg, lane, b, pc, m);
}

// full rounds (64 edges) of a workgroup's edge range: a range re-stages the
// row of the centre it starts in and pays one staging latency at its start.
// 8, 4 and 2 measured the same step time on the Si benchmark box (5.3k, 10.6k
// and 21.3k workgroups over 512 resident slots)
constexpr int LS_ROUNDS = 8;
// floats between two centres' staged dE/dagg rows: the row, skewed so that the
// stride is 64 B modulo the 256 B of the LDS banks.  A tile that spans centres
// reads the same row offset in up to four slots at once; with the slots 16
// banks apart, the 16-byte windows of (slot s, lane group g) and (s', g') are
// disjoint for D3 = 1, 3, 5 (4 (s - s') + D3 (g - g') is never 0 modulo 16 for
// |s - s'|, |g - g'| <= 3 unless both are 0).  Unskewed, SevenNet-0's middle row
// (12,032 B = 47 x 256) puts every slot on the same banks.
constexpr int ls_row_stride(int dms) { return dms + ((64 - dms * 4 % 256 + 256) % 256) / 4; }

// Backward of a first / middle block (per-edge dE/dx to dxc, summed per
// neighbour by the transposed-CSR gather; dE/dY -> dE/du; dE/dw . w' summed
// over the blocks -> dE/dr |radial, drad), each centre's dE/dagg row staged in
// LDS once per workgroup range (the four-slot window above).  Same pair
// structure as the forward (both blocks' w and tangents w' formed at the pair
// start from the same operand registers, next group's neighbour rows
// prefetched).
// waves per SIMD: the first block (128 input channels, 1,152 message channels:
// 34.8 KB of LDS per workgroup, two images) runs three (168 VGPRs with a few
// spills measured 2.57 -> 2.27 ms against two), the middle blocks two (their
// 241-254 VGPRs allow no more; 64.8 KB of LDS per workgroup, 81.2 KB with
// two pairs per barrier, LsQuads below)
template <class L>
struct BwdLsWaves {
  static constexpr int v = L::KIND == 0 ? 3 : 2;
};
// tiles (waves) per round and workgroup (one 8-wave workgroup per CU sharing each
// staged W2 pair, 124 KB of LDS, measured slower for the middle block)
constexpr int LS_WPG = 4;
// Double-buffered staging where two images fit (the middle blocks: backward
// 5.66 -> 5.53 ms per launch against one image, same box): the pair's pieces
// are loaded into registers a pair ahead (loads the compiler counts, so its
// waits leave the neighbour-row prefetch and the dE/dx stores in flight) and
// written into one of TWO images before the pair's ONE barrier -- the other
// image is the one the previous pair read, retired by the previous pair's
// barrier.  The two images are 2 x 8 KB (2 x 12 KB in the six-product
// builds); in the middle blocks the 0e x 0e -> 0e path's dE/dagg (C0 floats,
// moff 0) is read from L2 with the neighbour-row prefetch instead of staged (a
// choice made when the pair was staged as two 16 KB images and two workgroups
// would not otherwise fit a CU, as again with LsQuads' four images; staging
// the slice again measured no gain without them: DESIGN.md 8 item 1).  Where
// two images do not fit: one image, written between two barriers per pair.  Writing the images by LDS-DMA straight from L2 was
// measured and rejected (5.68 -> 5.77 ms: its explicit wait before the barrier
// drains every load and store in flight).
template <class L>
struct LsTwoImages {
  static constexpr int OFF0 = L::KIND == 1 ? L::P[0].mul : 0;   // path 0 (l 0 0 0, moff 0): C0 floats
  static constexpr int DMS = L::DM - OFF0;                       // staged dE/dagg floats per centre
  static constexpr int bytes = LS_WPG * ls_row_stride(DMS) * 4 + 2 * LS_IMG;
  static constexpr bool v = BwdLsWaves<L>::v * bytes <= 163840;
};
// Two pairs per barrier: each of the two buffers holds the images of two
// consecutive pairs (a group of four blocks), written and published at the
// group's start, so a tile runs half the barriers.  It needs every block's
// position in its group of four to be a compile-time constant (the channel
// groups of an input irrep unrolled until their blocks are a multiple of four)
// and 4 images beside the staged rows at the kernel's workgroups per CU:
// SevenNet-0's middle block (81,152 B, two per CU); c64's rows are too long,
// c32's l1 = 0 groups too few.  Step 37.64-38.06 -> 37.23-37.37 ms, launch 5.12 ->
// 4.87 ms against one pair per barrier (profiles/quads_bench.log).  The same kernel at THREE waves
// per SIMD (the l1 = 0 paths' dE/dagg from L2, 50.4 KB of LDS, 168 VGPRs) was
// measured first and ran no faster than at two: DESIGN.md 8 item 1.
template <class L>
struct LsQuads {
  static constexpr int unroll(int npi) { return npi % 4 == 0 ? 1 : npi % 2 == 0 ? 2 : 4; }
  static constexpr bool pos_ok() {
    if (L::W / 16 % 4) return false;
    for (int i = 0; i < 3; ++i)
      if (mul_of<L>(i) > 0 && (mul_of<L>(i) / 16 % unroll(paths_of<L>(i)) || blocks_before<L>(i) % 4)) return false;
    return true;
  }
  static constexpr int bytes = LS_WPG * ls_row_stride(L::DM - LsTwoImages<L>::OFF0) * 4 + 4 * LS_IMG;
  static constexpr bool v = L::KIND == 1 && LsTwoImages<L>::v && pos_ok() && BwdLsWaves<L>::v * bytes <= 163840;
};
// wave priority, raised around the lock-step backward's MFMA bursts
template <int P>
__device__ __forceinline__ void ls_prio() { __builtin_amdgcn_s_setprio(P); }
template <class L>
__global__ __launch_bounds__(64 * LS_WPG) __attribute__((amdgpu_waves_per_eu(BwdLsWaves<L>::v, BwdLsWaves<L>::v))) void k_conv_bwd_ls(
    const int* __restrict__ row_ptr, const int* __restrict__ nbr, const float* __restrict__ emb,
    const float* __restrict__ Y, const float* __restrict__ h, const float* __restrict__ gagg, MlpW W,
    float* __restrict__ dxc, float* __restrict__ dgu, const float* __restrict__ embd, float* __restrict__ drad,
    const int* __restrict__ center, int e_begin, int e_end, int c_end, int n_nodes) {
  constexpr int NBLK = L::W / 16, NPAIR = NBLK / 2;
  static_assert(NBLK % 2 == 0, "weight blocks come in pairs");
  constexpr int WPG = LS_WPG, NT = 64 * WPG;
  // staging pieces (b128) of a pair's image per thread: a straight copy of
  // the first LS_IMG bytes of the pair in MlpW::w2s
  constexpr int NST = LS_IMG / 16 / NT;
  static_assert(LS_IMG / 16 % NT == 0, "staging pieces per thread");
  constexpr bool TWO = LsTwoImages<L>::v;   // two images, one barrier per pair
  constexpr bool QUAD = LsQuads<L>::v;      // two pairs per image and barrier
  constexpr int NIMG = QUAD ? 2 : 1;        // pairs staged at a time
  // tile-start values kept in registers to the tile end (the first block at
  // three waves per SIMD: no VGPRs to spare)
  constexpr bool KEEP = BwdLsWaves<L>::v == 2;
  constexpr int OFF0 = TWO ? LsTwoImages<L>::OFF0 : 0, DMS = L::DM - OFF0;   // dE/dagg floats staged per centre
  static_assert(!TWO || (L::P[0].l1 == 0 && L::P[0].l2 == 0 && L::P[0].l3 == 0 && L::P[0].moff == 0 &&
                         OFF0 % 4 == 0), "path 0 is the 0e x 0e -> 0e slice at the row start");
  constexpr int RS = ls_row_stride(DMS);   // floats between two slots of the row window
  __shared__ __attribute__((aligned(16))) float smem[WPG * RS + (TWO ? 2 : 1) * NIMG * LS_IMG / 4];
  const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, g = lane >> 4, col = lane & 15;
  // the workgroup's edges [ws, we) of the launch's [e_begin, e_end)
  const int ws = e_begin + blockIdx.x * (LS_ROUNDS * 16 * WPG);
  const int we = min(ws + LS_ROUNDS * 16 * WPG, e_end);
  char* img = reinterpret_cast<char*>(smem + WPG * RS);
  int rhi = 0;   // centres below rhi have been staged (resident while in the window)
  // two images: the one the current pair reads (0 / 1)
  int rb = 0;
  const WRes R = make_wres(W, L::W);
  const __amdgpu_buffer_rsrc_t Rs = rsrc_bytes(W.w2s, NPAIR * w2img::PAIR_BYTES);   // the pair images
  const __amdgpu_buffer_rsrc_t Rx = rsrc_bytes(h, (int64_t)n_nodes * L::DX * 4);
  f32x4 st[NIMG * NST];
  auto issue = [&](int P) {   // pairs P .. P + NIMG - 1
#pragma unroll
    for (int i = 0; i < NIMG * NST; ++i)
      st[i] = ldw4(Rs, (tid + NT * (i % NST)) * 16, (P + i / NST) * w2img::PAIR_BYTES);
  };
  // the single image: the previous pair's reads retired, the pair written, published
  auto commit = [&]() {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NST; ++i) *reinterpret_cast<f32x4*>(img + (tid + NT * i) * 16) = st[i];
    __syncthreads();
  };
  constexpr bool STAMPED = std::is_same<L, LayerMid>::value && !E3GNN_STAMPS_FWD;   // SevenNet-0's
  STAMP_DECL
  issue(0);
  for (int qr = ws; qr < we;) {
    if constexpr (STAMPED) STAMP(0);
    // the round: edges [qr, end) of the centres cf .. cl (at most cf + 3)
    const int cf = __builtin_amdgcn_readfirstlane(center[qr]);
    const int end = __builtin_amdgcn_readfirstlane(min(min(qr + 16 * WPG, we), row_ptr[min(cf + 4, c_end)]));
    const int cl = __builtin_amdgcn_readfirstlane(center[end - 1]);
    // rows of the window not yet resident: cs0 .. cl (at most four)
    const int cs0 = max(cf, rhi), nnew = cl - cs0 + 1;
    rhi = cl + 1;
    const int q0 = qr + 16 * wid;
    qr = end;
    const bool act = q0 < end;   // wave-uniform
    const int er = (act && q0 + col < end) ? q0 + col : -1;
    // the lane's centre: its dE/dagg row (dacc[m] for m >= OFF0) in slot
    // centre & 3; path 0's slice (two images) through a descriptor over the
    // round's rows, the lane's row relative to cf (absolute byte offsets pass
    // 32 bits on large boxes)
    const int dc = er >= 0 ? center[er] - cf : 0;
    const float* dacc = smem + ((cf + dc) & 3) * RS - OFF0;
    const __amdgpu_buffer_rsrc_t Rg0 = rsrc_bytes(
        gagg + (int64_t)cf * L::DM, OFF0 > 0 ? ((int64_t)(cl - cf) * L::DM + OFF0) * 4 : 0);
    const int vg0 = (dc * L::DM + 4 * g) * 4;
    const int vx = (er >= 0 ? nbr[er] : 0) * L::DX * 4;
    float xpf[20];   // the lane's 4 channels x D1 of the next channel group
    float g0pf[4];   // two images: path 0's dE/dagg of that group (l1 = 0 groups)
    auto load_group = [&](auto Iq, int jq) {
      constexpr int D1q = 2 * Iq + 1;
      constexpr int XOq = iblock_xoff<L, Iq>();
      ldv<4 * D1q>(Rx, vx + 4 * g * D1q * 4, (XOq + 16 * jq * D1q) * 4, xpf);
      if constexpr (OFF0 > 0 && Iq == 0) ldv<4>(Rg0, vg0, 16 * jq * 4, g0pf);
    };
    float y[9];
    // KEEP: old values of the tile end's read-modify-writes
    float gu_old[3] = {0.f, 0.f, 0.f}, dr_old = 0.f;
    Op3 hq, hdq;   // H2 and its tangent H2' (mlp_chain_jvp)
    // neighbour rows (lanes without an edge read row 0: harmless, their y
    // and w are 0); issued unconditionally, like every vector-memory op
    // between two pair commits, so the commit's wait counts only the staging
    // loads and leaves younger loads and stores in flight
    load_group(std::integral_constant<int, first_I<L>()>{}, 0);
    // per-edge dE/dx rows of this tile: lanes without an edge, inactive tiles
    // and the first block (dxc == nullptr) store outside the descriptor
    const int nrow = (act && dxc) ? min(16, end - q0) : 0;
    const __amdgpu_buffer_rsrc_t Rd =
        rsrc_bytes(dxc ? dxc + (int64_t)(act ? q0 : 0) * L::DX : gagg, (int64_t)nrow * L::DX * 4);
    const int vd = col * L::DX * 4;
    float b[2], bd[2];
    if (act) {
#pragma unroll
      for (int q = 0; q < 9; ++q) y[q] = er >= 0 ? Y[(int64_t)er * 9 + q] : 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        b[s] = er >= 0 ? emb[(int64_t)er * 8 + 4 * s + g] : 0.f;
        bd[s] = er >= 0 ? embd[(int64_t)er * 8 + 4 * s + g] : 0.f;
      }
      if constexpr (KEEP) {
        // the tile end's read-modify-writes (dE/du, drad of the lane's
        // edge): old values read here, their latency under the whole tile
        if (g == 0 && er >= 0) {
#pragma unroll
          for (int k = 0; k < 3; ++k) gu_old[k] = dgu[(int64_t)er * 3 + k];
          dr_old = drad[er];
        }
      }
    }
    // The window's new rows are copied with the tile's edge loads in flight
    // (one exposed latency for both), every row's pieces requested before the
    // first is written.  The barrier stands between every wave's last read of
    // the rows they replace (the last barrier of a round is at its last
    // group's start) and the writes; the round's first staging barrier
    // publishes them.
    {
      constexpr int NRK = (DMS / 4 + NT - 1) / NT;   // b128 pieces of a row per thread
      const __amdgpu_buffer_rsrc_t Rr = rsrc_bytes(
          gagg + (int64_t)cs0 * L::DM + OFF0, nnew > 0 ? ((int64_t)(nnew - 1) * L::DM + DMS) * 4 : 0);
      __syncthreads();
      f32x4 rowv[4 * NRK];
#pragma unroll
      for (int i = 0; i < 4 * NRK; ++i)
        rowv[i] = ldw4(Rr, ((i / NRK) * L::DM + (tid + NT * (i % NRK)) * 4) * 4, 0);
#pragma unroll
      for (int i = 0; i < 4 * NRK; ++i) {
        const int k = tid + NT * (i % NRK);
        if (i / NRK < nnew && k < DMS / 4)
          reinterpret_cast<f32x4*>(smem + ((cs0 + i / NRK) & 3) * RS)[k] = rowv[i];
      }
    }
    if (act) mlp_chain_jvp(R, b, bd, lane, hq, hdq);
    if constexpr (STAMPED) STAMP(1);   // tile setup: edge loads, MLP chain and tangent, H2 / H2' splits
    float drl = 0.f;   // the lane's share of dE/dw . w' (edge c, channels 4g .. 4g+3 of every block)
    float dYa[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) dYa[q] = 0.f;
    f32x4 wv0 = zero4(), wv1 = zero4();   // w of the pair's two blocks
    f32x4 tv0 = zero4(), tv1 = zero4();   // and their tangents w'
    sfor<3>([&](auto I) {
      constexpr int MUL = iblock_mul<L, I>();
      if constexpr (MUL > 0) {
        constexpr int D1 = 2 * I + 1;
        constexpr int XOFF = iblock_xoff<L, I>();
        // an odd number of paths: two channel groups per iteration, so the
        // position of every block in its pair (QUAD: in its group of four) is a
        // compile-time constant (no branches around the staging: the wait
        // counts stay exact)
        constexpr int NPI = paths_of<L>(I), NB0 = blocks_before<L>(I);
        constexpr int U = QUAD ? LsQuads<L>::unroll(NPI) : (NPI & 1) ? 2 : 1;
        static_assert((MUL / 16) % U == 0, "channel groups come in pairs");
        auto groups = [&](const int j2) {
          sfor<U>([&](auto hh) {
            const int jj = j2 + hh;
            float x[4 * D1], dx[4 * D1], g0[4];
#pragma unroll
            for (int i = 0; i < 4 * D1; ++i) {
              x[i] = xpf[i];
              dx[i] = 0.f;
            }
            if constexpr (OFF0 > 0 && I == 0) {
#pragma unroll
              for (int i = 0; i < 4; ++i) g0[i] = g0pf[i];
            }
            if (jj + 1 < MUL / 16) {
              load_group(I, jj + 1);
            } else {
              constexpr int IN = next_I<L>(I);
              if constexpr (IN >= 0) load_group(std::integral_constant<int, IN>{}, 0);
            }
            sfor<L::NP>([&](auto pi) {
              constexpr PathDef p = L::P[pi];
              if constexpr (p.l1 == I) {
                constexpr int D3 = 2 * p.l3 + 1;
                constexpr int POS = (NB0 + hh * NPI + path_rank<L>(pi)) & (2 * NIMG - 1), ODD = POS & 1;
                const int nb = NB0 + jj * NPI + path_rank<L>(pi);
                // this pair's image (QUAD: the first or second of its buffer)
                const char* pimg = img + (TWO ? rb * NIMG * LS_IMG : 0) + (POS >> 1) * LS_IMG;
                if constexpr (POS == 0) {   // pair (QUAD: two pairs) start: stage, fetch the next
                  if constexpr (STAMPED) STAMP(5);
                  const int nextP = (nb >> 1) + NIMG < NPAIR ? (nb >> 1) + NIMG : 0;
                  if constexpr (TWO) {
                    // this pair's image (the one two pairs back read, retired
                    // by the previous pair's barrier), then the one barrier
#pragma unroll
                    for (int i = 0; i < NIMG * NST; ++i)
                      *reinterpret_cast<f32x4*>(img + (rb * NIMG + i / NST) * LS_IMG + (tid + NT * (i % NST)) * 16) = st[i];
                    __syncthreads();
                    issue(nextP);
                  } else {
                    commit();
                    issue(nextP);
                  }
                  if constexpr (STAMPED) STAMP(2);   // barriers + staging
                }
                if constexpr (!ODD) {
                  if constexpr (STAMPED && POS != 0) STAMP(5);   // tensor product (+ stores)
                  if (act) {
                    ls_prio<1>();   // MFMA bursts first
                    Op3 wq, wq1;   // both blocks' pieces read first
                    lds_op3<LS_PCS>(wq, pimg, 0, lane);
                    lds_op3<LS_PCS>(wq1, pimg, 1, lane);
                    phase();
                    wv0 = w2_block_bwd<false>(hq, wq);
                    tv0 = w2_block_tan<false>(hdq, wq);
                    wv1 = w2_block_bwd<false>(hq, wq1);
                    tv1 = w2_block_tan<false>(hdq, wq1);
                    ls_prio<0>();
                  }
                  if constexpr (STAMPED) STAMP(3);   // w recompute and tangent
                }
                if (act) {
                  const f32x4 wv = ODD ? wv1 : wv0, tv = ODD ? tv1 : tv0;
                  float gm[4 * D3];
                  if constexpr (OFF0 > 0 && pi == 0) {   // (two images: from L2, prefetched)
#pragma unroll
                    for (int k = 0; k < 4; ++k) gm[k] = g0[k];
                  } else {
                    const float* gl = dacc + p.moff + 16 * jj * D3 + 4 * g * D3;
#pragma unroll
                    for (int k = 0; k < 4 * D3; ++k) gm[k] = gl[k];
                  }
                  float dwr[4];
                  // padded slots: y = 0, so dE/dx = dE/dw = 0 there
                  tp_bwd_xw4<p.l1, p.l2, p.l3>(x, y + yoff(p.l2), wv, gm, dx, dYa + yoff(p.l2), dwr);
                  if constexpr (L::KIND != 0) pin<4 * D1>(dx);
                  pin<8>(dYa + 1);
#pragma unroll
                  for (int r = 0; r < 4; ++r) drl += dwr[r] * tv[r];   // dE/dw . dw/dr
                }
                if constexpr (TWO && POS == 2 * NIMG - 1) rb ^= 1;   // the next pair(s) read the other buffer
              }
            });
            // per-edge dE/dx[nbr]; the first block's inputs are the species
            // embedding, whose gradient no output needs: no stores at all (a
            // store to an empty descriptor still costs its issue and its
            // trip through the texture unit), and dx itself is dead code there
            if constexpr (L::KIND != 0)
              stv<4 * D1>(Rd, vd + 4 * g * D1 * 4, (XOFF + 16 * jj * D1) * 4, dx);
          });
        };
        if constexpr (QUAD) {
          // every group unrolled (two passes at most): with a loop left, the
          // branch around the prefetch kept three of its registers in scratch
          // memory, and each of those accesses waits for every load in flight
          sfor<MUL / 16 / U>([&](auto it) { groups(it * U); });
        } else {
          for (int j2 = 0; j2 < MUL / 16; j2 += U) groups(j2);
        }
      }
    });
    if constexpr (STAMPED) STAMP(5);   // (the last block's tensor product)
    if (act) {
      // dE/dY of edge c: sum over the 4 lane groups, then dE/du through the SH
      // polynomials (serial_code.py:50-70)
      {   // (grouped sums, like the forward's)
        float d4a[4] = {dYa[1], dYa[2], dYa[3], dYa[4]}, d4b[4] = {dYa[5], dYa[6], dYa[7], dYa[8]};
        sum_rows4_n<4>(d4a);
        sum_rows4_n<4>(d4b);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          dYa[1 + q] = d4a[q];
          dYa[5 + q] = d4b[q];
        }
      }
      if (g == 0 && er >= 0) {
        const float s3 = 1.7320508075688772f, s5 = 2.23606797749979f, c15 = s3 * s5;
        const float is3 = 0.57735026918962576f;  // 1 / sqrt(3)
        const float ux = y[1] * is3, uy = y[2] * is3, uz = y[3] * is3;
        const float* d = dYa + 1;  // d[0..2] = dE/dY_1, d[3..7] = dE/dY_2
        const float gx = s3 * d[0] + c15 * (uz * d[3] + uy * d[4]) - s5 * ux * d[5] - c15 * ux * d[7];
        const float gy = s3 * d[1] + c15 * (ux * d[4] + uz * d[6]) + 2.f * s5 * uy * d[5];
        const float gz = s3 * d[2] + c15 * (ux * d[3] + uy * d[6]) - s5 * uz * d[5] + c15 * uz * d[7];
        float* o = dgu + (int64_t)er * 3;
        if constexpr (KEEP) {
          o[0] = gu_old[0] + gx;
          o[1] = gu_old[1] + gy;
          o[2] = gu_old[2] + gz;
        } else {
          o[0] += gx;
          o[1] += gy;
          o[2] += gz;
        }
      }
      // dE/dr |radial of edge c: the same sum over the 4 lane groups
      const float dr = sum_rows4(drl);
      if (g == 0 && er >= 0) {
        if constexpr (KEEP) drad[er] = dr_old + dr;
        else drad[er] += dr;
      }
    }
    if constexpr (STAMPED) STAMP(6);   // tile end: dE/dY and dE/dr sums
  }
  if constexpr (STAMPED) STAMP_FLUSH(blockIdx.x * WPG + wid);
}

}  // namespace

template <class L>
static hipError_t bwd_ls_impl(const FusedArgs& a, hipStream_t s) {
  const int ne = a.e_end - a.e_begin, per = LS_ROUNDS * 16 * LS_WPG;   // edges per workgroup
  if (ne <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_conv_bwd_ls<L>, dim3((ne + per - 1) / per), dim3(64 * LS_WPG), 0, s, a.row_ptr, a.nbr,
                     a.emb, a.Y, a.h, a.gagg, a.W, a.dxc, a.dgu, a.embd, a.drad, a.center, a.e_begin, a.e_end,
                     a.c_end, a.n_nodes);
  return hipGetLastError();
}

template <class L>
static hipError_t fwd_impl(const FusedArgs& a, hipStream_t s) {
  const int nc = a.c_end - a.c_begin;  // centre range of this launch
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_conv_fwd<L>, dim3((nc + 3) / 4), dim3(256), 0, s, a.row_ptr, a.nbr, a.emb,
                     a.Y, a.h, a.agg, a.W, a.c_begin, a.c_end, a.n_nodes, a.denom);
  return hipGetLastError();
}

template <class L>
static hipError_t bwd_nbr_impl(const FusedArgs& a, hipStream_t s) {
  const int nn = a.node_end - a.node_begin;
  hipLaunchKernelGGL(k_conv_bwd_nbr<L>, dim3((nn + 3) / 4), dim3(256), 0, s, a.src_ptr, a.src_perm,
                     a.center, a.emb, a.Y, a.h, a.gagg, a.W, a.dh, a.dgu, a.n_centers, a.node_begin,
                     a.node_end, a.embd, a.drad);
  return hipGetLastError();
}

// kind code -> family (tp.h)
#define E3GNN_FAMILY_SWITCH(code, F_FIRST, F_MID, F_LAST)       \
  switch (code) {                                               \
    case 0: F_FIRST(0); case 1: F_MID(0); case 2: F_LAST(0);    \
    case 3: F_FIRST(1); case 4: F_MID(1); case 5: F_LAST(1);    \
    case 6: F_FIRST(2); case 7: F_MID(2); case 8: F_LAST(2);    \
    default: return hipErrorInvalidValue;                       \
  }

hipError_t launch_conv_bwd_ls(int kind, const FusedArgs& a, hipStream_t s) {
  const int nc = a.c_end - a.c_begin;
  if (nc <= 0 || a.n_nodes <= 0) return hipSuccess;
#define FIRST_(f) return bwd_ls_impl<Family<f>::First>(a, s)
#define MID_(f) return bwd_ls_impl<Family<f>::Mid>(a, s)
#define LAST_(f) return hipErrorInvalidValue   // the last block: launch_conv_bwd_nbr_last
  E3GNN_FAMILY_SWITCH(kind, FIRST_, MID_, LAST_)
#undef FIRST_
#undef MID_
#undef LAST_
}

hipError_t launch_conv_fwd(int kind, const FusedArgs& a, hipStream_t s) {
#define FIRST_(f) return fwd_impl<Family<f>::First>(a, s)
#define MID_(f) return fwd_impl<Family<f>::Mid>(a, s)
#define LAST_(f) return fwd_impl<Family<f>::Last>(a, s)
  E3GNN_FAMILY_SWITCH(kind, FIRST_, MID_, LAST_)
#undef FIRST_
#undef MID_
#undef LAST_
}

hipError_t launch_conv_bwd_nbr_last(int kind, const FusedArgs& a, hipStream_t s) {
  const int nn = a.node_end - a.node_begin;
  if (nn <= 0 || a.n_nodes <= 0) return hipSuccess;
#define FIRST_(f) return hipErrorInvalidValue
#define MID_(f) return hipErrorInvalidValue
#define LAST_(f) return bwd_nbr_impl<Family<f>::Last>(a, s)
  E3GNN_FAMILY_SWITCH(kind, FIRST_, MID_, LAST_)
#undef FIRST_
#undef MID_
#undef LAST_
}

template <class L>
static void kind_dims(int* dx, int* w, int* dm) {
  *dx = L::DX;
  *w = L::W;
  *dm = L::DM;
}
bool fused_kind_dims(int code, int* dx, int* w, int* dm) {
  auto f = [&]() -> hipError_t {
#define FIRST_(f) return kind_dims<Family<f>::First>(dx, w, dm), hipSuccess
#define MID_(f) return kind_dims<Family<f>::Mid>(dx, w, dm), hipSuccess
#define LAST_(f) return kind_dims<Family<f>::Last>(dx, w, dm), hipSuccess
    E3GNN_FAMILY_SWITCH(code, FIRST_, MID_, LAST_)
#undef FIRST_
#undef MID_
#undef LAST_
  };
  return f() == hipSuccess;
}

// algorithmic FLOP of one TP forward per edge: per path and channel 2 per CG
// entry + 1 per output component (SURVEY.md 8d's 3,456 / 16,832 / 1,184 for
// SevenNet-0's first / middle / last block)
template <class L>
constexpr double kind_tp_flops() {
  double f = 0;
  sfor_host<L::NP>([&](auto pi) {
    constexpr PathDef p = L::P[pi];
    f += (double)p.mul * (2 * CG<p.l1, p.l2, p.l3>::n + 2 * p.l3 + 1);
  });
  return f;
}
static_assert(kind_tp_flops<LayerFirst>() == 3456.0 && kind_tp_flops<LayerMid>() == 16832.0 &&
                  kind_tp_flops<LayerLast>() == 1184.0,
              "SURVEY.md 8d per-edge TP FLOP");
double fused_kind_tp_flops(int code) {
  switch (code) {
#define K_(c, f, T) \
  case c:           \
    return kind_tp_flops<Family<f>::T>();
    K_(0, 0, First) K_(1, 0, Mid) K_(2, 0, Last) K_(3, 1, First) K_(4, 1, Mid) K_(5, 1, Last)
    K_(6, 2, First) K_(7, 2, Mid) K_(8, 2, Last)
#undef K_
    default: return 0.0;
  }
}

template <class L>
static int kind_paths(PathDef* out, int max) {
  for (int p = 0; p < L::NP && p < max; ++p) out[p] = L::P[p];
  return L::NP;
}
int fused_kind_paths(int code, PathDef* out, int max) {
  auto f = [&]() -> int {
    switch (code) {
#define K_(c, f, T) \
  case c:           \
    return kind_paths<Family<f>::T>(out, max);
      K_(0, 0, First) K_(1, 0, Mid) K_(2, 0, Last) K_(3, 1, First) K_(4, 1, Mid) K_(5, 1, Last)
      K_(6, 2, First) K_(7, 2, Mid) K_(8, 2, Last)
#undef K_
      default: return 0;
    }
  };
  return f();
}

}  // namespace e3gnn

#ifdef E3GNN_STAMPS
// diagnostic builds only: the device buffer the middle backward's phase
// stamps go to ([waves][8] u64; null disables)
extern "C" int e3gnn_debug_stamps(void* p) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(e3gnn::g_stamp_buf), &p, sizeof(p));
}
#endif
