// Shared definitions for the e3gnn MI355X (gfx950) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

namespace e3gnn {

// ---------------------------------------------------------------- activations
// e3nn normalize2mom(silu): silu(x) * SILU_NORM (sevenn/_const.py:34-48 act
// table; the constant is frozen in serial_code.py as c5).
constexpr float SILU_NORM = 1.6791767923989418f;

// v_rcp_f32 (1 ulp) instead of an IEEE division (~10 VALU per call)
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float act_fwd(float x) { return x * sigmoidf_(x) * SILU_NORM; }
__device__ __forceinline__ float act_grad(float x) {
  const float s = sigmoidf_(x);
  return SILU_NORM * s * (1.0f + x * (1.0f - s));
}

// sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48), every
// lane gets the same bits: (r0 + r2) + (r1 + r3) via v_permlane32_swap /
// v_permlane16_swap (VALU, no LDS round trip).  Inline asm: the builtins'
// second result (the swapped source register) comes back as a copy of the
// first with this compiler (tools/microtests/permlane.hip); the s_nop pads the
// VALU-write -> permlane-read hazard, which hipcc does not insert inside asm.
__device__ __forceinline__ float sum_rows4(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  float s = a + b, t = s;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(s), "+v"(t));
  return s + t;
}

// the same for N values at once (N <= 5): each stage's N swaps back to back
// inside ONE asm statement, one hazard pad before and after the group instead
// of around every swap, and the N reductions' adds free to interleave
template <int N>
__device__ __forceinline__ void permlane_swap_n32(float (&a)[N], float (&b)[N]);
template <int N>
__device__ __forceinline__ void permlane_swap_n16(float (&a)[N], float (&b)[N]);
#define E3GNN_PL_SWAPS(W)                                                                             \
  template <>                                                                                         \
  __device__ __forceinline__ void permlane_swap_n##W<1>(float (&a)[1], float (&b)[1]) {               \
    asm volatile("s_nop 1\n\tv_permlane" #W "_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a[0]), "+v"(b[0]));    \
  }                                                                                                   \
  template <>                                                                                         \
  __device__ __forceinline__ void permlane_swap_n##W<2>(float (&a)[2], float (&b)[2]) {               \
    asm volatile("s_nop 1\n\tv_permlane" #W "_swap_b32 %0, %1\n\tv_permlane" #W "_swap_b32 %2, %3\n\ts_nop 1" \
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]));                                   \
  }                                                                                                   \
  template <>                                                                                         \
  __device__ __forceinline__ void permlane_swap_n##W<3>(float (&a)[3], float (&b)[3]) {               \
    asm volatile("s_nop 1\n\tv_permlane" #W "_swap_b32 %0, %1\n\tv_permlane" #W "_swap_b32 %2, %3"     \
                 "\n\tv_permlane" #W "_swap_b32 %4, %5\n\ts_nop 1"                                      \
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]));           \
  }                                                                                                   \
  template <>                                                                                         \
  __device__ __forceinline__ void permlane_swap_n##W<4>(float (&a)[4], float (&b)[4]) {               \
    asm volatile("s_nop 1\n\tv_permlane" #W "_swap_b32 %0, %1\n\tv_permlane" #W "_swap_b32 %2, %3"     \
                 "\n\tv_permlane" #W "_swap_b32 %4, %5\n\tv_permlane" #W "_swap_b32 %6, %7\n\ts_nop 1"  \
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]), "+v"(a[3]), \
                   "+v"(b[3]));                                                                       \
  }                                                                                                   \
  template <>                                                                                         \
  __device__ __forceinline__ void permlane_swap_n##W<5>(float (&a)[5], float (&b)[5]) {               \
    asm volatile("s_nop 1\n\tv_permlane" #W "_swap_b32 %0, %1\n\tv_permlane" #W "_swap_b32 %2, %3"     \
                 "\n\tv_permlane" #W "_swap_b32 %4, %5\n\tv_permlane" #W "_swap_b32 %6, %7"              \
                 "\n\tv_permlane" #W "_swap_b32 %8, %9\n\ts_nop 1"                                      \
                 : "+v"(a[0]), "+v"(b[0]), "+v"(a[1]), "+v"(b[1]), "+v"(a[2]), "+v"(b[2]), "+v"(a[3]), \
                   "+v"(b[3]), "+v"(a[4]), "+v"(b[4]));                                               \
  }
E3GNN_PL_SWAPS(32)
E3GNN_PL_SWAPS(16)
#undef E3GNN_PL_SWAPS
template <int N>
__device__ __forceinline__ void sum_rows4_n(float (&v)[N]) {
  static_assert(N >= 1 && N <= 5, "up to five values per group");
  float a[N], b[N];
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = b[i] = v[i];
  permlane_swap_n32<N>(a, b);
#pragma unroll
  for (int i = 0; i < N; ++i) a[i] = b[i] = a[i] + b[i];
  permlane_swap_n16<N>(a, b);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = a[i] + b[i];
}

// the same sums as a reduce-scatter: N different values need no N all-reduces
// when one row is to store each total.  Stage 1 swaps value q against value
// q + 2 (v_permlane32_swap: the upper 32 lanes of the first operand <-> the
// lower 32 of the second), so one swap + one add leave q's half sums r0 + r2
// (even row) and r1 + r3 (odd row) in lanes 0-31 and (q + 2)'s in lanes 32-63;
// stage 2 swaps the (0, 2) result against the (1, 3) result
// (v_permlane16_swap: the odd rows of the first <-> the even rows of the
// second) and adds.  Every total is (r0 + r2) + (r1 + r3), the pairs
// sum_rows4 adds: the same bits, only the lane holding them differs.
// Who holds what afterwards (row = lane >> 4):
//   N = 4: out[0] of row g is the total of v[g]               (3 swaps, 3 adds)
//   N = 3: rows 0, 1, 2 hold v[0], v[1], v[2]; row 3 v[1] again (same bits)
//   N = 2: rows 0 and 1 hold v[0], rows 2 and 3 hold v[1]     (2 swaps, 2 adds)
//   N = 1: every row holds v[0] (the all-reduce)
//   N = 5: out[0] as N = 4 for v[0..3], out[1] as N = 1 for v[4], the five
//          swaps in the same two hazard-padded groups         (5 swaps, 5 adds)
template <int N>
__device__ __forceinline__ void sum_rows4_scatter(const float (&v)[N], float (&out)[(N + 3) / 4]) {
  static_assert(N >= 1 && N <= 5, "up to five values per group");
  if constexpr (N <= 2) {
    float a[1] = {v[0]}, b[1] = {v[N - 1]};
    permlane_swap_n32<1>(a, b);
    float s[1] = {a[0] + b[0]};
    float t[1] = {s[0]};
    permlane_swap_n16<1>(s, t);
    out[0] = s[0] + t[0];
  } else if constexpr (N <= 4) {
    float a[2] = {v[0], v[1]}, b[2] = {v[2], v[N == 4 ? 3 : 1]};
    permlane_swap_n32<2>(a, b);
    float s[1] = {a[0] + b[0]}, t[1] = {a[1] + b[1]};
    permlane_swap_n16<1>(s, t);
    out[0] = s[0] + t[0];
  } else {
    float a[3] = {v[0], v[1], v[4]}, b[3] = {v[2], v[3], v[4]};
    permlane_swap_n32<3>(a, b);
    float s[2] = {a[0] + b[0], a[2] + b[2]};
    float t[2] = {a[1] + b[1], s[1]};
    permlane_swap_n16<2>(s, t);
    out[0] = s[0] + t[0];
    out[1] = s[1] + t[1];
  }
}

// sum over the 16 lanes of a DPP row (fixed order; every lane gets the total)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  v += dpp_mov<0x140>(v);  // row_mirror
  return v;
}

// the same row sums of NB different values (NB = 4, 8, 16) as a reduce-scatter:
// at a level a lane keeps one value of a pair and adds its partner's copy of
// it (the pair row_sum16 adds at that level, so the same bits), halving the
// values in flight; once one value is left the remaining levels are
// row_sum16's.  The partner of the two mirror levels differs in every lower
// lane bit, so the kept half is chosen by c0 = b0 ^ b2, c1 = b1 ^ b2,
// c2 = b2 ^ b3, b3 (b: bits of the lane's column), which a level's partner
// shares below that level and flips at it.  The lane ends with the total of
// v[row_scatter_own(col) % NB].
struct RowSel {
  bool c0, c1, c2, b3;
};
__device__ __forceinline__ RowSel row_scatter_sel(int col) {
  return {((col ^ (col >> 2)) & 1) != 0, (((col >> 1) ^ (col >> 2)) & 1) != 0,
          (((col >> 2) ^ (col >> 3)) & 1) != 0, (col & 8) != 0};
}
__device__ __forceinline__ int row_scatter_own(int col) {
  return ((col ^ (col >> 2)) & 1) | ((((col >> 1) ^ (col >> 2)) & 1) << 1) |
         ((((col >> 2) ^ (col >> 3)) & 1) << 2) | (col & 8);
}
template <int CTRL>
__device__ __forceinline__ float row_scatter_step(bool sel, float a, float b) {
  const float keep = sel ? b : a, send = sel ? a : b;
  return keep + dpp_mov<CTRL>(send);
}
template <int NB>
__device__ __forceinline__ float row_scatter16(const float* v, RowSel s) {
  static_assert(NB == 4 || NB == 8 || NB == 16, "a power of two of values");
  float w[NB / 2];
#pragma unroll
  for (int m = 0; m < NB / 2; ++m) w[m] = row_scatter_step<0xB1>(s.c0, v[2 * m], v[2 * m + 1]);
#pragma unroll
  for (int m = 0; m < NB / 4; ++m) w[m] = row_scatter_step<0x4E>(s.c1, w[2 * m], w[2 * m + 1]);
  if constexpr (NB >= 8) {
#pragma unroll
    for (int m = 0; m < NB / 8; ++m) w[m] = row_scatter_step<0x141>(s.c2, w[2 * m], w[2 * m + 1]);
  } else {
    w[0] += dpp_mov<0x141>(w[0]);
  }
  if constexpr (NB == 16) {
    w[0] = row_scatter_step<0x140>(s.b3, w[0], w[1]);
  } else {
    w[0] += dpp_mov<0x140>(w[0]);
  }
  return w[0];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- GEMM
// One sub-problem of a grouped f32 MFMA GEMM (gemm.hip).  Rows are (node, m)
// pairs so one problem covers a whole irrep block of an e3nn linear:
//   A(row, k)   = A[(row / R) * lda + a_off + k * R + row % R]
//   B(k, col)   = B[k * ldb + col]
//   C(row, col) = C[(row / R) * ldc + c_off + col * R + row % R]
// act: 0 none; 1 C = silu_n(acc), pre_out = acc; 2 C = acc * silu_n'(pre_in).
struct GemmProb {
  const float* A;
  const float* B;
  float* C;
  const float* pre_in;
  float* pre_out;
  int64_t lda, ldc;
  int M, N, K, R;
  int a_off, c_off, ldb;
  int beta, act;
  int tile_begin, tiles_n;
};
constexpr int GEMM_MAX_PROBS = 8;
struct GemmBatch {
  GemmProb p[GEMM_MAX_PROBS];
  int nprob;
  int total_tiles;
};
hipError_t launch_gemm(const GemmBatch& b, hipStream_t s);

// ---------------------------------------------------------------- node linears
// One irrep block of an e3nn linear (or of two linears into the same output
// block, K-concatenated: self_interaction_2 + self_connection forward,
// self_interaction_1^T + self_connection^T backward), node-aligned tiles
// (gemm.hip k_nodelin):
//   A(node, m, k) = k < K1 ? A [node * lda  + a_off  + k * R + m]
//                          : A2[node * lda2 + a_off2 + (k - K1) * R + m]
//   B(k, col)     = B[k * N + col]          (rows 0..K1-1 then K1..K-1)
//   C(node, m, col) = C[node * ldc + c_off + col * R + m]
// epi: 0 store, 1 accumulate, 2 store + xo[node, col] = act(v) for
// col < n_act (gate scalars / last block), 3 store + xo[node, xo_off + col * R
// + m] = act(C[node, gate_off + col]) * v (gated irreps; the gate columns were
// stored by an earlier launch).
// bias (use_bias_in_linear; R == 1 only, null: none): v += bias[col] before the
// store to C and before the activation -- C holds the biased pre-activations.
struct NlProb {
  const float* A;
  const float* A2;
  const float* B;
  const void* Bb;  // B as bf16 pieces (LinPair::Wb order): k_nodelin_b; null: k_nodelin
  const float* bias;  // the block's bias row (column 0 of the block first), 16-byte aligned

  float* C;
  float* xo;
  int64_t lda, lda2, ldc, ldxo;
  int a_off, a_off2, c_off, xo_off;
  int K1, K, N, R, nodes;
  int epi, n_act, gate_off;
  int wn, ns, tpn, tile_begin, tiles_n;  // set by add_nl
  int kind;  // set by add_nl: 0 k_nodelin (f32), 1 k_nodelin_b, 2 k_nodelin_s (bf16x6)
};
constexpr int NL_MAX_PROBS = 4;
struct NlBatch {
  NlProb p[NL_MAX_PROBS];
  int nprob;
  int total_tiles;
};
// false when the problem does not meet the kernel's layout assumptions
// (16-byte alignment of rows / offsets, K1 % 32 when split, R in {1, 3, 5},
// a bias on an R == 1 problem only)
bool add_nl(NlBatch& b, const NlProb& p);
hipError_t launch_nodelin(const NlBatch& b, hipStream_t s);

}  // namespace e3gnn
