// The reduce-scatter row sums of common.h against the all-reduces they
// replace: the lane that common.h names as the owner of value q must hold the
// bits the all-reduce gives for that value (random floats, so a different
// pairing of the summands would show as a different rounding).
//   sum_rows4_scatter<N>, N = 1..5   against sum_rows4   (four 16-lane rows)
//   row_scatter16<NB>, NB = 4, 8, 16 against row_sum16   (16 lanes of a row)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "../../sevennet_finetuning_amd/csrc/common.h"

// in: [16][64] values; ref4: [5][64]; got4: [5 (N)][2 (batch)][64];
// ref16: [16][64]; got16: [3 (NB = 4, 8, 16)][64]
__global__ void k(const float* in, float* ref4, float* got4, float* ref16, float* got16) {
  const int l = threadIdx.x;
  float v[16];
  for (int q = 0; q < 16; ++q) v[q] = in[64 * q + l];
  for (int q = 0; q < 5; ++q) ref4[64 * q + l] = e3gnn::sum_rows4(v[q]);
  float o1[1], o2[2] = {0.f, 0.f};
  const float v1[1] = {v[0]}, v2[2] = {v[0], v[1]}, v3[3] = {v[0], v[1], v[2]},
              v4[4] = {v[0], v[1], v[2], v[3]}, v5[5] = {v[0], v[1], v[2], v[3], v[4]};
  e3gnn::sum_rows4_scatter<1>(v1, o1);
  got4[(0 * 2 + 0) * 64 + l] = o1[0];
  e3gnn::sum_rows4_scatter<2>(v2, o1);
  got4[(1 * 2 + 0) * 64 + l] = o1[0];
  e3gnn::sum_rows4_scatter<3>(v3, o1);
  got4[(2 * 2 + 0) * 64 + l] = o1[0];
  e3gnn::sum_rows4_scatter<4>(v4, o1);
  got4[(3 * 2 + 0) * 64 + l] = o1[0];
  e3gnn::sum_rows4_scatter<5>(v5, o2);
  got4[(4 * 2 + 0) * 64 + l] = o2[0];
  got4[(4 * 2 + 1) * 64 + l] = o2[1];
  for (int q = 0; q < 16; ++q) ref16[64 * q + l] = e3gnn::row_sum16(v[q]);
  const e3gnn::RowSel s = e3gnn::row_scatter_sel(l & 15);
  got16[0 * 64 + l] = e3gnn::row_scatter16<4>(v, s);
  got16[1 * 64 + l] = e3gnn::row_scatter16<8>(v, s);
  got16[2 * 64 + l] = e3gnn::row_scatter16<16>(v, s);
}

// value index row g of batch b holds after sum_rows4_scatter<N> (-1: none)
static int owner4(int N, int b, int g) {
  if (b == 1) return N == 5 ? 4 : -1;
  switch (N) {
    case 1: return 0;
    case 2: return g / 2;
    case 3: return g == 3 ? 1 : g;
    default: return g;
  }
}
// e3gnn::row_scatter_own on the host
static int owner16(int col) {
  return ((col ^ (col >> 2)) & 1) | ((((col >> 1) ^ (col >> 2)) & 1) << 1) |
         ((((col >> 2) ^ (col >> 3)) & 1) << 2) | (col & 8);
}

int main() {
  static float h[16 * 64], ref4[5 * 64], got4[5 * 2 * 64], ref16[16 * 64], got16[3 * 64];
  srand(1);
  for (int i = 0; i < 16 * 64; ++i) h[i] = (float)(rand() & 0xffffff) / 8388608.f - 1.f;
  float *din, *dref4, *dgot4, *dref16, *dgot16;
  if (hipMalloc(&din, sizeof h) || hipMalloc(&dref4, sizeof ref4) || hipMalloc(&dgot4, sizeof got4) ||
      hipMalloc(&dref16, sizeof ref16) || hipMalloc(&dgot16, sizeof got16))
    return 2;
  (void)hipMemcpy(din, h, sizeof h, hipMemcpyHostToDevice);
  (void)hipMemset(dgot4, 0, sizeof got4);
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, din, dref4, dgot4, dref16, dgot16);
  if (hipMemcpy(ref4, dref4, sizeof ref4, hipMemcpyDeviceToHost) ||
      hipMemcpy(got4, dgot4, sizeof got4, hipMemcpyDeviceToHost) ||
      hipMemcpy(ref16, dref16, sizeof ref16, hipMemcpyDeviceToHost) ||
      hipMemcpy(got16, dgot16, sizeof got16, hipMemcpyDeviceToHost))
    return 2;
  int bad = 0;
  // the all-reduces against their documented pairings
  for (int q = 0; q < 5; ++q)
    for (int l = 0; l < 64; ++l) {
      const float* r = h + 64 * q + (l & 15);
      if (ref4[64 * q + l] != (r[0] + r[32]) + (r[16] + r[48])) ++bad;
    }
  printf("sum_rows4 mismatches: %d\n", bad);
  int bad16 = 0;
  for (int q = 0; q < 16; ++q)
    for (int l = 0; l < 64; ++l) {
      float s[16];
      for (int c = 0; c < 16; ++c) s[c] = h[64 * q + (l & 48) + c];
      const int c = l & 15;
      const float s1 = s[c] + s[c ^ 1], p1 = s[c ^ 2] + s[c ^ 3];                  // quad pairs
      const float q0 = s1 + p1;                                                    // the lane's quad
      const int m = (c & 8) | (7 - (c & 7));                                       // half mirror
      const float q1 = (s[m] + s[m ^ 1]) + (s[m ^ 2] + s[m ^ 3]);
      const int n = 15 - c, nm = (n & 8) | (7 - (n & 7));                          // row mirror
      const float q2 = (s[n] + s[n ^ 1]) + (s[n ^ 2] + s[n ^ 3]), q3 = (s[nm] + s[nm ^ 1]) + (s[nm ^ 2] + s[nm ^ 3]);
      if (ref16[64 * q + l] != (q0 + q1) + (q2 + q3)) ++bad16;
    }
  printf("row_sum16 mismatches: %d\n", bad16);
  bad += bad16;
  for (int N = 1; N <= 5; ++N) {
    int badn = 0;
    for (int b = 0; b < 2; ++b)
      for (int l = 0; l < 64; ++l) {
        const int q = owner4(N, b, l >> 4);
        if (q >= 0 && got4[((N - 1) * 2 + b) * 64 + l] != ref4[64 * q + l]) ++badn;
      }
    printf("sum_rows4_scatter<%d> mismatches: %d\n", N, badn);
    bad += badn;
  }
  for (int i = 0; i < 3; ++i) {
    const int NB = 4 << i;
    int badn = 0;
    for (int l = 0; l < 64; ++l)
      if (got16[i * 64 + l] != ref16[64 * (owner16(l & 15) & (NB - 1)) + l]) ++badn;
    printf("row_scatter16<%d> mismatches: %d\n", NB, badn);
    bad += badn;
  }
  return bad != 0;
}
