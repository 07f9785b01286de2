// The FCN readout in the fine-tune step (fcn_train.h): forward + first
// reverse, tangent forward and dual reverse, each one launch over the atoms.
//
// The scheme is k_readout_fcn's (node.hip): a wave owns FT_AW = 8 atoms per
// pass, four per half-wave; lane (h, l) = (lane / 32, lane % 32) owns unit l
// (+ 32, 64, 96) of a layer for the atoms 4h .. 4h + 3.  A layer's vector sits
// interleaved in LDS (v[i * 8 + atom]) and every sum runs over its inputs in
// ascending order: bitwise repeatable, no atomics (the final dot product is a
// fixed butterfly over the half-wave).  The packed weights (node.h FcnDims)
// are staged in LDS when they fit beside the scratch, else read from global
// memory in the same layout; their odd row stride keeps the forward's reads
// (lanes along a row) and the reverse's (lanes down a column) free of LDS bank
// conflicts.  What a later pass needs (z_k, z'_k, a_k, a'_k, z-bar_k) goes to
// global memory: a thread reads back only elements it wrote itself (the same
// (atom, unit) ownership in every pass), so no fence is needed within a launch.
#include "fcn_train.h"

#include "fcn_act.h"

namespace e3gnn {
namespace {

constexpr int FT_AW = 8;
constexpr int FT_VEC = FT_AW * FCN_MAX_WIDTH;   // one layer vector of a wave's atoms
constexpr int FT_WAVE_FLOATS = 4 * FT_VEC;      // (primal, tangent) x (in, out)

__device__ __forceinline__ float ft_half_wave_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// acc[q] = sum_{i < cnt} in[8 i + q] m[i * stride], ascending i
__device__ __forceinline__ void ft_mv(const float* in, const float* m, int cnt, int stride, float acc[4]) {
  acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
#pragma unroll 4
  for (int i = 0; i < cnt; ++i) {
    const float4 a = *reinterpret_cast<const float4*>(in + FT_AW * i);
    const float w = m[(int64_t)i * stride];
    acc[0] = fmaf(a.x, w, acc[0]);
    acc[1] = fmaf(a.y, w, acc[1]);
    acc[2] = fmaf(a.z, w, acc[2]);
    acc[3] = fmaf(a.w, w, acc[3]);
  }
}

__device__ __forceinline__ void ft_store4(float* p, const float v[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// the wave's rows of x [n, D], interleaved: dst[i * 8 + atom] (zero past n)
__device__ __forceinline__ void ft_load_rows(float* dst, const float* __restrict__ x, int a0, int n, int D,
                                             int lane) {
  for (int idx = lane; idx < FT_AW * D; idx += 64) {
    const int a = idx / D, i = idx - a * D;
    dst[i * FT_AW + a] = a0 + a < n ? x[(int64_t)a0 * D + idx] : 0.f;
  }
}

template <bool LDSW>
__device__ __forceinline__ const float* ft_weights(const FcnDims& d, const float* __restrict__ Wg, float* lds,
                                                   float*& scr) {
  scr = lds;
  if constexpr (LDSW) {
    const int nw = d.padded_floats();
    for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = Wg[i];
    scr = lds + nw;
    return lds;
  }
  return Wg;
}

// TANGENT false: x -> z_k, a_k, s, then dx = seed ds/dx (dx not null);
// TANGENT true:  x' -> z'_k = a'_{k-1} M, a'_k = c f'(z_k) z'_k, s' (zin = z)
template <bool LDSW, bool TANGENT>
__global__ __launch_bounds__(256) void k_fcn_train_fwd(int n, FcnDims d, const float* __restrict__ Wg,
                                                       const float* __restrict__ x,
                                                       const float* __restrict__ seed,
                                                       const float* __restrict__ zin, float* __restrict__ zout,
                                                       float* __restrict__ a, float* __restrict__ s,
                                                       float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float ft_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
  const int h4 = 4 * (lane >> 5), l = lane & 31;
  float* scr;
  const float* W = ft_weights<LDSW>(d, Wg, ft_lds, scr);
  const int D = d.w[0], nh = d.nh;
  float* b0 = scr + wave * FT_WAVE_FLOATS;
  float* b1 = b0 + FT_VEC;
  const float* wl = W + d.mat_off(nh);
  const int64_t n64 = n;
  __syncthreads();
  // (the loop bounds are the same for the whole workgroup: the barriers are legal)
#pragma unroll 1
  for (int base = blockIdx.x * nwave * FT_AW; base < n; base += gridDim.x * nwave * FT_AW) {
    const int a0 = base + wave * FT_AW;
    const int at = a0 + h4;                 // this lane's atoms at .. at + 3
    ft_load_rows(b0, x, a0, n, D, lane);
    __syncthreads();
    const float* ain = b0;
    float* aout = b1;
    float p[4] = {0.f, 0.f, 0.f, 0.f};
    int pre = 0;
#pragma unroll 1
    for (int k = 0; k < nh; ++k) {          // hidden layer k + 1
      const int wi = d.w[k], wo = d.w[k + 1], ws = d.stride(k);
      const float* M = W + d.mat_off(k);
      const bool lastk = k == nh - 1;
      float* ak = a + 2 * n64 * pre + (TANGENT ? n64 * wo : 0);
#pragma unroll 1
      for (int jb = 0; jb < wo; jb += 32) {
        const int j = jb + l < wo ? jb + l : wo - 1;   // (idle lanes repeat the last unit)
        float zz[4];
        ft_mv(ain + h4, M + j, wi, ws, zz);
        if (jb + l < wo) {
          const float wj = lastk ? wl[j] : 0.f;
          float av[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int64_t o = n64 * pre + (int64_t)(at + q) * wo + j;
            const bool live = at + q < n;
            float f, df;
            if constexpr (TANGENT) {
              fcn_act(d.kind, live ? zin[o] : 0.f, f, df);
              av[q] = d.c * df * zz[q];
            } else {
              fcn_act(d.kind, zz[q], f, df);
              av[q] = d.c * f;
            }
            if (live) {
              zout[o] = zz[q];
              ak[(int64_t)(at + q) * wo + j] = av[q];
            }
            p[q] = fmaf(av[q], wj, p[q]);
          }
          if (!lastk) ft_store4(aout + FT_AW * j + h4, av);
        }
      }
      __syncthreads();
      ain = aout;
      aout = aout == b0 ? b1 : b0;
      pre += wo;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      p[q] = ft_half_wave_sum(p[q]);
      if (l == 0 && at + q < n) s[at + q] = p[q];
    }
    if constexpr (!TANGENT) {
      if (dx != nullptr) {   // (uniform) first reverse: g_k = ds/dz_k, then dx through M_0
        float* gc = b0;
        float* gn = b1;
        pre -= d.w[nh];
        {
          const int wo = d.w[nh];
#pragma unroll 1
          for (int jb = 0; jb < wo; jb += 32) {
            const int j = jb + l;
            if (j < wo) {
              float gv[4];
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                float f, df;
                fcn_act(d.kind, at + q < n ? zout[n64 * pre + (int64_t)(at + q) * wo + j] : 0.f, f, df);
                gv[q] = d.c * df * wl[j];
              }
              ft_store4(gc + FT_AW * j + h4, gv);
            }
          }
        }
        __syncthreads();
#pragma unroll 1
        for (int k = nh - 1; k >= 0; --k) {   // through M_k to layer k (k = 0: x)
          const int wi = d.w[k], wo = d.w[k + 1], ws = d.stride(k);
          const float* M = W + d.mat_off(k);
          if (k > 0) pre -= wi;
#pragma unroll 1
          for (int ib = 0; ib < wi; ib += 32) {
            const int i = ib + l < wi ? ib + l : wi - 1;
            float g[4];
            ft_mv(gc + h4, M + (int64_t)i * ws, wo, 1, g);
            if (ib + l < wi) {
              if (k > 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  float f, df;
                  fcn_act(d.kind, at + q < n ? zout[n64 * pre + (int64_t)(at + q) * wi + i] : 0.f, f, df);
                  g[q] *= d.c * df;
                }
                ft_store4(gn + FT_AW * i + h4, g);
              } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                  if (at + q < n) dx[(int64_t)(at + q) * D + i] = (seed ? seed[at + q] : 1.f) * g[q];
              }
            }
          }
          __syncthreads();
          float* t = gc;
          gc = gn;
          gn = t;
        }
      }
    }
  }
}

// The reverse of (s, s') with seeds (sb, sbd): a-bar_nh = sb v, a'-bar_nh = sbd v;
//   z'-bar_k = c f'(z_k) a'-bar_k,  z-bar_k = c f'(z_k) a-bar_k + c f''(z_k) z'_k a'-bar_k,
//   (a-bar, a'-bar)_{k-1} = (z-bar, z'-bar)_k M_{k-1}^T;  layer 0 is xb [2n, D].
template <bool LDSW>
__global__ __launch_bounds__(256) void k_fcn_train_dual(int n, FcnDims d, const float* __restrict__ Wg,
                                                        const float* __restrict__ sb,
                                                        const float* __restrict__ sbd,
                                                        const float* __restrict__ z,
                                                        const float* __restrict__ zd, float* __restrict__ zb,
                                                        float* __restrict__ xb) {
  extern __shared__ __attribute__((aligned(16))) float ft_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
  const int h4 = 4 * (lane >> 5), l = lane & 31;
  float* scr;
  const float* W = ft_weights<LDSW>(d, Wg, ft_lds, scr);
  const int D = d.w[0], nh = d.nh;
  float* buf = scr + wave * FT_WAVE_FLOATS;
  const float* wl = W + d.mat_off(nh);
  const int64_t n64 = n;
  int pre_last = 0;
  for (int k = 1; k < nh; ++k) pre_last += d.w[k];
  __syncthreads();
#pragma unroll 1
  for (int base = blockIdx.x * nwave * FT_AW; base < n; base += gridDim.x * nwave * FT_AW) {
    const int at = base + wave * FT_AW + h4;
    float* gp = buf;                 // z-bar, z'-bar of the current layer
    float* gt = buf + FT_VEC;
    float* np_ = buf + 2 * FT_VEC;   // ... of the next (lower) one
    float* nt = buf + 3 * FT_VEC;
    float sp[4], st[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      sp[q] = at + q < n ? sb[at + q] : 0.f;
      st[q] = at + q < n ? sbd[at + q] : 0.f;
    }
    int pre = pre_last;
    // layer k's (a-bar, a'-bar) of unit j -> (z-bar, z'-bar): global and LDS
    auto step = [&](int wk, int j, const float ab[4], const float abd[4], float* op, float* ot) {
      float vp[4], vt[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool live = at + q < n;
        const int64_t o = n64 * pre + (int64_t)(at + q) * wk + j;
        const float zz = live ? z[o] : 0.f, zzd = live ? zd[o] : 0.f;
        float f, df;
        fcn_act(d.kind, zz, f, df);
        const float d2 = fcn_act2(d.kind, zz);
        vt[q] = d.c * df * abd[q];
        vp[q] = d.c * df * ab[q] + d.c * d2 * zzd * abd[q];
        if (live) {
          float* zk = zb + 2 * n64 * pre;
          zk[(int64_t)(at + q) * wk + j] = vp[q];
          zk[(n64 + at + q) * wk + j] = vt[q];
        }
      }
      ft_store4(op + FT_AW * j + h4, vp);
      ft_store4(ot + FT_AW * j + h4, vt);
    };
    {
      const int wo = d.w[nh];
#pragma unroll 1
      for (int jb = 0; jb < wo; jb += 32) {
        const int j = jb + l;
        if (j < wo) {
          float ab[4], abd[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ab[q] = sp[q] * wl[j];
            abd[q] = st[q] * wl[j];
          }
          step(wo, j, ab, abd, gp, gt);
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int k = nh - 1; k >= 0; --k) {
      const int wi = d.w[k], wo = d.w[k + 1], ws = d.stride(k);
      const float* M = W + d.mat_off(k);
      if (k > 0) pre -= wi;
#pragma unroll 1
      for (int ib = 0; ib < wi; ib += 32) {
        const int i = ib + l < wi ? ib + l : wi - 1;
        float ab[4], abd[4];
        ft_mv(gp + h4, M + (int64_t)i * ws, wo, 1, ab);
        ft_mv(gt + h4, M + (int64_t)i * ws, wo, 1, abd);
        if (ib + l < wi) {
          if (k > 0) {
            step(wi, i, ab, abd, np_, nt);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (at + q < n) {
                xb[(int64_t)(at + q) * D + i] = ab[q];
                xb[(n64 + at + q) * D + i] = abd[q];
              }
          }
        }
      }
      __syncthreads();
      float* t = gp;
      gp = np_;
      np_ = t;
      t = gt;
      gt = nt;
      nt = t;
    }
  }
}

bool ft_dims_ok(const FcnDims& d) {
  if (d.nh < 1 || d.nh > FCN_MAX_HIDDEN || d.kind < 0 || d.kind >= FCN_ACT_KINDS) return false;
  for (int k = 0; k <= d.nh; ++k)
    if (d.w[k] < 1 || d.w[k] > FCN_MAX_WIDTH) return false;
  return true;
}

// waves per workgroup and whether the weights are staged in LDS (64 KB in all)
void ft_shape(const FcnDims& d, int n, int& nwave, bool& ldsw, size_t& lds, int& grid) {
  const size_t lim = 64 * 1024, wave = (size_t)FT_WAVE_FLOATS * sizeof(float);
  const size_t wbytes = (size_t)d.padded_floats() * sizeof(float);
  ldsw = wbytes + wave <= lim;
  nwave = (int)(((ldsw ? lim - wbytes : lim)) / wave);
  if (nwave > 4) nwave = 4;
  const int per = nwave * FT_AW;
  if ((n + per - 1) / per < 2 && nwave > 1) {   // a few atoms: one wave per 8 of them
    nwave = (n + FT_AW - 1) / FT_AW;
    if (nwave < 1) nwave = 1;
  }
  lds = (ldsw ? wbytes : 0) + nwave * wave;
  grid = (n + nwave * FT_AW - 1) / (nwave * FT_AW);
  if (grid > 1024) grid = 1024;
}

}  // namespace

hipError_t launch_fcn_train_fwd(int n, const FcnDims& d, const float* W, const float* x, const float* seed,
                                float* z, float* a, float* s, float* dx, hipStream_t st) {
  if (!ft_dims_ok(d) || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int nwave, grid;
  bool ldsw;
  size_t lds;
  ft_shape(d, n, nwave, ldsw, lds, grid);
  if (ldsw)
    hipLaunchKernelGGL((k_fcn_train_fwd<true, false>), dim3(grid), dim3(64 * nwave), lds, st, n, d, W, x, seed,
                       (const float*)nullptr, z, a, s, dx);
  else
    hipLaunchKernelGGL((k_fcn_train_fwd<false, false>), dim3(grid), dim3(64 * nwave), lds, st, n, d, W, x, seed,
                       (const float*)nullptr, z, a, s, dx);
  return hipGetLastError();
}

hipError_t launch_fcn_train_tangent(int n, const FcnDims& d, const float* W, const float* xd, const float* z,
                                    float* zd, float* a, float* sd, hipStream_t st) {
  if (!ft_dims_ok(d) || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int nwave, grid;
  bool ldsw;
  size_t lds;
  ft_shape(d, n, nwave, ldsw, lds, grid);
  if (ldsw)
    hipLaunchKernelGGL((k_fcn_train_fwd<true, true>), dim3(grid), dim3(64 * nwave), lds, st, n, d, W, xd,
                       (const float*)nullptr, z, zd, a, sd, (float*)nullptr);
  else
    hipLaunchKernelGGL((k_fcn_train_fwd<false, true>), dim3(grid), dim3(64 * nwave), lds, st, n, d, W, xd,
                       (const float*)nullptr, z, zd, a, sd, (float*)nullptr);
  return hipGetLastError();
}

hipError_t launch_fcn_train_dual(int n, const FcnDims& d, const float* W, const float* sb, const float* sbd,
                                 const float* z, const float* zd, float* zb, float* xb, hipStream_t st) {
  if (!ft_dims_ok(d) || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int nwave, grid;
  bool ldsw;
  size_t lds;
  ft_shape(d, n, nwave, ldsw, lds, grid);
  if (ldsw)
    hipLaunchKernelGGL(k_fcn_train_dual<true>, dim3(grid), dim3(64 * nwave), lds, st, n, d, W, sb, sbd, z, zd, zb,
                       xb);
  else
    hipLaunchKernelGGL(k_fcn_train_dual<false>, dim3(grid), dim3(64 * nwave), lds, st, n, d, W, sb, sbd, z, zd, zb,
                       xb);
  return hipGetLastError();
}

}  // namespace e3gnn
