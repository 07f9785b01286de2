// The error recorder's sums (sevennet_finetuning_amd/error_recorder.py; the
// reference's sevenn/error_recorder.py accumulates them with one .item() per
// metric per batch): one launch per recorded batch, accumulated on the device
// in f64, read once an epoch.
//
// One workgroup per quantity -- total energy, energy per atom, force (vectors
// of 3), stress (vectors of 6, times s_scale) -- walks its vectors with a
// 256-wide stride and reduces its sums by a fixed-order tree (no atomics: two
// runs give equal bits).  d = (f64)pred - (f64)ref, so every term is formed
// from the f32 inputs without a rounding of the difference.  A NaN label drops
// its component (the reference's delete_unlabled, the rule of k_loss_efs);
// a vector enters the vector sums only when all its components are labelled;
// the prediction at a dropped label is never loaded.  The accumulation into
// `sums` is a read-modify-write by one thread per slot: no memset, no
// synchronisation, capturable in a HIP graph.  Built with -ffp-contract=off
// (build_lib.py): d * d and its addition round separately, as the torch
// definition in error_recorder.py does.
#include <hip/hip_runtime.h>

#include "../../include/e3gnn.h"
#include "error_sums.h"

namespace e3gnn {
namespace {

constexpr int NS = E3GNN_ERR_SUMS_PER_QUANTITY;

__device__ __forceinline__ double crit64(int c, double delta, double x) {
  if (c == 0) return x * x;
  const double a = fabs(x);
  return a < delta ? 0.5 * x * x : delta * (a - 0.5 * delta);
}

__global__ __launch_bounds__(256) void k_error_sums(ErrSumArgs a) {
  __shared__ double red[NS][256];
  const int q = blockIdx.x, t = threadIdx.x;
  const bool energy = q == E3GNN_ERRQ_TOTAL_ENERGY || q == E3GNN_ERRQ_ENERGY;
  const float* pred = energy ? a.e_pred : (q == E3GNN_ERRQ_FORCE ? a.f_pred : a.s_pred);
  const float* ref = energy ? a.e_ref : (q == E3GNN_ERRQ_FORCE ? a.f_ref : a.s_ref);
  const int vdim = energy ? 1 : (q == E3GNN_ERRQ_FORCE ? 3 : 6);
  const int64_t nvec = q == E3GNN_ERRQ_FORCE ? a.n : a.nb;
  if (!pred || nvec <= 0) return;   // (uniform over the block)
  const double delta = (double)a.delta, scale = (double)a.s_scale;
  double acc[NS] = {0, 0, 0, 0, 0, 0};
  for (int64_t v = t; v < nvec; v += 256) {
    int labelled = 0;
    double sq = 0.0;
    for (int c = 0; c < vdim; ++c) {
      const int64_t i = v * vdim + c;
      const float r = ref[i];
      if (r != r) continue;
      double d = (double)pred[i] - (double)r;
      if (q == E3GNN_ERRQ_ENERGY) d /= (double)a.natoms[v];
      if (q == E3GNN_ERRQ_STRESS) d *= scale;
      ++labelled;
      sq += d * d;
      acc[E3GNN_ERRS_ABS] += fabs(d);
      acc[E3GNN_ERRS_CRIT] += crit64(a.criterion, delta, d);
    }
    acc[E3GNN_ERRS_COMPONENTS] += (double)labelled;
    if (labelled == vdim) {
      // Σd² over the fully labelled vectors only: RMSE divides it by their count
      acc[E3GNN_ERRS_VECTORS] += 1.0;
      acc[E3GNN_ERRS_SQ_VECTORS] += sq;
      acc[E3GNN_ERRS_NORM] += sqrt(sq);
    }
    acc[E3GNN_ERRS_SQ] += sq;
  }
  for (int k = 0; k < NS; ++k) red[k][t] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < NS; ++k) red[k][t] += red[k][t + s];
    __syncthreads();
  }
  if (t < NS) a.sums[q * NS + t] += red[t][0];
}

}  // namespace

hipError_t launch_error_sums(const ErrSumArgs& a, hipStream_t s) {
  if (a.nb <= 0 && a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_error_sums, dim3(E3GNN_ERR_QUANTITIES), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace e3gnn
