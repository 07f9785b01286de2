// The activation of the FCN readout (FCN_e3nn, nn/linear.py:94-129), shared by
// the generic engine's k_gen_fcn_act (generic.hip) and the fused engine's
// k_readout_fcn (node.hip): f(z) and f'(z) of e3nn FullyConnectedNet's
// activation; the caller multiplies both by c = normalize2mom(f) (the
// manifest's readout.act_norm).
// kind: 0 relu, 1 silu, 2 tanh, 3 sigmoid, 4 abs, 5 elu (sevenn/_const.py ACTIVATION)
#pragma once
#include <hip/hip_runtime.h>

namespace e3gnn {

constexpr int FCN_ACT_KINDS = 6;
inline const char* const* fcn_act_names() {
  static const char* const names[FCN_ACT_KINDS] = {"relu", "silu", "tanh", "sigmoid", "abs", "elu"};
  return names;
}

__device__ __forceinline__ void fcn_act(int kind, float z, float& f, float& df) {
  switch (kind) {
    case 0: f = z > 0.f ? z : 0.f; df = z > 0.f ? 1.f : 0.f; break;
    case 1: {
      const float sg = 1.f / (1.f + __expf(-z));
      f = z * sg;
      df = sg * (1.f + z * (1.f - sg));
      break;
    }
    case 2: {
      const float t = tanhf(z);
      f = t;
      df = 1.f - t * t;
      break;
    }
    case 3: {
      const float sg = 1.f / (1.f + __expf(-z));
      f = sg;
      df = sg * (1.f - sg);
      break;
    }
    case 4: f = fabsf(z); df = z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f); break;
    default: f = z > 0.f ? z : expm1f(z); df = z > 0.f ? 1.f : __expf(z); break;
  }
}

// f''(z), for the fine-tune step's dual reverse of the readout (fcn_train.hip)
__device__ __forceinline__ float fcn_act2(int kind, float z) {
  switch (kind) {
    case 0: return 0.f;
    case 1: {
      const float sg = 1.f / (1.f + __expf(-z));
      return sg * (1.f - sg) * (2.f + z * (1.f - 2.f * sg));
    }
    case 2: {
      const float t = tanhf(z);
      return -2.f * t * (1.f - t * t);
    }
    case 3: {
      const float sg = 1.f / (1.f + __expf(-z));
      return sg * (1.f - sg) * (1.f - 2.f * sg);
    }
    case 4: return 0.f;
    default: return z > 0.f ? 0.f : __expf(z);
  }
}

}  // namespace e3gnn
