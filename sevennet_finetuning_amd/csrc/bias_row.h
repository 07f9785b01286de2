// e3nn o3.Linear(biases=True) (use_bias_in_linear), shared by the host sides of
// both engines (model_load.cpp, generic.cpp): the bias over the full output row -- b
// on the channels of every scalar (0e) output irrep, in output order, zero
// elsewhere.  `scalar(irrep)` says which irreps carry a bias; `name` is the
// tensor, for the error of a bias of the wrong size.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace e3gnn {

template <class IrrepsT, class Scalar>
std::vector<float> bias_row(const IrrepsT& out, Scalar scalar, const float* b, size_t numel,
                            const std::string& name) {
  size_t width = 0, nb = 0;
  for (auto& i : out) {
    width += (size_t)i.mul * (2 * i.l + 1);
    if (scalar(i)) nb += i.mul;
  }
  if (nb != numel)
    throw std::runtime_error("linear bias size mismatch: " + name + " has " + std::to_string(numel) +
                             " values, the output has " + std::to_string(nb) + " scalar channels");
  std::vector<float> v(width, 0.f);
  size_t off = 0, k = 0;
  for (auto& i : out) {
    if (scalar(i))
      for (int u = 0; u < i.mul; ++u) v[off + u] = b[k++];
    off += (size_t)i.mul * (2 * i.l + 1);
  }
  return v;
}

}  // namespace e3gnn
