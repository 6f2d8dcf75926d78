// quantize_host.hpp -- the layer-0 input quantiser on the host (quantize_host.cpp; host code, no GPU
// call), shared by its definition and by engine.hip's rnnt_quantize_features_host.
#pragma once
#include <stdint.h>

namespace rnnt {

// out[i] = q8(x[i] * s) for i < n: any n >= 0, any alignment; x and out must not overlap
void quantize_features_host(const float* x, int64_t n, float s, int8_t* out);

}  // namespace rnnt
