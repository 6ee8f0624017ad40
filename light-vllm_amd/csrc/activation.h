// The elementwise arithmetic of the activation kernels (activation.hip), shared with the GEMM epilogues that fuse
// them (dense_tiled_gemm.hip): ONE definition each, so that a fused launch leaves the bits of the unfused sequence.
#pragma once

#include "common.h"

namespace lvllm {

// silu_and_mul, csrc/activation_kernels.cu:9-30 of the reference: the activation is rounded to T before the T x T
// multiply
template <typename T>
__device__ inline typename T::store_t silu_mul(typename T::store_t x, typename T::store_t y) {
  const float xf = T::to_float(x);
  const typename T::store_t a = T::from_float(xf / (1.0f + expf(-xf)));
  return T::from_float(T::to_float(a) * T::to_float(y));
}

// exact (erf) GELU in fp32: T(0.5 x (1 + erf(x / sqrt 2)))
template <typename T>
__device__ inline typename T::store_t gelu_erf(typename T::store_t x) {
  const float f = T::to_float(x);
  return T::from_float(f * 0.5f * (1.0f + erff(f * 0.70710678118654752440f)));
}

}  // namespace lvllm
