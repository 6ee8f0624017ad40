// W4A16 (AWQ int4) dequantisation in registers, shared by the weight-streaming decode kernel (awq_gemm.hip) and the
// LDS-tiled prefill kernel (awq_tiled_gemm.hip): ONE definition of Wd[k,n] = T( float(q - z) * float(s) ), so that the
// two kernels and lvllm_awq_dequantize_packed produce the same bits.  The packed order and the arithmetic are described
// in the header of awq_gemm.hip.
#pragma once

#include "common.h"

namespace lvllm {

typedef __bf16 q_bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 q_f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 q_f16x2_t __attribute__((ext_vector_type(2)));
typedef float q_f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int q_u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int q_u32x2_t __attribute__((ext_vector_type(2)));

constexpr unsigned kW4OutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
#ifndef LVLLM_W4_AUX
#define LVLLM_W4_AUX 2  // nt: weights are read once per launch
#endif

// One group's scale and zero, prepared once, and the pair -> two T conversion
template <typename T>
struct W4Dequant;
template <>
struct W4Dequant<F16> {
  q_f16x2_t s2, nz2;  // {s, s} and {-(1024 + z)} x 2
  __device__ __forceinline__ explicit W4Dequant(const uint32_t m) {
    s2 = __builtin_bit_cast(q_f16x2_t, (m & 0xffffu) | (m << 16));
    const q_f16x2_t z2 = __builtin_bit_cast(q_f16x2_t, (m >> 16) | (m & 0xffff0000u));
    nz2 = -(z2 + q_f16x2_t{(_Float16)1024.f, (_Float16)1024.f});  // exact: z is an integer <= 15
  }
  __device__ __forceinline__ uint32_t pair(const uint32_t shifted) const {
    const q_f16x2_t h = __builtin_bit_cast(q_f16x2_t, (shifted & 0x000f000fu) | 0x64006400u);
    return __builtin_bit_cast(uint32_t, (h + nz2) * s2);
  }
};
template <>
struct W4Dequant<BF16> {
  float s, c;  // scale and -(128 + z) * s
  __device__ __forceinline__ explicit W4Dequant(const uint32_t m) {
    s = __builtin_bit_cast(float, m << 16);
    c = -((__builtin_bit_cast(float, m & 0xffff0000u) + 128.f) * s);
  }
  __device__ __forceinline__ uint32_t pair(const uint32_t shifted) const {
    const uint32_t h = (shifted & 0x000f000fu) | 0x43004300u;
    const float lo = __builtin_fmaf(__builtin_bit_cast(float, h << 16), s, c);
    const float hi = __builtin_fmaf(__builtin_bit_cast(float, h & 0xffff0000u), s, c);
    return (uint32_t)BF16::from_float(lo) | ((uint32_t)BF16::from_float(hi) << 16);
  }
};

// one packed word (8 nibbles of one row, 8 consecutive k) -> the lane's A fragment of one k-step
template <typename T>
__device__ __forceinline__ q_u32x4_t w4_dequant_word(const uint32_t w, const W4Dequant<T>& d) {
  return q_u32x4_t{d.pair(w), d.pair(w >> 4), d.pair(w >> 8), d.pair(w >> 12)};
}

template <typename T>
__device__ __forceinline__ q_f32x4_t w4_mfma(q_u32x4_t a, q_u32x4_t b, q_f32x4_t c);
template <>
__device__ __forceinline__ q_f32x4_t w4_mfma<BF16>(q_u32x4_t a, q_u32x4_t b, q_f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(q_bf16x8_t, a), __builtin_bit_cast(q_bf16x8_t, b),
                                                 c, 0, 0, 0);
}
template <>
__device__ __forceinline__ q_f32x4_t w4_mfma<F16>(q_u32x4_t a, q_u32x4_t b, q_f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(q_f16x8_t, a), __builtin_bit_cast(q_f16x8_t, b), c,
                                                0, 0, 0);
}

// the groups of one row and k-block: MW = 128 / G words in one load
template <int MW>
__device__ __forceinline__ void w4_load_meta(uint32_t (&m)[MW], __amdgpu_buffer_rsrc_t r, const unsigned off) {
  if constexpr (MW == 1) {
    m[0] = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, LVLLM_W4_AUX);
  } else if constexpr (MW == 2) {
    const q_u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, LVLLM_W4_AUX);
    m[0] = v.x; m[1] = v.y;
  } else {
    const q_u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, LVLLM_W4_AUX);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
  }
}

inline bool w4_group_ok(int G) { return G == 32 || G == 64 || G == 128; }

}  // namespace lvllm
