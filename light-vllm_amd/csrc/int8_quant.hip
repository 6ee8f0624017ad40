// int8 activation quantisation: static_scaled_int8_quant (one per-tensor scale) and dynamic_scaled_int8_quant (one
// scale per token) -- the operators of csrc/quantization/compressed_tensors/int8_quant_kernels.cu of the reference,
// which feed the W8A8 int8 GEMM (int8_gemm.hip).  Arithmetic, all fp32 and correctly rounded:
//   static:   q = sat_i8(rint(float(x) / scale))
//   dynamic:  a = max |x| over the row, scale = a / 127.0f, q = sat_i8(rint(float(x) * (127.0f / a)))
// rint rounds halves to even (v_rndne_f32), sat_i8 clamps to [-128, 127].  An all-zero row gives scale 0 and zeros
// (the reference divides 127 by 0 there and stores NaN-derived bytes).
//
// Organisation: a workgroup of 256 threads; TPR threads serve one row -- 64 (one wave per row, four rows per
// workgroup, the maximum by wave reduction alone) up to H = 1024, otherwise all 256 (wave reduction plus ONE exchange
// of four floats through LDS).  16-byte loads, 8- or 4-byte stores.  A thread keeps its first kVecs = 8 vectors of
// the row in registers between the two passes (maximum, then quantise): the dynamic kernel reads a row from memory
// ONCE up to H = 256 * 8 * 8 = 16384 elements of f16 / bf16 (8192 of f32; 4096 / 2048 in the wave-per-row form, which
// is only chosen far below that); vectors beyond are read again in the second pass.  Rows whose bytes are no multiple
// of 16 (or unaligned tensors) take the scalar loops, which read twice as well.
#include "common.h"

namespace lvllm {
namespace {

constexpr int kQuantThreads = 256;
constexpr int kVecs = 8;  // 16-byte vectors of a row that one thread keeps in registers

__device__ __forceinline__ int sat_i8(const float v) {  // v is integral already
  return (int)fmaxf(-128.f, fminf(v, 127.f));
}
// DIV: q = rint(x / s) with the IEEE quotient (static); otherwise q = rint(x * s) (dynamic, s = 127 / a)
template <bool DIV>
__device__ __forceinline__ int quant_one(const float x, const float s) {
  return sat_i8(__builtin_rintf(DIV ? __fdiv_rn(x, s) : x * s)) & 0xff;
}

template <typename T, bool DIV>
__device__ __forceinline__ void quant_store_vec(int8_t* __restrict__ out, const uint4 v, const float s) {
  using S = typename T::store_t;
  constexpr int X = 16 / sizeof(S);
  S e[X];
  *reinterpret_cast<uint4*>(e) = v;
  uint32_t w[X / 4];
#pragma unroll
  for (int k = 0; k < X / 4; ++k)
    w[k] = (uint32_t)quant_one<DIV>(T::to_float(e[4 * k]), s) | ((uint32_t)quant_one<DIV>(T::to_float(e[4 * k + 1]), s) << 8) |
           ((uint32_t)quant_one<DIV>(T::to_float(e[4 * k + 2]), s) << 16) |
           ((uint32_t)quant_one<DIV>(T::to_float(e[4 * k + 3]), s) << 24);
  if constexpr (X == 8) *reinterpret_cast<uint2*>(out) = uint2{w[0], w[1]};
  else *reinterpret_cast<uint32_t*>(out) = w[0];
}

template <typename T>
__device__ __forceinline__ float absmax_vec(const uint4 v) {
  using S = typename T::store_t;
  constexpr int X = 16 / sizeof(S);
  S e[X];
  *reinterpret_cast<uint4*>(e) = v;
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < X; ++k) m = fmaxf(m, fabsf(T::to_float(e[k])));
  return m;
}

// DYNAMIC: scales[row] is written; otherwise *scales is the one static scale.
template <typename T, int TPR, bool DYNAMIC>
__global__ __launch_bounds__(kQuantThreads) void int8_quant_kernel(int8_t* __restrict__ out, float* __restrict__ scales,
                                                                   const typename T::store_t* __restrict__ in,
                                                                   const int64_t rows, const int H, const bool vec_ok) {
  using S = typename T::store_t;
  constexpr int X = 16 / sizeof(S);
  constexpr int RPB = kQuantThreads / TPR;  // rows per workgroup
  __shared__ float red[kQuantThreads / 64];
  const int t = threadIdx.x % TPR;
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
  const bool live = row < rows;  // a whole wave at a time (TPR is a multiple of 64): no divergence inside a wave
  const S* src = in + (live ? row : 0) * H;
  int8_t* dst = out + (live ? row : 0) * H;
  const int nvec = (vec_ok && live) ? H / X : 0;
  const int nscalar = live ? H : 0;

  uint4 keep[kVecs];
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    const int i = j * TPR + t;
    keep[j] = i < nvec ? reinterpret_cast<const uint4*>(src)[i] : uint4{0u, 0u, 0u, 0u};
  }
  float s;
  if constexpr (DYNAMIC) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < kVecs; ++j) m = fmaxf(m, absmax_vec<T>(keep[j]));
    for (int i = kVecs * TPR + t; i < nvec; i += TPR) m = fmaxf(m, absmax_vec<T>(reinterpret_cast<const uint4*>(src)[i]));
    for (int i = nvec * X + t; i < nscalar; i += TPR) m = fmaxf(m, fabsf(T::to_float(src[i])));
    m = wave_max(m);
    if constexpr (TPR > 64) {  // the one exchange: every wave's maximum to every thread
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kQuantThreads / 64; ++w) m = fmaxf(m, red[w]);
    }
    if (live && t == 0) scales[row] = __fdiv_rn(m, 127.0f);
    s = m > 0.f ? __fdiv_rn(127.0f, m) : 0.f;  // all-zero row: zeros, not 0 * inf
  } else {
    s = *scales;
  }
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    const int i = j * TPR + t;
    if (i < nvec) quant_store_vec<T, !DYNAMIC>(dst + (int64_t)i * X, keep[j], s);
  }
  for (int i = kVecs * TPR + t; i < nvec; i += TPR)
    quant_store_vec<T, !DYNAMIC>(dst + (int64_t)i * X, reinterpret_cast<const uint4*>(src)[i], s);
  for (int i = nvec * X + t; i < nscalar; i += TPR) dst[i] = (int8_t)quant_one<!DYNAMIC>(T::to_float(src[i]), s);
}

template <bool DYNAMIC>
int launch_int8_quant(void* out, float* scales, const void* input, int64_t rows, int H, int dtype, void* stream) {
  LV_CHECK(rows >= 0 && H > 0, "bad sizes");
  if (rows == 0) return 0;
  const int esize = dtype == LVLLM_F32 ? 4 : 2;
  // every row starts on a 16-byte boundary of the input and an 8-byte one of the output
  const bool vec_ok = (((uintptr_t)input & 15) == 0) && (((uintptr_t)out & 7) == 0) && ((int64_t)H * esize) % 16 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (H <= 1024) {
    const int64_t grid = (rows + 3) / 4;
    LV_CHECK(grid < ((int64_t)1 << 31), "too many rows");
    LV_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((int8_quant_kernel<scalar_t, 64, DYNAMIC>), dim3((unsigned)grid),
                                                dim3(kQuantThreads), 0, s, (int8_t*)out, scales,
                                                (const typename scalar_t::store_t*)input, rows, H, vec_ok));
  } else {
    LV_CHECK(rows < ((int64_t)1 << 31), "too many rows");
    LV_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((int8_quant_kernel<scalar_t, kQuantThreads, DYNAMIC>),
                                                dim3((unsigned)rows), dim3(kQuantThreads), 0, s, (int8_t*)out, scales,
                                                (const typename scalar_t::store_t*)input, rows, H, vec_ok));
  }
  LV_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int lvllm_static_scaled_int8_quant(void* out, const void* input, const float* scale, int64_t num_tokens,
                                              int hidden_size, int dtype, void* stream) {
  LV_CHECK(scale != nullptr, "scale is a device pointer to one float");
  return launch_int8_quant<false>(out, const_cast<float*>(scale), input, num_tokens, hidden_size, dtype, stream);
}

extern "C" int lvllm_dynamic_scaled_int8_quant(void* out, float* scales, const void* input, int64_t num_tokens,
                                               int hidden_size, int dtype, void* stream) {
  LV_CHECK(scales != nullptr, "scales is a device pointer to num_tokens floats");
  return launch_int8_quant<true>(out, scales, input, num_tokens, hidden_size, dtype, stream);
}
