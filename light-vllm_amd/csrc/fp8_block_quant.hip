// Per-token-group fp8 (OCP e4m3fn) activation quantisation for block-scaled W8A8 (fp8_block_gemm.hip): one fp32 scale
// per token and 128 consecutive input channels.
//   x [M, K] bf16 / f16, rows ldx elements apart, K % 128 == 0  ->  xq [M, K] e4m3fn, xs [M, K/128] fp32
// Arithmetic per group, in fp32 (fixed: tests demand bits):
//   s  = fmaxf(absmax, 1e-10f) / 448.0f             IEEE division; an all-zero group gets 1e-10 / 448 and zeros
//   xq = e4m3(fmaxf(-448, fminf(x / s, 448)))       the clamp of fp8_quant.hip: a NaN comes out as +448; absmax skips
//                                                   NaNs (fmaxf); round to nearest even by v_cvt_pk_fp8_f32
// Work split: 16 lanes own one group -- 8 elements per lane, one 16-byte load, one 8-byte store; the absmax meets
// inside the 16 lanes by four DPP row rotations (a DPP row IS 16 lanes): no LDS, no atomics.  Lane 0 of the group
// writes the scale.  The grid runs over all M * K / 128 groups, 16 per workgroup of 256 threads, so one row of
// K = 14336 already spreads over 7 workgroups.
#include "common.h"

namespace lvllm {
namespace {

// v rotated right by N lanes inside each row of 16
template <int N>
__device__ __forceinline__ float row_ror(const float v) {
  const int i = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x120 + N, 0xf, 0xf, false));
}

__device__ __forceinline__ uint32_t group_pack4(const float* f, const float s) {
  auto prep = [s](float v) { return fmaxf(-448.f, fminf(v / s, 448.f)); };
  const uint32_t w = __builtin_amdgcn_cvt_pk_fp8_f32(prep(f[0]), prep(f[1]), 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(prep(f[2]), prep(f[3]), w, true);
}

template <typename T>
__global__ __launch_bounds__(256) void per_token_group_fp8_quant_kernel(uint8_t* __restrict__ xq, float* __restrict__ xs,
                                                                        const typename T::store_t* __restrict__ x,
                                                                        const int64_t groups, const int groups_per_row,
                                                                        const int64_t ldx) {
  using S = typename T::store_t;
  const int64_t gid = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (gid >= groups) return;  // whole rows of 16 lanes leave together
  const int l = threadIdx.x & 15;
  const int64_t row = gid / groups_per_row;
  const int64_t col = (gid - row * groups_per_row) * 128 + l * 8;
  S v[8];
  *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(x + row * ldx + col);
  float f[8], m = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    f[k] = T::to_float(v[k]);
    m = fmaxf(m, fabsf(f[k]));
  }
  m = fmaxf(m, row_ror<8>(m));
  m = fmaxf(m, row_ror<4>(m));
  m = fmaxf(m, row_ror<2>(m));
  m = fmaxf(m, row_ror<1>(m));
  const float s = fmaxf(m, 1e-10f) / 448.0f;
  *reinterpret_cast<uint2*>(xq + row * (int64_t)groups_per_row * 128 + col) = uint2{group_pack4(f, s), group_pack4(f + 4, s)};
  if (l == 0) xs[gid] = s;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int lvllm_per_token_group_fp8_quant(void* xq, float* xs, const void* x, int64_t M, int K, int64_t ldx,
                                               int dtype, void* stream) {
  LV_CHECK(M >= 0 && K > 0 && K % 128 == 0, "K must be a positive multiple of the 128-channel group");
  LV_CHECK(dtype == LVLLM_BF16 || dtype == LVLLM_F16, "x is bf16 or f16");
  LV_CHECK(ldx >= K && ldx % 8 == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)xq) & 7) == 0 && (((uintptr_t)xs) & 3) == 0,
           "rows of x 16-byte aligned (ldx % 8 == 0), xq 8-byte and xs 4-byte aligned");
  if (M == 0) return 0;
  const int gpr = K / 128;
  const int64_t groups = M * gpr;
  LV_CHECK((groups + 15) / 16 < ((int64_t)1 << 31), "too many groups for one launch");
  const dim3 grid((unsigned)((groups + 15) / 16));
  if (dtype == LVLLM_BF16)
    hipLaunchKernelGGL(per_token_group_fp8_quant_kernel<BF16>, grid, dim3(256), 0, (hipStream_t)stream, (uint8_t*)xq, xs,
                       (const uint16_t*)x, groups, gpr, ldx);
  else
    hipLaunchKernelGGL(per_token_group_fp8_quant_kernel<F16>, grid, dim3(256), 0, (hipStream_t)stream, (uint8_t*)xq, xs,
                       (const uint16_t*)x, groups, gpr, ldx);
  LV_LAUNCH_CHECK();
  return 0;
}
