// Block-scaled W8A8 fp8 weight-streaming GEMM for decode batches on gfx950 (the DeepSeek-V3 / Qwen3 "-FP8" checkpoint
// format: e4m3fn weights with one fp32 scale per 128 x 128 block, e4m3fn activations with one fp32 scale per token and
// 128 input channels, fp8_block_quant.hip):
//   Y[m,n] = T( sum_b xs[m,b] * ws[n/128,b] * sum_{k in block b} Xq[m,k] * Wq[n,k] + bias[n] ),
// M <= 64 rows, fp32 throughout, one rounding to T (bf16 / f16).
//
// Instruction: v_mfma_f32_16x16x128_f8f6f4, both operands fp8, no scales in the matrix pipe: its scaled variant takes
// E8M0 (power-of-two) scales only, and these are arbitrary fp32.  One k-step is 128 k = exactly one scale block, so
// the step is
//   p = mfma(w, x, 0);  f = xs[m = c, step] * ws[tile / 8, step];  acc = fma(p, f, acc)
// -- a fresh-accumulator MFMA per (m-tile, step), then one v_mul and four v_fma on its 16 x 16 partial.  W is the A
// operand and X the B operand, so lane (g = lane >> 4, c = lane & 15) ends with four consecutive n of row m = c: its
// four accumulators share xs, and ws is wave-uniform per (n-tile, step) since a 16-row n-tile never straddles a
// 128-row scale row.  Both operands use the 8-register fp8 layout measured for mxfp4_gemm.hip: k
// 16 g .. + 15 of the step in the low four registers, k 64 + 16 g .. + 15 in the high four.
//
// Packed weight (lvllm_fp8_block_pack, a pure permutation, once at load time):
//   [N/16][K/128][lane 64][32 bytes]   lane (g, c) of unit (t, s) owns W[16 t + c][128 s + 16 g .. + 15] in its low 16
//                                      bytes and W[16 t + c][128 s + 64 + 16 g .. + 15] in its high 16
// Two b128 loads per lane and step, a wave's step is 2 contiguous KiB.  The scales stay in checkpoint order:
// ws [ceil(N/128)][K/128] fp32, xs [M][K/128] fp32.
//
// Organisation (the family's, int8_gemm.hip / mxfp4_gemm.hip): X fragments resident in registers, W from HBM to VGPR
// to the A operand with no LDS, the 8 waves of a workgroup split K (1, 2 or 4 steps each), their partial tiles meet in
// double-buffered LDS and are summed in wave order, summed tiles wait in an LDS stage and leave in bursts after the
// stream.  xs of the wave's steps is loaded once, beside the X fragments (MT x steps floats per lane).  ws of a tile's
// steps travels with the tile's weights: lane l loads ws[tile / 8][first step + (l & 3)] -- one dword load per tile --
// and v_readlane hands step s's factor to the multiply as a scalar, so nothing waits on it inside the loop.  K beyond
// 8 waves x 4 steps = 4096 is split over blockIdx.y into fp32 partials, which the reduce kernel sums in the fixed
// order 0, 1, 2 ...: a launch is reproducible.  Steps a wave does not own load zero weights, zero activations and zero
// scales (out-of-range buffer offsets) and contribute +0.
//
// Register budget (256 per lane at 2 waves per SIMD), sized at MT = 4 m-tiles and 4 steps per wave:
//   X fragments   MT * steps * 8   = 128
//   W in flight   TIF * steps * 8  =  32 at TIF = 1
//   acc, 2 x p    3 * MT * 4       =  48
//   xs            MT * steps       =  16
//   addresses, masks, epilogue     ~  30
// The step is software-pipelined (tile_steps): the MFMAs of step s + 1 are issued before the multiply and the FMAs of
// step s, two sets of partials.  The compiler reports 99 / 135 / 216 VGPRs at MT = 1 / 2 / 4 and TIF = 1 (132 / 169 /
// 254 at TIF = 2, -DLVLLM_F8B_TIF=2: the A/B is in profiles/fp8_block_gemm.md), no scratch anywhere, no static LDS.
// That holds only with the per-step scheduling barrier: without it all MT x 4 independent MFMAs of a tile are issued
// first, 64 registers of partials stay alive and the MT = 4 kernel spills 72 bytes per lane.  In the ISA a step reads
// MFMA(s + 1) x MT, v_mul, FMAs(s) (v_pk_fma_f32 pairs or v_fma_f32), also at MT = 1.
#include <stdlib.h>

#include "common.h"

namespace lvllm {
namespace {

typedef int fb_i32x4_t __attribute__((ext_vector_type(4)));
typedef int fb_i32x8_t __attribute__((ext_vector_type(8)));
typedef float fb_f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kFbWaves = 8;
constexpr int kFbSteps = 4;                      // k-steps of 128 a wave may own
constexpr unsigned kFbOutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kFbMaxK = 131072;
#ifndef LVLLM_F8B_TIF
#define LVLLM_F8B_TIF 1  // n-tiles in flight per wave
#endif
constexpr int kFbAux = 2;  // nt: weights are read once per launch

// T( acc[r] + bias[r] ) for four consecutive n of one row, packed for one 8-byte store
template <typename T>
__device__ __forceinline__ uint2 fb_epilogue(const fb_f32x4_t acc, const typename T::store_t* __restrict__ bias4) {
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) f[r] = bias4 != nullptr ? acc[r] + T::to_float(bias4[r]) : acc[r];
  uint2 o;
  o.x = (uint32_t)T::from_float(f[0]) | ((uint32_t)T::from_float(f[1]) << 16);
  o.y = (uint32_t)T::from_float(f[2]) | ((uint32_t)T::from_float(f[3]) << 16);
  return o;
}

// one n-tile of one wave in flight: its k-steps' weights, and in lane l the weight scale of step l & 3
struct FbSlot {
  fb_i32x8_t w[kFbSteps];
  float ws;
};

// TIF: n-tiles in flight per wave
template <typename T, int MT, int TIF>
__global__ __launch_bounds__(kFbWaves * 64, 2) void skinny_gemm_fp8_block_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const uint8_t* __restrict__ xq, const uint8_t* __restrict__ wq, const float* __restrict__ xs,
    const float* __restrict__ ws, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int steps_per_wave, const int ntiles, const int stage_tiles) {
  constexpr int KSTEPS = kFbSteps;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  fb_f32x4_t* red = reinterpret_cast<fb_f32x4_t*>(smem_raw);  // [2][waves][MT][64]

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int total_steps = K >> 7;
  const int step0 = (blockIdx.y * kFbWaves + wave) * steps_per_wave;  // first k-step of this wave
  int nvalid = total_steps - step0;                                   // k-steps that exist
  nvalid = nvalid < 0 ? 0 : (nvalid > steps_per_wave ? steps_per_wave : nvalid);

  // descriptors sized to the tensors exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K), 0x00020000);
  __amdgpu_buffer_rsrc_t sr =
      __builtin_amdgcn_make_buffer_rsrc((void*)ws, 0, ((N + 127) >> 7) * total_steps * 4, 0x00020000);
  const unsigned w_lane = (unsigned)(lane * 32) + (unsigned)step0 * 2048u;
  const unsigned w_tile = (unsigned)total_steps * 2048u;
  // lane l asks for the scale of the wave's step l & 3; steps the wave does not own read 0
  // (a mask ORed in after the row offset is added: an out-of-range constant added first could wrap back in range)
  const unsigned s_lane = (unsigned)(step0 + (lane & 3)) * 4u;
  const unsigned s_mask = (lane & 3) < nvalid ? 0u : ~0u;
  const unsigned s_row = (unsigned)total_steps * 4u;

  // n-tiles are handed out round-robin: local tile i is tile blockIdx.x + i * gridDim.x
  const int my_tiles = ntiles > (int)blockIdx.x ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  auto tile_of = [&](const int i) __attribute__((always_inline)) { return (int)(blockIdx.x + i * gridDim.x); };
  // wave-uniform masks through an empty asm, so that the selects stay selects (see skinny_gemm.hip)
  auto opaque = [](unsigned v) __attribute__((always_inline)) {
    v = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
    asm("" : "+s"(v));
    return v;
  };
  unsigned kmask[KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) kmask[s] = opaque(s < nvalid ? 0u : ~0u);

  // a slot: one n-tile over this wave's k-steps, up to KSTEPS x 2 loads of 1 KiB and one of 256 bytes per wave
  FbSlot wslot[TIF];
  auto load_unit = [&](FbSlot& a, const int i) __attribute__((always_inline)) {
    const unsigned tmask = opaque(i < my_tiles ? 0u : ~0u);
    const unsigned t = (unsigned)tile_of(i);
    const unsigned base = w_lane + t * w_tile;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const unsigned off = base + (unsigned)s * 2048u, mask = tmask | kmask[s];
      const fb_i32x4_t lo =
          __builtin_bit_cast(fb_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, off | mask, 0, kFbAux));
      const fb_i32x4_t hi =
          __builtin_bit_cast(fb_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, (off + 16u) | mask, 0, kFbAux));
      a.w[s] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    a.ws = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(sr, (s_lane + (t >> 3) * s_row) | tmask | s_mask, 0, 0));
  };

  fb_i32x8_t xf[MT][KSTEPS];
  float xsr[MT][KSTEPS];  // xs[16 mt + c][step0 + s]
  fb_f32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = fb_f32x4_t{0.f, 0.f, 0.f, 0.f};

  // output stage: summed tiles wait in LDS (fp32, 1 KiB per (tile, m-tile)) and leave in one burst, so that no store
  // sits between weight loads (vmcnt retires in issue order)
  fb_f32x4_t* stage = red + (size_t)2 * kFbWaves * MT * 64;  // [stage_tiles][MT][64]
  int stage_base = 0;
  auto store_slab = [&](const int i, const int mt, const fb_f32x4_t sum) __attribute__((always_inline)) {
    // lane (g, c): columns n = n0 + r of row m = 16 mt + c
    const int n0 = 16 * tile_of(i) + 4 * g;
    const int m = mt * 16 + c;
    if (m < M && n0 < N) {
      if (partial != nullptr)
        *reinterpret_cast<fb_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = sum;
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) = fb_epilogue<T>(sum, bias != nullptr ? bias + n0 : nullptr);
    }
  };
  auto flush_stage = [&](const int end_tile) __attribute__((always_inline)) {
    __syncthreads();  // every reducer's slab is in the stage
    const int nslabs = (end_tile - stage_base) * MT;
    for (int sl = wave; sl < nslabs; sl += kFbWaves)
      store_slab(stage_base + sl / MT, sl % MT, stage[(size_t)sl * 64 + lane]);
    stage_base = end_tile;
    __syncthreads();  // the stage may be overwritten again
  };
  auto finish_tile = [&](const int i) __attribute__((always_inline)) {
    if (i + 1 - stage_base > stage_tiles) flush_stage(i);          // uniform: make room first
    fb_f32x4_t* buf = red + (size_t)(i & 1) * kFbWaves * MT * 64;  // [wave][mt][lane]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      buf[(wave * MT + mt) * 64 + lane] = acc[mt];
      acc[mt] = fb_f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    for (int mt = wave; mt < MT; mt += kFbWaves) {
      fb_f32x4_t sum = buf[mt * 64 + lane];
#pragma unroll
      for (int w2 = 1; w2 < kFbWaves; ++w2) sum += buf[(w2 * MT + mt) * 64 + lane];  // wave order: fixed
      stage[((size_t)(i - stage_base) * MT + mt) * 64 + lane] = sum;
    }
  };

  // ---- X fragments and their scales, kept for the whole launch.  The wave's 512 bytes of a row are 32 chunks of 16
  // bytes, handled in two passes of 16 chunks (2 k-steps).  Read in ROW order (a row's chunks side by side over 16
  // lanes, 4 rows per wave-wide load), then turned into fragment order through a wave-private LDS scratch; chunk q of
  // row r sits at position q ^ r, which spreads both the row-order writes and the fragment-order reads over the banks.
  // Lane (g, c) of step s takes chunks 8 (s mod 2) + g and + 4 + g of row c: the fp8 operand's k 16 g .. and
  // 64 + 16 g .. .
  {
    fb_i32x4_t xc[MT][2 * KSTEPS];
    __amdgpu_buffer_rsrc_t xr =
        __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);
    __amdgpu_buffer_rsrc_t xsr_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, M * total_steps * 4, 0x00020000);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = i * 4 + g, q = c ^ r;  // row-order roles: g = row of the load, c = position in the row
          const int ks = h * 2 + (q >> 3), m = mt * 16 + r;
          const unsigned off = (m < M && ks < nvalid)
                                   ? (unsigned)((int64_t)m * ldx + (int64_t)step0 * 128 + h * 256 + q * 16)
                                   : kFbOutOfRange;
          xc[mt][h * 4 + i] = __builtin_bit_cast(fb_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
        }
    // the first TIF tiles follow the activations into the queue
#pragma unroll
    for (int j = 0; j < TIF; ++j) load_unit(wslot[j], j);
    char* xt = reinterpret_cast<char*>(stage + (size_t)stage_tiles * MT * 64) + wave * 4096;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<fb_i32x4_t*>(xt + i * 1024 + lane * 16) = xc[mt][h * 4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xc[mt][h * 4 + j] =
              *reinterpret_cast<const fb_i32x4_t*>(xt + c * 256 + (((8 * (j >> 1) + 4 * (j & 1) + g) ^ c) * 16));
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s)
        xf[mt][s] = __builtin_shufflevector(xc[mt][2 * s], xc[mt][2 * s + 1], 0, 1, 2, 3, 4, 5, 6, 7);
    // the scales last: 16 more registers during the transpose would not fit beside the first tile's weights
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s) {
        const int m = mt * 16 + c;
        const unsigned off = (m < M && s < nvalid) ? (unsigned)(m * total_steps + step0 + s) * 4u : kFbOutOfRange;
        xsr[mt][s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xsr_rsrc, off, 0, 0));
      }
  }

  // one n-tile, software-pipelined over its steps: the fresh-accumulator MFMAs of step s + 1 are issued BEFORE the
  // scale multiply and the FMAs of step s, so the matrix pipe works on the next block while the VALU folds the previous
  // partial in -- at every MT, also at MT = 1, where no second m-tile could cover the FMAs.  Two sets of partials,
  // 2 x MT x 4 registers.  Left alone, the scheduler issues all MT x 4 independent MFMAs of the tile first and keeps
  // 64 registers of partials alive, which spills at MT = 4: the empty asm pins a step's FMAs and the next step's MFMAs
  // in front of the scheduling barrier, which holds the window to those two sets.
  auto mfma_step = [&](const FbSlot& a, const int s, fb_f32x4_t (&p)[MT]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      p[mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.w[s], xf[mt][s], fb_f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0,
                                                               0, 0, 0);
  };
  auto tile_steps = [&](const FbSlot& a) __attribute__((always_inline)) {
    fb_f32x4_t p[2][MT];
    mfma_step(a, 0, p[0]);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      if (s + 1 < KSTEPS) {
        mfma_step(a, s + 1, p[(s + 1) & 1]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) asm volatile("" : "+v"(p[(s + 1) & 1][mt]));
      }
      const float wss = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a.ws), s));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const float f = xsr[mt][s] * wss;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][r] = __builtin_fmaf(p[s & 1][mt][r], f, acc[mt][r]);
        asm volatile("" : "+v"(acc[mt]));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // slot j holds local tile base + j; it is refilled with tile base + j + TIF as soon as it is consumed, so TIF tiles
  // stay in flight, also across the meetings.  Tiles past my_tiles load nothing and compute nothing.
  for (int base = 0; base < my_tiles; base += TIF) {
#pragma unroll
    for (int j = 0; j < TIF; ++j) {
      const int i = base + j;
      if (i < my_tiles) tile_steps(wslot[j]);  // uniform
      load_unit(wslot[j], i + TIF);
      if (i < my_tiles) finish_tile(i);  // uniform over the workgroup
    }
  }
  flush_stage(my_tiles);  // all weights have been streamed: now the stores
}

// y[m, n] = T(sum_s partial[s, m, n] + bias[n]), s ascending
template <typename T>
__global__ void fb_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                 const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                 const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  fb_f32x4_t sum = *reinterpret_cast<const fb_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const fb_f32x4_t*>(partial + (int64_t)s * MN + i);
  const int n = (int)(i % N);
  *reinterpret_cast<uint2*>(y + i) = fb_epilogue<T>(sum, bias != nullptr ? bias + n : nullptr);
}

// checkpoint order -> streaming order, one thread per 16 bytes: piece (lane, h) of unit (t, s) is
// W[16 t + c][128 s + 64 h + 16 g .. + 15]
__global__ void fp8_block_pack_kernel(uint4* __restrict__ w_packed, const uint4* __restrict__ wq, const int64_t pieces,
                                      const int K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pieces) return;
  const int steps = K >> 7;
  const int h = (int)i & 1, lane = (int)(i >> 1) & 63, g = lane >> 4, c = lane & 15;
  const int64_t unit = i >> 7;  // (n-tile, k-step)
  const int64_t t = unit / steps;
  const int s = (int)(unit - t * steps);
  w_packed[i] = wq[((16 * t + c) * (int64_t)K + 128 * s + 64 * h + 16 * g) >> 4];
}

template <typename T, int MT>
void launch_fb(void* y, float* partial, const void* xq, const void* wq, const float* xs, const float* ws,
               const void* bias, int M, int N, int K, int64_t ldx, int steps_per_wave, int ntiles, int groups,
               int ksplit, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr int TIF = LVLLM_F8B_TIF;
  const size_t red_bytes = (size_t)2 * kFbWaves * MT * 64 * sizeof(fb_f32x4_t);
  const size_t xt_bytes = (size_t)kFbWaves * 4096;  // the activation transpose's scratch
  // output stage: as many tiles as the workgroup owns, capped by what is left of the 160 KiB LDS
  int stage_tiles = (ntiles + groups - 1) / groups;
  const int cap = (int)((160 * 1024 - red_bytes - xt_bytes) / ((size_t)MT * 1024));
  if (stage_tiles > cap) stage_tiles = cap;
  if (stage_tiles < 1) stage_tiles = 1;
  const size_t smem = red_bytes + (size_t)stage_tiles * MT * 64 * sizeof(fb_f32x4_t) + xt_bytes;
  auto kern = skinny_gemm_fp8_block_kernel<T, MT, TIF>;
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kern, dim3(groups, ksplit), dim3(kFbWaves * 64), smem, stream, (S*)y, partial,
                     (const uint8_t*)xq, (const uint8_t*)wq, xs, ws, (const S*)bias, M, N, K, ldx, steps_per_wave,
                     ntiles, stage_tiles);
}

inline int fb_ksplit(int K) {
  const int cap = kFbWaves * kFbSteps;
  return (K / 128 + cap - 1) / cap;
}
inline bool fb_shape_ok(int N, int K) {
  return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0 && K < kFbMaxK && (int64_t)N * K < ((int64_t)1 << 32) - 16;
}
// gemm_balance (common.h Tuning): the fewest workgroups that need no more rounds of n-tiles than `cap` would
inline int fb_balanced_groups(int units, int cap) {
  if (cap < 1) cap = 1;
  if (units <= cap) return units < 1 ? 1 : units;
  if (!tuning().gemm_balance) return cap;
  const int rounds = (units + cap - 1) / cap;
  return (units + rounds - 1) / rounds;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int lvllm_fp8_block_pack(void* w_packed, const void* wq, int N, int K, void* stream) {
  if (!fb_shape_ok(N, K) || ((((uintptr_t)w_packed | (uintptr_t)wq) & 15) != 0)) {
    set_error("lvllm_fp8_block_pack: outside the envelope (N % 16 == 0, K % 128 == 0, K < 131072, N * K < 2^32 - 16, "
              "16-byte aligned tensors)");
    return 3;
  }
  const int64_t pieces = (int64_t)N * K / 16;
  hipLaunchKernelGGL(fp8_block_pack_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint4*)w_packed, (const uint4*)wq, pieces, K);
  LV_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t lvllm_skinny_gemm_w8a8_fp8_block_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || M > 64 || N <= 0 || K < 128) return 0;
  const int ksplit = fb_ksplit(K);
  return ksplit > 1 ? (int64_t)ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_skinny_gemm_w8a8_fp8_block(void* y, const void* xq, const void* w_packed, const float* xs,
                                                const float* ws, const void* bias, int M, int N, int K, int64_t ldx,
                                                int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(xs != nullptr && ws != nullptr, "xs [M, K/128] and ws [ceil(N/128), K/128] are device pointers");
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || M > 64 || !fb_shape_ok(N, K) || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) || ((((uintptr_t)xq | (uintptr_t)w_packed) & 15) != 0) ||
      ((((uintptr_t)xs | (uintptr_t)ws) & 3) != 0) || (((uintptr_t)y) & 7) != 0 || (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_skinny_gemm_w8a8_fp8_block: shape outside the kernel's envelope");
    return 3;
  }
  const int total_steps = K / 128;
  const int ksplit = fb_ksplit(K);
  const int steps_per_wave = total_steps <= kFbWaves ? 1 : (total_steps <= 2 * kFbWaves ? 2 : 4);
  const int ntiles = N / 16;
  const int cus = (ntiles >= tuning().gemm_wide_min_tiles && tuning().gemm_workgroups_wide > 0)
                      ? tuning().gemm_workgroups_wide
                      : tuning().gemm_workgroups;
  const int groups = fb_balanced_groups(ntiles, cus / ksplit);
  float* partial = nullptr;
  if (ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_skinny_gemm_w8a8_fp8_block_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  const int MT = (M + 15) / 16;
#define LV_FB_ARGS y, partial, xq, w_packed, xs, ws, bias, M, N, K, ldx, steps_per_wave, ntiles, groups, ksplit, s
#define LV_FB_MT(T_)                                  \
  switch (MT) {                                       \
    case 1: launch_fb<T_, 1>(LV_FB_ARGS); break;      \
    case 2: launch_fb<T_, 2>(LV_FB_ARGS); break;      \
    default: launch_fb<T_, 4>(LV_FB_ARGS); break;     \
  }
  if (dtype == LVLLM_BF16) { LV_FB_MT(BF16) } else { LV_FB_MT(F16) }
#undef LV_FB_MT
#undef LV_FB_ARGS
  LV_LAUNCH_CHECK();
  if (ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(fb_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, ksplit);
    else
      hipLaunchKernelGGL(fb_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
