// W8A8 int8 weight-streaming GEMM for decode batches on gfx950 (the compressed-tensors / SmoothQuant scheme):
//   Y[M,N] = T( sx[m] * (sw[n] * float(acc[m,n])) + bias[n] ),  acc = Xq . Wq^T in int32,
// M <= 64 rows, Xq int8 [M, K] quantised beforehand (int8_quant.hip), one fp32 scale per token (sx) and one per
// output channel (sw); the two products are fp32 multiplications in this order (the weight scale first), the bias is
// a separate fp32 add, T is bf16 / f16.
//
// Instruction: v_mfma_i32_16x16x64_i8 -- 16 bytes per lane and operand, 64 k per instruction, int32 accumulators.  A
// k-step is therefore 64 k = 64 bytes of a weight row, and ONE 16-byte weight load is ONE MFMA per m-tile (the fp8
// variant of skinny_gemm.hip needs two 32-k instructions per load).
//
// Weight layout (int8_pack = lvllm_pack_weight on the [N, K/2] 16-bit view of the bytes): [N/16][K/64][lane 64][16
// bytes], one contiguous KiB per (n-tile, k-step); lane (g = lane >> 4, c = lane & 15) owns Wq[16 t + c][64 s + 16 g
// .. + 15].  X fragments are built in the same order -- lane (g, c) of m-tile mt holds Xq[16 mt + c][64 s + 16 g .. +
// 15] -- so W and X agree on which k sits in which byte of a lane's operand, which is all the contraction needs.
//
// Organisation (the family's, skinny_gemm.hip / awq_gemm.hip): X fragments resident in registers as the B operand, W
// from HBM to VGPR to the A operand with no LDS, the 8 waves of a workgroup split K, their partial tiles meet in
// double-buffered LDS, summed tiles wait in an LDS stage and leave in bursts after the stream.  X needs no arithmetic:
// row-order loads (whole row segments, all in flight at once), a wave-private LDS transpose, fragments.
//
// Exactness: every partial sum -- per k-step, per wave (the LDS meeting), per workgroup (the workspace when K is
// split over blockIdx.y) -- is an int32, |acc| <= K * 2^14 < 2^31 for K < 131072 (the envelope).  The reduce kernel
// sums int32 and only then applies the epilogue, so the result does not depend on how K was split.
//
// Register budget (256 per lane at 2 waves per SIMD), sized at MT = 4 m-tiles:
//   X fragments   MT * KSTEPS * 4   = 128 at KSTEPS = 8   (64 at KSTEPS = 4)
//   W in flight   TIF * KSTEPS * 4  =  32 at TIF = 1, 64 at TIF = 2  (8 / 16 loads of 1 KiB per wave)
//   accumulators  NT * MT * 4       =  16
//   addresses, masks, epilogue      ~  40   (the compiler reports 200 / 232 registers at TIF = 1 / 2, no spill)
// KSTEPS = 16 would put 256 registers of X alone at MT = 4; KSTEPS = 8 with three tiles in flight is 240 before any
// address.  So a wave owns at most 8 k-steps (512 k; a workgroup 4096 k, beyond that K is split over workgroups); a
// launch whose waves own at most 4 k-steps takes the KSTEPS = 4 variant with twice the tiles in flight (the same
// number of loads).  Both depths fit; measured (profiles/int8_gemm.md), 8 loads in flight per wave (64 KiB per CU)
// beat 16 on the large shapes by 2-5 %, and 4 k-steps per wave lose 5-15 % to 8, so the default is 8 steps and 8
// loads.  LVLLM_I8_STEPS=4 and LVLLM_I8_INFLIGHT=16 select the alternatives for A/B runs.
#include <stdlib.h>

#include "common.h"

namespace lvllm {
namespace {

typedef int i8_i32x4_t __attribute__((ext_vector_type(4)));
typedef float i8_f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kI8Waves = 8;
constexpr unsigned kI8OutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kI8MaxK = 131072;                  // K below this: no int32 overflow whatever the operands
#ifndef LVLLM_I8_AUX
#define LVLLM_I8_AUX 2  // nt: weights are read once per launch
#endif

// T( sx * (sw[r] * float(acc[r])) + bias[r] ) for four consecutive n of one row, packed for one 8-byte store
template <typename T>
__device__ __forceinline__ uint2 i8_epilogue(const i8_i32x4_t acc, const float sxm, const float* __restrict__ sw4,
                                             const typename T::store_t* __restrict__ bias4) {
  const i8_f32x4_t w = *reinterpret_cast<const i8_f32x4_t*>(sw4);
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    f[r] = sxm * (w[r] * (float)acc[r]);
    if (bias4 != nullptr) f[r] += T::to_float(bias4[r]);
  }
  uint2 o;
  o.x = (uint32_t)T::from_float(f[0]) | ((uint32_t)T::from_float(f[1]) << 16);
  o.y = (uint32_t)T::from_float(f[2]) | ((uint32_t)T::from_float(f[3]) << 16);
  return o;
}

// KSTEPS: k-steps of 64 a wave may own (its X fragments: MT * KSTEPS * 4 registers); TIF: n-tiles in flight per wave.
template <typename T, int MT, int KSTEPS, int TIF>
__global__ __launch_bounds__(kI8Waves * 64, 2) void skinny_gemm_i8_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    int* __restrict__ partial,            // [ksplit, M, N]  (ksplit > 1)
    const int8_t* __restrict__ xq, const int8_t* __restrict__ wq, const float* __restrict__ sx,
    const float* __restrict__ sw, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int steps_per_wave, const int ntiles, const int stage_tiles) {
  constexpr int NT = (MT == 1 && TIF % 2 == 0) ? 2 : 1;  // n-tiles accumulated between two wave meetings
  constexpr int HALF = KSTEPS / 2;
  static_assert(KSTEPS == 4 || KSTEPS == 8, "the transpose below handles rows of 8 or 16 chunks per pass");
  static_assert(TIF % NT == 0, "a meeting falls on a slot boundary");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  i8_i32x4_t* red = reinterpret_cast<i8_i32x4_t*>(smem_raw);  // [2][waves][NT * MT][64]

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int total_steps = K >> 6;
  const int step0 = (blockIdx.y * kI8Waves + wave) * steps_per_wave;  // first k-step of this wave
  int nvalid = total_steps - step0;                                   // k-steps that exist
  nvalid = nvalid < 0 ? 0 : (nvalid > steps_per_wave ? steps_per_wave : nvalid);

  // descriptor sized to the packed weight exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K), 0x00020000);
  const unsigned w_lane = (unsigned)(lane * 16) + (unsigned)step0 * 1024u;
  const unsigned w_tile = (unsigned)total_steps * 1024u;

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

  // a slot: one n-tile over this wave's k-steps, KSTEPS loads of 1 KiB per wave
  i8_i32x4_t wslot[TIF][KSTEPS];
  auto load_unit = [&](i8_i32x4_t (&a)[KSTEPS], const int i) __attribute__((always_inline)) {
    const unsigned tmask = opaque(i < my_tiles ? 0u : ~0u);
    const unsigned base = w_lane + (unsigned)tile_of(i) * w_tile;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
      a[s] = __builtin_bit_cast(i8_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                wr, (base + (unsigned)s * 1024u) | tmask | kmask[s], 0, LVLLM_I8_AUX));
  };

  i8_i32x4_t xf[MT][KSTEPS];
  i8_i32x4_t acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = i8_i32x4_t{0, 0, 0, 0};
  const int ngroups = (my_tiles + NT - 1) / NT;

  // output stage: summed tiles wait in LDS (int32, 1 KiB per (tile, m-tile)) and leave in one burst, so that no store
  // sits between weight loads (vmcnt retires in issue order)
  i8_i32x4_t* stage = red + (size_t)2 * kI8Waves * NT * MT * 64;  // [stage_tiles][MT][64]
  int stage_base = 0;
  auto store_slab = [&](const int i, const int mt, const i8_i32x4_t sum) __attribute__((always_inline)) {
    // lane (g, c): columns n = n0 + r of row m = 16 mt + c
    const int n0 = 16 * tile_of(i) + 4 * g;
    const int m = mt * 16 + c;
    if (m < M && n0 < N) {
      if (partial != nullptr)
        *reinterpret_cast<i8_i32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = sum;
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) =
            i8_epilogue<T>(sum, sx[m], sw + n0, bias != nullptr ? bias + n0 : nullptr);
    }
  };
  auto flush_stage = [&](const int end_tile) __attribute__((always_inline)) {
    __syncthreads();  // every reducer's slab is in the stage
    const int nslabs = (end_tile - stage_base) * MT;
    for (int sl = wave; sl < nslabs; sl += kI8Waves)
      store_slab(stage_base + sl / MT, sl % MT, stage[(size_t)sl * 64 + lane]);
    stage_base = end_tile;
    __syncthreads();  // the stage may be overwritten again
  };
  auto finish_group = [&](const int grp) __attribute__((always_inline)) {
    if ((grp + 1) * NT - stage_base > stage_tiles) flush_stage(grp * NT);  // uniform: make room first
    i8_i32x4_t* buf = red + (size_t)(grp & 1) * kI8Waves * NT * MT * 64;    // [wave][slab = j * MT + mt][lane]
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        buf[(wave * NT * MT + j * MT + mt) * 64 + lane] = acc[j][mt];
        acc[j][mt] = i8_i32x4_t{0, 0, 0, 0};
      }
    __syncthreads();
    for (int slab = wave; slab < NT * MT; slab += kI8Waves) {
      const int j = slab / MT, mt = slab - j * MT;
      const int i = grp * NT + j;
      if (i >= my_tiles) continue;
      i8_i32x4_t sum = buf[slab * 64 + lane];
#pragma unroll
      for (int w2 = 1; w2 < kI8Waves; ++w2) sum += buf[(w2 * NT * MT + slab) * 64 + lane];  // int32: exact
      stage[((size_t)(i - stage_base) * MT + mt) * 64 + lane] = sum;
    }
  };

  // ---- X fragments, kept for the whole launch.  Read in ROW order (a row's 16-byte chunks side by side over the
  // lanes), then turned into fragment order through a wave-private LDS scratch; chunk q of row r sits at position
  // q ^ (r mod NCH), which spreads both the row-order writes and the fragment-order reads over the banks.
  {
    constexpr int NCH = HALF * 4;  // 16-byte chunks of one row in one pass (4 per k-step)
    constexpr int RPI = 64 / NCH;  // rows per wave-wide load
    __amdgpu_buffer_rsrc_t xr =
        __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);
    const int b = lane / NCH, pos = lane % NCH;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
          const int r = i * RPI + b, q = pos ^ (r & (NCH - 1));
          const int ks = h * HALF + (q >> 2), m = mt * 16 + r;
          const unsigned off = (m < M && ks < nvalid)
                                   ? (unsigned)((int64_t)m * ldx + (int64_t)(step0 + ks) * 64 + (q & 3) * 16)
                                   : kI8OutOfRange;
          xf[mt][h * HALF + i] = __builtin_bit_cast(i8_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
        }
    // the first TIF tiles follow the activations into the queue
#pragma unroll
    for (int j = 0; j < TIF; ++j) load_unit(wslot[j], j);
    char* xs = reinterpret_cast<char*>(stage + (size_t)stage_tiles * MT * 64) + wave * (16 * NCH * 16);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < HALF; ++i)
          *reinterpret_cast<i8_i32x4_t*>(xs + i * 1024 + lane * 16) = xf[mt][h * HALF + i];
#pragma unroll
        for (int s2 = 0; s2 < HALF; ++s2)
          xf[mt][h * HALF + s2] =
              *reinterpret_cast<const i8_i32x4_t*>(xs + c * (NCH * 16) + (((4 * s2 + g) ^ (c & (NCH - 1))) * 16));
      }
  }

  // slot j holds local tile base + j; it is refilled with tile base + j + TIF as soon as it is consumed, so TIF tiles
  // stay in flight, also across the meetings.  Tiles past my_tiles load nothing and compute nothing.
  for (int base = 0; base < ngroups * NT; base += TIF) {
#pragma unroll
    for (int j = 0; j < TIF; ++j) {
      const int i = base + j;
      if (i < my_tiles) {  // uniform
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[j % NT][mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wslot[j][s], xf[mt][s], acc[j % NT][mt], 0, 0, 0);
      }
      load_unit(wslot[j], i + TIF);
      if (j % NT == NT - 1 && i / NT < ngroups) finish_group(i / NT);  // uniform over the workgroup
    }
  }
  flush_stage(my_tiles);  // all weights have been streamed: now the stores
}

// y[m, n] = epilogue(sum_s partial[s, m, n]): the int32 sum first, the scales after
template <typename T>
__global__ void i8_reduce_kernel(typename T::store_t* __restrict__ y, const int* __restrict__ partial,
                                 const float* __restrict__ sx, const float* __restrict__ sw,
                                 const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                 const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  i8_i32x4_t sum = *reinterpret_cast<const i8_i32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const i8_i32x4_t*>(partial + (int64_t)s * MN + i);
  const int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
  *reinterpret_cast<uint2*>(y + i) = i8_epilogue<T>(sum, sx[m], sw + n, bias != nullptr ? bias + n : nullptr);
}

template <typename T, int MT, int KSTEPS, int TIF>
void launch_i8(void* y, int* partial, const void* xq, const void* wq, const float* sx, const float* sw,
               const void* bias, int M, int N, int K, int64_t ldx, int steps_per_wave, int ntiles, int groups,
               int ksplit, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr int NT = (MT == 1 && TIF % 2 == 0) ? 2 : 1;
  const size_t red_bytes = (size_t)2 * kI8Waves * NT * MT * 64 * sizeof(i8_i32x4_t);
  const size_t xs_bytes = (size_t)kI8Waves * 16 * (KSTEPS / 2) * 64;  // the activation transpose's scratch
  // output stage: as many tiles as the workgroup owns, capped by what is left of the 160 KiB LDS
  int stage_tiles = (((ntiles + groups - 1) / groups + NT - 1) / NT) * NT;
  const int cap = (int)((160 * 1024 - red_bytes - xs_bytes) / ((size_t)MT * 1024) / NT) * NT;
  if (stage_tiles > cap) stage_tiles = cap;
  if (stage_tiles < NT) stage_tiles = NT;
  const size_t smem = red_bytes + (size_t)stage_tiles * MT * 64 * sizeof(i8_i32x4_t) + xs_bytes;
  auto kern = skinny_gemm_i8_kernel<T, MT, KSTEPS, TIF>;
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kern, dim3(groups, ksplit), dim3(kI8Waves * 64), smem, stream, (S*)y, partial,
                     (const int8_t*)xq, (const int8_t*)wq, sx, sw, (const S*)bias, M, N, K, ldx, steps_per_wave, ntiles,
                     stage_tiles);
}

// k-steps of 64 one wave may own (file header); LVLLM_I8_STEPS=4 halves it for A/B runs
inline int i8_max_steps_per_wave() {
  static const int forced = getenv("LVLLM_I8_STEPS") ? atoi(getenv("LVLLM_I8_STEPS")) : 0;
  return forced == 4 ? 4 : 8;
}
// weight loads (of 1 KiB per wave) in flight per wave: 8 by measurement, or 16 with LVLLM_I8_INFLIGHT=16
inline int i8_loads_in_flight() {
  static const int forced = getenv("LVLLM_I8_INFLIGHT") ? atoi(getenv("LVLLM_I8_INFLIGHT")) : 0;
  return forced == 16 ? 16 : 8;
}
inline int i8_ksplit(int K) {
  const int cap = kI8Waves * i8_max_steps_per_wave();
  return (K / 64 + cap - 1) / cap;
}
// gemm_balance (common.h Tuning): the fewest workgroups that need no more rounds of n-tiles than `cap` would
inline int i8_balanced_groups(int units, int cap) {
  if (cap < 1) cap = 1;
  if (units <= cap) return units < 1 ? 1 : units;
  if (!tuning().gemm_balance) return cap;
  const int rounds = (units + cap - 1) / cap;
  return (units + rounds - 1) / rounds;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_skinny_gemm_w8a8_int8_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || M > 64 || N <= 0 || K < 64) return 0;
  const int ksplit = i8_ksplit(K);
  return ksplit > 1 ? (int64_t)ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_skinny_gemm_w8a8_int8(void* y, const void* x_q, const void* w_packed, const float* x_scale,
                                           const float* w_scale, const void* bias, int M, int N, int K, int64_t ldx,
                                           int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(x_scale != nullptr && w_scale != nullptr, "x_scale [M] and w_scale [N] are device pointers");
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || M > 64 || K <= 0 || K >= kI8MaxK || (K % 64) != 0 ||
      (N % 16) != 0 || (int64_t)N * K >= ((int64_t)1 << 32) - 16 || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) ||
      ((((uintptr_t)x_q | (uintptr_t)w_packed | (uintptr_t)w_scale) & 15) != 0) || (((uintptr_t)y) & 7) != 0 ||
      (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_skinny_gemm_w8a8_int8: shape outside the kernel's envelope");
    return 3;
  }
  const int total_steps = K / 64;
  const int ksplit = i8_ksplit(K);
  const int steps_per_wg = (total_steps + ksplit - 1) / ksplit;
  const int steps_per_wave = (steps_per_wg + kI8Waves - 1) / kI8Waves;  // <= i8_max_steps_per_wave()
  const int ntiles = N / 16;
  const int cus = (ntiles >= tuning().gemm_wide_min_tiles && tuning().gemm_workgroups_wide > 0)
                      ? tuning().gemm_workgroups_wide
                      : tuning().gemm_workgroups;
  const int groups = i8_balanced_groups(ntiles, cus / ksplit);
  int* partial = nullptr;
  if (ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_skinny_gemm_w8a8_int8_workspace_bytes)");
    partial = (int*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  const int MT = (M + 15) / 16;
  const bool k4 = steps_per_wave <= 4;
  const bool deep = i8_loads_in_flight() == 16;
#define LV_I8_ARGS y, partial, x_q, w_packed, x_scale, w_scale, bias, M, N, K, ldx, steps_per_wave, ntiles, groups, ksplit, s
#define LV_I8(T_, MT_)                                                   \
  do {                                                                   \
    if (k4) {                                                            \
      if (deep) launch_i8<T_, MT_, 4, 4>(LV_I8_ARGS); else launch_i8<T_, MT_, 4, 2>(LV_I8_ARGS); \
    } else {                                                             \
      if (deep) launch_i8<T_, MT_, 8, 2>(LV_I8_ARGS); else launch_i8<T_, MT_, 8, 1>(LV_I8_ARGS); \
    }                                                                    \
  } while (0)
#define LV_I8_MT(T_)               \
  switch (MT) {                    \
    case 1: LV_I8(T_, 1); break;   \
    case 2: LV_I8(T_, 2); break;   \
    default: LV_I8(T_, 4); break;  \
  }
  if (dtype == LVLLM_BF16) { LV_I8_MT(BF16) } else { LV_I8_MT(F16) }
#undef LV_I8_MT
#undef LV_I8
#undef LV_I8_ARGS
  LV_LAUNCH_CHECK();
  if (ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(i8_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale, w_scale,
                         (const uint16_t*)bias, MN, N, ksplit);
    else
      hipLaunchKernelGGL(i8_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale, w_scale,
                         (const uint16_t*)bias, MN, N, ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
