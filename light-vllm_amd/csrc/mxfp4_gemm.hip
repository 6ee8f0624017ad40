// W4A8 MXFP4 weight-streaming GEMM for decode batches on gfx950 (OCP microscaling: e2m1 weights, one E8M0 scale per
// 32 consecutive k of a row; fp8 e4m3fn activations):
//   Y[M,N] = T( sx[m] * sum_k Xq[m,k] * W4[n,k] * 2^(E[n,k/32] - 127) + bias[n] ),
// M <= 64 rows, Xq quantised beforehand (fp8_quant.hip) with one fp32 scale per token (sx), fp32 accumulation in the
// matrix pipe, sx and the bias applied in fp32 in that order, one rounding to T (bf16 / f16).  There is no per-channel
// weight scale: MX has none.
//
// Instruction: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4 (A = fp4) and blgp = 0 (B = fp8 e4m3).  A k-step is 128
// k; lane (g = lane >> 4, c = lane & 15) holds row c of both operands.  Measured on an MI355X with one-hot operands
// (DESIGN 3.4d): the fp4 operand is 4 registers, k 32 g .. 32 g + 31 of the step in k order, the lower k of a byte in
// its low nibble -- the checkpoint's own bytes; the fp8 operand is 8 registers, k 16 g .. 16 g + 15 in the low four
// and k 64 + 16 g .. + 15 in the high four (the two 64-k halves of the unscaled layout, NOT 32 consecutive k).  A lane's
// 32 fp4 k are exactly one MX block, and the pipe applies to them the scale byte that the SAME lane passes (op_sel
// picks the byte of its register), so the A scale is one E8M0 byte per lane and step; the B scale is the constant 2^0
// (0x7f in every lane).  No weight is touched by a VALU instruction between its load and the MFMA.
//
// Packed layout (lvllm_mxfp4_pack, once at load time):
//   codes   [N/16][K/128][lane 64][16 bytes]      one contiguous KiB per (n-tile, k-step); lane (g, c) owns the 16
//                                                 checkpoint bytes of W4[16 t + c][128 s + 32 g .. + 31] as they are
//                                                 (element k in byte k/2, even k in the low nibble)
//   scales  [N/16][ceil(K/512)][lane 64][4 bytes] byte b of lane (g, c)'s word u = E[16 t + c][4 (4 u + b) + g], the
//                                                 scale of that lane's block in k-step 4 u + b; steps past K hold 127
// One dword load per lane feeds up to four MFMAs through op_sel, a wave's load is 256 contiguous bytes.
//
// Organisation (the family's, int8_gemm.hip): X fragments resident in registers as the B operand, W from HBM to VGPR to
// the A operand with no LDS, the 8 waves of a workgroup split K, their partial tiles meet in double-buffered LDS,
// summed tiles wait in an LDS stage and leave in bursts after the stream.  The prologue moves fp8 bytes only: row-order
// loads, a wave-private swizzled LDS transpose, fragments.  A wave owns 1, 2 or 4 consecutive k-steps that start at a
// multiple of their number, so they never straddle a scale word: the word is shifted once per tile by the wave-uniform
// 8 * (first step mod 4) and op_sel 0 .. 3 then picks the step.  K beyond 8 waves * 4 steps = 4096 is split over
// blockIdx.y into fp32 partials, which the reduce kernel sums in the fixed order 0, 1, 2 ...; the waves' tiles are
// summed in wave order.  fp32 sums depend on that order, which is fixed, so a launch is reproducible.
//
// Register budget (256 per lane at 2 waves per SIMD), sized at MT = 4 m-tiles and 4 steps per wave:
//   X fragments   MT * steps * 8      = 128   (512 k per wave, 4096 k per workgroup)
//   W in flight   TIF * (steps * 4 + 1) = 17 / 34 / 68 at TIF = 1 / 2 / 4
//   accumulators  NT * MT * 4         =  16
//   addresses, masks, epilogue        ~  40
// The compiler reports 186 / 217 / 251 VGPRs at MT = 4 and TIF = 1 / 2 / 4 (93 / 120 at MT = 1 / 2 and TIF = 1), no
// scratch anywhere, no static LDS (dynamic: 2 x 8 x MT KiB of meeting buffers, 32 KiB of transpose scratch, the
// output stage in what is left of 160 KiB).  Measured (profiles/mxfp4_gemm.md), one tile in flight -- 4 KiB per wave,
// 64 KiB per CU at two workgroups -- was fastest or level on 13 of 16 (shape, M) points (3-7 % ahead of two tiles at 32 and
// 64 rows on gate_up and down, 2 % behind them on down at M <= 8) and is the build's choice; -DLVLLM_MX4_TIF=2 or 4 rebuilds the
// alternatives for A/B runs.
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace lvllm {
namespace {

typedef int mx_i32x4_t __attribute__((ext_vector_type(4)));
typedef int mx_i32x8_t __attribute__((ext_vector_type(8)));
typedef float mx_f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kMxWaves = 8;
constexpr int kMxSteps = 4;                      // k-steps of 128 a wave may own
constexpr unsigned kMxOutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kMxMaxK = 131072;
#ifndef LVLLM_MX4_TIF
#define LVLLM_MX4_TIF 1  // n-tiles in flight per wave: 1, 2, 4 measured, 1 kept (profiles/mxfp4_gemm.md)
#endif
#ifndef LVLLM_MX4_AUX
#define LVLLM_MX4_AUX 2  // nt: weights are read once per launch
#endif

// T( sx * acc[r] + bias[r] ) for four consecutive n of one row, packed for one 8-byte store
template <typename T>
__device__ __forceinline__ uint2 mx_epilogue(const mx_f32x4_t acc, const float sxm,
                                             const typename T::store_t* __restrict__ bias4) {
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    f[r] = sxm * acc[r];
    if (bias4 != nullptr) f[r] += T::to_float(bias4[r]);
  }
  uint2 o;
  o.x = (uint32_t)T::from_float(f[0]) | ((uint32_t)T::from_float(f[1]) << 16);
  o.y = (uint32_t)T::from_float(f[2]) | ((uint32_t)T::from_float(f[3]) << 16);
  return o;
}

// one n-tile of one wave in flight: its k-steps' codes and the scale word that covers them
struct MxSlot {
  mx_i32x4_t w[kMxSteps];
  unsigned e;
};

// TIF: n-tiles in flight per wave
template <typename T, int MT, int TIF>
__global__ __launch_bounds__(kMxWaves * 64, 2) void skinny_gemm_mxfp4_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const uint8_t* __restrict__ xq, const uint8_t* __restrict__ wq, const uint8_t* __restrict__ eq,
    const float* __restrict__ sx, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int steps_per_wave, const int ntiles, const int stage_tiles) {
  constexpr int NT = (MT == 1 && TIF % 2 == 0) ? 2 : 1;  // n-tiles accumulated between two wave meetings
  constexpr int KSTEPS = kMxSteps;
  static_assert(TIF % NT == 0, "a meeting falls on a slot boundary");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  mx_f32x4_t* red = reinterpret_cast<mx_f32x4_t*>(smem_raw);  // [2][waves][NT * MT][64]

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int total_steps = K >> 7;
  const int step0 = (blockIdx.y * kMxWaves + wave) * steps_per_wave;  // first k-step of this wave
  int nvalid = total_steps - step0;                                   // k-steps that exist
  nvalid = nvalid < 0 ? 0 : (nvalid > steps_per_wave ? steps_per_wave : nvalid);

  // descriptors sized to the packed tensors exactly: a wrong offset reads zeros, never memory outside
  const int scale_words = (total_steps + 3) >> 2;  // per n-tile and lane
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K / 2), 0x00020000);
  __amdgpu_buffer_rsrc_t er =
      __builtin_amdgcn_make_buffer_rsrc((void*)eq, 0, (int)((int64_t)ntiles * scale_words * 256), 0x00020000);
  const unsigned w_lane = (unsigned)(lane * 16) + (unsigned)step0 * 1024u;
  const unsigned w_tile = (unsigned)total_steps * 1024u;
  const unsigned e_lane = (unsigned)(lane * 4) + (unsigned)(step0 >> 2) * 256u;
  const unsigned e_tile = (unsigned)scale_words * 256u;
  const unsigned e_shift = (unsigned)(step0 & 3) * 8u;  // the wave's first step inside its scale word

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

  // a slot: one n-tile over this wave's k-steps, up to KSTEPS loads of 1 KiB and one of 256 bytes per wave.  Steps the
  // wave does not own load zero codes, which contribute 0 whatever scale byte op_sel then picks (never NaN: the pack
  // refuses 0xFF, and the shift fills with zeros).
  MxSlot wslot[TIF];
  auto load_unit = [&](MxSlot& a, const int i) __attribute__((always_inline)) {
    const unsigned tmask = opaque(i < my_tiles ? 0u : ~0u);
    const unsigned t = (unsigned)tile_of(i);
    const unsigned base = w_lane + t * w_tile;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
      a.w[s] = __builtin_bit_cast(mx_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(
                                                  wr, (base + (unsigned)s * 1024u) | tmask | kmask[s], 0, LVLLM_MX4_AUX));
    a.e = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(er, (e_lane + t * e_tile) | tmask, 0, LVLLM_MX4_AUX);
  };

  mx_i32x8_t xf[MT][KSTEPS];
  mx_f32x4_t acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = mx_f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int ngroups = (my_tiles + NT - 1) / NT;

  // output stage: summed tiles wait in LDS (fp32, 1 KiB per (tile, m-tile)) and leave in one burst, so that no store
  // sits between weight loads (vmcnt retires in issue order)
  mx_f32x4_t* stage = red + (size_t)2 * kMxWaves * NT * MT * 64;  // [stage_tiles][MT][64]
  int stage_base = 0;
  auto store_slab = [&](const int i, const int mt, const mx_f32x4_t sum) __attribute__((always_inline)) {
    // lane (g, c): columns n = n0 + r of row m = 16 mt + c
    const int n0 = 16 * tile_of(i) + 4 * g;
    const int m = mt * 16 + c;
    if (m < M && n0 < N) {
      if (partial != nullptr)
        *reinterpret_cast<mx_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = sum;
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) =
            mx_epilogue<T>(sum, sx[m], bias != nullptr ? bias + n0 : nullptr);
    }
  };
  auto flush_stage = [&](const int end_tile) __attribute__((always_inline)) {
    __syncthreads();  // every reducer's slab is in the stage
    const int nslabs = (end_tile - stage_base) * MT;
    for (int sl = wave; sl < nslabs; sl += kMxWaves)
      store_slab(stage_base + sl / MT, sl % MT, stage[(size_t)sl * 64 + lane]);
    stage_base = end_tile;
    __syncthreads();  // the stage may be overwritten again
  };
  auto finish_group = [&](const int grp) __attribute__((always_inline)) {
    if ((grp + 1) * NT - stage_base > stage_tiles) flush_stage(grp * NT);  // uniform: make room first
    mx_f32x4_t* buf = red + (size_t)(grp & 1) * kMxWaves * NT * MT * 64;    // [wave][slab = j * MT + mt][lane]
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        buf[(wave * NT * MT + j * MT + mt) * 64 + lane] = acc[j][mt];
        acc[j][mt] = mx_f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    __syncthreads();
    for (int slab = wave; slab < NT * MT; slab += kMxWaves) {
      const int j = slab / MT, mt = slab - j * MT;
      const int i = grp * NT + j;
      if (i >= my_tiles) continue;
      mx_f32x4_t sum = buf[slab * 64 + lane];
#pragma unroll
      for (int w2 = 1; w2 < kMxWaves; ++w2) sum += buf[(w2 * NT * MT + slab) * 64 + lane];  // wave order: fixed
      stage[((size_t)(i - stage_base) * MT + mt) * 64 + lane] = sum;
    }
  };

  // ---- X fragments, kept for the whole launch.  The wave's 512 bytes of a row are 32 chunks of 16 bytes, handled in
  // two passes of 16 chunks (2 k-steps).  Read in ROW order (a row's chunks side by side over 16 lanes, 4 rows per
  // wave-wide load), then turned into fragment order through a wave-private LDS scratch; chunk q of row r sits at
  // position q ^ r, which spreads both the row-order writes and the fragment-order reads over the banks.  Lane (g, c)
  // of step s takes chunks 8 (s mod 2) + g and + 4 + g of row c: the fp8 operand's k 16 g .. and 64 + 16 g .. .
  {
    mx_i32x4_t xc[MT][2 * KSTEPS];
    __amdgpu_buffer_rsrc_t xr =
        __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);
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
                                   : kMxOutOfRange;
          xc[mt][h * 4 + i] = __builtin_bit_cast(mx_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
        }
    // the first TIF tiles follow the activations into the queue
#pragma unroll
    for (int j = 0; j < TIF; ++j) load_unit(wslot[j], j);
    char* xs = reinterpret_cast<char*>(stage + (size_t)stage_tiles * MT * 64) + wave * 4096;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<mx_i32x4_t*>(xs + i * 1024 + lane * 16) = xc[mt][h * 4 + i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          xc[mt][h * 4 + j] =
              *reinterpret_cast<const mx_i32x4_t*>(xs + c * 256 + (((8 * (j >> 1) + 4 * (j & 1) + g) ^ c) * 16));
      }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s)
        xf[mt][s] = __builtin_shufflevector(xc[mt][2 * s], xc[mt][2 * s + 1], 0, 1, 2, 3, 4, 5, 6, 7);
  }

  // op_sel is an immediate: the step index reaches the builtin as a constant
  auto mfma_step = [&](auto S, const MxSlot& a, const unsigned e, mx_f32x4_t (&d)[MT]) __attribute__((always_inline)) {
    constexpr int s = decltype(S)::value;
    const mx_i32x8_t w8 = {a.w[s][0], a.w[s][1], a.w[s][2], a.w[s][3], 0, 0, 0, 0};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      d[mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, xf[mt][s], d[mt], 4 /* A = fp4 */,
                                                              0 /* B = fp8 e4m3 */, s, (int)e, 0, 0x7f7f7f7f);
  };

  // slot j holds local tile base + j; it is refilled with tile base + j + TIF as soon as it is consumed, so TIF tiles
  // stay in flight, also across the meetings.  Tiles past my_tiles load nothing and compute nothing.
  for (int base = 0; base < ngroups * NT; base += TIF) {
#pragma unroll
    for (int j = 0; j < TIF; ++j) {
      const int i = base + j;
      if (i < my_tiles) {  // uniform
        const unsigned e = wslot[j].e >> e_shift;
        mfma_step(std::integral_constant<int, 0>{}, wslot[j], e, acc[j % NT]);
        mfma_step(std::integral_constant<int, 1>{}, wslot[j], e, acc[j % NT]);
        mfma_step(std::integral_constant<int, 2>{}, wslot[j], e, acc[j % NT]);
        mfma_step(std::integral_constant<int, 3>{}, wslot[j], e, acc[j % NT]);
      }
      load_unit(wslot[j], i + TIF);
      if (j % NT == NT - 1 && i / NT < ngroups) finish_group(i / NT);  // uniform over the workgroup
    }
  }
  flush_stage(my_tiles);  // all weights have been streamed: now the stores
}

// y[m, n] = epilogue(sum_s partial[s, m, n]), s ascending
template <typename T>
__global__ void mx_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                 const float* __restrict__ sx, const typename T::store_t* __restrict__ bias,
                                 const int64_t MN, const int N, const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  mx_f32x4_t sum = *reinterpret_cast<const mx_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const mx_f32x4_t*>(partial + (int64_t)s * MN + i);
  const int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
  *reinterpret_cast<uint2*>(y + i) = mx_epilogue<T>(sum, sx[m], bias != nullptr ? bias + n : nullptr);
}

// checkpoint order -> streaming order.  One thread per dword of packed codes; the first `ewords` threads also write
// one scale word each.  A scale byte of 0xFF (E8M0 NaN) raises *bad.
__global__ void mxfp4_pack_kernel(uint32_t* __restrict__ w_packed, uint32_t* __restrict__ e_packed,
                                  const uint32_t* __restrict__ codes, const uint8_t* __restrict__ scales,
                                  const int64_t wwords, const int64_t ewords, const int K, int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int steps = K >> 7, scale_words = (steps + 3) >> 2;
  const int lane = (int)(i >> 2) & 63, g = lane >> 4, c = lane & 15;
  if (i < wwords) {
    const int64_t unit = i >> 8;  // (n-tile, k-step)
    const int64_t t = unit / steps;
    const int s = (int)(unit - t * steps);
    // row 16 t + c, bytes 64 s + 16 g + 4 j .. + 3 of its K / 2
    w_packed[i] = codes[((16 * t + c) * (int64_t)(K >> 1) + 64 * s + 16 * g) / 4 + (i & 3)];
  }
  if (i < ewords) {
    const int el = (int)i & 63, eg = el >> 4, ec = el & 15;
    const int64_t t = (i >> 6) / scale_words;
    const int u = (int)((i >> 6) - t * scale_words);
    uint32_t word = 0;
    for (int b = 0; b < 4; ++b) {
      const int s = 4 * u + b;
      const uint32_t e = s < steps ? scales[(16 * t + ec) * (int64_t)(K >> 5) + 4 * s + eg] : 127u;
      if (e == 0xffu) atomicOr(bad, 1);
      word |= e << (8 * b);
    }
    e_packed[i] = word;
  }
}

template <typename T, int MT>
void launch_mx(void* y, float* partial, const void* xq, const void* wq, const void* eq, const float* sx,
               const void* bias, int M, int N, int K, int64_t ldx, int steps_per_wave, int ntiles, int groups,
               int ksplit, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr int TIF = LVLLM_MX4_TIF;
  constexpr int NT = (MT == 1 && TIF % 2 == 0) ? 2 : 1;
  const size_t red_bytes = (size_t)2 * kMxWaves * NT * MT * 64 * sizeof(mx_f32x4_t);
  const size_t xs_bytes = (size_t)kMxWaves * 4096;  // the activation transpose's scratch
  // output stage: as many tiles as the workgroup owns, capped by what is left of the 160 KiB LDS
  int stage_tiles = (((ntiles + groups - 1) / groups + NT - 1) / NT) * NT;
  const int cap = (int)((160 * 1024 - red_bytes - xs_bytes) / ((size_t)MT * 1024) / NT) * NT;
  if (stage_tiles > cap) stage_tiles = cap;
  if (stage_tiles < NT) stage_tiles = NT;
  const size_t smem = red_bytes + (size_t)stage_tiles * MT * 64 * sizeof(mx_f32x4_t) + xs_bytes;
  auto kern = skinny_gemm_mxfp4_kernel<T, MT, TIF>;
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kern, dim3(groups, ksplit), dim3(kMxWaves * 64), smem, stream, (S*)y, partial,
                     (const uint8_t*)xq, (const uint8_t*)wq, (const uint8_t*)eq, sx, (const S*)bias, M, N, K, ldx,
                     steps_per_wave, ntiles, stage_tiles);
}

inline int mx_ksplit(int K) {
  const int cap = kMxWaves * kMxSteps;
  return (K / 128 + cap - 1) / cap;
}
inline bool mx_shape_ok(int N, int K) {
  return N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0 && K < kMxMaxK && (int64_t)N * K / 2 < ((int64_t)1 << 32) - 16;
}
// gemm_balance (common.h Tuning): the fewest workgroups that need no more rounds of n-tiles than `cap` would
inline int mx_balanced_groups(int units, int cap) {
  if (cap < 1) cap = 1;
  if (units <= cap) return units < 1 ? 1 : units;
  if (!tuning().gemm_balance) return cap;
  const int rounds = (units + cap - 1) / cap;
  return (units + rounds - 1) / rounds;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_mxfp4_packed_bytes(int N, int K) { return mx_shape_ok(N, K) ? (int64_t)N * K / 2 : 0; }
extern "C" int64_t lvllm_mxfp4_scale_bytes(int N, int K) {
  return mx_shape_ok(N, K) ? (int64_t)(N / 16) * ((K / 128 + 3) / 4) * 256 : 0;
}

extern "C" int lvllm_mxfp4_pack(void* w_packed, void* e_packed, const void* codes, const void* scales, int N, int K,
                                void* stream) {
  if (!mx_shape_ok(N, K) || ((((uintptr_t)w_packed | (uintptr_t)e_packed | (uintptr_t)codes) & 3) != 0)) {
    set_error("lvllm_mxfp4_pack: N % 16 == 0, K % 128 == 0, K < 131072, 4-byte aligned tensors");
    return 3;
  }
  hipStream_t s = (hipStream_t)stream;
  int* bad = nullptr;
  int host_bad = 0;
  if (hipMalloc((void**)&bad, sizeof(int)) != hipSuccess || hipMemcpyAsync(bad, &host_bad, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) {
    (void)hipGetLastError();
    if (bad != nullptr) (void)hipFree(bad);
    set_error("lvllm_mxfp4_pack: no device memory for the scale check");
    return 2;
  }
  const int64_t wwords = lvllm_mxfp4_packed_bytes(N, K) / 4, ewords = lvllm_mxfp4_scale_bytes(N, K) / 4;
  hipLaunchKernelGGL(mxfp4_pack_kernel, dim3((unsigned)((wwords + 255) / 256)), dim3(256), 0, s, (uint32_t*)w_packed,
                     (uint32_t*)e_packed, (const uint32_t*)codes, (const uint8_t*)scales, wwords, ewords, K, bad);
  // load time: the answer of the scale check is waited for
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(&host_bad, bad, sizeof(int), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(bad);
  if (e != hipSuccess) {
    set_error(std::string("lvllm_mxfp4_pack: ") + hipGetErrorString(e));
    return 2;
  }
  LV_CHECK(host_bad == 0, "a scale byte is 0xFF (E8M0 NaN), which is outside the contract");
  return 0;
}

extern "C" int64_t lvllm_skinny_gemm_w4a8_mxfp4_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || M > 64 || N <= 0 || K < 128) return 0;
  const int ksplit = mx_ksplit(K);
  return ksplit > 1 ? (int64_t)ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_skinny_gemm_w4a8_mxfp4(void* y, const void* x_fp8, const void* w_packed, const void* e_packed,
                                            const float* x_scale, const void* bias, int M, int N, int K, int64_t ldx,
                                            int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(x_scale != nullptr, "x_scale [M] is a device pointer");
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || M > 64 || !mx_shape_ok(N, K) || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) || ((((uintptr_t)x_fp8 | (uintptr_t)w_packed) & 15) != 0) ||
      (((uintptr_t)e_packed) & 3) != 0 || (((uintptr_t)y) & 7) != 0 || (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_skinny_gemm_w4a8_mxfp4: shape outside the kernel's envelope");
    return 3;
  }
  const int total_steps = K / 128;
  const int ksplit = mx_ksplit(K);
  // 1, 2 or 4 steps per wave, so that a wave's steps start at a multiple of their number (file header)
  const int steps_per_wave = total_steps <= kMxWaves ? 1 : (total_steps <= 2 * kMxWaves ? 2 : 4);
  const int ntiles = N / 16;
  const int cus = (ntiles >= tuning().gemm_wide_min_tiles && tuning().gemm_workgroups_wide > 0)
                      ? tuning().gemm_workgroups_wide
                      : tuning().gemm_workgroups;
  const int groups = mx_balanced_groups(ntiles, cus / ksplit);
  float* partial = nullptr;
  if (ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_skinny_gemm_w4a8_mxfp4_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  const int MT = (M + 15) / 16;
#define LV_MX_ARGS y, partial, x_fp8, w_packed, e_packed, x_scale, bias, M, N, K, ldx, steps_per_wave, ntiles, groups, ksplit, s
#define LV_MX_MT(T_)                                  \
  switch (MT) {                                       \
    case 1: launch_mx<T_, 1>(LV_MX_ARGS); break;      \
    case 2: launch_mx<T_, 2>(LV_MX_ARGS); break;      \
    default: launch_mx<T_, 4>(LV_MX_ARGS); break;     \
  }
  if (dtype == LVLLM_BF16) { LV_MX_MT(BF16) } else { LV_MX_MT(F16) }
#undef LV_MX_MT
#undef LV_MX_ARGS
  LV_LAUNCH_CHECK();
  if (ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(mx_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale,
                         (const uint16_t*)bias, MN, N, ksplit);
    else
      hipLaunchKernelGGL(mx_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale,
                         (const uint16_t*)bias, MN, N, ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
