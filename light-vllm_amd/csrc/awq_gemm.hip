// W4A16 (AWQ int4, group-quantised) weight-streaming GEMM for decode batches on gfx950:
//   Y[M,N] = T( sum_k X[m,k] . Wd[k,n] (+ bias) ),  Wd[k,n] = T( float(q[k,n] - z[k/G,n]) * float(s[k/G,n]) ),
// M <= 64 rows, bf16/f16 activations, fp32 accumulate (the AWQ path of the reference: awq.py:103-175,
// csrc/quantization/awq/gemm_kernels.cu:372-401, dequantize.cuh:41-61).
//
// gfx950 has no int4 MFMA, so this is the organisation of skinny_gemm.hip -- X fragments resident in registers, W from
// HBM to VGPR to the MFMA A operand, 8 waves of a workgroup split K, partial tiles meet in double-buffered LDS,
// results parked in LDS and stored in bursts, K beyond one workgroup's reach split over blockIdx.y into fp32 partials
// -- with a dequantisation stage in registers between the load's arrival and v_mfma_f32_16x16x32_{bf16,f16}.
//
// Packed weight (lvllm_awq_pack, once at load time): [N/16][Kp/128][lane = 64][16 bytes], Kp = K rounded up to 128.
// Lane (g = lane >> 4, c = lane & 15) of unit (n-tile t, k-block b) owns the 32 nibbles
//   q[k = 128 b + 32 s + 8 g + e][n = 16 t + c],  s = 0..3 (32-bit word s of its 16 bytes), e = 0..7,
// so ONE buffer_load_b128 per lane is its A fragments for four k-steps and one wave load is one contiguous KiB.
// Inside a word nibble i (bits 4i..4i+3) holds e = 2 i for i < 4 and e = 2 (i - 4) + 1 for i >= 4: the pair the MFMA
// wants in one register, (e = 2j, e = 2j + 1), is then `(word >> 4 j) & 0x000f000f` -- one shift and one v_and_or per
// PAIR, the nibbles already in the low bits of the two 16-bit halves.
// Metadata: [N/16][Kp/128][row c = 16][128/G] 32-bit words {T scale (low half), T(zero) (high half)}.  A lane fetches
// all groups of its row and k-block with ONE load of 4 / 8 / 16 bytes (G = 128 / 64 / 32), issued with the block's
// weights; the four g lanes of a row read the same address.  This is the [N/16][K/G][16] order with the groups of one
// k-block moved next to each other per row: the same 4 bytes per group and row, a quarter of the load instructions at
// G = 32, and identical to it at G = 128.  k >= K (K % 128 != 0: outside the kernel's envelope, the packed form still
// exists for the dequantise-and-multiply route) is padded with nibble 0, scale 0, zero 0.
//
// Dequantisation, exact (one rounding, to T, as the reference's sub.f16x2 + fma.rn.f16x2(., s, 0)):
//   f16:  h = pair | 0x64006400           -> (1024 + q) in both halves (ulp of f16 at 1024 is 1)
//         v_pk_add_f16 h, -(1024 + z)     -> q - z, exact
//         v_pk_mul_f16 ., s               -> the one rounding
//   bf16: h = pair | 0x43004300           -> (128 + q) in both halves (ulp of bf16 at 128 is 1); each half widened to
//         fp32 by a shift / a mask; fma(128 + q, s, c) with c = -(128 + z) * s: (128 + z) and s have 8 significant bits
//         each, so c, the product and the sum (q - z) * s are exact in fp32 (|s| < 2^119, far above any real scale);
//         v_cvt_pk_bf16_f32 is the one rounding.
// No LDS, no table: 3-4 VALU per pair for f16, 6 for bf16.
//
// Pipeline: a W4 unit (n-tile, wave's k-blocks) is 1/4 of the bytes of a 16-bit unit, so the number of n-tiles in
// flight per wave is a parameter (LVLLM_W4_TIF): each slot is refilled right after it is consumed and stays in flight
// across the wave meetings.  Measured at 2, 4 and 6 (profiles/awq_gemm.md): 2 is fastest on every shape and row count
// (4-8 KiB per wave in flight), so 2 is the default; a deeper build caps the variant with two m-tiles and 16 k-steps
// at 3 (2 at G = 32), the most that fits beside its 128 registers of X without spilling.
#include "common.h"
#include "w4_dequant.h"

namespace lvllm {
namespace {

// W4Dequant, w4_dequant_word, w4_mfma, w4_load_meta and the vector types: w4_dequant.h, shared with awq_tiled_gemm.hip
constexpr int kW4Waves = 8;
#ifndef LVLLM_W4_TIF
#define LVLLM_W4_TIF 2  // n-tiles in flight per wave (by measurement, see above)
#endif

// checkpoint order: nibble i of a qweight / qzeros word holds column 8 j + kAwqOrder[i] (dequantize.cuh:41-61)
__device__ __forceinline__ int awq_nibble_of_column(const int r) { return ((r & 1) << 2) | (r >> 1); }  // inverse of [0,2,4,6,1,3,5,7]

// KSTEPS: k-steps of 32 a wave may own (its X fragments: MT * KSTEPS * 4 registers), in whole k-blocks of 4;
// G: group size; TIF: n-tiles in flight per wave.
template <typename T, int MT, int KSTEPS, int G, int TIF>
__global__ __launch_bounds__(kW4Waves * 64, 2) void skinny_gemm_w4_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const typename T::store_t* __restrict__ x, const uint32_t* __restrict__ w4, const uint32_t* __restrict__ meta,
    const typename T::store_t* __restrict__ bias, const int M, const int N, const int K, const int64_t ldx,
    const int blocks_per_wave, const int ntiles, const int stage_tiles) {
  constexpr int KB = KSTEPS / 4;   // k-blocks of 128 per wave
  constexpr int MW = 128 / G;      // metadata words per row and k-block
  constexpr int HALF = KSTEPS / 2;
  constexpr int NT = 2 / MT > 0 ? 2 / MT : 1;  // n-tiles accumulated between two wave meetings (NT * MT slabs)
  static_assert(KSTEPS == 8 || KSTEPS == 16, "two or four k-blocks per wave");
  static_assert(G == 32 || G == 64 || G == 128, "group sizes of the envelope");
  static_assert(TIF % NT == 0, "a meeting falls on a slot boundary");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  q_f32x4_t* red = reinterpret_cast<q_f32x4_t*>(smem_raw);  // [2][waves][NT * MT][64]

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int kblocks = K >> 7;
  const int blk0 = (blockIdx.y * kW4Waves + wave) * blocks_per_wave;  // first k-block of this wave
  int nvb = kblocks - blk0;                                           // k-blocks that exist
  nvb = nvb < 0 ? 0 : (nvb > blocks_per_wave ? blocks_per_wave : nvb);
  const int step0 = 4 * blk0, nvalid = 4 * nvb;

  // descriptors sized to the packed buffers exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc((void*)w4, 0, (int)((int64_t)ntiles * kblocks * 1024), 0x00020000);
  __amdgpu_buffer_rsrc_t mr =
      __builtin_amdgcn_make_buffer_rsrc((void*)meta, 0, (int)((int64_t)ntiles * kblocks * 64 * MW), 0x00020000);
  const unsigned w_lane = (unsigned)(lane * 16) + (unsigned)blk0 * 1024u;
  const unsigned w_tile = (unsigned)kblocks * 1024u;
  const unsigned m_lane = (unsigned)(c * 4 * MW) + (unsigned)blk0 * (64u * MW);
  const unsigned m_tile = (unsigned)kblocks * (64u * MW);

  // n-tiles are handed out round-robin: local tile i is tile blockIdx.x + i * gridDim.x
  const int my_tiles = ntiles > (int)blockIdx.x ? (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  auto tile_of = [&](const int i) __attribute__((always_inline)) { return (int)(blockIdx.x + i * gridDim.x); };
  // wave-uniform masks through an empty asm, so that the selects stay selects (see skinny_gemm.hip)
  auto opaque = [](unsigned v) __attribute__((always_inline)) {
    v = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
    asm("" : "+s"(v));
    return v;
  };
  unsigned kmask[KB];
#pragma unroll
  for (int b = 0; b < KB; ++b) kmask[b] = opaque(b < nvb ? 0u : ~0u);

  // a slot: the weights and the metadata of one n-tile over this wave's k-blocks
  q_u32x4_t wq[TIF][KB];
  uint32_t mq[TIF][KB][MW];
  auto load_unit = [&](q_u32x4_t (&a)[KB], uint32_t (&m)[KB][MW], const int i) __attribute__((always_inline)) {
    const unsigned t = (unsigned)tile_of(i);
    const unsigned tmask = opaque(i < my_tiles ? 0u : ~0u);
#pragma unroll
    for (int b = 0; b < KB; ++b) {
      a[b] = __builtin_amdgcn_raw_buffer_load_b128(wr, (w_lane + t * w_tile + (unsigned)b * 1024u) | tmask | kmask[b],
                                                   0, LVLLM_W4_AUX);
      w4_load_meta<MW>(m[b], mr, (m_lane + t * m_tile + (unsigned)b * (64u * MW)) | tmask | kmask[b]);
    }
  };

  q_u32x4_t xf[MT][KSTEPS];
  q_f32x4_t acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = q_f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int ngroups = (my_tiles + NT - 1) / NT;

  // output stage: summed tiles wait in LDS (fp32, 1 KiB per (tile, m-tile)) and leave in one burst, so that no store
  // sits between weight loads (vmcnt retires in issue order)
  q_f32x4_t* stage = red + (size_t)2 * kW4Waves * NT * MT * 64;  // [stage_tiles][MT][64]
  int stage_base = 0;
  auto store_slab = [&](const int i, const int mt, q_f32x4_t sum) __attribute__((always_inline)) {
    // lane (g, c): columns n = n0 + r of row m = 16 mt + c
    const int n0 = 16 * tile_of(i) + 4 * g;
    const int m = mt * 16 + c;
    if (m < M && n0 < N) {
      if (partial != nullptr) {
        *reinterpret_cast<q_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = sum;
      } else {
        if (bias != nullptr) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sum[r] += T::to_float(bias[n0 + r]);
        }
        uint2 o;
        o.x = (uint32_t)T::from_float(sum[0]) | ((uint32_t)T::from_float(sum[1]) << 16);
        o.y = (uint32_t)T::from_float(sum[2]) | ((uint32_t)T::from_float(sum[3]) << 16);
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) = o;
      }
    }
  };
  auto flush_stage = [&](const int end_tile) __attribute__((always_inline)) {
    __syncthreads();  // every reducer's slab is in the stage
    const int nslabs = (end_tile - stage_base) * MT;
    for (int sl = wave; sl < nslabs; sl += kW4Waves)
      store_slab(stage_base + sl / MT, sl % MT, stage[(size_t)sl * 64 + lane]);
    stage_base = end_tile;
    __syncthreads();  // the stage may be overwritten again
  };
  auto finish_group = [&](const int grp) __attribute__((always_inline)) {
    if ((grp + 1) * NT - stage_base > stage_tiles) flush_stage(grp * NT);  // uniform: make room first
    q_f32x4_t* buf = red + (size_t)(grp & 1) * kW4Waves * NT * MT * 64;     // [wave][slab = j * MT + mt][lane]
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        buf[(wave * NT * MT + j * MT + mt) * 64 + lane] = acc[j][mt];
        acc[j][mt] = q_f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    __syncthreads();
    for (int slab = wave; slab < NT * MT; slab += kW4Waves) {
      const int j = slab / MT, mt = slab - j * MT;
      const int i = grp * NT + j;
      if (i >= my_tiles) continue;
      q_f32x4_t sum = buf[slab * 64 + lane];
#pragma unroll
      for (int w2 = 1; w2 < kW4Waves; ++w2) {
        const q_f32x4_t v = buf[(w2 * NT * MT + slab) * 64 + lane];
        sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
      }
      stage[((size_t)(i - stage_base) * MT + mt) * 64 + lane] = sum;
    }
  };

  // dequantise one slot and multiply: per k-block its groups' constants, per k-step 4 pairs -> one A fragment
  auto compute_unit = [&](const q_u32x4_t (&a)[KB], const uint32_t (&m)[KB][MW], q_f32x4_t (&ac)[MT])
                          __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
      for (int gl = 0; gl < MW; ++gl) {
        const W4Dequant<T> d(m[b][gl]);
#pragma unroll
        for (int s = gl * (4 / MW); s < (gl + 1) * (4 / MW); ++s) {  // the k-steps of this group
          const q_u32x4_t af = w4_dequant_word<T>(a[b][s], d);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) ac[mt] = w4_mfma<T>(af, xf[mt][4 * b + s], ac[mt]);
        }
      }
  };

  // ---- X fragments: X[m = 16 mt + c][k = 32 (step0 + s) + 8 g ..], kept for the whole launch.  Read in ROW order
  // (64 lanes x 16 bytes = whole row segments, all loads in flight at once), then turned into fragment order through
  // a wave-private LDS scratch; chunk q of row r sits at position q ^ r (skinny_gemm.hip has the measurements).
  {
    constexpr int NCH = HALF * 4;  // 16-byte chunks of one row in one pass
    constexpr int RPI = 64 / NCH;  // rows per wave-wide load
    __amdgpu_buffer_rsrc_t xr =
        __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(((int64_t)(M - 1) * ldx + K) * 2), 0x00020000);
    const int b = lane / NCH, pos = lane % NCH;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < HALF; ++i) {
          const int r = i * RPI + b, q = pos ^ r;
          const int ks = h * HALF + (q >> 2), m = mt * 16 + r;
          const unsigned off = (m < M && ks < nvalid)
                                   ? (unsigned)(((int64_t)m * ldx + (int64_t)(step0 + ks) * 32 + (q & 3) * 8) * 2)
                                   : kW4OutOfRange;
          xf[mt][h * HALF + i] = __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0);
        }
    // the first TIF tiles follow the activations into the queue
#pragma unroll
    for (int j = 0; j < TIF; ++j) load_unit(wq[j], mq[j], j);
    char* xs = reinterpret_cast<char*>(stage + (size_t)stage_tiles * MT * 64) + wave * (16 * NCH * 16);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < HALF; ++i)
          *reinterpret_cast<q_u32x4_t*>(xs + i * 1024 + lane * 16) = xf[mt][h * HALF + i];
#pragma unroll
        for (int s2 = 0; s2 < HALF; ++s2)
          xf[mt][h * HALF + s2] = *reinterpret_cast<const q_u32x4_t*>(xs + c * (NCH * 16) + (((4 * s2 + g) ^ c) * 16));
      }
  }

  // slot j holds local tile base + j; it is refilled with tile base + j + TIF as soon as it is consumed, so TIF tiles
  // stay in flight, also across the meetings.  Tiles past my_tiles load nothing (out-of-range offsets).
  for (int base = 0; base < ngroups * NT; base += TIF) {
#pragma unroll
    for (int j = 0; j < TIF; ++j) {
      const int i = base + j;
      if (i < my_tiles) compute_unit(wq[j], mq[j], acc[j % NT]);  // uniform: empty slots cost no VALU / MFMA
      load_unit(wq[j], mq[j], i + TIF);
      if (j % NT == NT - 1 && i / NT < ngroups) finish_group(i / NT);  // uniform over the workgroup
    }
  }
  flush_stage(my_tiles);  // all weights have been streamed: now the stores
}

// out[m, n] = T(sum_s partial[s, m, n] + bias[n])
template <typename T>
__global__ void w4_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                 const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                 const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  q_f32x4_t sum = *reinterpret_cast<const q_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) {
    const q_f32x4_t v = *reinterpret_cast<const q_f32x4_t*>(partial + (int64_t)s * MN + i);
    sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
  }
  if (bias != nullptr) {
    const int n = (int)(i % N);
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] += T::to_float(bias[n + r]);
  }
  uint2 o;
  o.x = (uint32_t)T::from_float(sum[0]) | ((uint32_t)T::from_float(sum[1]) << 16);
  o.y = (uint32_t)T::from_float(sum[2]) | ((uint32_t)T::from_float(sum[3]) << 16);
  *reinterpret_cast<uint2*>(y + i) = o;
}

// ---- load-time repack: checkpoint tensors -> the streaming order (file header) ----------------------------------
// One thread per destination word: unit (t, b), lane (g, c), word s <- 8 nibbles of column 16 t + c, rows k0 .. k0 + 7
__global__ void awq_pack_weight_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ qweight,
                                       const int64_t nwords, const int N, const int K, const int kblocks_p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  const int s = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const int64_t unit = i >> 8;
  const int t = (int)(unit / kblocks_p), b = (int)(unit - (int64_t)t * kblocks_p);
  const int n = 16 * t + (lane & 15), k0 = 128 * b + 32 * s + 8 * (lane >> 4);
  const int shift = 4 * awq_nibble_of_column(n & 7);
  uint32_t out = 0;
  if (k0 < K) {  // K % 8 == 0: the 8 rows exist together
#pragma unroll
    for (int nib = 0; nib < 8; ++nib) {
      const int e = nib < 4 ? 2 * nib : 2 * (nib - 4) + 1;
      out |= ((qweight[(int64_t)(k0 + e) * (N >> 3) + (n >> 3)] >> shift) & 15u) << (4 * nib);
    }
  }
  dst[i] = out;
}

// One thread per metadata word: unit (t, b), row c, group gl of the k-block
template <typename T>
__global__ void awq_pack_meta_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ qzeros,
                                     const typename T::store_t* __restrict__ scales, const int64_t nwords, const int N,
                                     const int K, const int G, const int kblocks_p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  const int mw = 128 / G;
  const int gl = (int)(i % mw), c = (int)((i / mw) & 15);
  const int64_t unit = i / (16 * mw);
  const int t = (int)(unit / kblocks_p), b = (int)(unit - (int64_t)t * kblocks_p);
  const int n = 16 * t + c, grp = b * mw + gl;
  uint32_t out = 0;
  if (grp < K / G) {
    const uint32_t z = (qzeros[(int64_t)grp * (N >> 3) + (n >> 3)] >> (4 * awq_nibble_of_column(n & 7))) & 15u;
    out = (uint32_t)scales[(int64_t)grp * N + n] | ((uint32_t)T::from_float((float)z) << 16);
  }
  dst[i] = out;
}

// ---- Wd [K, N] from the checkpoint tensors (awq_dequantize): one thread per qweight word = 8 columns of one row ----
template <typename T>
__global__ void awq_dequantize_kernel(typename T::store_t* __restrict__ out, const uint32_t* __restrict__ qweight,
                                      const uint32_t* __restrict__ qzeros,
                                      const typename T::store_t* __restrict__ scales, const int64_t nwords,
                                      const int N, const int G) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  const int nw = N >> 3;
  const int64_t k = i / nw;
  const int j = (int)(i - k * nw);
  const int64_t grp = k / G;
  const uint32_t q = qweight[i], z = qzeros[grp * nw + j];
  typename T::store_t o[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int sh = 4 * awq_nibble_of_column(r);
    const int d = (int)((q >> sh) & 15u) - (int)((z >> sh) & 15u);
    o[r] = T::from_float((float)d * T::to_float(scales[grp * N + 8 * j + r]));
  }
  uint4 v;
  v.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
  v.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
  v.z = (uint32_t)o[4] | ((uint32_t)o[5] << 16);
  v.w = (uint32_t)o[6] | ((uint32_t)o[7] << 16);
  *reinterpret_cast<uint4*>(out + k * N + 8 * j) = v;
}

// ---- Wd [K, N] from the PACKED form, with the streaming kernel's own dequantisation: one thread per packed word ----
template <typename T>
__global__ void awq_dequantize_packed_kernel(typename T::store_t* __restrict__ out, const uint32_t* __restrict__ w4,
                                             const uint32_t* __restrict__ meta, const int64_t nwords, const int N,
                                             const int K, const int G, const int kblocks_p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwords) return;
  const int mw = 128 / G;
  const int s = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const int64_t unit = i >> 8;
  const int t = (int)(unit / kblocks_p), b = (int)(unit - (int64_t)t * kblocks_p);
  const int c = lane & 15, n = 16 * t + c, k0 = 128 * b + 32 * s + 8 * (lane >> 4);
  if (k0 >= K) return;
  const W4Dequant<T> d(meta[(unit * 16 + c) * mw + ((s * mw) >> 2)]);
  const q_u32x4_t f = w4_dequant_word<T>(w4[i], d);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[(int64_t)(k0 + 2 * j) * N + n] = (typename T::store_t)(f[j] & 0xffffu);
    out[(int64_t)(k0 + 2 * j + 1) * N + n] = (typename T::store_t)(f[j] >> 16);
  }
}

template <typename T, int MT, int KSTEPS, int G>
int launch_w4(void* y, float* partial, const void* x, const void* w4, const void* meta, const void* bias, int M, int N,
              int K, int64_t ldx, int blocks_per_wave, int ntiles, int groups, int ksplit, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr int NT = 2 / MT > 0 ? 2 / MT : 1;
  const size_t red_bytes = (size_t)2 * kW4Waves * NT * MT * 64 * sizeof(q_f32x4_t);
  const size_t xs_bytes = (size_t)kW4Waves * 16 * (KSTEPS / 2) * 64;  // the activation transpose's scratch
  // output stage: as many tiles as the workgroup owns, capped by what is left of the 160 KiB LDS
  int stage_tiles = (((ntiles + groups - 1) / groups + NT - 1) / NT) * NT;
  const int cap = (int)((160 * 1024 - red_bytes - xs_bytes) / ((size_t)MT * 1024) / NT) * NT;
  if (stage_tiles > cap) stage_tiles = cap;
  if (stage_tiles < NT) stage_tiles = NT;
  const size_t smem = red_bytes + (size_t)stage_tiles * MT * 64 * sizeof(q_f32x4_t) + xs_bytes;
  // 16 k-steps of two m-tiles are 128 registers of X: three slots of 4 KiB fit beside them without spilling
  constexpr int kFit = (MT == 2 && KSTEPS == 16) ? (G == 32 ? 2 : 3) : LVLLM_W4_TIF;
  constexpr int TIF = kFit < LVLLM_W4_TIF ? kFit : LVLLM_W4_TIF;
  auto kern = skinny_gemm_w4_kernel<T, MT, KSTEPS, G, TIF>;
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kern, dim3(groups, ksplit), dim3(kW4Waves * 64), smem, stream, (S*)y, partial, (const S*)x,
                     (const uint32_t*)w4, (const uint32_t*)meta, (const S*)bias, M, N, K, ldx, blocks_per_wave, ntiles,
                     stage_tiles);
  return 0;
}

// k-blocks of 128 one wave may own: its X fragments (MT * 4 * blocks * 4 VGPRs) must stay in registers
inline int w4_max_blocks_per_wave(int M) { return M <= 32 ? 4 : 2; }
inline int w4_ksplit(int M, int K) {
  const int cap = kW4Waves * w4_max_blocks_per_wave(M);
  return (K / 128 + cap - 1) / cap;
}
// gemm_balance (common.h Tuning): the fewest workgroups that need no more rounds of n-tiles than `cap` would
inline int w4_balanced_groups(int units, int cap) {
  if (cap < 1) cap = 1;
  if (units <= cap) return units < 1 ? 1 : units;
  if (!tuning().gemm_balance) return cap;
  const int rounds = (units + cap - 1) / cap;
  return (units + rounds - 1) / rounds;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_awq_packed_bytes(int N, int K) { return (int64_t)(N / 16) * ((K + 127) / 128) * 1024; }
extern "C" int64_t lvllm_awq_meta_bytes(int N, int K, int group_size) {
  return w4_group_ok(group_size) ? (int64_t)(N / 16) * ((K + 127) / 128) * 64 * (128 / group_size) : 0;
}

extern "C" int lvllm_awq_pack(void* w4_packed, void* meta, const void* qweight, const void* qzeros, const void* scales,
                              int N, int K, int group_size, int dtype, void* stream) {
  LV_CHECK(dtype == LVLLM_BF16 || dtype == LVLLM_F16, "16-bit scales only");
  LV_CHECK(w4_group_ok(group_size), "group_size must be 32, 64 or 128");
  LV_CHECK(N > 0 && K > 0 && N % 16 == 0 && K % group_size == 0, "N must be a multiple of 16 and K of group_size");
  LV_CHECK(lvllm_awq_packed_bytes(N, K) < ((int64_t)1 << 32) - 16, "packed weight of 4 GiB or more");
  const int kblocks_p = (K + 127) / 128;
  const int64_t wwords = lvllm_awq_packed_bytes(N, K) / 4, mwords = lvllm_awq_meta_bytes(N, K, group_size) / 4;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(awq_pack_weight_kernel, dim3((unsigned)((wwords + 255) / 256)), dim3(256), 0, s,
                     (uint32_t*)w4_packed, (const uint32_t*)qweight, wwords, N, K, kblocks_p);
  if (dtype == LVLLM_BF16)
    hipLaunchKernelGGL(awq_pack_meta_kernel<BF16>, dim3((unsigned)((mwords + 255) / 256)), dim3(256), 0, s,
                       (uint32_t*)meta, (const uint32_t*)qzeros, (const uint16_t*)scales, mwords, N, K, group_size,
                       kblocks_p);
  else
    hipLaunchKernelGGL(awq_pack_meta_kernel<F16>, dim3((unsigned)((mwords + 255) / 256)), dim3(256), 0, s,
                       (uint32_t*)meta, (const uint32_t*)qzeros, (const uint16_t*)scales, mwords, N, K, group_size,
                       kblocks_p);
  LV_LAUNCH_CHECK();
  return 0;
}

extern "C" int lvllm_awq_dequantize(void* out, const void* qweight, const void* qzeros, const void* scales, int N,
                                    int K, int group_size, int dtype, void* stream) {
  LV_CHECK(dtype == LVLLM_BF16 || dtype == LVLLM_F16, "16-bit scales only");
  LV_CHECK(N > 0 && K > 0 && group_size > 0 && N % 8 == 0 && K % group_size == 0,
           "N must be a multiple of 8 and K of group_size");
  LV_CHECK((((uintptr_t)out) & 15) == 0, "out must be 16-byte aligned");
  const int64_t nwords = (int64_t)K * (N / 8);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LVLLM_BF16)
    hipLaunchKernelGGL(awq_dequantize_kernel<BF16>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s,
                       (uint16_t*)out, (const uint32_t*)qweight, (const uint32_t*)qzeros, (const uint16_t*)scales,
                       nwords, N, group_size);
  else
    hipLaunchKernelGGL(awq_dequantize_kernel<F16>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s,
                       (uint16_t*)out, (const uint32_t*)qweight, (const uint32_t*)qzeros, (const uint16_t*)scales,
                       nwords, N, group_size);
  LV_LAUNCH_CHECK();
  return 0;
}

extern "C" int lvllm_awq_dequantize_packed(void* out, const void* w4_packed, const void* meta, int N, int K,
                                           int group_size, int dtype, void* stream) {
  LV_CHECK(dtype == LVLLM_BF16 || dtype == LVLLM_F16, "16-bit element types only");
  LV_CHECK(w4_group_ok(group_size), "group_size must be 32, 64 or 128");
  LV_CHECK(N > 0 && K > 0 && N % 16 == 0 && K % group_size == 0, "N must be a multiple of 16 and K of group_size");
  const int kblocks_p = (K + 127) / 128;
  const int64_t nwords = lvllm_awq_packed_bytes(N, K) / 4;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LVLLM_BF16)
    hipLaunchKernelGGL(awq_dequantize_packed_kernel<BF16>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s,
                       (uint16_t*)out, (const uint32_t*)w4_packed, (const uint32_t*)meta, nwords, N, K, group_size,
                       kblocks_p);
  else
    hipLaunchKernelGGL(awq_dequantize_packed_kernel<F16>, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s,
                       (uint16_t*)out, (const uint32_t*)w4_packed, (const uint32_t*)meta, nwords, N, K, group_size,
                       kblocks_p);
  LV_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t lvllm_skinny_gemm_w4a16_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || M > 64 || N <= 0 || K < 128) return 0;
  const int ksplit = w4_ksplit(M, K);
  return ksplit > 1 ? (int64_t)ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_skinny_gemm_w4a16(void* y, const void* x, const void* w4_packed, const void* meta,
                                       const void* bias, int M, int N, int K, int group_size, int64_t ldx, int dtype,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || M > 64 || K <= 0 || (K % 128) != 0 || (N % 16) != 0 ||
      !w4_group_ok(group_size) || lvllm_awq_packed_bytes(N, K) >= ((int64_t)1 << 32) - 16 || (ldx % 8) != 0 ||
      ((int64_t)(M - 1) * ldx + K) * 2 >= ((int64_t)1 << 31) ||
      ((((uintptr_t)x | (uintptr_t)w4_packed | (uintptr_t)meta | (uintptr_t)y) & 15) != 0)) {
    set_error("lvllm_skinny_gemm_w4a16: shape outside the kernel's envelope");
    return 3;
  }
  const int kblocks = K / 128;
  const int ksplit = w4_ksplit(M, K);
  const int blocks_per_wg = (kblocks + ksplit - 1) / ksplit;
  const int blocks_per_wave = (blocks_per_wg + kW4Waves - 1) / kW4Waves;  // <= w4_max_blocks_per_wave(M)
  const int ntiles = N / 16;
  const int cus = (ntiles >= tuning().gemm_wide_min_tiles && tuning().gemm_workgroups_wide > 0)
                      ? tuning().gemm_workgroups_wide
                      : tuning().gemm_workgroups;
  const int groups = w4_balanced_groups(ntiles, cus / ksplit);
  float* partial = nullptr;
  if (ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)ksplit * M * N * 4,
             "workspace too small (see lvllm_skinny_gemm_w4a16_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  const int MT = (M + 15) / 16;
  const bool k8 = blocks_per_wave <= 2;
#define LV_W4_ARGS y, partial, x, w4_packed, meta, bias, M, N, K, ldx, blocks_per_wave, ntiles, groups, ksplit, s
#define LV_W4_MT(T_, G_)                                                             \
  switch (MT) {                                                                      \
    case 1:                                                                          \
      if (k8) launch_w4<T_, 1, 8, G_>(LV_W4_ARGS); else launch_w4<T_, 1, 16, G_>(LV_W4_ARGS); \
      break;                                                                         \
    case 2:                                                                          \
      if (k8) launch_w4<T_, 2, 8, G_>(LV_W4_ARGS); else launch_w4<T_, 2, 16, G_>(LV_W4_ARGS); \
      break;                                                                         \
    default: launch_w4<T_, 4, 8, G_>(LV_W4_ARGS); break;                             \
  }
#define LV_W4_G(T_)                                 \
  switch (group_size) {                             \
    case 32: LV_W4_MT(T_, 32) break;                \
    case 64: LV_W4_MT(T_, 64) break;                \
    default: LV_W4_MT(T_, 128) break;               \
  }
  if (dtype == LVLLM_BF16) { LV_W4_G(BF16) } else { LV_W4_G(F16) }
#undef LV_W4_G
#undef LV_W4_MT
#undef LV_W4_ARGS
  LV_LAUNCH_CHECK();
  if (ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(w4_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, ksplit);
    else
      hipLaunchKernelGGL(w4_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
