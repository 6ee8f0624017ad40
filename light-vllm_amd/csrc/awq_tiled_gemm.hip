// W4A16 (AWQ int4, group-quantised) GEMM for prefill batches on gfx950: the operand-reusing counterpart of awq_gemm.hip.
//   Y[M,N] = T( sum_k X[m,k] . Wd[k,n] (+ bias) ),  Wd[k,n] = T( float(q[k,n] - z[k/G,n]) * float(s[k/G,n]) ),
// any M >= 1 (meant for M > 64), bf16/f16 activations, fp32 accumulate, the same packed pair ([N/16][K/128][lane 64]
// [16 bytes] + metadata [N/16][K/128][16][128/G], read as it is) and the same dequantisation (w4_dequant.h) as the
// decode kernel: Wd is the same bits in both and in lvllm_awq_dequantize_packed.
//
// Work split: a workgroup of 4 waves owns an output tile of 128 rows x 128 columns; the waves split N ONLY: a wave owns
// all 128 rows (8 m-tiles of 16) x 32 columns (2 n-tiles of 16), 16 accumulator tiles = 64 fp32 registers.  W is the
// MFMA A operand and X the B operand of v_mfma_f32_16x16x32_{bf16,f16}, as in the family: lane (g, c) ends with four
// consecutive n of row m = c, one 8-byte store.
//
// W never touches LDS.  The pack order is the A-fragment order (lane (g, c) of unit (n-tile, k-block) holds
// q[128 b + 32 s + 8 g + e][16 t + c], word s = k-step s) and an n-tile has exactly one consumer wave in the
// workgroup, so that wave loads its units HBM / L2 -> VGPR with one buffer_load_b128 per lane, n-tile and k-block and
// the row's groups with one metadata load, and dequantises in registers: every weight element is dequantised once per
// workgroup tile and each dequantised fragment feeds 8 MFMAs.  (With a 2 x 2 split of the waves every fragment would
// be dequantised twice per tile or travel through LDS as 16-bit.)
//
// X goes through LDS, shared by the four waves.  Per k-chunk of 64 elements (two k-steps) the workgroup stages 128
// rows x 128 bytes: eight lanes load one row segment (coalesced), 16-byte chunk q of row r is stored at position
// q ^ (r & 7), so the row-order stores and the fragment reads (16 rows, one chunk column) both spread over all banks
// (the swizzle of int8_tiled_gemm.hip, which has 128-byte rows as well).  Two stages (2 x 16 KiB): the global loads
// of chunk i + 1 are issued before the MFMAs of chunk i, land in registers under them and are written to the other
// stage after them; one barrier per chunk separates a stage's writers from its readers.  32 KiB of LDS: occupancy is
// bounded by registers; built for two workgroups per CU so that one workgroup's dequantisation runs under the
// other's MFMAs.
//
// Pipeline inside the wave: the packed words and metadata of k-block b + 1 are in flight while block b is computed,
// and the A fragments of k-step s + 1 are dequantised before the MFMAs of k-step s are issued, so that the scheduler
// has independent VALU work to put between them.
//
// Bounds: buffer descriptors sized exactly to X, the packed weight and the metadata; rows past M, n-tiles past N and
// k-blocks past a split's end are loaded from an out-of-range offset and read zeros (nibble 0, scale 0, zero 0
// dequantise to 0).  Stores are guarded.
//
// Few tiles: when the output has fewer tiles than the device holds workgroups (two per CU), K is split over blockIdx.y
// in whole k-blocks; fp32 partials travel in the caller's workspace and a second kernel sums them in the order of the
// splits and applies bias and rounding.  Unlike the int8 kernel's the sum is not exact, so the result may depend on
// the split; it is deterministic for a given shape and tuning.
#include "common.h"
#include "w4_dequant.h"

namespace lvllm {
namespace {

constexpr int kT4Threads = 256;         // 4 waves along n
constexpr int kT4MT = 8;                // m-tiles of 16 per wave = per workgroup tile (128 rows)
constexpr int kT4NT = 2;                // n-tiles of 16 per wave; 8 per workgroup tile (128 columns)
constexpr int kT4Rows = 16 * kT4MT;
constexpr int kT4RowBytes = 128;        // one X row of one chunk: 64 elements, two k-steps
constexpr int kT4Stage = kT4Rows * kT4RowBytes;
constexpr int kT4XL = kT4Stage / (kT4Threads * 16);  // 16-byte X loads per lane and chunk (= 4)
constexpr int kT4MinSplitBlocks = 8;    // a K split owns at least 1024 k
constexpr int kT4MaxSplit = 16;

template <typename T, int G>
__global__ __launch_bounds__(kT4Threads, 2) void tiled_gemm_w4_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const typename T::store_t* __restrict__ x, const uint32_t* __restrict__ w4, const uint32_t* __restrict__ meta,
    const typename T::store_t* __restrict__ bias, const int M, const int N, const int K, const int64_t ldx,
    const int mtiles, const int blocks_per_split) {
  constexpr int MT = kT4MT, NT = kT4NT;
  constexpr int MW = 128 / G;  // metadata words per row and k-block
  static_assert(G == 32 || G == 64 || G == 128, "group sizes of the envelope");
  static_assert(kT4RowBytes == 128, "the swizzle below is for rows of eight 16-byte chunks");
  __shared__ __attribute__((aligned(16))) char smem[2 * kT4Stage];  // [2][128 rows][128 bytes], swizzled

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int m0 = (int)(blockIdx.x % mtiles) * kT4Rows;              // m-tiles vary fastest: neighbours share the W columns
  const int t0 = (int)(blockIdx.x / mtiles) * (4 * NT) + wave * NT;  // this wave's first n-tile of 16
  const int ntiles = N >> 4, kblocks = K >> 7;
  const int b_begin = blockIdx.y * blocks_per_split;
  int nblk = kblocks - b_begin;  // k-blocks of this split
  nblk = nblk < 0 ? 0 : (nblk > blocks_per_split ? blocks_per_split : nblk);
  const int nchunks = 2 * nblk;

  // descriptors sized to the operands exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc((void*)w4, 0, (int)((int64_t)ntiles * kblocks * 1024), 0x00020000);
  __amdgpu_buffer_rsrc_t mr =
      __builtin_amdgcn_make_buffer_rsrc((void*)meta, 0, (int)((int64_t)ntiles * kblocks * 64 * MW), 0x00020000);
  __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(((int64_t)(M - 1) * ldx + K) * 2), 0x00020000);

  // ---- W: unit (n-tile t0 + j, k-block b_begin + b) -> registers; a mask of all ones puts the offset out of range
  unsigned w_base[NT], m_base[NT], tmask[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const unsigned unit0 = (unsigned)(t0 + j) * (unsigned)kblocks + (unsigned)b_begin;
    w_base[j] = unit0 * 1024u + (unsigned)lane * 16u;
    m_base[j] = unit0 * (64u * MW) + (unsigned)c * (4u * MW);
    tmask[j] = t0 + j < ntiles ? 0u : ~0u;
  }
  auto load_w = [&](q_u32x4_t (&a)[NT], uint32_t (&m)[NT][MW], const int b) __attribute__((always_inline)) {
    const unsigned bmask = b < nblk ? 0u : ~0u;  // uniform
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      a[j] = __builtin_amdgcn_raw_buffer_load_b128(wr, (w_base[j] + (unsigned)b * 1024u) | tmask[j] | bmask, 0, 0);
      w4_load_meta<MW>(m[j], mr, (m_base[j] + (unsigned)b * (64u * MW)) | tmask[j] | bmask);
    }
  };
  // the A fragments of k-step ks (0..3) of a k-block: 4 pairs per n-tile with the constants of the k-step's group
  auto dequant = [&](const q_u32x4_t (&a)[NT], const uint32_t (&m)[NT][MW], const int ks, q_u32x4_t (&af)[NT])
                     __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const W4Dequant<T> d(m[j][ks * MW / 4]);
      af[j] = w4_dequant_word<T>(a[j][ks], d);
    }
  };

  // ---- X: chunk ci -> registers -> stage.  Pass i covers rows 32 i .. 32 i + 31, eight lanes per row; lane position
  // p = tid & 7 holds chunk p ^ (r & 7), so the store is linear in the thread index
  unsigned x_base[kT4XL], xmask[kT4XL];
#pragma unroll
  for (int i = 0; i < kT4XL; ++i) {
    const int r = i * 32 + (tid >> 3), q = (tid & 7) ^ (r & 7);
    const int m = m0 + r;
    xmask[i] = m < M ? 0u : ~0u;
    x_base[i] = (unsigned)(((int64_t)m * ldx + (int64_t)b_begin * 128 + q * 8) * 2);  // < 2^31 where m < M
  }
  q_u32x4_t xreg[kT4XL];
  auto load_x = [&](const int ci) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kT4XL; ++i)
      xreg[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, (x_base[i] + (unsigned)ci * kT4RowBytes) | xmask[i], 0, 0);
  };
  auto store_x = [&](const int stage) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kT4XL; ++i)
      *reinterpret_cast<q_u32x4_t*>(smem + stage * kT4Stage + i * 4096 + tid * 16) = xreg[i];
  };

  q_f32x4_t acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = q_f32x4_t{0.f, 0.f, 0.f, 0.f};

  q_u32x4_t wq[NT], wn[NT], af[NT];
  uint32_t mq[NT][MW], mn[NT][MW];
  if (nchunks > 0) {  // uniform
    load_w(wq, mq, 0);
    load_x(0);
    store_x(0);
    __syncthreads();
    dequant(wq, mq, 0, af);
  }
  for (int b = 0; b < nblk; ++b) {
    load_w(wn, mn, b + 1);  // in flight under this block's MFMAs (zeros past the split's end)
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // chunk ci = 2 b + h lies in stage h
      const int ci = 2 * b + h;
      const bool more = ci + 1 < nchunks;  // uniform
      if (more) load_x(ci + 1);            // in flight under this chunk's MFMAs
      const char* st = smem + h * kT4Stage;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ks = 2 * h + s;
        q_u32x4_t xf[MT], an[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          xf[mt] = *reinterpret_cast<const q_u32x4_t*>(st + (16 * mt + c) * kT4RowBytes + (((4 * s + g) ^ (c & 7)) * 16));
        // the next k-step's fragments, independent of the MFMAs below
        if (ks < 3) dequant(wq, mq, ks + 1, an); else dequant(wn, mn, 0, an);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[j][mt] = w4_mfma<T>(af[j], xf[mt], acc[j][mt]);
#pragma unroll
        for (int j = 0; j < NT; ++j) af[j] = an[j];
      }
      // the other stage was last read in the previous chunk, which every wave left through the barrier below
      if (more) {
        store_x(h ^ 1);
        __syncthreads();
      }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      wq[j] = wn[j];
#pragma unroll
      for (int i = 0; i < MW; ++i) mq[j][i] = mn[j][i];
    }
  }

  // lane (g, c): columns n0 .. n0 + 3 of row m
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + 16 * mt + c;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n0 = (t0 + j) * 16 + 4 * g;
      if (n0 >= N) continue;
      q_f32x4_t sum = acc[j][mt];
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
  }
}

// y[m, n] = T(sum_s partial[s, m, n] + bias[n]), s in ascending order
template <typename T>
__global__ void t4_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
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

struct T4Plan {
  int mtiles, nblocks;  // workgroup tiles along m and n
  int ksplit, blocks_per_split;
};

// the rule of t8_plan (int8_tiled_gemm.hip) in k-blocks of 128
inline T4Plan t4_plan(int M, int N, int K) {
  T4Plan p;
  p.mtiles = (M + kT4Rows - 1) / kT4Rows;
  p.nblocks = (N + 127) / 128;
  const int64_t tiles = (int64_t)p.mtiles * p.nblocks;
  const int kblocks = K / 128;
  int ks = 1;
  const int64_t slots = 2 * (int64_t)tuning().gemm_workgroups;  // two workgroups fit a CU: fewer tiles leave slots empty
  if (tiles < slots) {
    ks = (int)(slots / tiles);
    if (ks > kblocks / kT4MinSplitBlocks) ks = kblocks / kT4MinSplitBlocks;
    if (ks > kT4MaxSplit) ks = kT4MaxSplit;
    if (ks < 1) ks = 1;
  }
  p.blocks_per_split = (kblocks + ks - 1) / ks;
  p.ksplit = (kblocks + p.blocks_per_split - 1) / p.blocks_per_split;  // no empty split; the last may be short
  return p;
}

inline bool t4_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && (K % 128) == 0 && (N % 16) == 0 &&
         (int64_t)(N / 16) * (K / 128) * 1024 < ((int64_t)1 << 32) - 16;
}

template <typename T, int G>
void launch_t4(void* y, float* partial, const void* x, const void* w4, const void* meta, const void* bias, int M, int N,
               int K, int64_t ldx, const T4Plan& p, hipStream_t stream) {
  using S = typename T::store_t;
  hipLaunchKernelGGL((tiled_gemm_w4_kernel<T, G>), dim3((unsigned)(p.mtiles * p.nblocks), p.ksplit), dim3(kT4Threads), 0,
                     stream, (S*)y, partial, (const S*)x, (const uint32_t*)w4, (const uint32_t*)meta, (const S*)bias, M,
                     N, K, ldx, p.mtiles, p.blocks_per_split);
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_gemm_w4a16_workspace_bytes(int M, int N, int K) {
  if (!t4_shape_ok(M, N, K)) return 0;
  const T4Plan p = t4_plan(M, N, K);
  return p.ksplit > 1 ? (int64_t)p.ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_gemm_w4a16(void* y, const void* x, const void* w4_packed, const void* meta, const void* bias,
                                int M, int N, int K, int group_size, int64_t ldx, int dtype, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || !t4_shape_ok(M, N, K) || !w4_group_ok(group_size) || ldx < K ||
      (ldx % 8) != 0 || ((int64_t)(M - 1) * ldx + K) * 2 >= ((int64_t)1 << 31) ||
      (int64_t)M * N >= ((int64_t)1 << 40) || ((((uintptr_t)x | (uintptr_t)w4_packed | (uintptr_t)meta) & 15) != 0) || (((uintptr_t)y) & 7) != 0 ||
      (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_gemm_w4a16: shape outside the kernel's envelope");
    return 3;
  }
  const T4Plan p = t4_plan(M, N, K);
  float* partial = nullptr;
  if (p.ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)p.ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_gemm_w4a16_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
#define LV_T4_G(T_)                                                                                             \
  switch (group_size) {                                                                                         \
    case 32: launch_t4<T_, 32>(y, partial, x, w4_packed, meta, bias, M, N, K, ldx, p, s); break;                \
    case 64: launch_t4<T_, 64>(y, partial, x, w4_packed, meta, bias, M, N, K, ldx, p, s); break;                \
    default: launch_t4<T_, 128>(y, partial, x, w4_packed, meta, bias, M, N, K, ldx, p, s); break;               \
  }
  if (dtype == LVLLM_BF16) { LV_T4_G(BF16) } else { LV_T4_G(F16) }
#undef LV_T4_G
  LV_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(t4_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, p.ksplit);
    else
      hipLaunchKernelGGL(t4_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial,
                         (const uint16_t*)bias, MN, N, p.ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
