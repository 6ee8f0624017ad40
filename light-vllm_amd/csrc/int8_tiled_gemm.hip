// W8A8 int8 GEMM for prefill batches on gfx950: the operand-reusing counterpart of int8_gemm.hip.
//   Y[M,N] = T( sx[m] * (sw[n] * float(acc[m,n])) + bias[n] ),  acc = Xq . Wq^T in int32,
// any M >= 1 (meant for M > 64), same operands, same packed weight ([N/16][K/64][lane 64][16 bytes], read as it is)
// and same epilogue arithmetic as the decode kernel, so that without bias the two agree bit for bit.
//
// Work split: a workgroup of 4 waves (2 along m x 2 along n) owns an output tile of 128 rows x 128 columns and walks K
// in chunks of 128 bytes (two k-steps of v_mfma_i32_16x16x64_i8).  A wave owns 64 rows x 64 columns: 4 n-tiles x 4
// m-tiles of 16 x 16, 64 accumulator registers; 64 KiB of LDS, two workgroups per CU.  W is the MFMA A operand and X
// the B operand, as in the family: lane (g, c) ends with four consecutive n of row m = c, one 8-byte store.  (A 256 x
// 128 tile with 8 m-tiles per wave was measured and lost: profiles/int8_tiled_gemm.md.)
//
// Data path: both operands go HBM -> registers -> LDS -> fragments.  Per chunk the workgroup stages
//   W  8 n-tiles x 2 k-steps = 16 contiguous KiB, already in fragment order: copied linearly, read back with one
//      ds_read_b128 per lane at lane * 16 (conflict-free), by the two waves that share the n-range;
//   X  128 rows x 128 bytes: eight lanes load one row segment (coalesced), chunk q of row r is stored at position
//      q ^ (r & 7), so the row-order stores and the fragment reads (16 rows, one chunk column) both spread over all
//      banks.
// LDS holds two stages; the global loads of chunk i + 1 are issued before the MFMAs of chunk i and land in registers
// under them, are written to the other stage after them, and one barrier per chunk separates the stage's writers from
// its readers.  Per k-step a wave reads 4 + 4 fragments for 16 MFMAs: 128 bytes of LDS per clock and CU if an MFMA
// takes 16 clocks -- LDS bandwidth and the per-chunk barrier are the supposed bound (not traced), HBM is not.
//
// Bounds: buffer descriptors sized exactly to X and to the packed weight; rows past M, n-tiles past N and k-steps
// past the split's end are loaded from an out-of-range offset and read zeros.  Stores are guarded.
//
// Few tiles: when the output has fewer tiles than the device holds workgroups (two per CU), K is split over blockIdx.y in whole chunks;
// partials travel as int32 in the caller's workspace and a second kernel sums them as int32 before the epilogue, so
// the result does not depend on the split (|acc| <= K * 2^14 < 2^31 for K < 131072).
#include "common.h"

namespace lvllm {
namespace {

typedef int t8_i32x4_t __attribute__((ext_vector_type(4)));
typedef float t8_f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kT8Threads = 256;                  // 4 waves: wave = 2 wm + wn
constexpr int kT8MT = 4;                         // m-tiles of 16 per wave: the workgroup tile has 128 rows
constexpr int kT8NTiles = 8;                     // n-tiles of 16 per workgroup tile (128 columns), 4 per wave
constexpr int kT8KC = 2;                         // k-steps of 64 per chunk
constexpr int kT8RowBytes = kT8KC * 64;          // bytes of one X row in one chunk
constexpr int kT8WBytes = kT8NTiles * kT8KC * 1024;  // W bytes of one stage
constexpr unsigned kT8OutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kT8MaxK = 131072;                  // K below this: no int32 overflow whatever the operands
constexpr int kT8MinSplitChunks = 8;             // a K split owns at least 1024 k
constexpr int kT8MaxSplit = 16;

// The arithmetic of i8_epilogue in int8_gemm.hip, operation for operation: T( sx * (sw[r] * float(acc[r])) + bias[r] )
// for four consecutive n of one row, packed for one 8-byte store.
template <typename T>
__device__ __forceinline__ uint2 t8_epilogue(const t8_i32x4_t acc, const float sxm, const float* __restrict__ sw4,
                                             const typename T::store_t* __restrict__ bias4) {
  const t8_f32x4_t w = *reinterpret_cast<const t8_f32x4_t*>(sw4);
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

template <typename T>
__global__ __launch_bounds__(kT8Threads, 2) void tiled_gemm_i8_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    int* __restrict__ partial,            // [ksplit, M, N]  (ksplit > 1)
    const int8_t* __restrict__ xq, const int8_t* __restrict__ wq, const float* __restrict__ sx,
    const float* __restrict__ sw, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int mtiles, const int chunks_per_split) {
  constexpr int MT = kT8MT;
  constexpr int ROWS = 32 * MT;                               // rows of the workgroup tile
  constexpr int XL = ROWS * kT8RowBytes / (kT8Threads * 16);  // 16-byte X loads per lane and chunk (= MT)
  constexpr int WL = kT8WBytes / (kT8Threads * 16);           // 16-byte W loads per lane and chunk (= 4)
  constexpr int STAGE = kT8WBytes + ROWS * kT8RowBytes;
  static_assert(kT8RowBytes == 128, "the swizzle below is for rows of eight 16-byte chunks");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // [2][ W: [8 n-tiles][KC][64 lanes][16] | X: [ROWS][128] ]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = (int)(blockIdx.x % mtiles) * ROWS;      // m-tiles vary fastest: neighbours share the W columns
  const int t0 = (int)(blockIdx.x / mtiles) * kT8NTiles;  // first n-tile of 16
  const int ntiles = N >> 4;
  const int total_steps = K >> 6;
  const int s_begin = blockIdx.y * chunks_per_split * kT8KC;
  int s_end = s_begin + chunks_per_split * kT8KC;
  if (s_end > total_steps) s_end = total_steps;
  const int nchunks = (s_end - s_begin + kT8KC - 1) / kT8KC;

  // descriptors sized to the operands exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K), 0x00020000);
  __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);

  t8_i32x4_t wreg[WL], xreg[XL];
  // chunk ci -> registers.  W unit u = i * 4 + wave is (n-tile u / KC, k-step u % KC), one KiB, lane * 16 within it;
  // X pass i covers rows 32 i .. 32 i + 31, eight lanes per row, lane position p holds chunk p ^ (r & 7)
  auto load_chunk = [&](const int ci) __attribute__((always_inline)) {
    const int step0 = s_begin + ci * kT8KC;
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int u = i * 4 + wave;
      const int t = t0 + u / kT8KC, step = step0 + u % kT8KC;
      const unsigned off = (t < ntiles && step < s_end)
                               ? ((unsigned)t * (unsigned)total_steps + (unsigned)step) * 1024u + (unsigned)lane * 16u
                               : kT8OutOfRange;
      wreg[i] = __builtin_bit_cast(t8_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int r = i * 32 + (tid >> 3), q = (tid & 7) ^ (r & 7);
      const int m = m0 + r, step = step0 + (q >> 2);
      const unsigned off = (m < M && step < s_end) ? (unsigned)((int64_t)m * ldx + (int64_t)step * 64 + (q & 3) * 16)
                                                   : kT8OutOfRange;
      xreg[i] = __builtin_bit_cast(t8_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
  };
  // registers -> stage ci & 1, both linear in the thread index
  auto store_chunk = [&](const int ci) __attribute__((always_inline)) {
    char* st = smem_raw + (ci & 1) * STAGE;
#pragma unroll
    for (int i = 0; i < WL; ++i) *reinterpret_cast<t8_i32x4_t*>(st + (i * 4 + wave) * 1024 + lane * 16) = wreg[i];
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<t8_i32x4_t*>(st + kT8WBytes + i * 4096 + tid * 16) = xreg[i];
  };

  t8_i32x4_t acc[4][MT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = t8_i32x4_t{0, 0, 0, 0};

  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int ci = 0; ci < nchunks; ++ci) {
    const bool more = ci + 1 < nchunks;  // uniform
    if (more) load_chunk(ci + 1);        // in flight under this chunk's MFMAs
    const char* st = smem_raw + (ci & 1) * STAGE;
#pragma unroll
    for (int s = 0; s < kT8KC; ++s) {
      t8_i32x4_t wf[4], xf[MT];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        wf[j] = *reinterpret_cast<const t8_i32x4_t*>(st + ((wn * 4 + j) * kT8KC + s) * 1024 + lane * 16);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        xf[mt] = *reinterpret_cast<const t8_i32x4_t*>(st + kT8WBytes + (wm * 16 * MT + 16 * mt + c) * kT8RowBytes +
                                                      (((4 * s + g) ^ (c & 7)) * 16));
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[j][mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[j], xf[mt], acc[j][mt], 0, 0, 0);
    }
    // the other stage was last read in the previous iteration, which every wave left through the barrier below
    if (more) {
      store_chunk(ci + 1);
      __syncthreads();
    }
  }

  // lane (g, c): columns n0 .. n0 + 3 of row m
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * 16 * MT + 16 * mt + c;
    if (m >= M) continue;
    const float sxm = partial != nullptr ? 0.f : sx[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n0 = (t0 + wn * 4 + j) * 16 + 4 * g;
      if (n0 >= N) continue;
      if (partial != nullptr)
        *reinterpret_cast<t8_i32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = acc[j][mt];
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) =
            t8_epilogue<T>(acc[j][mt], sxm, sw + n0, bias != nullptr ? bias + n0 : nullptr);
    }
  }
}

// y[m, n] = epilogue(sum_s partial[s, m, n]): the int32 sum first, the scales after
template <typename T>
__global__ void t8_reduce_kernel(typename T::store_t* __restrict__ y, const int* __restrict__ partial,
                                 const float* __restrict__ sx, const float* __restrict__ sw,
                                 const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                 const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  t8_i32x4_t sum = *reinterpret_cast<const t8_i32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const t8_i32x4_t*>(partial + (int64_t)s * MN + i);
  const int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
  *reinterpret_cast<uint2*>(y + i) = t8_epilogue<T>(sum, sx[m], sw + n, bias != nullptr ? bias + n : nullptr);
}

struct T8Plan {
  int mtiles, nblocks;  // workgroup tiles along m and n
  int ksplit, chunks_per_split;
};

inline T8Plan t8_plan(int M, int N, int K) {
  T8Plan p;
  const int cus = tuning().gemm_workgroups;
  const int nblocks = (N + 127) / 128;
  p.mtiles = (M + 32 * kT8MT - 1) / (32 * kT8MT);
  p.nblocks = nblocks;
  const int64_t tiles = (int64_t)p.mtiles * nblocks;
  const int nchunks = (K / 64 + kT8KC - 1) / kT8KC;
  int ks = 1;
  const int64_t slots = 2 * (int64_t)cus;  // two workgroups fit a CU: fewer tiles than that leave slots empty
  if (tiles < slots) {
    ks = (int)(slots / tiles);
    if (ks > nchunks / kT8MinSplitChunks) ks = nchunks / kT8MinSplitChunks;
    if (ks > kT8MaxSplit) ks = kT8MaxSplit;
    if (ks < 1) ks = 1;
  }
  p.chunks_per_split = (nchunks + ks - 1) / ks;
  p.ksplit = (nchunks + p.chunks_per_split - 1) / p.chunks_per_split;  // no empty split; the last may be short
  return p;
}

inline bool t8_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && K < kT8MaxK && (K % 64) == 0 && (N % 16) == 0 &&
         (int64_t)N * K < ((int64_t)1 << 32) - 16;
}

template <typename T>
void launch_t8(void* y, int* partial, const void* xq, const void* wq, const float* sx, const float* sw,
               const void* bias, int M, int N, int K, int64_t ldx, const T8Plan& p, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr size_t smem = (size_t)2 * (kT8WBytes + 32 * kT8MT * kT8RowBytes);
  static_assert(smem <= 64 * 1024, "beyond 64 KiB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL(tiled_gemm_i8_kernel<T>, dim3((unsigned)(p.mtiles * p.nblocks), p.ksplit), dim3(kT8Threads), smem, stream, (S*)y,
                     partial, (const int8_t*)xq, (const int8_t*)wq, sx, sw, (const S*)bias, M, N, K, ldx, p.mtiles,
                     p.chunks_per_split);
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_gemm_w8a8_int8_workspace_bytes(int M, int N, int K) {
  if (!t8_shape_ok(M, N, K)) return 0;
  const T8Plan p = t8_plan(M, N, K);
  return p.ksplit > 1 ? (int64_t)p.ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_gemm_w8a8_int8(void* y, const void* x_q, const void* w_packed, const float* x_scale,
                                    const float* w_scale, const void* bias, int M, int N, int K, int64_t ldx, int dtype,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(x_scale != nullptr && w_scale != nullptr, "x_scale [M] and w_scale [N] are device pointers");
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || !t8_shape_ok(M, N, K) || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) || (int64_t)M * N >= ((int64_t)1 << 40) ||
      ((((uintptr_t)x_q | (uintptr_t)w_packed | (uintptr_t)w_scale) & 15) != 0) || (((uintptr_t)y) & 7) != 0 ||
      (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_gemm_w8a8_int8: shape outside the kernel's envelope");
    return 3;
  }
  const T8Plan p = t8_plan(M, N, K);
  int* partial = nullptr;
  if (p.ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)p.ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_gemm_w8a8_int8_workspace_bytes)");
    partial = (int*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LVLLM_BF16)
    launch_t8<BF16>(y, partial, x_q, w_packed, x_scale, w_scale, bias, M, N, K, ldx, p, s);
  else
    launch_t8<F16>(y, partial, x_q, w_packed, x_scale, w_scale, bias, M, N, K, ldx, p, s);
  LV_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    const int grid = (int)((MN / 4 + 255) / 256);
    if (dtype == LVLLM_BF16)
      hipLaunchKernelGGL(t8_reduce_kernel<BF16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale, w_scale,
                         (const uint16_t*)bias, MN, N, p.ksplit);
    else
      hipLaunchKernelGGL(t8_reduce_kernel<F16>, dim3(grid), dim3(256), 0, s, (uint16_t*)y, partial, x_scale, w_scale,
                         (const uint16_t*)bias, MN, N, p.ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}
