// W8A8 fp8 GEMM for prefill batches on gfx950: the fp8 sibling of int8_tiled_gemm.hip.
//   Y[M,N] = T( (acc[m,n] * sx[m]) * sw[n] + bias[n] ),  acc = sum_k float(xq[m,k]) * float(wq[n,k]) in fp32,
// any M >= 1 (meant for M > 64).  Operands are OCP e4m3fn bytes, quantised by the caller (scaled_fp8_quant): an X
// tile is re-read by every column of workgroups, quantising here would repeat the conversion N / 128 times and
// double X's LDS bytes.  sx has 1 or M entries, sw 1 or N.  The packed weight of the decode kernel
// ([N/16][K/64][lane 64][16 bytes], lane (g, c) of unit (t, b) = k 64 b + 16 g .. + 15 of row 16 t + c) is read as
// it is.
//
// Matrix instruction: v_mfma_f32_16x16x128_f8f6f4 (both operands fp8, no block scales), W the A operand and X the B
// operand as in the family: lane (g, c) ends with four consecutive n of row m = c, one 8-byte store.  A 128-k A
// operand is the lane's 16 bytes of packed unit 2 j followed by its 16 bytes of unit 2 j + 1; the instruction does not
// care which k a lane holds as long as both operands agree, so the B operand of lane (g, c) is X[c][128 j + 16 g ..
// + 15] followed by X[c][128 j + 64 + 16 g .. + 15]: two 16-byte LDS reads each.  K / 64 odd: the missing unit and
// the missing half of X come from an out-of-range buffer offset and are 0x00 = +0.
//
// Work split: a workgroup of 4 waves (2 along m x 2 along n) owns 128 rows x 128 columns and walks K in chunks of
// 128 bytes = one MFMA k-step.  A wave owns 64 x 64: 4 n-tiles x 4 m-tiles, 64 accumulator registers, 4 + 4
// fragments of 8 registers per k-step.  Two stages of 32 KiB, 64 KiB of LDS, two workgroups per CU.  (A 256-byte chunk
// -- two k-steps, 64 KiB per stage, one workgroup per CU -- was measured and lost from 256 rows on, by a third at 8192:
// profiles/fp8_tiled_gemm.md.)
//
// Data path: both operands go HBM -> registers -> LDS -> fragments.  Per chunk the workgroup stages
//   W  8 n-tiles x 2 units = 16 contiguous KiB, already in fragment order: copied linearly, read back with two
//      ds_read_b128 per lane at lane * 16 (conflict-free), by the two waves that share the n-range;
//   X  128 rows x 128 bytes: eight lanes load one row segment (coalesced), 16-byte piece q of row r is stored at
//      position q ^ (r & 7), so the row-order stores and the fragment reads (16 rows, one piece column) both spread
//      over the banks.
// The global loads of chunk i + 1 are issued before the MFMAs of chunk i and land in registers under them, are
// written to the other stage after them, and one barrier per chunk separates the stage's writers from its readers:
// half the barriers per byte of the int8 kernel, the same LDS bytes per MAC.  LDS bandwidth is the supposed bound
// (not traced).
//
// Bounds: buffer descriptors sized exactly to X ((M - 1) ldx + K bytes) and to the packed weight; rows past M,
// n-tiles past N and units past the split's end are loaded from an out-of-range offset and read zeros.  Stores are
// guarded.
//
// Few tiles: when the output has fewer tiles than the device holds workgroups (two per CU), K is split over
// blockIdx.y in whole chunks; partials travel as fp32 in the caller's workspace and a second kernel sums them in the
// order of the splits before the epilogue: a result depends on the shape and the tuning, never on timing.
#include "common.h"

namespace lvllm {
namespace {

typedef int f8t_i32x4_t __attribute__((ext_vector_type(4)));
typedef int f8t_i32x8_t __attribute__((ext_vector_type(8)));
typedef float f8t_f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kF8Threads = 256;                   // 4 waves: wave = 2 wm + wn
constexpr int kF8MT = 4;                          // m-tiles of 16 per wave: the workgroup tile has 128 rows
constexpr int kF8NTiles = 8;                      // n-tiles of 16 per workgroup tile (128 columns), 4 per wave
constexpr int kF8KS = 1;                          // MFMA k-steps of 128 per chunk
constexpr int kF8Units = 2 * kF8KS;               // packed units of 64 k per chunk
constexpr int kF8RowBytes = 128 * kF8KS;          // bytes of one X row in one chunk
constexpr int kF8Pieces = kF8RowBytes / 16;       // 16-byte pieces of such a row
constexpr int kF8Rows = 32 * kF8MT;               // rows of the workgroup tile
constexpr int kF8WBytes = kF8NTiles * kF8Units * 1024;  // W bytes of one stage
constexpr int kF8Stage = kF8WBytes + kF8Rows * kF8RowBytes;
constexpr int kF8PerCU = 2;                       // workgroups a CU holds: 2 x 64 KiB of its 160 KiB of LDS
constexpr unsigned kF8OutOfRange = 0xfffffff0u;   // >= any descriptor size: the load returns 0
constexpr int kF8MinSplitChunks = 8 / kF8KS;      // a K split owns at least 1024 k
constexpr int kF8MaxSplit = 16;

// T( (acc[r] * sx) * sw[r] + bias[r] ) for four consecutive n of one row, packed for one 8-byte store; sw4 points at
// the four channel scales, or at the single one when `per_channel` is false
template <typename T>
__device__ __forceinline__ uint2 f8t_epilogue(const f8t_f32x4_t acc, const float sxm, const float* __restrict__ sw4,
                                              const bool per_channel,
                                              const typename T::store_t* __restrict__ bias4) {
  f8t_f32x4_t w;
  if (per_channel) {
    w = *reinterpret_cast<const f8t_f32x4_t*>(sw4);
  } else {
    const float s = sw4[0];
    w = f8t_f32x4_t{s, s, s, s};
  }
  float f[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    f[r] = (acc[r] * sxm) * w[r];
    if (bias4 != nullptr) f[r] += T::to_float(bias4[r]);
  }
  uint2 o;
  o.x = (uint32_t)T::from_float(f[0]) | ((uint32_t)T::from_float(f[1]) << 16);
  o.y = (uint32_t)T::from_float(f[2]) | ((uint32_t)T::from_float(f[3]) << 16);
  return o;
}

template <typename T>
__global__ __launch_bounds__(kF8Threads, kF8PerCU) void tiled_gemm_fp8_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const uint8_t* __restrict__ xq, const uint8_t* __restrict__ wq, const float* __restrict__ sx,
    const float* __restrict__ sw, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int sx_per_row, const int sw_per_channel, const int mtiles, const int chunks_per_split) {
  constexpr int MT = kF8MT;
  constexpr int XL = kF8Rows * kF8RowBytes / (kF8Threads * 16);  // 16-byte X loads per lane and chunk
  constexpr int WL = kF8WBytes / (kF8Threads * 16);              // 16-byte W loads per lane and chunk
  constexpr int RPP = kF8Threads / kF8Pieces;                    // X rows per load pass
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // [2][ W: [8 n-tiles][units][64 lanes][16] | X: [rows][row bytes] ]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = (int)(blockIdx.x % mtiles) * kF8Rows;     // m-tiles vary fastest: neighbours share the W columns
  const int t0 = (int)(blockIdx.x / mtiles) * kF8NTiles;  // first n-tile of 16
  const int ntiles = N >> 4;
  const int total_units = K >> 6;
  const int u_begin = blockIdx.y * chunks_per_split * kF8Units;
  int u_end = u_begin + chunks_per_split * kF8Units;
  if (u_end > total_units) u_end = total_units;
  const int nchunks = (u_end - u_begin + kF8Units - 1) / kF8Units;

  // descriptors sized to the operands exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K), 0x00020000);
  __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);

  f8t_i32x4_t wreg[WL], xreg[XL];
  // chunk ci -> registers.  W load i covers unit (n-tile, k-unit) = (v / units, v % units), v = i * 4 + wave, one
  // KiB, lane * 16 within it; X pass i covers rows RPP i .. RPP i + RPP - 1, lane position p holds piece p ^ (r & mask)
  auto load_chunk = [&](const int ci) __attribute__((always_inline)) {
    const int unit0 = u_begin + ci * kF8Units;
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int v = i * 4 + wave;
      const int t = t0 + v / kF8Units, u = unit0 + v % kF8Units;
      const unsigned off = (t < ntiles && u < u_end)
                               ? ((unsigned)t * (unsigned)total_units + (unsigned)u) * 1024u + (unsigned)lane * 16u
                               : kF8OutOfRange;
      wreg[i] = __builtin_bit_cast(f8t_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int r = i * RPP + tid / kF8Pieces, q = (tid % kF8Pieces) ^ (r & (kF8Pieces - 1));
      const int m = m0 + r, u = unit0 + (q >> 2);
      const unsigned off = (m < M && u < u_end) ? (unsigned)((int64_t)m * ldx + (int64_t)u * 64 + (q & 3) * 16)
                                                : kF8OutOfRange;
      xreg[i] = __builtin_bit_cast(f8t_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
  };
  // registers -> stage ci & 1, both linear in the thread index
  auto store_chunk = [&](const int ci) __attribute__((always_inline)) {
    char* st = smem_raw + (ci & 1) * kF8Stage;
#pragma unroll
    for (int i = 0; i < WL; ++i) *reinterpret_cast<f8t_i32x4_t*>(st + (i * 4 + wave) * 1024 + lane * 16) = wreg[i];
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<f8t_i32x4_t*>(st + kF8WBytes + i * 4096 + tid * 16) = xreg[i];
  };

  f8t_f32x4_t acc[4][MT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = f8t_f32x4_t{0.f, 0.f, 0.f, 0.f};

  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int ci = 0; ci < nchunks; ++ci) {
    const bool more = ci + 1 < nchunks;  // uniform
    if (more) load_chunk(ci + 1);        // in flight under this chunk's MFMAs
    const char* st = smem_raw + (ci & 1) * kF8Stage;
#pragma unroll
    for (int s = 0; s < kF8KS; ++s) {
      f8t_i32x8_t wf[4], xf[MT];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const char* p = st + ((wn * 4 + j) * kF8Units + 2 * s) * 1024 + lane * 16;
        wf[j] = __builtin_shufflevector(*reinterpret_cast<const f8t_i32x4_t*>(p),
                                        *reinterpret_cast<const f8t_i32x4_t*>(p + 1024), 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int r = wm * 16 * MT + 16 * mt + c;
        const char* p = st + kF8WBytes + r * kF8RowBytes;
        const int sz = r & (kF8Pieces - 1);
        xf[mt] = __builtin_shufflevector(*reinterpret_cast<const f8t_i32x4_t*>(p + ((8 * s + g) ^ sz) * 16),
                                         *reinterpret_cast<const f8t_i32x4_t*>(p + ((8 * s + 4 + g) ^ sz) * 16), 0, 1,
                                         2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[j][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], xf[mt], acc[j][mt], 0, 0, 0, 0, 0, 0);
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
    const float sxm = partial != nullptr ? 0.f : sx[sx_per_row ? m : 0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n0 = (t0 + wn * 4 + j) * 16 + 4 * g;
      if (n0 >= N) continue;
      if (partial != nullptr)
        *reinterpret_cast<f8t_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = acc[j][mt];
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) = f8t_epilogue<T>(
            acc[j][mt], sxm, sw_per_channel ? sw + n0 : sw, sw_per_channel != 0, bias != nullptr ? bias + n0 : nullptr);
    }
  }
}

// y[m, n] = epilogue(partial[0, m, n] + partial[1, m, n] + ...): the fp32 sum in the order of the splits
template <typename T>
__global__ void f8t_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                  const float* __restrict__ sx, const float* __restrict__ sw,
                                  const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                  const int sx_per_row, const int sw_per_channel, const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  f8t_f32x4_t sum = *reinterpret_cast<const f8t_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const f8t_f32x4_t*>(partial + (int64_t)s * MN + i);
  const int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
  *reinterpret_cast<uint2*>(y + i) = f8t_epilogue<T>(sum, sx[sx_per_row ? m : 0], sw_per_channel ? sw + n : sw,
                                                     sw_per_channel != 0, bias != nullptr ? bias + n : nullptr);
}

struct F8Plan {
  int mtiles, nblocks;  // workgroup tiles along m and n
  int ksplit, chunks_per_split;
};

// the rule of t8_plan (int8_tiled_gemm.hip) in chunks of this kernel
inline F8Plan f8t_plan(int M, int N, int K) {
  F8Plan p;
  const int cus = tuning().gemm_workgroups;
  p.mtiles = (M + kF8Rows - 1) / kF8Rows;
  p.nblocks = (N + 16 * kF8NTiles - 1) / (16 * kF8NTiles);
  const int64_t tiles = (int64_t)p.mtiles * p.nblocks;
  const int nchunks = (K / 64 + kF8Units - 1) / kF8Units;
  int ks = 1;
  const int64_t slots = (int64_t)kF8PerCU * cus;  // fewer tiles than the CUs hold workgroups leave slots empty
  if (tiles < slots) {
    ks = (int)(slots / tiles);
    if (ks > nchunks / kF8MinSplitChunks) ks = nchunks / kF8MinSplitChunks;
    if (ks > kF8MaxSplit) ks = kF8MaxSplit;
    if (ks < 1) ks = 1;
  }
  p.chunks_per_split = (nchunks + ks - 1) / ks;
  p.ksplit = (nchunks + p.chunks_per_split - 1) / p.chunks_per_split;  // no empty split; the last may be short
  return p;
}

inline bool f8t_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && (K % 64) == 0 && (N % 16) == 0 && (int64_t)N * K < ((int64_t)1 << 32) - 16;
}

template <typename T>
int launch_f8t(void* y, float* partial, const void* xq, const void* wq, const float* sx, const float* sw,
               const void* bias, int M, int N, int K, int64_t ldx, int sx_per_row, int sw_per_channel,
               const F8Plan& p, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr size_t smem = (size_t)2 * kF8Stage;
  static_assert(smem <= 64 * 1024, "beyond 64 KiB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL(tiled_gemm_fp8_kernel<T>, dim3((unsigned)(p.mtiles * p.nblocks), p.ksplit), dim3(kF8Threads), smem, stream, (S*)y,
                     partial, (const uint8_t*)xq, (const uint8_t*)wq, sx, sw, (const S*)bias, M, N, K, ldx, sx_per_row,
                     sw_per_channel, p.mtiles, p.chunks_per_split);
  LV_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    hipLaunchKernelGGL(f8t_reduce_kernel<T>, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, (S*)y,
                       partial, sx, sw, (const S*)bias, MN, N, sx_per_row, sw_per_channel, p.ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_gemm_w8a8_fp8_workspace_bytes(int M, int N, int K) {
  if (!f8t_shape_ok(M, N, K)) return 0;
  const F8Plan p = f8t_plan(M, N, K);
  return p.ksplit > 1 ? (int64_t)p.ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_gemm_w8a8_fp8(void* y, const void* x_fp8, const void* w_packed, const float* x_scale,
                                   const float* w_scale, int x_scale_count, int w_scale_count, const void* bias, int M,
                                   int N, int K, int64_t ldx, int dtype, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(x_scale != nullptr && w_scale != nullptr, "x_scale and w_scale are device pointers");
  LV_CHECK((x_scale_count == 1 || x_scale_count == M) && (w_scale_count == 1 || w_scale_count == N),
           "x_scale has 1 or M entries, w_scale 1 or N");
  const bool sw_per_channel = w_scale_count == N && N > 1;
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || !f8t_shape_ok(M, N, K) || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) || (int64_t)M * N >= ((int64_t)1 << 40) ||
      ((((uintptr_t)x_fp8 | (uintptr_t)w_packed) & 15) != 0) || (sw_per_channel && (((uintptr_t)w_scale) & 15) != 0) ||
      (((uintptr_t)y) & 7) != 0 || (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_gemm_w8a8_fp8: shape outside the kernel's envelope");
    return 3;
  }
  const F8Plan p = f8t_plan(M, N, K);
  float* partial = nullptr;
  if (p.ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)p.ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_gemm_w8a8_fp8_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  const int per_row = x_scale_count == M && M > 1;
  if (dtype == LVLLM_BF16)
    return launch_f8t<BF16>(y, partial, x_fp8, w_packed, x_scale, w_scale, bias, M, N, K, ldx, per_row, sw_per_channel,
                            p, s);
  return launch_f8t<F16>(y, partial, x_fp8, w_packed, x_scale, w_scale, bias, M, N, K, ldx, per_row, sw_per_channel, p,
                         s);
}
