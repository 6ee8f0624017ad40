// bf16 / f16 GEMM for prefill batches on gfx950: the 16-bit member of the LDS-tiled family (int8_tiled_gemm.hip,
// awq_tiled_gemm.hip, fp8_tiled_gemm.hip, mxfp4_tiled_gemm.hip) and the big-M sibling of skinny_gemm.hip.
//   Y[M,N] = epilogue(acc[m,n]),  acc = sum_k float(x[m,k]) * float(w[n,k]) in fp32,
// any M >= 1 (meant for M > 64).  The weight is read in the order lvllm_pack_weight writes for the decode kernels
// ([N/16][K/32][lane 64][16 bytes], lane (g, c) of unit (t, b) = k 32 b + 8 g .. + 7 of row 16 t + c): no second
// packing, no row-major W.
//
// Epilogues (template parameter ACT), arithmetic pinned so that a fused launch leaves the bits of the unfused sequence:
//   0  y = T(acc + float(bias[n])), one rounding; bias may be null
//   1  y = gelu_erf(T(acc + bias)): the value is rounded to T first, then the arithmetic of lvllm_gelu (activation.h)
//   2  SwiGLU: W rows are [gate (N/2) | up (N/2)], y is [M, N/2] = silu_mul(T(gate + bias), T(up + bias)), the
//      arithmetic of lvllm_silu_and_mul (activation.h).  A workgroup's 128 columns are then 4 gate n-tiles and the 4
//      up n-tiles of the same output columns (n-tiles t and t + N/32), two of each per wave: a lane holds gate and up
//      of the same four output columns and the product never leaves registers.  K is never split.
//
// Matrix instruction: v_mfma_f32_16x16x32_bf16 / _f16, W the A operand and X the B operand as in the family: lane
// (g, c) holds W[16 t + c][32 b + 8 g .. + 7] (its 16 bytes of the packed unit) and X[m = c][32 b + 8 g .. + 7], and
// ends with four consecutive n of row m = c, one 8-byte store.
//
// Work split: a workgroup of 4 waves (2 along m x 2 along n) owns 128 rows x 128 columns and walks K in chunks of 64
// elements = 128 bytes of a row = two packed units per n-tile = two MFMA k-steps.  A wave owns 64 x 64: 4 n-tiles x 4
// m-tiles, 64 accumulator registers, 4 + 4 fragments of 4 registers per k-step.  Two stages of 32 KiB, 64 KiB of LDS,
// two workgroups per CU.
//
// Data path: both operands go HBM -> registers -> LDS -> fragments.  Per chunk the workgroup stages
//   W  8 n-tiles x 2 units = 16 KiB, already in fragment order: copied linearly, read back with one ds_read_b128 per
//      lane and fragment at lane * 16 (conflict-free), by the two waves that share the n-range;
//   X  128 rows x 128 bytes: eight lanes load one row segment (coalesced), 16-byte piece q of row r is stored at
//      position q ^ (r & 7), so the row-order stores and the fragment reads (16 rows, one piece column) both spread
//      over the banks.
// The global loads of chunk i + 1 are issued before the MFMAs of chunk i and land in registers under them, are
// written to the other stage after them, and one barrier per chunk separates the stage's writers from its readers.
//
// Bounds: buffer descriptors sized exactly to X (((M - 1) ldx + K) * 2 bytes) and to the packed weight; rows past M,
// n-tiles past N and units past K or past the split's end are loaded from an out-of-range offset and read zeros
// (K / 32 odd: the missing half chunk is zero).  Stores are guarded.
//
// Few tiles: when the output has fewer tiles than the device holds workgroups (two per CU), K is split over
// blockIdx.y in whole chunks, at least 1024 k each; partials travel as fp32 in the caller's workspace and a second
// kernel sums them in the order of the splits before the epilogue: a result depends on the shape and the tuning, never
// on timing.
#include "activation.h"
#include "common.h"

namespace lvllm {
namespace {

typedef int dt_i32x4_t __attribute__((ext_vector_type(4)));
typedef float dt_f32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 dt_bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 dt_f16x8_t __attribute__((ext_vector_type(8)));

constexpr int kDtThreads = 256;                  // 4 waves: wave = 2 wm + wn
constexpr int kDtMT = 4;                         // m-tiles of 16 per wave: the workgroup tile has 128 rows
constexpr int kDtNTiles = 8;                     // n-tiles of 16 per workgroup tile (128 columns), 4 per wave
constexpr int kDtUnits = 2;                      // packed units of 32 k (= MFMA k-steps) per chunk
constexpr int kDtRowBytes = 64 * kDtUnits;       // bytes of one X row in one chunk
constexpr int kDtPieces = kDtRowBytes / 16;      // 16-byte pieces of such a row
constexpr int kDtRows = 32 * kDtMT;              // rows of the workgroup tile
constexpr int kDtWBytes = kDtNTiles * kDtUnits * 1024;  // W bytes of one stage
constexpr int kDtStage = kDtWBytes + kDtRows * kDtRowBytes;
constexpr int kDtPerCU = 2;                      // workgroups a CU holds: 2 x 64 KiB of its 160 KiB of LDS
constexpr unsigned kDtOutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kDtMinSplitChunks = 1024 / (32 * kDtUnits);  // a K split owns at least 1024 k
constexpr int kDtMaxSplit = 16;

template <typename T>
__device__ __forceinline__ dt_f32x4_t dt_mfma(dt_i32x4_t a, dt_i32x4_t b, dt_f32x4_t c);
template <>
__device__ __forceinline__ dt_f32x4_t dt_mfma<BF16>(dt_i32x4_t a, dt_i32x4_t b, dt_f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dt_bf16x8_t, a), __builtin_bit_cast(dt_bf16x8_t, b),
                                                 c, 0, 0, 0);
}
template <>
__device__ __forceinline__ dt_f32x4_t dt_mfma<F16>(dt_i32x4_t a, dt_i32x4_t b, dt_f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(dt_f16x8_t, a), __builtin_bit_cast(dt_f16x8_t, b), c,
                                                0, 0, 0);
}

// T(acc[r] + float(bias[r])) for four consecutive n of one row: the projection's value as act = 0 stores it
template <typename T>
__device__ __forceinline__ void dt_round4(typename T::store_t (&o)[4], const dt_f32x4_t acc,
                                          const typename T::store_t* __restrict__ bias4) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float f = acc[r];
    if (bias4 != nullptr) f += T::to_float(bias4[r]);
    o[r] = T::from_float(f);
  }
}

__device__ __forceinline__ uint2 dt_pack4(const uint16_t (&v)[4]) {
  uint2 o;
  o.x = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
  o.y = (uint32_t)v[2] | ((uint32_t)v[3] << 16);
  return o;
}

// epilogue 0 or 1 of four consecutive n of one row, packed for one 8-byte store
template <typename T, int ACT>
__device__ __forceinline__ uint2 dt_epilogue(const dt_f32x4_t acc, const typename T::store_t* __restrict__ bias4) {
  typename T::store_t v[4];
  dt_round4<T>(v, acc, bias4);
  if (ACT == 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf<T>(v[r]);
  }
  return dt_pack4(v);
}

template <typename T, int ACT>
__global__ __launch_bounds__(kDtThreads, kDtPerCU) void dense_tiled_gemm_kernel(
    typename T::store_t* __restrict__ y,  // [M, N] (N / 2 for ACT 2), rows ldy apart  (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]                            (ksplit > 1)
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, const typename T::store_t* __restrict__ bias,
    const int M, const int N, const int K, const int64_t ldx, const int64_t ldy, const int mtiles,
    const int chunks_per_split) {
  constexpr int MT = kDtMT;
  constexpr int XL = kDtRows * kDtRowBytes / (kDtThreads * 16);  // 16-byte X loads per lane and chunk
  constexpr int WL = kDtWBytes / (kDtThreads * 16);              // 16-byte W loads per lane and chunk
  constexpr int RPP = kDtThreads / kDtPieces;                    // X rows per load pass
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // [2][ W: [8 slots][units][64 lanes][16] | X: [rows][row bytes] ]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = (int)(blockIdx.x % mtiles) * kDtRows;  // m-tiles vary fastest: neighbours share the W columns
  const int nb = (int)(blockIdx.x / mtiles);
  const int ntiles = N >> 4;
  const int half = N >> 5;  // ACT 2: n-tiles of the result
  const int total_units = K >> 5;
  const int u_begin = blockIdx.y * chunks_per_split * kDtUnits;
  int u_end = u_begin + chunks_per_split * kDtUnits;
  if (u_end > total_units) u_end = total_units;
  const int nchunks = (u_end - u_begin + kDtUnits - 1) / kDtUnits;

  // the n-tile of W staged in slot s = 4 wn + j of the workgroup tile, -1 past N.  ACT 2: wave wn holds output
  // n-tiles 4 nb + 2 wn + (j & 1), their gate rows in j = 0, 1 and their up rows (N/32 tiles on) in j = 2, 3
  auto tile_of = [&](const int s) __attribute__((always_inline)) {
    if (ACT == 2) {
      const int o = nb * 4 + (s >> 2) * 2 + (s & 1);
      return o < half ? o + ((s >> 1) & 1) * half : -1;
    }
    const int t = nb * kDtNTiles + s;
    return t < ntiles ? t : -1;
  };

  // descriptors sized to the operands exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (int)((int64_t)N * K * 2), 0x00020000);
  __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (int)(((int64_t)(M - 1) * ldx + K) * 2), 0x00020000);

  dt_i32x4_t wreg[WL], xreg[XL];
  // chunk ci -> registers.  W load i covers (slot, unit) = (v / units, v % units), v = i * 4 + wave, one KiB, lane *
  // 16 within it; X pass i covers rows RPP i .. RPP i + RPP - 1, lane position p holds piece p ^ (r & 7)
  auto load_chunk = [&](const int ci) __attribute__((always_inline)) {
    const int unit0 = u_begin + ci * kDtUnits;
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int v = i * 4 + wave;
      const int t = tile_of(v / kDtUnits), u = unit0 + v % kDtUnits;
      const unsigned off = (t >= 0 && u < u_end)
                               ? ((unsigned)t * (unsigned)total_units + (unsigned)u) * 1024u + (unsigned)lane * 16u
                               : kDtOutOfRange;
      wreg[i] = __builtin_bit_cast(dt_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int r = i * RPP + tid / kDtPieces, q = (tid % kDtPieces) ^ (r & (kDtPieces - 1));
      const int m = m0 + r, u = unit0 + (q >> 2);
      const unsigned off = (m < M && u < u_end) ? (unsigned)(((int64_t)m * ldx + (int64_t)u * 32 + (q & 3) * 8) * 2)
                                                : kDtOutOfRange;
      xreg[i] = __builtin_bit_cast(dt_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
  };
  // registers -> stage ci & 1, both linear in the thread index
  auto store_chunk = [&](const int ci) __attribute__((always_inline)) {
    char* st = smem_raw + (ci & 1) * kDtStage;
#pragma unroll
    for (int i = 0; i < WL; ++i) *reinterpret_cast<dt_i32x4_t*>(st + (i * 4 + wave) * 1024 + lane * 16) = wreg[i];
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<dt_i32x4_t*>(st + kDtWBytes + i * 4096 + tid * 16) = xreg[i];
  };

  dt_f32x4_t acc[4][MT];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = dt_f32x4_t{0.f, 0.f, 0.f, 0.f};

  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int ci = 0; ci < nchunks; ++ci) {
    const bool more = ci + 1 < nchunks;  // uniform
    if (more) load_chunk(ci + 1);        // in flight under this chunk's MFMAs
    const char* st = smem_raw + (ci & 1) * kDtStage;
#pragma unroll
    for (int s = 0; s < kDtUnits; ++s) {
      dt_i32x4_t wf[4], xf[MT];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        wf[j] = *reinterpret_cast<const dt_i32x4_t*>(st + ((wn * 4 + j) * kDtUnits + s) * 1024 + lane * 16);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int r = wm * 16 * MT + 16 * mt + c;
        xf[mt] = *reinterpret_cast<const dt_i32x4_t*>(st + kDtWBytes + r * kDtRowBytes +
                                                      ((4 * s + g) ^ (r & (kDtPieces - 1))) * 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[j][mt] = dt_mfma<T>(wf[j], xf[mt], acc[j][mt]);
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
    if (ACT == 2) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int o = nb * 4 + wn * 2 + j;
        if (o >= half) continue;
        const int n0 = o * 16 + 4 * g;
        typename T::store_t gate[4], up[4];
        dt_round4<T>(gate, acc[j][mt], bias != nullptr ? bias + n0 : nullptr);
        dt_round4<T>(up, acc[j + 2][mt], bias != nullptr ? bias + (N >> 1) + n0 : nullptr);
#pragma unroll
        for (int r = 0; r < 4; ++r) gate[r] = silu_mul<T>(gate[r], up[r]);
        *reinterpret_cast<uint2*>(y + (int64_t)m * ldy + n0) = dt_pack4(gate);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n0 = (nb * kDtNTiles + wn * 4 + j) * 16 + 4 * g;
        if (n0 >= N) continue;
        if (partial != nullptr)
          *reinterpret_cast<dt_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = acc[j][mt];
        else
          *reinterpret_cast<uint2*>(y + (int64_t)m * ldy + n0) =
              dt_epilogue<T, ACT>(acc[j][mt], bias != nullptr ? bias + n0 : nullptr);
      }
    }
  }
}

// y[m, n] = epilogue(partial[0, m, n] + partial[1, m, n] + ...): the fp32 sum in the order of the splits
template <typename T, int ACT>
__global__ void dt_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                 const typename T::store_t* __restrict__ bias, const int64_t MN, const int N,
                                 const int64_t ldy, const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  dt_f32x4_t sum = *reinterpret_cast<const dt_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const dt_f32x4_t*>(partial + (int64_t)s * MN + i);
  const int64_t m = i / N;
  const int n = (int)(i - m * N);
  *reinterpret_cast<uint2*>(y + m * ldy + n) = dt_epilogue<T, ACT>(sum, bias != nullptr ? bias + n : nullptr);
}

struct DtPlan {
  int mtiles, nblocks;  // workgroup tiles along m and n
  int ksplit, chunks_per_split;
};

// the rule of f8t_plan (fp8_tiled_gemm.hip) in chunks of this kernel; the SwiGLU epilogue needs gate and up of a
// whole K in one workgroup and takes the tiles it has
inline DtPlan dt_plan(int M, int N, int K, int act) {
  DtPlan p;
  const int cus = tuning().gemm_workgroups;
  p.mtiles = (M + kDtRows - 1) / kDtRows;
  p.nblocks = act == 2 ? (N / 32 + kDtNTiles / 2 - 1) / (kDtNTiles / 2) : (N / 16 + kDtNTiles - 1) / kDtNTiles;
  const int64_t tiles = (int64_t)p.mtiles * p.nblocks;
  const int nchunks = (K / 32 + kDtUnits - 1) / kDtUnits;
  int ks = 1;
  const int64_t slots = (int64_t)kDtPerCU * cus;  // fewer tiles than the CUs hold workgroups leave slots empty
  if (tiles < slots && act != 2) {
    ks = (int)(slots / tiles);
    if (ks > nchunks / kDtMinSplitChunks) ks = nchunks / kDtMinSplitChunks;
    if (ks > kDtMaxSplit) ks = kDtMaxSplit;
    if (ks < 1) ks = 1;
  }
  p.chunks_per_split = (nchunks + ks - 1) / ks;
  p.ksplit = (nchunks + p.chunks_per_split - 1) / p.chunks_per_split;  // no empty split; the last may be short
  return p;
}

inline bool dt_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && (K % 32) == 0 && (N % 16) == 0 && (int64_t)N * K * 2 < ((int64_t)1 << 32) - 16;
}

template <typename T, int ACT>
int launch_dt(void* y, float* partial, const void* x, const void* w, const void* bias, int M, int N, int K, int64_t ldx,
              int64_t ldy, const DtPlan& p, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr size_t smem = (size_t)2 * kDtStage;
  static_assert(smem <= 64 * 1024, "beyond 64 KiB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL((dense_tiled_gemm_kernel<T, ACT>), dim3((unsigned)(p.mtiles * p.nblocks), p.ksplit),
                     dim3(kDtThreads), smem, stream, (S*)y, partial, (const uint16_t*)x, (const uint16_t*)w,
                     (const S*)bias, M, N, K, ldx, ldy, p.mtiles, p.chunks_per_split);
  LV_LAUNCH_CHECK();
  if constexpr (ACT != 2) {
    if (p.ksplit <= 1) return 0;
    const int64_t MN = (int64_t)M * N;
    hipLaunchKernelGGL((dt_reduce_kernel<T, ACT>), dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, (S*)y,
                       partial, (const S*)bias, MN, N, ldy, p.ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}

template <typename T>
int launch_dt_act(int act, void* y, float* partial, const void* x, const void* w, const void* bias, int M, int N, int K,
                  int64_t ldx, int64_t ldy, const DtPlan& p, hipStream_t stream) {
  if (act == 0) return launch_dt<T, 0>(y, partial, x, w, bias, M, N, K, ldx, ldy, p, stream);
  if (act == 1) return launch_dt<T, 1>(y, partial, x, w, bias, M, N, K, ldx, ldy, p, stream);
  return launch_dt<T, 2>(y, nullptr, x, w, bias, M, N, K, ldx, ldy, p, stream);
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_tiled_gemm_workspace_bytes(int M, int N, int K) {
  if (!dt_shape_ok(M, N, K)) return 0;
  const DtPlan p = dt_plan(M, N, K, 0);
  return p.ksplit > 1 ? (int64_t)p.ksplit * M * N * 4 : 0;
}

#define LV_ENVELOPE(cond, msg)                                    \
  do {                                                            \
    if (!(cond)) {                                                \
      set_error(std::string("lvllm_tiled_gemm: ") + msg);         \
      return 3;                                                   \
    }                                                             \
  } while (0)

extern "C" int lvllm_tiled_gemm(void* y, const void* x, const void* w_packed, const void* bias, int M, int N, int K,
                                int64_t ldx, int64_t ldy, int dtype, int act, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_ENVELOPE(dtype == LVLLM_BF16 || dtype == LVLLM_F16, "dtype must be bf16 or f16");
  LV_ENVELOPE(act >= 0 && act <= 2, "act must be 0 (bias), 1 (GELU) or 2 (SwiGLU)");
  LV_ENVELOPE(K > 0 && (K % 32) == 0, "K must be a positive multiple of 32");
  LV_ENVELOPE((N % 16) == 0, "N must be a multiple of 16");
  LV_ENVELOPE(act != 2 || (N % 32) == 0, "N must be a multiple of 32 for act = 2");
  LV_ENVELOPE((int64_t)N * K * 2 < ((int64_t)1 << 32) - 16, "N * K: the packed weight must stay below 4 GiB");
  LV_ENVELOPE(ldx >= K && (ldx % 8) == 0, "ldx must be at least K and a multiple of 8");
  const int width = act == 2 ? N / 2 : N;
  LV_ENVELOPE(ldy >= width && (ldy % 4) == 0, "ldy must be at least the output width and a multiple of 4");
  LV_ENVELOPE(((int64_t)(M - 1) * ldx + K) * 2 < ((int64_t)1 << 31), "M, ldx: x must span less than 2 GiB");
  LV_ENVELOPE(((((uintptr_t)x | (uintptr_t)w_packed) & 15) == 0) && ((((uintptr_t)y) & 7) == 0) &&
                  ((((uintptr_t)bias) & 1) == 0),
              "x and w_packed must be 16-byte aligned, y 8-byte aligned");
  LV_CHECK(y != nullptr && x != nullptr && w_packed != nullptr, "y, x and w_packed are device pointers");
  const DtPlan p = dt_plan(M, N, K, act);
  float* partial = nullptr;
  if (p.ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)p.ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_tiled_gemm_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LVLLM_BF16) return launch_dt_act<BF16>(act, y, partial, x, w_packed, bias, M, N, K, ldx, ldy, p, s);
  return launch_dt_act<F16>(act, y, partial, x, w_packed, bias, M, N, K, ldx, ldy, p, s);
}
#undef LV_ENVELOPE
