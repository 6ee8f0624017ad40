// W4A8 MXFP4 GEMM for prefill batches on gfx950: the LDS-tiled sibling of mxfp4_gemm.hip, as fp8_tiled_gemm.hip is
// that of the fp8 decode kernel.
//   Y[M,N] = T( sx[m] * sum_k Xq[m,k] * W4[n,k] * 2^(E[n,k/32] - 127) + bias[n] ),
// any M >= 1 (meant for M > 64).  Xq is fp8 e4m3fn, quantised by the caller with one fp32 scale per row; the weight is
// the packed pair of lvllm_mxfp4_pack, read as it is: codes [N/16][K/128][lane 64][16 bytes], scales
// [N/16][ceil(K/512)][lane 64][4 bytes] (mxfp4_gemm.hip's header has the lane maps).
//
// Matrix instruction: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4 (A = fp4, 4 registers) and B = fp8, W the A
// operand and X the B operand: lane (g, c) ends with four consecutive n of row m = c, one 8-byte store.  The B
// fragment is the fp8 tiled kernel's, X[c][128 j + 16 g .. + 15] followed by X[c][128 j + 64 + 16 g .. + 15]; the A
// scale is the lane's own E8M0 byte of its scale word, picked by op_sel; the B scale is the constant 0x7f.  No VALU
// instruction touches a weight.
//
// Work split: a workgroup of 4 waves (2 along m x 2 along n) owns 128 rows x 128 columns and walks K in chunks of one
// k-step (128 k).  A wave owns 64 x 64: 4 n-tiles x 4 m-tiles, 64 accumulator registers, 4 fragments of 4 registers
// and 4 of 8 per k-step.
//
// Data path: codes and activations go HBM -> registers -> LDS -> fragments.  Per chunk the workgroup stages
//   W  8 n-tiles x 1 KiB, already in fragment order: copied linearly, read back with one ds_read_b128 per lane and
//      tile at lane * 16 (conflict-free), by the two waves that share the n-range;
//   X  128 rows x 128 bytes: eight lanes load one row segment, 16-byte piece q of row r sits at position q ^ (r & 7).
// One stage is 8 + 16 = 24 KiB, two stages 48 KiB.  The global loads of chunk i + 1 are issued before the MFMAs of
// chunk i, written to the other stage after them, one barrier per chunk.
//
// Scales do not pass through LDS: a wave loads, for each of its 4 n-tiles, the lane's dword of the current scale word
// (4 k-steps; 256 contiguous bytes per tile) straight into registers, one word ahead.  op_sel is an immediate, so the
// chunk loop is unrolled by four, one scale word per trip.  Steps past K inside the last word load zero codes and
// zero activations from an out-of-range offset; the pack wrote scale 127 there; they add +0.
//
// Few tiles: when the output has fewer tiles than the device holds workgroups, K is split over blockIdx.y in whole
// scale words (multiples of 512 k: a split never starts inside a word), at least 1024 k per split, at most 16
// splits; partials travel as fp32 in the caller's workspace and a second kernel sums them in the order of the splits
// before the epilogue: a result depends on the shape and the tuning, never on timing.
//
// Bounds: buffer descriptors sized exactly to X ((M - 1) ldx + K bytes), to the codes and to the scales; rows past M,
// n-tiles past N and steps past K are loaded from an out-of-range offset and read zeros.  Stores are guarded.
//
// Register and LDS budget (the compiler's report, profiles/mxfp4_tiled_gemm.md): 150 VGPRs, no AGPRs, no scratch, no
// static LDS, 48 KiB dynamic: three workgroups per CU (3 waves per SIMD, 170 registers each; 144 of 160 KiB of LDS),
// which __launch_bounds__ asks for.  Of the 150: accumulators 64, X fragments 32, W fragments 16, the next chunk in
// flight 24, two scale words 8.
//
// Measured and dropped (same file): a 128 x 256 workgroup tile (-DLVLLM_MX4T_NTW=8 rebuilds it: a wave owns 64 x 128,
// 128 accumulators, 237 VGPRs, 16 + 16 KiB per stage, two workgroups per CU).  The outcome is mixed, not a clear loss:
// per resident round it does twice the work in 1.2x the time (2.3 against 2.1 Pflop/s at 8192 rows) and wins where the
// 128-column grid needs more than one round of workgroups (by 8 - 10 % at 8192 rows on qkv, o and down, by 26 % on
// gate_up at 512), but it halves the number of tiles and loses where they no longer fill the device: by 13 - 18 % at
// 128 rows on three shapes, by 9 % on qkv and 25 % on o at 2048.  This tile is kept for the smaller worst case at the
// row counts the default route starts from; choosing between the two per launch has not been tried.  Against the
// 64-row chunks this kernel is faster beyond the spread on all four 8B projections from 256 rows on (1.3x - 1.5x
// there, 2.7x - 7.3x at 8192) and slower at 65 and 128 rows on qkv and o (0.76x - 0.83x) and on gate_up at 128
// (0.88x), hence mxfp4_tiled_min_rows = 256.  Whether LDS bandwidth or the matrix pipe bounds it has not been traced.
#include <type_traits>

#include "common.h"

namespace lvllm {
namespace {

typedef int mxt_i32x4_t __attribute__((ext_vector_type(4)));
typedef int mxt_i32x8_t __attribute__((ext_vector_type(8)));
typedef float mxt_f32x4_t __attribute__((ext_vector_type(4)));

#ifndef LVLLM_MX4T_NTW
#define LVLLM_MX4T_NTW 4  // n-tiles of 16 per wave: 4 (128-column workgroup tile) and 8 (256) measured
#endif
#ifndef LVLLM_MX4T_PER_CU
#define LVLLM_MX4T_PER_CU (LVLLM_MX4T_NTW == 4 ? 3 : 2)  // workgroups a CU holds, by LDS and by registers
#endif

constexpr int kMtThreads = 256;                 // 4 waves: wave = 2 wm + wn
constexpr int kMtMT = 4;                        // m-tiles of 16 per wave: the workgroup tile has 128 rows
constexpr int kMtNTW = LVLLM_MX4T_NTW;          // n-tiles of 16 per wave
constexpr int kMtNTiles = 2 * kMtNTW;           // n-tiles per workgroup tile
constexpr int kMtRows = 32 * kMtMT;             // rows of the workgroup tile
constexpr int kMtWBytes = kMtNTiles * 1024;     // W bytes of one stage
constexpr int kMtStage = kMtWBytes + kMtRows * 128;
constexpr int kMtPerCU = LVLLM_MX4T_PER_CU;
constexpr unsigned kMtOutOfRange = 0xfffffff0u;  // >= any descriptor size: the load returns 0
constexpr int kMtMinSplitWords = 2;              // a K split owns at least 1024 k
constexpr int kMtMaxSplit = 16;
constexpr int kMtMaxK = 131072;

// T( sx * acc[r] + bias[r] ) for four consecutive n of one row, packed for one 8-byte store (mxfp4_gemm.hip's order)
template <typename T>
__device__ __forceinline__ uint2 mxt_epilogue(const mxt_f32x4_t acc, const float sxm,
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

template <typename T>
__global__ __launch_bounds__(kMtThreads, kMtPerCU) void tiled_gemm_mxfp4_kernel(
    typename T::store_t* __restrict__ y,  // [M, N]          (ksplit == 1)
    float* __restrict__ partial,          // [ksplit, M, N]  (ksplit > 1)
    const uint8_t* __restrict__ xq, const uint8_t* __restrict__ wq, const uint8_t* __restrict__ eq,
    const float* __restrict__ sx, const typename T::store_t* __restrict__ bias, const int M, const int N, const int K,
    const int64_t ldx, const int mtiles, const int words_per_split) {
  constexpr int MT = kMtMT, NTW = kMtNTW;
  constexpr int XL = kMtRows * 128 / (kMtThreads * 16);  // 16-byte X loads per lane and chunk
  constexpr int WL = kMtWBytes / (kMtThreads * 16);      // 16-byte W loads per lane and chunk
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];  // [2][ W: [n-tiles][64 lanes][16] | X: [rows][128] ]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, c = lane & 15;
  const int m0 = (int)(blockIdx.x % mtiles) * kMtRows;     // m-tiles vary fastest: neighbours share the W columns
  const int t0 = (int)(blockIdx.x / mtiles) * kMtNTiles;  // first n-tile of 16
  const int ntiles = N >> 4;
  const int total_steps = K >> 7;
  const int total_words = (total_steps + 3) >> 2;
  const int w_begin = blockIdx.y * words_per_split;  // scale words [w_begin, w_end) are this split's
  int w_end = w_begin + words_per_split;
  if (w_end > total_words) w_end = total_words;
  const int nwords = w_end - w_begin;
  const int step0 = 4 * w_begin;

  // descriptors sized to the operands exactly: a wrong offset reads zeros, never memory outside
  __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)wq, 0, (int)((int64_t)N * K / 2), 0x00020000);
  __amdgpu_buffer_rsrc_t er =
      __builtin_amdgcn_make_buffer_rsrc((void*)eq, 0, (int)((int64_t)ntiles * total_words * 256), 0x00020000);
  __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)xq, 0, (int)((int64_t)(M - 1) * ldx + K), 0x00020000);

  mxt_i32x4_t wreg[WL], xreg[XL];
  // chunk ci -> registers.  W load i covers n-tile i * 4 + wave of the workgroup tile, one KiB, lane * 16 within it;
  // X pass i covers rows 32 i .. 32 i + 31, lane position p of a row holds piece p ^ (r & 7)
  auto load_chunk = [&](const int ci) __attribute__((always_inline)) {
    const int step = step0 + ci;
    const bool live = ci < 4 * nwords && step < total_steps;  // uniform
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int t = t0 + i * 4 + wave;
      const unsigned off = (t < ntiles && live)
                               ? ((unsigned)t * (unsigned)total_steps + (unsigned)step) * 1024u + (unsigned)lane * 16u
                               : kMtOutOfRange;
      wreg[i] = __builtin_bit_cast(mxt_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int r = i * 32 + (tid >> 3), q = (tid & 7) ^ (r & 7);
      const int m = m0 + r;
      const unsigned off =
          (m < M && live) ? (unsigned)((int64_t)m * ldx + (int64_t)step * 128 + q * 16) : kMtOutOfRange;
      xreg[i] = __builtin_bit_cast(mxt_i32x4_t, __builtin_amdgcn_raw_buffer_load_b128(xr, off, 0, 0));
    }
  };
  // registers -> stage `stage`, both linear in the thread index
  auto store_chunk = [&](const int stage) __attribute__((always_inline)) {
    char* st = smem_raw + stage * kMtStage;
#pragma unroll
    for (int i = 0; i < WL; ++i) *reinterpret_cast<mxt_i32x4_t*>(st + (i * 4 + wave) * 1024 + lane * 16) = wreg[i];
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<mxt_i32x4_t*>(st + kMtWBytes + i * 4096 + tid * 16) = xreg[i];
  };
  // the lane's scale dwords of scale word w_begin + wi for the wave's n-tiles: byte b is the scale of k-step 4 wi + b
  auto load_scales = [&](unsigned (&e)[NTW], const int wi) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int t = t0 + wn * NTW + j;
      const unsigned off = (t < ntiles && wi < nwords)
                               ? ((unsigned)t * (unsigned)total_words + (unsigned)(w_begin + wi)) * 256u + (unsigned)lane * 4u
                               : kMtOutOfRange;
      e[j] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(er, off, 0, 0);
    }
  };

  mxt_f32x4_t acc[NTW][MT];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[j][mt] = mxt_f32x4_t{0.f, 0.f, 0.f, 0.f};

  // one chunk: chunk ci = 4 wi + S sits in stage S & 1; op_sel = S reaches the builtin as a constant
  auto chunk = [&](auto S, const unsigned (&e)[NTW]) __attribute__((always_inline)) {
    constexpr int s = decltype(S)::value;
    const char* st = smem_raw + (s & 1) * kMtStage;
    mxt_i32x8_t wf[NTW], xf[MT];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const mxt_i32x4_t w = *reinterpret_cast<const mxt_i32x4_t*>(st + (wn * NTW + j) * 1024 + lane * 16);
      wf[j] = mxt_i32x8_t{w[0], w[1], w[2], w[3], 0, 0, 0, 0};
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int r = wm * 16 * MT + 16 * mt + c;
      const char* p = st + kMtWBytes + r * 128;
      const int sz = r & 7;
      xf[mt] = __builtin_shufflevector(*reinterpret_cast<const mxt_i32x4_t*>(p + (g ^ sz) * 16),
                                       *reinterpret_cast<const mxt_i32x4_t*>(p + ((4 + g) ^ sz) * 16), 0, 1, 2, 3, 4,
                                       5, 6, 7);
    }
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[j][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], xf[mt], acc[j][mt], 4 /* A = fp4 */,
                                                                      0 /* B = fp8 e4m3 */, s, (int)e[j], 0, 0x7f7f7f7f);
    // the fences keep a chunk's MFMAs in their chunk: carried past the barrier into the next chunk's, the fragments
    // of two chunks would be live at once
    __builtin_amdgcn_sched_barrier(0);
    // the other stage was last read in the previous chunk, which every wave left through the barrier below
    store_chunk((s + 1) & 1);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  };

  unsigned ecur[NTW], enext[NTW];
  load_scales(ecur, 0);
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  // A trip is branch-free on purpose: the chunk after the split's last one loads zeros from the out-of-range offset
  // and is staged but never read.  (With a branch around that load the compiler sinks every MFMA of the trip below
  // the branch, past three barriers, and the accumulators spill.)
  for (int wi = 0; wi < nwords; ++wi) {
    load_scales(enext, wi + 1);  // one word ahead; past the split: zeros, never used
    load_chunk(4 * wi + 1);      // in flight under this chunk's MFMAs
    chunk(std::integral_constant<int, 0>{}, ecur);
    load_chunk(4 * wi + 2);
    chunk(std::integral_constant<int, 1>{}, ecur);
    load_chunk(4 * wi + 3);
    chunk(std::integral_constant<int, 2>{}, ecur);
    load_chunk(4 * wi + 4);
    chunk(std::integral_constant<int, 3>{}, ecur);
#pragma unroll
    for (int j = 0; j < NTW; ++j) ecur[j] = enext[j];
  }

  // lane (g, c): columns n0 .. n0 + 3 of row m
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + wm * 16 * MT + 16 * mt + c;
    if (m >= M) continue;
    const float sxm = partial != nullptr ? 0.f : sx[m];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int n0 = (t0 + wn * NTW + j) * 16 + 4 * g;
      if (n0 >= N) continue;
      if (partial != nullptr)
        *reinterpret_cast<mxt_f32x4_t*>(partial + ((int64_t)blockIdx.y * M + m) * N + n0) = acc[j][mt];
      else
        *reinterpret_cast<uint2*>(y + (int64_t)m * N + n0) =
            mxt_epilogue<T>(acc[j][mt], sxm, bias != nullptr ? bias + n0 : nullptr);
    }
  }
}

// y[m, n] = epilogue(partial[0, m, n] + partial[1, m, n] + ...): the fp32 sum in the order of the splits
template <typename T>
__global__ void mxt_reduce_kernel(typename T::store_t* __restrict__ y, const float* __restrict__ partial,
                                  const float* __restrict__ sx, const typename T::store_t* __restrict__ bias,
                                  const int64_t MN, const int N, const int ksplit) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= MN) return;
  mxt_f32x4_t sum = *reinterpret_cast<const mxt_f32x4_t*>(partial + i);
  for (int s = 1; s < ksplit; ++s) sum += *reinterpret_cast<const mxt_f32x4_t*>(partial + (int64_t)s * MN + i);
  const int m = (int)(i / N), n = (int)(i - (int64_t)m * N);
  *reinterpret_cast<uint2*>(y + i) = mxt_epilogue<T>(sum, sx[m], bias != nullptr ? bias + n : nullptr);
}

struct MxtPlan {
  int mtiles, nblocks;  // workgroup tiles along m and n
  int ksplit, words_per_split;
};

// the rule of f8t_plan (fp8_tiled_gemm.hip) in scale words of 512 k
inline MxtPlan mxt_plan(int M, int N, int K) {
  MxtPlan p;
  const int cus = tuning().gemm_workgroups;
  p.mtiles = (M + kMtRows - 1) / kMtRows;
  p.nblocks = (N + 16 * kMtNTiles - 1) / (16 * kMtNTiles);
  const int64_t tiles = (int64_t)p.mtiles * p.nblocks;
  const int words = (K / 128 + 3) / 4;
  int ks = 1;
  const int64_t slots = (int64_t)kMtPerCU * cus;  // fewer tiles than the CUs hold workgroups leave slots empty
  if (tiles < slots) {
    ks = (int)(slots / tiles);
    if (ks > words / kMtMinSplitWords) ks = words / kMtMinSplitWords;
    if (ks > kMtMaxSplit) ks = kMtMaxSplit;
    if (ks < 1) ks = 1;
  }
  p.words_per_split = (words + ks - 1) / ks;
  p.ksplit = (words + p.words_per_split - 1) / p.words_per_split;  // no empty split; the last may be short
  return p;
}

// the envelope of lvllm_mxfp4_pack
inline bool mxt_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0 && K < kMtMaxK &&
         (int64_t)N * K / 2 < ((int64_t)1 << 32) - 16;
}

template <typename T>
int launch_mxt(void* y, float* partial, const void* xq, const void* wq, const void* eq, const float* sx,
               const void* bias, int M, int N, int K, int64_t ldx, const MxtPlan& p, hipStream_t stream) {
  using S = typename T::store_t;
  constexpr size_t smem = (size_t)2 * kMtStage;
  static_assert(smem <= 64 * 1024, "beyond 64 KiB a launch needs hipFuncAttributeMaxDynamicSharedMemorySize");
  hipLaunchKernelGGL(tiled_gemm_mxfp4_kernel<T>, dim3((unsigned)(p.mtiles * p.nblocks), p.ksplit), dim3(kMtThreads),
                     smem, stream, (S*)y, partial, (const uint8_t*)xq, (const uint8_t*)wq, (const uint8_t*)eq, sx,
                     (const S*)bias, M, N, K, ldx, p.mtiles, p.words_per_split);
  LV_LAUNCH_CHECK();
  if (p.ksplit > 1) {
    const int64_t MN = (int64_t)M * N;
    hipLaunchKernelGGL(mxt_reduce_kernel<T>, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, stream, (S*)y,
                       partial, sx, (const S*)bias, MN, N, p.ksplit);
    LV_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace lvllm

using namespace lvllm;

extern "C" int64_t lvllm_gemm_w4a8_mxfp4_workspace_bytes(int M, int N, int K) {
  if (!mxt_shape_ok(M, N, K)) return 0;
  const MxtPlan p = mxt_plan(M, N, K);
  return p.ksplit > 1 ? (int64_t)p.ksplit * M * N * 4 : 0;
}

extern "C" int lvllm_gemm_w4a8_mxfp4(void* y, const void* x_fp8, const void* w_packed, const void* e_packed,
                                     const float* x_scale, const void* bias, int M, int N, int K, int64_t ldx,
                                     int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M <= 0 || N <= 0) return 0;
  LV_CHECK(x_scale != nullptr, "x_scale [M] is a device pointer");
  if (!(dtype == LVLLM_BF16 || dtype == LVLLM_F16) || !mxt_shape_ok(M, N, K) || ldx < K || (ldx % 16) != 0 ||
      (int64_t)(M - 1) * ldx + K >= ((int64_t)1 << 31) || (int64_t)M * N >= ((int64_t)1 << 40) ||
      ((((uintptr_t)x_fp8 | (uintptr_t)w_packed) & 15) != 0) || (((uintptr_t)e_packed) & 3) != 0 ||
      (((uintptr_t)y) & 7) != 0 || (((uintptr_t)bias) & 1) != 0) {
    set_error("lvllm_gemm_w4a8_mxfp4: shape outside the kernel's envelope");
    return 3;
  }
  const MxtPlan p = mxt_plan(M, N, K);
  float* partial = nullptr;
  if (p.ksplit > 1) {
    LV_CHECK(workspace != nullptr && workspace_bytes >= (int64_t)p.ksplit * M * N * 4 && (((uintptr_t)workspace) & 15) == 0,
             "workspace too small or unaligned (see lvllm_gemm_w4a8_mxfp4_workspace_bytes)");
    partial = (float*)workspace;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LVLLM_BF16)
    return launch_mxt<BF16>(y, partial, x_fp8, w_packed, e_packed, x_scale, bias, M, N, K, ldx, p, s);
  return launch_mxt<F16>(y, partial, x_fp8, w_packed, e_packed, x_scale, bias, M, N, K, ldx, p, s);
}
