// MXFP4 prefill GEMM on the block-scaled MFMA (W4A8), included by gemm_w4.hip
// (which states the weight's fragment order):
//
//   C[M,N] = act(dq(A8)[M,K] . dq(W)[N,K]^T + bias[n]) (+ R[M,N]),   M >= 1
//
// A8: MX e4m3 activations (quant_rows_mx / layernorm_q8_mx: rows of kpad bytes,
// one e8m0 scale per (row, 128 columns) in the mx_index layout, columns past K
// zero).  W: the Mxfp4Weight codes and scale bytes as stored.  One
// v_mfma_scale_f32_16x16x128_f8f6f4 multiplies 16 weight rows by 16 activation
// rows over 128 k: source A = the lane's 16 bytes of codes (cbsz 4: e2m1, the
// low 4 dwords of the operand) with the lane's own e8m0 block scale, source B =
// 32 e4m3 bytes with the row's e8m0 scale.  Nothing is expanded or converted,
// and the MFMAs issue at the fp8 rate.  Weights in source A: transposed
// accumulators, the shared epilogues of gemm_epilogue.h.
//
// Work split: 8 waves, an output tile of 128 MQ rows x 256 columns, one K-tile
// = 128 k.  Wave (wr = wave >> 2, wc = wave & 3) owns the four 16-row fragments
// 64 wr + 16 i of each 128-row half and the four column tiles 4 wc + j of the
// tile's 16: 16 MQ accumulators.
//   * Weights never enter LDS.  Lane l of the wave loads its 16 bytes of (tile,
//     chunk) straight from global memory: the stored order is the operand, so a
//     wave reads one contiguous 1 KiB per column tile and K-tile, plus 64 scale
//     bytes.  Two register sets: the loads of K-tile t + 2 are issued right
//     behind the MFMAs of K-tile t into the set they have just left, so they
//     are between one and two K-tiles ahead of their use.  The four scale bytes
//     of a wave's column tiles are packed into one dword per lane and selected
//     by op_sel (byte j = tile j); the activation scales are one dword per lane
//     and 64-row block, byte i = fragment i (mx_index), as bg_mfma_f8x reads them.
//   * A goes through LDS by LDS-DMA (stage_half, the staging of the bf16 / fp8
//     tile kernels: 128-byte rows, 16 KiB per 128 rows and K-tile).  Against the
//     fp8 kernel the B half of the LDS footprint, traffic and DMA is gone.  The
//     room goes into DEPTH: a ring of 4 stages (128 KiB at MQ = 2), three
//     K-tiles of A in flight, ONE barrier per K-tile (the fp8 kernel: 8).  Two
//     workgroups per CU are not an option at MQ = 2: 128 accumulator registers
//     per wave leave no room for a second 8-wave workgroup on the SIMDs.  At
//     MQ = 1 (64 accumulators, 64 KiB of LDS) a second workgroup would need the
//     wave under 128 registers; it takes about 170 (accumulators, two weight
//     sets, two fragments, addresses), so it keeps one workgroup per CU and the
//     same ring rather than spill for occupancy (not measured).
//     Iteration t: wait for the wave's own DMAs of tile t, barrier (every part
//     of tile t landed; every wave is past its reads of tile t - 1), start the
//     DMAs of tile t + 3 into the stage tile t - 1 has left, read and multiply
//     tile t, request the weights of tile t + 2.  A wave issues P = 3 MQ + 8
//     memory operations per iteration in a fixed order, so the wait is the
//     counted vmcnt(2 P): everything older than the last two iterations has
//     landed, tile t's DMAs (three iterations old) among them.  Loads past the
//     last K-tile are clamped to it (refills of dead stages and registers), so
//     the count is uniform.  Known gap: with register loads and LDS-DMAs both
//     pending the compiler's own wait at the first use of a weight register set
//     is a full vmcnt(0) (seen in the assembly of every other K-tile), which
//     also retires the newest DMAs, so the ring's depth is only half used.
//     Registers (-Rpass-analysis=kernel-resource-usage): MQ = 1 about 170
//     VGPRs, no scratch; MQ = 2 sits at the 256-register limit and spills 1-7
//     registers (SILU_MUL: about 16) of epilogue-only values around the loop.
//     Where the compiler places a reload inside the loop it is one more memory
//     operation than P in that iteration: the counted wait then retires more
//     than it must (stricter, never looser), and SwiGLU pays that traffic.
//   * Fragment reads.  The two operand formats order K differently (found on
//     the device with one-hot activation columns, not in the ISA text): the
//     4-register e2m1 operand of lane group g holds k 32 g .. 32 g + 31, the
//     stored weight order, while the 8-register e4m3 operand holds k 16 g ..
//     16 g + 15 in registers 0-3 and k 64 + 16 g .. 64 + 16 g + 15 in
//     registers 4-7.  So the lane reads the 16-byte chunks g and 4 + g of its
//     row, as bg_read does; chunks 2 g and 2 g + 1 (bytes 32 g .. 32 g + 31)
//     pair activation chunk c with the weight's chunk (c >> 1) + 4 (c & 1) and
//     fail the exact test.  Both chunks lie in the row's one 128-column scale
//     block, so the per-lane activation scale is the row's either way.
//     Swizzle: chunk c of row r is stored at chunk position c ^ ((r >> 1) & 7)
//     (swz_chunk, applied to the DMA's source address).  A ds_read_b128 is
//     served 16 lanes at a time, 16 x 16 B = the 64 banks once; the 16 lanes of
//     a lane group read ONE chunk c (g, then 4 + g) of rows r0 .. r0 + 15,
//     r0 a multiple of 16.  The bank of a 16-byte slot is fixed by (r & 1, the
//     chunk position): rows of equal parity are 256 B = 64 banks apart.  Among
//     the 8 rows of one parity (r >> 1) & 7 takes every value once, so
//     c ^ ((r >> 1) & 7) takes 8 distinct positions, for any c: 16 distinct
//     slots, every bank once, no conflict, for both reads.
//   * MQ = 1 (128-row tiles): M <= 128, where a 256-row tile would be half or
//     three quarters empty, and wherever 256-row tiles would leave half the CUs
//     without a workgroup (reasoned from the CU count, not measured).
//   * Summation order: one workgroup per output tile over the whole of K in
//     ascending k inside the MFMA accumulators; no K split, no atomics: the
//     same bits on every launch.
// Edges: rows >= M read row M - 1 (stage_half) and the last 64-row scale block,
// column tiles past N re-read the last real tile; neither is stored.  K % 128
// != 0: the weight's pad blocks are zero codes with scale 127 and the
// activation pad bytes are zero, so the last K-tile needs no special case.
#pragma once
#include <type_traits>
#include <utility>

#include "gemm_epilogue.h"
#include "gemm_tile.h"

namespace dnn {

typedef int w48_i32x8 __attribute__((ext_vector_type(8)));

constexpr int W48_STAGES = 4;
constexpr int W48_HALF = 128 * 128;  // 16 KiB: 128 rows of one K-tile
constexpr int W48_N = 256;

// accumulator (I, J) of a 128-row half: column tile J (op_sel byte J of ws) x row fragment I (byte I of as)
// (op_sel is an immediate, hence the templates.)  a[] holds the fragments I0, I0 + 1.
template <int I0, int IJ>
__device__ __forceinline__ void w48_mfma1(f32x4 (&acc)[4][4], const i32x4 (&w)[4], const w48_i32x8 (&a)[2],
                                          uint32_t ws, uint32_t as) {
  constexpr int I = I0 + IJ / 4, J = IJ % 4;
  const w48_i32x8 w8 = __builtin_shufflevector(w[J], w[J], 0, 1, 2, 3, -1, -1, -1, -1);  // cbsz 4 reads 4 dwords
  acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, a[IJ / 4], acc[I][J], 4, 0, J, ws, I, as);
}
template <int I0, int... IJ>
__device__ __forceinline__ void w48_mfma8(f32x4 (&acc)[4][4], const i32x4 (&w)[4], const w48_i32x8 (&a)[2],
                                          uint32_t ws, uint32_t as, std::integer_sequence<int, IJ...>) {
  (w48_mfma1<I0, IJ>(acc, w, a, ws, as), ...);
}

template <int ACT, int MQ>
__global__ __launch_bounds__(512, 1) void gemm_w4a8_kernel(const uint8_t* __restrict__ A8, int lda_b,
                                                           const uint32_t* __restrict__ sx,
                                                           const uint8_t* __restrict__ Wq,
                                                           const uint8_t* __restrict__ Ws, bf16_t* __restrict__ C,
                                                           int ldc, const float* __restrict__ bias,
                                                           const bf16_t* __restrict__ R, int ldr, int M, int N, int K) {
  static_assert(MQ == 1 || MQ == 2, "128- or 256-row tiles");
  constexpr int TM = 128 * MQ, STAGE = MQ * W48_HALF;
  constexpr int P = 3 * MQ + 8;  // memory operations per wave and iteration: 2 MQ DMAs, 4 + 4 weight loads, MQ scales
  __shared__ __attribute__((aligned(1024))) char smem[W48_STAGES * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = (N + W48_N - 1) / W48_N, ntm = (M + TM - 1) / TM;
  int tm, tn;
  tile_coords(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, tm, tn);
  const int m0 = tm * TM, n0 = tn * W48_N;
  const int wr = wave >> 2, wc = wave & 3;
  const int g = lane >> 4, r = lane & 15;
  const int nk = (K + 127) >> 7;
  const int ntile = (N + 15) >> 4, nb64 = mx_mpad(M) >> 6;

  // this wave's column tiles (a tile past N repeats the last real one and stores nothing) and scale blocks
  // wave-uniform element offsets (scalar registers); the lane's part is a 32-bit offset
  size_t woff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) woff[j] = (size_t)min((n0 >> 4) + wc * 4 + j, ntile - 1) * nk;  // + K-tile: 1 KiB / 64 B blocks
  size_t soff[MQ];
#pragma unroll
  for (int q = 0; q < MQ; ++q) soff[q] = (size_t)min((m0 >> 6) + 2 * q + wr, nb64 - 1);  // + K-tile * nb64: 16-dword blocks
  const uint32_t lane16 = lane * 16u, lane4 = lane & 60u, r4 = r * 4u;
  // v_perm selectors: byte lane & 3 of each of two dwords into the low / the high half, the other half zero
  const uint32_t bsel = lane & 3u, sel_lo = 0x0c0c0000u | ((4u + bsel) << 8) | bsel, sel_hi = sel_lo << 16 | 0x0c0cu;

  f32x4 acc[MQ][4][4];
#pragma unroll
  for (int q = 0; q < MQ; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[q][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // e4m3 rows staged as bf16 rows of half the length (byte-identical)
  const bf16_t* A = reinterpret_cast<const bf16_t*>(A8);
  auto stA = [&](int t) {  // K-tile t (clamped) into stage t & 3
    char* dst = smem + (t & (W48_STAGES - 1)) * STAGE;
    const int tc = t < nk ? t : nk - 1;
#pragma unroll
    for (int q = 0; q < MQ; ++q) stage_half(A, lda_b >> 1, m0 + q * 128, M, tc * 64, dst + q * W48_HALF, wave, lane);
  };
  i32x4 wv[2][4];
  uint32_t wsb[2][4], sxd[2][MQ];
  auto ldW = [&](int t, auto scst) {  // codes and scales of K-tile t (clamped) into register set s
    constexpr int s = decltype(scst)::value;
    const size_t tc = t < nk ? t : nk - 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[s][j] = *reinterpret_cast<const i32x4*>(Wq + (woff[j] + tc) * 1024 + lane16);
#pragma unroll
    for (int j = 0; j < 4; ++j)  // the aligned dword around the lane's scale byte (its byte lane & 3 is picked at the use)
      wsb[s][j] = *reinterpret_cast<const uint32_t*>(Ws + (woff[j] + tc) * 64 + lane4);
#pragma unroll
    for (int q = 0; q < MQ; ++q)
      sxd[s][q] = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(sx) + (tc * nb64 + soff[q]) * 64 + r4);
  };

  stA(0);
  ldW(0, std::integral_constant<int, 0>{});
  stA(1);
  ldW(1, std::integral_constant<int, 1>{});
  stA(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const int frow = wr * 64 + r;  // + 16 i: the lane's row of fragment i inside a half
  auto ktile = [&](const int t, auto scst) {
    constexpr int s = decltype(scst)::value;
    // nothing is scheduled up to the counted wait: a use of the newest loads there would force a full wait
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * P) : "memory");
    bg_barrier();
    stA(t + 3);
    __builtin_amdgcn_sched_barrier(0);
    // byte j = the scale of column tile j (v_perm: selector 0..3 = bytes of the second operand, 4..7 of the first)
    const uint32_t ws = __builtin_amdgcn_perm(wsb[s][1], wsb[s][0], sel_lo) |
                        __builtin_amdgcn_perm(wsb[s][3], wsb[s][2], sel_hi);
    const char* st = smem + (t & (W48_STAGES - 1)) * STAGE;
#pragma unroll
    for (int q = 0; q < MQ; ++q) {
      // two fragments (16 registers) at a time: all four would not fit beside 128 accumulators and two weight sets
      auto pairI = [&](auto i0cst) {
        constexpr int i0 = decltype(i0cst)::value;
        w48_i32x8 af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = frow + (i0 + i) * 16;
          const char* rp = st + q * W48_HALF + row * 128;
          const i32x4 lo = *reinterpret_cast<const i32x4*>(rp + ((g ^ swz_chunk(row)) << 4));
          const i32x4 hi = *reinterpret_cast<const i32x4*>(rp + (((4 + g) ^ swz_chunk(row)) << 4));
          af[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        __builtin_amdgcn_s_setprio(1);
        w48_mfma8<i0>(acc[q], wv[s], af, ws, sxd[s][q], std::make_integer_sequence<int, 8>{});
        __builtin_amdgcn_s_setprio(0);
      };
      pairI(std::integral_constant<int, 0>{});
      pairI(std::integral_constant<int, 2>{});
    }
    __builtin_amdgcn_sched_barrier(0);
    ldW(t + 2, scst);
  };
  int t = 0;
  for (; t + 1 < nk; t += 2) {
    ktile(t, std::integral_constant<int, 0>{});
    ktile(t + 1, std::integral_constant<int, 1>{});
  }
  if (t < nk) ktile(t, std::integral_constant<int, 0>{});
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA outlives the workgroup's LDS

  const bool vec = epi_vec_ok(C, ldc, bias, R, ldr);
  const bool pair = vec && epi_pair_ok(C, ldc, bias, R, ldr);
#pragma unroll
  for (int q = 0; q < MQ; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + q * 128 + frow + i * 16;
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const int nb = n0 + (wc * 4 + j) * 16;  // the pair of column tiles j, j + 1 (wave-uniform)
        if (nb >= N) continue;
        if constexpr (ACT == ACT_SILU_MUL) {
          epi_silu_pair<false>(acc[q][i][j], acc[q][i][j + 1], m, nb / 2, M, N / 2, C, ldc, vec, lane);
        } else if (pair && nb + 31 < N) {
          epi_pair_bf16<ACT>(acc[q][i][j], acc[q][i][j + 1], m, nb, M, C, ldc, bias, R, ldr, lane);
        } else {
          epi_t4<ACT, false>(acc[q][i][j], m, nb + g * 4, M, N, C, ldc, bias, R, ldr, vec);
          epi_t4<ACT, false>(acc[q][i][j + 1], m, nb + 16 + g * 4, M, N, C, ldc, bias, R, ldr, vec);
        }
      }
    }
}

}  // namespace dnn

template <int ACT>
static int launch_w4a8(const void* A8, const void* sx, const void* Wq, const void* Ws, void* C, int ldc,
                       const float* bias, const void* R, int ldr, int M, int N, int K, hipStream_t st) {
  using namespace dnn;
  const int kpad = (K + 127) / 128 * 128;
  const long long ntn = (N + W48_N - 1) / W48_N, t256 = (long long)((M + 255) / 256) * ntn;
  const bool narrow = M <= 128 || t256 <= 128;  // 256 CUs: 256-row tiles would leave half of them idle
  const long long tiles = narrow ? (long long)((M + 127) / 128) * ntn : t256;
  if (tiles > 0x7fffffffll) return -3;
#define W48_LAUNCH(MQ)                                                                                             \
  hipLaunchKernelGGL((gemm_w4a8_kernel<ACT, MQ>), dim3((unsigned)tiles), dim3(512), 0, st, (const uint8_t*)A8, kpad, \
                     (const uint32_t*)sx, (const uint8_t*)Wq, (const uint8_t*)Ws, (bf16_t*)C, ldc, bias,           \
                     (const bf16_t*)R, ldr, M, N, K)
  if (narrow) W48_LAUNCH(1);
  else W48_LAUNCH(2);
#undef W48_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int dnn_gemm_w4a8(const void* A8, const void* sx, const void* Wq, const void* Ws, void* C, int ldc,
                             const float* bias, const void* R, int ldr, int M, int N, int K, int act,
                             hipStream_t st) {
  if (A8 == nullptr || sx == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (M < 1) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || act < dnn::ACT_NONE || act > dnn::ACT_SILU_MUL ||
      (act == dnn::ACT_SILU_MUL && N % 16 != 0))
    return -3;
  const int NO = act == dnn::ACT_SILU_MUL ? N / 2 : N;
  if (ldc < NO || (R != nullptr && ldr < NO)) return -4;
  if ((((uintptr_t)A8 | (uintptr_t)Wq) & 15) != 0 || (((uintptr_t)sx | (uintptr_t)Ws) & 3) != 0) return -5;
  switch (act) {
    case dnn::ACT_NONE: return launch_w4a8<dnn::ACT_NONE>(A8, sx, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, st);
    case dnn::ACT_RELU: return launch_w4a8<dnn::ACT_RELU>(A8, sx, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, st);
    case dnn::ACT_GELU: return launch_w4a8<dnn::ACT_GELU>(A8, sx, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, st);
    default: return launch_w4a8<dnn::ACT_SILU_MUL>(A8, sx, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, st);
  }
}
