// MXFP4 weights (OCP e2m1 codes, one e8m0 scale per 32 k): the W4A16 decode GEMM
// and the expansion to row-major bf16 that feeds the prefill tile kernels.
//
//   C[M,N] = act(norm(A)[M,K] . dq(W)[N,K]^T + bias[n]) (+ R[M,N]),   1 <= M <= 64
//
// Every dequantised value (a 2-bit significand times a power of two) is a bf16
// value, so v_cvt_scalef32_pk_bf16_fp4 (one byte = two codes, times the block's
// fp32 scale, to a packed bf16 pair) loses nothing and the product runs on the
// bf16 MFMA against the unchanged bf16 activations.
//
// Weight layout (ops/w4.py pack_mxfp4; N padded to 16, K to 128, pads zero):
//   codes   [tile t = n / 16][chunk c = k / 128][lane l = 16 g + r][16 bytes]
//           lane l holds row 16 t + r, k = 128 c + 32 g .. + 31 (exactly one MX
//           block); byte b = codes of k + 2 b (low nibble) and k + 2 b + 1 (high);
//           the convert puts the low nibble in the low bf16 half (the lower k)
//   scales  [tile][chunk][lane]   one e8m0 byte (1..254; fp32 scale = e << 23)
// so a wave reads one contiguous 1 KiB of codes and 64 B of scales per chunk,
// and the chunks of a column tile are consecutive along K.
//
// dnn_gemm_w4.  A workgroup owns ONE column tile (16 output channels) and all M
// rows: KS = min(8, chunks) waves split K into contiguous slices (balanced to
// one chunk), so every weight byte is loaded exactly once for all <= 64 rows,
// by a non-temporal 16-byte load.  Per chunk a lane converts its 16 bytes with
// its one scale (16 converts -> four bf16x8) and issues four
// mfma_f32_16x16x32_bf16 per 16-row M tile: MFMA h pairs codes 8 h .. 8 h + 7
// with the activation piece h (16 B) of the same 32 k, so the lane reads 64
// contiguous activation bytes per chunk and M tile.  The KS partial sums and
// the shifted row statistics (folded RMS / LayerNorm, from the A fragments the
// wave streams anyway) meet in LDS; wave w finishes M tiles w, w + KS, ...
// with the shared transposed-accumulator epilogue (gemm_epilogue.h).
// Choices, and why (figures: bench/probes/w4_decode_ab.py, profiles/w4_decode_ab.jsonl):
//   * one column tile per workgroup: N / 16 workgroups of up to 8 waves keep the
//     most weight loads in flight, which is what batch 1 needs (Llama-3 8B
//     projections at M = 1: 0.86-0.90 x the W8A16 time), and SwiGLU needs one
//     tile only (pack_gate_up pairs gate and up inside 16 columns).  Its price:
//     every workgroup reads all M activation rows, so at M = 32..64 the kernel
//     is bound by activation traffic from L2 (gate|up at M = 64: 1792
//     workgroups x 512 KiB), not by weight bytes, and measures 1.3-4 x slower
//     than W8A16, whose stream and one-shot kernels share A through LDS.  More
//     column tiles per workgroup divide that traffic but leave the narrow
//     projections (1600 wide: 100 tiles) a handful of workgroups; sharing A
//     through LDS across waves that split N is the open lever.
//   * chunks in flight: U = 4 (M <= 32) or 2 (M > 32) per wave, all loads of a
//     batch issued before its first convert; with 4 M tiles a chunk's
//     activation fragments are 64 VGPRs, which bounds U (no spills: at most 214
//     VGPRs, under the 256 that 8 waves per workgroup leave a wave).
//   * no M split over workgroups: it would load every weight byte once per M
//     tile (from L2 at best), which the fixed design excludes; narrow N with
//     many rows stays at N / 16 workgroups.
//   * epilogue operands are not prefetched: their registers go to the chunks in
//     flight, and bias / colsum are 64 B per tile.
// K % 128 != 0: the last chunk's 32-k groups at or past K are not read (the
// address is clamped to the chunk's first group, the fragment zeroed and left
// out of the statistics).  A wave's short last batch clamps its surplus loads
// to its last chunk and skips their math.
//
// Further kernels on the same weight, included below: gemm_w4_mid.h (65..256 rows, A through LDS), gemm_w4_mn.h
// (65..256 rows on narrow projections), gemm_w4_tile.h (any number of rows, 128 x 128 blocks: the compute-bound
// form, mxfp4_prefill "w4a16"), gemm_w4a8.h (prefill on MX e4m3 activations), gemm_w4_head.h (the vocabulary head).
//
// dnn_w4_expand.  One wave per (tile, chunk) block: it reads the block as the
// GEMM does (1 KiB of codes, 64 scale bytes), converts its 32 codes to 64 B of
// bf16 and transposes through LDS (row pitch 272 B, so the 16 rows of a lane
// group fall in distinct banks): store j of 4 then covers rows 4 j .. 4 j + 3,
// 16 consecutive lanes writing the 256 contiguous bytes of one row's chunk.
#include <algorithm>
#include "gemm_epilogue.h"

namespace dnn {

enum W4Norm { W4_NORM_NONE = 0, W4_NORM_RMS = 1, W4_NORM_LN = 2 };

// 16 bytes = 32 e2m1 codes of one MX block -> four bf16x8 (dword h = codes 8 h .. 8 h + 7)
__device__ __forceinline__ void w4_to_bf16(const i32x4& w, float scale, bf16x8 (&o)[4]) {
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint32_t d = (uint32_t)w[h];
    bf16x2v p[4];
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
    __builtin_memcpy(&o[h], p, 16);
  }
}

// Shifted sum and sum of squares of the 8 bf16 of one A fragment (x - c, c = the
// row's first element: no cancellation when |mean| >> std); RMS: squares only.
template <int NORM>
__device__ __forceinline__ void w4_stats(const i32x4& a, float c, float& s1, float& s2) {
  if constexpr (NORM == W4_NORM_RMS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x2v v = __builtin_bit_cast(bf16x2v, (uint32_t)a[i]);
      s2 = __builtin_amdgcn_fdot2_f32_bf16(v, v, s2, false);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = __uint_as_float((uint32_t)a[i] << 16) - c;
    const float hi = __uint_as_float((uint32_t)a[i] & 0xffff0000u) - c;
    s1 += lo + hi;
    s2 = fmaf(lo, lo, fmaf(hi, hi, s2));
  }
}

template <int ACT, int NORM, int MT, int U>
__global__ __launch_bounds__(512) void gemm_w4_kernel(const uint8_t* __restrict__ A, int lda_b,
                                                       const uint8_t* __restrict__ Wq,
                                                       const uint8_t* __restrict__ Ws, bf16_t* __restrict__ C,
                                                       int ldc, const float* __restrict__ bias,
                                                       const bf16_t* __restrict__ R, int ldr, int M, int N, int K,
                                                       const float* __restrict__ colsum, float eps) {
  extern __shared__ __attribute__((aligned(16))) f32x4 w4_red[];  // [KS][MT][64], then [KS][MT][2][16] statistics
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), KS = blockDim.x >> 6;
  const int tile = blockIdx.x, n0 = tile * 16;
  const int g = lane >> 4;
  const int nch = (K + 127) >> 7;  // 128-k chunks (the last may be partial)
  const int kg = K >> 5;           // valid 32-k groups
  const uint8_t* wp = Wq + ((size_t)tile * nch * 64 + lane) * 16;  // + chunk * 1024
  const uint8_t* sp = Ws + (size_t)tile * nch * 64 + lane;         // + chunk * 64
  const uint8_t* ap[MT];
  float st1[MT], st2[MT], shift[MT];
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = min(t * 16 + (lane & 15), M - 1);
    ap[t] = A + (size_t)m * lda_b;  // + chunk * 256 + group * 64 + piece * 16
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    st1[t] = st2[t] = 0.f;
    shift[t] = 0.f;
    if constexpr (NORM == W4_NORM_LN)
      shift[t] = __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(ap[t])) << 16);
  }
  // balanced contiguous K slices: nch = q KS + r, the first r waves take q + 1 chunks
  const int q = nch / KS, r = nch - q * KS;
  const int c0 = wave * q + min(wave, r), c1 = c0 + q + (wave < r ? 1 : 0);
  const int nb = (c1 - c0 + U - 1) / U;
  int c = c0;
  for (int b = 0; b < nb; ++b, c += U) {
    i32x4 wv[U], av[MT][U][4];
    uint32_t sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ci = min(c + u, c1 - 1);
      wv[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (size_t)ci * 1024));
      sc[u] = sp[(size_t)ci * 64];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ci = min(c + u, c1 - 1);
      const int go = ci * 4 + g < kg ? g : 0;  // a group at or past K reads the chunk's first group instead
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int h = 0; h < 4; ++h)
          av[t][u][h] = *reinterpret_cast<const i32x4*>(ap[t] + (size_t)ci * 256 + go * 64 + h * 16);
    }
    // every load of the batch ahead of its math (one wait, not one per chunk)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ci = c + u;
      if (ci < c1) {  // wave-uniform
        bool ok = true;
        if (ci * 4 + 4 > kg) {  // wave-uniform: the partial last chunk
          ok = ci * 4 + g < kg;
          if (!ok) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
              for (int h = 0; h < 4; ++h) av[t][u][h] = i32x4{0, 0, 0, 0};
          }
        }
        if constexpr (NORM != W4_NORM_NONE) {
          if (ok) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
              for (int h = 0; h < 4; ++h) w4_stats<NORM>(av[t][u][h], shift[t], st1[t], st2[t]);
          }
        }
        bf16x8 wb[4];
        w4_to_bf16(wv[u], __uint_as_float(sc[u] << 23), wb);
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            bf16x8 ab;
            __builtin_memcpy(&ab, &av[t][u][h], 16);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[h], ab, acc[t], 0, 0, 0);
          }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) w4_red[(wave * MT + t) * 64 + lane] = acc[t];
  float* w4_st = reinterpret_cast<float*>(w4_red + KS * MT * 64);
  if constexpr (NORM != W4_NORM_NONE) {
    // the 4 lane groups hold disjoint k of the same 16 rows
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      float a = st1[t], s = st2[t];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (lane < 16) {
        w4_st[((wave * MT + t) * 2 + 0) * 16 + lane] = a;
        w4_st[((wave * MT + t) * 2 + 1) * 16 + lane] = s;
      }
    }
  }
  __syncthreads();

  // reduction over the KS waves + epilogue: wave w finishes M tiles w, w + KS, ...
  const int NO = ACT == ACT_SILU_MUL ? N / 2 : N;
  const bool vec = epi_vec_ok(C, ldc, bias, R, ldr);
  for (int t = wave; t < MT; t += KS) {
    f32x4 s = w4_red[t * 64 + lane];
    for (int w = 1; w < KS; ++w) s += w4_red[(w * MT + t) * 64 + lane];
    const int m = t * 16 + (lane & 15);
    const int n = n0 + g * 4;
    if constexpr (NORM != W4_NORM_NONE) {
      float a = 0.f, sq = 0.f;
      for (int w = 0; w < KS; ++w) {
        a += w4_st[((w * MT + t) * 2 + 0) * 16 + (lane & 15)];
        sq += w4_st[((w * MT + t) * 2 + 1) * 16 + (lane & 15)];
      }
      const float invk = 1.f / (float)K;
      const float d = a * invk;  // E[x - c]
      float mean = 0.f;
      if constexpr (NORM == W4_NORM_LN)  // the row's shift again (shift[] is indexed by the unrolled main loop only)
        mean = d + __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(m, M - 1) * lda_b))
                                   << 16);
      const float var = NORM == W4_NORM_LN ? fmaxf(sq * invk - d * d, 0.f) : sq * invk;
      const float rstd = rsqrtf(var + eps);
      if constexpr (NORM == W4_NORM_LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = rstd * (s[i] - mean * (n + i < N ? colsum[n + i] : 0.f));
      } else {
        s *= rstd;
      }
    }
    if constexpr (ACT == ACT_SILU_MUL) {
      epi_silu_t4<false>(s, m, n0 / 2, M, NO, C, ldc, vec, lane);
    } else {
      epi_t4<ACT, false>(s, m, n, M, N, C, ldc, bias, R, ldr, vec);
    }
  }
}

}  // namespace dnn

#include "gemm_w4_mid.h"  // dnn_gemm_w4_mid's kernel: up to 256 rows, A shared through LDS
#include "gemm_w4_mn.h"   // dnn_gemm_w4_mn's kernel: up to 256 rows on narrow projections, an M x N grid, waves split K
#include "gemm_w4_tile.h"  // dnn_gemm_w4_tile's kernel: any number of rows, 128 x 128 blocks over the whole of K, compute-bound
#include "gemm_w4a8.h"    // dnn_gemm_w4a8: prefill on MX e4m3 activations, the codes on the scaled MFMA
#include "gemm_w4_head.h"  // dnn_gemm_w4_head: the vocabulary head, persistent workgroups, argmax partials

namespace dnn {

constexpr int W4X_PITCH = 272;  // LDS bytes per row of a wave's 16 x 256 B block (+16: bank spread)

__global__ __launch_bounds__(256) void w4_expand_kernel(const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ Ws,
                                                         bf16_t* __restrict__ W, int ldw, int N, int K, int nch,
                                                         int nblk) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][16 * W4X_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blk = min((int)blockIdx.x * 4 + wave, nblk - 1);  // a surplus wave repeats the last block (same bytes)
  const int tile = blk / nch, ch = blk - tile * nch;
  const i32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(Wq + ((size_t)blk * 64 + lane) * 16));
  const uint32_t e = Ws[(size_t)blk * 64 + lane];
  bf16x8 wb[4];
  w4_to_bf16(wv, __uint_as_float(e << 23), wb);
  // lane 16 g + r: row r, bytes 64 g .. 64 g + 63 of the block's 256-byte rows
  uint8_t* mine = lds[wave] + (lane & 15) * W4X_PITCH + (lane >> 4) * 64;
#pragma unroll
  for (int h = 0; h < 4; ++h) *reinterpret_cast<bf16x8*>(mine + 16 * h) = wb[h];
  __syncthreads();
  // store j: row 4 j + (lane >> 4), 16 B piece lane & 15 -> 256 contiguous bytes per row
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int rr = 4 * j + (lane >> 4), p = lane & 15;
    const int n = tile * 16 + rr, k = ch * 128 + p * 8;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(lds[wave] + rr * W4X_PITCH + p * 16);
    if (n < N && k < K) *reinterpret_cast<bf16x8*>(W + (size_t)n * ldw + k) = v;  // K % 32 == 0: whole pieces
  }
}

}  // namespace dnn

using namespace dnn;

template <int ACT, int NORM, int MT>
static int launch_w4_mt(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc, const float* bias,
                        const void* R, int ldr, int M, int N, int K, const float* colsum, float eps, hipStream_t st) {
  constexpr int U = MT <= 2 ? 4 : 2;
  const int nch = (K + 127) / 128, KS = std::min(8, nch);
  const size_t smem = (size_t)KS * MT * (64 * 16 + 2 * 16 * 4);
  hipLaunchKernelGGL((gemm_w4_kernel<ACT, NORM, MT, U>), dim3((N + 15) / 16), dim3(64 * KS), smem, st,
                     (const uint8_t*)A, lda * 2, (const uint8_t*)Wq, (const uint8_t*)Ws, (bf16_t*)C, ldc, bias,
                     (const bf16_t*)R, ldr, M, N, K, colsum, eps);
  return (int)hipGetLastError();
}

template <int ACT, int NORM>
static int launch_w4(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc, const float* bias,
                     const void* R, int ldr, int M, int N, int K, const float* colsum, float eps, hipStream_t st) {
#define W4_ARGS A, lda, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, colsum, eps, st
  switch ((M + 15) / 16) {
    case 1: return launch_w4_mt<ACT, NORM, 1>(W4_ARGS);
    case 2: return launch_w4_mt<ACT, NORM, 2>(W4_ARGS);
    case 3: return launch_w4_mt<ACT, NORM, 3>(W4_ARGS);
    default: return launch_w4_mt<ACT, NORM, 4>(W4_ARGS);
  }
}

template <int ACT>
static int launch_w4_norm(int norm, const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                          const float* bias, const void* R, int ldr, int M, int N, int K, const float* colsum,
                          float eps, hipStream_t st) {
  switch (norm) {
    case W4_NORM_NONE: return launch_w4<ACT, W4_NORM_NONE>(W4_ARGS);
    case W4_NORM_RMS: return launch_w4<ACT, W4_NORM_RMS>(W4_ARGS);
    default: return launch_w4<ACT, W4_NORM_LN>(W4_ARGS);
  }
}

extern "C" int dnn_gemm_w4(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                           const float* bias, const void* R, int ldr, int M, int N, int K, int act, int norm,
                           const float* colsum, float eps, hipStream_t st) {
  if (A == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (norm == W4_NORM_LN && colsum == nullptr) return -1;
  if (M < 1 || M > 64) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || act < ACT_NONE || act > ACT_SILU_MUL || norm < 0 || norm > W4_NORM_LN ||
      (act == ACT_SILU_MUL && N % 16 != 0))
    return -3;
  const int NO = act == ACT_SILU_MUL ? N / 2 : N;
  if (ldc < NO || lda < K || (R != nullptr && ldr < NO)) return -4;
  if ((((uintptr_t)A | (uintptr_t)Wq) & 15) != 0 || (lda & 7) != 0) return -5;
  switch (act) {
    case ACT_NONE: return launch_w4_norm<ACT_NONE>(norm, W4_ARGS);
    case ACT_RELU: return launch_w4_norm<ACT_RELU>(norm, W4_ARGS);
    case ACT_GELU: return launch_w4_norm<ACT_GELU>(norm, W4_ARGS);
    default: return launch_w4_norm<ACT_SILU_MUL>(norm, W4_ARGS);
  }
#undef W4_ARGS
}

// dnn_gemm_w4_mid: MT = 8 (M <= 128) or 16 M tiles, NT = 2 column tiles per wave where N / 128 workgroups
// still cover half the CUs, else 1 (gemm_w4_mid.h, "Choices").
template <int ACT, int NORM>
static int launch_w4_mid(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc, const float* bias,
                         const void* R, int ldr, int M, int N, int K, const float* colsum, float eps, hipStream_t st) {
  const int mt = (M + 15) / 16, ntile = (N + 15) / 16;
  const size_t smem = (size_t)mt * (2 * 16 * W4M_ROW + 16 * sizeof(float2));
#define W4M_LAUNCH(MT, NT)                                                                                        \
  hipLaunchKernelGGL((gemm_w4_mid_kernel<ACT, NORM, MT, NT>), dim3((ntile + W4M_WAVES * NT - 1) / (W4M_WAVES * NT)), \
                     dim3(64 * W4M_WAVES), smem, st, (const uint8_t*)A, lda * 2, (const uint8_t*)Wq,              \
                     (const uint8_t*)Ws, (bf16_t*)C, ldc, bias, (const bf16_t*)R, ldr, M, N, K, colsum, eps)
  if (N >= 16384) {
    if (mt <= 8) W4M_LAUNCH(8, 2);
    else W4M_LAUNCH(16, 2);
  } else {
    W4M_LAUNCH(16, 1);
  }
#undef W4M_LAUNCH
  return (int)hipGetLastError();
}

template <int ACT>
static int launch_w4_mid_norm(int norm, const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                              const float* bias, const void* R, int ldr, int M, int N, int K, const float* colsum,
                              float eps, hipStream_t st) {
#define W4_ARGS A, lda, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, colsum, eps, st
  switch (norm) {
    case W4_NORM_NONE: return launch_w4_mid<ACT, W4_NORM_NONE>(W4_ARGS);
    case W4_NORM_RMS: return launch_w4_mid<ACT, W4_NORM_RMS>(W4_ARGS);
    default: return launch_w4_mid<ACT, W4_NORM_LN>(W4_ARGS);
  }
}

extern "C" int dnn_gemm_w4_mid(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                               const float* bias, const void* R, int ldr, int M, int N, int K, int act, int norm,
                               const float* colsum, float eps, hipStream_t st) {
  if (A == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (norm == W4_NORM_LN && colsum == nullptr) return -1;
  if (M < 1 || M > 256) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || act < ACT_NONE || act > ACT_SILU_MUL || norm < 0 || norm > W4_NORM_LN ||
      (act == ACT_SILU_MUL && N % 16 != 0))
    return -3;
  const int NO = act == ACT_SILU_MUL ? N / 2 : N;
  if (ldc < NO || lda < K || (R != nullptr && ldr < NO)) return -4;
  if ((((uintptr_t)A | (uintptr_t)Wq) & 15) != 0 || (lda & 7) != 0) return -5;
  switch (act) {
    case ACT_NONE: return launch_w4_mid_norm<ACT_NONE>(norm, W4_ARGS);
    case ACT_RELU: return launch_w4_mid_norm<ACT_RELU>(norm, W4_ARGS);
    case ACT_GELU: return launch_w4_mid_norm<ACT_GELU>(norm, W4_ARGS);
    default: return launch_w4_mid_norm<ACT_SILU_MUL>(norm, W4_ARGS);
  }
#undef W4_ARGS
}

// dnn_gemm_w4_mn: one workgroup per 64 rows x 32 columns, its waves split K by chunk parity (gemm_w4_mn.h).
template <int ACT>
static int launch_w4_mn(int norm, const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                        const float* bias, const void* R, int ldr, int M, int N, int K, const float* colsum, float eps,
                        hipStream_t st) {
  const dim3 grid(((N + 15) / 16 + 1) / 2, (M + W4N_BM - 1) / W4N_BM);
#define W4N_LAUNCH(NORM)                                                                                         \
  hipLaunchKernelGGL((gemm_w4_mn_kernel<ACT, NORM>), grid, dim3(256), W4N_LDS, st, (const uint8_t*)A, lda * 2, \
                     (const uint8_t*)Wq, (const uint8_t*)Ws, (bf16_t*)C, ldc, bias, (const bf16_t*)R, ldr, M, N, K, \
                     colsum, eps)
  switch (norm) {
    case W4_NORM_NONE: W4N_LAUNCH(W4_NORM_NONE); break;
    case W4_NORM_RMS: W4N_LAUNCH(W4_NORM_RMS); break;
    default: W4N_LAUNCH(W4_NORM_LN); break;
  }
#undef W4N_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int dnn_gemm_w4_mn(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                              const float* bias, const void* R, int ldr, int M, int N, int K, int act, int norm,
                              const float* colsum, float eps, hipStream_t st) {
  if (A == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (norm == W4_NORM_LN && colsum == nullptr) return -1;
  if (M < 1 || M > 256) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || act < ACT_NONE || act > ACT_SILU_MUL || norm < 0 || norm > W4_NORM_LN ||
      (act == ACT_SILU_MUL && N % 16 != 0))
    return -3;
  const int NO = act == ACT_SILU_MUL ? N / 2 : N;
  if (ldc < NO || lda < K || (R != nullptr && ldr < NO)) return -4;
  if ((((uintptr_t)A | (uintptr_t)Wq) & 15) != 0 || (lda & 7) != 0) return -5;
#define W4_ARGS A, lda, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, colsum, eps, st
  switch (act) {
    case ACT_NONE: return launch_w4_mn<ACT_NONE>(norm, W4_ARGS);
    case ACT_RELU: return launch_w4_mn<ACT_RELU>(norm, W4_ARGS);
    case ACT_GELU: return launch_w4_mn<ACT_GELU>(norm, W4_ARGS);
    default: return launch_w4_mn<ACT_SILU_MUL>(norm, W4_ARGS);
  }
#undef W4_ARGS
}

// dnn_gemm_w4_tile: one workgroup per 128 rows x 128 columns over the whole of K, the row blocks in grid x so that
// the workgroups of a column block are dispatched together (gemm_w4_tile.h).
template <int ACT>
static int launch_w4_tile(int norm, const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                          const float* bias, const void* R, int ldr, int M, int N, int K, const float* colsum,
                          float eps, hipStream_t st) {
  const dim3 grid((M + W4T_BM - 1) / W4T_BM, (N + W4T_BN - 1) / W4T_BN);
#define W4T_LAUNCH(NORM)                                                                                           \
  hipLaunchKernelGGL((gemm_w4_tile_kernel<ACT, NORM>), grid, dim3(256), W4T_LDS, st, (const uint8_t*)A, lda * 2, \
                     (const uint8_t*)Wq, (const uint8_t*)Ws, (bf16_t*)C, ldc, bias, (const bf16_t*)R, ldr, M, N, K, \
                     colsum, eps)
  switch (norm) {
    case W4_NORM_NONE: W4T_LAUNCH(W4_NORM_NONE); break;
    case W4_NORM_RMS: W4T_LAUNCH(W4_NORM_RMS); break;
    default: W4T_LAUNCH(W4_NORM_LN); break;
  }
#undef W4T_LAUNCH
  return (int)hipGetLastError();
}

extern "C" int dnn_gemm_w4_tile(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                                const float* bias, const void* R, int ldr, int M, int N, int K, int act, int norm,
                                const float* colsum, float eps, hipStream_t st) {
  if (A == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (norm == W4_NORM_LN && colsum == nullptr) return -1;
  if (M < 1) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || act < ACT_NONE || act > ACT_SILU_MUL || norm < 0 || norm > W4_NORM_LN ||
      (act == ACT_SILU_MUL && N % 16 != 0) || (N + W4T_BN - 1) / W4T_BN > 65535)
    return -3;
  const int NO = act == ACT_SILU_MUL ? N / 2 : N;
  if (ldc < NO || lda < K || (R != nullptr && ldr < NO)) return -4;
  if ((((uintptr_t)A | (uintptr_t)Wq) & 15) != 0 || (lda & 7) != 0) return -5;
#define W4_ARGS A, lda, Wq, Ws, C, ldc, bias, R, ldr, M, N, K, colsum, eps, st
  switch (act) {
    case ACT_NONE: return launch_w4_tile<ACT_NONE>(norm, W4_ARGS);
    case ACT_RELU: return launch_w4_tile<ACT_RELU>(norm, W4_ARGS);
    case ACT_GELU: return launch_w4_tile<ACT_GELU>(norm, W4_ARGS);
    default: return launch_w4_tile<ACT_SILU_MUL>(norm, W4_ARGS);
  }
#undef W4_ARGS
}

// dnn_gemm_w4_head: one persistent workgroup per 8 column tiles, at most one per CU (gemm_w4_head.h).
static int w4_head_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cus[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cus[dev] = v;
  }
  return cus[dev];
}

extern "C" int dnn_gemm_w4_head(const void* A, int lda, const void* Wq, const void* Ws, void* C, int ldc,
                                const float* bias, int M, int N, int K, int norm, const float* colsum, float eps,
                                void* part, int part_cap, hipStream_t st) {
  if (A == nullptr || Wq == nullptr || Ws == nullptr || C == nullptr) return -1;
  if (norm == W4_NORM_LN && colsum == nullptr) return -1;
  if (M < 1 || M > 64) return -2;
  if (N < 1 || K < 32 || K % 32 != 0 || norm < 0 || norm > W4_NORM_LN) return -3;
  const int ntile = (N + 15) / 16, cus = w4_head_cus();
  if (cus <= 0) return -6;
  const int grid = std::min(cus, (ntile + W4H_WAVES - 1) / W4H_WAVES);
  if (part != nullptr && part_cap < grid) return -3;
  if (ldc < N || lda < K) return -4;
  if ((((uintptr_t)A | (uintptr_t)Wq | (uintptr_t)C) & 15) != 0 || (lda & 7) != 0 || (ldc & 7) != 0) return -5;
  const int mt = (M + 15) / 16, nch = (K + 127) / 128, cpp = std::min(nch, W4H_IMG / mt);
  const size_t smem = (size_t)mt * 16 * cpp * 256 + W4H_TAIL;
#define W4H_LAUNCH(NORM)                                                                                          \
  hipLaunchKernelGGL((gemm_w4_head_kernel<NORM>), dim3(grid), dim3(64 * W4H_WAVES), smem, st, (const uint8_t*)A, \
                     lda * 2, (const uint8_t*)Wq, (const uint8_t*)Ws, (bf16_t*)C, ldc, bias, colsum, eps, M, N, K, \
                     (int2*)part)
  switch (norm) {
    case W4_NORM_NONE: W4H_LAUNCH(W4_NORM_NONE); break;
    case W4_NORM_RMS: W4H_LAUNCH(W4_NORM_RMS); break;
    default: W4H_LAUNCH(W4_NORM_LN); break;
  }
#undef W4H_LAUNCH
  return hipGetLastError() != hipSuccess ? -7 : grid;
}

extern "C" int dnn_w4_expand(const void* Wq, const void* Ws, void* W, int ldw, int N, int K, hipStream_t st) {
  if (Wq == nullptr || Ws == nullptr || W == nullptr) return -1;
  if (N < 1 || K < 32 || K % 32 != 0) return -3;
  if (ldw < K) return -4;
  if ((((uintptr_t)Wq | (uintptr_t)W) & 15) != 0 || (ldw & 7) != 0) return -5;
  const int nch = (K + 127) / 128;
  const long long nblk = (long long)((N + 15) / 16) * nch;
  if (nblk > 0x7fffffffll) return -3;
  hipLaunchKernelGGL(w4_expand_kernel, dim3((unsigned)((nblk + 3) / 4)), dim3(256), 0, st, (const uint8_t*)Wq,
                     (const uint8_t*)Ws, (bf16_t*)W, ldw, N, K, nch, (int)nblk);
  return (int)hipGetLastError();
}
