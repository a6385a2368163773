// MXFP4 W4A16 GEMM for decode microbatches of up to 256 rows ("mid" kernel),
// included by gemm_w4.hip (which states the weight's fragment order and holds
// w4_to_bf16 / w4_stats):
//
//   C[M,N] = act(norm(A)[M,K] . dq(W)[N,K]^T + bias[n]) (+ R[M,N]),   1 <= M <= 256
//
// dnn_gemm_w4 gives every column tile its own workgroup, whose waves split K
// and each load all M activation rows: at 64 rows it is bound by activation
// traffic, and above 64 rows the stage used to expand the weight to bf16
// (dnn_w4_expand) and run the bf16 tile kernels: 8.5 x the bytes of the codes.
// Here the waves of a workgroup split N and share A through LDS:
//   * a workgroup of 4 waves owns 64 NT output columns (wave w: column tiles
//     NT w .. NT w + NT - 1 of the workgroup's) and ALL M rows, over the whole
//     of K: every weight byte is loaded once per step, no M split, no
//     cross-workgroup K split, no atomics, one fixed summation order (the
//     chunks in ascending k inside the MFMA accumulators), so a result is the
//     same bits on every launch;
//   * weights: a wave streams its tiles' chunks (1 KiB of codes and 64 scale
//     bytes per tile and 128 k) straight to VGPRs with non-temporal 16-byte
//     loads, U = 4 chunks in flight as a ring (chunk c + 4 is requested as soon
//     as chunk c is converted); v_cvt_scalef32_pk_bf16_fp4 is exact, and the
//     bf16 16x16x32 MFMA takes the weight as its first operand: transposed
//     accumulators, the shared epi_t4 / epi_silu_t4 epilogues;
//   * A: one K step is one 128-k chunk.  The 256 threads stage it in full row
//     segments: thread (sr = tid >> 4, sj = tid & 15) loads 16-byte slot sj of
//     rows 16 i + sr (16 consecutive lanes: the 256 contiguous bytes of one
//     row's chunk, global_load_dwordx4) and writes it with ds_write_b128.  Two
//     LDS stages: chunk c + 1 is requested before chunk c's MFMAs and written
//     to the other stage after them, one barrier per chunk;
//   * row statistics (folded RMS / LayerNorm, the shifted form of w4_stats) are
//     taken in the staging pass, which holds every A element in registers
//     exactly once per workgroup; the 16 lanes of a row meet by shuffles in a
//     fixed order and leave {sum, sum of squares} per row in LDS.
//
// LDS image of a stage: 16 mt rows x 256 B (mt = M tiles of 16 rows), 16-byte
// slot j (= 4 g + h: k 32 g + 8 h .. + 7 of the chunk) of row r stored at slot
// j ^ (r & 15).  A staging ds_write_b128 puts 16 consecutive lanes on the 16
// slots of one row; a fragment ds_read_b128 (MFMA h of M tile t: lane 16 g + r
// reads slot 4 g + h of row 16 t + r) puts the 16 lanes of each of its four
// lane groups on 16 distinct slots of 16 rows at a 256-byte pitch.  Checked
// exhaustively on the host (every t < 16, h < 4, lane group, and every staging
// write of 16 tiles; 64 banks of 4 bytes, 16 lanes per pass): each pass touches
// every bank exactly once, 0 conflicts in 256 read passes and 1024 write
// passes; without the xor every read pass is a 16-way conflict.
// LDS: 2 stages x 4 KiB x mt + 128 B x mt of statistics: 130 KiB at 256 rows
// (one workgroup per CU), 65 KiB at 128 rows (two).
//
// Choices:
//   * NT, column tiles per wave.  NT = 1 issues one ds_read_b128 of A per MFMA,
//     NT = 2 one per two MFMAs, at 4 MT x NT accumulator registers (16 tiles:
//     64 / 128, in AGPRs).  NT = 2 halves the workgroups (N / 128), and no K or
//     M split refills them, so it is used only where N / 128 still covers at
//     least half of the 256 CUs (N >= 16384: Llama-3 8B gate|up); everything
//     narrower takes NT = 1 (N / 64 workgroups).  Measured against expansion +
//     bf16 GEMM (bench/probes/w4_mid_ab.py, profiles/w4_mid_ab.jsonl, us per
//     launch at 96 / 128 / 256 rows): 4096 -> 6144 37.5 / 46.0 / 77.4 against
//     75.1 / 84.4 / 142.8; 4096 -> 28672 (NT = 2) 45.5 / 54.8 / 122.2 against
//     107.7 / 102.7 / 122.7, a tie at 256 rows; 1600 -> 1600 (25 workgroups)
//     17.8 / 21.3 / 34.5 against 17.2 / 17.3 / 26.4: narrow N loses, and
//     ops/w4.py w4_mid_ok keeps such shapes on the expansion.
//   * 4 waves per workgroup: at 256 rows the two stages fill the CU's LDS, so
//     the CU holds one workgroup, one wave per SIMD with the whole register
//     file for the staging registers (4 MT), the accumulators and the ring.
//   * M templates: NT = 2 has 8 and 16 M tiles (8: at most 248 VGPRs, no AGPRs,
//     two waves per SIMD); NT = 1 has 16 only (the 8-tile form spilled under
//     the two-waves bound; 16 tiles take 163-217 VGPRs + 64 AGPRs, two waves
//     per SIMD without LayerNorm).  Tiles at or past mt are skipped on a
//     wave-uniform condition, row addresses past M - 1 clamp.
//   * registers (-Rpass-analysis=kernel-resource-usage): no instantiation uses
//     scratch; the largest, LayerNorm at MT 16 / NT 2, 255 VGPRs + 128 AGPRs.
// K % 128 != 0: the last chunk's 32-k groups at or past K are not read (the
// address falls back to the chunk's first group, the slot is zeroed and left
// out of the statistics).  Column tiles past N (N = 40: tiles 3 of 4) read the
// last real tile's weights and store nothing.
#pragma once
#include "gemm_epilogue.h"

namespace dnn {

constexpr int W4M_WAVES = 4;   // waves per workgroup, each NT column tiles
constexpr int W4M_U = 4;       // weight chunks in flight per wave and tile
constexpr int W4M_ROW = 256;   // LDS bytes per row and stage: one 128-k chunk of bf16

template <int ACT, int NORM, int MT, int NT>
__global__ __launch_bounds__(64 * W4M_WAVES, MT <= 8 ? 2 : 1) void gemm_w4_mid_kernel(
    const uint8_t* __restrict__ A, int lda_b, const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ Ws,
    bf16_t* __restrict__ C, int ldc, const float* __restrict__ bias, const bf16_t* __restrict__ R, int ldr, int M,
    int N, int K, const float* __restrict__ colsum, float eps) {
  extern __shared__ __attribute__((aligned(16))) uint8_t w4m_lds[];  // [2][16 mt][256], then float2 [16 mt] statistics
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int mt = (M + 15) >> 4;    // M tiles in use (<= MT)
  const int nch = (K + 127) >> 7;  // 128-k chunks (the last may be partial)
  const int kg = K >> 5;           // valid 32-k groups
  const int ntile = (N + 15) >> 4;
  const int stage_b = mt * 16 * W4M_ROW;
  float2* w4m_st = reinterpret_cast<float2*>(w4m_lds + 2 * stage_b);

  // this wave's column tiles (a tile past N repeats the last real one and stores nothing)
  const int ct0 = ((int)blockIdx.x * W4M_WAVES + wave) * NT;
  const uint8_t* wp[NT];
  const uint8_t* sp[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int ct = min(ct0 + j, ntile - 1);
    wp[j] = Wq + ((size_t)ct * nch * 64 + lane) * 16;  // + chunk * 1024
    sp[j] = Ws + (size_t)ct * nch * 64 + lane;         // + chunk * 64
  }

  // staging role: slot sj of rows 16 i + sr
  const int sj = tid & 15, sr = tid >> 4;
  const int lds_w = sr * W4M_ROW + ((sj ^ sr) << 4);  // + i * 16 rows, + stage
  float st1[MT], st2[MT], shift[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    st1[i] = st2[i] = 0.f;
    shift[i] = 0.f;
    if constexpr (NORM == W4_NORM_LN) {
      if (i < mt)
        shift[i] = __uint_as_float(
            (uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(16 * i + sr, M - 1) * lda_b)) << 16);
    }
  }
  i32x4 areg[MT];
  // request chunk c of A (rows past M - 1 clamp; a group at or past K reads the chunk's first group)
  auto a_load = [&](int c) {
    const bool ok = c * 4 + (sj >> 2) < kg;
    const int so = c * W4M_ROW + (ok ? sj : (sj & 3)) * 16;
#pragma unroll
    for (int i = 0; i < MT; ++i)
      if (i < mt) areg[i] = *reinterpret_cast<const i32x4*>(A + (size_t)min(16 * i + sr, M - 1) * lda_b + so);
  };
  // statistics of the chunk in areg, then its ds_write_b128 into stage s
  auto a_store = [&](int c, int s) {
    const bool ok = c * 4 + (sj >> 2) < kg;
    uint8_t* dst = w4m_lds + s * stage_b + lds_w;
#pragma unroll
    for (int i = 0; i < MT; ++i)
      if (i < mt) {
        if (!ok) areg[i] = i32x4{0, 0, 0, 0};
        if constexpr (NORM != W4_NORM_NONE) {
          if (ok) w4_stats<NORM>(areg[i], shift[i], st1[i], st2[i]);
        }
        *reinterpret_cast<i32x4*>(dst + i * 16 * W4M_ROW) = areg[i];
      }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the first U weight chunks and A chunk 0
  i32x4 wv[W4M_U][NT];
  uint32_t sc[W4M_U][NT];
#pragma unroll
  for (int u = 0; u < W4M_U; ++u) {
    const int ci = min(u, nch - 1);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      wv[u][j] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[j] + (size_t)ci * 1024));
      sc[u][j] = sp[j][(size_t)ci * 64];
    }
  }
  a_load(0);
  a_store(0, 0);
  __syncthreads();

  const int lds_r = r * W4M_ROW;  // fragment reads: + 16 t rows, slot (4 g + h) ^ r
#pragma unroll 1
  for (int cb = 0; cb < nch; cb += W4M_U) {
#pragma unroll
    for (int u = 0; u < W4M_U; ++u) {
      const int c = cb + u;
      if (c < nch) {  // uniform over the workgroup
        const bool more = c + 1 < nch;
        if (more) a_load(c + 1);  // in flight under this chunk's MFMAs
        bf16x8 wb[NT][4];
#pragma unroll
        for (int j = 0; j < NT; ++j) w4_to_bf16(wv[u][j], __uint_as_float(sc[u][j] << 23), wb[j]);
        {  // the ring: chunk c + U into the registers chunk c has left (a surplus load repeats the last chunk)
          const int ci = min(c + W4M_U, nch - 1);
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            wv[u][j] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[j] + (size_t)ci * 1024));
            sc[u][j] = sp[j][(size_t)ci * 64];
          }
        }
        const uint8_t* src = w4m_lds + (c & 1) * stage_b + lds_r;
#pragma unroll
        for (int t = 0; t < MT; ++t)
          if (t < mt) {  // wave-uniform
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const bf16x8 ab = *reinterpret_cast<const bf16x8*>(src + t * 16 * W4M_ROW + (((4 * g + h) ^ r) << 4));
#pragma unroll
              for (int j = 0; j < NT; ++j)
                acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j][h], ab, acc[j][t], 0, 0, 0);
            }
            // two workgroups per CU leave a wave 256 registers: the scheduler may hoist the fragment reads
            // of 4 M tiles (64 registers) ahead of their MFMAs, not of all 8 (it spilled)
            if constexpr (MT <= 8) {
              if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
          }
        if (more) a_store(c + 1, (c + 1) & 1);
        __syncthreads();  // stage (c + 1) & 1 written, stage c & 1 free for chunk c + 2
      }
    }
  }

  if constexpr (NORM != W4_NORM_NONE) {
    // the 16 lanes tid = 16 sr + sj of a row hold disjoint k
#pragma unroll
    for (int i = 0; i < MT; ++i)
      if (i < mt) {
        float a = st1[i], s = st2[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          a += __shfl_xor(a, o, 64);
          s += __shfl_xor(s, o, 64);
        }
        if (sj == 0) w4m_st[16 * i + sr] = make_float2(a, s);
      }
    __syncthreads();
  }

  const int NO = ACT == ACT_SILU_MUL ? N / 2 : N;
  const bool vec = epi_vec_ok(C, ldc, bias, R, ldr);
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    if (t >= mt) continue;  // wave-uniform
    const int m = t * 16 + r;
    float mean = 0.f, rstd = 1.f;
    if constexpr (NORM != W4_NORM_NONE) {
      const float2 st = w4m_st[m];
      const float invk = 1.f / (float)K;
      const float d = st.x * invk;  // E[x - c]
      if constexpr (NORM == W4_NORM_LN)
        mean = d + __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(m, M - 1) * lda_b))
                                   << 16);
      const float var = NORM == W4_NORM_LN ? fmaxf(st.y * invk - d * d, 0.f) : st.y * invk;
      rstd = rsqrtf(var + eps);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n0 = (ct0 + j) * 16;
      if (n0 >= N) continue;  // wave-uniform: a tile past N
      const int n = n0 + g * 4;
      f32x4 s = acc[j][t];
      if constexpr (NORM == W4_NORM_LN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = rstd * (s[i] - mean * (n + i < N ? colsum[n + i] : 0.f));
      } else if constexpr (NORM == W4_NORM_RMS) {
        s *= rstd;
      }
      if constexpr (ACT == ACT_SILU_MUL) {
        epi_silu_t4<false>(s, m, n0 / 2, M, NO, C, ldc, vec, lane);
      } else {
        epi_t4<ACT, false>(s, m, n, M, N, C, ldc, bias, R, ldr, vec);
      }
    }
  }
}

}  // namespace dnn
