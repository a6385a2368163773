// MXFP4 W4A16 GEMM for decode microbatches of up to 256 rows on NARROW
// projections ("mn" kernel: workgroups tile M and N), included by gemm_w4.hip
// (which states the weight's fragment order and holds w4_to_bf16 / w4_stats):
//
//   C[M,N] = act(norm(A)[M,K] . dq(W)[N,K]^T + bias[n]) (+ R[M,N]),   1 <= M <= 256
//
// dnn_gemm_w4_mid gives a workgroup 64 columns and ALL rows: N / 64 workgroups,
// 25 on a 1600-wide projection, cannot fill 256 CUs, and such shapes stayed on
// the expansion (8.5 x the bytes of the codes, two launches).  Here the grid
// tiles both M and N and the waves of a workgroup split K:
//   * a workgroup owns 64 rows (4 M tiles) x 32 columns (2 column tiles) over
//     the whole of K; grid = ceil(N / 32) x ceil(M / 64): 200 workgroups for
//     1600 columns x 256 rows, 96 for 768 x 256.  Every M block reads the codes
//     again, from L2: these weights are a few MB at most (which is what makes
//     the M split right here and wrong in dnn_gemm_w4);
//   * 4 waves = (column tile w & 1, chunk parity w >> 1).  One K step is two
//     128-k chunks (256 k): waves 0 / 1 multiply the even chunk, waves 2 / 3 the
//     odd one.  With an odd chunk count the last step has no odd chunk: waves
//     2 / 3 skip it on a wave-uniform condition (at K = 128 they add nothing);
//   * weights: a wave streams its tile's chunks of its parity (1 KiB of codes
//     and 64 scale bytes per chunk) straight to VGPRs with non-temporal 16-byte
//     loads, a ring of U = 8 chunks (16 chunks = 2048 k of the tile in flight
//     per column tile); w4_to_bf16 is exact, the weight is the first operand of
//     mfma_f32_16x16x32_bf16: transposed accumulators, 4 per wave;
//   * A: the 256 threads stage a step in full row segments: thread (sr =
//     tid >> 5, sj = tid & 31) loads 16-byte slot sj of rows 8 i + sr (32
//     consecutive lanes: the 512 contiguous bytes of one row's step,
//     global_load_dwordx4) and writes it with ds_write_b128.  Two LDS stages:
//     step s + 1 is requested before step s's MFMAs and written to the other
//     stage after them, one barrier per step;
//   * row statistics (folded RMS / LayerNorm, the shifted form of w4_stats) are
//     taken in the staging pass, every A element once per workgroup; the 32
//     lanes of a row meet by shuffles in a fixed order;
//   * reduction: after the last step waves 2 / 3 leave their 4 accumulators in
//     stage 0 (free by then), waves 0 / 1 add them (even part + odd part) and
//     run the shared epi_t4 / epi_silu_t4 epilogues.  No atomics, no
//     cross-workgroup state, one fixed summation order: a result is the same
//     bits on every launch and under graph replay.
//
// LDS image of a stage: 64 rows x 512 B, 16-byte slot j (= 16 p + 4 g + h:
// chunk parity p, k 32 g + 8 h .. + 7 of that chunk) of row r stored at slot
// j ^ (r & 15) (the xor moves the low four bits only: a slot stays in its
// chunk's half of the row).  A staging ds_write_b128 puts 16 consecutive lanes
// on 16 slots of one half row; a fragment ds_read_b128 (parity p, MFMA h of M
// tile t: lane 16 g + r reads slot 16 p + 4 g + h of row 16 t + r) puts the 16
// lanes of each of its four lane groups on 16 distinct slots (mod 16) of 16
// rows at a 512-byte pitch.  Enumerated on the host (64 banks of 4 bytes, 16
// lanes per pass; every t < 4, h < 4, p < 2 and lane group: 128 read passes;
// every staging write of 8 row groups x 16 passes: 128 write passes): each pass
// touches every bank exactly once, 0 conflicts; without the xor every read
// pass is a 16-way conflict (a 512-byte pitch puts all rows on the same banks).
// LDS: 2 stages x 32 KiB + 512 B of statistics = 64.5 KiB, two workgroups per
// CU (8 waves, 2 per SIMD).
//
// Edges.  Rows past M - 1 clamp on load and are not stored; M tiles of the last
// block at or past M are skipped on a wave-uniform condition.  A column tile
// past N (N = 40: tile 3 of block 1) repeats the last real tile's weights and
// stores nothing.  K % 128 != 0: 32-k groups at or past K are not read (the
// address falls back to the step's first group, the slot is zeroed and left
// out of the statistics); surplus ring loads repeat the last chunk.
//
// Choices:
//   * 64 x 32 block, parity K split: the starting design, kept; every block
//     reads 64 rows of A per 32 columns, so A traffic from L2 is N / 32 x M x
//     2 K bytes (1600 -> 1600 at 256 rows: 41 MB, against 1.3 MB of codes read
//     four times).  A 64 x 64 block halves that and halves the workgroups:
//     not measured, no other split was tried.  Measured against the mid
//     kernel and against expansion + bf16 GEMM (bench/probes/w4_mn_ab.py,
//     profiles/w4_mn_ab.jsonl, us per launch at 96 / 128 / 256 rows, mn | mid
//     | expand): 768 -> 2304 6.8 / 6.8 / 8.2 | 10.4 / 12.2 / 18.9 | 11.2 /
//     13.2 / 17.5; 1600 -> 1600 11.3 / 11.3 / 11.9 | 17.7 / 21.2 / 34.3 |
//     16.9 / 17.0 / 26.0; 6400 -> 1600 32.1 / 32.3 / 34.7 | 55.8 / 68.8 /
//     116.6 | 47.8 / 47.6 / 76.3; 4096 -> 6144 24.9 / 28.9 / 47.4 | 37.4 /
//     46.0 / 76.7 | 74.1 / 83.4 / 142.5.  It wins all nine shapes of the probe
//     at all three row counts; ops/w4.py w4_mn_ok holds the routing rule and
//     the whole table.
//   * U = 8: the narrow projections have 6..50 chunks, 3..25 per wave, so the
//     ring holds most or all of a wave's weights from the prologue on (40
//     VGPRs); the kernel is bound by latency, not by registers.  Reasoned:
//     U = 4 was not measured against it.
//   * registers (-Rpass-analysis=kernel-resource-usage), the 12 instantiations
//     (ACT 0..3 x NORM 0..2): no norm 206-207 VGPRs, RMS 216-217, LayerNorm
//     232-234; no AGPRs, no scratch, no spills; two waves per SIMD, which is
//     what the two workgroups per CU that LDS allows need.
#pragma once
#include "gemm_epilogue.h"

namespace dnn {

constexpr int W4N_U = 8;        // weight chunks in flight per wave
constexpr int W4N_ROW = 512;    // LDS bytes per row and stage: two 128-k chunks of bf16
constexpr int W4N_BM = 64;      // rows per workgroup (4 M tiles)
constexpr int W4N_STAGE = W4N_BM * W4N_ROW;
constexpr int W4N_LDS = 2 * W4N_STAGE + W4N_BM * (int)sizeof(float2);

template <int ACT, int NORM>
__global__ __launch_bounds__(256, 2) void gemm_w4_mn_kernel(
    const uint8_t* __restrict__ A, int lda_b, const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ Ws,
    bf16_t* __restrict__ C, int ldc, const float* __restrict__ bias, const bf16_t* __restrict__ R, int ldr, int M,
    int N, int K, const float* __restrict__ colsum, float eps) {
  extern __shared__ __attribute__((aligned(16))) uint8_t w4n_lds[];  // [2][64][512], then float2 [64] statistics
  float2* w4n_st = reinterpret_cast<float2*>(w4n_lds + 2 * W4N_STAGE);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int par = wave >> 1;               // chunk parity of this wave
  const int nch = (K + 127) >> 7;          // 128-k chunks (the last may be partial)
  const int nst = (nch + 1) >> 1;          // K steps of two chunks
  const int kg = K >> 5;                   // valid 32-k groups
  const int ntile = (N + 15) >> 4;
  const int m0 = (int)blockIdx.y * W4N_BM;  // < M by the grid
  const int mtl = min(4, (M - m0 + 15) >> 4);  // M tiles in use in this block (>= 1)

  // this wave's column tile (a tile past N repeats the last real one and stores nothing)
  const int ct0 = (int)blockIdx.x * 2 + (wave & 1);
  const int ct = min(ct0, ntile - 1);
  const uint8_t* wp = Wq + ((size_t)ct * nch * 64 + lane) * 16;  // + chunk * 1024
  const uint8_t* sp = Ws + (size_t)ct * nch * 64 + lane;         // + chunk * 64

  // staging role: slot sj of rows 8 i + sr
  const int sj = tid & 31, sr = tid >> 5;
  float st1[8], st2[8], shift[8];
  const uint8_t* arow[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    arow[i] = A + (size_t)min(m0 + 8 * i + sr, M - 1) * lda_b;
    st1[i] = st2[i] = 0.f;
    shift[i] = 0.f;
    if constexpr (NORM == W4_NORM_LN) {
      if (i < 2 * mtl) shift[i] = __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(arow[i])) << 16);
    }
  }
  i32x4 areg[8];
  // request step s of A (a group at or past K reads the step's first group, which exists)
  auto a_load = [&](int s) {
    const bool ok = s * 8 + (sj >> 2) < kg;
    const int so = s * W4N_ROW + (ok ? sj : (sj & 3)) * 16;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < 2 * mtl) areg[i] = *reinterpret_cast<const i32x4*>(arow[i] + so);
  };
  // statistics of the step in areg, then its ds_write_b128 into stage st
  auto a_store = [&](int s, int st) {
    const bool ok = s * 8 + (sj >> 2) < kg;
    uint8_t* dst = w4n_lds + st * W4N_STAGE + sr * W4N_ROW;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < 2 * mtl) {
        if (!ok) areg[i] = i32x4{0, 0, 0, 0};
        if constexpr (NORM != W4_NORM_NONE) {
          if (ok) w4_stats<NORM>(areg[i], shift[i], st1[i], st2[i]);
        }
        // row 8 i + sr: (row & 15) = 8 (i & 1) + sr
        *reinterpret_cast<i32x4*>(dst + i * 8 * W4N_ROW + ((sj ^ (8 * (i & 1) + sr)) << 4)) = areg[i];
      }
  };

  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the wave's first U chunks (of its parity) and A step 0
  i32x4 wv[W4N_U];
  uint32_t sc[W4N_U];
#pragma unroll
  for (int u = 0; u < W4N_U; ++u) {
    const int ci = min(2 * u + par, nch - 1);
    wv[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (size_t)ci * 1024));
    sc[u] = sp[(size_t)ci * 64];
  }
  a_load(0);
  a_store(0, 0);
  __syncthreads();

  const int lds_r = r * W4N_ROW;  // fragment reads: + 16 t rows, slot (16 par + 4 g + h) ^ r
#pragma unroll 1
  for (int sb = 0; sb < nst; sb += W4N_U) {
#pragma unroll
    for (int u = 0; u < W4N_U; ++u) {
      const int s = sb + u;
      if (s < nst) {  // uniform over the workgroup
        const bool more = s + 1 < nst;
        if (more) a_load(s + 1);  // in flight under this step's MFMAs
        if (2 * s + par < nch) {  // wave-uniform: the last step of an odd chunk count has no odd chunk
          bf16x8 wb[4];
          w4_to_bf16(wv[u], __uint_as_float(sc[u] << 23), wb);
          {  // the ring: the wave's chunk U steps on, into the registers this one has left
            const int ci = min(2 * (s + W4N_U) + par, nch - 1);
            wv[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp + (size_t)ci * 1024));
            sc[u] = sp[(size_t)ci * 64];
          }
          const uint8_t* src = w4n_lds + (s & 1) * W4N_STAGE + lds_r;
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (t < mtl) {  // wave-uniform
#pragma unroll
              for (int h = 0; h < 4; ++h) {
                const bf16x8 ab =
                    *reinterpret_cast<const bf16x8*>(src + t * 16 * W4N_ROW + (((16 * par + 4 * g + h) ^ r) << 4));
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[h], ab, acc[t], 0, 0, 0);
              }
            }
        }
        if (more) a_store(s + 1, (s + 1) & 1);
        __syncthreads();  // stage (s + 1) & 1 written, stage s & 1 free for step s + 2
      }
    }
  }

  // both stages are free: the odd-parity waves leave their partial sums in stage 0
  f32x4* red = reinterpret_cast<f32x4*>(w4n_lds) + (wave & 1) * 4 * 64 + lane;  // + t * 64
  if (par == 1) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (t < mtl) red[t * 64] = acc[t];
  }
  if constexpr (NORM != W4_NORM_NONE) {
    // the 32 lanes tid = 32 sr + sj of a row hold disjoint k
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < 2 * mtl) {
        float a = st1[i], q = st2[i];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          a += __shfl_xor(a, o, 64);
          q += __shfl_xor(q, o, 64);
        }
        if (sj == 0) w4n_st[8 * i + sr] = make_float2(a, q);
      }
  }
  __syncthreads();
  if (par == 1) return;

  const int NO = ACT == ACT_SILU_MUL ? N / 2 : N;
  const bool vec = epi_vec_ok(C, ldc, bias, R, ldr);
  const int n0 = ct0 * 16;
  if (n0 >= N) return;  // wave-uniform: a tile past N
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t >= mtl) continue;  // wave-uniform
    const int m = m0 + t * 16 + r;
    f32x4 s = acc[t] + red[t * 64];  // even part + odd part
    if constexpr (NORM != W4_NORM_NONE) {
      const float2 st = w4n_st[t * 16 + r];
      const float invk = 1.f / (float)K;
      const float d = st.x * invk;  // E[x - c]
      float mean = 0.f;
      if constexpr (NORM == W4_NORM_LN)
        mean = d + __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(m, M - 1) * lda_b))
                                   << 16);
      const float var = NORM == W4_NORM_LN ? fmaxf(st.y * invk - d * d, 0.f) : st.y * invk;
      const float rstd = rsqrtf(var + eps);
      const int n = n0 + g * 4;
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
      epi_t4<ACT, false>(s, m, n0 + g * 4, M, N, C, ldc, bias, R, ldr, vec);
    }
  }
}

}  // namespace dnn
