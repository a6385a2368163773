// MXFP4 W4A16 tile GEMM for any number of rows ("tile" kernel), included by
// gemm_w4.hip (which states the weight's fragment order and holds w4_to_bf16 /
// w4_stats):
//
//   C[M,N] = act(norm(A)[M,K] . dq(W)[N,K]^T + bias[n]) (+ R[M,N]),   M >= 1
//
// dnn_gemm_w4_mid holds all M rows in one workgroup (256 at most) and
// dnn_gemm_w4_mn gives a workgroup 64 x 32 outputs whose waves split K: both
// are weight-stream kernels.  Every other step of more than 64 rows (prefill
// pieces at bf16 activation fidelity, decode above 256 rows, all-position
// logits) used to expand the projection to bf16 (dnn_w4_expand) and run the
// bf16 tile kernels on it: 8.5 x the bytes of the codes, written and read back
// once per projection and step.  This kernel is the compute-bound form on the
// codes:
//   * split: the grid tiles M (x, the fast index: the workgroups of one column
//     block are neighbours in dispatch order, so its codes come from HBM once
//     and from L2 afterwards) and N (y).  A workgroup of 4 waves owns a 128 x
//     128 output block over the whole of K; wave (wm = wave >> 1, wn = wave & 1)
//     owns M tiles 4 wm .. + 3 and column tiles 4 wn .. + 3 of the block: 64 x
//     64, 16 accumulator tiles.  No K split, no atomics, one fixed summation
//     order (the chunks in ascending k inside the MFMA accumulators), so a
//     result is the same bits on every launch;
//   * A: one K step is one 128-k chunk of the block's 128 rows.  The 256
//     threads stage it as the mid kernel does (thread (sr = tid >> 4, sj = tid
//     & 15): 16-byte slot sj of rows 16 i + sr, i < 8; global_load_dwordx4,
//     ds_write_b128), two LDS stages of 32 KiB, chunk c + 1 requested before
//     chunk c's MFMAs and written after them, one barrier per chunk.  The LDS
//     image and its xor slot swizzle are gemm_w4_mid.h's (slot j of row r at
//     slot j ^ (r & 15): conflict-free for these writes and fragment reads);
//   * per chunk a wave reads its 16 A fragments (4 M tiles x 4 h,
//     ds_read_b128) once: they feed the 64 MFMAs of its four column tiles;
//   * weights: a wave streams the chunks of its four column tiles straight to
//     VGPRs with 16-byte loads (1 KiB of codes and 64 scale bytes per tile and
//     chunk), U = 2 chunks in flight as a ring (chunk c + 2 of a tile is
//     requested as soon as chunk c of it is converted).  The loads are plain,
//     not non-temporal: the two waves wm = 0 / 1 and every M block read the
//     same bytes.  A tile's 32 codes per lane are converted
//     (v_cvt_scalef32_pk_bf16_fp4, exact) right before that tile's 16 MFMAs,
//     so one tile's four bf16x8 are live at a time, and the converted fragment
//     serves all four M tiles: one convert per 8 MFMA-k-steps of output rows,
//     a quarter of the mid kernel's per output at its 16-row granularity;
//   * the weight is the MFMA's first operand: transposed accumulators, the
//     shared epi_t4 / epi_silu_t4 epilogues (R may be C: a lane reads the four
//     residual values it then overwrites);
//   * row statistics (folded RMS / LayerNorm, the shifted form of w4_stats) are
//     taken in the staging pass, which holds every A element of the block's
//     rows in registers exactly once; the 16 lanes of a row meet by shuffles
//     in a fixed order and leave {sum, sum of squares} per row in LDS.
// LDS: 2 stages x 32 KiB + 1 KiB of statistics = 65 KiB: two workgroups per CU.
//
// Edges.  Rows past M - 1 clamp on load and store nothing; the M tiles of a
// block at or past ceil(rows / 16) are neither staged nor multiplied (uniform
// over the wave).  K % 128 != 0: the last chunk's 32-k groups at or past K are
// not read (the address falls back to the chunk's first group, the slot is
// zeroed and left out of the statistics).  A column tile past N (N = 40: tiles
// 3..7 of the block; N = 50257: the last block holds 5 real tiles) reads the
// last real tile's weights and stores nothing.
//
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950): no instantiation
// uses scratch.  Without a norm: 252 VGPRs, no AGPRs, two waves per SIMD (two
// workgroups per CU, which the LDS allows).  With the folded norm the staging
// statistics push the two-workgroup form past 256 registers (it spilled 28-100
// bytes per lane), so those instantiations are bounded at one workgroup per
// CU: RMS 198 VGPRs + 64 AGPRs (the accumulators), LayerNorm 214 (216 with
// SiLU-mul) + 64.
// Measured against expansion + bf16 GEMM (bench/probes/w4_tile_ab.py,
// profiles/w4_tile_ab.jsonl: HIP graphs rotating over weight copies, the two
// arms replayed in turn, medians of 5 rounds; the min-max spread of an arm is
// under 7 % except gate|up at 129 rows, tile arm, 23 %), us per launch
// at 129 / 384 / 512 / 1024 / 2048 / 8192 / 32768 rows, tile | expand:
//  768 -> 2304    13 / 13 / 13 / 14 / 18 / 43 / 158  |  13 / 15 / 15 / 15 / 20 / 43 / 113
//  3072 -> 768    37 / 38 / 38 / 38 / 38 / 50 / 174  |  18 / 37 / 39 / 41 / 40 / 47 / 119
//  1600 -> 6400   23 / 24 / 24 / 32 / 58 / 188 / 778  |  51 / 33 / 32 / 34 / 44 / 148 / 518
//  6400 -> 1600   72 / 75 / 74 / 74 / 75 / 188 / 943  |  48 / 114 / 77 / 75 / 76 / 130 / 552
//  4096 -> 6144   49 / 50 / 50 / 66 / 109 / 400 / 1806  |  95 / 62 / 61 / 67 / 89 / 280 / 1117
//  4096 -> 28672  71 / 111 / 131 / 229 / 439 / 1800 / 8363  |  115 / 136 / 138 / 224 / 399 / 1339 / 5160
//  14336 -> 4096  157 / 161 / 161 / 163 / 231 / 914 / 5399  |  215 / 176 / 173 / 178 / 231 / 644 / 2544
//  768 -> 50257   50 / 73 / 97 / 169 / 309 / 1129 / 4716  |  62 / 102 / 103 / 185 / 318 / 1180 / 4718
// At 129 rows the tile kernel is 1.0-2.2 x as fast, except on the two deep
// narrow projections (3072 -> 768, 6400 -> 1600: 6 and 13 column blocks, 2.0
// and 1.5 x slower; in decode those are dnn_gemm_w4_mn's).  At 384..1024 rows
// it is level or faster on every shape (1.0-1.5 x) but for two cases 2-3 %
// slower (3072 -> 768 at 384 rows, gate|up at 1024).  Above that the tuned
// 256 x 256 bf16 tiles win once the expansion is amortised: at 2048 rows the
// wide shapes run at 0.76-0.91 x (the GPT-2 small shapes, 6400 -> 1600, down
// and the head are level or faster), at 8192 rows 0.69-1.0 x, at 32768 rows
// 0.47-0.72 x, where this kernel reaches 710-920 TFLOP/s (the head, bound by
// its 3.3 GB of logits: level from 8192 rows, faster below).  The mode is
// opt-in and routes by step kind, not by a fitted predicate, so these losses
// are its documented price for holding no scratch; levers not tried: 256-row
// blocks, a deeper ring at one workgroup per CU, the norm forms at two
// workgroups per CU.
#pragma once
#include "gemm_epilogue.h"

namespace dnn {

constexpr int W4T_BM = 128;    // rows per workgroup: 2 waves x 4 M tiles
constexpr int W4T_BN = 128;    // columns per workgroup: 2 waves x 4 column tiles
constexpr int W4T_MT = 4;      // M tiles per wave
constexpr int W4T_NT = 4;      // column tiles per wave
constexpr int W4T_U = 2;       // weight chunks in flight per wave and tile
constexpr int W4T_ROW = 256;   // LDS bytes per row and stage: one 128-k chunk of bf16
constexpr int W4T_STAGE = W4T_BM * W4T_ROW;
constexpr int W4T_LDS = 2 * W4T_STAGE + W4T_BM * 8;  // two stages, then float2 [128] statistics

template <int ACT, int NORM>
__global__ __launch_bounds__(256, NORM == W4_NORM_NONE ? 2 : 1) void gemm_w4_tile_kernel(
    const uint8_t* __restrict__ A, int lda_b, const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ Ws,
    bf16_t* __restrict__ C, int ldc, const float* __restrict__ bias, const bf16_t* __restrict__ R, int ldr, int M,
    int N, int K, const float* __restrict__ colsum, float eps) {
  extern __shared__ __attribute__((aligned(16))) uint8_t w4t_lds[];
  constexpr int SI = W4T_BM / 16;  // staging passes: rows 16 i + sr
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, r = lane & 15;
  const int m0 = (int)blockIdx.x * W4T_BM;              // < M: the grid has ceil(M / 128) row blocks
  const int mtb = (min(W4T_BM, M - m0) + 15) >> 4;      // M tiles of this block in use (1..8)
  const int mtw = max(0, min(W4T_MT, mtb - wm * W4T_MT));  // of this wave (0..4)
  const int nch = (K + 127) >> 7;  // 128-k chunks (the last may be partial)
  const int kg = K >> 5;           // valid 32-k groups
  const int ntile = (N + 15) >> 4;
  float2* w4t_st = reinterpret_cast<float2*>(w4t_lds + 2 * W4T_STAGE);

  // this wave's column tiles (a tile past N repeats the last real one and stores nothing)
  const int ct0 = (int)blockIdx.y * (W4T_BN / 16) + wn * W4T_NT;
  // (uniform block indices: the addresses are a scalar base plus the lane's 32-bit offset)
  size_t wblk[W4T_NT];
#pragma unroll
  for (int j = 0; j < W4T_NT; ++j) wblk[j] = (size_t)min(ct0 + j, ntile - 1) * nch;  // + chunk: the 1 KiB block
  const uint32_t lane16 = (uint32_t)lane * 16u, lane1 = (uint32_t)lane;
  auto w_load = [&](int j, int ci, i32x4& w, uint32_t& e) {
    const size_t blk = wblk[j] + ci;
    w = *reinterpret_cast<const i32x4*>(Wq + blk * 1024 + lane16);
    e = Ws[blk * 64 + lane1];
  };

  // staging role: slot sj of the block's rows 16 i + sr
  const int sj = tid & 15, sr = tid >> 4;
  const int lds_w = sr * W4T_ROW + ((sj ^ sr) << 4);  // + i * 16 rows, + stage
  float st1[SI], st2[SI], shift[SI];
#pragma unroll
  for (int i = 0; i < SI; ++i) {
    st1[i] = st2[i] = 0.f;
    shift[i] = 0.f;
    if constexpr (NORM == W4_NORM_LN) {
      if (i < mtb)
        shift[i] = __uint_as_float(
            (uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(m0 + 16 * i + sr, M - 1) * lda_b)) << 16);
    }
  }
  i32x4 areg[SI];
  // request chunk c of A (a group at or past K reads the chunk's first group)
  auto a_load = [&](int c) {
    const bool ok = c * 4 + (sj >> 2) < kg;
    const int so = c * W4T_ROW + (ok ? sj : (sj & 3)) * 16;
#pragma unroll
    for (int i = 0; i < SI; ++i)
      if (i < mtb)
        areg[i] = *reinterpret_cast<const i32x4*>(A + (size_t)min(m0 + 16 * i + sr, M - 1) * lda_b + so);
  };
  // statistics of the chunk in areg, then its ds_write_b128 into stage s
  auto a_store = [&](int c, int s) {
    const bool ok = c * 4 + (sj >> 2) < kg;
    uint8_t* dst = w4t_lds + s * W4T_STAGE + lds_w;
#pragma unroll
    for (int i = 0; i < SI; ++i)
      if (i < mtb) {
        if (!ok) areg[i] = i32x4{0, 0, 0, 0};
        if constexpr (NORM != W4_NORM_NONE) {
          if (ok) w4_stats<NORM>(areg[i], shift[i], st1[i], st2[i]);
        }
        *reinterpret_cast<i32x4*>(dst + i * 16 * W4T_ROW) = areg[i];
      }
  };

  f32x4 acc[W4T_NT][W4T_MT];
#pragma unroll
  for (int j = 0; j < W4T_NT; ++j)
#pragma unroll
    for (int t = 0; t < W4T_MT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the first U weight chunks and A chunk 0
  i32x4 wv[W4T_U][W4T_NT];
  uint32_t sc[W4T_U][W4T_NT];
#pragma unroll
  for (int u = 0; u < W4T_U; ++u) {
    const int ci = min(u, nch - 1);
#pragma unroll
    for (int j = 0; j < W4T_NT; ++j) w_load(j, ci, wv[u][j], sc[u][j]);
  }
  a_load(0);
  a_store(0, 0);
  __syncthreads();

  // fragment reads: row 16 (4 wm + t) + r of the block, slot (4 g + h) ^ r
  const int lds_r = (wm * W4T_MT * 16 + r) * W4T_ROW;
#pragma unroll 1
  for (int cb = 0; cb < nch; cb += W4T_U) {
#pragma unroll
    for (int u = 0; u < W4T_U; ++u) {
      const int c = cb + u;
      if (c < nch) {  // uniform over the workgroup
        const bool more = c + 1 < nch;
        if (more) a_load(c + 1);  // in flight under this chunk's MFMAs
        const uint8_t* src = w4t_lds + (c & 1) * W4T_STAGE + lds_r;
        bf16x8 ab[W4T_MT][4];  // the chunk's 16 A fragments, shared by the four column tiles
#pragma unroll
        for (int t = 0; t < W4T_MT; ++t)
          if (t < mtw) {  // wave-uniform
#pragma unroll
            for (int h = 0; h < 4; ++h)
              ab[t][h] = *reinterpret_cast<const bf16x8*>(src + t * 16 * W4T_ROW + (((4 * g + h) ^ r) << 4));
          }
        const int ci = min(c + W4T_U, nch - 1);  // the ring's next chunk (a surplus load repeats the last chunk)
#pragma unroll
        for (int j = 0; j < W4T_NT; ++j) {
          bf16x8 wb[4];
          w4_to_bf16(wv[u][j], __uint_as_float(sc[u][j] << 23), wb);
          w_load(j, ci, wv[u][j], sc[u][j]);
#pragma unroll
          for (int t = 0; t < W4T_MT; ++t)
            if (t < mtw) {
#pragma unroll
              for (int h = 0; h < 4; ++h)
                acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[h], ab[t][h], acc[j][t], 0, 0, 0);
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
    for (int i = 0; i < SI; ++i)
      if (i < mtb) {
        float a = st1[i], s = st2[i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          a += __shfl_xor(a, o, 64);
          s += __shfl_xor(s, o, 64);
        }
        if (sj == 0) w4t_st[16 * i + sr] = make_float2(a, s);
      }
    __syncthreads();
  }

  const int NO = ACT == ACT_SILU_MUL ? N / 2 : N;
  const bool vec = epi_vec_ok(C, ldc, bias, R, ldr);
#pragma unroll
  for (int t = 0; t < W4T_MT; ++t) {
    if (t >= mtw) continue;  // wave-uniform
    const int ml = (wm * W4T_MT + t) * 16 + r;  // row of the block
    const int m = m0 + ml;
    float mean = 0.f, rstd = 1.f;
    if constexpr (NORM != W4_NORM_NONE) {
      const float2 st = w4t_st[ml];
      const float invk = 1.f / (float)K;
      const float d = st.x * invk;  // E[x - c]
      if constexpr (NORM == W4_NORM_LN)
        mean = d + __uint_as_float((uint32_t)(*reinterpret_cast<const uint16_t*>(A + (size_t)min(m, M - 1) * lda_b))
                                   << 16);
      const float var = NORM == W4_NORM_LN ? fmaxf(st.y * invk - d * d, 0.f) : st.y * invk;
      rstd = rsqrtf(var + eps);
    }
#pragma unroll
    for (int j = 0; j < W4T_NT; ++j) {
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
