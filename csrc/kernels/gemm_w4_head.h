// MXFP4 vocabulary head with the greedy argmax's first pass (W4A16), included
// by gemm_w4.hip (which states the weight's fragment order and holds
// w4_to_bf16 / w4_stats):
//
//   logits[m, n] = bf16( rstd[m] (A[m,:] . dq(W')[n,:] - mean[m] colsum[n]) + bias[n] ),   1 <= M <= 64
//   part[m, wg]  = argmax over the workgroup's columns of the rounded logits[m, :]   (part != nullptr)
//
// (ln_f folded into W' on the host, ops/gemm.py fold_norm(quant="mxfp4").)  A
// head is 2 to 4.5 times as wide as the widest layer projection: dnn_gemm_w4
// (one column tile per workgroup, every workgroup re-reading all M rows from
// L2) is bound by activation traffic there, and gemm_head.h, whose design this
// follows, knows neither the MXFP4 fragment order nor the block scales.
//   * grid = min(CUs, ceil(tiles / 8)) persistent workgroups of 8 waves.
//     Workgroup b owns the contiguous tiles [b T / grid, (b + 1) T / grid)
//     (equal bytes to one tile), taken in rounds of 16: in round i wave w has
//     tiles first + 16 i + w and + 8 more (NT = 2).  No K split over waves or
//     workgroups and no atomics: a column's sum is the chunks in ascending k
//     inside one wave's MFMA accumulators, the same bits on every launch.
//   * A: the mt = ceil(M / 16) M tiles of a K pass are staged once per
//     workgroup: thread (tid >> 4, tid & 15) loads 16-byte slot tid & 15 of a
//     (row, chunk) unit (16 consecutive lanes: the 256 contiguous bytes of one
//     row's chunk), four units in flight, and writes it with ds_write_b128.
//     Rows past M - 1 clamp; a 32-k group at or past K is not read (the address
//     falls back to the chunk's first group), its slots are zeroed and left
//     out of the statistics.
//   * weights: a wave streams its two tiles' chunks of the pass (1 KiB of codes
//     and 64 scale bytes per tile and 128 k) straight to VGPRs by non-temporal
//     16-byte loads in stored order, U = 4 chunks x 2 tiles in flight as a ring
//     (chunk c + 4 is requested as soon as chunk c is converted; the first four
//     are requested ahead of the staging, so they land under it): 8 KiB per
//     wave, 64 KiB per CU.  v_cvt_scalef32_pk_bf16_fp4 is exact, and the
//     bf16 16x16x32 MFMA takes the weight as first operand (transposed
//     accumulators: lane 16 g + r holds row 16 t + r, columns 4 g .. 4 g + 3).
//     One A fragment read feeds both tiles' MFMAs.
//   * statistics: from the image, wave w rows 8 w .. 8 w + 7, 8 lanes per row,
//     the shifted form of w4_stats, once per workgroup (round 0 only).
//   * epilogue per tile: folded norm, fp32 bias, bf16 round, 8-byte stores
//     (always aligned: C is 16-byte aligned, ldc % 8 == 0), and with part the
//     running argmax of the ROUNDED values per row (ties -> smallest column);
//     columns at or past N are neither stored nor compared.  The 8 waves'
//     winners meet in LDS and the workgroup writes one {value bits, index} per
//     row at part[row * grid + wg]: dnn_gemm_head's format, merged by the
//     unchanged dnn_argmax_final.  part == nullptr: logits only.
//
// LDS image and passes.  Row pitch = cpp x 256 B (cpp = chunks per pass), 16-byte
// slot j of row r stored at slot j ^ (r & 15), inside its 256-byte group.  The
// pitch is a multiple of 256 B = 64 banks, so the bank pattern is that of
// gemm_w4_mid.h: a fragment ds_read_b128 (lane 16 g + r: slot 16 c + 4 g + h
// of row 16 t + r) puts the 16 lanes of each lane group on 16 distinct slots,
// a staging ds_write_b128 puts 16 consecutive lanes on the 16 slots of one
// row's chunk.  Checked exhaustively on the host (64 banks of 4 bytes, 16 lanes
// per pass; every cpp 1..36, t < 4, h < 4, lane group, chunk, and every
// staging write of 64 rows): 0 conflicts in 42624 fragment read passes and
// 42624 staging write passes; without the xor every read pass is a 16-way
// conflict.  The statistics reads (once per workgroup) put the two rows of a
// 16-lane pass on the two halves of a 256-byte group (slot ^ 8 for odd rows):
// 0 conflicts in 42624 passes as well.
// The image takes 36 blocks of 4 KiB (16 rows x 128 k) = 144 KiB of the CU's
// 160 KiB (4.5 KiB more hold the statistics and the argmax exchange), so
// cpp = min(chunks, 36 / mt): 36 / 18 / 12 / 9 chunks = 4608 / 2304 / 1536 /
// 1152 k at up to 16 / 32 / 48 / 64 rows.  K = 768 is one image at every M;
// K = 1600 (200 KiB at 64 rows) is one image up to 32 rows and two passes
// above; K = 4096 is one image up to 16 rows and 2 / 3 / 4 passes above.  With
// passes the image is restaged between them (and again for the next round) and
// the accumulators stay in registers.
//
// Choices:
//   * NT = 2 tiles per wave, 16 per round: GPT-2's 3142 tiles on 256 CUs are
//     12-13 per workgroup (one round, every wave busy on 1-2 tiles); Llama-3's
//     8016 are 31-32 (two rounds).  NT = 4 would make that one round but leave
//     GPT-2's waves one tile in four and its ring a quarter full.  A fragment
//     read (the LDS bandwidth: 16 ds_read_b128 per chunk at 64 rows) is shared
//     by the two tiles.
//   * U = 4: with NT = 2 the ring is 40 VGPRs; at K = 768 a tile's pass is 6
//     chunks, so a wave has two thirds of its bytes requested before its first
//     MFMA.  No surplus loads: a ring slot past the pass's last chunk is left
//     empty (wave-uniform), a tile past the workgroup's range is skipped whole.
//   * M is not a template parameter: M tiles at or past mt are skipped on a
//     wave-uniform condition.
//   * registers (-Rpass-analysis=kernel-resource-usage, gfx950): 185 (no norm)
//     / 194 (RMS) / 197 (LayerNorm) VGPRs, no AGPRs, two waves per SIMD; no
//     instantiation uses scratch.
// Measured (bench/probes/w4_head_ab.py, profiles/w4_head_ab.jsonl, us per greedy
// head step at M = 1 / 32 / 64 against the bf16 head in the same process):
// 768 -> 50257 15.6 / 19.8 / 26.8 against 23.6 / 25.6 / 27.0; 1600 -> 50257
// 22.1 / 28.1 / 40.8 against 40.5 / 41.9 / 44.3; 4096 -> 128256 61.4 / 93.5 /
// 149.7 against 158.1 / 187.5 / 216.1.  At 64 rows the e4m3 head is faster on
// the GPT-2 shapes (22.7 / 36.3 us): there the bound is the fragment reads and
// MFMAs per chunk (16 each per tile), not the weight stream (0.8-1.9 TB/s).
#pragma once
#include "gemm_epilogue.h"

namespace dnn {

constexpr int W4H_WAVES = 8;  // waves per workgroup
constexpr int W4H_NT = 2;     // column tiles per wave and round
constexpr int W4H_U = 4;      // weight chunks in flight per wave and tile
constexpr int W4H_IMG = 36;   // LDS image budget in 4 KiB blocks (16 rows x one 128-k chunk)
constexpr int W4H_TAIL = (2 * 64 + 2 * W4H_WAVES * 64) * 4;  // statistics + argmax exchange after the image

__device__ __forceinline__ void w4h_amax(float& best, int& bi, float v, int i) {
  if (v > best || (v == best && i < bi)) {
    best = v;
    bi = i;
  }
}

template <int NORM>
__global__ __launch_bounds__(64 * W4H_WAVES, 1) void gemm_w4_head_kernel(
    const uint8_t* __restrict__ A, int lda_b, const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ Ws,
    bf16_t* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ colsum, float eps,
    int M, int N, int K, int2* __restrict__ part) {
  constexpr int NT = W4H_NT, U = W4H_U;
  extern __shared__ __attribute__((aligned(16))) uint8_t w4h_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int mt = (M + 15) >> 4, R = mt * 16;  // M tiles and image rows in use
  const int nch = (K + 127) >> 7;             // 128-k chunks (the last may be partial)
  const int kg = K >> 5;                      // valid 32-k groups
  const int cpp = min(nch, W4H_IMG / mt);     // chunks per pass
  const int npass = (nch + cpp - 1) / cpp;
  const int RP = cpp * 256;                   // image row pitch in bytes
  float* st_mean = reinterpret_cast<float*>(w4h_lds + R * RP);
  float* st_rstd = st_mean + 64;
  float* xbest = st_rstd + 64;                                  // [8 waves][64 rows]
  int* xidx = reinterpret_cast<int*>(xbest + W4H_WAVES * 64);  // [8 waves][64 rows]

  const int ntile = (N + 15) >> 4;
  const int wt0 = (int)((long long)blockIdx.x * ntile / gridDim.x);
  const int wt1 = (int)((long long)(blockIdx.x + 1) * ntile / gridDim.x);
  const int nround = (wt1 - wt0 + W4H_WAVES * NT - 1) / (W4H_WAVES * NT);

  // statistics role: row 8 wave + (lane >> 3), its 16-byte slots lane & 7, + 8, ... (odd rows: slot ^ 8)
  const int srow = 8 * wave + (lane >> 3), ssub = (lane & 7) ^ ((lane & 8));
  float shift = 0.f, s1 = 0.f, s2 = 0.f;

  float best[4];
  int bi[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    best[t] = -INFINITY;
    bi[t] = 0x7fffffff;
  }

  const int lds_r = r * RP;  // fragment reads: + 16 t rows, slot (16 c + 4 g + h) ^ r
#pragma unroll 1
  for (int rnd = 0; rnd < nround; ++rnd) {
    int tl[NT];
    bool has[NT];
    const uint8_t* wp[NT];
    const uint8_t* sp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      tl[j] = wt0 + (rnd * NT + j) * W4H_WAVES + wave;
      has[j] = tl[j] < wt1;  // wave-uniform
      const int ct = min(tl[j], wt1 - 1);
      wp[j] = Wq + ((size_t)ct * nch * 64 + lane) * 16;  // + chunk * 1024
      sp[j] = Ws + (size_t)ct * nch * 64 + lane;         // + chunk * 64
    }
    f32x4 acc[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int p = 0; p < npass; ++p) {
      const int pc0 = p * cpp, pc1 = min(nch, pc0 + cpp), npc = pc1 - pc0;
      // the ring's first U chunks, ahead of the staging
      i32x4 wv[U][NT];
      uint32_t sc[U][NT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          wv[u][j] = i32x4{0, 0, 0, 0};
          sc[u][j] = 127;
          if (has[j] && pc0 + u < pc1) {
            wv[u][j] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[j] + (size_t)(pc0 + u) * 1024));
            sc[u][j] = sp[j][(size_t)(pc0 + u) * 64];
          }
        }
      if (npass > 1 || rnd == 0) {
        if (rnd + p > 0) __syncthreads();  // every wave is done reading the previous image
        const int sj = tid & 15, units = npc * R;
#pragma unroll 1
        for (int u0 = tid >> 4; u0 < units; u0 += 32 * 4) {
          i32x4 v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int u = u0 + 32 * i;
            if (u < units) {
              const int c = u / R, rr = u - c * R;
              const bool ok = (pc0 + c) * 4 + (sj >> 2) < kg;
              v[i] = *reinterpret_cast<const i32x4*>(A + (size_t)min(rr, M - 1) * lda_b + (size_t)(pc0 + c) * 256 +
                                                     (ok ? sj : (sj & 3)) * 16);
            }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int u = u0 + 32 * i;
            if (u < units) {
              const int c = u / R, rr = u - c * R;
              if ((pc0 + c) * 4 + (sj >> 2) >= kg) v[i] = i32x4{0, 0, 0, 0};
              *reinterpret_cast<i32x4*>(w4h_lds + rr * RP + c * 256 + ((sj ^ (rr & 15)) << 4)) = v[i];
            }
          }
        }
        __syncthreads();
      }

      if constexpr (NORM != W4_NORM_NONE) {
        if (rnd == 0 && srow < R) {
          const uint8_t* rp = w4h_lds + srow * RP;
          if constexpr (NORM == W4_NORM_LN) {
            if (p == 0) shift = bf2f(*reinterpret_cast<const bf16_t*>(rp + ((srow & 15) << 4)));  // element 0
          }
          for (int sl = ssub; sl < npc * 16; sl += 16) {
#pragma unroll
            for (int o = 0; o < 16; o += 8) {
              const int ps = sl ^ o;                                   // stored slot
              const int k16 = pc0 * 16 + (ps ^ (srow & 15));           // the 16-byte piece of the row it holds
              if ((k16 >> 2) < kg) w4_stats<NORM>(*reinterpret_cast<const i32x4*>(rp + ps * 16), shift, s1, s2);
            }
          }
        }
      }

      if (has[0]) {
#pragma unroll 1
        for (int cb = pc0; cb < pc1; cb += U) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int c = cb + u;
            if (c < pc1) {  // wave-uniform
              bf16x8 wb[NT][4];
#pragma unroll
              for (int j = 0; j < NT; ++j) w4_to_bf16(wv[u][j], __uint_as_float(sc[u][j] << 23), wb[j]);
              if (c + U < pc1) {  // the ring: chunk c + U into the registers chunk c has left
#pragma unroll
                for (int j = 0; j < NT; ++j)
                  if (has[j]) {
                    wv[u][j] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(wp[j] + (size_t)(c + U) * 1024));
                    sc[u][j] = sp[j][(size_t)(c + U) * 64];
                  }
              }
              const uint8_t* src = w4h_lds + lds_r + (c - pc0) * 256;
#pragma unroll
              for (int t = 0; t < 4; ++t)
                if (t < mt) {  // wave-uniform
#pragma unroll
                  for (int h = 0; h < 4; ++h) {
                    const bf16x8 ab = *reinterpret_cast<const bf16x8*>(src + t * 16 * RP + (((4 * g + h) ^ r) << 4));
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[0][h], ab, acc[0][t], 0, 0, 0);
                    if (has[1]) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[1][h], ab, acc[1][t], 0, 0, 0);
                  }
                }
            }
          }
        }
      }
    }

    if constexpr (NORM != W4_NORM_NONE) {
      if (rnd == 0) {
        // the 8 lanes of a row hold disjoint k
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
          s1 += __shfl_xor(s1, o, 64);
          s2 += __shfl_xor(s2, o, 64);
        }
        if ((lane & 7) == 0 && srow < R) {
          const float invk = 1.f / (float)K, d = s1 * invk;  // E[x - c]
          const float var = NORM == W4_NORM_LN ? fmaxf(s2 * invk - d * d, 0.f) : s2 * invk;
          st_mean[srow] = NORM == W4_NORM_LN ? shift + d : 0.f;
          st_rstd[srow] = rsqrtf(var + eps);
        }
        __syncthreads();
      }
    }

    // epilogue per tile (lane: row 16 t + r, columns n0 .. n0 + 3) + running argmax of the rounded values
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (!has[j]) continue;  // wave-uniform
      const int n0 = tl[j] * 16 + g * 4;
      float cs[4], bs[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = n0 + i < N;
        cs[i] = (NORM == W4_NORM_LN && ok) ? colsum[n0 + i] : 0.f;
        bs[i] = (bias != nullptr && ok) ? bias[n0 + i] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int m = 16 * t + r;
        if (t >= mt || m >= M) continue;
        float mean = 0.f, rstd = 1.f;
        if constexpr (NORM != W4_NORM_NONE) {
          mean = st_mean[m];
          rstd = st_rstd[m];
        }
        bf16_t b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = acc[j][t][i];
          if constexpr (NORM == W4_NORM_LN) v = rstd * (v - mean * cs[i]);
          if constexpr (NORM == W4_NORM_RMS) v *= rstd;
          b[i] = f2bf(v + bs[i]);
        }
        bf16_t* cp = C + (size_t)m * ldc + n0;
        if (n0 + 3 < N) {
          *reinterpret_cast<uint2*>(cp) =
              make_uint2((uint32_t)b[0] | (uint32_t)b[1] << 16, (uint32_t)b[2] | (uint32_t)b[3] << 16);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n0 + i < N) cp[i] = b[i];
        }
        if (part != nullptr) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n0 + i < N) w4h_amax(best[t], bi[t], bf2f(b[i]), n0 + i);
        }
      }
    }
  }

  if (part == nullptr) return;  // uniform over the grid
  // winners: the 4 lane groups, then the 8 waves, then one partial per row
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float ov = __shfl_xor(best[t], o, 64);
      const int oi = __shfl_xor(bi[t], o, 64);
      w4h_amax(best[t], bi[t], ov, oi);
    }
    if (lane < 16) {
      xbest[wave * 64 + 16 * t + lane] = best[t];
      xidx[wave * 64 + 16 * t + lane] = bi[t];
    }
  }
  __syncthreads();
  if (tid < M) {
    float b = xbest[tid];
    int i = xidx[tid];
#pragma unroll
    for (int w = 1; w < W4H_WAVES; ++w) w4h_amax(b, i, xbest[w * 64 + tid], xidx[w * 64 + tid]);
    part[(size_t)tid * gridDim.x + blockIdx.x] = make_int2(__float_as_int(b), i);
  }
}

}  // namespace dnn
