// Prompt log-probabilities: the vocabulary head GEMM with the softmax reduction
// in its epilogue, so that no (rows x vocabulary) logits tensor exists.  For
// hidden rows A (M, d) bf16, the folded head weight W (V, d) bf16 row-major
// (FoldedLinear.w, the tensor linear_norm reads) and a target column per row:
//   l[m, v]  = bf16_rne(fold(a_m . w_v))       the unfused head's stored logit:
//              fold(x) = fma(shift_m, colsum[v], rstd_m x) + bias[v] with rowstat
//              = {rstd, shift = -mean rstd} as row_stats_kernel writes it
//              (gemm_epilogue.h epi_norm4 + epi_t4, same operations, same order)
//   lse[m]   = log sum_v exp(l[m, v])           fp32
//   tok_lp   = l[m, target[m]] - lse,  top_id = argmax_v l (value descending,
//              index ascending on the bf16 order key, as logprobs.hip),
//   top_lp   = l[m, top_id] - lse
// Two plain launches, a fixed split and a fixed merge order: no atomics, no
// workgroup waits for another, so a result is the same bits on every launch.
//
// Launch 1 (head_lse_kernel).  Grid = ceil(M / 128) row blocks (x) x NS
// vocabulary slices (y).  NS depends on (M, V) alone (hl_plan: about two
// workgroups per CU of a 256-CU chip while M is small, 2 at 32768 rows), never
// on the device, so the split and with it every rounding is the same on every
// box.  A workgroup of 4 waves walks the 128-column tiles of its slice one
// after another; per tile it runs the K loop in steps of 64:
//   * A (128 rows x 64 k) and W (128 columns x 64 k) go through LDS, two
//     stages of 32 KiB: step s + 1 is requested from memory before step s's
//     MFMAs and written to LDS after them, one barrier per step, and the ring
//     runs on across tile boundaries.  Thread (sr = tid >> 3, sj = tid & 7)
//     stages the 16-byte slot sj of rows sr + 32 i, i < 4, of both operands;
//     slot j of row r sits at slot j ^ ((r >> 1) & 7) of its 128-byte row, so
//     the 16 lanes of a ds_write_b128 / ds_read_b128 group hit 16 different
//     16-byte units of a 256-byte bank line.  A is re-read once per tile: a
//     block's rows (128 x d bf16, 192 KiB at d = 768) stay in L2;
//   * wave w owns rows 32 w .. 32 w + 31 of the block against all 128 columns
//     of the tile: 2 M tiles x 8 column tiles of v_mfma_f32_16x16x32_bf16, 64
//     accumulator registers.  The tile is 128 and not 256 columns wide so that
//     accumulators, staging registers and the running state stay under 256
//     VGPRs and two workgroups (2 x 64 KiB of LDS) share a CU.  The waves split
//     rows, not columns: a row's whole tile lives in one wave, so its
//     reduction needs no LDS exchange at all;
//   * W is the MFMA's first operand (transposed accumulators): lane 16 g + r
//     holds row r of the M tile and columns 16 j + 4 g + i.  A row's 128
//     logits of the tile are 32 values in each of 4 lanes (r, g = 0..3), which
//     meet by two xor shuffles (16, 32);
//   * the tile's epilogue folds, rounds to bf16 and updates the row's running
//     state, held in registers across the tiles (the flash-attention
//     recurrence over the vocabulary): the largest order key with its column,
//     sum exp(l - max), rescaled when the max moves, and the target's logit.
// At the end of its slice the workgroup leaves one 16-byte partial per row in
// the workspace (M, NS, 4 words): max, sum, argmax column, target logit bits
// (HL_NONE when the target column is not in the slice).
//
// Launch 2 (head_lse_finish_kernel): a wave per row.  Lane k folds partials
// k, k + 64, .. in slice order, the lanes meet in one fixed butterfly; lane 0
// writes tok_lp / top_id / top_lp at out_idx[row] (the (B, L) histories are
// scattered into directly), or nothing when target[row] is -1 or outside
// [0, V), or out_idx[row] is outside [0, out_len).
//
// Edges: rows past M - 1 and columns past V - 1 clamp on load (the last real
// row / column is read again) and are left out of every reduction and store; M
// tiles past the block's rows are neither staged nor multiplied.  d must be a
// multiple of 64 (768, 1600, 4096 are).
// Registers (-Rpass-analysis=kernel-resource-usage, gfx950): 203 VGPRs, no AGPRs, no scratch: two waves per SIMD.
// Measured against linear_norm to all-position logits (chunks of at most 8192 rows) + logprobs_rows n = 1
// (bench/probes/prompt_logprobs_ab.py, profiles/prompt_logprobs_ab.jsonl: one process, arms in turn, medians of
// 5 rounds, min-max spread under 7 %), us per call at 2048 / 8192 / 32768 rows, fused | unfused:
//   768 -> 50257     379 / 1312 / 5182     |  353 / 1314 / 5240     extra memory 1.1-1.6 MB | 0.2-0.8 GB
//   4096 -> 128256  3506 / 13588 / 60539   | 1899 / 7572 / 30640    extra memory 1.1-1.6 MB | 0.5-2.2 GB
// Level on the GPT-2 head; on the Llama-3 head the GEMM dominates and these 128 x 128 tiles (about 570 TFLOP/s)
// lose 1.8-2.0 x to the tuned 256 x 256 bf16 tiles.  Levers not tried: 256-row blocks at one workgroup per CU,
// W fragments streamed to registers as gemm_w4_tile.h does.
// Built with -ffp-contract=off (ops/build.py): the only fused multiply-add of
// the fold is the one written out, and (l - max) - lse stays two subtractions.
#include "common.h"
#include "sampler_common.h"

namespace dnn {

constexpr int HL_BM = 128;            // rows per workgroup: 4 waves x 2 M tiles
constexpr int HL_BN = 128;            // columns per tile: 8 column tiles per wave
constexpr int HL_KS = 64;             // k per step: two MFMA k-steps of 32
constexpr int HL_ROWB = HL_KS * 2;    // LDS bytes per row and step
constexpr int HL_OP = HL_BM * HL_ROWB;  // one operand's tile of one step: 16 KiB
constexpr int HL_STAGE = 2 * HL_OP;   // A then W
constexpr int HL_LDS = 2 * HL_STAGE;  // two stages
constexpr int HL_TARGET_WG = 512;     // workgroups hl_plan aims at while M is small
constexpr int HL_MAX_NS = 512;
constexpr uint32_t HL_NONE = 0xFFFFFFFFu;  // no target logit (a bf16 widened to 32 bits has a zero low half)
constexpr float HL_LOG2E = 1.44269504088896341f;

// exp(x) for x <= 0 as one v_exp_f32; exp(-inf) = 0, exp(0) = 1 exactly
__device__ __forceinline__ float hl_exp(float x) { return __builtin_amdgcn_exp2f(x * HL_LOG2E); }

__global__ __launch_bounds__(256, 2) void head_lse_kernel(
    const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ W, int ldw, const float2* __restrict__ rowstat,
    const float* __restrict__ colsum, const float* __restrict__ bias, const int* __restrict__ target, int M, int V,
    int d, int tps, int NS, uint4* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint8_t hl_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, r = lane & 15;
  const int m0 = (int)blockIdx.x * HL_BM;  // < M
  const int slice = (int)blockIdx.y;
  const int ntile = (V + HL_BN - 1) / HL_BN;
  const int t0 = slice * tps;
  const int ntl = min(tps, ntile - t0);  // >= 1: hl_plan leaves no slice empty
  const int nk = d / HL_KS;
  const int rows = min(HL_BM, M - m0);
  const int mtw = max(0, min(2, (rows - wave * 32 + 15) >> 4));  // M tiles of this wave in use
  const int ngrp = (rows + 31) >> 5;                             // 32-row staging groups in use
  const float ninf = -__builtin_inff();

  // staging role: slot sj of rows sr + 32 i of both operands
  const int sr = tid >> 3, sj = tid & 7;
  const int lds_w = sr * HL_ROWB + ((sj ^ ((sr >> 1) & 7)) << 4);  // + i * 32 rows, + operand, + stage
  i32x4 areg[4], wreg[4];
  auto g_load = [&](int tile, int kk) {
    const int k0 = kk * HL_KS + sj * 8;
    const int n0 = (t0 + tile) * HL_BN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < ngrp)
        areg[i] = *reinterpret_cast<const i32x4*>(A + (size_t)min(m0 + 32 * i + sr, M - 1) * lda + k0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      wreg[i] = *reinterpret_cast<const i32x4*>(W + (size_t)min(n0 + 32 * i + sr, V - 1) * ldw + k0);
  };
  auto l_store = [&](int s) {
    uint8_t* dst = hl_lds + s * HL_STAGE + lds_w;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < ngrp) *reinterpret_cast<i32x4*>(dst + i * 32 * HL_ROWB) = areg[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<i32x4*>(dst + HL_OP + i * 32 * HL_ROWB) = wreg[i];
  };

  // fragment reads: lane (g, r) takes k = 32 h + 8 g .. + 7 (slot 4 h + g) of row r of a 16-row tile
  const int swz = (r >> 1) & 7;
  const int a_rd = (wave * 32 + r) * HL_ROWB;  // + t * 16 rows
  const int w_rd = HL_OP + r * HL_ROWB;        // + j * 16 rows

  f32x4 acc[8][2];
  uint32_t rkey[2] = {0u, 0u};  // order key + 1 of the running max (0: none yet)
  int rid[2] = {0, 0};
  float rsum[2] = {0.f, 0.f};
  uint32_t rtgt[2] = {HL_NONE, HL_NONE};

  g_load(0, 0);
  l_store(0);
  __syncthreads();

  int tile = 0, kk = 0;
  const int nstep = ntl * nk;
#pragma unroll 1
  for (int s = 0; s < nstep; ++s) {
    const bool more = s + 1 < nstep;
    const bool last_k = kk + 1 == nk;
    if (more) g_load(last_k ? tile + 1 : tile, last_k ? 0 : kk + 1);  // in flight under this step's MFMAs
    if (kk == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (mtw > 0) {  // wave-uniform
      const uint8_t* base = hl_lds + (s & 1) * HL_STAGE;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int so = ((4 * h + g) ^ swz) << 4;
        bf16x8 af[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (t < mtw) af[t] = *reinterpret_cast<const bf16x8*>(base + a_rd + t * 16 * HL_ROWB + so);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bf16x8 wf = *reinterpret_cast<const bf16x8*>(base + w_rd + j * 16 * HL_ROWB + so);
#pragma unroll
          for (int t = 0; t < 2; ++t)
            if (t < mtw) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af[t], acc[j][t], 0, 0, 0);
        }
      }
    }

    if (last_k && mtw > 0) {
      // ---- the tile's epilogue: fold, round, update the rows' running state
      const int n0 = (t0 + tile) * HL_BN;
      float2 st[2];
      int tg[2];
      uint32_t best[2] = {0u, 0u};  // (key + 1) << 8 | (127 - column of the tile): unique per column
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int mc = min(m0 + wave * 32 + t * 16 + r, M - 1);
        st[t] = rowstat != nullptr ? rowstat[mc] : make_float2(1.f, 0.f);
        tg[t] = target[mc];
        if (tg[t] < 0 || tg[t] >= V) tg[t] = -1;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cl = j * 16 + 4 * g, nb = n0 + cl;
        f32x4 cs = f32x4{0.f, 0.f, 0.f, 0.f}, bs = f32x4{0.f, 0.f, 0.f, 0.f};
        if (nb + 3 < V) {
          if (colsum != nullptr) cs = *reinterpret_cast<const f32x4*>(colsum + nb);
          if (bias != nullptr) bs = *reinterpret_cast<const f32x4*>(bias + nb);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (colsum != nullptr && nb + i < V) cs[i] = colsum[nb + i];
            if (bias != nullptr && nb + i < V) bs[i] = bias[nb + i];
          }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t >= mtw) continue;  // wave-uniform
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = acc[j][t][i];
            if (rowstat != nullptr) {
              v = v * st[t].x;
              if (colsum != nullptr) v = __fmaf_rn(st[t].y, cs[i], v);
            }
            if (bias != nullptr) v = v + bs[i];
            const bf16_t b = f2bf(v);
            const bool ok = nb + i < V;
            const uint32_t c = ((bf16_key((short)b) + 1u) << 8) | (uint32_t)(HL_BN - 1 - (cl + i));
            best[t] = max(best[t], ok ? c : 0u);
            if (nb + i == tg[t]) rtgt[t] = (uint32_t)b << 16;
            acc[j][t][i] = ok ? bf2f(b) : ninf;
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t >= mtw) continue;  // wave-uniform
        uint32_t bt = best[t];
        bt = max(bt, (uint32_t)__shfl_xor((int)bt, 16, 64));
        bt = max(bt, (uint32_t)__shfl_xor((int)bt, 32, 64));
        // bt > 0: column n0 of the tile is below V.  A later tile wins only with a larger key, so
        // ties go to the smaller column.
        const float omax = rkey[t] != 0u ? key_to_f(rkey[t] - 1u) : ninf;
        if ((bt >> 8) > rkey[t]) {
          rkey[t] = bt >> 8;
          rid[t] = n0 + (HL_BN - 1 - (int)(bt & 0xFFu));
        }
        const float nmax = key_to_f(rkey[t] - 1u);
        float ls = 0.f;
        if (nmax > ninf) {  // a row of -inf alone adds nothing (and -inf - -inf is no number)
#pragma unroll
          for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) ls += hl_exp(acc[j][t][i] - nmax);
        }
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        const float scale = omax > ninf ? hl_exp(omax - nmax) : 0.f;
        rsum[t] = rsum[t] * scale + ls;
      }
    }

    if (more) l_store((s + 1) & 1);
    __syncthreads();  // stage (s + 1) & 1 written, stage s & 1 free for step s + 2
    if (last_k) {
      ++tile;
      kk = 0;
    } else {
      ++kk;
    }
  }

#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t >= mtw) continue;
    uint32_t tg = rtgt[t];  // set by the one lane that held the column
    tg = min(tg, (uint32_t)__shfl_xor((int)tg, 16, 64));
    tg = min(tg, (uint32_t)__shfl_xor((int)tg, 32, 64));
    const int m = m0 + wave * 32 + t * 16 + r;
    if (g == 0 && m < M) {
      const float mx = rkey[t] != 0u ? key_to_f(rkey[t] - 1u) : ninf;
      ws[(size_t)m * NS + slice] = make_uint4(__float_as_uint(mx), __float_as_uint(rsum[t]), (uint32_t)rid[t], tg);
    }
  }
}

__device__ __forceinline__ uint32_t hl_wave_max_u(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t hl_wave_min_u(uint32_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void head_lse_finish_kernel(const uint4* __restrict__ ws, int NS,
                                                              const int* __restrict__ target,
                                                              const int* __restrict__ out_idx, int M, int V,
                                                              float* __restrict__ tok_lp, int* __restrict__ top_id,
                                                              float* __restrict__ top_lp, long long out_len) {
  const int lane = threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  const int tg = target[row];
  const long long o = out_idx[row];
  if (tg < 0 || tg >= V || o < 0 || o >= out_len) return;
  const uint4* p = ws + (size_t)row * NS;
  const float ninf = -__builtin_inff();
  // the largest order key, then the smallest column among its holders
  uint32_t k = 0u;
  for (int s = lane; s < NS; s += 64) k = max(k, bf16_key((short)(p[s].x >> 16)) + 1u);
  k = hl_wave_max_u(k);
  const float mx = key_to_f(k - 1u);
  uint32_t id = HL_NONE, tl = HL_NONE;
  float sum = 0.f;
  for (int s = lane; s < NS; s += 64) {  // a lane's partials in slice order
    const uint4 q = p[s];
    if (bf16_key((short)(q.x >> 16)) + 1u == k) id = min(id, q.z);
    tl = min(tl, q.w);
    const float pm = __uint_as_float(q.x);
    if (pm > ninf) sum += __uint_as_float(q.y) * hl_exp(pm - mx);
  }
  id = hl_wave_min_u(id);
  tl = hl_wave_min_u(tl);
  sum = wave_sum(sum);
  if (lane == 0) {
    const float lse = logf(sum);
    // a target in [0, V) lies in exactly one slice, so tl is a logit
    tok_lp[o] = (__uint_as_float(tl) - mx) - lse;
    top_id[o] = (int)id;
    top_lp[o] = (mx - mx) - lse;  // l[top_id] is the max
  }
}

// the split: tiles per slice and the number of slices, from (M, V) alone
static int hl_plan(int M, int V, int* tps) {
  const long ntile = ((long)V + HL_BN - 1) / HL_BN, rb = ((long)M + HL_BM - 1) / HL_BM;
  long ns = (HL_TARGET_WG + rb - 1) / rb;
  if (ns > ntile) ns = ntile;
  if (ns > HL_MAX_NS) ns = HL_MAX_NS;
  const long per = (ntile + ns - 1) / ns;
  if (tps != nullptr) *tps = (int)per;
  return (int)((ntile + per - 1) / per);  // no empty slice
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_head_lse_slices(int M, int V) {
  if (M < 1 || V < 1) return 0;
  return hl_plan(M, V, nullptr);
}

extern "C" int dnn_head_lse(const void* A, int lda, const void* W, int ldw, const float* rowstat, const float* colsum,
                            const float* bias, const int* target, int M, int V, int d, void* ws, long long ws_bytes,
                            hipStream_t st) {
  if (A == nullptr || W == nullptr || target == nullptr || ws == nullptr) return -1;
  if (M < 1 || V < 1 || d < HL_KS || (d % HL_KS) != 0 || lda < d || ldw < d || (lda % 8) != 0 || (ldw % 8) != 0)
    return -1;
  if (colsum != nullptr && rowstat == nullptr) return -1;
  const uintptr_t al16 = reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W) |
                         reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(colsum) |
                         reinterpret_cast<uintptr_t>(bias);
  if ((al16 & 15u) != 0 || (reinterpret_cast<uintptr_t>(rowstat) & 7u) != 0 ||
      (reinterpret_cast<uintptr_t>(target) & 3u) != 0)
    return -1;
  int tps = 0;
  const int NS = hl_plan(M, V, &tps);
  if (ws_bytes < (long long)M * NS * 16) return -1;
  hipLaunchKernelGGL(head_lse_kernel, dim3((M + HL_BM - 1) / HL_BM, NS), dim3(256), HL_LDS, st, (const bf16_t*)A, lda,
                     (const bf16_t*)W, ldw, (const float2*)rowstat, colsum, bias, target, M, V, d, tps, NS,
                     (uint4*)ws);
  return (int)hipGetLastError();
}

extern "C" int dnn_head_lse_finish(const void* ws, long long ws_bytes, const int* target, const int* out_idx, int M,
                                   int V, float* tok_lp, int* top_id, float* top_lp, long long out_len,
                                   hipStream_t st) {
  if (ws == nullptr || target == nullptr || out_idx == nullptr || tok_lp == nullptr || top_id == nullptr ||
      top_lp == nullptr)
    return -1;
  if (M < 1 || V < 1 || out_len < 1) return -1;
  const uintptr_t al4 = reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(out_idx) |
                        reinterpret_cast<uintptr_t>(tok_lp) | reinterpret_cast<uintptr_t>(top_id) |
                        reinterpret_cast<uintptr_t>(top_lp);
  if ((reinterpret_cast<uintptr_t>(ws) & 15u) != 0 || (al4 & 3u) != 0) return -1;
  const int NS = hl_plan(M, V, nullptr);
  if (ws_bytes < (long long)M * NS * 16) return -1;
  hipLaunchKernelGGL(head_lse_finish_kernel, dim3((M + 3) / 4), dim3(256), 0, st, (const uint4*)ws, NS, target,
                     out_idx, M, V, tok_lp, top_id, top_lp, out_len);
  return (int)hipGetLastError();
}
