// Hard constraints on the last stage's logits, as one launch behind the penalty
// launch and in front of dnn_stop_suppress and the argmax / sampler kernels
// (which stay as they are): logit_bias, allowed_token_ids, bad_words_ids and
// no_repeat_ngram_size.  runtime/sampling.py constraints_ref is the written
// definition and the torch mirror; this kernel is bitwise equal to it.
//
// A row's context is c[0..len): its own prompt tokens, then its generated
// tokens in order, in ctx[row, :] (int32, row stride ctx_ld); len = pos[row] +
// pos_off (pos null: pos_off).  A decode step passes the previous step's token
// prev[row]: when it lies in [0, N) it IS c[len-1] and is stored there first
// (-1 stores nothing).  len outside [0, ctx_ld] is clamped and stores nothing.
// Per row, in this order:
//   1. logit_bias {id: b}: x[id] = bf16(float(x[id]) + b), one fp32 add rounded
//      to nearest even (ops/build.py builds this file with -ffp-contract=off);
//      the ids are distinct; every other entry keeps its bits.
//   2. allowed_token_ids: every entry of [0, N) whose bit in the mask is clear
//      becomes bf16 -inf (bits 0xFF80).
//   3. bad_words_ids: for sequence s of length L, when len >= L - 1 and
//      c[len-L+1 .. len) == s[0 .. L-1), entry s[L-1] becomes -inf.
//   4. no_repeat_ngram_size n: for every j with j + n - 1 <= len - 1, when
//      c[j .. j+n-1) == c[len-n+1 .. len), entry c[j+n-1] becomes -inf.
// A ban wins over a bias.  Context ids outside [0, N) are compared, never used
// as an index.
//
// Layout: blockIdx.y is the row, 256 threads.  Without an allowed-id mask one
// workgroup per row owns all of [0, N) and touches only the listed entries.
// With a mask the row is split over blockIdx.x like the penalty launch (2048
// columns per workgroup, one 16-byte vector and one mask byte per thread), and
// every workgroup runs all four phases but writes only inside its own columns:
// its vector read-modify-write of phase 2 would otherwise put back an entry
// that another workgroup has biased or banned meanwhile.  The same hazard
// inside a workgroup is what the two barriers are for (bias before any ban,
// the vector pass before the single-entry bans).  All bans store the same 16
// bits, so duplicates are benign.  The store of prev needs no barrier of its
// own: readers take index len - 1 from the register, never from memory.
#include "api.h"
#include "common.h"

namespace dnn {

constexpr int CON_TH = 256;
constexpr int CON_COLS = CON_TH * 8;
constexpr bf16_t CON_NEG_INF = (bf16_t)0xFF80u;

__global__ __launch_bounds__(CON_TH) void logit_constraints_kernel(
    bf16_t* __restrict__ x, int ld, int N, int* ctx, int ctx_ld, const int* __restrict__ pos, int pos_off,
    const int* __restrict__ prev, const int* __restrict__ bias_ids, const float* __restrict__ bias_vals, int n_bias,
    const uint8_t* __restrict__ allow, const int* __restrict__ bad_ids, const int* __restrict__ bad_len, int n_bad,
    int ngram) {
  const int row = blockIdx.y;
  const int tid = threadIdx.x;
  bf16_t* xr = x + (size_t)row * ld;
  int lo = 0, hi = N;
  if (allow != nullptr) {
    lo = blockIdx.x * CON_COLS;
    hi = lo + CON_COLS < N ? lo + CON_COLS : N;
  }

  if (n_bias > 0) {
    for (int k = tid; k < n_bias; k += CON_TH) {
      const int id = bias_ids[k];
      if (id >= lo && id < hi) xr[id] = f2bf(bf2f(xr[id]) + bias_vals[k]);
    }
    __syncthreads();
  }

  if (allow != nullptr) {
    const int i0 = lo + tid * 8;
    if (i0 < N) {
      const uint32_t m = allow[i0 >> 3];
      if (i0 + 8 <= N) {
        if (m != 0xFFu) {
          bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (m != 0u) v = *reinterpret_cast<const bf16x8*>(xr + i0);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (((m >> e) & 1u) == 0u) v[e] = (short)CON_NEG_INF;
          *reinterpret_cast<bf16x8*>(xr + i0) = v;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (i0 + e < N && ((m >> e) & 1u) == 0u) xr[i0 + e] = CON_NEG_INF;
      }
    }
    __syncthreads();
  }

  // the context: len, and the previous token kept in a register as c[len-1]
  const int* cr = nullptr;
  int len = 0, p = -1;
  if (ctx != nullptr) {
    cr = ctx + (size_t)row * ctx_ld;
    const int raw = (pos != nullptr ? pos[row] : 0) + pos_off;
    len = raw < 0 ? 0 : (raw > ctx_ld ? ctx_ld : raw);
    if (prev != nullptr && raw == len && len >= 1) {
      const int t = prev[row];
      if (t >= 0 && t < N) p = t;
    }
    if (p >= 0 && blockIdx.x == 0 && tid == 0) ctx[(size_t)row * ctx_ld + len - 1] = p;
  }
  const int last = len - 1;
  const auto at = [&](int i) { return (i == last && p >= 0) ? p : cr[i]; };

  if (tid < n_bad) {
    const int L = bad_len[tid];
    if (L >= 1 && L <= DNN_CON_MAX_BAD_LEN) {
      const int* s = bad_ids + tid * DNN_CON_MAX_BAD_LEN;
      const int t = s[L - 1];
      if (t >= lo && t < hi) {
        bool hit = L == 1;
        if (!hit && cr != nullptr && len >= L - 1) {
          hit = true;
          for (int k = 0; k < L - 1; ++k)
            if (at(len - L + 1 + k) != s[k]) {
              hit = false;
              break;
            }
        }
        if (hit) xr[t] = CON_NEG_INF;
      }
    }
  }

  if (ngram > 0 && cr != nullptr && len >= ngram) {
    const int s0 = len - ngram + 1;  // the suffix c[s0 .. len): ngram - 1 tokens
    for (int j = tid; j <= len - ngram; j += CON_TH) {
      bool hit = true;
      for (int k = 0; k < ngram - 1; ++k)
        if (cr[j + k] != at(s0 + k)) {  // j + k <= len - 2: never the entry prev goes to
          hit = false;
          break;
        }
      if (hit) {
        const int t = at(j + ngram - 1);
        if (t >= lo && t < hi) xr[t] = CON_NEG_INF;
      }
    }
  }
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_logit_constraints(void* x, int ld, int M, int N, int* ctx, int ctx_ld, const int* pos, int pos_off,
                                     const int* prev, const int* bias_ids, const float* bias_vals, int n_bias,
                                     const unsigned char* allow, const int* bad_ids, const int* bad_len, int n_bad,
                                     int ngram, const int* h_bias_ids, const float* h_bias_vals, const int* h_bad_ids,
                                     const int* h_bad_len, hipStream_t st) {
  if (M <= 0) return 0;
  if (x == nullptr || N <= 0 || (ld % 8) != 0 || ld < N) return -1;
  if ((reinterpret_cast<uintptr_t>(x) & 15u) != 0) return -1;  // 16-byte vectors
  if (n_bias < 0 || n_bias > DNN_CON_MAX_BIAS || n_bad < 0 || n_bad > DNN_CON_MAX_BAD) return -1;
  if (ngram < 0 || ngram > DNN_CON_MAX_NGRAM) return -1;
  if (n_bias > 0 && (bias_ids == nullptr || bias_vals == nullptr || h_bias_ids == nullptr || h_bias_vals == nullptr))
    return -1;
  if (n_bad > 0 && (bad_ids == nullptr || bad_len == nullptr || h_bad_ids == nullptr || h_bad_len == nullptr))
    return -1;
  const auto finite = [](float v) { return v - v == 0.f; };  // false for +-inf and NaN
  for (int k = 0; k < n_bias; ++k)
    if (h_bias_ids[k] < 0 || h_bias_ids[k] >= N || !finite(h_bias_vals[k])) return -1;
  bool need_ctx = ngram > 0;
  for (int s = 0; s < n_bad; ++s) {
    const int L = h_bad_len[s];
    if (L < 1 || L > DNN_CON_MAX_BAD_LEN) return -1;
    for (int j = 0; j < L; ++j) {
      const int e = h_bad_ids[s * DNN_CON_MAX_BAD_LEN + j];
      if (e < 0 || e >= N) return -1;
    }
    need_ctx = need_ctx || L > 1;
  }
  if (need_ctx && ctx == nullptr) return -1;
  if (ctx != nullptr && ctx_ld <= 0) return -1;
  if (M > 65535 || N > (1 << 30)) return -2;  // rows are blockIdx.y; column indices stay in int
  if (n_bias == 0 && allow == nullptr && n_bad == 0 && ngram == 0 && (ctx == nullptr || prev == nullptr)) return 0;
  const int gx = allow != nullptr ? (N + CON_COLS - 1) / CON_COLS : 1;
  hipLaunchKernelGGL(logit_constraints_kernel, dim3(gx, M), dim3(CON_TH), 0, st, (bf16_t*)x, ld, N, ctx, ctx_ld, pos,
                     pos_off, prev, bias_ids, bias_vals, n_bias, (const uint8_t*)allow, bad_ids, bad_len, n_bad, ngram);
  return (int)hipGetLastError();
}
