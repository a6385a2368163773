// Stop tokens, stop sequences and min_new_tokens on the last stage, as device
// state updated inside the decode graphs (runtime/sampling.py holds the same
// definition as the docstring of stop_ref, and the torch mirror).
//
// Per sequence, generated tokens count from 1: the token sampled from the
// prompt's last position is token 1.  g = tokens generated before this step.
//   1. Suppression (min_new > 0 only; dnn_stop_suppress, after the penalty
//      launch and before the argmax / sampler launch): while g < min_new every
//      stop id's logit becomes bf16 -inf (bits 0xFF80).  A finished row is left
//      alone.
//   2. The unchanged argmax / sampler launch picks token t; its tail writes it
//      to `out`, to the next input ids and to hist[row, p], and advances the
//      position.
//   3. dnn_stop_rows, last in the step, per row:
//      finished already: t is replaced by `pad` wherever the tail wrote it
//        (tok, `also`, hist[row, p] with p = pos[row] + pos_off); the finish
//        record does not change.
//      running: g += 1, t enters the row's window of the last 15 generated
//        tokens.  The row finishes with length g when t is a stop id (reason
//        1 + index), else when the last len(s) generated tokens equal stop
//        sequence s and g >= max(min_new, len(s)) (reason 17 + index).  A stop
//        id wins over a sequence, the lowest index wins within a kind; the
//        stop token / sequence stays in the output.  Prompt tokens never take
//        part: g >= len(s) means all len(s) compared tokens were generated
//        (the window starts as -1).
// Positions advance for finished rows too: the graphs stay static and a
// finished row's work is wasted, not skipped.
//
// State: DNN_STOP_STATE_WORDS = 18 int32 per KV-cache row,
//   [0] g   [1] finish length (0 = running)   [2] reason code
//   [3..18) the window, newest first.
//
// Layout: a wave per row, four rows per workgroup.  Lanes 0..17 hold the row's
// state (one coalesced load, one coalesced store).  With h[0] = t and h[j] =
// window[j - 1], sequence s matches when rseq[s][j] == h[j] for every j <
// len(s), rseq being s newest-first.  Lane l compares (s = l / 8, j = l % 8 and
// j + 8); one ballot of the mismatches decides all eight sequences (byte s of
// the mask is zero), a second picks the lowest matching one, a third the lowest
// matching stop id.  The tables (16 ids, 8 x 16 sequence entries, the lengths)
// are kernel arguments by value: a few hundred bytes, the same for every row,
// read from the kernarg segment and never from a token-indexed address: the
// kernel only compares token values, so an out-of-range id cannot fault it.
#include "api.h"
#include "common.h"

namespace dnn {

constexpr int STW = DNN_STOP_STATE_WORDS;
constexpr int STOP_ROWS_PER_WG = 4;

struct StopTables {
  int ids[DNN_STOP_MAX_IDS];
  int rseq[DNN_STOP_MAX_SEQS][DNN_STOP_MAX_SEQ_LEN];  // newest first
  unsigned long long lens;                            // byte s = len(s), 0 = no such sequence
  int n_ids;
};

struct StopIds {
  int ids[DNN_STOP_MAX_IDS];
  int n_ids;
};

__global__ __launch_bounds__(64 * STOP_ROWS_PER_WG) void stop_rows_kernel(int* __restrict__ tok, int* __restrict__ also,
                                                                         int* __restrict__ hist, int hist_ld,
                                                                         const int* __restrict__ pos, int pos_off,
                                                                         int* __restrict__ state, const StopTables tb,
                                                                         int min_new, int pad, int M) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * STOP_ROWS_PER_WG + (threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  int* st = state + (size_t)row * STW;
  const int v = lane < STW ? st[lane] : 0;
  const int t = tok[row];
  const int g = __builtin_amdgcn_readlane(v, 0);
  const int fin = __builtin_amdgcn_readlane(v, 1);
  if (fin != 0) {  // finished: pad wherever the step tail wrote t, the record stays
    if (lane == 0) tok[row] = pad;
    if (lane == 1 && also != nullptr) also[row] = pad;
    if (lane == 2 && hist != nullptr) {
      const int p = (pos != nullptr ? pos[row] : 0) + pos_off;
      if (p >= 0 && p < hist_ld) hist[(size_t)row * hist_ld + p] = pad;
    }
    return;
  }
  const int g1 = g + 1;
  const int s = lane >> 3, j0 = lane & 7;
  const int len = (int)((tb.lens >> (8 * s)) & 0xFFull);
  const int wa = __shfl(v, j0 + 2, 64);  // window[j0 - 1] (j0 = 0: unused)
  const int hb = __shfl(v, j0 + 10, 64);  // window[j0 + 7]
  const int ha = j0 == 0 ? t : wa;
  const bool mis = (j0 < len && tb.rseq[s][j0] != ha) || (j0 + 8 < len && tb.rseq[s][j0 + 8] != hb);
  const unsigned long long bal = __ballot(mis);
  const int len_l = (int)((tb.lens >> (8 * (lane & 7))) & 0xFFull);
  const bool seq_hit = lane < DNN_STOP_MAX_SEQS && len_l > 0 && g1 >= (min_new > len_l ? min_new : len_l) &&
                       ((bal >> (8 * (lane & 7))) & 0xFFull) == 0ull;
  const unsigned long long seq_m = __ballot(seq_hit);
  const bool id_hit = lane < tb.n_ids && tb.ids[lane & (DNN_STOP_MAX_IDS - 1)] == t;
  const unsigned long long id_m = __ballot(id_hit);
  int reason = 0;
  if (id_m != 0ull)
    reason = 1 + __builtin_ctzll(id_m);
  else if (seq_m != 0ull)
    reason = 1 + DNN_STOP_MAX_IDS + __builtin_ctzll(seq_m);
  const int older = __shfl_up(v, 1, 64);  // the window moves one place: word l takes word l - 1
  int nv = older;
  if (lane == 0) nv = g1;
  if (lane == 1) nv = reason != 0 ? g1 : 0;
  if (lane == 2) nv = reason;
  if (lane == 3) nv = t;
  if (lane < STW) st[lane] = nv;
}

// thread (row, k): stop id k of an unfinished row with g < min_new gets -inf
__global__ __launch_bounds__(256) void stop_suppress_kernel(bf16_t* __restrict__ x, int ld, int M, int N,
                                                            const int* __restrict__ state, const StopIds tb,
                                                            int min_new) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int row = i / DNN_STOP_MAX_IDS, k = i % DNN_STOP_MAX_IDS;
  if (row >= M || k >= tb.n_ids) return;
  const int* st = state + (size_t)row * STW;
  if (st[1] != 0 || st[0] >= min_new) return;
  const int id = tb.ids[k];
  if (id < 0 || id >= N) return;  // checked on the host too
  x[(size_t)row * ld + id] = (bf16_t)0xFF80u;
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_stop_rows(int* tok, int* also, int* hist, int hist_ld, const int* pos, int pos_off, int* state,
                             const int* stop_ids, int n_ids, const int* seqs, const int* seq_len, int n_seq,
                             int min_new, int pad, int M, hipStream_t st) {
  if (M <= 0) return 0;
  if (tok == nullptr || state == nullptr) return -1;
  if (n_ids < 0 || n_ids > DNN_STOP_MAX_IDS || n_seq < 0 || n_seq > DNN_STOP_MAX_SEQS) return -1;
  if ((n_ids > 0 && stop_ids == nullptr) || (n_seq > 0 && (seqs == nullptr || seq_len == nullptr))) return -1;
  if (pad < 0 || min_new < 0 || (hist != nullptr && hist_ld <= 0)) return -1;
  StopTables tb;
  for (int k = 0; k < DNN_STOP_MAX_IDS; ++k) tb.ids[k] = -1;
  for (int s = 0; s < DNN_STOP_MAX_SEQS; ++s)
    for (int j = 0; j < DNN_STOP_MAX_SEQ_LEN; ++j) tb.rseq[s][j] = -1;
  tb.lens = 0ull;
  tb.n_ids = n_ids;
  for (int k = 0; k < n_ids; ++k) {
    if (stop_ids[k] < 0) return -1;
    tb.ids[k] = stop_ids[k];
  }
  for (int s = 0; s < n_seq; ++s) {
    const int len = seq_len[s];
    if (len < 1 || len > DNN_STOP_MAX_SEQ_LEN) return -1;
    for (int j = 0; j < len; ++j) {
      const int e = seqs[s * DNN_STOP_MAX_SEQ_LEN + len - 1 - j];
      if (e < 0) return -1;
      tb.rseq[s][j] = e;
    }
    tb.lens |= (unsigned long long)len << (8 * s);
  }
  if (M > (1 << 24)) return -2;
  hipLaunchKernelGGL(stop_rows_kernel, dim3((M + STOP_ROWS_PER_WG - 1) / STOP_ROWS_PER_WG),
                     dim3(64 * STOP_ROWS_PER_WG), 0, st, tok, also, hist, hist_ld, pos, pos_off, state, tb, min_new, pad,
                     M);
  return (int)hipGetLastError();
}

extern "C" int dnn_stop_suppress(void* x, int ld, int M, int N, const int* state, const int* stop_ids, int n_ids,
                                 int min_new, hipStream_t st) {
  if (M <= 0) return 0;
  if (x == nullptr || state == nullptr || (ld % 8) != 0 || ld < N || N <= 0) return -1;
  if ((reinterpret_cast<uintptr_t>(x) & 15u) != 0) return -1;
  if (n_ids < 0 || n_ids > DNN_STOP_MAX_IDS || (n_ids > 0 && stop_ids == nullptr) || min_new < 0) return -1;
  StopIds tb;
  for (int k = 0; k < DNN_STOP_MAX_IDS; ++k) tb.ids[k] = -1;
  tb.n_ids = n_ids;
  for (int k = 0; k < n_ids; ++k) {
    if (stop_ids[k] < 0 || stop_ids[k] >= N) return -1;
    tb.ids[k] = stop_ids[k];
  }
  if (n_ids == 0 || min_new == 0) return 0;  // nothing to suppress
  if (M > (1 << 24) || N > (1 << 30)) return -2;
  const int threads = M * DNN_STOP_MAX_IDS;
  hipLaunchKernelGGL(stop_suppress_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, (bf16_t*)x, ld, M, N, state,
                     tb, min_new);
  return (int)hipGetLastError();
}
