// Per-token log-probabilities and the top-n alternatives of the last stage's
// logits, as a launch of its own behind the argmax / sampler launch (which
// stays as it is and whose token this one reads).  For a row x of N bf16
// logits (after the penalties, before temperature and filters):
//   m = max x,  s = sum exp(x - m)  in fp32,  lp(i) = (x_i - m) - log(s)
//   chosen = lp(tok[row]);  top[0..n) = the n entries largest by (value
//   descending, index ascending), taken on the sampler's 16-bit ordered key
//   (sampler_common.h), so the order depends on the bf16 bits alone; -inf
//   entries have lp = -inf and come last.
// The results go to device histories indexed like the token history:
//   lp_hist[row, p], top_id_hist[row, p, 0..n), top_lp_hist[row, p, 0..n)
// with p = pos[row] + pos_off (a fused step tail has advanced pos already:
// pos_off = -1); p outside [0, hist_ld) writes nothing.
// runtime/sampling.py logprobs_ref is the fp64 mirror.  Built with
// -ffp-contract=off (ops/build.py): the two subtractions stay two roundings.
//
// Layout: at B = 64 a workgroup per row would use a quarter of the chip, so a
// row is split into chunks of 2048 columns (blockIdx.x; blockIdx.y is the
// row; 25 x M workgroups at GPT-2's vocabulary), one 16-byte vector per
// thread, read once.  Every workgroup leaves {m, s} of its chunk and the
// chunk's n best (key, index) pairs in the workspace; the workgroup of a row
// that arrives last merges them in the same launch and writes the histories.
// Top-n: n rounds of a workgroup-wide maximum over one 32-bit composite per
// element, (key + 1) << 11 | (2047 - place), which is unique per element, so
// the winner clears itself and ties resolve to the smaller place.  The chunks
// are in index order and each chunk's candidates are in (value, index) order,
// so in the merge the candidate's slot (chunk * n + rank, < 2048) is the
// place: the same routine serves both levels.
// Hand-off (as gemm_stream.h's in-launch split-K combine): partials stored
// write-through (relaxed agent-scope atomics = sc1 stores) and drained by
// every wave, a workgroup barrier, one lane's ticket add; the merging
// workgroup reads every partial with sc1 loads and re-arms the ticket, so
// the counters are zero again when the kernel ends (graph replays start clean).
#include "common.h"
#include "sampler_common.h"

namespace dnn {

constexpr int LP_TH = 256;
constexpr int LP_CHUNK = LP_TH * 8;
constexpr int LP_MAX_N = 20;
constexpr int LP_CNT_LD = 32;  // words a row's arrival counter has to itself
constexpr int LP_MAX_SPLIT = LP_CHUNK / LP_MAX_N;  // 102 chunks: every candidate of a row has a slot < 2048

typedef GLB_AS unsigned gu32_t;
__device__ __forceinline__ void lp_store(void* p, uint32_t v) {
  __hip_atomic_store((gu32_t*)(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lp_load(const void* p) {
  return __hip_atomic_load((gu32_t*)(const_cast<void*>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
  v = max(v, dpp_u<0xB1>(v));
  v = max(v, dpp_u<0x4E>(v));
  v = max(v, dpp_u<0x141>(v));
  v = max(v, dpp_u<0x140>(v));
  v = max(v, (uint32_t)__shfl_xor((int)v, 16, 64));
  v = max(v, (uint32_t)__shfl_xor((int)v, 32, 64));
  return v;
}

struct LpShared {
  float redf[2][4];
  uint32_t redu[2][4];
  uint32_t win[LP_MAX_N];
  uint32_t last;
};

// workgroup-wide max / sum of one float per thread (every thread gets it); `buf` alternates between calls
__device__ __forceinline__ float block_max_f(float v, float* buf) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(buf[0], buf[1]), fmaxf(buf[2], buf[3]));
}
__device__ __forceinline__ float block_sum_f(float v, float* buf) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
  __syncthreads();
  return (buf[0] + buf[1]) + (buf[2] + buf[3]);
}

// sh.win[r] = the r-th largest composite of the workgroup's 8 x 256 (0 = none
// left), r < n.  One barrier per round: round r + 2 reuses round r's buffer
// only behind the barrier of round r + 1, which every reader of round r has
// reached.
__device__ __forceinline__ void select_top(uint32_t (&c)[8], int n, LpShared& sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = 0; r < n; ++r) {
    uint32_t b = c[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) b = max(b, c[e]);
    b = wave_max_u(b);
    uint32_t* buf = sh.redu[r & 1];
    if (lane == 0) buf[wave] = b;
    __syncthreads();
    const uint32_t w = max(max(buf[0], buf[1]), max(buf[2], buf[3]));
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (c[e] == w) c[e] = 0u;  // composites are unique: only the winner goes
    if (threadIdx.x == 0) sh.win[r] = w;
  }
  __syncthreads();
}

// workspace: ws_ld 32-bit words per row, each row's block on its own (row r of a call uses block r):
//   [0, 32)                    the row's arrival counter on a 128-byte line of its own (the S tickets of a
//                              row queue there), zero between launches
//   + S * 2                    {m, s} per chunk
//   + S * n                    key + 1 of the chunk's candidates (0 = none)
//   + S * n                    their column indices
// A counter's place depends on the workspace (ws_ld) alone, never on the M, N or n of a call, and no call
// writes anything else into a block's first 32 words: calls of different shapes may share a workspace.
__global__ __launch_bounds__(LP_TH) void logprobs_kernel(const bf16_t* __restrict__ x, int ld, int N,
                                                         const int* __restrict__ tok, const int* __restrict__ pos,
                                                         int pos_off, int n, float* __restrict__ lp_hist,
                                                         int* __restrict__ top_id_hist,
                                                         float* __restrict__ top_lp_hist, int hist_ld, int top_ld,
                                                         uint32_t* __restrict__ ws, int ws_ld) {
  __shared__ LpShared sh;
  const int row = blockIdx.y, chunk = blockIdx.x, S = gridDim.x;
  const int tid = threadIdx.x;
  const bf16_t* xr = x + (size_t)row * ld;
  uint32_t* cnt = ws + (size_t)row * ws_ld;
  uint32_t* ms = cnt + LP_CNT_LD;
  uint32_t* ckey = ms + S * 2;
  uint32_t* cidx = ckey + S * n;
  const float ninf = -__builtin_inff();

  // the row's position and its token's logit: fetched now by every workgroup (a few bytes), so the one that
  // merges does not wait for two more dependent round trips at the end
  const int p = (pos != nullptr ? pos[row] : 0) + pos_off;
  float x_tok = __builtin_nanf("");
  if (tid == LP_TH - 1) {
    const int t = tok[row];
    if (t >= 0 && t < N) x_tok = bf2f(xr[t]);
  }

  // ---- this chunk: max, sum of exponentials, n best
  const int li0 = tid * 8, i0 = chunk * LP_CHUNK + li0;
  float f[8];
  uint32_t c[8];
  if (i0 + 8 <= N) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + i0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = bf2f_s(v[e]);
      c[e] = ((bf16_key(v[e]) + 1u) << 11) | (uint32_t)(LP_CHUNK - 1 - (li0 + e));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = ninf;  // [N, ld) is never read
      c[e] = 0u;
      if (i0 + e < N) {
        const bf16_t v = xr[i0 + e];
        f[e] = bf2f(v);
        c[e] = ((bf16_key((short)v) + 1u) << 11) | (uint32_t)(LP_CHUNK - 1 - (li0 + e));
      }
    }
  }
  float m = f[0];
#pragma unroll
  for (int e = 1; e < 8; ++e) m = fmaxf(m, f[e]);
  m = block_max_f(m, sh.redf[0]);
  float s = 0.f;
  if (m > ninf) {  // a chunk of -inf alone adds nothing (and -inf - -inf is no number)
#pragma unroll
    for (int e = 0; e < 8; ++e) s += expf(f[e] - m);
  }
  s = block_sum_f(s, sh.redf[1]);
  if (n > 0) select_top(c, n, sh);
  if (tid < n) {
    const uint32_t w = sh.win[tid];
    lp_store(ckey + (size_t)chunk * n + tid, w >> 11);
    lp_store(cidx + (size_t)chunk * n + tid, (uint32_t)(chunk * LP_CHUNK + (LP_CHUNK - 1 - (int)(w & (LP_CHUNK - 1)))));
  }
  if (tid == LP_TH - 1) {
    lp_store(ms + chunk * 2, __float_as_uint(m));
    lp_store(ms + chunk * 2 + 1, __float_as_uint(s));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = old == (unsigned)S - 1;
    if (last) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh.last = last ? 1u : 0u;
  }
  __syncthreads();
  if (sh.last == 0u) return;

  // ---- the row's last workgroup: merge the S chunks
  if (p < 0 || p >= hist_ld) return;  // workgroup-uniform
  float pm = ninf, ps = 0.f;
  if (tid < S) {
    pm = __uint_as_float(lp_load(ms + tid * 2));
    ps = __uint_as_float(lp_load(ms + tid * 2 + 1));
  }
  const float mx = block_max_f(pm, sh.redf[0]);
  const float sum = block_sum_f(pm > ninf ? ps * expf(pm - mx) : 0.f, sh.redf[1]);
  const float lse = logf(sum);
  const size_t slot = (size_t)row * hist_ld + p;
  if (tid == LP_TH - 1) lp_hist[slot] = (x_tok - mx) - lse;  // NaN for a token outside [0, N)
  if (n == 0) return;
  const int ncand = S * n;  // <= 2048
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int sl = li0 + e;
    const uint32_t k1 = sl < ncand ? lp_load(ckey + sl) : 0u;
    c[e] = k1 != 0u ? (k1 << 11) | (uint32_t)(LP_CHUNK - 1 - sl) : 0u;
  }
  select_top(c, n, sh);
  if (tid < n) {
    const uint32_t w = sh.win[tid];
    int id = -1;
    float lp = ninf;
    if (w != 0u) {
      id = (int)lp_load(cidx + (LP_CHUNK - 1 - (int)(w & (LP_CHUNK - 1))));
      lp = (key_to_f((w >> 11) - 1u) - mx) - lse;
    }
    top_id_hist[slot * top_ld + tid] = id;
    top_lp_hist[slot * top_ld + tid] = lp;
  }
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_logprobs_ws_row_words(int N, int n) {
  if (N <= 0 || n < 0 || n > LP_MAX_N) return 0;
  const long S = (N + LP_CHUNK - 1) / LP_CHUNK;
  if (S > LP_MAX_SPLIT) return 0;
  const long w = LP_CNT_LD + S * 2 + 2 * S * n;
  return (int)((w + LP_CNT_LD - 1) / LP_CNT_LD * LP_CNT_LD);  // every block starts on a 128-byte line
}

extern "C" int dnn_logprobs_rows(const void* x, int ld, int M, int N, const int* tok, const int* pos, int pos_off,
                                 int n, float* lp_hist, int* top_id_hist, float* top_lp_hist, int hist_ld, int top_ld,
                                 void* ws, int ws_rows, int ws_ld, hipStream_t st) {
  if (M <= 0) return 0;
  if (x == nullptr || tok == nullptr || lp_hist == nullptr || ws == nullptr || N <= 0 || hist_ld <= 0) return -1;
  if ((ld % 8) != 0 || ld < N || (reinterpret_cast<uintptr_t>(x) & 15u) != 0) return -1;  // 16-byte vectors
  if (n < 0 || n > LP_MAX_N || n > N) return -1;
  if (n > 0 && (top_id_hist == nullptr || top_lp_hist == nullptr || top_ld < n)) return -1;
  const int S = (N + LP_CHUNK - 1) / LP_CHUNK;
  if (M > 65535 || S > LP_MAX_SPLIT) return -2;  // rows are blockIdx.y; a row's candidates fill one workgroup
  if ((reinterpret_cast<uintptr_t>(ws) & 3u) != 0 || ws_rows < M || (ws_ld % LP_CNT_LD) != 0 ||
      ws_ld < dnn_logprobs_ws_row_words(N, n))
    return -1;
  hipLaunchKernelGGL(logprobs_kernel, dim3(S, M), dim3(LP_TH), 0, st, (const bf16_t*)x, ld, N, tok, pos, pos_off, n,
                     lp_hist, top_id_hist, top_lp_hist, hist_ld, top_ld, (uint32_t*)ws, ws_ld);
  return (int)hipGetLastError();
}
