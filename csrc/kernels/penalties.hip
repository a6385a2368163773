// Repetition / presence / frequency penalties on the last stage's logits, as a
// launch of its own in front of the argmax / sampler kernels (which stay as
// they are).  State: one uint16 per (row, vocabulary entry),
//   bit 15     P  the token occurs in the prompt
//   bits 0..14 g  times the token was generated in this generation (saturates)
// and per row, in this order:
//   1. prev[row] (the previous step's token, when given and inside [0, N)):
//      g += 1 unless g = 0x7FFF; P is kept
//   2. for every entry with P or g > 0, in fp32 without contraction
//      (ops/build.py builds this file with -ffp-contract=off):
//        x = float(logit)
//        if rep != 1:  x = x > 0 ? x / rep : x * rep     (IEEE division)
//        if g > 0:     x = x - freq * float(g);  x = x - pres
//        logit = bf16(x)  (round to nearest even)
//      every other entry keeps its bits.
// runtime/sampling.py apply_penalties_ref does the same operations in the same
// order in torch fp32 and is bitwise equal.
//
// Layout: the work is element-wise, so a row is split over blockIdx.x (2048
// columns per workgroup, one 16-byte vector of 8 state entries per thread) and
// blockIdx.y is the row: 25 x M workgroups at GPT-2's vocabulary.  The thread
// that owns column prev[row] counts it in its register and writes the one
// entry back, so no barrier and no second pass.  The state is almost all
// zeros: a vector (and, by a wave-uniform branch, a wave) whose 8 entries are
// zero neither loads nor stores logits, so the traffic is the state table plus
// the touched logits vectors.
#include "common.h"

namespace dnn {

constexpr int PEN_TH = 256;

__device__ __forceinline__ float penalise(float x, uint32_t c, float rep, float freq, float pres) {
  const uint32_t g = c & 0x7FFFu;
  if (rep != 1.f) x = x > 0.f ? x / rep : x * rep;
  if (g > 0u) {
    x = x - freq * (float)g;
    x = x - pres;
  }
  return x;
}

__global__ __launch_bounds__(PEN_TH) void logit_penalties_kernel(bf16_t* __restrict__ x, int ld, int N,
                                                                 uint16_t* __restrict__ cnt, int cnt_ld,
                                                                 const int* __restrict__ prev, float rep, float freq,
                                                                 float pres) {
  const int row = blockIdx.y;
  const int i0 = (blockIdx.x * PEN_TH + threadIdx.x) * 8;
  uint16_t* cr = cnt + (size_t)row * cnt_ld;
  bf16_t* xr = x + (size_t)row * ld;
  const bool full = i0 + 8 <= N;
  bf16x8 s = {0, 0, 0, 0, 0, 0, 0, 0};
  if (full) {
    s = *reinterpret_cast<const bf16x8*>(cr + i0);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (i0 + e < N) s[e] = (short)cr[i0 + e];
  }
  if (prev != nullptr) {
    const int p = prev[row];
    if (p >= i0 && p < i0 + 8 && p < N) {  // i0 >= 0: a negative token matches no thread
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (p - i0 == e) {
          uint16_t c = (uint16_t)s[e];
          if ((c & 0x7FFFu) != 0x7FFFu) {
            c = (uint16_t)(c + 1u);
            cr[p] = c;
            s[e] = (short)c;
          }
        }
    }
  }
  const i32x4 w = __builtin_bit_cast(i32x4, s);
  const bool any = (w[0] | w[1] | w[2] | w[3]) != 0;
  if (!__any(any)) return;  // the usual case: nothing of this wave's 512 columns was seen
  if (!any) return;
  if (full) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + i0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t c = (uint16_t)s[e];
      if (c != 0u) v[e] = (short)f2bf(penalise(bf2f_s(v[e]), c, rep, freq, pres));
    }
    *reinterpret_cast<bf16x8*>(xr + i0) = v;  // unseen entries go back with the bits they came with
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t c = (uint16_t)s[e];  // 0 past N: never read, never written
      if (c != 0u) xr[i0 + e] = f2bf(penalise(bf2f(xr[i0 + e]), c, rep, freq, pres));
    }
  }
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_logit_penalties(void* x, int ld, int M, int N, unsigned short* cnt, int cnt_ld, const int* prev,
                                   float rep, float freq, float pres, hipStream_t st) {
  if (M <= 0) return 0;
  if (x == nullptr || cnt == nullptr || (ld % 8) != 0 || (cnt_ld % 8) != 0 || cnt_ld < N || ld < N) return -1;
  const auto finite = [](float v) { return v - v == 0.f; };  // false for +-inf and NaN
  if (!(rep > 0.f) || !finite(freq) || !finite(pres)) return -1;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cnt)) & 15u) != 0) return -1;  // 16-byte vectors
  if (N <= 0) return 0;
  if (M > 65535 || N > (1 << 30)) return -2;  // rows are blockIdx.y; column indices stay in int
  const int per_wg = PEN_TH * 8;
  hipLaunchKernelGGL(logit_penalties_kernel, dim3((N + per_wg - 1) / per_wg, M), dim3(PEN_TH), 0, st, (bf16_t*)x, ld,
                     N, (uint16_t*)cnt, cnt_ld, prev, rep, freq, pres);
  return (int)hipGetLastError();
}
