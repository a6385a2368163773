// Helpers shared by the samplers (sampler.hip: argmax, temperature + top-k;
// sample_filter.hip: + top-p / min-p with the decode step tail).
#pragma once
#include "common.h"

namespace dnn {

// ties -> smallest index (numpy semantics)
__device__ __forceinline__ void argmax_merge(float& best, int& bi, float v, int i) {
  if (v > best || (v == best && i < bi)) { best = v; bi = i; }
}

// Token history (multi-step decode graphs): `hist[row * hist_ld + pos]` gets
// the sampled id at the row's position before the advance, so K decode steps
// replayed as one graph leave every step's token in device memory (no host
// bookkeeping per step); positions outside [0, hist_ld) are not written.
__device__ __forceinline__ void step_tail(int row, int bi, int* out, int* out2, int* pos_inc, int* hist,
                                          int hist_ld) {
  out[row] = bi;
  if (out2 != nullptr) out2[row] = bi;
  if (pos_inc != nullptr) {
    const int p = pos_inc[row];
    if (hist != nullptr && p >= 0 && p < hist_ld) hist[(size_t)row * hist_ld + p] = bi;
    pos_inc[row] = p + 1;
  }
}

// bf16 bits -> 16-bit key with the order of the values (-NaN < -inf < ... < +inf < +NaN)
__device__ __forceinline__ uint32_t bf16_key(short v) {
  const uint32_t u = (uint16_t)v;
  return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ float key_to_f(uint32_t k) {
  const uint32_t u = (k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu);
  return __uint_as_float(u << 16);
}

}  // namespace dnn
