// Stochastic sampler with the usual filter chain and the decode step tail:
//   temperature -> top-k -> top-p (nucleus) -> min-p -> Gumbel-max draw
// in one launch per step.  The layout is sample_topk_kernel's (sampler.hip): one
// workgroup per row, the bf16 row kept in VGPRs as packed order-preserving
// 16-bit keys.  Every filter is a threshold on that key and the kept set is
//   key_i >= max(thr_k, thr_p, thr_m)
//   thr_k  the k-th largest key (16-step bisection on a block-wide count)
//   thr_p  the largest key t with  sum_{key_i >= t} w_i >= top_p * Z,
//          w_i = exp((x_i - x_max) / T) over the top-k survivors, Z = sum w_i:
//          the same bisection with the count replaced by a probability mass
//          (true at t = 0, false above the row maximum: the nucleus is never
//          empty and tokens tied at the boundary key are all kept)
//   thr_m  the smallest key whose value passes (x - x_max) / T >= log(min_p)
//          (plain fp32 subtract, then multiply: a scalar bisection over the key
//          space, no pass over the row)
// Determinism: every block-wide float sum runs in a fixed order (per-lane in
// index order, xor-shuffle tree in the wave, serial over the waves from LDS);
// no float atomics.  The draw is sample_topk_kernel's (same hash, same score),
// so with top_p = 1 and min_p = 0 the tokens are the same.
#include "common.h"
#include "sampler_common.h"

namespace dnn {

// Block-wide sum of w_i over key_i >= lo, the same value in every thread.
// One barrier per call: consecutive reductions alternate between two LDS
// buffers (`red` is this call's), so a wave that runs ahead writes the other
// buffer, and it reaches this one again only through the next call's barrier,
// which every wave passes after it has read this call's sums.
// vmx holds each 16-B vector's largest key (2 per dword): a vector none of
// whose 8 x 64 keys in the wave reaches `lo` is skipped by a wave-uniform
// branch (it would add exact zeros), which is most of them once the bisection
// has closed in on the head of the distribution.
template <int NV, int TH>
__device__ __forceinline__ float row_mass(const uint32_t (&kw)[NV][4], const uint32_t (&vmx)[(NV + 1) / 2],
                                          uint32_t lo, float xmax, float inv_temp, float* red, int lane, int wave) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    // the asm statements keep the unpack (and the loop-invariant weights) inside
    // the caller's bisection loop: hoisted, they would cost a VGPR per element
    uint32_t vw = vmx[j >> 1];
    asm volatile("" : "+v"(vw));
    const uint32_t vm = (vw >> ((j & 1) * 16)) & 0xFFFFu;
    if (__any(vm >= lo)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint32_t w = kw[j][e];
        asm volatile("" : "+v"(w));
        const uint32_t k0 = w & 0xFFFFu, k1 = w >> 16;
        if (k0 >= lo) s += __expf((key_to_f(k0) - xmax) * inv_temp);
        if (k1 >= lo) s += __expf((key_to_f(k1) - xmax) * inv_temp);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < TH / 64; ++w) tot += red[w];
  return tot;
}

template <int NV, int TH>
__global__ __launch_bounds__(TH) void sample_rows_kernel(const bf16_t* __restrict__ x, int ld, int M, int N, int* out,
                                                         float inv_temp, int topk, float top_p, float log_min_p,
                                                         int use_min_p, uint32_t seed, const int* step, int* out2,
                                                         int* pos_inc, int* hist, int hist_ld, int* thr_out) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (row >= M) return;
  const bf16_t* xr = x + (size_t)row * ld;
  // the row lives in VGPRs as packed 16-bit order-preserving keys (2 per dword)
  uint32_t kw[NV][4];
  uint32_t vmx[(NV + 1) / 2] = {};
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i0 = (tid + TH * j) * 8;
    bf16x8 p;
    if (i0 + 8 <= N) {
      p = *reinterpret_cast<const bf16x8*>(xr + i0);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] = (short)(i0 + e < N ? xr[i0 + e] : (bf16_t)0xFF80u);  // -inf pad
    }
    uint32_t vm = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t a = bf16_key(p[2 * e]), b = bf16_key(p[2 * e + 1]);
      kw[j][e] = a | (b << 16);
      asm volatile("" : "+v"(kw[j][e]));  // only the packed word stays live (not its two halves as well)
      vm = max(vm, max(a, b));
    }
    asm volatile("" : "+v"(vm));  // computed here, while the halves are at hand (not sunk to its first use)
    vmx[j >> 1] |= vm << ((j & 1) * 16);
  }
  __shared__ int red[2][16];  // two buffers each, used in turn (see row_mass)
  __shared__ float redf[2][16];
  __shared__ float bv[16];
  __shared__ int bi_s[16];
  uint32_t thr_k = 0;
  if (topk > 0 && topk < N) {
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t cand = thr_k | (1u << bit);
      int c = 0;
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          uint32_t w = kw[j][e];
          asm volatile("" : "+v"(w));  // keep the unpack inside the loop (no hoisted 2x copy)
          c += ((w & 0xFFFFu) >= cand ? 1 : 0) + ((w >> 16) >= cand ? 1 : 0);
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      int* rb = red[bit & 1];
      if (lane == 0) rb[wave] = c;
      __syncthreads();
      int tot = 0;
#pragma unroll
      for (int w = 0; w < TH / 64; ++w) tot += rb[w];
      if (tot >= topk) thr_k = cand;
    }
  }
  uint32_t thr = thr_k;
  if (top_p < 1.f || use_min_p) {
    // row maximum (integer max of the keys: exact, order-free)
    int km = 0;
#pragma unroll
    for (int j = 0; j < (NV + 1) / 2; ++j) km = max(km, (int)max(vmx[j] & 0xFFFFu, vmx[j] >> 16));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) km = max(km, __shfl_xor(km, o, 64));
    if (lane == 0) red[1][wave] = km;  // the count loop ended on buffer 0
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TH / 64; ++w) km = max(km, red[1][w]);
    const uint32_t kmax = (uint32_t)km;
    const float xmax = key_to_f(kmax);
    if (top_p < 1.f) {
      const float need = top_p * row_mass<NV, TH>(kw, vmx, thr_k, xmax, inv_temp, redf[0], lane, wave);
      uint32_t t = 0;
      int pass = 1;
      for (int bit = 15; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        // at or below thr_k the mass is Z itself; above the row maximum it is 0:
        // only the bits that split [thr_k, kmax] cost a pass over the row
        if (cand <= thr_k) { t = cand; continue; }
        if (cand > kmax) continue;
        if (row_mass<NV, TH>(kw, vmx, cand, xmax, inv_temp, redf[pass & 1], lane, wave) >= need) t = cand;
        ++pass;
      }
      thr = max(thr, t);
    }
    if (use_min_p) {
      // t = the largest key up to +inf (0xFF80) whose value fails the test; values
      // rise with the key, so everything above t passes
      uint32_t t = 0;
      for (int bit = 15; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        if (cand <= 0xFF80u && !((key_to_f(cand) - xmax) * inv_temp >= log_min_p)) t = cand;
      }
      thr = max(thr, min(t + 1u, kmax));  // the row maximum always stays
    }
  }
  const uint32_t st = step != nullptr ? (uint32_t)step[row] : (pos_inc != nullptr ? (uint32_t)pos_inc[row] : 0u);
  const uint32_t base = mix32(seed ^ mix32((uint32_t)row * 0x9E3779B9u ^ mix32(st + 0x632BE5ABu)));
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint32_t vm = (vmx[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
    if (!__any(vm >= thr)) continue;  // no survivor in this vector, wave-wide
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = (tid + TH * j) * 8 + e;
      const uint32_t k = (kw[j][e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
      if (i < N && k >= thr) {
        const uint32_t h = mix32(base ^ (uint32_t)i * 0x85EBCA6Bu);
        const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float sc = key_to_f(k) * inv_temp - __logf(-__logf(u));
        if (sc > best) { best = sc; bi = i; }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { bv[wave] = best; bi_s[wave] = bi; }
  // every thread has read its step above: the tail's position write comes after this barrier
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TH / 64; ++w)
      if (bv[w] > best || (bv[w] == best && bi_s[w] < bi)) { best = bv[w]; bi = bi_s[w]; }
    bi = bi == 0x7fffffff ? 0 : bi;
    if (thr_out != nullptr) thr_out[row] = (int)thr;
    step_tail(row, bi, out, out2, pos_inc, hist, hist_ld);
  }
}

}  // namespace dnn

using namespace dnn;

// thr_out (optional, M ints): the final key threshold of every row (tests).
extern "C" int dnn_sample_rows(const void* x, int ld, int M, int N, int* out, float temperature, int topk, float top_p,
                               float min_p, unsigned seed, const int* step, hipStream_t st, int* out2, int* pos_inc,
                               int* hist, int hist_ld, int* thr_out) {
  if (M <= 0) return 0;
  if (!(temperature > 0.f) || (ld % 8) != 0) return -1;
  if (!(top_p > 0.f && top_p <= 1.f) || !(min_p >= 0.f && min_p < 1.f)) return -1;
  if (hist != nullptr && (pos_inc == nullptr || hist_ld <= 0)) return -1;
  const int nv = (N + 8 * 1024 - 1) / (8 * 1024);
  const float it = 1.f / temperature;
  const int use_mp = min_p > 0.f ? 1 : 0;
  const float lmp = use_mp ? logf(min_p) : 0.f;
#define SAMP(NVV, THV)                                                                                                \
  {                                                                                                                   \
    hipLaunchKernelGGL((sample_rows_kernel<NVV, THV>), dim3(M), dim3(THV), 0, st, (const bf16_t*)x, ld, M, N, out, it, \
                       topk, top_p, lmp, use_mp, (uint32_t)seed, step, out2, pos_inc, hist, hist_ld, thr_out);        \
    return (int)hipGetLastError();                                                                                    \
  }
  // the dispatch of dnn_sample_topk: <= 64K entries on 1024 threads, Llama-3's
  // 128K on 512 threads x 32 vectors (128 key VGPRs + 16 of vector maxima)
  if (nv <= 1) SAMP(1, 1024)
  if (nv <= 2) SAMP(2, 1024)
  if (nv <= 4) SAMP(4, 1024)
  if (nv <= 8) SAMP(8, 1024)
  if (nv <= 16) SAMP(32, 512)
#undef SAMP
  return -2;  // vocabulary > 128K entries
}
