// Ragged prompts: the hidden row of every sequence's own last prompt position,
// gathered out of one piece of a right-padded prefill (runtime/sampling.py
// ragged_last_rows_ref is the torch mirror).
//
// A piece covers prompt positions [t0, t0 + Tc) of B sequences; h holds its
// hidden states as rows (b * Tc + t) of ld entries.  Sequence b's prompt has
// lens[b] tokens, so its last position falls into this piece when
//   q = lens[b] - 1 - t0   lies in [0, Tc).
// Then row h[(b * Tc + q) * ld : +d] is copied to dst[b * dst_ld : +d];
// otherwise dst row b keeps what it holds (an earlier or later piece owns it).
// lens[b] <= 0 gives q < 0 for every t0 >= 0 and never matches.
//
// Layout: a wave per sequence, four per workgroup.  The row moves as 16-byte
// pieces, lane l taking pieces l, l + 64, ...: d is a multiple of 8 and every
// row starts 16-byte aligned (checked by the entry point), so no piece touches
// the gap between d and ld / dst_ld.  The decision is wave-uniform.
#include "api.h"
#include "common.h"

namespace dnn {

constexpr int RAGGED_ROWS_PER_WG = 4;

__global__ __launch_bounds__(64 * RAGGED_ROWS_PER_WG) void ragged_last_rows_kernel(
    const bf16_t* __restrict__ h, long ld, const int* __restrict__ lens, int t0, int Tc, int B, int d,
    bf16_t* __restrict__ dst, long dst_ld) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * RAGGED_ROWS_PER_WG + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform
  const long q = (long)lens[b] - 1 - (long)t0;
  if (q < 0 || q >= (long)Tc) return;  // wave-uniform: another piece holds this row's last position
  const bf16x8* src = reinterpret_cast<const bf16x8*>(h + ((size_t)b * Tc + (size_t)q) * (size_t)ld);
  bf16x8* out = reinterpret_cast<bf16x8*>(dst + (size_t)b * (size_t)dst_ld);
  const int n = d >> 3;
  for (int i = lane; i < n; i += 64) out[i] = src[i];
}

}  // namespace dnn

using namespace dnn;

extern "C" int dnn_ragged_last_rows(const void* h, int ld, const int* lens, int t0, int Tc, int B, int d, void* dst,
                                    int dst_ld, hipStream_t st) {
  if (B <= 0) return 0;
  if (h == nullptr || lens == nullptr || dst == nullptr) return -1;
  if (d <= 0 || (d % 8) != 0 || Tc <= 0 || t0 < 0) return -1;
  if (ld < d || dst_ld < d || (ld % 8) != 0 || (dst_ld % 8) != 0) return -1;
  if ((reinterpret_cast<uintptr_t>(h) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dst) & 15u) != 0) return -1;
  if (B > (1 << 24)) return -2;
  hipLaunchKernelGGL(ragged_last_rows_kernel, dim3((B + RAGGED_ROWS_PER_WG - 1) / RAGGED_ROWS_PER_WG),
                     dim3(64 * RAGGED_ROWS_PER_WG), 0, st, (const bf16_t*)h, (long)ld, lens, t0, Tc, B, d, (bf16_t*)dst,
                     (long)dst_ld);
  return (int)hipGetLastError();
}
