// Tile helpers shared by the LDS-staged GEMMs (gemm_bf16.hip: the bf16 and fp8
// tile kernels; gemm_w4a8.h): the 128-byte-row LDS image with its chunk
// swizzle, the half-tile staging by LDS-DMA, the tile order and the raw barrier.
#pragma once
#include "common.h"

namespace dnn {

// 16-byte chunk c of LDS row `row` (128-byte rows) is stored at chunk position
// c ^ swz_chunk(row): the swizzle is applied to the DMA's SOURCE address, the
// LDS writes stay lane-linear.
__device__ __forceinline__ int swz_chunk(int row) { return (row >> 1) & 7; }

// Tile order: the XCD remap gives each XCD a contiguous run of logical ids;
// inside it tiles go GROUP_M rows of M-tiles at a time, M fastest, so the ~32-64
// tiles co-resident on one XCD share a few A and W panels in its L2.
__device__ __forceinline__ void tile_coords(int logical, int ntm, int ntn, int& tm, int& tn) {
  constexpr int GROUP_M = 8;
  const int per_group = GROUP_M * ntn;
  const int grp = logical / per_group;
  const int first = grp * GROUP_M;
  const int gm = min(ntm - first, GROUP_M);
  const int r = logical - grp * per_group;
  tm = first + r % gm;
  tn = r / gm;
}

// Stage one 128x64 half-tile: 2 glds per thread, 8 rows per wave-instruction.
__device__ __forceinline__ void stage_half(const bf16_t* __restrict__ src, int ld, int r0, int nrows, int k0,
                                           char* dst, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int piece = i * 8 + wave;
    const int rl = piece * 8 + (lane >> 3);
    const int cs = (lane & 7) ^ swz_chunk(rl);
    int r = r0 + rl;
    r = r < nrows ? r : nrows - 1;
    glds16(src + (size_t)r * ld + k0 + cs * 8, dst + piece * 1024);
  }
}

__device__ __forceinline__ void bg_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

}  // namespace dnn
