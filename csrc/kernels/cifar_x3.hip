// CIFAR-10 ConvNet at the reference's fp32 precision on bf16 MFMA ("bf16x3").
//
// The reference computes and ships fp32 (cifar_model_parts.py:7-26,
// node.py:45-48).  gfx950 has f32-input MFMA, but at 1/16 of the bf16 rate
// (cdna_hip_programming.md §3 "FP32-input MFMA"), so every fp32 operand here
// is split into two bf16 terms, x = hi + lo with hi = bf16(x), lo = bf16(x - hi)
// (|x - hi - lo| <= 2^-17 |x|), and each product is accumulated in fp32 as
//     a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi        (a_lo*b_lo < 2^-16 |ab| dropped)
// = 3 bf16 MFMAs per fp32 product: 5.3x the f32-MFMA rate at ~2^-16 relative
// error per product before fp32 accumulation.
//
// Kernels:
//  * cifar_stage0_x3_kernel: conv1+bias+ReLU+pool -> conv2+bias+ReLU+pool ->
//    NCHW flatten, fp32 in, fp32 (B,4096) out (reference ModelPart0_2Node,
//    cifar_model_parts.py:37-42).  Persistent, 512 threads: waves 0-3
//    ("producers") stage input image it+1 and run conv1 of image it, waves 4-7
//    ("consumers") run conv2 of image it-1, one barrier per image, so each SIMD
//    pairs a VALU/LDS-heavy wave with an MFMA-heavy one.  Per image: 32 conv1
//    tiles x 3 k-steps x 3 terms + 16 conv2 tiles x 18 k-steps x 3 terms = 1152
//    v_mfma_f32_32x32x16_bf16.  LDS (126,464 B): input double-buffered as
//    hi/lo HWC4 planes [34][40][4] (pitch 40: conflict-free conv1 b64 reads),
//    pooled conv1 map double-buffered as hi/lo planes [18][18][32] with the
//    16-B chunk XORed by (Y & 3), which makes every conv2 ds_read_b128 fragment
//    (four 16-lane groups) conflict-free; conv2 results leave straight from
//    the accumulators as 8-B fp32 stores (no LDS staging).  By default conv2
//    runs instead on v_mfma_f32_16x16x32_bf16 (template parameter C2 = 1, "conv2
//    on v_mfma_f32_16x16x32_bf16" below: 1728 of them per image at the same
//    MFMA cycles, chunk XOR (2*Y & 3), 16-B stores); the 32x32x16 consumer
//    stays compiled as the A/B's other arm (dnn_cifar_s0_set_mfma).
//    conv1 on K = 32 (template parameter C1 = 1, dnn_cifar_s0_set_conv1; the
//    K = 48 producer above stays compiled as the other arm): the zero fourth
//    channel and the zero kx = 3 tap go, 32 tiles x 2 k-steps x 3 terms = 192
//    conv1 MFMAs per image instead of 288 (33,792 matrix-pipe cycles per image
//    with conv2 instead of 36,864).  LDS (113,408 B): the input double-buffered
//    as hi/lo channel-packed planes [34 rows][112 bf16] (pitch 224 B = 56
//    dwords): one zero element, then 34 pixels x 3 channels, halo included, so
//    image pixel x sits at element 3x + 4 and four pixels are 24 B on an 8-B
//    boundary (three ds_write_b64 per plane and thread; 16 contiguous lanes
//    stage rows y and y + 2, 48 dwords = 16 banks apart: conflict-free).  Pixel
//    x's 9-element window of one ky starts at element 3x + 1; the 4-B-aligned
//    5-dword read that covers it starts at 3x (even x: [junk, v0..v8]) or 3x + 1
//    (odd x: [v0..v8, junk]), and the junk element meets a zero weight, so an M
//    tile holds pixels of one x parity and each parity has its own resident
//    weight set [32 oc][32 k] (ops/cifar.py::_conv1_k32).  A tile is 4 rows x 8
//    columns of one parity (lane: row l>>3 & 3, column index l & 7, K half
//    h = l>>5); the even and the odd tile of the same 4 x 16 pixels run as one
//    pair, and the 2x2 pool is the max over the two accumulators.  K order:
//    half 0 holds dwords 0-3 of padded row 0 (k-step 0) and row 1 (k-step 1),
//    half 1 dwords 0-3 of row 2 (k-step 0) and dword 4 of rows 0, 1, 2 plus a
//    repeat of the last as filler (k-step 1); the last read of a row ends at
//    element 103 of 112, inside the same plane.  All reads are 32-bit
//    (ds_read2_b32; a 64- or 128-bit read at 4-B alignment would replay): each
//    32-lane half reads 4 rows x 8 columns at 56 r + 3 c dwords, and 56 = 24
//    (mod 32) is, with 8, the only pitch class for which {24 r + 3 c} are 32
//    distinct banks (searched over all pitches >= 51 dwords).  The pooled conv1
//    planes, their swizzle and the consumers are the same in both arms.
//    uint8 input (template parameter IN = 1, dnn_cifar_stage0_x3_u8; K = 32
//    producer only): the image arrives as (B,32,32,3) bytes and is normalised
//    by a [3][256] table of packed bf16 hi/lo halves, copied into LDS behind
//    the planes (116,480 B); the planes come out bit-identical to the fp32
//    input's (see at the kernel).
//    Issue priority: the conv2 waves carry 82 % of the MFMA cycles and, as the
//    second-dispatched half of the workgroup, lose issue arbitration to their
//    SIMD's conv1 wave.  Barrier stamps (s_memtime per role, a diagnostic build):
//    conv2 work 10,120 cycles per image with the conv1 waves idle for 2,400 at
//    the barrier.  Handing the conv2 waves the arbitration for the whole image
//    (role swap, or one s_setprio 1) brings them to 9,000 but the conv1 waves,
//    whose MFMAs and VALU then wait for gaps in a saturated pipe, to 11,400: the
//    pole moves and the kernel is 5-6 % slower.  What pays is a share: a conv2
//    wave runs the first C2_PRIO_STEPS = 9 of the 18 k-steps of each band at
//    priority 1 and the rest, with the band's epilogue, at 0 (two s_setprio per
//    band), and the conv1 waves issue fewer vector instructions so that they
//    fit in what is left: image loads and boundary stores through buffer
//    descriptors over one image (base in SGPRs, one lane offset per kernel, no
//    64-bit per-lane arithmetic), pooled-map store offsets as lane constants plus
//    a wave-uniform term, and conv1_store's parity branch (both sides ran, one
//    after the other) as selects: image loop 193 -> 170 non-MFMA vector
//    instructions (static), conv1 work 8,060 -> 6,510 cycles.  Neither half wins
//    alone (partial priority on the old addressing +1.1 %, lean addressing
//    alone a tie); together conv1 9,140 / conv2 9,660 cycles and -2.5 to -2.9 %
//    in every interleaved round (profiles/cifar_s0_arb_ab.jsonl).
//  * cifar_fc1_x3_kernel: fc1 + bias + ReLU on the fp32 boundary tensor, the
//    split done in registers while staging A (no split copy in HBM): 256x256x32
//    tiles, 8 waves of 128x64, per k32 step 3 x 32 mfma_f32_16x16x32_bf16 per
//    wave (A_hi W_hi + A_hi W_lo + A_lo W_hi) on 24 conflict-free ds_read_b128.
//    Waves 0-3 and 4-7 run half a k-step apart, so each SIMD pairs a wave
//    issuing MFMAs with one reading, splitting and restaging (the schedule above
//    the kernel).  The default arm is "LEAN": that schedule with the packed split
//    (split2<true>) and all global addressing through buffer descriptors, 51
//    non-MFMA vector instructions per k-step instead of 207; the same schedule
//    with scalar conversions and per-segment addressing stays compiled as the
//    A/B's other arm (dnn_cifar_fc1_set_sched: 1 staggered, 2 lean).
//  * cifar_split3_kernel: fp32 (B,K) -> bf16 (B,3K) = [hi | hi | lo], the A
//    operand of the small-batch fc1 (one skinny bf16 GEMM over K' = 3K against
//    W' = [W_hi | W_lo | W_hi]) when the 256^2 tiles cannot fill the chip.
//  * cifar_head_tail_x3_kernel: fc2 (512->10) + bias + softmax + per-row argmax
//    on fp32 hidden rows, 3-term split on mfma_f32_16x16x32_bf16.
//  * cifar_head_tail_kernel: the same on bf16 hidden rows and bf16 fc2 weights (the
//    bf16 precision's head tail; here for this file's IEEE exp and division).
#include <type_traits>

#include "gemm_epilogue.h"

namespace dnn {
namespace x3 {

// 2 floats -> packed bf16 hi pair and lo pair (element a in the low half).
// PK: both conversions as one v_cvt_pk_bf16_f32 per pair (6 VALU per pair
// instead of ~11.5, bitwise the same values); the empty asm keeps the two
// subtracts scalar (SLP would pack them into v_pk_add_f32, which costs more
// than it saves beside MFMAs).  PK = false is the form the
// staggered fc1 arm and the head kernel keep: their code is unchanged.
template <bool PK>
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  if constexpr (PK) {
    hi = pack2bf_pk(a, b);
    const float ah = __uint_as_float(hi << 16), bh = __uint_as_float(hi & 0xffff0000u);
    float da = a - ah;
    const float db = b - bh;
    asm("" : "+v"(da));
    lo = pack2bf_pk(da, db);
  } else {
    hi = pack2bf(a, b);
    const float ah = __uint_as_float(hi << 16), bh = __uint_as_float(hi & 0xffff0000u);
    lo = pack2bf(a - ah, b - bh);
  }
}

// Raw-buffer loads of 16 B per lane: the address is the descriptor's wave-uniform
// base + the lane's 32-bit voff + the scalar soff, with no per-lane 64-bit address
// arithmetic.  The range check drops a lane whose voff + 16 passes ``bytes``: it
// reads as 0 and touches no memory.  Do not count on soff being checked: put
// whatever can leave the allocation into base / bytes or into voff.
// base and bytes must be wave-uniform SGPR values, or every load gets a waterfall
// loop.  Device pass only: the host has no buffer resource type.
__device__ __forceinline__ float4 buf_load16(const void* base, int bytes, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
#else
  return float4{};
#endif
}
// the 4-B load and the 16-B / 8-B stores of the same addressing (a store past ``bytes`` is dropped)
__device__ __forceinline__ uint32_t buf_load4(const void* base, int bytes, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
  return __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, soff, 0);
#else
  return 0;
#endif
}
__device__ __forceinline__ void buf_store16(void* base, int bytes, int voff, int soff, uint4 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, rsrc, voff, soff, 0);
#endif
}
__device__ __forceinline__ void buf_store8(void* base, int bytes, int voff, int soff, uint2 v) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(u32x2{v.x, v.y}, rsrc, voff, soff, 0);
#endif
}
// the same load as LDS DMA (glds16's layout: lane l lands at lds_wave_base + 16 l)
__device__ __forceinline__ void buf_glds16(const void* base, int bytes, int voff, int soff, void* lds_wave_base) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (LDS_AS void*)lds_wave_base, 16, voff, soff, 0, 0);
#endif
}

__device__ __forceinline__ int dpp_xor1(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_xor2(int v) { return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false); }

constexpr int XW = 40;                        // xin row pitch (pixels); HWC4 bf16 = 8 B/pixel
constexpr int XPL = 34 * XW * 8;              // 10880: one input plane
constexpr int A1PL = 18 * 18 * 64;            // 20736: one pooled-conv1 plane [18][18][32] bf16
constexpr int XP32 = 224;                     // C1 = 1: xin row pitch in bytes (56 dwords, 103 bf16 used)
constexpr int XPL32 = 34 * XP32;              // 7616: one channel-packed input plane
// Issue arbitration between the two waves of a SIMD (the conv1 wave and the conv2 wave): a conv2
// wave runs the first C2_PRIO_STEPS of the 18 k-steps of each band at s_setprio 1 and the rest,
// with the band's epilogue, at 0 ("Issue priority" in the header).
constexpr int C2_PRIO_STEPS = 9;

// C1: conv1 producer path.  0: HWC4 planes, K = 48; 1: channel-packed planes, K = 32.
template <int C1>
__device__ __forceinline__ constexpr int xpl() {
  return C1 ? XPL32 : XPL;
}
template <int C1>
__device__ __forceinline__ constexpr int lds_bytes() {  // 126464 (C1 = 0), 113408 (C1 = 1)
  return 4 * xpl<C1>() + 4 * A1PL;
}
// IN: input kind.  0: fp32 NCHW (B,3,32,32); 1: uint8 NHWC (B,32,32,3), normalised by a table
// uint32 [3 channels][256 byte values], bf16 hi bits in the low half and bf16 lo bits in the high
// half of an entry: what split2<true> gives for the normalised float ("uint8 input" at the kernel).
constexpr int TAB_BYTES = 3 * 256 * 4;
struct U8Input {
  const unsigned char* x;
  const uint32_t* table;
};
template <int IN>
using s0_input_t = std::conditional_t<IN == 1, U8Input, const float* __restrict__>;

template <int C1>
__device__ __forceinline__ int xin_off(int k, int lo) {
  return ((k & 1) * 2 + lo) * xpl<C1>();
}
template <int C1>
__device__ __forceinline__ int a1_off(int k, int lo) {
  return 4 * xpl<C1>() + ((k & 1) * 2 + lo) * A1PL;
}

// conv2 A-fragment immediate offset for k-step S (tap = S>>1, kx = tap % 3),
// tile column I (tx2) and plane (LO): the lane/ky/parity part lives in the base.
template <int S, int I, int LO>
__device__ __forceinline__ constexpr int c2_imm() {
  return (8 * I + (S >> 1) % 3) * 64 + LO * A1PL;
}

// 4 reads of k-step S: [hi t0, hi t1, lo t0, lo t1]
template <int S>
__device__ __forceinline__ void c2_issue(const uint32_t (&b)[3][2], bf16x8 (&a)[4]) {
  constexpr int ky = (S >> 1) / 3, par = S & 1;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[0]) : "v"(b[ky][par]), "i"(c2_imm<S, 0, 0>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[1]) : "v"(b[ky][par]), "i"(c2_imm<S, 1, 0>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[2]) : "v"(b[ky][par]), "i"(c2_imm<S, 0, 1>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[3]) : "v"(b[ky][par]), "i"(c2_imm<S, 1, 1>()));
}

// k-step S: issue step S+1's reads, wait for step S's (counted lgkmcnt; the
// caller has no other LDS op in flight), then 6 MFMAs alternating the two
// tiles' accumulators.  sched_barriers keep hipcc from hoisting MFMAs above
// the wait (cdna_hip_programming.md §5.7).
template <int S>
__device__ __forceinline__ void c2_step(const uint32_t (&b)[3][2], const bf16x8 (&wh)[18], const bf16x8 (&wl)[18],
                                        f32x16 (&acc)[2], bf16x8 (&cur)[4], bf16x8 (&nxt)[4]) {
  if constexpr (S == C2_PRIO_STEPS) __builtin_amdgcn_s_setprio(0);
  if constexpr (S + 1 < 18) {
    c2_issue<S + 1>(b, nxt);
    asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[0], wh[S], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[1], wh[S], acc[1], 0, 0, 0);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[0], wl[S], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[1], wl[S], acc[1], 0, 0, 0);
  acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[2], wh[S], acc[0], 0, 0, 0);
  acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cur[3], wh[S], acc[1], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (S + 1 < 18) c2_step<S + 1>(b, wh, wl, acc, nxt, cur);
}

template <int N>
__device__ __forceinline__ void resident_fence(const bf16x8 (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) asm volatile("" ::"v"(w[i]));
}

// ---------------------------------------------------------------------------
// conv2 on v_mfma_f32_16x16x32_bf16 (C2 = 1): the same wave work, LDS reads
// and MFMA cycles as the 32x32x16 path above, on the shape that holds a higher
// clock under load.  An M tile is a 4x4 pixel block in window-major order
// (A row m = 8*y1 + 4*x1 + 2*y0 + x0 is pixel (2*y1 + y0, 2*x1 + x0)), so the
// four accumulator rows of a lane (4*(lane>>4)..+3) are one 2x2 pool window;
// an N tile is 16 output channels; one K = 32 step is one tap over the 32
// input channels.  The 16-B chunk of plane row Y is XORed by (2*Y & 3): every
// ds_read_b128 lane group of a tile then hits 16 distinct slots for all 9 taps
// (Y & 3, conflict-free for 32x8 tiles, is 2-way conflicted for 4x4 blocks).
// ---------------------------------------------------------------------------
template <int C2>
__device__ __forceinline__ int a1_swz(int Y) {
  return C2 ? (2 * Y) & 3 : Y & 3;
}

// A-fragment immediate offset of half-step T (tap = T>>1, M tiles 2*(T&1) + J), plane LO
template <int T, int J, int LO>
__device__ __forceinline__ constexpr int m16_imm() {
  return (((T >> 1) / 3) * 18 + 4 * (2 * (T & 1) + J) + (T >> 1) % 3) * 64 + LO * A1PL;
}

// 4 reads of half-step T: [hi m0, hi m1, lo m0, lo m1]; the base depends on the parity of ky only
template <int T>
__device__ __forceinline__ void m16_issue(const uint32_t (&b)[2], bf16x8 (&a)[4]) {
  constexpr int kyp = ((T >> 1) / 3) & 1;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[0]) : "v"(b[kyp]), "i"(m16_imm<T, 0, 0>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[1]) : "v"(b[kyp]), "i"(m16_imm<T, 1, 0>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[2]) : "v"(b[kyp]), "i"(m16_imm<T, 0, 1>()));
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[3]) : "v"(b[kyp]), "i"(m16_imm<T, 1, 1>()));
}

// half-step T: issue T+1's reads, wait for T's (counted lgkmcnt, no other LDS
// op in flight), then 12 MFMAs over 4 accumulators (2 M x 2 N), term-major so
// that consecutive MFMAs never share an accumulator.
template <int T>
__device__ __forceinline__ void m16_step(const uint32_t (&b)[2], const bf16x8 (&wh)[2][9], const bf16x8 (&wl)[2][9],
                                         f32x4 (&acc)[4][2], bf16x8 (&cur)[4], bf16x8 (&nxt)[4]) {
  constexpr int tap = T >> 1, m0 = 2 * (T & 1);
  if constexpr (T == C2_PRIO_STEPS) __builtin_amdgcn_s_setprio(0);
  if constexpr (T + 1 < 18) {
    m16_issue<T + 1>(b, nxt);
    asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int term = 0; term < 3; ++term)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[m0 + j][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[(term == 2 ? 2 : 0) + j],
                                                                  term == 1 ? wl[nt][tap] : wh[nt][tap], acc[m0 + j][nt], 0, 0, 0);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (T + 1 < 18) m16_step<T + 1>(b, wh, wl, acc, nxt, cur);
}

// bias + ReLU + in-lane 2x2 max-pool of N tile NT of a band (PY = its pooled
// row for this lane): lane row q = lane>>4 holds pooled column 2*mt + (q & 1)
// of M tile mt, so lanes l and l^16 hold the columns of opposite parity of the
// same (oc, PY); one v_permlane16_swap per dword hands the even row columns
// 0-3 and the odd row columns 4-7: one 16-B store per lane (8-B hi + 8-B lo in
// the blocked encoding, the split of the same fp32 values).
// The stores go through a buffer descriptor over the image's 16 KiB of the boundary: ``lane`` is
// the lane's byte offset at band 0 and N tile 0 (computed once per kernel), the band p and the N
// tile go into the scalar offset, so a store costs no per-lane address arithmetic.
//   fp32:  4*(oc*64 + PY*8 + 4*x1),  PY = 4*(rw>>1) + 2*p + y1  ->  lane + 64*p + 4096*NT
//   split: (oc*2 + (PY>>2))*128 + ((PY&3)*8 + 4*x1)*2           ->  lane + 32*p + 4096*NT  (lo: + 64)
template <bool SPLIT_OUT, int NT>
__device__ __forceinline__ void m16_epilogue(const f32x4 (&acc)[4][2], float bias, float* img, int lane, int p) {
  float v[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const f32x4& a = acc[mt][NT];
    v[mt] = fmaxf(fmax_nan(fmax_nan(a[0], a[1]), fmax_nan(a[2], a[3])) + bias, 0.f);
  }
  const auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[0]), __float_as_uint(v[2]), false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[1]), __float_as_uint(v[3]), false, false);
  if constexpr (SPLIT_OUT) {
    uint2 hi, lo;
    split2<true>(__uint_as_float(s0[0]), __uint_as_float(s0[1]), hi.x, lo.x);
    split2<true>(__uint_as_float(s1[0]), __uint_as_float(s1[1]), hi.y, lo.y);
    buf_store8(img, 16384, lane, 32 * p + 4096 * NT, hi);
    buf_store8(img, 16384, lane, 32 * p + 4096 * NT + 64, lo);
  } else {
    buf_store16(img, 16384, lane, 64 * p + 4096 * NT, make_uint4(s0[0], s0[1], s1[0], s1[1]));
  }
}

}  // namespace x3

using namespace x3;

// SPLIT_OUT: the boundary leaves in the blocked hi/lo encoding
// (cifar_split_blocked_kernel) that cifar_fc1_x3_kernel<true> stages by DMA.
// C2: conv2 consumer path.  0: v_mfma_f32_32x32x16_bf16 (32x8-pixel M tiles);
// 1: v_mfma_f32_16x16x32_bf16 (4x4-pixel M tiles, 16-B stores only), the default:
// the same MFMA cycles, a higher clock held under load (docs/ARCHITECTURE.md §2).
// IN = 1, "uint8 input" (C1 = 1 only): x is the image as it exists, (B,32,32,3) bytes, and the
// normalisation is a table lookup in the producer.  The channel-packed plane of a row is the
// byte order of an HWC row (element 3x + c <-> byte 3x + c), so the 12 bytes a thread loads are
// its 12 plane elements in order and the channel of byte i is i % 3.  The table sits in LDS
// behind the planes (3,072 B, outside the zeroed region, complete before the barrier that ends
// the zeroing); an entry already holds the hi and lo halves of split2<true>, so the planes are
// bit-identical to those of IN = 0 fed the normalised floats and everything after them is the
// same code.  Per thread and image: 3 dword loads instead of 3 float4, 12 ds_read_b32 (issued
// together) and 12 v_perm_b32 instead of 6 split2.
template <bool WIDE, bool SPLIT_OUT, int C2 = 0, int C1 = 0, int IN = 0>
__global__ __launch_bounds__(512, 1) void cifar_stage0_x3_kernel(
    s0_input_t<IN> x, float* __restrict__ out, const bf16_t* __restrict__ w1h,
    const bf16_t* __restrict__ w1l, const float* __restrict__ b1, const bf16_t* __restrict__ w2h,
    const bf16_t* __restrict__ w2l, const float* __restrict__ b2, int B) {
  static_assert(IN == 0 || C1 == 1, "uint8 input exists in the K = 32 producer only");
  constexpr int LDS_BYTES = lds_bytes<C1>();
  __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES + (IN ? TAB_BYTES : 0)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool producer = wave < 4;
  const int rw = wave & 3;
  const int rt = tid & 255;
  const int h = lane >> 5, r32 = lane & 31;
  const int n = B > (int)blockIdx.x ? (B - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;

  // every halo (input and pooled map) is zero for the whole launch; interiors are rewritten per image
  for (int i = tid; i < LDS_BYTES / 16; i += 512) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
  if constexpr (IN == 1)
    for (int i = tid; i < TAB_BYTES / 4; i += 512) reinterpret_cast<uint32_t*>(smem + LDS_BYTES)[i] = x.table[i];

  __syncthreads();  // halos zeroed (and the table in place) before any image is staged

  // The two roles run disjoint loops (wave-uniform branch, the same number of
  // barriers on both sides) so their resident operands never share live ranges:
  // producers hold conv1's split weights + the input prefetch, consumers the
  // 144 VGPRs of conv2's split weights.
  if (producer) {
    const float bias = b1[r32];
    asm volatile("" ::"v"(bias));
    const int q = ((r32 & 1) ? 2 : 0) + ((r32 & 2) ? 1 : 0);
    const int cb = r32 & ~3;

    // The pooled-map store offset of a lane is (Y*18 + X)*64 + (((cb>>3) ^ swizzle(Y)) << 4) + 2*(cb&7) at
    // pooled pixel (Y, X) = (Y0 + (q>>1), X0 + (q&1) + xh), Y0 = 2*ty + 1.  a1_lane(par, xh) is its
    // lane part, computed once, for tiles whose row index ty has parity par (the chunk XOR depends on
    // ty through that parity only); the rest, (Y0*18 + X0)*64 and the slot, is wave-uniform.
    auto a1_lane = [&](int par, int xh) {
      const int Y = 2 * par + 1 + (q >> 1);
      return ((q >> 1) * 18 + (q & 1) + xh) * 64 + ((((cb >> 3) ^ a1_swz<C2>(Y))) << 4) + (cb & 7) * 2;
    };
    // v = bias + ReLU + 2x2 max-pool of the lane's 2x2 pooled pixels of channel r32: quad-DPP gather
    // of 4 channels of one pooled pixel per lane, hi/lo split, one 8-B store per plane at
    // ob = a1_lane + the hi plane of the slot + the uniform (Y0*18 + X0)*64 of the call
    auto conv1_store = [&](const float (&v)[4], int ob) {
      const bool odd = r32 & 1;
      const int s0 = __float_as_int(odd ? v[0] : v[2]), s1 = __float_as_int(odd ? v[1] : v[3]);
      const float r0 = __int_as_float(dpp_xor1(s0)), r1 = __int_as_float(dpp_xor1(s1));
      uint32_t u0h, u0l, u1h, u1l;
      // even lane: (v[0], r0), (v[1], r1); odd lane: (r0, v[2]), (r1, v[3]).  The operands are
      // selected and each pair split once: a branch on the lane's parity runs both sides of the
      // split one after the other
      const float k0 = odd ? v[2] : v[0], k1 = odd ? v[3] : v[1];
      split2<true>(odd ? r0 : k0, odd ? k0 : r0, u0h, u0l);
      split2<true>(odd ? r1 : k1, odd ? k1 : r1, u1h, u1l);
      const bool hi2 = r32 & 2;
      const uint32_t rch = (uint32_t)dpp_xor2((int)(hi2 ? u0h : u1h));
      const uint32_t rcl = (uint32_t)dpp_xor2((int)(hi2 ? u0l : u1l));
      const uint32_t mh = hi2 ? u1h : u0h, ml = hi2 ? u1l : u0l;
      uint2 wh, wl;
      wh.x = hi2 ? rch : mh;
      wh.y = hi2 ? mh : rch;
      wl.x = hi2 ? rcl : ml;
      wl.y = hi2 ? ml : rcl;
      *reinterpret_cast<uint2*>(smem + ob) = wh;
      *reinterpret_cast<uint2*>(smem + ob + A1PL) = wl;
    };
    // one barrier per image: conv1 of image it, then staging of image it+1 from the prefetch registers
    auto produce = [&](auto&& load_img, auto&& stage_img, auto&& conv1_img) {
      if (n > 0) {
        load_img(0);
        stage_img(0);
        if (n > 1) load_img(1);
      }
      __syncthreads();
      for (int it = 0; it <= n; ++it) {
        if (it < n) {
          conv1_img(it);
          if (it + 1 < n) {
            stage_img(it + 1);
            if (it + 2 < n) load_img(it + 2);
          }
        }
        __syncthreads();
      }
    };

    if constexpr (C1 == 0 && IN == 0) {
      bf16x8 w1hf[3], w1lf[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        w1hf[s] = *reinterpret_cast<const bf16x8*>(w1h + r32 * 48 + s * 16 + h * 8);
        w1lf[s] = *reinterpret_cast<const bf16x8*>(w1l + r32 * 48 + s * 16 + h * 8);
      }
      resident_fence(w1hf);
      resident_fence(w1lf);

      float pf[4][3];
      // a buffer descriptor over image k alone (scalar arithmetic), one lane offset for the kernel
      auto load_img = [&](int k) {
        const float* xb = x + (size_t)(blockIdx.x + (size_t)k * gridDim.x) * 3072;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            pf[i][c] = __uint_as_float(buf_load4(xb, 12288, 4 * rt, 4 * (c * 1024 + 256 * i)));
      };
      auto stage_img = [&](int k) {  // prefetch registers -> padded HWC4 hi / lo planes
        char* xh = smem + xin_off<C1>(k, 0);
        char* xl = smem + xin_off<C1>(k, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = rt + 256 * i, yy = p >> 5, xx = p & 31;
          uint2 vh, vl;
          split2<true>(pf[i][0], pf[i][1], vh.x, vl.x);
          split2<true>(pf[i][2], 0.f, vh.y, vl.y);
          const int o = ((yy + 1) * XW + xx + 1) * 8;
          *reinterpret_cast<uint2*>(xh + o) = vh;
          *reinterpret_cast<uint2*>(xl + o) = vl;
        }
      };
      const int c1_lane = ((r32 >> 3) * XW + (r32 & 7) + 2 * h) * 8;

      // bias + ReLU + 2x2 max-pool in registers (max(a)+b == max(a+b) exactly)
      // tile t = rw + 8 j has an even row index ty = 2 j, its pair partner t + 4 the odd 2 j + 1
      const int a1l[2] = {a1_lane(0, 2 * h), a1_lane(1, 2 * h)};
      auto conv1_epi = [&](int t, const f32x16& acc, int k, int par) {
        const int ty = t >> 2, tx = t & 3;
        float v[4];
#pragma unroll
        for (int qy = 0; qy < 2; ++qy)
#pragma unroll
          for (int qx = 0; qx < 2; ++qx) {
            const int g0 = (2 * qy) * 4 + 2 * qx;
            v[qy * 2 + qx] =
                fmaxf(fmax_nan(fmax_nan(acc[g0], acc[g0 + 1]), fmax_nan(acc[g0 + 4], acc[g0 + 5])) + bias, 0.f);
          }
        conv1_store(v, a1l[par] + a1_off<C1>(k, 0) + ((2 * ty + 1) * 18 + 4 * tx + 1) * 64);
      };
      auto frag = [&](const char* p) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        const uint2 b = *reinterpret_cast<const uint2*>(p + 8);
        return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
      };
      // two conv1 tiles at once: all 24 A-fragment reads up front, two accumulation chains interleaved
      auto conv1_pair = [&](int ta, int tb, int k) {
        const char* xh = smem + xin_off<C1>(k, 0);
        const int oa = c1_lane + ((4 * (ta >> 2)) * XW + 8 * (ta & 3)) * 8;
        const int ob = c1_lane + ((4 * (tb >> 2)) * XW + 8 * (tb & 3)) * 8;
        bf16x8 fah[3], fal[3], fbh[3], fbl[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          fah[s] = frag(xh + oa + s * XW * 8);
          fbh[s] = frag(xh + ob + s * XW * 8);
          fal[s] = frag(xh + XPL + oa + s * XW * 8);
          fbl[s] = frag(xh + XPL + ob + s * XW * 8);
        }
        f32x16 acca = {}, accb = {};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[s], w1hf[s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fbh[s], w1hf[s], accb, 0, 0, 0);
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[s], w1lf[s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fbh[s], w1lf[s], accb, 0, 0, 0);
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal[s], w1hf[s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fbl[s], w1hf[s], accb, 0, 0, 0);
        }
        conv1_epi(ta, acca, k, 0);
        conv1_epi(tb, accb, k, 1);
      };
      produce(load_img, stage_img, [&](int it) {
#pragma unroll 1
        for (int t = rw; t < 32; t += 8) conv1_pair(t, t + 4, it);
      });
    } else if constexpr (C1 == 1) {
      // conv1 with the 27 taps in K = 32 (see "conv1 on K = 32" in the header): per x parity a
      // resident weight set [par][k-step], B-operand k = 16*s + 8*h + 0..7
      bf16x8 w1hf[2][2], w1lf[2][2];
#pragma unroll
      for (int par = 0; par < 2; ++par)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          w1hf[par][s] = *reinterpret_cast<const bf16x8*>(w1h + par * 1024 + r32 * 32 + s * 16 + h * 8);
          w1lf[par][s] = *reinterpret_cast<const bf16x8*>(w1l + par * 1024 + r32 * 32 + s * 16 + h * 8);
        }
      resident_fence(w1hf[0]);
      resident_fence(w1hf[1]);
      resident_fence(w1lf[0]);
      resident_fence(w1lf[1]);

      // a thread stages pixels 4j..4j+3 of one row: 12 contiguous bf16 per plane from element
      // 12j + 4 (8-B aligned).  16 contiguous lanes take rows y and y + 2 (24 dwords mod 32
      // apart would collide, 48 do not): conflict-free ds_write_b64
      const int sj = rt & 7, r5 = rt >> 3;
      const int sy = (r5 & ~3) | ((r5 & 1) << 1) | ((r5 >> 1) & 1);
      // the input prefetch: three float4 (IN = 0) or three dwords of bytes (IN = 1)
      std::conditional_t<IN == 1, uint32_t, float4> pf[3];
      // Loads go through a buffer descriptor over image k alone: its base is scalar arithmetic (no
      // 32-bit limit on the batch), the lane's offset inside an image is computed once, and nothing
      // per lane is 64-bit.  The image index is in range by construction (k < n), and a lane's
      // bytes end at the image's last byte at most.
      // IN = 1: bytes 12 sj .. 12 sj + 11 of row sy: pixels 4 sj .. 4 sj + 3, HWC
      const int ld_lane = IN == 1 ? sy * 96 + sj * 12 : (sy * 32 + sj * 4) * 4;
      auto load_img = [&](int k) {
        if constexpr (IN == 1) {
          const unsigned char* xb = x.x + (size_t)(blockIdx.x + (size_t)k * gridDim.x) * 3072;
#pragma unroll
          for (int c = 0; c < 3; ++c) pf[c] = buf_load4(xb, 3072, ld_lane, 4 * c);
        } else {
          const float* xb = x + (size_t)(blockIdx.x + (size_t)k * gridDim.x) * 3072;
#pragma unroll
          for (int c = 0; c < 3; ++c) pf[c] = buf_load16(xb, 12288, ld_lane, c * 4096);
        }
      };
      auto stage_img = [&](int k) {  // prefetch registers -> padded channel-packed hi / lo planes
        const int o = (sy + 1) * XP32 + 8 + 24 * sj;
        char* xh = smem + xin_off<C1>(k, 0) + o;
        char* xl = smem + xin_off<C1>(k, 1) + o;
        uint2 vh[3], vl[3];
        if constexpr (IN == 1) {
          // byte i is plane element i, channel i % 3: all 12 table reads first, then per pair of
          // entries the hi dword (the two low halves) and the lo dword (the two high halves)
          const char* tab = smem + LDS_BYTES;
          uint32_t e[12];
#pragma unroll
          for (int i = 0; i < 12; ++i)
            e[i] = *reinterpret_cast<const uint32_t*>(tab + (i % 3) * 1024 + ((pf[i >> 2] >> (8 * (i & 3))) & 0xffu) * 4);
          uint32_t ph[6], pl[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            ph[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x05040100u);
            pl[i] = __builtin_amdgcn_perm(e[2 * i + 1], e[2 * i], 0x07060302u);
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            vh[i] = make_uint2(ph[2 * i], ph[2 * i + 1]);
            vl[i] = make_uint2(pl[2 * i], pl[2 * i + 1]);
          }
        } else {
          split2<true>(pf[0].x, pf[1].x, vh[0].x, vl[0].x);
          split2<true>(pf[2].x, pf[0].y, vh[0].y, vl[0].y);
          split2<true>(pf[1].y, pf[2].y, vh[1].x, vl[1].x);
          split2<true>(pf[0].z, pf[1].z, vh[1].y, vl[1].y);
          split2<true>(pf[2].z, pf[0].w, vh[2].x, vl[2].x);
          split2<true>(pf[1].w, pf[2].w, vh[2].y, vl[2].y);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          *reinterpret_cast<uint2*>(xh + 8 * i) = vh[i];
          *reinterpret_cast<uint2*>(xl + 8 * i) = vl[i];
        }
      };
      // lane (pixel row rr, column index c of the tile; K half h): k-step 0 reads dwords 0-3
      // of padded row rr + 2h, k-step 1 dwords 0-3 of row rr + 1 (h = 0) or dword 4 of rows
      // rr, rr + 1, rr + 2 and a repeat of the last as filler (h = 1)
      const int rr = r32 >> 3, cc = r32 & 7;
      const int l0 = (rr + 2 * h) * XP32 + 12 * cc;
      int l1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        l1[i] = h ? (rr + (i < 2 ? i : 2)) * XP32 + 12 * cc + 16 : (rr + 1) * XP32 + 12 * cc + 4 * i;
      auto ld32 = [&](const char* p) { return *reinterpret_cast<const uint32_t*>(p); };
      // a wave's tile pairs tp = rw + 4 j all have row indices ty = (rw >> 1) + 2 j of one parity
      const int a1l = a1_lane((rw >> 1) & 1, 4 * h);
      // the even and the odd tile of 4 rows x 16 columns: 32 dword reads up front, two
      // accumulation chains interleaved, the 2x2 pool across the two accumulators
      auto conv1_pair = [&](int tp, int k) {
        const int ty = tp >> 1, tx2 = tp & 1;
        const char* xh = smem + xin_off<C1>(k, 0) + 4 * ty * XP32 + 96 * tx2;
        bf16x8 f[2][2][2];  // [x parity][hi, lo][k-step]
#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
          for (int pl = 0; pl < 2; ++pl) {
            const char* p = xh + pl * XPL32 + 8 * par;
            f[par][pl][0] = __builtin_bit_cast(
                bf16x8, make_uint4(ld32(p + l0), ld32(p + l0 + 4), ld32(p + l0 + 8), ld32(p + l0 + 12)));
            f[par][pl][1] = __builtin_bit_cast(
                bf16x8, make_uint4(ld32(p + l1[0]), ld32(p + l1[1]), ld32(p + l1[2]), ld32(p + l1[3])));
          }
        f32x16 acca = {}, accb = {};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[0][0][s], w1hf[0][s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[1][0][s], w1hf[1][s], accb, 0, 0, 0);
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[0][0][s], w1lf[0][s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[1][0][s], w1lf[1][s], accb, 0, 0, 0);
          acca = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[0][1][s], w1hf[0][s], acca, 0, 0, 0);
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[1][1][s], w1hf[1][s], accb, 0, 0, 0);
        }
        // accumulator g of both tiles: pixel row 2*qy + ((g >> 2) & 1), column index (g & 3) + 4h
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          float v[4];
#pragma unroll
          for (int qy = 0; qy < 2; ++qy)
#pragma unroll
            for (int qx = 0; qx < 2; ++qx) {
              const int g = 8 * qy + 2 * e + qx;
              v[qy * 2 + qx] =
                  fmaxf(fmax_nan(fmax_nan(acca[g], accb[g]), fmax_nan(acca[g + 4], accb[g + 4])) + bias, 0.f);
            }
          conv1_store(v, a1l + a1_off<C1>(k, 0) + ((2 * ty + 1) * 18 + 8 * tx2 + 2 * e + 1) * 64);
        }
      };
      produce(load_img, stage_img, [&](int it) {
#pragma unroll 1
        for (int tp = rw; tp < 16; tp += 4) conv1_pair(tp, it);
      });
    }
  } else if constexpr (C2 != 0) {
    const int m = lane & 15, q16 = lane >> 4, y1 = q16 >> 1, x1 = q16 & 1;
    const int oc = (rw & 1) * 32 + m;  // N tile nt: oc + 16*nt
    bf16x8 w2hf[2][9], w2lf[2][9];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        w2hf[nt][tap] = *reinterpret_cast<const bf16x8*>(w2h + (oc + 16 * nt) * 288 + tap * 32 + q16 * 8);
        w2lf[nt][tap] = *reinterpret_cast<const bf16x8*>(w2l + (oc + 16 * nt) * 288 + tap * 32 + q16 * 8);
      }
    const float bias0 = b2[oc], bias1 = b2[oc + 16];
    resident_fence(w2hf[0]);
    resident_fence(w2hf[1]);
    resident_fence(w2lf[0]);
    resident_fence(w2lf[1]);
    asm volatile("" ::"v"(bias0), "v"(bias1));
    // lane base per parity of ky: pixel (py, px) of the 4x4 block, chunk q16 ^ swizzle of row
    // Y = 4*ty2 + py + ky (4*ty2 even: the XOR depends on the parity of py + ky only)
    const int py = 2 * (m >> 3) + ((m >> 1) & 1), px = 2 * ((m >> 2) & 1) + (m & 1);
    uint32_t lb[2];
#pragma unroll
    for (int kyp = 0; kyp < 2; ++kyp) lb[kyp] = (uint32_t)((py * 18 + px) * 64 + ((q16 ^ a1_swz<C2>(py + kyp)) << 4));

    // the lane's byte offset inside an image's boundary at band 0 and N tile 0 (m16_epilogue)
    const int st_lane = SPLIT_OUT ? (oc * 2 + (rw >> 1)) * 128 + (y1 * 8 + 4 * x1) * 2
                                  : (oc * 64 + ((rw >> 1) * 4 + y1) * 8 + 4 * x1) * 4;
    auto conv2_img = [&](int k) {  // conv2 + bias + ReLU + pool of image k -> out
      float* img = out + (size_t)(blockIdx.x + (size_t)k * gridDim.x) * 4096;
      const uint32_t plane = (uint32_t)(uintptr_t)(smem + a1_off<C1>(k, 0));
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int ty2 = (rw >> 1) * 2 + p;
        const uint32_t rb = plane + ty2 * 4 * 18 * 64;
        const uint32_t b[2] = {rb + lb[0], rb + lb[1]};
        f32x4 acc[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = f32x4{};
        bf16x8 a0[4], a1[4];
        __builtin_amdgcn_s_setprio(1);  // back to 0 inside m16_step<C2_PRIO_STEPS>
        m16_issue<0>(b, a0);
        m16_step<0>(b, w2hf, w2lf, acc, a0, a1);
        m16_epilogue<SPLIT_OUT, 0>(acc, bias0, img, st_lane, p);
        m16_epilogue<SPLIT_OUT, 1>(acc, bias1, img, st_lane, p);
      }
    };

    __syncthreads();
    for (int it = 0; it <= n; ++it) {
      if (it >= 1) conv2_img(it - 1);
      __syncthreads();
    }
  } else {
    const int oc2 = (rw & 1) * 32 + r32;
    bf16x8 w2hf[18], w2lf[18];
#pragma unroll
    for (int s = 0; s < 18; ++s) {
      w2hf[s] = *reinterpret_cast<const bf16x8*>(w2h + oc2 * 288 + s * 16 + h * 8);
      w2lf[s] = *reinterpret_cast<const bf16x8*>(w2l + oc2 * 288 + s * 16 + h * 8);
    }
    const float bias = b2[oc2];
    resident_fence(w2hf);
    resident_fence(w2lf);
    asm volatile("" ::"v"(bias));
    // lane base for (ky, channel-chunk parity): pixel row Y = 4*ty2 + (r32>>3) + ky,
    // Y & 3 = ((r32>>3) + ky) & 3 (4*ty2 = 0 mod 4), chunk = 2*par + h
    uint32_t lb[3][2];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const int yr = (r32 >> 3) + ky;
        lb[ky][par] = (uint32_t)((yr * 18 + (r32 & 7)) * 64 + (((2 * par + h) ^ (yr & 3)) << 4));
      }

    auto conv2_img = [&](int k) {  // conv2 + bias + ReLU + pool of image k -> out (fp32, NCHW flatten)
      float* ob = out + (size_t)(blockIdx.x + (size_t)k * gridDim.x) * 4096 + oc2 * 64;
      const uint32_t plane = (uint32_t)(uintptr_t)(smem + a1_off<C1>(k, 0));
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int ty2 = (rw >> 1) * 2 + p;
        const uint32_t rb = plane + ty2 * 4 * 18 * 64;
        uint32_t b[3][2];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int par = 0; par < 2; ++par) b[ky][par] = rb + lb[ky][par];
        f32x16 acc[2] = {f32x16{}, f32x16{}};
        bf16x8 a0[4], a1[4];
        __builtin_amdgcn_s_setprio(1);  // back to 0 inside c2_step<C2_PRIO_STEPS>
        c2_issue<0>(b, a0);
        c2_step<0>(b, w2hf, w2lf, acc, a0, a1);
        if constexpr (WIDE) {
          // 16-B stores: lane half h holds pooled columns 4i+2h..+1 of both
          // tiles; one v_permlane32_swap per dword gives half 0 columns 0-3
          // (its own tile-0 pair + the other half's) and half 1 columns 4-7,
          // so a row leaves as one dwordx4 per lane instead of two dwordx2
#pragma unroll
          for (int qy = 0; qy < 2; ++qy) {
            const int g0 = (2 * qy) * 4;
            float v[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              v[i][0] = fmaxf(fmax_nan(fmax_nan(acc[i][g0], acc[i][g0 + 1]), fmax_nan(acc[i][g0 + 4], acc[i][g0 + 5])) + bias, 0.f);
              v[i][1] = fmaxf(fmax_nan(fmax_nan(acc[i][g0 + 2], acc[i][g0 + 3]), fmax_nan(acc[i][g0 + 6], acc[i][g0 + 7])) + bias,
                              0.f);
            }
            const auto sx = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0][0]), __float_as_uint(v[1][0]), false,
                                                             false);
            const auto sy = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[0][1]), __float_as_uint(v[1][1]), false,
                                                             false);
            const int PY = 2 * ty2 + qy;
            if constexpr (SPLIT_OUT) {  // k = oc2*64 + PY*8 + 4h + 0..3: one 8-B hi and one 8-B lo store
              uint2 hi, lo;
              split2<true>(__uint_as_float(sx[0]), __uint_as_float(sy[0]), hi.x, lo.x);
              split2<true>(__uint_as_float(sx[1]), __uint_as_float(sy[1]), hi.y, lo.y);
              char* bp = reinterpret_cast<char*>(ob - oc2 * 64) + (oc2 * 2 + (PY >> 2)) * 128 + ((PY & 3) * 8 + 4 * h) * 2;
              *reinterpret_cast<uint2*>(bp) = hi;
              *reinterpret_cast<uint2*>(bp + 64) = lo;
            } else {
              *reinterpret_cast<uint4*>(ob + PY * 8 + 4 * h) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
            }
          }
        } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int qy = 0; qy < 2; ++qy) {
            float2 pv;
            const int g0 = (2 * qy) * 4;
            pv.x = fmaxf(fmax_nan(fmax_nan(acc[i][g0], acc[i][g0 + 1]), fmax_nan(acc[i][g0 + 4], acc[i][g0 + 5])) + bias, 0.f);
            pv.y = fmaxf(fmax_nan(fmax_nan(acc[i][g0 + 2], acc[i][g0 + 3]), fmax_nan(acc[i][g0 + 6], acc[i][g0 + 7])) + bias,
                         0.f);
            const int PY = 2 * ty2 + qy, PX = 4 * i + 2 * h;
            if constexpr (SPLIT_OUT) {
              uint32_t hi, lo;
              split2<true>(pv.x, pv.y, hi, lo);
              char* bp = reinterpret_cast<char*>(ob - oc2 * 64) + (oc2 * 2 + (PY >> 2)) * 128 + ((PY & 3) * 8 + PX) * 2;
              *reinterpret_cast<uint32_t*>(bp) = hi;
              *reinterpret_cast<uint32_t*>(bp + 64) = lo;
            } else {
              *reinterpret_cast<float2*>(ob + PY * 8 + PX) = pv;
            }
          }
        }
        }
      }
    };

    __syncthreads();
    for (int it = 0; it <= n; ++it) {
      if (it >= 1) conv2_img(it - 1);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------
// fc1 at fp32 precision: C = relu(A . W^T + bias), A fp32 [M][K], W = W_hi + W_lo
// (bf16 [N][K] each), C fp32.  A is read from HBM once per tile pair as fp32 and
// split in registers (global_load_dwordx4 -> split2 -> ds_write_b128) while the
// W halves stream into LDS by DMA (global_load_lds, source-side swizzle).  LDS:
// 2 buffers x [A_hi A_lo W_hi W_lo] planes of 256 rows x 32 k (64-B rows, 16 KiB)
// = 128 KiB.  The 16-B chunk c of row r is stored at c ^ ((r >> 2) & 2): the
// four ds_read_b128 lane groups ({0-3,12-15,20-27}, ...) of a fragment read
// (lane: row l & 15, chunk l >> 4) then hit 16 distinct slots, and the A
// writes (8 contiguous lanes = 2 rows x 4 chunks) 8 distinct ds_write slots.
// The k loop's schedule (two wave groups half a k-step apart) is described at
// the kernel.
// ---------------------------------------------------------------------------
constexpr int F1_T = 256, F1_K = 32, F1_PLANE = 256 * 64;

__device__ __forceinline__ int f1_swz(int r) { return (r >> 2) & 2; }

__device__ __forceinline__ bf16x8 f1_frag(const char* plane, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(plane + row * 64 + ((chunk ^ f1_swz(row)) << 4));
}

__device__ __forceinline__ void f1_tile_coords(int logical, int ntm, int ntn, int& tm, int& tn) {
  // M fastest inside groups of 8 M-tiles: the ntn column tiles of one A panel
  // run close together on one XCD, so A's second read hits L2 / MALL
  constexpr int G = 8;
  const int per = G * ntn, grp = logical / per, first = grp * G;
  const int gm = min(ntm - first, G), r = logical - grp * per;
  tm = first + r % gm;
  tn = r / gm;
}

// A goes to registers one k-step ahead.  Measured alternatives, dropped: A by
// DMA into a 32 KiB fp32 staging area two k-steps ahead (5 % slower), the
// split+store between the two MFMA halves (flat), a second register set for A
// two k-steps ahead once the loads were coalesced (flat, 6 spilled VGPRs).  Probes
// (profiles/archive/r2_cifar_fc1_probes.jsonl): without the A stream the kernel runs
// 0.51 ms, without any load 0.45 ms (1.8 PF/s), with both 0.80 ms.  On the
// staggered schedule (profiles/cifar_fc1_sched_ab.jsonl): s_setprio 1 around
// the MFMA segment and static s_setprio 1 for waves 4-7 both lost 0.4-0.5 %;
// the bias in registers with a branch-free store path for full tiles was
// -0.75 % with overlapping rounds: dropped.
//
// SPLIT_IN: A arrives pre-split in the blocked boundary encoding (see
// cifar_split_blocked_kernel: per row and 32-k block, 32 bf16 hi then 32 bf16
// lo — the same 4 bytes per element as fp32, the same hi/lo this kernel would
// form in registers), so A is staged by DMA exactly like W: no VGPR round
// trip, no split ALU, no vmcnt stall on A inside the k loop.
//
// Schedule.  With all eight waves reading their fragments, multiplying and
// restaging at the same time (one barrier per k-step), a SIMD's matrix pipe
// idles while both of its waves read or split: every interleaved round slower,
// with bitwise the same outputs (profiles/cifar_fc1_sched_ab.jsonl,
// profiles/cifar_fc1_sched_after.md).  So group 0 (waves
// 0-3, rows 0-127 of the tile) and group 1 (waves 4-7) run half a k-step apart:
// a k-step is two segments between s_barriers, and in each segment one wave of
// every SIMD issues its 96 MFMAs from 24 fragments already in registers while
// its partner runs its load segment (split + ds_write of its share of A(t+1),
// its global loads, the 24 ds_read_b128 of its next MFMA segment).  Segment s:
//     s = 2t      group 0: load segment of step t     group 1: MFMAs of step t-1
//     s = 2t + 1  group 0: MFMAs of step t            group 1: load segment of step t
// Buffer (t+1)&1 is last read (step t-1) in segment 2t-1 and first read (step
// t+1) in segment 2t+2, so everything that writes it goes into segments 2t and
// 2t+1: both groups issue its DMAs in segment 2t (group 1 ahead of its MFMAs)
// and retire them with a counted vmcnt before the barrier that ends segment
// 2t+1; group 0 writes its A rows in segment 2t, group 1 in segment 2t+1, each
// behind the lgkmcnt(0) of the segment's barrier.  The A registers are loaded
// two segments ahead of their split, right after the previous split frees them,
// and after the step's DMAs in program order, so vmcnt(4) retires the DMAs and
// leaves the A loads in flight.  Every wave passes 1 + 2 nk barriers for any
// nk >= 1: group 0 ends with the barrier after its last MFMAs and goes to its
// epilogue while group 1 runs its last MFMA segment.  Each accumulator sees its
// MFMAs in k order, W_hi A_hi, W_lo A_hi, W_hi A_lo per k-step, in both groups.
//
// LEAN: the same segments, barriers, counted vmcnt and MFMA order,
// with what a load segment issues next to its partner's MFMAs cut to the split
// itself.  The staggered arm rebuilds every row pointer and LDS offset per
// segment (64-bit per-lane arithmetic, ~85 VALU per k-step) because it has no
// VGPRs to keep them; none of it depends on the k-step except through a
// wave-uniform offset.  Here A, W and (SPLIT_IN) the blocked A go through buffer
// descriptors built from block-uniform values (buf_load16 / buf_glds16): one
// loop-invariant 32-bit lane offset per stream, the k-step, the hi / lo half
// and the 16-row piece in the scalar offset.  The A ds_write address and the
// A / W fragment ds_read_b128 addresses are one VGPR base each plus immediates;
// the buffer toggle is 65536 B, one past the largest ds immediate, so it is one
// v_add per base and segment.  Five persistent VGPRs replace the recomputation
// (256 VGPRs, no scratch, as before).  Rows past M: instead of the clamp to
// row M - 1 the descriptors end with the tile's last valid row (fp32 A: four
// descriptors of 64 rows, one per piece, since the piece offset must not ride
// in the scalar offset, which the check may not cover; blocked A: one descriptor, the row in the
// lane offset), so such a row is dropped by the range check, reads as zero and
// is never stored.  split2<true> converts each pair with one
// v_cvt_pk_bf16_f32: the same instruction and rounding on the same values, so
// the outputs are bitwise those of the other arm.  Measured in
// profiles/cifar_lean_after.md: fc1 0.646 -> 0.572 ms interleaved, every round.
template <bool SPLIT_IN, bool LEAN>
__global__ __launch_bounds__(512, 1) void cifar_fc1_x3_kernel(const float* __restrict__ A, int lda,
                                                              const bf16_t* __restrict__ Wh,
                                                              const bf16_t* __restrict__ Wl, int ldw,
                                                              const float* __restrict__ bias, float* __restrict__ C,
                                                              int ldc, int M, int N, int K) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * 4 * F1_PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntn = N / F1_T, ntm = (M + F1_T - 1) / F1_T;
  int tm, tn;
  f1_tile_coords(xcd_remap(blockIdx.x, ntm * ntn), ntm, ntn, tm, tn);
  const int m0 = tm * F1_T, n0 = tn * F1_T;
  const int wr = wave >> 2, wc = wave & 3;
  const int nk = K / F1_K;
  auto plane = [&](int u, int p) { return smem + (u * 4 + p) * F1_PLANE; };  // p: 0 A_hi, 1 A_lo, 2 W_hi, 3 W_lo

  // A: 2 chunks (8 fp32 each) per thread; chunk q = tid + 512 i -> row q >> 2, k-chunk q & 3
  // A: 4 pieces of 16 B per thread; piece k: row (tid >> 3) + 64 k, floats
  // 4 (tid & 7) .. +3, so every wave load instruction reads 8 whole 128-B row
  // segments and the split halves land as ds_write_b64 into half of a 16-B LDS
  // chunk.  (The first mapping, 32 contiguous bytes per lane in two loads,
  // touched every 128-B line twice per wave: 0.85 -> 0.68 ms.)
  // The staging lambdas take their lane addressing from ``ltid`` (= tid).  The
  // staggered loop hands them a fresh opaque copy per segment (fresh_tid), so
  // the row pointers and LDS offsets are recomputed under the partner's MFMAs
  // instead of living in VGPRs across the loop: 128 accumulators + 96 fragment
  // registers + 16 of A in flight leave 16 for everything else at 2 waves/SIMD.
  int ltid = tid;
  float4 ar[4];
  // LEAN addressing (see above the kernel): descriptors from block-uniform
  // values, one 32-bit lane offset per stream, one LDS base per access kind.
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  // fp32 A, piece k (rows m0 + 64 k ..+63): the records end with row M - 1, so
  // a row past M is dropped by the range check (reads as 0, is never stored)
  // (readfirstlane: the clamp compiles to v_med3_i32, and a record count in a
  // VGPR would put a waterfall loop around every load)
  int a_rows[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) a_rows[k] = __builtin_amdgcn_readfirstlane(max(min(M - m0 - 64 * k, 64), 0));
  // blocked A (SPLIT_IN): the tile's rows in one descriptor, the row in the lane offset
  const float* const a_tile = A + (size_t)m0 * lda;
  const int a_tile_bytes = min(M - m0, F1_T) * lda * 4;
  // DMA lane offset: row wave * 32 + (lane >> 2) of pitch ld bytes, swizzled 16-B chunk (piece j: + 16 rows)
  auto dma_voff = [&](int ld_bytes) {
    return (wave * 32 + (lane >> 2)) * ld_bytes + (((lane & 3) ^ ((lane >> 4) & 2)) << 4);
  };
  int a_voff = 0, a_voff1 = 0, w_voff = 0;
  LDS_AS char* aw_base = nullptr;
  LDS_AS char* fa_base = nullptr;
  LDS_AS char* fw_base = nullptr;
  if constexpr (LEAN) {
    LDS_AS char* const lds = (LDS_AS char*)smem;
    const int fr = lane & 15, fc = lane >> 4;
    const int fo = fr * 64 + ((fc ^ ((fr >> 2) & 2)) << 4);  // f1_frag's row fr, chunk fc
    fa_base = lds + (wave >> 2) * 128 * 64 + fo;
    fw_base = lds + 2 * F1_PLANE + (wave & 3) * 64 * 64 + fo;
    w_voff = dma_voff(ldw * 2);
    if constexpr (SPLIT_IN) {
      a_voff = dma_voff(lda * 4);
      a_voff1 = a_voff + 16 * lda * 4;
      asm volatile("" : "+v"(a_voff1));
    } else {
      const int r = tid >> 3, c = (tid & 7) >> 1, half = tid & 1;
      a_voff = r * lda * 4 + (tid & 7) * 16;
      aw_base = lds + r * 64 + ((c ^ f1_swz(r)) << 4) + half * 8;
      asm volatile("" : "+v"(aw_base));
    }
    asm volatile("" : "+v"(a_voff), "+v"(w_voff), "+v"(fa_base), "+v"(fw_base));
  }
  constexpr int F1_BUF = 4 * F1_PLANE;  // 65536: one past the largest ds_* immediate
  auto load_a = [&](int t, auto) {
    if constexpr (LEAN) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        ar[k] = buf_load16(A + (size_t)(m0 + 64 * k) * lda, a_rows[k] * lda * 4, a_voff, t * 128);
      return;
    }
    const int x = ltid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = min(m0 + (x >> 3) + 64 * k, M - 1);
      ar[k] = *reinterpret_cast<const float4*>(A + (size_t)row * lda + t * F1_K + (x & 7) * 4);
    }
  };
  auto store_a = [&](int u, auto) {
    if constexpr (LEAN) {
      LDS_AS char* const w = aw_base + u * F1_BUF;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint2 hi, lo;
        split2<true>(ar[k].x, ar[k].y, hi.x, lo.x);
        split2<true>(ar[k].z, ar[k].w, hi.y, lo.y);
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<LDS_AS u32x2*>(w + k * 4096) = u32x2{hi.x, hi.y};
        *reinterpret_cast<LDS_AS u32x2*>(w + F1_PLANE + k * 4096) = u32x2{lo.x, lo.y};
      }
      return;
    }
    const int x = ltid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = (x >> 3) + 64 * k, c = (x & 7) >> 1, half = x & 1;
      uint2 hi, lo;
      split2<false>(ar[k].x, ar[k].y, hi.x, lo.x);
      split2<false>(ar[k].z, ar[k].w, hi.y, lo.y);
      const int o = r * 64 + ((c ^ f1_swz(r)) << 4) + half * 8;
      *reinterpret_cast<uint2*>(plane(u, 0) + o) = hi;
      *reinterpret_cast<uint2*>(plane(u, 1) + o) = lo;
    }
  };
  // W: per plane 16 pieces of 16 rows (1 KiB per wave instruction), 2 per wave
  // SPLIT_IN: A hi / lo planes by DMA, 2 pieces of 16 rows per wave and plane (as W)
  auto stage_a = [&](int u, int t) {
    if constexpr (LEAN) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          buf_glds16(a_tile, a_tile_bytes, j ? a_voff1 : a_voff, t * 128 + p * 64,
                     plane(u, p) + (wave_u * 2 + j) * 1024);
      return;
    }
    const char* Ab = reinterpret_cast<const char*>(A);
    const int lane = ltid & 63, wave = ltid >> 6;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int piece = wave * 2 + j, rl = piece * 16 + (lane >> 2);
        const int c = (lane & 3) ^ f1_swz(rl);
        const int row = min(m0 + rl, M - 1);
        glds16(Ab + (size_t)row * lda * 4 + t * 128 + p * 64 + c * 16, plane(u, p) + piece * 1024);
      }
    }
  };
  auto stage_w = [&](int u, int t) {
    if constexpr (LEAN) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          buf_glds16((p ? Wl : Wh) + (size_t)n0 * ldw, F1_T * ldw * 2, w_voff, j * 16 * ldw * 2 + t * 64,
                     plane(u, 2 + p) + (wave_u * 2 + j) * 1024);
      return;
    }
    const int lane = ltid & 63, wave = ltid >> 6;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const bf16_t* W = p ? Wl : Wh;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int piece = wave * 2 + j, rl = piece * 16 + (lane >> 2);
        const int c = (lane & 3) ^ f1_swz(rl);
        glds16(W + (size_t)(n0 + rl) * ldw + t * F1_K + c * 8, plane(u, 2 + p) + piece * 1024);
      }
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  using I0 = std::integral_constant<int, 0>;
  if constexpr (SPLIT_IN) {
    stage_a(0, 0);
    stage_w(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    load_a(0, I0{});
    stage_w(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    store_a(0, I0{});
    if (nk > 1) load_a(1, I0{});  // both groups split A(1) in their first load segment
  }
  // raw barrier: A(1) stays in flight across it
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  const int fr = lane & 15, fc = lane >> 4;  // epilogue lane map
  // raw barrier (lgkmcnt for this step's LDS writes; the DMAs were waited
  // above): 6 % faster than __syncthreads here
  auto barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  bf16x8 fbh[4], fbl[4], fah[8], fal[8];
  auto read_frags = [&](int u) {  // all 24 fragments of a step: 8 W, 16 A
    if constexpr (LEAN) {
      LDS_AS char* const fw = fw_base + u * F1_BUF;
      LDS_AS char* const fa = fa_base + u * F1_BUF;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        fbh[j] = *reinterpret_cast<LDS_AS bf16x8*>(fw + j * 1024);
        fbl[j] = *reinterpret_cast<LDS_AS bf16x8*>(fw + F1_PLANE + j * 1024);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        fah[i] = *reinterpret_cast<LDS_AS bf16x8*>(fa + i * 1024);
        fal[i] = *reinterpret_cast<LDS_AS bf16x8*>(fa + F1_PLANE + i * 1024);
      }
      return;
    }
    const int fr = ltid & 15, fc = (ltid >> 4) & 3, wc = (ltid >> 6) & 3, wr = ltid >> 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fbh[j] = f1_frag(plane(u, 2), wc * 64 + j * 16 + fr, fc);
      fbl[j] = f1_frag(plane(u, 3), wc * 64 + j * 16 + fr, fc);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      fah[i] = f1_frag(plane(u, 0), wr * 128 + i * 16 + fr, fc);
      fal[i] = f1_frag(plane(u, 1), wr * 128 + i * 16 + fr, fc);
    }
  };
  // per accumulator W_hi A_hi, W_lo A_hi, W_hi A_lo; term-major
  // inside a row block so that consecutive MFMAs never share an accumulator
  auto mfma_seg = [&]() {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int term = 0; term < 3; ++term)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(term == 1 ? fbl[j] : fbh[j], term == 2 ? fal[i] : fah[i],
                                                              acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // retire this wave's DMAs of the next step; the 4 A loads issued after them stay in flight
  auto retire_dma = [&](bool a_in_flight) {
    if (a_in_flight)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  auto stage_next = [&](int u, int t) {
    if constexpr (SPLIT_IN) stage_a(u, t);
    stage_w(u, t);
  };
  // One program for both groups, group 1 one barrier behind: it passes an extra
  // barrier ahead of the loop (segment 0, where it only issues the DMAs of step
  // 1) and skips the one after its last MFMA segment, which group 0 passes on
  // its way to the epilogue.  What differs is where a group's DMAs sit: group 0
  // issues those of step t+1 in its load segment of step t (segment 2t), group 1
  // ahead of its MFMAs of step t-1 (the same segment 2t).
  const bool g1 = __builtin_amdgcn_readfirstlane(wr) != 0;
  auto fresh_tid = [&]() {
    if constexpr (LEAN) return;  // nothing to recompute: the lean state is five VGPRs
    ltid = tid;
    asm volatile("" : "+v"(ltid));
  };
  if (g1) {
    if (nk > 1) stage_next(1, 1);
    barrier();
  }
  for (int t = 0; t < nk; ++t) {
    const int u = t & 1;
    // load segment: group 0 segment 2t, group 1 segment 2t + 1
    fresh_tid();
    read_frags(u);
    if (t + 1 < nk) {
      if constexpr (!SPLIT_IN) store_a(u ^ 1, I0{});
      if (!g1) stage_next(u ^ 1, t + 1);
      if constexpr (!SPLIT_IN) {
        if (t + 2 < nk) load_a(t + 2, I0{});
      }
      if (g1) retire_dma(!SPLIT_IN && t + 2 < nk);
    }
    barrier();
    // MFMA segment: group 0 segment 2t + 1, group 1 segment 2t + 2
    if (g1 && t + 2 < nk) {
      fresh_tid();
      stage_next(u, t + 2);
    }
    mfma_seg();
    if (!g1 && t + 1 < nk) retire_dma(!SPLIT_IN && t + 2 < nk);
    if (!g1 || t + 1 < nk) barrier();
  }

  // epilogue (transposed accumulators): row m0 + wr*128 + i*16 + (lane & 15), cols n..n+3
  const bool vec = epi_vec_ok(C, ldc, bias, nullptr, 0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + wr * 128 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      epi_t4<ACT_RELU, true>(acc[i][j], m, n0 + wc * 64 + j * 16 + fc * 4, M, N, C, ldc, bias, nullptr, 0, vec);
  }
}

// Blocked boundary encoding of an fp32 (M,K) tensor, in place of the same
// 4 bytes per element: row r, 32-k block b holds 32 bf16 hi then 32 bf16 lo
// (hi + lo == x to ~2^-17 relative, the exact operand split of the x3 MFMAs).
// dir 0: fp32 -> blocked, dir 1: blocked -> fp32 (hi + lo).  K % 32 == 0.
__global__ __launch_bounds__(256) void cifar_split_blocked_kernel(const float* __restrict__ a, float* __restrict__ o,
                                                                  int M, int K, int dir) {
  const int per_row = K / 8;  // 8-element pieces
  const long total = (long)M * per_row;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e / per_row), k = (int)(e % per_row) * 8;
    char* rowp = reinterpret_cast<char*>(o + (size_t)m * K);
    const char* rowa = reinterpret_cast<const char*>(a + (size_t)m * K);
    const int hoff = (k >> 5) * 128 + (k & 31) * 2;
    if (dir == 0) {
      const float4 u = *reinterpret_cast<const float4*>(rowa + k * 4);
      const float4 v = *reinterpret_cast<const float4*>(rowa + k * 4 + 16);
      uint4 hi, lo;
      split2<true>(u.x, u.y, hi.x, lo.x);
      split2<true>(u.z, u.w, hi.y, lo.y);
      split2<true>(v.x, v.y, hi.z, lo.z);
      split2<true>(v.z, v.w, hi.w, lo.w);
      *reinterpret_cast<uint4*>(rowp + hoff) = hi;
      *reinterpret_cast<uint4*>(rowp + hoff + 64) = lo;
    } else {
      const uint4 hi = *reinterpret_cast<const uint4*>(rowa + hoff);
      const uint4 lo = *reinterpret_cast<const uint4*>(rowa + hoff + 64);
      const uint32_t h[4] = {hi.x, hi.y, hi.z, hi.w}, l[4] = {lo.x, lo.y, lo.z, lo.w};
      float r[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        r[2 * i] = __uint_as_float(h[i] << 16) + __uint_as_float(l[i] << 16);
        r[2 * i + 1] = __uint_as_float(h[i] & 0xffff0000u) + __uint_as_float(l[i] & 0xffff0000u);
      }
      *reinterpret_cast<float4*>(rowp + k * 4) = float4{r[0], r[1], r[2], r[3]};
      *reinterpret_cast<float4*>(rowp + k * 4 + 16) = float4{r[4], r[5], r[6], r[7]};
    }
  }
}

// fp32 (M,K) -> bf16 (M,3K) rows [hi | hi | lo]; K % 8 == 0, 16-B aligned rows.
// blocked = 1: a is in the blocked hi/lo encoding (the split is already done).
__global__ __launch_bounds__(256) void cifar_split3_kernel(const float* __restrict__ a, int lda,
                                                           bf16_t* __restrict__ o, int ldo, int M, int K,
                                                           int blocked) {
  const int per_row = K / 8;
  const long total = (long)M * per_row;
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e / per_row), c = (int)(e % per_row) * 8;
    uint4 hi, lo;
    if (blocked) {
      const char* rowa = reinterpret_cast<const char*>(a + (size_t)m * lda) + (c >> 5) * 128 + (c & 31) * 2;
      hi = *reinterpret_cast<const uint4*>(rowa);
      lo = *reinterpret_cast<const uint4*>(rowa + 64);
    } else {
      const float4 u = *reinterpret_cast<const float4*>(a + (size_t)m * lda + c);
      const float4 v = *reinterpret_cast<const float4*>(a + (size_t)m * lda + c + 4);
      split2<true>(u.x, u.y, hi.x, lo.x);
      split2<true>(u.z, u.w, hi.y, lo.y);
      split2<true>(v.x, v.y, hi.z, lo.z);
      split2<true>(v.z, v.w, hi.w, lo.w);
    }
    bf16_t* r = o + (size_t)m * ldo + c;
    *reinterpret_cast<uint4*>(r) = hi;
    *reinterpret_cast<uint4*>(r + K) = hi;
    *reinterpret_cast<uint4*>(r + 2 * K) = lo;
  }
}

// fc2 (512->10) + bias + softmax + argmax on fp32 hidden rows (fc1+ReLU output).
// One wave per 16 rows and iteration, mfma_f32_16x16x32_bf16 with the 3-term split:
// A = hid rows (lane: row l&15, k 8*(l>>4)+j), B = W2 hi/lo padded to 16 classes in VGPRs.
__global__ __launch_bounds__(256) void cifar_head_tail_x3_kernel(const float* __restrict__ hid,
                                                                 const bf16_t* __restrict__ w2h,
                                                                 const bf16_t* __restrict__ w2l,
                                                                 const float* __restrict__ b2,
                                                                 float* __restrict__ probs, int* __restrict__ pred,
                                                                 int B) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  const int col = lane & 15, kq = (lane >> 4) * 8;
  bf16x8 wfh[16], wfl[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    wfh[s] = *reinterpret_cast<const bf16x8*>(w2h + col * 512 + s * 32 + kq);
    wfl[s] = *reinterpret_cast<const bf16x8*>(w2l + col * 512 + s * 32 + kq);
  }
  const float bias = col < 10 ? b2[col] : 0.f;
  for (int r0 = gw * 16; r0 < B; r0 += nw * 16) {
    const int row = r0 + (lane & 15);
    const int rc = row < B ? row : B - 1;
    const float* ap = hid + (size_t)rc * 512 + kq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float4 u = *reinterpret_cast<const float4*>(ap + s * 32);
      const float4 v = *reinterpret_cast<const float4*>(ap + s * 32 + 4);
      uint4 hi, lo;
      // split2<false>: here the compiler already pairs the conversions, and with no MFMA
      // stream to protect its packed subtracts win (the packed form measured 37 -> 43 us)
      split2<false>(u.x, u.y, hi.x, lo.x);
      split2<false>(u.z, u.w, hi.y, lo.y);
      split2<false>(v.x, v.y, hi.z, lo.z);
      split2<false>(v.z, v.w, hi.w, lo.w);
      const bf16x8 ah = __builtin_bit_cast(bf16x8, hi), al = __builtin_bit_cast(bf16x8, lo);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wfh[s], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, wfl[s], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, wfh[s], acc, 0, 0, 0);
    }
    // acc[r] = logit(row = r0 + (lane>>4)*4 + r, class = col)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = col < 10 ? acc[r] + bias : -INFINITY;
      float mx = z;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      const float e = col < 10 ? expf(z - mx) : 0.f;
      float sum = e;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      int cand = (z == mx) ? col : 16;  // smallest class index attaining the max (numpy semantics)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) cand = min(cand, __shfl_xor(cand, o, 64));
      const int m = r0 + (lane >> 4) * 4 + r;
      if (m < B) {
        if (col < 10) probs[(size_t)m * 10 + col] = e / sum;
        if (col == 0) pred[m] = cand;
      }
    }
  }
}

// The bf16 precision's head tail: fc2 (512->10) + bias + softmax + argmax. hid: (B,512) bf16
// (fc1+ReLU output).  One wave handles 16 rows per iteration with mfma_f32_16x16x32_bf16:
// A = hid rows (lane: row l&15, k 8*(l>>4)+j), B = W2 padded to 16 classes held
// in VGPRs. Softmax across each 16-lane row group with xor-shuffles.
// It lives in this file, not in cifar_fused.hip, for the IEEE expf and division of this file's
// build: under cifar_fused.hip's -ffast-math, expf (and __expf under any flags) is
// v_exp_f32(log2e * x), whose rounded product is a relative error of the probability that grows
// with the gap to the max (3.5e-6 measured at a gap of 72), and __expf also flushes probabilities
// below 2^-126 to 0.  The IEEE forms cost 0.4 us of 18 at B = 65536.  The probabilities are fp32
// outputs in both precisions, held to one bound (tests/test_cifar_head_tail_gpu.py).
__global__ __launch_bounds__(256) void cifar_head_tail_kernel(const bf16_t* __restrict__ hid, const bf16_t* __restrict__ w2p,
                                                              const float* __restrict__ b2, float* __restrict__ probs,
                                                              int* __restrict__ pred, int B) {
  const int lane = threadIdx.x & 63;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nw = (gridDim.x * blockDim.x) >> 6;
  const int col = lane & 15, kq = (lane >> 4) * 8;
  bf16x8 wf[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) wf[s] = *reinterpret_cast<const bf16x8*>(w2p + col * 512 + s * 32 + kq);
  const float bias = col < 10 ? b2[col] : 0.f;
  for (int r0 = gw * 16; r0 < B; r0 += nw * 16) {
    const int row = r0 + (lane & 15);
    const int rc = row < B ? row : B - 1;
    const bf16_t* ap = hid + (size_t)rc * 512 + kq;
    bf16x8 a[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) a[s] = *reinterpret_cast<const bf16x8*>(ap + s * 32);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], wf[s], acc, 0, 0, 0);
    // acc[r] = logit(row = r0 + (lane>>4)*4 + r, class = col)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float z = col < 10 ? acc[r] + bias : -INFINITY;
      float mx = z;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      const float e = col < 10 ? expf(z - mx) : 0.f;
      float sum = e;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) sum += __shfl_xor(sum, o, 64);
      // argmax: smallest class index attaining the max (numpy semantics)
      int cand = (z == mx) ? col : 16;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) cand = min(cand, __shfl_xor(cand, o, 64));
      const int m = r0 + (lane >> 4) * 4 + r;
      if (m < B) {
        if (col < 10) probs[(size_t)m * 10 + col] = e / sum;
        if (col == 0) pred[m] = cand;
      }
    }
  }
}

}  // namespace dnn

using namespace dnn;

// stage-0 boundary stores of the 32x32x16 conv2 path: 16-B (permlane32-paired, 1) or 8-B (0); A/B switch
static int g_s0_wide_store = 1;
// conv2 MFMA shape: 1 = 16x16x32 (default; every interleaved round faster than 32x32x16,
// profiles/cifar_s0_mfma16_ab.jsonl), 0 = 32x32x16 (the A/B's other arm)
static int g_s0_mfma = 1;

extern "C" int dnn_cifar_s0_set_mfma(int v) {
  if (v < 0 || v > 1) return 1;
  g_s0_mfma = v;
  return 0;
}

extern "C" int dnn_cifar_s0_get_mfma() { return g_s0_mfma; }

extern "C" int dnn_cifar_s0_set_wide_store(int on) {
  g_s0_wide_store = on ? 1 : 0;
  return 0;
}

extern "C" int dnn_cifar_s0_get_wide_store() { return g_s0_wide_store; }

// conv1 K packing: 1 = K = 32 on channel-packed planes (default; every interleaved round faster than
// K = 48, profiles/cifar_conv1_k32_ab.jsonl), 0 = K = 48 on HWC4 planes (the A/B's other arm)
static int g_s0_conv1 = 1;

extern "C" int dnn_cifar_s0_set_conv1(int v) {
  if (v < 0 || v > 1) return 1;
  g_s0_conv1 = v;
  return 0;
}

extern "C" int dnn_cifar_s0_get_conv1() { return g_s0_conv1; }

template <bool SPLIT_OUT, int C1, int IN = 0>
static int launch_stage0_x3(s0_input_t<IN> x, float* out, const void* w1h, const void* w1l, const float* b1,
                            const void* w2h, const void* w2l, const float* b2, int B, int grid, hipStream_t st) {
  if (g_s0_mfma == 1)
    hipLaunchKernelGGL((cifar_stage0_x3_kernel<true, SPLIT_OUT, 1, C1, IN>), dim3(grid), dim3(512), 0, st, x, out,
                       (const bf16_t*)w1h, (const bf16_t*)w1l, b1, (const bf16_t*)w2h, (const bf16_t*)w2l, b2, B);
  else if (g_s0_wide_store)
    hipLaunchKernelGGL((cifar_stage0_x3_kernel<true, SPLIT_OUT, 0, C1, IN>), dim3(grid), dim3(512), 0, st, x, out,
                       (const bf16_t*)w1h, (const bf16_t*)w1l, b1, (const bf16_t*)w2h, (const bf16_t*)w2l, b2, B);
  else
    hipLaunchKernelGGL((cifar_stage0_x3_kernel<false, SPLIT_OUT, 0, C1, IN>), dim3(grid), dim3(512), 0, st, x, out,
                       (const bf16_t*)w1h, (const bf16_t*)w1l, b1, (const bf16_t*)w2h, (const bf16_t*)w2l, b2, B);
  return (int)hipGetLastError();
}

// split_out = 1: the (B,4096) boundary in the blocked hi/lo encoding, else fp32.
// w1h / w1l: conv1 [32][48] (K = 48 arm); w1h32 / w1l32: conv1 [2][32][32] (K = 32 arm, required by it).
extern "C" int dnn_cifar_stage0_x3(const float* x, float* out, const void* w1h, const void* w1l, const float* b1,
                                   const void* w2h, const void* w2l, const float* b2, int B, int grid,
                                   hipStream_t st, int split_out, const void* w1h32, const void* w1l32) {
  if (B <= 0) return 0;
  if (grid <= 0) grid = 256;
  if (grid > B) grid = B;
  if (g_s0_conv1 == 1) {
    if (!w1h32 || !w1l32) return -1;
    return split_out ? launch_stage0_x3<true, 1>(x, out, w1h32, w1l32, b1, w2h, w2l, b2, B, grid, st)
                     : launch_stage0_x3<false, 1>(x, out, w1h32, w1l32, b1, w2h, w2l, b2, B, grid, st);
  }
  return split_out ? launch_stage0_x3<true, 0>(x, out, w1h, w1l, b1, w2h, w2l, b2, B, grid, st)
                   : launch_stage0_x3<false, 0>(x, out, w1h, w1l, b1, w2h, w2l, b2, B, grid, st);
}

// The same stage on uint8 NHWC input (B,32,32,3), normalised by ``table`` (uint32 [3][256]: bf16 hi
// bits low, bf16 lo bits high).  K = 32 conv1 arm only.  Rejected (negative, nothing launched):
// -1 a null table or K = 32 weight pointer, -2 the conv1 switch is on K = 48, -3 x or table not
// 4-byte aligned (the kernel reads both as dwords).
extern "C" int dnn_cifar_stage0_x3_u8(const unsigned char* x, const unsigned* table, float* out, const void* w1h32,
                                      const void* w1l32, const float* b1, const void* w2h, const void* w2l,
                                      const float* b2, int B, int grid, hipStream_t st, int split_out) {
  if (B <= 0) return 0;
  if (g_s0_conv1 != 1) return -2;
  if (!table || !w1h32 || !w1l32) return -1;
  if (((uintptr_t)x | (uintptr_t)table) & 3) return -3;
  if (grid <= 0) grid = 256;
  if (grid > B) grid = B;
  const U8Input in{x, table};
  return split_out ? launch_stage0_x3<true, 1, 1>(in, out, w1h32, w1l32, b1, w2h, w2l, b2, B, grid, st)
                   : launch_stage0_x3<false, 1, 1>(in, out, w1h32, w1l32, b1, w2h, w2l, b2, B, grid, st);
}

// fc1 k-loop arm: 1 = staggered wave groups, 2 = lean (the same schedule with the packed split and
// loop-invariant buffer addressing); the A/B's arms, bitwise-equal outputs
static int g_fc1_sched = 2;

extern "C" int dnn_cifar_fc1_set_sched(int v) {
  if (v < 1 || v > 2) return 1;
  g_fc1_sched = v;
  return 0;
}

extern "C" int dnn_cifar_fc1_get_sched() { return g_fc1_sched; }

template <bool SPLIT_IN>
static int launch_fc1_x3(const float* A, int lda, const void* Wh, const void* Wl, int ldw, const float* bias, float* C,
                         int ldc, int M, int N, int K, int blocks, hipStream_t st) {
  if (g_fc1_sched == 2)
    hipLaunchKernelGGL((cifar_fc1_x3_kernel<SPLIT_IN, true>), dim3(blocks), dim3(512), 0, st, A, lda,
                       (const bf16_t*)Wh, (const bf16_t*)Wl, ldw, bias, C, ldc, M, N, K);
  else
    hipLaunchKernelGGL((cifar_fc1_x3_kernel<SPLIT_IN, false>), dim3(blocks), dim3(512), 0, st, A, lda,
                       (const bf16_t*)Wh, (const bf16_t*)Wl, ldw, bias, C, ldc, M, N, K);
  return (int)hipGetLastError();
}

extern "C" int dnn_cifar_fc1_x3(const float* A, int lda, const void* Wh, const void* Wl, int ldw, const float* bias,
                                float* C, int ldc, int M, int N, int K, hipStream_t st, int a_split) {
  if (M <= 0) return 0;
  if (N % F1_T != 0 || K < F1_K || K % F1_K != 0 || lda % 4 != 0 || ldw % 8 != 0 || ldc % 4 != 0) return -1;
  const int blocks = ((M + F1_T - 1) / F1_T) * (N / F1_T);
  return a_split ? launch_fc1_x3<true>(A, lda, Wh, Wl, ldw, bias, C, ldc, M, N, K, blocks, st)
                 : launch_fc1_x3<false>(A, lda, Wh, Wl, ldw, bias, C, ldc, M, N, K, blocks, st);
}

extern "C" int dnn_cifar_split_blocked(const float* a, float* o, int M, int K, int dir, hipStream_t st) {
  if (M <= 0) return 0;
  if (K % 32 != 0 || a == o) return -1;
  const long total = (long)M * (K / 8);
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cifar_split_blocked_kernel, dim3((int)blocks), dim3(256), 0, st, a, o, M, K, dir);
  return (int)hipGetLastError();
}

extern "C" int dnn_cifar_split3(const float* a, int lda, void* o, int ldo, int M, int K, hipStream_t st, int blocked) {
  if (M <= 0) return 0;
  if (K % 8 != 0 || lda % 4 != 0 || ldo % 8 != 0 || ldo < 3 * K || (blocked && K % 32 != 0)) return -1;
  const long total = (long)M * (K / 8);
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cifar_split3_kernel, dim3((int)blocks), dim3(256), 0, st, a, lda, (bf16_t*)o, ldo, M, K, blocked);
  return (int)hipGetLastError();
}

extern "C" int dnn_cifar_head_tail_x3(const float* hid, const void* w2h, const void* w2l, const float* b2,
                                      float* probs, int* pred, int B, hipStream_t st) {
  if (B <= 0) return 0;
  int waves = (B + 15) / 16;
  int blocks = (waves + 3) / 4;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(cifar_head_tail_x3_kernel, dim3(blocks), dim3(256), 0, st, hid, (const bf16_t*)w2h,
                     (const bf16_t*)w2l, b2, probs, pred, B);
  return (int)hipGetLastError();
}

extern "C" int dnn_cifar_head_tail(const void* hid, const void* w2p, const float* b2, float* probs, int* pred, int B,
                                   hipStream_t st) {
  if (B <= 0) return 0;
  int waves = (B + 15) / 16;
  int blocks = (waves + 3) / 4;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(cifar_head_tail_kernel, dim3(blocks), dim3(256), 0, st, (const bf16_t*)hid, (const bf16_t*)w2p,
                     b2, probs, pred, B);
  return (int)hipGetLastError();
}
