"""OCP MXFP4 weights: e2m1 codes with one e8m0 scale per 32 elements along K
(4.25 bits per weight), the W4A16 decode GEMM and the expansion that feeds the
bf16 prefill kernels (``csrc/kernels/gemm_w4.hip``).

``Mxfp4Weight`` is the only stored copy of a weight, in the decode kernel's
fragment order.  N is zero-padded to a multiple of 16; K must be a multiple of
32 and is zero-padded to a multiple of 128.

* ``q`` (uint8): ``[tile = n // 16][chunk = k // 128][lane = 16 g + r][16 bytes]``
  — lane ``l`` holds the 32 codes of row ``16 tile + r``, k = ``128 chunk + 32 g
  .. + 31`` (one MX block); byte ``b`` holds k + 2 b in its low nibble and
  k + 2 b + 1 in its high nibble.  The 16 x 128 codes of (tile, chunk) are one
  contiguous 1 KiB block; the blocks of a tile are consecutive along K.
* ``scales`` (uint8 e8m0, 1..254): ``[tile][chunk][lane]``, the scale of the
  lane's block; the value is ``2 ** (e - 127)``, as fp32 the bit pattern
  ``e << 23``.  Pad blocks carry 127.

Code ``c``: bit 3 = sign, bits 0..2 index (0, 0.5, 1, 1.5, 2, 3, 4, 6).

Decode-sized M (<= 64) runs ``dnn_gemm_w4``.  65..256 rows without a scratch
run ``dnn_gemm_w4_mid`` (``csrc/kernels/gemm_w4_mid.h``: the codes are read
once, A is shared through LDS, nothing is expanded): the decode microbatches.
Projections too narrow for its N / 64 workgroups run ``dnn_gemm_w4_mn``
(``csrc/kernels/gemm_w4_mn.h``: workgroups tile M and N, their waves split K;
``linear_w4(mn=True)``, the shapes of ``w4_mn_ok``).
With a caller-supplied bf16 scratch, more than 64 rows expand the weight
(``dnn_w4_expand``) and run the bf16 tile kernels on it, with their
folded-norm, QKV-scatter, GELU, SwiGLU and residual epilogues unchanged: the
prefill route, and without ``tile`` the only one above 256 rows.
``linear_w4(tile=True)`` runs any M > 64 as one ``dnn_gemm_w4_tile`` launch
instead (``csrc/kernels/gemm_w4_tile.h``: 128 x 128 output blocks over the
whole of K, A through LDS, the codes converted in registers; no scratch, no row
limit): what ``mxfp4_prefill: "w4a16"`` runs wherever the other modes expand.

A vocabulary head (``fold_norm(quant="mxfp4")`` of ``lm_head``) at up to 64 rows
runs ``head_w4`` (``dnn_gemm_w4_head``, ``csrc/kernels/gemm_w4_head.h``):
persistent workgroups with the activations in LDS, and optionally the greedy
argmax's first pass in the epilogue.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ._lib import check, lib, ptr, stream_ptr

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
W4_MAX_M = 64
W4_MID_MAX_M = 256


def w4_mid_ok(M: int, N: int, K: int) -> bool:
    """Whether a decode step of 65..256 rows runs ``dnn_gemm_w4_mid`` on this
    projection rather than expanding it (bench/probes/w4_mid_ab.py,
    profiles/w4_mid_ab.jsonl: the mid kernel against expand + bf16 GEMM).  It
    has no M or cross-workgroup K split, so N / 64 workgroups must fill the
    device: N >= 4096 measured 1.2-2.2 x faster at 96..256 rows, N = 1600
    0.66-0.97 x (slower), and N = 28672 at 256 rows a tie (excluded).  A weight
    of at most 1 Mi elements also goes there: both routes are then bound by
    launches, one against two (reasoned, not measured)."""
    if not W4_MAX_M < M <= W4_MID_MAX_M:
        return False
    if N * K <= 1 << 20:
        return True
    return N >= 4096 and not (N >= 16384 and M > 128)


def w4_mn_ok(M: int, N: int, K: int) -> bool:
    """Whether a decode step of 65..256 rows runs ``dnn_gemm_w4_mn`` on this
    projection, ahead of both ``dnn_gemm_w4_mid`` and the expansion
    (bench/probes/w4_mn_ab.py, profiles/w4_mn_ab.jsonl: three arms, 5 rounds,
    us per launch at 96 / 128 / 256 rows, mn | mid | expand + bf16 GEMM):
      768 -> 768     6.6 /  6.6 /  6.7 | 10.2 / 12.1 /  18.7 |  9.0 /  9.0 /  11.0
      768 -> 2304    6.8 /  6.8 /  8.2 | 10.4 / 12.2 /  18.9 | 11.2 / 13.2 /  17.5
      768 -> 3072    6.8 /  6.8 /  8.3 | 10.4 / 12.2 /  19.0 | 13.8 / 13.9 /  20.2
      3072 -> 768   16.7 / 16.9 / 16.8 | 28.7 / 35.1 /  58.5 | 17.7 / 17.7 /  23.2
      1280 -> 3840   9.1 /  9.2 / 11.8 | 14.5 / 17.3 /  27.9 | 20.3 / 23.8 /  37.3
      1600 -> 1600  11.3 / 11.3 / 11.9 | 17.7 / 21.2 /  34.3 | 16.9 / 17.0 /  26.0
      6400 -> 1600  32.1 / 32.3 / 34.7 | 55.8 / 68.8 / 116.6 | 47.8 / 47.6 /  76.3
      1600 -> 4800  12.9 / 15.1 / 24.0 | 17.8 / 21.2 /  34.4 | 31.3 / 35.8 /  58.6
      4096 -> 6144  24.9 / 28.9 / 47.4 | 37.4 / 46.0 /  76.7 | 74.1 / 83.4 / 142.5
    In all 27 cases the slowest mn round is faster than the fastest round of
    both other arms (the spread between rounds of one arm is below 2 %; the
    narrowest margin, 3072 -> 768 at 96 rows, is 16.73 against 17.65), the two
    guard shapes that the mid kernel held included, and 768 -> 768, a weight
    of at most 1 Mi elements, too.  The rule is the box those shapes span:
    N <= 6144 and K <= 6400.  Wider or deeper projections (Llama-3 8B gate|up
    and down, any vocabulary head) are not measured and stay where
    ``w4_mid_ok`` puts them: every workgroup of this kernel reads 64 rows of A
    per 32 columns, N / 32 x M x 2 K bytes from L2, which grows with N x K."""
    return W4_MAX_M < M <= W4_MID_MAX_M and N <= 6144 and K <= 6400


def _table(device) -> torch.Tensor:
    mag = torch.tensor(E2M1, dtype=torch.float32, device=device)
    return torch.cat([mag, -mag])


@dataclass
class Mxfp4Weight:
    q: torch.Tensor       # uint8 codes in fragment order, (ceil(n / 16) * 16) * kpad / 2 bytes
    scales: torch.Tensor  # uint8 e8m0 in fragment order, (ceil(n / 16) * 16) * kpad / 32 bytes
    n: int
    k: int

    @property
    def shape(self):
        return (self.n, self.k)

    @property
    def kpad(self) -> int:
        return -(-self.k // 128) * 128

    @property
    def npad(self) -> int:
        return -(-self.n // 16) * 16

    def _scale_rows(self) -> torch.Tensor:
        """The scale bytes viewed as (tile, chunk, g, r): row 16 tile + r."""
        return self.scales.view(self.npad // 16, self.kpad // 128, 4, 16)

    def scale_rows_pow2(self, r: torch.Tensor) -> None:
        """Multiply row n by ``r[n]`` (powers of two) in place: the codes stay,
        the block exponents move."""
        sh = torch.log2(r.float()).round().to(torch.int32)
        if not torch.equal(torch.exp2(sh.float()), r.float()):
            raise ValueError("scale_rows_pow2: powers of two only")
        pad = torch.zeros(self.npad, dtype=torch.int32, device=sh.device)
        pad[:self.n] = sh
        e = self._scale_rows().to(torch.int32) + pad.view(-1, 1, 1, 16)
        if int(e.min()) < 1 or int(e.max()) > 254:
            raise ValueError("scale_rows_pow2: block exponent leaves 1..254")
        self._scale_rows().copy_(e.to(torch.uint8))


def pack_mxfp4(codes: torch.Tensor, exps: torch.Tensor) -> Mxfp4Weight:
    """Raw codes (N, K) in 0..15 and e8m0 block exponents (N, K / 32) in
    1..254 -> fragment order."""
    N, K = codes.shape
    if K % 32 or K == 0:
        raise ValueError(f"pack_mxfp4: K={K} must be a positive multiple of 32 (the MX block)")
    if tuple(exps.shape) != (N, K // 32):
        raise ValueError(f"pack_mxfp4: exponents {tuple(exps.shape)} for codes {tuple(codes.shape)}")
    if int(codes.min()) < 0 or int(codes.max()) > 15:
        raise ValueError("pack_mxfp4: codes outside 0..15")
    if int(exps.min()) < 1 or int(exps.max()) > 254:
        raise ValueError("pack_mxfp4: e8m0 exponents outside 1..254 (0 and 255 are rejected)")
    Np, Kp = -(-N // 16) * 16, -(-K // 128) * 128
    c = torch.zeros((Np, Kp), dtype=torch.uint8, device=codes.device)
    c[:N, :K] = codes.to(torch.uint8)
    b = c[:, 0::2] | (c[:, 1::2] << 4)
    q = b.view(Np // 16, 16, Kp // 128, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)
    e = torch.full((Np, Kp // 32), 127, dtype=torch.uint8, device=codes.device)
    e[:N, :K // 32] = exps.to(torch.uint8)
    s = e.view(Np // 16, 16, Kp // 128, 4).permute(0, 2, 3, 1).contiguous().view(-1)
    return Mxfp4Weight(q, s, N, K)


def unpack_mxfp4(w: Mxfp4Weight):
    """Inverse of ``pack_mxfp4``: codes (N, K) uint8 and exponents (N, K / 32) uint8."""
    Np, Kp = w.npad, w.kpad
    b = w.q.view(Np // 16, Kp // 128, 4, 16, 16).permute(0, 3, 1, 2, 4).reshape(Np, Kp // 2)
    c = torch.stack([b & 15, b >> 4], dim=2).reshape(Np, Kp)
    e = w._scale_rows().permute(0, 3, 1, 2).reshape(Np, Kp // 32)
    return c[:w.n, :w.k].contiguous(), e[:w.n, :w.k // 32].contiguous()


def dequantize(w: Mxfp4Weight) -> torch.Tensor:
    """fp32 (N, K) values of the weight, in plain torch."""
    c, e = unpack_mxfp4(w)
    v = _table(c.device)[c.long()]
    s = torch.exp2(e.float() - 127.0)
    return (v.view(w.n, w.k // 32, 32) * s[:, :, None]).view(w.n, w.k)


def quantize_weight_mxfp4(w: torch.Tensor, device) -> Mxfp4Weight:
    """Round-to-nearest-even onto the e2m1 grid, saturating at +-6, with the
    block exponent ``e = clamp(floor(log2(amax)) - 2 + 127, 1, 254)`` (127 for
    an all-zero block): the block's amax lands in [4, 8) before rounding.
    Idempotent on its own output."""
    wf = w.to(device).float()
    N, K = wf.shape
    if K % 32 or K == 0:
        raise ValueError(f"quantize_weight_mxfp4: K={K} must be a positive multiple of 32 (the MX block)")
    blk = wf.view(N, K // 32, 32)
    amax = blk.abs().amax(dim=2)
    _, ex = torch.frexp(amax)  # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    e = (ex - 1 - 2 + 127).clamp(1, 254)
    e = torch.where(amax > 0, e, torch.full_like(e, 127))
    x = blk * torch.exp2(127.0 - e.float())[:, :, None]
    a = x.abs().clamp(max=6.0)
    # the grid's steps: 0.5 below 2, 1 below 4, 2 above; torch.round is half-to-even, and
    # the even multiples of each step are the codes with an even significand
    v = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
    idx = torch.where(v < 2, v * 2, torch.where(v < 4, v + 2, v / 2 + 4)).to(torch.uint8)
    codes = idx | ((x < 0) & (idx > 0)).to(torch.uint8) << 3
    return pack_mxfp4(codes.view(N, K), e.to(torch.uint8))


def expand(w: Mxfp4Weight, scratch: torch.Tensor) -> torch.Tensor:
    """Dequantise into the front of the bf16 ``scratch`` (``dnn_w4_expand``)
    and return its (N, K) row-major view (row stride K)."""
    if scratch.dtype != torch.bfloat16 or not scratch.is_contiguous() or scratch.numel() < w.n * w.k:
        raise ValueError(f"w4.expand: contiguous bf16 scratch of >= {w.n * w.k} elements expected")
    out = scratch.view(-1)[:w.n * w.k].view(w.n, w.k)
    check(lib().w4_expand(ptr(w.q), ptr(w.scales), ptr(out), w.k, w.n, w.k, stream_ptr()), "w4_expand")
    return out


def expand_folded(f, scratch: torch.Tensor):
    """A transient bf16 ``gemm.FoldedLinear`` over ``scratch`` holding the
    expanded weight of the MXFP4 ``FoldedLinear`` ``f`` (same bias, colsum and
    norm): what the bf16 prefill kernels run on.  Valid until the next
    expansion into ``scratch``."""
    from .gemm import FoldedLinear
    return FoldedLinear(expand(f.w, scratch), f.bias, f.colsum, f.norm, f.eps)


def linear_w4a8(x: torch.Tensor, w: Mxfp4Weight, bias: Optional[torch.Tensor] = None, act: int = 0,
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                q8: Optional[torch.Tensor] = None, sx: Optional[torch.Tensor] = None,
                prequantized: bool = False) -> torch.Tensor:
    """bf16 x (M, K) times an MXFP4 weight on MX e4m3 activations (W4A8,
    ``dnn_gemm_w4a8``: the codes on the scaled MFMA, nothing expanded), bf16
    out, any M >= 1: the prefill route of ``mxfp4_prefill: "e4m3"``.  ``q8``
    (>= M * kpad bytes) and ``sx`` (>= ``fp8.mx_scale_bytes(M, kpad)`` bytes)
    receive the quantised rows and their e8m0 scales (``fp8.quant_rows_mx``);
    with ``prequantized`` they already hold them (``layernorm_q8_mx``) and x
    only gives M and K."""
    from .fp8 import mx_scale_bytes, quant_rows_mx
    M, K = x.shape
    N, kp = w.n, w.kpad
    if K != w.k:
        raise ValueError(f"linear_w4a8: x {tuple(x.shape)} vs weight {w.shape}")
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise TypeError("linear_w4a8: bf16 activations with a contiguous last dim")
    if q8 is None or sx is None or q8.numel() * q8.element_size() < M * kp or \
            sx.numel() * sx.element_size() < mx_scale_bytes(M, kp):
        raise ValueError(f"linear_w4a8: q8 of >= {M * kp} bytes and sx of >= {mx_scale_bytes(M, kp)} bytes expected")
    Nout = N // 2 if act == 3 else N
    if out is None:
        out = torch.empty((M, Nout), dtype=torch.bfloat16, device=x.device)
    if out.dtype != torch.bfloat16 or out.stride(1) != 1 or out.shape[0] < M or out.shape[1] < Nout:
        raise ValueError("linear_w4a8: bad output buffer")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("linear_w4a8: bias must be fp32")
    if residual is not None and (residual.shape[0] < M or residual.stride(1) != 1):
        raise ValueError("linear_w4a8: bad residual")
    if not prequantized:
        quant_rows_mx(x, q8, sx, M)
    check(lib().gemm_w4a8(ptr(q8), ptr(sx), ptr(w.q), ptr(w.scales), ptr(out), out.stride(0), ptr(bias),
                          ptr(residual), 0 if residual is None else residual.stride(0), M, N, K, act, stream_ptr()),
          "gemm_w4a8")
    return out


def linear_w4(x: torch.Tensor, w: Mxfp4Weight, bias: Optional[torch.Tensor] = None, act: int = 0,
              residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, norm: int = 0,
              colsum: Optional[torch.Tensor] = None, eps: float = 0.0, scratch: Optional[torch.Tensor] = None,
              std_buf: Optional[torch.Tensor] = None, ones: Optional[torch.Tensor] = None,
              mn: bool = False, tile: bool = False) -> torch.Tensor:
    """bf16 x (M, K) times an MXFP4 weight, bf16 out.  ``norm`` (1 RMS / 2 LN,
    with ``colsum`` for LN) is a folded pre-norm (``gemm.fold_norm(quant="mxfp4")``).
    M <= 64: one ``dnn_gemm_w4`` launch.  M > 64 with ``scratch`` (bf16, >= N K
    elements): the weight is expanded into it and the bf16 ``gemm.linear`` /
    ``gemm.linear_norm`` run on it (``std_buf`` / ``ones`` as ``linear_norm``).
    65 <= M <= 256 without a scratch: one ``dnn_gemm_w4_mid`` launch on the
    codes, or with ``mn`` one ``dnn_gemm_w4_mn`` launch (the M x N grid for
    narrow projections, ``w4_mn_ok``).  More than 256 rows need the scratch,
    unless ``tile``: then M > 64 is one ``dnn_gemm_w4_tile`` launch on the codes
    (any M, no scratch; ``mn`` and ``scratch`` are not used)."""
    M, K = x.shape
    N = w.n
    if K != w.k:
        raise ValueError(f"linear_w4: x {tuple(x.shape)} vs weight {w.shape}")
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise TypeError("linear_w4: bf16 activations with a contiguous last dim")
    if M > W4_MAX_M and not tile and (scratch is not None or M > W4_MID_MAX_M):
        from .gemm import FoldedLinear, linear, linear_norm
        if scratch is None:
            raise ValueError("linear_w4: more than 256 rows need the bf16 expand scratch")
        if norm:
            return linear_norm(x, expand_folded(FoldedLinear(w, bias, colsum, norm, eps), scratch), act, residual,
                               out, std_buf=std_buf, ones=ones)
        return linear(x, expand(w, scratch), bias, act, residual, out)
    Nout = N // 2 if act == 3 else N
    if out is None:
        out = torch.empty((M, Nout), dtype=torch.bfloat16, device=x.device)
    if out.dtype != torch.bfloat16 or out.stride(1) != 1 or out.shape[0] < M or out.shape[1] < Nout:
        raise ValueError("linear_w4: bad output buffer")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError("linear_w4: bias must be fp32")
    if residual is not None and (residual.shape[0] < M or residual.stride(1) != 1):
        raise ValueError("linear_w4: bad residual")
    if M <= W4_MAX_M:
        fn, name = lib().gemm_w4, "gemm_w4"
    elif tile:
        fn, name = lib().gemm_w4_tile, "gemm_w4_tile"
    elif mn:
        fn, name = lib().gemm_w4_mn, "gemm_w4_mn"
    else:
        fn, name = lib().gemm_w4_mid, "gemm_w4_mid"
    check(fn(ptr(x), x.stride(0), ptr(w.q), ptr(w.scales), ptr(out), out.stride(0), ptr(bias), ptr(residual),
             0 if residual is None else residual.stride(0), M, N, K, act, norm, ptr(colsum), eps, stream_ptr()), name)
    return out


def head_w4(x: torch.Tensor, f, logits: torch.Tensor, part: Optional[torch.Tensor] = None,
            ids_out: Optional[torch.Tensor] = None, also: Optional[torch.Tensor] = None,
            advance: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MXFP4 vocabulary head (``dnn_gemm_w4_head``): ``logits = linear(norm(x), W)``
    for the folded-norm ``gemm.FoldedLinear`` ``f`` holding an ``Mxfp4Weight``, at
    1..64 rows, in one launch.  With ``part`` (contiguous int32, >= 2 *
    ``gemm.HEAD_PART_PER_ROW`` * M entries) every workgroup also writes its
    argmax per row of the rounded logits there, and a second launch
    (``argmax_final``) writes the ids to ``ids_out`` and does the decode step
    tail as ``gemm.head_argmax`` (``also``, ``hist[row, advance]``, ``advance +=
    1``).  Without ``part``: the logits only (sampled, penalised and constrained
    steps).  Returns ``logits``."""
    from .gemm import HEAD_PART_PER_ROW
    w = f.w
    M, K = x.shape
    N = w.n
    if not isinstance(w, Mxfp4Weight) or K != w.k:
        raise ValueError(f"head_w4: x {tuple(x.shape)} vs weight {getattr(w, 'shape', None)}")
    if x.dtype != torch.bfloat16 or x.stride(1) != 1:
        raise TypeError("head_w4: bf16 activations with a contiguous last dim")
    if not 1 <= M <= W4_MAX_M:
        raise ValueError(f"head_w4: 1..{W4_MAX_M} rows, got {M}")
    if logits.dtype != torch.bfloat16 or logits.stride(1) != 1 or logits.shape[0] < M or logits.shape[1] < N:
        raise ValueError("head_w4: bad logits buffer")
    if f.bias is not None and f.bias.dtype != torch.float32:
        raise TypeError("head_w4: bias must be fp32")
    hist_ld = 0
    if part is None:
        if any(t is not None for t in (ids_out, also, advance, hist)):
            raise ValueError("head_w4: ids_out / also / advance / hist need part")
    else:
        if part.dtype != torch.int32 or not part.is_contiguous() or part.numel() < 2 * HEAD_PART_PER_ROW * M:
            raise ValueError(f"head_w4: part must be contiguous int32 with >= {2 * HEAD_PART_PER_ROW * M} entries")
        if ids_out is None:
            raise ValueError("head_w4: part needs ids_out")
        for t, nm in ((ids_out, "ids_out"), (also, "also"), (advance, "advance")):
            if t is not None and (t.dtype != torch.int32 or t.numel() < M or not t.is_contiguous()):
                raise ValueError(f"head_w4: {nm} must be contiguous int32 with >= {M} entries")
        from .transformer_ops import check_hist
        hist_ld = check_hist(hist, advance, M, "head_w4")
    S = lib().gemm_w4_head(ptr(x), x.stride(0), ptr(w.q), ptr(w.scales), ptr(logits), logits.stride(0), ptr(f.bias),
                           M, N, K, f.norm, ptr(f.colsum), f.eps, ptr(part), HEAD_PART_PER_ROW, stream_ptr())
    if S <= 0:
        raise RuntimeError(f"gemm_w4_head failed ({S})")
    if part is not None:
        check(lib().argmax_final(ptr(part), S, M, ptr(ids_out), ptr(also), ptr(advance), stream_ptr(), ptr(hist),
                                 hist_ld), "argmax_final")
    return logits
