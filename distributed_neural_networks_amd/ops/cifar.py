"""CIFAR-10 ConvNet on the fused gfx950 kernels.

Two precisions, packed once at load (reference ``node.py:305-306`` only moves
fp32 modules to the device):

* ``fp32`` (the reference's precision, default): ``csrc/kernels/cifar_x3.hip``.
  Every fp32 operand is split into bf16 hi + lo and each product is three bf16
  MFMAs (hi*hi + hi*lo + lo*hi) accumulated in fp32.  Stage boundary tensor
  ``(B,4096)`` fp32 exactly as the reference ships it (``node.py:45-48``).
  fc1 at large batch is ``cifar_fc1_x3``: the fp32 boundary rows are split in
  registers while staged to LDS (A read once as fp32, no split copy); at small
  batch (too few 256-row tiles to fill the chip) it runs as ONE skinny/128^2
  bf16 GEMM over K' = 3*4096 on ``[A_hi | A_hi | A_lo]`` x ``[W_hi | W_lo | W_hi]``.
  Optional boundary encoding ``boundary="split"`` (fp32 only, both ends of
  the hop must be these kernels): the same 16 KiB/img, each row as 32-k blocks
  of 32 bf16 hi then 32 bf16 lo — the very hi/lo operands the x3 MFMAs consume
  (hi + lo = the fp32 value to ~2^-17) — written by the stage-0 epilogue and
  staged into LDS by DMA in fc1 (no register split pass): fc1 0.710 -> 0.632
  ms at B=65536 with bit-identical outputs (profiles/r3_fc1_split_ab.jsonl),
  but the split stores cost the stage-0 epilogue as much, so the 2-stage step
  is unchanged (2.541 vs 2.548 ms, profiles/r3_boundary_ab.jsonl) and the
  pipelines keep plain fp32 (also the wire format a reference peer expects).
  ``decode_boundary`` / ``encode_boundary`` convert.
* ``bf16``: ``csrc/kernels/cifar_fused.hip`` (v4 persistent kernel), bf16
  boundary, an explicitly reduced-precision mode.

Weight layouts:

* conv1 ``(32,3,3,3)`` -> ``[32][48]`` with ``k = ky*16 + kx*4 + c`` (kx<3, c<3 real): the
  bf16 kernel and the fp32 kernel's ``k48`` arm; and, for the fp32 kernel's default ``k32`` arm
  (``STAGE0_CONV1``), ``[2 x parity][32][32]`` with ``k = conv1_k32_slot(ky, p + kx*3 + c)``,
  p = 1 for even x and 0 for odd x, every other slot zero (``_conv1_k32``);
* conv2 ``(64,32,3,3)`` -> ``[64][288]`` with ``k = (ky*3+kx)*32 + c`` (HWC activation image);
* fc1 ``[512][4096]`` (K-contiguous for the GEMM), fc2 ``(10,512)`` -> ``[16][512]``
  zero-padded to one MFMA N-tile.  Biases are fp32.
The flatten order is the reference's NCHW ``c*64 + h*8 + w`` (``cifar_model_parts.py:41``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from ._lib import check, lib, ptr, stream_ptr
from .gemm import ACT_RELU, linear

PRECISIONS = ("fp32", "bf16")


def split_bf16(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 -> (hi, lo) bf16 with hi + lo == w to ~2^-17 relative."""
    w = w.float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi, lo


def _conv1_k48(sd) -> torch.Tensor:
    w = torch.zeros(32, 3, 4, 4)  # (oc, ky, kx, c) zero-padded kx=3, c=3
    w[:, :, :3, :3] = sd["conv1.weight"].float().permute(0, 2, 3, 1)
    return w.reshape(32, 48)


def conv1_k32_slot(ky: int, e: int) -> int:
    """K index of element ``e`` (0..9) of the 5-dword read of padded input row
    ``ky`` in the K = 32 conv1 (``cifar_x3.hip``, "conv1 on K = 32"): the MFMA's
    k is ``16*step + 8*half + 0..7``; lane half 0 holds dwords 0-3 of rows 0
    (step 0) and 1 (step 1), half 1 dwords 0-3 of row 2 (step 0) and dword 4 of
    rows 0, 1, 2 (step 1).  K slots 30 and 31 are filler."""
    if e < 8:
        return (0, 16, 8)[ky] + e
    return 24 + 2 * ky + (e - 8)


def _conv1_k32(sd) -> torch.Tensor:
    """conv1 ``(32,3,3,3)`` -> ``[2 x parity][32 oc][32 k]``.  An input row is
    one zero element, then 34 pixels x 3 channels; pixel x's 9-element window of
    one ky starts at element 3x + 1, and the 4-byte-aligned 10-element read that
    covers it starts at 3x (even x: window at e = 1..9, e = 0 junk) or 3x + 1
    (odd x: window at e = 0..8, e = 9 junk).  Junk and filler slots stay zero."""
    w = sd["conv1.weight"].float()  # (oc, c, ky, kx)
    out = torch.zeros(2, 32, 32)
    for par in range(2):
        for ky in range(3):
            for kx in range(3):
                for c in range(3):
                    out[par, :, conv1_k32_slot(ky, (1 - par) + kx * 3 + c)] = w[:, c, ky, kx]
    return out


def _conv2_k288(sd) -> torch.Tensor:
    return sd["conv2.weight"].float().permute(0, 2, 3, 1).reshape(64, 288)  # (oc, ky, kx, c)


def _fc2_pad(sd) -> torch.Tensor:
    w = torch.zeros(16, 512)
    w[:10] = sd["fc2.weight"].float()
    return w


@dataclass
class CifarStage0Weights:
    precision: str
    b1: torch.Tensor
    b2: torch.Tensor
    w1: torch.Tensor = None    # bf16: [32][48]
    w2: torch.Tensor = None    # bf16: [64][288]
    w1h: torch.Tensor = None   # fp32 path: split conv weights
    w1l: torch.Tensor = None
    w2h: torch.Tensor = None
    w2l: torch.Tensor = None
    w1h32: torch.Tensor = None  # fp32 path: conv1 in the K = 32 packing [2][32][32]
    w1l32: torch.Tensor = None


@dataclass
class CifarHeadWeights:
    precision: str
    w_fc1: torch.Tensor = None   # bf16: [512][4096]; fp32: [512][3*4096] = [hi | lo | hi] (small batch)
    w_fc1h: torch.Tensor = None  # fp32 path, large batch: W hi / lo [512][4096] each (cifar_fc1_x3)
    w_fc1l: torch.Tensor = None
    b_fc1: torch.Tensor = None
    w_fc2: torch.Tensor = None   # bf16: [16][512]
    w_fc2h: torch.Tensor = None  # fp32 path: split fc2
    w_fc2l: torch.Tensor = None
    b_fc2: torch.Tensor = None


def _check_precision(p: str) -> str:
    if p not in PRECISIONS:
        raise ValueError(f"CIFAR precision must be one of {PRECISIONS}, got {p!r}")
    return p


def pack_stage0(sd: Dict[str, torch.Tensor], device, precision: str = "fp32") -> CifarStage0Weights:
    _check_precision(precision)
    b1 = sd["conv1.bias"].float().to(device).contiguous()
    b2 = sd["conv2.bias"].float().to(device).contiguous()
    w1, w2 = _conv1_k48(sd), _conv2_k288(sd)
    if precision == "bf16":
        return CifarStage0Weights("bf16", b1, b2,
                                  w1=w1.to(device=device, dtype=torch.bfloat16).contiguous(),
                                  w2=w2.to(device=device, dtype=torch.bfloat16).contiguous())
    (w1h, w1l), (w2h, w2l) = split_bf16(w1), split_bf16(w2)
    w1h32, w1l32 = split_bf16(_conv1_k32(sd))
    dv = lambda t: t.to(device).contiguous()  # noqa: E731
    return CifarStage0Weights("fp32", b1, b2, w1h=dv(w1h), w1l=dv(w1l), w2h=dv(w2h), w2l=dv(w2l),
                              w1h32=dv(w1h32), w1l32=dv(w1l32))


def pack_head(sd: Dict[str, torch.Tensor], device, fc1: bool = True, fc2: bool = True,
              precision: str = "fp32") -> CifarHeadWeights:
    _check_precision(precision)
    w = CifarHeadWeights(precision)
    if fc1:
        f = sd["fc1.weight"].float()
        if precision == "bf16":
            w.w_fc1 = f.to(device=device, dtype=torch.bfloat16).contiguous()
        else:
            hi, lo = split_bf16(f)
            w.w_fc1 = torch.cat([hi, lo, hi], dim=1).to(device).contiguous()
            w.w_fc1h, w.w_fc1l = hi.to(device).contiguous(), lo.to(device).contiguous()
        w.b_fc1 = sd["fc1.bias"].float().to(device).contiguous()
    if fc2:
        f2 = _fc2_pad(sd)
        if precision == "bf16":
            w.w_fc2 = f2.to(device=device, dtype=torch.bfloat16).contiguous()
        else:
            hi, lo = split_bf16(f2)
            w.w_fc2h, w.w_fc2l = hi.to(device).contiguous(), lo.to(device).contiguous()
        w.b_fc2 = sd["fc2.bias"].float().to(device).contiguous()
    return w


def act_dtype(precision: str) -> torch.dtype:
    """dtype of the stage-boundary activations (flattened conv map, fc1 hidden)."""
    return torch.float32 if _check_precision(precision) == "fp32" else torch.bfloat16


STAGE0_GRID = 0  # persistent stage-0 workgroups; 0 = one per CU (256)
# fused fp32 fc1 from this batch on: 2 x B/256 tiles of 128 k32 steps each need
# >= 128 tiles to occupy the chip; below, split3 + the K-concat GEMM is faster
FC1_X3_MIN_ROWS = 16384


def set_stage0_grid(grid: int = 0) -> None:
    """Persistent stage-0 grid size (0 = one workgroup per CU).  With fewer
    workgroups than CUs the spare CUs stay free for concurrent kernels (an RCCL
    hop kernel cannot start a workgroup on a CU the stage-0 kernel holds)."""
    global STAGE0_GRID
    STAGE0_GRID = int(grid)


STAGE0_MFMA = {"32x32x16": 0, "16x16x32": 1}  # compiled conv2 consumer paths (fp32); 1 is the default


def set_stage0_mfma(shape) -> int:
    """Select the MFMA shape of the fp32 stage-0 conv2 consumer (a key or value
    of ``STAGE0_MFMA``); returns the previous setting so callers can restore it."""
    v = STAGE0_MFMA[shape] if isinstance(shape, str) else int(shape)
    prev = lib().cifar_s0_get_mfma()
    check(lib().cifar_s0_set_mfma(v), "cifar_s0_set_mfma")
    return prev


def set_stage0_wide_store(on) -> int:
    """Boundary stores of the 32x32x16 conv2 consumer: 16-byte (1, the default) or
    8-byte (0); the 16x16x32 consumer ignores it.  Returns the previous setting so
    callers can restore it."""
    prev = lib().cifar_s0_get_wide_store()
    check(lib().cifar_s0_set_wide_store(int(bool(on))), "cifar_s0_set_wide_store")
    return prev


STAGE0_CONV1 = {"k48": 0, "k32": 1}  # compiled conv1 producer paths (fp32); 1 is the default


def set_stage0_conv1(packing) -> int:
    """Select the K packing of the fp32 stage-0 conv1 producer (a key or value
    of ``STAGE0_CONV1``); returns the previous setting so callers can restore it."""
    v = STAGE0_CONV1[packing] if isinstance(packing, str) else int(packing)
    prev = lib().cifar_s0_get_conv1()
    check(lib().cifar_s0_set_conv1(v), "cifar_s0_set_conv1")
    return prev


# compiled k-loop arms of the fused fp32 fc1 (cifar_fc1_x3), both on the staggered schedule; "lean"
# adds the packed bf16 split and loop-invariant buffer addressing (the default)
FC1_SCHED = {"staggered": 1, "lean": 2}


def set_fc1_sched(sched) -> int:
    """Select the k-loop schedule of the fused fp32 fc1 (a key or value of
    ``FC1_SCHED``); returns the previous setting so callers can restore it."""
    v = FC1_SCHED[sched] if isinstance(sched, str) else int(sched)
    prev = lib().cifar_fc1_get_sched()
    check(lib().cifar_fc1_set_sched(v), "cifar_fc1_set_sched")
    return prev


def _check_act(t: torch.Tensor, shape, dtype, what: str) -> None:
    if t.dtype != dtype or tuple(t.shape[1:]) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what}: expected contiguous {dtype} (B,{','.join(map(str, shape))}), "
                         f"got {t.dtype} {tuple(t.shape)}")


BOUNDARIES = ("fp32", "split")


def _split_boundary(boundary: str, precision: str) -> int:
    if boundary not in BOUNDARIES:
        raise ValueError(f"boundary must be one of {BOUNDARIES}, got {boundary!r}")
    if boundary == "split" and precision != "fp32":
        raise ValueError("the split boundary encoding exists for the fp32 precision only")
    return int(boundary == "split")


def encode_boundary(h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 (B,K) -> the blocked hi/lo boundary encoding (same shape and dtype)."""
    out = torch.empty_like(h) if out is None else out
    check(lib().cifar_split_blocked(ptr(h), ptr(out), h.shape[0], h.shape[1], 0, stream_ptr()), "encode_boundary")
    return out


def decode_boundary(h: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Blocked hi/lo boundary encoding -> fp32 values (hi + lo)."""
    out = torch.empty_like(h) if out is None else out
    check(lib().cifar_split_blocked(ptr(h), ptr(out), h.shape[0], h.shape[1], 1, stream_ptr()), "decode_boundary")
    return out


# ---------------------------------------------------------------------------
# uint8 input.  A CIFAR image exists as (32,32,3) bytes; its normalisation is a
# per-channel function of a byte, so it is a (3,256) table, and the table *is*
# the definition of the transform.  The fp32 stage-0 kernel looks the bytes up
# while it stages them (cifar_x3.hip, "uint8 input"): 3 KiB/img instead of 12.
# ---------------------------------------------------------------------------
INPUT_DTYPES = ("fp32", "uint8")


def make_input_table(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """``(3,256)`` fp32 CPU tensor: entry ``[c][b]`` is byte ``b`` of channel ``c`` after
    ``ToTensor`` and ``Normalize(mean, std)``, in their fp32 arithmetic
    (``(b / 255 - mean[c]) / std[c]``; ``cli.load_image`` computes the same bits)."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f"input table: mean and std need three entries each, got {mean!r}, {std!r}")
    if any(float(s) == 0.0 for s in std):
        raise ValueError(f"input table: std must be nonzero, got {std!r}")
    b = torch.arange(256, dtype=torch.float32).div(255)
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).view(3, 1)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32).view(3, 1)
    return ((b.view(1, 256) - m) / s).contiguous()


def _check_table(table: torch.Tensor) -> None:
    if tuple(table.shape) != (3, 256) or table.dtype != torch.float32:
        raise ValueError(f"input table: expected (3,256) fp32, got {table.dtype} {tuple(table.shape)}")


def pack_input_table(table: torch.Tensor, device) -> torch.Tensor:
    """``(3,256)`` fp32 -> ``(3,256)`` int32 on ``device``, the kernel's form: the low 16 bits
    of an entry are the bf16 bits of ``hi = bf16(t)``, the high 16 bits those of
    ``lo = bf16(t - hi)`` (``split_bf16``), exactly what the kernel's ``split2<true>`` gives
    for the float ``t``.  Entries are expected to be 0 or of magnitude >= 2^-100: the residue
    of a smaller one is denormal, and denormal residues are not part of the contract."""
    _check_table(table)
    hi, lo = split_bf16(table.detach().cpu())
    hb = hi.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    lb = lo.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    packed = hb | (lb << 16)  # int32 wraps: bit 31 is lo's sign
    return packed.to(torch.int32).to(device).contiguous()


def normalize_u8(x_u8: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """``(B,32,32,3)`` uint8 -> ``(B,3,32,32)`` fp32 by gather from the ``(3,256)`` fp32
    ``table``: the torch mirror of the kernel's lookup (CPU path, tests)."""
    _check_table(table)
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or tuple(x_u8.shape[1:]) != (32, 32, 3):
        raise ValueError(f"normalize_u8: expected uint8 (B,32,32,3), got {x_u8.dtype} {tuple(x_u8.shape)}")
    t = table.to(x_u8.device)
    idx = x_u8.permute(0, 3, 1, 2).long()  # (B,3,32,32)
    out = torch.empty(idx.shape, dtype=torch.float32, device=x_u8.device)
    for c in range(3):
        out[:, c] = t[c][idx[:, c]]
    return out


def _stage0_u8(x: torch.Tensor, w: CifarStage0Weights, table: Optional[torch.Tensor], out: Optional[torch.Tensor],
               grid: int, split: int) -> torch.Tensor:
    """The uint8 arm of ``stage0_forward``: every rejection is raised before the launch."""
    if w.precision != "fp32":
        raise ValueError("stage0: uint8 input exists for the fp32 precision only (the bf16 kernel has no table path)")
    if table is None:
        raise ValueError("stage0: uint8 input needs a packed input table (pack_input_table(make_input_table(), device))")
    if table.dtype != torch.int32 or tuple(table.shape) != (3, 256) or not table.is_contiguous() \
            or table.device != x.device:
        raise ValueError(f"stage0: the input table must be a packed (3,256) int32 tensor on {x.device} "
                         f"(pack_input_table), got {table.dtype} {tuple(table.shape)} on {table.device}")
    if x.dim() != 4 or tuple(x.shape[1:]) != (32, 32, 3):
        raise ValueError(f"stage0: uint8 input must be NHWC (B,32,32,3), got {tuple(x.shape)}"
                         + (" (NCHW: permute(0,2,3,1) first)" if tuple(x.shape[1:]) == (3, 32, 32) else ""))
    if not x.is_contiguous():
        raise ValueError("stage0: uint8 input must be contiguous")
    if x.data_ptr() % 4:
        raise ValueError(f"stage0: uint8 input must be 4-byte aligned (the kernel loads dwords), "
                         f"data_ptr {x.data_ptr():#x} is misaligned")
    if lib().cifar_s0_get_conv1() != STAGE0_CONV1["k32"]:
        raise ValueError("stage0: uint8 input exists on the k32 conv1 arm only; the conv1 switch is on k48 "
                         "(set_stage0_conv1('k32'))")
    B = x.shape[0]
    if out is None:
        out = torch.empty((B, 4096), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, 4096) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("stage0: bad output buffer")
    rc = lib().cifar_stage0_x3_u8(ptr(x), ptr(table), ptr(out), ptr(w.w1h32), ptr(w.w1l32), ptr(w.b1), ptr(w.w2h),
                                  ptr(w.w2l), ptr(w.b2), B, grid, stream_ptr(), split)
    if rc < 0:  # the library's own rejections, for a caller that raced the checks above
        why = {-1: "a null table or weight pointer", -2: "the conv1 switch is on k48", -3: "misaligned input or table"}
        raise ValueError(f"stage0: uint8 launch rejected: {why.get(rc, rc)}")
    check(rc, "cifar_stage0_x3_u8")
    return out


def stage0_forward(x: torch.Tensor, w: CifarStage0Weights, out: Optional[torch.Tensor] = None,
                   grid: int = 0, boundary: str = "fp32", table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Units 0-1: x (B,3,32,32) fp32 contiguous -> (B,4096) fp32 (or bf16 in bf16 mode;
    ``boundary="split"``: the blocked hi/lo encoding in the fp32 tensor).  Or x (B,32,32,3)
    uint8 contiguous with a 4-byte-aligned ``data_ptr`` and ``table`` = its packed
    normalisation table (``pack_input_table``; fp32 precision, ``k32`` conv1 arm): the
    result is bitwise that of the fp32 input ``normalize_u8(x, table)``."""
    split = _split_boundary(boundary, w.precision)
    grid = grid or STAGE0_GRID
    if x.dtype == torch.uint8:
        return _stage0_u8(x, w, table, out, grid, split)
    _check_act(x, (3, 32, 32), torch.float32, "stage0 input")
    B = x.shape[0]
    dt = act_dtype(w.precision)
    if out is None:
        out = torch.empty((B, 4096), dtype=dt, device=x.device)
    if tuple(out.shape) != (B, 4096) or out.dtype != dt or not out.is_contiguous():
        raise ValueError("stage0: bad output buffer")
    if w.precision == "fp32":
        check(lib().cifar_stage0_x3(ptr(x), ptr(out), ptr(w.w1h), ptr(w.w1l), ptr(w.b1), ptr(w.w2h), ptr(w.w2l),
                                    ptr(w.b2), B, grid, stream_ptr(), split, ptr(w.w1h32), ptr(w.w1l32)),
              "cifar_stage0_x3")
    else:
        check(lib().cifar_stage0_v4(ptr(x), ptr(out), ptr(w.w1), ptr(w.b1), ptr(w.w2), ptr(w.b2), B, grid,
                                    stream_ptr()), "cifar_stage0_v4")
    return out


def fc1_forward(h: torch.Tensor, w: CifarHeadWeights, out: Optional[torch.Tensor] = None,
                scratch: Optional[torch.Tensor] = None, boundary: str = "fp32") -> torch.Tensor:
    """Unit 2: (B,4096) -> relu(fc1) (B,512) on the MFMA GEMM (fp32: split operand,
    ``scratch`` = (>=B, 12288) bf16 for the [hi | hi | lo] rows; ``boundary``:
    the encoding of ``h``)."""
    split = _split_boundary(boundary, w.precision)
    dt = act_dtype(w.precision)
    _check_act(h, (4096,), dt, "fc1 input")
    B = h.shape[0]
    if w.precision == "bf16":
        return linear(h, w.w_fc1, w.b_fc1, act=ACT_RELU, out=out)
    if B >= FC1_X3_MIN_ROWS:
        if out is None:
            out = torch.empty((B, 512), dtype=torch.float32, device=h.device)
        check(lib().cifar_fc1_x3(ptr(h), 4096, ptr(w.w_fc1h), ptr(w.w_fc1l), 4096, ptr(w.b_fc1), ptr(out), 512,
                                 B, 512, 4096, stream_ptr(), split), "cifar_fc1_x3")
        return out
    if scratch is None or scratch.shape[0] < B or tuple(scratch.shape[1:]) != (3 * 4096,):
        scratch = torch.empty((B, 3 * 4096), dtype=torch.bfloat16, device=h.device)
    a3 = scratch[:B]
    check(lib().cifar_split3(ptr(h), 4096, ptr(a3), 3 * 4096, B, 4096, stream_ptr(), split), "cifar_split3")
    if out is None:
        out = torch.empty((B, 512), dtype=torch.float32, device=h.device)
    return linear(a3, w.w_fc1, w.b_fc1, act=ACT_RELU, out=out)


def head_tail(hid: torch.Tensor, w: CifarHeadWeights, probs: Optional[torch.Tensor] = None,
              pred: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Unit 3: (B,512) -> fc2 + softmax (B,10) fp32 + per-row argmax (B,) int32."""
    _check_act(hid, (512,), act_dtype(w.precision), "head_tail input")
    B = hid.shape[0]
    probs = probs if probs is not None else torch.empty((B, 10), dtype=torch.float32, device=hid.device)
    pred = pred if pred is not None else torch.empty((B,), dtype=torch.int32, device=hid.device)
    if w.precision == "fp32":
        check(lib().cifar_head_tail_x3(ptr(hid), ptr(w.w_fc2h), ptr(w.w_fc2l), ptr(w.b_fc2), ptr(probs), ptr(pred),
                                       B, stream_ptr()), "cifar_head_tail_x3")
    else:
        check(lib().cifar_head_tail(ptr(hid), ptr(w.w_fc2), ptr(w.b_fc2), ptr(probs), ptr(pred), B, stream_ptr()),
              "cifar_head_tail")
    return probs, pred


def head_forward(h: torch.Tensor, w: CifarHeadWeights, hid: Optional[torch.Tensor] = None,
                 probs: Optional[torch.Tensor] = None, pred: Optional[torch.Tensor] = None,
                 boundary: str = "fp32") -> Tuple[torch.Tensor, torch.Tensor]:
    """Units 2-3: h (B,4096) -> (probs (B,10) fp32, pred (B,) int32)."""
    hid = fc1_forward(h, w, out=hid, boundary=boundary)
    return head_tail(hid, w, probs, pred)
