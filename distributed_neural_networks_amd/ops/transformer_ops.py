"""Thin wrappers over the transformer kernels (norms, embedding, attention,
sampler, fp8).  Shapes are validated on the host before launch — a kernel is
only ever launched with the operand shapes its grid assumes."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..config import (CON_MAX_BAD_LEN, CON_MAX_BAD_WORDS, CON_MAX_BIAS, CON_MAX_NGRAM, LOGPROBS_MAX_N, STOP_MAX_IDS,
                      STOP_MAX_SEQ_LEN, STOP_MAX_SEQS)

STOP_STATE_WORDS = 18  # csrc/kernels/api.h DNN_STOP_STATE_WORDS
from ._lib import check, lib, ptr, stream_ptr


def _bf16_2d(x: torch.Tensor, name: str) -> None:
    if x.dtype != torch.bfloat16 or x.stride(-1) != 1:
        raise ValueError(f"{name}: expected bf16 with contiguous last dim, got {x.dtype} strides {x.stride()}")


def layernorm(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], out: torch.Tensor, eps: float = 1e-5,
              rms: bool = False, rows: Optional[int] = None, ldx: Optional[int] = None) -> torch.Tensor:
    """Row-wise LayerNorm (rms=False, with bias) or RMSNorm over the last dim.
    ``rows``/``ldx`` allow normalising a strided subset of rows (e.g. the last
    position of every sequence: ldx = T*d, x pointing at row T-1)."""
    _bf16_2d(x, "layernorm")
    N = x.shape[-1]
    M = rows if rows is not None else x.numel() // N
    ldx = ldx if ldx is not None else N
    if w.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise TypeError("layernorm: fp32 weight/bias expected")
    if N % 8 or N > 8192:
        raise ValueError(f"layernorm: unsupported width {N}")
    if out.numel() < M * N:
        raise ValueError("layernorm: output too small")
    check(lib().layernorm(ptr(x), ldx, ptr(w), ptr(b), ptr(out), N, M, N, eps, 1 if rms else 0, stream_ptr()),
          "layernorm")
    return out


def row_stats(x: torch.Tensor, stats: torch.Tensor, eps: float = 1e-5, rms: bool = False, rows: Optional[int] = None,
              ldx: Optional[int] = None) -> torch.Tensor:
    """Per-row {rstd, -mean * rstd} (fp32 (M, 2); RMSNorm: {rstd, 0}) of a bf16
    (M, N) activation: the statistics a folded-norm GEMM applies in its epilogue."""
    _bf16_2d(x, "row_stats")
    N = x.shape[-1]
    M = rows if rows is not None else x.numel() // N
    ldx = ldx if ldx is not None else N
    if stats.dtype != torch.float32 or stats.numel() < 2 * M or not stats.is_contiguous():
        raise ValueError("row_stats: stats must be contiguous fp32 with 2 * M entries")
    if N % 8 or N > 8192:
        raise ValueError(f"row_stats: unsupported width {N}")
    check(lib().row_stats(ptr(x), ldx, ptr(stats), M, N, eps, 1 if rms else 0, stream_ptr()), "row_stats")
    return stats


def layernorm_q8(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], q_out: torch.Tensor,
                 s_out: torch.Tensor, kpad: int, eps: float = 1e-5, rms: bool = False, rows: Optional[int] = None,
                 ldx: Optional[int] = None, split: bool = False) -> torch.Tensor:
    """Normalise rows and quantise them to e4m3 with per-row scales in one pass
    (the ``quant_rows`` layout: q_out (M, kpad) bytes, K padding zeroed; s_out (M,);
    ``split``: (M, 2 kpad), the residual plane after the hi bytes, ``fp8.attach_split``)."""
    _bf16_2d(x, "layernorm_q8")
    N = x.shape[-1]
    M = rows if rows is not None else x.numel() // N
    ldx = ldx if ldx is not None else N
    if w.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise TypeError("layernorm_q8: fp32 weight/bias expected")
    if N % 8 or N > 8192 or kpad < N or kpad % 8:
        raise ValueError(f"layernorm_q8: unsupported width {N} / kpad {kpad}")
    ldq = kpad * (2 if split else 1)
    if q_out.numel() * q_out.element_size() < M * ldq or s_out.numel() < M:
        raise ValueError("layernorm_q8: output too small")
    check(lib().layernorm_q8(ptr(x), ldx, ptr(w), ptr(b), ptr(q_out), ldq, ptr(s_out), M, N, kpad, eps,
                             1 if rms else 0, stream_ptr(), int(split)), "layernorm_q8")
    return q_out


def layernorm_q8_mx(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], q_out: torch.Tensor,
                    sx_out: torch.Tensor, kpad: int, eps: float = 1e-5, rms: bool = False,
                    rows: Optional[int] = None, ldx: Optional[int] = None) -> torch.Tensor:
    """``layernorm_q8`` with MX scales: one e8m0 byte per (row, 128 columns)
    in ``sx_out`` (``fp8.mx_scale_bytes``; csrc/kernels/common.h mx_index)
    instead of a per-row fp32 scale — the input layout of ``fp8.linear_fp8(...,
    sx=)``."""
    from .fp8 import mx_scale_bytes
    _bf16_2d(x, "layernorm_q8_mx")
    N = x.shape[-1]
    M = rows if rows is not None else x.numel() // N
    ldx = ldx if ldx is not None else N
    if w.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise TypeError("layernorm_q8_mx: fp32 weight/bias expected")
    if N % 8 or N > 8192 or kpad < N or kpad % 128:
        raise ValueError(f"layernorm_q8_mx: unsupported width {N} / kpad {kpad}")
    if q_out.numel() * q_out.element_size() < M * kpad or sx_out.numel() * sx_out.element_size() < mx_scale_bytes(M, kpad):
        raise ValueError("layernorm_q8_mx: output too small")
    check(lib().layernorm_q8_mx(ptr(x), ldx, ptr(w), ptr(b), ptr(q_out), kpad, ptr(sx_out), M, N, kpad, eps,
                                1 if rms else 0, stream_ptr()), "layernorm_q8_mx")
    return q_out


def embed(idx: torch.Tensor, wte: torch.Tensor, wpe: Optional[torch.Tensor], out: torch.Tensor,
          pos: Optional[torch.Tensor]) -> torch.Tensor:
    """out[b*T+t] = wte[idx[b,t]] (+ wpe[pos[b]+t]). idx int32 (B,T)."""
    if idx.dtype != torch.int32 or idx.dim() != 2:
        raise ValueError("embed: idx must be int32 (B,T)")
    B, T = idx.shape
    d = wte.shape[1]
    if out.numel() < B * T * d:
        raise ValueError("embed: output too small")
    check(lib().embed_gpt2(ptr(idx), ptr(wte), ptr(wpe), ptr(out), B, T, d, ptr(pos), wte.shape[0],
                           0 if wpe is None else wpe.shape[0], stream_ptr()), "embed")
    return out


KV8_DTYPES = (torch.float8_e4m3fn, torch.uint8)  # e4m3 KV cache storage (unit scale)


def _kv8(kc: torch.Tensor, vc: torch.Tensor) -> int:
    """1 for an OCP e4m3 KV cache (decode attention / QKV-mode prefill read and
    write it as bytes, attention.hip KV8), 0 for bf16."""
    k8, v8 = kc.dtype in KV8_DTYPES, vc.dtype in KV8_DTYPES
    if k8 != v8:
        raise TypeError("K and V caches must share a dtype")
    if not k8 and kc.dtype != torch.bfloat16:
        raise TypeError(f"KV cache dtype {kc.dtype}: bf16 or float8_e4m3fn")
    return 1 if k8 else 0


def qkv_split(qkv: torch.Tensor, q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, B: int, T: int, H: int,
              Hkv: int, hd: int, pos: torch.Tensor, cos: Optional[torch.Tensor] = None,
              sin: Optional[torch.Tensor] = None) -> None:
    S = kc.shape[2]
    if kc.shape[:2] != (B, Hkv) or kc.shape[3] != hd or vc.shape != kc.shape:
        raise ValueError(f"qkv_split: cache {tuple(kc.shape)} does not match B={B} Hkv={Hkv} hd={hd}")
    if qkv.numel() < B * T * (H + 2 * Hkv) * hd or q.numel() < B * T * H * hd:
        raise ValueError("qkv_split: buffers too small")
    rope = cos is not None
    check(lib().qkv_split(ptr(qkv), ptr(q), ptr(kc), ptr(vc), B, T, H, Hkv, hd, S, ptr(pos), ptr(cos), ptr(sin),
                          1 if rope else 0, stream_ptr(), kv8=_kv8(kc, vc)), "qkv_split")


def flash_attn(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, out: torch.Tensor, B: int, T: int, H: int,
               Hkv: int, hd: int, pos: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """Causal attention of T new queries per sequence against the cache
    (positions 0..pos[b]+T-1). q (B,H,T,hd); out (B*T, H*hd)."""
    if hd not in (64, 128):
        raise ValueError(f"flash_attn: head_dim {hd} unsupported (64/128)")
    S = kc.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    check(lib().flash_attn(ptr(q), ptr(kc), ptr(vc), ptr(out), B, T, H, Hkv, hd, S, ptr(pos), scale, stream_ptr(),
                           kv8=_kv8(kc, vc)), "flash_attn")
    return out


def flash_attn_qkv(qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, out: torch.Tensor, B: int, T: int, H: int,
                   Hkv: int, hd: int, pos: torch.Tensor, scale: Optional[float] = None) -> torch.Tensor:
    """Causal prefill straight from the c_attn output (no RoPE): qkv (B*T, ld)
    rows [q | k | v]; the new keys/values are written into the cache rows
    pos[b].. as a side effect (what qkv_split would have done)."""
    if hd not in (64, 128):
        raise ValueError(f"flash_attn_qkv: head_dim {hd} unsupported (64/128)")
    S = kc.shape[2]
    if kc.shape[:2] != (B, Hkv) or kc.shape[3] != hd or vc.shape != kc.shape:
        raise ValueError(f"flash_attn_qkv: cache {tuple(kc.shape)} does not match B={B} Hkv={Hkv} hd={hd}")
    if qkv.dim() != 2 or qkv.shape[0] < B * T or qkv.shape[1] < (H + 2 * Hkv) * hd or qkv.stride(1) != 1:
        raise ValueError(f"flash_attn_qkv: qkv {tuple(qkv.shape)} too small")
    if not (kc.is_contiguous() and vc.is_contiguous()):
        raise ValueError("flash_attn_qkv: cache slices must be contiguous")
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    check(lib().flash_attn_qkv(ptr(qkv), qkv.stride(0), ptr(kc), ptr(vc), ptr(out), B, T, H, Hkv, hd, S, ptr(pos),
                               scale, stream_ptr(), kv8=_kv8(kc, vc)), "flash_attn_qkv")
    return out


DEC_LDS_SCORES = 160 * 1024 // 4  # fp32 scores one decode-attention workgroup can hold in LDS


def decode_splits(S: int, B: int, Hkv: int, G: int = 1) -> int:
    """Split-K factor for decode attention: one split once B*Hkv alone gives 2
    workgroups per CU; else enough workgroups for ~4 per CU (1024), at most one
    split per 256 keys of cache capacity.  Each split takes
    ``ceil(len/splits)`` of the *runtime* length, so short contexts stay
    balanced; with one split the kernel writes the output itself (no combine).
    Long contexts: a split keeps its G x chunk scores in LDS (160 KiB), so the
    split count never drops below ceil(S / floor(40960 / G)) (14 for a 128 K-token
    Llama-3 cache, G = 4), whatever the batch."""
    lds_min = max(1, -(-S // (DEC_LDS_SCORES // max(1, G))))  # ceil(S/splits) * G <= 40960
    if B * Hkv >= 512:  # >= 2 workgroups per CU already: the combine pass costs more than it hides
        return lds_min    # (GPT-2 B=64: 0.754 -> 0.703 ms/step, profiles/archive/r1_decode_benches_v6.jsonl)
    want = max(1, -(-1024 // max(1, B * Hkv)))
    return max(lds_min, min(want, -(-S // 256)))  # >= 256 keys per split: short contexts skip the combine


def attn_decode(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, out: torch.Tensor, B: int, H: int, Hkv: int,
                hd: int, lens: torch.Tensor, ws: torch.Tensor, splits: int, scale: Optional[float] = None):
    S = kc.shape[2]
    G = H // Hkv
    need = B * Hkv * splits * G * (hd + 2)
    if ws.numel() < need or ws.dtype != torch.float32:
        raise ValueError(f"attn_decode: workspace needs {need} fp32")
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    check(lib().attn_decode(ptr(q), ptr(kc), ptr(vc), ptr(out), B, H, Hkv, hd, S, ptr(lens), scale, splits, ptr(ws),
                            stream_ptr(), kv8=_kv8(kc, vc)), "attn_decode")
    return out


def attn_decode_qkv(qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, out: torch.Tensor, B: int, H: int,
                    Hkv: int, hd: int, pos: torch.Tensor, ws: torch.Tensor, splits: int,
                    cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None,
                    scale: Optional[float] = None) -> torch.Tensor:
    """One decode step straight from the QKV projection rows (B, (H+2Hkv)*hd):
    RoPE (when cos/sin), the new k/v written into the cache at ``pos[b]`` and
    attention over ``pos[b]+1`` keys, in one launch (no qkv_split)."""
    S = kc.shape[2]
    if kc.shape[:2] != (B, Hkv) or kc.shape[3] != hd or vc.shape != kc.shape:
        raise ValueError(f"attn_decode_qkv: cache {tuple(kc.shape)} does not match B={B} Hkv={Hkv} hd={hd}")
    if qkv.dim() != 2 or qkv.shape[0] < B or qkv.shape[1] < (H + 2 * Hkv) * hd or qkv.stride(1) != 1:
        raise ValueError(f"attn_decode_qkv: qkv {tuple(qkv.shape)} too small")
    if out.numel() < B * H * hd or pos.numel() < B or pos.dtype != torch.int32:
        raise ValueError("attn_decode_qkv: bad out/pos")
    if cos is not None and (cos.shape[0] < S or cos.shape[1] != hd // 2):
        raise ValueError("attn_decode_qkv: RoPE table does not cover the cache")
    G = H // Hkv
    need = B * Hkv * splits * G * (hd + 2)
    if ws.numel() < need or ws.dtype != torch.float32:
        raise ValueError(f"attn_decode_qkv: workspace needs {need} fp32")
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    check(lib().attn_decode_qkv(ptr(qkv), qkv.stride(0), ptr(kc), ptr(vc), ptr(out), B, H, Hkv, hd, S, ptr(pos),
                                ptr(cos), ptr(sin), scale, splits, ptr(ws), stream_ptr(), kv8=_kv8(kc, vc)),
          "attn_decode_qkv")
    return out


ARGMAX_PART_PER_ROW = 64  # int2 partials per row of the row-split argmax workspace
ARGMAX_SPLIT = True  # use the workspace when one is given (A/B switch, bench/probes/decode_ab.py)


def check_hist(hist: Optional[torch.Tensor], advance: Optional[torch.Tensor], M: int, who: str) -> int:
    """Token-history buffer of the decode step tail: (>= M, L) int32, rows
    contiguous; needs ``advance`` (the positions it is indexed by).  Returns L."""
    if hist is None:
        return 0
    if advance is None:
        raise ValueError(f"{who}: hist needs advance (the positions)")
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] < M or hist.stride(1) != 1:
        raise ValueError(f"{who}: hist must be int32 (>= {M}, L) with contiguous rows")
    return hist.stride(0)


def argmax_rows(x: torch.Tensor, out: torch.Tensor, n: Optional[int] = None, also: Optional[torch.Tensor] = None,
                advance: Optional[torch.Tensor] = None, part: Optional[torch.Tensor] = None,
                hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-row argmax (ties -> smallest index) into ``out`` (int32).  Decode
    step tail in the same launch: ``also`` receives a copy of the ids,
    ``hist[row, advance[row]]`` the id (token history of a multi-step decode
    graph) and ``advance[row] += 1`` (int32 positions).  ``part`` (int32, >=
    128 M entries): workspace that lets small batches split each row over
    many workgroups (a partial and a merge launch, sampler.hip)."""
    M = x.shape[0]
    N = n if n is not None else x.shape[1]
    for t, nm in ((out, "out"), (also, "also"), (advance, "advance")):
        if t is not None and (t.dtype != torch.int32 or t.numel() < M or not t.is_contiguous()):
            raise ValueError(f"argmax_rows: {nm} must be contiguous int32 with >= {M} entries")
    hist_ld = check_hist(hist, advance, M, "argmax_rows")
    if part is not None and (part.dtype != torch.int32 or part.numel() < 2 * ARGMAX_PART_PER_ROW * M
                             or not part.is_contiguous()):
        raise ValueError(f"argmax_rows: part must be contiguous int32 with >= {2 * ARGMAX_PART_PER_ROW * M} entries")
    check(lib().argmax_rows(ptr(x), x.stride(0), M, N, ptr(out), 1 if x.dtype == torch.float32 else 0,
                            stream_ptr(), ptr(also), ptr(advance), ptr(part if ARGMAX_SPLIT else None), ptr(hist),
                            hist_ld), "argmax_rows")
    return out


def sample_topk(logits: torch.Tensor, out: torch.Tensor, n: int, temperature: float, top_k: int = 0, seed: int = 0,
                step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Temperature / top-k sampling per row (Gumbel-max over the k largest
    logits), bf16 logits only.  ``step`` (device int32 per row, e.g. the
    sequence position) decorrelates successive decode steps inside one graph."""
    if logits.dtype != torch.bfloat16:
        raise TypeError("sample_topk: bf16 logits expected")
    if not temperature > 0:
        raise ValueError("sample_topk: temperature must be > 0 (use argmax_rows for greedy)")
    M = logits.shape[0]
    check(lib().sample_topk(ptr(logits), logits.stride(0), M, n, ptr(out), float(temperature), int(top_k),
                            int(seed) & 0xFFFFFFFF, ptr(step), stream_ptr()), "sample_topk")
    return out


SAMPLE_FUSED_TAIL = True  # sampling last stage fuses the decode step tail (A/B switch, bench/probes/sample_decode_ab.py)


def sample_rows(logits: torch.Tensor, out: torch.Tensor, n: int, temperature: float, top_k: int = 0,
                top_p: float = 1.0, min_p: float = 0.0, seed: int = 0, step: Optional[torch.Tensor] = None,
                also: Optional[torch.Tensor] = None, advance: Optional[torch.Tensor] = None,
                hist: Optional[torch.Tensor] = None, thr_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Temperature -> top-k -> top-p (nucleus) -> min-p sampling per row of bf16
    logits (sample_filter.hip; ``runtime/sampling.sample_ref`` is the mirror),
    with the decode step tail of ``argmax_rows`` in the same launch: ``also``
    receives a copy of the ids, ``hist[row, advance[row]]`` the id and
    ``advance[row] += 1``.  ``step`` (device int32 per row) seeds the draw per
    decode step; it defaults to ``advance`` (the position before the
    increment).  ``thr_out`` (int32, tests): each row's final key threshold."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("sample_rows: bf16 (M, >= n) logits with contiguous rows expected")
    if not temperature > 0:
        raise ValueError("sample_rows: temperature must be > 0 (use argmax_rows for greedy)")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"sample_rows: top_p must be in (0, 1], got {top_p!r}")
    if not 0.0 <= min_p < 1.0:
        raise ValueError(f"sample_rows: min_p must be in [0, 1), got {min_p!r}")
    M = logits.shape[0]
    if not 0 < n <= logits.shape[1]:
        raise ValueError(f"sample_rows: n = {n} outside the row width {logits.shape[1]}")
    for t, nm in ((out, "out"), (also, "also"), (advance, "advance"), (step, "step"), (thr_out, "thr_out")):
        if t is not None and (t.dtype != torch.int32 or t.numel() < M or not t.is_contiguous()):
            raise ValueError(f"sample_rows: {nm} must be contiguous int32 with >= {M} entries")
    hist_ld = check_hist(hist, advance, M, "sample_rows")
    if step is None:
        step = advance
    check(lib().sample_rows(ptr(logits), logits.stride(0), M, n, ptr(out), float(temperature), int(top_k),
                            float(top_p), float(min_p), int(seed) & 0xFFFFFFFF, ptr(step), stream_ptr(), ptr(also),
                            ptr(advance), ptr(hist), hist_ld, ptr(thr_out)), "sample_rows")
    return out


def logit_penalties(logits: torch.Tensor, cnt: torch.Tensor, prev: Optional[torch.Tensor], rep: float, freq: float,
                    pres: float, n: int) -> torch.Tensor:
    """Repetition / presence / frequency penalties in place on the first ``n``
    entries of every row of bf16 ``logits`` (penalties.hip;
    ``runtime/sampling.apply_penalties_ref`` is the bitwise mirror).  ``cnt``
    (int16 / uint16, >= M rows, >= n wide): per entry bit 15 = in the prompt,
    bits 0..14 = times generated.  ``prev`` (int32 per row, or None): the token
    each row generated last; its count goes up by one first (out-of-range
    tokens are ignored)."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logit_penalties: bf16 (M, >= n) logits with contiguous rows expected")
    if cnt.dtype not in (torch.int16, torch.uint16) or cnt.dim() != 2 or cnt.stride(1) != 1:
        raise TypeError("logit_penalties: int16 / uint16 (M, >= n) state with contiguous rows expected")
    M = logits.shape[0]
    if not 0 < n <= logits.shape[1]:
        raise ValueError(f"logit_penalties: n = {n} outside the row width {logits.shape[1]}")
    if cnt.shape[0] < M or cnt.shape[1] < n:
        raise ValueError(f"logit_penalties: state {tuple(cnt.shape)} does not cover ({M}, {n})")
    ld, cnt_ld = (logits.stride(0), cnt.stride(0)) if M > 1 else (logits.shape[1], cnt.shape[1])
    if ld % 8 or cnt_ld % 8 or ld < n or cnt_ld < n or logits.data_ptr() % 16 or cnt.data_ptr() % 16:
        raise ValueError("logit_penalties: rows must start 16-byte aligned (row strides multiples of 8, >= n)")
    if prev is not None and (prev.dtype != torch.int32 or prev.numel() < M or not prev.is_contiguous()):
        raise ValueError(f"logit_penalties: prev must be contiguous int32 with >= {M} entries")
    rep, freq, pres = float(rep), float(freq), float(pres)
    if not (rep > 0 and math.isfinite(rep)):
        raise ValueError(f"logit_penalties: repetition penalty must be a finite number > 0, got {rep!r}")
    if not (math.isfinite(freq) and math.isfinite(pres)):
        raise ValueError(f"logit_penalties: frequency / presence penalties must be finite, got {freq!r}, {pres!r}")
    check(lib().logit_penalties(x=ptr(logits), ld=ld, M=M, N=n, cnt=ptr(cnt), cnt_ld=cnt_ld, prev=ptr(prev), rep=rep,
                                freq=freq, pres=pres, st=stream_ptr()), "logit_penalties")
    return logits




def logprobs_workspace(rows: int, n_vocab: int, n: int, device) -> torch.Tensor:
    """Zeroed workspace of ``logprobs_rows`` for up to ``rows`` rows of up to
    ``n_vocab`` logits and up to ``n`` alternatives: int32 (rows, words), one
    block per row: its arrival counter in the first 32 words (which the kernel
    leaves at zero and never uses for anything else) and the per-chunk partial
    results of one launch behind them.  A counter's place depends on the tensor
    alone, so calls on fewer rows, a smaller vocabulary or fewer alternatives
    may share one workspace; one launch at a time."""
    words = int(lib().logprobs_ws_row_words(N=int(n_vocab), n=int(n)))
    if rows <= 0 or words <= 0:
        raise ValueError(f"logprobs_workspace: unsupported rows {rows}, vocabulary {n_vocab} or n {n}")
    return torch.zeros((int(rows), words), dtype=torch.int32, device=device)


def logprobs_rows(logits: torch.Tensor, tokens: torch.Tensor, n_vocab: int, n: int, chosen: torch.Tensor,
                  top_ids: Optional[torch.Tensor], top_lps: Optional[torch.Tensor], ws: torch.Tensor,
                  pos: Optional[torch.Tensor] = None, pos_off: int = 0) -> None:
    """Log-probabilities of one step (logprobs.hip; ``runtime/sampling.logprobs_ref``
    is the fp64 mirror).  For every row of bf16 ``logits`` (M, >= n_vocab):
    ``lse = logsumexp`` over the first ``n_vocab`` entries, and at position
    ``p = pos[row] + pos_off`` (``pos`` None: ``pos_off``) of the histories
    ``chosen[row, p] = logits[row, tokens[row]] - lse`` (NaN for a token outside
    the vocabulary) and, with ``n`` >= 1, ``top_ids[row, p, :n]`` /
    ``top_lps[row, p, :n]`` = the ``n`` largest entries ordered by (value
    descending, index ascending).  ``chosen`` fp32 (>= M, L), ``top_ids`` int32
    and ``top_lps`` fp32 (>= M, L, >= n), all contiguous; a position outside
    [0, L) writes nothing.  ``pos_off = -1`` serves a step whose fused tail has
    advanced ``pos`` already.  ``ws``: ``logprobs_workspace``."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logprobs_rows: bf16 (M, >= n_vocab) logits with contiguous rows expected")
    M = logits.shape[0]
    if not 0 < n_vocab <= logits.shape[1]:
        raise ValueError(f"logprobs_rows: n_vocab = {n_vocab} outside the row width {logits.shape[1]}")
    n = int(n)
    if not 0 <= n <= min(LOGPROBS_MAX_N, n_vocab):
        raise ValueError(f"logprobs_rows: n = {n} outside [0, {min(LOGPROBS_MAX_N, n_vocab)}]")
    ld = logits.stride(0) if M > 1 else logits.shape[1]
    if ld % 8 or ld < n_vocab or logits.data_ptr() % 16:
        raise ValueError("logprobs_rows: rows must start 16-byte aligned (row stride a multiple of 8, >= n_vocab)")
    if tokens.dtype != torch.int32 or tokens.numel() < M or not tokens.is_contiguous():
        raise ValueError(f"logprobs_rows: tokens must be contiguous int32 with >= {M} entries")
    if pos is not None and (pos.dtype != torch.int32 or pos.numel() < M or not pos.is_contiguous()):
        raise ValueError(f"logprobs_rows: pos must be contiguous int32 with >= {M} entries")
    if chosen.dtype != torch.float32 or chosen.dim() != 2 or not chosen.is_contiguous() or chosen.shape[0] < M:
        raise ValueError(f"logprobs_rows: chosen must be contiguous fp32 (>= {M}, L), got {chosen.dtype} "
                         f"{tuple(chosen.shape)}")
    L = chosen.shape[1]
    top_ld = 0
    if n > 0:
        if top_ids is None or top_lps is None:
            raise ValueError("logprobs_rows: n >= 1 needs top_ids and top_lps")
        for t, dt, name in ((top_ids, torch.int32, "top_ids"), (top_lps, torch.float32, "top_lps")):
            if (t.dtype != dt or t.dim() != 3 or not t.is_contiguous() or t.shape[0] < M or t.shape[1] != L
                    or t.shape[2] < n):
                raise ValueError(f"logprobs_rows: {name} must be contiguous {dt} (>= {M}, {L}, >= {n}), got "
                                 f"{t.dtype} {tuple(t.shape)}")
        if top_ids.shape[2] != top_lps.shape[2]:
            raise ValueError("logprobs_rows: top_ids and top_lps differ in their last dimension")
        top_ld = top_ids.shape[2]
    need = int(lib().logprobs_ws_row_words(N=int(n_vocab), n=n))
    if (ws.dtype != torch.int32 or ws.dim() != 2 or not ws.is_contiguous() or ws.shape[0] < M or ws.shape[1] % 32
            or need <= 0 or ws.shape[1] < need):
        raise ValueError(f"logprobs_rows: workspace {ws.dtype} {tuple(ws.shape)}, contiguous int32 (>= {M}, >= {need}) "
                         f"needed (logprobs_workspace)")
    check(lib().logprobs_rows(x=ptr(logits), ld=ld, M=M, N=int(n_vocab), tok=ptr(tokens), pos=ptr(pos),
                              pos_off=int(pos_off), n=n, lp_hist=ptr(chosen), top_id_hist=ptr(top_ids if n else None),
                              top_lp_hist=ptr(top_lps if n else None), hist_ld=L, top_ld=top_ld, ws=ptr(ws),
                              ws_rows=ws.shape[0], ws_ld=ws.shape[1], st=stream_ptr()), "logprobs_rows")


def stop_state(rows: int, device) -> torch.Tensor:
    """The stop state of ``rows`` KV-cache rows at the beginning of a generation
    (stop.hip): int32 (rows, 18) = g, finish length, reason code and the
    15-entry window, the window all -1."""
    st = torch.zeros((int(rows), STOP_STATE_WORDS), dtype=torch.int32, device=device)
    st[:, 3:] = -1
    return st


def _stop_tables(stop_ids, stop_seqs, who: str):
    ids = [int(i) for i in stop_ids]
    seqs = [[int(e) for e in s] for s in stop_seqs]
    if len(ids) > STOP_MAX_IDS or len(seqs) > STOP_MAX_SEQS:
        raise ValueError(f"{who}: at most {STOP_MAX_IDS} stop ids and {STOP_MAX_SEQS} stop sequences, got {len(ids)} "
                         f"and {len(seqs)}")
    if any(not 1 <= len(s) <= STOP_MAX_SEQ_LEN for s in seqs):
        raise ValueError(f"{who}: a stop sequence holds 1..{STOP_MAX_SEQ_LEN} ids")
    if any(i < 0 for i in ids) or any(e < 0 for s in seqs for e in s):
        raise ValueError(f"{who}: negative id")
    return ids, seqs


def stop_rows(tokens: torch.Tensor, state: torch.Tensor, stop_ids, stop_seqs, min_new: int, pad: int,
              also: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None,
              pos: Optional[torch.Tensor] = None, pos_off: int = 0) -> None:
    """The stop launch of one step (stop.hip; ``runtime/sampling.stop_ref`` is
    the mirror and states the semantics) on the M tokens the argmax / sampler
    launch just wrote to ``tokens`` (int32).  A row of ``state`` (int32 (>= M,
    18), ``stop_state``) that has finished gets ``pad`` in ``tokens``, in
    ``also`` (the next input ids, when given) and in ``hist[row, p]`` (the token
    history, when given) with ``p = pos[row] + pos_off`` (``pos`` None:
    ``pos_off``; ``pos_off = -1`` when the step tail has advanced ``pos``
    already; ``p`` outside the history writes nothing).  A running row counts
    its token, pushes it into its window and finishes on a stop id or a stop
    sequence."""
    M = tokens.numel()
    ids, seqs = _stop_tables(stop_ids, stop_seqs, "stop_rows")
    if int(min_new) < 0 or int(pad) < 0:
        raise ValueError(f"stop_rows: min_new {min_new!r} and pad {pad!r} must be >= 0")
    for t, nm in ((tokens, "tokens"), (also, "also"), (pos, "pos")):
        if t is not None and (t.dtype != torch.int32 or t.numel() < M or not t.is_contiguous()):
            raise ValueError(f"stop_rows: {nm} must be contiguous int32 with >= {M} entries")
    if (state.dtype != torch.int32 or state.dim() != 2 or state.shape[1] != STOP_STATE_WORDS or state.shape[0] < M
            or not state.is_contiguous()):
        raise ValueError(f"stop_rows: state must be contiguous int32 (>= {M}, {STOP_STATE_WORDS}), got {state.dtype} "
                         f"{tuple(state.shape)}")
    hist_ld = 0
    if hist is not None:
        if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[0] < M or hist.stride(1) != 1:
            raise ValueError(f"stop_rows: hist must be int32 (>= {M}, L) with contiguous rows")
        hist_ld = hist.stride(0) if hist.shape[0] > 1 else hist.shape[1]
        if hist_ld < hist.shape[1]:
            raise ValueError("stop_rows: overlapping hist rows")
    check(lib().stop_rows(tok=ptr(tokens), also=ptr(also), hist=ptr(hist), hist_ld=hist_ld, pos=ptr(pos),
                          pos_off=int(pos_off), state=ptr(state), stop_ids=ids, stop_seqs=seqs, min_new=int(min_new),
                          pad=int(pad), M=M, st=stream_ptr()), "stop_rows")


def stop_suppress(logits: torch.Tensor, n_vocab: int, state: torch.Tensor, stop_ids, min_new: int) -> torch.Tensor:
    """bf16 -inf in place at every stop id of each row of ``logits`` (M, >=
    n_vocab) whose ``state`` row is running with fewer than ``min_new`` tokens
    generated (stop.hip; mirror ``runtime/sampling.stop_suppress_ref``)."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("stop_suppress: bf16 (M, >= n_vocab) logits with contiguous rows expected")
    M = logits.shape[0]
    if not 0 < n_vocab <= logits.shape[1]:
        raise ValueError(f"stop_suppress: n_vocab = {n_vocab} outside the row width {logits.shape[1]}")
    ids, _ = _stop_tables(stop_ids, (), "stop_suppress")
    if any(i >= n_vocab for i in ids):
        raise ValueError(f"stop_suppress: stop id outside [0, {n_vocab})")
    if int(min_new) < 0:
        raise ValueError(f"stop_suppress: min_new {min_new!r} must be >= 0")
    ld = logits.stride(0) if M > 1 else logits.shape[1]
    if ld % 8 or ld < n_vocab or logits.data_ptr() % 16:
        raise ValueError("stop_suppress: rows must start 16-byte aligned (row stride a multiple of 8, >= n_vocab)")
    if (state.dtype != torch.int32 or state.dim() != 2 or state.shape[1] != STOP_STATE_WORDS or state.shape[0] < M
            or not state.is_contiguous()):
        raise ValueError(f"stop_suppress: state must be contiguous int32 (>= {M}, {STOP_STATE_WORDS})")
    check(lib().stop_suppress(x=ptr(logits), ld=ld, M=M, N=int(n_vocab), state=ptr(state), stop_ids=ids,
                              min_new=int(min_new), st=stream_ptr()), "stop_suppress")
    return logits


def ragged_last_rows(h: torch.Tensor, lens: torch.Tensor, t0: int, Tc: int, B: int, dst: torch.Tensor,
                     d: Optional[int] = None) -> torch.Tensor:
    """Ragged prompts (ragged.hip; mirror ``runtime/sampling.ragged_last_rows_ref``):
    ``h`` bf16 (>= B * Tc, >= d) holds one prefill piece's hidden states, prompt
    positions ``[t0, t0 + Tc)`` of B sequences (row ``b * Tc + t``); ``lens``
    int32 (>= B) the prompt lengths.  Row ``b`` of ``dst`` bf16 (>= B, >= d)
    takes ``h[b * Tc + q, :d]`` when ``q = lens[b] - 1 - t0`` lies in
    ``[0, Tc)``; every other row keeps what it holds.  ``d`` defaults to the
    width of ``dst``."""
    for t, nm in ((h, "h"), (dst, "dst")):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError(f"ragged_last_rows: {nm} must be bf16 (rows, width) with contiguous rows, got {t.dtype} "
                            f"{tuple(t.shape)}")
    B, Tc, t0 = int(B), int(Tc), int(t0)
    d = dst.shape[1] if d is None else int(d)
    if B < 1 or Tc < 1 or t0 < 0:
        raise ValueError(f"ragged_last_rows: B = {B}, Tc = {Tc} must be >= 1 and t0 = {t0} >= 0")
    if d < 8 or d % 8 or d > h.shape[1] or d > dst.shape[1]:
        raise ValueError(f"ragged_last_rows: d = {d} must be a multiple of 8 within the widths {h.shape[1]} and "
                         f"{dst.shape[1]}")
    if h.shape[0] < B * Tc or dst.shape[0] < B:
        raise ValueError(f"ragged_last_rows: h holds {h.shape[0]} rows (B * Tc = {B * Tc} needed), dst {dst.shape[0]} "
                         f"(B = {B} needed)")
    if lens.dtype != torch.int32 or lens.numel() < B or not lens.is_contiguous():
        raise ValueError(f"ragged_last_rows: lens must be contiguous int32 with >= {B} entries")
    if h.device != dst.device or lens.device != h.device:
        raise ValueError("ragged_last_rows: h, lens and dst must be on one device")
    ld = h.stride(0) if h.shape[0] > 1 else h.shape[1]
    dst_ld = dst.stride(0) if dst.shape[0] > 1 else dst.shape[1]
    if ld % 8 or dst_ld % 8 or ld < d or dst_ld < d or h.data_ptr() % 16 or dst.data_ptr() % 16:
        raise ValueError("ragged_last_rows: rows must start 16-byte aligned (row strides multiples of 8, >= d)")
    check(lib().ragged_last_rows(h=ptr(h), ld=ld, lens=ptr(lens), t0=t0, Tc=Tc, B=B, d=d, dst=ptr(dst),
                                 dst_ld=dst_ld, st=stream_ptr()), "ragged_last_rows")
    return dst


class ConstraintTables:
    """The device tables of ``dnn_logit_constraints`` (constraints.hip) for one
    ``config.ConstraintConfig`` and vocabulary, built once (``constraint_tables``):
    bias ids (int32) and values (fp32), the allowed-id bitmask over ``[0, n_vocab)``
    (uint8, bit ``i % 8`` of byte ``i // 8``; None = everything allowed), the bad
    words as int32 (n, 16) with their lengths, and ``no_repeat_ngram_size``.  The
    host copies travel with every launch, where the entry point checks them."""

    __slots__ = ("n_vocab", "device", "bias_ids", "bias_vals", "allow", "bad_ids", "bad_len", "ngram", "h_bias_ids",
                 "h_bias_vals", "h_bad", "needs_context")


def constraint_tables(cons, n_vocab: int, device) -> ConstraintTables:
    """Validate ``cons`` (``config.ConstraintConfig``) against ``n_vocab`` and the
    caps, and put its tables on ``device``."""
    n_vocab = int(n_vocab)
    ids = [int(k) for k, _ in cons.logit_bias]
    vals = [float(v) for _, v in cons.logit_bias]
    words = [[int(e) for e in s] for s in cons.bad_words_ids]
    allowed = None if cons.allowed_token_ids is None else [int(i) for i in cons.allowed_token_ids]
    ngram = int(cons.no_repeat_ngram_size)
    if len(ids) > CON_MAX_BIAS or len(words) > CON_MAX_BAD_WORDS:
        raise ValueError(f"constraint_tables: at most {CON_MAX_BIAS} bias ids and {CON_MAX_BAD_WORDS} bad words, got "
                         f"{len(ids)} and {len(words)}")
    if any(not 1 <= len(s) <= CON_MAX_BAD_LEN for s in words):
        raise ValueError(f"constraint_tables: a bad word holds 1..{CON_MAX_BAD_LEN} ids")
    if not 0 <= ngram <= CON_MAX_NGRAM:
        raise ValueError(f"constraint_tables: no_repeat_ngram_size {ngram} outside [0, {CON_MAX_NGRAM}]")
    bad = [i for i in ids + [e for s in words for e in s] + (allowed or []) if not 0 <= i < n_vocab]
    if bad:
        raise ValueError(f"constraint_tables: ids outside [0, {n_vocab}): {bad!r}")
    if len(set(ids)) != len(ids):
        raise ValueError("constraint_tables: the bias ids must be distinct")
    if any(not math.isfinite(v) for v in vals):
        raise ValueError("constraint_tables: a bias must be finite")
    if allowed is not None and not allowed:
        raise ValueError("constraint_tables: allowed_token_ids must not be empty")
    t = ConstraintTables()
    t.n_vocab, t.device, t.ngram = n_vocab, torch.device(device), ngram
    t.h_bias_ids, t.h_bias_vals, t.h_bad = ids, vals, words
    t.needs_context = ngram > 0 or any(len(s) > 1 for s in words)
    t.bias_ids = torch.tensor(ids, dtype=torch.int32, device=device) if ids else None
    t.bias_vals = torch.tensor(vals, dtype=torch.float32, device=device) if ids else None
    t.allow = None
    if allowed is not None:
        bits = torch.zeros((-(-n_vocab // 8) * 8,), dtype=torch.uint8)
        bits[torch.tensor(allowed, dtype=torch.int64)] = 1
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32)
        t.allow = (bits.view(-1, 8).to(torch.int32) * weights).sum(1).to(torch.uint8).to(device)
    t.bad_ids = t.bad_len = None
    if words:
        flat = torch.full((len(words), CON_MAX_BAD_LEN), -1, dtype=torch.int32)
        for s, w in enumerate(words):
            flat[s, :len(w)] = torch.tensor(w, dtype=torch.int32)
        t.bad_ids = flat.to(device)
        t.bad_len = torch.tensor([len(w) for w in words], dtype=torch.int32, device=device)
    return t


def logit_constraints(logits: torch.Tensor, n_vocab: int, tables: ConstraintTables,
                      ctx: Optional[torch.Tensor] = None, pos: Optional[torch.Tensor] = None, pos_off: int = 0,
                      prev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logit_bias, allowed_token_ids, bad_words_ids and no_repeat_ngram_size in
    place on the first ``n_vocab`` entries of every row of bf16 ``logits``, one
    launch (constraints.hip; ``runtime/sampling.constraints_ref`` is the bitwise
    mirror and states the rules).  ``ctx`` (int32 (>= M, L), contiguous rows):
    each row's prompt + generated tokens, of which ``pos[row] + pos_off``
    (``pos`` None: ``pos_off``) are valid; needed when ``tables.needs_context``.
    ``prev`` (int32 per row, or None): the token each row generated last, stored
    as the newest context entry first (-1 / out-of-range: nothing stored)."""
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise TypeError("logit_constraints: bf16 (M, >= n_vocab) logits with contiguous rows expected")
    M = logits.shape[0]
    if not 0 < n_vocab <= logits.shape[1] or int(n_vocab) != tables.n_vocab:
        raise ValueError(f"logit_constraints: n_vocab = {n_vocab} outside the row width {logits.shape[1]} or not the "
                         f"tables' {tables.n_vocab}")
    ld = logits.stride(0) if M > 1 else logits.shape[1]
    if ld % 8 or ld < n_vocab or logits.data_ptr() % 16:
        raise ValueError("logit_constraints: rows must start 16-byte aligned (row stride a multiple of 8, >= n_vocab)")
    ctx_ld = 0
    if ctx is not None:
        if ctx.dtype != torch.int32 or ctx.dim() != 2 or ctx.shape[0] < M or ctx.stride(1) != 1:
            raise ValueError(f"logit_constraints: ctx must be int32 (>= {M}, L) with contiguous rows")
        ctx_ld = ctx.stride(0) if ctx.shape[0] > 1 else ctx.shape[1]
        if ctx_ld < ctx.shape[1]:
            raise ValueError("logit_constraints: overlapping ctx rows")
    elif tables.needs_context:
        raise ValueError("logit_constraints: these constraints need the context table ctx")
    for t, nm in ((pos, "pos"), (prev, "prev")):
        if t is not None and (t.dtype != torch.int32 or t.numel() < M or not t.is_contiguous()):
            raise ValueError(f"logit_constraints: {nm} must be contiguous int32 with >= {M} entries")
    check(lib().logit_constraints(x=ptr(logits), ld=ld, M=M, N=int(n_vocab), ctx=ptr(ctx), ctx_ld=ctx_ld, pos=ptr(pos),
                                  pos_off=int(pos_off), prev=ptr(prev if ctx is not None else None),
                                  bias_ids=ptr(tables.bias_ids), bias_vals=ptr(tables.bias_vals), allow=ptr(tables.allow),
                                  bad_ids=ptr(tables.bad_ids), bad_len=ptr(tables.bad_len), ngram=tables.ngram,
                                  h_bias_ids=tables.h_bias_ids, h_bias_vals=tables.h_bias_vals, h_bad=tables.h_bad,
                                  st=stream_ptr()), "logit_constraints")
    return logits
