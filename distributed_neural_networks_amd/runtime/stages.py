"""Stage compute objects: one pipeline stage's forward over preallocated buffers.

``StageCompute`` is what a pipeline rank runs per microbatch.  Two families:

* ``CifarHipStage`` — the MI355X path: fused gfx950 kernels over weights
  packed once at load (``ops/cifar.py``; fp32 by default, the reference's
  precision, or bf16); no torch op runs in ``forward``.
* ``TorchStage`` — the golden torch module on CPU (fp32): the data path of the
  reference's CPU/gRPC configuration (``BASELINE.json`` configs[0]) and the
  oracle in tests.  It is never used on a GPU device.

The GPT-2 / Llama stages live in ``runtime/transformer.py`` (same interface).
Reference: the stage forward is ``my_model_part(input_torch)`` in
``node.py:52-53``; the result argmax is ``node.py:61`` (there over the flattened
batch; here per row).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from ..models import cifar, model_info

Spec = Tuple[Tuple[int, ...], torch.dtype]


@dataclass
class StageOutput:
    """Last-stage result: probabilities/logits and per-row predictions."""
    probs: torch.Tensor
    pred: torch.Tensor


class StageCompute:
    first: bool
    last: bool
    device: torch.device

    def in_spec(self, batch: int) -> Spec:
        raise NotImplementedError

    def out_spec(self, batch: int) -> Spec:
        raise NotImplementedError

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None):
        raise NotImplementedError


class CifarHipStage(StageCompute):
    """CIFAR units [start, end] on the fused HIP kernels.

    Units 0-1 always run together (the fused conv1/pool/conv2/pool kernel), so
    the supported ranges are (0,1) = reference part 0, (2,3) = reference part 1,
    (0,3) = whole model, (2,2) = fc1 alone (3-stage pipelines), and the fc1 cut (0,2) | (3,3) whose stage boundary is
    the 512-wide hidden (2 KiB/img in fp32 instead of 16 KiB: what the
    multi-GPU placement uses when the xGMI hop, not compute, would bound the
    pipeline, parallel/partition.py ``cifar_cut``).

    ``precision`` "fp32" (default, the reference's: fp32 in, fp32 boundary,
    3-term bf16 split products accumulated in fp32) or "bf16".

    ``boundary`` (fp32, the conv|fc cut): "fp32" values on the 16 KiB/img
    boundary (default; what a reference peer expects over gRPC), or "split" —
    the blocked hi/lo encoding of the same 16 KiB (``ops/cifar.py``;
    bit-identical results, measured neutral end to end).  Both stages of a hop
    must agree.

    ``input_dtype`` "uint8" (first stage, fp32 precision): the stage takes the
    images as they exist, ``(B,32,32,3)`` bytes, and the stage-0 kernel
    normalises them by ``input_table`` (a ``(3,256)`` fp32 table, default
    ``make_input_table()``: the reference's Normalize(0.5, 0.5)); the result is
    bitwise that of the fp32 input ``normalize_u8(x, input_table)``."""

    SUPPORTED = {(0, 1), (2, 3), (0, 3), (0, 2), (2, 2), (3, 3)}

    def __init__(self, sd: Dict[str, torch.Tensor], start: int, end: int, device: torch.device,
                 precision: str = "fp32", boundary: str = "fp32", input_dtype: str = "fp32", input_table=None):
        from ..ops import cifar as cops
        if (start, end) not in self.SUPPORTED:
            raise ValueError(f"HIP CIFAR backend supports unit ranges {sorted(self.SUPPORTED)}, got ({start},{end})")
        self.start, self.end, self.device = start, end, torch.device(device)
        self.first, self.last = start == 0, end == cifar.NUM_UNITS - 1
        self.precision = precision
        if boundary not in cops.BOUNDARIES:
            raise ValueError(f"boundary must be one of {cops.BOUNDARIES}")
        # the encoding only exists on the 4096-wide conv|fc boundary of the fp32 path
        self.boundary = boundary if precision == "fp32" else "fp32"
        self._cops = cops
        self.adt = cops.act_dtype(precision)
        self.w0 = cops.pack_stage0(sd, self.device, precision) if start == 0 else None
        self.wh = cops.pack_head(sd, self.device, fc1=start <= 2 <= end, fc2=end == 3, precision=precision)
        self._scratch: Dict[int, Dict[str, torch.Tensor]] = {}
        if input_dtype not in cops.INPUT_DTYPES:
            raise ValueError(f"input_dtype must be one of {cops.INPUT_DTYPES}, got {input_dtype!r}")
        # only a first stage sees images; the others ignore the pipeline-wide setting
        self.input_dtype = input_dtype if self.first else "fp32"
        self.input_table = None
        if self.input_dtype == "uint8":
            if precision != "fp32":
                raise ValueError("uint8 input exists for the fp32 precision only (the bf16 kernel has no table path)")
            self.input_table = cops.pack_input_table(cops.make_input_table() if input_table is None else input_table,
                                                     self.device)

    def _boundary(self, unit: int):
        return ((cifar.FLAT_DIM if unit == 1 else 512), self.adt)

    def in_spec(self, batch):
        if self.first:
            if self.input_dtype == "uint8":
                return (batch, 32, 32, 3), torch.uint8
            return (batch, 3, 32, 32), torch.float32
        w, dt = self._boundary(self.start - 1)
        return (batch, w), dt

    def out_spec(self, batch):
        if self.last:
            return (batch, 10), torch.float32
        w, dt = self._boundary(self.end)
        return (batch, w), dt

    def _buf(self, batch):
        b = self._scratch.get(batch)
        if b is None:
            d = self.device
            b = {}
            if self.first and self.end >= 2:
                b["mid"] = torch.empty((batch, 4096), dtype=self.adt, device=d)
            if self.start <= 2 <= self.end and self.precision == "fp32" and batch < self._cops.FC1_X3_MIN_ROWS:
                b["split"] = torch.empty((batch, 3 * 4096), dtype=torch.bfloat16, device=d)
            if self.last:
                b["hid"] = torch.empty((batch, 512), dtype=self.adt, device=d)
                b["pred"] = torch.empty((batch,), dtype=torch.int32, device=d)
            self._scratch[batch] = b
        return b

    def forward(self, x, out=None):
        B = x.shape[0]
        buf = self._buf(B)
        h = x
        if self.first:
            if self.input_dtype == "uint8":
                if h.dtype != torch.uint8:
                    raise ValueError(f"stage 0 was built for uint8 (B,32,32,3) input, got {h.dtype} {tuple(h.shape)}")
            elif h.dtype != torch.float32:
                h = h.float()
            h = self._cops.stage0_forward(h.contiguous(), self.w0, buf["mid"] if self.end >= 2 else out,
                                          boundary=self.boundary, table=self.input_table)
            if self.end == 1:
                return h
        elif h.dtype != self.adt:
            h = h.to(self.adt)
        if self.start <= 2 <= self.end:
            h = self._cops.fc1_forward(h.contiguous(), self.wh, out if self.end == 2 else buf["hid"],
                                       scratch=buf.get("split"), boundary=self.boundary)
            if self.end == 2:
                return h
        probs, pred = self._cops.head_tail(h.contiguous(), self.wh, out, buf["pred"])
        return StageOutput(probs, pred)


class TorchStage(StageCompute):
    """Golden torch module as a stage (CPU fp32 plumbing path / tests)."""

    def __init__(self, model: str, sd: Dict[str, torch.Tensor], start: int, end: int, first: bool, last: bool,
                 device="cpu", dtype=torch.float32, sampling=(0.0, 0, 0), input_dtype: str = "fp32", input_table=None):
        from ..models import build_golden_stage
        # sampling = (temperature, top_k, seed[, top_p, min_p[, repetition, presence, frequency penalty[, logprobs
        #             [, stop (config.StopConfig or None)[, constraints (config.ConstraintConfig or None)]]]]])
        if len(sampling) not in (3, 5, 8, 9, 10, 11):
            raise ValueError(f"sampling: 3, 5, 8, 9, 10 or 11 entries expected, got {len(sampling)}")
        self.temperature, self.top_k, self.seed = float(sampling[0]), int(sampling[1]), int(sampling[2])
        self.top_p, self.min_p = (float(sampling[3]), float(sampling[4])) if len(sampling) >= 5 else (1.0, 0.0)
        self.rep_pen, self.pres_pen, self.freq_pen = ((float(sampling[5]), float(sampling[6]), float(sampling[7]))
                                                      if len(sampling) >= 8 else (1.0, 0.0, 0.0))
        # log-probabilities (last stage): every last_only step records its token's and the top-n through
        # the mirror (runtime/sampling.py logprobs_ref) into the histories bound to its cache rows
        nlp = sampling[8] if len(sampling) >= 9 else 0
        from ..config import LOGPROBS_MAX_N
        if not isinstance(nlp, int) or isinstance(nlp, bool) or not 0 <= nlp <= LOGPROBS_MAX_N:
            raise ValueError(f"logprobs must be an integer in [0, {LOGPROBS_MAX_N}], got {nlp!r}")
        self.logprobs = nlp if last else 0
        self._lp_hist: Dict[int, tuple] = {}
        # stop conditions (last stage): the mirror's state (runtime/sampling.py stop_ref) per microbatch offset
        self.stop = sampling[9] if len(sampling) >= 10 and last else None
        self._stop_st: Dict[int, torch.Tensor] = {}
        # logit constraints (last stage): through the mirror (runtime/sampling.py constraints_ref); per microbatch
        # offset the rows' contexts (prompt, then generated tokens, as lists) and the token generated last
        self.constraints = sampling[10] if len(sampling) == 11 and last else None
        self._con_ctx: Dict[int, list] = {}
        self._con_prev: Dict[int, Optional[torch.Tensor]] = {}
        import math
        if not (self.rep_pen > 0 and math.isfinite(self.rep_pen)):
            raise ValueError(f"repetition penalty must be a finite number > 0, got {sampling[5]!r}")
        if not (math.isfinite(self.pres_pen) and math.isfinite(self.freq_pen)):
            raise ValueError(f"presence / frequency penalties must be finite, got {sampling[6]!r}, {sampling[7]!r}")
        self.penalties_on = bool(last) and (self.rep_pen != 1.0 or self.pres_pen != 0.0 or self.freq_pen != 0.0)
        # penalty state per microbatch offset b0 (runtime/sampling.py mirror of the device state) and the
        # token the rows generated last, counted by the next decode step
        self._pen: Dict[int, torch.Tensor] = {}
        self._pen_prev: Dict[int, Optional[torch.Tensor]] = {}
        self.model, self.start, self.end, self.first, self.last = model, start, end, first, last
        self.device = torch.device(device)
        self.family = model_info(model).family
        self.module = build_golden_stage(model, start, end, first, last)
        missing, unexpected = self.module.load_state_dict(sd, strict=False)
        if missing:
            raise KeyError(f"stage [{start},{end}] missing weights: {missing[:8]}")
        self.module = self.module.to(device=self.device, dtype=dtype).eval()
        # CPU CIFAR convolutions in NHWC (oneDNN's preferred layout): stage 0
        # at B = 255 on 4 threads 56 -> 29 ms; the flatten to the (B, 4096)
        # boundary still follows the reference's NCHW order (a logical reshape).
        # GPU golden stages keep NCHW (the fp32 oracle of the HIP kernels).
        self.nhwc = self.family == "cifar" and self.device.type == "cpu"
        if self.nhwc:
            self.module = self.module.to(memory_format=torch.channels_last)
        self.dtype = dtype
        # CIFAR first stage on uint8 (B,32,32,3) images: normalised by table before the module
        if input_dtype not in ("fp32", "uint8"):
            raise ValueError(f"input_dtype must be 'fp32' or 'uint8', got {input_dtype!r}")
        self.input_dtype = input_dtype if (self.family == "cifar" and first) else "fp32"
        if input_dtype == "uint8" and self.family != "cifar":
            raise ValueError("uint8 input exists for the CIFAR family only")
        self.input_table = None
        if self.input_dtype == "uint8":
            from ..ops.cifar import make_input_table
            self.input_table = (make_input_table() if input_table is None else input_table).to(self.device)

    def in_spec(self, batch, seq: int = 0):
        if self.family == "cifar":
            if self.input_dtype == "uint8":
                return (batch, 32, 32, 3), torch.uint8
            return cifar.input_shape(self.start, batch), self.dtype
        info = model_info(self.model)
        if self.first:
            return (batch, seq), torch.int64
        return (batch, seq, info.cfg.n_embd), self.dtype

    def out_spec(self, batch, seq: int = 0):
        if self.family == "cifar":
            return cifar.output_shape(self.end, batch), self.dtype
        info = model_info(self.model)
        if self.last:
            return (batch, seq, info.cfg.vocab_size), self.dtype
        return (batch, seq, info.cfg.n_embd), self.dtype

    @property
    def d(self) -> int:
        return model_info(self.model).cfg.n_embd

    @property
    def act_dtype(self) -> torch.dtype:
        return self.dtype

    def penalty_begin(self, b0: int, ids: torch.Tensor, lens=None) -> None:
        """Start a generation on cache rows [b0, b0 + B): the (B, T) prompt's
        tokens are marked, nothing is counted yet (``TransformerStage.penalty_begin``).
        ``lens`` (ragged prompts): only ``ids[b, :lens[b]]`` are marked."""
        from .sampling import penalty_state
        if not self.penalties_on:
            raise ValueError("penalty_begin: this stage has no penalties")
        V = model_info(self.model).cfg.vocab_size
        if lens is None:
            self._pen[b0] = penalty_state(ids, V)
        else:
            ls = [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
            self._pen[b0] = torch.cat([penalty_state(ids[b:b + 1, :ls[b]], V) for b in range(ids.shape[0])], 0)
        self._pen_prev[b0] = None

    def penalty_forget(self, b0: int, B: int) -> None:
        """The sample of a prefill piece before the last one is no generated token."""
        self._pen_prev[b0] = None

    @property
    def constraints_need_context(self) -> bool:
        return self.constraints is not None and self.constraints.needs_context

    def constraint_begin(self, b0: int, ids: torch.Tensor, lens=None) -> None:
        """Start a generation on cache rows [b0, b0 + B): each row's context is
        its own prompt (``TransformerStage.constraint_begin``)."""
        if not self.constraints_need_context:
            raise ValueError("constraint_begin: this stage keeps no context")
        B, T = ids.shape
        ls = [T] * B if lens is None else [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
        self._con_ctx[b0] = [[int(v) for v in ids[b, :ls[b]].tolist()] for b in range(B)]
        self._con_prev[b0] = None

    def constraint_forget(self, b0: int, B: int) -> None:
        """The sample of a prefill piece before the last one is no generated token."""
        self._con_prev[b0] = None

    def constraint_snapshot(self, b0: int, B: int):
        return b0, B, [list(c) for c in self._con_ctx[b0]], self._con_prev[b0]

    def constraint_restore(self, snap) -> None:
        self._con_ctx[snap[0]] = [list(c) for c in snap[2]]
        self._con_prev[snap[0]] = snap[3]

    def stop_begin(self, b0: int, B: int) -> None:
        """Start a generation on cache rows [b0, b0 + B) (``TransformerStage.stop_begin``)."""
        from .sampling import stop_state
        if self.stop is None:
            raise ValueError("stop_begin: this stage has no stop conditions")
        self._stop_st[b0] = stop_state(B)

    def stop_forget(self, b0: int, B: int) -> None:
        """The sample of a prefill piece before the last one is neither counted nor matched."""
        self.stop_begin(b0, B)

    def stop_snapshot(self, b0: int, B: int):
        return b0, B, self._stop_st[b0].clone()

    def stop_restore(self, snap) -> None:
        self._stop_st[snap[0]] = snap[2].clone()

    @property
    def stop_state(self) -> Optional[torch.Tensor]:
        """The stop state of every begun row, in cache-row order (None: no stop conditions)."""
        if self.stop is None:
            return None
        from .sampling import stop_state
        n = max((b0 + st.shape[0] for b0, st in self._stop_st.items()), default=0)
        out = stop_state(n)
        for b0, st in self._stop_st.items():
            out[b0:b0 + st.shape[0]] = st
        return out

    def bind_logprobs(self, b0: int, chosen: torch.Tensor, top_ids: torch.Tensor, top_lps: torch.Tensor) -> None:
        """The histories of cache rows [b0, b0 + B) (``TransformerStage.bind_logprobs``):
        fp32 (B, L), int32 (B, L, n), fp32 (B, L, n); a ``last_only`` step writes
        position ``pos + T - 1``, the position its token was sampled at."""
        if not self.logprobs:
            raise ValueError("bind_logprobs: this stage records no log-probabilities")
        self._lp_hist[b0] = (chosen, top_ids, top_lps)

    def _hidden(self, h, kv, p: int):
        """The module's blocks (and embedding) without its head: (B, T, d)."""
        return self.module(h, kv, p, head=False)

    def _head(self, x):
        return self.module.head(x)

    @torch.no_grad()
    def step(self, x, pos, B: int, T: int, b0: int = 0, out=None, last_only: bool = True, lens=None, t0: int = 0):
        """KV-cached transformer step (CPU golden path; same contract as
        ``TransformerStage.step``): x = ids (B,T) on the first stage, else
        hidden (B*T, d); ``pos`` = tokens already cached; rows ``[b0, b0+B)``
        of the cache (one KV cache per microbatch offset).  Positions that
        differ between the rows (decode after ragged prompts) run the rows one
        at a time on row views of the cache.  ``lens`` (int (B,)): a piece of a
        ragged prefill covering prompt positions ``[t0, t0 + T)``; the last
        stage then samples nothing and keeps each row's hidden state of its
        own last prompt position for ``ragged_first_token``."""
        cfg = model_info(self.model).cfg
        if isinstance(pos, torch.Tensor):
            ps = [int(v) for v in pos.reshape(-1)[:B].tolist()]
        else:
            ps = [int(pos)] * B
        p = ps[0]
        uniform = all(v == p for v in ps)
        caches = getattr(self, "_kv", None)
        if caches is None:
            caches = self._kv = {}
        kv = caches.get(b0)
        if kv is None or kv[0][0].shape[0] != B:
            S = getattr(cfg, "block_size", getattr(cfg, "max_seq", 1024))
            hkv = getattr(cfg, "n_kv_head", cfg.n_head)
            hd = cfg.n_embd // cfg.n_head
            n = len(self.module.h if self.family == "gpt2" else self.module.layers)
            kv = caches[b0] = [(torch.zeros(B, hkv, S, hd, dtype=self.dtype), torch.zeros(B, hkv, S, hd, dtype=self.dtype))
                               for _ in range(n)]
        if self.first:
            h = x.to(torch.int64).view(B, T)
        else:
            h = x.view(B, T, cfg.n_embd).to(self.dtype)
        if lens is not None and self.last:
            from .sampling import ragged_last_rows_ref
            hid = self._hidden(h, kv, p).reshape(B * T, cfg.n_embd)
            keep = getattr(self, "_h_last", None)
            if keep is None:
                keep = self._h_last = {}
            if b0 not in keep or keep[b0].shape[0] != B:
                keep[b0] = torch.zeros((B, cfg.n_embd), dtype=self.dtype)
            keep[b0] = ragged_last_rows_ref(hid, torch.as_tensor(lens), t0, T, B, cfg.n_embd, keep[b0])
            return None
        if uniform and not self.last:
            y = self.module(h, kv, p)
        elif uniform:
            hid = self._hidden(h, kv, p)
            y = self._head(hid[:, -1:, :] if last_only else hid)
        else:
            hid = torch.cat([self._hidden(h[b:b + 1], [(k[b:b + 1], v[b:b + 1]) for k, v in kv], ps[b])
                             for b in range(B)], 0)
            y = hid if not self.last else self._head(hid[:, -1:, :] if last_only else hid)
        if self.last:
            step = pos if isinstance(pos, torch.Tensor) else torch.full((B,), p, dtype=torch.int32)
            return self._tail(y, b0, B, T, step, [v + T - 1 for v in ps], out, last_only)
        y = y.reshape(B * T, cfg.n_embd)
        if out is not None:
            out.view(B * T, cfg.n_embd).copy_(y)
            return out
        return y

    @torch.no_grad()
    def ragged_first_token(self, b0: int, B: int, lens, out=None) -> StageOutput:
        """Last stage, after the last piece of a ragged prefill of cache rows
        [b0, b0 + B): the tail of a ``last_only`` step on the hidden states the
        pieces kept (each row's own last prompt position), so every row's first
        token.  The sampler's step operand is 0 for every row, what an
        unchunked equal-length prefill passes; the log-probabilities go to
        history position ``lens - 1``."""
        if not self.last:
            raise ValueError("ragged_first_token: last stage only")
        keep = getattr(self, "_h_last", {}).get(b0)
        if keep is None or keep.shape[0] != B:
            raise ValueError(f"ragged_first_token: no ragged prefill piece ran on the {B} cache rows at {b0}")
        y = self._head(keep[:, None, :])
        ls = [int(v) for v in torch.as_tensor(lens).reshape(-1)[:B].tolist()]
        return self._tail(y, b0, B, 0, torch.zeros((B,), dtype=torch.int32), [v - 1 for v in ls], out, True)

    def _tail(self, y, b0: int, B: int, T: int, step, lp_q, out, last_only: bool):
        """What the last stage does with its head's output ``y`` (B, 1 or T, V):
        penalties, constraints (row b's context holds ``lp_q[b] + 1`` tokens),
        suppression, pick, log-probabilities (row b at history position
        ``lp_q[b]``), stop conditions.  ``T == 1`` marks a decode step
        (it counts the rows' previous token)."""
        from .sampling import pick
        logits = y[:, -1, :] if last_only else y.reshape(y.shape[0] * y.shape[1], -1)
        if self.penalties_on and last_only:
            # as the device stage: a decode step counts the rows' previous token, then every sampled
            # position's logits (rounded to bf16) take the penalties
            from .sampling import apply_penalties_ref, penalty_count
            if b0 not in self._pen:
                raise ValueError(f"penalties: no penalty_begin for cache rows at {b0}")
            if T == 1 and self._pen_prev[b0] is not None:
                self._pen[b0] = penalty_count(self._pen[b0], self._pen_prev[b0])
            logits = apply_penalties_ref(logits, self._pen[b0], self.rep_pen, self.freq_pen, self.pres_pen)
            y = logits[:, None, :]
        con = self.constraints is not None and last_only
        if con:
            from .sampling import constraints_ref
            ctx = lens = None
            if self.constraints.needs_context:
                if b0 not in self._con_ctx or len(self._con_ctx[b0]) != B:
                    raise ValueError(f"constraints: no constraint_begin for the {B} cache rows at {b0}")
                rows = self._con_ctx[b0]
                if T == 1 and self._con_prev[b0] is not None:  # a decode step appends the rows' previous token
                    for b, t in enumerate(self._con_prev[b0].tolist()):
                        rows[b].append(int(t))
                lens = [q + 1 for q in lp_q]
                width = max(max(lens), max(len(r) for r in rows), 1)
                ctx = torch.tensor([r + [-1] * (width - len(r)) for r in rows], dtype=torch.int32)
            logits = constraints_ref(logits, self.constraints, ctx, lens)
            y = logits[:, None, :]
        stp = self.stop is not None and last_only
        if stp:
            from .sampling import stop_ref, stop_suppress_ref
            if b0 not in self._stop_st or self._stop_st[b0].shape[0] != B:
                raise ValueError(f"stop: no stop_begin for the {B} cache rows at {b0}")
            if self.stop.min_new_tokens > 0 and self.stop.stop_token_ids:
                logits = stop_suppress_ref(logits, self._stop_st[b0], self.stop.stop_token_ids,
                                           self.stop.min_new_tokens)
                y = logits[:, None, :]
        pred = pick(y[:, -1, :], self.temperature, self.top_k, self.seed, step, top_p=self.top_p,
                    min_p=self.min_p).to(torch.int32)
        if self.penalties_on and last_only:
            self._pen_prev[b0] = pred.clone()
        if con and self.constraints.needs_context:
            self._con_prev[b0] = pred.clone()
        if self.logprobs and last_only:
            from .sampling import logprobs_ref
            if b0 not in self._lp_hist:
                raise ValueError(f"logprobs: no bind_logprobs for cache rows at {b0}")
            chosen, top_ids, top_lps = self._lp_hist[b0]
            c, ti, tl = logprobs_ref(logits, pred, self.logprobs)
            for b, q in enumerate(lp_q):
                if 0 <= q < chosen.shape[1]:
                    chosen[b, q] = c[b]
                    top_ids[b, q, :self.logprobs] = ti[b]
                    top_lps[b, q, :self.logprobs] = tl[b]
        if stp:  # last in the step: finished rows give the pad token, running rows count and match theirs
            self._stop_st[b0], pred = stop_ref(self._stop_st[b0], pred, self.stop.stop_token_ids,
                                               self.stop.stop_sequences, self.stop.min_new_tokens,
                                               self.stop.pad_token_id)
        if out is not None and last_only:
            out.copy_(pred)
            pred = out
        return StageOutput(logits, pred)

    @torch.no_grad()
    def forward(self, x, out=None):
        x = x.to(self.device)
        with torch.no_grad():  # no autograd graph: a third of the CPU conv stage's time
            if self.input_dtype == "uint8":
                from ..ops.cifar import normalize_u8
                x = normalize_u8(x, self.input_table).to(self.dtype)
            if self.nhwc and x.dim() == 4:
                x = x.contiguous(memory_format=torch.channels_last)
            y = self.module(x)
            if y.dim() == 4:
                y = y.contiguous()  # a 4-D boundary crosses the wire in NCHW order
        if self.last:
            if self.family == "cifar":
                return StageOutput(y, y.argmax(dim=1).to(torch.int32))
            return StageOutput(y, y[:, -1, :].argmax(dim=-1).to(torch.int32))
        if out is not None:
            out.copy_(y)
            return out
        return y
