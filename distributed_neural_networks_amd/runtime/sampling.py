"""Token sampling: greedy, or temperature + top-k by the Gumbel-max trick.

The device kernel is ``sample_topk`` (csrc/kernels/sampler.hip); this module is
its bit-compatible torch mirror for the CPU/gloo golden path and the tests:

    token = argmax_{i : key(x_i) >= key(k-th largest)} ( x_i / T + G_i ),
    G_i = -log(-log(U_i)),  U_i = hash(seed, row, step[row], i)

``sample_rows`` (csrc/kernels/sample_filter.hip) adds the nucleus (top-p) and
min-p filters, each one more threshold on the same 16-bit key
(``filter_thresholds``); ``sample_ref`` mirrors it.

The counter-based hash needs no RNG state (one captured HIP graph serves every
decode step; runs are reproducible from ``seed``).  The reference has no
sampler at all: ``np.argmax`` on the host (``node.py:61,190``).
"""
from __future__ import annotations

from typing import Optional

import torch

from ..config import LOGPROBS_MAX_N, STOP_MAX_IDS, STOP_MAX_SEQ_LEN

_M32 = 0xFFFFFFFF


def _mix32(x: torch.Tensor) -> torch.Tensor:
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & _M32
    return x ^ (x >> 16)


def _keys(x_bf16: torch.Tensor) -> torch.Tensor:
    u = x_bf16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    return torch.where((u & 0x8000) != 0, (~u) & 0xFFFF, u | 0x8000)


def sample_topk_ref(logits: torch.Tensor, temperature: float, top_k: int = 0, seed: int = 0,
                    step: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Torch mirror of the device sampler; ``logits`` (M, N) (rounded to bf16)."""
    x = logits.to(torch.bfloat16).cpu()
    M, N = x.shape
    keys = _keys(x)
    if 0 < top_k < N:
        thr = keys.sort(dim=1, descending=True).values[:, top_k - 1:top_k]
    else:
        thr = torch.zeros((M, 1), dtype=torch.int64)
    return _draw(x, keys, thr, temperature, seed, step)


def _draw(x: torch.Tensor, keys: torch.Tensor, thr: torch.Tensor, temperature: float, seed: int,
          step: Optional[torch.Tensor]) -> torch.Tensor:
    """Gumbel-max over ``keys >= thr`` (x bf16 (M, N) on the CPU, thr (M, 1))."""
    M, N = x.shape
    st = (step.cpu().to(torch.int64) if step is not None else torch.zeros(M, dtype=torch.int64)) & _M32
    rows = torch.arange(M, dtype=torch.int64)
    inner = _mix32(st + 0x632BE5AB)
    base = _mix32((seed & _M32) ^ _mix32(((rows * 0x9E3779B9) & _M32) ^ inner))
    idx = torch.arange(N, dtype=torch.int64)
    h = _mix32(base[:, None] ^ ((idx[None, :] * 0x85EBCA6B) & _M32))
    u = ((h >> 8).to(torch.float32) + 0.5) * (1.0 / 16777216.0)
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    score = x.float() * inv_t - torch.log(-torch.log(u))
    score = torch.where(keys >= thr, score, torch.full_like(score, float("-inf")))
    return score.argmax(dim=1).to(torch.int32)


def _key_values() -> torch.Tensor:
    """The fp32 value of every 16-bit key (the kernel's ``key_to_f``)."""
    k = torch.arange(65536, dtype=torch.int64)
    u = torch.where((k & 0x8000) != 0, k & 0x7FFF, (~k) & 0xFFFF)
    bits = u << 16
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)


def filter_thresholds(logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0,
                      min_p: float = 0.0) -> torch.Tensor:
    """Per-row key threshold (M, 1) of the device sampler's filter chain
    (``sample_rows``, csrc/kernels/sample_filter.hip): the kept set is
    ``key_i >= max(thr_k, thr_p, thr_m)`` with

    * ``thr_k`` the k-th largest key (0 when top_k is off);
    * ``thr_p`` the largest key t with ``sum_{key_i >= t} w_i >= top_p * Z``,
      ``w_i = exp((x_i - x_max) / T)`` over the top-k survivors, ``Z = sum w_i``
      (masses in float64; ``top_p >= 1`` switches it off);
    * ``thr_m`` the smallest key whose value passes ``(x - x_max) / T >=
      log(min_p)`` in fp32, never above the row maximum (``min_p <= 0``: off)."""
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    if not 0.0 <= min_p < 1.0:
        raise ValueError(f"min_p must be in [0, 1), got {min_p!r}")
    x = logits.to(torch.bfloat16).cpu()
    M, N = x.shape
    keys = _keys(x)
    skeys = keys.sort(dim=1, descending=True).values
    thr = skeys[:, top_k - 1:top_k].clone() if 0 < top_k < N else torch.zeros((M, 1), dtype=torch.int64)
    if not (top_p < 1.0 or min_p > 0.0):
        return thr
    inv_t = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temperature, dtype=torch.float32)
    kval = _key_values()
    kmax = skeys[:, :1]
    xmax = kval[kmax]  # (M, 1) fp32
    if top_p < 1.0:
        w = torch.exp(((kval[skeys] - xmax) * inv_t).double())
        w = torch.where(skeys >= thr, w, torch.zeros_like(w))  # thr is thr_k here
        need = float(torch.tensor(top_p, dtype=torch.float32)) * w.sum(dim=1, keepdim=True)
        # descending keys: the first position whose running mass reaches `need`
        # holds the boundary key (the mass of `key >= t` includes all of t's ties)
        j = (w.cumsum(dim=1) >= need).to(torch.int8).argmax(dim=1, keepdim=True)
        thr = torch.maximum(thr, skeys.gather(1, j))
    if min_p > 0.0:
        lmp = torch.log(torch.tensor(min_p, dtype=torch.float32).double()).float()
        ok = ((kval[None, :0xFF81] - xmax) * inv_t) >= lmp  # (M, keys up to +inf), monotone in the key
        first = torch.where(ok.any(dim=1, keepdim=True), ok.to(torch.int8).argmax(dim=1, keepdim=True),
                            torch.full((M, 1), 0xFF81, dtype=torch.int64))
        thr = torch.maximum(thr, torch.minimum(first, kmax))
    return thr


def sample_ref(logits: torch.Tensor, temperature: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
               seed: int = 0, step: Optional[torch.Tensor] = None, thr: Optional[torch.Tensor] = None,
               return_thr: bool = False):
    """Torch mirror of ``sample_rows``: the filter chain of
    ``filter_thresholds``, then ``sample_topk_ref``'s draw over the kept set.
    ``thr`` (M,) or (M, 1) overrides the final per-row key threshold (compare
    only the draw against a device run); ``return_thr`` also returns it (M,)."""
    x = logits.to(torch.bfloat16).cpu()
    M, N = x.shape
    keys = _keys(x)
    if thr is None:
        thr = filter_thresholds(x, temperature, top_k, top_p, min_p)
    thr = thr.cpu().to(torch.int64).reshape(M, 1)
    ids = _draw(x, keys, thr, temperature, seed, step)
    return (ids, thr.reshape(M).to(torch.int32)) if return_thr else ids


# ---------------------------------------------------------------------- penalties
# Torch mirror of csrc/kernels/penalties.hip.  State: one int16 per (row,
# vocabulary entry), bit 15 = P (the token occurs in the prompt), bits 0..14 =
# g (times generated in this generation, the prefill's token included;
# saturates at 0x7FFF).
PEN_P = 0x8000
PEN_G = 0x7FFF


def penalty_state(prompt_ids: torch.Tensor, vocab: int) -> torch.Tensor:
    """(B, vocab) int16 state of the (B, T) prompts: P set for every prompt token, g = 0."""
    ids = prompt_ids.to(device="cpu", dtype=torch.int64)
    st = torch.zeros((ids.shape[0], vocab), dtype=torch.int16)
    st.scatter_(1, ids, torch.full(ids.shape, -0x8000, dtype=torch.int16))
    return st


def penalty_count(state: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
    """A new state with ``g + 1`` (saturating) at ``tokens[row]`` of every row; P
    is kept and a token outside [0, vocab) is ignored."""
    u = state.cpu().view(torch.int16).to(torch.int64) & 0xFFFF
    tok = tokens.cpu().to(torch.int64).reshape(-1)
    for r in range(u.shape[0]):
        t = int(tok[r])
        if 0 <= t < u.shape[1] and (int(u[r, t]) & PEN_G) != PEN_G:
            u[r, t] += 1
    return torch.where(u >= 0x8000, u - 0x10000, u).to(torch.int16)


def apply_penalties_ref(logits: torch.Tensor, state: torch.Tensor, rep: float, freq: float,
                        pres: float) -> torch.Tensor:
    """The kernel's rule in torch fp32, operation by operation (so bitwise equal
    to it): for an entry with P or g > 0, ``x = x / rep if x > 0 else x * rep``
    (when rep != 1), then for g > 0 ``x = x - freq * g`` and ``x = x - pres``,
    rounded to bf16; every other entry keeps its bf16 bits.  ``logits`` (M, N)
    (rounded to bf16 first), ``state`` (M, >= N); returns bf16 on the CPU."""
    xb = logits.detach().to(device="cpu", dtype=torch.bfloat16)
    u = state.cpu().view(torch.int16)[:, :xb.shape[1]].to(torch.int64) & 0xFFFF
    g = u & PEN_G
    seen = u != 0
    f32 = torch.float32
    x = xb.to(f32)
    if float(rep) != 1.0:
        r = torch.tensor(float(rep), dtype=f32)
        x = torch.where(seen, torch.where(x > 0, x / r, x * r), x)
    gen = g > 0
    y = x - torch.tensor(float(freq), dtype=f32) * g.to(f32)
    y = y - torch.tensor(float(pres), dtype=f32)
    x = torch.where(gen, y, x)
    return torch.where(seen, x.to(torch.bfloat16), xb)


# ---------------------------------------------------------------------- log-probabilities
def logprobs_ref(logits: torch.Tensor, tokens: torch.Tensor, n: int):
    """Torch mirror of csrc/kernels/logprobs.hip: the fp64 ``log_softmax`` of
    the (M, N) logits rounded to bf16 (the values the argmax / sampler reads:
    after the penalties, before temperature and filters).  Returns
    ``(chosen (M,) fp32, top_ids (M, n) int32, top_lps (M, n) fp32)`` on the
    CPU: the log-probability of ``tokens[row]`` and the ``n`` most likely
    entries by a stable descending sort on the kernel's ordered key of the bf16
    bits, so equal bit patterns (common in bf16) come in ascending index order,
    -inf entries (log-probability -inf) last, and, as on the device, +0.0
    before -0.0 (equal as values, equal log-probabilities, distinct keys)."""
    n = int(n)
    xb = logits.detach().to(device="cpu", dtype=torch.bfloat16)
    M, N = xb.shape
    if not 0 <= n <= min(LOGPROBS_MAX_N, N):
        raise ValueError(f"logprobs: n = {n} outside [0, {min(LOGPROBS_MAX_N, N)}]")
    x = xb.to(torch.float64)
    lp = torch.log_softmax(x, dim=1)
    tok = tokens.detach().to(device="cpu", dtype=torch.int64).reshape(M)
    chosen = lp.gather(1, tok[:, None])[:, 0].to(torch.float32)
    order = torch.sort(_keys(xb), dim=1, descending=True, stable=True).indices[:, :n]
    return chosen, order.to(torch.int32), lp.gather(1, order).to(torch.float32)


# ---------------------------------------------------------------------- stop conditions
STOP_STATE_WORDS = 18  # csrc/kernels/api.h DNN_STOP_STATE_WORDS: g, finish length, reason code, 15 window entries
_STOP_WIN = STOP_STATE_WORDS - 3


def stop_state(rows: int, device="cpu") -> torch.Tensor:
    """The stop state of ``rows`` sequences at the beginning of a generation:
    int32 (rows, 18) = ``[g, finish length, reason code, window[0..15)]`` with
    nothing generated, nothing finished and the window all -1."""
    st = torch.zeros((rows, STOP_STATE_WORDS), dtype=torch.int32, device=device)
    st[:, 3:] = -1
    return st


def stop_reason(code: int):
    """A state's reason code as ``None`` (running), ``("token", index)`` or
    ``("sequence", index)``; the index is the one in the stage's list."""
    code = int(code)
    if code == 0:
        return None
    return ("token", code - 1) if code <= STOP_MAX_IDS else ("sequence", code - 1 - STOP_MAX_IDS)


def stop_ref(state: torch.Tensor, tokens: torch.Tensor, stop_ids, stop_seqs, min_new: int, pad: int):
    """One step of the stop conditions on host tensors: the torch mirror of
    ``dnn_stop_rows`` (csrc/kernels/stop.hip) and the one written definition.

    Per sequence, generated tokens count from 1: the token sampled from the
    prompt's last position is token 1.  ``g`` = tokens generated before this
    step.

    1. Suppression (``min_new > 0`` only, ``stop_suppress_ref``): while
       ``g < min_new`` every stop id's logit is bf16 -inf, after the penalties
       and before the argmax / sampler.  A finished row is left alone.
    2. The unchanged argmax / sampler picks token ``t``.
    3. This function, last in the step, per row:
       * finished already: ``t`` is replaced by ``pad``; the finish record does
         not change.
       * running: ``g += 1`` and ``t`` enters the row's window of the last 15
         generated tokens.  The row finishes with length ``g`` when ``t`` is a
         stop id (reason code 1 + index), else when the last ``len(s)``
         generated tokens equal stop sequence ``s`` and
         ``g >= max(min_new, len(s))`` (reason code 17 + index).  A stop id wins
         over a sequence, the lowest index wins within a kind.  The stop token
         or sequence stays in the output.  Prompt tokens never take part in a
         match (``g >= len(s)``: every compared token was generated; the
         window starts as -1).

    ``state`` int32 (M, 18) as ``stop_state`` lays it out (window newest
    first), ``tokens`` (M,) int.  Returns ``(new state, padded tokens int32)``;
    neither argument is changed."""
    st = state.detach().to(device="cpu", dtype=torch.int32).clone()
    M = st.shape[0]
    t = tokens.detach().to(device="cpu", dtype=torch.int32).reshape(M)
    if st.shape[1] != STOP_STATE_WORDS:
        raise ValueError(f"stop_ref: state (M, {STOP_STATE_WORDS}) expected, got {tuple(st.shape)}")
    fin = st[:, 1] != 0
    g1 = st[:, 0] + 1
    h = torch.cat([t[:, None], st[:, 3:]], 1)  # the last 16 generated tokens, newest first
    reason = torch.zeros((M,), dtype=torch.int32)
    for k in reversed(range(len(stop_seqs))):  # lower indices overwrite higher ones
        s = [int(e) for e in stop_seqs[k]]
        L = len(s)
        if not 1 <= L <= STOP_MAX_SEQ_LEN:
            raise ValueError(f"stop_ref: sequence length {L} outside 1..{STOP_MAX_SEQ_LEN}")
        hit = (h[:, :L] == torch.tensor(s[::-1], dtype=torch.int32)).all(1) & (g1 >= max(int(min_new), L))
        reason = torch.where(hit, torch.tensor(1 + STOP_MAX_IDS + k, dtype=torch.int32), reason)
    for k in reversed(range(len(stop_ids))):  # ... and a stop id overwrites every sequence
        reason = torch.where(t == int(stop_ids[k]), torch.tensor(1 + k, dtype=torch.int32), reason)
    run = ~fin
    new = st.clone()
    new[:, 0] = torch.where(run, g1, st[:, 0])
    new[:, 1] = torch.where(run & (reason != 0), g1, st[:, 1])
    new[:, 2] = torch.where(run, reason, st[:, 2])
    new[:, 3:] = torch.where(run[:, None], h[:, :_STOP_WIN], st[:, 3:])
    return new, torch.where(fin, torch.tensor(int(pad), dtype=torch.int32), t)


def stop_suppress_ref(logits: torch.Tensor, state: torch.Tensor, stop_ids, min_new: int) -> torch.Tensor:
    """Mirror of ``dnn_stop_suppress``: a copy of the (M, N) ``logits`` with -inf
    at every stop id of each row that is running and has generated fewer than
    ``min_new`` tokens."""
    x = logits.clone()
    if int(min_new) <= 0 or len(stop_ids) == 0:
        return x
    st = state.to(device=x.device)
    rows = (st[: x.shape[0], 1] == 0) & (st[: x.shape[0], 0] < int(min_new))
    ids = torch.tensor([int(i) for i in stop_ids], dtype=torch.int64, device=x.device)
    sub = x[:, ids]
    x[:, ids] = torch.where(rows[:, None], torch.full_like(sub, float("-inf")), sub)
    return x


# ---------------------------------------------------------------------- logit constraints
def constraints_store_prev(ctx: torch.Tensor, lens, prev, vocab: int) -> torch.Tensor:
    """A copy of the context table ``ctx`` (M, L) in which row ``r`` holds
    ``prev[r]`` at ``lens[r] - 1`` when ``prev[r]`` lies in ``[0, vocab)`` and
    ``1 <= lens[r] <= L``: the previous step's token becomes the newest entry
    of the row's context (what ``dnn_logit_constraints`` stores first)."""
    c = ctx.detach().to(device="cpu", dtype=torch.int32).clone()
    ls = [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
    ps = [int(v) for v in torch.as_tensor(prev).reshape(-1).tolist()]
    for r in range(c.shape[0]):
        if 0 <= ps[r] < int(vocab) and 1 <= ls[r] <= c.shape[1]:
            c[r, ls[r] - 1] = ps[r]
    return c


def constraints_ref(logits: torch.Tensor, cons, ctx: Optional[torch.Tensor] = None, lens=None,
                    prev=None) -> torch.Tensor:
    """The hard constraints on one step's logits: the torch mirror of
    ``dnn_logit_constraints`` (csrc/kernels/constraints.hip), bitwise equal to
    it, and the one written definition.

    A row's context is ``c[0..len)``: its own prompt tokens, then its generated
    tokens in order (``ctx[row, :len]``; pads are never part of it, a ragged
    row's context starts at its own length).  The rules run after the penalties
    and before the ``min_new_tokens`` suppression and the argmax / sampler, per
    row in this order:

    1. ``logit_bias`` ``{id: b}``: ``x[id] = bf16(float(x[id]) + b)``, one fp32
       add rounded to nearest even.  Entries not listed keep their bits.
    2. ``allowed_token_ids``: every entry of ``[0, V)`` not in the list becomes
       bf16 ``-inf``.
    3. ``bad_words_ids``: for each sequence ``s`` of length ``L``, when
       ``len >= L - 1`` and ``c[len-L+1 .. len) == s[0 .. L-1)``, the entry
       ``s[L-1]`` becomes ``-inf``.  A one-token sequence is banned at every
       step; prompt tokens take part in the match.
    4. ``no_repeat_ngram_size`` = n: for every ``j`` with ``0 <= j`` and
       ``j + n - 1 <= len - 1``, when ``c[j .. j+n-1) == c[len-n+1 .. len)``, the
       entry ``c[j+n-1]`` becomes ``-inf``.  ``n = 1`` bans every token of the
       context, a row with ``len < n`` bans nothing, and the suffix never
       matches itself (the token behind it does not exist yet).

    A ban wins over a bias on the same entry.  Context ids outside ``[0, V)``
    are compared but never used as an index.

    ``logits`` (M, V) (rounded to bf16 first); ``cons`` a
    ``config.ConstraintConfig``; ``ctx`` int (M, L) and ``lens`` (M,) ints (only
    read by rules 3 and 4; ``lens[r]`` outside ``[0, L]`` is clamped); ``prev``
    (M,) ints: ``constraints_store_prev`` first.  Returns bf16 on the CPU."""
    x = logits.detach().to(device="cpu", dtype=torch.bfloat16).clone()
    M, V = x.shape
    neg = float("-inf")
    if cons.logit_bias:
        ids = torch.tensor([k for k, _ in cons.logit_bias], dtype=torch.int64)
        b = torch.tensor([v for _, v in cons.logit_bias], dtype=torch.float32)
        x[:, ids] = (x[:, ids].to(torch.float32) + b[None, :]).to(torch.bfloat16)
    if cons.allowed_token_ids is not None:
        keep = torch.zeros((V,), dtype=torch.bool)
        keep[torch.tensor(list(cons.allowed_token_ids), dtype=torch.int64)] = True
        x[:, ~keep] = neg
    n = int(cons.no_repeat_ngram_size)
    if not cons.needs_context:
        for s in cons.bad_words_ids:
            x[:, int(s[0])] = neg
        return x
    if ctx is None or lens is None:
        raise ValueError("constraints_ref: bad words longer than one token and no_repeat_ngram_size need ctx and lens")
    c_all = ctx.detach().to(device="cpu", dtype=torch.int64)
    ls = [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
    if prev is not None:
        c_all = constraints_store_prev(c_all, ls, prev, V).to(torch.int64)
    for r in range(M):
        ln = min(max(ls[r], 0), c_all.shape[1])
        c = c_all[r, :ln]
        for s in cons.bad_words_ids:
            L = len(s)
            if ln >= L - 1 and (L == 1 or bool((c[ln - L + 1:] == torch.tensor(s[:-1], dtype=torch.int64)).all())):
                x[r, int(s[-1])] = neg
        if n > 0 and ln >= n:
            w = c.unfold(0, n, 1)  # window j = c[j .. j+n): ln - n + 1 of them
            hit = (w[:, :n - 1] == c[ln - n + 1:][None, :]).all(1)
            t = w[hit, n - 1]
            t = t[(t >= 0) & (t < V)]
            x[r, t] = neg
    return x


# ---------------------------------------------------------------------- ragged prompts
def ragged_last_rows_ref(h: torch.Tensor, lens: torch.Tensor, t0: int, Tc: int, B: int, d: int,
                         dst: torch.Tensor) -> torch.Tensor:
    """Torch mirror of ``dnn_ragged_last_rows`` (csrc/kernels/ragged.hip): ``h``
    (>= B * Tc, >= d) holds the hidden states of prompt positions
    ``[t0, t0 + Tc)`` of B sequences, row ``b * Tc + t``.  A copy of ``dst``
    (>= B, >= d) in which row ``b`` took ``h[b * Tc + q, :d]`` when
    ``q = lens[b] - 1 - t0`` lies in ``[0, Tc)``: the sequence's own last
    prompt position falls into this piece.  Every other row, and the columns
    past ``d``, keep what they held; ``lens[b] <= 0`` never matches."""
    out = dst.clone()
    q = lens.detach().to(device=h.device, dtype=torch.int64).reshape(-1)[:B] - 1 - int(t0)
    hit = (q >= 0) & (q < int(Tc))
    rows = torch.arange(B, dtype=torch.int64, device=h.device)[hit]
    out[rows, :d] = h[rows * int(Tc) + q[hit], :d].to(out.dtype)
    return out


def pick(logits: torch.Tensor, temperature: float = 0.0, top_k: int = 0, seed: int = 0,
         step: Optional[torch.Tensor] = None, top_p: float = 1.0, min_p: float = 0.0) -> torch.Tensor:
    """Greedy when temperature <= 0, else the Gumbel sample over the top-k /
    top-p / min-p survivors (CPU path)."""
    if temperature <= 0:
        return logits.argmax(dim=-1).to(torch.int32)
    if top_p >= 1.0 and min_p <= 0.0:
        return sample_topk_ref(logits, temperature, top_k, seed, step)
    return sample_ref(logits, temperature, top_k, top_p, min_p, seed, step)
