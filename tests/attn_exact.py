"""Exact-arithmetic "selector" fixtures for the attention kernels (helper module,
no tests, CPU torch only).

For one query every key score is one of three values, so the softmax weights
are exactly 0 or 1/n and a single key too many, too few or taken twice changes
the bf16 output:

  keys      ``4 * Had[c(j)]``: ``Had`` is the hd x hd Sylvester Hadamard matrix,
            ``c(j)`` a code in [0, hd).  A query is ``4 * Had[cq]``.  Entries
            are +-4 (exact in bf16 and e4m3); ``q . k`` is 16 hd for equal codes
            and 0 otherwise.  At the production scale 1/sqrt(hd) (times log2 e
            in the kernels) the gap is >= 184 in the exponent of exp2, so a
            non-selected probability is 0 in fp32 and a selected one exactly 1.
  values    whole numbers in [-15, 15], independent per key and dimension.
  counts    every query selects n in {1, 2, 4, 8, 16} of the keys it may see:
            the output is sum / n with |sum| <= 240, a bf16 number, whatever the
            block order, the split count and the way 1/l is formed.
  rescale   until a block or split meets its first selected key its maximum is
            0 and it sums the non-selected values at weight 1 (at most 2048 x 15,
            exact in fp32); the rescale or the combine weight must multiply
            that by exactly 0.
  poison    cache rows at or past a sequence's length (and the stale row a
            fused step overwrites) hold ``8 * Had[cq]`` in K: twice the selected
            score, a leaked key takes the whole softmax.  In V they hold NaN
            (bf16 0x7FC0, e4m3 0x7F).
  RoPE      cos / sin tables of quarter turns, entries in {0, +-1}, drawn per
            (position, frequency): the rotation is an exact signed permutation,
            and the fixture stores the inverse-rotated q and new k so that the
            rotated vectors are the Hadamard codes.  A wrong table row breaks
            the orthogonality.

The expected output is fp64 attention over the logical keys, rounded once to
bf16; the comparison is ``torch.equal``.

Prefill (``prefill``): key codes are pseudo-random over all hd codes (see
``_key_codes``); a query at absolute position p takes a code whose count among
keys 0..p is in {1, 2, 4, 8, 16}: c(p) (the diagonal is in the selected set),
c(p + 1) (the first masked key would match), or an eligible code whose keys
lie in two 64-key blocks (see ``_pick_queries``).  Heads of one kv group take
different codes (from position 32 on at the latest: the first few keys of a
sequence carry fewer codes than a group has heads).

Decode (``decode``): one query per (sequence, head), so the selected sets are
placed by hand: key len - 1 (the new key of a fused step), key 0, both sides of
every split boundary s * ceil(len / NS), and both sides of each ``edges`` entry
(a 16-key MFMA tile edge, a batch of rows in flight), dealt round-robin to the
heads of the kv group (each key has one code, so the sets of a group are
disjoint), then padded with free keys to a power of two (or cut to 16).  A
group with more heads than keys lets head g share the code of head
g % len.  All other keys take codes outside the group's reserved ones.
"""
import functools
import math
from dataclasses import dataclass
from typing import List, Optional

import torch

OK_COUNTS = (1, 2, 4, 8, 16)
VMAX = 15
BF16_NAN = 0x7FC0
E4M3_NAN = 0x7F
F8 = torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def hadamard(hd: int) -> torch.Tensor:
    """Sylvester Hadamard matrix (hd, hd), fp32 entries +-1."""
    h = torch.ones(1, 1)
    while h.shape[0] < hd:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == hd
    return h


def code_vec(codes: torch.Tensor, hd: int, amp: float = 4.0) -> torch.Tensor:
    """``amp * Had[codes]``: (..., hd) fp32."""
    return amp * hadamard(hd)[codes.long()]


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2**31))


def rope_tables(S: int, hd: int, seed: int = 0):
    """Quarter-turn tables (S, hd/2): (cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)} per entry."""
    k = torch.randint(0, 4, (S, hd // 2), generator=_gen(7, S, hd, seed))
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[k]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[k]
    return cos.contiguous(), sin.contiguous()


def rope(x: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor) -> torch.Tensor:
    """Rotate-half RoPE of x (..., hd) by table rows broadcastable to (..., hd/2), as the kernels write it."""
    h2 = x.shape[-1] // 2
    a, c = x[..., :h2], x[..., h2:]
    return torch.cat([a * cos_row - c * sin_row, c * cos_row + a * sin_row], -1)


def rope_inv(y: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor) -> torch.Tensor:
    """The vector whose rotation is y (the rotation is orthogonal: its transpose)."""
    return rope(y, cos_row, -sin_row)


def to_cache(x: torch.Tensor, kv8: bool) -> torch.Tensor:
    """fp32 (finite or NaN) -> the cache's storage type, NaN as 0x7FC0 / 0x7F."""
    nan = torch.isnan(x)
    y = torch.where(nan, torch.zeros_like(x), x)
    if kv8:
        out = y.to(F8)
        assert torch.equal(out.float(), y)
        out.view(torch.uint8)[nan] = E4M3_NAN
    else:
        out = y.to(torch.bfloat16)
        assert torch.equal(out.float(), y)
        out.view(torch.int16)[nan] = BF16_NAN
    return out


def bits(x: torch.Tensor) -> torch.Tensor:
    """Integer view of a bf16 / e4m3 tensor (NaN compares equal to itself)."""
    return x.view(torch.uint8 if x.element_size() == 1 else torch.int16)


def _nan_bytes(dtype) -> List[int]:
    """The sentinel pattern of one element, little endian: NaN (all-ones bits for integers)."""
    return {torch.bfloat16: [0xC0, 0x7F], F8: [E4M3_NAN], torch.float32: [0x00, 0x00, 0xC0, 0x7F]}.get(
        dtype, [0xFF] * torch.empty(0, dtype=dtype).element_size())


def _fill_nan(x: torch.Tensor) -> None:
    pat = torch.tensor(_nan_bytes(x.dtype), dtype=torch.uint8, device=x.device)
    x.view(torch.uint8).view(-1, pat.numel())[:] = pat


def guarded(x: torch.Tensor, dev) -> tuple:
    """A copy of x (n, ...) on ``dev`` between two sentinel slabs of NaN, each the size of x[0]: (buffer, view).
    The view is contiguous; ``guards_intact`` checks the slabs afterwards."""
    buf = torch.empty((x.shape[0] + 2,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
    _fill_nan(buf[0])
    _fill_nan(buf[-1])
    buf[1:-1] = x.to(dev)
    return buf, buf[1:-1]


def nan_like(shape, dtype, dev) -> tuple:
    """A NaN-filled output (n, ...) between two NaN sentinel slabs: (buffer, view)."""
    buf = torch.empty((shape[0] + 2,) + tuple(shape[1:]), dtype=dtype, device=dev)
    _fill_nan(buf)
    return buf, buf[1:-1]


def guards_intact(buf: torch.Tensor) -> bool:
    pat = torch.tensor(_nan_bytes(buf.dtype), dtype=torch.uint8, device=buf.device)
    return all(bool((buf[i].view(torch.uint8).view(-1, pat.numel()) == pat).all()) for i in (0, -1))


def untouched(x: torch.Tensor) -> torch.Tensor:
    """Per element: still the sentinel pattern ``nan_like`` wrote."""
    pat = torch.tensor(_nan_bytes(x.dtype), dtype=torch.uint8, device=x.device)
    return (x.contiguous().view(torch.uint8).view(-1, pat.numel()) == pat).all(-1).view(x.shape)


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
    """fp64 softmax(q k^T / sqrt(hd)) v for q (..., hd), k / v (n, hd): the fp64 result and its bf16 rounding."""
    hd = q.shape[-1]
    s = (q.double() @ k.double().T) / math.sqrt(hd)
    o = torch.softmax(s, -1) @ v.double()
    return o, o.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Prefill:
    B: int
    T: int
    H: int
    Hkv: int
    hd: int
    S: int
    pos: List[int]
    kcode: List[torch.Tensor]       # per b: (Hkv, pos[b] + T) key codes (cached and new)
    qcode: torch.Tensor             # (B, H, T)
    vals: List[torch.Tensor]        # per b: (Hkv, pos[b] + T, hd) fp32 whole numbers
    qkv: torch.Tensor               # (B*T, (H + 2 Hkv) hd) bf16: rows [q | k | v] of the chunk
    k0: torch.Tensor                # (B, Hkv, S, hd) fp32 cache before the chunk, poison from pos[b] on
    v0: torch.Tensor                # same, NaN from pos[b] on
    k1: torch.Tensor                # the cache after the chunk: rows pos[b] .. min(pos[b] + T, S) - 1 written
    v1: torch.Tensor
    out64: torch.Tensor             # (B*T, H*hd) fp64
    out: torch.Tensor               # the same rounded once to bf16
    rows: torch.Tensor              # (B*T,) bool: queries inside the cache (pos[b] + t < S)

    @property
    def G(self):
        return self.H // self.Hkv

    def selected(self, b: int, h: int, t: int) -> torch.Tensor:
        """Positions of the keys query (b, h, t) selects."""
        p = self.pos[b] + t
        return (self.kcode[b][h // self.G, :p + 1] == self.qcode[b, h, t]).nonzero().flatten()


_OWN_BEFORE = (0, 1, 3, 7, 15)   # counts a code may have before key p takes it, for c(p) to be eligible at query p
_NXT_BEFORE = OK_COUNTS          # counts among keys 0..p for c(p + 1) to be eligible at query p


def _key_codes(p0: int, T: int, G: int, hd: int, g: torch.Generator) -> List[int]:
    """Key codes of one kv head, pseudo-random over all hd codes.  Cached keys are uniform over the lower quarter.  Of the chunk's keys,
    nine in ten are drawn so that a preference of ``_pick_queries`` can hold: at chunk offsets 0, 1 (mod 4) the
    key's own query may select it, at offsets 2, 3 the query before it finds its code eligible.  The
    tenth key is a filler on a code neither preference can use at its count."""
    L = p0 + T
    uni = torch.randint(0, hd, (L,), generator=g).tolist()
    r = torch.rand(L, 2, generator=g).tolist()
    cnt = [0] * hd
    first = [-1] * hd
    out = []
    for p in range(L):
        c = uni[p] if p >= p0 else uni[p] // 4  # cached keys: the lower quarter, the chunk finds fresh codes
        t = p - p0
        cands = []
        if t >= 0 and p >= 64 and (t % 16 >= 12 or t >= T - 4):
            # the queries at t = 15, 31 (mod 32) and T - 1 must select keys in two 64-key blocks, each head of a
            # group its own: four keys in a row take a code so far seen only in earlier blocks
            cands = [x for x in range(hd) if cnt[x] in (1, 3, 7, 15) and first[x] != p >> 6]
        elif t >= 0 and r[p][0] < 0.9:
            before = _OWN_BEFORE if t % 4 < 2 else _NXT_BEFORE
            cands = [x for x in range(hd) if cnt[x] in before]
        elif t >= 0:  # a filler: a code at a count where neither preference can use it
            cands = [x for x in range(hd) if cnt[x] not in _OWN_BEFORE + _NXT_BEFORE]
        if cands:
            c = cands[uni[p] % len(cands)]
        n_elig = sum(n in OK_COUNTS for n in cnt)

        def elig_after(x):
            return n_elig + (cnt[x] + 1 in OK_COUNTS) - (cnt[x] in OK_COUNTS)

        if elig_after(c) < G:  # keep a code per head of the group eligible (the first positions cannot)
            best = max(elig_after(x) for x in range(hd))
            cands = [x for x in range(hd) if elig_after(x) == best]
            c = cands[uni[p] % len(cands)]
        cnt[c] += 1
        if first[c] < 0:
            first[c] = p >> 6
        out.append(c)
    return out


def _pick_queries(kl: List[int], p0: int, T: int, G: int, hd: int, g: torch.Generator) -> torch.Tensor:
    """Query codes (G, T) of one kv head with key codes kl (p0 + T).  At chunk offset t the head t % G takes c(p)
    when it is eligible ("own": the diagonal is selected) and the head (t + 1) % G takes c(p + 1) ("next": the
    first masked key would match); a single head takes own at even t and next at odd t, or whichever holds.  The
    queries at t = 15, 31 (mod 32) and the last one, and every head without a role, take an eligible code whose
    keys lie in two 64-key blocks where there is one."""
    kv_len = p0 + T
    cnt = [0] * hd
    first = [-1] * hd
    last = [-1] * hd
    tie = torch.rand(T, hd, generator=g).tolist()
    out = torch.zeros(G, T, dtype=torch.long)
    for p in range(kv_len):
        c = kl[p]
        cnt[c] += 1
        last[c] = p >> 6
        if first[c] < 0:
            first[c] = p >> 6
        if p < p0:
            continue
        t = p - p0
        elig = [x for x in range(hd) if cnt[x] in OK_COUNTS]
        assert elig, "no eligible code"
        elig.sort(key=lambda x: (first[x] == last[x], tie[t][x]))  # two-block codes first, then pseudo-random
        own = c if cnt[c] in OK_COUNTS else None
        nxt = kl[p + 1] if p + 1 < kv_len and cnt[kl[p + 1]] in OK_COUNTS and kl[p + 1] != c else None
        role = {}
        if t % 32 not in (15, 31) and t != T - 1:
            if G == 1:
                a, b_ = (own, nxt) if t % 2 == 0 else (nxt, own)
                role[0] = a if a is not None else b_
            else:
                role[t % G], role[(t + 1) % G] = own, nxt
        used = {x for x in role.values() if x is not None}
        for hg in range(G):
            pick = role.get(hg)
            if pick is None:
                # the first few positions of a sequence have fewer eligible codes than heads: share one
                pick = next((x for x in elig if x not in used), elig[hg % len(elig)])
            used.add(pick)
            out[hg, t] = pick
    return out


@functools.lru_cache(maxsize=64)
def prefill(B: int, T: int, H: int, Hkv: int, hd: int, pos: tuple, S: int, seed: int = 0) -> Prefill:
    G = H // Hkv
    had = hadamard(hd)
    g = _gen(1, B, T, H, Hkv, hd, S, seed, *pos)
    kcode, vals = [], []
    qcode = torch.zeros(B, H, T, dtype=torch.long)
    for b in range(B):
        L = pos[b] + T
        kcode.append(torch.tensor([_key_codes(pos[b], T, G, hd, g) for _ in range(Hkv)]))
        vals.append(torch.randint(-VMAX, VMAX + 1, (Hkv, L, hd), generator=g).float())
        for kvh in range(Hkv):
            qcode[b, kvh * G:(kvh + 1) * G] = _pick_queries(kcode[b][kvh].tolist(), pos[b], T, G, hd, g)
    ld = (H + 2 * Hkv) * hd
    qkv = torch.zeros(B, T, H + 2 * Hkv, hd)
    k0 = torch.zeros(B, Hkv, S, hd)
    v0 = torch.full((B, Hkv, S, hd), float("nan"))
    out64 = torch.zeros(B, T, H, hd, dtype=torch.float64)
    for b in range(B):
        p0, L = pos[b], pos[b] + T
        kfull = 4.0 * had[kcode[b]]                                   # (Hkv, L, hd)
        qkv[b, :, :H] = (4.0 * had[qcode[b]]).transpose(0, 1)
        qkv[b, :, H:H + Hkv] = kfull[:, p0:].transpose(0, 1)
        qkv[b, :, H + Hkv:] = vals[b][:, p0:].transpose(0, 1)
        k0[b, :, :p0] = kfull[:, :min(p0, S)]
        v0[b, :, :p0] = vals[b][:, :min(p0, S)]
        # poison: row r >= pos[b] matches one of the last (up to 32) queries of the chunk, each head of the group in turn
        r = torch.arange(p0, S)
        tq = T - 1 - ((r - p0) // G) % min(T, 32)
        for kvh in range(Hkv):
            k0[b, kvh, p0:] = 8.0 * had[qcode[b, kvh * G + (r - p0) % G, tq]]
        mask = torch.arange(L)[None, :] <= (p0 + torch.arange(T))[:, None]  # (T, L) causal at absolute positions
        for h in range(H):
            s = (4.0 * had[qcode[b, h]]).double() @ kfull[h // G].double().T / math.sqrt(hd)
            s = s.masked_fill(~mask, float("-inf"))
            out64[b, :, h] = torch.softmax(s, -1) @ vals[b][h // G].double()
    k1, v1 = k0.clone(), v0.clone()
    for b in range(B):
        n = min(pos[b] + T, S) - pos[b]
        k1[b, :, pos[b]:pos[b] + n] = qkv[b, :n, H:H + Hkv].transpose(0, 1)
        v1[b, :, pos[b]:pos[b] + n] = qkv[b, :n, H + Hkv:].transpose(0, 1)
    rows = torch.tensor([pos[b] + t < S for b in range(B) for t in range(T)])
    out64 = out64.reshape(B * T, H * hd)
    return Prefill(B, T, H, Hkv, hd, S, list(pos), kcode, qcode, vals, qkv.reshape(B * T, ld).to(torch.bfloat16), k0,
                   v0, k1, v1, out64, out64.to(torch.bfloat16), rows)


def prefill_rope_rows(fx: Prefill, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """``fx.qkv`` with q and k inverse-rotated at their positions (rows past the cache: the row is dropped, any
    table row does), so that qkv_split with these tables gives back the Hadamard codes."""
    x = fx.qkv.float().view(fx.B, fx.T, fx.H + 2 * fx.Hkv, fx.hd).clone()
    for b in range(fx.B):
        p = (fx.pos[b] + torch.arange(fx.T)).clamp(max=fx.S - 1)
        x[b, :, :fx.H + fx.Hkv] = rope_inv(x[b, :, :fx.H + fx.Hkv], cos[p][:, None], sin[p][:, None])
    return x.reshape(fx.B * fx.T, -1).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Decode:
    B: int
    H: int
    Hkv: int
    hd: int
    S: int
    splits: int
    fused: bool
    rope: bool
    lens: List[int]                 # keys attended per sequence
    pos: Optional[List[int]]        # fused: tokens already cached (pos[b] == S: the new row is dropped)
    kcode: List[torch.Tensor]       # per b: (Hkv, lens[b])
    qcode: torch.Tensor             # (B, H)
    sel: List[List[List[int]]]      # [b][h]: the selected key positions
    vals: List[torch.Tensor]        # per b: (Hkv, lens[b], hd)
    q: torch.Tensor                 # (B, H, hd) bf16 (head-major route)
    qkv: Optional[torch.Tensor]     # fused: (B, ld) bf16 rows [q | k | v | NaN pad], inverse-rotated when rope
    cos: Optional[torch.Tensor]
    sin: Optional[torch.Tensor]
    k0: torch.Tensor                # (B, Hkv, S, hd) fp32 before the step
    v0: torch.Tensor
    k1: torch.Tensor                # after the step (fused: row pos[b] written where pos[b] < S)
    v1: torch.Tensor
    out64: torch.Tensor             # (B, H*hd)
    out: torch.Tensor

    @property
    def G(self):
        return self.H // self.Hkv


def boundaries(n: int, ns: int) -> List[int]:
    """First keys of splits 1.. of a context of n keys cut into ns splits of ceil(n / ns), as the kernels cut it."""
    chunk = -(-n // ns)
    return [s * chunk for s in range(1, ns) if s * chunk < n]


def _place(n: int, G: int, ns: int, edges, rot: int, g: torch.Generator):
    """Selected key sets of the heads of one kv group over n keys: [head] -> sorted positions."""
    extra = boundaries(n, ns) + [e for e in edges if e < n]
    extra = extra[rot % max(1, len(extra)):] + extra[:rot % max(1, len(extra))]  # the 16-key cap drops the tail
    must = [n - 1, 0]
    for e in extra:
        must += [e - 1, e]
    must = list(dict.fromkeys(must))
    nh = min(G, n)
    sets = [[] for _ in range(nh)]
    for i, key in enumerate(must):
        sets[(i + rot) % nh].append(key)
    taken = set(must)
    pool = [x for x in torch.randperm(n, generator=g).tolist() if x not in taken]
    for s in sets:  # n >= nh keys: a head the deal left empty finds a free key
        if not s:
            s.append(pool.pop())
    for s in sets:
        del s[16:]
        want = 1
        while want < len(s):
            want *= 2
        while len(s) < want and pool:
            s.append(pool.pop())
        while len(s) not in OK_COUNTS:  # the pool ran dry: cut to the power of two below
            s.pop()
    return [sorted(s) for s in sets]


@functools.lru_cache(maxsize=8)
def decode(B: int, H: int, Hkv: int, hd: int, S: int, lens: tuple, splits: int, fused: bool = False,
           rope_on: bool = False, edges: tuple = (16,), seed: int = 0, ld_pad: int = 8) -> Decode:
    """``lens``: keys attended (head-major route) or, fused, the positions pos[b] (pos[b] == S drops the new row)."""
    G = H // Hkv
    assert G <= 8 and hd >= 2 * G
    had = hadamard(hd)
    g = _gen(2, B, H, Hkv, hd, S, splits, fused, rope_on, seed, *lens, *edges)
    pos = list(lens) if fused else None
    n_of = [min(p + 1, S) for p in lens] if fused else [min(n, S) for n in lens]
    cos = sin = None
    if rope_on:
        cos, sin = rope_tables(S, hd, seed)
    qcode = torch.zeros(B, H, dtype=torch.long)
    kcode, vals, sel = [], [], []
    k0 = torch.zeros(B, Hkv, S, hd)
    v0 = torch.full((B, Hkv, S, hd), float("nan"))
    out64 = torch.zeros(B, H, hd, dtype=torch.float64)
    for b in range(B):
        n = n_of[b]
        kc = torch.zeros(Hkv, n, dtype=torch.long)
        sel_b = [None] * H
        for kvh in range(Hkv):
            perm = torch.randperm(hd, generator=g)
            res, free = perm[:G], perm[G:]
            kc[kvh] = free[torch.randint(0, hd - G, (n,), generator=g)]
            sets = _place(n, G, splits, edges, b + kvh, g)
            for hg in range(G):
                j = hg % len(sets)
                qcode[b, kvh * G + hg] = res[j]
                kc[kvh, sets[j]] = res[j]
                sel_b[kvh * G + hg] = sets[j]
            # poison past the length: 8 x the code of each head of the group in turn
            r = torch.arange(n, S)
            k0[b, kvh, n:] = 8.0 * had[res[r % min(G, n)]]
        kcode.append(kc)
        sel.append(sel_b)
        vals.append(torch.randint(-VMAX, VMAX + 1, (Hkv, n, hd), generator=g).float())
        k0[b, :, :n] = 4.0 * had[kc]
        v0[b, :, :n] = vals[b]
        for h in range(H):
            out64[b, h] = reference(4.0 * had[qcode[b, h]], k0[b, h // G, :n], vals[b][h // G])[0]
    qv = 4.0 * had[qcode]                                              # (B, H, hd)
    k1, v1 = k0.clone(), v0.clone()
    qkv = None
    if fused:
        ld = (H + 2 * Hkv) * hd + ld_pad
        row = torch.full((B, ld), float("nan"))
        for b in range(B):
            p = pos[b]
            pr = min(p, S - 1)
            qb = qv[b]
            if p < S:  # the new row: taken out of the cache, stale poison (the row's own head codes) in its place
                kn, vn = k0[b, :, p].clone(), v0[b, :, p].clone()
                heads = [next(h for h in range(kvh * G, (kvh + 1) * G) if p in sel[b][h]) for kvh in range(Hkv)]
                k0[b, :, p] = 8.0 * had[qcode[b, heads]]
                v0[b, :, p] = float("nan")
            else:      # dropped: the row offered is poison and must not be used
                kn = 8.0 * had[qcode[b, ::G]]
                vn = torch.full((Hkv, hd), float("nan"))
            if rope_on:
                qb = rope_inv(qb, cos[pr], sin[pr])
                kn = rope_inv(kn, cos[pr], sin[pr])
            row[b, :H * hd] = qb.reshape(-1)
            row[b, H * hd:(H + Hkv) * hd] = kn.reshape(-1)
            row[b, (H + Hkv) * hd:(H + 2 * Hkv) * hd] = vn.reshape(-1)
        qkv = to_cache(row, False)
    out64 = out64.reshape(B, H * hd)
    return Decode(B, H, Hkv, hd, S, splits, fused, rope_on, n_of, pos, kcode, qcode, sel, vals, qv.to(torch.bfloat16),
                  qkv, cos, sin, k0, v0, k1, v1, out64, out64.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------
# the cases shared by the CPU and GPU tests
# ---------------------------------------------------------------------------------------------------------------
# (B, T, pos, S): T + pos crosses the 32-row wave slab, the 64-key block and the 128-query block at -1, 0, +1;
# the fourth has a different pos per sequence; the last has S = pos + T - 1 (the overflow row is dropped)
PREFILL_CASES = [(2, 1, (0, 0), 6), (1, 33, (40,), 78), (2, 129, (64, 64), 198), (2, 130, (63, 64), 199),
                 (3, 193, (0, 0, 0), 198), (2, 300, (250, 250), 549)]
PREFILL_HEADS = [(4, 4), (4, 2), (8, 2), (4, 1)]  # (H, Hkv): MHA, G = 2, G = 4, G = 4 on a single kv head


def decode_lens(S: int, splits: int, batch: int, fused: bool = False) -> tuple:
    """Context lengths of one decode case: 1 and 2; splits - 1, splits, splits + 1 (empty splits); 15, 16, 17; one
    below, at and one above ``batch`` (a full batch of rows in flight); S.  Fused: the positions len - 1, and
    pos = S (the new row is dropped, attention over the S cached keys)."""
    ls = [1, 2, splits - 1, splits, splits + 1, 15, 16, 17, batch - 1, batch, batch + 1, S]
    ls = list(dict.fromkeys(n for n in ls if 1 <= n <= S))
    return tuple([n - 1 for n in ls] + [S]) if fused else tuple(ls)


def prefill_id(case):
    B, T, pos, S = case
    return f"B{B}-T{T}-p{'_'.join(map(str, pos))}-S{S}"


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' summation orders (CPU tests)
# ---------------------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634


def _bf16r(x):
    return x.to(torch.bfloat16).float()


def emulate_online(q, k, v, qpos, order=1, block=64):
    """fp32 online softmax of queries q (T, hd) at absolute positions qpos (T,) over keys k / v (L, hd) in blocks
    of ``block`` keys walked forwards (order 1) or backwards (-1), as flash_attn_kernel does it: raw-score maximum,
    scale folded into the exp2 argument, probabilities rounded to bf16 for P.V, one final multiply by 1 / l."""
    hd = q.shape[1]
    sl2 = torch.tensor(LOG2E / math.sqrt(hd), dtype=torch.float32)
    T, L = q.shape[0], k.shape[0]
    m = torch.full((T,), float("-inf"))
    l = torch.zeros(T)
    o = torch.zeros(T, hd)
    starts = list(range(0, L, block))[::order]
    for kb0 in starts:
        kk = torch.arange(kb0, min(kb0 + block, L))
        s = (q @ k[kk].T).float()
        s = s.masked_fill(kk[None, :] > qpos[:, None], float("-inf"))
        m_new = torch.maximum(m, s.max(-1).values * sl2)
        m_use = torch.where(m_new == float("-inf"), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_use)
        p = torch.exp2(s * sl2 - m_use[:, None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[:, None] + _bf16r(p) @ v[kk]
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return (o * inv[:, None]).to(torch.bfloat16)


def emulate_split(q, k, v, ns):
    """fp32 split-and-combine of one query q (hd,) over k / v (n, hd) cut into ns splits of ceil(n / ns), as
    attn_decode_kernel and the combine kernels do it (empty splits neutral)."""
    hd = q.shape[0]
    sl2 = torch.tensor(LOG2E / math.sqrt(hd), dtype=torch.float32)
    n = k.shape[0]
    chunk = -(-n // ns)
    parts = []
    for s in range(ns):
        k0_, k1_ = s * chunk, min(n, (s + 1) * chunk)
        if k0_ >= k1_:
            parts.append((torch.zeros(hd), torch.tensor(float("-inf")), torch.tensor(0.0)))
            continue
        sc = (k[k0_:k1_] @ q).float() * sl2
        mx = sc.max()
        e = torch.exp2(sc - mx)
        parts.append((_bf16r(e) @ v[k0_:k1_], mx, e.sum()))
    if ns == 1:
        return (parts[0][0] / parts[0][2]).to(torch.bfloat16)
    m = torch.stack([p[1] for p in parts]).max()
    l = torch.tensor(0.0)
    acc = torch.zeros(hd)
    for o_, m_, l_ in parts:
        if m_ != float("-inf"):
            e = torch.exp2(m_ - m)
            l = l + l_ * e
            acc = acc + o_ * e
    return (acc * (1.0 / l)).to(torch.bfloat16)
