"""Element-exact fixtures for LayerNorm / RMSNorm and the folded-norm GEMMs (helper module, no tests).

The norm routes cannot be bit-exact in every order: 1 / K is no power of two, ``rsqrtf`` is not
correctly rounded and ``eps`` is added to the variance.  Everything else is made exact.  The
activations are whole numbers (bf16-exact), the folded weights ``W diag(gamma)`` lie on the grids of
tests/gemm_exact.py, so ``acc = x . W'^T`` is a whole number of units below 2^24: exact in fp32 in
any order.  ``colsum``, the folded bias ``W beta + b`` and the residual are exact too.  What is left
to the device is a relative error of a few 2^-24 in ``mean`` and ``rstd`` and three or four fp32
roundings in the epilogue.  The expected output is therefore ``bf16(y64)`` with

    y64 = rstd64 (acc - mean64 colsum) + bias' -> act (+ residual)              (folded GEMMs)
    y64 = (x - mean64) rstd64 gamma + beta                                      (plain norm)

in fp64 with the same ``eps``, and the device must match it bit for bit at every element whose
``y64`` lies further than ``tau S`` from the nearest bf16 rounding boundary;
``S = |rstd acc| + |rstd mean colsum| + |bias'| + |residual|`` (plain norm: ``NC |(x - mean) rstd
gamma| + |mean rstd gamma| + |beta|``, see ``plain_terms``) is the magnitude the fp32 epilogue actually holds.  Elements inside the band are
left out; the band is narrow.

``tau`` is not chosen: it is 16 times the worst *need* of the fp32 mirrors of the kernels' arithmetic
on the fixtures below, rounded up to a power of two.  The need of a mirror is the largest
``distance / S`` over its elements that differ from ``bf16(y64)``.  The mirrors (sums in a fixed order,
so the needs do not depend on the host):

  two_pass   norm_kernel / row_stats_kernel + epi_norm4:  mean = sum / K;  var = sum (x - mean)^2 / K
             (each lane its fragments in turn, then a butterfly);  v = acc rstd + (-mean rstd) colsum
  one_pass   sk_stats and the skinny / stream / one-shot / head epilogues: shifted by c = x[0],
             d = s1 (1 / K); mean = c + d; var = max(q (1 / K) - d d, 0); v = rstd (acc - mean colsum)
  partials   epi_rowstat16 + rowstat_merge: {mean, M2} per 16 columns, merged by 8 lanes with the shift
             of partial 0; the one_pass epilogue
  plain      norm_kernel's output: two_pass statistics, (x - mean) rstd gamma + beta

The shifted one-pass formula is worse conditioned than a two-pass one where the row's first element
lies off the mean (class e, by design): ``condition`` adds what that costs to ``S`` of the one_pass and
partials forms, from the data, so that one ``tau`` serves every row.

tests/test_norm_exact.py computes the needs and the masked shares and compares them with the
constants here and its own records.  Fixtures (M, N, K), LayerNorm and RMSNorm, none and ReLU, bias +
residual; masked shares at ``TAU`` are the worst over the three forms:

  fixture                  worst need   class (e) rows, one_pass   masked: all / ordinary row / c, f row / column
  thin  (64, 1024, 768)    2^-24.15     2^-25.58                   3.0 % / 4.0 % / 14.0 % / 14.1 %
  dense (64, 400, 1600)    2^-24.58     2^-26.17                   2.8 % / 6.5 % / 14.7 % / 10.9 %
  dense (33, 512, 4096)    2^-24.05     2^-30.04                   3.1 % / 5.1 % / 13.9 % / 18.2 %

  NEED_LOG2 = -24 (the worst, rounded up to a whole power of two), TAU = 2^(NEED_LOG2 + 4) = 2^-20.

  plain norm (rows of ``activations(N, plain=True)``, gamma and beta of ``_plain_tables``), 37 rows, widths
  8 .. 8192, LayerNorm with and without beta, RMSNorm: worst need 2^-24.16 (at 256; 2^-24.18 at 8192, no
  differing element at 8).  NEED_PLAIN_LOG2 = -24, TAU_PLAIN = 2^-20.  Masked at most 1.7 % overall, 3.3 % in
  an ordinary row (one element of eight at N = 8), 12.5 % in a large-mean row, 16.2 % in a column.

Caps (asserted on the CPU for the GEMM fixtures and for every width and variant of the plain norm):
masked share at most 5 % overall, 10 % in
any row of the ordinary classes, 50 % in any large-mean or constant row, 25 % in any column, no row
or column fully masked.

Activations: whole numbers, |x| <= ``xmax(K)`` (256 up to K = 1024, halved for each doubling of K,
so that K xmax max|w'| stays below 2^24 units: ``bound_units``).  Row m is of class
``CLASSES[m % 8]``, so adjacent rows never share statistics:

  a  sigma about 1, mean 0                       e  first-element outlier: x[0] about 6 sigma off the mean
  b  sigma about 16, mean about 10               f  zero row, as a padding row (variance 0, rstd = eps^-1/2)
  c  |mean| / sigma >= 50 (+-25 +- 1)            g  zero but for the last 8 columns
  d  spike row: constant but for 12 spikes at    h  random sigma and mean
     0, K - 1, both sides of the 8-, 64- and 512-element boundaries and of K / 2 and K / 4

For every row the shifted sums ``sum (x - x[0])`` and ``sum (x - x[0])^2`` stay below 2^24, so the
one-pass kernels' statistics sums are exact in any order and only their last few operations round.

Weights: ``gamma`` in {+-1/2, +-1, +-2}, ``beta`` small whole numbers / 4, W on the dense / thin grid
of gemm_exact.py, the residual whole numbers / 4 and the bias whole numbers / 4 + 2^-7: off the 2^-6 grid
of W beta + residual, so that a zero row's output, which nothing else moves, is never an exact tie.  The bf16 layers go through the real ``ops.gemm.fold_norm``, so the fold itself is under test.  The
W8A16 layers do not: ``fold_norm(fp8=True)`` quantises with absmax / 448, which is no power of two, so
``folded`` builds them from (q, power-of-two scale) with its own copy of the fold's formulas, and
``assert_fold_exact`` then checks that construction, not the project's fp8 fold.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

import gemm_exact as ge

EPS = 1e-5
CLASSES = "abcdefgh"
M_MAX, K_MAX = 384, 8192
NEED_LOG2 = -24
TAU_LOG2 = NEED_LOG2 + 4
TAU = 2.0 ** TAU_LOG2
NEED_PLAIN_LOG2 = -24          # the plain norm's mirror, widths up to 8192 (its sum of squares has 8192 terms)
TAU_PLAIN = 2.0 ** (NEED_PLAIN_LOG2 + 4)
PLAIN_WIDTHS = (8, 256, 520, 768, 1600, 4096, 8192)
PLAIN_ROWS = 37
# row_stats: log2 of the relative tolerance of {rstd, -mean rstd} per width, (LayerNorm, RMSNorm): 16 x the fp32
# two-pass mirror's worst relative error on the first 37 rows of ``activations(N)``, rounded up to a power of two
ROWSTAT_TOL_LOG2 = {8: (-19, -19), 256: (-18, -19), 520: (-18, -19), 768: (-19, -19), 1600: (-18, -19), 4096: (-16, -19), 8192: (-15, -19)}
CAPS = {"all": 0.05, "row": 0.10, "row_cf": 0.50, "col": 0.25}
BF16_FMT = (8, -126)   # significant bits, exponent of the smallest normal number
E4M3_FMT = (4, -6)


def xmax(K: int) -> int:
    """The activation range at width K: K * xmax * 60 < 2^24 (60 units = the dense weight's 15 times
    gamma = 2 on the grid of gamma = 1/2)."""
    return 256 if K <= 1024 else 128 if K <= 2048 else 64 if K <= 4096 else 32


def spike_positions(K: int):
    pos = {0, K - 1, K // 2 - 1, K // 2, K // 4 - 1, K // 4}
    for b in (8, 64, 512):
        if b < K:
            pos |= {b - 1, b}
    return sorted(p for p in pos if 0 <= p < K)


@functools.lru_cache(maxsize=None)
def activations(K: int, seed: int = 0, plain: bool = False) -> torch.Tensor:
    """(M_MAX, K) fp32 whole numbers, row m of class ``CLASSES[m % 8]``; smaller M is a prefix.
    ``plain``: the rows of the plain-norm fixtures.  The plain norm subtracts the mean from each element,
    so an element that sits on the mean leaves nothing but the mean's own rounding; there the large-mean
    rows (c) are +-120 +- 1, 2 or 3 with no element on the mean (|mean| / sigma >= 50) and the spike rows
    (d) stand on a base that steps above and below its level; the means of the b, e and h rows lie half
    way between whole numbers.  Rows of one class differ in their value sets and sigma, so that their
    normalised values do not coincide: a column whose beta cancels one of them (an output next to zero,
    inside the band) then loses that row, not the class."""
    g = torch.Generator().manual_seed(7000 + 13 * seed + K + (500000 if plain else 0))
    xm = xmax(K)

    def normal(sigma, mean):
        if plain and mean != 0:  # a mean half way between whole numbers: no element within 1 / 2 of it
            mean += 0.5
        return (torch.randn(K, generator=g, dtype=torch.float64) * sigma + mean).round().clamp(-xm, xm)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))

    rows = []
    for m in range(M_MAX):
        c, sign = CLASSES[m % 8], 1 - 2 * ((m // 8) % 2)
        wide = 1 + 0.3 * ((m // 8) % 5) if plain else 1.0  # plain: no two rows of a class with one sigma
        if c == "a":
            r = normal(1.0 * wide, 0.0)
        elif c == "b":
            r = normal(min(16.0, xm / 8), sign * min(10.0, xm / 8))
        elif c == "c" and plain:  # 120 +- 1 or +- a, a = 2 or 3, shares that differ from one c row to the next
            i = m // 8
            amp = torch.where(torch.rand(K, generator=g) < 0.3 + 0.1 * (i % 5), 1.0, 2.0 + i % 2).double()
            r = sign * 120.0 + amp * (1 - 2 * torch.randint(0, 2, (K,), generator=g).double())
        elif c == "c":  # +-25 + {-1, 0, 1}, a tenth each: sigma = sqrt(0.2), |mean| / sigma = 56
            t = torch.randint(0, 10, (K,), generator=g)
            r = sign * 25.0 + (t == 0).double() - (t == 1).double()
            r[0] = sign * 25.0  # the one-pass shift sits on the mean: the class is about |mean| / sigma alone
        elif c == "d":
            r = torch.full((K,), float(sign * 3), dtype=torch.float64)
            if plain:  # the base: one element i + 1 above the level, then i + 1 elements one below
                i = (m // 8) % 5
                r += torch.where(torch.arange(K) % (i + 2) == 0, float(i + 1), -1.0).double()
            for i, p in enumerate(spike_positions(K)):
                r[p] += (1 - 2 * (i % 2)) * (1 if p == 0 else 2 + (5 * i + m // 8) % (xm // 8))
        elif c == "e":
            sg = max(1.0, xm / 64)
            r = normal(sg * wide, sign * 2.0)
            r[0] = sign * 2.0 + round(6 * sg)
        elif c == "f":
            r = torch.zeros(K, dtype=torch.float64)
        elif c == "g":
            r = torch.zeros(K, dtype=torch.float64)
            t = torch.randint(1, xm // 4 + 1, (8,), generator=g).double()
            r[K - 8:] = t * (1 - 2 * torch.randint(0, 2, (8,), generator=g).double())
        else:
            r = normal(1 + ri(0, max(1, xm // 10) - 1), sign * ri(0, max(1, 20 * xm // 256)))
        rows.append(r)
    x = torch.stack(rows)
    d = x - x[:, :1]
    assert float(d.abs().sum(1).max()) < 2**24 and float((d * d).sum(1).max()) < 2**24, "shifted sums leave 2^24"
    return ge._roundtrip(x, torch.bfloat16)


def row_classes(M: int) -> str:
    return "".join(CLASSES[m % 8] for m in range(M))


@functools.lru_cache(maxsize=None)
def _norm_tables(K: int, seed: int = 0):
    g = torch.Generator().manual_seed(9000 + seed)
    e = torch.randint(-1, 2, (K_MAX,), generator=g).double()
    s = 1 - 2 * torch.randint(0, 2, (K_MAX,), generator=g).double()
    beta = torch.randint(-4, 5, (K_MAX,), generator=g).double() / 4
    return (s * 2.0**e)[:K], beta[:K]


@dataclass(frozen=True)
class NormFixture:
    kind: str                     # dense / thin: the grid of W
    wfmt: str                     # bf16 / w8
    x: torch.Tensor               # (M,K) fp32 whole numbers
    gamma: torch.Tensor           # (K,) fp32
    beta: torch.Tensor            # (K,) fp32 (LayerNorm only)
    w: torch.Tensor               # (N,K) fp32: W before the fold (w8: before the channel scale)
    sw: Optional[torch.Tensor]    # (N,) fp32 channel scales, w8 only
    bias: torch.Tensor            # (N,) fp32
    res: torch.Tensor             # (M,N) fp32, bf16-exact
    bound_units: float            # K * xmax * max|w'| in units of the accumulator's grid


def fixture(kind: str, M: int, N: int, K: int, wfmt: str = "bf16", seed: int = 0) -> NormFixture:
    if not (1 <= M <= M_MAX and 1 <= N <= ge.N_MAX and 8 <= K <= K_MAX):
        raise ValueError((M, N, K))
    _, wi, _, _ = ge._tables(kind, seed)
    _, _, bi, ri = ge._tables("thin", seed)
    dense, w8 = kind == "dense", wfmt == "w8"
    step_w = 2.0**-4 if dense and not w8 else 1.0
    gamma, beta = _norm_tables(K, seed)
    sw = 2.0 ** -(3 + torch.arange(N) % 3).double() if w8 else None
    wmax_units = (15 if dense else 1) * 4  # |w| max times gamma = 2, in units of gamma = 1/2
    bound = K * xmax(K) * wmax_units
    assert bound < 2**24, (K, bound)
    return NormFixture(kind, wfmt, activations(K, seed)[:M], gamma.float(), beta.float(),
                       (wi[:N, :K].double() * step_w).float(), None if sw is None else sw.float(),
                       (bi[:N].double() / 4 + 2.0**-7).float(), ge._roundtrip(ri[:M, :N].double() / 4, torch.bfloat16), float(bound))


def fixture_from_x(kind: str, x: torch.Tensor, N: int, wfmt: str = "bf16", seed: int = 0) -> NormFixture:
    """The fixture of ``kind`` at (M, N, K) with the given whole-number activations ``x`` (M, K) in place
    of the class rows: the consumer of a producer GEMM's output.  (The shifted sums of such rows are not
    held below 2^24: the one-pass statistics then round in their sums too, within ``condition``.)"""
    M, K = x.shape
    f = fixture(kind, min(M, M_MAX), N, K, wfmt, seed)
    x = ge._roundtrip(x.double(), torch.bfloat16)
    assert torch.equal(x, x.round())
    bound = K * float(x.abs().max()) * (15 if kind == "dense" else 1) * 4
    assert bound < 2**24
    return NormFixture(kind, wfmt, x, f.gamma, f.beta, f.w, f.sw, f.bias, f.res[:M], bound)


@dataclass(frozen=True)
class Fold64:
    q: torch.Tensor        # (N,K) fp64: W diag(gamma) before the channel scale (bf16: the folded weight itself)
    w: torch.Tensor        # (N,K) fp64: the folded weight W' = q * sw
    bias: torch.Tensor     # (N,) fp64: W beta + b (RMSNorm, or bias False and no beta: b or zeros)
    colsum: torch.Tensor   # (N,) fp64: row sums of W' (RMSNorm: zeros)


def fold64(fx: NormFixture, rms: bool, bias: bool = True, beta: bool = True) -> Fold64:
    """The fold in fp64 (exact: every term is a whole number of units far below 2^53)."""
    sw = torch.ones(fx.w.shape[0], dtype=torch.float64) if fx.sw is None else fx.sw.double()
    q = fx.w.double() * fx.gamma.double()[None, :]
    w = q * sw[:, None]
    b = fx.bias.double() if bias else torch.zeros(fx.w.shape[0], dtype=torch.float64)
    if beta and not rms:
        b = b + (fx.w.double() * sw[:, None]) @ fx.beta.double()
    return Fold64(q, w, b, torch.zeros_like(b) if rms else w.sum(1))


@dataclass(frozen=True)
class Stats64:
    mean: torch.Tensor       # (M,) (RMSNorm: zeros)
    var: torch.Tensor        # (M,)
    rstd: torch.Tensor       # (M,)
    partials: torch.Tensor   # (M, ceil(K / 16), 2): {mean, M2} of each 16-column tile
    rowstat: torch.Tensor    # (M, 2): {rstd, -mean rstd}


def stats_of(x64: torch.Tensor, rms: bool = False, eps: float = EPS) -> Stats64:
    M, K = x64.shape
    mean = torch.zeros(M, dtype=torch.float64, device=x64.device) if rms else x64.mean(1)
    var = ((x64 - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    P = -(-K // 16)
    xp = torch.nn.functional.pad(x64, (0, 16 * P - K)).view(M, P, 16)
    cnt = torch.full((P,), 16.0, dtype=torch.float64, device=x64.device)
    cnt[-1] = K - 16 * (P - 1)
    pm = xp.sum(-1) / cnt
    valid = (torch.arange(16 * P, device=x64.device) < K).view(P, 16)
    m2 = (((xp - pm[..., None]) ** 2) * valid).sum(-1)
    return Stats64(mean, var, rstd, torch.stack([pm, m2], -1), torch.stack([rstd, -mean * rstd], -1))


def stats64(fx: NormFixture, rms: bool = False, eps: float = EPS) -> Stats64:
    return stats_of(fx.x.double(), rms, eps)


@dataclass(frozen=True)
class Terms:
    """The fp64 terms of ``y = rstd (acc - mean colsum) + bias -> act (+ res)`` on one device."""
    acc: torch.Tensor                # (M,N)
    mean: torch.Tensor               # (M,)
    rstd: torch.Tensor               # (M,)
    colsum: torch.Tensor             # (N,)
    bias: torch.Tensor               # (N,)
    res: Optional[torch.Tensor]      # (M,N) or None
    act: Optional[str]
    cond: Optional[torch.Tensor] = None  # (M, 2) ``condition`` of a one-pass route, or None

    def rows(self, M: int) -> "Terms":
        return Terms(self.acc[:M], self.mean[:M], self.rstd[:M], self.colsum, self.bias,
                     None if self.res is None else self.res[:M], self.act, None if self.cond is None else self.cond[:M])

    def with_(self, **kw) -> "Terms":
        d = dict(acc=self.acc, mean=self.mean, rstd=self.rstd, colsum=self.colsum, bias=self.bias, res=self.res,
                 act=self.act, cond=self.cond)
        d.update(kw)
        return Terms(**d)

    def to(self, device) -> "Terms":
        mv = lambda t: None if t is None else t.to(device)
        return Terms(mv(self.acc), mv(self.mean), mv(self.rstd), mv(self.colsum), mv(self.bias), mv(self.res), self.act,
                     mv(self.cond))


FORMS = ("two_pass", "one_pass", "partials")


def condition(x64: torch.Tensor, form: str, rms: bool, eps: float = EPS) -> Optional[torch.Tensor]:
    """(M, 2) {A, |c - mean|}: what the shifted one-pass statistics add to ``S``.  Those kernels compute
    d = E[x - c], mean = c + d and var = E[(x - c)^2] - d^2 with c = x[0] (``partials``: c = the mean of
    the first 16 columns).  Both terms of var are up to A = 1 + (c - mean)^2 / var times var and carry
    fp32 roundings of their own size, so the relative error of var, and half of it in rstd, is A times
    a two-pass formula's: rstd is a common factor of ``rstd (acc - mean colsum)``, so this adds
    (A - 1) |rstd (acc - mean colsum)|.  d carries a relative rounding, so the mean an absolute one of
    |c - mean| 2^-24, which adds rstd |c - mean| |colsum|.  Two-pass routes and RMSNorm (c = 0, nothing
    subtracted): None."""
    if rms or form == "two_pass":
        return None
    st = stats_of(x64, False, eps)
    c = x64[:, 0] if form == "one_pass" else st.partials[:, 0, 0]
    return torch.stack([1.0 + (c - st.mean) ** 2 / (st.var + eps), (c - st.mean).abs()], -1)


def terms(fx: NormFixture, rms: bool, eps: float = EPS, bias: bool = True, res: bool = True, act=None,
          form: str = "two_pass", device=None) -> Terms:
    f = fold64(fx, rms, bias)
    st = stats64(fx, rms, eps)
    t = Terms(fx.x.double() @ f.w.t(), st.mean, st.rstd, f.colsum, f.bias, fx.res.double() if res else None,
              None if act in (None, "none") else act, condition(fx.x.double(), form, rms, eps))
    return t if device is None else t.to(device)


def truth_of(t: Terms) -> torch.Tensor:
    y = t.rstd[:, None] * (t.acc - t.mean[:, None] * t.colsum[None, :]) + t.bias[None, :]
    if t.act == "relu":
        y = torch.relu(y)
    elif t.act is not None:
        raise ValueError(t.act)
    if t.res is not None:
        y = y + t.res
    return y + 0.0


def magnitude_of(t: Terms) -> torch.Tensor:
    s = (t.rstd[:, None] * t.acc).abs() + (t.rstd * t.mean)[:, None].abs() * t.colsum[None, :].abs()
    if t.cond is not None:
        core = t.rstd[:, None] * (t.acc - t.mean[:, None] * t.colsum[None, :])
        s = s + (t.cond[:, :1] - 1.0) * core.abs() + (t.rstd * t.cond[:, 1])[:, None] * t.colsum[None, :].abs()
    s = s + t.bias[None, :].abs()
    return s if t.res is None else s + t.res.abs()


def truth64(fx, rms, eps=EPS, bias=True, res=True, act=None) -> torch.Tensor:
    return truth_of(terms(fx, rms, eps, bias, res, act))


def magnitude(fx, rms, eps=EPS, bias=True, res=True, act=None, form="two_pass") -> torch.Tensor:
    return magnitude_of(terms(fx, rms, eps, bias, res, act, form))


def _ulp(y64: torch.Tensor, fmt) -> torch.Tensor:
    """The spacing of the format's grid at ``y64``, from the fp64 exponent bits alone (no pow, exp2 or
    ldexp, which need not be exact on every device)."""
    bits, emin = fmt
    e = ((y64.abs().view(torch.int64) >> 52) & 0x7FF) - 1023  # floor(log2 |y|); zero and fp64 subnormals: -1023
    return ((e.clamp(min=emin) - (bits - 1) + 1023) << 52).view(torch.float64)


def round_to(y64: torch.Tensor, fmt=BF16_FMT) -> torch.Tensor:
    """``y64`` rounded once to nearest-even on the format's grid (fp64 in, fp64 out; no overflow handling)."""
    u = _ulp(y64, fmt)
    return torch.round(y64 / u) * u


def boundary_distance(y64: torch.Tensor, fmt=BF16_FMT) -> torch.Tensor:
    """The distance of ``y64`` from the nearest rounding boundary (midpoint of two neighbouring values)
    of bf16 (``BF16_FMT``) or e4m3 (``E4M3_FMT``)."""
    bits, emin = fmt
    u = _ulp(y64, fmt)
    t = y64.abs() / u
    k = torch.floor(t)
    f = t - k
    d = (f - 0.5).abs()
    low = (k == 2 ** (bits - 1)) & (u > 2.0 ** (emin - bits + 1))  # first value of a binade: the ulp below is half
    d = torch.where(low, torch.minimum(d, f + 0.25), d)
    return d * u


def mask_of(t: Terms, tau: float = TAU, fmt=BF16_FMT) -> torch.Tensor:
    """True where the element is left out: ``y64`` within ``tau S`` of a rounding boundary.  With ReLU the
    boundary that matters below zero is zero itself: a pre-activation below ``-tau S`` is cut to exactly
    0 on the device as in fp64 (the output is the residual, or +0: compared), one within ``tau S`` of 0
    may fall on either side (left out)."""
    S = magnitude_of(t)
    m = boundary_distance(truth_of(t), fmt) < tau * S
    if t.act == "relu":
        pre = truth_of(t.with_(act=None, res=None))
        band = tau * magnitude_of(t.with_(res=None))
        m = (m & ~(pre < -band)) | (pre.abs() <= band)
    return m


def mask(fx, tau=TAU, rms=False, eps=EPS, bias=True, res=True, act=None, form="two_pass") -> torch.Tensor:
    return mask_of(terms(fx, rms, eps, bias, res, act, form), tau)


def want_bf16(y64: torch.Tensor) -> torch.Tensor:
    r = round_to(y64)
    w = r.to(torch.bfloat16)
    assert torch.equal(w.double(), r), "the rounded fp64 value is no bf16 value"
    return w


def compare(got: torch.Tensor, y64: torch.Tensor, S: torch.Tensor, tau: float, what: str = "", masked=None):
    """``got`` (bf16) equals ``bf16(y64)`` at every element outside the band (``masked``, by default
    the elements within ``tau S`` of a rounding boundary).  Returns (compared, masked)."""
    want = want_bf16(y64)
    if masked is None:
        masked = boundary_distance(y64) < tau * S
    bad = ~(got == want) & ~masked  # a NaN differs from everything
    if bool(bad.any()):
        idx = bad.nonzero()
        i = tuple(idx[0].tolist())
        rows = sorted(set(idx[:, 0].tolist()))
        dist = (boundary_distance(y64)[i] / S[i]).item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ outside the band, in "
                             f"{len(rows)} rows (first rows {rows[:8]}); first at {i}: got {got[i].item()!r}, want "
                             f"{want[i].item()!r} (y64 = {y64[i].item()!r}), boundary distance / S = 2^"
                             f"{math.log2(max(dist, 1e-300)):.1f} against tau = 2^{math.log2(tau):.0f}")
    assert not bool(masked.all(1).any()), f"{what}: a row is fully masked"
    if got.shape[0] >= 16:  # a column of fewer rows is a handful of elements: M = 1 would forbid any masked element
        assert not bool(masked.all(0).any()), f"{what}: a column is fully masked"
    return got.numel() - int(masked.sum()), int(masked.sum())


def assert_rounded(buf: torch.Tensor, M: int, N: int, t: Terms, tau: float = TAU, what: str = ""):
    """``buf[:M, :N]`` against ``t`` through the mask, and everything around it still NaN (the buffers of
    ``gemm_exact.nan_buffer``).  Returns (compared, masked)."""
    r = compare(buf[:M, :N], truth_of(t), magnitude_of(t), tau, what, mask_of(t, tau))
    assert bool(buf[M:].isnan().all()) and bool(buf[:M, N:].isnan().all()), f"{what}: written outside (M, N)"
    return r


# ----------------------------------------------------------------------------- the fp32 mirrors
def _f32(t):
    return t.to(torch.float32)


def acc32(fx: NormFixture, rms: bool) -> torch.Tensor:
    """acc = x . W'^T in fp32, asserted exact."""
    f = fold64(fx, rms)
    a64 = fx.x.double() @ f.w.t()
    a = _f32(a64)
    assert torch.equal(a.double(), a64)
    return a


def _seq_sum(t: torch.Tensor) -> torch.Tensor:
    """Sum over the last dim, one element after the other: a fixed order, whatever the host's vector width."""
    s = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for i in range(t.shape[-1]):
        s = s + t[..., i]
    return s


def _wave_sum(t: torch.Tensor) -> torch.Tensor:
    """(M, K) -> (M,) in the order of norm_kernel: lane l adds its 8-element fragments l, l + 64, ... one
    element after the other, then a butterfly over the 64 lanes."""
    M, K = t.shape
    nc = -(-K // 512)
    lanes = _seq_sum(torch.nn.functional.pad(t, (0, 512 * nc - K)).view(M, nc, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, nc * 8))
    o = 32
    while o:
        lanes = lanes[:, :o] + lanes[:, o:2 * o]
        o //= 2
    return lanes[:, 0]


def _rsqrt(v: torch.Tensor) -> torch.Tensor:
    return 1.0 / torch.sqrt(v)


def stats_two_pass(x: torch.Tensor, rms: bool, eps: float = EPS, drop_last: bool = False, unshifted: bool = False):
    """(mean, rstd) fp32 as norm_kernel / row_stats_kernel compute them.  Faults: ``drop_last`` leaves
    the row's last element out of the variance; ``unshifted`` is E[x^2] - mean^2 in fp32."""
    K = x.shape[1]
    mean = torch.zeros(x.shape[0]) if rms else x.sum(1) / K
    if unshifted:
        var = (_wave_sum(x * x) / K - mean * mean).clamp(min=0)
    else:
        d = x - mean[:, None]
        if drop_last:
            d = d[:, :-1]
        var = _wave_sum(d * d) / K
    return mean, _rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def stats_one_pass(x: torch.Tensor, rms: bool, eps: float = EPS, drop_last: bool = False):
    """(mean, rstd) fp32 as sk_stats and the decode epilogues compute them."""
    K = x.shape[1]
    c = torch.zeros(x.shape[0]) if rms else x[:, 0].clone()
    d = x - c[:, None]
    s1 = torch.zeros(x.shape[0]) if rms else d.sum(1)
    dd = d[:, :-1] if drop_last else d
    s2 = (dd * dd).sum(1)
    invk = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    e = s1 * invk
    var = s2 * invk if rms else (s2 * invk - e * e).clamp(min=0)
    return (c + e), _rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def partials32(x: torch.Tensor) -> torch.Tensor:
    """epi_rowstat16 in fp32: (M, P, 2) {mean, M2} of each 16-column tile."""
    M, K = x.shape
    P = -(-K // 16)
    xp = torch.nn.functional.pad(x, (0, 16 * P - K)).view(M, P, 16)
    cnt = torch.full((P,), 16.0)
    cnt[-1] = K - 16 * (P - 1)
    pm = xp.sum(-1) / cnt
    valid = (torch.arange(16 * P) < K).view(P, 16)
    dv = (xp - pm[..., None]) * valid
    return torch.stack([pm, _seq_sum(dv * dv)], -1)


def _strided_sum(t: torch.Tensor, tpr: int) -> torch.Tensor:
    """(M, P) -> (M,): lane s of ``tpr`` adds elements s, s + tpr, ... in turn, then a butterfly."""
    M, P = t.shape
    n = -(-P // tpr)
    lanes = _seq_sum(torch.nn.functional.pad(t, (0, n * tpr - P)).view(M, n, tpr).transpose(1, 2))
    o = tpr // 2
    while o:
        lanes = lanes[:, :o] + lanes[:, o:2 * o]
        o //= 2
    return lanes[:, 0]


def stats_partials(p: torch.Tensor, K: int, rms: bool, eps: float = EPS, tpr: int = 8):
    """rowstat_merge in fp32 on the (M, P, 2) partials ``p``, ``tpr`` lanes per row (the one-shot
    kernel: 256 / rows of the workgroup; 8 for its 32-row tile)."""
    P = p.shape[1]
    n = torch.full((P,), 16.0)
    n[-1] = K - 16 * (P - 1)
    c = torch.zeros(p.shape[0]) if rms else p[:, 0, 0].clone()
    d = p[..., 0] - c[:, None]
    s1, s2, sm = _strided_sum(n * d, tpr), _strided_sum(n * d * d, tpr), _strided_sum(p[..., 1], tpr)
    invk = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    var = (sm + s2) * invk if rms else ((sm + s2 - s1 * s1 * invk) * invk).clamp(min=0)
    mean = torch.zeros(p.shape[0]) if rms else c + s1 * invk
    return mean, _rsqrt(var + torch.tensor(eps, dtype=torch.float32))


def epilogue32(acc, mean, rstd, colsum, bias, res, act, form: str) -> torch.Tensor:
    """The fp32 epilogue -> bf16.  ``form``: "rowstat" = acc rstd + (-mean rstd) colsum (epi_norm4),
    "decode" = rstd (acc - mean colsum) (the skinny, stream, one-shot and head kernels)."""
    if form == "rowstat":
        v = acc * rstd[:, None] + (-mean * rstd)[:, None] * colsum[None, :]
    else:
        v = rstd[:, None] * (acc - mean[:, None] * colsum[None, :])
    v = v + bias[None, :]
    if act == "relu":
        v = torch.relu(v)
    if res is not None:
        v = v + res
    return v.to(torch.bfloat16)


MIRRORS = ("two_pass", "one_pass", "partials")


def mirror(fx: NormFixture, which: str, rms: bool, eps: float = EPS, bias=True, res=True, act=None, stats=None,
           colsum=None, fbias=None) -> torch.Tensor:
    """The bf16 output of mirror ``which``.  ``stats`` / ``colsum`` / ``fbias`` override the mirror's
    own (mean, rstd), column sums and folded bias: how the sensitivity test injects its faults."""
    f = fold64(fx, rms, bias)
    with ge._one_thread():
        if stats is None:
            if which == "two_pass":
                stats = stats_two_pass(fx.x, rms, eps)
            elif which == "one_pass":
                stats = stats_one_pass(fx.x, rms, eps)
            else:
                stats = stats_partials(partials32(fx.x), fx.x.shape[1], rms, eps)
        cs = _f32(f.colsum) if colsum is None else colsum
        b = _f32(f.bias) if fbias is None else fbias
        return epilogue32(acc32(fx, rms), stats[0], stats[1], cs, b, fx.res if res else None, act,
                          "rowstat" if which == "two_pass" else "decode")


def need_of(got: torch.Tensor, y64: torch.Tensor, S: torch.Tensor, rows=None) -> float:
    """The largest boundary distance / S over the elements of ``got`` that differ from bf16(y64) (0 if none)."""
    bad = ~(got == want_bf16(y64))
    if rows is not None:
        keep = torch.zeros_like(bad)
        keep[rows] = True
        bad &= keep
    if not bool(bad.any()):
        return 0.0
    return float((boundary_distance(y64)[bad] / S[bad]).max())


# ----------------------------------------------------------------------------- plain norm
def plain_terms(x64, gamma64, beta64, rms: bool, eps: float = EPS):
    """(y64, S) of the plain norm ``(x - mean) rstd gamma + beta``.  S = NC |(x - mean) rstd gamma| +
    |mean rstd gamma| + |beta|: as in the folded form, the mean's own rounding (2^-24 |mean|) enters
    every element at the size of the mean, whatever is left of x - mean.  An element that equals its
    row's mean exactly (every element of a zero row; a whole-number mean) has S = 0: the sum of whole
    numbers and the correctly rounded division give that mean in fp32 too, x - mean is exactly zero and
    the output is beta itself, rounded once; it is always compared."""
    st = stats_of(x64, rms, eps)
    core = (x64 - st.mean[:, None]) * st.rstd[:, None] * gamma64[None, :]
    # the variance is summed by each lane over its NC = ceil(N / 512) fragments one element after the other:
    # the roundings accumulate along that chain, so rstd's relative error, which multiplies x - mean, grows with NC
    nc = -(-x64.shape[1] // 512)
    S = nc * core.abs() + (st.mean * st.rstd)[:, None].abs() * gamma64[None, :].abs()
    y = core
    if beta64 is not None and not rms:
        y, S = core + beta64[None, :], S + beta64[None, :].abs()
    return y + 0.0, torch.where(x64 == st.mean[:, None], torch.zeros_like(S), S)


@functools.lru_cache(maxsize=None)
def _plain_tables(N: int):
    """gamma (+-[0.5, 2), any fp32 value) and beta (whole numbers / 64, sigma 0.5) of the plain-norm
    fixtures, as fp64.  The plain norm has no sum over gamma to keep exact, and values off a grid keep a
    row of few distinct whole numbers from landing in the band all at once; beta is a bf16 value, so an
    output that is beta plus next to nothing (zero elements of a row with a small mean) lies half an ulp
    from the boundaries and a column does not go into the band for all such rows together."""
    g = torch.Generator().manual_seed(9100)
    gam = (0.5 + 1.5 * torch.rand(K_MAX, generator=g)) * (1 - 2 * torch.randint(0, 2, (K_MAX,), generator=g).float())
    bet = (32 * torch.randn(K_MAX, generator=g)).round().clamp(-127, 127) / 64
    return gam[:N].double(), bet[:N].double()


def plain_case(N: int, variant: str):
    """(x, gamma, beta, y64, S) of the plain-norm fixture at width N: ``PLAIN_ROWS`` class rows;
    ``variant`` in ln_beta / ln / rms."""
    x = activations(N, plain=True)[:PLAIN_ROWS]
    gamma, beta = _plain_tables(N)
    beta = beta if variant == "ln_beta" else None
    y64, S = plain_terms(x.double(), gamma, beta, variant == "rms")
    return x, gamma, beta, y64, S


def rowstat_mirror_error(x: torch.Tensor, rms: bool) -> float:
    """The fp32 two-pass mirror's worst relative error in {rstd, -mean rstd} against fp64 (entries that
    are zero in fp64 must be zero and are left out)."""
    st = stats_of(x.double(), rms)
    with ge._one_thread():
        mean, rstd = stats_two_pass(x, rms)
    got = torch.stack([rstd, -mean * rstd], -1).double()
    err = (got - st.rowstat).abs() / st.rowstat.abs().clamp(min=1e-300)
    return float(err[st.rowstat != 0].max())


def mirror_plain(x, gamma, beta, rms: bool, eps: float = EPS) -> torch.Tensor:
    with ge._one_thread():
        mean, rstd = stats_two_pass(x, rms, eps)
    v = (x - mean[:, None]) * rstd[:, None] * gamma[None, :]
    if beta is not None and not rms:
        v = v + beta[None, :]
    return v.to(torch.bfloat16)


# ----------------------------------------------------------------------------- the folded layer, as the kernels get it
def folded(fx: NormFixture, rms: bool, device, bias: bool = True):
    """The ``FoldedLinear`` of ``fx``.  bf16: through the real ``ops.gemm.fold_norm``.  w8: the e4m3 bytes
    of W diag(gamma) with the fixture's power-of-two channel scales, and the bias and column sums by
    ``fold_norm``'s own formulas on the dequantised weight."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, kpad_of
    from distributed_neural_networks_amd.ops.gemm import NORM_LN, NORM_RMS, FoldedLinear, fold_norm
    b = fx.bias if bias else None
    if fx.wfmt == "bf16":
        return fold_norm(fx.w, fx.gamma, None if rms else fx.beta, b, rms, EPS, device)
    N, K = fx.w.shape
    qf = (fx.w * fx.gamma[None, :]).to(device)
    q8 = qf.to(torch.float8_e4m3fn)
    assert torch.equal(q8.float(), qf), "W diag(gamma) does not round-trip through e4m3"
    q = torch.zeros((N, kpad_of(K)), dtype=torch.uint8, device=device)
    q[:, :K] = q8.view(torch.uint8)
    sw = fx.sw.to(device).contiguous()
    wdq = q8.float() * sw[:, None]
    fb = None if b is None else b.to(device)
    if not rms:
        wb = (fx.w.to(device) * sw[:, None]) @ fx.beta.to(device)
        fb = wb if fb is None else wb + fb
    return FoldedLinear(Fp8Weight(q.view(torch.float8_e4m3fn), sw, K), None if fb is None else fb.contiguous(),
                        None if rms else wdq.sum(1).contiguous(), NORM_RMS if rms else NORM_LN, EPS)


def assert_fold_exact(f, fx: NormFixture, rms: bool, bias: bool = True) -> None:
    """``f`` (``folded``) holds the fp64 fold exactly: weight, bias and column sums."""
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight
    g = fold64(fx, rms, bias)
    K = fx.w.shape[1]
    if isinstance(f.w, Fp8Weight):
        assert torch.equal(f.w.q[:, :K].double().cpu(), g.q) and torch.equal(f.w.scale.double().cpu(), fx.sw.double())
        assert not bool(f.w.q[:, K:].float().any())
    else:
        assert f.w.dtype == torch.bfloat16 and torch.equal(f.w.double().cpu(), g.w)
    if f.bias is None:
        assert not bool(g.bias.any())
    else:
        assert f.bias.dtype == torch.float32 and torch.equal(f.bias.double().cpu(), g.bias)
    if rms:
        assert f.colsum is None
    else:
        assert f.colsum.dtype == torch.float32 and torch.equal(f.colsum.double().cpu(), g.colsum)
