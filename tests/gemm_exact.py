"""Exact-arithmetic fixtures for the transformer GEMMs (helper module, no tests).

Every GEMM route here accumulates products of bf16 or e4m3 operands in fp32 and
differs from the next route only in tiling and summation order.  With operands
that are whole numbers times powers of two, every product and every partial sum
is a whole number of units ``u`` below 2^24, so it is exact in fp32 in any
order, any split-K and any workgroup reduction; power-of-two channel and row
scales, the bias and the residual keep it exact.  ``A . W^T (+ bias) -> act
(+ residual)`` in fp64 is then the expected output: bit for bit for fp32
outputs, and after one round-to-nearest-even for bf16 outputs.  Any difference
from it is a bug, located to the element.

  fixture   A                              W                              bias                  residual               output unit
  dense     ints [-15,15] * 2^-3, bf16     ints [-15,15] * 2^-4, bf16     ints [-2^15,2^15] u   ints [-127,127] 64 u   u = 2^-7
  thin      {-1,0,1}, a quarter nonzero    {-1,0,1}, a quarter nonzero    ints [-64,64]         ints [-64,64]          u = 1
  w8        as dense or thin (bf16)        e4m3 bytes holding the same    on the column's grid  dense: on the          per column
                                           ints; scale_n = 2^-(3 + n % 3)                       coarsest column grid;
                                                                                                thin: the element's
  a8w8      e4m3 bytes holding the ints;   as w8                          on the column's grid  as w8                  per (row, column)
            row scale 2^-(2 + m % 3)                                      at the coarsest row
  w8_codes  one-hot rows: +-2^j at k(m)    all 254 finite e4m3 codes      none                  none                   bf16-exact
            (a8w8: an e4m3 code at k(m))   (subnormals, +-0, +-448)

``dense``: full-width products.  The fp32 output is exact; the bf16 output is
the fp64 value rounded once, so it checks the rounding mode and double
rounding (a few percent of the outputs are exact ties).  ``thin``: every output
is a whole number below 256 in magnitude times a power of two, so the **bf16**
output is exact too, and one lost, duplicated or mis-paired product changes
it: for the routes that only write bf16.  ``w8`` / ``a8w8`` reuse the integer
tables of ``dense`` / ``thin``: ints up to 15 are exact in e4m3, power-of-two
scales are exact, and a scale that varies with n (m) catches a mis-indexed
scale; the ``Fp8Weight`` is built from (q, scale, k) directly, since
``quantize_weight``'s absmax / 448 is no power of two.  ``w8_codes``: the
in-register e4m3 -> bf16 conversion and the fp8 MFMA's operand decoding,
exhaustively: output[m, n] = W[n, k(m)] * scale_n * A[m, k(m)].

Worst cases by construction (``bound_units``, in units of the element's own
grid step, which is what the fp32 accumulator and epilogue hold): K * 15 * 15 +
the bias + the residual; ``dense`` at K = 8192
is 8192 * 225 + 2^15 + 127 * 64 < 2^21, with both scales 8192 * 225 + 2^12 * 4 +
127 * 64 * 16 < 2^21.  On the data, ``dense`` at (300, 2320, 4096) peaks at
about 3.0e5 units (2^18.2) of sum |a||w| + |bias| + |residual|, ``thin`` at the
same shape at an output of 191, and at (33, 4112, 8192) of 202, against the
limit of 256.

Every fixture is generated once at (M_MAX, N_MAX, K_MAX); each smaller
(M, N, K) is a prefix: the first rows and columns.  Operands are asserted to
round-trip through their storage type (bf16, e4m3 or fp32).

fp8 MFMA operand width.  tests/test_cifar_stage0_exact_gpu.py established that
the bf16 MFMA sums grid operands exactly; for the fp8 MFMA the smallest a8w8
cases (one tile, K = 128: the 128^2 kernel, the 256^2 kernel and the fp8 arm of
the skinny kernel) and for the scaled fp8 MFMA of the MX path the smallest case
it takes (256, 256, 128) were run first, ahead of the fp8 groups
(``test_fp8_mfma_sums_exactly`` and ``test_mx[smallest]``).  Both instructions
sum operands of the full width, ints in [-15, 15], exactly on the MI355X: no
narrowing to [-7, 7] or [-3, 3] was needed.  FP8_INT_MAX below records it.

``tests/test_gemm_exact.py`` asserts the preconditions and the order
independence on the CPU; ``tests/test_gemm_exact_gpu.py`` (decode routes) and
``tests/test_gemm_exact_prefill_gpu.py`` (tile kernels, fp8, MX) hold the
kernels to the reference.
"""
import contextlib
import functools
from dataclasses import dataclass
from typing import Optional

import torch

KINDS = ("dense", "thin")
SEED = 0
M_MAX, N_MAX, K_MAX = 512, 16400, 8192  # the generated shape; every smaller shape is a prefix
FP8_INT_MAX = 15  # the operand width at which the fp8 MFMAs sum exactly (see the docstring)

_AMAX = {"dense": 15, "thin": 1}
_BMAX = {"dense": 2**15, "thin": 64}
_RMAX = {"dense": 127, "thin": 64}


@dataclass(frozen=True)
class Fixture:
    kind: str                    # dense / thin
    wfmt: str                    # bf16 / w8 (e4m3 bytes + channel scale)
    afmt: str                    # bf16 / a8 (e4m3 bytes + row scale)
    a: torch.Tensor              # (M,K) fp32: the stored operand values (a8: the e4m3 values before the row scale)
    sa: Optional[torch.Tensor]   # (M,) fp32 row scales, a8 only
    w: torch.Tensor              # (N,K) fp32: the stored operand values (w8: the e4m3 values before the channel scale)
    sw: Optional[torch.Tensor]   # (N,) fp32 channel scales, w8 only
    bias: torch.Tensor           # (N,) fp32
    res: torch.Tensor            # (M,N) fp32, bf16-exact
    u: float                     # the finest output grid step (``unit_grid``: each element's own)
    bound_units: float           # worst case of sum |a||w| + |bias| + |res| in the element's own units, by construction


@contextlib.contextmanager
def _one_thread():
    """The emulations are hundreds of small steps: one thread runs them in a second or two,
    where a thread pool on a busy machine spends its time waiting."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _tables(kind: str, seed: int):
    """The integer tables of ``kind`` at the generated shape (int8 / int32, made once)."""
    g = torch.Generator().manual_seed(1000 * seed + 300 + KINDS.index(kind))

    def ints(m, shape, dtype=torch.int8):
        return torch.randint(-m, m + 1, shape, generator=g, dtype=dtype)

    def sparse(shape):  # {-1, 0, 1}, a quarter nonzero
        t = torch.randint(0, 8, shape, generator=g, dtype=torch.int8)
        return (t == 1).to(torch.int8) - (t == 0).to(torch.int8)

    if kind == "dense":
        ai, wi = ints(15, (M_MAX, K_MAX)), ints(15, (N_MAX, K_MAX))
    elif kind == "thin":
        ai, wi = sparse((M_MAX, K_MAX)), sparse((N_MAX, K_MAX))
    else:
        raise KeyError(kind)
    bi = ints(_BMAX[kind], (N_MAX,), torch.int32)
    ri = ints(_RMAX[kind], (M_MAX, N_MAX))
    return ai, wi, bi, ri


def _roundtrip(t64: torch.Tensor, dtype) -> torch.Tensor:
    """``t64`` as fp32, asserted to survive its storage type unchanged."""
    assert torch.equal(t64.to(dtype).double(), t64), f"values do not round-trip through {dtype}"
    return t64.float()


def fixture(kind: str, M: int, N: int, K: int, wfmt: str = "bf16", afmt: str = "bf16", seed: int = SEED) -> Fixture:
    """Fixture ``kind`` cut to (M, N, K) with bf16 or e4m3 (``w8``) weights and bf16 or e4m3
    (``a8``) activations.  ``A = a * sa[:, None]`` and ``W = w * sw[:, None]`` are the operand
    values (scales of 1 where None)."""
    if not (1 <= M <= M_MAX and 1 <= N <= N_MAX and 1 <= K <= K_MAX):
        raise ValueError(f"shape must be within {(M_MAX, N_MAX, K_MAX)}")
    if wfmt not in ("bf16", "w8") or afmt not in ("bf16", "a8") or (afmt == "a8" and wfmt != "w8"):
        raise ValueError((wfmt, afmt))
    ai, wi, bi, ri = _tables(kind, seed)
    ai, wi, bi, ri = ai[:M, :K].double(), wi[:N, :K].double(), bi[:N].double(), ri[:M, :N].double()
    dense, w8, a8 = kind == "dense", wfmt == "w8", afmt == "a8"
    step_a = 2.0**-3 if dense and not a8 else 1.0
    step_w = 2.0**-4 if dense and not w8 else 1.0
    sa = 2.0 ** -(2 + torch.arange(M) % 3).double() if a8 else None
    sw = 2.0 ** -(3 + torch.arange(N) % 3).double() if w8 else None
    sa_max, sa_min = (2.0**-2, 2.0**-4) if a8 else (1.0, 1.0)
    sw_max, sw_min = (2.0**-3, 2.0**-5) if w8 else (1.0, 1.0)
    col = step_a * step_w * sa_max * (sw if w8 else torch.ones(N, dtype=torch.float64))  # (N,) the column's grid
    if a8:
        bi = (bi / (8 if dense else 4)).trunc()  # the coarsest row's grid is 4 of the finest row's units
    bias = bi * col
    if dense:
        res = ri * (64 * step_a * step_w * sa_max * sw_max)  # one grid for the whole matrix: the coarsest column's
    else:
        res = ri * col[None, :] * ((sa / sa_max)[:, None] if a8 else 1.0)  # the element's own unit
    u = step_a * step_w * sa_min * sw_min
    ratio = (sa_max / sa_min) * (sw_max / sw_min)
    bmax = _BMAX[kind] / ((8 if dense else 4) if a8 else 1)
    bound = K * _AMAX[kind] ** 2 + bmax * (sa_max / sa_min) + _RMAX[kind] * (64 * ratio if dense else 1)
    f8 = torch.float8_e4m3fn
    return Fixture(kind, wfmt, afmt,
                   _roundtrip(ai * step_a, f8 if a8 else torch.bfloat16), None if sa is None else sa.float(),
                   _roundtrip(wi * step_w, f8 if w8 else torch.bfloat16), None if sw is None else sw.float(),
                   _roundtrip(bias, torch.float32), _roundtrip(res, torch.bfloat16), u, float(bound))


def operands64(fx: Fixture, device=None):
    """(A, W) in fp64 with their scales applied."""
    a, w = fx.a.to(device).double(), fx.w.to(device).double()
    if fx.sa is not None:
        a = a * fx.sa.to(device).double()[:, None]
    if fx.sw is not None:
        w = w * fx.sw.to(device).double()[:, None]
    return a, w


def epilogue64(prod: torch.Tensor, fx: Fixture, act=None, bias: bool = True, res: bool = True) -> torch.Tensor:
    """``prod (+ bias) -> act (+ residual)`` in fp64, on ``prod``'s device; ``+ 0.0`` makes every
    zero a positive zero."""
    y = prod
    if bias:
        y = y + fx.bias.to(y.device).double()
    if act == "relu":
        y = torch.relu(y)
    elif act not in (None, "none"):
        raise ValueError(act)
    if res:
        y = y + fx.res.to(y.device).double()
    return y + 0.0


def reference64(fx: Fixture, act=None, bias: bool = True, res: bool = True, device=None) -> torch.Tensor:
    """The GEMM in fp64: exact (every term is a whole number of units far below 2^53)."""
    a, w = operands64(fx, device)
    return epilogue64(a @ w.t(), fx, act, bias, res)


def expected(y64: torch.Tensor, dtype, exact: bool) -> torch.Tensor:
    """The expected output tensor for the fp64 result ``y64``: fp32 outputs (asserted exact), or
    bf16 outputs as its one round-to-nearest-even; ``exact`` (``thin``): asserted exact too."""
    y32 = y64.float()
    assert torch.equal(y32.double(), y64), "the fp64 reference does not round-trip through fp32"
    if dtype == torch.float32:
        return y32
    e = y32.to(torch.bfloat16)  # fp32 -> bf16 is one rounding to nearest-even, and y32 == y64
    if exact:
        assert torch.equal(e.double(), y64), "a thin output is not exact in bf16"
    return e


def unit_grid(fx: Fixture) -> torch.Tensor:
    """(M,N) fp64: the grid step of each output element, ``u`` times the element's row and
    channel scales relative to the smallest ones."""
    g = torch.full((fx.a.shape[0], fx.w.shape[0]), fx.u, dtype=torch.float64)
    if fx.sa is not None:
        g = g * (fx.sa.double() / 2.0**-4)[:, None]
    if fx.sw is not None:
        g = g * (fx.sw.double() / 2.0**-5)[None, :]
    return g


def magnitude_units(fx: Fixture) -> float:
    """max(sum |a||w| + |bias| + |res|) in each element's own units, on the data: what the fp32
    accumulator and epilogue must hold exactly, below ``bound_units``."""
    a, w = operands64(fx)
    return ((a.abs() @ w.abs().t() + fx.bias.double().abs() + fx.res.double().abs()) / unit_grid(fx)).max().item()


def units(t: torch.Tensor, u: float) -> torch.Tensor:
    """``t / u`` in fp64, asserted to be whole numbers."""
    n = t.double() / u
    assert torch.equal(n, n.round()), "values off the grid"
    return n


def accumulate_fp32(fx: Fixture, order_seed=None, slabs: int = 1, chunk: int = 64) -> torch.Tensor:
    """A . W^T as the kernels accumulate it, in fp32 throughout: ``chunk``-wide k-chunks added one
    after the other, in natural order or (``order_seed``) a random one, dealt round-robin to
    ``slabs`` partial sums that are added at the end (split-K); scales applied after the sum."""
    K = fx.a.shape[1]
    nch = K // chunk
    assert nch * chunk == K
    order = (torch.arange(nch) if order_seed is None
             else torch.randperm(nch, generator=torch.Generator().manual_seed(order_seed)))
    part = [torch.zeros(fx.a.shape[0], fx.w.shape[0], dtype=torch.float32) for _ in range(slabs)]
    with _one_thread():
        for i, c in enumerate(order.tolist()):
            s = slice(c * chunk, (c + 1) * chunk)
            part[i % slabs] = part[i % slabs] + fx.a[:, s] @ fx.w[:, s].t()
        acc = part[0]
        for p in part[1:]:
            acc = acc + p
    if fx.sa is not None:
        acc = acc * fx.sa[:, None]
    if fx.sw is not None:
        acc = acc * fx.sw[None, :]
    return acc


# ---------------------------------------------------------------------------
# Codes: every finite e4m3 byte as a weight, selected by one-hot activation rows.
# W[n, k] = CODES[(k + 3 n) % 254] (3 and 254 are coprime: for a fixed k, 254
# consecutive rows n hold every code once); scale_n = 2^-(3 + n % 3); row m of A
# is zero except at k(m) = (29 m + 5) % K, where it holds (-1)^m 2^(m % 7 - 3)
# (bf16), or for the a8w8 variant the e4m3 code CODES[(5 m) % 254] with the row
# scale 2^-(2 + m % 3) (254 consecutive rows hold every code once).  A product
# of two e4m3 values has at most 8 significant bits and its exponent stays
# within bf16's normal range, so the bf16 output is exact.
# ---------------------------------------------------------------------------
CODES_N, CODES_K, CODES_M_MAX = 300, 256, 300


def finite_codes() -> torch.Tensor:
    """The 254 finite e4m3 bytes (0x7f and 0xff are the NaNs), as uint8."""
    b = torch.arange(256, dtype=torch.int32)
    return b[(b & 0x7F) != 0x7F].to(torch.uint8)


@dataclass(frozen=True)
class CodesFixture:
    a: torch.Tensor              # (M,K) fp32 one-hot rows (bf16-exact; a8: e4m3-exact values before the row scale)
    sa: Optional[torch.Tensor]   # (M,) fp32, a8 only
    wq: torch.Tensor             # (N,K) uint8 e4m3 bytes
    sw: torch.Tensor             # (N,) fp32
    k_of_m: torch.Tensor         # (M,) the selected column of each row


@functools.lru_cache(maxsize=None)
def codes_fixture(M: int, a8: bool = False) -> CodesFixture:
    if not 1 <= M <= CODES_M_MAX:
        raise ValueError(f"M must be in 1..{CODES_M_MAX}")
    codes = finite_codes()
    n, k, m = torch.arange(CODES_N), torch.arange(CODES_K), torch.arange(M)
    wq = codes[(k[None, :] + 3 * n[:, None]) % 254]
    sw = 2.0 ** -(3 + n % 3).float()
    km = (29 * m + 5) % CODES_K
    a = torch.zeros(M, CODES_K, dtype=torch.float32)
    if a8:
        a[m, km] = codes[(5 * m) % 254].view(torch.float8_e4m3fn).float()
        sa = 2.0 ** -(2 + m % 3).float()
    else:
        a[m, km] = (1.0 - 2.0 * (m % 2)) * 2.0 ** (m % 7 - 3).float()
        sa = None
        assert torch.equal(a.to(torch.bfloat16).float(), a)
    assert bool(torch.isfinite(wq.view(torch.float8_e4m3fn).float()).all())
    return CodesFixture(a, sa, wq, sw, km)


def codes_reference64(fx: CodesFixture) -> torch.Tensor:
    """output[m, n] = W[n, k(m)] scale_n A[m, k(m)] in fp64, asserted exact in bf16."""
    w = fx.wq.view(torch.float8_e4m3fn).double() * fx.sw.double()[:, None]
    a = fx.a.double() * (1.0 if fx.sa is None else fx.sa.double()[:, None])
    y = a @ w.t() + 0.0
    m = torch.arange(a.shape[0])
    assert torch.equal(y, (a[m, fx.k_of_m][:, None] * w[:, fx.k_of_m].t()) + 0.0)
    assert torch.equal(y.to(torch.bfloat16).double(), y), "a codes output is not exact in bf16"
    return y


def unshuffle_index(N: int, row_bytes: int) -> torch.Tensor:
    """(Np, row_bytes) flat byte offsets into ``ops.gemm.shuffle_weight``'s output, from its
    documented layout alone: column tile t = n // 16 and 64-B chunk c form one 1 KiB block,
    blocks of a tile consecutive along K; inside it lane 16 g + r holds row r = n % 16, bytes
    16 g .. 16 g + 15 of the chunk.  Np = N padded to a multiple of 16."""
    Np = -(-N // 16) * 16
    n = torch.arange(Np)[:, None]
    b = torch.arange(row_bytes)[None, :]
    t, r, c, g, j = n // 16, n % 16, b // 64, (b % 64) // 16, b % 16
    return (((t * (row_bytes // 64) + c) * 4 + g) * 16 + r) * 16 + j


# ---------------------------------------------------------------------------
# What the GPU tests share: operands and fp64 products on the device (made once
# per shape, never modified), NaN-guarded output buffers and the comparison.
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class DeviceCase:
    fx: Fixture
    a: torch.Tensor              # (M,K) bf16, or e4m3 (a8)
    sa: Optional[torch.Tensor]
    w: torch.Tensor              # (N,K) bf16, or e4m3 (w8)
    sw: Optional[torch.Tensor]
    bias: torch.Tensor           # (N,) fp32
    res: torch.Tensor            # (M,N) bf16
    prod64: torch.Tensor         # (M,N) fp64: A . W^T with the scales applied, computed on the device


@functools.lru_cache(maxsize=None)
def _device_case(kind, M, N, K, wfmt, afmt, device) -> DeviceCase:
    fx = fixture(kind, M, N, K, wfmt, afmt)
    f8 = torch.float8_e4m3fn
    a = fx.a.to(f8 if afmt == "a8" else torch.bfloat16).to(device)
    w = fx.w.to(f8 if wfmt == "w8" else torch.bfloat16).to(device)
    sa = None if fx.sa is None else fx.sa.to(device)
    sw = None if fx.sw is None else fx.sw.to(device)
    a64, w64 = a.double(), w.double()  # from the stored bytes: what the kernel reads
    if sa is not None:
        a64 = a64 * sa.double()[:, None]
    if sw is not None:
        w64 = w64 * sw.double()[:, None]
    return DeviceCase(fx, a, sa, w, sw, fx.bias.to(device), fx.res.to(torch.bfloat16).to(device), a64 @ w64.t())


def device_case(kind: str, M: int, N: int, K: int, wfmt: str = "bf16", afmt: str = "bf16", device="cuda",
                m_cap: int = 0) -> DeviceCase:
    """Fixture (kind, M, N, K) on the device with its fp64 product.  ``m_cap`` >= M: the case is made
    once at ``m_cap`` rows and cut to its first M (the prefix property), so the M values of one
    (N, K) share one product and one weight upload."""
    if m_cap <= M:
        return _device_case(kind, M, N, K, wfmt, afmt, str(device))
    c = _device_case(kind, m_cap, N, K, wfmt, afmt, str(device))
    f = c.fx
    fx = Fixture(f.kind, f.wfmt, f.afmt, f.a[:M], None if f.sa is None else f.sa[:M], f.w, f.sw, f.bias, f.res[:M], f.u,
                 f.bound_units)
    return DeviceCase(fx, c.a[:M], None if c.sa is None else c.sa[:M], c.w, c.sw, c.bias, c.res[:M], c.prod64[:M])


def want(case: DeviceCase, dtype, act=None, bias: bool = True, res: bool = True) -> torch.Tensor:
    """The expected output of ``case`` on its device."""
    return expected(epilogue64(case.prod64, case.fx, act, bias, res), dtype, exact=case.fx.kind == "thin")


def nan_buffer(M: int, N: int, dtype, device="cuda", ldc: Optional[int] = None, extra_rows: int = 3) -> torch.Tensor:
    """An output buffer taller and wider than (M, N), every element NaN.  ``ldc`` defaults to
    N + 8: as N modulo 8, so the epilogue's vector or scalar path is the one a contiguous (M, N)
    output would take."""
    return torch.full((M + extra_rows, N + 8 if ldc is None else ldc), float("nan"), dtype=dtype, device=device)


def assert_exact(buf: torch.Tensor, M: int, N: int, expect: torch.Tensor, what="") -> None:
    """``buf[:M, :N]`` equals ``expect`` by value (``torch.equal``: +0 and -0 alike, no NaN
    allowed) and everything around it is still NaN.  On a difference: the first differing
    (m, n), both values and the number of differing elements."""
    got = buf[:M, :N]
    if not torch.equal(got, expect):
        bad = ~(got == expect)  # a NaN differs from everything
        m, n = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {M * N} elements differ; first at (m, n) = ({m}, {n}): "
                             f"got {got[m, n].item()!r}, expected {expect[m, n].item()!r}")
    assert bool(buf[M:].isnan().all()) and bool(buf[:M, N:].isnan().all()), f"{what}: written outside (M, N)"
