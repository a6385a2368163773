"""Exact-arithmetic fixtures for the fp32 CIFAR kernels: stage 0 first, the head tail and the
fused fc1 further down (helper module, no tests).

The fp32 kernels compute every layer as ``a_hi*w_hi + a_hi*w_lo + a_lo*w_hi`` on
bf16 MFMAs with fp32 accumulation.  With inputs and weights on power-of-two
grids, every product and every partial sum is exactly representable in fp32, so
the result is the same in every summation order and the fp64 torch stage, cast
to fp32, is the bit-exact expected output.  Let ``u`` be the
product of the two operands' grid steps of a layer; the layer is exact if

  (i)   each operand equals its ``split_bf16`` ``hi + lo`` exactly,
  (ii)  one of the two operands is bf16-exact (``lo == 0``, so the dropped
        ``a_lo*w_lo`` term is exactly zero),
  (iii) ``max(conv(|a|, |w|) + |b|) / u < 2^24`` (the fixtures stay below 2^22),
  (iv)  conv1's pooled output is below 2^16 units, so it passes through the
        kernel's hi/lo planes unchanged.

Four fixtures, so that each ``lo`` term meets a dense layer (``m`` = random
integers in [-m, m]):

  fixture    x            conv1               b1           conv2              exercises
  c1_xwide   511 * 2^-7   w 4 * 2^-2 dense    64 * 2^-9    selector           conv1 x_lo * w_hi
  c1_wwide   8 * 2^-1     w 511 * 2^-9 dense  64 * 2^-10   selector           conv1 x_hi * w_lo
  c2_awide   511 * 2^-7   pass-through        255 * 2^-7   w 8 * 2^-3 dense   conv2 a_lo * w_hi
  c2_wwide   12 * 2^-2    pass-through        3 * 2^-2     w 511 * 2^-9 dense conv2 a_hi * w_lo

Selector conv2: each output channel has one nonzero weight, +1 or -1, at a random
(c, ky, kx).  Pass-through conv1: output channel o has weight 1 at
(c = o % 3, ky = 1, kx = 1).  b2 lies on conv2's grid; channels with a -1 weight
get a bias large enough to survive the ReLU.

``tests/test_cifar_exact.py`` asserts (i)-(iv) and the order independence on the
CPU; ``tests/test_cifar_stage0_exact_gpu.py`` holds the kernels to the reference.
"""
import contextlib
import functools
from dataclasses import dataclass
from typing import Dict

import torch
import torch.nn.functional as F

NAMES = ("c1_xwide", "c1_wwide", "c2_awide", "c2_wwide")
SEED = 0
B_MAX = 257  # the largest batch any test uses; smaller batches are its first images


@dataclass(frozen=True)
class Fixture:
    name: str
    sd: Dict[str, torch.Tensor]  # conv1.weight, conv1.bias, conv2.weight, conv2.bias (fp32)
    x: torch.Tensor              # (B,3,32,32) fp32
    u1: float                    # conv1's unit: x grid step * conv1.weight grid step
    u: float                     # conv2's unit (the output's grid step): u1 * conv2.weight grid step


def _ints(g, m, shape):
    return torch.randint(-m, m + 1, shape, generator=g).double()


def _selector(g):
    w = torch.zeros(64, 32, 3, 3, dtype=torch.float64)
    c = torch.randint(0, 32, (64,), generator=g)
    ky = torch.randint(0, 3, (64,), generator=g)
    kx = torch.randint(0, 3, (64,), generator=g)
    sign = torch.randint(0, 2, (64,), generator=g).double() * 2 - 1
    w[torch.arange(64), c, ky, kx] = sign
    return w, sign


def _passthrough():
    w = torch.zeros(32, 3, 3, 3, dtype=torch.float64)
    o = torch.arange(32)
    w[o, o % 3, 1, 1] = 1.0
    return w


def _selector_bias(g, sign, s):
    """b2 in conv2 units: +1 channels get [-3s, 0] (about half of their outputs survive the
    ReLU), -1 channels [s/2, 3s] (large enough that most of theirs do)."""
    pos = -torch.randint(0, 3 * s + 1, (64,), generator=g).double()
    neg = torch.randint(s // 2, 3 * s + 1, (64,), generator=g).double()
    return torch.where(sign > 0, pos, neg)


@functools.lru_cache(maxsize=None)
def _build(name: str, seed: int) -> Fixture:
    """The fixture at B_MAX images (generated once; every smaller batch is a prefix)."""
    g = torch.Generator().manual_seed(1000 * seed + NAMES.index(name))
    B = B_MAX
    if name == "c1_xwide":
        x = _ints(g, 511, (B, 3, 32, 32)) * 2.0**-7
        w1 = _ints(g, 4, (32, 3, 3, 3)) * 2.0**-2
        u1 = 2.0**-9
        b1 = _ints(g, 64, (32,)) * u1
        w2, sign = _selector(g)
        u = u1
        b2 = _selector_bias(g, sign, 4096) * u
    elif name == "c1_wwide":
        x = _ints(g, 8, (B, 3, 32, 32)) * 2.0**-1
        w1 = _ints(g, 511, (32, 3, 3, 3)) * 2.0**-9
        u1 = 2.0**-10
        b1 = _ints(g, 64, (32,)) * u1
        w2, sign = _selector(g)
        u = u1
        b2 = _selector_bias(g, sign, 8192) * u
    elif name == "c2_awide":
        x = _ints(g, 511, (B, 3, 32, 32)) * 2.0**-7
        w1 = _passthrough()
        u1 = 2.0**-7
        b1 = _ints(g, 255, (32,)) * u1
        w2 = _ints(g, 8, (64, 32, 3, 3)) * 2.0**-3
        u = u1 * 2.0**-3
        b2 = (_ints(g, 8192, (64,)) - 16384) * u
    elif name == "c2_wwide":
        x = _ints(g, 12, (B, 3, 32, 32)) * 2.0**-2
        w1 = _passthrough()
        u1 = 2.0**-2
        b1 = _ints(g, 3, (32,)) * u1
        w2 = _ints(g, 511, (64, 32, 3, 3)) * 2.0**-9
        u = u1 * 2.0**-9
        b2 = (_ints(g, 8192, (64,)) - 24576) * u
    else:
        raise KeyError(name)
    sd = {"conv1.weight": w1.float(), "conv1.bias": b1.float(), "conv2.weight": w2.float(), "conv2.bias": b2.float()}
    for k, v64 in (("conv1.weight", w1), ("conv1.bias", b1), ("conv2.weight", w2), ("conv2.bias", b2)):
        assert torch.equal(sd[k].double(), v64), k  # the grids are exact in fp32
    assert torch.equal(x.float().double(), x)
    return Fixture(name, sd, x.float(), u1, u)


def fixture(name: str, B: int = 3, seed: int = SEED) -> Fixture:
    """State-dict entries, ``B`` images and the units of fixture ``name``.  The images of a
    batch all differ; the first ``B`` of the ``B_MAX`` generated, so a reference computed
    for a larger batch holds for every smaller one."""
    if not 1 <= B <= B_MAX:
        raise ValueError(f"B must be in 1..{B_MAX}")
    fx = _build(name, seed)
    return Fixture(fx.name, fx.sd, fx.x[:B], fx.u1, fx.u)


def conv1_pooled64(fx: Fixture) -> torch.Tensor:
    """Unit 0 in fp64: (B,32,16,16), conv2's activation operand."""
    sd = fx.sd
    return F.max_pool2d(F.relu(F.conv2d(fx.x.double(), sd["conv1.weight"].double(), sd["conv1.bias"].double(),
                                        padding=1)), 2, 2)


def reference64(fx: Fixture) -> torch.Tensor:
    """Units 0-1 (``CifarStage(0, 1)``) in fp64: (B,4096), NCHW flatten.  ``+ 0.0`` makes
    every zero a positive zero, as the ReLU of the kernels gives."""
    sd = fx.sd
    a = conv1_pooled64(fx)
    y = F.max_pool2d(F.relu(F.conv2d(a, sd["conv2.weight"].double(), sd["conv2.bias"].double(), padding=1)), 2, 2)
    return y.reshape(-1, 4096) + 0.0


@functools.lru_cache(maxsize=None)
def reference(name: str, seed: int = SEED) -> torch.Tensor:
    """The bit-exact expected fp32 boundary of fixture ``name`` at B_MAX images (computed once;
    rows [:B] are the expected output of ``fixture(name, B)``).  Do not modify."""
    fx = fixture(name, B_MAX, seed)
    ref64 = reference64(fx)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), "the fp64 reference does not round-trip through fp32"
    return ref


def units(t: torch.Tensor, u: float) -> torch.Tensor:
    """``t / u`` in fp64, asserted to be whole numbers."""
    n = t.double() / u
    assert torch.equal(n, n.round()), "values off the grid"
    return n


def magnitude_bounds(fx: Fixture):
    """(max(conv(|x|,|w1|) + |b1|) / u1, max(conv(|a|,|w2|) + |b2|) / u): precondition (iii)."""
    sd = fx.sd
    m1 = F.conv2d(fx.x.double().abs(), sd["conv1.weight"].double().abs(), sd["conv1.bias"].double().abs(), padding=1)
    m2 = F.conv2d(conv1_pooled64(fx), sd["conv2.weight"].double().abs(), sd["conv2.bias"].double().abs(), padding=1)
    return m1.max().item() / fx.u1, m2.max().item() / fx.u


def split_bf16(t: torch.Tensor):
    """hi = bf16(t), lo = bf16(t - hi), as ``ops.cifar.split_bf16`` and the kernels' split2."""
    t = t.float()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return hi.float(), lo.float()


@contextlib.contextmanager
def _one_thread():
    """The emulations are thousands of small element-wise steps: one thread runs them in a
    second or two, where a thread pool on a busy machine spends its time waiting."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _x3_conv_fp32(a: torch.Tensor, w: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """3x3 pad-1 convolution as the kernels' three-term split, every product and every
    addition rounded to fp32, summed tap by tap in ``order`` (a permutation of C*9)."""
    B, C, H, W = a.shape
    O = w.shape[0]
    ah, al = split_bf16(a)
    wh, wl = split_bf16(w)
    ch, cl = F.unfold(ah, 3, padding=1), F.unfold(al, 3, padding=1)  # (B, C*9, H*W), k = c*9 + ky*3 + kx
    wh, wl = wh.reshape(O, C * 9), wl.reshape(O, C * 9)
    acc = torch.zeros(B, O, H * W, dtype=torch.float32)
    with _one_thread():
        for k in order.tolist():
            acc = acc + ch[:, k:k + 1, :] * wh[None, :, k:k + 1]
            acc = acc + ch[:, k:k + 1, :] * wl[None, :, k:k + 1]
            acc = acc + cl[:, k:k + 1, :] * wh[None, :, k:k + 1]
    return acc.reshape(B, O, H, W)


def emulate_x3_fp32(fx: Fixture, order_seed=None) -> torch.Tensor:
    """Units 0-1 as the fp32 kernels compute them, in fp32 throughout: three bf16-term
    products per tap, bias after the accumulation, ReLU, pool, conv1's pooled map through
    its hi/lo split.  ``order_seed`` None: taps in their natural order; else a random order."""
    sd = fx.sd

    def order(n, salt):
        if order_seed is None:
            return torch.arange(n)
        return torch.randperm(n, generator=torch.Generator().manual_seed(order_seed + salt))

    c1 = _x3_conv_fp32(fx.x, sd["conv1.weight"], order(27, 0)) + sd["conv1.bias"].view(1, -1, 1, 1)
    a = F.max_pool2d(F.relu(c1), 2, 2)
    c2 = _x3_conv_fp32(a, sd["conv2.weight"], order(288, 1)) + sd["conv2.bias"].view(1, -1, 1, 1)
    return F.max_pool2d(F.relu(c2), 2, 2).reshape(-1, 4096) + 0.0


# ---------------------------------------------------------------------------
# Head tail (fc2 + softmax + argmax): exact logits.  K = 512 costs 9 bits, so
# with hid on a grid (non-negative, about a quarter exact zeros, as after ReLU)
# and fc2 on a grid, sum(|hid||w|) + |b| stays below 2^22 units and the logits
# are exact in fp32 in any order; what the kernels add is the softmax's own
# rounding.  fc2 rows 3 and 7 are identical, bias included, and so are rows 0
# and 9: their logits tie exactly in every image.
#
#   fixture    precision   hid              fc2.weight     fc2.bias       u
#   hid_wide   fp32        0..511 * 2^-7    8 * 2^-3       16384 * 2^-10  2^-10
#   w_wide     fp32        0..15 * 2^-2     511 * 2^-9     32768 * 2^-11  2^-11
#   bf16       bf16        0..255 * 2^-6    8 * 2^-3       8192 * 2^-9    2^-9
#
# Worst cases by construction: 512*511*8 + 16384, 512*15*511 + 32768 and
# 512*255*8 + 8192 units, all below 2^22.  Each class's weights sum to zero
# (hid is non-negative: otherwise one class wins every row).  The logits have a
# standard deviation of about 28; every 8th row is loud, with a gap above 104
# between two of its logits, so its smallest probabilities underflow to 0.
# ---------------------------------------------------------------------------
HEAD_NAMES = ("hid_wide", "w_wide", "bf16")
HEAD_B_MAX = 300
_HEAD = {  # name: (precision, hid max int, hid step, weight max int, weight step, bias max int)
    "hid_wide": ("fp32", 511, 2.0**-7, 8, 2.0**-3, 16384),
    "w_wide": ("fp32", 15, 2.0**-2, 511, 2.0**-9, 32768),
    "bf16": ("bf16", 255, 2.0**-6, 8, 2.0**-3, 8192),
}


@dataclass(frozen=True)
class HeadFixture:
    name: str
    precision: str
    sd: Dict[str, torch.Tensor]  # fc2.weight (10,512), fc2.bias (10,) fp32
    hid: torch.Tensor            # (B,512) fp32 values (bf16-exact for the bf16 precision)
    u: float                     # the logits' grid step
    bound_units: float           # worst case of sum(|hid||w|) + |b| in units, by construction


@functools.lru_cache(maxsize=None)
def _build_head(name: str, seed: int) -> HeadFixture:
    precision, hm, hs, wm, ws, bm = _HEAD[name]
    g = torch.Generator().manual_seed(1000 * seed + 100 + HEAD_NAMES.index(name))
    hid = torch.randint(0, hm + 1, (HEAD_B_MAX, 512), generator=g).double()
    hid = hid * (torch.rand((HEAD_B_MAX, 512), generator=g) >= 0.25)  # a quarter exact zeros
    w = _ints(g, wm, (10, 512))
    # hid >= 0, so a class whose weights do not sum to zero wins or loses every row: centre each class
    w = (w - w.mean(dim=1, keepdim=True).round()).clamp(-wm, wm)
    for c in range(10):
        r = int(w[c].sum().item())
        step = 1.0 if r > 0 else -1.0
        ok = ((w[c] - step).abs() <= wm).nonzero().flatten()
        w[c, ok[torch.randperm(ok.numel(), generator=g)[:abs(r)]]] -= step
        assert w[c].sum().item() == 0
    b = _ints(g, bm, (10,))
    b[0], b[3] = b[0].abs(), b[3].abs()  # the tied classes are the row maximum often enough to matter
    # every 8th row (row 0 included) is loud: nonzero only where class a's weight exceeds class b's, so
    # the gap between the two logits passes 104 and the smaller probabilities underflow to exactly 0
    for i in range(0, HEAD_B_MAX, 8):
        a, c = torch.tensor([0, 1, 2, 3, 4, 5, 6, 8])[torch.randperm(8, generator=g)[:2]].tolist()  # untied classes
        hid[i] = torch.where(w[a] > w[c], hid[i], torch.zeros(()).double())
    w[7], b[7] = w[3], b[3]
    w[9], b[9] = w[0], b[0]
    u = hs * ws
    sd = {"fc2.weight": (w * ws).float(), "fc2.bias": (b * u).float()}
    assert torch.equal(sd["fc2.weight"].double(), w * ws) and torch.equal(sd["fc2.bias"].double(), b * u)
    return HeadFixture(name, precision, sd, (hid * hs).float(), u, 512.0 * hm * wm + bm)


def head_fixture(name: str, B: int = HEAD_B_MAX, seed: int = SEED) -> HeadFixture:
    """fc2 state-dict entries and ``B`` hidden rows (the first B of HEAD_B_MAX) of fixture ``name``."""
    if not 1 <= B <= HEAD_B_MAX:
        raise ValueError(f"B must be in 1..{HEAD_B_MAX}")
    fx = _build_head(name, seed)
    return HeadFixture(fx.name, fx.precision, fx.sd, fx.hid[:B], fx.u, fx.bound_units)


def head_logits64(fx: HeadFixture) -> torch.Tensor:
    """fc2 in fp64: (B,10), exact."""
    return fx.hid.double() @ fx.sd["fc2.weight"].double().t() + fx.sd["fc2.bias"].double()


def first_argmax(logits: torch.Tensor) -> torch.Tensor:
    """Per row, the smallest class index attaining the maximum."""
    n = logits.shape[1]
    at_max = logits == logits.max(dim=1, keepdim=True).values
    return torch.where(at_max, torch.arange(n), torch.tensor(n)).min(dim=1).values


def emulate_head_logits_fp32(fx: HeadFixture, order_seed=None) -> torch.Tensor:
    """The logits as the head kernels accumulate them, in fp32 throughout: per k the three
    bf16-term products (fp32 precision) or the one bf16 product (bf16), then the bias."""
    order = (torch.arange(512) if order_seed is None
             else torch.randperm(512, generator=torch.Generator().manual_seed(order_seed)))
    hh, hl = split_bf16(fx.hid)
    wh, wl = split_bf16(fx.sd["fc2.weight"])
    acc = torch.zeros(fx.hid.shape[0], 10, dtype=torch.float32)
    with _one_thread():
        for k in order.tolist():
            acc = acc + hh[:, k:k + 1] * wh[None, :, k]
            if fx.precision == "fp32":
                acc = acc + hh[:, k:k + 1] * wl[None, :, k]
                acc = acc + hl[:, k:k + 1] * wh[None, :, k]
    return acc + fx.sd["fc2.bias"]


# ---------------------------------------------------------------------------
# Fused fc1 (relu(A . W^T + b), K = 4096): exact outputs.  K = 4096 costs 12
# bits, so the narrow operand is five values wide; the wide one carries 10 bits
# and so a nonzero lo half.  Every product and partial sum is a whole number of
# units below 2^24, so relu(A . W^T + b) in fp64, cast to fp32, is the expected
# output bit for bit in any summation order.
#
#   fixture   A                W               b               u       exercises
#   a_wide    511 * 2^-7       2 * 2^-1        32768 * 2^-8    2^-8    a_lo * w_hi
#   w_wide    2 * 2^-1         511 * 2^-9      32768 * 2^-10   2^-10   a_hi * w_lo
#
# Worst case by construction: 4096*511*2 + 32768 units, below 2^23.  The bias is
# of the size of the sums (standard deviation about 27000 units at K = 4096), so
# that the sign under the ReLU depends on the product, not on the bias alone.
# Every smaller shape is a prefix: rows [:M] of A, rows [:N] of W and of b,
# columns [:K] of both.
# ---------------------------------------------------------------------------
FC1_NAMES = ("a_wide", "w_wide")
FC1_M_MAX, FC1_N, FC1_K = 300, 512, 4096
_FC1 = {  # name: (A max int, A step, W max int, W step, bias max int)
    "a_wide": (511, 2.0**-7, 2, 2.0**-1, 32768),
    "w_wide": (2, 2.0**-1, 511, 2.0**-9, 32768),
}


@dataclass(frozen=True)
class Fc1Fixture:
    name: str
    a: torch.Tensor     # (M,K) fp32
    w: torch.Tensor     # (N,K) fp32
    b: torch.Tensor     # (N,) fp32, on the product grid
    u: float            # the outputs' grid step
    bound_units: float  # worst case of sum(|a||w|) + |b| in units, by construction


@functools.lru_cache(maxsize=None)
def _build_fc1(name: str, seed: int) -> Fc1Fixture:
    am, astep, wm, wstep, bm = _FC1[name]
    g = torch.Generator().manual_seed(1000 * seed + 200 + FC1_NAMES.index(name))
    a = _ints(g, am, (FC1_M_MAX, FC1_K)) * astep
    w = _ints(g, wm, (FC1_N, FC1_K)) * wstep
    u = astep * wstep
    b = _ints(g, bm, (FC1_N,)) * u
    for t in (a, w, b):
        assert torch.equal(t.float().double(), t)  # the grids are exact in fp32
    return Fc1Fixture(name, a.float(), w.float(), b.float(), u, float(FC1_K * am * wm + bm))


def fc1_fixture(name: str, M: int = FC1_M_MAX, N: int = FC1_N, K: int = FC1_K, seed: int = SEED) -> Fc1Fixture:
    """Fixture ``name`` cut to (M, N, K): the first rows and columns of the one generated."""
    if not (1 <= M <= FC1_M_MAX and 1 <= N <= FC1_N and 1 <= K <= FC1_K):
        raise ValueError(f"shape must be within {(FC1_M_MAX, FC1_N, FC1_K)}")
    fx = _build_fc1(name, seed)
    return Fc1Fixture(fx.name, fx.a[:M, :K], fx.w[:N, :K], fx.b[:N], fx.u, fx.bound_units)


def fc1_reference64(fx: Fc1Fixture) -> torch.Tensor:
    """relu(A . W^T + b) in fp64: (M,N), exact.  ``+ 0.0`` makes every zero a positive zero."""
    return torch.relu(fx.a.double() @ fx.w.double().t() + fx.b.double()) + 0.0


def emulate_fc1_fp32(fx: Fc1Fixture, order_seed=None) -> torch.Tensor:
    """fc1 as the fused kernel accumulates it, in fp32 throughout: per k the three bf16-term
    products, then bias and ReLU.  ``order_seed`` None: k in its natural order; else a random order."""
    K = fx.a.shape[1]
    order = (torch.arange(K) if order_seed is None
             else torch.randperm(K, generator=torch.Generator().manual_seed(order_seed)))
    ah, al = split_bf16(fx.a)
    wh, wl = split_bf16(fx.w)
    acc = torch.zeros(fx.a.shape[0], fx.w.shape[0], dtype=torch.float32)
    with _one_thread():
        for k in order.tolist():
            acc = acc + ah[:, k:k + 1] * wh[None, :, k]
            acc = acc + ah[:, k:k + 1] * wl[None, :, k]
            acc = acc + al[:, k:k + 1] * wh[None, :, k]
    return torch.relu(acc + fx.b) + 0.0
