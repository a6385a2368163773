"""Exact-arithmetic fc2 fixtures on top of ``cifar_exact.fc1_fixture`` for the fused fc1 + fc2
kernel (helper module, no tests).

``fc1_fixture`` gives relu(A . W^T + b) exactly, as whole numbers of units ``u``, up to about 2^17
of them at every K (the bias alone reaches 2^15).  The kernels split each hidden value into
``hh = bf16(hid)`` and ``hl = bf16(hid - hh)`` (whole units again; what is left after ``hl`` is
dropped, by the fused and the unfused path alike) and accumulate ``hh*wh + hh*wl + hl*wh`` per
class in fp32.  A class's sum is exact in every order if all its terms are multiples of one
quantum ``q`` and sum(|terms|) + |bias| < 2^24 q; classes never meet in a sum, so ``q`` is per
class.  With hidden values that large the budget allows only sparse fc2 rows:

  * narrow classes (0-5, 9): six weights of +-1 or +-2 times 2^-6 at random hidden columns
    (bf16-exact, ``wl == 0``; their columns carry hidden values that need ``hl``); q = u 2^-6;
  * wide classes (6, 8): one weight, 257 and -259 times 2^-14 (nine significant bits:
    ``wl != 0``), at the two columns whose largest hidden value is smallest; q = u 2^-14;
  * class 7 is class 3, bias included: their logits tie exactly in every row.

``exact_fc2`` asserts all of this in fp64 and returns the exact logits of the three terms.
"""
from dataclasses import dataclass

import torch

import cifar_exact as ce

NARROW, WIDE, TIED = (0, 1, 2, 3, 4, 5, 9), (6, 8), (3, 7)
WIDE_INTS = (257.0, -259.0)


@dataclass(frozen=True)
class ExactHead:
    fx: ce.Fc1Fixture
    w2: torch.Tensor      # (10,512) fp32
    b2: torch.Tensor      # (10,) fp32
    z64: torch.Tensor     # (M,10) fp64: hh.wh + hh.wl + hl.wh + b2, exact
    hid: torch.Tensor     # (M,512) fp32: the exact fc1 output
    sum_units: float      # max over rows and classes of (sum|terms| + |bias|) / q


def exact_fc2(name: str, M: int, K: int) -> ExactHead:
    fx = ce.fc1_fixture(name, M, 512, K)
    hid64 = ce.fc1_reference64(fx)
    hid = hid64.float()
    assert torch.equal(hid.double(), hid64)
    hu = ce.units(hid64, fx.u)
    g = torch.Generator().manual_seed(7000 + 10 * K + ce.FC1_NAMES.index(name))
    w = torch.zeros(10, 512, dtype=torch.float64)
    step = torch.full((10,), 2.0**-6, dtype=torch.float64)
    for c in NARROW:
        cols = torch.randperm(512, generator=g)[:6]
        w[c, cols] = (torch.randint(1, 3, (6,), generator=g) * (torch.randint(0, 2, (6,), generator=g) * 2 - 1)).double()
    cmax = hu.max(dim=0).values
    order = torch.argsort(torch.where(cmax > 0, cmax, torch.full_like(cmax, float("inf"))))
    for j, c in enumerate(WIDE):
        w[c, order[j]] = WIDE_INTS[j]
        step[c] = 2.0**-14
    w = w * step[:, None]
    b = torch.randint(-64, 65, (10,), generator=g).double() * 2.0**-4
    b[list(WIDE)] = torch.randint(-4, 5, (2,), generator=g).double() * 2.0**-8
    b[3] = b[3].abs() + 2.0  # the tied pair wins often enough to matter
    w[7], b[7] = w[3], b[3]
    q = fx.u * step

    hh, hl = ce.split_bf16(hid)
    wh, wl = ce.split_bf16(w.float())
    hh, hl, wh, wl = hh.double(), hl.double(), wh.double(), wl.double()
    assert torch.equal(w.float().double(), w) and torch.equal(wh + wl, w)
    # every term is a whole number of q: both factors are whole numbers of their steps
    ce.units(hh, fx.u), ce.units(hl, fx.u)
    for c in range(10):
        ce.units(wh[c], step[c].item()), ce.units(wl[c], step[c].item()), ce.units(b[c:c + 1], q[c].item())
    total = (hh.abs() @ wh.abs().t() + hh.abs() @ wl.abs().t() + hl.abs() @ wh.abs().t() + b.abs()) / q
    assert total.max().item() < 2.0**24, total.max().item()
    # both lo terms are exercised
    used = (w != 0).any(dim=0)
    assert bool((hl[:, used] != 0).any()), "no used hidden value needs hid_lo"
    for c in WIDE:
        assert bool((wl[c] != 0).any()) and bool(((hh @ wl[c]) != 0).any()), f"class {c}: the w_lo term is zero"
    for c in NARROW:
        assert not bool(wl[c].any())
    z = hh @ wh.t() + hh @ wl.t() + hl @ wh.t() + b
    assert torch.equal(z.float().double(), z)
    assert torch.equal(z[:, TIED[0]], z[:, TIED[1]])
    return ExactHead(fx, w.float(), b.float(), z, hid, total.max().item())
