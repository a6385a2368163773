"""Exact-arithmetic fixtures for the uint8 input of the fp32 CIFAR stage 0 (helper module, no tests).

``cifar_exact`` places images and weights on power-of-two grids so that the fp64 stage, cast to
fp32, is the bit-exact expected output of the kernels in any summation order.  With uint8 input
the image values are whatever the normalisation table holds, so the table is drawn from the very
values the fixture's images take: every looked-up pixel is then one of the fixture's own values,
the preconditions of ``cifar_exact`` (which depend on the value set and the weights only) carry
over, and the weights, biases and units are the fixture's unchanged.

``u8_fixture(name)`` for ``name`` in ``cifar_exact.NAMES``:

1. ``vals``: the distinct values of ``fixture(name, 257).x``;
2. a generator seeded with ``4242 + NAMES.index(name)``;
3. per channel 256 table entries from ``vals``: a ``randperm`` prefix where there are at least
   256 values, else ``randint`` with repetition, so the table is not monotone in the byte;
4. ``(257,32,32,3)`` random bytes;
5. ``x = normalize_u8(bytes, table)``, with the fixture's weights and units.

``tests/test_cifar_u8_input.py`` asserts the preconditions on the CPU;
``tests/test_cifar_u8_input_gpu.py`` holds the kernel to ``u8_reference``.
"""
import functools
from dataclasses import dataclass

import torch

import cifar_exact as ce

SEED0 = 4242


@dataclass(frozen=True)
class U8Fixture:
    fx: ce.Fixture        # the fixture's weights and units, x = normalize_u8(u8, table)
    u8: torch.Tensor      # (B,32,32,3) uint8
    table: torch.Tensor   # (3,256) fp32


@functools.lru_cache(maxsize=None)
def _build(name: str) -> U8Fixture:
    from distributed_neural_networks_amd.ops.cifar import normalize_u8
    base = ce.fixture(name, ce.B_MAX)
    vals = base.x.unique()
    g = torch.Generator().manual_seed(SEED0 + ce.NAMES.index(name))
    rows = []
    for _ in range(3):
        if vals.numel() >= 256:
            idx = torch.randperm(vals.numel(), generator=g)[:256]
        else:
            idx = torch.randint(0, vals.numel(), (256,), generator=g)
        rows.append(vals[idx])
    table = torch.stack(rows).contiguous()
    u8 = torch.randint(0, 256, (ce.B_MAX, 32, 32, 3), dtype=torch.uint8, generator=g)
    x = normalize_u8(u8, table)
    return U8Fixture(ce.Fixture(base.name, base.sd, x, base.u1, base.u), u8, table)


def u8_fixture(name: str, B: int = ce.B_MAX) -> U8Fixture:
    """The uint8 fixture ``name`` at its first ``B`` images (generated once at 257)."""
    if not 1 <= B <= ce.B_MAX:
        raise ValueError(f"B must be in 1..{ce.B_MAX}")
    f = _build(name)
    return U8Fixture(ce.Fixture(f.fx.name, f.fx.sd, f.fx.x[:B], f.fx.u1, f.fx.u), f.u8[:B], f.table)


@functools.lru_cache(maxsize=None)
def u8_reference(name: str) -> torch.Tensor:
    """The bit-exact expected fp32 boundary of ``u8_fixture(name)`` at 257 images (computed once;
    rows [:B] hold for every smaller batch).  Do not modify."""
    ref64 = ce.reference64(_build(name).fx)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), "the fp64 reference does not round-trip through fp32"
    return ref
