"""The exact-arithmetic GEMM fixtures of tests/gemm_exact.py, checked on the CPU:
the preconditions of that module on the data itself (storage round-trip,
magnitudes below 2^24 units, ``thin`` outputs exact in bf16, smaller shapes are
prefixes), an fp32 emulation of the kernels' chunked and split-K accumulation
equal to the fp64 reference bit for bit in every order, ``shuffle_weight`` as a
pure permutation, and the sensitivity of a ``thin`` output to one product.

Seed 0 gives, in each element's own units (the cap is 2^24 = 16777216):

  fixture                      shape               max sum |a||w| + |b| + |r|   worst case by construction
  dense                        (300, 2320, 4096)   297069                       962496
  dense  w8 + a8               (512, 1600, 1664)   251477                       520832
  thin   (largest |output|)    (33, 4112, 8192)    202 of 256
"""
import pytest
import torch

import gemm_exact as ge

FORMATS = [("dense", "bf16", "bf16"), ("thin", "bf16", "bf16"), ("dense", "w8", "bf16"), ("thin", "w8", "bf16"),
           ("dense", "w8", "a8"), ("thin", "w8", "a8")]
SHAPE = (70, 300, 1664)  # odd sizes, a K that is 26 chunks of 64: the emulations run in a second


@pytest.fixture(params=FORMATS, ids=["-".join(f) for f in FORMATS])
def fx(request):
    kind, wfmt, afmt = request.param
    return ge.fixture(kind, *SHAPE, wfmt=wfmt, afmt=afmt)


def test_operands_round_trip_through_their_storage(fx):
    """bf16 or e4m3 operands, fp32 scales and bias, bf16 residual: all unchanged by the cast
    (``fixture`` asserts it while building; here once more from the outside), scales powers of two."""
    f8 = torch.float8_e4m3fn
    assert torch.equal(fx.a.to(f8 if fx.afmt == "a8" else torch.bfloat16).float(), fx.a)
    assert torch.equal(fx.w.to(f8 if fx.wfmt == "w8" else torch.bfloat16).float(), fx.w)
    assert torch.equal(fx.res.to(torch.bfloat16).float(), fx.res)
    for s in (fx.sa, fx.sw):
        if s is not None:
            assert torch.equal(torch.exp2(torch.log2(s).round()), s) and s.unique().numel() == 3
    assert fx.a.abs().max().item() * (8 if fx.kind == "dense" and fx.afmt == "bf16" else 1) == ge._AMAX[fx.kind]
    assert ge.FP8_INT_MAX == 15


def test_magnitudes_leave_headroom(fx):
    """sum |a||w| + |bias| + |res| in each element's units: on the data below the bound by
    construction, that below 2^24; every output on its element's grid."""
    mag = ge.magnitude_units(fx)
    y = ge.reference64(fx)
    n = y / ge.unit_grid(fx)
    assert torch.equal(n, n.round())
    print(f"{fx.kind} {fx.wfmt} {fx.afmt}: {mag:.0f} units (worst case {fx.bound_units:.0f})")
    assert mag <= fx.bound_units < 2**24
    assert y.unique().numel() >= 200  # not a constant map


@pytest.mark.parametrize("kind", ge.KINDS)
def test_bounds_at_the_largest_shapes(kind):
    """The worst case by construction at the deepest K and with both scales stays below 2^21
    (dense) and the thin outputs of the largest shapes the GPU tests use stay below 256."""
    for K, wfmt, afmt in ((8192, "bf16", "bf16"), (8192, "w8", "bf16"), (8192, "w8", "a8")):
        assert ge.fixture(kind, 1, 16, K, wfmt, afmt).bound_units < 2**21
    if kind == "thin":
        for shape in ((33, 4112, 8192), (300, 2320, 4096)):
            f = ge.fixture(kind, *shape)
            y = ge.reference64(f)
            print(f"thin {shape}: largest |output| {y.abs().max().item():.0f}")
            assert y.abs().max().item() < 256
            ge.expected(y, torch.bfloat16, exact=True)


def test_expected_outputs(fx):
    """fp32 outputs equal the fp64 reference; bf16 outputs of ``thin`` equal it too; bf16 outputs
    of ``dense`` are its one rounding, with real ties in it (a truncating or double-rounding
    epilogue would show) and no trivial agreement."""
    for act in (None, "relu"):
        y = ge.reference64(fx, act)
        assert torch.equal(ge.expected(y, torch.float32, False).double(), y)
        e = ge.expected(y, torch.bfloat16, exact=fx.kind == "thin")
        if fx.kind == "dense":
            inexact = (e.double() != y)
            assert inexact.double().mean().item() > (0.3 if act else 0.6)  # under the ReLU about half are the residual alone
            ulp = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(1e-30))) - 7)
            ties = ((y - e.double()).abs() == ulp / 2).double().mean().item()
            print(f"{fx.kind} {fx.wfmt} {fx.afmt} {act}: {100 * ties:.1f} % exact ties")
            assert ties > 0.005
    assert (ge.reference64(fx, "relu", res=False) == 0).double().mean().item() > 0.2  # the ReLU cuts


def test_smaller_shapes_are_prefixes():
    for kind, wfmt, afmt in FORMATS:
        big = ge.fixture(kind, 130, 520, 512, wfmt, afmt)
        small = ge.fixture(kind, 17, 100, 192, wfmt, afmt)
        assert torch.equal(small.a, big.a[:17, :192]) and torch.equal(small.w, big.w[:100, :192])
        assert torch.equal(small.bias, big.bias[:100]) and torch.equal(small.res, big.res[:17, :100])
        if big.sa is not None:
            assert torch.equal(small.sa, big.sa[:17])
        if big.sw is not None:
            assert torch.equal(small.sw, big.sw[:100])
        assert small.u == big.u
        # a reference at a larger M and N holds for the smaller ones at the same K
        full = ge.reference64(ge.fixture(kind, 130, 520, 192, wfmt, afmt))
        assert torch.equal(ge.reference64(small), full[:17, :100])


def test_accumulation_is_order_independent(fx):
    """A . W^T accumulated in fp32 in 64-wide k-chunks: natural order, two random orders, and
    split into 2, 3 and 7 partial slabs added afterwards.  Each equals the fp64 product."""
    want = ge.reference64(fx, bias=False, res=False)
    assert torch.equal(want.float().double(), want)
    want = want.float()
    for order_seed, slabs in ((None, 1), (5, 1), (6, 1), (None, 2), (7, 3), (None, 7)):
        emu = ge.accumulate_fp32(fx, order_seed, slabs)
        assert emu.dtype == torch.float32
        assert torch.equal(emu, want), (order_seed, slabs)


@pytest.mark.parametrize("N", [16, 100, 2306])
@pytest.mark.parametrize("fmt", ["bf16", "e4m3"])
def test_shuffle_weight_is_a_permutation_with_zero_padding(N, fmt):
    """``shuffle_weight`` inverted by index arithmetic from its documented layout: the original
    rows come back, the pad rows are zero, nothing else is in the buffer."""
    from distributed_neural_networks_amd.ops.gemm import shuffle_weight
    K = 192
    f = ge.fixture("dense", 1, N, K, "w8" if fmt == "e4m3" else "bf16")
    w = f.w.to(torch.float8_e4m3fn if fmt == "e4m3" else torch.bfloat16)
    raw = w.view(torch.uint8).reshape(N, -1)
    sh = shuffle_weight(w)
    Np = -(-N // 16) * 16
    assert sh.dtype == torch.uint8 and sh.dim() == 1 and sh.numel() == Np * raw.shape[1]
    idx = ge.unshuffle_index(N, raw.shape[1])
    assert idx.unique().numel() == sh.numel()  # a bijection onto the buffer
    back = sh[idx]
    assert torch.equal(back[:N], raw)
    assert int(back[N:].to(torch.int32).abs().sum()) == 0
    assert len(raw.unique()) > 8  # not a constant table


def test_codes_fixture_is_exhaustive():
    """Every finite e4m3 byte meets every one-hot row (bf16 rows), and every byte is an activation
    too (a8 rows); the outputs are exact in bf16 (asserted in ``codes_reference64``)."""
    codes = ge.finite_codes()
    assert codes.numel() == 254 and bool(torch.isfinite(codes.view(torch.float8_e4m3fn).float()).all())
    v = codes.view(torch.float8_e4m3fn).float()
    assert v.abs().max().item() == 448 and v[v != 0].abs().min().item() == 2.0**-9
    for M in (1, 16, 17, 64):
        c = ge.codes_fixture(M)
        sel = c.wq[:, c.k_of_m]  # (N, M): the byte each output reads
        for m in range(M):
            assert sel[:, m].unique().numel() == 254
        assert (c.a != 0).sum(1).eq(1).all()
        ge.codes_reference64(c)
    c = ge.codes_fixture(ge.CODES_M_MAX, a8=True)
    assert c.a.to(torch.float8_e4m3fn).view(torch.uint8)[torch.arange(300), c.k_of_m].unique().numel() >= 253  # -0 = +0 as a value
    y = ge.codes_reference64(c)
    assert y.abs().max().item() > 1000 and y[y != 0].abs().min().item() < 1e-5


def test_one_product_changes_a_thin_output():
    """Sensitivity: every nonzero product of ``thin`` is +1 or -1 element units, every output a
    whole number n with |n| < 256, and n - 1, n, n + 1 are three different bf16 values: removing
    (or duplicating) any one nonzero product changes the bf16 output."""
    for wfmt, afmt in (("bf16", "bf16"), ("w8", "bf16"), ("w8", "a8")):
        f = ge.fixture("thin", 64, 520, 4096, wfmt, afmt)
        assert set(f.a.unique().tolist()) == {-1.0, 0.0, 1.0} == set(f.w.unique().tolist())
        assert 0.2 < (f.a != 0).float().mean().item() < 0.3 and 0.2 < (f.w != 0).float().mean().item() < 0.3
        g = ge.unit_grid(f)
        y = ge.reference64(f)
        n = y / g
        assert torch.equal(n, n.round()) and n.abs().max().item() < 256
        e = ge.expected(y, torch.bfloat16, exact=True)
        for d in (-1.0, 1.0):
            other = ((n + d) * g).to(torch.bfloat16)
            assert torch.equal(other.double(), (n + d) * g)
            assert bool((other != e).all())
