"""The exact-arithmetic stage-0 fixtures of tests/cifar_exact.py, checked on the
CPU: preconditions (i)-(iv) of that module on the data itself, the fp64
reference through fp32 unchanged, an fp32 emulation of the kernels' three-term
split equal to it bit for bit in two summation orders, and enough nonzero and
distinct outputs that an all-zero or constant map cannot pass.

The caps are conditions on the fixtures, not measurements: a seed is kept only
if they hold.  Seed 0 at B = 3 gives (units of the layer's grid step)

  fixture    max conv(|x|,|w1|)+|b1|   max conv(|a|,|w2|)+|b2|   nonzero   distinct
  c1_xwide   29308                     27898                     64 %      4678
  c1_wwide   49294                     51127                     65 %      5200
  c2_awide   764                       569004                    47 %      5364
  c2_wwide   15                        751210                    39 %      4668

all below 2^22 = 4194304, conv1's below 2^16; the 257 images the GPU tests use
stay below 60000 and 850000 (asserted there on the data, once per fixture).

The head-tail and fused-fc1 fixtures of the same module follow, held to the
same preconditions.
"""
import pytest
import torch

import cifar_exact as ce

B = 3


@pytest.fixture(params=ce.NAMES)
def fx(request):
    return ce.fixture(request.param, B)


def _is_bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).float(), t.float())


def test_operands_equal_their_split(fx):
    """(i): x, both weights and conv1's pooled map are hi + lo of their bf16 split, exactly."""
    a = ce.conv1_pooled64(fx)
    assert torch.equal(a.float().double(), a)
    for what, t in (("x", fx.x), ("conv1.weight", fx.sd["conv1.weight"]), ("conv2.weight", fx.sd["conv2.weight"]),
                    ("conv1 pooled", a.float())):
        hi, lo = ce.split_bf16(t)
        assert torch.equal(hi.double() + lo.double(), t.double()), what


def test_one_operand_per_layer_is_bf16_exact(fx):
    """(ii): the dropped a_lo * w_lo term is exactly zero in both layers, and the wide operand
    the fixture is named after really has a nonzero lo plane."""
    x, w1, w2 = fx.x, fx.sd["conv1.weight"], fx.sd["conv2.weight"]
    a = ce.conv1_pooled64(fx).float()
    assert _is_bf16_exact(x) or _is_bf16_exact(w1)
    assert _is_bf16_exact(a) or _is_bf16_exact(w2)
    wide = {"c1_xwide": x, "c1_wwide": w1, "c2_awide": a, "c2_wwide": w2}[fx.name]
    lo = ce.split_bf16(wide)[1]
    assert (lo != 0).float().mean().item() > 0.25, "the lo plane under test is almost empty"
    if fx.name.startswith("c1"):
        assert not _is_bf16_exact(a)  # conv2's a_lo plane carries conv1's low bits to the output


def test_magnitudes_leave_headroom(fx):
    """(iii) and (iv), in units of each layer's grid step; every value on its grid."""
    m1, m2 = ce.magnitude_bounds(fx)
    a_units = ce.units(ce.conv1_pooled64(fx), fx.u1)
    ce.units(ce.reference64(fx), fx.u)
    print(f"{fx.name}: conv1 {m1:.0f} units, conv2 {m2:.0f} units, max pooled conv1 {a_units.max().item():.0f}")
    assert m1 < 2**16 and m2 < 2**22
    assert a_units.max().item() < 2**16


def test_reference_round_trips_and_is_order_independent(fx):
    """The fp64 stage survives the cast to fp32, and the fp32 three-term emulation equals it
    bit for bit with the taps in their natural order and in a random order."""
    ref64 = ce.reference64(fx)
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    assert torch.equal(ref, ce.reference(fx.name)[:B])
    for order_seed in (None, 7):
        emu = ce.emulate_x3_fp32(fx, order_seed)
        assert emu.dtype == torch.float32
        assert torch.equal(emu.view(torch.int32), ref.view(torch.int32)), (fx.name, order_seed)


def test_outputs_are_not_degenerate(fx):
    ref = ce.reference64(fx)
    nz = (ref != 0).double().mean().item()
    distinct = ref.unique().numel()
    print(f"{fx.name}: {100 * nz:.0f} % nonzero, {distinct} distinct values")
    assert 0.30 <= nz <= 0.90
    assert distinct >= 1000
    assert ref.unique(dim=0).shape[0] == B  # the images of a batch give different rows


def test_smaller_batches_are_prefixes():
    """The GPU tests slice one reference per fixture: fixture(name, B) is its first B images."""
    for name in ce.NAMES:
        assert torch.equal(ce.fixture(name, 7).x, ce.fixture(name, ce.B_MAX).x[:7])
        assert torch.equal(ce.reference64(ce.fixture(name, 2)).float(), ce.reference(name)[:2])


# --- head tail (fc2 + softmax + argmax) fixtures ---------------------------------------------

@pytest.fixture(params=ce.HEAD_NAMES)
def hfx(request):
    return ce.head_fixture(request.param)


def test_head_operands_and_headroom(hfx):
    """(i)-(iii) for fc2: operands equal their split, one of them is bf16-exact (both for the bf16
    precision), and sum(|hid||w|) + |b| is below 2^22 units by construction and on the data."""
    hid, w, b = hfx.hid, hfx.sd["fc2.weight"], hfx.sd["fc2.bias"]
    for what, t in (("hid", hid), ("fc2.weight", w)):
        hi, lo = ce.split_bf16(t)
        assert torch.equal(hi.double() + lo.double(), t.double()), what
    if hfx.precision == "bf16":
        assert _is_bf16_exact(hid) and _is_bf16_exact(w)
    else:
        assert _is_bf16_exact(hid) != _is_bf16_exact(w)  # exactly one wide operand: its lo term is exercised
        wide = w if _is_bf16_exact(hid) else hid
        assert (ce.split_bf16(wide)[1] != 0).float().mean().item() > 0.1  # 9-bit values: the low bit of the upper half
    mag = (hid.double().abs() @ w.double().abs().t() + b.double().abs()).max().item() / hfx.u
    ce.units(ce.head_logits64(hfx), hfx.u)
    print(f"{hfx.name}: sum|hid||w| + |b| {mag:.0f} units (worst case {hfx.bound_units:.0f})")
    assert mag <= hfx.bound_units < 2**22


def test_head_rows_look_like_relu_output(hfx):
    assert bool((hfx.hid >= 0).all())
    zeros = (hfx.hid == 0).float().mean().item()
    assert 0.2 <= zeros <= 0.4, zeros


def test_head_logits_exact_in_any_order(hfx):
    z = ce.head_logits64(hfx)
    assert torch.equal(z.float().double(), z)
    for order_seed in (None, 11):
        emu = ce.emulate_head_logits_fp32(hfx, order_seed)
        assert torch.equal(emu.view(torch.int32), z.float().view(torch.int32)), (hfx.name, order_seed)


def test_head_logits_spread_ties_and_underflow(hfx):
    """Spread of roughly +-40 and more, exact ties between classes 3/7 and 0/9 that are the row
    maximum often enough to exercise the first-index rule, and in every 8th row (so in every batch
    the GPU test uses) a gap above 104, where exp underflows to exactly 0 in fp32."""
    z = ce.head_logits64(hfx)
    assert torch.equal(z[:, 3], z[:, 7]) and torch.equal(z[:, 0], z[:, 9])
    assert 15.0 <= z.std().item() <= 40.0
    first = ce.first_argmax(z)
    assert int((first == 0).sum()) >= 20 and int((first == 3).sum()) >= 20
    assert int((first == 7).sum()) == 0 and int((first == 9).sum()) == 0
    assert len(first.unique()) == 8  # every class that can win does
    gap = z.max(dim=1).values - z.min(dim=1).values
    assert bool((gap[::8] > 104).all())
    p32 = torch.softmax(z.float(), dim=1)
    assert bool((p32[::8] == 0).any(dim=1).all())
    for B in (1, 15, 16, 17):
        assert torch.equal(ce.head_fixture(hfx.name, B).hid, hfx.hid[:B])


# --- fused fc1 fixtures -----------------------------------------------------------------------

@pytest.fixture(params=ce.FC1_NAMES)
def ffx(request):
    return ce.fc1_fixture(request.param)


def test_fc1_operands_and_headroom(ffx):
    """(i)-(iii) for fc1: operands equal their split, exactly one of them is bf16-exact and the other
    has a well-filled lo half, and sum(|a||w|) + |b| is below 2^24 units by construction and on the data."""
    for what, t in (("a", ffx.a), ("w", ffx.w)):
        hi, lo = ce.split_bf16(t)
        assert torch.equal(hi.double() + lo.double(), t.double()), what
    assert _is_bf16_exact(ffx.a) != _is_bf16_exact(ffx.w)
    wide = {"a_wide": ffx.a, "w_wide": ffx.w}[ffx.name]
    assert not _is_bf16_exact(wide)
    lo_fill = (ce.split_bf16(wide)[1] != 0).float().mean().item()
    assert lo_fill > 0.2, lo_fill
    mag = (ffx.a.double().abs() @ ffx.w.double().abs().t() + ffx.b.double().abs()).max().item() / ffx.u
    ce.units(ffx.b, ffx.u)
    ce.units(ce.fc1_reference64(ffx), ffx.u)
    print(f"{ffx.name}: lo nonzero {100 * lo_fill:.0f} %, sum|a||w| + |b| {mag:.0f} units (worst case {ffx.bound_units:.0f})")
    assert mag <= ffx.bound_units < 2**24
    assert ffx.b.abs().max().item() / ffx.u <= 2**20


def test_fc1_reference_is_exact_in_any_order(ffx):
    """The fp64 result survives the cast to fp32, about half of it survives the ReLU, and the fp32
    three-term emulation equals it bit for bit with k in its natural order and in a random order
    (44 rows: the emulation is 3 * 4096 element-wise steps)."""
    ref64 = ce.fc1_reference64(ffx)
    assert torch.equal(ref64.float().double(), ref64)
    nz = (ref64 != 0).double().mean().item()
    assert 0.35 <= nz <= 0.65, nz
    assert ref64.unique().numel() >= 1000
    part = ce.fc1_fixture(ffx.name, M=44)
    want = ref64[:44].float().view(torch.int32)
    assert torch.equal(ce.fc1_reference64(part).float().view(torch.int32), want)  # smaller shapes are prefixes
    for order_seed in (None, 13):
        emu = ce.emulate_fc1_fp32(part, order_seed)
        assert emu.dtype == torch.float32
        assert torch.equal(emu.view(torch.int32), want), (ffx.name, order_seed)


def test_fc1_k_prefixes_are_not_degenerate():
    """The GPU test also runs K = 32, 64 and 96: there too about half the outputs survive the ReLU."""
    for name in ce.FC1_NAMES:
        for M, N, K in ((1, 256, 32), (255, 256, 64), (257, 512, 96)):
            ref = ce.fc1_reference64(ce.fc1_fixture(name, M, N, K))
            nz = (ref != 0).double().mean().item()
            assert 0.3 <= nz <= 0.7, (name, M, N, K, nz)
