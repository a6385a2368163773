"""fp32 stage 0 against a bit-exact reference, on every compiled arm.

tests/cifar_exact.py places inputs and weights on power-of-two grids so that
every product and partial sum of the kernels' three-term bf16 split is exactly
representable in fp32 (its preconditions are asserted on the CPU in
tests/test_cifar_exact.py).  The result is then the same in every summation
order, so the fp64 torch stage cast to fp32 is the expected output of every arm
bit for bit: no tolerance, and one wrong low-order term, one small wrong element
or a lo plane that is stale by one image all fail.  Every arm is compared with
the one reference, which makes the arms equal to each other: conv1 in
{k48, k32} x conv2 in {16x16x32, 32x32x16 with 16-byte stores, 32x32x16 with
8-byte stores (set_stage0_wide_store(0))}.

Shapes are those of test_cifar_stage0_mfma_gpu.py: one image (prologue and
drain only), two images in one workgroup (both double-buffer parities), 4 + 3
images in two workgroups, 257 images on the default grid.  The images of a
batch all differ, so a stale input or pooled-map slot shows as another image's
row.  Guards: output and input are the middle of larger buffers; the output's
margins keep their sentinel and the images past either end are NaN.  Race
screen: 20 launches of the default arms, each into a re-filled buffer.
"""
import functools

import pytest
import torch

import cifar_exact as ce

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(1, 0), (2, 1), (7, 2), (257, 0)]  # (B, grid); grid 0 = the default, one workgroup per CU
CONV2 = {"16x16x32": ("16x16x32", 1), "32x32x16": ("32x32x16", 1), "32x32x16-store8": ("32x32x16", 0)}
MARGIN = 64
SENTINEL = 0x7FC5A5A5  # int32 bits of a NaN with a payload that no arithmetic produces


@functools.lru_cache(maxsize=None)
def _golden(name):
    """Per fixture, once: packed weights, the 257 images and the expected boundary (int32 bits,
    fp32 and blocked hi/lo encoding) on the device; preconditions (iii) and (iv) on all 257."""
    from distributed_neural_networks_amd.ops import cifar as cops
    fx = ce.fixture(name, ce.B_MAX)
    m1, m2 = ce.magnitude_bounds(fx)
    assert m1 < 2**16 and m2 < 2**22, (name, m1, m2)
    ref = ce.reference(name)
    assert ref.unique(dim=0).shape[0] == ce.B_MAX
    w0 = cops.pack_stage0(fx.sd, DEV)
    refd = ref.to(DEV)
    encd = cops.encode_boundary(refd)
    torch.cuda.synchronize()
    return w0, fx.x.to(DEV), refd.view(torch.int32), encd.view(torch.int32)


@pytest.fixture(params=["k48", "k32"])
def conv1(request):
    """Force one compiled conv1 packing; restore the previous setting afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    assert sorted(cops.STAGE0_CONV1) == ["k32", "k48"]  # every compiled arm is covered here
    prev = cops.set_stage0_conv1(request.param)
    yield request.param
    cops.set_stage0_conv1(prev)


@pytest.fixture(params=list(CONV2))
def conv2(request):
    """Force one compiled conv2 consumer (MFMA shape and store width); restore both afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    assert sorted(cops.STAGE0_MFMA) == ["16x16x32", "32x32x16"]  # every compiled arm is covered here
    shape, wide = CONV2[request.param]
    prev_mfma = cops.set_stage0_mfma(shape)
    prev_wide = cops.set_stage0_wide_store(wide)
    yield request.param
    cops.set_stage0_wide_store(prev_wide)
    cops.set_stage0_mfma(prev_mfma)


def _assert_bits(got, want, what):
    """got, want: (B,4096) int32 bit patterns on the device."""
    if torch.equal(got, want):
        return
    g, w = got.cpu(), want.cpu()
    bad = (g != w).nonzero()
    img, el = bad[0].tolist()
    gv, wv = g[img, el].view(torch.float32).item(), w[img, el].view(torch.float32).item()
    print(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in {bad[:, 0].unique().numel()} images; first at "
          f"image {img} element {el}: got {gv!r} ({g[img, el].item() & 0xFFFFFFFF:#010x}), "
          f"expected {wv!r} ({w[img, el].item() & 0xFFFFFFFF:#010x})")
    pytest.fail(f"{what}: image {img} element {el}: got {gv!r}, expected {wv!r} ({bad.shape[0]} elements differ)")


@pytest.mark.parametrize("B,grid", CASES)
@pytest.mark.parametrize("name", ce.NAMES)
def test_stage0_is_bitwise_the_fp64_reference(name, conv1, conv2, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, x, ref, enc = _golden(name)
    what = f"{name} conv1 {conv1} conv2 {conv2} B {B} grid {grid}"
    h = cops.stage0_forward(x[:B], w0, grid=grid)
    hs = cops.stage0_forward(x[:B], w0, grid=grid, boundary="split")
    torch.cuda.synchronize()
    _assert_bits(h.view(torch.int32), ref[:B], what + " fp32 boundary")
    _assert_bits(hs.view(torch.int32), enc[:B], what + " split boundary")


@pytest.mark.parametrize("B,grid", CASES)
@pytest.mark.parametrize("name", ["c1_wwide", "c2_awide"])
def test_stage0_stays_inside_its_batch(name, conv1, conv2, B, grid):
    """Rows [64 : 64 + B] of a sentinel-filled output, images [64 : 64 + B] of an input whose
    other images are NaN: both margins keep the sentinel and the result is still the reference."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, x, ref, enc = _golden(name)
    xin = torch.full((B + 2 * MARGIN, 3, 32, 32), float("nan"), device=DEV)
    xin[MARGIN:MARGIN + B] = x[:B]
    for boundary, want in (("fp32", ref), ("split", enc)):
        what = f"{name} conv1 {conv1} conv2 {conv2} B {B} grid {grid} {boundary} boundary, guarded"
        buf = torch.full((B + 2 * MARGIN, 4096), SENTINEL, dtype=torch.int32, device=DEV)
        out = buf.view(torch.float32)[MARGIN:MARGIN + B]
        cops.stage0_forward(xin[MARGIN:MARGIN + B], w0, out=out, grid=grid, boundary=boundary)
        torch.cuda.synchronize()
        assert bool((buf[:MARGIN] == SENTINEL).all()), what + ": rows before the batch were written"
        assert bool((buf[MARGIN + B:] == SENTINEL).all()), what + ": rows past the batch were written"
        _assert_bits(buf[MARGIN:MARGIN + B], want[:B], what)


@pytest.mark.parametrize("B,grid", [(7, 2), (257, 0)])
@pytest.mark.parametrize("name", ce.NAMES)
def test_stage0_repeated_launches(name, B, grid):
    """Race screen on the default arms: 20 launches into a buffer re-filled with the sentinel,
    every one bitwise the reference."""
    from distributed_neural_networks_amd.ops import cifar as cops
    w0, x, ref, _ = _golden(name)
    buf = torch.empty((B, 4096), dtype=torch.int32, device=DEV)
    for i in range(20):
        buf.fill_(SENTINEL)
        cops.stage0_forward(x[:B], w0, out=buf.view(torch.float32), grid=grid)
        torch.cuda.synchronize()
        _assert_bits(buf, ref[:B], f"{name} B {B} grid {grid} launch {i}")
