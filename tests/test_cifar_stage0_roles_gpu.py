"""The role handshake of fp32 stage 0 where the other exact tests do not reach.

The kernel's two wave groups (conv1 with input staging, conv2 with the boundary stores) meet at
one barrier per image and hand images over through two double buffers (input planes, pooled
conv1 map).  test_cifar_stage0_exact_gpu.py and test_cifar_u8_input_gpu.py run one, two, 4 + 3
and one-per-workgroup images; here the per-workgroup image counts are 1 to 4 inside one launch
and unequal across workgroups, so the fill (load, stage, second load before the first barrier),
the drain (the iteration in which only conv2 works) and both parities of both double buffers
are met by workgroups that run side by side with different trip counts:

    (B, grid)   images per workgroup
    (3, 1)      3
    (4, 1)      4
    (5, 2)      3, 2
    (6, 4)      2, 2, 1, 1
    (9, 4)      3, 2, 2, 2
    (2, 4)      grid above B: the entry point launches min(grid, B) workgroups, 1, 1
    (1, 8)      the same, 1

The default arm on fp32 input and on uint8 input, on the fixtures of cifar_exact.py and
cifar_u8_exact.py, compared as int32 bit patterns with ``reference(name)`` and
``u8_reference(name)``: no tolerance.  The images of a batch all differ, so an image computed
from a stale slot shows as another image's row.  Both boundary encodings on (5, 2).  Race
screen: 20 back-to-back launches at (9, 4) into one buffer, each compared, for both inputs.
"""
import functools

import pytest
import torch

import cifar_exact as ce
import cifar_u8_exact as cu

pytestmark = pytest.mark.gpu

DEV = "cuda"
COUNTS = [(3, 1), (4, 1), (5, 2), (6, 4), (9, 4)]  # (B, grid): 1-4 images per workgroup, unequal
EMPTY = [(2, 4), (1, 8)]                           # more workgroups asked for than images
INPUTS = ("fp32", "u8")
SENTINEL = 0x7FC5A5A5  # int32 bits of a NaN with a payload that no arithmetic produces


@functools.lru_cache(maxsize=None)
def _golden(name, kind):
    """Per fixture and input kind, once: packed weights, the images, the packed table (uint8 input) and
    the expected boundary (int32 bits, fp32 and blocked hi/lo encoding) on the device."""
    from distributed_neural_networks_amd.ops import cifar as cops
    if kind == "u8":
        f = cu.u8_fixture(name)
        sd, x, table, ref = f.fx.sd, f.u8.to(DEV), cops.pack_input_table(f.table, DEV), cu.u8_reference(name)
    else:
        fx = ce.fixture(name, ce.B_MAX)
        sd, x, table, ref = fx.sd, fx.x.to(DEV), None, ce.reference(name)
    refd = ref.to(DEV)
    encd = cops.encode_boundary(refd)
    torch.cuda.synchronize()
    return cops.pack_stage0(sd, DEV), x, table, refd.view(torch.int32), encd.view(torch.int32)


def _assert_bits(got, want, what):
    """got, want: (B,4096) int32 bit patterns on the device."""
    if torch.equal(got, want):
        return
    g, w = got.cpu(), want.cpu()
    bad = (g != w).nonzero()
    img, el = bad[0].tolist()
    gv, wv = g[img, el].view(torch.float32).item(), w[img, el].view(torch.float32).item()
    print(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in images {bad[:, 0].unique().tolist()}; first at "
          f"image {img} element {el}: got {gv!r} ({g[img, el].item() & 0xFFFFFFFF:#010x}), "
          f"expected {wv!r} ({w[img, el].item() & 0xFFFFFFFF:#010x})")
    pytest.fail(f"{what}: image {img} element {el}: got {gv!r}, expected {wv!r} ({bad.shape[0]} elements differ)")


def _default_arm():
    from distributed_neural_networks_amd.ops import cifar as cops
    lib = cops.lib()
    assert (lib.cifar_s0_get_conv1(), lib.cifar_s0_get_mfma(), lib.cifar_s0_get_wide_store()) == (1, 1, 1)


@pytest.mark.parametrize("B,grid", COUNTS + EMPTY)
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("name", ce.NAMES)
def test_unequal_image_counts_are_bitwise_the_reference(name, kind, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    _default_arm()
    w0, x, table, ref, _ = _golden(name, kind)
    buf = torch.full((B, 4096), SENTINEL, dtype=torch.int32, device=DEV)
    cops.stage0_forward(x[:B], w0, out=buf.view(torch.float32), grid=grid, table=table)
    torch.cuda.synchronize()
    _assert_bits(buf, ref[:B], f"{name} {kind} input B {B} grid {grid}")


@pytest.mark.parametrize("boundary", ["fp32", "split"])
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("name", ce.NAMES)
def test_both_boundary_encodings(name, kind, boundary):
    from distributed_neural_networks_amd.ops import cifar as cops
    _default_arm()
    B, grid = 5, 2
    w0, x, table, ref, enc = _golden(name, kind)
    buf = torch.full((B, 4096), SENTINEL, dtype=torch.int32, device=DEV)
    cops.stage0_forward(x[:B], w0, out=buf.view(torch.float32), grid=grid, boundary=boundary, table=table)
    torch.cuda.synchronize()
    _assert_bits(buf, (ref if boundary == "fp32" else enc)[:B], f"{name} {kind} input B {B} grid {grid} {boundary} boundary")


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("name", ce.NAMES)
def test_back_to_back_launches_into_one_buffer(name, kind):
    """Race screen: 20 launches queued without a host wait between them, each followed on the stream
    by a copy of the buffer; every copy is bitwise the reference."""
    from distributed_neural_networks_amd.ops import cifar as cops
    _default_arm()
    B, grid = 9, 4
    w0, x, table, ref, _ = _golden(name, kind)
    buf = torch.full((B, 4096), SENTINEL, dtype=torch.int32, device=DEV)
    kept = torch.empty((20, B, 4096), dtype=torch.int32, device=DEV)
    for i in range(20):
        cops.stage0_forward(x[:B], w0, out=buf.view(torch.float32), grid=grid, table=table)
        kept[i].copy_(buf)
    torch.cuda.synchronize()
    for i in range(20):
        _assert_bits(kept[i], ref[:B], f"{name} {kind} input B {B} grid {grid} launch {i}")
