"""The K = 32 packing of the fp32 stage-0 conv1 (`ops.cifar._conv1_k32`) against
`torch.nn.functional.conv2d`, through a pure-torch im2col that follows the
layout `csrc/kernels/cifar_x3.hip` documents ("conv1 on K = 32"):

* a padded input row is one zero element, then 34 pixels x 3 channels (halo
  pixels included), in a row of 112 elements (56 dwords);
* pixel x's 10-element read of padded row y + ky starts at element 3x (even x)
  or 3x + 1 (odd x); its element e goes to K slot `conv1_k32_slot(ky, e)`;
* the weights are one `[32 oc][32 k]` set per x parity.

Every K slot the window does not own (the junk element of each read, slots 30
and 31) is filled with 1e3 in A, so a non-zero weight there shows as an error of
1e3 times that weight.  Both parities, x = 0 and x = 31 and the first and last
row are covered: the whole 32x32 image is compared.  Bound: 1e-4 absolute on
unit-normal data (fp32 summation order only; measured 5.7e-6 when the layout
was first emulated).
"""
import torch
import torch.nn.functional as F

from distributed_neural_networks_amd.ops import cifar as cops

ROW = 112  # elements per padded row
FILL = 1e3


def _planes(x):
    """(B,3,32,32) -> (B,34,ROW): zero element, 34 pixels x 3 channels, zero tail."""
    B = x.shape[0]
    p = torch.zeros(B, 34, ROW)
    xp = F.pad(x, (1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(B, 34, 102)  # (B, Y, X*3 + c)
    p[:, :, 1:103] = xp
    return p


def _im2col(x):
    """A (B,32,32,32 k) with the filler constant in every slot no tap owns."""
    B = x.shape[0]
    p = _planes(x)
    A = torch.full((B, 32, 32, 32), FILL)
    for xx in range(32):
        start = 3 * xx + (xx & 1)
        assert start % 2 == 0 and start + 10 <= ROW  # 4-byte aligned, inside the row
        junk = 0 if xx % 2 == 0 else 9
        for ky in range(3):
            rd = p[:, ky:ky + 32, start:start + 10]  # (B, y, e)
            for e in range(10):
                if e != junk:
                    A[:, :, xx, cops.conv1_k32_slot(ky, e)] = rd[:, :, e]
    return A


def test_k32_slots_are_a_bijection_onto_0_29():
    slots = sorted(cops.conv1_k32_slot(ky, e) for ky in range(3) for e in range(10))
    assert slots == list(range(30))


def test_conv1_k32_packing_matches_conv2d():
    torch.manual_seed(7)
    sd = {"conv1.weight": torch.randn(32, 3, 3, 3)}
    x = torch.randn(2, 3, 32, 32)
    w = cops._conv1_k32(sd)
    assert tuple(w.shape) == (2, 32, 32)
    assert int((w != 0).sum()) == 2 * 32 * 27  # exactly the 27 taps per parity and channel
    A = _im2col(x)
    out = torch.empty(2, 32, 32, 32)  # (B, y, x, oc)
    for par in range(2):
        out[:, :, par::2] = A[:, :, par::2] @ w[par].t()
    ref = F.conv2d(x, sd["conv1.weight"], padding=1).permute(0, 2, 3, 1)
    err = (out - ref).abs()
    print(f"max|err| {err.max().item():.3e}; x=0 {err[:, :, 0].max().item():.3e}, x=31 {err[:, :, 31].max().item():.3e}, "
          f"y=0 {err[:, 0].max().item():.3e}, y=31 {err[:, 31].max().item():.3e}")
    assert err.max().item() <= 1e-4


def test_pack_stage0_carries_both_conv1_packings():
    torch.manual_seed(8)
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    sd = NeuralNetwork().state_dict()
    w0 = cops.pack_stage0(sd, "cpu")
    assert tuple(w0.w1h.shape) == (32, 48) and tuple(w0.w1h32.shape) == (2, 32, 32)
    full = cops._conv1_k32(sd)
    assert (w0.w1h32.float() + w0.w1l32.float() - full).abs().max().item() <= 2.0 ** -16 * full.abs().max().item()
    assert sorted(cops.STAGE0_CONV1) == ["k32", "k48"]
