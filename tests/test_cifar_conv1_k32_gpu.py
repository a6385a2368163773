"""fp32 stage 0 with its conv1 producer forced onto each compiled K packing
(`ops.cifar.STAGE0_CONV1`) crossed with each conv2 MFMA shape
(`ops.cifar.STAGE0_MFMA`): the boundary against the fp32 torch stage, the
blocked hi/lo boundary against the same arm's fp32 output, and the colocated
pipeline on an uneven per-workgroup image count; then, per conv1 arm, every one
of the 27 taps alone and the halo.

Shapes and bounds are those of test_cifar_stage0_mfma_gpu.py: one image
(prologue and drain only), two images in one workgroup (both double-buffer
parities), 4 + 3 images in two workgroups, 257 images on the default grid;
2e-5 * max(1, max|mid|) on the boundary, 1e-5 on the probabilities.  On these
inputs the two conv1 arms are not compared with each other: they sum K in
different orders.  tests/test_cifar_stage0_exact_gpu.py compares them bitwise, on
inputs for which every order gives the same bits.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [(1, 0), (2, 1), (7, 2), (257, 0)]  # (B, grid); grid 0 = the default, one workgroup per CU


@functools.lru_cache(maxsize=None)
def _golden(B):
    """state dict, images, fp32 torch boundary and probabilities (CPU; computed once per B)."""
    from distributed_neural_networks_amd.models.cifar import CifarStage, NeuralNetwork
    torch.manual_seed(300 + B)
    model = NeuralNetwork().eval()
    sd = model.state_dict()
    x = torch.randn(B, 3, 32, 32)
    with torch.no_grad():
        part0 = CifarStage(0, 1).eval()
        part0.load_state_dict(sd, strict=False)
        mid = part0(x)
        ref = model(x)
    return sd, x, mid, ref


def _torch_stage0(sd, x):
    from distributed_neural_networks_amd.models.cifar import CifarStage
    with torch.no_grad():
        part0 = CifarStage(0, 1).eval()
        part0.load_state_dict(sd, strict=False)
        return part0(x)


@pytest.fixture(params=["k48", "k32"])
def conv1(request):
    """Force one compiled conv1 packing; restore the default afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    assert sorted(cops.STAGE0_CONV1) == ["k32", "k48"]  # every compiled arm is covered here
    prev = cops.set_stage0_conv1(request.param)
    yield request.param
    cops.set_stage0_conv1(prev)


@pytest.fixture(params=["32x32x16", "16x16x32"])
def mfma(request):
    """Force one compiled conv2 shape; restore the default afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    prev = cops.set_stage0_mfma(request.param)
    yield request.param
    cops.set_stage0_mfma(prev)


def _check_boundary(sd, x, mid, grid, what):
    from distributed_neural_networks_amd.ops import cifar as cops
    h = cops.stage0_forward(x.to(DEV), cops.pack_stage0(sd, DEV), grid=grid)
    torch.cuda.synchronize()
    err = (h.cpu() - mid).abs().max().item()
    print(f"{what}: max|err| {err:.3e} (max|mid| {mid.abs().max().item():.3f})")
    assert err <= 2e-5 * max(1.0, mid.abs().max().item()), (what, err)


@pytest.mark.parametrize("B,grid", CASES)
def test_stage0_boundary_matches_fp32_torch(conv1, mfma, B, grid):
    sd, x, mid, _ = _golden(B)
    _check_boundary(sd, x, mid, grid, f"conv1 {conv1} conv2 {mfma} B {B} grid {grid}")


@pytest.mark.parametrize("B,grid", CASES)
def test_stage0_split_boundary_is_encode_of_own_fp32(conv1, mfma, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    sd, x, _, _ = _golden(B)
    w0 = cops.pack_stage0(sd, DEV)
    xd = x.to(DEV)
    h32 = cops.stage0_forward(xd, w0, grid=grid, boundary="fp32")
    hsp = cops.stage0_forward(xd, w0, grid=grid, boundary="split")
    torch.cuda.synchronize()
    assert torch.equal(cops.encode_boundary(h32).view(torch.int32), hsp.view(torch.int32))


def test_colocated_pipeline_7_images(conv1, mfma):
    from distributed_neural_networks_amd.ops import cifar as cops
    from distributed_neural_networks_amd.runtime.pipeline import ColocatedPipeline
    from distributed_neural_networks_amd.runtime.stages import CifarHipStage
    sd, x, _, ref = _golden(7)
    grid0 = cops.STAGE0_GRID
    cops.set_stage0_grid(2)
    try:
        st = [CifarHipStage(sd, 0, 1, DEV), CifarHipStage(sd, 2, 3, DEV)]
        out = ColocatedPipeline(st, 7)(x.to(DEV))
        torch.cuda.synchronize()
    finally:
        cops.set_stage0_grid(grid0)
    probs, pred = out.probs.cpu(), out.pred.cpu().long()
    dp = (probs - ref).abs().max().item()
    print(f"conv1 {conv1} conv2 {mfma}: max|dprob| {dp:.3e}")
    assert dp <= 1e-5, dp
    assert torch.equal(pred, probs.argmax(1))


def test_every_tap_alone(conv1):
    """conv1 weight 1 at one tap for every output channel, 0 elsewhere; the other
    layers random.  A permuted or parity-swapped packing fails at a named tap."""
    sd0, x, _, _ = _golden(2)
    for c in range(3):
        for ky in range(3):
            for kx in range(3):
                sd = dict(sd0)
                w = torch.zeros_like(sd0["conv1.weight"])
                w[:, c, ky, kx] = 1.0
                sd["conv1.weight"] = w
                _check_boundary(sd, x, _torch_stage0(sd, x), 1, f"conv1 {conv1} tap c={c} ky={ky} kx={kx}")


@pytest.mark.parametrize("ring", ["only_ring", "no_ring"])
def test_halo(conv1, ring):
    """An image that is zero except its outermost ring of pixels, and one that is
    zero on that ring; two images in one workgroup, so both buffer parities."""
    sd, x, _, _ = _golden(2)
    m = torch.zeros(32, 32)
    m[0, :] = m[31, :] = m[:, 0] = m[:, 31] = 1.0
    xr = x * (m if ring == "only_ring" else 1.0 - m)
    _check_boundary(sd, xr, _torch_stage0(sd, xr), 1, f"conv1 {conv1} halo {ring}")
