"""fp32 stage 0 with its conv2 consumer forced onto each compiled MFMA shape
(`ops.cifar.STAGE0_MFMA`), whichever is the default: the boundary against the
fp32 torch stage, the blocked hi/lo boundary against the same arm's fp32
output, and the colocated pipeline on an uneven per-workgroup image count.

Shapes are the smallest at which the persistent producer/consumer pipeline can
go wrong: one image (prologue and drain only), two images in one workgroup
(both double-buffer parities), 4 + 3 images in two workgroups (uneven counts,
parity wrap), and 257 images on the default grid (one workgroup with two images
beside 255 with one).  The bounds are those of test_kernels_gpu.py's
test_cifar_fp32_stage0_and_head and test_cifar_split_boundary_bit_identical.
On these inputs the arms are not compared with each other: the shapes sum K in
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
    torch.manual_seed(100 + B)
    model = NeuralNetwork().eval()
    sd = model.state_dict()
    x = torch.randn(B, 3, 32, 32)
    with torch.no_grad():
        part0 = CifarStage(0, 1).eval()
        part0.load_state_dict(sd, strict=False)
        mid = part0(x)
        ref = model(x)
    return sd, x, mid, ref


@pytest.fixture(params=["32x32x16", "16x16x32"])
def arm(request):
    """Force one compiled conv2 shape; restore the default afterwards."""
    from distributed_neural_networks_amd.ops import cifar as cops
    assert sorted(cops.STAGE0_MFMA) == ["16x16x32", "32x32x16"]  # every compiled arm is covered here
    prev = cops.set_stage0_mfma(request.param)
    yield request.param
    cops.set_stage0_mfma(prev)


@pytest.mark.parametrize("B,grid", CASES)
def test_stage0_boundary_matches_fp32_torch(arm, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    sd, x, mid, _ = _golden(B)
    w0 = cops.pack_stage0(sd, DEV)
    h = cops.stage0_forward(x.to(DEV), w0, grid=grid)
    torch.cuda.synchronize()
    err = (h.cpu() - mid).abs().max().item()
    print(f"arm {arm} B {B} grid {grid}: max|err| {err:.3e} (max|mid| {mid.abs().max().item():.3f})")
    assert err <= 2e-5 * max(1.0, mid.abs().max().item()), err


@pytest.mark.parametrize("B,grid", CASES)
def test_stage0_split_boundary_is_encode_of_own_fp32(arm, B, grid):
    from distributed_neural_networks_amd.ops import cifar as cops
    sd, x, _, _ = _golden(B)
    w0 = cops.pack_stage0(sd, DEV)
    xd = x.to(DEV)
    h32 = cops.stage0_forward(xd, w0, grid=grid, boundary="fp32")
    hsp = cops.stage0_forward(xd, w0, grid=grid, boundary="split")
    torch.cuda.synchronize()
    assert torch.equal(cops.encode_boundary(h32).view(torch.int32), hsp.view(torch.int32))


def test_colocated_pipeline_7_images(arm):
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
    print(f"arm {arm}: max|dprob| {dp:.3e}")
    assert dp <= 1e-5, dp
    assert torch.equal(pred, probs.argmax(1))
