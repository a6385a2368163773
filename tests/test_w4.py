"""MXFP4 weights on the host (ops/w4.py): packer, quantiser, dequantiser, config."""
import json

import pytest
import torch

from distributed_neural_networks_amd.ops import w4

GRID = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


def test_pack_dequantize_table():
    """Fragment order and its inverse against a table lookup: (40, 160) pads both
    N (to 48) and K (to 256), and every code occurs."""
    g = torch.Generator().manual_seed(0)
    N, K = 40, 160
    codes = torch.randint(0, 16, (N, K), generator=g)
    codes[0, :16] = torch.arange(16)
    exps = torch.randint(120, 135, (N, K // 32), generator=g)
    w = w4.pack_mxfp4(codes, exps)
    assert w.q.numel() == 48 * 256 // 2 and w.scales.numel() == 48 * 256 // 32 and w.shape == (N, K)
    ref = GRID[codes] * torch.exp2(exps.float() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(w4.dequantize(w), ref)
    # lane 16 g + r of block (tile 0, chunk 1) holds row r, k = 128 + 32 g ..: its first byte and its scale
    blk = w.q.view(3, 2, 64, 16)[0, 1]
    assert int(blk[5, 0]) == int(codes[5, 128] | (codes[5, 129] << 4))
    assert int(w.scales.view(3, 2, 64)[0, 1, 5]) == int(exps[5, 4])


def test_quantize_rounding():
    """Ties go to the even code, values saturate at +-6, an all-zero block gets
    exponent 127, and quantising the dequantised weight changes nothing."""
    x = torch.zeros(3, 32)
    # block amax 6 -> scale 1: ties 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    ties = torch.tensor([6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, -.25, -.75, -2.5, -5])
    x[0, :12] = ties
    x[1, :3] = torch.tensor([7.9, -7.5, 4.0])  # amax 7.9 -> scale 1: both saturate
    w = w4.quantize_weight_mxfp4(x, "cpu")
    d = w4.dequantize(w)
    assert d[0, :12].tolist() == [6, 0, 1, 1, 2, 2, 4, 4, 0, -1, -2, -4]
    assert d[1, :3].tolist() == [6, -6, 4]
    assert w4.unpack_mxfp4(w)[1].view(-1).tolist() == [127, 127, 127]
    r = torch.randn(40, 160, generator=torch.Generator().manual_seed(1)) * torch.logspace(-3, 3, 40)[:, None]
    q1 = w4.quantize_weight_mxfp4(r, "cpu")
    q2 = w4.quantize_weight_mxfp4(w4.dequantize(q1), "cpu")
    assert torch.equal(q1.q, q2.q) and torch.equal(q1.scales, q2.scales)


@pytest.mark.parametrize("bad", [0, 255])
def test_pack_rejects(bad):
    codes = torch.zeros(16, 64, dtype=torch.int64)
    exps = torch.full((16, 2), 127)
    exps[3, 1] = bad
    with pytest.raises(ValueError, match="1..254"):
        w4.pack_mxfp4(codes, exps)
    with pytest.raises(ValueError, match="multiple of 32"):
        w4.pack_mxfp4(torch.zeros(16, 48, dtype=torch.int64), torch.full((16, 1), 127))


def test_config_mxfp4_loads():
    from distributed_neural_networks_amd.config import load_node
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                        "gpt2_4stage_1gpu_mxfp4.json")
    assert load_node(path, "node1").pipeline.dtype == "mxfp4"
    base = json.load(open(path.replace("_mxfp4", "")))
    new = json.load(open(path))
    assert {k: v for k, v in new.items() if k != "dtype"} == {k: v for k, v in base.items() if k != "dtype"}
