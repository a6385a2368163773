"""The ``mxfp4_head`` config key and the packing of a head-shaped MXFP4 weight (no GPU)."""
import copy
import json
import os

import pytest
import torch

from distributed_neural_networks_amd.config import ConfigError, load_node, resolve_node

CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")


def _base():
    with open(os.path.join(CONFIGS, "gpt2_4stage_1gpu_mxfp4.json")) as f:
        return json.load(f)


def test_mxfp4_head_values_and_default():
    c = _base()
    assert resolve_node(c, "node1").pipeline.mxfp4_head == "bf16"
    for v in ("bf16", "mxfp4"):
        c["mxfp4_head"] = v
        assert resolve_node(copy.deepcopy(c), "node1").pipeline.mxfp4_head == v


@pytest.mark.parametrize("key,val", [("mxfp4_head", "fp8"), ("dtype", "bf16"), ("dtype", "fp8")])
def test_mxfp4_head_errors(key, val):
    """Any other value, or "mxfp4" with a dtype other than mxfp4, is a ConfigError."""
    c = _base()
    c["mxfp4_head"] = "mxfp4"
    c[key] = val
    with pytest.raises(ConfigError, match="mxfp4_head"):
        resolve_node(c, "node1")


def test_shipped_config_loads():
    ctx = load_node(os.path.join(CONFIGS, "gpt2_4stage_1gpu_mxfp4_head.json"), "node1")
    assert ctx.pipeline.dtype == "mxfp4" and ctx.pipeline.mxfp4_head == "mxfp4"


def test_fold_norm_head_shape_packs_to_whole_tiles():
    """A 50257-row head folds and packs to ceil(N / 16) = 3142 tiles; the 15 pad rows carry zero codes, so a
    tile past N dequantises to zeros."""
    from distributed_neural_networks_amd.ops.gemm import fold_norm
    from distributed_neural_networks_amd.ops.w4 import Mxfp4Weight
    N, K = 50257, 64
    g = torch.Generator().manual_seed(0)
    f = fold_norm(torch.randn(N, K, generator=g), torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g),
                  None, False, 1e-5, "cpu", quant="mxfp4")
    assert isinstance(f.w, Mxfp4Weight) and f.w.shape == (N, K) and f.colsum.shape == (N,) and f.bias.shape == (N,)
    tiles = -(-N // 16)
    assert f.w.npad == tiles * 16 and f.w.q.numel() == tiles * 1024 and f.w.scales.numel() == tiles * 64
    last = f.w.q.view(tiles, 4, 16, 16)[-1]  # (group, row in tile, byte); chunk 0 is the only chunk
    assert bool((last[:, N % 16:] == 0).all()) and bool((last[:2, :N % 16] != 0).any())
