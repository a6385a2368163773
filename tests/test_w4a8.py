"""The ``mxfp4_prefill`` config key (no GPU)."""
import copy
import json
import os

import pytest

from distributed_neural_networks_amd.config import ConfigError, load_node, resolve_node

CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")


def _base():
    with open(os.path.join(CONFIGS, "gpt2_4stage_1gpu_mxfp4.json")) as f:
        return json.load(f)


def test_mxfp4_prefill_values_and_default():
    c = _base()
    assert resolve_node(c, "node1").pipeline.mxfp4_prefill == "bf16"
    for v in ("bf16", "e4m3"):
        c["mxfp4_prefill"] = v
        assert resolve_node(copy.deepcopy(c), "node1").pipeline.mxfp4_prefill == v


@pytest.mark.parametrize("key,val", [("mxfp4_prefill", "fp4"), ("dtype", "bf16"), ("dtype", "fp8")])
def test_mxfp4_prefill_errors(key, val):
    """Any other value, or "e4m3" with a dtype other than mxfp4, is a ConfigError."""
    c = _base()
    c["mxfp4_prefill"] = "e4m3"
    c[key] = val
    with pytest.raises(ConfigError, match="mxfp4_prefill"):
        resolve_node(c, "node1")


def test_shipped_config_loads():
    ctx = load_node(os.path.join(CONFIGS, "gpt2_4stage_1gpu_mxfp4_a8.json"), "node1")
    assert ctx.pipeline.dtype == "mxfp4" and ctx.pipeline.mxfp4_prefill == "e4m3"
