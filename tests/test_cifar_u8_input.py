"""uint8 image input of CIFAR stage 0, the parts that need no GPU: the normalisation table and
its packed form, the torch mirror of the kernel's lookup, image loading, the config keys, the
stage classes, and the preconditions of the exact uint8 fixtures (tests/cifar_u8_exact.py).
Every comparison of values is on bit patterns: the table *is* the transform, so there is no
tolerance to grant.  tests/test_cifar_u8_input_gpu.py holds the kernel to the same definitions.
"""
import json
import os

import numpy as np
import pytest
import torch

import cifar_exact as ce
import cifar_u8_exact as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIFAR_MEAN, CIFAR_STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
REF = {
    "nodes": [{"id": "node1", "address": "127.0.0.1:50051", "part_index": 0},
              {"id": "node2", "address": "127.0.0.1:50052", "part_index": 1}],
    "model_weights": "./cifar10_model.pth", "num_parts": 2, "return_to_node_id": "node1",
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_default_table_is_load_image_arithmetic():
    """Every byte value through cli.load_image's own arithmetic (numpy / 255, torch (t - 0.5) / 0.5)."""
    from distributed_neural_networks_amd.ops.cifar import make_input_table
    a = np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0
    want = (torch.from_numpy(a) - 0.5) / 0.5
    t = make_input_table()
    assert t.shape == (3, 256) and t.dtype == torch.float32 and t.device.type == "cpu"
    for c in range(3):
        assert torch.equal(_bits(t[c]), _bits(want))


def test_gather_equals_broadcast_arithmetic():
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (5, 32, 32, 3), dtype=torch.uint8, generator=g)
    mean = torch.tensor(CIFAR_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
    want = (x.permute(0, 3, 1, 2).float().div(255) - mean) / std
    got = normalize_u8(x, make_input_table(CIFAR_MEAN, CIFAR_STD))
    assert got.shape == (5, 3, 32, 32) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(_bits(got), _bits(want))


def _special_table():
    from distributed_neural_networks_amd.ops.cifar import make_input_table
    t = make_input_table(CIFAR_MEAN, CIFAR_STD).clone()
    t[0, 0], t[0, 1], t[1, 7], t[2, 200], t[2, 201] = 0.0, -0.0, float("nan"), float("inf"), float("-inf")
    return t


@pytest.mark.parametrize("which", ["default", "cifar", "special"])
def test_packed_table_halves(which):
    """Low 16 bits bf16(t), high 16 bits bf16(t - float(bf16(t))), as bit patterns."""
    from distributed_neural_networks_amd.ops.cifar import make_input_table, pack_input_table
    t = {"default": make_input_table, "cifar": lambda: make_input_table(CIFAR_MEAN, CIFAR_STD),
         "special": _special_table}[which]()
    p = pack_input_table(t, "cpu")
    assert p.shape == (3, 256) and p.dtype == torch.int32 and p.is_contiguous()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    want_lo16 = hi.view(torch.int16).to(torch.int32) & 0xFFFF
    want_hi16 = lo.view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(p & 0xFFFF, want_lo16)
    assert torch.equal((p >> 16) & 0xFFFF, want_hi16)


def test_table_argument_checks():
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8, pack_input_table
    with pytest.raises(ValueError, match="std"):
        make_input_table(std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError, match="three"):
        make_input_table(mean=(0.5, 0.5))
    with pytest.raises(ValueError, match="table"):
        pack_input_table(torch.zeros(3, 255), "cpu")
    with pytest.raises(ValueError, match="normalize_u8"):
        normalize_u8(torch.zeros(2, 3, 32, 32, dtype=torch.uint8), make_input_table())


def test_load_image_u8_then_normalize_is_load_image(tmp_path, capsys):
    from PIL import Image
    from distributed_neural_networks_amd.cli import load_image, load_image_u8
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8
    rng = np.random.default_rng(5)
    img = tmp_path / "x.png"
    Image.fromarray(rng.integers(0, 256, (40, 57, 3), dtype=np.uint8)).save(img)
    u8 = load_image_u8(str(img), "t")
    assert u8.shape == (1, 32, 32, 3) and u8.dtype == torch.uint8 and u8.is_contiguous()
    want = load_image(str(img), "t")
    assert torch.equal(_bits(normalize_u8(u8, make_input_table())), _bits(want))
    out = capsys.readouterr().out.splitlines()
    assert out[0] == f"[t] Loaded input image '{img}', shape: {u8.shape}"


def test_load_image_u8_missing_file(tmp_path, capsys):
    from distributed_neural_networks_amd.cli import load_image, load_image_u8
    missing = str(tmp_path / "nope.png")
    u8 = load_image_u8(missing, "n1")
    line_u8 = capsys.readouterr().out
    load_image(missing, "n1")
    assert line_u8 == capsys.readouterr().out == f"[n1] Input image '{missing}' not found. Using dummy data.\n"
    assert u8.shape == (1, 32, 32, 3) and u8.dtype == torch.uint8
    assert torch.equal(u8, load_image_u8(missing, "n1"))  # seeded


def test_load_image_u8_error_path(tmp_path, capsys):
    from distributed_neural_networks_amd.cli import load_image_u8
    bad = tmp_path / "bad.png"
    bad.write_bytes(b"not an image")
    u8 = load_image_u8(str(bad), "n1")
    assert capsys.readouterr().out.startswith("[n1] Error loading image: ")
    assert u8.shape == (1, 32, 32, 3) and u8.dtype == torch.uint8


def test_requests_pick_the_variant(tmp_path):
    """One function serves the three call sites: the default config gives exactly cifar_request's
    tensors, uint8 gives (rows,32,32,3) bytes, seeded per request."""
    from types import SimpleNamespace
    from distributed_neural_networks_amd.cli import cifar_request, make_cifar_request
    from distributed_neural_networks_amd.config import resolve_node
    args = SimpleNamespace(input_image=str(tmp_path / "nope.png"))
    torch.manual_seed(0)
    want = cifar_request(args, "n", 4, 2)
    torch.manual_seed(0)
    got = make_cifar_request(resolve_node(REF, "node1").pipeline, args, "n", 4, 2)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    c = dict(REF, input_dtype="uint8")
    pipe = resolve_node(c, "node1").pipeline
    a, b = make_cifar_request(pipe, args, "n", 4, 2), make_cifar_request(pipe, args, "n", 4, 2)
    assert a.shape == (4, 32, 32, 3) and a.dtype == torch.uint8 and torch.equal(a, b)
    assert not torch.equal(a[1:], make_cifar_request(pipe, args, "n", 4, 3)[1:])
    assert a.float().mean().item() == pytest.approx(127.5, abs=8)  # bytes over the whole range


def test_config_defaults_unchanged_and_values():
    from distributed_neural_networks_amd.config import resolve_node
    p = resolve_node(REF, "node1").pipeline
    assert p.input_dtype == "fp32" and p.input_mean == (0.5, 0.5, 0.5) and p.input_std == (0.5, 0.5, 0.5)
    c = dict(REF, input_dtype="uint8", input_mean=list(CIFAR_MEAN), input_std=list(CIFAR_STD))
    p = resolve_node(c, "node1").pipeline
    assert p.input_dtype == "uint8" and p.input_mean == CIFAR_MEAN and p.input_std == CIFAR_STD


@pytest.mark.parametrize("key,val", [("input_dtype", "int8"), ("input_dtype", 8), ("input_std", [0.5, 0.0, 0.5]),
                                     ("input_std", [0.5, 0.5]), ("input_mean", [0.5, 0.5, 0.5, 0.5]),
                                     ("input_mean", "0.5"), ("input_mean", [0.5, "x", 0.5]), ("input_std", 0.5)])
def test_config_rejects(key, val):
    from distributed_neural_networks_amd.config import ConfigError, resolve_node
    with pytest.raises(ConfigError, match=key):
        resolve_node(dict(REF, **{key: val}), "node1")


def test_config_rejects_uint8_for_other_models():
    from distributed_neural_networks_amd.config import ConfigError, resolve_node
    c = dict(REF, model="gpt2-tiny", model_weights="synthetic", input_dtype="uint8")
    with pytest.raises(ConfigError, match="input_dtype"):
        resolve_node(c, "node1")


def test_new_config_file_loads():
    from distributed_neural_networks_amd.config import load_node
    path = os.path.join(ROOT, "configs", "cifar_1gpu_colocated_u8.json")
    ctx = load_node(path, "node1")
    assert ctx.pipeline.input_dtype == "uint8" and ctx.pipeline.transport == "colocated"
    base = json.load(open(os.path.join(ROOT, "configs", "cifar_1gpu_colocated.json")))
    assert dict(json.load(open(path))) == dict(base, input_dtype="uint8")


def _torch_stages(**kw):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    sd0 = ckpt.random_stage_state_dict("cifar10", 0, 1, True, False, 9)
    sd1 = ckpt.random_stage_state_dict("cifar10", 2, 3, False, True, 9)
    return TorchStage("cifar10", sd0, 0, 1, True, False, **kw), TorchStage("cifar10", sd1, 2, 3, False, True, **kw)


@pytest.mark.parametrize("table", ["default", "cifar"])
def test_torch_stage_uint8_equals_default_on_normalised_input(table):
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8
    t = make_input_table() if table == "default" else make_input_table(CIFAR_MEAN, CIFAR_STD)
    s0, _ = _torch_stages()
    u0, u1 = _torch_stages(input_dtype="uint8", input_table=None if table == "default" else t)
    assert u0.in_spec(5) == ((5, 32, 32, 3), torch.uint8)
    assert u1.in_spec(5) == s0.out_spec(5)  # only a first stage sees images
    assert s0.in_spec(5) == ((5, 3, 32, 32), torch.float32)
    x = torch.randint(0, 256, (5, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    got, want = u0.forward(x), s0.forward(normalize_u8(x, t))
    assert torch.equal(_bits(got), _bits(want))


def test_colocated_pipeline_on_cpu_takes_uint8():
    """The pipeline sizes its input buffer from in_spec: uint8 NHWC, and the step is that of the
    default pipeline on the normalised images."""
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8
    from distributed_neural_networks_amd.runtime.pipeline import ColocatedPipeline
    x = torch.randint(0, 256, (5, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    cp = ColocatedPipeline(_torch_stages(input_dtype="uint8"), 5)
    assert cp.x.dtype == torch.uint8 and tuple(cp.x.shape) == (5, 32, 32, 3)
    got = cp(x)
    want = ColocatedPipeline(_torch_stages(), 5)(normalize_u8(x, make_input_table()))
    assert torch.equal(_bits(got.probs), _bits(want.probs)) and torch.equal(got.pred, want.pred)


def test_stage_classes_reject_bad_input_dtype():
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    sd0 = ckpt.random_stage_state_dict("cifar10", 0, 1, True, False, 9)
    with pytest.raises(ValueError, match="input_dtype"):
        TorchStage("cifar10", sd0, 0, 1, True, False, input_dtype="int8")


@pytest.mark.parametrize("name", ce.NAMES)
def test_u8_fixture_preconditions(name):
    """The recipe of tests/cifar_u8_exact.py keeps cifar_exact's preconditions: magnitudes,
    the fp64 reference's round trip through fp32, 257 distinct expected rows; and the fixture
    is what it says: table entries and pixels among the base fixture's values, bytes over the
    whole range, a table that is not monotone."""
    f = cu.u8_fixture(name)
    m1, m2 = ce.magnitude_bounds(f.fx)
    print(f"{name}: m1 = {m1:.0f} units (< 65536), m2 = {m2:.0f} units (< 4194304)")
    assert m1 < 2**16 and m2 < 2**22, (name, m1, m2)
    ref = cu.u8_reference(name)  # asserts the round trip
    assert ref.shape == (ce.B_MAX, 4096) and ref.dtype == torch.float32
    assert ref.unique(dim=0).shape[0] == ce.B_MAX
    vals = set(ce.fixture(name, ce.B_MAX).x.unique().tolist())
    assert set(f.table.flatten().tolist()) <= vals
    assert f.u8.shape == (ce.B_MAX, 32, 32, 3) and f.u8.dtype == torch.uint8
    assert int(f.u8.min()) == 0 and int(f.u8.max()) == 255
    for c in range(3):
        d = f.table[c, 1:] - f.table[c, :-1]
        assert bool((d > 0).any()) and bool((d < 0).any())
    small = cu.u8_fixture(name, 3)
    assert torch.equal(small.fx.x, f.fx.x[:3]) and torch.equal(small.u8, f.u8[:3])


def test_cli_colocated_uint8_on_cpu_matches_golden(tmp_path):
    """node.py with ``input_dtype: "uint8"`` (what this test is about: the CLI's request path):
    the image and the synthetic rows reach the stages as bytes, and every prediction is the
    golden model's on the normalised request."""
    import subprocess
    import sys
    from types import SimpleNamespace
    from PIL import Image
    from distributed_neural_networks_amd.cli import cifar_request_u8
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    from distributed_neural_networks_amd.ops.cifar import make_input_table, normalize_u8
    torch.manual_seed(11)
    m = NeuralNetwork().eval()
    pth, img, cfg = tmp_path / "cifar10_model.pth", tmp_path / "x.png", tmp_path / "c.json"
    torch.save(m.state_dict(), pth)
    Image.fromarray(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8)).save(img)
    c = dict(REF, model_weights=str(pth), transport="colocated", model="cifar10", input_dtype="uint8",
             input_mean=list(CIFAR_MEAN), input_std=list(CIFAR_STD), micro_batch_size=3, num_microbatches=2)
    cfg.write_text(json.dumps(c))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--input_image", str(img), "--device", "cpu"],
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"Loaded input image '{img}', shape: torch.Size([1, 32, 32, 3])" in r.stdout
    line = [l for l in r.stdout.splitlines() if "***** FINAL PREDICTION (Index):" in l]
    assert line, r.stdout[-2000:]
    got = json.loads(line[-1].split("(Index):")[1].split("*")[0].strip())
    x8 = cifar_request_u8(SimpleNamespace(input_image=str(img)), "t", 6, 0)
    with torch.no_grad():
        want = m(normalize_u8(x8, make_input_table(CIFAR_MEAN, CIFAR_STD))).argmax(1).tolist()
    assert got == want
