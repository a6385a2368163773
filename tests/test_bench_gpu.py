"""bench.py on one GPU, as it is run for every change: the plain headline run
and ``--dump-outputs``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
ENV.update(PYTHONPATH=ROOT)
BATCH = 2304  # more than one workgroup's images and no multiple of 1024


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=ENV,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(tmp_path):
    """The plain line holds the headline only; the dumped arrays are the
    pipeline's results for the seeded images (fp32 torch on the same images
    and weights, the bound of ``smoke()``), identical in a second run."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    runs = []
    for name in ("a", "b"):
        d = _bench("--steps", "3", "--warmup", "1", "--batch", str(BATCH), "--dump-outputs", str(tmp_path / name))
        assert d["metric"] == "images/sec CIFAR-10 2-stage" and d["unit"] == "images/s" and d["higher_is_better"]
        assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"].startswith("fp32")
        assert d["value"] == pytest.approx(BATCH / (d["ms_per_step"] * 1e-3), rel=1e-2)
        assert not [k for k in d if k.startswith(("bf16_", "gpt2", "llama3", "max_abs_dprob"))], sorted(d)
        assert sorted(os.listdir(tmp_path / name)) == ["pred.npy", "probs.npy"]
        runs.append((np.load(tmp_path / name / "probs.npy"), np.load(tmp_path / name / "pred.npy")))
    (probs, pred), (probs2, pred2) = runs
    assert probs.dtype == np.float32 and probs.shape == (BATCH, 10) and pred.shape == (BATCH,)
    assert np.array_equal(probs, probs2) and np.array_equal(pred, pred2)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)  # bench_colocated's images
    x = torch.randn((BATCH, 3, 32, 32), device=dev, generator=g).cpu()
    m = NeuralNetwork().eval()
    m.load_state_dict(ckpt.random_stage_state_dict("cifar10", 0, 3, True, True, 0))
    with torch.no_grad():
        want = m(x).numpy()
    assert np.abs(probs - want).max() < 1e-5
    assert (pred == probs.argmax(1)).all()
