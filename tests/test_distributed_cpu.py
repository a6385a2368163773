"""Multi-process paths on CPU (gloo): the CLI transports, the streaming pipeline
schedule, and bench.py's distributed placements.  Same code as the RCCL path
on MI355X; only the backend and the stage compute differ."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _write_image(path):
    from PIL import Image
    import numpy as np
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (40, 48, 3), dtype=np.uint8)).save(path)


def _golden_pred(ckpt_path, img_path):
    from distributed_neural_networks_amd.cli import load_image
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    m = NeuralNetwork().eval()
    m.load_state_dict(torch.load(ckpt_path, weights_only=True))
    with torch.no_grad():
        return int(m(load_image(img_path, "t")).argmax(1).item())


@pytest.fixture
def cifar_setup(tmp_path):
    from distributed_neural_networks_amd.checkpoint import make_full_checkpoint
    ck = tmp_path / "cifar10_model.pth"
    make_full_checkpoint("cifar10", str(ck), 3)
    img = tmp_path / "img.png"
    _write_image(str(img))
    return tmp_path, ck, img


def _cfg(tmp_path, transport, n=2, model="cifar10", weights=None, **extra):
    ports = [free_port() for _ in range(n)]
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{ports[i]}", "part_index": i} for i in range(n)],
         "model_weights": weights, "num_parts": n, "return_to_node_id": "node1", "transport": transport,
         "model": model}
    c.update(extra)
    p = tmp_path / f"cfg_{transport}_{n}.json"
    p.write_text(json.dumps(c))
    return p


def _run_nodes(cfg, n, img, extra0=(), timeout=120):
    procs = []
    for i in range(1, n):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", f"node{i + 1}",
                                       "--config", str(cfg), "--serve_seconds", "90"], env=ENV,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                             "--input_image", str(img), "--shutdown_pipeline", *extra0], env=ENV,
                            capture_output=True, text=True, timeout=timeout)
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=60)[0])
            except subprocess.TimeoutExpired:
                p.kill()
                outs.append(p.communicate()[0])
        return r0, outs
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def _final_pred(out):
    lines = [l for l in out.splitlines() if "***** FINAL PREDICTION (Index):" in l]
    assert lines, out[-3000:]
    return int(lines[-1].split("(Index):")[1].split("*")[0].strip())


@pytest.mark.parametrize("transport", ["grpc", "gloo"])
def test_cli_two_stage_matches_golden(cifar_setup, transport):
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, transport, 2, weights=str(ck))
    r0, outs = _run_nodes(cfg, 2, img)
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-3000:]
    assert _final_pred(r0.stdout) == _golden_pred(str(ck), str(img))
    if transport == "grpc":
        assert "--- Node Configuration ---" in r0.stdout
        assert "Processing complete. Prediction:" in r0.stdout


def test_cli_three_stage_grpc_chain(cifar_setup):
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "grpc", 3, weights=str(ck))
    r0, outs = _run_nodes(cfg, 3, img)
    assert r0.returncode == 0, r0.stdout[-2000:]
    assert _final_pred(r0.stdout) == _golden_pred(str(ck), str(img))
    assert "[node2] Forwarded. Next node status: [node3] Processing complete." in r0.stdout
    assert any("Response from next node" in o for o in outs)


def test_cli_config_errors(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "x", "--config",
                        str(tmp_path / "missing.json")], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "ERROR: Config file not found" in r.stdout


def test_cli_missing_weights(tmp_path):
    cfg = _cfg(tmp_path, "grpc", 2, weights=str(tmp_path / "nope.pth"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node2", "--config", str(cfg)],
                       env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Weights file not found" in r.stdout


def test_cli_gpt2_tiny_gloo(tmp_path):
    cfg = _cfg(tmp_path, "gloo", 2, model="gpt2-tiny", weights="synthetic:1", seq_len=12, decode_steps=3)
    img = tmp_path / "none.png"
    r0, outs = _run_nodes(cfg, 2, img, extra0=("--prompt", "1,2,3,4,5"))
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:]
    toks = json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0])
    # golden greedy decode
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import build_golden_stage
    s = build_golden_stage("gpt2-tiny", 0, 3, True, True)
    s.load_state_dict(ckpt.random_stage_state_dict("gpt2-tiny", 0, 3, True, True, 1))
    seq = torch.tensor([[1, 2, 3, 4, 5]])
    ref = []
    with torch.no_grad():
        for _ in range(3):
            nid = s(seq)[:, -1].argmax(-1)
            ref.append(int(nid))
            seq = torch.cat([seq, nid[:, None]], 1)
    assert toks[0] == ref


def _launch(cfg, *extra, timeout=240):
    return subprocess.run([sys.executable, "-m", "distributed_neural_networks_amd.tools.launch", "--config", str(cfg),
                           "--timeout", "200", *extra], env=ENV, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT)


def test_cli_replicas_cifar_gloo(cifar_setup):
    """Data-parallel copies of the pipeline from the CLI (config ``replicas`` 2 x
    2 stages = 4 gloo ranks, tools/launch.py): replica k serves requests k, k+2,
    ...; every prediction equals the golden one."""
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "gloo", 2, weights=str(ck), replicas=2)
    r = _launch(cfg, "--input_image", str(img), "--num_requests", "3")
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    gold = _golden_pred(str(ck), str(img))
    lines = [l for l in out.splitlines() if "***** FINAL PREDICTION (Index):" in l]
    assert sorted("(replica 1)" in l for l in lines) == [False, False, True], lines
    assert all(_final_pred(l) == gold for l in lines)
    assert "rank 3/4 ready" in out


def test_cli_replicas_gpt2_tiny_gloo(tmp_path):
    """Two data-parallel decode rings (gpt2-tiny, 2 stages each, 4 gloo ranks):
    both generate the golden greedy tokens of the shared prompt."""
    cfg = _cfg(tmp_path, "gloo", 2, model="gpt2-tiny", weights="synthetic:1", seq_len=12, decode_steps=3, replicas=2)
    r = _launch(cfg, "--prompt", "1,2,3,4,5")
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    gen = [json.loads(l.split("generated tokens:")[1].strip()) for l in out.splitlines() if "generated tokens:" in l]
    assert len(gen) == 2, out[-3000:]
    assert "replica 1" in out
    assert gen[0] == gen[1]


def test_config_replicas_validation(tmp_path):
    from distributed_neural_networks_amd.config import ConfigError, load_node
    bad = _cfg(tmp_path, "grpc", 2, weights="x.pth", replicas=2)
    with pytest.raises(ConfigError, match="replicas"):
        load_node(str(bad), "node1")
    good = _cfg(tmp_path, "gloo", 3, weights="x.pth", replicas=2)
    ctx = load_node(str(good), "node2", replica=1)
    assert (ctx.rank, ctx.world, ctx.peer(0), ctx.peer(2)) == (4, 6, 3, 5)
    with pytest.raises(ConfigError, match="replica"):
        load_node(str(good), "node2", replica=2)


def _worker_stream(rank, world, port, q):
    os.environ["DNN_DEBUG_ORDER"] = "1"  # slot-ordering checks on (runtime/ordering.py)
    import torch.distributed as dist
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import cifar
    from distributed_neural_networks_amd.parallel import comm
    from distributed_neural_networks_amd.parallel.links import P2PLink
    from distributed_neural_networks_amd.runtime.scheduler import run_gpipe
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    torch.set_num_threads(1)
    info = comm.init("gloo", rank=rank, world=world, master_addr="127.0.0.1", master_port=port)
    ranges = cifar.stage_ranges(world)
    a, b = ranges[rank]
    sd = ckpt.random_stage_state_dict("cifar10", a, b, rank == 0, rank == world - 1, 4)
    st = TorchStage("cifar10", sd, a, b, rank == 0, rank == world - 1)
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(3, 3, 32, 32, generator=g) for _ in range(5)]
    res = {}
    prev = P2PLink(rank - 1, info.device) if rank > 0 else None
    nxt = P2PLink(rank + 1, info.device) if rank < world - 1 else None
    run_gpipe(st, 5, 3, prev, nxt, source=lambda i: xs[i],
                     sink=(lambda i, y: res.__setitem__(i, y.probs.clone())) if rank == world - 1 else None, depth=2)
    if rank == world - 1:
        q.put({i: v.numpy() for i, v in res.items()})
    comm.shutdown()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_stream_schedule_gloo(world):
    import torch.multiprocessing as mp
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_worker_stream, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    out = q.get(timeout=120)
    for p in ps:
        p.join(60)
    m = NeuralNetwork().eval()
    m.load_state_dict(ckpt.random_stage_state_dict("cifar10", 0, 3, True, True, 4))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for i in range(5):
            x = torch.randn(3, 3, 32, 32, generator=g)
            assert torch.allclose(torch.from_numpy(out[i]), m(x), atol=1e-5)


def _bench_cpu(n, *extra, timeout=420, launcher="torchrun", gpus=None):
    args = [os.path.join(ROOT, "bench.py"), "--gpus", str(gpus or n), "--cpu", "--batch", "16", "--steps", "2",
            "--warmup", "1", "--microbatches", "2", "--latency_iters", "3", *extra]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), *args]
    else:  # exactly as the driver invokes it: no launcher, bench.py spawns its own ranks
        cmd = [sys.executable, *args]
    env = dict(ENV, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]  # rank 0 prints exactly one line
    return json.loads(lines[-1])


@pytest.mark.parametrize("n,launcher", [(2, "torchrun"), (4, "self"), (8, "torchrun")])
def test_bench_pp2_schedule_cpu(n, launcher):
    """bench.py's N > 1 headline with gloo on CPU (the driver's N = 2/4/8
    scaling runs use the same schedule over RCCL): the reference cut and
    metric at every N, a real p50 through the hop and back, and the extra
    keys of BASELINE configs 3-5 (decode rings with per-token p50).  N = 4
    runs as the driver launches it, ``python bench.py --gpus 4`` with no
    launcher: bench.py must spawn the 4 ranks itself."""
    d = _bench_cpu(n, "--full", launcher=launcher)
    assert d["n_gpus"] == n and d["value"] > 0 and d["metric"] == "images/sec CIFAR-10 2-stage"
    assert d["dtype"].startswith("fp32") and "schedule test" in d["dtype"] and d["scaling"] == "weak"
    assert d["config"]["stage_cut"] == "conv|fc (reference split, 16 KiB/img hop)"
    assert d["config"]["receiver_fill_images_per_step"] == 0
    assert d["config"]["p2p"] == "gloo"  # native RCCL preflight applies to nccl runs only
    assert d["config"]["parallelism"].startswith(f"pp2-gloo-cpu-{n // 2}x{n // 2}")
    # every phase's seconds, inside the run's budget
    ph = d["phase_s"]
    assert {"startup_s", "init_s", "headline_s", "hop_s", "fc1cut_s", "gpt2_4stage_s", "total_s"} <= set(ph), ph
    assert ph["total_s"] < d["time_budget_s"]
    assert d["config"]["global_batch"] == (n // 2) * 16
    assert set(d["config"]) >= {"model", "global_batch", "seq_len", "parallelism"}
    assert d["p50_latency_ms"] is not None and d["p50_latency_ms"] > 0
    # the hop on its own (what bounds the reference cut at N >= 2)
    assert "hop_GBps_error" not in d and d["hop_GBps_per_pair"] > 0
    assert d["hop_bound_images_per_s"] == pytest.approx((n // 2) * d["hop_GBps_per_pair"] * 1e9 / 16384, rel=0.02)
    assert "extras_error" not in d and d["fc1cut_images_per_s"] > 0
    # the answer that crossed the hops: every stage-0 rank's
    # images through the distributed pipeline and back, against fp32 torch
    assert "dist_verify_error" not in d, d.get("dist_verify_error")
    assert d["dist_argmax_agreement_vs_fp32_torch"] == 1.0
    assert d["dist_pred_is_argmax_of_returned_probs"] == 1.0
    assert d["dist_max_abs_dprob"] < 1e-5
    assert d["dist_verify_images"] == (n // 2) * 256
    for key, groups in (("gpt2_4stage", min(n, 4)), ("llama3_8b_8stage_b32", min(n, 4)),
                        ("gpt2xl_fp8_8stage_b64", min(n, 4))):
        assert key + "_error" not in d, d.get(key + "_error")
        assert d[key + "_decode_tok_s"] > 0 and d[key + "_prefill_tok_s"] > 0
        assert d[key + "_p50_token_ms"] > 0
        assert d[key + "_config"]["gpu_groups"] == groups
        # the ring's greedy tokens vs the same stages colocated on rank 0
        assert d[key + "_dist_token_agreement_vs_colocated"] == 1.0, key
        assert d[key + "_dist_verify_tokens"] == 8 * d[key + "_config"]["global_batch"] // d[key + "_config"]["replicas"]


def test_bench_verify_sees_a_bad_hop_cpu(monkeypatch):
    """The distributed checks are not vacuous: with the stage-1 input of the
    check corrupted (every 7th row negated) and the ring's prompts changed for
    one microbatch, the keys fall below 1."""
    monkeypatch.setitem(ENV, "DNN_TEST_CORRUPT_VERIFY", "1")
    d = _bench_cpu(2, "--full", "--no_extra")
    assert d["dist_argmax_agreement_vs_fp32_torch"] < 1.0
    assert d["dist_max_abs_dprob"] > 1e-3
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench", "gpt_bench.py"), "--gpus", "2",
           "--cpu", "--model", "gpt2-tiny", "--stages", "2", "--batch", "2", "--prompt", "8", "--steps", "2",
           "--warmup", "1", "--prefill_iters", "1"]
    r = subprocess.run(cmd, env=dict(ENV, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    g = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert g["dist_token_agreement_vs_colocated"] < 1.0


def test_bench_gpus_must_match_world():
    """Under a launcher, --gpus that disagrees with WORLD_SIZE is an error,
    never a silently mislabelled number."""
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "4", "--cpu",
           "--batch", "16", "--steps", "1", "--warmup", "1", "--no_extra"]
    r = subprocess.run(cmd, env=dict(ENV, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--gpus 4 but the job has 2 rank(s)" in r.stdout + r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_self_launch_failing_rank_fails_job():
    """A self-launched job whose ranks fail (pp2 needs an even GPU count)
    exits non-zero and prints no result line."""
    env = {k: v for k, v in ENV.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--cpu", "--batch", "16",
                        "--steps", "1", "--warmup", "1", "--no_extra", "--launch_timeout", "120"],
                       env=dict(env, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=180)
    assert r.returncode != 0
    assert "even GPU count" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_self_launch_timeout_kills_ranks(tmp_path):
    """The launcher's wall-clock limit ends a hung job with 124 and leaves no rank behind."""
    from distributed_neural_networks_amd.parallel import selflaunch
    script = tmp_path / "hang.py"
    pidfile = tmp_path / "pids"
    script.write_text("import os, time\n"
                      f"open({str(pidfile)!r}, 'a').write(str(os.getpid()) + '\\n')\n"
                      "time.sleep(600)\n")
    rc = selflaunch.spawn_ranks(2, str(script), [], timeout_s=3)
    assert rc == 124
    pids = [int(x) for x in pidfile.read_text().split()]
    assert len(pids) == 2
    for p in pids:
        with pytest.raises(ProcessLookupError):
            os.kill(p, 0)


@pytest.mark.parametrize("placement,n,fill", [("fc1cut", 4, 8), ("interleaved", 2, 0)])
def test_bench_other_placements_cpu(placement, n, fill):
    """The opt-in placements: the fc1 cut with replicated stage 0 and receiver
    fill, and the all-to-all interleaved variant."""
    d = _bench_cpu(n, "--placement", placement, "--fill_rows", str(fill), "--no_extra")
    assert d["n_gpus"] == n and d["value"] > 0 and d["metric"] == "images/sec CIFAR-10 2-stage"
    if placement == "fc1cut":
        from distributed_neural_networks_amd.parallel.partition import linear_plan
        plan = linear_plan(n, "fp32", cuts=(2,))
        assert d["config"]["parallelism"] == f"pp2-fc1cut-{plan['n0']}x{plan['n1']}+fill"
        assert d["config"]["global_batch"] == plan["n0"] * 16 + plan["n1"] * fill * 2
        assert d["config"]["receiver_fill_images_per_step"] == plan["n1"] * fill * 2


def test_bench_plain_run_dumps_outputs_cpu(tmp_path):
    """A plain run (no ``--full``) measures the headline only, and
    ``--dump-outputs`` writes what the last timed step's stage-1 rank computed:
    the fp32 model's probabilities and predictions of rank 0's seeded images."""
    import numpy as np
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    d = _bench_cpu(2, "--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "images/s"
    assert d["value"] == pytest.approx(16 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["p50_latency_ms"] is None
    assert not [k for k in d if k.startswith(("dist_", "hop_", "fc1cut_", "gpt2", "llama3"))], sorted(d)
    assert sorted(os.listdir(tmp_path / "out")) == ["pred_rank1.npy", "probs_rank1.npy"]
    probs, pred = np.load(tmp_path / "out" / "probs_rank1.npy"), np.load(tmp_path / "out" / "pred_rank1.npy")
    assert probs.dtype == np.float32 and probs.shape == (16, 10) and pred.dtype == np.float32 and pred.shape == (16,)
    g = torch.Generator().manual_seed(1)  # bench_pp2: rank r draws its images from seed 1 + r
    x = torch.cat([torch.randn((8, 3, 32, 32), generator=g) for _ in range(2)])
    m = NeuralNetwork().eval()
    m.load_state_dict(ckpt.random_stage_state_dict("cifar10", 0, 3, True, True, 0))
    with torch.no_grad():
        want = m(x)
    assert np.abs(probs - want.numpy()).max() < 1e-5
    assert (pred == probs.argmax(1)).all()


@pytest.mark.parametrize("n", [4, 8])
def test_gpt_decode_ring_bench_cpu(n):
    """bench/gpt_bench.py's microbatched decode ring over n gloo ranks (4
    stage groups; 8 ranks = 2 replicas of the 4-stage ring)."""
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench", "gpt_bench.py"), "--gpus", str(n),
           "--cpu", "--model", "gpt2-tiny", "--stages", "4", "--batch", "2", "--prompt", "8", "--steps", "4",
           "--warmup", "1", "--prefill_iters", "1"]
    env = dict(ENV, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == n and d["value"] > 0
    assert d["config"]["gpu_groups"] == 4 and d["config"]["replicas"] == n // 4
    assert d["config"]["microbatches"] == 4
    assert d["decode_p50_token_latency_ms"] > 0
    assert d["dist_token_agreement_vs_colocated"] == 1.0 and d["dist_first_token_agreement_vs_colocated"] == 1.0


# ----------------------------------------------------------------------------- failure detection
def test_health_barrier_timeout(cifar_setup):
    """Stage 0 refuses to start when a downstream stage never becomes healthy
    (the reference would sleep 2 s and then fail inside the RPC)."""
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "grpc", 2, weights=str(ck), health_timeout_s=2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--input_image", str(img)], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "did not become healthy" in r.stdout


def test_downstream_stage_killed_midrun(cifar_setup):
    """Kill the last stage while stage 0 is streaming requests: stage 0 must
    report the failed RPCs and exit non-zero instead of hanging."""
    import time
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "grpc", 2, weights=str(ck), rpc_timeout_s=5)
    p2 = subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node2", "--config", str(cfg),
                           "--serve_seconds", "120", "--quiet"], env=ENV, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    p1 = subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                           "--input_image", str(img), "--num_requests", "100000"], env=ENV, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True)
    try:
        deadline = time.time() + 120
        seen = ""
        while time.time() < deadline:  # wait until requests flow
            line = p1.stdout.readline()
            seen += line
            if "FINAL PREDICTION" in line:
                break
        assert "FINAL PREDICTION" in seen
        p2.kill()
        p2.wait()
        # stage 0 keeps going but every request now fails -> bounded; stop it and check it saw failures
        out = ""
        t_end = time.time() + 30
        while time.time() < t_end:
            line = p1.stdout.readline()
            out += line
            if "SendTensor RPC failed" in line or "Error forwarding" in line or "tensor not included" in line:
                break
        assert ("SendTensor RPC failed" in out) or ("tensor not included" in out), out[-2000:]
    finally:
        for p in (p1, p2):
            if p.poll() is None:
                p.kill()
                p.wait()


def test_trace_and_metrics(cifar_setup, tmp_path):
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "grpc", 2, weights=str(ck))
    tr = tmp_path / "node2_trace.json"
    p2 = subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node2", "--config", str(cfg),
                           "--serve_seconds", "90", "--trace", str(tr), "--metrics"], env=ENV,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                         "--input_image", str(img), "--num_requests", "3", "--shutdown_pipeline"], env=ENV,
                        capture_output=True, text=True, timeout=120)
    out2 = p2.communicate(timeout=60)[0]
    assert r0.returncode == 0
    line = [l for l in out2.splitlines() if l.startswith("METRICS ")][0]
    m = json.loads(line[len("METRICS "):])
    assert m["requests"] == 3 and m["latency_ms_p50"] > 0
    ev = json.load(open(tr))["traceEvents"]
    assert sum(1 for e in ev if e["name"] == "SendTensor.forward") == 3


def test_cli_gloo_many_microbatches(cifar_setup):
    """2-stage CIFAR stream with 8 microbatches per request over gloo: the
    last stage's back-edge sends never stall its forward stream (one slot per
    microbatch, the return rank's receives are posted up front on the
    back-edge communicator), so M >= 6 no longer deadlocks."""
    tmp, ck, img = cifar_setup
    cfg = _cfg(tmp, "gloo", 2, weights=str(ck), micro_batch_size=2, num_microbatches=8)
    r0, outs = _run_nodes(cfg, 2, img, extra0=("--num_requests", "2"))
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-3000:]
    lines = [l for l in r0.stdout.splitlines() if "***** FINAL PREDICTION (Index):" in l]
    assert len(lines) == 2
    from distributed_neural_networks_amd.cli import cifar_request
    from distributed_neural_networks_amd.models.cifar import NeuralNetwork
    m = NeuralNetwork().eval()
    m.load_state_dict(torch.load(str(ck), weights_only=True))

    class A:
        input_image = str(img)
    for req, line in enumerate(lines):  # every row that crossed the hop and came back
        preds = json.loads(line.split("(Index):")[1].split("*****")[0].strip())
        with torch.no_grad():
            assert preds == m(cifar_request(A, "t", 16, req)).argmax(1).tolist()
    assert json.loads(lines[0].split("(Index):")[1].split("*****")[0].strip())[0] == _golden_pred(str(ck), str(img))


def test_cli_gloo_stage_build_failure_aborts_peers(cifar_setup):
    """A rank that fails while building its stage (here: fc weights missing
    from the checkpoint, so only stage 1 fails) publishes the abort; stage 0
    exits non-zero within the heartbeat timeout instead of waiting in the
    first barrier for comm_timeout_s."""
    import time
    tmp, ck, img = cifar_setup
    sd = torch.load(str(ck), weights_only=True)
    for k in [k for k in sd if k.startswith("fc")]:
        del sd[k]
    bad = tmp / "no_fc.pth"
    torch.save(sd, str(bad))
    cfg = _cfg(tmp, "gloo", 2, weights=str(bad), heartbeat_timeout_s=5, comm_timeout_s=120)
    t0 = time.time()
    r0, outs = _run_nodes(cfg, 2, img, timeout=100)
    assert r0.returncode != 0
    assert time.time() - t0 < 60
    assert "pipeline failure" in (r0.stdout + "".join(outs))
