"""Per-token log-probabilities and top-n alternatives: the config key, the
torch mirror of the device kernel (runtime/sampling.py logprobs_ref), the CPU /
gloo generation paths (``TorchStage`` on the decode ring), and the fp32
preconditions of the exact fixtures that tests/test_logprobs_gpu.py runs."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import apply_penalties_ref, logprobs_ref, penalty_count, \
    penalty_state, pick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
NINF = float("-inf")


# ---------------------------------------------------------------------- config
def _cfg(**kw):
    d = {"nodes": [{"id": "a", "address": "127.0.0.1:1", "part_index": 0}], "model_weights": "synthetic:0",
         "num_parts": 1, "model": "gpt2-tiny"}
    d.update(kw)
    return d


def test_config_key():
    from distributed_neural_networks_amd.config import ConfigError, load_json, parse_pipeline
    assert parse_pipeline(_cfg()).logprobs == 0
    assert parse_pipeline(_cfg(logprobs=0)).logprobs == 0
    for n in (1, 5, 20):
        p = parse_pipeline(_cfg(logprobs=n))
        assert p.logprobs == n and isinstance(p.logprobs, int)
    for v in (-1, 21, 2.5, 1.0, True, "3", None):
        with pytest.raises(ConfigError, match=r"'logprobs' must be an integer in \[0, 20\]"):
            parse_pipeline(_cfg(logprobs=v))
    with pytest.raises(ConfigError, match="exists for the generating models only"):
        parse_pipeline(_cfg(model="cifar10", logprobs=3))
    assert parse_pipeline(_cfg(model="cifar10", logprobs=0)).logprobs == 0
    path = os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_logprobs.json")
    p = parse_pipeline(load_json(path), path)
    assert p.logprobs == 5
    q = parse_pipeline(load_json(os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_sampled.json")))
    assert q.logprobs == 0
    for key in ("temperature", "top_k", "top_p", "seed", "model", "num_parts", "decode_steps", "micro_batch_size"):
        assert getattr(p, key) == getattr(q, key)  # the sampled config plus the one key


# ---------------------------------------------------------------------- the mirror
def test_mirror_against_log_softmax_and_topk():
    """Rows without ties: fp64 log_softmax of the bf16 values, torch.topk's order."""
    g = torch.Generator().manual_seed(3)
    M, N = 4, 300
    # distinct bf16 values per row: a shuffled arithmetic progression (step 1/16 up to 18.75: exact in bf16)
    x = torch.stack([(torch.randperm(N, generator=g).float() / 16 - 9) for _ in range(M)]).bfloat16()
    assert all(len(set(r.tolist())) == N for r in x.float())
    tok = torch.tensor([0, N - 1, 17, int(x[3].float().argmax())], dtype=torch.int32)
    for n in (0, 1, 5, 20):
        chosen, ids, lps = logprobs_ref(x, tok, n)
        assert chosen.dtype == torch.float32 and ids.dtype == torch.int32 and lps.dtype == torch.float32
        assert chosen.shape == (M,) and ids.shape == (M, n) and lps.shape == (M, n)
        lp = torch.log_softmax(x.double(), 1)
        assert torch.equal(chosen, lp[torch.arange(M), tok.long()].float())
        if n:
            tv, ti = torch.topk(x.double(), n, dim=1)
            assert torch.equal(ids.long(), ti)
            assert torch.equal(lps, lp.gather(1, ti).float())
    # fp32 logits are rounded to bf16 first: the values the device sampler reads
    xf = x.float() + 1e-4
    assert torch.equal(logprobs_ref(xf, tok, 5)[2], logprobs_ref(xf.bfloat16(), tok, 5)[2])
    # the probabilities of a whole row sum to one
    assert abs(float(torch.exp(logprobs_ref(x[:1, :20], tok[:1], 20)[2].double()).sum()) - 1.0) < 1e-6
    for bad in (-1, 21):
        with pytest.raises(ValueError, match="logprobs: n ="):
            logprobs_ref(x, tok, bad)
    with pytest.raises(ValueError, match="logprobs: n ="):
        logprobs_ref(x[:, :10], tok.clamp(max=9), 11)  # more alternatives than entries


def test_mirror_tie_rule():
    """A few distinct bf16 values: equal values come in ascending index order."""
    x = torch.tensor([[1.0, 3.0, 2.0, 3.0, 1.0, 3.0, 2.0, 0.5],
                      [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]).bfloat16()
    chosen, ids, lps = logprobs_ref(x, torch.tensor([3, 7], dtype=torch.int32), 7)
    assert ids.tolist() == [[1, 3, 5, 2, 6, 0, 4], [0, 1, 2, 3, 4, 5, 6]]
    assert torch.equal(lps[0, 0], lps[0, 2]) and torch.equal(lps[0, 3], lps[0, 4]) and lps[0, 2] > lps[0, 3]
    assert torch.equal(chosen[0], lps[0, 0])  # the chosen token is one of the tied maxima
    assert abs(float(chosen[1]) + math.log(8)) < 1e-7 and bool((lps[1] == chosen[1]).all())


def test_mirror_orders_by_the_bf16_bits():
    """The order is the one of the device's 16-bit key of the bf16 bits: +0.0
    and -0.0 are equal as values (and have equal log-probabilities) but +0.0
    comes first, each kind in ascending index order."""
    x = torch.tensor([[-0.0, 0.0, -1.0, -0.0, 0.0, 1.0]]).bfloat16()
    chosen, ids, lps = logprobs_ref(x, torch.tensor([0], dtype=torch.int32), 6)
    assert ids.tolist() == [[5, 1, 4, 0, 3, 2]]
    assert bool((lps[0, 1:5] == lps[0, 1]).all()) and torch.equal(chosen[0], lps[0, 1])


def test_mirror_minus_inf_entries():
    x = torch.tensor([[NINF, 2.0, NINF, 1.0, NINF]]).bfloat16()
    chosen, ids, lps = logprobs_ref(x, torch.tensor([2], dtype=torch.int32), 5)
    assert ids.tolist() == [[1, 3, 0, 2, 4]]  # -inf last, among themselves by index
    assert float(chosen[0]) == NINF and lps[0, 2:].tolist() == [NINF] * 3
    lse = math.log(math.exp(2) + math.exp(1))
    assert abs(float(lps[0, 0]) - (2 - lse)) < 1e-6 and abs(float(lps[0, 1]) - (1 - lse)) < 1e-6


# ---------------------------------------------------------------------- exact-fixture preconditions
def test_exact_fixture_preconditions_fp32():
    """The one-hot rows of test_logprobs_gpu.py: one entry a = 8, every other an
    integer in [-150, -121].  In fp32 exp(x - a) is exactly 0 (e^-129 is below
    the smallest denormal 2^-149 = e^-103.3), so the sum is exactly 1, its log
    exactly 0, and lp is x - a with no rounding: integers of magnitude < 2^24,
    exact in bf16 (8 significant bits suffice for [-150, -121]: checked) too."""
    a = torch.tensor(8.0)
    others = torch.arange(-150, -120, dtype=torch.float32)
    assert torch.equal(others.bfloat16().float(), others)  # bf16 holds them exactly
    assert bool((torch.exp(others - a) == 0).all())
    assert float(torch.exp(a - a)) == 1.0 and float(torch.log(torch.tensor(1.0))) == 0.0
    # a chunk without the one-hot entry: its own sum s >= 1 scaled by exp(m - a) = 0 adds exactly 0
    m = others.max()
    s = torch.exp(others - m).sum()
    assert float(s) >= 1.0 and float(s * torch.exp(m - a)) == 0.0
    # lp = (x - a) - 0 exactly, and 0 for the maximum; the mirror (fp64, rounded to fp32) agrees bit for bit
    x = torch.cat([others[:7], a[None], others[7:]])[None].bfloat16()
    chosen, ids, lps = logprobs_ref(x, torch.tensor([7], dtype=torch.int32), 5)
    assert float(chosen[0]) == 0.0 and not math.copysign(1.0, float(chosen[0])) < 0
    want = (x[0].float() - a)
    assert torch.equal(lps[0], want[ids[0].long()])
    assert ids[0].tolist() == [7, 30, 29, 28, 27]  # -121, -122, ... follow the maximum


# ---------------------------------------------------------------------- TorchStage on the ring vs a naive host loop
PEN = (1.3, 0.4, 0.3)  # repetition, presence, frequency


def _tiny(seed=5):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import build_golden_stage, model_info
    model = "gpt2-tiny"
    n = model_info(model).num_layers
    sd = ckpt.random_stage_state_dict(model, 0, n - 1, True, True, seed)
    gold = build_golden_stage(model, 0, n - 1, True, True)
    gold.load_state_dict(sd)
    return model, n, sd, gold.eval(), model_info(model).cfg.vocab_size


def _prompts(V, Mb, B, T, seed=4):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randint(0, V, (B, T), generator=g) for _ in range(Mb)]
    for p in ps:
        p[:, 5] = p[:, 1]
    return ps


def _naive(gold, prompt, toks, pen, V):
    """Full-prefix recompute per token, teacher-forced with the ring's tokens:
    fp64 log_softmax of every step's (penalised) logits, not rounded to bf16
    unless the penalties round them.  Returns (steps) lists of (B, V) fp64
    log-probabilities and the largest |logit| met."""
    B, T = prompt.shape
    state = penalty_state(prompt, V) if pen else None
    seq = prompt.clone()
    out, amax = [], 0.0
    with torch.no_grad():
        for j in range(toks.shape[1]):
            logits = gold(seq)[:, -1]
            if pen:
                logits = apply_penalties_ref(logits, state, pen[0], pen[2], pen[1]).float()
                state = penalty_count(state, toks[:, j])
            amax = max(amax, float(logits.abs().max()))
            out.append(torch.log_softmax(logits.double(), 1))
            seq = torch.cat([seq, toks[:, j, None].long()], 1)
    return out, amax


@pytest.mark.parametrize("pen", [(), PEN], ids=["plain", "penalised"])
@pytest.mark.parametrize("sampling", [(0.0, 0, 0, 1.0, 0.0), (0.8, 20, 7, 0.9, 0.0)], ids=["greedy", "sampled"])
def test_torch_stage_ring_against_full_prefix_loop(sampling, pen):
    """Bound: the stage rounds its logits to bf16 (what the device reads), the
    loop does not.  Rounding moves a logit by at most |x| 2^-9, the
    log-sum-exp by at most the largest such move, so a log-probability by at
    most 2 max|x| 2^-9; 1e-4 on top covers the KV-cached against the
    full-prefix fp32 forward."""
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, gold, V = _tiny()
    Mb, B, T, steps, ntop = 2, 2, 8, 6, 5
    prompts = _prompts(V, Mb, B, T)
    st = TorchStage(model, sd, 0, n - 1, True, True, sampling=sampling + (pen or (1.0, 0.0, 0.0)) + (ntop,))
    assert st.logprobs == ntop and st.penalties_on == bool(pen)
    ring = DecodeRing([st], RingLinks(), 1, Mb, B, use_graphs=False)
    toks = ring.generate(prompts, T, steps)
    lp = ring.logprobs()
    assert lp["chosen"].shape == (Mb * B, steps) and lp["chosen"].dtype == torch.float32
    assert lp["top_ids"].shape == (Mb * B, steps, ntop) and lp["top_ids"].dtype == torch.int32
    assert lp["top_lps"].shape == (Mb * B, steps, ntop) and lp["top_lps"].dtype == torch.float32
    # the key changes no token
    base = sampling + pen if pen else sampling
    plain = DecodeRing([TorchStage(model, sd, 0, n - 1, True, True, sampling=base)], RingLinks(), 1, Mb, B,
                       use_graphs=False)
    assert torch.equal(plain.generate(prompts, T, steps), toks)
    with pytest.raises(ValueError, match="records none"):
        plain.logprobs()
    for m in range(Mb):
        rows = slice(m * B, (m + 1) * B)
        want, amax = _naive(gold, prompts[m], toks[rows], pen, V)
        tol = 2 * amax * 2.0 ** -9 + 1e-4
        for j in range(steps):
            w = want[j]
            got_c = lp["chosen"][rows, j].double()
            assert float((got_c - w.gather(1, toks[rows, j, None].long())[:, 0]).abs().max()) <= tol, (m, j)
            ids = lp["top_ids"][rows, j].long()
            got_t = lp["top_lps"][rows, j].double()
            assert float((got_t - w.gather(1, ids)).abs().max()) <= tol, (m, j)
            # the top-n really is the top: descending, and nothing outside it is larger (up to the rounding)
            assert bool((got_t[:, :-1] >= got_t[:, 1:]).all())
            rest = w.clone().scatter_(1, ids, NINF)
            assert bool((rest.max(1).values <= got_t[:, -1] + tol).all())
            if sampling[0] == 0:  # greedy: the chosen token heads the list
                assert torch.equal(ids[:, 0].int(), toks[rows, j]) and torch.equal(lp["chosen"][rows, j],
                                                                                   lp["top_lps"][rows, j, 0])
    # a second generation (other prompts) starts a clean history, aligned with its own tokens
    prompts2 = _prompts(V, Mb, B, T - 2, seed=9)
    toks2 = ring.generate(prompts2, T - 2, steps - 2)
    lp2 = ring.logprobs()
    assert lp2["chosen"].shape == (Mb * B, steps - 2)
    fresh = DecodeRing([TorchStage(model, sd, 0, n - 1, True, True, sampling=sampling + (pen or (1.0, 0.0, 0.0))
                                   + (ntop,))], RingLinks(), 1, Mb, B, use_graphs=False)
    assert torch.equal(fresh.generate(prompts2, T - 2, steps - 2), toks2)
    lpf = fresh.logprobs()
    assert all(torch.equal(lp2[k], lpf[k]) for k in lp2)


def test_torch_stage_and_ring_arguments():
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, _, _ = _tiny()
    for bad in (-1, 21, 2.5, True):
        with pytest.raises(ValueError, match="logprobs must be an integer"):
            TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, bad))
    off = TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0))
    assert off.logprobs == 0
    with pytest.raises(ValueError, match="records no log-probabilities"):
        off.bind_logprobs(0, None, None, None)
    # only a last stage records
    assert TorchStage(model, sd, 0, n - 2, True, False, sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 4)).logprobs == 0
    # a stage that records needs its histories before its first sampled step
    on = TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 2))
    with pytest.raises(ValueError, match="no bind_logprobs"):
        on.step(torch.zeros((1, 3), dtype=torch.int64), 0, 1, 3)


# ---------------------------------------------------------------------- two gloo ranks vs one process
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_nodes(cfg, n, extra0=(), timeout=120, env=ENV):
    procs = []
    for i in range(1, n):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", f"node{i + 1}",
                                       "--config", str(cfg), "--serve_seconds", "90"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                             "--input_image", "none.png", "--shutdown_pipeline", *extra0], env=env,
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


def test_cli_two_gloo_ranks_equal_one_process(tmp_path):
    """The last rank prints the LOGPROBS line (with every sequence's top-n:
    DNN_LOGPROBS_ALL=1); the whole dict equals, bit for bit, what one process
    with both stages records (the line's numbers read back exactly)."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, steps, ids, ntop = "gpt2-tiny", 6, [1, 2, 3, 2, 5, 2, 7, 3], 3
    ports = [_free_port() for _ in range(2)]
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{ports[i]}", "part_index": i} for i in range(2)],
         "model_weights": "synthetic:1", "num_parts": 2, "return_to_node_id": "node1", "transport": "gloo",
         "model": model, "seq_len": 12, "decode_steps": steps, "micro_batch_size": 2, "num_microbatches": 2,
         "temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 7, "logprobs": ntop}
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r0, outs = _run_nodes(cfg, 2, extra0=("--prompt", ",".join(map(str, ids))), env=dict(ENV, DNN_LOGPROBS_ALL="1"))
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:] + "".join(o[-2000:] for o in outs)
    toks = torch.tensor(json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    assert "LOGPROBS" not in r0.stdout  # rank 0 has the tokens, the last rank the log-probabilities
    line = json.loads(outs[0].split("LOGPROBS ")[1].splitlines()[0])
    ranges = default_ranges(model, 2)
    samp = (0.8, 20, 7, 0.9, 0.0, 1.0, 0.0, 0.0, ntop)
    stages = [TorchStage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1), a, b, i == 0, i == 1,
                         sampling=samp) for i, (a, b) in enumerate(ranges)]
    ring = DecodeRing(stages, RingLinks(), 1, 2, 2, use_graphs=False)
    prompt = torch.tensor([ids]).repeat(2, 1)
    want_t = ring.generate([prompt, prompt], len(ids), steps)
    want = ring.logprobs()
    assert torch.equal(toks, want_t)
    assert line["n"] == ntop and line["top_ids_seq0"] == want["top_ids"][0].tolist()
    assert torch.equal(torch.tensor(line["chosen"], dtype=torch.float32), want["chosen"])
    assert torch.equal(torch.tensor(line["top_logprobs_seq0"], dtype=torch.float32), want["top_lps"][0])
    assert torch.equal(torch.tensor(line["top_ids"], dtype=torch.int32), want["top_ids"])
    assert torch.equal(torch.tensor(line["top_logprobs"], dtype=torch.float32), want["top_lps"])
    assert bool(torch.isfinite(want["top_lps"]).all())  # no null in the line
