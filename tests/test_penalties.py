"""Repetition / presence / frequency penalties: config keys, the torch mirror
of the device kernel (runtime/sampling.py) against a plain loop, and the
CPU / gloo generation paths (``TorchStage`` on the decode ring)."""
import json
import os
import struct
import subprocess
import sys

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import (apply_penalties_ref, penalty_count, penalty_state, pick)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


# ---------------------------------------------------------------------- config
def _cfg(**kw):
    d = {"nodes": [{"id": "a", "address": "127.0.0.1:1", "part_index": 0}], "model_weights": "synthetic:0",
         "num_parts": 1, "model": "gpt2-tiny"}
    d.update(kw)
    return d


def test_config_keys():
    from distributed_neural_networks_amd.config import ConfigError, load_json, parse_pipeline
    p = parse_pipeline(_cfg())
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.0, 0.0, 0.0)
    p = parse_pipeline(_cfg(repetition_penalty=1.3, presence_penalty=-0.5, frequency_penalty=2))
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.3, -0.5, 2.0)
    assert isinstance(p.frequency_penalty, float)
    for v in (0, -1, True, "x", float("nan"), float("inf")):
        with pytest.raises(ConfigError, match="'repetition_penalty' must be a finite number > 0"):
            parse_pipeline(_cfg(repetition_penalty=v))
    for key in ("presence_penalty", "frequency_penalty"):
        for v in (True, "x", float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ConfigError, match=f"'{key}' must be a finite number"):
                parse_pipeline(_cfg(**{key: v}))
        assert getattr(parse_pipeline(_cfg(**{key: -1})), key) == -1.0  # negative values reward repetition: valid
    # json.load accepts the NaN / Infinity literals: they are rejected all the same
    for text in ("NaN", "Infinity"):
        with pytest.raises(ConfigError, match="repetition_penalty"):
            parse_pipeline(json.loads(json.dumps(_cfg()).replace('"num_parts"', f'"repetition_penalty": {text}, '
                                                                                f'"num_parts"')))
    path = os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_penalised.json")
    p = parse_pipeline(load_json(path), path)
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.25, 0.0, 0.25)
    assert (p.temperature, p.top_k, p.top_p, p.seed, p.model, p.num_parts) == (0.8, 50, 0.95, 1, "gpt2", 4)


def test_config_rejects_penalties_for_cifar():
    from distributed_neural_networks_amd.config import ConfigError, parse_pipeline
    for kw in ({"repetition_penalty": 1.2}, {"presence_penalty": 0.5}, {"frequency_penalty": -0.25}):
        with pytest.raises(ConfigError, match="exists for the generating models only"):
            parse_pipeline(_cfg(model="cifar10", **kw))
    p = parse_pipeline(_cfg(model="cifar10", repetition_penalty=1, presence_penalty=0.0, frequency_penalty=0))
    assert p.repetition_penalty == 1.0  # the neutral values are no penalty


# ---------------------------------------------------------------------- mirror vs a plain loop
def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite values and infinities)."""
    u = struct.unpack("I", struct.pack("f", x))[0]
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def _loop(bits, state, rep, freq, pres):
    """The rule of the issue on bf16 bit patterns, one entry at a time; every
    fp32 operation is rounded on its own (``_f32`` after each)."""
    rep, freq, pres = _f32(rep), _f32(freq), _f32(pres)
    out = [row[:] for row in bits]
    for r, row in enumerate(bits):
        for i, b in enumerate(row):
            c = state[r][i] & 0xFFFF
            g = c & 0x7FFF
            if c == 0:
                continue
            x = struct.unpack("f", struct.pack("I", b << 16))[0]
            if rep != 1.0:
                x = _f32(x / rep) if x > 0 else _f32(x * rep)
            if g > 0:
                x = _f32(x - _f32(freq * float(g)))
                x = _f32(x - pres)
            out[r][i] = _bf16_bits(x)
    return out


def _example():
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(3, 40, generator=g) * 3).bfloat16()
    st = torch.zeros(3, 40, dtype=torch.int64)
    st[0, 3] = 0x8000            # prompt only
    st[0, 7] = 2                 # generated only
    st[0, 11] = 0x8000 | 5       # both
    st[0, 0] = 1
    st[0, 39] = 0x8000
    x[0, 13] = 0.0
    st[0, 13] = 0x8000 | 1       # a zero logit
    x[0, 14] = -0.0
    st[0, 14] = 0x8000
    x[0, 17] = -2.5
    st[0, 17] = 3                # a negative logit
    x[0, 19] = 1.7
    st[0, 19] = 0x7FFF           # g saturated
    x[0, 21] = float("inf")
    st[0, 21] = 0x8000
    st[1, 5] = 0xFFFF            # P with g saturated
    x[1, 6] = -7.25
    st[1, 6] = 0x8000
    # row 2 stays unseen
    st16 = torch.where(st >= 0x8000, st - 0x10000, st).to(torch.int16)
    return x, st, st16


@pytest.mark.parametrize("rep,freq,pres", [(2.0, 0.25, 0.5), (0.5, -0.5, 0.0), (1.3, 0.37, 0.21), (1.0, 0.37, 0.0),
                                           (1.3, 0.0, 0.0)])
def test_mirror_equals_plain_loop(rep, freq, pres):
    x, st, st16 = _example()
    bits = (x.view(torch.int16).to(torch.int64) & 0xFFFF).tolist()
    want = torch.tensor(_loop(bits, st.tolist(), rep, freq, pres), dtype=torch.int64)
    got = apply_penalties_ref(x, st16, rep, freq, pres)
    assert got.dtype == torch.bfloat16
    gb = got.view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(gb, want)
    # unseen entries keep their bits, the unseen row as a whole; seen ones moved
    xb = x.view(torch.int16).to(torch.int64) & 0xFFFF
    assert torch.equal(gb[st == 0], xb[st == 0]) and torch.equal(gb[2], xb[2])
    assert int((gb != xb).sum()) >= 5  # at least the generated tokens' logits (seven of them) mostly moved
    assert int(gb[0, 14]) == 0x8000  # -0.0 stays -0.0 under the repetition penalty alone
    if rep != 1.0:
        assert int(gb[0, 21]) == 0x7F80  # +inf stays +inf
    # the uint16 view of the same state gives the same result
    assert torch.equal(apply_penalties_ref(x, st16.view(torch.uint16), rep, freq, pres), got)


def test_state_and_count():
    ids = torch.tensor([[1, 5, 5, 9], [0, 39, 2, 2]])
    st = penalty_state(ids, 40)
    assert st.dtype == torch.int16 and st.shape == (2, 40)
    u = st.to(torch.int64) & 0xFFFF
    assert u[0].nonzero().flatten().tolist() == [1, 5, 9] and u[1].nonzero().flatten().tolist() == [0, 2, 39]
    assert bool((u[u != 0] == 0x8000).all())
    st2 = penalty_count(st, torch.tensor([5, 7], dtype=torch.int32))
    u2 = st2.to(torch.int64) & 0xFFFF
    assert int(u2[0, 5]) == 0x8001 and int(u2[1, 7]) == 1  # P kept; a fresh token starts at 1
    assert torch.equal(st, penalty_state(ids, 40))  # a new state: the argument is not touched
    sat = st2.clone()
    sat[0, 5] = -1          # 0xFFFF: P and g = 0x7FFF
    sat[1, 7] = 0x7FFF
    st3 = penalty_count(sat, torch.tensor([5, 7]))
    assert torch.equal(st3, sat)  # saturated: stays
    st4 = penalty_count(st2, torch.tensor([-1, 40]))
    assert torch.equal(st4, st2)  # out of range: ignored


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
        p[:, 5] = p[:, 1]  # a repeated token in every row
        p[:, 6] = p[:, 1]
    return ps


def _naive(gold, prompt, steps, sampling, pen, V, first_step=0):
    """Full-prefix recompute per token; the mirror applied to the last position.
    The draw is seeded by the tokens cached before the call: ``first_step`` for
    the prompt's token (0, or where a chunked prefill's last piece starts)."""
    temperature, top_k, seed, top_p, min_p = sampling
    rep, pres, freq = pen
    B, T = prompt.shape
    state = penalty_state(prompt, V)
    seq = prompt.clone()
    toks = []
    with torch.no_grad():
        for j in range(steps):
            logits = gold(seq)[:, -1]
            x = apply_penalties_ref(logits, state, rep, freq, pres)
            step = torch.full((B,), first_step if j == 0 else T + j - 1, dtype=torch.int32)  # tokens cached before the call
            tok = pick(x, temperature, top_k, seed, step, top_p=top_p, min_p=min_p).to(torch.int32)
            state = penalty_count(state, tok)
            toks.append(tok)
            seq = torch.cat([seq, tok[:, None].long()], 1)
    return torch.stack(toks, 1)


@pytest.mark.parametrize("sampling", [(0.0, 0, 0, 1.0, 0.0), (0.8, 20, 7, 0.9, 0.0)], ids=["greedy", "sampled"])
def test_torch_stage_ring_equals_naive_loop(sampling):
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, gold, V = _tiny()
    Mb, B, T, steps = 2, 2, 8, 6
    prompts = _prompts(V, Mb, B, T)
    st = TorchStage(model, sd, 0, n - 1, True, True, sampling=sampling + PEN)
    assert st.penalties_on and (st.rep_pen, st.pres_pen, st.freq_pen) == PEN
    ring = DecodeRing([st], RingLinks(), 1, Mb, B, use_graphs=False)
    toks = ring.generate(prompts, T, steps)
    want = torch.cat([_naive(gold, p, steps, sampling, PEN, V) for p in prompts], 0)
    assert torch.equal(toks, want)
    # the penalties bite: the same ring without them generates something else
    plain = DecodeRing([TorchStage(model, sd, 0, n - 1, True, True, sampling=sampling)], RingLinks(), 1, Mb, B,
                       use_graphs=False)
    assert not plain.stages[0].penalties_on
    assert not torch.equal(plain.generate(prompts, T, steps), toks)
    # a second generation starts from the prompt again, and a chunked prefill marks the whole prompt first
    assert torch.equal(ring.generate(prompts, T, steps), want)
    for chunk, t_last in ((3, 6), (7, 7)):  # 7 + 1: a last piece of one token is decode-shaped, the piece
        # before it must leave nothing to count
        want_c = torch.cat([_naive(gold, p, steps, sampling, PEN, V, first_step=t_last) for p in prompts], 0)
        assert torch.equal(ring.generate(prompts, T, steps, chunk=chunk), want_c)


def test_torch_stage_arguments():
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, _, _ = _tiny()
    for bad in ((0.0, 0, 0, 1.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0, 0, 1.0, 0.0, -1.0, 0.0, 0.0),
                (0.0, 0, 0, 1.0, 0.0, 1.0, float("nan"), 0.0), (0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, float("inf")),
                (0.0, 0, 0, 1.0)):
        with pytest.raises(ValueError):
            TorchStage(model, sd, 0, n - 1, True, True, sampling=bad)
    assert not TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0)).penalties_on
    assert not TorchStage(model, sd, 0, n - 2, True, False, sampling=(0.0, 0, 0, 1.0, 0.0) + PEN).penalties_on


def test_ring_needs_the_prompt_ids_flag():
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, _, _ = _tiny()
    from distributed_neural_networks_amd import checkpoint as ckpt
    sd1 = ckpt.random_stage_state_dict(model, n // 2, n - 1, False, True, 5)
    last = TorchStage(model, sd1, n // 2, n - 1, False, True, sampling=(0.0, 0, 0, 1.0, 0.0) + PEN)
    with pytest.raises(ValueError, match="forward_prompt_ids"):
        DecodeRing([last], RingLinks(), 2, 1, 2, use_graphs=False)


# ---------------------------------------------------------------------- two gloo ranks vs colocated
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_nodes(cfg, n, extra0=(), timeout=120):
    procs = []
    for i in range(1, n):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", f"node{i + 1}",
                                       "--config", str(cfg), "--serve_seconds", "90"], env=ENV,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                             "--input_image", "none.png", "--shutdown_pipeline", *extra0], env=ENV,
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


@pytest.mark.parametrize("sampling", [{}, {"temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 7}],
                         ids=["greedy", "sampled"])
def test_cli_two_gloo_ranks_equal_colocated(tmp_path, sampling):
    """The prompt ids reach the last rank: two gloo ranks with penalties generate
    what one process with both stages generates."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, steps, ids = "gpt2-tiny", 6, [1, 2, 3, 2, 5, 2, 7, 3]
    ports = [_free_port() for _ in range(2)]
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{ports[i]}", "part_index": i} for i in range(2)],
         "model_weights": "synthetic:1", "num_parts": 2, "return_to_node_id": "node1", "transport": "gloo",
         "model": model, "seq_len": 12, "decode_steps": steps, "micro_batch_size": 2, "num_microbatches": 2,
         "repetition_penalty": PEN[0], "presence_penalty": PEN[1], "frequency_penalty": PEN[2]}
    c.update(sampling)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r0, outs = _run_nodes(cfg, 2, extra0=("--prompt", ",".join(map(str, ids))))
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:] + "".join(o[-2000:] for o in outs)
    toks = torch.tensor(json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    n = model_info(model).num_layers
    from distributed_neural_networks_amd.models import default_ranges
    ranges = default_ranges(model, 2)
    samp = (c.get("temperature", 0.0), c.get("top_k", 0), c.get("seed", 0), c.get("top_p", 1.0), 0.0) + PEN
    stages = [TorchStage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1), a, b, i == 0, i == 1,
                         sampling=samp) for i, (a, b) in enumerate(ranges)]
    assert ranges[-1][1] == n - 1 and stages[1].penalties_on and not stages[0].penalties_on
    ring = DecodeRing(stages, RingLinks(), 1, 2, 2, use_graphs=False)
    prompt = torch.tensor([ids]).repeat(2, 1)
    want = ring.generate([prompt, prompt], len(ids), steps)
    assert toks.shape == (4, steps) and torch.equal(toks, want)
    plain = DecodeRing([TorchStage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1), a, b, i == 0,
                                   i == 1, sampling=samp[:5]) for i, (a, b) in enumerate(ranges)],
                       RingLinks(), 1, 2, 2, use_graphs=False)
    assert not torch.equal(plain.generate([prompt, prompt], len(ids), steps), want)
