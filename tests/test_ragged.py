"""Ragged prompts on the CPU: ``--prompt`` / ``prompts`` parsing and the
METRICS keys, the torch mirror of csrc/kernels/ragged.hip against a plain
loop, ``TorchStage`` rings against a per-row host loop over unpadded prompts
(greedy, sampled, with penalties + log-probabilities + stop ids, chunked,
two microbatches with different longest prompts), two gloo ranks against one
process, and the ragged path forced on equal lengths against the existing one."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import (apply_penalties_ref, logprobs_ref, penalty_count,
                                                              penalty_state, pick, ragged_last_rows_ref, stop_ref,
                                                              stop_state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


# ---------------------------------------------------------------------- parsing
def _cfg(**kw):
    c = {"nodes": [{"id": "node1", "address": "127.0.0.1:50051", "part_index": 0}], "model_weights": "synthetic:1",
         "num_parts": 1, "transport": "colocated", "model": "gpt2-tiny", "micro_batch_size": 2, "num_microbatches": 2,
         "seq_len": 8, "decode_steps": 4}
    c.update(kw)
    return c


def test_prompt_flag_and_prompts_key():
    from distributed_neural_networks_amd.config import ConfigError, parse_pipeline
    from distributed_neural_networks_amd.runtime.generate import make_prompt_batch, make_prompts, pad_id, prompt_lists
    pipe = parse_pipeline(_cfg())
    assert pipe.prompts is None and prompt_lists(pipe, None) is None
    ids, lens = make_prompt_batch(pipe, None)  # random ids as before, no lengths
    assert tuple(ids.shape) == (4, 8) and lens is None
    # ';' separates prompts, entry i % n goes to sequence i, pads are 0 without a pad_token_id
    ids, lens = make_prompt_batch(pipe, "464,206,75;40;11,12")
    assert ids.tolist() == [[464, 206, 75], [40, 0, 0], [11, 12, 0], [464, 206, 75]] and ids.dtype == torch.int64
    assert lens.tolist() == [3, 1, 2, 3] and lens.dtype == torch.int32
    assert torch.equal(make_prompts(pipe, "464,206,75;40;11,12"), ids)
    # one prompt still replicates, and equal lengths give no lengths: the existing path runs
    ids, lens = make_prompt_batch(pipe, "5,6,7")
    assert ids.tolist() == [[5, 6, 7]] * 4 and lens is None
    ids, lens = make_prompt_batch(pipe, "5,6;7,8")
    assert ids.tolist() == [[5, 6], [7, 8]] * 2 and lens is None
    # the config key, the same cycling rule, pads from pad_token_id when the config has one
    pipe = parse_pipeline(_cfg(prompts=[[1, 2, 3, 4], [9]], pad_token_id=77, eos_token_id=5))
    assert pipe.prompts == ((1, 2, 3, 4), (9,)) and pad_id(pipe) == 77
    ids, lens = make_prompt_batch(pipe, None)
    assert ids.tolist() == [[1, 2, 3, 4], [9, 77, 77, 77]] * 2 and lens.tolist() == [4, 1, 4, 1]
    ids, lens = make_prompt_batch(pipe, "8;9,10")  # --prompt overrides the key
    assert ids.tolist() == [[8, 77], [9, 10]] * 2 and lens.tolist() == [1, 2, 1, 2]
    # rejections
    for bad, what in (([], "non-empty list"), ([[1], []], "empty prompt"), ([[1, 512]], "outside"), ([[-1]], "outside"),
                      ([[1]] * 5, "5 prompts"), ([1, 2], "list of lists"), ([[1.5]], "list of lists"),
                      ([[True]], "list of lists")):
        with pytest.raises(ConfigError, match=what):
            parse_pipeline(_cfg(prompts=bad))
    with pytest.raises(ConfigError, match="generating models only"):
        parse_pipeline(_cfg(model="cifar10", prompts=[[1]]))
    pipe = parse_pipeline(_cfg())
    for bad, what in (("1,2;;3", "empty prompt"), ("1;2;3;4;5", "5 prompts"), ("1,999", "outside"), ("1,x", "integers"),
                      (";", "empty prompt")):
        with pytest.raises(ConfigError, match=what):
            prompt_lists(pipe, bad)


def test_longest_prompt_is_checked_before_any_weight_loads():
    from distributed_neural_networks_amd import cli
    from distributed_neural_networks_amd.config import ConfigError, resolve_node
    limit = 256  # gpt2-tiny block_size
    ctx = resolve_node(_cfg(prompts=[[1], list(range(limit - 4))], decode_steps=4), "node1")
    args = types.SimpleNamespace(prompt=None)
    assert cli.kv_needs(ctx, args) == (4, limit)
    cli.check_config_capacity(ctx, args)
    ctx = resolve_node(_cfg(prompts=[[1], list(range(limit - 3))], decode_steps=4), "node1")
    with pytest.raises(ConfigError, match="exceeds the model's limit"):
        cli.check_config_capacity(ctx, args)
    ctx = resolve_node(_cfg(decode_steps=4), "node1")
    long = ",".join(str(i % 500) for i in range(limit - 3))
    with pytest.raises(ConfigError, match="exceeds the model's limit"):
        cli.check_config_capacity(ctx, types.SimpleNamespace(prompt="1;" + long))
    with pytest.raises(ConfigError, match="outside"):
        cli.check_config_capacity(ctx, types.SimpleNamespace(prompt="1;600"))
    assert cli.kv_needs(ctx, types.SimpleNamespace(prompt="1,2,3;4")) == (4, 3 + 4)


def test_metrics_keys():
    from distributed_neural_networks_amd.runtime.generate import metrics
    m = metrics("n", 0.5, 1.0, 4, 16, 3, 2, 1)
    assert m["prompt_len"] == 16 and m["prompt_tokens"] == 64 and "prompt_lens" not in m
    assert m["prefill_tokens_per_s"] == 128.0
    m = metrics("n", 0.5, 1.0, 4, 16, 3, 2, 1, torch.tensor([16, 1, 9, 4], dtype=torch.int32))
    assert m["prompt_len"] == 16 and m["prompt_tokens"] == 30 and m["prompt_lens"] == [16, 1, 9, 4]
    assert m["prefill_tokens_per_s"] == 60.0 and m["decode_steps"] == 2
    json.dumps(m)


def test_ragged_config_file():
    from distributed_neural_networks_amd.config import load_json, parse_pipeline
    pipe = parse_pipeline(load_json(os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_ragged.json")))
    assert len(pipe.prompts) == 3 and len({len(q) for q in pipe.prompts}) == 3 and pipe.temperature > 0


# ---------------------------------------------------------------------- the mirror against a plain loop
def _loop(h, lens, t0, Tc, B, d, dst):
    out = dst.clone()
    for b in range(B):
        q = int(lens[b]) - 1 - t0
        if 0 <= q < Tc:
            for j in range(d):
                out[b, j] = h[b * Tc + q, j]
    return out


@pytest.mark.parametrize("B,Tc,t0,d,ld,dst_ld", [(7, 5, 10, 8, 8, 8), (7, 5, 10, 8, 16, 24), (6, 1, 3, 16, 16, 16),
                                                 (9, 4, 0, 8, 8, 8)])
def test_mirror_against_plain_loop(B, Tc, t0, d, ld, dst_ld):
    g = torch.Generator().manual_seed(B * 100 + Tc)
    h = torch.randn((B * Tc + 2, ld), generator=g).to(torch.bfloat16)
    dst = torch.full((B + 2, dst_ld), -7.0, dtype=torch.bfloat16)
    # L - 1 at t0 - 1, t0, t0 + Tc - 1, t0 + Tc, and L <= 0
    cases = [t0, t0 + 1, t0 + Tc, t0 + Tc + 1, 0, -3, t0 + (Tc + 1) // 2, 1, t0 + 1]
    lens = torch.tensor(cases[:B], dtype=torch.int32)
    got = ragged_last_rows_ref(h, lens, t0, Tc, B, d, dst)
    want = _loop(h, lens, t0, Tc, B, d, dst)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    hit = [0 <= int(v) - 1 - t0 < Tc for v in lens.tolist()]
    assert any(hit) and not all(hit)
    assert bool((got[B:] == -7.0).all()) and bool((got[:, d:] == -7.0).all())  # rows past B and the gap keep theirs
    for b in range(B):
        assert bool((got[b, :d] == -7.0).all()) != hit[b] or d == 0
    assert bool((dst == -7.0).all())  # the argument is not changed


# ---------------------------------------------------------------------- TorchStage rings against a per-row host loop
PAD = 3  # the pad id of the ragged batches: absent from every valid prompt (so a wrongly marked pad shows)


def _model(model, seed=5):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import build_golden_stage, default_ranges, model_info
    ranges = default_ranges(model, 2)
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, seed) for i, (a, b) in enumerate(ranges)]
    golden = []
    for i, (a, b) in enumerate(ranges):
        gm = build_golden_stage(model, a, b, i == 0, i == 1)
        gm.load_state_dict(sds[i])
        golden.append(gm.eval())
    return ranges, sds, golden, model_info(model).cfg.vocab_size


def _batch(V, lens, seed=11):
    """Right-padded ids (n, max lens) with PAD in the pads and never in a prompt."""
    g = torch.Generator().manual_seed(seed)
    T = max(lens)
    ids = torch.randint(0, V - 1, (len(lens), T), generator=g)
    ids = torch.where(ids >= PAD, ids + 1, ids)  # skip PAD
    for b, L in enumerate(lens):
        ids[b, L:] = PAD
    return ids


def _stages(model, ranges, sds, samp):
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    return [TorchStage(model, sds[i], a, b, i == 0, i == 1, sampling=samp) for i, (a, b) in enumerate(ranges)]


def _ring(model, ranges, sds, samp, M, B):
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    return DecodeRing(_stages(model, ranges, sds, samp), RingLinks(), 1, M, B, use_graphs=False, early_exit=False)


def _oracle(golden, V, ids, lens, B, steps, samp):
    """Each row on its own unpadded prompt: a full-prefix forward of the golden
    modules per token, and the stage's own tail on the microbatch's B logits
    rows (the sampler's hash takes the row's index in its microbatch)."""
    temp, top_k, seed, top_p, min_p, rep, pres, freq, nlp, stop = samp
    pen = rep != 1.0 or pres != 0.0 or freq != 0.0
    toks, chosen, top_ids, fin = [], [], [], []
    for m0 in range(0, len(lens), B):
        seqs = [ids[b, :lens[b]].tolist() for b in range(m0, m0 + B)]
        state = torch.cat([penalty_state(torch.tensor([q]), V) for q in seqs], 0) if pen else None
        st = stop_state(B) if stop is not None else None
        prev, out, lp_c, lp_i = None, [], [], []
        for k in range(steps):
            rows = []
            with torch.no_grad():
                for q in seqs:
                    h = torch.tensor([q], dtype=torch.int64)
                    for gm in golden:
                        h = gm(h)
                    rows.append(h[0, -1])
            logits = torch.stack(rows, 0)
            if pen:
                if k > 0:
                    state = penalty_count(state, prev)
                logits = apply_penalties_ref(logits, state, rep, freq, pres)
            step = (torch.zeros((B,), dtype=torch.int32) if k == 0
                    else torch.tensor([len(q) - 1 for q in seqs], dtype=torch.int32))
            pred = pick(logits, temp, top_k, seed, step, top_p=top_p, min_p=min_p).to(torch.int32)
            prev = pred.clone()
            if nlp:
                c, ti, _ = logprobs_ref(logits, pred, nlp)
                lp_c.append(c)
                lp_i.append(ti)
            if stop is not None:
                st, pred = stop_ref(st, pred, stop.stop_token_ids, stop.stop_sequences, stop.min_new_tokens,
                                    stop.pad_token_id)
            out.append(pred)
            for q, t in zip(seqs, pred.tolist()):
                q.append(t)
        toks.append(torch.stack(out, 1))
        if nlp:
            chosen.append(torch.stack(lp_c, 1))
            top_ids.append(torch.stack(lp_i, 1))
        if stop is not None:
            fin.append(st)
    return (torch.cat(toks, 0), torch.cat(chosen, 0) if chosen else None, torch.cat(top_ids, 0) if top_ids else None,
            torch.cat(fin, 0) if fin else None)


def _generate(ring, ids, lens, B, steps, chunk=0):
    M = len(lens) // B
    T = ids.shape[1]
    return ring.generate([ids[m * B:(m + 1) * B] for m in range(M)], T, steps, chunk,
                         lens=[torch.tensor(lens[m * B:(m + 1) * B]) for m in range(M)])


LENS = [1, 12, 7, 4]
STEPS = 6
PLAIN = (1.0, 0.0, 0.0, 0, None)


@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
@pytest.mark.parametrize("sampling", [(0.0, 0, 0, 1.0, 0.0), (0.9, 40, 3, 0.95, 0.0)], ids=["greedy", "sampled"])
def test_ring_equals_per_row_loop(model, sampling):
    ranges, sds, golden, V = _model(model)
    ids = _batch(V, LENS)
    samp = sampling + PLAIN
    want = _oracle(golden, V, ids, LENS, 4, STEPS, samp)[0]
    got = _generate(_ring(model, ranges, sds, samp, 1, 4), ids, LENS, 4, STEPS)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    # chunked: pieces of 5 (12 = 5 + 5 + 2: rows end in the first, second and third piece)
    got_c = _generate(_ring(model, ranges, sds, samp, 1, 4), ids, LENS, 4, STEPS, chunk=5)
    assert torch.equal(got_c, want), (got_c.tolist(), want.tolist())


@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
@pytest.mark.parametrize("sampling", [(0.0, 0, 0, 1.0, 0.0), (0.9, 40, 3, 0.95, 0.0)], ids=["greedy", "sampled"])
def test_ring_with_penalties_logprobs_and_stops(model, sampling):
    from distributed_neural_networks_amd.config import StopConfig
    ranges, sds, golden, V = _model(model)
    ids = _batch(V, LENS)
    free = _oracle(golden, V, ids, LENS, 4, STEPS, sampling + (1.3, 0.2, 0.1, 0, None))[0]
    stop = StopConfig((int(free[1, 2]),), (), 0, PAD)  # row 1 stops at its third token
    samp = sampling + (1.3, 0.2, 0.1, 3, stop)
    want_t, want_c, want_i, want_st = _oracle(golden, V, ids, LENS, 4, STEPS, samp)
    assert 0 < int(want_st[1, 1]) <= 3 and bool((want_st[:, 1] == 0).any())
    for chunk in (0, 5):
        ring = _ring(model, ranges, sds, samp, 1, 4)
        got = _generate(ring, ids, LENS, 4, STEPS, chunk)
        assert torch.equal(got, want_t), (chunk, got.tolist(), want_t.tolist())
        lp, fin = ring.logprobs(), ring.finished()
        length = torch.where(want_st[:, 1] != 0, want_st[:, 1], torch.tensor(STEPS, dtype=torch.int32))
        assert torch.equal(fin["length"], length)
        for b in range(4):  # columns past a row's length are unspecified
            n = int(length[b])
            assert torch.equal(lp["top_ids"][b, :n], want_i[b, :n])
            assert torch.allclose(lp["chosen"][b, :n], want_c[b, :n], rtol=0, atol=1e-4)
    # the pad id is never "seen in the prompt": the last stage marked ids[b, :L_b] only
    pen = ring.stages[-1]._pen[0]
    for b, L in enumerate(LENS):
        seen_in_prompt = (pen[b].to(torch.int64) & 0x8000) != 0
        assert set(torch.nonzero(seen_in_prompt).flatten().tolist()) == set(ids[b, :L].tolist())


def test_two_microbatches_skip_pieces():
    """M = 2: microbatch 0's longest prompt is 9, microbatch 1's 16; with
    pieces of 5 the first runs two pieces (5 + 4), the second four."""
    model = "gpt2-tiny"
    ranges, sds, golden, V = _model(model)
    lens = [9, 2, 5, 16, 1, 11]
    ids = _batch(V, lens)
    samp = (0.9, 40, 3, 0.95, 0.0, 1.0, 0.0, 0.0, 2, None)
    want_t, want_c, want_i, _ = _oracle(golden, V, ids, lens, 3, STEPS, samp)
    for chunk in (0, 5):
        ring = _ring(model, ranges, sds, samp, 2, 3)
        calls = []
        last = ring.stages[-1]
        real = last.step
        last.step = lambda *a, **k: (calls.append((k.get("b0", 0), a[3], k.get("t0"))), real(*a, **k))[1]
        got = _generate(ring, ids, lens, 3, STEPS, chunk)
        assert torch.equal(got, want_t), (chunk, got.tolist(), want_t.tolist())
        pieces = [(b0, T, t0) for b0, T, t0 in calls if t0 is not None]
        if chunk:
            assert pieces == [(0, 5, 0), (0, 4, 5), (3, 5, 0), (3, 5, 5), (3, 5, 10), (3, 1, 15)]
        else:
            assert pieces == [(0, 9, 0), (3, 16, 0)]
        lp = ring.logprobs()
        assert torch.equal(lp["top_ids"], want_i) and torch.allclose(lp["chosen"], want_c, rtol=0, atol=1e-4)


@pytest.mark.parametrize("sampling,chunk", [((0.0, 0, 0, 1.0, 0.0), 0), ((0.0, 0, 0, 1.0, 0.0), 5),
                                            ((0.9, 40, 3, 0.95, 0.0), 0)], ids=["greedy", "greedy-chunked", "sampled"])
def test_forced_ragged_path_equals_existing_path(sampling, chunk):
    """All lengths equal through the ragged path against the existing path.
    Chunked only when greedy: the sampler's step operand of a chunked
    equal-length prefill is its last piece's start, of the ragged path always
    0, so sampled runs are equal for the unchunked prefill alone."""
    from distributed_neural_networks_amd.config import StopConfig
    model = "gpt2-tiny"
    ranges, sds, golden, V = _model(model)
    T, B, M = 12, 2, 2
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (M * B, T), generator=g)
    prompts = [ids[m * B:(m + 1) * B] for m in range(M)]
    base = sampling + (1.3, 0.2, 0.1, 3)
    free = _ring(model, ranges, sds, base + (None,), M, B).generate(prompts, T, STEPS)
    samp = base + (StopConfig((int(free[2, 3]),), (), 0, PAD),)
    old = _ring(model, ranges, sds, samp, M, B)
    want = old.generate(prompts, T, STEPS, chunk)
    new = _ring(model, ranges, sds, samp, M, B)
    got = new.generate(prompts, T, STEPS, chunk, lens=[torch.full((B,), T)] * M)
    assert torch.equal(got, want)
    a, b = old.logprobs(), new.logprobs()
    assert all(torch.equal(a[k], b[k]) for k in a)
    fa, fb = old.finished(), new.finished()
    assert torch.equal(fa["length"], fb["length"]) and fa["reason"] == fb["reason"]
    assert any(r is not None for r in fa["reason"])


def test_ring_arguments():
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model = "gpt2-tiny"
    ranges, sds, golden, V = _model(model)
    ring = _ring(model, ranges, sds, (0.0, 0, 0), 1, 2)
    ids = _batch(V, [3, 2])
    for bad in ([0, 2], [4, 2], [1, 2, 3]):
        with pytest.raises(ValueError, match="lengths of microbatch 0"):
            ring.generate([ids], 3, 2, lens=[torch.tensor(bad)])
    first = TorchStage(model, sds[0], *ranges[0], True, False)
    with pytest.raises(ValueError, match="last stage only"):
        first.ragged_first_token(0, 2, torch.tensor([1, 2]))
    last = TorchStage(model, sds[1], *ranges[1], False, True)
    with pytest.raises(ValueError, match="no ragged prefill piece"):
        last.ragged_first_token(0, 2, torch.tensor([1, 2]))


def test_received_lengths_are_checked_on_every_rank():
    """A rank other than 0 derives its pieces from the lengths it receives: a
    length outside [1, T] raises there instead of giving other pieces than the
    sender's."""
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model = "gpt2-tiny"
    ranges, sds, golden, V = _model(model)

    class Link:
        def __init__(self, lens):
            self.lens = lens

        def recv(self, t):
            t.copy_(torch.tensor(self.lens, dtype=t.dtype))

    last = TorchStage(model, sds[1], *ranges[1], False, True)
    for bad in ([5, 2], [0, 3], [-1, 4]):
        ring = DecodeRing([last], RingLinks(prev=Link(bad), back_out=Link(bad)), 2, 1, 2, use_graphs=False, ragged=True)
        with pytest.raises(ValueError, match="lengths of microbatch 0"):
            ring.prefill(None, 4)


def test_grpc_transport_rejects_different_lengths(tmp_path):
    """The gRPC request path runs one full-prefix forward and reads every row's
    prediction at the last position, so prompts of different lengths are
    rejected there before any weight loads; equal lengths still pass."""
    from distributed_neural_networks_amd import cli
    from distributed_neural_networks_amd.config import ConfigError, resolve_node
    grpc = dict(transport="grpc")
    ctx = resolve_node(_cfg(**grpc), "node1")
    with pytest.raises(ConfigError, match="different lengths.*decode ring"):
        cli.check_prompt_transport(ctx, types.SimpleNamespace(prompt="1,2,3;4"))
    with pytest.raises(ConfigError, match="different lengths"):
        cli.make_prompt(ctx, "1,2,3;4")
    cli.check_prompt_transport(ctx, types.SimpleNamespace(prompt="1,2,3;4,5,6"))
    cli.check_prompt_transport(ctx, types.SimpleNamespace(prompt=None))
    assert cli.make_prompt(ctx, "1,2,3;4,5,6").tolist() == [[1, 2, 3], [4, 5, 6]] * 2
    with pytest.raises(ConfigError, match="different lengths"):
        cli.check_prompt_transport(resolve_node(_cfg(prompts=[[1, 2], [3]], **grpc), "node1"),
                                   types.SimpleNamespace(prompt=None))
    # the default transport is gRPC
    c = _cfg(prompts=[[1, 2], [3]])
    del c["transport"]
    with pytest.raises(ConfigError, match="different lengths"):
        cli.check_prompt_transport(resolve_node(c, "node1"), types.SimpleNamespace(prompt=None))
    # two prompts of different lengths that the run's single sequence never mixes
    one = resolve_node(_cfg(micro_batch_size=1, num_microbatches=1, prompts=[[1, 2]], **grpc), "node1")
    cli.check_prompt_transport(one, types.SimpleNamespace(prompt=None))
    # the ring transports take them
    for tr in ("colocated", "gloo", "rccl", "gloo_gpu"):
        cli.check_prompt_transport(resolve_node(_cfg(transport=tr), "node1"), types.SimpleNamespace(prompt="1,2,3;4"))
    # the command line: the error, exit code 1, no weight loaded
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(_cfg(**grpc)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                        "--prompt", "1,2,3;4"], env=ENV, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "different lengths" in r.stdout and "weights" not in r.stdout.lower(), r.stdout[-2000:]


# ---------------------------------------------------------------------- two gloo ranks against one process
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_cli_two_gloo_ranks_equal_one_process(tmp_path):
    """Penalties on, so the lengths and the prompt ids both travel down the
    stage links; only stage 0 sees ``--prompt``."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.config import parse_pipeline
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.generate import make_prompt_batch
    model, steps = "gpt2-tiny", 6
    ranges = default_ranges(model, 2)
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{_free_port()}", "part_index": i} for i in range(2)],
         "model_weights": "synthetic:1", "num_parts": 2, "return_to_node_id": "node1", "transport": "gloo",
         "model": model, "seq_len": 12, "decode_steps": steps, "micro_batch_size": 2, "num_microbatches": 2,
         "temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 7, "repetition_penalty": 1.3, "logprobs": 2,
         "prefill_chunk": 4, "pad_token_id": PAD, "eos_token_id": 1}
    flag = "464,206,75,9,10,11,12;40;11,12,13"
    pipe = parse_pipeline(c)
    ids, lens = make_prompt_batch(pipe, flag)
    assert lens.tolist() == [7, 1, 3, 7]
    samp = (0.8, 20, 7, 0.9, 0.0, 1.3, 0.0, 0.0, 2, pipe.stop)
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1) for i, (a, b) in enumerate(ranges)]
    ring = _ring(model, ranges, sds, samp, 2, 2)
    want = _generate(ring, ids, lens.tolist(), 2, steps, chunk=4)
    want_lp = ring.logprobs()
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    node = os.path.join(ROOT, "node.py")
    p1 = subprocess.Popen([sys.executable, node, "--node_id", "node2", "--config", str(cfg), "--serve_seconds", "90"],
                          env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        r0 = subprocess.run([sys.executable, node, "--node_id", "node1", "--config", str(cfg), "--input_image",
                             "none.png", "--shutdown_pipeline", "--prompt", flag], env=ENV, capture_output=True,
                            text=True, timeout=120)
        try:
            out1 = p1.communicate(timeout=60)[0]
        except subprocess.TimeoutExpired:
            p1.kill()
            out1 = p1.communicate()[0]
    finally:
        if p1.poll() is None:
            p1.kill()
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:] + out1[-2000:]
    toks = torch.tensor(json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    assert torch.equal(toks, want), (toks.tolist(), want.tolist())
    m = json.loads(r0.stdout.split("METRICS ")[1].splitlines()[0])
    assert m["prompt_lens"] == [7, 1, 3, 7] and m["prompt_tokens"] == 18 and m["prompt_len"] == 7
    line = json.loads(out1.split("LOGPROBS ")[1].splitlines()[0])  # the last rank's, aligned per row
    assert torch.allclose(torch.tensor(line["chosen"]), want_lp["chosen"], rtol=0, atol=1e-5)
    assert line["top_ids_seq0"] == want_lp["top_ids"][0].tolist()
    assert "FINISH " in out1
