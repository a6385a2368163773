"""Ragged prompts on the device: csrc/kernels/ragged.hip against its torch
mirror with guard words around the destination, the rejections, and rings of
two colocated stages on right-padded prompts of different lengths: against the
fp32 golden on each row's own unpadded prompt, pad invariance, the ragged path
forced on equal lengths against the existing path (bf16 and calibrated fp8 KV),
the ring variants, two microbatches with different longest prompts, the CLI."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import ragged_last_rows_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64  # poisoned bf16 words on either side of the destination
POISON = -123.0


def _bits(t):
    return t.cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------- the kernel against the mirror
def _lens_for(B, Tc, t0):
    """L - 1 at t0 - 1, t0, t0 + Tc - 1, t0 + Tc, L <= 0, and inside the piece."""
    cases = [t0, t0 + 1, t0 + Tc, t0 + Tc + 1, 0, -2, t0 + (Tc + 1) // 2, 1]
    return torch.tensor([cases[(b * 3 + b // 8) % len(cases)] if B > 1 else t0 + Tc for b in range(B)],
                        dtype=torch.int32)


@pytest.mark.parametrize("d", [8, 64, 1600])
@pytest.mark.parametrize("Tc", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_kernel_against_mirror(B, Tc, d):
    from distributed_neural_networks_amd.ops import transformer_ops as T_
    t0, ld, dst_ld, extra = 7, d + 8, d + 16, 2
    g = torch.Generator().manual_seed(B * 1000 + Tc * 10 + d)
    h = torch.randn((B * Tc, ld), generator=g).to(torch.bfloat16).to(DEV)
    whole = torch.full(((B + extra) * dst_ld + 2 * GUARD,), POISON, dtype=torch.bfloat16, device=DEV)
    dst = whole[GUARD:GUARD + (B + extra) * dst_ld].view(B + extra, dst_ld)  # the gap and the rows past B poisoned too
    assert dst.data_ptr() % 16 == 0
    lens = _lens_for(B, Tc, t0)
    want = ragged_last_rows_ref(h.cpu(), lens, t0, Tc, B, d, dst.cpu())
    out = T_.ragged_last_rows(h, lens.to(DEV), t0, Tc, B, dst, d=d)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    assert torch.equal(_bits(dst), _bits(want))
    hit = (lens - 1 - t0 >= 0) & (lens - 1 - t0 < Tc)
    assert bool(hit.any()) and (B == 1 or not bool(hit.all()))
    got = dst.cpu()
    for b in range(B):  # a matching row holds its source row, the others keep their poison
        q = int(lens[b]) - 1 - t0
        if hit[b]:
            assert torch.equal(_bits(got[b, :d]), _bits(h[b * Tc + q, :d]))
        else:
            assert bool((got[b] == POISON).all())
    assert bool((got[:, d:] == POISON).all()) and bool((got[B:] == POISON).all())
    assert bool((whole[:GUARD] == POISON).all()) and bool((whole[-GUARD:] == POISON).all())


def test_kernel_rejections():
    from distributed_neural_networks_amd.ops import transformer_ops as T_
    from distributed_neural_networks_amd.ops._lib import lib, ptr, stream_ptr
    B, Tc, d = 4, 3, 16
    h = torch.ones((B * Tc, d), dtype=torch.bfloat16, device=DEV)
    dst = torch.full((B, d), POISON, dtype=torch.bfloat16, device=DEV)
    lens = torch.full((B,), 2, dtype=torch.int32, device=DEV)  # every row matches: a launch would write
    good = dict(h=ptr(h), ld=d, lens=ptr(lens), t0=0, Tc=Tc, B=B, d=d, dst=ptr(dst), dst_ld=d, st=stream_ptr())
    bad = [dict(d=12), dict(d=0), dict(h=0), dict(lens=0), dict(dst=0), dict(h=ptr(h) + 2), dict(dst=ptr(dst) + 2),
           dict(ld=8), dict(dst_ld=8), dict(ld=20), dict(dst_ld=20), dict(Tc=0), dict(t0=-1)]
    for kw in bad:
        assert lib().ragged_last_rows(**dict(good, **kw)) < 0, kw
    assert lib().ragged_last_rows(**dict(good, B=0, h=0)) == 0  # an empty batch launches nothing
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())
    # the wrapper refuses the same before the library is called
    with pytest.raises(ValueError, match="multiple of 8"):
        T_.ragged_last_rows(h, lens, 0, Tc, B, dst, d=12)
    wide = torch.ones((B * Tc + 1, d + 4), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="16-byte aligned"):
        T_.ragged_last_rows(wide[:, :d], lens, 0, Tc, B, dst)  # row stride 20
    flat = torch.ones((B * d + 8,), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="16-byte aligned"):
        T_.ragged_last_rows(h, lens, 0, Tc, B, flat[1:1 + B * d].view(B, d))  # starts 2 bytes off
    with pytest.raises(TypeError, match="bf16"):
        T_.ragged_last_rows(h.to(torch.float16), lens, 0, Tc, B, dst)
    with pytest.raises(TypeError, match="bf16"):
        T_.ragged_last_rows(h, lens, 0, Tc, B, dst.float())
    with pytest.raises(ValueError, match="lens"):
        T_.ragged_last_rows(h, lens[:B - 1], 0, Tc, B, dst)
    with pytest.raises(ValueError, match="lens"):
        T_.ragged_last_rows(h, lens.long(), 0, Tc, B, dst)
    with pytest.raises(ValueError, match="rows"):
        T_.ragged_last_rows(h[:B * Tc - 1], lens, 0, Tc, B, dst)
    with pytest.raises(ValueError, match="one device"):
        T_.ragged_last_rows(h, lens.cpu(), 0, Tc, B, dst)
    torch.cuda.synchronize()
    assert bool((dst == POISON).all())


# ---------------------------------------------------------------------- rings: the fixture
LENS = [1, 16, 9, 5, 12, 2, 16, 7]
NB, T, STEPS, K = 8, 16, 8, 4
KINDS = {"greedy": {}, "sampled": dict(temperature=0.8, top_k=20, top_p=0.9, seed=5)}
EXTRAS = dict(repetition_penalty=1.3, logprobs=3)


@functools.lru_cache(maxsize=None)
def _weights(model):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    n = model_info(model).num_layers
    ranges = [(0, n // 2 - 1), (n // 2, n - 1)]
    return ranges, [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 7, nontrivial=True)
                    for i, (a, b) in enumerate(ranges)]


@functools.lru_cache(maxsize=None)
def _ids(model):
    from distributed_neural_networks_amd.models import model_info
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, model_info(model).cfg.vocab_size, (NB, T), generator=g)


def _padded(model, pads="zero"):
    ids = _ids(model).clone()
    g = torch.Generator().manual_seed(99)
    rnd = torch.randint(0, 512, (NB, T), generator=g)
    for b, L in enumerate(LENS):
        ids[b, L:] = rnd[b, L:] if pads == "random" else 0
    return ids


def _stages(model, max_batch=NB, **last_kw):
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    ranges, sds = _weights(model)
    kv = {k: last_kw.pop(k) for k in ("kv_dtype", "kv_scale") if k in last_kw}
    return [TransformerStage(model, sds[i], a, b, i == 0, i == 1, DEV, max_batch=max_batch, max_seq=T + STEPS + K + 2,
                             **kv, **(last_kw if i == 1 else {})) for i, (a, b) in enumerate(ranges)]


def _run(model, ids, lens, M=1, chunk=0, graphs=False, ms=0, steps=STEPS, max_batch=None, **kw):
    """(tokens, ring) of one generation of M microbatches; ``lens`` None: the existing path."""
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    B = ids.shape[0] // M
    ring = DecodeRing(_stages(model, max_batch=max_batch or ids.shape[0], **kw), RingLinks(), 1, M, B, use_graphs=graphs,
                      multi_step=ms, early_exit=False)
    ml = None if lens is None else [torch.tensor(lens[m * B:(m + 1) * B]) for m in range(M)]
    toks = ring.generate([ids[m * B:(m + 1) * B] for m in range(M)], ids.shape[1], steps, chunk, lens=ml)
    torch.cuda.synchronize()
    return toks, ring


def _everything(toks, ring):
    out = {"tokens": toks}
    if ring.lp_chosen is not None:
        out.update(ring.logprobs())
    if ring.stp is not None:
        fin = ring.finished()
        out["length"] = fin["length"]
        out["reason"] = torch.tensor([-1 if r is None else r[1] for r in fin["reason"]])
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, a[k].tolist(), b[k].tolist())


# ---------------------------------------------------------------------- against the fp32 golden
@functools.lru_cache(maxsize=None)
def _golden(model):
    from distributed_neural_networks_amd.models import build_golden_stage
    ranges, sds = _weights(model)
    mods = []
    for i, (a, b) in enumerate(ranges):
        gm = build_golden_stage(model, a, b, i == 0, i == 1)
        gm.load_state_dict(sds[i])
        mods.append(gm.eval())
    return mods


@pytest.mark.parametrize("chunk", [0, 5])
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
def test_against_the_fp32_golden(model, chunk):
    """Each row on its own unpadded prompt, following the device's sequence: a
    token may differ from the golden's argmax only where the golden's top-2
    logits are within 2e-2 * |top1| (the rule of the transformer smoke run),
    and that at no more than 16 of the 64 (row, step) pairs.  On this fixture
    the golden alone, following its own continuation, has 4 such pairs for
    gpt2-tiny and 6 for llama3-tiny; the cap is about 2.5 times that."""
    toks, _ = _run(model, _padded(model), LENS, chunk=chunk)
    ids = _ids(model)
    excused = 0
    with torch.no_grad():
        for b, L in enumerate(LENS):
            seq = ids[b:b + 1, :L].clone()
            for t in range(STEPS):
                h = seq
                for gm in _golden(model):
                    h = gm(h)
                last = h[0, -1]
                top2 = last.topk(2).values
                if int(toks[b, t]) != int(last.argmax()):
                    tie = (top2[0] - top2[1]).item() <= 2e-2 * top2[0].abs().item()
                    assert tie, (model, chunk, b, t, toks[b].tolist(), int(last.argmax()))
                    excused += 1
                seq = torch.cat([seq, toks[b:b + 1, t:t + 1].long()], 1)  # follow the device's sequence
    print(f"{model} chunk {chunk}: {excused} of {NB * STEPS} pairs excused")
    assert excused <= 16, excused


# ---------------------------------------------------------------------- pad invariance
@functools.lru_cache(maxsize=None)
def _stop_for(model, kind):
    """A stop id that the unstopped ragged run meets midway in some row."""
    from distributed_neural_networks_amd.config import StopConfig
    free, _ = _run(model, _padded(model), LENS, **KINDS[kind], **EXTRAS)
    return StopConfig((int(free[1, 3]),), (), 0, 1)


@pytest.mark.parametrize("kind", list(KINDS))
def test_pad_invariance(kind):
    """What the pads hold never reaches a valid position (causal attention) nor
    the penalty state, so everything is equal bit for bit; an off-by-one into a
    pad row would read the pad's hidden state and differ."""
    model = "gpt2-tiny"
    kw = dict(stop=_stop_for(model, kind), **KINDS[kind], **EXTRAS)
    for chunk in (0, 5):
        a = _everything(*_run(model, _padded(model, "zero"), LENS, chunk=chunk, **kw))
        b = _everything(*_run(model, _padded(model, "random"), LENS, chunk=chunk, **kw))
        _assert_same(a, b, f"pads, chunk {chunk}")
        assert bool((a["length"] < STEPS).any()) and bool((a["length"] == STEPS).any())


def test_pad_invariance_fp8_kv_unit_scale():
    model = "gpt2-tiny"
    kw = dict(kv_dtype="fp8", kv_scale="unit", logprobs=3)
    a = _everything(*_run(model, _padded(model, "zero"), LENS, **kw))
    b = _everything(*_run(model, _padded(model, "random"), LENS, **kw))
    _assert_same(a, b, "pads, fp8 KV")


# ---------------------------------------------------------------------- equal lengths through the ragged path
@pytest.mark.parametrize("model,kv", [("gpt2-tiny", "bf16"), ("llama3-tiny", "bf16"), ("gpt2-tiny", "fp8-calibrated")])
def test_equal_lengths_through_the_ragged_path(model, kv):
    kw = dict(stop=_stop_for(model, "sampled"), **KINDS["sampled"], **EXTRAS)
    if kv != "bf16":
        kw.update(kv_dtype="fp8", kv_scale="calibrated")
    ids = _ids(model)
    old = _everything(*_run(model, ids, None, **kw))
    new = _everything(*_run(model, ids, [T] * NB, **kw))
    _assert_same(old, new, "forced ragged path")
    old_k = _everything(*_run(model, ids, None, graphs=True, ms=K, **kw))
    new_k = _everything(*_run(model, ids, [T] * NB, graphs=True, ms=K, **kw))
    _assert_same(old_k, new_k, "forced ragged path, K-step graphs")
    _assert_same(old, old_k, "graphs")


# ---------------------------------------------------------------------- ring variants
@pytest.mark.parametrize("kind", list(KINDS))
def test_ring_variants_agree(kind):
    from distributed_neural_networks_amd.ops import transformer_ops as Tops
    model = "gpt2-tiny"
    kw = dict(stop=_stop_for(model, kind), **KINDS[kind], **EXTRAS)
    ids = _padded(model)
    eager = _everything(*_run(model, ids, LENS, **kw))
    toks, ring = _run(model, ids, LENS, graphs=True, ms=0, **kw)
    assert ring.graphs and ring.graph_k is None
    _assert_same(eager, _everything(toks, ring), "single-step graphs")
    toks, ring = _run(model, ids, LENS, graphs=True, ms=K, **kw)
    assert ring.graph_k is not None and ring.graph_k_steps == K and ring.hist is not None
    _assert_same(eager, _everything(toks, ring), "K-step graphs")
    again = ring.generate([ids], T, STEPS, lens=[torch.tensor(LENS)])  # the graphs replayed on a new generation
    torch.cuda.synchronize()
    _assert_same(eager, _everything(again, ring), "K-step graphs, second generation")
    # the unfused tail is an arm of the sampler launch alone: greedy decoding never reads the switch
    if "temperature" in KINDS[kind]:
        assert Tops.SAMPLE_FUSED_TAIL
        Tops.SAMPLE_FUSED_TAIL = False
        try:
            toks, ring = _run(model, ids, LENS, graphs=True, ms=0, **kw)
            assert ring.hist is None
        finally:
            Tops.SAMPLE_FUSED_TAIL = True
        _assert_same(eager, _everything(toks, ring), "unfused tail")


# ---------------------------------------------------------------------- two microbatches
def test_two_microbatches_with_different_longest_prompts():
    """Microbatch 0's longest prompt is 9, microbatch 1's 16: the ring of both
    runs for each exactly the pieces of a ring that holds it alone (same shapes,
    so the same bits), and tokens() / logprobs() stay aligned per row."""
    model = "gpt2-tiny"
    order = [0, 2, 3, 5, 1, 4, 6, 7]  # lengths 1, 9, 5, 2 | 16, 12, 16, 7
    lens = [LENS[i] for i in order]
    ids = _padded(model)[order]
    kw = dict(logprobs=3, **KINDS["sampled"])
    for chunk, graphs, ms in ((0, False, 0), (5, True, K)):
        both = _everything(*_run(model, ids, lens, M=2, chunk=chunk, graphs=graphs, ms=ms, **kw))
        # each microbatch in a ring of its own, prompts padded to its own longest one (stages of the same size:
        # the decode attention's split count follows max_batch)
        alone = [_everything(*_run(model, ids[m * 4:(m + 1) * 4, :Tm].contiguous(), lens[m * 4:(m + 1) * 4],
                                   chunk=chunk, graphs=graphs, ms=ms, max_batch=NB, **kw))
                 for m, Tm in ((0, 9), (1, 16))]
        _assert_same({k: v[:4] for k, v in both.items()}, alone[0], f"microbatch 0, chunk {chunk}")
        _assert_same({k: v[4:] for k, v in both.items()}, alone[1], f"microbatch 1, chunk {chunk}")
    # per-row alignment: every row's first log-probability is that of its own first token
    toks, ring = _run(model, ids, lens, M=2, chunk=5, **kw)
    lp = ring.logprobs()
    assert tuple(lp["chosen"].shape) == (NB, STEPS) and tuple(lp["top_ids"].shape) == (NB, STEPS, 3)
    assert bool(torch.isfinite(lp["chosen"]).all()) and bool((lp["chosen"] <= 0).all())
    for b, L in enumerate(lens):
        row = ring.lp_chosen[b // 4][b % 4].cpu()
        assert bool((row[:L - 1] == 0).all()) and torch.equal(row[L - 1:L - 1 + STEPS], lp["chosen"][b])
        if ring.hist is not None:
            assert torch.equal(ring.hist[b // 4][b % 4, L:L + STEPS - 1].cpu(), toks[b, 1:])


# ---------------------------------------------------------------------- the CLI
def test_cli_ragged_config():
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.config import load_json, parse_pipeline
    from distributed_neural_networks_amd.runtime.generate import make_prompt_batch
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import build_device_stage
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "configs", "gpt2_4stage_1gpu_ragged.json")
    pipe = parse_pipeline(load_json(path))
    ids, lens = make_prompt_batch(pipe, None)
    n, Tp = ids.shape
    steps = pipe.decode_steps
    assert lens is not None and len(set(lens.tolist())) == 3 and pipe.stop is not None
    r = subprocess.run([sys.executable, os.path.join(root, "node.py"), "--node_id", "node1", "--config", path],
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    toks = torch.tensor(json.loads(r.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    metrics = json.loads(r.stdout.split("METRICS ")[1].splitlines()[0])
    finish = json.loads(r.stdout.split("FINISH ")[1].splitlines()[0])
    assert metrics["prompt_lens"] == lens.tolist() and metrics["prompt_tokens"] == int(lens.sum())
    assert metrics["prompt_len"] == Tp and len(finish["length"]) == n
    seed = ckpt.synthetic_seed(pipe.model_weights)
    st = [build_device_stage(pipe.model, ckpt.random_stage_state_dict(pipe.model, *nd.layers, i == 0,
                                                                      i == pipe.num_parts - 1, seed, device=DEV),
                             *nd.layers, i == 0, i == pipe.num_parts - 1, torch.device(DEV, 0), dtype=pipe.dtype,
                             max_batch=n, max_seq=Tp + steps, max_tokens=n * (Tp + steps),
                             temperature=pipe.temperature, top_k=pipe.top_k, seed=pipe.seed, top_p=pipe.top_p,
                             min_p=pipe.min_p, stop=pipe.stop) for i, nd in enumerate(pipe.stages)]
    ring = DecodeRing(st, RingLinks(), 1, 1, n)
    want = ring.generate([ids], Tp, steps, lens=[lens])
    torch.cuda.synchronize()
    assert torch.equal(toks, want), (toks.tolist(), want.tolist())
    assert finish["length"] == ring.finished()["length"].tolist()
