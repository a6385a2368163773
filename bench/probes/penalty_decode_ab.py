"""Decode with and without the repetition / presence / frequency penalties,
alternating in one process (box-to-box clock differences cancel): GPT-2 small,
4 stages colocated, B = 64, prompt 512, K = 8 steps per graph.

  greedy_off   greedy (the fused head + argmax merge)
  greedy_on    greedy + penalties: the unfused head, the penalty launch, argmax_rows
  sampled_off  temperature 0.8, top_k 50, top_p 0.95 (configs/gpt2_4stage_1gpu_sampled.json)
  sampled_on   the same + penalties (configs/gpt2_4stage_1gpu_penalised.json)

Every arm keeps its own stages and ring (same seeded weights, same prompts);
each round re-prefills and times ``--steps`` decode steps per arm in turn, a
host clock around work that ends in a device synchronise.  The "off" arms are
built without the penalty arguments: the code path of a build without the
feature.  Also times the penalty launch alone at the decode shape (M = 64 rows
of GPT-2's vocabulary): on one buffer pair (the state table stays in the
caches) and rotating over enough buffer pairs to exceed them; enqueued one by
one (host-bound: the wrapper's enqueue rate) and replayed as one HIP graph of
64 launches, as microseconds and as GB/s of the state table it reads
(M x Vpad x 2 bytes).  ``--launch_only`` runs just that part (for a kernel
trace: ``rocprofv3 --kernel-trace --stats -- python ... --launch_only``).

    python bench/probes/penalty_decode_ab.py [--rounds 3] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PEN = dict(repetition_penalty=1.25, frequency_penalty=0.25)
SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.95, seed=1)
ARMS = [("greedy_off", dict()), ("greedy_on", dict(PEN)), ("sampled_off", dict(SAMPLED)),
        ("sampled_on", dict(SAMPLED, **PEN))]


def build(a, dev, kw):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    ranges = default_ranges(a.model, a.stages)
    S = len(ranges)
    max_seq = a.prompt + a.warmup + a.steps + a.multi_step + 4
    stages = []
    for s, (lo, hi) in enumerate(ranges):
        sd = ckpt.random_stage_state_dict(a.model, lo, hi, s == 0, s == S - 1, 0, device=dev)
        stages.append(TransformerStage(a.model, sd, lo, hi, s == 0, s == S - 1, dev, max_batch=a.batch,
                                       max_seq=max_seq, **kw))
        del sd
    return DecodeRing(stages, RingLinks(), 1, 1, a.batch, use_graphs=True, record=True, multi_step=a.multi_step)


def timed(ring, prompts, a):
    ring.prefill(prompts, a.prompt)
    ring.capture()  # first round only
    ring.decode_rounds(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ring.decode_rounds(a.steps)
    ring.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    toks = ring.tokens()
    assert toks.shape == (a.batch, 1 + a.warmup + a.steps), toks.shape
    return dt / a.steps * 1e3, toks


def launch_alone(dev, M, V, prompt, iters=400):
    """The penalty launch alone at the decode shape, us per launch and GB/s of
    the state table (M x Vpad x 2 bytes): ``prompt`` tokens marked per row and a
    previous token to count, as a decode step has them."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    Vpad = -(-V // 64) * 64
    table = M * Vpad * 2
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V, (M, prompt), generator=g).to(dev)
    prev = torch.randint(0, V, (M,), generator=g, dtype=torch.int32).to(dev)

    def pair():
        st = torch.zeros((M, Vpad), dtype=torch.int16, device=dev)
        st.scatter_(1, ids, -0x8000)
        return (torch.randn(M, Vpad, device=dev) * 3).bfloat16(), st

    res = {"rows": M, "vocab": V, "state_table_bytes": table, "iters": iters}
    # 1 pair: the table stays cache-resident between launches; 64 pairs (logits + state, 2 x 6.4 MB each):
    # 0.8 GB, more than the 256 MB last-level cache, so every launch reads its table from HBM
    for name, n in (("same_buffers", 1), ("rotating_64_buffers", 64)):
        pairs = [pair() for _ in range(n)]
        for i in range(max(10, n)):
            T.logit_penalties(*pairs[i % n], prev, 1.25, 0.25, 0.0, V)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            T.logit_penalties(*pairs[i % n], prev, 1.25, 0.25, 0.0, V)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / iters * 1e3
        # the same launches as one HIP graph (as a decode step runs them): no host enqueue cost per launch
        n_g = max(n, 64)
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                for i in range(n_g):
                    T.logit_penalties(*pairs[i % n], prev, 1.25, 0.25, 0.0, V)
        torch.cuda.current_stream(dev).wait_stream(s)
        graph.replay()
        torch.cuda.synchronize()
        reps = 20
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us_g = e0.elapsed_time(e1) / (reps * n_g) * 1e3
        res[name] = {"eager_us": round(us, 2), "graph_us": round(us_g, 2),
                     "graph_state_GBps": round(table / (us_g * 1e-6) / 1e9, 1)}
        del graph, pairs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--stages", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--multi_step", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--launch_only", action="store_true")
    a = ap.parse_args()
    from distributed_neural_networks_amd.models import model_info
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V = model_info(a.model).cfg.vocab_size
    if a.launch_only:
        print(json.dumps({"probe": "penalty_launch", "penalty_launch": launch_alone(dev, a.batch, V, a.prompt)}),
              flush=True)
        return
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)]
    rings = [(name, build(a, dev, kw)) for name, kw in ARMS]
    ms = {name: [] for name, _ in rings}
    toks, stable = {}, {}
    for _ in range(a.rounds):
        for name, ring in rings:
            t, tk = timed(ring, prompts, a)
            ms[name].append(round(t, 4))
            if name in toks:
                stable[name] = stable.get(name, True) and bool(torch.equal(toks[name], tk))
            toks[name] = tk
    best = {k: min(v) for k, v in ms.items()}

    def distinct(t):  # mean number of distinct tokens per generated row: what the penalties are for
        return round(sum(len(set(r.tolist())) for r in t) / t.shape[0], 2)
    rec = {"probe": "penalty_decode_ab", "model": a.model, "stages": a.stages, "batch": a.batch, "prompt": a.prompt,
           "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step, "rounds": a.rounds, "penalties": PEN,
           "sampling": SAMPLED, "ms_per_step": ms, "ms_per_step_min": best,
           "greedy_on_minus_off_us": round((best["greedy_on"] - best["greedy_off"]) * 1e3, 1),
           "sampled_on_minus_off_us": round((best["sampled_on"] - best["sampled_off"]) * 1e3, 1),
           "graph_k": {name: ring.graph_k is not None for name, ring in rings},
           "tokens_same_every_round": stable, "distinct_tokens_per_row": {k: distinct(v) for k, v in toks.items()},
           "penalty_launch": launch_alone(dev, a.batch, V, a.prompt), "device": torch.cuda.get_device_name(dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "penalties_decode_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
