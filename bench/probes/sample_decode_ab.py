"""Greedy vs sampled decode, alternating in one process (box-to-box clock
differences cancel): GPT-2 small, 4 stages colocated, B = 64, prompt 512.

  a  greedy
  b  temperature 0.8, top_k 50, unfused tail (sample_topk + ids copy + position
     add + cur copy), single-step graphs: the behaviour before sample_rows
  c  the same draw with the fused tail and K steps per graph
  d  c + top_p 0.95
  e  d + min_p 0.05

Every variant keeps its own stages and ring (same seeded weights, same
prompts); each round re-prefills and times ``--steps`` decode steps per variant
in turn.  The ring records tokens (``record=True``), as a generation does.
Also times the sampler launch alone at B = 1, N = 128256 (Llama-3's vocabulary).

    python bench/probes/sample_decode_ab.py [--rounds 3] [--out profiles]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

VARIANTS = [("a_greedy", dict(), True, None),
            ("b_topk_unfused_k1", dict(temperature=0.8, top_k=50, seed=1), False, 0),
            ("c_topk_fused", dict(temperature=0.8, top_k=50, seed=1), True, None),
            ("d_topk_top_p", dict(temperature=0.8, top_k=50, seed=1, top_p=0.95), True, None),
            ("e_topk_top_p_min_p", dict(temperature=0.8, top_k=50, seed=1, top_p=0.95, min_p=0.05), True, None)]


def build(a, dev, kw, fused, multi_step):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.ops import transformer_ops as T
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
    T.SAMPLE_FUSED_TAIL = fused  # read when the ring is built and when its graphs are captured
    ring = DecodeRing(stages, RingLinks(), 1, 1, a.batch, use_graphs=True, record=True,
                      multi_step=a.multi_step if multi_step is None else multi_step)
    return ring


def timed(ring, fused, prompts, a):
    from distributed_neural_networks_amd.ops import transformer_ops as T
    T.SAMPLE_FUSED_TAIL = fused
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
    T.SAMPLE_FUSED_TAIL = True
    return dt / a.steps * 1e3, toks


def kernel_times(dev, iters=200):
    """Back-to-back launches of one row of 128256 logits, us per launch."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    N = 128256
    torch.manual_seed(0)
    x = (torch.randn(1, N, device=dev) * 3).bfloat16()
    out = torch.empty(1, device=dev, dtype=torch.int32)
    step = torch.zeros(1, device=dev, dtype=torch.int32)
    part = torch.empty(2 * T.ARGMAX_PART_PER_ROW, device=dev, dtype=torch.int32)
    calls = {
        "argmax_rows": lambda: T.argmax_rows(x, out, N, part=part),
        "sample_topk_k50": lambda: T.sample_topk(x, out, N, 0.8, 50, 1, step),
        "sample_rows_k50": lambda: T.sample_rows(x, out, N, 0.8, 50, seed=1, step=step),
        "sample_rows_k50_p95": lambda: T.sample_rows(x, out, N, 0.8, 50, 0.95, seed=1, step=step),
        "sample_rows_k50_p95_m05": lambda: T.sample_rows(x, out, N, 0.8, 50, 0.95, 0.05, seed=1, step=step),
        "sample_rows_p95_no_topk": lambda: T.sample_rows(x, out, N, 0.8, 0, 0.95, seed=1, step=step),
        "sample_rows_p95_T1.3_no_topk": lambda: T.sample_rows(x, out, N, 1.3, 0, 0.95, seed=1, step=step),
    }
    res = {}
    for name, f in calls.items():
        for _ in range(10):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) / iters * 1e3, 2)
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
    a = ap.parse_args()
    from distributed_neural_networks_amd.models import model_info
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V = model_info(a.model).cfg.vocab_size
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)]
    rings = [(name, build(a, dev, kw, fused, ms), fused) for name, kw, fused, ms in VARIANTS]
    ms = {name: [] for name, _, _ in rings}
    toks, stable = {}, {}
    for _ in range(a.rounds):
        for name, ring, fused in rings:
            t, tk = timed(ring, fused, prompts, a)
            ms[name].append(round(t, 4))
            if name in toks:
                stable[name] = stable.get(name, True) and bool(torch.equal(toks[name], tk))
            toks[name] = tk
    same_bc = bool(torch.equal(toks["b_topk_unfused_k1"], toks["c_topk_fused"]))
    rec = {"probe": "sample_decode_ab", "model": a.model, "stages": a.stages, "batch": a.batch, "prompt": a.prompt,
           "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step, "rounds": a.rounds,
           "ms_per_step": ms, "ms_per_step_min": {k: min(v) for k, v in ms.items()},
           "graph_k": {name: ring.graph_k is not None for name, ring, _ in rings},
           "tokens_b_equal_c": same_bc, "tokens_same_every_round": stable,
           "sampler_us_B1_N128256": kernel_times(dev), "device": torch.cuda.get_device_name(dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sample_decode_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
