"""End-to-end cost of ``prompt_logprobs``: GPT-2 small, 4 stages colocated,
B = 64, prompt 512, one prefill per round with the key 0 and 1 in turn in one
process (two rings on their own stages, same weights), median of ``--rounds``
with the min-max spread.  Host clock around work that ends in a device
synchronise.  One JSON line.

    python bench/probes/prompt_logprobs_prefill_ab.py [--rounds 7] [--out profiles/prompt_logprobs_prefill_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402


def build(a, dev, key):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    ranges = default_ranges(a.model, a.stages)
    S = len(ranges)
    stages = []
    for s, (lo, hi) in enumerate(ranges):
        sd = ckpt.random_stage_state_dict(a.model, lo, hi, s == 0, s == S - 1, 0, device=dev)
        stages.append(TransformerStage(a.model, sd, lo, hi, s == 0, s == S - 1, dev, max_batch=a.batch,
                                       max_seq=a.prompt + 8, prompt_logprobs=key if s == S - 1 else 0))
        del sd
    return DecodeRing(stages, RingLinks(), 1, 1, a.batch, use_graphs=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--stages", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from distributed_neural_networks_amd.models import model_info
    dev = torch.device("cuda", 0)
    V = model_info(a.model).cfg.vocab_size
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=torch.Generator().manual_seed(7), dtype=torch.int32)]
    rings = {k: build(a, dev, k) for k in (0, 1)}
    ms = {0: [], 1: []}
    for r in range(a.rounds + 1):  # round 0 warms up (allocations, first launches)
        for k in (0, 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rings[k].prefill(prompts, a.prompt)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    ntok = a.batch * a.prompt
    rec = {"model": a.model, "batch": a.batch, "prompt": a.prompt, "rounds": a.rounds}
    for k, name in ((0, "off"), (1, "on")):
        med = statistics.median(ms[k])
        rec[name] = {"prefill_ms": round(med, 3), "minmax_ms": [round(min(ms[k]), 3), round(max(ms[k]), 3)],
                     "tokens_per_s": round(ntok / med * 1e3)}
    lp = rings[1].prompt_logprobs()[0]["tok_lp"]
    rec["mean_nll_seq0"] = round(float(-lp[0][1:].double().mean()), 4)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
