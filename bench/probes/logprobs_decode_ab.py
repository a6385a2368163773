"""Decode with and without per-token log-probabilities, alternating in one
process (box-to-box clock differences cancel): GPT-2 small, 4 stages
colocated, B = 64, prompt 512, K = 8 steps per graph, greedy and sampled
(temperature 0.8, top_k 50, top_p 0.95: configs/gpt2_4stage_1gpu_sampled.json),
each with ``logprobs`` 0 / 1 / 5 / 20 (configs/gpt2_4stage_1gpu_logprobs.json
is sampled + 5).

Every arm keeps its own stages and ring (same seeded weights, same prompts);
each round re-prefills and times ``--steps`` decode steps per arm in turn, a
host clock around work that ends in a device synchronise.  The "0" arms are
built without the argument.  ``--parent_root DIR`` (a built checkout of the
parent commit) also measures the two "0" arms on the parent's library, in a
child process before and one after this process's own rounds: "off" must equal
the parent within the spread of the parent's own runs.  Also times the
log-probability launch alone at the decode shape (M = 64 rows of GPT-2's
vocabulary) per n: on one logits buffer (cache-resident) and rotating over 64
buffers (0.4 GB, past the 256 MB last-level cache), replayed as one HIP graph
of 64 launches; the yardstick is the penalty launch on the same bytes
(profiles/penalties_decode_ab.jsonl: 3.4 us cache-resident, 5.0 us from HBM).

    python bench/probes/logprobs_decode_ab.py [--rounds 3] [--parent_root DIR] [--out profiles]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if "--root" in sys.argv:  # measure another checkout's package (the parent commit's) with this file
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.95, seed=1)
NS = (0, 1, 5, 20)


def arms(ns):
    out = []
    for kind, kw in (("greedy", {}), ("sampled", SAMPLED)):
        for n in ns:
            out.append((f"{kind}_{n}", dict(kw, **({"logprobs": n} if n else {}))))
    return out


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
                                       max_seq=max_seq, **(kw if s == S - 1 else {})))
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


def launch_alone(dev, M, V, reps=20):
    """The log-probability launch alone at the decode shape, us per launch, per n."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    Vpad = -(-V // 64) * 64
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V, (M,), generator=g, dtype=torch.int32).to(dev)
    pos = torch.zeros((M,), dtype=torch.int32, device=dev)
    res = {"rows": M, "vocab": V, "logits_bytes": M * Vpad * 2}
    for name, nb in (("same_buffer", 1), ("rotating_64_buffers", 64)):
        bufs = [(torch.randn(M, Vpad, device=dev) * 3).bfloat16() for _ in range(nb)]
        res[name] = {}
        for n in NS:
            ws = T.logprobs_workspace(M, V, n, dev)
            c = torch.zeros((M, 4), dtype=torch.float32, device=dev)
            i = torch.zeros((M, 4, max(n, 1)), dtype=torch.int32, device=dev)
            t = torch.zeros((M, 4, max(n, 1)), dtype=torch.float32, device=dev)

            def run(k):
                T.logprobs_rows(bufs[k % nb], tok, V, n, c, i if n else None, t if n else None, ws, pos=pos)
            run(0)
            graph = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                with torch.cuda.graph(graph, stream=s):
                    for k in range(64):
                        run(k)
            torch.cuda.current_stream(dev).wait_stream(s)
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name][f"n{n}_graph_us"] = round(e0.elapsed_time(e1) / (reps * 64) * 1e3, 2)
            del graph
        del bufs
    return res


def measure(a, ns, dev):
    from distributed_neural_networks_amd.models import model_info
    V = model_info(a.model).cfg.vocab_size
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)]
    rings = [(name, build(a, dev, kw)) for name, kw in arms(ns)]
    ms = {name: [] for name, _ in rings}
    toks, stable = {}, {}
    for _ in range(a.rounds):
        for name, ring in rings:
            t, tk = timed(ring, prompts, a)
            ms[name].append(round(t, 4))
            if name in toks:
                stable[name] = stable.get(name, True) and bool(torch.equal(toks[name], tk))
            toks[name] = tk
    same = {k: bool(torch.equal(toks[k], toks[k.split("_")[0] + "_0"])) for k in toks}
    return {"ms_per_step": ms, "ms_per_step_min": {k: min(v) for k, v in ms.items()},
            "graph_k": {name: ring.graph_k is not None for name, ring in rings},
            "tokens_same_every_round": stable, "tokens_equal_to_off": same}, V


def parent_run(a):
    """The two "0" arms on the parent checkout's package, in a fresh child process."""
    cmd = [sys.executable, HERE, "--root", a.parent_root, "--off_only", "--rounds", str(a.rounds), "--steps",
           str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch), "--prompt", str(a.prompt), "--multi_step",
           str(a.multi_step), "--model", a.model, "--stages", str(a.stages)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"parent run failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


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
    ap.add_argument("--root", default=None, help="package root to measure (default: this checkout)")
    ap.add_argument("--parent_root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent_label", default="parent commit, built in its own checkout",
                    help="what the record calls the --parent_root runs")
    ap.add_argument("--off_only", action="store_true", help="the two logprobs = 0 arms only; prints, writes no file")
    a = ap.parse_args()
    parent = [parent_run(a)] if a.parent_root else []  # before this process opens the GPU
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.off_only:
        res, _ = measure(a, (0,), dev)
        from distributed_neural_networks_amd.ops import _lib
        print(json.dumps({"library": os.path.basename(_lib.library_path()), **res}), flush=True)
        return
    res, V = measure(a, NS, dev)
    if a.parent_root:
        parent.append(parent_run(a))
    best = res["ms_per_step_min"]
    rec = {"probe": "logprobs_decode_ab", "model": a.model, "stages": a.stages, "batch": a.batch, "prompt": a.prompt,
           "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step, "rounds": a.rounds, "sampling": SAMPLED,
           **res,
           "added_us_per_step": {f"{k}_{n}": round((best[f"{k}_{n}"] - best[f"{k}_0"]) * 1e3, 1)
                                 for k in ("greedy", "sampled") for n in NS[1:]},
           "parent_off_runs": [{"label": a.parent_label, "ms_per_step": p["ms_per_step"], "library": p["library"]}
                               for p in parent],
           "logprobs_launch": launch_alone(dev, a.batch, V), "device": torch.cuda.get_device_name(dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "logprobs_decode_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
