"""Decode with and without logit constraints, alternating in one process
(box-to-box clock differences cancel): GPT-2 small, 4 stages colocated,
B = 64, prompt 512, K = 8 steps per graph, greedy and sampled (temperature
0.8, top_k 50, top_p 0.95: configs/gpt2_4stage_1gpu_sampled.json), each as

  off      built without the argument (the graphs of a build without the feature)
  bias     logit_bias on 256 ids
  bad      bad_words_ids, 64 sequences of 16 tokens
  ngram    no_repeat_ngram_size 3
  allowed  allowed_token_ids, half the vocabulary
  all      the four together

The bias and bad-word ids are ids that the "off" arms never generate (the bias
is negative), and the allowed half holds every id they do generate, so those
arms' constraints never fire and their tokens are compared with "off".  The
n-gram rule fires whenever a row repeats a 3-gram, so its tokens may differ.
Every arm keeps its own stages and ring (same seeded weights, same prompts);
each round re-prefills and times ``--steps`` decode steps per arm in turn, a
host clock around work that ends in a device synchronise.  ``--parent_root DIR``
(a built checkout of the parent commit) also measures the two "off" arms on the
parent's library, in a child process before and one after this process's own
rounds.  ``--trace`` lists the kernel names of one eager decode step of the
greedy and the sampled "off" arm (the parent children do the same, so the two
lists can be compared).  Also: the constraint launch alone at M = 64 as a HIP
graph of 64 launches, next to the penalty launch measured the same way in the
same process.

    python bench/probes/constraints_decode_ab.py [--rounds 3] [--parent_root DIR] [--out profiles]
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
KINDS = (("greedy", {}), ("sampled", SAMPLED))


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


def run_rounds(a, rings, prompts):
    ms = {name: [] for name, _ in rings}
    toks, stable = {}, {}
    for _ in range(a.rounds):
        for name, ring in rings:
            t, tk = timed(ring, prompts, a)
            ms[name].append(round(t, 4))
            if name in toks:
                stable[name] = stable.get(name, True) and bool(torch.equal(toks[name], tk))
            toks[name] = tk
    return ms, toks, stable


def kernel_names(ring, prompts, a):
    """The kernel names of one eager decode step, in launch order."""
    from torch.profiler import ProfilerActivity, profile
    graphs, ring.use_graphs = ring.use_graphs, False  # eager: the profiler sees every launch by name
    try:
        ring.prefill(prompts, a.prompt)
        ring.decode_rounds(1)  # allocations and lazy initialisation outside the trace
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            ring.decode_rounds(1)
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        ev.sort(key=lambda e: e.time_range.start)
        return [e.name for e in ev]
    except Exception as e:  # noqa: BLE001  (a profiler that cannot trace is reported, not hidden)
        return ["error: " + repr(e)]
    finally:
        ring.use_graphs = graphs


def graph_us(dev, fn, reps=20, n=64):
    """us per launch of ``fn`` replayed as one HIP graph of ``n`` launches."""
    fn()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            for _ in range(n):
                fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / (reps * n) * 1e3, 2)


def launches_alone(dev, M, V, prompt, arms):
    """The constraint launch of every arm and, as the yardstick, the penalty
    launch at M rows on contexts of ``prompt`` + 32 tokens."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    Vpad = -(-V // 64) * 64
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V - 64, (M,), generator=g, dtype=torch.int32).to(dev)
    logits = (torch.randn(M, Vpad, device=dev) * 3).bfloat16()
    ctx = torch.randint(0, V, (M, prompt + 64), generator=g, dtype=torch.int32).to(dev)
    pos = torch.full((M,), prompt + 32, dtype=torch.int32, device=dev)
    res = {"rows": M, "context_len": prompt + 33}
    for name, cons in arms.items():
        t = T.constraint_tables(cons, V, dev)
        c = ctx if t.needs_context else None
        res[f"constraints_{name}_graph_us"] = graph_us(
            dev, lambda: T.logit_constraints(logits, V, t, ctx=c, pos=pos if c is not None else None, pos_off=1,
                                             prev=tok if c is not None else None))
    pids = torch.randint(0, V, (M, prompt), generator=g).to(dev)
    pst = torch.zeros((M, Vpad), dtype=torch.int16, device=dev)
    pst.scatter_(1, pids, -0x8000)
    res["penalty_launch_graph_us"] = graph_us(dev, lambda: T.logit_penalties(logits, pst, tok, 1.25, 0.25, 0.0, V))
    return res


def parent_run(a):
    """The two "off" arms on the parent checkout's package, in a fresh child process."""
    cmd = [sys.executable, HERE, "--root", a.parent_root, "--off_only", "--rounds", str(a.rounds), "--steps",
           str(a.steps), "--warmup", str(a.warmup), "--batch", str(a.batch), "--prompt", str(a.prompt), "--multi_step",
           str(a.multi_step), "--model", a.model, "--stages", str(a.stages)] + (["--trace"] if a.trace else [])
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
    ap.add_argument("--off_only", action="store_true", help="the two off arms only; prints, writes no file")
    ap.add_argument("--trace", action="store_true", help="also list the kernel names of one decode step of the off arms")
    a = ap.parse_args()
    parent = [parent_run(a)] if a.parent_root else []  # before this process opens the GPU
    from distributed_neural_networks_amd.models import model_info
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V = model_info(a.model).cfg.vocab_size
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)]
    off = [(f"{k}_off", build(a, dev, kw)) for k, kw in KINDS]
    names = {n: kernel_names(r, prompts, a) for n, r in off} if a.trace else None
    if a.off_only:
        ms, _, stable = run_rounds(a, off, prompts)
        from distributed_neural_networks_amd.ops import _lib
        print(json.dumps({"library": os.path.basename(_lib.library_path()), "ms_per_step": ms,
                          "tokens_same_every_round": stable, "kernel_names": names}), flush=True)
        return
    from distributed_neural_networks_amd.config import ConstraintConfig
    _, toks0, _ = run_rounds(argparse.Namespace(**dict(vars(a), rounds=1)), off, prompts)  # which ids are generated
    used = set(prompts[0].flatten().tolist())
    for t in toks0.values():
        used |= set(t.flatten().tolist())
    free = [i for i in range(V - 1, -1, -1) if i not in used]
    bias = tuple((i, -5.0) for i in free[:256])
    bad = tuple(tuple(free[256 + 16 * s:272 + 16 * s]) for s in range(64))
    gen = set()
    for t in toks0.values():
        gen |= set(t.flatten().tolist())
    allowed = sorted(gen) + [i for i in range(V) if i not in gen][:V // 2 - len(gen)]
    arms = {"bias": ConstraintConfig(bias, None, (), 0), "bad": ConstraintConfig((), None, bad, 0),
            "ngram": ConstraintConfig((), None, (), 3), "allowed": ConstraintConfig((), tuple(allowed), (), 0),
            "all": ConstraintConfig(bias, tuple(allowed), bad, 3)}
    rings = []
    for k, kw in KINDS:
        rings.append(next(r for r in off if r[0] == f"{k}_off"))
        for name, cons in arms.items():
            rings.append((f"{k}_{name}", build(a, dev, dict(kw, constraints=cons))))
    ms, toks, stable = run_rounds(a, rings, prompts)
    if a.parent_root:
        parent.append(parent_run(a))
    best = {k: min(v) for k, v in ms.items()}
    del rings, off
    rec = {"probe": "constraints_decode_ab", "model": a.model, "stages": a.stages, "batch": a.batch,
           "prompt": a.prompt, "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step, "rounds": a.rounds,
           "sampling": SAMPLED, "ms_per_step": ms, "ms_per_step_min": best,
           "added_us_per_step": {k: round((best[k] - best[k.split("_")[0] + "_off"]) * 1e3, 1) for k in best
                                 if not k.endswith("_off")},
           "tokens_same_every_round": stable,
           "tokens_equal_to_off": {k: bool(torch.equal(toks[k], toks[k.split("_")[0] + "_off"])) for k in toks},
           "parent_off_runs": [{"ms_per_step": p["ms_per_step"], "library": p["library"]} for p in parent],
           "launches_alone": launches_alone(dev, a.batch, V, a.prompt, arms), "device": torch.cuda.get_device_name(dev)}
    if a.trace:
        same = {}
        for k, v in names.items():
            par = [(p.get("kernel_names") or {}).get(k) for p in parent]
            same[k] = {"kernels_traced": len(v), "kernel_names_equal": bool(par) and all(q == v for q in par)}
            if par and not same[k]["kernel_names_equal"]:
                same[k]["parent_only"] = sorted(set(par[0] or []) - set(v))
                same[k]["new_only"] = sorted(set(v) - set(par[0] or []))
        rec["off_same_kernels_as_parent"] = same
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "constraints_decode_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
