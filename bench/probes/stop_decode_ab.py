"""Decode with and without stop conditions, alternating in one process
(box-to-box clock differences cancel): GPT-2 small, 4 stages colocated,
B = 64, prompt 512, K = 8 steps per graph, greedy and sampled (temperature
0.8, top_k 50, top_p 0.95: configs/gpt2_4stage_1gpu_sampled.json), each as

  off       built without the argument (the graphs of a build without the feature)
  ids       16 stop ids
  ids_seqs  16 stop ids and 8 stop sequences of 16 tokens
  ids_min   16 stop ids and min_new_tokens past the end of the run: the
            suppression launch in every step, and greedy loses the fused head

The stop ids and sequences are ids that the "off" arms never generate, so no
row stops and every arm runs the same rounds; the stop arms keep the early-exit
check (a pinned copy of the state and an event per K-step replay).  Every arm
keeps its own stages and ring (same seeded weights, same prompts); each round
re-prefills and times ``--steps`` decode steps per arm in turn, a host clock
around work that ends in a device synchronise.  ``--parent_root DIR`` (a built
checkout of the parent commit) also measures the two "off" arms on the
parent's library, in a child process before and one after this process's own
rounds.  Also: the stop launch and the suppression launch alone at M = 64 as a
HIP graph of 64 launches, next to the penalty launch measured the same way in
the same process; and the early-exit case: 64 equal prompts, greedy, a stop
sequence that ends every row at token 16 of 128, wall time of the decode
against the same ring without stop conditions.

    python bench/probes/stop_decode_ab.py [--rounds 3] [--parent_root DIR] [--out profiles]
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


def build(a, dev, kw, batch=None, max_seq=None):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.transformer import TransformerStage
    ranges = default_ranges(a.model, a.stages)
    S = len(ranges)
    max_seq = max_seq or a.prompt + a.warmup + a.steps + a.multi_step + 4
    stages = []
    for s, (lo, hi) in enumerate(ranges):
        sd = ckpt.random_stage_state_dict(a.model, lo, hi, s == 0, s == S - 1, 0, device=dev)
        stages.append(TransformerStage(a.model, sd, lo, hi, s == 0, s == S - 1, dev, max_batch=batch or a.batch,
                                       max_seq=max_seq, **(kw if s == S - 1 else {})))
        del sd
    return DecodeRing(stages, RingLinks(), 1, 1, batch or a.batch, use_graphs=True, record=True,
                      multi_step=a.multi_step)


def timed(ring, prompts, a):
    ring.prefill(prompts, a.prompt)
    ring.capture()  # first round only
    ring.decode_rounds(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ran = ring.decode_rounds(a.steps)
    ring.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    toks = ring.tokens()
    assert ran in (None, a.steps) and toks.shape == (a.batch, 1 + a.warmup + a.steps), (ran, toks.shape)
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


def unused_ids(toks, V, n):
    used = set()
    for t in toks:
        used |= set(t.flatten().tolist())
    out, i = [], V - 1
    while len(out) < n:
        if i not in used:
            out.append(i)
        i -= 1
    return out


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


def launches_alone(dev, M, V, prompt, ids, seqs):
    """The stop launch, the suppression launch and, as the yardstick, the penalty
    launch (same buffers: its state table stays cache-resident) at M rows."""
    from distributed_neural_networks_amd.ops import transformer_ops as T
    Vpad = -(-V // 64) * 64
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V - 64, (M,), generator=g, dtype=torch.int32).to(dev)
    also = tok.clone()
    hist = torch.zeros((M, 64), dtype=torch.int32, device=dev)
    pos = torch.full((M,), 5, dtype=torch.int32, device=dev)
    logits = (torch.randn(M, Vpad, device=dev) * 3).bfloat16()
    res = {"rows": M}
    for name, i, q in (("stop_rows_16_ids", ids, ()), ("stop_rows_16_ids_8_seqs", ids, seqs), ("stop_rows_1_id", ids[:1], ())):
        st = T.stop_state(M, dev)
        res[name + "_graph_us"] = graph_us(dev, lambda: T.stop_rows(tok, st, i, q, 0, 0, also=also, hist=hist, pos=pos,
                                                                    pos_off=-1))
    st = T.stop_state(M, dev)
    st[:, 1] = 3  # every row finished: the pad path (three stores per row)
    res["stop_rows_all_finished_graph_us"] = graph_us(dev, lambda: T.stop_rows(tok, st, ids, seqs, 0, 0, also=also,
                                                                              hist=hist, pos=pos, pos_off=-1))
    st0 = T.stop_state(M, dev)
    res["stop_suppress_16_ids_graph_us"] = graph_us(dev, lambda: T.stop_suppress(logits, V, st0, ids, 1 << 20))
    pids = torch.randint(0, V, (M, prompt), generator=g).to(dev)
    pst = torch.zeros((M, Vpad), dtype=torch.int16, device=dev)
    pst.scatter_(1, pids, -0x8000)
    res["penalty_launch_graph_us"] = graph_us(dev, lambda: T.logit_penalties(logits, pst, tok, 1.25, 0.25, 0.0, V))
    return res


def early_exit_case(a, dev, V, total=128, at=16):
    """64 equal prompts, greedy: every row generates the same tokens, so one
    stop sequence (the shortest n-gram ending at token ``at`` that has not
    occurred before) ends them all at token ``at`` of ``total``."""
    from distributed_neural_networks_amd.config import StopConfig
    g = torch.Generator().manual_seed(11)
    one = torch.randint(0, V, (1, a.prompt), generator=g, dtype=torch.int32)
    prompts = [one.repeat(a.batch, 1).to(dev)]
    max_seq = a.prompt + total + a.multi_step + 4

    def decode(ring):
        ring.prefill(prompts, a.prompt)
        ring.capture()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ran = ring.decode_rounds(total - 1)
        ring.drain()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, ran, ring.tokens()

    off = build(a, dev, {}, max_seq=max_seq)
    decode(off)
    ms_off, _, toks = zip(*[decode(off) for _ in range(a.rounds)])
    row = toks[0][0].tolist()
    assert all(r.tolist() == row for r in toks[0])
    seq = None
    for n in range(1, 17):
        cand = row[at - n:at]
        if n <= at and not any(row[j - n:j] == cand for j in range(n, at)):
            seq = cand
            break
    if seq is None:
        return {"skipped": "no n-gram of at most 16 tokens ends at the wanted token for the first time"}
    del off
    on = build(a, dev, dict(stop=StopConfig((), (tuple(seq),), 0, 0)), max_seq=max_seq)
    decode(on)
    res = [decode(on) for _ in range(a.rounds)]
    fin = on.finished()
    return {"tokens": total, "stop_at": at, "stop_sequence_len": len(seq), "multi_step": a.multi_step,
            "off_decode_ms": [round(m, 3) for m in ms_off], "stop_decode_ms": [round(r[0], 3) for r in res],
            "rounds_run": [r[1] for r in res], "lengths": sorted(set(fin["length"].tolist())),
            "tokens_equal_truncated": bool(torch.equal(res[0][2][:, :at], toks[0][:, :at]))}


def parent_run(a):
    """The two "off" arms on the parent checkout's package, in a fresh child process."""
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
    ap.add_argument("--off_only", action="store_true", help="the two off arms only; prints, writes no file")
    a = ap.parse_args()
    parent = [parent_run(a)] if a.parent_root else []  # before this process opens the GPU
    from distributed_neural_networks_amd.models import model_info
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V = model_info(a.model).cfg.vocab_size
    g = torch.Generator().manual_seed(7)
    prompts = [torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)]
    off = [(f"{k}_off", build(a, dev, kw)) for k, kw in KINDS]
    if a.off_only:
        ms, _, stable = run_rounds(a, off, prompts)
        from distributed_neural_networks_amd.ops import _lib
        print(json.dumps({"library": os.path.basename(_lib.library_path()), "ms_per_step": ms,
                          "tokens_same_every_round": stable}), flush=True)
        return
    from distributed_neural_networks_amd.config import StopConfig
    _, toks0, _ = run_rounds(argparse.Namespace(**dict(vars(a), rounds=1)), off, prompts)  # which ids are never generated
    free = unused_ids(toks0.values(), V, 16 + 8 * 16)
    ids, seqs = tuple(free[:16]), tuple(tuple(free[16 + 16 * s:32 + 16 * s]) for s in range(8))
    far = a.warmup + a.steps + 64
    rings = []
    for k, kw in KINDS:
        rings.append(next(r for r in off if r[0] == f"{k}_off"))
        rings.append((f"{k}_ids", build(a, dev, dict(kw, stop=StopConfig(ids, (), 0, ids[0])))))
        rings.append((f"{k}_ids_seqs", build(a, dev, dict(kw, stop=StopConfig(ids, seqs, 0, ids[0])))))
        rings.append((f"{k}_ids_min", build(a, dev, dict(kw, stop=StopConfig(ids, (), far, ids[0])))))
    ms, toks, stable = run_rounds(a, rings, prompts)
    if a.parent_root:
        parent.append(parent_run(a))
    best = {k: min(v) for k, v in ms.items()}
    finished = {name: int((ring.finished()["length"] < 1 + a.warmup + a.steps).sum()) for name, ring in rings
                if ring.stp is not None}
    del rings, off
    rec = {"probe": "stop_decode_ab", "model": a.model, "stages": a.stages, "batch": a.batch, "prompt": a.prompt,
           "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step, "rounds": a.rounds, "sampling": SAMPLED,
           "ms_per_step": ms, "ms_per_step_min": best,
           "added_us_per_step": {k: round((best[k] - best[k.split("_")[0] + "_off"]) * 1e3, 1) for k in best
                                 if not k.endswith("_off")},
           "tokens_same_every_round": stable,
           "tokens_equal_to_off": {k: bool(torch.equal(toks[k], toks[k.split("_")[0] + "_off"])) for k in toks},
           "rows_finished": finished,
           "parent_off_runs": [{"ms_per_step": p["ms_per_step"], "library": p["library"]} for p in parent],
           "launches_alone": launches_alone(dev, a.batch, V, a.prompt, ids, seqs),
           "early_exit": early_exit_case(a, dev, V), "device": torch.cuda.get_device_name(dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "stop_decode_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
