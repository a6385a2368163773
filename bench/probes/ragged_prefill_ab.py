"""Ragged prompts: what the equal-length path, the ragged machinery and the
pads cost.  GPT-2 small, 4 stages colocated, B = 64, K = 8 steps per graph,
greedy, three arms on ONE ring (the same stages and the same captured graphs),
interleaved in one process, best of ``--rounds``:

  equal    prompts of 512 tokens through the existing path (no lengths given)
  forced   the same prompts through the ragged path (all lengths 512): the
           difference to ``equal`` is the machinery, one gather launch per
           prefill piece and one head call per microbatch
  ragged   lengths uniform in [64, 512] (fixed seed), right-padded to the longest

Each round re-prefills (host clock around work that ends in a device
synchronise) and times ``--steps`` decode steps per arm in turn.
``--parent_root DIR`` (a built checkout of the parent commit) also measures the
``equal`` arm on the parent's package, in a child process before and one after
this process's own rounds, and before either compares the parent's token output
and the kernel names of one traced prefill + decode step (torch.profiler, in
child processes of their own) with this checkout's.

    python bench/probes/ragged_prefill_ab.py [--rounds 3] [--parent_root DIR] [--out profiles]
"""
import argparse
import hashlib
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


def build(a, dev):
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
        stages.append(TransformerStage(a.model, sd, lo, hi, s == 0, s == S - 1, dev, max_batch=a.batch, max_seq=max_seq))
        del sd
    return DecodeRing(stages, RingLinks(), 1, 1, a.batch, use_graphs=True, record=True, multi_step=a.multi_step)


def timed(ring, prompts, a, lens=None):
    """(prefill ms, decode ms per step, tokens) of one generation."""
    kw = {} if lens is None else {"lens": lens}  # the parent's prefill has no such argument
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ring.prefill(prompts, a.prompt, **kw)
    torch.cuda.synchronize()
    pf = time.perf_counter() - t0
    ring.capture()  # first generation only
    ring.decode_rounds(a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ring.decode_rounds(a.steps)
    ring.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    toks = ring.tokens()
    assert toks.shape == (a.batch, 1 + a.warmup + a.steps), toks.shape
    return pf * 1e3, dt / a.steps * 1e3, toks


def digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()[:16]


def make_prompts(a, dev):
    from distributed_neural_networks_amd.models import model_info
    g = torch.Generator().manual_seed(7)
    V = model_info(a.model).cfg.vocab_size
    return torch.randint(0, V, (a.batch, a.prompt), generator=g, dtype=torch.int32).to(dev)


def kernel_names(a, dev):
    """The device kernels of one eager equal-length prefill and one eager decode step, in launch order."""
    from torch.profiler import ProfilerActivity, profile
    ring = build(a, dev)
    ring.use_graphs = False  # eager: the profiler sees every launch by name
    prompts = [make_prompts(a, dev)]
    ring.prefill(prompts, a.prompt)  # allocations and lazy initialisation outside the trace
    ring.decode_rounds(1)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        ring.prefill(prompts, a.prompt)
        ring.decode_rounds(1)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ev.sort(key=lambda e: e.time_range.start)
    return [e.name for e in ev]


def child(a, mode, root):
    cmd = [sys.executable, HERE, "--root", root, mode, "--rounds", str(a.rounds), "--steps", str(a.steps), "--warmup",
           str(a.warmup), "--batch", str(a.batch), "--prompt", str(a.prompt), "--multi_step", str(a.multi_step),
           "--model", a.model, "--stages", str(a.stages)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child run failed ({mode}, {root}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--stages", type=int, default=4)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--min_prompt", type=int, default=64)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--multi_step", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--root", default=None, help="package root to measure (default: this checkout)")
    ap.add_argument("--parent_root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--equal_only", action="store_true", help="the equal arm only; prints, writes no file")
    ap.add_argument("--names_only", action="store_true", help="the kernel names of one traced step; prints them")
    a = ap.parse_args()
    same = None
    parent = []
    if a.parent_root:  # before this process opens the GPU
        here = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
        n_par, n_new = child(a, "--names_only", a.parent_root), child(a, "--names_only", here)
        same = {"kernels_traced": len(n_new["kernels"]), "kernel_names_equal": n_par["kernels"] == n_new["kernels"],
                "trace_error": n_par.get("error") or n_new.get("error")}
        if not same["kernel_names_equal"]:
            same["parent_only"] = sorted(set(n_par["kernels"]) - set(n_new["kernels"]))
            same["new_only"] = sorted(set(n_new["kernels"]) - set(n_par["kernels"]))
        parent.append(child(a, "--equal_only", a.parent_root))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.names_only:
        try:
            print(json.dumps({"kernels": kernel_names(a, dev)}), flush=True)
        except Exception as e:  # noqa: BLE001  (a profiler that cannot trace is reported, not hidden)
            print(json.dumps({"kernels": [], "error": repr(e)}), flush=True)
        return
    prompts = [make_prompts(a, dev)]
    ring = build(a, dev)
    if a.equal_only:
        timed(ring, prompts, a)  # capture and first-use costs outside the rounds
        res = [timed(ring, prompts, a) for _ in range(a.rounds)]
        from distributed_neural_networks_amd.ops import _lib
        print(json.dumps({"library": _lib.library_path(), "prefill_ms": [round(r[0], 3) for r in res],
                          "decode_ms_per_step": [round(r[1], 4) for r in res], "tokens": digest(res[0][2]),
                          "tokens_same_every_round": all(digest(r[2]) == digest(res[0][2]) for r in res)}), flush=True)
        return
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(a.min_prompt, a.prompt + 1, (a.batch,), generator=g, dtype=torch.int32)
    lens[0] = a.prompt  # the longest prompt stays 512: the same pieces as the other arms
    arms = {"equal": None, "forced": [torch.full((a.batch,), a.prompt, dtype=torch.int32)], "ragged": [lens]}
    for ln in arms.values():  # capture and first-use costs outside the rounds
        timed(ring, prompts, a, ln)
    pf = {k: [] for k in arms}
    dec = {k: [] for k in arms}
    toks = {}
    for _ in range(a.rounds):
        for name, ln in arms.items():
            p, d, t = timed(ring, prompts, a, ln)
            pf[name].append(round(p, 3))
            dec[name].append(round(d, 4))
            toks[name] = t
    if a.parent_root:
        parent.append(child(a, "--equal_only", a.parent_root))
    real = int(lens.sum())
    padded = a.batch * a.prompt
    best_pf = {k: min(v) for k, v in pf.items()}
    best_dec = {k: min(v) for k, v in dec.items()}
    rec = {"probe": "ragged_prefill_ab", "model": a.model, "stages": a.stages, "batch": a.batch, "prompt": a.prompt,
           "min_prompt": a.min_prompt, "steps": a.steps, "warmup": a.warmup, "multi_step": a.multi_step,
           "rounds": a.rounds, "prefill_ms": pf, "decode_ms_per_step": dec, "prefill_ms_min": best_pf,
           "decode_ms_per_step_min": best_dec,
           "machinery_prefill_us": round((best_pf["forced"] - best_pf["equal"]) * 1e3, 1),
           "forced_tokens_equal_to_equal": bool(torch.equal(toks["forced"], toks["equal"])),
           "ragged": {"real_tokens": real, "padded_tokens": padded, "pad_share": round(1 - real / padded, 4),
                      "real_tokens_per_s": round(real / best_pf["ragged"] * 1e3, 1),
                      "padded_tokens_per_s": round(padded / best_pf["ragged"] * 1e3, 1),
                      "equal_tokens_per_s": round(padded / best_pf["equal"] * 1e3, 1)},
           "parent_equal_runs": [{"prefill_ms": p["prefill_ms"], "decode_ms_per_step": p["decode_ms_per_step"],
                                  "tokens_equal_to_equal_arm": p["tokens"] == digest(toks["equal"])} for p in parent],
           "same_kernels_as_parent": same, "device": torch.cuda.get_device_name(dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ragged_prompts_ab.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
