"""MXFP4 decode projections at 96..256 rows on narrow shapes, three arms
alternating in one process per shape:

  mn      ``linear_w4(..., mn=True)``: ``dnn_gemm_w4_mn`` on the codes
  mid     ``linear_w4`` without a scratch: ``dnn_gemm_w4_mid`` on the codes
  expand  ``linear_w4(..., scratch=)``: ``dnn_w4_expand`` + the bf16 tile GEMM
          (what a decode step of these shapes ran before the mn kernel)

Shapes (K -> N): every projection of GPT-2 small, GPT-2 large's QKV, GPT-2
XL's attention output and c_proj, and two guards that the mid kernel already
wins (1600 -> 4800, 4096 -> 6144).  Each arm is a HIP graph of launches
rotating over weight copies past the 256 MB MALL; a round replays the graphs
in turn; the figures are the median, min and max over ``--rounds`` of time per
launch.  One JSON line per (shape, M) goes to ``--out``/w4_mn_ab.jsonl.

    python bench/probes/w4_mn_ab.py [--rounds 5] [--launches 16] [--out profiles]

``--e2e MODEL:STAGES:BATCH`` appends the end-to-end pair instead (``e2e``).
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from w4_decode_ab import ROTATE_BYTES, graph_of  # noqa: E402
from w4_mid_ab import time_graphs  # noqa: E402

SHAPES = [("gpt2 o", 768, 768), ("gpt2 qkv", 768, 2304), ("gpt2 fc", 768, 3072), ("gpt2 proj", 3072, 768),
          ("gpt2-large qkv", 1280, 3840), ("gpt2-xl o", 1600, 1600), ("gpt2-xl proj", 6400, 1600),
          ("gpt2-xl qkv (guard)", 1600, 4800), ("llama3-8b qkv (guard)", 4096, 6144)]
MS = (96, 128, 256)


def child(a):
    import torch
    from distributed_neural_networks_amd.ops import w4
    name, K, N = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    copies = max(2, min(512, -(-ROTATE_BYTES // (N * K // 2))))  # of the 4-bit weight, past the MALL
    n = max(a.launches, copies)
    q4 = w4.quantize_weight_mxfp4(W, dev)
    w4s = [w4.Mxfp4Weight(q4.q.clone(), q4.scales.clone(), N, K) for _ in range(copies)]
    scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
    dq = w4.dequantize(q4)
    for M in MS:
        x = torch.randn(M, K, device=dev).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        arms = {"mn": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, mn=True),
                "mid": lambda i: w4.linear_w4(x, w4s[i % copies], out=out),
                "expand": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, scratch=scratch)}
        ref = x.float() @ dq.t()
        err = ((arms["mn"](0).float() - ref).norm() / ref.norm()).item()
        assert err < 1e-2, err  # a time means something only for a right result
        t = time_graphs({k: graph_of(f, n) for k, f in arms.items()}, a.rounds, n)
        ln = {"probe": "w4_mn_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies, "rounds": a.rounds,
              "mn_rel_err": err}
        for k, (med, lo, hi) in t.items():
            ln.update({f"{k}_us": round(med, 2), f"{k}_min_us": round(lo, 2), f"{k}_max_us": round(hi, 2)})
        # mn wins a case when its slowest round beats the fastest round of both other arms
        ln["mn_wins"] = bool(t["mn"][2] < min(t["mid"][1], t["expand"][1]))
        print("RESULT " + json.dumps(ln), flush=True)


def e2e(a):
    """``--e2e MODEL:STAGES:BATCH``: the bench/gpt_bench.py decode (one GPU, ``dtype: "mxfp4"``) in this one
    process, alternating the parent's routing (``w4_mn_ok`` held False: these shapes expand) with the present
    one, ``--rounds`` runs of each; one JSON line with the ms/step of every run."""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import gpt_bench
    from distributed_neural_networks_amd.ops import w4
    model, stages, batch = a.e2e.split(":")
    ga = gpt_bench.parse(["--gpus", "1", "--model", model, "--stages", stages, "--batch", batch, "--dtype", "mxfp4",
                          "--steps", "64", "--warmup", "8", "--prompt", "64", "--prefill_iters", "1",
                          "--verify_steps", "0"])
    mn_ok, ms = w4.w4_mn_ok, {"expand": [], "mn": []}
    for _ in range(a.rounds):
        for arm in ("expand", "mn"):
            w4.w4_mn_ok = mn_ok if arm == "mn" else (lambda M, N, K: False)
            ms[arm].append(gpt_bench.run(ga)["ms_per_step"])
    w4.w4_mn_ok = mn_ok
    ln = {"probe": "w4_mn_ab", "e2e": a.e2e, "steps": 64, "prompt": 64, "expand_ms_per_step": ms["expand"],
          "mn_ms_per_step": ms["mn"], "mn_wins": max(ms["mn"]) < min(ms["expand"])}
    with open(os.path.join(a.out, "w4_mn_ab.jsonl"), "a") as f:
        f.write(json.dumps(ln) + "\n")
    print(json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", default="", help="MODEL:STAGES:BATCH: the end-to-end pair instead of the shapes")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shape", type=int, default=-1, help="child: index into SHAPES")
    a = ap.parse_args()
    if a.rounds < 3:
        raise SystemExit("at least three rounds")
    if a.shape >= 0:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    if a.e2e:
        return e2e(a)
    path = os.path.join(a.out, "w4_mn_ab.jsonl")
    with open(path, "w") as f:
        for i in range(len(SHAPES)):  # one fresh process per shape, one at a time
            r = subprocess.run([sys.executable, HERE, "--shape", str(i), "--rounds", str(a.rounds), "--launches",
                                str(a.launches)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"shape {SHAPES[i][0]}: child exited {r.returncode}")
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT "):
                    f.write(ln[7:] + "\n")
                    f.flush()
                    print(ln[7:], flush=True)
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
