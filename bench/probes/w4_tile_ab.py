"""MXFP4 projections at 129..32768 rows, two arms alternating in one process
per shape:

  tile    ``linear_w4(..., tile=True)``: ``dnn_gemm_w4_tile`` on the codes
          (``mxfp4_prefill: "w4a16"``)
  expand  ``linear_w4(..., scratch=)``: ``dnn_w4_expand`` + the bf16 tile GEMM
          (``mxfp4_prefill: "bf16"``, which stays in the build)

Shapes (K -> N): GPT-2 small's QKV and c_proj, GPT-2 XL's c_fc and c_proj,
Llama-3 8B's QKV, gate|up and down, and the GPT-2 vocabulary head.  Each arm
is a HIP graph of launches rotating over weight copies past the 256 MB MALL
(fewer launches where one takes milliseconds); a round replays the graphs in
turn; the figures are the median, min and max over ``--rounds`` of time per
launch.  One JSON line per (shape, M) goes to ``--out``/w4_tile_ab.jsonl.

    python bench/probes/w4_tile_ab.py [--rounds 5] [--launches 16] [--out profiles]

``--e2e MODEL:STAGES`` appends the end-to-end pair instead: bench/gpt_bench.py
with ``--dtype mxfp4`` and ``--mxfp4-prefill`` bf16 / w4a16 alternating in this
one process, prefill tokens/s and decode ms/step at B = 512 and 1024.
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

SHAPES = [("gpt2 qkv", 768, 2304), ("gpt2 proj", 3072, 768), ("gpt2-xl fc", 1600, 6400),
          ("gpt2-xl proj", 6400, 1600), ("llama3-8b qkv", 4096, 6144), ("llama3-8b gate|up", 4096, 28672),
          ("llama3-8b down", 14336, 4096), ("gpt2 head", 768, 50257)]
MS = (129, 384, 512, 1024, 2048, 8192, 32768)
GRAPH_FLOP = 4e13  # at most this much work per graph replay


def child(a):
    import torch
    from distributed_neural_networks_amd.ops import w4
    name, K, N = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    copies = max(2, min(512, -(-ROTATE_BYTES // (N * K // 2))))  # of the 4-bit weight, past the MALL
    q4 = w4.quantize_weight_mxfp4(W, dev)
    w4s = [w4.Mxfp4Weight(q4.q.clone(), q4.scales.clone(), N, K) for _ in range(copies)]
    scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
    dq = w4.dequantize(q4)
    for M in MS:
        n = max(2, min(max(a.launches, copies), int(GRAPH_FLOP // (2.0 * M * N * K))))
        x = torch.randn(M, K, device=dev).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        arms = {"tile": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, tile=True),
                "expand": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, scratch=scratch)}
        ref = x[-128:].float() @ dq.t()  # the last rows: the partial last block at 129
        err = ((arms["tile"](0)[-128:].float() - ref).norm() / ref.norm()).item()
        assert err < 1e-2, err  # a time means something only for a right result
        t = time_graphs({k: graph_of(f, n) for k, f in arms.items()}, a.rounds, n)
        ln = {"probe": "w4_tile_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies, "launches": n,
              "rounds": a.rounds, "tile_rel_err": err}
        for k, (med, lo, hi) in t.items():
            ln.update({f"{k}_us": round(med, 2), f"{k}_min_us": round(lo, 2), f"{k}_max_us": round(hi, 2)})
        ln["tile_tflops"] = round(2.0 * M * N * K / t["tile"][0] / 1e6, 1)
        # tile wins a case when its slowest round beats the expansion's fastest round, and loses the other way round
        ln["tile_wins"] = bool(t["tile"][2] < t["expand"][1])
        ln["tile_loses"] = bool(t["tile"][1] > t["expand"][2])
        print("RESULT " + json.dumps(ln), flush=True)
        del x, out, ref


def e2e(a):
    """``--e2e MODEL:STAGES``: prefill and decode of bench/gpt_bench.py (one GPU, ``dtype: "mxfp4"``) in this one
    process, the two ``mxfp4_prefill`` modes alternating, ``--rounds`` runs of each per batch; one JSON line per
    batch with the prefill tokens/s and the decode ms/step of every run."""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import gpt_bench
    model, stages = a.e2e.split(":")
    for batch in (512, 1024):
        res = {m: {"prefill_tok_s": [], "ms_per_step": []} for m in ("bf16", "w4a16")}
        for _ in range(a.rounds):
            for mode in res:
                ga = gpt_bench.parse(["--gpus", "1", "--model", model, "--stages", stages, "--batch", str(batch),
                                      "--dtype", "mxfp4", "--mxfp4-prefill", mode, "--steps", "32", "--warmup", "4",
                                      "--prompt", "64", "--prefill_iters", "2", "--verify_steps", "0"])
                r = gpt_bench.run(ga)
                res[mode]["ms_per_step"].append(r["ms_per_step"])
                res[mode]["prefill_tok_s"].append(r.get("prefill_tokens_per_s"))
        ln = {"probe": "w4_tile_ab", "e2e": a.e2e, "batch": batch, "steps": 32, "prompt": 64, **res}
        with open(os.path.join(a.out, "w4_tile_ab.jsonl"), "a") as f:
            f.write(json.dumps(ln) + "\n")
        print(json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--e2e", default="", help="MODEL:STAGES: the end-to-end pairs instead of the shapes")
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
    path = os.path.join(a.out, "w4_tile_ab.jsonl")
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
