"""The greedy vocabulary head with MXFP4, bf16 and e4m3 weights, alternating in
one process per shape: ``head_w4`` with partials + ``argmax_final``
(csrc/kernels/gemm_w4_head.h) against ``head_argmax`` on the bf16 and on the
e4m3 folded head, and ``linear_w4`` (``dnn_gemm_w4``) + ``argmax_rows`` for
orientation, at M in {1, 32, 64} on

  GPT-2 small  768 -> 50257     GPT-2 XL  1600 -> 50257     Llama-3 8B  4096 -> 128256

Where ``head_argmax`` does not cover a shape (it returns False: no K = 4096
config, a vocabulary over two column tiles per wave) the arm runs what the
stage runs there, ``linear_norm`` + ``argmax_rows``, and the line says so
(``*_route``).  Each arm is a HIP graph of at least ``--launches`` steps that
rotate over enough copies of the weight to pass the 256 MB MALL, so every step
streams its weight from HBM; a round replays the graphs in turn, device events
around each replay; the figure is the median over ``--rounds`` of time per step
with the min-max spread, and the weight bytes over it.  One JSON line per
(shape, M) goes to ``--out``/w4_head_ab.jsonl.

    python bench/probes/w4_head_ab.py [--rounds 9] [--launches 48] [--out profiles]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

SHAPES = [("gpt2 head", 768, 50257, False), ("gpt2-xl head", 1600, 50257, False),
          ("llama3-8b head", 4096, 128256, True)]
MS = (1, 32, 64)
ROTATE_BYTES = 512 << 20


def graph_of(fn, n):
    import torch
    fn(0)  # warm-up: code objects, lazy buffers
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
    return g


def time_graphs(graphs, rounds, per):
    """(median, min, max) ms per step of every graph, replayed in turn each round."""
    import torch
    ms = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if r:  # round 0 warms the graphs
                ms[k].append(a.elapsed_time(b) / per)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def child(a):
    import torch
    from distributed_neural_networks_amd.ops import w4
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight
    from distributed_neural_networks_amd.ops.gemm import (HEAD_PART_PER_ROW, FoldedLinear, attach_shuffled, fold_norm,
                                                          head_argmax, linear_norm)
    from distributed_neural_networks_amd.ops.transformer_ops import ARGMAX_PART_PER_ROW, argmax_rows
    name, K, N, rms = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    gamma = torch.rand(K, device=dev) + 0.5
    beta = None if rms else torch.randn(K, device=dev) * 0.1
    f4 = fold_norm(W, gamma, beta, None, rms, 1e-5, dev, quant="mxfp4")
    fb = attach_shuffled(fold_norm(W, gamma, beta, None, rms, 1e-5, dev))
    f8 = attach_shuffled(fold_norm(W, gamma, beta, None, rms, 1e-5, dev, True))
    del W
    by = {"w4_head": f4.w.q.numel() + f4.w.scales.numel(), "bf16": 2 * N * K, "e4m3": N * K}
    by["w4_gemm"] = by["w4_head"]
    # enough copies of the smallest (4-bit) weight to pass the MALL, and a graph that visits them all
    copies = max(2, min(512, -(-ROTATE_BYTES // by["w4_head"])))
    a.launches = max(a.launches, copies)
    f4s = [FoldedLinear(w4.Mxfp4Weight(f4.w.q.clone(), f4.w.scales.clone(), N, K), f4.bias, f4.colsum, f4.norm, f4.eps)
           for _ in range(copies)]
    fbs, f8s = [], []
    for _ in range(copies):
        c = FoldedLinear(fb.w, fb.bias, fb.colsum, fb.norm, fb.eps)
        c.ws = fb.ws.clone()
        fbs.append(c)
        f8s.append(FoldedLinear(Fp8Weight(f8.w.q, f8.w.scale, f8.w.k, shuf=f8.w.shuf.clone()), f8.bias, f8.colsum,
                                f8.norm, f8.eps))
    ldc = -(-N // 64) * 64
    lines = []
    for M in MS:
        x = (torch.randn(M, K, device=dev) + 0.3).bfloat16()
        logits = torch.empty(M, ldc, device=dev, dtype=torch.bfloat16)[:, :N]
        part = torch.empty(2 * max(HEAD_PART_PER_ROW, ARGMAX_PART_PER_ROW) * M, dtype=torch.int32, device=dev)
        ids = torch.empty(M, dtype=torch.int32, device=dev)
        route = {}

        def head_or_gemm(fs, key):
            route[key] = "head_argmax" if head_argmax(x, fs[0], logits, part, ids) else "linear_norm+argmax_rows"
            if route[key] == "head_argmax":
                return lambda i: head_argmax(x, fs[i % copies], logits, part, ids)
            return lambda i: (linear_norm(x, fs[i % copies], out=logits), argmax_rows(logits, ids, n=N, part=part))

        arms = {"w4_head": lambda i: w4.head_w4(x, f4s[i % copies], logits, part, ids),
                "bf16": head_or_gemm(fbs, "bf16"), "e4m3": head_or_gemm(f8s, "e4m3"),
                "w4_gemm": lambda i: (w4.linear_w4(x, f4s[i % copies].w, f4.bias, out=logits, norm=f4.norm,
                                                   colsum=f4.colsum, eps=f4.eps),
                                      argmax_rows(logits, ids, n=N, part=part))}
        # results must agree before a time means anything: the new arm against dnn_gemm_w4 on the same weight
        arms["w4_gemm"](0)
        ref, ref_ids = logits.float().clone(), ids.clone()
        arms["w4_head"](0)
        err = ((logits.float() - ref).norm() / ref.norm()).item()
        lf = logits.float()
        first = torch.where(lf == lf.max(1, keepdim=True).values, torch.arange(N, device=dev), N).min(1).values
        assert err < 1e-2 and torch.equal(ids, first.int()), (err, ids, ref_ids)
        t = time_graphs({k: graph_of(f, a.launches) for k, f in arms.items()}, a.rounds, a.launches)
        lines.append({"probe": "w4_head_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies,
                      "w4_head_vs_w4_gemm_rel": err, **{f"{k}_route": v for k, v in route.items()},
                      **{f"{k}_us": round(v[0] * 1e3, 3) for k, v in t.items()},
                      **{f"{k}_us_min_max": [round(v[1] * 1e3, 3), round(v[2] * 1e3, 3)] for k, v in t.items()},
                      **{f"{k}_TBps": round(by[k] / (t[k][0] * 1e-3) / 1e12, 3) for k in t}})
    for ln in lines:
        print("RESULT " + json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shape", type=int, default=-1, help="child: index into SHAPES")
    a = ap.parse_args()
    if a.shape >= 0:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "w4_head_ab.jsonl")
    with open(path, "w") as f:
        for i in range(len(SHAPES)):  # one fresh process per shape, one at a time
            r = subprocess.run([sys.executable, HERE, "--shape", str(i), "--rounds", str(a.rounds), "--launches",
                                str(a.launches)], capture_output=True, text=True, timeout=600)
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
