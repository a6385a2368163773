"""Decode projections with MXFP4, e4m3 and bf16 weights, alternating in one
process per shape: ``linear_w4`` (W4A16, csrc/kernels/gemm_w4.hip) against
``linear_w8`` (W8A16) and bf16 ``linear`` with fragment-order weights, at M in
{1, 32, 64} on the projection shapes K -> N of

  GPT-2 XL     1600 -> 4800 / 1600 / 6400, 6400 -> 1600   (1600: K pad inside a chunk)
  Llama-3 8B   4096 -> 6144 / 4096 / 28672, 14336 -> 4096

Each arm is a HIP graph of at least ``--launches`` launches that rotate over
enough copies of the weight to pass the 256 MB MALL (the graph visits every
copy), so every launch streams its weight from HBM; a round replays the three graphs in turn, device events around
each replay; the figure is the median over ``--rounds`` of time per launch.
Also: ``dnn_w4_expand`` of the shape's weight against a plain device copy that
moves the same bytes (read + write), in bytes/s.  One JSON line per (shape, M)
and per expansion goes to ``--out``/w4_decode_ab.jsonl.

    python bench/probes/w4_decode_ab.py [--rounds 9] [--launches 48] [--out profiles]
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

SHAPES = [("gpt2-xl qkv", 1600, 4800), ("gpt2-xl o", 1600, 1600), ("gpt2-xl fc", 1600, 6400),
          ("gpt2-xl proj", 6400, 1600), ("llama3-8b qkv", 4096, 6144), ("llama3-8b o", 4096, 4096),
          ("llama3-8b gate_up", 4096, 28672), ("llama3-8b down", 14336, 4096)]
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
    """Median ms per launch of every graph, replayed in turn each round."""
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
    return {k: statistics.median(v) for k, v in ms.items()}


def child(a):
    import torch
    from distributed_neural_networks_amd.ops.fp8 import Fp8Weight, linear_w8, quantize_weight
    from distributed_neural_networks_amd.ops.gemm import attach_shuffled, decode_workspace, linear
    from distributed_neural_networks_amd.ops import w4
    name, K, N = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    # enough copies of the smallest (4-bit) weight to pass the MALL, and a graph that visits them all
    copies = max(2, min(512, -(-ROTATE_BYTES // (N * K // 2))))
    a.launches = max(a.launches, copies)
    q4 = w4.quantize_weight_mxfp4(W, dev)
    w4s = [w4.Mxfp4Weight(q4.q.clone(), q4.scales.clone(), N, K) for _ in range(copies)]
    q8 = attach_shuffled(quantize_weight(W, dev))
    w8s = [Fp8Weight(q8.q, q8.scale, q8.k, shuf=q8.shuf.clone()) for _ in range(copies)]
    wb = W.bfloat16()
    wbs = [attach_shuffled(wb) for _ in range(copies)]
    ws = decode_workspace(dev, 0)
    lines = []
    for M in MS:
        x = torch.randn(M, K, device=dev).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        arms = {"w4": lambda i: w4.linear_w4(x, w4s[i % copies], out=out),
                "w8": lambda i: linear_w8(x, w8s[i % copies], out=out, ws=ws),
                "bf16": lambda i: linear(x, wb, out=out, w_shuf=wbs[i % copies], ws=ws)}
        # results must agree before a time means anything: each arm against fp32 on its own weight values
        ref4 = x.float() @ w4.dequantize(q4).t()
        err4 = ((arms["w4"](0).float() - ref4).norm() / ref4.norm()).item()
        assert err4 < 1e-2, err4
        t = time_graphs({k: graph_of(f, a.launches) for k, f in arms.items()}, a.rounds, a.launches)
        by = {"w4": q4.q.numel() + q4.scales.numel(), "w8": N * K, "bf16": 2 * N * K}
        lines.append({"probe": "w4_decode_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies,
                      "w4_rel_err": err4, **{f"{k}_us": round(v * 1e3, 3) for k, v in t.items()},
                      **{f"{k}_GBps": round(by[k] / (t[k] * 1e-3) / 1e9, 1) for k in t}})
    # expansion against a device copy moving the same bytes (read + write)
    scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
    moved = q4.q.numel() + q4.scales.numel() + 2 * N * K
    src = torch.empty(moved // 2, device=dev, dtype=torch.uint8)
    dst = torch.empty_like(src)
    t = time_graphs({"expand": graph_of(lambda i: w4.expand(w4s[i % copies], scratch), a.launches),
                     "copy": graph_of(lambda i: dst.copy_(src), a.launches)}, a.rounds, a.launches)
    lines.append({"probe": "w4_expand", "shape": name, "K": K, "N": N, "bytes_moved": moved,
                  **{f"{k}_us": round(v * 1e3, 3) for k, v in t.items()},
                  **{f"{k}_GBps": round(moved / (v * 1e-3) / 1e9, 1) for k, v in t.items()}})
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
    path = os.path.join(a.out, "w4_decode_ab.jsonl")
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
