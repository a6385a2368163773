"""MXFP4 decode projections at 96..256 rows, three arms alternating in one
process per shape (the shapes of w4_decode_ab.py):

  mid     ``linear_w4`` without a scratch: ``dnn_gemm_w4_mid`` on the codes
  expand  ``linear_w4(..., scratch=)``: ``dnn_w4_expand`` + the bf16 tile GEMM
          (what a decode step of these sizes ran before the mid kernel)
  bf16    ``linear`` on a resident row-major bf16 weight (what a bf16 stage pays)

and, for information, M in {32, 64}: the mid kernel (``lib().gemm_w4_mid``)
against ``dnn_gemm_w4``.  Each arm is a HIP graph of launches rotating over
weight copies past the 256 MB MALL; a round replays the graphs in turn; the
figures are the median, min and max over ``--rounds`` of time per launch.  One
JSON line per (shape, M) goes to ``--out``/w4_mid_ab.jsonl.

    python bench/probes/w4_mid_ab.py [--rounds 9] [--launches 16] [--out profiles]
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
sys.path.insert(0, os.path.dirname(HERE))

from w4_decode_ab import ROTATE_BYTES, SHAPES, graph_of  # noqa: E402

MS = (96, 128, 256)
MS_INFO = (32, 64)


def time_graphs(graphs, rounds, per):
    """(median, min, max) us per launch of every graph, replayed in turn each round."""
    import torch
    us = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            if r:  # round 0 warms the graphs
                us[k].append(a.elapsed_time(b) / per * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def child(a):
    import torch
    from distributed_neural_networks_amd.ops import w4
    from distributed_neural_networks_amd.ops._lib import check, lib, ptr, stream_ptr
    from distributed_neural_networks_amd.ops.gemm import linear
    name, K, N = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    copies = max(2, min(512, -(-ROTATE_BYTES // (N * K // 2))))  # of the 4-bit weight, past the MALL
    cb = max(2, -(-ROTATE_BYTES // (2 * N * K)))                 # of the bf16 weight
    n = max(a.launches, copies)
    q4 = w4.quantize_weight_mxfp4(W, dev)
    w4s = [w4.Mxfp4Weight(q4.q.clone(), q4.scales.clone(), N, K) for _ in range(copies)]
    wbs = [W.bfloat16() for _ in range(cb)]
    scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
    dq = w4.dequantize(q4)

    def mid(x, out, i):
        w = w4s[i % copies]
        check(lib().gemm_w4_mid(ptr(x), x.stride(0), ptr(w.q), ptr(w.scales), ptr(out), out.stride(0), 0, 0, 0,
                                x.shape[0], N, K, 0, 0, 0, 0.0, stream_ptr()), "gemm_w4_mid")
        return out

    for M in MS_INFO + MS:
        x = torch.randn(M, K, device=dev).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        if M <= 64:
            arms = {"mid": lambda i: mid(x, out, i), "w4": lambda i: w4.linear_w4(x, w4s[i % copies], out=out)}
        else:
            arms = {"mid": lambda i: w4.linear_w4(x, w4s[i % copies], out=out),
                    "expand": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, scratch=scratch),
                    "bf16": lambda i: linear(x, wbs[i % cb], out=out)}
        ref = x.float() @ dq.t()
        err = ((arms["mid"](0).float() - ref).norm() / ref.norm()).item()
        assert err < 1e-2, err  # a time means something only for a right result
        t = time_graphs({k: graph_of(f, n) for k, f in arms.items()}, a.rounds, n)
        ln = {"probe": "w4_mid_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies, "mid_rel_err": err}
        for k, (med, lo, hi) in t.items():
            ln.update({f"{k}_us": round(med, 2), f"{k}_min_us": round(lo, 2), f"{k}_max_us": round(hi, 2)})
        print("RESULT " + json.dumps(ln), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shape", type=int, default=-1, help="child: index into SHAPES")
    a = ap.parse_args()
    if a.shape >= 0:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "w4_mid_ab.jsonl")
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
