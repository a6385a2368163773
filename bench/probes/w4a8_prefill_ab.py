"""MXFP4 prefill projections at 384 / 2048 / 32768 rows, three arms alternating
in one process per shape (the GPT-2 XL and Llama-3 8B shapes of w4_decode_ab.py):

  w4a8    ``linear_w4a8``: the MX quantise pass + ``dnn_gemm_w4a8`` on the codes
  expand  ``linear_w4(..., scratch=)``: ``dnn_w4_expand`` + the bf16 tile GEMM
          (the ``mxfp4_prefill: "bf16"`` route)
  fp8mx   for orientation only: ``linear_fp8(..., sx=)`` on an e4m3 weight of the
          same shape (quantise pass + ``gemm_fp8_mx``: the same MFMA count and A
          path, what the instruction allows with both operands through LDS)

Each arm is a HIP graph of launches rotating over weight copies past the 256 MB
MALL; a round replays the graphs in turn; the figures are the median, min and
max over ``--rounds`` of time per launch.  One JSON line per (shape, M) goes to
``--out``/w4a8_prefill_ab.jsonl.

    python bench/probes/w4a8_prefill_ab.py [--rounds 7] [--launches 8] [--out profiles]
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

from w4_decode_ab import ROTATE_BYTES, SHAPES, graph_of  # noqa: E402
from w4_mid_ab import time_graphs  # noqa: E402

MS = (384, 2048, 32768)


def child(a):
    import torch
    from distributed_neural_networks_amd.ops import fp8, w4
    name, K, N = SHAPES[a.shape]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    W = torch.randn(N, K, device=dev) * 0.02
    copies = max(2, min(64, -(-ROTATE_BYTES // (N * K // 2))))  # of the 4-bit weight, past the MALL
    c8 = max(2, min(64, -(-ROTATE_BYTES // (N * K))))            # of the e4m3 weight
    q4 = w4.quantize_weight_mxfp4(W, dev)
    w4s = [w4.Mxfp4Weight(q4.q.clone(), q4.scales.clone(), N, K) for _ in range(copies)]
    q8w = fp8.quantize_weight(W, dev)
    w8s = [fp8.Fp8Weight(q8w.q.clone(), q8w.scale.clone(), K) for _ in range(c8)]
    scratch = torch.empty(N * K, device=dev, dtype=torch.bfloat16)
    dq = w4.dequantize(q4)
    kp = q4.kpad
    for M in MS:
        n = max(a.launches if M < 32768 else 2, 2)
        x = torch.randn(M, K, device=dev).bfloat16()
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        q8 = torch.empty(M * kp, dtype=torch.uint8, device=dev)
        sx = torch.empty(fp8.mx_scale_bytes(M, kp), dtype=torch.uint8, device=dev)
        arms = {"w4a8": lambda i: w4.linear_w4a8(x, w4s[i % copies], out=out, q8=q8, sx=sx),
                "expand": lambda i: w4.linear_w4(x, w4s[i % copies], out=out, scratch=scratch),
                "fp8mx": lambda i: fp8.linear_fp8(x, w8s[i % c8], out=out, qbuf=q8, sx=sx)}
        ref = x[:256].float() @ dq.t()
        err = ((arms["w4a8"](0)[:256].float() - ref).norm() / ref.norm()).item()
        assert err < 8e-2, err  # a time means something only for a right result (e4m3 activations: a few %)
        t = time_graphs({k: graph_of(f, n) for k, f in arms.items()}, a.rounds, n)
        ln = {"probe": "w4a8_prefill_ab", "shape": name, "K": K, "N": N, "M": M, "copies": copies,
              "w4a8_rel_err": round(err, 4)}
        for k, (med, lo, hi) in t.items():
            ln.update({f"{k}_us": round(med, 2), f"{k}_min_us": round(lo, 2), f"{k}_max_us": round(hi, 2)})
        print("RESULT " + json.dumps(ln), flush=True)
        del x, out, q8, sx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--shape", type=int, default=-1, help="child: index into SHAPES")
    a = ap.parse_args()
    if a.shape >= 0:
        return child(a)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "w4a8_prefill_ab.jsonl")
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
