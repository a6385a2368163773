"""A/B probe of the prompt log-probability launch (csrc/kernels/head_lse.hip,
``ops.gemm.head_lse``) against the unfused route: ``linear_norm`` to
all-position logits, in row chunks so that the logits buffer fits, then
``logprobs_rows`` (n = 1) per chunk.

One process, the two arms in turn, medians of ``--rounds`` rounds (each the
mean of ``--iters`` calls between two events) with the min-max spread, and the
peak extra device memory of each arm.  One JSON line per (shape, rows).

  python bench/probes/prompt_logprobs_ab.py --out profiles/prompt_logprobs_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = [(768, 50257, False), (4096, 128256, True)]  # (d, V, RMSNorm): GPT-2, Llama-3
ROWS = [2048, 8192, 32768]
CHUNK = 8192  # rows of logits the unfused arm materialises at a time


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from distributed_neural_networks_amd.ops import transformer_ops as T
    from distributed_neural_networks_amd.ops.gemm import fold_norm, head_lse, head_lse_workspace, linear_norm
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for d, V, rms in SHAPES:
        w = torch.randn(V, d, device=dev, generator=g) / d ** 0.5
        gamma = 1 + 0.1 * torch.randn(d, device=dev, generator=g)
        f = fold_norm(w, gamma, None if rms else 0.1 * torch.randn(d, device=dev, generator=g), None, rms, 1e-5, dev)
        del w
        for M in ROWS:
            x = torch.randn(M, d, device=dev, generator=g).bfloat16()
            tgt = torch.randint(0, V, (M,), device=dev, generator=g).to(torch.int32)
            oidx = torch.arange(M, device=dev, dtype=torch.int32)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            ws, stats = head_lse_workspace(M, V, dev), torch.empty(2 * M, dtype=torch.float32, device=dev)
            outs = (torch.zeros(M, device=dev), torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, device=dev))
            fused = lambda: head_lse(x, f, tgt, oidx, *outs, ws, stats=stats)  # noqa: E731
            fused()
            torch.cuda.synchronize()
            mem_f = torch.cuda.max_memory_allocated(dev) - base
            torch.cuda.reset_peak_memory_stats(dev)
            C = min(CHUNK, M)
            ld = (V + 7) // 8 * 8
            logits = torch.empty((C, ld), dtype=torch.bfloat16, device=dev)
            std, ones = torch.empty((C, d), dtype=torch.bfloat16, device=dev), torch.ones(d, device=dev)
            lws = T.logprobs_workspace(C, V, 1, dev)
            ch = torch.zeros((C, 1), device=dev)
            ti, tl = torch.zeros((C, 1, 1), dtype=torch.int32, device=dev), torch.zeros((C, 1, 1), device=dev)

            def unfused():
                for r0 in range(0, M, C):
                    linear_norm(x[r0:r0 + C], f, out=logits[:, :V], std_buf=std, ones=ones)
                    T.logprobs_rows(logits, tgt[r0:r0 + C], V, 1, ch, ti, tl, lws)
            unfused()
            torch.cuda.synchronize()
            mem_u = torch.cuda.max_memory_allocated(dev) - base - mem_f
            tf, tu = [], []
            for _ in range(a.rounds):
                tf.append(_time(fused, a.iters))
                tu.append(_time(unfused, a.iters))
            rec = {"d": d, "V": V, "rows": M, "fused_us": round(statistics.median(tf), 1),
                   "fused_minmax_us": [round(min(tf), 1), round(max(tf), 1)],
                   "unfused_us": round(statistics.median(tu), 1),
                   "unfused_minmax_us": [round(min(tu), 1), round(max(tu), 1)], "unfused_chunk_rows": C,
                   "fused_extra_bytes": int(mem_f), "unfused_extra_bytes": int(mem_u)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x, logits, std, lws, ws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
