"""A/Bs of the fp32 fc1 at large batch.  Prints one JSON line.

    python bench/probes/cifar_fc1_ab.py [B]                       # paths
    python bench/probes/cifar_fc1_ab.py --switch sched [--batch B] [--rounds 10] [--iters 20] [--split_in 0]

Without ``--switch``: split3 + K-concat bf16 GEMM vs the fused cifar_fc1_x3
kernel (same math, same weights).

``--switch sched``: every k-loop arm of the fused kernel (``FC1_SCHED``: 1
staggered, 2 lean), interleaved rounds in one process (box-to-box
clock differences cancel), each round one replay of a HIP graph of ``iters``
launches.  Every round is printed, with median and range per arm; an arm beats
another only if every one of its rounds is faster than every round of the
other.  All outputs must be bitwise equal.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def paths(B):
    from distributed_neural_networks_amd.ops import cifar as cops
    from distributed_neural_networks_amd.ops.gemm import ACT_RELU, linear
    from distributed_neural_networks_amd.ops._lib import check, lib, ptr, stream_ptr
    from distributed_neural_networks_amd import checkpoint as ckpt
    dev = torch.device("cuda", 0)
    sd = ckpt.random_stage_state_dict("cifar10", 2, 3, False, True, 0)
    w = cops.pack_head(sd, dev)
    h = torch.randn(B, 4096, device=dev).relu_()
    out_a = torch.empty(B, 512, device=dev)
    out_b = torch.empty(B, 512, device=dev)
    scratch = torch.empty(B, 3 * 4096, dtype=torch.bfloat16, device=dev)

    def a():
        check(lib().cifar_split3(ptr(h), 4096, ptr(scratch), 3 * 4096, B, 4096, stream_ptr()), "split3")
        linear(scratch, w.w_fc1, w.b_fc1, act=ACT_RELU, out=out_a)

    def b():
        check(lib().cifar_fc1_x3(ptr(h), 4096, ptr(w.w_fc1h), ptr(w.w_fc1l), 4096, ptr(w.b_fc1), ptr(out_b), 512,
                                 B, 512, 4096, stream_ptr()), "fc1_x3")

    res = {"B": B}
    outs = {}
    for name, fn in (("split3_concat_gemm", a), ("fused_fc1_x3", b)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        res[name + "_ms"] = round(ms, 4)
        res[name + "_pflops"] = round(3 * 2 * B * 512 * 4096 / ms / 1e12, 3)
        outs[name] = (out_a if fn is a else out_b).clone()
    res["max_abs_diff"] = (outs["split3_concat_gemm"] - outs["fused_fc1_x3"]).abs().max().item()
    print(json.dumps(res), flush=True)


def sched(a):
    from distributed_neural_networks_amd.ops import cifar as cops
    from distributed_neural_networks_amd import checkpoint as ckpt
    dev = torch.device("cuda", 0)
    B = a.batch
    sd = ckpt.random_stage_state_dict("cifar10", 2, 3, False, True, 0)
    w = cops.pack_head(sd, dev)
    torch.manual_seed(0)
    h = torch.randn(B, 4096, device=dev).relu_()
    boundary = "split" if a.split_in else "fp32"
    if a.split_in:
        h = cops.encode_boundary(h)
    names = {v: k for k, v in cops.FC1_SCHED.items()}
    arms = tuple(sorted(names))
    outs = {v: torch.empty(B, 512, device=dev) for v in arms}
    default = cops.set_fc1_sched(arms[0])
    graphs = {}
    side = torch.cuda.Stream()
    for v in arms:  # the schedule is read at launch, so each arm is captured under its own setting
        cops.set_fc1_sched(v)
        cops.fc1_forward(h, w, outs[v], boundary=boundary)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(a.iters):
                cops.fc1_forward(h, w, outs[v], boundary=boundary)
        graphs[v] = g
    cops.set_fc1_sched(default)
    for v in arms:
        graphs[v].replay()  # warm-up replay of each graph
    torch.cuda.synchronize()
    times = {v: [] for v in arms}
    for r in range(a.rounds):
        for v in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[v].replay()
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / a.iters)
            print(f"round {r} {names[v]}: {times[v][-1]:.4f} ms", flush=True)
    equal = all(torch.equal(outs[arms[0]].view(torch.int32), outs[v].view(torch.int32)) for v in arms[1:])
    print(json.dumps({"switch": "sched", "B": B, "iters": a.iters, "split_in": a.split_in,
                      "default": names[default],
                      **{f"{names[v]}_ms": round(sorted(t)[len(t) // 2], 4) for v, t in times.items()},
                      **{f"{names[v]}_range_ms": [round(min(t), 4), round(max(t), 4)] for v, t in times.items()},
                      **{f"{names[v]}_rounds_ms": [round(t_, 4) for t_ in t] for v, t in times.items()},
                      **{f"every_round_of_{names[x]}_faster_than_{names[y]}": max(times[x]) < min(times[y])
                         for x in arms for y in arms if x != y},
                      "outputs_bitwise_equal": equal}), flush=True)
    assert equal, "the arms' outputs differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("B", nargs="?", type=int, default=None, help="batch of the path A/B (no --switch)")
    ap.add_argument("--switch", default=None, choices=["sched"])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--split_in", type=int, default=0, choices=[0, 1])
    a = ap.parse_args()
    if a.switch == "sched":
        sched(a)
    else:
        paths(a.B if a.B is not None else a.batch)


if __name__ == "__main__":
    main()
