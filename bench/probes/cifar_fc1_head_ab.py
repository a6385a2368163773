"""A/B of the fused fp32 head (``ops.cifar.set_head_fusion``) in one process: units 2-3 at
B rows, the switch on and off in alternating rounds, device events around ``--iters`` calls each.
One JSON line per arm and round, then a summary line.

    python bench/probes/cifar_fc1_head_ab.py --batch 65536 --rounds 5 --iters 50
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from distributed_neural_networks_amd.models.cifar import NeuralNetwork  # noqa: E402
from distributed_neural_networks_amd.ops import cifar as cops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    w = cops.pack_head(NeuralNetwork().state_dict(), dev)
    B = a.batch
    h = torch.relu(torch.randn(B, 4096, device=dev))
    bufs = {"hid": torch.empty(B, 512, device=dev), "part": torch.empty(2, B, 16, device=dev),
            "probs": torch.empty(B, 10, device=dev), "pred": torch.empty(B, dtype=torch.int32, device=dev)}

    def call():
        return cops.head_forward(h, w, hid=bufs["hid"], probs=bufs["probs"], pred=bufs["pred"], part=bufs["part"])

    prev = cops.set_head_fusion(True)
    ms = {True: [], False: []}
    pred = {}
    try:
        for r in range(a.rounds):
            for on in (False, True):
                cops.set_head_fusion(on)
                for _ in range(5):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call()
                e1.record()
                torch.cuda.synchronize()
                t = e0.elapsed_time(e1) / a.iters
                ms[on].append(t)
                pred[on] = bufs["pred"].clone()
                print(json.dumps({"round": r, "fused": on, "batch": B, "ms_per_call": round(t, 5)}), flush=True)
    finally:
        cops.set_head_fusion(prev)
    print(json.dumps({"summary": True, "batch": B, "unfused_ms": [round(x, 5) for x in ms[False]],
                      "fused_ms": [round(x, 5) for x in ms[True]],
                      "fused_faster_every_round": all(f < u for f, u in zip(ms[True], ms[False])),
                      "pred_rows_differing": int((pred[True] != pred[False]).sum())}))


if __name__ == "__main__":
    main()
