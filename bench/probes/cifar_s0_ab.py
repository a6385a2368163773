"""Interleaved in-process A/B of a stage-0 kernel switch (box-to-box clock
differences cancel): stage-0 time at B=65536 on random images for each arm,
every round's time and the median, plus the max |difference| of the two
outputs (0 for wide_store; the MFMA shapes sum K in different orders, so
~1e-6 for mfma16).  One JSON line.

    python bench/probes/cifar_s0_ab.py [--switch wide_store|mfma16|conv1_k32] [--arms 0,1] [--batch 65536]

mfma16 arms: 0 = conv2 on 32x32x16, 1 = on 16x16x32.  conv1_k32 arms: 0 = conv1
on K = 48 (HWC4 input planes), 1 = on K = 32 (channel-packed planes, parity
weight sets); they sum K in different orders (~1e-6).  An arm wins only if every
one of its rounds is faster than every round of the other.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from distributed_neural_networks_amd.models.cifar import NeuralNetwork  # noqa: E402
from distributed_neural_networks_amd.ops import _lib, cifar as cops  # noqa: E402

# wide_store is a switch of the 32x32x16 conv2 path: it is compared with that path forced
SWITCHES = {"wide_store": lambda v: _lib.lib().cifar_s0_set_mfma(0) or _lib.lib().cifar_s0_set_wide_store(v),
            "mfma16": lambda v: _lib.lib().cifar_s0_set_mfma(v),
            "conv1_k32": lambda v: _lib.lib().cifar_s0_set_conv1(v)}
DEFAULTS = {"wide_store": lambda: 1, "mfma16": lambda: _lib.lib().cifar_s0_get_mfma(),
            "conv1_k32": lambda: _lib.lib().cifar_s0_get_conv1()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--switch", default="wide_store", choices=sorted(SWITCHES))
    ap.add_argument("--arms", default="0,1", help="the two switch values to compare")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    arms = tuple(int(v) for v in a.arms.split(","))
    assert len(arms) == 2 and arms[0] != arms[1]
    default, mfma_default = DEFAULTS[a.switch](), _lib.lib().cifar_s0_get_mfma()
    torch.manual_seed(0)
    sd = NeuralNetwork().state_dict()
    w0 = cops.pack_stage0(sd, "cuda")
    x = torch.randn(a.batch, 3, 32, 32, device="cuda")
    outs = {v: torch.empty(a.batch, 4096, device="cuda") for v in arms}
    times = {v: [] for v in arms}
    for _ in range(a.rounds):
        for v in arms:
            assert SWITCHES[a.switch](v) == 0
            cops.stage0_forward(x, w0, outs[v])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                cops.stage0_forward(x, w0, outs[v])
            e1.record()
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / a.iters)
    SWITCHES[a.switch](default)
    _lib.lib().cifar_s0_set_mfma(mfma_default)
    lo, hi = arms
    print(json.dumps({"switch": a.switch, "B": a.batch, "iters": a.iters,
                      **{f"{a.switch}{v}_ms": round(sorted(t)[len(t) // 2], 4) for v, t in times.items()},
                      **{f"{a.switch}{v}_rounds_ms": [round(t_, 4) for t_ in t] for v, t in times.items()},
                      f"every_round_of_{hi}_faster": max(times[hi]) < min(times[lo]),
                      f"every_round_of_{lo}_faster": max(times[lo]) < min(times[hi]),
                      "max_abs_diff": (outs[lo] - outs[hi]).abs().max().item()}), flush=True)


if __name__ == "__main__":
    main()
