"""Interleaved in-process A/B of the CIFAR stage-0 input kind (box-to-box clock differences
cancel): the 2-stage colocated graph at B = 65536 as bench.py runs it, arm ``fp32`` on
(B,3,32,32) fp32 images and arm ``uint8`` on (B,32,32,3) bytes normalised by table in the kernel.
Both arms see the same images: the fp32 arm gets ``normalize_u8`` of the uint8 arm's bytes.
Alternating rounds; per round the graph's step time and the stage-0 kernel's own time.  The two
arms' probabilities and predictions are asserted bitwise equal.  One JSON line.

    python bench/probes/cifar_u8_ab.py [--batch 65536] [--rounds 5] [--iters 20]

An arm is slower only if every one of its rounds is slower than every round of the other.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from distributed_neural_networks_amd import checkpoint as ckpt  # noqa: E402
from distributed_neural_networks_amd.ops import cifar as cops  # noqa: E402
from distributed_neural_networks_amd.runtime.pipeline import ColocatedPipeline  # noqa: E402
from distributed_neural_networks_amd.runtime.stages import CifarHipStage  # noqa: E402

ARMS = ("fp32", "uint8")


def _timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd0 = ckpt.random_stage_state_dict("cifar10", 0, 1, True, False, 0)  # bench.py's weights
    sd1 = ckpt.random_stage_state_dict("cifar10", 2, 3, False, True, 0)
    table = cops.make_input_table()
    x8 = torch.randint(0, 256, (a.batch, 32, 32, 3), dtype=torch.uint8, device=dev,
                       generator=torch.Generator(device=dev).manual_seed(0))
    xs = {"uint8": x8, "fp32": cops.normalize_u8(x8, table)}
    pipes, s0 = {}, {}
    for arm in ARMS:
        s0[arm] = CifarHipStage(sd0, 0, 1, dev, input_dtype=arm, input_table=table)
        pipes[arm] = ColocatedPipeline([s0[arm], CifarHipStage(sd1, 2, 3, dev)], a.batch)
        pipes[arm].x.copy_(xs[arm])
        pipes[arm].capture()
    step, kern = {arm: [] for arm in ARMS}, {arm: [] for arm in ARMS}
    for _ in range(a.rounds):
        for arm in ARMS:
            step[arm].append(_timed(pipes[arm], a.iters))
            p = pipes[arm]
            kern[arm].append(_timed(lambda: cops.stage0_forward(p.x, s0[arm].w0, p.bufs[0],
                                                                table=s0[arm].input_table), a.iters))
    res = {arm: pipes[arm]() for arm in ARMS}
    torch.cuda.synchronize()
    same = (torch.equal(res["fp32"].probs.view(torch.int32), res["uint8"].probs.view(torch.int32))
            and torch.equal(res["fp32"].pred, res["uint8"].pred))
    assert same, "the uint8 arm's probabilities differ from the fp32 arm's on the same images"
    med = lambda t: round(sorted(t)[len(t) // 2], 4)  # noqa: E731
    r4 = lambda t: [round(v, 4) for v in t]  # noqa: E731
    print(json.dumps({"probe": "cifar_u8_ab", "B": a.batch, "iters": a.iters, "rounds": a.rounds,
                      **{f"{arm}_step_ms": med(step[arm]) for arm in ARMS},
                      **{f"{arm}_step_rounds_ms": r4(step[arm]) for arm in ARMS},
                      **{f"{arm}_stage0_ms": med(kern[arm]) for arm in ARMS},
                      **{f"{arm}_stage0_rounds_ms": r4(kern[arm]) for arm in ARMS},
                      "input_bytes_per_image": {"fp32": 12288, "uint8": 3072},
                      "every_uint8_step_round_slower": min(step["uint8"]) > max(step["fp32"]),
                      "every_uint8_step_round_faster": max(step["uint8"]) < min(step["fp32"]),
                      "every_uint8_stage0_round_slower": min(kern["uint8"]) > max(kern["fp32"]),
                      "every_uint8_stage0_round_faster": max(kern["uint8"]) < min(kern["fp32"]),
                      "probabilities_bitwise_equal": same}), flush=True)


if __name__ == "__main__":
    main()
