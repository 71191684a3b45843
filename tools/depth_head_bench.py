"""Time the depth head (Linear(128,128) ReLU Linear(128,128) ReLU Linear(128,1) per edge) at config 4.

usage: python tools/depth_head_bench.py [E] [--reps R] [--trials T] [--out profiles/depth_head.jsonl]
E defaults to config 4's 4,001,638 edges.  Two variants, forward + backward through autograd on the
same inputs: the fused HIP head (gasfm_amd.depth_head, csrc/depth_head.hip) and the aten Sequential
as the model ran it before.  They run interleaved: a warm-up block of each, then --trials rounds of
one timed block of --reps calls each (between device events on the launch stream); a line reports
the median block with the minimum and maximum, the algorithmic FLOPs and the fraction of the
157.3 TFLOPS fp32-MFMA peak they stand for, and torch.cuda.max_memory_allocated over one forward +
backward beyond what was resident before it (P, dd, the weights).  The fused forward and backward
are also timed apart.  One JSON line per variant, printed and written to --out.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gasfm_amd import depth_head  # noqa: E402
from gasfm_amd.model import get_linear_layers  # noqa: E402

PEAK_TFLOPS = 157.3   # fp32 MFMA, MI355X
W = 128
PRODUCT = 2 * W * W   # FLOPs of one 128 x 128 product per edge
# algorithmic FLOPs per edge: forward 2 products + the 128-wide dot; backward 2 input-gradient and 2
# weight-gradient products + the dot's two (the fused backward also recomputes the forward twice: 10
# products run, 6 + 2 counted as work done)
FLOP_FWD = 2 * PRODUCT + 2 * W
FLOP_BWD = 4 * PRODUCT + 4 * W
FLOP_RUN_FUSED = 10 * PRODUCT + 6 * W


def _block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def interleaved(fns, reps, trials):
    """{name: sorted us per call of `trials` timed blocks}, the variants taking turns block by block."""
    for fn in fns.values():
        _block(fn, reps)
    t = {k: [] for k in fns}
    for _ in range(trials):
        for k, fn in fns.items():
            t[k].append(_block(fn, reps))
    return {k: sorted(v) for k, v in t.items()}


def spread(t):
    return {"us": round(t[len(t) // 2], 1), "us_min": round(t[0], 1), "us_max": round(t[-1], 1)}


def peak_new_bytes(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("E", type=int, nargs="?", default=4_001_638)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5, help="timed blocks per variant")
    ap.add_argument("--out", default=os.path.join("profiles", "depth_head.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    E = args.E
    torch.manual_seed(0)
    seq = get_linear_layers(3 * [W] + [1], norm=False).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randn(E, W, device=dev, generator=g).requires_grad_(True)
    dd = torch.randn(E, 1, device=dev, generator=g)
    assert depth_head.fusable(seq, P)

    def step(fn):
        def run():
            P.grad = None
            for prm in seq.parameters():
                prm.grad = None
            fn(seq, P).backward(dd)
        return run

    variants = {"fused HIP head fwd+bwd": step(depth_head.apply), "aten Sequential fwd+bwd": step(lambda s, x: s(x))}
    times = interleaved(variants, args.reps, args.trials)
    mem = {}
    for k, fn in variants.items():
        P.grad = None
        for prm in seq.parameters():
            prm.grad = None
        mem[k] = peak_new_bytes(fn)
    P.grad = None

    def fwd_only():
        with torch.no_grad():
            depth_head.apply(seq, P)

    y = depth_head.apply(seq, P)
    parts = interleaved({"fused HIP head fwd": fwd_only,
                         "fused HIP head bwd": lambda: torch.autograd.grad(y, P, dd, retain_graph=True)},
                        args.reps, args.trials)
    # the backward line includes the two colsum launches over the partial rows; its parameter
    # gradients are not requested, dP is
    lines = []
    for k, t in times.items():
        s = spread(t)
        flop = (FLOP_FWD + FLOP_BWD) * E
        r = {"op": k, "E": E, **s, "algorithmic_GFLOP": round(flop / 1e9, 1),
             "frac_fp32_mfma_peak": round(flop / (s["us"] * 1e-6) / (PEAK_TFLOPS * 1e12), 3),
             "peak_new_bytes": mem[k], "peak_new_over_P": round(mem[k] / (E * W * 4), 3)}
        if k.startswith("fused"):
            r["frac_peak_incl_recompute"] = round(FLOP_RUN_FUSED * E / (s["us"] * 1e-6) / (PEAK_TFLOPS * 1e12), 3)
        lines.append(r)
    for k, t in parts.items():
        s = spread(t)
        flop = (FLOP_FWD if k.endswith("fwd") else FLOP_RUN_FUSED - FLOP_FWD) * E
        lines.append({"op": k, "E": E, **s, "run_GFLOP": round(flop / 1e9, 1),
                      "frac_fp32_mfma_peak": round(flop / (s["us"] * 1e-6) / (PEAK_TFLOPS * 1e12), 3)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
