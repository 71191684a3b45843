"""Kernel times of the gradient norm, the in-place clip and the capturable Adam (csrc/adam.hip) over
the learning conf's parameter set (886 tensors, 145 M values), against torch on the same tensors.

    python tools/grad_clip_bench.py [--reps 20] [--out profiles/grad_clip_kernels.jsonl]

Times are device events around ``reps`` back-to-back calls after a warm-up; bytes are what the
algorithm needs (4 B per value for the sum of squares, 8 for the clip, 28 for Adam), the peak 8.0 TB/s.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gasfm_amd  # noqa: E402
from gasfm_amd import optim  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ts.sort()
    return {"ms_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.learning_conf()).to(dev)
    ps = list(net.parameters())
    for p in ps:
        p.grad = torch.randn_like(p) * 1e-3
    n = sum(p.numel() for p in ps)
    rows = []

    def row(name, bytes_per_value, t):
        r = {"what": name, "values": n, "tensors": len(ps), **t}
        if bytes_per_value:
            r["bytes_per_value"] = bytes_per_value
            r["TB_per_s"] = bytes_per_value * n / (t["ms_median"] * 1e-3) / 1e12
            r["share_of_8TBps_peak"] = bytes_per_value * n / (t["ms_median"] * 1e-3) / PEAK
        rows.append(r)
        print(json.dumps(r), flush=True)

    row("grad_norm (sum of squares + ordered finish)", 4, timed(lambda: optim.grad_norm(ps), args.reps))
    row("clip_grad_norm_ (norm + in-place scale, coefficient 1)", 12,
        timed(lambda: optim.clip_grad_norm_(ps, 1e9), args.reps))
    row("torch.nn.utils.clip_grad_norm_", None,
        timed(lambda: torch.nn.utils.clip_grad_norm_(ps, 1e9), args.reps))
    row("torch cat-and-norm (train.py:139)", None,
        timed(lambda: torch.cat([p.grad.flatten() for p in ps]).norm(), max(2, args.reps // 4)))
    host = optim.Adam(ps, lr=1e-4)
    row("Adam, host-launched (gasfm_adam_step)", 28, timed(host.step, args.reps))
    plain = optim.Adam(ps, lr=1e-4, capturable=True)
    row("Adam, device path (control + gasfm_adam_step_ctl)", 28, timed(plain.step, args.reps))
    full = optim.Adam(ps, lr=1e-4, capturable=True, grad_clip_mode="norm", grad_clip_th=1.0, track_grad_norm=True)
    loss = torch.tensor(1.0, device=dev)
    row("Adam, device path + norm + clip + loss guard", 32, timed(lambda: full.step(loss=loss), args.reps))
    loss.zero_()
    row("the same, step skipped by the guard (reads the gradients only)", 4,
        timed(lambda: full.step(loss=loss), args.reps))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
