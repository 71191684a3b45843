"""Time the depth-head evaluation's per-edge operations at config 4.

usage: python tools/depth_eval_bench.py [--m M] [--n N] [--reps R] [--trials T] [--out profiles/depth_eval.jsonl]
Defaults: config 4 (m = 1000, n = 200,000, E = 4,001,638 edges; gasfm_amd.synthetic.config4).  Each
operation runs as the HIP kernels (gasfm_amd.depth_eval, csrc/depth_eval.hip) and as its restatement
in torch ops on the device (float32 per edge, the same tensors), interleaved: a warm-up block of
each, then --trials rounds of one timed block of --reps calls each (between device events on the
launch stream); a line reports the median block with the minimum and maximum.  The last pair is the
whole compute_core_errors sequence: scales -> keys -> pairing -> 2-view error -> colsum.  One JSON
line per variant, printed and written to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gasfm_amd import depth_eval, synthetic  # noqa: E402
from gasfm_amd.depth_eval import _binding  # noqa: E402
from gasfm_amd import _native  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=None)
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5, help="timed blocks per variant")
    ap.add_argument("--out", default=os.path.join("profiles", "depth_eval.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sc = synthetic.config4() if args.m is None else synthetic.config4(args.m, args.n)
    m, n, E = sc.m, sc.n, sc.cam.shape[0]
    rng = np.random.default_rng(0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    cam, pt = t(sc.cam, torch.int32), t(sc.pt, torch.int32)
    order = np.argsort(sc.pt, kind="stable")
    perm = t(order, torch.int32)
    ptr = t(np.concatenate([[0], np.cumsum(np.bincount(sc.pt, minlength=n))]), torch.int32)
    # geometry only has to be finite: cameras near the identity in front of the points
    K = np.repeat(synthetic.K_DEFAULT[None], m, 0)
    Rt = np.zeros((m, 3, 4))
    Rt[:, :, :3] = np.eye(3) + 0.01 * rng.standard_normal((m, 3, 3))
    Rt[:, :, 3] = 0.1 * rng.standard_normal((m, 3)) + np.array([0, 0, 4.0])
    tab = depth_eval.camera_table(t(K, torch.float64), t(K @ Rt, torch.float64))
    xy = t(rng.uniform(0, 1000, size=(E, 2)), torch.float32)
    dg = t(rng.uniform(2, 6, size=E), torch.float32)
    dp = (dg * 3.7 * (1 + 0.05 * torch.randn(E, device=dev))).contiguous()
    torch.manual_seed(0)
    key = depth_eval.draw_keys(E, dev)
    src, bad = depth_eval.track_cycle(ptr, perm, key)
    assert torch.equal(src, depth_eval.track_cycle_torch(ptr, perm, key)[0])
    scales, _ = depth_eval.depth_norm_stats(dp, dg, stats=False)
    scale = scales[1] / scales[0]

    def core(track, stats, view):
        def run():
            s, _ = stats(dp, dg, False)
            p, _ = track(ptr, perm, depth_eval.draw_keys(E, dev))
            return view(cam, None, xy, dp, s[1] / s[0], p, tab)
        return run

    kernel_view = lambda *a: _native.colsum(_binding.backproj_2view(*a))  # noqa: E731
    torch_view = lambda *a: depth_eval.backproj_2view_torch(*a)[2]  # noqa: E731
    pairs = {
        "track_cycle": (lambda: _binding.track_cycle(ptr, perm, key),
                        lambda: depth_eval.track_cycle_torch(ptr, perm, key)),
        "backproj_2view (sum, count)": (lambda: kernel_view(cam, None, xy, dp, scale, src, tab),
                                        lambda: torch_view(cam, None, xy, dp, scale, src, tab)),
        "depth_norm_stats": (lambda: _binding.depth_norm_stats(dp, dg), lambda: depth_eval.depth_norm_stats_torch(dp, dg)),
        "core errors: scales, keys, pairing, 2-view, colsum": (
            core(_binding.track_cycle, _binding.depth_norm_stats, kernel_view),
            core(depth_eval.track_cycle_torch, depth_eval.depth_norm_stats_torch, torch_view)),
    }
    lines = []
    for op, (hip, ref) in pairs.items():
        times = interleaved({"HIP kernels": hip, "torch ops": ref}, args.reps, args.trials)
        for variant, v in times.items():
            lines.append({"op": op, "variant": variant, "m": m, "n": n, "E": E, **spread(v)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
