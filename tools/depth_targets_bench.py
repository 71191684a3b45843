"""Cost of the per-edge depth targets (csrc/depth_targets.hip, scene_device.py) beside the same scene
builds without them and beside a torch-op restatement of the reference's dense [m, n] approach.

usage: python tools/depth_targets_bench.py [--reps 20] [--out profiles/depth_targets.jsonl] [--skip-config4]

  config 3   a 100-view, 20k-point scene resident on the device; per sample: 20 consecutive views
             (SceneData.sample_data), rotational homography augmentation 15 / 20, one graph build
             (sample_data_device(build=False) + apply_rotational_homography_aug_device)
  config 4   the full-scene build of m = 1000, n = 200k (scene_from_dense_device), triangulation
             included when the targets are on

The scenes are geometrically consistent (cameras on a circle looking at points in [-1, 1]^3, the
windowed visibility of gasfm_amd.synthetic, pixels by projection), so every depth is positive.
Each figure is the wall time of a call that ends in a device synchronise (the builds read sizes
back to the host, so device events alone would miss the host's share): median, min and max over
--reps runs after 3 warm-up runs, the variants interleaved.  The dense restatement keeps
depths [m, n] on the device: (Ns y X)[:, 2, :] for a full scene, row / column selection for a
sample, and the dense divide / multiply of SceneData.py:434 for the augmentation, then reads the
edges (it runs on the scene without targets and finds the kept columns with one more mask pass
of its own); no other device path for the targets exists to compare with.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gasfm_amd import scene_device as sd, synthetic  # noqa: E402


def consistent_scene(m, n, seed, dev):
    """(M [2m, n], Ns, Ps_gt) on the device: windowed visibility, pixels = projections of real points."""
    sc = synthetic.windowed_scene(m, n, seed=seed)
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, m, endpoint=False)
    ts = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.3 * rng.standard_normal(m)], 1)
    Rs = np.stack([synthetic.rotation_look_at(c) for c in ts])
    K = synthetic.K_DEFAULT
    Ps = np.einsum("ij,cjk->cik", K, np.concatenate([Rs.transpose(0, 2, 1),
                                                     -np.einsum("cji,cj->ci", Rs, ts)[:, :, None]], 2))
    X = np.concatenate([rng.uniform(-1, 1, size=(n, 3)), np.ones((n, 1))], 1)
    q = np.einsum("eij,ej->ei", Ps[sc.cam], X[sc.pt])
    xy = torch.from_numpy((q[:, :2] / q[:, 2:3]).astype(np.float32)).to(dev)
    cam, pt = torch.from_numpy(sc.cam).to(dev), torch.from_numpy(sc.pt).to(dev)
    M = torch.zeros((2 * m, n), dtype=torch.float32, device=dev)
    M[2 * cam, pt], M[2 * cam + 1, pt] = xy[:, 0], xy[:, 1]
    Ns = torch.from_numpy(np.repeat(np.linalg.inv(K)[None], m, 0).astype(np.float32)).to(dev)
    return M, Ns, torch.from_numpy(Ps.astype(np.float32)).to(dev)


def timed(variants, reps, warmup=3):
    """{name: (median, min, max) ms} of the interleaved variants."""
    ms = {k: [] for k in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def sample_aug(full, views, dense=None):
    np.random.seed(1)
    torch.manual_seed(1)
    s = sd.sample_data_device(full, views, build=False)
    a = sd.apply_rotational_homography_aug_device(s, 15, 20)
    if dense is None:
        return a
    # the reference's dense path beside it, in torch ops on the device: SceneData.py:326, :334, :434
    np.random.seed(1)
    idx = torch.from_numpy(sd.sample_indices(len(full.y), views, True)).to(dense.device)
    rows = torch.stack([2 * idx, 2 * idx + 1], 1).view(-1)
    keep = torch.nonzero(sd._native.scene_mask(full._M[rows].contiguous())[2] > 0).view(-1)
    d = dense[idx][:, keep]
    torch.manual_seed(1)
    R = sd.rotational_homography(views, 15, 20).to(dense.device)
    h = torch.cat([s._M.view(views, 2, -1), torch.ones((views, 1, s._M.shape[1]), device=dense.device)], 1)
    old = s.Ns @ h
    new = R @ old
    d = d / old[:, 2, :] * new[:, 2, :]
    a.depths = d[a.x.indices[0], a.x.indices[1]]
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "depth_targets.jsonl"))
    ap.add_argument("--skip-config4", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []

    def record(workload, shape, t):
        for name, (med, lo, hi) in t.items():
            rows.append({"workload": workload, **shape, "variant": name, "reps": args.reps,
                         "median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)})
            print(json.dumps(rows[-1]), flush=True)

    # ---- config 3: sample + augmentation + one graph build
    M, Ns, Ps = consistent_scene(100, 20_000, 100, dev)
    plain = sd.scene_from_dense_device(M, Ns, Ps, "train0")
    full = sd.scene_from_dense_device(M, Ns, Ps, "train0", store_depth_targets=True)
    dense = torch.zeros((100, 20_000), device=dev)
    dense[full.x.indices[0], full.x.indices[1]] = full.depths
    E = int(sample_aug(full, 20).depths.shape[0])
    a, b = sample_aug(full, 20), sample_aug(plain, 20, dense)
    err = float((a.depths - b.depths).abs().max())
    record("config3 sample(20 views) + rhaug 15/20 + build", {"m": 100, "n": 20_000, "E_sample": E,
                                                                "max_abs_diff_vs_dense": err},
           timed({"no targets": lambda: sample_aug(plain, 20), "per-edge targets (HIP)": lambda: sample_aug(full, 20),
                  "dense [m, n] restatement (torch)": lambda: sample_aug(plain, 20, dense)}, args.reps))

    # ---- config 4: the full-scene build
    if not args.skip_config4:
        del dense, full, plain
        M, Ns, Ps = consistent_scene(1000, 200_000, 4, dev)
        full = sd.scene_from_dense_device(M, Ns, Ps, "config4", store_depth_targets=True)
        E = int(full.depths.shape[0])
        b = {"cam": full.x.indices[0], "pt": full.x.indices[1], **full._scene_build}

        def dense_build():
            s = sd.scene_from_dense_device(M, Ns, Ps, "config4")
            X = sd.triangulate_scene_device(M, Ns, Ps, b)
            d = ((Ns @ Ps) @ X.t())[:, 2, :]  # [m, n]: 800 MB
            s.depths = d[s.x.indices[0], s.x.indices[1]]
            return s
        err = float((dense_build().depths - full.depths).abs().max())
        reps = max(3, args.reps // 4)
        t = timed({"no targets": lambda: sd.scene_from_dense_device(M, Ns, Ps, "config4"),
                   "per-edge targets (HIP, DLT included)": lambda: sd.scene_from_dense_device(
                       M, Ns, Ps, "config4", store_depth_targets=True),
                   "dense [m, n] restatement (torch, DLT included)": dense_build}, reps, warmup=2)
        args.reps = reps
        record("config4 full-scene build", {"m": 1000, "n": 200_000, "E": E, "max_abs_diff_vs_dense": err}, t)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
