"""Event-timed forward and forward+backward of SetOfSetNet (the shipped dpesfm conf, width 256) on
one GPU: the fused HIP path against the torch-op composite path (the baseline: there is no earlier
SetOfSet path to measure), and the edge-update forward kernel alone against the fp32 MFMA peak.

    python tools/setofset_bench.py [--size small|config4|both] [--runs 7] [--warmup 3]
    python tools/setofset_bench.py --batch 4      (a batch of sampled scenes: per-scene loop / forward_batch)

small: synthetic.windowed_scene(40, 4000) (a sampled training scene); config4: synthetic.config4()
(1000 cameras, 200k points, ~4.0M edges; an [E, 256] activation is ~4 GB).  Reports the median of
--runs timed runs after --warmup, with min / max, one JSON line per size."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gasfm_amd  # noqa: E402
from gasfm_amd import _native, setofset, synthetic  # noqa: E402
from gasfm_amd.conf import dpesfm_conf  # noqa: E402
from oracle.weights import deterministic_state_dict  # noqa: E402

PEAK_FP32_MATRIX_TFLOPS = 157.3  # MI355X, fp32 MFMA


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": runs}


def bench(name, sc, runs, warmup, composite_too=True):
    dev = torch.device("cuda", 0)
    data = gasfm_amd.SceneData.from_synthetic(sc).to(dev)
    net = gasfm_amd.SetOfSetNet(dpesfm_conf())
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.to(dev)
    E = int(data.x.values.shape[0])
    out = {"size": name, "m": sc.m, "n": sc.n, "edges": E}

    def fwd():
        with torch.no_grad():
            return net(data)

    def fwd_bwd():
        for p in net.parameters():
            p.grad = None
        pred = net(data)
        (pred["Ps_norm"].sum() + pred["pts3D"].sum()).backward()

    for label, composite in (("hip", False),) + ((("composite", True),) if composite_too else ()):
        net.composite = composite
        out[label] = {"forward": timed(fwd, runs, warmup), "forward_backward": timed(fwd_bwd, runs, warmup)}
        torch.cuda.empty_cache()
    # the 256 -> 256 edge-update forward kernel alone
    edges = setofset.scene_edge_index(data, dev)
    X = torch.randn(E, 256, device=dev)
    W = torch.randn(256, 256, device=dev) / 16
    S, V = torch.randn(sc.n, 256, device=dev), torch.randn(sc.m, 256, device=dev)
    cm = torch.randn(256, device=dev)
    Y = torch.empty(E, 256, device=dev)
    t = timed(lambda: _native.sos_edge_fwd(X, W, edges.cam, edges.pt, S, V, cm, None, True, out=Y), runs, warmup)
    tflops = 2.0 * E * 256 * 256 / (t["median_ms"] * 1e-3) / 1e12
    out["edge_fwd_256"] = dict(t, tflops=tflops, fraction_of_fp32_mfma_peak=tflops / PEAK_FP32_MATRIX_TFLOPS)
    print(json.dumps(out), flush=True)


def bench_batch(B, runs, warmup):
    """B sampled training-size scenes (tools/train_step_bench.py's sampling: 10-20 adjacent views of a
    100-view, 20k-point scene, rotational-homography augmented), forward + ESFMLoss + backward:
    scene by scene (losses summed, one backward) against one union-graph forward (forward_batch,
    the union built inside the timed region as a training step builds it)."""
    import numpy as np
    from gasfm_amd.batch import SceneBatch, forward_batch
    from gasfm_amd.loss import ESFMLoss
    from gasfm_amd.scene_device import (apply_rotational_homography_aug_device, sample_data_device,
                                        scene_from_dense_device)
    dev = torch.device("cuda", 0)
    np.random.seed(0)
    torch.manual_seed(0)
    datas = []
    for i in range(B):
        sc = synthetic.windowed_scene(100, 20_000, seed=100 + i)
        full = scene_from_dense_device(torch.from_numpy(sc.dense_M()).to(dev), torch.from_numpy(sc.Ns()).to(dev),
                                       torch.from_numpy(sc.Ps_gt()).to(dev), f"train{i}")
        s = sample_data_device(full, int(np.random.randint(10, 21)), build=False)
        datas.append(apply_rotational_homography_aug_device(s, 15, 20))
    conf = dpesfm_conf()
    conf.put("loss", {"infinity_pts_margin": 1e-4, "pts_grad_equalization_pre_perspective_divide": True,
                      "normalize_grad_wrt_valid_projections_only": True, "hinge_loss": True,
                      "hinge_loss_weight": 1.0})
    net = gasfm_amd.SetOfSetNet(conf)
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.to(dev)
    lossf = ESFMLoss(conf)

    def step(forward):
        for p in net.parameters():
            p.grad = None
        sum(lossf(p, d) for p, d in zip(forward(), datas)).backward()

    fixed = SceneBatch(datas)
    out = {"batch": B, "views": [int(d.x.shape[0]) for d in datas], "points": [int(d.x.shape[1]) for d in datas],
           "edges": [int(d.x.values.shape[0]) for d in datas],
           "per_scene_loop": timed(lambda: step(lambda: [net(d) for d in datas]), runs, warmup),
           "forward_batch": timed(lambda: step(lambda: forward_batch(net, datas)), runs, warmup),
           "union_built_once": timed(lambda: step(lambda: fixed.split(net(fixed))), runs, warmup)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0,
                    help="B > 0: time a batch of B sampled training-size scenes, forward + ESFMLoss + backward, as "
                         "the per-scene loop and as forward_batch (instead of the --size rows)")
    ap.add_argument("--size", default="both", choices=["small", "config4", "both"])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-composite", action="store_true", help="time the HIP path only")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    if a.batch > 0:
        bench_batch(a.batch, a.runs, a.warmup)
        return
    if a.size in ("small", "both"):
        bench("windowed_scene(40, 4000)", synthetic.windowed_scene(40, 4000), a.runs, a.warmup, not a.no_composite)
    if a.size in ("config4", "both"):
        bench("config4", synthetic.config4(), a.runs, a.warmup, not a.no_composite)


if __name__ == "__main__":
    main()
