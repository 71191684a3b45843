"""Time a depth-head training step over a batch: captured (StaticTrainer) against the eager union.

usage: python tools/depth_batch_bench.py [--views 12,15,17,20] [--m M] [--n N] [--layers L] [--reps R] [--trials T]
                                         [--out profiles/depth_batch.jsonl]
A config-3 style batch: scenes of --m views and --n points (gasfm_amd.synthetic.windowed_scene's
visibility over cameras on a circle, so that the depth targets can be triangulated), each sampled to
one of --views views and augmented on the device, with per-edge depth targets; the GASFM learning
conf with the 128-wide depth head and no view / scenepoint head.  Variants, interleaved: a warm-up
block of each, then --trials rounds of one timed block of --reps calls each (between device events on
the launch stream); a line reports the median block with the minimum and maximum.

  step      StaticTrainer.step (fill + one graph replay: forward, DirectDepthLoss, 2-view error,
            backward) against the eager union step on the same tree: SceneBatch forward, per-scene
            DirectDepthLoss, per-scene 2-view error (evaluation.backproj_2view_error), backward
  loss      the segmented loss forward + backward against B calls of the single-scene kernels
  2-view    scales -> pairing -> segmented 2-view error against B single-scene sequences
One JSON line per variant, printed and written to --out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gasfm_amd  # noqa: E402
from gasfm_amd import _native, depth_batch, depth_eval, evaluation, static_batch, synthetic  # noqa: E402
from gasfm_amd.batch import SceneBatch  # noqa: E402
from gasfm_amd.loss import DirectDepthLoss  # noqa: E402
from gasfm_amd.scene_device import (apply_rotational_homography_aug_device, sample_data_device,  # noqa: E402
                                    scene_from_dense_device)

from depth_eval_bench import interleaved, spread  # noqa: E402


def full_scene(dev, m, n, seed):
    sc = synthetic.windowed_scene(m, n, mean_extra=6, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    ang = np.linspace(0, 2 * np.pi, m, endpoint=False)
    C = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.3 * rng.standard_normal(m)], 1)
    R = np.stack([synthetic.rotation_look_at(c) for c in C])
    Rt = np.concatenate([R.transpose(0, 2, 1), -(R.transpose(0, 2, 1) @ C[:, :, None])], 2)
    X = rng.uniform(-1, 1, size=(n, 3))
    q = np.einsum("eij,ej->ei", Rt[sc.cam], np.concatenate([X[sc.pt], np.ones((sc.num_edges, 1))], 1))
    pix = q @ sc.K.T
    sc.xy = (pix[:, :2] / pix[:, 2:]).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return scene_from_dense_device(t(sc.dense_M()), t(sc.Ns()), t((sc.K[None] @ Rt).astype(np.float32)), f"s{seed}",
                                   store_depth_targets=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="12,15,17,20")
    ap.add_argument("--m", type=int, default=40)
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5, help="timed blocks per variant")
    ap.add_argument("--out", default=os.path.join("profiles", "depth_batch.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    np.random.seed(0)
    torch.manual_seed(0)
    views = [int(v) for v in args.views.split(",")]
    datas = [apply_rotational_homography_aug_device(sample_data_device(full_scene(dev, args.m, args.n, 10 + i), v), 15, 20)
             for i, v in enumerate(views)]
    off = {"enabled": False, "n_hidden_layers": 2}
    conf = gasfm_amd.learning_conf(num_layers=args.layers, depth_head={"enabled": True, "n_feat": 128, "n_hidden_layers": 2},
                                   view_head=dict(off, rot_representation="quat"), scenepoint_head=off)
    conf.put("loss.cost_fcn", "L2")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(dev)
    lossf = DirectDepthLoss(conf)
    B = len(datas)
    st = static_batch.BatchStats(datas)
    if st.expressible() is not None:
        raise SystemExit(f"the batch does not fit the padded scheme: {st.expressible()}")
    trainer = static_batch.StaticTrainer(net, lossf, two_view_error=True)
    trainer.step(datas, stats=st)
    sb, step = next(iter(trainer.buckets.values()))[:2]
    info = {"B": B, "views": views, "E": st.E, "E_cap": sb.caps.E, "layers": args.layers, "captured": step.captured,
            "fallbacks": trainer.fallbacks}

    def captured():
        return trainer.step(datas, stats=st, read_errors=False)

    def eager():
        for p in net.parameters():
            p.grad = None
        union = SceneBatch(datas)
        preds = union.split(net(union))
        loss = sum(lossf(p, d) for p, d in zip(preds, datas))
        errs = [evaluation.backproj_2view_error(d, *evaluation._depth_pair(d, p))[0] for p, d in zip(preds, datas)]
        loss.backward()
        return loss, errs

    # the kernels alone, on the filled bucket
    with torch.no_grad():
        a = net(sb)["depths"].values[:, 0].contiguous()
    eo = sb.offsets[2]
    dloss = torch.ones(1, device=dev)
    per = [(a[eo[i]:eo[i + 1]].contiguous(), d.depths, d) for i, d in enumerate(datas)]

    def seg_loss():
        loss, sums, tot = depth_batch.depth_loss_seg_fwd(a, sb.depths, sb.eoff, sb.weight, True)
        return depth_batch.depth_loss_seg_bwd(a, sb.depths, sb.eoff, sb.weight, sums, tot, True, dloss)

    def single_loss():
        out = []
        for x, y, _ in per:
            sums, tot = _native.depth_loss_fwd(x, y, True)
            out.append(_native.depth_loss_bwd(x, y, sums, tot, True, dloss))
        return out

    def seg_2view():
        scales = depth_batch.depth_scales_seg(a, sb.depths, sb.eoff)
        src, _ = depth_eval.track_cycle(sb.pt_ptr, sb.perm, sb.pair_keys)
        return depth_batch.backproj_2view_seg(sb.cam32, None, sb.xy, a, scales, src, sb.eoff, sb.camtab)

    def single_2view():
        return [evaluation.backproj_2view_error(d, x, y)[0] for x, y, d in per]

    pairs = {"step: forward, DirectDepthLoss, 2-view error, backward": {"captured (fill + replay)": captured,
                                                                       "eager union": eager},
             "loss forward + backward": {"segmented": seg_loss, f"{B} single-scene calls": single_loss},
             "scales, pairing, 2-view error": {"segmented": seg_2view, f"{B} single-scene sequences": single_2view}}
    lines = []
    for op, fns in pairs.items():
        for variant, v in interleaved(fns, args.reps, args.trials).items():
            lines.append({"op": op, "variant": variant, **info, **spread(v)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
