"""Time a depth conf's last (32 -> 128) block on the fused edge kernels against the unfused route.

usage: python tools/wide_block_bench.py [--reps R] [--trials T] [--skip-config4] [--out profiles/wide_block.jsonl]
The GASFM learning conf with the 128-wide depth head and no view / scenepoint head.  The last block's
inputs (P, the three state features, P0) are recorded from one real forward; its forward + backward
(GraphAttnSfMLayer.forward_plan, then backward of P' against a fixed gradient) then runs with
model.EDGE_WIDE on (edge_block.WideEpilogueFn, csrc/edge_wide.hip) and off (layer_norm_relu,
projection_update and the skip projection on aten, the route before the kernels existed), on the same
tensors.  Variants run interleaved: a warm-up block of each, then --trials rounds of one timed block of
--reps calls each (between device events on the launch stream); a line reports the median block with
the minimum and maximum, and torch.cuda.max_memory_allocated over one forward + backward beyond what
was resident before it.

  config 4   one scene, m = 1000, n = 200k, E = 4,001,638
  batch      the 4-scene config-3 style depth batch of tools/depth_batch_bench.py in its padded bucket;
             also StaticTrainer's captured step with the route on against the route off
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
from gasfm_amd import edge_block, model, static_batch, synthetic  # noqa: E402
from gasfm_amd.loss import DirectDepthLoss  # noqa: E402
from gasfm_amd.scene_device import apply_rotational_homography_aug_device, sample_data_device  # noqa: E402

from depth_batch_bench import full_scene  # noqa: E402
from depth_eval_bench import interleaved, spread  # noqa: E402
from depth_head_bench import peak_new_bytes  # noqa: E402


def last_block_inputs(net, data):
    """The last block's forward_plan arguments in one real forward of net on data (no gradient)."""
    blk = net.equivariant_blocks[-1]
    seen = {}
    orig = blk.forward_plan

    def record(P, plans, edges, prev_pt=None, prev_view=None, prev_glob=None, P0=None, carry=None, nxt=None):
        P = edge_block.materialize(P)
        seen.update(P=P, plans=plans, edges=edges, prev=(prev_pt, prev_view, prev_glob), P0=P0)
        return orig(P, plans, edges, prev_pt, prev_view, prev_glob, P0=P0, carry=carry, nxt=nxt)

    blk.forward_plan = record
    try:
        with torch.no_grad():
            net(data)
    finally:
        del blk.forward_plan
    return seen


def block_step(net, seen, wide):
    """forward + backward of the last block on the recorded inputs, the route on (wide) or off."""
    blk = net.equivariant_blocks[-1]
    leaf = lambda t: t.detach().clone().requires_grad_(True)  # noqa: E731
    P, P0 = leaf(seen["P"]), leaf(seen["P0"])
    prev = tuple(leaf(t) for t in seen["prev"])
    g = torch.Generator(device=P.device).manual_seed(1)
    dPo = torch.randn(P.shape[0], 128, device=P.device, generator=g)

    def run():
        model.EDGE_WIDE = wide
        for t in (P, P0, *prev, *blk.parameters()):
            t.grad = None
        out = blk.forward_plan(P, seen["plans"], seen["edges"], *prev, P0=P0)[0]
        assert blk.last_route == ("wide" if wide else "unfused")
        out.backward(dPo)
    return run


def measure_block(net, data, tag, args, lines):
    seen = last_block_inputs(net, data)
    E = int(seen["P"].shape[0])
    fns = {"fused edge kernels (route on)": block_step(net, seen, True),
           "unfused aten route (route off)": block_step(net, seen, False)}
    times = interleaved(fns, args.reps, args.trials)
    for k, fn in fns.items():
        mem = peak_new_bytes(fn)
        lines.append({"op": "last block forward + backward", "case": tag, "variant": k, "E": E, **spread(times[k]),
                      "peak_new_bytes": mem, "peak_new_over_Pout": round(mem / (E * 128 * 4), 3)})
        print(json.dumps(lines[-1]), flush=True)
    model.EDGE_WIDE = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trials", type=int, default=5, help="timed blocks per variant")
    ap.add_argument("--skip-config4", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "wide_block.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    np.random.seed(0)
    torch.manual_seed(0)
    off = {"enabled": False, "n_hidden_layers": 2}
    conf = gasfm_amd.learning_conf(depth_head={"enabled": True, "n_feat": 128, "n_hidden_layers": 2},
                                   view_head=dict(off, rot_representation="quat"), scenepoint_head=off)
    conf.put("loss.cost_fcn", "L2")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(dev)
    lines = []

    # the 4-scene batch: the block on the filled bucket, then the captured step with the route on and off
    views = [12, 15, 17, 20]
    datas = [apply_rotational_homography_aug_device(sample_data_device(full_scene(dev, 40, 4000, 10 + i), v), 15, 20)
             for i, v in enumerate(views)]
    lossf = DirectDepthLoss(conf)
    st = static_batch.BatchStats(datas)
    if st.expressible() is not None:
        raise SystemExit(f"the batch does not fit the padded scheme: {st.expressible()}")
    trainers = {}
    for wide in (True, False):
        model.EDGE_WIDE = wide
        tr = trainers[wide] = static_batch.StaticTrainer(net, lossf, two_view_error=True)
        tr.step(datas, stats=st)
        assert net.equivariant_blocks[-1].last_route == ("wide" if wide else "unfused")
    model.EDGE_WIDE = True
    sb, step = next(iter(trainers[True].buckets.values()))[:2]
    measure_block(net, sb, "4-scene batch bucket", args, lines)
    info = {"B": len(datas), "views": views, "E": st.E, "E_cap": sb.caps.E}
    fns = {"route on": lambda: trainers[True].step(datas, stats=st, read_errors=False),
           "route off": lambda: trainers[False].step(datas, stats=st, read_errors=False)}
    for k, v in interleaved(fns, args.reps, args.trials).items():
        tr = trainers[k == "route on"]
        lines.append({"op": "captured step (fill + replay)", "case": "4-scene batch", "variant": k, **info,
                      "captured": next(iter(tr.buckets.values()))[1].captured, "fallbacks": tr.fallbacks, **spread(v)})
        print(json.dumps(lines[-1]), flush=True)
    del trainers, sb, step

    if not args.skip_config4:
        data = gasfm_amd.SceneData.from_synthetic(synthetic.config4()).to(dev)
        measure_block(net, data, "config 4", args, lines)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in lines:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
