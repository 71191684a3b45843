"""Time a training loss at config 4 (m = 1000, n = 200k, ~4M edges) on the GPU box.

usage: python tools/loss_bench.py [--reps R] [--loss {esfm,ose,depth}]
Lines (JSON): the HIP loss kernels one by one (HIP events on the launch stream) with achieved
GB/s from their algorithmic bytes, the whole HIP loss forward+backward, and the
reference formulation (code/loss_functions.py:85-123: dense Ps @ pts3D [m, 3, n], masks,
gradient hook) run by torch on the same GPU for comparison.

Each line is the median of --trials timed blocks of --reps calls after a warm-up block, with the
blocks' min and max.  --loss ose / depth: ExpDepthRegularizedOSELoss / DirectDepthLoss; the
comparison is the same per-edge formula in torch ops (gather, elementwise, index_add backward).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gasfm_amd import Conf, SceneData, _native, synthetic  # noqa: E402
from gasfm_amd.loss import ESFMLoss, _edge_tensors  # noqa: E402


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _time_spread(fn, reps, trials):
    """Median / min / max us per call over `trials` timed blocks (after one warm-up block)."""
    _time(fn, reps)
    t = sorted(_time(fn, reps) for _ in range(trials))
    return {"us": round(t[len(t) // 2], 1), "us_min": round(t[0], 1), "us_max": round(t[-1], 1)}


def torch_edge_ose(Ps, X, cam, pt, vals, w_reg):
    """The OSE loss per edge in torch ops: gathers, elementwise, autograd's index_add backward."""
    y = torch.bmm(Ps.index_select(0, cam), X.index_select(1, pt).T.unsqueeze(2)).squeeze(2)
    r = y[:, :2] - y[:, 2:3] * vals
    return (r.norm(dim=1) + w_reg * torch.exp(-y[:, 2])).mean()


def bench_ose(args, dev, data, Ps, X, E, m, n):
    from gasfm_amd.loss import ExpDepthRegularizedOSELoss
    w_reg = 0.1
    lossf = ExpDepthRegularizedOSELoss(Conf({"model": {"view_head": {"enabled": True},
                                                       "scenepoint_head": {"enabled": True}},
                                             "loss": {"depth_regul_weight": w_reg}}))

    def report(name, t, nbytes=None, **kw):
        r = {"op": name, **t, **kw}
        if nbytes:
            r["GBps"] = round(nbytes / t["us"] / 1e3, 1)
            r["bytes_per_edge"] = round(nbytes / E, 1)
        print(json.dumps(r), flush=True)

    (cam, pt), vals, cptr, pptr, perm = _edge_tensors(data)
    P = Ps.reshape(m, 12).contiguous()
    # algorithmic bytes as the ESFM kernels: forward cam + pt + 2 values per edge, points and cameras once
    report("ose_fwd", _time_spread(lambda: _native.ose_fwd(cam, pt, vals, P, X, w_reg), args.reps, args.trials),
           16 * E + 16 * n + 48 * m)
    dloss = torch.ones(1, device=dev)
    dP, dX = torch.empty_like(P), torch.empty_like(X)
    # camera pass: pt + 2 values per edge, points once, dP; point pass: perm + cam + 2 values per edge, X + dX
    report("ose_bwd (cam + pt kernels)",
           _time_spread(lambda: _native.ose_bwd(cptr, pptr, perm, cam, pt, vals, P, X, w_reg, dloss, dP, dX),
                        args.reps, args.trials), (12 * E + 16 * n + 96 * m) + (16 * E + 36 * n + 48 * m))
    Pr, Xr = Ps.clone().requires_grad_(True), X.clone().requires_grad_(True)

    def hip_step():
        Pr.grad = Xr.grad = None
        lossf({"Ps_norm": Pr, "pts3D": Xr}, data).backward()

    report("ExpDepthRegularizedOSELoss fwd+bwd (HIP, autograd)", _time_spread(hip_step, args.reps, args.trials), E=E)
    cam64, pt64 = data.x.indices[0].contiguous(), data.x.indices[1].contiguous()

    def torch_step():
        Pr.grad = Xr.grad = None
        torch_edge_ose(Pr, Xr, cam64, pt64, vals, w_reg).backward()

    report("per-edge formula fwd+bwd (torch ops, same GPU)",
           _time_spread(torch_step, max(3, args.reps // 4), args.trials), E=E)


def bench_depth(args, dev, E):
    g = torch.Generator(device=dev).manual_seed(0)
    a = 0.5 + 2.0 * torch.rand(E, device=dev, generator=g)
    b = 1.0 + 3.0 * torch.rand(E, device=dev, generator=g)
    L = _native.lib()

    def report(name, t, nbytes=None, **kw):
        r = {"op": name, **t, **kw}
        if nbytes:
            r["GBps"] = round(nbytes / t["us"] / 1e3, 1)
            r["bytes_per_edge"] = round(nbytes / E, 1)
        print(json.dumps(r), flush=True)

    part = torch.empty((L.gasfm_depth_loss_part_rows(E), 2), device=dev)
    p, st = _native._p, _native._stream
    sums, tot = _native.depth_loss_fwd(a, b, False)
    dloss = torch.ones(1, device=dev)
    report("depth_loss_sums", _time_spread(lambda: L.gasfm_depth_loss_sums(p(a), p(b), E, p(part), st(a)), args.reps,
                                           args.trials), 8 * E)
    report("depth_loss_fwd", _time_spread(lambda: L.gasfm_depth_loss_fwd(p(a), p(b), E, p(sums), 0, p(part), st(a)),
                                          args.reps, args.trials), 8 * E)
    report("depth_loss_bwd", _time_spread(lambda: _native.depth_loss_bwd(a, b, sums, tot, False, dloss), args.reps,
                                          args.trials), 12 * E)
    from gasfm_amd.loss import DepthLossFn
    ar = a.clone().requires_grad_(True)

    def hip_step():
        ar.grad = None
        DepthLossFn.apply(ar, b, False).backward()

    report("DirectDepthLoss L1 fwd+bwd (HIP, autograd)", _time_spread(hip_step, args.reps, args.trials), E=E)

    def torch_step():
        ar.grad = None
        (ar / ar.mean() - b / b.mean()).abs().mean().backward()

    report("same formula fwd+bwd (torch ops, same GPU)", _time_spread(torch_step, args.reps, args.trials), E=E)


def dense_reference_loss(Ps, pts3D, norm_M, valid, margin=1e-4, w=1.0):
    """The reference's ESFMLoss.forward for the conf/learning loss section, on dense tensors."""
    pts_2d = Ps @ pts3D
    mask = pts_2d[:, 2, :] >= margin
    npos = max(1, torch.sum(valid & mask).item())
    pts_2d.register_hook(lambda g: torch.where(mask[:, None, :].repeat(1, 3, 1), F.normalize(g, dim=1) / npos, g))
    hinge = (margin - pts_2d[:, 2, :]) * w
    pts_2d = pts_2d / torch.where(mask, pts_2d[:, 2, :], torch.ones_like(mask).float()).unsqueeze(1)
    reproj = (pts_2d[:, 0:2, :] - norm_M.reshape(Ps.shape[0], 2, -1)).norm(dim=1)
    return torch.where(mask, reproj, hinge)[valid].mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--loss", choices=("esfm", "ose", "depth"), default="esfm")
    ap.add_argument("--trials", type=int, default=5, help="timed blocks per line")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sc = synthetic.config4()
    data = SceneData.from_synthetic(sc).to(dev)
    E, m, n = sc.num_edges, sc.m, sc.n
    g = torch.Generator(device=dev).manual_seed(0)
    Ps = torch.zeros((m, 3, 4), device=dev)
    Ps[:, :, :3] = torch.eye(3, device=dev) + 0.1 * torch.randn((m, 3, 3), device=dev, generator=g)
    Ps[:, :, 3] = 0.3 * torch.randn((m, 3), device=dev, generator=g)
    X = torch.randn((4, n), device=dev, generator=g)
    X[2] = 2.0 + 1.5 * X[2]
    X[3] = 1.0
    if args.loss == "ose":
        return bench_ose(args, dev, data, Ps, X, E, m, n)
    if args.loss == "depth":
        return bench_depth(args, dev, E)
    conf = Conf({"model": {"view_head": {"enabled": True}, "scenepoint_head": {"enabled": True}},
                 "loss": {"infinity_pts_margin": 1e-4, "pts_grad_equalization_pre_perspective_divide": True,
                          "normalize_grad_wrt_valid_projections_only": True, "hinge_loss": True,
                          "hinge_loss_weight": 1.0}})
    lossf = ESFMLoss(conf)

    def report(name, t, nbytes=None, **kw):
        r = {"op": name, **t, **kw}
        if nbytes:
            r["GBps"] = round(nbytes / t["us"] / 1e3, 1)
        print(json.dumps(r), flush=True)

    def timed(fn, reps):
        return _time_spread(fn, reps, args.trials)

    (cam, pt), vals, cptr, pptr, perm = _edge_tensors(data)
    P = Ps.reshape(m, 12).contiguous()
    part = torch.empty((_native.esfm_part_rows(E), 2), device=dev)
    margin, w, hinge, eq, vo = lossf.kernel_conf()
    # algorithmic bytes: per edge cam + pt + 2 values (16 B) + each point's 4 coords once + cameras once
    fwd_bytes = 16 * E + 16 * n + 48 * m
    report("esfm_fwd", timed(lambda: _native.esfm_fwd(cam, pt, vals, P, X, margin, w, hinge, part), args.reps),
           fwd_bytes)
    # compute_core_errors' reprojection error (gasfm_reproj_error): same bytes as esfm_fwd
    report("reproj_error", timed(lambda: _native.reproj_error(cam, pt, vals, P, X), args.reps), fwd_bytes)
    tot = _native.colsum(part)
    dloss = torch.ones(1, device=dev)
    dP, dX = torch.empty_like(P), torch.empty_like(X)
    # camera pass: pt + 2 values per edge + point coords; point pass: perm + cam + 2 values per edge + dX
    bwd_bytes = (12 * E + 16 * n + 48 * m) + (16 * E + 32 * n + 4 * n + 48 * m)
    report("esfm_bwd (cam + pt kernels)",
           timed(lambda: _native.esfm_bwd(cptr, pptr, perm, cam, pt, vals, P, X, margin, w, hinge, eq, vo, dloss,
                                          tot, dP, dX), args.reps), bwd_bytes)

    Pr, Xr = Ps.clone().requires_grad_(True), X.clone().requires_grad_(True)

    def hip_step():
        Pr.grad = Xr.grad = None
        lossf({"Ps_norm": Pr, "pts3D": Xr}, data).backward()

    report("ESFMLoss fwd+bwd (HIP, autograd)", timed(hip_step, args.reps), E=E)
    if not args.no_dense:
        nm = torch.zeros((m, n, 2), device=dev)
        nm[data.x.indices[0], data.x.indices[1]] = data.x.values
        norm_M = nm.permute(0, 2, 1).reshape(2 * m, n)
        valid = torch.zeros((m, n), dtype=torch.bool, device=dev)
        valid[data.x.indices[0], data.x.indices[1]] = True

        def dense_step():
            Pr.grad = Xr.grad = None
            dense_reference_loss(Pr, Xr, norm_M, valid).backward()

        report("reference formulation fwd+bwd (torch dense, same GPU)", timed(dense_step, max(3, args.reps // 4)),
               E=E)


if __name__ == "__main__":
    main()
