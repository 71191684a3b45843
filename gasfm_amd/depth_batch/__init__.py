"""The depth branch over a union batch (csrc/depth_batch.hip): DirectDepthLoss, the depth scales and
the 2-view error per scene of a ``static_batch.StaticBatch``, with launch geometry fixed by the bucket.

A union batch: scene s owns the edges [eoff[s], eoff[s + 1]) of E_cap edges (eoff int32 [S + 1]), the
batch loss is sum_s weight[s] * loss_s, the pad scene has weight 0 and contributes exact zeros even
where its depths are NaN.  A weighted scene without edges makes the loss NaN, as the reference's
mean of nothing.

  depth_loss_seg_fwd / _bwd   DirectDepthLoss per scene (loss.DepthLossFn's formula)
  depth_scales_seg            (mean dp, mean dg) per scene (depth_eval.depth_norm_stats' scales)
  backproj_2view_seg          depth_eval.backproj_2view with each scene's own rescale factor

Pairing needs nothing new: the scenes' tracks are disjoint, so ``depth_eval.track_cycle`` over the
union's point CSR pairs within scenes, and because the rank is (key, edge id) and a scene's union
edge ids are its own plus its edge offset, the union pairing of scene s minus eoff[s] is the
single-scene pairing from keys[eoff[s]:eoff[s + 1]].

Each entry runs the kernel for float32 CUDA tensors and a restatement in torch ops (``*_torch``)
otherwise: what CPU tensors and fp64 take, the tests' oracle and the benchmark's baseline.  The
restatements read eoff and weight on the host.
"""
import torch

from ..depth_eval import backproj_2view_torch, depth_norm_stats_torch
from . import _binding
from ._binding import SEG_G

__all__ = ["depth_loss_seg_fwd", "depth_loss_seg_fwd_torch", "depth_loss_seg_bwd", "depth_loss_seg_bwd_torch",
           "depth_scales_seg", "depth_scales_seg_torch", "backproj_2view_seg", "backproj_2view_seg_torch", "SEG_G"]


def _kernels(t):
    return t.device.type == "cuda" and t.dtype == torch.float32


def _scenes(eoff, weight=None):
    """[(s, e0, e1, weight)] on the host."""
    eo = [int(v) for v in eoff.tolist()]
    w = [1.0] * (len(eo) - 1) if weight is None else [float(v) for v in weight.tolist()]
    return [(s, eo[s], eo[s + 1], w[s]) for s in range(len(eo) - 1)]


def _u(a, b, Sa, Sb):
    """u_e = a / s_a - b / s_b the way csrc/depth_term.hpp evaluates it."""
    E = a.shape[0]
    return (a * Sb - b * Sa) * (E / (Sa * Sb))


# ------------------------------------------------------------------ DirectDepthLoss
def depth_loss_seg_fwd_torch(a, b, eoff, weight, l2):
    """gasfm_depth_loss_seg_sums + _seg_fwd in torch ops, in a's dtype: (loss [1], sums [S, 2], tot [S, 2])."""
    S = eoff.shape[0] - 1
    sums, tot = a.new_zeros((S, 2)), a.new_zeros((S, 2))
    loss = a.new_zeros(())
    for s, e0, e1, w in _scenes(eoff, weight):
        if w == 0.0:
            continue
        x, y = a[e0:e1], b[e0:e1]
        Sa, Sb = x.sum(), y.sum()
        u = _u(x, y, Sa, Sb)
        g = 2 * u if l2 else torch.sign(u)
        sums[s, 0], sums[s, 1] = Sa, Sb
        tot[s, 0], tot[s, 1] = (u * u if l2 else u.abs()).sum(), (g * x).sum()
        loss = loss + w * (tot[s, 0] / (e1 - e0) if e1 > e0 else a.new_tensor(float("nan")))
    return loss.reshape(1), sums, tot


def depth_loss_seg_bwd_torch(a, b, eoff, weight, sums, tot, l2, dloss):
    """gasfm_depth_loss_seg_bwd in torch ops: da [E_cap], exact zeros in a scene of weight 0."""
    da = torch.zeros_like(a)
    for s, e0, e1, w in _scenes(eoff, weight):
        if w == 0.0 or e1 <= e0:
            continue
        E = e1 - e0
        x, y = a[e0:e1], b[e0:e1]
        Sa, Sb = sums[s, 0], sums[s, 1]
        u = _u(x, y, Sa, Sb)
        g = 2 * u if l2 else torch.sign(u)
        inv_sa = E / Sa
        da[e0:e1] = dloss.reshape(()) * w / E * inv_sa * (g - tot[s, 1] / E * inv_sa)
    return da


def depth_loss_seg_fwd(a, b, eoff, weight, l2):
    """(loss [1], sums [S, 2], tot [S, 2]): the kernels for float32 CUDA tensors, else the restatement."""
    if _kernels(a):
        return _binding.depth_loss_seg_fwd(a, b, eoff, weight, l2)
    return depth_loss_seg_fwd_torch(a, b, eoff, weight, l2)


def depth_loss_seg_bwd(a, b, eoff, weight, sums, tot, l2, dloss):
    if _kernels(a):
        return _binding.depth_loss_seg_bwd(a, b, eoff, weight, sums, tot, l2, dloss)
    return depth_loss_seg_bwd_torch(a, b, eoff, weight, sums, tot, l2, dloss)


# ------------------------------------------------------------------ depth scales
def depth_scales_seg_torch(dp, dg, eoff):
    """gasfm_depth_scales_seg in torch ops: scales [S, 2] (dp's dtype), depth_norm_stats_torch's per scene."""
    return torch.stack([depth_norm_stats_torch(dp[e0:e1], dg[e0:e1], stats=False)[0] for _, e0, e1, _ in _scenes(eoff)])


def depth_scales_seg(dp, dg, eoff):
    if _kernels(dp):
        return _binding.depth_scales_seg(dp.contiguous(), dg.contiguous(), eoff)
    return depth_scales_seg_torch(dp, dg, eoff)


# ------------------------------------------------------------------ 2-view error
def backproj_2view_seg_torch(cam, pt, xy, d, scales, src, eoff, camtab):
    """gasfm_backproj_2view_seg in torch ops, in ``camtab``'s dtype: (tot [S, 2], err [E_cap], rdepth [E_cap]);
    err / rdepth are NaN outside the scenes.  The union's src is followed across the whole edge list and
    each destination edge takes its scene's factor scales[s][1] / scales[s][0]."""
    dt, E = camtab.dtype, cam.shape[0]
    spans = _scenes(eoff)
    err = torch.full((E,), float("nan"), dtype=dt, device=camtab.device)
    rdepth = err.clone()
    tot = camtab.new_zeros((len(spans), 2))
    for s, e0, e1, _ in spans:
        # the whole union with scene s's factor, of which scene s's destination edges are kept
        factor = scales[s, 1].to(dt) / scales[s, 0].to(dt)
        e_s, r_s, _ = backproj_2view_torch(cam, pt, xy, d, factor, src, camtab)
        err[e0:e1], rdepth[e0:e1] = e_s[e0:e1], r_s[e0:e1]
        good = ~torch.isnan(e_s[e0:e1])
        tot[s, 0], tot[s, 1] = e_s[e0:e1][good].sum(), good.sum()
    return tot, err, rdepth


def backproj_2view_seg(cam, pt, xy, d, scales, src, eoff, camtab, per_edge=False):
    """tot [S, 2] = per scene (sum of the non-NaN 2-view errors, count), with ``per_edge`` also err and
    rdepth [E_cap].  float32 CUDA operands run gasfm_backproj_2view_seg, anything else the restatement."""
    if _kernels(camtab):
        E, dev = cam.shape[0], cam.device
        nan = float("nan")
        err = torch.full((E,), nan, dtype=torch.float32, device=dev) if per_edge else None
        rdepth = torch.full((E,), nan, dtype=torch.float32, device=dev) if per_edge else None
        tot = _binding.backproj_2view_seg(cam, pt, xy, d, scales, src, eoff, camtab, err, rdepth)
        return (tot, err, rdepth) if per_edge else tot
    tot, err, rdepth = backproj_2view_seg_torch(cam, pt, xy, d, scales, src, eoff, camtab)
    return (tot, err, rdepth) if per_edge else tot
