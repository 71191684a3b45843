"""Depth-head evaluation over the visibility edges (csrc/depth_eval.hip).

Reference: evaluation.py:33-72 and 241-301 with geo_utils.reprojection_error_backproj_random_view_pairs
(geo_utils.py:393-464): backproject every observed pixel with its predicted depth, hand the point to
another view of the same track (a random cyclic shift of the track) and reproject it there with the
ground-truth cameras.  The reference does this on dense [m, n, 3] fp64 arrays on the host (4.8 GB
each at m = 1000, n = 200k); here it is three per-edge operations,

  track_cycle       src[e'] = the edge whose backprojected point is reprojected at e'
  backproj_2view    err[e'], rdepth[e'] and the (sum, count) of the non-NaN errors
  depth_norm_stats  the mean depths (determine_depth_scale) and sum / min / max of the normalised depths

each with the kernel for float32 CUDA tensors and a restatement in torch ops (``*_torch``) beside it:
what CPU tensors and fp64 take, the tests' oracle and the benchmark's baseline.
"""
import torch

from .. import _native
from . import _binding
from ._binding import CAMTAB_FLOATS

__all__ = ["track_cycle", "track_cycle_torch", "draw_keys", "camera_table", "backproj_2view", "backproj_2view_torch",
           "depth_norm_stats", "depth_norm_stats_torch", "CAMTAB_FLOATS"]


def _kernels(t):
    return t.device.type == "cuda"


# ------------------------------------------------------------------ pairing
def draw_keys(E, device):
    """One random int32 key per edge from torch's generator of ``device`` (torch.manual_seed governs it)."""
    return torch.randint(0, 2 ** 31 - 1, (E,), dtype=torch.int32, device=device)


def track_cycle_torch(pt_ptr, perm, key):
    """gasfm_track_cycle in torch ops: (src [E] int32, bad [1] int32).  Within each track (the edges
    perm[pt_ptr[p] : pt_ptr[p + 1]]) the edges are ordered by (key, edge id); each takes its
    predecessor, the first takes the last.  Tracks of length 1 give -1 and are counted."""
    E, dev = key.shape[0], key.device
    ptr = pt_ptr.to(torch.int64)
    n = ptr.shape[0] - 1
    L = ptr[1:] - ptr[:-1]
    bad = (L == 1).sum().to(torch.int32).view(1)
    src = torch.full((E,), -1, dtype=torch.int32, device=dev)
    if E == 0 or n == 0:
        return src, bad
    edge = torch.arange(E, device=dev) if perm is None else perm.to(torch.int64)  # pt_ptr[n] == E
    track = torch.repeat_interleave(torch.arange(n, device=dev), L, output_size=E)
    word = (key.to(torch.int64)[edge] << 32) | edge
    by_word = torch.argsort(word, stable=True)
    order = by_word[torch.argsort(track[by_word], stable=True)]  # CSR positions by (track, key, edge id)
    e_sorted, t_sorted = edge[order], track[order]
    pos = torch.arange(e_sorted.shape[0], device=dev)
    first = pos == ptr[:-1][t_sorted]
    prev = torch.where(first, ptr[1:][t_sorted] - 1, pos - 1)
    val = torch.where(L[t_sorted] == 1, torch.full_like(e_sorted, -1), e_sorted[prev])
    src[e_sorted] = val.to(torch.int32)
    return src, bad


def track_cycle(pt_ptr, perm, key):
    """(src [E] int32, bad [1] int32): the kernel for CUDA tensors, the restatement otherwise."""
    if _kernels(key):
        return _binding.track_cycle(pt_ptr, perm, key)
    return track_cycle_torch(pt_ptr, perm, key)


# ------------------------------------------------------------------ 2-view error
def camera_table(K, y, dtype=torch.float32):
    """[m, CAMTAB_FLOATS]: per camera [R | t] = K^-1 y (12) | K^-1 (9) | K (9) | 0 0, from the calibration
    matrices K [m, 3, 3] and the ground-truth cameras y = K [R | t] [m, 3, 4]; m-sized batched fp64
    work on K's device, rounded to ``dtype`` at the end."""
    K64 = K.detach().to(torch.float64)
    Kinv = torch.linalg.inv(K64)
    Rt = Kinv @ y.detach().to(device=K64.device, dtype=torch.float64)
    m = K64.shape[0]
    tab = torch.zeros((m, CAMTAB_FLOATS), dtype=torch.float64, device=K64.device)
    tab[:, :12], tab[:, 12:21], tab[:, 21:30] = Rt.reshape(m, 12), Kinv.reshape(m, 9), K64.reshape(m, 9)
    return tab.to(dtype).contiguous()


def backproj_2view_torch(cam, pt, xy, d, scale, src, camtab):
    """gasfm_backproj_2view in torch ops, in ``camtab``'s dtype: (err [E], rdepth [E], tot [2] = the
    sum of the non-NaN errors and their count).  ``pt`` None: src is trusted to stay within its track."""
    dt, E, m = camtab.dtype, cam.shape[0], camtab.shape[0]
    cam, src = cam.to(torch.int64), src.to(torch.int64)
    ok = (src >= 0) & (src < E) & (cam >= 0) & (cam < m)
    e = torch.where(ok, src, torch.zeros_like(src))
    c2 = torch.where(ok, cam, torch.zeros_like(cam))
    c = cam[e] if E else cam
    ok = ok & (c >= 0) & (c < m)
    if pt is not None and E:
        ok = ok & (pt[e] == pt)
    c = torch.where(ok, c, torch.zeros_like(c))
    A, B = camtab[c], camtab[c2]
    Rt, Kinv = A[:, :12].view(-1, 3, 4), A[:, 12:21].view(-1, 3, 3)
    Rt2, K2 = B[:, :12].view(-1, 3, 4), B[:, 21:30].view(-1, 3, 3)
    xy = xy.to(dt)
    u, v = xy[e, 0], xy[e, 1]
    h = [Kinv[:, i, 0] * u + Kinv[:, i, 1] * v + Kinv[:, i, 2] for i in range(3)]
    dd = scale.to(dt).reshape(()) * d.to(dt)[e]
    loc = torch.stack([dd * (h[0] / h[2]), dd * (h[1] / h[2]), dd], 1) - Rt[:, :, 3]
    X = (Rt[:, :, :3].transpose(1, 2) @ loc[:, :, None])[:, :, 0]
    q = (Rt2[:, :, :3] @ X[:, :, None])[:, :, 0] + Rt2[:, :, 3]
    yp = (K2 @ q[:, :, None])[:, :, 0]
    nan = torch.full((), float("nan"), dtype=dt, device=camtab.device)
    err = torch.where(ok, torch.hypot(xy[:, 0] - yp[:, 0] / yp[:, 2], xy[:, 1] - yp[:, 1] / yp[:, 2]), nan)
    rdepth = torch.where(ok, q[:, 2], nan)
    good = ~torch.isnan(err)
    tot = torch.stack([torch.where(good, err, torch.zeros_like(err)).sum(), good.sum().to(dt)])
    return err, rdepth, tot


def backproj_2view(cam, pt, xy, d, scale, src, camtab, per_edge=False):
    """tot [2] = (sum of the non-NaN 2-view errors, their count), with ``per_edge`` also err [E] and
    rdepth [E].  float32 CUDA operands run gasfm_backproj_2view + gasfm_colsum; anything else the
    restatement in ``camtab``'s dtype."""
    if _kernels(camtab) and camtab.dtype == torch.float32:
        E, dev = cam.shape[0], cam.device
        err = torch.empty(E, dtype=torch.float32, device=dev) if per_edge else None
        rdepth = torch.empty(E, dtype=torch.float32, device=dev) if per_edge else None
        tot = _native.colsum(_binding.backproj_2view(cam, pt, xy, d, scale, src, camtab, err, rdepth))
        return (tot, err, rdepth) if per_edge else tot
    err, rdepth, tot = backproj_2view_torch(cam, pt, xy, d, scale, src, camtab)
    return (tot, err, rdepth) if per_edge else tot


# ------------------------------------------------------------------ depth scales and statistics
def depth_norm_stats_torch(dp, dg, stats=True):
    """gasfm_depth_norm_stats in torch ops: scales [2] (dp's dtype) = the means from an fp64 sum;
    stats [7] float64 = sum, min, max of dp / s_p; of dg / s_g; sum of |dp / s_p - dg / s_g|, the
    divisions and the difference in dp's dtype, the sums in fp64.  NaN propagates; no edges or no
    targets give NaN."""
    dev, E = dp.device, dp.shape[0]
    nan64 = torch.full((), float("nan"), dtype=torch.float64, device=dev)

    def mean(t):
        return (t.double().sum() / E).to(dp.dtype) if t is not None and E else nan64.to(dp.dtype)

    def red(t):  # torch.min / max propagate NaN as ndarray.min / max do
        return [t.double().sum(), t.min().double(), t.max().double()] if t is not None and E else [nan64] * 3

    scales = torch.stack([mean(dp), mean(dg)])
    if not stats:
        return scales, None
    a = dp / scales[0]
    b = dg / scales[1] if dg is not None else None
    diff = (a - b).abs().double().sum() if b is not None and E else nan64
    return scales, torch.stack(red(a) + red(b) + [diff])


def depth_norm_stats(dp, dg, stats=True):
    """(scales [2], stats [7] float64 or None): the kernel for float32 CUDA tensors, else the restatement."""
    if _kernels(dp) and dp.dtype == torch.float32:
        return _binding.depth_norm_stats(dp.contiguous(), None if dg is None else dg.contiguous(), stats)
    return depth_norm_stats_torch(dp, dg, stats)
