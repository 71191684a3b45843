"""A rank's point shard of a device scene, built on the device (csrc/scene_shard.hip).

``dist_train.shard_device_scene`` copies every edge and value of the sampled scene to the host, runs
``distributed.shard_scene`` in numpy there (partition_points, boolean selection, SceneData.from_sparse,
seven AttnPlan.from_targets calls through gasfm_build_csr / gasfm_plan_work) and copies the shard back.
``shard_scene_on_device`` returns the same (network shard, loss shard) pair -- every index, count, value
and plan array equal element for element -- from the scene's own device arrays:

  boundaries          gasfm_scene_shard_bounds     partition_points over the stable point CSR
  per-camera runs     gasfm_scene_shard_cam_range  edges are cam-major with points ascending inside a
                                                   camera: a rank's edges of a camera are one run;
                                                   the local cam_ptr is their exclusive scan
                                                   (gasfm_scan_i32)
  local edges         gasfm_scene_shard_emit       indices, int32 copies, bit copies of the network's
                                                   values, the loss's values and the pixel measurements
  local point CSR     gasfm_scene_shard_point_csr  sliced and re-based from the global one (the stable
                                                   order gasfm_build_csr gives the local edges)
  work items          scene_device.plan_work_device / _plan over those CSR arrays (torch device ops)

Host reads: two, of a few integers each, whatever E, m and n are.
  1. gasfm_scene_shard_stats' nine scalars: p0, p1, E_loc, and (count, first invalid index) of the
     valid views, of the own camera rows' valid views and of the local valid points.  They size the
     outputs and fix camera_max_piece(E_loc), the global graphs' piece lengths and whether their
     source lists are identities.
  2. the piece counts of the camera- and point-direction plans (scene_device._piece_stats) and
     whether the local edge list is point-sorted (then the point direction needs no permutation),
     nine integers in one ``.tolist()``.
Host writes: the two-entry seg_ptr of each one-target plan, and ``point_bounds`` when given.

CPU tensors take a restatement of the kernels in torch ops (searchsorted, cumsum, repeat_interleave,
index arithmetic), as StaticBatch.fill_torch stands beside fill: the kernels' second oracle, and what
the CPU suite runs.  CUDA tensors take the kernels; without the native library that is an error, as
everywhere in this package (``kernels=False`` asks for the torch restatement on the device).
"""
import copy

import numpy as np
import torch

from . import _native
from .attention import DEFAULT_MAX_PIECE, camera_max_piece
from .distributed import ShardContext, camera_rows
from .evaluation import _pixel_measurements
from .scene import (MIN_N_POINTS_PER_VIEW, MIN_N_VIEWS_PER_POINT, AxialAggregationGraphWrapper, SceneData,
                    SparseMat)
from .scene_device import _piece_stats, _plan, _star_source_plan


def _csr_arrays(data):
    """(cam_ptr, pt_ptr, perm or None) of a scene: the device scene build's arrays while its graph
    wrappers are not built (batch._scene_arrays' rule), else its plans' (perm None: point-sorted)."""
    b = data.__dict__.get("_scene_build")
    if b is not None and "graph_wrappers" not in data.__dict__:
        return b["cam_ptr"], b["pt_ptr"], b["perm"]
    gw = data.graph_wrappers
    p = gw["proj2scenepoint"].plan
    return gw["proj2view"].plan.seg_ptr, p.seg_ptr, p.perm


# ------------------------------------------------------------------ the kernels, restated in torch ops
def _bounds_torch(pt_ptr, world):
    """gasfm_scene_shard_bounds: the smallest i with pt_ptr[i] * world >= E * r (64-bit integers; equal
    to partition_points' float searchsorted for every E * world < 2^53)."""
    ptl = pt_ptr.to(torch.int64)
    dev = ptl.device
    n = ptl.shape[0] - 1
    r = torch.arange(1, world, dtype=torch.int64, device=dev)
    inner = torch.searchsorted(ptl * world, ptl[-1] * r)
    edge = torch.tensor([0, n], dtype=torch.int64).to(dev)
    return torch.cat([edge[:1], inner, edge[1:]]).to(torch.int32)


def _ranges_torch(cam_ptr, pt_ptr, cam, pt, bounds, rank, c0, c1):
    """gasfm_scene_shard_cam_range + _stats + the scan (``_native.scene_shard_ranges``)."""
    dev = cam_ptr.device
    m, n = cam_ptr.shape[0] - 1, pt_ptr.shape[0] - 1
    i64 = dict(dtype=torch.int64, device=dev)
    b = bounds.to(torch.int64)
    p0, p1 = b[rank], b[rank + 1]
    # cam-major with points ascending: camera c's edges with pt >= p are those with key >= c * n + p
    key = cam.to(torch.int64) * n + pt.to(torch.int64)
    cams = torch.arange(m, **i64)
    lo = torch.searchsorted(key, cams * n + p0)
    count = torch.searchsorted(key, cams * n + p1) - lo
    lcam_ptr = torch.cat([torch.zeros(1, **i64), torch.cumsum(count, 0)])
    cl = cam_ptr.to(torch.int64)
    ptl = pt_ptr.to(torch.int64)
    valid_v = (cl[1:] - cl[:-1]) >= MIN_N_POINTS_PER_VIEW
    own_v = valid_v[c0:c1]
    pts = torch.arange(n, **i64)
    mine = (pts >= p0) & (pts < p1)
    valid_p = (ptl[1:] - ptl[:-1]) >= MIN_N_VIEWS_PER_POINT

    def first_invalid(bad, ids, length):  # smallest id among the bad ones, ``length`` when there is none
        length = torch.as_tensor(length, **i64).view(1)
        return torch.cat([torch.where(bad, ids, length), length]).min()

    stats = torch.stack([
        p0, p1, ptl.gather(0, p1.view(1))[0] - ptl.gather(0, p0.view(1))[0],
        valid_v.sum(), first_invalid(~valid_v, cams, m),
        own_v.sum(), first_invalid(~own_v, torch.arange(c1 - c0, **i64), c1 - c0),
        (valid_p & mine).sum(), first_invalid(mine & ~valid_p, pts - p0, p1 - p0)])
    return {"lo": lo.to(torch.int32), "count": count.to(torch.int32), "lcam_ptr": lcam_ptr.to(torch.int32),
            "pts_per_cam": count, "valid_view": valid_v, "stats": stats}


def _emit_torch(r, pt, p0, E_loc, sources):
    """gasfm_scene_shard_emit (``_native.scene_shard_emit``)."""
    dev = pt.device
    m = r["count"].shape[0]
    c = torch.repeat_interleave(torch.arange(m, dtype=torch.int64, device=dev), r["count"].to(torch.int64),
                                output_size=E_loc)
    j = torch.arange(E_loc, dtype=torch.int64, device=dev)
    sel = r["lo"].to(torch.int64)[c] + j - r["lcam_ptr"].to(torch.int64)[c]
    q = pt.to(torch.int64)[sel] - p0
    return (sel, torch.stack([c, q]), c.to(torch.int32), q.to(torch.int32),
            [s.index_select(0, sel).contiguous() for s in sources])


def _point_csr_torch(r, pt_ptr, perm, cam, p0, p1, E_loc):
    """gasfm_scene_shard_point_csr (``_native.scene_shard_point_csr``)."""
    dev = cam.device
    ptl = pt_ptr.to(torch.int64)
    base = ptl[p0]
    lpt_ptr = (ptl[p0:p1 + 1] - base).to(torch.int32)
    cpp = ptl[p0 + 1:p1 + 1] - ptl[p0:p1]
    k = torch.arange(E_loc, dtype=torch.int64, device=dev)
    g = base + k if perm is None else perm.to(torch.int64)[base + k]
    c = cam.to(torch.int64)[g]
    ids = r["lcam_ptr"].to(torch.int64)[c] + g - r["lo"].to(torch.int64)[c]
    lpos = torch.empty(E_loc, dtype=torch.int32, device=dev)
    lpos[ids] = k.to(torch.int32)
    return lpt_ptr, cpp, cpp >= MIN_N_VIEWS_PER_POINT, ids.to(torch.int32), lpos


# ------------------------------------------------------------------ the shard
def _star(src, src_rows, max_piece, tag, ident, all_partial=False):
    """scene_device._star_source_plan as AttnPlan.from_targets builds the plan on the host: without
    any source it takes its unsorted branch, whose perm is the (empty) order instead of None."""
    plan = _star_source_plan(src, src_rows, max_piece, tag, ident=ident, all_partial=all_partial)
    if src.shape[0] == 0:
        plan.perm = src.to(torch.int32)
        plan.pos = plan.perm.clone() if src_rows == 0 else None
    return plan


def shard_scene_on_device(data, rank, world, inputs=None, cameras=False, emulate=False, max_piece=None,
                          point_bounds=None, kernels=None):
    """(network shard, loss shard) of a scene for this rank, as ``dist_train.shard_device_scene``
    returns them, without moving the scene's edges to the host (module docstring).

    data: the clean scene (loss, errors); inputs: the network's scene with the same edges, default
    ``data``.  cameras / emulate / max_piece / point_bounds: as ``distributed.shard_scene``.  kernels:
    None = the HIP kernels for CUDA tensors and the torch restatement for CPU tensors; False = the
    restatement on any device."""
    inputs = data if inputs is None else inputs
    idx = data.x.indices
    if inputs.x.indices.shape != idx.shape:
        raise ValueError("shard_scene_on_device: the network's input scene has other edges than the loss's")
    if not 0 <= rank < world:
        raise ValueError(f"shard_scene_on_device: rank {rank} of {world}")
    dev = data.x.values.device
    m, n = int(data.x.shape[0]), int(data.x.shape[1])
    E = int(idx.shape[1])
    use_kernels = dev.type == "cuda" if kernels is None else bool(kernels)
    cam_ptr, pt_ptr, perm = _csr_arrays(data)
    cam, pt = idx[0], idx[1]
    if point_bounds is None:
        bounds = _native.scene_shard_bounds(pt_ptr, world) if use_kernels else _bounds_torch(pt_ptr, world)
    else:
        hb = np.asarray(point_bounds, dtype=np.int64)
        if hb.shape != (world + 1,) or hb[0] != 0 or hb[-1] != n or np.any(np.diff(hb) < 0):
            raise ValueError(f"point_bounds must be {world + 1} non-decreasing boundaries from 0 to {n}")
        bounds = torch.from_numpy(hb.astype(np.int32)).to(dev)
    cams = None
    c0 = c1 = 0
    if cameras:
        c0, c1, chunk = camera_rows(m, world, rank)
        cams = (c0, c1, chunk, m)
    ranges, emit, point_csr = ((_native.scene_shard_ranges, _native.scene_shard_emit, _native.scene_shard_point_csr)
                               if use_kernels else
                               (lambda cp, pp, p, b, r, a0, a1: _ranges_torch(cp, pp, cam, p, b, r, a0, a1),
                                _emit_torch, _point_csr_torch))
    r = ranges(cam_ptr, pt_ptr, pt, bounds, rank, c0, c1)
    p0, p1, E_loc, n_vv, z_v, n_own, z_own, n_vp, z_p = (int(v) for v in r["stats"].tolist())  # host read 1
    n_loc = p1 - p0

    vals_loss = data.x.values.detach().float().contiguous()
    vals_net = vals_loss if inputs is data else inputs.x.values.detach().float().contiguous()
    xy = _pixel_measurements(data)
    sources = [vals_loss, xy] if inputs is data else [vals_loss, xy, vals_net]
    sel, indices, cam32, pt32, rows = emit(r, pt, p0, E_loc, sources)
    lpt_ptr, cam_per_pts, valid_p, lperm, lpos = point_csr(r, pt_ptr, perm, cam, p0, p1, E_loc)

    mp_cam = camera_max_piece(E_loc) if max_piece is None else max_piece
    mp_pt = DEFAULT_MAX_PIECE if max_piece is None else max_piece
    z = torch.zeros(4, dtype=torch.int64, device=dev)
    ln_c = r["count"].to(torch.int64)
    ln_p = (lpt_ptr[1:] - lpt_ptr[:-1]).to(torch.int64)
    # the stable grouping of a point-sorted edge list is the identity
    is_sorted = (lperm == torch.arange(E_loc, dtype=torch.int32, device=dev)).all().to(torch.int64).view(1)
    counts = torch.cat([is_sorted, _piece_stats(ln_c, mp_cam)[3] if m else z,
                        _piece_stats(ln_p, mp_pt)[3] if n_loc else z]).tolist()  # host read 2
    # AttnPlan.from_targets takes its sorted branch (perm None) only for a non-empty sorted list
    no_perm = bool(counts[0]) and E_loc > 0

    p2v = AxialAggregationGraphWrapper(m, n_loc, 1, indices, build_plan=False)
    p2s = AxialAggregationGraphWrapper(m, n_loc, 0, indices, build_plan=False)
    lcam_ptr = r["lcam_ptr"]
    p2v.plan = _plan(lcam_ptr, None, None, m, E_loc, E_loc, mp_cam, "proj2view", counts=counts[1:5])
    p2s.plan = _plan(lpt_ptr, None if no_perm else lperm, None if no_perm else lpos, n_loc, E_loc, E_loc, mp_pt,
                     "proj2scenepoint", counts=counts[5:9])
    partial = {"proj2view": _plan(lcam_ptr, None, None, m, E_loc, E_loc, mp_cam, "proj2view_partial",
                                  all_partial=True, counts=counts[1:5])}
    if E_loc == 0:  # from_targets' unsorted branch again: the (empty) order as perm, its inverse as pos
        for plan in (p2v.plan, partial["proj2view"]):
            plan.perm, plan.pos = lperm, lpos

    # view validity is a GLOBAL property (>= 8 points over all ranks): the view2global graph is replicated
    vv = torch.nonzero_static(r["valid_view"], size=n_vv).view(-1)
    vp = torch.nonzero_static(valid_p, size=n_vp).view(-1)
    v2g = AxialAggregationGraphWrapper(m, 1, 0, torch.stack([vv, torch.zeros_like(vv)]), build_plan=False)
    s2g = AxialAggregationGraphWrapper(1, n_loc, 1, torch.stack([torch.zeros_like(vp), vp]), build_plan=False)
    mp_g = min(256, max(16, -(-n_vp // 4096)))
    s2g.plan = _star(vp, n_loc, mp_g, "scenepoint2global", z_p >= n_vp)
    partial["scenepoint2global"] = _star(vp, n_loc, mp_g, "scenepoint2global_partial", z_p >= n_vp, all_partial=True)
    if cameras:
        own = torch.nonzero_static(r["valid_view"][c0:c1], size=n_own).view(-1)
        v2g.plan = _star(own, c1 - c0, 8, "view2global", z_own >= n_own)
        partial["view2global"] = _star(own, c1 - c0, 8, "view2global_partial", z_own >= n_own, all_partial=True)
    else:
        v2g.plan = _star(vv, m, 8, "view2global", z_v >= n_vv)

    net = SceneData.__new__(SceneData)
    net.scene_name = f"shard{rank}"
    net.calibrated = True
    net.y = None
    net._M = None
    net.Ns = None
    net.device = dev
    shape = (m, n_loc, 2)
    cpp, ppc = cam_per_pts.unsqueeze(1), r["pts_per_cam"].unsqueeze(1)
    net.x = SparseMat(rows[0] if inputs is data else rows[2], indices, cpp, ppc, shape)
    net.graph_wrappers = {"proj2view": p2v, "proj2scenepoint": p2s, "view2global": v2g, "scenepoint2global": s2g}
    net.partial_plans = partial
    if cameras:
        net.camera_slice = slice(c0, c1)
    net.point_slice = slice(p0, p1)
    net.n_global = n
    net.n_edges_global = E
    net.shard = ShardContext(rank, world, cams=cams, emulate=emulate)
    net.edge_ids = sel  # the local edges' ids in the whole scene
    # the loss's int32 edge indices (loss._edge_tensors' cache, keyed on the index tensor)
    p2v.plan._caches = {"esfm_edges": ((indices.data_ptr(), indices._version, tuple(indices.shape)), (cam32, pt32))}

    loss = copy.copy(net)
    loss.x = SparseMat(rows[0], indices, cpp, ppc, shape)
    loss.xy = rows[1]
    loss.Ns = data.Ns
    loss.Ns_invT = getattr(data, "Ns_invT", None)
    return net, loss
