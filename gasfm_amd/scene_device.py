"""Device-side scene graph construction.

The reference rebuilds every training sample's graph on the CPU, in DataLoader workers, from
the dense measurement matrix: ``get_M_valid_points`` / ``M2sparse`` / ``normalize_M``
(utils/dataset_utils.py:86-156, utils/geo_utils.py:689-703) and the four star graphs of
``SceneData.create_axial_aggregation_graphs`` (datasets/SceneData.py:153-239).  When M is
already in HBM, ``scene_from_dense_device`` builds the same ``SceneData`` on the GPU:

  edges, values, counts, point CSR   gasfm_scene_mask / _emit / _point_csr (csrc/scene_build.hip)
  work items of the attention plans  ``plan_work_device``: gasfm_plan_work (host_graph.cpp)
                                     restated over segment lengths with torch device ops
                                     (O(segments) glue, bit-identical items / slots / combines)

Everything the model reads is bit-identical to the host builder (``SceneData(M, Ns, ...)``):
edge order, indices, counts, plans; values agree to fp32 rounding of the 2x3 normalisation.
Host syncs: the edge count, the item counts of the four plans, and the small combine lists.

Per-sample transforms before the build (§8(f) rank 3), with M staying on the device:
``sample_data_device`` (SceneData.sample_data) and ``apply_rotational_homography_aug_device``
(SceneData.apply_rotational_homography_aug, image points through gasfm_scene_homography); their
random draws come from the same numpy / torch CPU generators, in the reference's order.

Depth targets (SceneData's ``store_depth_targets`` / ``depths``) ride along per edge, float32 [E] in
the order of ``data.x.indices``: gasfm_depth_targets at the build, gasfm_depth_gather through
sampling, gasfm_depth_rescale through the augmentation (csrc/depth_targets.hip).
"""
import math

import numpy as np
import torch

from . import _native
from .attention import DEFAULT_MAX_PIECE, L1_THRESHOLD, AttnPlan
from .scene import (MIN_N_POINTS_PER_VIEW, MIN_N_VIEWS_PER_POINT, AxialAggregationGraphWrapper, SceneData,
                    SparseMat)


def _piece_stats(ln, max_piece):
    """Per-segment piece counts of plan_work_device and the four host scalars it needs, on the device:
    (pieces, split, sp, scalars = [n_items, n_split, split pieces, level-1 combine entries])."""
    split = ln > max_piece
    pieces = torch.where(split, (ln + max_piece - 1) // max_piece, torch.ones_like(ln))
    sp = torch.where(split, pieces, torch.zeros_like(pieces))
    scalars = torch.stack([pieces.sum(), split.sum(), sp.sum(), _l1_groups(sp).sum()])
    return pieces, split, sp, scalars


def _l1_groups(cnt):
    """Level-1 entries of a combine over cnt slots (attention._two_level: groups of ceil(sqrt(cnt))
    when cnt > L1_THRESHOLD, else none); cnt = 0 gives 0."""
    g = torch.ceil(torch.sqrt(cnt.to(torch.float64))).to(torch.int64).clamp_(min=1)
    return torch.where(cnt > L1_THRESHOLD, (cnt + g - 1) // g, torch.zeros_like(cnt))


def _piece_counts_host(lengths, max_piece):
    """The scalars of _piece_stats for segment lengths known on the host (the one-segment global plans)."""
    n_items = n_split = n_sp = n_l1 = 0
    for ln in lengths:
        if ln > max_piece:
            pc = -(-ln // max_piece)
            n_items += pc
            n_split += 1
            n_sp += pc
            if pc > L1_THRESHOLD:
                g = int(math.ceil(math.sqrt(pc)))
                n_l1 += -(-pc // g)
        else:
            n_items += 1
    return [n_items, n_split, n_sp, n_l1]


def plan_work_device(seg_ptr, max_piece, all_partial=False, counts=None):
    """gasfm_plan_work (host_graph.cpp) on device tensors, with attention._two_level's split of the
    long combines: (items [I, 4], combine [K, 4], combine_l1 [K1, 4] or None, n_slots).

    Segment s of length len > max_piece splits into ceil(len / max_piece) pieces whose lengths
    differ by at most one (the first len % pieces are one longer); pieces take consecutive
    partial slots in segment order, from N when ``all_partial`` (then unsplit segments write
    slot s), else from 0 (unsplit: slot -1).  counts: the 4 host scalars of _piece_stats when the
    caller read them already (one host read per scene build instead of one per plan)."""
    ptr = seg_ptr.to(torch.int64)
    dev = ptr.device
    N = ptr.shape[0] - 1
    ln = ptr[1:] - ptr[:-1]
    pieces, split, sp, scalars = _piece_stats(ln, max_piece)
    if counts is None:
        counts = scalars.tolist() if N else [0, 0, 0, 0]
    n_items, n_split, n_sp, n_l1 = (int(v) for v in counts)
    seg = torch.repeat_interleave(torch.arange(N, device=dev), pieces, output_size=n_items)
    first = torch.cumsum(pieces, 0) - pieces
    p = torch.arange(n_items, device=dev) - first[seg]
    base, rem = ln // pieces, ln % pieces
    begin = ptr[:-1][seg] + p * base[seg] + torch.minimum(p, rem[seg])
    end = begin + base[seg] + (p < rem[seg]).to(torch.int64)
    s0 = N if all_partial else 0
    slot_first = s0 + torch.cumsum(sp, 0) - sp
    unsplit = seg if all_partial else torch.full_like(seg, -1)
    slot = torch.where(split[seg], slot_first[seg] + p, unsplit)
    n_slots = s0 + n_sp
    cs = torch.nonzero_static(split, size=n_split).view(-1)
    cnt, b = pieces[cs], slot_first[cs]
    items = torch.stack([seg, begin, end, slot], 1).to(torch.int32).contiguous()
    if n_l1 == 0:
        combine = torch.stack([cs, b, cnt, torch.ones_like(cs)], 1).to(torch.int32).contiguous()
        return items, combine, None, n_slots
    # two levels (attention._two_level): an entry over cnt > L1_THRESHOLD slots becomes ng level-1
    # entries over groups of g = ceil(sqrt(cnt)) slots (partial rows n_slots + k, in entry order)
    # and a level-2 entry over those rows
    ng = _l1_groups(cnt)
    g = torch.ceil(torch.sqrt(cnt.to(torch.float64))).to(torch.int64)
    first_l1 = n_slots + torch.cumsum(ng, 0) - ng
    e = torch.repeat_interleave(torch.arange(cs.shape[0], device=dev), ng, output_size=n_l1)
    k = torch.arange(n_l1, device=dev) - (torch.cumsum(ng, 0) - ng)[e]
    lo = b[e] + k * g[e]
    l1 = torch.stack([first_l1[e] + k, lo, torch.minimum(g[e], b[e] + cnt[e] - lo), torch.ones_like(e)], 1)
    big = ng > 0
    combine = torch.stack([cs, torch.where(big, first_l1, b), torch.where(big, ng, cnt), torch.ones_like(cs)], 1)
    return items, combine.to(torch.int32).contiguous(), l1.to(torch.int32).contiguous(), n_slots


def _plan(seg_ptr, perm, pos, num_targets, num_edges, src_rows, max_piece, tag, all_partial=False, counts=None):
    items, comb, comb_l1, n_slots = plan_work_device(seg_ptr, max_piece, all_partial, counts)
    plan = AttnPlan(seg_ptr, perm, items, comb, n_slots, num_targets, num_edges, src_rows, all_partial, max_piece,
                    pos=pos, combine_l1=comb_l1)
    plan.tag = tag
    return plan


def _star_source_plan(src, src_rows, max_piece, tag, ident=None, all_partial=False):
    """One-target plan over source rows ``src`` (the global graphs): perm = src unless identity
    (ident: that test's answer when the caller read it already).  all_partial: the exchange form of
    a point shard (distributed.shard_scene's partial plans)."""
    k = int(src.shape[0])
    dev = src.device
    seg_ptr = torch.tensor([0, k], dtype=torch.int32, device=dev)
    if ident is None:
        ident = k == 0 or bool(torch.equal(src, torch.arange(k, device=dev, dtype=src.dtype)))
    perm = None if ident else src.to(torch.int32).contiguous()
    return _plan(seg_ptr, perm, None, 1, k, src_rows, max_piece, tag, all_partial=all_partial,
                 counts=_piece_counts_host([k], max_piece))


def graph_wrappers_device(b, m, n, max_piece=None):
    """The four wrappers of build_graph_wrappers (scene.py) from ``_native.scene_build`` output.
    Every host scalar the four plans need (piece counts, valid view / point counts, sortedness)
    crosses to the host in ONE read."""
    mp = DEFAULT_MAX_PIECE if max_piece is None else max_piece
    cam, pt = b["cam"], b["pt"]
    E = int(cam.shape[0])
    indices = torch.stack([cam, pt])
    p2v = AxialAggregationGraphWrapper(m, n, 1, indices, build_plan=False)
    p2s = AxialAggregationGraphWrapper(m, n, 0, indices, build_plan=False)
    pts_per_cam = b["cam_ptr"][1:] - b["cam_ptr"][:-1]
    valid_v = pts_per_cam >= MIN_N_POINTS_PER_VIEW
    valid_p = b["pt_count"] >= MIN_N_VIEWS_PER_POINT
    ln_c = (b["cam_ptr"][1:] - b["cam_ptr"][:-1]).to(torch.int64)
    ln_p = (b["pt_ptr"][1:] - b["pt_ptr"][:-1]).to(torch.int64)
    sorted_pt = (pt[1:] >= pt[:-1]).all() if E > 1 else torch.ones((), dtype=torch.bool, device=cam.device)
    z = torch.zeros(4, dtype=torch.int64, device=cam.device)
    # valid ids == arange(k) <=> the valid flags are a prefix of ones
    vals = torch.cat([torch.stack([sorted_pt.to(torch.int64), valid_v.sum(), valid_p.sum(),
                                   (valid_v.to(torch.int64).cumprod(0).sum() if m else z[0]),
                                   (valid_p.to(torch.int64).cumprod(0).sum() if n else z[0])]),
                      _piece_stats(ln_c, mp)[3] if m else z, _piece_stats(ln_p, mp)[3] if n else z]).tolist()
    is_sorted, n_vv, n_vp, pre_v, pre_p = (int(v) for v in vals[:5])
    # camera direction: edges are cam-major already (seg_ptr = cam_ptr, no permutation)
    p2v.plan = _plan(b["cam_ptr"], None, None, m, E, E, mp, "proj2view", counts=vals[5:9])
    # point direction: the stable point CSR; a point-sorted edge list needs no permutation
    # (AttnPlan.from_targets takes its sorted branch then)
    perm, pos = (None, None) if is_sorted else (b["perm"], b["pos"])
    p2s.plan = _plan(b["pt_ptr"], perm, pos, n, E, E, mp, "proj2scenepoint", counts=vals[9:13])
    vv = torch.nonzero_static(valid_v, size=n_vv).view(-1)
    vp = torch.nonzero_static(valid_p, size=n_vp).view(-1)
    v2g = AxialAggregationGraphWrapper(m, 1, 0, torch.stack([vv, torch.zeros_like(vv)]), build_plan=False)
    s2g = AxialAggregationGraphWrapper(1, n, 1, torch.stack([torch.zeros_like(vp), vp]), build_plan=False)
    v2g.plan = _star_source_plan(vv, m, 8, "view2global", ident=pre_v == n_vv)
    s2g.plan = _star_source_plan(vp, n, min(256, max(16, -(-n_vp // 4096))), "scenepoint2global",
                                 ident=pre_p == n_vp)
    return {"proj2view": p2v, "proj2scenepoint": p2s, "view2global": v2g, "scenepoint2global": s2g}


# ------------------------------------------------------------------ per-edge depth targets
# The reference's SceneData.depths is a dense [m, n] matrix (SceneData.py:57-134); here a scene carries
# depths [E] float32 in its edge order (csrc/depth_targets.hip).  Each of the three kernels has a
# restatement in torch ops beside it: what CPU tensors take, the CPU suite runs and the GPU tests
# compare the kernels with.
def depth_targets_torch(a, X, cam, pt):
    """gasfm_depth_targets in torch ops: (d [E] = a[cam] . X[pt], bad [1] int32)."""
    d = (a[cam] * X[pt]).sum(1)
    return d, (~(torch.isfinite(d) & (d > 0))).sum().to(torch.int32).view(1)


def depth_gather_torch(pcam_ptr, ppt, pd, view_idx, keep, cam, pt):
    """gasfm_depth_gather in torch ops: the parent's edges are sorted by (camera, point), so one
    searchsorted over that key finds every sampled edge; (d [E], missing [1] int32)."""
    Ep = ppt.shape[0]
    if cam.shape[0] == 0 or Ep == 0:
        return (torch.full((cam.shape[0],), float("nan"), dtype=torch.float32, device=cam.device),
                torch.full((1,), cam.shape[0], dtype=torch.int32, device=cam.device))
    ptr = pcam_ptr.to(torch.int64)
    stride = int(max(int(ppt.max()), int(keep.max()) if keep.numel() else 0)) + 1
    pcam = torch.repeat_interleave(torch.arange(ptr.shape[0] - 1, device=ppt.device), ptr[1:] - ptr[:-1],
                                   output_size=Ep)
    key = pcam * stride + ppt.to(torch.int64)
    want = view_idx[cam] * stride + keep[pt]
    pos = torch.searchsorted(key, want).clamp_(max=Ep - 1)
    found = key[pos] == want
    d = torch.where(found, pd[pos], torch.full_like(pd[pos], float("nan")))
    return d, (~found).sum().to(torch.int32).view(1)


def depth_rescale_torch(d, cam, pt, M, Ns, R):
    """gasfm_depth_rescale in torch ops: d / z_old * z_new per edge, in the kernel's order."""
    u, v = M[2 * cam, pt], M[2 * cam + 1, pt]
    N, r = Ns[cam], R[cam]
    q = [N[:, i, 0] * u + N[:, i, 1] * v + N[:, i, 2] for i in range(3)]
    z_new = r[:, 2, 0] * q[0] + r[:, 2, 1] * q[1] + r[:, 2, 2] * q[2]
    return d / q[2] * z_new


def _kernels(t):
    return t.device.type == "cuda"


def depth_rows(Ns_c, y_c):
    """a [m, 4]: the third rows of Ns[c] @ y[c] in fp32 on the host, as the reference computes
    ``K_inv @ self.y`` (SceneData.py:99); m-sized, like the augmentation's 3x3 products."""
    return (Ns_c.float().cpu() @ y_c.float().cpu())[:, 2, :].contiguous()


def depth_targets_from_points(a, X, cam, pt, scene_name="scene"):
    """d [E] = a[cam] . X[pt] (float32, on cam's device).  Raises ValueError when an edge's depth is
    not finite or not > 0, the reference's asserts at SceneData.py:104 and :132: one host read."""
    dev = cam.device
    a, X = a.to(dev, torch.float32).contiguous(), X.to(dev, torch.float32).contiguous()
    d, bad = (_native.depth_targets if _kernels(cam) else depth_targets_torch)(a, X, cam, pt)
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"{scene_name}: {n_bad} of {cam.shape[0]} depth targets are not finite or not > 0 "
                         "(a point behind a camera, or not triangulated)")
    return d


def triangulate_scene_device(M, Ns, y, b):
    """``n_view_triangulation(y, M, Ns)`` cast to float32 (SceneData.py:70-74) from the scene's edges:
    X [n, 4], last coordinate 1, NaN rows for points in < 2 views (no edge reads them).  gasfm_ba_dlt
    in fp64 on the inputs the reference's DLT sees: the cameras Ns @ y as an fp32 host product and the
    normalised observations rounded to fp32 (normalize_points_cams stores both in float32 arrays)."""
    from . import ba
    dev = M.device
    m, n = M.shape[0] // 2, M.shape[1]
    cam, pt = b["cam"], b["pt"]
    obs = torch.stack([M[2 * cam, pt], M[2 * cam + 1, pt]], 1).to(ba.F64)
    nP = (Ns.float().cpu() @ y.float().cpu()).to(dev, ba.F64).contiguous()
    nx = ba.normalized_observations(Ns.to(dev, ba.F64), cam, obs).float().to(ba.F64).contiguous()
    X = torch.empty((n, 4), dtype=ba.F64, device=dev)
    _native.check(_native.lib().gasfm_ba_dlt(n, _native._p(b["pt_ptr"]), _native._p(b["perm"]),
                                             _native._p(cam.to(torch.int32).contiguous()), _native._p(nP),
                                             _native._p(nx), _native._p(X), _native._stream(X)), "gasfm_ba_dlt")
    return X.float()


def _scene_depths(M, Ns, y, b, calibrated, scene_name, depths):
    """data.depths of scene_from_dense_device(store_depth_targets=True): adopted, or triangulated."""
    cam, pt = b["cam"], b["pt"]
    E = cam.shape[0]
    if depths is not None:
        if depths.dim() == 2:  # the reference's dense form: gathered once, per edge from here on
            if tuple(depths.shape) != (M.shape[0] // 2, M.shape[1]):
                raise ValueError(f"depths must be [m, n] or [E], got {tuple(depths.shape)}")
            return depths.to(M.device)[cam, pt].float().contiguous()
        if tuple(depths.shape) != (E,):
            raise ValueError(f"per-edge depths have {tuple(depths.shape)} entries for {E} edges")
        return depths.to(M.device, torch.float32).contiguous()
    if not calibrated:
        raise NotImplementedError("depth targets of an uncalibrated scene (as the reference, SceneData.py:66-68)")
    if y is None:
        raise ValueError("store_depth_targets needs the ground-truth cameras Ps_gt")
    X = triangulate_scene_device(M, Ns, y, b)
    return depth_targets_from_points(depth_rows(Ns, y), X, cam, pt, scene_name)


def _per_edge_depths(data, dev):
    """(cam_ptr int32 [m + 1], pt [E], depths [E] float32) on ``dev`` of a scene that carries targets,
    per edge or as the reference's dense [m, n] matrix (gathered at the edges, as loss.py does); kept
    on the scene, so a full scene pays for it once and not once per sample."""
    dep = data.depths
    if dep is None:
        raise ValueError("the scene stores depth targets but carries no depths")
    cache = data.__dict__.get("_gasfm_depth_edges")
    if cache is not None and cache[0] is dep and cache[1] == dep._version and cache[2][0].device == dev:
        return cache[2]
    idx = data.x.indices.to(dev)
    sb = data.__dict__.get("_scene_build")
    if sb is not None and sb["cam_ptr"].device == dev:
        cam_ptr = sb["cam_ptr"]
    else:
        cam_ptr = torch.zeros(data.x.shape[0] + 1, dtype=torch.int32, device=dev)
        cam_ptr[1:] = torch.cumsum(data.x.pts_per_cam.view(-1).to(dev), 0)
    if dep.dim() == 2:
        d = dep.to(dev)[idx[0], idx[1]].float().contiguous()
    elif tuple(dep.shape) == (idx.shape[1],):
        d = dep.to(dev, torch.float32).contiguous()
    else:
        raise ValueError(f"depths must be [m, n] or [E], got {tuple(dep.shape)} for {idx.shape[1]} edges")
    out = (cam_ptr, idx[1].contiguous(), d)
    try:
        data._gasfm_depth_edges = (dep, dep._version, out)
    except AttributeError:
        pass
    return out


class _DepthSource:
    """What the gather of a sampled scene needs from its parent: the parent's cam_ptr / pt / depths
    per edge, the sampled views' parent cameras (in M's row order) and the kept parent points; n_edges:
    the sampled M's edge count, a device scalar."""

    def __init__(self, cam_ptr, pt, depths, view_idx, keep, n_edges):
        self.cam_ptr, self.pt, self.depths, self.view_idx, self.keep, self.n_edges = \
            cam_ptr, pt, depths, view_idx, keep, n_edges

    def gather(self, cam, pt):
        """(depths of the edges (cam, pt) of the sampled scene, missing count [1])."""
        fn = _native.depth_gather if _kernels(cam) else depth_gather_torch
        return fn(self.cam_ptr, self.pt, self.depths, self.view_idx, self.keep, cam.contiguous(), pt.contiguous())


def _missing_error(n_missing, scene_name):
    return ValueError(f"{scene_name}: {n_missing} sampled edges have no edge in the parent scene")


def scene_from_dense_device(M, Ns, Ps_gt=None, scene_name="scene", calibrated=True, max_piece=None,
                            store_depth_targets=False, depths=None):
    """``SceneData(M, Ns, Ps_gt, scene_name)`` built on M's device (a CUDA tensor).

    store_depth_targets (SceneData.py:57-134): ``data.depths`` becomes the per-edge float32 [E] depth
    targets in the order of ``data.x.indices`` -- ``depths`` when given ([E], or the reference's dense
    [m, n], gathered here), else (K_inv y X)[2] on the points triangulated from Ps_gt and M, which
    raises ValueError for a depth that is not finite or not > 0 and NotImplementedError for an
    uncalibrated scene.  Without the flag ``data.depths`` is None, as in the reference."""
    m, n = M.shape[0] // 2, M.shape[1]
    M = M.contiguous()
    b = _native.scene_build(M, Ns)
    cam_per_pts = b["pt_count"].to(torch.int64).unsqueeze(1)
    pts_per_cam = (b["cam_ptr"][1:] - b["cam_ptr"][:-1]).to(torch.int64).unsqueeze(1)
    self = SceneData.__new__(SceneData)
    self.scene_name = scene_name
    self.calibrated = calibrated
    self.y = Ps_gt
    self._M = M
    self.Ns = Ns
    self.device = M.device
    self.x = SparseMat(b["values"], torch.stack([b["cam"], b["pt"]]), cam_per_pts, pts_per_cam, (m, n, 2))
    # the graph wrappers are built on first use (SceneData.__getattr__); batch.SceneBatch reads these
    self._scene_build = {k: b[k] for k in ("cam_ptr", "pt_ptr", "perm", "pos", "pt")}
    self._lazy_graph = lambda: graph_wrappers_device(b, m, n, max_piece)
    self.store_depth_targets = bool(store_depth_targets)
    self.depths = _scene_depths(M, Ns, Ps_gt, b, calibrated, scene_name, depths) if store_depth_targets else None
    return self


def create_scene_data_device(conf, M, Ns, Ps_gt, scene_name, calibrated=None, max_piece=None):
    """The SceneData part of the reference's ``create_scene_data`` (SceneData.py:267-303) for raw data
    already on the device: ``model.depth_head.enabled`` switches the depth targets on, and
    ``dataset.calibrated`` is read unless overridden."""
    store_depth_targets = conf.get_bool("model.depth_head.enabled", default=False)
    calibrated = calibrated if calibrated is not None else conf.get_bool("dataset.calibrated")
    return scene_from_dense_device(M, Ns, Ps_gt, scene_name, calibrated=calibrated, max_piece=max_piece,
                                   store_depth_targets=store_depth_targets)


# ------------------------------------------------------------------ per-sample transforms on the device
def _dense_M(data):
    M = getattr(data, "M", None)
    if M is None:
        M = getattr(data, "_M", None)
    if M is None:
        raise ValueError("the scene carries no dense measurement matrix M")
    return M


def sample_indices(N, num_samples, adjacent):
    """dataset_utils.sample_indices (utils/dataset_utils.py:25-40), same numpy RNG calls."""
    if num_samples == 1:
        return np.arange(N)
    if num_samples < 1:
        num_samples = int(np.ceil(num_samples * N))
    num_samples = max(2, num_samples)
    if num_samples >= N:
        return np.arange(N)
    if adjacent:
        start = np.random.randint(0, N - num_samples + 1)
        return np.arange(start, start + num_samples)
    return np.random.choice(N, num_samples, replace=False)


class DenseScene:
    """A sampled scene before its graph is built (``sample_data_device(..., build=False)``): the
    dense M with Ns / y, enough for ``apply_rotational_homography_aug_device`` (which builds the
    graph once, instead of once per transform)."""

    def __init__(self, M, Ns, y, scene_name, calibrated=True, host_Ns_y=None, depth_src=None):
        self._M, self.Ns, self.y, self.scene_name, self.calibrated = M, Ns, y, scene_name, calibrated
        self.device = M.device
        self._host_Ns_y = host_Ns_y  # fp32 CPU copies of (Ns, y): the augmentation's 3x3 products
        # depth targets: no edge list exists yet, so the scene carries what the gather needs from its
        # parent (_DepthSource) and the transform that builds the graph gathers them
        self.store_depth_targets = depth_src is not None
        self.depths = None
        self._depth_src = depth_src


def sample_data_device(data, num_views, consecutive_views=True, max_piece=None, build=True):
    """SceneData.sample_data (datasets/SceneData.py:306-353) with M on the device: the view subset's
    rows, the points still seen in >= 2 of those views (gasfm_scene_mask's counts), then the
    device graph build (``build=False``: a DenseScene for a following transform that builds it).
    The view choice draws from numpy's global RNG exactly as the reference.

    A scene with ``store_depth_targets`` hands its targets on per edge (gasfm_depth_gather; a host
    scene's dense [m, n] ``depths`` is gathered to its edges once).  The targets follow M's rows, which
    are in ascending view order; the reference indexes its dense matrix with the views as drawn, which
    is the same for consecutive views and pairs other rows than M's for an unsorted random choice."""
    M = _dense_M(data)
    idx = sample_indices(len(data.y), num_views, adjacent=consecutive_views)
    m_idx = np.sort(np.concatenate((2 * idx, 2 * idx + 1)))
    dev = M.device
    ti = torch.from_numpy(idx).to(dev)
    y, Ns = data.y.to(dev)[ti], data.Ns.to(dev)[ti]
    Ms = M.index_select(0, torch.from_numpy(m_idx).to(dev)).contiguous()
    _, _, pt_count, _ = _native.scene_mask(Ms)
    keep = torch.nonzero(pt_count > 0).view(-1)  # get_M_valid_points(M).any(dim=0)
    Ms = Ms.index_select(1, keep).contiguous()
    src = None
    if getattr(data, "store_depth_targets", False):
        views = torch.from_numpy(np.sort(idx).astype(np.int64)).to(dev)
        src = _DepthSource(*_per_edge_depths(data, dev), views, keep, pt_count.sum())
    if not build:
        # host copies of the full scene's Ns / y, read once per scene (not once per sample)
        hc = getattr(data, "_gasfm_host_Ns_y", None)
        if hc is None:
            hc = (data.Ns.float().cpu(), data.y.float().cpu())
            try:
                data._gasfm_host_Ns_y = hc
            except AttributeError:
                pass
        ih = torch.from_numpy(idx)
        return DenseScene(Ms, Ns.contiguous(), y, data.scene_name, getattr(data, "calibrated", True),
                          host_Ns_y=(hc[0][ih], hc[1][ih]), depth_src=src)
    out = scene_from_dense_device(Ms, Ns.contiguous(), y, data.scene_name,
                                  calibrated=getattr(data, "calibrated", True), max_piece=max_piece)
    return _carry_depths(out, data, src, None, None, None)


def _carry_depths(out, data, src, M_old, Ns, R):
    """The depth targets of ``out``, the scene built from ``data``'s sampled and / or augmented M:
    gathered from the parent (src, a _DepthSource) or taken from ``data`` as they are, then rescaled
    by the augmentation's rotations R over the old measurements M_old (None: no augmentation).  One
    host read checks that every edge was found and that the transform kept the edge count."""
    if not getattr(data, "store_depth_targets", False):
        return out
    cam, pt = out.x.indices[0], out.x.indices[1]
    E = int(cam.shape[0])
    if src is not None:
        d, missing = src.gather(cam, pt)
        n_missing, E_old = torch.stack([missing[0].to(torch.int64), src.n_edges.to(torch.int64)]).tolist()
        if n_missing:
            raise _missing_error(n_missing, data.scene_name)
    else:
        d = _per_edge_depths(data, cam.device)[2]
        E_old = int(d.shape[0])
    if E != E_old:
        raise ValueError(f"{data.scene_name}: the transform changed the observed entries of M "
                         f"({E_old} edges before, {E} after); the depth targets no longer apply")
    if R is not None:
        fn = _native.depth_rescale if _kernels(cam) else depth_rescale_torch
        d = fn(d, cam.contiguous(), pt.contiguous(), M_old, Ns, R)
    out.depths, out.store_depth_targets = d, True
    return out


def _axis_angle_to_matrix(axis_angle):
    """pytorch3d.transforms.axis_angle_to_matrix (published formula: axis-angle -> quaternion with
    the small-angle series below 1e-6 -> quaternion_to_matrix, real part first)."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = angles * 0.5
    small = angles.abs() < 1e-6
    safe = torch.where(small, torch.ones_like(angles), angles)
    s = torch.where(small, 0.5 - angles * angles / 48, torch.sin(half) / safe)
    q = torch.cat([torch.cos(half), axis_angle * s], dim=-1)
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def rotational_homography(num_views, inplane_rot_aug_max_angle=None, tilt_rot_aug_max_angle=None):
    """R_aug [m, 3, 3] of SceneData.apply_rotational_homography_aug (SceneData.py:373-406), drawn from
    torch's global CPU RNG in the reference's order (in-plane angle, tilt angle, tilt axis)."""
    R = torch.eye(3)[None, :, :].repeat(num_views, 1, 1)
    inplane = inplane_rot_aug_max_angle or 0
    tilt = tilt_rot_aug_max_angle or 0
    assert inplane >= 0 and tilt >= 0
    if inplane > 0:
        ang = inplane * (2 * torch.rand((num_views,), dtype=torch.float32) - 1)
        vec = torch.zeros((num_views, 3), dtype=torch.float32)
        vec[:, 2] = ang / 180. * math.pi
        R = _axis_angle_to_matrix(vec) @ R
    if tilt > 0:
        ang = tilt * (2 * torch.rand((num_views,), dtype=torch.float32) - 1)
        alpha = torch.rand((num_views,), dtype=torch.float32) * 2 * math.pi
        axis = torch.zeros((num_views, 3), dtype=torch.float32)
        axis[:, 0] = torch.cos(alpha)
        axis[:, 1] = torch.sin(alpha)
        R = _axis_angle_to_matrix(axis * ang[:, None] / 180. * math.pi) @ R
    return R


def apply_rotational_homography_aug_device(data, inplane_rot_aug_max_angle=None, tilt_rot_aug_max_angle=None,
                                           max_piece=None):
    """SceneData.apply_rotational_homography_aug (datasets/SceneData.py:355-440) with M on the device:
    the per-camera 3x3 products (R_aug, H_aug = Ns^-1 R_aug Ns, y' = H_aug y) on the host in fp32
    as the reference computes them, the image points through gasfm_scene_homography, then the
    device graph build."""
    M = _dense_M(data)
    m = data.y.shape[0]
    dev = M.device
    hc = getattr(data, "_host_Ns_y", None)
    Ns_c, y_c = hc if hc is not None else (data.Ns.float().cpu(), data.y.float().cpu())
    src = getattr(data, "_depth_src", None)
    if not (inplane_rot_aug_max_angle or tilt_rot_aug_max_angle):
        out = scene_from_dense_device(M, data.Ns.to(dev), data.y.to(dev), data.scene_name, max_piece=max_piece)
        return _carry_depths(out, data, src, None, None, None)
    R = rotational_homography(m, inplane_rot_aug_max_angle, tilt_rot_aug_max_angle)
    Ninv = torch.linalg.inv(Ns_c)
    y = (Ninv @ R @ Ns_c) @ y_c
    M = M.contiguous()
    Ns_d, R_d = Ns_c.to(dev).contiguous(), R.to(dev).contiguous()
    Mn = _native.scene_homography(M, Ns_d, R_d, Ninv.to(dev).contiguous())
    out = scene_from_dense_device(Mn, Ns_c.to(dev), y.to(dev), data.scene_name,
                                  calibrated=getattr(data, "calibrated", True), max_piece=max_piece)
    # SceneData.py:431-434: the targets scale with the third coordinate under the rotation; the
    # augmentation moves the observed entries of M and creates or removes none (checked)
    return _carry_depths(out, data, src, M, Ns_d, R_d)
