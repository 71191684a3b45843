"""ESFMLoss over the visibility edges (csrc/esfm_loss.hip).

Drop-in for the reference's ``loss_functions.ESFMLoss`` (code/loss_functions.py:69-123): same
constructor (reads ``loss.infinity_pts_margin``, ``loss.pts_grad_equalization_pre_perspective_divide``,
``loss.normalize_grad_wrt_valid_projections_only``, ``loss.hinge_loss``, ``loss.hinge_loss_weight``
and asserts both heads are enabled), same ``forward(pred_dict, data, epoch=None)`` returning the
scalar loss, and the same gradients, including the ones the reference's gradient hook on the
projections imposes (loss_functions.py:104-113).

The reference projects every point into every camera (``Ps @ pts3D``: [m, 3, n], 2.4 GB at
m = 1000, n = 200k) and masks with the dense valid-observation matrix; here only the E observed
(camera, point) pairs -- the same edges the network runs on -- are projected:
  forward   one kernel -> per-workgroup (sum of loss terms, #valid-depth) -> colsum
  backward  one workgroup per camera (dPs) + one thread per point (dpts3D), no atomics
``#valid-depth`` stays on the device: the reference's ``.item()`` host sync (loss_functions.py:107)
is gone, so the loss can sit inside a captured step.

The measurement of edge e is ``data.x.values[e]``: M2sparse(normalize=True) (dataset_utils.py:116)
stores exactly the entries of ``data.norm_M`` (geo_utils.normalize_M, geo_utils.py:689) at the
valid positions, in the same cam-major order as ``data.x.indices``.

The reference's other training losses follow the same scheme: ``ExpDepthRegularizedOSELoss``
(csrc/ose_loss.hip, also over a union batch: static_batch.batch_loss) and ``DirectDepthLoss``
(csrc/depth_loss.hip); ``get_loss_func(conf)`` picks the loss ``loss.func`` names.
"""
import torch

from . import _native


def _check_projection_inputs(name, Ps, pts3D):
    for t, tname in ((Ps, "Ps_norm"), (pts3D, "pts3D")):
        if not t.is_cuda or t.dtype != torch.float32:
            raise TypeError(f"{name}: {tname} must be a float32 CUDA tensor (no CPU fallback)")
    if Ps.dim() != 3 or tuple(Ps.shape[1:]) != (3, 4) or pts3D.dim() != 2 or pts3D.shape[0] != 4:
        raise ValueError(f"{name}: expected Ps_norm [m, 3, 4] and pts3D [4, n], got {tuple(Ps.shape)}, "
                         f"{tuple(pts3D.shape)}")


def _flat_inputs(Ps, pts3D):
    """(P [m, 12], X [4, n]) contiguous, as the per-edge kernels read them."""
    return Ps.reshape(Ps.shape[0], 12).contiguous(), pts3D.contiguous()


def _grad_buffers(dloss, P, X):
    """(dloss [1] float32, dP, dX) for a per-edge backward; it returns dP.view(-1, 3, 4), dX."""
    return dloss.reshape(1).to(torch.float32).contiguous(), torch.empty_like(P), torch.empty_like(X)


class ESFMLossFn(torch.autograd.Function):
    """(Ps [m, 3, 4], pts3D [4, n]) -> mean over the edges of the per-edge loss term."""

    @staticmethod
    def forward(ctx, Ps, pts3D, edges, vals, cam_ptr, pt_ptr, pt_perm, conf, shard=None, E_global=None):
        """shard (gasfm_amd.distributed.ShardContext) / E_global: point-sharded scene.  Every rank
        holds all cameras and its own points with ALL their edges, so the loss is the global one
        from (sum of terms, #valid-depth) all-reduced over the ranks and divided by the global
        edge count; backward: dpts3D is rank-local and complete, dPs is summed over the ranks."""
        margin, hinge_w, hinge, equalize, valid_only = conf
        cam, pt = edges
        P, X = _flat_inputs(Ps, pts3D)
        part = torch.empty((_native.esfm_part_rows(cam.shape[0]), 2), dtype=torch.float32, device=X.device)
        _native.esfm_fwd(cam, pt, vals, P, X, margin, hinge_w, hinge, part)
        tot = _native.colsum(part)  # (sum of terms, #valid-depth)
        E = cam.shape[0]
        if shard is not None:
            tot = shard.all_reduce_(tot)
            E = int(E_global)
        ctx.save_for_backward(P, X, cam, pt, vals, cam_ptr, pt_ptr, pt_perm, tot)
        ctx.conf, ctx.shard, ctx.E = conf, shard, E
        return tot[0] / E

    @staticmethod
    def backward(ctx, dloss):
        P, X, cam, pt, vals, cam_ptr, pt_ptr, pt_perm, tot = ctx.saved_tensors
        margin, hinge_w, hinge, equalize, valid_only = ctx.conf
        dloss, dP, dX = _grad_buffers(dloss, P, X)
        # E_norm = the global edge count on a sharded scene: the un-equalized terms and the equalized
        # (normalize(G) / E) branch both divide by it, as loss_functions.py:110 divides by sum(valid_pts)
        _native.esfm_bwd(cam_ptr, pt_ptr, pt_perm, cam, pt, vals, P, X, margin, hinge_w, hinge, equalize, valid_only,
                         dloss, tot, dP, dX, E_norm=ctx.E)
        if ctx.shard is not None:
            ctx.shard.all_reduce_(dP)
        return (dP.view(-1, 3, 4), dX) + (None,) * 8


def scene_csr(data):
    """(cache dict, camera CSR, point CSR, point-order edge ids or None) of a scene: from the device
    scene build while its graph wrappers are not built (scene_device builds them on first use), else
    from the network's own plans (proj2view: camera segments over the cam-major edges;
    proj2scenepoint: point segments with perm = edge ids in point order).  The cache dict lives as
    long as that source (per device)."""
    b = data.__dict__.get("_scene_build")
    if b is not None and "graph_wrappers" not in data.__dict__:
        return b.setdefault("caches", {}), b["cam_ptr"], b["pt_ptr"], b["perm"]
    gw = data.graph_wrappers
    pv, ps = gw["proj2view"].plan, gw["proj2scenepoint"].plan
    if pv.perm is not None:
        raise ValueError("ESFMLoss: proj2view plan must cover cam-major sorted edges")
    if "_caches" not in pv.__dict__:
        pv._caches = {}
    return pv._caches, pv.seg_ptr, ps.seg_ptr, ps.perm


def _edge_tensors(data):
    """int32 (cam, pt), contiguous float32 values and the camera / point CSRs (scene_csr).  The int32
    indices are cached, keyed on the index tensor's storage and version."""
    caches, cam_ptr, pt_ptr, pt_perm = scene_csr(data)
    idx = data.x.indices
    key = (idx.data_ptr(), idx._version, tuple(idx.shape))  # an in-place edit of the indices invalidates it
    cache = caches.get("esfm_edges")
    if cache is None or cache[0] != key:
        cache = (key, (idx[0].to(torch.int32).contiguous(), idx[1].to(torch.int32).contiguous()))
        caches["esfm_edges"] = cache
    vals = data.x.values
    if vals.dtype != torch.float32 or not vals.is_contiguous():
        vals = vals.float().contiguous()
    return cache[1], vals, cam_ptr, pt_ptr, pt_perm


class ESFMLoss(torch.nn.Module):
    def __init__(self, conf):
        super().__init__()
        assert conf.get_bool("model.view_head.enabled", default=False)
        assert conf.get_bool("model.scenepoint_head.enabled", default=False)
        self.infinity_pts_margin = conf.get_float("loss.infinity_pts_margin")
        self.pts_grad_equalization_pre_perspective_divide = conf.get_bool(
            "loss.pts_grad_equalization_pre_perspective_divide")
        self.normalize_grad_wrt_valid_projections_only = False
        if self.pts_grad_equalization_pre_perspective_divide:
            self.normalize_grad_wrt_valid_projections_only = conf.get_bool(
                "loss.normalize_grad_wrt_valid_projections_only")
        self.hinge_loss = conf.get_bool("loss.hinge_loss")
        self.hinge_loss_weight = conf.get_float("loss.hinge_loss_weight") if self.hinge_loss else 0

    def kernel_conf(self):
        return (float(self.infinity_pts_margin), float(self.hinge_loss_weight), bool(self.hinge_loss),
                bool(self.pts_grad_equalization_pre_perspective_divide),
                bool(self.normalize_grad_wrt_valid_projections_only))

    def forward(self, pred_dict, data, epoch=None):
        Ps, pts3D = pred_dict["Ps_norm"], pred_dict["pts3D"]
        _check_projection_inputs("ESFMLoss", Ps, pts3D)
        edges, vals, cam_ptr, pt_ptr, pt_perm = _edge_tensors(data)
        if edges[0].shape[0] == 0:
            raise ValueError("ESFMLoss: no valid observations (the reference's mean would be NaN)")
        shard = getattr(data, "shard", None)
        E_global = getattr(data, "n_edges_global", None)
        if shard is not None and E_global is None:
            raise ValueError("ESFMLoss: a sharded scene must carry n_edges_global (distributed.shard_scene)")
        return ESFMLossFn.apply(Ps, pts3D, edges, vals, cam_ptr, pt_ptr, pt_perm, self.kernel_conf(), shard,
                                E_global)


class OSELossFn(torch.autograd.Function):
    """(Ps [m, 3, 4], pts3D [4, n]) -> mean over the edges of ||y_xy - y_z m_e|| + w_reg exp(-y_z)
    (csrc/ose_loss.hip)."""

    @staticmethod
    def forward(ctx, Ps, pts3D, edges, vals, cam_ptr, pt_ptr, pt_perm, w_reg):
        cam, pt = edges
        P, X = _flat_inputs(Ps, pts3D)
        tot = _native.colsum(_native.ose_fwd(cam, pt, vals, P, X, w_reg))
        ctx.save_for_backward(P, X, cam, pt, vals, cam_ptr, pt_ptr, pt_perm)
        ctx.w_reg = w_reg
        return tot[0] / cam.shape[0]

    @staticmethod
    def backward(ctx, dloss):
        P, X, cam, pt, vals, cam_ptr, pt_ptr, pt_perm = ctx.saved_tensors
        dloss, dP, dX = _grad_buffers(dloss, P, X)
        _native.ose_bwd(cam_ptr, pt_ptr, pt_perm, cam, pt, vals, P, X, ctx.w_reg, dloss, dP, dX)
        return (dP.view(-1, 3, 4), dX) + (None,) * 6


class ExpDepthRegularizedOSELoss(torch.nn.Module):
    """The reference's ``loss_functions.ExpDepthRegularizedOSELoss`` (code/loss_functions.py:126-150):
    object space error plus ``loss.depth_regul_weight * exp(-depth)``, a smooth loss with no barrier
    at the principal plane, over the visibility edges instead of the dense [m, 3, n] projections."""

    def __init__(self, conf):
        super().__init__()
        assert conf.get_bool("model.view_head.enabled", default=False)
        assert conf.get_bool("model.scenepoint_head.enabled", default=False)
        self.depth_regul_weight = conf.get_float("loss.depth_regul_weight")

    def forward(self, pred_dict, data, epoch=None):
        Ps, pts3D = pred_dict["Ps_norm"], pred_dict["pts3D"]
        _check_projection_inputs("ExpDepthRegularizedOSELoss", Ps, pts3D)
        if getattr(data, "shard", None) is not None:
            raise ValueError("ExpDepthRegularizedOSELoss: point-sharded scenes are not supported")
        edges, vals, cam_ptr, pt_ptr, pt_perm = _edge_tensors(data)
        if edges[0].shape[0] == 0:
            raise ValueError("ExpDepthRegularizedOSELoss: no valid observations (the reference's mean would be NaN)")
        return OSELossFn.apply(Ps, pts3D, edges, vals, cam_ptr, pt_ptr, pt_perm, float(self.depth_regul_weight))


class DepthLossFn(torch.autograd.Function):
    """(a [E], b [E]) -> mean |a / mean a - b / mean b| or its square (csrc/depth_loss.hip)."""

    @staticmethod
    def forward(ctx, a, b, l2):
        a = a.contiguous()
        sums, tot = _native.depth_loss_fwd(a, b, l2)
        ctx.save_for_backward(a, b, sums, tot)
        ctx.l2 = l2
        return tot[0] / a.shape[0]

    @staticmethod
    def backward(ctx, dloss):
        a, b, sums, tot = ctx.saved_tensors
        dloss = dloss.reshape(1).to(torch.float32).contiguous()
        return _native.depth_loss_bwd(a, b, sums, tot, ctx.l2, dloss), None, None


def _edge_depth_targets(data, indices):
    """float32 [E] target depths in edge order from ``data.depths``: a per-edge [E] tensor as it is,
    or the reference's dense [m, n] tensor gathered at ``indices`` on the device, once (cached like
    _edge_tensors' indices, keyed on both tensors' storage and version)."""
    dep = getattr(data, "depths", None)
    if dep is None:
        raise ValueError("DirectDepthLoss: the scene carries no data.depths")
    E = indices.shape[1]
    if dep.dim() == 1:
        if dep.shape[0] != E:
            raise ValueError(f"DirectDepthLoss: per-edge data.depths has {dep.shape[0]} entries for {E} edges")
        if not dep.is_cuda or dep.dtype != torch.float32:
            raise TypeError("DirectDepthLoss: per-edge data.depths must be a float32 CUDA tensor")
        return dep.contiguous()
    if dep.dim() != 2:
        raise ValueError(f"DirectDepthLoss: data.depths must be [m, n] or [E], got {tuple(dep.shape)}")
    caches = scene_csr(data)[0]
    key = (dep.data_ptr(), dep._version, tuple(dep.shape), indices.data_ptr(), indices._version, E)
    cache = caches.get("depth_targets")
    if cache is None or cache[0] != key:
        cache = (key, dep.to(indices.device)[indices[0], indices[1]].float().contiguous())
        caches["depth_targets"] = cache
    return cache[1]


class DirectDepthLoss(torch.nn.Module):
    """The reference's ``loss_functions.DirectDepthLoss`` (code/loss_functions.py:24-66): L1 / L2
    distance of the mean-normalised predicted and target depths of the observed projections."""

    def __init__(self, conf):
        super().__init__()
        assert conf.get_bool("model.depth_head.enabled")
        self.cost_fcn = conf.get_string("loss.cost_fcn")
        assert self.cost_fcn in ["L1", "L2"]
        if not conf.get_bool("dataset.calibrated"):
            raise NotImplementedError("DirectDepthLoss: uncalibrated data (as the reference)")

    def forward(self, pred_dict, data, epoch=None):
        dep = pred_dict["depths"]
        a = dep.values
        if not a.is_cuda or a.dtype != torch.float32:
            raise TypeError("DirectDepthLoss: depths must be a float32 CUDA tensor (no CPU fallback)")
        if a.dim() != 2 or a.shape[1] != 1:
            raise ValueError(f"DirectDepthLoss: expected depths values [E, 1], got {tuple(a.shape)}")
        if a.shape[0] == 0:
            raise ValueError("DirectDepthLoss: no valid observations (the reference's mean would be NaN)")
        b = _edge_depth_targets(data, dep.indices)
        return DepthLossFn.apply(a[:, 0], b, self.cost_fcn == "L2")


class GTLoss(torch.nn.Module):
    def __init__(self, conf):
        raise NotImplementedError(
            "GTLoss is not built: it is camera-sized with no hot path, and the reference's calibrated branch "
            "calls geo_utils.rot_to_quat, which does not exist in the reference tree, so there is nothing to "
            "check a port against")


_LOSSES = {"ESFMLoss": ESFMLoss, "ExpDepthRegularizedOSELoss": ExpDepthRegularizedOSELoss, "GTLoss": GTLoss,
           "DirectDepthLoss": DirectDepthLoss}


def get_loss_func(conf):
    """The reference's ``loss_functions.get_loss_func`` (code/loss_functions.py:8-21): the loss
    ``loss.func`` names, after checking that the enabled heads are the ones it trains."""
    spec = conf.get_string("loss.func")
    if spec in ("ESFMLoss", "ExpDepthRegularizedOSELoss", "GTLoss"):
        assert conf.get_bool("model.view_head.enabled")
        assert conf.get_bool("model.scenepoint_head.enabled")
        assert not conf.get_bool("model.depth_head.enabled"), \
            "Make sure that model.depth_head.enabled=False, if there is no loss applied on such output."
    elif spec == "DirectDepthLoss":
        assert conf.get_bool("model.depth_head.enabled")
        assert not conf.get_bool("model.view_head.enabled"), \
            "Make sure that model.view_head.enabled=False, if there is no loss applied on such output."
        assert not conf.get_bool("model.scenepoint_head.enabled"), \
            "Make sure that model.scenepoint_head.enabled=False, if there is no loss applied on such output."
    else:
        assert False, "Unknown loss function: {}.".format(spec)
    return _LOSSES[spec](conf)
