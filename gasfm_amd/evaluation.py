"""Per-step "core" errors on the device (with loss.py's ESFMLoss).

Drop-in for the reference's ``evaluation.compute_core_errors(data, pred_dict, conf)``
(code/evaluation.py:8-74), which train.py:91 calls on every training step.  The reference
copies M, Ns and the predictions to the host and projects every point into every camera in
numpy (geo_utils.reprojection_error_with_points, geo_utils.py:371-391: an [m, 3, n] array);
here only the E observed (camera, point) pairs are projected, by ``gasfm_reproj_error``
(csrc/esfm_loss.hip), and np.nanmean's sum and count are reduced on the device.

  our_repro = nanmean_e || xy_e - pi(Ns_c^-1 Ps_norm_c pflat(pts3D)_p) ||   (pixels)

The visible set is ``get_M_valid_points(xs)`` -- exactly the network's edges (data.x.indices).
The depth-head branch (``eval.calc_reprojerr_with_gtposes_for_depth_pred``) adds
``repro_backproj_rnd_gt_2view``: every edge's pixel is backprojected with its predicted depth
(rescaled by s_gt / s_pred, the mean depths) and reprojected at another edge of the same track with
the ground-truth cameras -- gasfm_depth_norm_stats, gasfm_track_cycle and gasfm_backproj_2view
(csrc/depth_eval.hip, gasfm_amd/depth_eval) in place of the reference's dense [m, n, 3] fp64 arrays.
The random pairing is drawn on the device (torch.manual_seed governs it); ``pairing=`` takes a
ready src [E] instead.  Without a depth head or a calibrated scene it raises like the reference.

Scene evaluation (train.epoch_evaluation, reference train.py:170-259) runs on the same edges:
``prepare_predictions`` / ``compute_errors`` / ``get_dummy_errors`` keep the reference's signatures
and dict keys (code/evaluation.py:76-432), for the explicit heads, the depth head, or both.  The
depth head adds ``depth_{pred,gt}_norm_*``, ``depth_pred_err_mean`` and, with the flag above,
``repro_backproj_*_rnd_gt_2view``; quantiles are one device sort per array (np.quantile's linear rule).

  triangulation      gasfm_ba_dlt through ba._Edges built from the scene's own edges
  repro errors       gasfm_reproj_error (our_repro, triangulated_repro, repro_ba)
  depth metrics      gasfm_depth_stats (csrc/eval_metrics.hip) instead of the dense [m, 3, n]
                     ``Ps @ pts3D_pred`` of evaluation.py:351-363
  poses, alignment   m-sized fp64 work on the host: decompose_camera_matrix, and align_cameras
                     with the reference's cvxpy problem  min_{c, t} sum_i || g_i - (c p_i + t) ||
                     (unsquared norms; convex, 4 unknowns) solved by a damped Newton iteration
                     started from the closed-form least-squares fit (``fit_scale_translation``)
  bundle adjustment  ba.euc_ba / ba.proj_ba with ``edges=``

``outputs['xs']``, the dense [m, n, 2] array the reference stores up front (1.6 GB at m = 1000,
n = 200k), is built on first access; the device tensors compute_errors needs travel under
``outputs['_device']``.  A scene without a dense M (SceneData.from_sparse) is evaluated when it
carries ``pixel_xy`` ([E, 2] pixel measurements in edge order), ``Ns`` and, if calibrated, ``y``.
"""
from time import time

import numpy as np
import torch

from . import _native, depth_eval
from .loss import _edge_depth_targets, _edge_tensors, scene_csr


def _pixel_measurements(data):
    """[E, 2] pixel coordinates of the edges, gathered from the dense M once per scene/device."""
    xy = getattr(data, "pixel_xy", None)
    if xy is not None:
        return xy.to(device=data.x.indices.device, dtype=torch.float32).contiguous()
    caches = scene_csr(data)[0]
    M = getattr(data, "M", None)
    if M is None:
        M = getattr(data, "_M", None)
    if M is None:
        raise ValueError("compute_core_errors: the scene carries no dense measurement matrix M")
    idx = data.x.indices
    # keyed on both tensors' storage and version: an in-place edit of M (augmentation) or of the
    # indices recomputes the gather
    key = (M.data_ptr(), M._version, tuple(M.shape), idx.data_ptr(), idx._version)
    cached = caches.get("pixel_xy")
    if cached is None or cached[0] != key:
        Md = M.to(idx.device)
        xy = torch.stack([Md[2 * idx[0], idx[1]], Md[2 * idx[0] + 1, idx[1]]], 1).float().contiguous()
        cached = (key, xy)
        caches["pixel_xy"] = cached
    return cached[1]


def _pixel_cameras(data, Ps_norm):
    """Ps = Ns^-1 Ps_norm (evaluation.py:22,27)."""
    Ns_invT = getattr(data, "Ns_invT", None)
    if Ns_invT is not None:
        Ns_inv = Ns_invT.transpose(1, 2)
    else:
        Ns_inv = torch.linalg.inv(data.Ns.double().cpu()).float()
    Ns_inv = Ns_inv.to(device=Ps_norm.device, dtype=torch.float32)
    return (Ns_inv @ Ps_norm.detach()).reshape(-1, 12).contiguous()


def reprojection_error_mean(data, pred_dict, per_edge=False):
    """0-d device tensor nanmean of the reprojection errors (no host sync); with ``per_edge`` also
    the [E] errors in data.x.indices order."""
    Ps_norm, pts3D = pred_dict["Ps_norm"], pred_dict["pts3D"]
    if not Ps_norm.is_cuda or not pts3D.is_cuda:
        raise TypeError("compute_core_errors: predictions must be CUDA tensors (no CPU fallback)")
    (cam, pt), _, _, _, _ = _edge_tensors(data)
    xy = _pixel_measurements(data)
    P = _pixel_cameras(data, Ps_norm)
    X = pts3D.detach().float().contiguous()
    err = torch.empty(cam.shape[0], dtype=torch.float32, device=X.device) if per_edge else None
    part = _native.reproj_error(cam, pt, xy, P, X, err)
    tot = _native.colsum(part)
    mean = tot[0] / tot[1]  # count 0 -> nan, as np.nanmean of an all-NaN array
    return (mean, err) if per_edge else mean


# ------------------------------------------------------------------ depth head
def _per_edge(t, E, name):
    """[E] values of a SparseMat ([E, 1] values) or of a plain [E] / [E, 1] tensor, detached."""
    v = t if torch.is_tensor(t) else t.values
    v = v.detach()
    if v.dim() == 2 and v.shape[1] == 1:
        v = v[:, 0]
    if v.dim() != 1 or v.shape[0] != E:
        raise ValueError(f"{name}: expected {E} per-edge values, got {tuple(v.shape)}")
    return v.contiguous()


def _depth_pair(data, pred_dict):
    """(predicted depths [E], target depths [E]) in the scene's edge order."""
    dep = pred_dict["depths"]
    idx = data.x.indices
    dp = _per_edge(dep, idx.shape[1], "pred_dict['depths']")
    tgt = getattr(data, "depths", None)
    if tgt is not None and tgt.dim() == 1 and not tgt.is_cuda:  # per-edge targets of a CPU scene
        return dp, _per_edge(tgt, idx.shape[1], "data.depths")
    return dp, _edge_depth_targets(data, idx)


def _camera_table(data, dtype, device):
    """depth_eval.camera_table of the scene's ground-truth cameras, once per scene, device and dtype:
    keyed on the storage and version of y and Ns, as _pixel_measurements keys pixel_xy.  Ks is
    Ns_invT^T where the scene carries it (the reference's Ks), else Ns^-1 in fp64."""
    if data.y is None:
        raise ValueError("depth evaluation: the scene carries no ground-truth cameras y")
    Ns_invT = getattr(data, "Ns_invT", None)
    Ksrc = Ns_invT if Ns_invT is not None else data.Ns
    if Ksrc is None:
        raise ValueError("depth evaluation: the scene carries no normalisation matrices Ns")
    caches = scene_csr(data)[0]
    key = (data.y.data_ptr(), data.y._version, Ksrc.data_ptr(), Ksrc._version, str(device), dtype)
    cached = caches.get("camtab")
    if cached is None or cached[0] != key:
        Ksrc = Ksrc.to(device)
        K = Ksrc.transpose(1, 2) if Ns_invT is not None else torch.linalg.inv(Ksrc.double())
        cached = (key, depth_eval.camera_table(K, data.y.to(device), dtype))
        caches["camtab"] = cached
    return cached[1]


def _pairing(pairing, E, device):
    src = torch.as_tensor(pairing).to(device=device, dtype=torch.int32).contiguous()
    if src.dim() != 1 or src.shape[0] != E:
        raise ValueError(f"pairing: expected src [{E}], got {tuple(src.shape)}")
    return src


def backproj_2view_error(data, dp, dg, pairing=None, per_edge=False):
    """The 2-view error of per-edge depths dp, rescaled to the targets dg: scales -> keys -> pairing ->
    2-view kernel -> colsum, nothing read on the host.  Returns (tot [2] = sum and count of the non-NaN
    errors, scales [2] = s_pred, s_gt), with ``per_edge`` also (err [E], rdepth [E]).  ``pairing``:
    a ready src [E] (checked to stay within the tracks) instead of a random draw."""
    (cam, pt), _, _, pt_ptr, pt_perm = _edge_tensors(data)
    dev = cam.device
    xy = _pixel_measurements(data)
    kernels = dp.is_cuda and dp.dtype == torch.float32
    scales, _ = depth_eval.depth_norm_stats(dp, dg, stats=False)
    scale = scales[1] / scales[0]  # predicted depths / s_pred * s_gt without a rescaled copy
    if pairing is None:
        src, _ = depth_eval.track_cycle(pt_ptr, pt_perm, depth_eval.draw_keys(cam.shape[0], dev))
        check = None
    else:
        src, check = _pairing(pairing, cam.shape[0], dev), pt
    tab = _camera_table(data, torch.float32 if kernels else torch.float64, dev)
    res = depth_eval.backproj_2view(cam, check, xy, dp, scale, src, tab, per_edge)
    return (res[0], scales) + tuple(res[1:]) if per_edge else (res, scales)


def _depth_conf(conf):
    """(depth head enabled, 2-view error wanted), with the reference's refusals (evaluation.py:33-49)."""
    depth_head = conf.get_bool("model.depth_head.enabled", default=False)
    two_view = conf.get_bool("eval.calc_reprojerr_with_gtposes_for_depth_pred", default=False)
    if two_view:
        if not conf.get_bool("dataset.calibrated"):
            raise ValueError("calc_reprojerr_with_gtposes_for_depth_pred needs a calibrated dataset")
        if not depth_head:
            # the reference raises NotImplementedError with both explicit heads and asserts otherwise
            raise NotImplementedError("calc_reprojerr_with_gtposes_for_depth_pred requires the depth head")
    return depth_head, two_view


def compute_core_errors(data, pred_dict, conf, pairing=None):
    core_errors = {}
    view_head_enabled = conf.get_bool("model.view_head.enabled", default=False)
    scenepoint_head_enabled = conf.get_bool("model.scenepoint_head.enabled", default=False)
    _, two_view = _depth_conf(conf)
    if view_head_enabled and scenepoint_head_enabled:
        core_errors["our_repro"] = float(reprojection_error_mean(data, pred_dict))
    if two_view:
        tot, _ = backproj_2view_error(data, *_depth_pair(data, pred_dict), pairing=pairing)
        core_errors["repro_backproj_rnd_gt_2view"] = float(tot[0] / tot[1])  # count 0 -> nan (np.nanmean)
    return core_errors


# ------------------------------------------------------------------ scene evaluation
def _heads(conf):
    """(calibrated, both explicit heads enabled)."""
    explicit = conf.get_bool("model.view_head.enabled", default=False) and conf.get_bool(
        "model.scenepoint_head.enabled", default=False)
    return conf.get_bool("dataset.calibrated"), explicit


class PredictionOutputs(dict):
    """prepare_predictions' result: the reference's keys; ``xs`` ([m, n, 2], dense) and the dense
    [m, n] ``depths_pred_dense`` / ``depths_gt_dense`` are built from the scene on first access."""

    def _dense_depths(self, key):
        dev = dict.__getitem__(self, "_device")
        if key == "depths_gt_dense" and dev.get("depths_gt_dense") is not None:
            return dev["depths_gt_dense"].detach().cpu().numpy()  # the scene's own dense data.depths
        per_edge = dev["depths_pred" if key == "depths_pred_dense" else "depths_gt"]
        dense = np.zeros((dev["m"], dev["n"]), dtype=per_edge.cpu().numpy().dtype)  # to_dense(): 0 elsewhere
        dense[dev["cam"].cpu().numpy(), dev["pt"].cpu().numpy()] = per_edge.cpu().numpy()
        return dense

    def __missing__(self, key):
        if key in ("depths_pred_dense", "depths_gt_dense") and "depths_pred" in dict.__getitem__(self, "_device"):
            self[key] = self._dense_depths(key)
            return self[key]
        if key != "xs":
            raise KeyError(key)
        dev = dict.__getitem__(self, "_device")
        if dev["M"] is not None:  # geo_utils.M_to_xs
            xs = dev["M"].cpu().numpy().reshape(dev["m"], 2, dev["n"]).transpose(0, 2, 1)
        else:
            xs = np.zeros((dev["m"], dev["n"], 2), dtype=np.float32)
            xs[dev["cam"].cpu().numpy(), dev["pt"].cpu().numpy()] = dev["xy"].cpu().numpy()
        self["xs"] = xs
        return xs


def decompose_camera_matrix(Ps, Ks=None):
    """geo_utils.decompose_camera_matrix (geo_utils.py:149-171) with inverse_direction_camera2global:
    (R^T, camera centres -R^T t) of K^-1 P, in fp64."""
    Ps = np.asarray(Ps, dtype=np.float64)
    Rt = np.linalg.inv(np.asarray(Ks, dtype=np.float64)) @ Ps if Ks is not None else Ps
    Rs = np.transpose(Rt[:, :3, :3], (0, 2, 1))
    return Rs, -(Rs @ Rt[:, :3, 3:4])[:, :, 0]


def compare_rotations(R1, R2):
    """Angle between rotations in degrees (geo_utils.py:14-22)."""
    cos = (np.einsum("nij,nij->n", R1, R2) - 1) / 2  # trace(R1 R2^T)
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def translation_rotation_errors(R_fixed, t_fixed, gt_Rs, gt_ts):
    return compare_rotations(R_fixed, gt_Rs), np.linalg.norm(t_fixed - gt_ts, axis=-1)


def _norm_sum(g, p, c, t):
    return float(np.linalg.norm(g - (c * p + t), axis=1).sum())


def least_squares_scale_translation(g, p):
    """Closed-form minimiser of sum || g_i - (c p_i + t) ||^2."""
    pm, gm = p.mean(0), g.mean(0)
    den = float(((p - pm) ** 2).sum())
    c = float(((p - pm) * (g - gm)).sum()) / den if den > 0 else 1.0
    return c, gm - c * pm


def fit_scale_translation(g, p, gtol=1e-10, fit_tol=1e-12, max_iter=100):
    """min over (c, t) of  f = sum_i || g_i - (c p_i + t) ||_2  (align_cameras' cvxpy objective,
    geo_utils.py:94-107) -> (c, t [3], converged).

    f is convex in the 4 unknowns.  From the least-squares fit, Newton steps on f (Hessian
    sum_i J_i^T (I - u_i u_i^T) J_i / r_i, J_i = [p_i | I], u_i = residual direction) with a
    backtracking line search on f.  Residual norms are floored (1e-15 of the mean spread of g) so
    a vanishing residual divides by a positive number.  Converged when the gradient norm is
    <= gtol * S, S = sum || g_i - mean(g) ||, or when f <= fit_tol * S (an exact fit, where the
    gradient of the norms is undefined)."""
    g, p = np.asarray(g, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if not (np.isfinite(g).all() and np.isfinite(p).all()) or g.shape[0] == 0:
        return 1.0, np.zeros(3), False
    S = float(np.linalg.norm(g - g.mean(0), axis=1).sum())
    c, t = least_squares_scale_translation(g, p)
    if S == 0.0:
        return c, t, _norm_sum(g, p, c, t) == 0.0
    floor = 1e-15 * S / g.shape[0]
    J = np.concatenate([p[:, :, None], np.broadcast_to(np.eye(3), (p.shape[0], 3, 3))], axis=2)  # [m, 3, 4]
    f = _norm_sum(g, p, c, t)
    for _ in range(max_iter):
        if f <= fit_tol * S:
            return c, t, True
        res = g - (c * p + t)
        r = np.maximum(np.linalg.norm(res, axis=1), floor)
        u = res / r[:, None]
        grad = -np.einsum("mi,mij->j", u, J)
        if np.linalg.norm(grad) <= gtol * S:
            return c, t, True
        Pu = (np.eye(3)[None] - u[:, :, None] * u[:, None, :]) / r[:, None, None]
        H = np.einsum("mki,mkl,mlj->ij", J, Pu, J)
        H += 1e-12 * np.trace(H) / 4 * np.eye(4)  # collinear residuals leave H singular
        try:
            step = -np.linalg.solve(H, grad)
        except np.linalg.LinAlgError:
            return c, t, False
        slope, a = float(grad @ step), 1.0
        while a > 1e-12:
            fn = _norm_sum(g, p, c + a * step[0], t + a * step[1:])
            if fn <= f + 1e-4 * a * slope:
                break
            a *= 0.5
        else:
            # no representable decrease left along a descent direction: f is at its floating-point
            # minimum; accept it only under the looser bar the tests hold the solver to
            return c, t, bool(np.linalg.norm(grad) <= 1e-8 * S)
        c, t, f = c + a * step[0], t + a * step[1:], fn
    return c, t, False


def align_cameras(pred_Rs, gt_Rs, pred_ts, gt_ts, return_alignment=False):
    """geo_utils.align_cameras (geo_utils.py:54-126): the rotation from the SVD of
    sum_i R_gt,i R_pred,i^T with the determinant fix, scale and translation from
    fit_scale_translation.  On SVD failure or a fit that does not converge the predictions come
    back unchanged with similarity_mat = eye(4), as in the reference.  ("ts" are camera centres.)"""
    pred_Rs, gt_Rs = np.asarray(pred_Rs, dtype=np.float64), np.asarray(gt_Rs, dtype=np.float64)
    pred_ts, gt_ts = np.asarray(pred_ts, dtype=np.float64), np.asarray(gt_ts, dtype=np.float64)

    def unchanged(why):
        print(f"[WARNING] Camera alignment failed at {why}. Simply return predicted poses as-is.")
        return (pred_Rs.copy(), pred_ts.copy(), np.eye(4)) if return_alignment else (pred_Rs.copy(), pred_ts.copy())

    Q = np.sum(gt_Rs @ np.transpose(pred_Rs, (0, 2, 1)), axis=0)
    try:
        if not np.isfinite(Q).all():
            raise np.linalg.LinAlgError("non-finite rotations")
        Uq, _, Vqh = np.linalg.svd(Q)
    except np.linalg.LinAlgError:
        return unchanged("SVD")
    sv = np.ones(3)
    sv[-1] = np.linalg.det(Uq @ Vqh)
    R_opt = Uq @ np.diag(sv) @ Vqh
    R_fixed = R_opt[None] @ pred_Rs
    rotated = pred_ts @ R_opt.T
    c, t, ok = fit_scale_translation(gt_ts, rotated)
    if not ok:
        return unchanged("optimization")
    t_fixed = c * rotated + t[None]
    if not return_alignment:
        return R_fixed, t_fixed
    sim = np.eye(4)
    sim[:3, :3] = c * R_opt
    sim[:3, 3] = t
    return R_fixed, t_fixed, sim


def _f32_points(X4n, dev):
    """[4, n] numpy / tensor -> contiguous float32 device tensor (the error kernels' pts3D)."""
    return torch.as_tensor(X4n).to(device=dev, dtype=torch.float32).contiguous()


_BA_REPEAT_KEYS = ("repro_before", "repro_middle", "repro_middle_triangulated", "repro_after")


def prepare_predictions(data, pred_dict, conf, bundle_adjustment):
    from . import ba
    calibrated, explicit = _heads(conf)
    depth_head, two_view = _depth_conf(conf)
    outputs = PredictionOutputs()
    outputs["scene_name"] = data.scene_name
    (cam, pt), _, cam_ptr, pt_ptr, pt_perm = _edge_tensors(data)
    dev = cam.device
    xy = _pixel_measurements(data)
    m, n = int(data.x.shape[0]), int(data.x.shape[1])
    M = getattr(data, "M", None)
    state = {"cam": cam, "pt": pt, "xy": xy, "cam_ptr": cam_ptr, "pt_ptr": pt_ptr, "perm": pt_perm, "m": m, "n": n,
             "M": M if M is not None else getattr(data, "_M", None)}
    outputs["_device"] = state
    if data.Ns is None:
        raise ValueError("prepare_predictions: the scene carries no normalisation matrices Ns")
    Ns = data.Ns.detach().cpu().numpy()
    Ns_invT = getattr(data, "Ns_invT", None)
    Ns_inv = (Ns_invT.transpose(1, 2).cpu().numpy() if Ns_invT is not None
              else np.linalg.inv(Ns.astype(np.float64)))
    if calibrated:
        Ks = Ns_inv  # Ks for calibrated scenes, a normalisation matrix otherwise
        outputs["Ks"] = Ks
    if depth_head:
        # evaluation.py:99-126; the dense depths_pred_dense / depths_gt_dense are built on first access
        dp, dg = _depth_pair(data, pred_dict)
        state["depths_pred"], state["depths_gt"] = dp, dg
        tgt = getattr(data, "depths", None)
        state["depths_gt_dense"] = tgt if tgt is not None and tgt.dim() == 2 else None
        scales, _ = depth_eval.depth_norm_stats(dp, dg, stats=False)
        state["scales"] = scales
        s = scales.cpu().numpy()
        outputs["s_pred"], outputs["s_gt"] = s[0], s[1]
        if two_view:
            outputs["Ps_gt"] = data.y.detach().cpu().numpy()
            state["camtab"] = _camera_table(data, torch.float32 if dp.is_cuda and dp.dtype == torch.float32
                                            else torch.float64, dev)
    if not explicit:
        return outputs

    Ps_norm_d, pts3D_d = pred_dict["Ps_norm"], pred_dict["pts3D"]
    if not Ps_norm_d.is_cuda or not pts3D_d.is_cuda:
        raise TypeError("prepare_predictions: predictions must be CUDA tensors (no CPU fallback)")
    dev = pts3D_d.device
    P = _pixel_cameras(data, Ps_norm_d)  # [m, 12] float32, Ns^-1 Ps_norm
    X = pts3D_d.detach().float().contiguous()
    state["P"], state["X"] = P, X
    Ps_norm = Ps_norm_d.detach().cpu().numpy()
    Ps = P.view(m, 3, 4).cpu().numpy()
    pts3D_pred = (X / X[-1]).cpu().numpy()  # pflat

    # DLT triangulation from the predicted cameras (n_view_triangulation, geo_utils.py:659-671);
    # may differ from the one BA optionally starts from
    ed = ba._Edges.from_edges(cam, pt, xy, m, n)
    F64 = torch.float64
    Ns64 = torch.as_tensor(Ns).to(dev, F64)
    P64 = torch.as_tensor(Ns_inv).to(dev, F64) @ Ps_norm_d.detach().to(F64)  # un-normalised in fp64
    X_tri = ed.dlt(P64, Ns64).t().contiguous()  # [4, n], NaN where undetermined
    state["X_tri"] = X_tri.float().contiguous()
    pts3D_triangulated = X_tri.cpu().numpy()

    outputs["Ps"] = Ps
    outputs["Ps_norm"] = Ps_norm
    outputs["pts3D_pred"] = pts3D_pred
    outputs["pts3D_triangulated"] = pts3D_triangulated

    def run_ba(fn, **kw):
        begin = time()
        res = fn(Xs_our=pts3D_pred.T, Ns=Ns, repeat=conf.get_bool("ba.repeat"),
                 triangulation=conf.get_bool("ba.triangulation"), return_repro=True,
                 print_out=conf.get_bool("ba.print_out", default=True), device=dev, edges=ed, **kw)
        outputs["ba_time"] = time() - begin
        outputs["Xs_ba"] = res["Xs"].T  # 4, n
        outputs["Ps_ba"] = res["Ps"]
        outputs["ba_converged1"] = res["converged1"]
        if conf.get_bool("ba.repeat"):
            for k in _BA_REPEAT_KEYS:
                outputs[k.replace("repro_", "repro_ba_")] = res[k]
            outputs["ba_converged2"] = res["converged2"]
        state["P_ba"] = torch.as_tensor(res["Ps"]).to(dev, torch.float32).reshape(m, 12).contiguous()
        state["X_ba"] = _f32_points(outputs["Xs_ba"], dev)
        return res

    if calibrated:
        # NOTE: as in the reference, "Rs" are R^T and "ts" the camera centres
        Rs_gt, ts_gt = decompose_camera_matrix(data.y.detach().cpu().numpy(), Ks)
        Rs_pred, ts_pred = decompose_camera_matrix(Ps_norm)
        outputs["Rs_gt"], outputs["ts_gt"] = Rs_gt, ts_gt
        outputs["Rs"], outputs["ts"] = Rs_pred, ts_pred
        outputs["cam_centers"], outputs["cam_centers_gt"] = ts_pred, ts_gt
        Rs_fixed, ts_fixed, sim = align_cameras(Rs_pred, Rs_gt, ts_pred, ts_gt, return_alignment=True)
        outputs["Rs_fixed"], outputs["ts_fixed"] = Rs_fixed, ts_fixed
        outputs["pts3D_pred_fixed"] = sim @ pts3D_pred
        outputs["pts3D_triangulated_fixed"] = sim @ pts3D_triangulated
        if bundle_adjustment:
            res = run_ba(lambda **kw: ba.euc_ba(None, Rs=Rs_pred, ts=ts_pred, Ks=np.linalg.inv(Ns), Ps=None, **kw))
            outputs["Rs_ba"], outputs["ts_ba"] = res["Rs"], res["ts"]
            R_ba_fixed, t_ba_fixed, sim = align_cameras(res["Rs"], Rs_gt, res["ts"], ts_gt, return_alignment=True)
            outputs["Rs_ba_fixed"], outputs["ts_ba_fixed"] = R_ba_fixed, t_ba_fixed
            outputs["Xs_ba_fixed"] = sim @ outputs["Xs_ba"]
    elif bundle_adjustment:
        run_ba(lambda **kw: ba.proj_ba(Ps=Ps, xs=None, normalize_in_tri=True, **kw))
    return outputs


def _nanmean_repro(state, P, X):
    tot = _native.colsum(_native.reproj_error(state["cam"], state["pt"], state["xy"], P, X, None))
    return float(tot[0] / tot[1])  # count 0 -> nan, as np.nanmean of an all-NaN array


_QUANTILES = (10, 25, 50, 75, 90)


def _quantiles(x):
    """np.quantile(x, 0.01 * [10, 25, 50, 75, 90]) (the default linear rule) of a per-edge device
    vector as a [5] float64 device tensor: one sort, then the two neighbours of h = (E - 1) q
    interpolated in fp64 the way numpy's lerp does.  A NaN anywhere gives NaN, as in numpy."""
    E = x.shape[0]
    if E == 0:
        return torch.full((5,), float("nan"), dtype=torch.float64, device=x.device)
    s = torch.sort(x).values  # NaN sorts last
    h = (E - 1) * (0.01 * np.array(_QUANTILES))
    lo = np.floor(h).astype(np.int64)
    t = torch.as_tensor(h - lo, dtype=torch.float64, device=x.device)
    a = s[torch.as_tensor(lo, device=x.device)].double()
    b = s[torch.as_tensor(np.minimum(lo + 1, E - 1), device=x.device)].double()
    q = torch.where(t >= 0.5, b - (b - a) * (1 - t), a + (b - a) * t)
    return torch.where(torch.isnan(s[-1]), torch.full_like(q, float("nan")), q)


def _norm_keys(prefix, suffix=""):
    return ([f"{prefix}_mean{suffix}"] + [f"{prefix}_q{q:02d}{suffix}" for q in _QUANTILES]
            + [f"{prefix}_min{suffix}", f"{prefix}_max{suffix}"])


def _depth_errors(state, two_view, pairing):
    """The depth head's keys of compute_errors (evaluation.py:241-301), in the reference's order;
    every number is reduced on the device and read in one copy."""
    dp, dg, scales = state["depths_pred"], state["depths_gt"], state["scales"]
    E = dp.shape[0]
    _, st = depth_eval.depth_norm_stats(dp, dg)
    vals = [st[0] / E, _quantiles(dp / scales[0]), st[1:3], st[3:4] / E, _quantiles(dg / scales[1]), st[4:6],
            st[6:7] / E]
    keys = _norm_keys("depth_pred_norm") + _norm_keys("depth_gt_norm") + ["depth_pred_err_mean"]
    if two_view:
        cam, pt = state["cam"], state["pt"]
        if pairing is None:
            src, _ = depth_eval.track_cycle(state["pt_ptr"], state["perm"], depth_eval.draw_keys(E, cam.device))
            check = None
        else:
            src, check = _pairing(pairing, E, cam.device), pt
        tot, _, rdepth = depth_eval.backproj_2view(cam, check, state["xy"], dp, scales[1] / scales[0], src,
                                                   state["camtab"], per_edge=True)
        rn = rdepth / scales[1].to(rdepth.dtype)  # back to the normalised depth scale
        vals += [tot[0:1].double() / tot[1:2].double(), rn.double().sum().view(1) / E if E else st[0:1],
                 rn.min().view(1).double() if E else st[1:2], rn.max().view(1).double() if E else st[2:3],
                 _quantiles(rn)]
        sfx = "_rnd_gt_2view"
        keys += ["repro_backproj" + sfx, "repro_backproj_depth_norm_mean" + sfx, "repro_backproj_depth_norm_min" + sfx,
                 "repro_backproj_depth_norm_max" + sfx] + [f"repro_backproj_depth_norm_q{q:02d}{sfx}"
                                                           for q in _QUANTILES]
    host = torch.cat([v.reshape(-1).double() for v in vals]).cpu().numpy()
    assert host.shape[0] == len(keys)
    return dict(zip(keys, host))


def compute_errors(outputs, conf, bundle_adjustment, pairing=None):
    calibrated, explicit = _heads(conf)
    depth_head, two_view = _depth_conf(conf)
    model_errors = {}
    state = outputs["_device"]
    if depth_head:
        model_errors.update(_depth_errors(state, two_view, pairing))
    if not explicit:
        return model_errors
    model_errors["our_repro"] = _nanmean_repro(state, state["P"], state["X"])
    model_errors["triangulated_repro"] = _nanmean_repro(state, state["P"], state["X_tri"])

    def pose_errors(Rs_fixed, ts_fixed, suffix):
        R_err, t_err = translation_rotation_errors(Rs_fixed, ts_fixed, outputs["Rs_gt"], outputs["ts_gt"])
        model_errors["t_err" + suffix + "_mean"] = np.mean(t_err)
        model_errors["t_err" + suffix + "_med"] = np.median(t_err)
        model_errors["R_err" + suffix + "_mean"] = np.mean(R_err)
        model_errors["R_err" + suffix + "_med"] = np.median(R_err)

    if calibrated:
        pose_errors(outputs["Rs_fixed"], outputs["ts_fixed"], "")
        for key in ("cam_centers", "cam_centers_gt"):
            C = outputs[key]
            # np.mean(..., keepdims=True) without an axis: the mean over ALL elements, as written
            # in the reference (evaluation.py:324-325)
            model_errors[key + "_std"] = np.mean(np.linalg.norm(C - np.mean(C, keepdims=True), axis=1))
    if bundle_adjustment:
        model_errors["repro_ba"] = _nanmean_repro(state, state["P_ba"], state["X_ba"])
        model_errors["ba_time"] = outputs["ba_time"]
        model_errors["ba_converged1"] = 1 if outputs["ba_converged1"] else 0
        if conf.get_bool("ba.repeat"):
            for k in _BA_REPEAT_KEYS:
                k = k.replace("repro_", "repro_ba_")
                model_errors[k] = outputs[k]
            model_errors["ba_converged2"] = 1 if outputs["ba_converged2"] else 0
        if calibrated:
            pose_errors(outputs["Rs_ba_fixed"], outputs["ts_ba_fixed"], "_ba")

    cam_neg, pt_neg, stats = _native.depth_stats(state["cam"], state["pt"], state["cam_ptr"], state["pt_ptr"],
                                                 state["perm"], state["P"], state["X"],
                                                 conf.get_float("loss.infinity_pts_margin"))
    flagged = torch.stack([cam_neg.sum(), pt_neg.sum()]).cpu().numpy().astype(np.float64)
    n_neg, n_views, _, d_sum, d_min, d_max = stats.cpu().numpy()
    E = np.float64(state["cam"].shape[0])
    # The reference computes n_pts as np.any(visible, axis=1).sum() (evaluation.py:357): the number
    # of non-empty VIEWS, not points, so fraction_points_neg_depth_in_any_view is divided by the
    # view count and can exceed 1.  A drop-in reports what the reference reports.
    n_pts = n_views
    with np.errstate(invalid="ignore", divide="ignore"):
        model_errors["fraction_views_neg_depth_for_any_point"] = flagged[0] / n_views
        model_errors["fraction_points_neg_depth_in_any_view"] = flagged[1] / n_pts
        model_errors["total_fraction_points_neg_depth"] = n_neg / E
        model_errors["point_depth_mean"] = d_sum / E
    model_errors["point_depth_min"] = d_min
    model_errors["point_depth_max"] = d_max
    return model_errors


def get_dummy_errors(conf, bundle_adjustment):
    """The keys compute_errors would set, all NaN (after an out-of-memory scene).  Like the
    reference's (evaluation.py:368-432) it has no ba_time and no cam_centers*_std."""
    calibrated, explicit = _heads(conf)
    keys = []
    # the depth keys come first and in the reference's dummy order (mean, min, max, quantiles), which
    # is not compute_errors' order; as there, each group follows its own conf key alone
    def dummy_norm(prefix, sfx=""):
        return [f"{prefix}_{k}{sfx}" for k in ("mean", "min", "max")] + [f"{prefix}_q{q:02d}{sfx}" for q in _QUANTILES]

    if conf.get_bool("eval.calc_reprojerr_with_gtposes_for_depth_pred", default=False):
        keys += ["repro_backproj_rnd_gt_2view"] + dummy_norm("repro_backproj_depth_norm", "_rnd_gt_2view")
    if conf.get_bool("model.depth_head.enabled", default=False):
        keys += dummy_norm("depth_pred_norm") + dummy_norm("depth_gt_norm") + ["depth_pred_err_mean"]
    if not explicit:
        return {k: np.nan for k in keys}
    pose = ("t_err{}_mean", "t_err{}_med", "R_err{}_mean", "R_err{}_med")
    keys += ["our_repro", "triangulated_repro"]
    if calibrated:
        keys += [k.format("") for k in pose]
    if bundle_adjustment:
        keys += ["repro_ba", "ba_converged1"]
        if conf.get_bool("ba.repeat"):
            keys += [k.replace("repro_", "repro_ba_") for k in _BA_REPEAT_KEYS] + ["ba_converged2"]
        if calibrated:
            keys += [k.format("_ba") for k in pose]
    keys += ["fraction_views_neg_depth_for_any_point", "fraction_points_neg_depth_in_any_view",
             "total_fraction_points_neg_depth", "point_depth_mean", "point_depth_min", "point_depth_max"]
    return {k: np.nan for k in keys}
