"""fp64 per-edge restatements of ExpDepthRegularizedOSELoss and DirectDepthLoss (the references of
tests/test_gpu_losses.py), pinned here to the reference's dense formulation, and get_loss_func.

``ose_loss_edges`` / ``depth_loss_edges`` are written from the formulas of code/loss_functions.py:24-66
and 126-150.  ``ose_loss_dense`` / ``depth_loss_dense`` write those forwards out as the reference
does (``Ps @ pts3D`` [m, 3, n], ``norm_M.reshape(m, 2, n)``, ``[valid_pts].mean()``; the dense depth
matrix indexed at the sparse indices).  A fixture made by the reference's own classes is not possible
without a GPU: both projection losses assert ``data.valid_pts.is_cuda``.
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd.loss import DirectDepthLoss, ESFMLoss, ExpDepthRegularizedOSELoss, get_loss_func


def ose_loss_edges(Ps, X, cam, pt, vals, w_reg):
    """mean over the edges of ||y_xy - y_z m_e|| + w_reg exp(-y_z), y_e = P_c [X_p; w_p]."""
    y = torch.einsum("eij,je->ei", Ps[cam], X[:, pt])
    r = y[:, :2] - y[:, 2:3] * vals
    return (r.norm(dim=1) + w_reg * torch.exp(-y[:, 2])).mean()


def depth_loss_edges(a, b, cost_fcn):
    """mean |a / mean a - b / mean b| (L1) or its square (L2)."""
    u = a / a.mean() - b / b.mean()
    return u.abs().mean() if cost_fcn == "L1" else (u ** 2).mean()


def ose_loss_dense(Ps, X, norm_M, valid_pts, w_reg):
    """ExpDepthRegularizedOSELoss.forward (code/loss_functions.py:138-150) written out."""
    pts_2d = Ps @ X  # [m, 3, n]
    depth_reg_term = w_reg * torch.exp(-pts_2d[:, 2, :])
    pts_2d_gt = norm_M.reshape(Ps.shape[0], 2, -1)
    ose_err = (pts_2d[:, :2, :] - pts_2d[:, [2], :] * pts_2d_gt).norm(dim=1)
    return (ose_err + depth_reg_term)[valid_pts].mean()


def depth_loss_dense(values, indices, depths_dense, cost_fcn):
    """DirectDepthLoss.forward (code/loss_functions.py:36-66) written out."""
    depths_pred = values.squeeze(1)
    depths_gt = depths_dense[indices[0, :], indices[1, :]]
    depths_pred = depths_pred / torch.mean(depths_pred)
    depths_gt = depths_gt / torch.mean(depths_gt)
    if cost_fcn == "L1":
        return torch.mean(torch.abs(depths_pred - depths_gt))
    return torch.mean((depths_pred - depths_gt) ** 2)


def hand_scene():
    """3 cameras x 4 points, camera 1 and point 2 without an observation."""
    cam = torch.tensor([0, 0, 0, 2, 2])
    pt = torch.tensor([0, 1, 3, 0, 3])
    g = torch.Generator().manual_seed(3)
    m, n = 3, 4
    Ps = torch.zeros((m, 3, 4), dtype=torch.float64)
    Ps[:, :, :3] = torch.eye(3, dtype=torch.float64) + 0.1 * torch.randn((m, 3, 3), generator=g, dtype=torch.float64)
    Ps[:, :, 3] = 0.3 * torch.randn((m, 3), generator=g, dtype=torch.float64)
    X = torch.randn((4, n), generator=g, dtype=torch.float64)
    X[2] += 2.0
    vals = 0.3 * torch.randn((cam.shape[0], 2), generator=g, dtype=torch.float64)
    return m, n, cam, pt, Ps, X, vals, g


@pytest.mark.parametrize("w_reg", [0.0, 0.1])
def test_ose_edges_equal_dense_formulation(w_reg):
    m, n, cam, pt, Ps, X, vals, g = hand_scene()
    valid = torch.zeros((m, n), dtype=torch.bool)
    valid[cam, pt] = True
    # the unobserved entries of norm_M hold anything: they are masked out
    M = torch.randn((m, 2, n), generator=g, dtype=torch.float64)
    M[cam, :, pt] = vals
    norm_M = M.reshape(2 * m, n)
    out = []
    for f in (lambda P, Y: ose_loss_edges(P, Y, cam, pt, vals, w_reg),
              lambda P, Y: ose_loss_dense(P, Y, norm_M, valid, w_reg)):
        P, Y = Ps.clone().requires_grad_(True), X.clone().requires_grad_(True)
        loss = f(P, Y)
        (0.75 * loss).backward()
        out.append((loss.detach(), P.grad, Y.grad))
    for a, b in zip(*out):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-12)
    assert float(out[0][1][1].abs().max()) == 0.0 and float(out[0][2][:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("cost_fcn", ["L1", "L2"])
def test_depth_edges_equal_dense_formulation(cost_fcn):
    m, n, cam, pt, _, _, _, g = hand_scene()
    indices = torch.stack([cam, pt])
    dense = 1.0 + torch.rand((m, n), generator=g, dtype=torch.float64)
    values = 0.5 + torch.rand((cam.shape[0], 1), generator=g, dtype=torch.float64)
    out = []
    for f in (lambda v: depth_loss_edges(v[:, 0], dense[cam, pt], cost_fcn),
              lambda v: depth_loss_dense(v, indices, dense, cost_fcn)):
        v = values.clone().requires_grad_(True)
        loss = f(v)
        (0.75 * loss).backward()
        out.append((loss.detach(), v.grad))
    for a, b in zip(*out):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-12)


def _conf(func, view=True, pts=True, depth=False, calibrated=True):
    return gasfm_amd.Conf({
        "dataset": {"calibrated": calibrated},
        "model": {"view_head": {"enabled": view}, "scenepoint_head": {"enabled": pts},
                  "depth_head": {"enabled": depth}},
        "loss": {"func": func, "infinity_pts_margin": 1e-4, "pts_grad_equalization_pre_perspective_divide": True,
                 "normalize_grad_wrt_valid_projections_only": True, "hinge_loss": True, "hinge_loss_weight": 1.0,
                 "depth_regul_weight": 0.1, "cost_fcn": "L1"}})


def test_get_loss_func_returns_the_named_class():
    assert gasfm_amd.get_loss_func is get_loss_func
    assert type(get_loss_func(_conf("ESFMLoss"))) is ESFMLoss
    ose = get_loss_func(_conf("ExpDepthRegularizedOSELoss"))
    assert type(ose) is ExpDepthRegularizedOSELoss and ose.depth_regul_weight == 0.1
    dep = get_loss_func(_conf("DirectDepthLoss", view=False, pts=False, depth=True))
    assert type(dep) is DirectDepthLoss and dep.cost_fcn == "L1"


@pytest.mark.parametrize("func,kw", [
    ("ESFMLoss", dict(depth=True)), ("ExpDepthRegularizedOSELoss", dict(depth=True)),
    ("ExpDepthRegularizedOSELoss", dict(view=False)), ("ExpDepthRegularizedOSELoss", dict(pts=False)),
    ("GTLoss", dict(depth=True)), ("DirectDepthLoss", dict(view=False, pts=False, depth=False)),
    ("DirectDepthLoss", dict(view=True, pts=False, depth=True)),
    ("DirectDepthLoss", dict(view=False, pts=True, depth=True))])
def test_get_loss_func_head_assertions(func, kw):
    with pytest.raises(AssertionError):
        get_loss_func(_conf(func, **kw))


def test_get_loss_func_gtloss_and_unknown_name():
    with pytest.raises(NotImplementedError, match="rot_to_quat"):
        get_loss_func(_conf("GTLoss"))
    with pytest.raises(AssertionError, match="Unknown loss function: NoSuchLoss"):
        get_loss_func(_conf("NoSuchLoss"))


def test_direct_depth_loss_constructor_checks():
    with pytest.raises(NotImplementedError):
        DirectDepthLoss(_conf("DirectDepthLoss", view=False, pts=False, depth=True, calibrated=False))
    with pytest.raises(AssertionError):
        DirectDepthLoss(_conf("DirectDepthLoss", view=False, pts=False, depth=False))
    bad = _conf("DirectDepthLoss", view=False, pts=False, depth=True).put("loss.cost_fcn", "L3")
    with pytest.raises(AssertionError):
        DirectDepthLoss(bad)


def test_ose_loss_constructor_checks():
    with pytest.raises(AssertionError):
        ExpDepthRegularizedOSELoss(_conf("ExpDepthRegularizedOSELoss", view=False))
    with pytest.raises(AssertionError):
        ExpDepthRegularizedOSELoss(_conf("ExpDepthRegularizedOSELoss", pts=False))
