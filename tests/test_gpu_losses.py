"""The HIP ExpDepthRegularizedOSELoss (csrc/ose_loss.hip), its union-batch / captured-step form
(gasfm_ose_seg_fwd / _bwd, static_batch.batch_loss, StaticTrainer) and DirectDepthLoss
(csrc/depth_loss.hip) against the fp64 per-edge restatements of tests/test_losses_cpu.py, which that
file pins to the reference's dense formulation.

Tolerance, as tests/test_gpu_esfm_loss.py (fp32 kernel vs fp64 reference):
    loss:   |got - ref| <= 1e-5 |ref|
    grads:  ||got - ref|| <= 1e-4 ||ref|| per tensor (normwise), |got - ref| <= 1e-4 max|ref|
Inputs come from that file's ``predictions()``: y_z stays within a few units of 2, so exp(-y_z)
is far from fp32 overflow.  The trainer test uses tests/test_gpu_train_step.py's bounds: loss 1e-4,
gradients ||got - ref|| <= 1e-3 ||ref|| per tensor plus 1e-6 x the step's largest gradient norm.
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd import static_batch, synthetic
from gasfm_amd.loss import DirectDepthLoss, ExpDepthRegularizedOSELoss
from gasfm_amd.scene import SparseMat

from test_gpu_esfm_loss import close, predictions
from test_gpu_static_batch import _eager, _scenes
from test_gpu_train_step import conf_with_loss
from test_losses_cpu import depth_loss_edges, ose_loss_edges

pytestmark = pytest.mark.gpu


def ose_conf(w_reg):
    return gasfm_amd.Conf({"model": {"view_head": {"enabled": True}, "scenepoint_head": {"enabled": True}},
                           "loss": {"depth_regul_weight": w_reg}})


def depth_conf(cost_fcn):
    return gasfm_amd.Conf({"dataset": {"calibrated": True}, "model": {"depth_head": {"enabled": True}},
                           "loss": {"cost_fcn": cost_fcn}})


def run_ose(data, Ps, X, w_reg, dloss=1.0):
    Ps = Ps.detach().float().clone().requires_grad_(True)
    X = X.detach().float().clone().requires_grad_(True)
    loss = ExpDepthRegularizedOSELoss(ose_conf(w_reg))({"Ps_norm": Ps, "pts3D": X}, data)
    (loss * dloss).backward()
    return loss.detach(), Ps.grad, X.grad


def oracle_ose(Ps, X, cam, pt, vals, w_reg, dloss=1.0):
    Ps, X = Ps.double().clone().requires_grad_(True), X.double().clone().requires_grad_(True)
    loss = ose_loss_edges(Ps, X, cam, pt, vals.double(), w_reg)
    (loss * dloss).backward()
    return loss.detach(), Ps.grad, X.grad


@pytest.fixture(scope="module")
def config4_case(device):
    """One scaled config-4 edge list and predictions, shared and left unchanged."""
    sc = synthetic.scaled_config4(0.02, seed=5)
    Ps, X = predictions(sc.m, sc.n, 9, device)
    return sc, Ps, X, {}


@pytest.mark.parametrize("w_reg", [0.0, 0.1])
@pytest.mark.parametrize("max_piece", [None, 64])
def test_ose_scaled_config4_vs_fp64(device, config4_case, w_reg, max_piece):
    """Long camera segments (one workgroup per camera walks its edges in strides of 256) and ~20-edge
    points; dloss != 1; two runs bitwise equal."""
    sc, Ps, X, refs = config4_case
    data = gasfm_amd.SceneData.from_synthetic(sc, max_piece=max_piece).to(device)
    loss, dP, dX = run_ose(data, Ps, X, w_reg, dloss=0.75)
    if w_reg not in refs:
        refs[w_reg] = oracle_ose(Ps, X, data.x.indices[0], data.x.indices[1], data.x.values, w_reg, dloss=0.75)
    rl, rP, rX = refs[w_reg]
    print(f"ose w_reg={w_reg} max_piece={max_piece}: loss {loss.item():.9g} ref {rl.item():.9g}")
    np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-5)
    close(dP, rP, "dPs")
    close(dX, rX, "dpts3D")
    again = run_ose(data, Ps, X, w_reg, dloss=0.75)
    for u, v in zip((loss, dP, dX), again):
        assert torch.equal(u, v)


def test_ose_edge_cases(device):
    """The 5-edge hand scene of test_gpu_esfm_loss.test_edge_cases: r_e exactly 0 on edge 0 (the
    norm's gradient is 0 there, the exp term remains), camera 1 and point 2 without an edge (exactly
    zero gradients), camera 2 sees point 3 at y_z = -0.5 (finite, no barrier)."""
    cam = np.array([0, 0, 0, 2, 2], dtype=np.int64)
    pt = np.array([0, 1, 3, 0, 3], dtype=np.int64)
    vals = np.array([[0.0, 0.0], [0.1, -0.2], [0.3, 0.3], [0.5, 0.25], [-0.1, 0.0]], dtype=np.float32)
    m, n = 3, 4
    Ps = torch.zeros((m, 3, 4), dtype=torch.float64)
    Ps[:, :, :3] = torch.eye(3, dtype=torch.float64)
    Ps[2, 2, 3] = -1.5
    X = torch.tensor([[0.0, 1.0, 7.0, 0.5], [0.0, -1.0, 7.0, 0.5], [1.0, 2.0, 7.0, 1.0], [1.0, 1.0, 1.0, 1.0]],
                     dtype=torch.float64)
    data = gasfm_amd.SceneData.from_sparse(cam, pt, vals, m, n).to(device)
    for w_reg in (0.0, 0.1):
        loss, dP, dX = run_ose(data, Ps.to(device), X.to(device), w_reg, dloss=0.75)
        rl, rP, rX = oracle_ose(Ps, X, torch.from_numpy(cam), torch.from_numpy(pt), torch.from_numpy(vals), w_reg,
                                dloss=0.75)
        assert torch.isfinite(loss) and torch.isfinite(dP).all() and torch.isfinite(dX).all()
        np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-5)
        np.testing.assert_allclose(dP.cpu().numpy(), rP.numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(dX.cpu().numpy(), rX.numpy(), rtol=1e-5, atol=1e-7)
        assert float(dP[1].abs().max()) == 0.0 and float(dX[:, 2].abs().max()) == 0.0
    # w_reg = 0: edge 0 (r = 0) adds nothing, so point 0's gradient is camera 2's edge alone
    _, _, dX0 = run_ose(data, Ps.to(device), X.to(device), 0.0)
    keep = np.array([1, 2, 3, 4])
    d1 = gasfm_amd.SceneData.from_sparse(cam[keep], pt[keep], vals[keep], m, n).to(device)
    _, _, dX1 = run_ose(d1, Ps.to(device), X.to(device), 0.0, dloss=4.0 / 5.0)
    np.testing.assert_allclose(dX0[:, 0].cpu().numpy(), dX1[:, 0].cpu().numpy(), rtol=1e-6, atol=1e-9)


def test_ose_input_checks(device):
    data = gasfm_amd.SceneData.from_sparse(np.array([0, 1]), np.array([0, 0]), np.zeros((2, 2), np.float32), 2,
                                           1).to(device)
    lossf = ExpDepthRegularizedOSELoss(ose_conf(0.1))
    Ps, X = torch.zeros((2, 3, 4), device=device), torch.ones((4, 1), device=device)
    with pytest.raises(TypeError):
        lossf({"Ps_norm": Ps.cpu(), "pts3D": X}, data)
    with pytest.raises(ValueError):
        lossf({"Ps_norm": Ps.reshape(2, 12), "pts3D": X}, data)
    data.shard = object()
    with pytest.raises(ValueError, match="shard"):
        lossf({"Ps_norm": Ps, "pts3D": X}, data)


# ---------------------------------------------------------------- union batch, captured step
@pytest.fixture
def s2g_pieces(monkeypatch):
    monkeypatch.setattr(static_batch, "S2G_PIECES", 128)  # the test scenes have ~1-2k valid points


def _seg_check(sb, datas, lossf, device, seed):
    """batch_loss on the filled bucket against the sum of the single-scene losses on the same
    predictions; the pad scene's predictions are NaN: its gradient rows must be exact zeros."""
    c = sb.caps
    mo, no, _ = sb.offsets
    Ps, X = predictions(c.M, c.N, seed, device)
    Ps, X = Ps.float(), X.float()
    Ps[mo[-1]:] = float("nan")
    X[:, no[-1]:] = float("nan")
    P1, X1 = Ps.clone().requires_grad_(True), X.clone().requires_grad_(True)
    ref = sum(lossf({"Ps_norm": P1[mo[i]:mo[i + 1]], "pts3D": X1[:, no[i]:no[i + 1]]}, d)
              for i, d in enumerate(datas))
    (0.75 * ref).backward()
    P2, X2 = Ps.clone().requires_grad_(True), X.clone().requires_grad_(True)
    loss = static_batch.batch_loss({"Ps_norm": P2, "pts3D": X2}, sb, lossf)
    (0.75 * loss).backward()
    print(f"seg B={len(datas)}: loss {loss.item():.9g} ref {ref.item():.9g}")
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5)
    assert float(P2.grad[mo[-1]:].abs().max()) == 0.0 and float(X2.grad[:, no[-1]:].abs().max()) == 0.0
    assert not torch.isnan(P2.grad).any() and not torch.isnan(X2.grad).any()
    close(P2.grad[:mo[-1]], P1.grad[:mo[-1]], "dPs")
    close(X2.grad[:, :no[-1]], X1.grad[:, :no[-1]], "dpts3D")


@pytest.mark.parametrize("views", [(14,), (14, 16, 18)])
def test_ose_segmented_equals_sum_of_scenes(device, s2g_pieces, views):
    lossf = ExpDepthRegularizedOSELoss(ose_conf(0.1))
    datas = _scenes(device, views, seed=0)
    st = static_batch.BatchStats(datas)
    assert st.expressible() is None and len(set(st.Es)) == len(views)
    caps = static_batch.Caps.for_batch(st)
    sb = static_batch.StaticBatch(caps, device)
    sb.fill(datas, st)
    _seg_check(sb, datas, lossf, device, 11)
    if len(views) == 3:  # the same bucket refilled with other, smaller scenes
        datas = _scenes(device, (10, 12, 13), seed=1)
        st = static_batch.BatchStats(datas)
        assert caps.pad(st) is not None
        sb.fill(datas, st)
        _seg_check(sb, datas, lossf, device, 12)


def test_batch_loss_refuses_direct_depth_loss(device):
    with pytest.raises(TypeError, match="DirectDepthLoss"):
        static_batch.batch_loss({}, None, DirectDepthLoss(depth_conf("L1")))


def test_static_trainer_with_ose_loss(device, s2g_pieces):
    """Two steps of one StaticTrainer on a 2-scene batch (9-block conf): the bucket's step is
    captured, and each replay leaves the eager union step's loss and gradients."""
    torch.manual_seed(5)
    conf = conf_with_loss(gasfm_amd.optim_conf())
    conf.put("loss.depth_regul_weight", 0.1)
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = ExpDepthRegularizedOSELoss(conf)
    datas = _scenes(device, (12, 15), seed=3)
    _, loss_ref, g_ref, _ = _eager(net, lossf, datas)
    floor = 1e-6 * max(float(g.double().norm()) for g in g_ref if g is not None)
    trainer = static_batch.StaticTrainer(net, lossf)
    for k in range(2):
        loss, _ = trainer.step(datas)
        assert trainer.captures >= 1 and trainer.fallbacks == [] and trainer.eager_steps == 0
        assert next(iter(trainer.buckets.values()))[1].captured
        print(f"trainer step {k}: loss {float(loss):.9g} ref {loss_ref:.9g}")
        assert abs(float(loss) - loss_ref) <= 1e-4 * abs(loss_ref)
        for (name, p), b in zip(net.named_parameters(), g_ref):
            assert (p.grad is None) == (b is None), name
            if b is not None:
                err, nr = float((p.grad.double() - b.double()).norm()), float(b.double().norm())
                assert err <= 1e-3 * nr + floor, f"step {k} {name}: {err:.3e} / {nr:.3e}"
    assert trainer.captures == 1 and len(trainer.buckets) == 1


# ---------------------------------------------------------------- DirectDepthLoss
def _depth_scene(E, device, seed):
    """An E-edge scene (cameras of up to 7 points, the last one shorter) with dense [m, n] depth targets."""
    n = min(7, E)
    m = -(-E // n)
    e = np.arange(E)
    cam, pt = e // n, e % n
    g = torch.Generator().manual_seed(seed)
    data = gasfm_amd.SceneData.from_sparse(cam.astype(np.int64), pt.astype(np.int64),
                                           np.zeros((E, 2), np.float32), m, n).to(device)
    dense = (1.0 + 3.0 * torch.rand((m, n), generator=g, dtype=torch.float64)).float()
    a = (0.5 + 2.0 * torch.rand(E, generator=g, dtype=torch.float64)).float()
    return data, dense, a, torch.from_numpy(cam), torch.from_numpy(pt)


def run_depth(data, a, targets, cost_fcn, device, dloss=1.0):
    data.depths = targets
    v = a.to(device).reshape(-1, 1).clone().requires_grad_(True)
    x = data.x
    pred = {"depths": SparseMat(v, x.indices, x.cam_per_pts, x.pts_per_cam, [x.shape[0], x.shape[1], 1])}
    loss = DirectDepthLoss(depth_conf(cost_fcn))(pred, data)
    (loss * dloss).backward()
    return loss.detach(), v.grad[:, 0]


def oracle_depth(a, b, cost_fcn, dloss=1.0):
    a = a.double().clone().requires_grad_(True)
    loss = depth_loss_edges(a, b.double(), cost_fcn)
    (loss * dloss).backward()
    return loss.detach(), a.grad


@pytest.mark.parametrize("cost_fcn", ["L1", "L2"])
@pytest.mark.parametrize("E", [1, 1000])
def test_direct_depth_loss_vs_fp64(device, cost_fcn, E):
    """E = 1 (u = 0: zero loss and gradient) and E = 1000 = 3 workgroups of 256 + 232; dense [m, n]
    targets and the same targets per edge give identical results."""
    data, dense, a, cam, pt = _depth_scene(E, device, 21)
    b = dense[cam, pt]
    loss, da = run_depth(data, a, dense.to(device), cost_fcn, device, dloss=0.75)
    loss_e, da_e = run_depth(data, a, b.to(device), cost_fcn, device, dloss=0.75)
    assert torch.equal(loss, loss_e) and torch.equal(da, da_e)
    rl, ra = oracle_depth(a, b, cost_fcn, dloss=0.75)
    print(f"depth {cost_fcn} E={E}: loss {loss.item():.9g} ref {rl.item():.9g}")
    np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-5, atol=0)
    close(da, ra, "ddepths")


def test_direct_depth_loss_zero_residuals(device):
    """Equal scales and some equal depths: those u_e are exactly 0; L1 takes sign(0) = 0 as torch."""
    data, _, _, cam, pt = _depth_scene(6, device, 22)
    a = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    b = torch.tensor([1.0, 2.0, 4.0, 3.0, 5.0, 6.0])
    for cost_fcn in ("L1", "L2"):
        loss, da = run_depth(data, a, b.to(device), cost_fcn, device)
        rl, ra = oracle_depth(a, b, cost_fcn)
        np.testing.assert_allclose(loss.item(), rl.item(), rtol=1e-5)
        np.testing.assert_allclose(da.cpu().numpy(), ra.numpy(), rtol=1e-5, atol=1e-7)


def test_direct_depth_loss_reaches_the_depth_head(device):
    """GraphAttnSfMNet (2 blocks, reduced widths) with the depth head: one backward of
    DirectDepthLoss leaves finite, nonzero gradients on the depth head's weights."""
    torch.manual_seed(7)
    sc = synthetic.windowed_scene(12, 300, seed=31)
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    conf = gasfm_amd.conf.small_conf(2, depth_head={"enabled": True, "n_feat": 32, "n_hidden_layers": 2})
    conf.put("loss.cost_fcn", "L1")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    E = data.x.indices.shape[1]
    data.depths = 1.0 + 3.0 * torch.rand(E, device=device)
    pred = net(data)
    assert tuple(pred["depths"].values.shape) == (E, 1)
    loss = DirectDepthLoss(conf)(pred, data)
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in net.depth_head.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert all(float(g.abs().max()) > 0 for g in grads if g.dim() == 2)
