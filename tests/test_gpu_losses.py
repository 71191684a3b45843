"""The HIP ExpDepthRegularizedOSELoss (csrc/ose_loss.hip), its union-batch / captured-step form
(gasfm_ose_seg_fwd / _bwd, static_batch.batch_loss, StaticTrainer) and DirectDepthLoss
(csrc/depth_loss.hip) against the fp64 per-edge restatements of tests/test_losses_cpu.py, which that
file pins to the reference's dense formulation; and the per-edge scaffold the ESFM and OSE kernels
share (csrc/edge_loss.hpp) on hand-made plans.

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
from gasfm_amd import _native, static_batch, synthetic
from gasfm_amd.loss import DirectDepthLoss, ExpDepthRegularizedOSELoss
from gasfm_amd.scene import SparseMat

from test_gpu_esfm_loss import VARIANTS, close, oracle_run, predictions
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


# ---------------------------------------------------------------- the shared per-edge scaffold
HAND_M, HAND_N, HAND_DLOSS, HAND_WREG = 4, 259, 0.75, 0.1
HAND_WEIGHTS = (1.0, 0.0, 0.5)  # of the three copies of a plan in the segmented form
HAND_ESFM = VARIANTS[0]  # (margin, equalize, valid_only, hinge, hinge_w): equalize + valid_only
# Points seen by each of the 4 cameras, edges in camera-major order.  "perm": 0, 1, 257 and 64 edges
# (an empty range, a single lane, one lap past the 256-thread workgroup, exactly one wave); edge 0
# sees point 5, so the point CSR needs a non-identity perm.  "sorted": camera-major edges that are
# also point-sorted (perm = None), which 259 points allow with 0, 1, 257 and 2 edges.  Both: 259
# points = one full point workgroup + 3 threads, point 258 has no edge.
HAND_PLANS = {"perm": [[], [5], range(257), range(194, 258)], "sorted": [[], [0], range(257), [256, 257]]}


def _hand_case(name, seed, device):
    counts = [len(p) for p in HAND_PLANS[name]]
    cam = np.repeat(np.arange(HAND_M), counts)
    pt = np.concatenate([np.asarray(p, dtype=np.int64) for p in HAND_PLANS[name]])
    perm = np.argsort(pt, kind="stable")
    assert (name == "sorted") == bool((perm == np.arange(len(pt))).all())
    cam_ptr = np.concatenate([[0], np.cumsum(counts)])
    pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=HAND_N))])
    assert pt_ptr[-1] == pt_ptr[-2] == len(pt)
    Ps, X = predictions(HAND_M, HAND_N, seed, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    vals = (0.5 * torch.randn((len(pt), 2), generator=g, dtype=torch.float64)).float()
    cam_t, pt_t = torch.from_numpy(cam), torch.from_numpy(pt)
    # the fp64 reference stays away from the kinks: no depth within 1e-3 of the margin (fp32 roundoff
    # of y_z is ~1e-6), both sides of it present, no residual below 1e-3
    y = torch.einsum("eij,je->ei", Ps[cam_t], X[:, pt_t])
    margin, eq, vo, hinge, w = HAND_ESFM
    pos = y[:, 2] >= margin
    assert float((y[:, 2] - margin).abs().min()) > 1e-3 and pos.any() and not pos.all()
    assert float((y[pos, :2] / y[pos, 2:3] - vals[pos]).norm(dim=1).min()) > 1e-3
    assert float((y[:, :2] - y[:, 2:3] * vals).norm(dim=1).min()) > 1e-3
    # per scene weight: the equalized gradient is normalised per edge, so it is not linear in the weight
    refs = {}
    for sw in HAND_WEIGHTS:
        if sw != 0:
            refs["esfm", sw] = oracle_run(Ps, X, cam_t, pt_t, vals, HAND_ESFM, dloss=HAND_DLOSS * sw)
            refs["ose", sw] = oracle_ose(Ps, X, cam_t, pt_t, vals, HAND_WREG, dloss=HAND_DLOSS * sw)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=torch.int32)
    return {"cam": i32(cam), "pt": i32(pt), "cam_ptr": i32(cam_ptr), "pt_ptr": i32(pt_ptr),
            "perm": None if name == "sorted" else i32(perm), "vals": vals.to(device),
            "P": Ps.float().reshape(HAND_M, 12).to(device), "X": X.float().to(device),
            "refs": {k: tuple(t.detach() for t in v) for k, v in refs.items()}, "npos": int(pos.sum())}


@pytest.fixture(scope="module")
def hand_cases(device):
    """The two hand-made plans with their fp64 autograd references, shared and left unchanged."""
    return {"perm": _hand_case("perm", 41, device), "sorted": _hand_case("sorted", 43, device)}


def _hand_run(loss, c, P, X, seg=None):
    """(loss [1] or 0-d, tot, dP, dX) through the _native wrappers, dloss = HAND_DLOSS; ``seg`` =
    (eoff, scene_of_cam, scene_of_pt, weight) runs the union-batch pair."""
    margin, eq, vo, hinge, w = HAND_ESFM
    dP, dX = torch.full_like(P, 7.0), torch.full_like(X, 7.0)
    dloss = torch.full((1,), HAND_DLOSS, device=P.device)
    edges, csr, E = (c["cam"], c["pt"], c["vals"]), (c["cam_ptr"], c["pt_ptr"], c["perm"]), c["cam"].shape[0]
    if seg is None and loss == "esfm":
        part = torch.empty((_native.esfm_part_rows(E), 2), device=P.device)
        _native.esfm_fwd(*edges, P, X, margin, w, hinge, part)
        tot = _native.colsum(part)
        _native.esfm_bwd(*csr, *edges, P, X, margin, w, hinge, eq, vo, dloss, tot, dP, dX)
        return tot[0] / E, tot, dP, dX
    if seg is None:
        tot = _native.colsum(_native.ose_fwd(*edges, P, X, HAND_WREG))
        _native.ose_bwd(*csr, *edges, P, X, HAND_WREG, dloss, dP, dX)
        return tot[0] / E, tot, dP, dX
    eoff, soc, sop, weight = seg
    if loss == "esfm":
        out, tot = _native.esfm_seg_fwd(*edges, eoff, weight, P, X, margin, w, hinge)
        _native.esfm_seg_bwd(*csr, *edges, eoff, soc, sop, weight, P, X, margin, w, hinge, eq, vo, dloss, tot, dP, dX)
    else:
        out, tot = _native.ose_seg_fwd(*edges, eoff, weight, P, X, HAND_WREG)
        _native.ose_seg_bwd(*csr, *edges, eoff, soc, sop, weight, P, X, HAND_WREG, dloss, dP, dX)
    return out[0], tot, dP, dX


def _hand_union(c, weights):
    """len(weights) copies of a hand case as one union batch; the predictions of the weight-0 copies are NaN."""
    S, E, dev = len(weights), c["cam"].shape[0], c["P"].device
    rep = lambda v, step: torch.cat([v + s * step for s in range(S)])
    ptr = lambda v: torch.cat([v[:-1] + s * E for s in range(S)] + [v.new_tensor([S * E])])
    u = {"cam": rep(c["cam"], HAND_M), "pt": rep(c["pt"], HAND_N), "vals": c["vals"].repeat(S, 1),
         "cam_ptr": ptr(c["cam_ptr"]), "pt_ptr": ptr(c["pt_ptr"]),
         "perm": None if c["perm"] is None else rep(c["perm"], E)}
    P, X = c["P"].repeat(S, 1), c["X"].repeat(1, S)
    for s, w in enumerate(weights):
        if w == 0:
            P[s * HAND_M:(s + 1) * HAND_M] = float("nan")
            X[:, s * HAND_N:(s + 1) * HAND_N] = float("nan")
    arange = torch.arange(S, dtype=torch.int32, device=dev)
    seg = (arange.new_tensor([s * E for s in range(S + 1)]), arange.repeat_interleave(HAND_M),
           arange.repeat_interleave(HAND_N), torch.tensor(weights, dtype=torch.float32, device=dev))
    return u, P, X, seg


@pytest.mark.parametrize("form", ["flat", "segmented"])
@pytest.mark.parametrize("loss", ["esfm", "ose"])
def test_edge_scaffold_hand_plans_vs_fp64(device, hand_cases, loss, form):
    """Every branch of the shared per-edge scaffold (csrc/edge_loss.hpp) at its smallest size, for a
    two-stat term with the equalized gradient and a one-stat term: HAND_PLANS, with and without a
    point perm, against fp64 autograd of the same per-edge formula.  Segmented: three copies with
    weights (1, 0, 0.5); the weight-0 copy's predictions are NaN and its gradients exact zeros, the
    total is the weighted sum of the flat losses (to the loss tolerance: 32 slices per scene against
    2 workgroups + colsum order the sums differently), and a copy's gradients are those of
    weight x loss (the equalized gradient is normalised per edge, so not the weight x the gradients)."""
    for name, c in hand_cases.items():
        rl, rP, rX = c["refs"][loss, 1.0]
        fl, ftot, fP, fX = _hand_run(loss, c, c["P"], c["X"])
        if form == "flat":
            print(f"hand {loss} {name}: loss {fl.item():.9g} ref {rl.item():.9g}")
            np.testing.assert_allclose(fl.item(), rl.item(), rtol=1e-5)
            close(fP, rP.reshape(HAND_M, 12), "dPs")
            close(fX, rX, "dpts3D")
            assert float(fP[0].abs().max()) == 0.0 and float(fX[:, -1].abs().max()) == 0.0
            if loss == "esfm":
                assert ftot[1].item() == c["npos"]
            continue
        weights = HAND_WEIGHTS
        u, P, X, seg = _hand_union(c, weights)
        sl, stot, sP, sX = _hand_run(loss, u, P, X, seg)
        print(f"hand {loss} {name} segmented: loss {sl.item():.9g} flat {fl.item():.9g} ref {rl.item():.9g}")
        np.testing.assert_allclose(sl.item(), sum(weights) * rl.item(), rtol=1e-5)
        np.testing.assert_allclose(sl.item(), sum(w * fl.item() for w in weights), rtol=1e-5)
        for s, w in enumerate(weights):
            gP, gX = sP[s * HAND_M:(s + 1) * HAND_M], sX[:, s * HAND_N:(s + 1) * HAND_N]
            if w == 0:
                assert float(gP.abs().max()) == 0.0 and float(gX.abs().max()) == 0.0
                continue
            close(gP, c["refs"][loss, w][1].reshape(HAND_M, 12), f"dPs scene {s}")
            close(gX, c["refs"][loss, w][2], f"dpts3D scene {s}")
            assert float(gP[0].abs().max()) == 0.0 and float(gX[:, -1].abs().max()) == 0.0
            if loss == "esfm":
                assert stot[s, 1].item() == c["npos"]


def test_ose_input_checks(device, hand_cases):
    # a segmented wrapper validates its index tensors; float2 reads need 8-byte aligned values
    c = hand_cases["perm"]
    u, P, X, seg = _hand_union(c, (1.0,))
    with pytest.raises(TypeError, match="cam"):
        _native.ose_seg_fwd(u["cam"].long(), u["pt"], u["vals"], seg[0], seg[3], P, X, HAND_WREG)
    E = c["cam"].shape[0]
    odd = torch.zeros(2 * E + 1, device=device)[1:].view(E, 2)
    assert odd.is_contiguous() and odd.data_ptr() % 8 == 4
    margin, eq, vo, hinge, w = HAND_ESFM
    dP, dX = torch.full_like(c["P"], 7.0), torch.full_like(c["X"], 7.0)
    one, tot = torch.ones(1, device=device), torch.ones(2, device=device)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        _native.esfm_bwd(c["cam_ptr"], c["pt_ptr"], c["perm"], c["cam"], c["pt"], odd, c["P"], c["X"], margin, w,
                         hinge, eq, vo, one, tot, dP, dX)
    assert float(dP.min()) == 7.0 and float(dX.min()) == 7.0  # nothing was launched

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
