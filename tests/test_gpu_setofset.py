"""The fused set-of-set kernels (csrc/setofset.hip) and SetOfSetNet on the MI355X against the
fp64 torch-op composite path and the reference fixture (tests/golden/setofset.npz)."""
import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import check_grad, golden
from gasfm_amd import _native, setofset, synthetic
from gasfm_amd.conf import dpesfm_conf
from gasfm_amd.graph_step import CapturedStep
from gasfm_amd.loss import ESFMLoss
from oracle.weights import deterministic_state_dict
from test_setofset_cpu import VARIANTS, check_against_fixture, fixture_net, run_linear_loss

pytestmark = pytest.mark.gpu

OUT_ATOL, OUT_RTOL = 1e-4, 1e-3
M_CAMS, N_PTS = 7, 300


def hand_scene(E, max_piece=4, seed=0):
    """7 cameras x 300 points, E edges: camera 0 has no edges, camera 1 exactly one (point 0), point 0 is
    seen by every camera that has edges, points 260..279 by camera 2 alone, points 280..299 by none;
    max_piece = 4 splits every camera but 0 / 1 and every point seen by more than 4 cameras."""
    rng = np.random.default_rng(seed)
    sizes = {2: 200, 3: 200, 4: 200, 5: 200}
    sizes[6] = E - 1 - sum(sizes.values())
    assert 1 <= sizes[6] <= 259
    cam, pt = [1], [0]
    for c in range(2, 7):
        own = list(range(260, 280)) if c == 2 else []
        k = sizes[c] - 1 - len(own)
        pts = sorted([0] + own + list(rng.choice(np.arange(1, 260), size=k, replace=False)))
        cam += [c] * len(pts)
        pt += pts
    cam, pt = np.asarray(cam, np.int64), np.asarray(pt, np.int64)
    assert cam.shape[0] == E
    vals = rng.standard_normal((E, 2)).astype(np.float32)
    return gasfm_amd.SceneData.from_sparse(cam, pt, vals, M_CAMS, N_PTS, max_piece=max_piece)


ROW_TILE = 128  # gasfm_sos_row_tile of every output wider than 2
SCENE_EDGES = (8 * ROW_TILE + 1, 8 * ROW_TILE - 1)
_SCENES = {}


def scene_edges(E, device):
    if E not in _SCENES:
        data = hand_scene(E).to(device)
        _SCENES[E] = (data, setofset.scene_edge_index(data, device))
    return _SCENES[E][1]


def test_row_tile_is_what_the_scene_sizes_assume():
    assert _native.sos_row_tile(256) == ROW_TILE and _native.sos_row_tile(32) == ROW_TILE
    assert _native.sos_row_tile(2) == 256 and SCENE_EDGES[0] % 256 == 1


def test_hand_scene_has_the_edge_cases(device):
    e = scene_edges(SCENE_EDGES[0], device)
    pp, pc = e.plans["proj2scenepoint"], e.plans["proj2view"]
    degc, degp = pc.segment_lengths(), pp.segment_lengths()
    assert degc[0] == 0 and degc[1] == 1 and degp[0] == 6 and (degp[280:] == 0).all() and (degp[260:280] == 1).all()
    assert pp.n_combine > 0 and pc.n_combine > 0 and pp.perm is not None and pc.perm is None


@pytest.mark.parametrize("E", SCENE_EDGES)
@pytest.mark.parametrize("D", [2, 32, 256])
def test_segment_means_match_fp64(device, D, E):
    edges = scene_edges(E, device)
    X = torch.randn(E, D, device=device)
    mp, mc = setofset.segment_means(X, edges)
    rp, rc, _ = setofset._composite_means(X.double(), edges)
    torch.testing.assert_close(mp.double(), rp, atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(mc.double(), rc, atol=1e-6, rtol=1e-5)
    assert not mc[0].any() and not mp[280:].any()
    # masked sums (the backward's dS / dV): rows masked by Ym > 0, scaled
    Ym = torch.randn(E, D, device=device)
    got = _native.sos_segment_sum(edges.plans["proj2scenepoint"], X, 0.25, mask=Ym)
    ref = torch.zeros(N_PTS, D, dtype=torch.float64, device=device).index_add(
        0, edges.pt.long(), 0.25 * (X * (Ym > 0)).double())
    torch.testing.assert_close(got.double(), ref, atol=1e-6, rtol=1e-5)


def layer_pair(d_in, d_out, device, seed=0):
    torch.manual_seed(seed)
    layer = setofset.SetOfSetLayer(d_in, d_out)
    return layer.to(device), [p.detach().clone() for p in layer.parameters()]


def layer_run(layer, X, edges, center, relu, R, C, composite):
    for p in layer.parameters():
        p.grad = None
    X = X.clone().requires_grad_(True)
    R = None if R is None else R.clone().requires_grad_(True)
    Y = layer(X, edges, center=center, relu=relu, residual=R, composite=composite)
    (Y * C).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in layer.named_parameters()}
    grads["X"] = X.grad
    if R is not None:
        grads["R"] = R.grad
    return Y.detach(), grads


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("act", [False, True], ids=["plain", "center_relu"])
@pytest.mark.parametrize("d_in,d_out", [(2, 256), (256, 256), (256, 128), (32, 32)])
def test_edge_update_matches_fp64(device, d_in, d_out, act, skip):
    """One layer, forward and every gradient (dX, dW, db, the S / V / g paths through their linears)
    against the fp64 composite, with the fp32 composite's own error as check_grad's ref32."""
    E = SCENE_EDGES[0] if (d_in + d_out) % 64 == 0 else SCENE_EDGES[1]
    edges = scene_edges(E, device)
    layer, _ = layer_pair(d_in, d_out, device, seed=d_in + d_out)
    torch.manual_seed(1)
    X = torch.randn(E, d_in, device=device)
    R = torch.randn(E, d_out, device=device) if skip else None
    C = torch.randn(E, d_out, device=device)
    with _native.dispatch_record() as rec:
        Y, g = layer_run(layer, X, edges, act, act, R, C, composite=False)
    assert rec.counts["sos_edge_fwd"] == 1 and rec.counts["sos_edge_dx"] == 1 and rec.counts["sos_edge_dw"] == 1
    assert rec.counts["sos_segsum"] == 4
    Y32, g32 = layer_run(layer, X, edges, act, act, R, C, composite=True)
    l64 = layer.double()
    Y64, g64 = layer_run(l64, X.double(), edges, act, act, None if R is None else R.double(), C.double(), True)
    layer.float()
    torch.testing.assert_close(Y.double(), Y64, atol=OUT_ATOL, rtol=OUT_RTOL)
    for k in g64:
        check_grad(g[k], g64[k].cpu().numpy(), f"{d_in}->{d_out} {k}", ref32=g32[k].double().cpu().numpy())


def test_outputs_stay_inside_their_rows(device):
    """Forward and dX written into NaN-filled buffers with guard rows before and after: the guards
    stay NaN (the ABI's outputs are contiguous, so there are no guard columns)."""
    E, G = SCENE_EDGES[0], 3
    edges = scene_edges(E, device)
    for d_in, d_out in ((2, 256), (256, 128)):
        X, W = torch.randn(E, d_in, device=device), torch.randn(d_out, d_in, device=device)
        S, V = torch.randn(N_PTS, d_out, device=device), torch.randn(M_CAMS, d_out, device=device)
        buf = torch.full((E + 2 * G, d_out), float("nan"), device=device)
        Y = _native.sos_edge_fwd(X, W, edges.cam, edges.pt, S, V, None, None, False, out=buf[G:G + E])
        ref = 0.25 * (X.double() @ W.double().t() + S.double()[edges.pt.long()] + V.double()[edges.cam.long()])
        torch.testing.assert_close(Y.double(), ref, atol=OUT_ATOL, rtol=OUT_RTOL)
        assert buf[:G].isnan().all() and buf[G + E:].isnan().all() and not buf[G:G + E].isnan().any()
        dY = torch.randn(E, d_out, device=device)
        A, B = torch.randn(M_CAMS, d_in, device=device), torch.randn(N_PTS, d_in, device=device)
        buf = torch.full((E + 2 * G, d_in), float("nan"), device=device)
        dX = _native.sos_edge_dx(dY, Y, W, edges.cam, edges.pt, A, B, E, d_in, out=buf[G:G + E])
        ref = (0.25 * dY * (Y > 0)).double() @ W.double() + A.double()[edges.cam.long()] + B.double()[edges.pt.long()]
        torch.testing.assert_close(dX.double(), ref, atol=OUT_ATOL, rtol=OUT_RTOL)
        assert buf[:G].isnan().all() and buf[G + E:].isnan().all() and not buf[G:G + E].isnan().any()


def test_nan_in_one_edge_row_stays_with_its_camera_and_point(device):
    """A NaN in one edge row of X reaches its own row of Y and, through the segment means, the rows of
    its camera and of its point, and no other row.  The global row is left out altogether (centring
    off, no lin_global term): a zeroed lin_global would still multiply the NaN mean, and 0 * NaN is
    NaN in the reference's Linear as well, so it cannot be switched off by its weights."""
    E = SCENE_EDGES[0]
    edges = scene_edges(E, device)
    torch.manual_seed(2)
    X = torch.randn(E, 256, device=device)
    W, Wsp, Wv = (torch.randn(256, 256, device=device) / 16 for _ in range(3))
    bad = 700
    X[bad, 5] = float("nan")
    mp, mc = setofset.segment_means(X, edges)
    c, p = int(edges.cam[bad]), int(edges.pt[bad])
    assert mp[p].isnan().any() and mc[c].isnan().any()
    assert int(mp.isnan().any(dim=1).sum()) == 1 and int(mc.isnan().any(dim=1).sum()) == 1
    Y = _native.sos_edge_fwd(X, W, edges.cam, edges.pt, mp @ Wsp.t(), mc @ Wv.t(), None, None, True)
    touched = (edges.cam == c) | (edges.pt == p)
    assert int(touched.sum()) > 1 and Y[bad].isnan().all()
    assert Y[touched].isnan().all()
    assert not Y[~touched].isnan().any()


def gpu_config1(device, device_built=False):
    sc = synthetic.config1()
    M, Ns, Ps = torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()), torch.from_numpy(sc.Ps_gt())
    if device_built:
        from gasfm_amd.scene_device import scene_from_dense_device
        return scene_from_dense_device(M.to(device), Ns.to(device), Ps.to(device), "synthetic_config1")
    return gasfm_amd.SceneData(M, Ns, Ps, "synthetic_config1").to(device)


@pytest.mark.parametrize("device_built", [False, True], ids=["host_scene", "device_scene"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_model_matches_reference_fixture(device, name, device_built):
    f = golden("setofset.npz")
    net = fixture_net(f, name, torch.float32, device)
    with _native.dispatch_record() as rec:
        outs, grads = run_linear_loss(net, gpu_config1(device, device_built), f, torch.float32)
    assert rec.counts["sos_edge_fwd"] == sum(len(b.layers) for b in net.equivariant_blocks)
    check_against_fixture(f, name, outs, grads, torch.float32)


def full_width_net(device):
    net = gasfm_amd.SetOfSetNet(dpesfm_conf())
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    return net.to(device)


_FULL = {}


def full_width_case(device):
    """The shipped conf at width 256 on windowed_scene(12, 600): fused run, fp32 and fp64 composite runs
    (computed once, shared)."""
    if not _FULL:
        sc = synthetic.windowed_scene(12, 600)
        data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
        net = full_width_net(device)
        torch.manual_seed(5)
        cP, cX = torch.randn(sc.m, 3, 4, device=device), torch.randn(4, sc.n, device=device)

        def run(dtype, composite):
            net.to(dtype)
            net.composite = composite
            data.x.values = data.x.values.to(dtype)
            for p in net.parameters():
                p.grad = None
            pred = net(data)
            ((pred["Ps_norm"] * cP.to(dtype)).sum() + (pred["pts3D"] * cX.to(dtype)).sum()).backward()
            return ({k: v.detach().clone() for k, v in pred.items()},
                    {k: p.grad.detach().clone() for k, p in net.named_parameters()})

        _FULL["c64"] = run(torch.float64, True)
        _FULL["c32"] = run(torch.float32, True)
        _FULL["f1"] = run(torch.float32, False)
        _FULL["f2"] = run(torch.float32, False)
        net.composite = False
        _FULL["net"], _FULL["data"], _FULL["coef"] = net, data, (cP, cX)
    return _FULL


def test_full_width_model_matches_fp64_composite(device):
    case = full_width_case(device)
    (o, g), (o32, g32), (o64, g64) = case["f1"], case["c32"], case["c64"]
    for k in o64:
        torch.testing.assert_close(o[k].double(), o64[k], atol=OUT_ATOL, rtol=OUT_RTOL)
    for k in g64:
        check_grad(g[k], g64[k].cpu().numpy(), k, ref32=g32[k].double().cpu().numpy())


def test_two_runs_are_bitwise_equal(device):
    case = full_width_case(device)
    (o1, g1), (o2, g2) = case["f1"], case["f2"]
    assert all(torch.equal(o1[k], o2[k]) for k in o1)
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])]


def test_empty_scene_on_the_device(device):
    net = full_width_net(device)
    d0 = gasfm_amd.SceneData.from_sparse(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 2), np.float32),
                                         3, 5).to(device)
    pred = net(d0)
    assert tuple(pred["Ps_norm"].shape) == (3, 3, 4) and tuple(pred["pts3D"].shape) == (4, 5)
    assert all(bool(torch.isfinite(v).all()) for v in pred.values())
    (pred["Ps_norm"].sum() + pred["pts3D"].sum()).backward()
    for k, p in net.named_parameters():
        if "lin_proj" in k and k.endswith("weight"):
            assert p.grad is not None and not p.grad.any(), k


def test_captured_step_replays_the_eager_gradients(device):
    case = full_width_case(device)
    net, data, (cP, cX) = case["net"], case["data"], case["coef"]

    def fwd_bwd():
        pred = net(data)
        loss = (pred["Ps_norm"] * cP).sum() + (pred["pts3D"] * cX).sum()
        loss.backward()
        return loss

    step = CapturedStep(fwd_bwd, list(net.parameters()))
    assert step.fallback_reason is None and step.captured
    step()
    torch.cuda.synchronize()
    g1 = case["f1"][1]
    bad = [k for k, p in net.named_parameters() if not torch.equal(p.grad, g1[k])]
    assert not bad, bad


def test_training_step_with_esfm_loss_and_adam(device):
    from gasfm_amd import evaluation
    sc = synthetic.windowed_scene(12, 600)
    conf = dpesfm_conf()
    conf.put("loss", {"infinity_pts_margin": 1e-4, "pts_grad_equalization_pre_perspective_divide": True,
                      "normalize_grad_wrt_valid_projections_only": False, "hinge_loss": True,
                      "hinge_loss_weight": 1.0})
    conf.put("eval.calc_reprojerr_with_gtposes_for_depth_pred", False)
    data = gasfm_amd.SceneData(torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()),
                               torch.from_numpy(sc.Ps_gt()), "train").to(device)
    losses = {}
    for composite in (True, False):
        net = full_width_net(device)
        net.composite = composite
        opt = gasfm_amd.optim.Adam(net.parameters(), lr=1e-4)
        pred = net(data)
        loss = ESFMLoss(conf)(pred, data)
        assert np.isfinite(evaluation.compute_core_errors(data, pred, conf)["our_repro"])
        loss.backward()
        opt.step()
        losses[composite] = float(loss.detach())
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert np.isfinite(losses[False])
    np.testing.assert_allclose(losses[False], losses[True], rtol=1e-3)


@pytest.mark.parametrize("width", [32, 128, 256, 48])
def test_dispatch_by_width(device, width):
    """Widths 2 (every first layer), 32, 128, 256 run the fused kernels; 48 takes the composite path;
    all match the fp64 composite."""
    sc = synthetic.config1()
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    net = gasfm_amd.SetOfSetNet(dpesfm_conf(num_features=width))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.to(device)
    with _native.dispatch_record() as rec:
        pred = net(data)
        (pred["Ps_norm"].sum() + pred["pts3D"].sum()).backward()
    if width == 48:
        assert rec.counts["sos_edge_fwd"] == 0 and rec.counts["sos_edge_dw"] == 0
    else:  # 3 layers: 2 -> w, w -> w, w -> w; the first layer's input needs no gradient
        assert rec.counts["sos_edge_fwd"] == 3 and rec.counts["sos_edge_dw"] == 3
        assert rec.counts["sos_edge_dx"] == 2 + 1  # + the final update's gather-only launch
    net.double()
    net.composite = True
    data.x.values = data.x.values.double()
    ref = net(data)
    for k in ref:
        torch.testing.assert_close(pred[k].detach().double(), ref[k].detach(), atol=OUT_ATOL, rtol=OUT_RTOL)
