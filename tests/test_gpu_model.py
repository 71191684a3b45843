"""End-to-end parity of gasfm_amd.GraphAttnSfMNet on the MI355X against the oracle / fixtures.

Tolerance (fp32 network vs fp64 reference):
    outputs:  |got - ref| <= 1e-4 + 1e-3 * |ref|  (Ps_norm, pts3D after 9-12 LN-heavy blocks)
    grads:    ||got - ref|| <= 1e-3 ||ref|| per parameter tensor (normwise: fp32 sums over
              up to E edges), and elementwise |got - ref| <= 1e-3 max|ref| + 1e-2 |ref|
The measured fp32-vs-fp64 gap of the reference itself on these fixtures is
<= 1e-6 (net_learning12.npz: Ps_norm_fp32 vs Ps_norm), so the bounds are >= 100x it.
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import check_grad, golden
from oracle import gasfm_ref, scenes
from oracle.weights import deterministic_state_dict

pytestmark = pytest.mark.gpu

OUT_ATOL, OUT_RTOL = 1e-4, 1e-3


def scene_from_fixture(device):
    s = golden("scene_config1.npz")
    data = gasfm_amd.SceneData(torch.from_numpy(s["M"]), torch.from_numpy(s["Ns"]), None, "config1")
    return s, data.to(device)


def test_scene_build_matches_reference():
    s, data = scene_from_fixture("cpu")
    np.testing.assert_array_equal(data.x.indices.numpy(), s["indices"])
    np.testing.assert_allclose(data.x.values.numpy(), s["values"], atol=1e-7)
    for name, key in (("proj2view", "p2v_edge_index"), ("proj2scenepoint", "p2s_edge_index")):
        np.testing.assert_array_equal(data.graph_wrappers[name].edge_index.numpy(), s[key])


def test_net_small_forward_backward(device):
    f = golden("net_small.npz")
    _, data = scene_from_fixture(device)
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.conf.small_conf(2))
    sd = {k[3:]: torch.from_numpy(f[k]).float() for k in f.files if k.startswith("sd/")}
    net.load_state_dict(sd)
    net = net.to(device)
    pred = net(data)
    # every hub output handed between the blocks (model.BlockCarry) was consumed
    assert net.last_carry is not None and net.last_carry.pending() == []
    np.testing.assert_allclose(pred["Ps_norm"].detach().cpu().numpy(), f["Ps_norm"], atol=OUT_ATOL, rtol=OUT_RTOL)
    np.testing.assert_allclose(pred["pts3D"].detach().cpu().numpy(), f["pts3D"], atol=OUT_ATOL, rtol=OUT_RTOL)
    loss = (pred["Ps_norm"] * torch.from_numpy(f["cP"]).float().to(device)).sum() + \
        (pred["pts3D"] * torch.from_numpy(f["cX"]).float().to(device)).sum()
    loss.backward()
    for k, p in net.named_parameters():
        assert p.grad is not None, f"{k} has no gradient (train.py:137 concatenates every p.grad)"
        check_grad(p.grad, f["grad/" + k], k)


@pytest.mark.parametrize("tag,layers", [("learning12", 12), ("optim9", 9)])
def test_full_width_forward(device, tag, layers):
    f = golden(f"net_{tag}.npz")
    _, data = scene_from_fixture(device)
    conf = gasfm_amd.learning_conf() if layers == 12 else gasfm_amd.optim_conf()
    net = gasfm_amd.GraphAttnSfMNet(conf)
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net = net.to(device).eval()
    with torch.no_grad():
        pred = net(data)
    np.testing.assert_allclose(pred["Ps_norm"].cpu().numpy(), f["Ps_norm"], atol=OUT_ATOL, rtol=OUT_RTOL)
    np.testing.assert_allclose(pred["pts3D"].cpu().numpy(), f["pts3D"], atol=OUT_ATOL, rtol=OUT_RTOL)


def test_reference_style_wrappers_without_plans(device):
    """A reference SceneData carries wrappers with no .plan: plans are derived from valid_indices."""
    f = golden("net_small.npz")
    _, data = scene_from_fixture(device)
    for w in data.graph_wrappers.values():
        w.plan = None
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.conf.small_conf(2))
    net.load_state_dict({k[3:]: torch.from_numpy(f[k]).float() for k in f.files if k.startswith("sd/")})
    pred = net.to(device)(data)
    np.testing.assert_allclose(pred["Ps_norm"].detach().cpu().numpy(), f["Ps_norm"], atol=OUT_ATOL, rtol=OUT_RTOL)


@pytest.mark.parametrize("scale", [0.01, 0.05])
def test_scaled_config4_vs_oracle(device, scale):
    """Synthetic config-4 scene (SfM-like windows, long camera segments) at oracle-friendly size."""
    from gasfm_amd import synthetic
    sc = synthetic.scaled_config4(scale, seed=11)
    vals = sc.normalized_values()
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    conf = gasfm_amd.learning_conf(num_layers=3)
    net = gasfm_amd.GraphAttnSfMNet(conf)
    sd = deterministic_state_dict(net.state_dict(), torch.float64)
    net.load_state_dict({k: v.float() for k, v in sd.items()})
    net = net.to(device)
    pred = net(data)
    g = scenes.graph_from_edges(sc.cam, sc.pt, sc.m, sc.n)
    sdp = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = gasfm_ref.forward(sdp, torch.from_numpy(vals).double(), g)
    np.testing.assert_allclose(pred["Ps_norm"].detach().cpu().numpy(), ref["Ps_norm"].detach().numpy(),
                               atol=OUT_ATOL, rtol=OUT_RTOL)
    np.testing.assert_allclose(pred["pts3D"].detach().cpu().numpy(), ref["pts3D"].detach().numpy(),
                               atol=OUT_ATOL, rtol=OUT_RTOL)
    gen = torch.Generator().manual_seed(3)
    cP = torch.randn(ref["Ps_norm"].shape, generator=gen, dtype=torch.float64)
    cX = torch.randn(ref["pts3D"].shape, generator=gen, dtype=torch.float64)
    ((ref["Ps_norm"] * cP).sum() + (ref["pts3D"] * cX).sum()).backward()
    ((pred["Ps_norm"] * cP.float().to(device)).sum() + (pred["pts3D"] * cX.float().to(device)).sum()).backward()
    # the same oracle in fp32: its distance to fp64 is the roundoff an fp32 implementation incurs
    sd32 = {k: v.float().clone().requires_grad_(True) for k, v in sd.items()}
    r32 = gasfm_ref.forward(sd32, torch.from_numpy(vals).float(), g, dtype=torch.float32)
    ((r32["Ps_norm"] * cP.float()).sum() + (r32["pts3D"] * cX.float()).sum()).backward()
    for k, p in net.named_parameters():
        r = sdp[k].grad
        r = torch.zeros_like(sdp[k]) if r is None else r
        q = sd32[k].grad
        q = torch.zeros_like(sd32[k]) if q is None else q
        check_grad(p.grad, r.numpy(), k, q.numpy())


def test_oom_maps_to_torch_oom(device):
    from gasfm_amd import _native
    with pytest.raises(torch.OutOfMemoryError):
        _native.check(_native.GASFM_ERR_OOM, "probe")


def test_captured_step_bitwise_vs_eager(device):
    """The whole step replayed from a captured hipGraph (graph_step.CapturedStep) gives bitwise the
    loss and gradients of the eager step (every reduction is ordered: no float atomics)."""
    from gasfm_amd import graph_step, synthetic
    sc = synthetic.scaled_config4(0.02, seed=7)
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    torch.manual_seed(0)
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.learning_conf(num_layers=4)).to(device)
    gen = torch.Generator().manual_seed(3)
    cP = torch.randn((sc.m, 3, 4), generator=gen).to(device)
    cX = torch.randn((4, sc.n), generator=gen).to(device)

    def fwd_bwd():
        pred = net(data)
        loss = (pred["Ps_norm"] * cP).sum() + (pred["pts3D"] * cX).sum()
        loss.backward()
        return loss

    def run(capture):
        for p in net.parameters():
            p.grad = None
        if capture:
            step = graph_step.CapturedStep(fwd_bwd, net.parameters())
            assert step.captured, step.fallback_reason
            loss = step()
        else:
            loss = fwd_bwd()
        torch.cuda.synchronize()
        return float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    l1, g1 = run(False)
    l2, g2 = run(True)
    assert l1 == l2
    bad = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not bad, f"{len(bad)} of {len(g1)} gradients differ: {bad[:12]}"


@pytest.mark.gpu
def test_several_forwards_one_backward(device):
    """train.py sums the losses of a batch of scenes and runs ONE backward: every parameter then
    receives one gradient contribution per scene.  With the batched end-of-backward weight sums
    (deferred colsums) the gradients must equal the undeferred ones, and both must equal the sum
    of the per-scene backward passes.  (Regression: the second contribution was added to the
    first, still-unfilled deferred sum: garbage, then NaN after an optimizer step.)"""
    from gasfm_amd import synthetic
    scenes = [gasfm_amd.SceneData.from_synthetic(synthetic.scaled_config4(s, seed=k)).to(device)
              for s, k in ((0.01, 3), (0.015, 4), (0.008, 5))]
    torch.manual_seed(0)
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.learning_conf(num_layers=3)).to(device)
    gen = torch.Generator().manual_seed(2)
    funcs = [((torch.randn((d.x.shape[0], 3, 4), generator=gen).to(device)),
              torch.randn((4, d.x.shape[1]), generator=gen).to(device)) for d in scenes]

    def loss_of(d, f):
        p = net(d)
        return (p["Ps_norm"] * f[0]).sum() + (p["pts3D"] * f[1]).sum()

    def grads(batched, defer):
        net.batch_weight_grads = defer
        for p in net.parameters():
            p.grad = None
        if batched:
            sum(loss_of(d, f) for d, f in zip(scenes, funcs)).backward()
        else:
            for d, f in zip(scenes, funcs):
                loss_of(d, f).backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}

    ref = grads(False, False)
    for batched, defer in ((True, True), (True, False), (False, True)):
        g = grads(batched, defer)
        assert g.keys() == ref.keys()
        for k in ref:
            assert torch.isfinite(g[k]).all(), k
            torch.testing.assert_close(g[k], ref[k], rtol=1e-4, atol=1e-5, msg=f"{k} batched={batched} defer={defer}")
    net.batch_weight_grads = True


def test_fused_point_tail_hub_bitwise_in_model(device, monkeypatch):
    """The model with the point tail + hub forward as one kernel (point_block.FUSED_TAIL_HUB, round 6)
    against the two-kernel path: bitwise the same outputs, loss and every parameter gradient (the fused
    kernel runs the same tile bodies, and the backward the same kernels in the same order), with the
    fused Function recorded as taken in every block that has a next block."""
    from gasfm_amd import point_block, synthetic
    sc = synthetic.scaled_config4(0.02, seed=5)
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    torch.manual_seed(0)
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.learning_conf(num_layers=4)).to(device)
    gen = torch.Generator().manual_seed(4)
    cP = torch.randn((sc.m, 3, 4), generator=gen).to(device)
    cX = torch.randn((4, sc.n), generator=gen).to(device)
    calls = []
    orig = point_block.PointTailHubFn.apply
    monkeypatch.setattr(point_block.PointTailHubFn, "apply", lambda *a: calls.append(1) or orig(*a))

    def run(fused):
        monkeypatch.setattr(point_block, "FUSED_TAIL_HUB", fused)
        for p in net.parameters():
            p.grad = None
        pred = net(data)
        loss = (pred["Ps_norm"] * cP).sum() + (pred["pts3D"] * cX).sum()
        loss.backward()
        torch.cuda.synchronize()
        return pred, float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    p2, l2, g2 = run(False)
    assert not calls
    p1, l1, g1 = run(True)
    assert len(calls) == 3, calls  # blocks 1..3 each have a next consumer; block 0 / the final update do not
    assert torch.equal(p1["Ps_norm"], p2["Ps_norm"]) and torch.equal(p1["pts3D"], p2["pts3D"])
    assert l1 == l2
    bad = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not bad, f"{len(bad)} of {len(g1)} gradients differ: {bad[:12]}"
