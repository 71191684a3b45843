"""The depth branch over a union batch on the device: the segmented kernels (csrc/depth_batch.hip)
against their per-scene oracles, and a depth-head training step captured by StaticTrainer.

Bounds.  U = 2^-24.

* Segmented DirectDepthLoss: the bounds tests/test_gpu_losses.py holds DirectDepthLoss and ESFMLoss to,
  against the fp64 per-edge oracle (tests/test_losses_cpu.py) per scene and against the sum of
  single-scene DirectDepthLoss calls: loss rtol 1e-5, gradients 1e-4 normwise and max-abs (``close``).
  The L1 gradient is a sign: the L1 inputs (seeds checked on the CPU) keep the oracle's min |u_e| over
  the weighted edges above 1e-4 except where it is exactly 0 (a one-edge scene), asserted on the oracle,
  so no sign can flip under fp32 summation order (u_e is of order 1, fp32 moves it by ~1e-6).
* Segmented 2-view error: the bound of tests/test_gpu_depth_eval.py.  The float32 torch restatement is
  measured against its fp64 self on the same float32 inputs, per scene, in the test; the kernel's
  per-edge errors get 8 x that maximum, the per-scene sums count x that plus the float32 summation
  chain (a thread's terms, 6 steps across the wave, 4 waves, 32 partial rows) x U x the sum.  Counts and
  the pairing are integers and must be equal.
* Captured step: the bars of test_static_trainer_with_ose_loss: loss 1e-4 relative to the eager union
  step, gradients ||got - ref|| <= 1e-3 ||ref|| + 1e-6 x the step's largest gradient norm.  The replayed
  per-scene 2-view errors are held to batch_depth_errors run eagerly on the same filled bucket at rtol
  1e-4: the replay may differ from an eager pass by a library GEMM's algorithm (as
  tests/test_gpu_static_batch.py notes), i.e. ~1e-6 relative on a depth, and an error of tens of pixels
  moves by about (pixel displacement / error) x that, well below 1e-4.
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd import depth_batch, depth_eval, evaluation, static_batch, synthetic
from gasfm_amd.batch import forward_batch
from gasfm_amd.depth_batch import SEG_G
from gasfm_amd.loss import DepthLossFn, DirectDepthLoss
from gasfm_amd.scene_device import apply_rotational_homography_aug_device, sample_data_device, scene_from_dense_device

from test_gpu_batch import _grads
from test_gpu_esfm_loss import close
from test_gpu_losses import oracle_depth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DLOSS = 0.75
# scenes of 1, 255, 256, 257 and SEG_G * 256 + 3 edges (slice remainders, a slice walked twice, u exactly
# 0) and a zero-weight pad scene; a layout with an empty zero-weight scene.  (sizes, weights, seed)
LAYOUTS = {"pad": ((1, 255, 256, 257, SEG_G * 256 + 3, 100), (1.0, 0.5, 1.0, 1.0, 2.0, 0.0), 4),
           "empty": ((257, 0, 1000, 3), (1.0, 0.0, 0.5, 0.0), 0)}


@pytest.fixture(autouse=True)
def s2g_pieces(monkeypatch):
    monkeypatch.setattr(static_batch, "S2G_PIECES", 128)  # the test scenes have ~1-2k valid points


# ------------------------------------------------------------------ segmented DirectDepthLoss
def _loss_case(name):
    sizes, weights, seed = LAYOUTS[name]
    g = torch.Generator().manual_seed(seed)
    E = sum(sizes)
    a = (0.5 + 2.0 * torch.rand(E, generator=g, dtype=torch.float64)).float()
    b = (1.0 + 3.0 * torch.rand(E, generator=g, dtype=torch.float64)).float()
    eo = np.concatenate([[0], np.cumsum(sizes)])
    return a, b, eo, weights


@pytest.fixture(scope="module")
def loss_refs():
    """fp64 per-scene oracles (loss, gradient at dloss = DLOSS x weight, min |u|), shared and left unchanged."""
    refs = {}
    for name in LAYOUTS:
        a, b, eo, weights = _loss_case(name)
        for cost in ("L1", "L2"):
            out = []
            for s, w in enumerate(weights):
                x, y = a[eo[s]:eo[s + 1]], b[eo[s]:eo[s + 1]]
                if w == 0 or len(x) == 0:
                    out.append(None)
                    continue
                u = (x.double() / x.double().mean() - y.double() / y.double().mean()).abs()
                out.append(oracle_depth(x, y, cost, dloss=DLOSS * w) + (u,))
            refs[name, cost] = out
    return refs


@pytest.mark.parametrize("cost", ["L1", "L2"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_segmented_depth_loss(device, loss_refs, name, cost):
    a, b, eo, weights = _loss_case(name)
    refs = loss_refs[name, cost]
    l2 = cost == "L2"
    if not l2:  # no sign can flip: |u_e| is exactly 0 or above 1e-4 on every weighted edge
        for r in refs:
            if r is not None:
                u = r[2]
                assert float(u[u != 0].min() if (u != 0).any() else 1.0) > 1e-4 and (len(u) > 1 or float(u[0]) == 0.0)
    ad, bd = a.clone(), b.clone()
    for s, w in enumerate(weights):
        if w == 0:  # NaN predictions and targets in a zero-weight scene reach nothing
            ad[eo[s]:eo[s + 1]] = float("nan")
            bd[eo[s]:eo[s + 1]] = float("nan")
    ad, bd = ad.to(device), bd.to(device)
    eoff = torch.tensor(eo, dtype=torch.int32, device=device)
    weight = torch.tensor(weights, dtype=torch.float32, device=device)
    dloss = torch.full((1,), DLOSS, device=device)

    def run():
        loss, sums, tot = depth_batch.depth_loss_seg_fwd(ad, bd, eoff, weight, l2)
        return loss, sums, tot, depth_batch.depth_loss_seg_bwd(ad, bd, eoff, weight, sums, tot, l2, dloss)

    loss, sums, tot, da = run()
    assert loss.is_cuda and tuple(tot.shape) == (len(weights), 2)
    ref_loss = sum(w * float(r[0]) for w, r in zip(weights, refs) if r is not None)
    single_loss = 0.0
    assert not torch.isnan(da).any() and not torch.isnan(loss).any() and not torch.isnan(tot).any()
    for s, (w, r) in enumerate(zip(weights, refs)):
        g = da[eo[s]:eo[s + 1]]
        if w == 0:
            assert len(g) == 0 or float(g.abs().max()) == 0.0  # exact zeros
            assert float(tot[s].abs().max()) == 0.0 and float(sums[s].abs().max()) == 0.0
            continue
        close(g, r[1], f"ddepths scene {s}")
        # the single-scene kernels on the same scene, same helper
        x = ad[eo[s]:eo[s + 1]].clone().requires_grad_(True)
        ls = DepthLossFn.apply(x, bd[eo[s]:eo[s + 1]].contiguous(), l2)
        (ls * DLOSS * w).backward()
        single_loss += w * float(ls.detach())
        close(g, x.grad, f"ddepths scene {s} against the single-scene kernel")
        np.testing.assert_allclose(float(tot[s, 0]) / len(g), float(ls.detach()), rtol=1e-5, atol=0)
        if len(g) == 1:
            assert float(tot[s, 0]) == 0.0 and float(g[0]) == 0.0  # u exactly 0
    print(f"depth seg {name} {cost}: loss {loss.item():.9g} fp64 {ref_loss:.9g} single-scene {single_loss:.9g}")
    np.testing.assert_allclose(loss.item(), ref_loss, rtol=1e-5, atol=0)
    np.testing.assert_allclose(loss.item(), single_loss, rtol=1e-5, atol=0)
    for u, v in zip((loss, sums, tot, da), run()):  # two runs are bitwise equal
        assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes()


# ------------------------------------------------------------------ device scenes with depth targets
def _full_scene(device, m, n, seed, name):
    """synthetic.windowed_scene's visibility with geometry under it, so that the scene build can
    triangulate its depth targets (windowed_scene's own pixels are random and its cameras all [I | 0]):
    cameras on a circle looking at points in [-1, 1]^3, as tests/test_gpu_depth_eval.py's handmade scene."""
    sc = synthetic.windowed_scene(m, n, mean_extra=6 if m > 20 else 4, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    ang = np.linspace(0, 2 * np.pi, m, endpoint=False)
    C = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.3 * rng.standard_normal(m)], 1)
    R = np.stack([synthetic.rotation_look_at(c) for c in C])  # camera-to-world
    Rt = np.concatenate([R.transpose(0, 2, 1), -(R.transpose(0, 2, 1) @ C[:, :, None])], 2)
    X = rng.uniform(-1, 1, size=(n, 3))
    q = np.einsum("eij,ej->ei", Rt[sc.cam], np.concatenate([X[sc.pt], np.ones((sc.num_edges, 1))], 1))
    pix = q @ sc.K.T
    sc.xy = (pix[:, :2] / pix[:, 2:]).astype(np.float32)
    assert q[:, 2].min() > 1.0
    Ps = (sc.K[None] @ Rt).astype(np.float32)
    return scene_from_dense_device(torch.from_numpy(sc.dense_M()).to(device), torch.from_numpy(sc.Ns()).to(device),
                                   torch.from_numpy(Ps).to(device), name, store_depth_targets=True)


def _bucket(device, datas, caps=None):
    st = static_batch.BatchStats(datas)
    assert st.expressible() is None
    caps = static_batch.Caps.for_batch(st) if caps is None else caps
    assert caps.pad(st) is not None
    return st, caps


def _check_2view(sb, datas, st, device, seed):
    """The segmented pipeline on the filled bucket against each scene's own evaluation."""
    mo, no, eo = sb.offsets
    g = torch.Generator().manual_seed(seed)
    d = sb.depths.clone()  # predictions: the targets with 5% noise at another scale per scene; the pad keeps 1
    for s in range(st.B):
        noise = 1 + 0.05 * torch.randn(st.Es[s], generator=g, dtype=torch.float64)
        d[eo[s]:eo[s + 1]] *= (noise * (0.3 + 1.7 * s)).float().to(device)
    scales = depth_batch.depth_scales_seg(d, sb.depths, sb.eoff)
    src, _ = depth_eval.track_cycle(sb.pt_ptr, sb.perm, sb.pair_keys)
    tot, err, _ = depth_batch.backproj_2view_seg(sb.cam32, None, sb.xy, d, scales, src, sb.eoff, sb.camtab, per_edge=True)
    tot_checked = depth_batch.backproj_2view_seg(sb.cam32, sb.pt32, sb.xy, d, scales, src, sb.eoff, sb.camtab)
    assert torch.equal(tot, tot_checked)  # a valid pairing: the track check changes nothing
    assert torch.isfinite(tot).all() and float(tot[st.B, 1]) > 0  # the pad scene is a scene like the others
    for s, data in enumerate(datas):
        e0, e1 = eo[s], eo[s + 1]
        (cam, pt), _, _, pt_ptr, perm = evaluation._edge_tensors(data)
        # pairing: the union's, restricted to the scene and shifted, is the scene's own from its keys
        own, _ = depth_eval.track_cycle(pt_ptr, perm, sb.pair_keys[e0:e1].contiguous())
        sliced = torch.where(src[e0:e1] >= 0, src[e0:e1] - e0, src[e0:e1])
        assert torch.equal(sliced, own), s
        dp, dg = d[e0:e1].contiguous(), data.depths
        assert torch.equal(dg, sb.depths[e0:e1])
        (tot_s, scales_s, err_s, _) = evaluation.backproj_2view_error(data, dp, dg, pairing=sliced, per_edge=True)
        np.testing.assert_allclose(scales[s].cpu().numpy(), scales_s.cpu().numpy(), rtol=2 * U)
        # the float32 restatement against its fp64 self on the same inputs: the bar (module docstring)
        c = lambda t: t.cpu()  # noqa: E731
        tab64 = evaluation._camera_table(data, torch.float32, device).cpu().double()
        xy = evaluation._pixel_measurements(data)
        scale = (scales_s[1] / scales_s[0]).cpu()
        args = (c(cam), c(pt), c(xy), c(dp), scale, c(sliced))
        r32 = depth_eval.backproj_2view_torch(*args, tab64.float())
        r64 = depth_eval.backproj_2view_torch(*args, tab64)
        ok = ~torch.isnan(r64[0])
        m_err = float((r32[0].double() - r64[0])[ok].abs().max())
        count = int(r64[2][1])
        assert int(tot[s, 1]) == int(tot_s[1]) == count > 0
        k_err = float((err[e0:e1].cpu().double() - r64[0])[ok].abs().max())
        chain = -(-(e1 - e0) // (256 * SEG_G)) + 6 + 4 + SEG_G
        bar = count * 8 * m_err + chain * U * float(r64[2][0])
        print(f"2view scene {s}: E {e1 - e0} fp32 restatement {m_err:.3e} px, kernel {k_err:.3e} px (bar {8 * m_err:.3e}); "
              f"sum {float(tot[s, 0]):.6f} single-scene {float(tot_s[0]):.6f} fp64 {float(r64[2][0]):.6f} (bar {bar:.3e})")
        assert torch.equal(torch.isnan(err[e0:e1]).cpu(), ~ok)
        assert k_err <= 8 * m_err
        assert abs(float(tot[s, 0]) - float(tot_s[0])) <= bar
        assert abs(float(tot[s, 0]) - float(r64[2][0])) <= bar
        assert float((err[e0:e1] - err_s).abs().nan_to_num(0).max()) <= 8 * m_err


def test_segmented_2view_error(device):
    datas = [_full_scene(device, m, 1500, 60 + m, f"s{m}") for m in (10, 12, 14)]
    st, caps = _bucket(device, datas)
    sb = static_batch.StaticBatch(caps, device).enable_depth()
    torch.manual_seed(3)
    sb.fill(datas, st)
    assert sb.two_view_ready and sb.pair_keys.is_cuda
    _check_2view(sb, datas, st, device, 1)
    # the same bucket refilled with smaller scenes: nothing stale is read
    small = [_full_scene(device, m, 1400, 80 + m, f"t{m}") for m in (10, 11, 13)]
    st2, _ = _bucket(device, small, caps)
    sb.fill(small, st2)
    _check_2view(sb, small, st2, device, 2)
    # fill_torch writes the same depth inputs
    other = static_batch.StaticBatch(caps, device).enable_depth()
    other.fill_torch(small, st2)
    assert torch.equal(other.depths, sb.depths) and torch.equal(other.camtab, sb.camtab)


# ------------------------------------------------------------------ the captured step
def depth_conf(cost_fcn):
    conf = gasfm_amd.conf.small_conf(2, depth_head={"enabled": True, "n_feat": 128, "n_hidden_layers": 2},
                                     view_head={"enabled": False, "n_hidden_layers": 2, "rot_representation": "quat"},
                                     scenepoint_head={"enabled": False, "n_hidden_layers": 2})
    conf.put("loss.cost_fcn", cost_fcn)
    return conf


def _train_scenes(device, views, seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    out = []
    for i, v in enumerate(views):
        full = _full_scene(device, 40, 3000, 20 + i + 7 * seed, f"s{i}")
        out.append(apply_rotational_homography_aug_device(sample_data_device(full, v), 15, 20))
        assert out[-1].depths is not None and out[-1].depths.shape[0] == out[-1].x.indices.shape[1]
    return out


def _eager_union(net, lossf, datas):
    net.zero_grad(set_to_none=True)
    pred = forward_batch(net, datas)
    loss = sum(lossf(p, d) for p, d in zip(pred, datas))
    loss.backward()
    return float(loss), _grads(net)


def _check_step_grads(net, g_ref, tag):
    floor = 1e-6 * max(float(g.double().norm()) for g in g_ref if g is not None)
    for (name, p), b in zip(net.named_parameters(), g_ref):
        assert (p.grad is None) == (b is None), name
        if b is not None:
            err, nr = float((p.grad.double() - b.double()).norm()), float(b.double().norm())
            assert err <= 1e-3 * nr + floor, f"{tag} {name}: {err:.3e} / {nr:.3e}"


def test_static_trainer_with_direct_depth_loss(device, monkeypatch):
    monkeypatch.setattr(static_batch, "MAX_WASTE", 10.0)  # the second batch reuses the first one's bucket
    torch.manual_seed(5)
    conf = depth_conf("L2")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = DirectDepthLoss(conf)
    datas = _train_scenes(device, (12, 15), seed=3)
    loss_ref, g_ref = _eager_union(net, lossf, datas)
    trainer = static_batch.StaticTrainer(net, lossf, two_view_error=True)
    for k in range(2):
        loss, errs = trainer.step(datas)
        assert trainer.captures == 1 and trainer.fallbacks == [] and trainer.eager_steps == 0
        sb, step = next(iter(trainer.buckets.values()))[:2]
        assert step.captured
        print(f"depth trainer step {k}: loss {float(loss):.9g} ref {loss_ref:.9g} errors {errs}")
        assert abs(float(loss) - loss_ref) <= 1e-4 * abs(loss_ref)
        _check_step_grads(net, g_ref, f"step {k}")
        # the replayed errors: finite, and batch_depth_errors run eagerly on the same filled bucket
        assert len(errs) == 2 and all(np.isfinite(e) and e > 0 for e in errs)
        with torch.no_grad():
            tot = static_batch.batch_depth_errors(net(sb), sb).tolist()
        np.testing.assert_allclose(errs, [a / b for a, b in tot[:2]], rtol=1e-4)
    # another batch filled into the same bucket: the replay gives that batch's loss (nothing baked in)
    other = _train_scenes(device, (10, 13), seed=4)
    loss2, errs2 = trainer.step(other)
    assert trainer.captures == 1 and len(trainer.buckets) == 1 and trainer.eager_steps == 0
    ref2, g2 = _eager_union(net, lossf, other)
    assert abs(ref2 - loss_ref) > 1e-3 * abs(loss_ref)  # the batches differ
    assert abs(float(loss2) - ref2) <= 1e-4 * abs(ref2)
    assert all(np.isfinite(e) for e in errs2)
    # without the flag the errors are NaN per scene
    plain = static_batch.StaticTrainer(net, lossf)
    loss3, errs3 = plain.step(datas)
    assert plain.fallbacks == [] and abs(float(loss3) - loss_ref) <= 1e-4 * abs(loss_ref)
    assert len(errs3) == 2 and all(np.isnan(e) for e in errs3)


def test_static_trainer_with_direct_depth_loss_l1(device):
    torch.manual_seed(6)
    conf = depth_conf("L1")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = DirectDepthLoss(conf)
    datas = _train_scenes(device, (12, 15), seed=5)
    loss_ref, _ = _eager_union(net, lossf, datas)
    trainer = static_batch.StaticTrainer(net, lossf, two_view_error=True)
    for k in range(2):
        loss, _ = trainer.step(datas)
        assert trainer.captures == 1 and trainer.fallbacks == [] and trainer.eager_steps == 0
        assert next(iter(trainer.buckets.values()))[1].captured
        assert abs(float(loss) - loss_ref) <= 1e-4 * abs(loss_ref)


def test_static_trainer_depth_refusals(device):
    conf = depth_conf("L2")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = DirectDepthLoss(conf)
    datas = _train_scenes(device, (12,), seed=6)
    trainer = static_batch.StaticTrainer(net, lossf, two_view_error=True)
    keep = datas[0].y
    datas[0].y = None
    with pytest.raises(ValueError, match="'s0' carries no ground-truth cameras"):
        trainer.step(datas)
    datas[0].y = keep
    datas[0].depths = None
    with pytest.raises(ValueError, match="'s0' carries no depths"):
        trainer.step(datas)
    with pytest.raises(ValueError, match="two_view_error"):
        from gasfm_amd.loss import ExpDepthRegularizedOSELoss
        static_batch.StaticTrainer(net, ExpDepthRegularizedOSELoss.__new__(ExpDepthRegularizedOSELoss),
                                   two_view_error=True)
    assert trainer.captures == 0
