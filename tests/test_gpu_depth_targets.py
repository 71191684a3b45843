"""Per-edge depth targets on the device (csrc/depth_targets.hip, scene_device.py): the three kernels
against their torch restatements and an fp64 evaluation of the same float32 inputs, and the scene
path (build, sample, augment) against the reference's dense depths read at ``data.x.indices``
(tests/golden/depth_targets.npz).  Bounds: the module docstring of tests/test_depth_targets_cpu.py
(targets 4u S against fp64 and 6u S against the reference; rescale B against fp64, 2B against the
reference); the gather is exact.  After sampling and augmentation the targets carry both errors:
2B for the rescale plus the targets' 6u S scaled by |z_new / z_old| (1 + 2u), the factor the rescale
applies to an input error.
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd import _native, scene_device as sd
from gasfm_amd.loss import DirectDepthLoss
from gasfm_amd.scene_device import (apply_rotational_homography_aug_device, sample_data_device,
                                    scene_from_dense_device)

from test_depth_targets_cpu import (U, VIEW_CASES, assert_within, cam_ptr_of, fixture, parent_arrays, rescale_fp64,
                                    sample_case, targets_fp64)
from test_gpu_esfm_loss import close

pytestmark = pytest.mark.gpu

GUARD = 64


def big_E():
    """An edge count above grid x block of the kernels (each slot is one wave of a 256-thread block)."""
    return int(_native.lib().gasfm_depth_part_slots(1 << 40)) // 4 * 256 + 77


EDGE_COUNTS = [0, 1, 63, 64, 65, 257, "big"]


def guarded(E, device):
    """(buffer of NaNs, its [GUARD, GUARD + E) window the kernel writes)."""
    buf = torch.full((E + 2 * GUARD,), float("nan"), device=device)
    return buf, buf[GUARD:GUARD + E]


def guards_untouched(buf, E):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + E:]).all())


@pytest.fixture(scope="module")
def fx():
    return fixture()


@pytest.fixture(scope="module")
def full_scene(fx, device):
    """The fixture's scene built on the device with targets; shared and left unchanged."""
    return scene_from_dense_device(fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device), "fixture",
                                   store_depth_targets=True)


def dense_target_bound(fx):
    """6u sum_i |a_ci||X_pi| for every (camera, point) of the fixture's scene."""
    a = sd.depth_rows(fx["Ns"], fx["Ps_gt"]).double().abs()
    return 6 * U * (a @ fx["X"].double().abs().nan_to_num(0.0))


# ------------------------------------------------------------------ kernels
def _random_edges(E, m, n, seed):
    g = torch.Generator().manual_seed(seed)
    cam = torch.sort(torch.randint(0, m, (E,), generator=g)).values
    pt = torch.randint(0, n, (E,), generator=g)
    return g, cam, pt


@pytest.mark.parametrize("E", EDGE_COUNTS)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_depth_targets_kernel(device, E, idx):
    E = big_E() if E == "big" else E
    m, n = 7, 131
    g, cam, pt = _random_edges(E, m, n, 3)
    a = torch.randn((m, 4), generator=g) * 0.5
    a[:, 3] = 3.0 + torch.rand(m, generator=g)
    X = torch.cat([torch.rand((n, 3), generator=g) * 2 - 1, torch.ones(n, 1)], 1)
    X[5, :3] = torch.tensor([-40.0, -40.0, -40.0]) * a[0, :3].sign()  # behind every camera like camera 0
    X[9] = float("nan")  # a point no camera triangulated
    want_d, want_bad = sd.depth_targets_torch(a, X, cam, pt)
    buf, out = guarded(E, device)
    args = (a.to(device), X.to(device), cam.to(device, idx), pt.to(device, idx))
    d, bad = _native.depth_targets(*args, out=out)
    assert guards_untouched(buf, E)
    ok = torch.isfinite(want_d)
    assert torch.equal(torch.isfinite(d.cpu()), ok)
    exact, S = targets_fp64(a, X, cam, pt)
    assert_within(d.cpu()[ok], exact[ok], (4 * U * S)[ok], f"targets kernel E={E} vs fp64")
    assert_within(d.cpu()[ok], want_d[ok], (8 * U * S)[ok], f"targets kernel E={E} vs restatement")  # 4u S each
    # the count: NaN rows, depths below 0 (none of the 917 (camera, point) values is within rounding of 0)
    assert (exact.abs() > 1e-4).sum() == ok.sum()
    assert int(bad) == int(want_bad) == int((~(exact > 0)).sum())
    d2, bad2 = _native.depth_targets(*args)
    assert torch.equal(d2.isnan(), d.isnan()) and torch.equal(d2.nan_to_num(0), d.nan_to_num(0))
    assert torch.equal(bad2, bad)


def _random_parent(E, seed):
    """A parent scene and a sample of it with exactly E sampled edges (a prefix of the camera-major
    list of the sample's edges is itself a valid edge list)."""
    g = torch.Generator().manual_seed(seed)
    mp = 9
    npnt = max(40, 3 * E // 5 + 16)  # ~2.4 sampled edges per parent point
    vis = torch.rand((mp, npnt), generator=g) < 0.6
    vis[4] = False  # an empty parent row
    vis[4, npnt // 2] = True  # ... of length 1
    pcam, ppt = torch.nonzero(vis, as_tuple=True)
    pd = torch.rand(pcam.shape[0], generator=g) + 1.0
    views = torch.tensor([0, 2, 3, 4, 7, 8])
    keep = torch.nonzero(torch.rand(npnt, generator=g) < 0.8).view(-1)
    if npnt // 2 not in keep.tolist():
        keep = torch.sort(torch.cat([keep, torch.tensor([npnt // 2])])).values
    sub = vis[views][:, keep]
    cam, pt = torch.nonzero(sub, as_tuple=True)
    assert cam.shape[0] >= E
    dense = torch.zeros((mp, npnt))
    dense[pcam, ppt] = pd
    cam, pt = cam[:E].contiguous(), pt[:E].contiguous()
    return cam_ptr_of(pcam, mp), ppt.contiguous(), pd, views, keep, cam, pt, dense[views[cam], keep[pt]]


@pytest.mark.parametrize("E", EDGE_COUNTS)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_depth_gather_kernel(device, E, idx):
    E = big_E() if E == "big" else E
    pcam_ptr, ppt, pd, views, keep, cam, pt, want = _random_parent(E, 5)
    d_t, miss_t = sd.depth_gather_torch(pcam_ptr, ppt, pd, views, keep, cam, pt)
    assert torch.equal(d_t, want) and int(miss_t) == 0
    buf, out = guarded(E, device)
    args = (pcam_ptr.to(device), ppt.to(device, idx), pd.to(device), views.to(device), keep.to(device),
            cam.to(device, idx), pt.to(device, idx))
    d, missing = _native.depth_gather(*args, out=out)
    assert guards_untouched(buf, E)
    assert torch.equal(d.cpu(), want) and int(missing) == 0
    d2, missing2 = _native.depth_gather(*args)
    assert torch.equal(d2, d) and torch.equal(missing2, missing)


@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_depth_gather_kernel_fixture_cases(device, fx, name):
    """The row of length 1, hits at the first and the last element of a row, the sampled camera whose
    points were all dropped, points dropped for < 2 sampled views, non-adjacent views
    (test_depth_targets_cpu.VIEW_CASES): equal to dense indexing of the reference's matrix."""
    views, keep, _, cam, pt, want = sample_case(fx, VIEW_CASES[name])
    pcam_ptr, ppt, pd = parent_arrays(fx)
    d, missing = _native.depth_gather(pcam_ptr.to(device), ppt.to(device), pd.to(device), views.to(device),
                                      keep.to(device), cam.to(device), pt.to(device))
    assert int(missing) == 0 and torch.equal(d.cpu(), want)


def test_depth_gather_kernel_counts_missing_and_stays_in_range(device, fx):
    """Edges without a parent edge, and indices outside every array, are counted and NaN: nothing is
    read out of range."""
    views, keep, _, cam, pt, want = sample_case(fx, [2, 3, 4, 5])
    pcam_ptr, ppt, pd = parent_arrays(fx)
    keep = keep.clone()
    keep[pt[0]] = 59  # no camera sees point 59
    cam, pt, views = cam.clone(), pt.clone(), views.clone()
    bad = pt == pt[0]
    cam[-1], pt[-2], views[1] = 17, -3, 99  # outside view_idx, outside keep, outside the parent's cameras
    bad[-1] = bad[-2] = True
    bad |= cam == 1
    d, missing = _native.depth_gather(pcam_ptr.to(device), ppt.to(device), pd.to(device), views.to(device),
                                      keep.to(device), cam.to(device), pt.to(device))
    assert int(missing) == int(bad.sum())
    assert torch.equal(d.cpu().isnan(), bad) and torch.equal(d.cpu()[~bad], want[~bad])


@pytest.mark.parametrize("E", EDGE_COUNTS)
@pytest.mark.parametrize("idx", [torch.int64, torch.int32])
def test_depth_rescale_kernel(device, E, idx):
    E = big_E() if E == "big" else E
    m, n = 5, 203
    g, cam, pt = _random_edges(E, m, n, 7)
    M = torch.rand((2 * m, n), generator=g) * 999 + 1
    K = torch.tensor([[800.0, 0.0, 500.0], [0.0, 800.0, 500.0], [0.0, 0.0, 1.0]])
    Ns = torch.linalg.inv(K)[None].repeat(m, 1, 1).contiguous()
    Ns[:, 0, 0] *= 1 + 0.1 * torch.rand(m, generator=g)
    torch.manual_seed(11)
    R = sd.rotational_homography(m, 15.0, 20.0).contiguous()
    d0 = torch.rand(E, generator=g) * 4 + 1
    want = sd.depth_rescale_torch(d0, cam, pt, M, Ns, R)
    exact, bound, _ = rescale_fp64(d0, cam, pt, M, Ns, R)
    buf, out = guarded(E, device)
    args = (d0.to(device), cam.to(device, idx), pt.to(device, idx), M.to(device), Ns.to(device), R.to(device))
    d = _native.depth_rescale(*args, out=out)
    assert guards_untouched(buf, E)
    assert_within(d.cpu(), exact, bound, f"rescale kernel E={E} vs fp64")
    assert_within(d.cpu(), want, 2 * bound, f"rescale kernel E={E} vs restatement")
    assert torch.equal(_native.depth_rescale(*args), d)


# ------------------------------------------------------------------ end to end
def _dense_at(dense, data):
    i = data.x.indices.cpu()
    return dense[i[0], i[1]]


def _sampled(full_scene, fx, build):
    nv, npseed = int(fx["params"][0]), int(fx["params"][1])
    np.random.seed(npseed)
    return sample_data_device(full_scene, nv, build=build)


def _augmented(s, fx):
    torch.manual_seed(int(fx["params"][2]))
    return apply_rotational_homography_aug_device(s, float(fx["params"][3]), float(fx["params"][4]))


def test_full_scene_targets(device, fx, full_scene):
    data = full_scene
    assert data.store_depth_targets and data.depths.dtype == torch.float32 and data.depths.is_cuda
    assert torch.equal(data.x.indices.cpu(), fx["indices"])
    assert_within(data.depths, _dense_at(fx["depths"], data), _dense_at(dense_target_bound(fx), data),
                  "full scene vs the reference")
    again = scene_from_dense_device(fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device), "fixture",
                                    store_depth_targets=True)
    assert torch.equal(again.depths, data.depths)  # two runs bitwise equal
    # X as the reference: pflat, NaN only where no edge reads it
    X = sd.triangulate_scene_device(fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device),
                                    {"cam": data.x.indices[0], "pt": data.x.indices[1], **data._scene_build})
    seen = data.x.indices[1].unique()
    assert bool((X[seen, 3] == 1).all()) and bool(torch.isfinite(X[seen]).all()) and bool(X[58:].isnan().all())
    torch.testing.assert_close(X[seen].cpu(), fx["X"].t()[seen.cpu()], rtol=1e-5, atol=1e-6)


def test_adopted_and_conf_switched_targets(device, fx, full_scene):
    M, Ns, Ps = fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device)
    e = _dense_at(fx["depths"], full_scene)
    for given in (e.to(device), fx["depths"]):  # [E], and the reference's dense [m, n]
        s = scene_from_dense_device(M, Ns, Ps, "fixture", store_depth_targets=True, depths=given)
        assert torch.equal(s.depths.cpu(), e) and s.depths.is_cuda
    conf = gasfm_amd.conf.small_conf(2, depth_head={"enabled": True, "n_feat": 32, "n_hidden_layers": 2})
    assert torch.equal(sd.create_scene_data_device(conf, M, Ns, Ps, "fixture").depths, full_scene.depths)
    off = sd.create_scene_data_device(gasfm_amd.conf.small_conf(2), M, Ns, Ps, "fixture")
    assert off.depths is None and off.store_depth_targets is False
    with pytest.raises(NotImplementedError):
        scene_from_dense_device(M, Ns, Ps, "fixture", calibrated=False, store_depth_targets=True)


def test_sampled_scene_targets(device, fx, full_scene):
    s = _sampled(full_scene, fx, build=True)
    assert torch.equal(s.x.indices.cpu(), fx["s_indices"]) and torch.equal(s._M.cpu(), fx["s_M"])
    # the gather is exact: the full scene's targets at the sampled edges, whose reference values ...
    views, keep, _, cam, pt, _ = sample_case(fx, fx["s_views"])
    parent = torch.zeros((6, 60))
    parent[fx["indices"][0], fx["indices"][1]] = full_scene.depths.cpu()
    assert torch.equal(s.depths.cpu(), parent[views[cam], keep[pt]])
    # ... are the reference's sampled dense depths
    bound = dense_target_bound(fx)[views][:, keep]
    assert_within(s.depths, _dense_at(fx["s_depths"], s), _dense_at(bound, s), "sampled scene vs the reference")
    assert torch.equal(_sampled(full_scene, fx, build=True).depths, s.depths)


def test_host_scene_with_dense_depths_is_gathered_once(device, fx):
    """A host scene in the reference's form (dense [m, n] depths) entering sample_data_device."""
    host = gasfm_amd.SceneData(fx["M"], fx["Ns"], fx["Ps_gt"], "host")
    host._M = fx["M"].to(device)
    host.store_depth_targets, host.depths = True, fx["depths"]
    np.random.seed(int(fx["params"][1]))
    s = sample_data_device(host, int(fx["params"][0]))
    assert torch.equal(s.depths.cpu(), _dense_at(fx["s_depths"], s)) and s.depths.dim() == 1
    assert host._gasfm_depth_edges[2][2].is_cuda


@pytest.mark.parametrize("build", [False, True])
def test_sampled_and_augmented_scene_targets(device, fx, full_scene, build):
    s = _sampled(full_scene, fx, build=build)
    if not build:
        assert isinstance(s, sd.DenseScene) and s.store_depth_targets and s.depths is None
    a = _augmented(s, fx)
    assert torch.equal(a.x.indices.cpu(), fx["a_indices"])
    cam, pt = fx["a_indices"][0], fx["a_indices"][1]
    views, keep, _, _, _, _ = sample_case(fx, fx["s_views"])
    _, B, ratio = rescale_fp64(fx["s_depths"][cam, pt], cam, pt, fx["s_M"], fx["Ns"][views], fx["R_aug"])
    carried = dense_target_bound(fx)[views][:, keep][cam, pt] * ratio.abs() * (1 + 2 * U)
    assert_within(a.depths, fx["a_depths"][cam, pt], 2 * B + carried, f"sample + augmentation (build={build})")
    assert torch.equal(_augmented(_sampled(full_scene, fx, build=build), fx).depths, a.depths)
    if build:  # both orders of building give the same targets, bit for bit
        assert torch.equal(_augmented(_sampled(full_scene, fx, build=False), fx).depths, a.depths)
    # no angles: the targets pass through
    p = apply_rotational_homography_aug_device(_sampled(full_scene, fx, build=build))
    assert torch.equal(p.depths.cpu(), _sampled(full_scene, fx, build=True).depths.cpu())


def test_point_behind_a_camera_raises(device, fx):
    Ps = fx["Ps_gt"].clone()
    Ps[1] = -Ps[1]  # the same projections and triangulation; every depth of camera 1 changes sign
    with pytest.raises(ValueError, match="depth targets are not finite or not > 0"):
        scene_from_dense_device(fx["M"].to(device), fx["Ns"].to(device), Ps.to(device), "behind",
                                store_depth_targets=True)


def _arrays(s):
    out = {"M": s._M, "y": s.y, "Ns": s.Ns, "values": s.x.values, "indices": s.x.indices,
           "cam_per_pts": s.x.cam_per_pts, "pts_per_cam": s.x.pts_per_cam}
    for name, w in s.graph_wrappers.items():
        out[name + ".edge_index"] = w.edge_index
        for k in ("seg_ptr", "perm", "pos", "items", "combine", "combine_l1"):
            if getattr(w.plan, k) is not None:
                out[f"{name}.{k}"] = getattr(w.plan, k)
    return out


def test_without_the_flag_nothing_changes(device, fx, full_scene):
    """store_depth_targets=False: depths is None on every scene, and every array of the built, the
    sampled and the augmented scene is equal to the one the flag-carrying calls produce: the
    targets ride along and change nothing else."""
    plain = scene_from_dense_device(fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device), "fixture")
    chains = []
    for full in (plain, full_scene):
        s = _sampled(full, fx, build=True)
        chains.append([full, s, _augmented(s, fx), _augmented(_sampled(full, fx, build=False), fx)])
    for p, w in zip(*chains):
        assert p.depths is None and p.store_depth_targets is False and w.depths is not None
        ap, aw = _arrays(p), _arrays(w)
        assert ap.keys() == aw.keys()
        for k in ap:
            assert torch.equal(ap[k], aw[k]), k
    host = gasfm_amd.SceneData(fx["M"], fx["Ns"], fx["Ps_gt"], "host")
    assert torch.equal(plain.x.indices.cpu(), host.x.indices)
    s = _sampled(plain, fx, build=False)
    assert s.depths is None and s.store_depth_targets is False and s._depth_src is None


def test_direct_depth_loss_on_device_targets(device, fx, full_scene):
    """A 3-block net with the depth head: DirectDepthLoss and backward on the targets of this path
    against the same step fed the reference's dense matrix, at tests/test_gpu_losses.py's bars (loss
    1e-5 relative; gradients 1e-4 normwise and of the largest entry)."""
    conf = gasfm_amd.conf.small_conf(3, depth_head={"enabled": True, "n_feat": 32, "n_hidden_layers": 2})
    conf.put("loss.cost_fcn", "L1")
    torch.manual_seed(3)
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = DirectDepthLoss(conf)
    results = []
    data = full_scene
    for targets in (full_scene.depths, fx["depths"].to(device)):
        net.zero_grad(set_to_none=True)
        d = scene_from_dense_device(fx["M"].to(device), fx["Ns"].to(device), fx["Ps_gt"].to(device), "fixture",
                                    store_depth_targets=True, depths=targets)
        assert torch.equal(d.x.indices, data.x.indices)
        loss = lossf(net(d), d)
        loss.backward()
        results.append((loss.detach(), {k: p.grad.clone() for k, p in net.depth_head.named_parameters()}))
    (la, ga), (lb, gb) = results
    print(f"depth loss: device targets {la.item():.9g}, reference targets {lb.item():.9g}")
    assert torch.isfinite(la) and float(la) > 0
    np.testing.assert_allclose(la.item(), lb.item(), rtol=1e-5, atol=0)
    assert ga and all(float(g.abs().max()) > 0 for g in ga.values() if g.dim() == 2)
    for k in ga:
        close(ga[k], gb[k], f"depth_head.{k}")
