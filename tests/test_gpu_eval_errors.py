"""Scene evaluation on the device (gasfm_amd/evaluation.py: prepare_predictions / compute_errors,
csrc/eval_metrics.hip) against the reference's own results (tests/golden/eval_errors.npz,
make_golden_eval.py) and an fp64 numpy restatement of evaluation.py:351-363.

Bars.  Counts are integers, so the three fractions agree to 1e-12.  A depth is four fp32 products
and a divide per term: |depth - ref| <= 8 * 2^-24 * sum_j |P_2j| |X_j| (evaluated in fp64), min and
max with it; the mean adds 2^-23 |mean|.  Reprojection errors: the bars of test_gpu_core_errors.py
(per edge rtol 1e-4 + atol 1e-3, mean rtol 2e-5); DLT: the bar of test_gpu_ba.py (rtol 1e-8);
poses: rtol 1e-6 (fp32 inputs, fp64 work).
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import golden
from gasfm_amd import _native, evaluation, synthetic
from test_eval_errors_cpu import (DictConf, test_alignment_exact_similarity,  # noqa: F401
                                  test_alignment_noisy_stationary)

pytestmark = pytest.mark.gpu

DEPTH_KEYS = ("fraction_views_neg_depth_for_any_point", "fraction_points_neg_depth_in_any_view",
              "total_fraction_points_neg_depth", "point_depth_mean", "point_depth_min", "point_depth_max")
U = 2.0 ** -24


def _scene(M, Ns, y, device, name="scene"):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return gasfm_amd.SceneData(t(M), t(Ns), t(y), name).to(device)


def _pred(Ps_norm, pts3D, device):
    return {"Ps_norm": torch.from_numpy(Ps_norm).to(device), "pts3D": torch.from_numpy(pts3D).to(device)}


def _dense_depth_metrics(Ps, X, vis, margin):
    """evaluation.py:351-363 restated in fp64 numpy on the dense [m, 3, n] array; also the edge
    depths and the per-edge fp32 bound."""
    Xf = X / X[-1]
    depth = (Ps @ Xf)[:, 2, :]
    neg = ~(depth >= margin) & vis
    n_views = vis.any(axis=1).sum()
    n_pts = vis.any(axis=1).sum()  # sic: the reference counts views here as well
    out = {"fraction_views_neg_depth_for_any_point": neg.any(axis=1).sum() / n_views,
           "fraction_points_neg_depth_in_any_view": neg.any(axis=0).sum() / n_pts,
           "total_fraction_points_neg_depth": neg.sum() / vis.sum(),
           "point_depth_mean": depth[vis].mean(), "point_depth_min": depth[vis].min(),
           "point_depth_max": depth[vis].max()}
    bound = 8 * U * (np.abs(Ps[:, 2, :]) @ np.abs(Xf))
    return out, depth, bound


def _check_depth_metrics(got, ref, bound_edges):
    for k in DEPTH_KEYS[:3]:
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    if np.isnan(ref["point_depth_mean"]):
        assert all(np.isnan(got[k]) for k in DEPTH_KEYS[3:])
        return
    b = np.nanmax(bound_edges)
    assert abs(got["point_depth_min"] - ref["point_depth_min"]) <= b
    assert abs(got["point_depth_max"] - ref["point_depth_max"]) <= b
    mean = ref["point_depth_mean"]
    assert abs(got["point_depth_mean"] - mean) <= np.nanmean(bound_edges) + 2 * U * abs(mean)


def _edge_depths(state, margin):
    depth = torch.empty(state["cam"].shape[0], dtype=torch.float32, device=state["cam"].device)
    out = _native.depth_stats(state["cam"], state["pt"], state["cam_ptr"], state["pt_ptr"], state["perm"],
                              state["P"], state["X"], margin, depth)
    return depth.cpu().numpy(), out


def test_depth_set_matches_reference(device):
    f = golden("eval_errors.npz")
    conf = DictConf(dataset__calibrated=False)
    data = _scene(f["d_M"], f["d_Ns"], None, device)
    assert np.array_equal(data.x.indices.cpu().numpy(), np.stack([f["d_cam"], f["d_pt"]]))
    outputs = evaluation.prepare_predictions(data, _pred(f["d_Ps_norm"], f["d_pts3D"], device), conf, False)
    got = evaluation.compute_errors(outputs, conf, False)
    ref = {k[6:]: float(f[k]) for k in f.files if k.startswith("d_err_")}
    assert set(got) == set(ref) and len(ref) == 8
    for k in sorted(got):
        print(k, got[k], ref[k])
    np.testing.assert_allclose(got["our_repro"], ref["our_repro"], rtol=2e-5)
    np.testing.assert_allclose(got["triangulated_repro"], ref["triangulated_repro"], rtol=2e-5)
    # per-edge depths against the reference's (Ps @ pts3D_pred)[:, 2, :] at the edges
    Ps = np.linalg.inv(f["d_Ns"].astype(np.float64)) @ f["d_Ps_norm"].astype(np.float64)
    X = f["d_pts3D"].astype(np.float64)
    bound = 8 * U * np.einsum("ej,je->e", np.abs(Ps[f["d_cam"], 2, :]), np.abs(X / X[-1])[:, f["d_pt"]])
    depth, (cam_neg, pt_neg, stats) = _edge_depths(outputs["_device"], float(f["d_margin"]))
    err = np.abs(depth - f["d_depth"])
    print("depth: max err / bound", (err / bound).max())
    assert (err <= bound).all()
    assert stats[4].item() == depth.min() and stats[5].item() == depth.max()
    _check_depth_metrics(got, ref, bound)
    assert 0 < got["fraction_views_neg_depth_for_any_point"] < 1
    neg_pts = np.unique(f["d_pt"][f["d_depth"] < float(f["d_margin"])])
    assert np.array_equal(np.nonzero(pt_neg.cpu().numpy())[0], neg_pts)


def test_geometry_set_matches_reference(device):
    f = golden("eval_errors.npz")
    conf = DictConf(dataset__calibrated=True)
    data = _scene(f["g_M"], f["g_Ns"], f["g_y"], device)
    assert np.array_equal(data.x.indices.cpu().numpy(), np.stack([f["g_cam"], f["g_pt"]]))
    outputs = evaluation.prepare_predictions(data, _pred(f["g_Ps_norm"], f["g_pts3D"], device), conf, False)
    for k in ("Rs", "ts", "Rs_gt", "ts_gt"):
        np.testing.assert_allclose(outputs[k], f["g_" + k], rtol=1e-6, err_msg=k)
    assert outputs["cam_centers"] is outputs["ts"] and outputs["cam_centers_gt"] is outputs["ts_gt"]
    R_err, t_err = evaluation.translation_rotation_errors(outputs["Rs"], outputs["ts"], outputs["Rs_gt"],
                                                          outputs["ts_gt"])
    np.testing.assert_allclose(R_err, f["g_R_err"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(t_err, f["g_t_err"], rtol=1e-6)
    tri, ref_tri = outputs["pts3D_triangulated"], f["g_pts3D_triangulated"]
    assert tri.shape == ref_tri.shape and np.array_equal(np.isnan(tri), np.isnan(ref_tri))
    np.testing.assert_allclose(tri, ref_tri, rtol=1e-8, atol=1e-10)
    st = outputs["_device"]
    err = torch.empty(st["cam"].shape[0], dtype=torch.float32, device=device)
    _native.reproj_error(st["cam"], st["pt"], st["xy"], st["P"], st["X_tri"], err)
    np.testing.assert_allclose(err.cpu().numpy(), f["g_triangulated_edge_errors"], rtol=1e-4, atol=1e-3)
    got = evaluation.compute_errors(outputs, conf, False)
    np.testing.assert_allclose(got["triangulated_repro"], float(f["g_triangulated_repro"]), rtol=2e-5)
    np.testing.assert_allclose(got["our_repro"], float(f["g_our_repro"]), rtol=2e-5)
    # the aligned poses are at least as close as the raw ones were, and the shapes are the reference's
    assert got["t_err_mean"] <= f["g_t_err"].mean() and got["R_err_mean"] <= f["g_R_err"].mean() + 1e-9
    assert outputs["Rs_fixed"].shape == (8, 3, 3) and outputs["ts_fixed"].shape == (8, 3)
    assert outputs["pts3D_pred_fixed"].shape == outputs["pts3D_triangulated_fixed"].shape == (4, 60)
    C = outputs["cam_centers"]
    assert got["cam_centers_std"] == np.mean(np.linalg.norm(C - C.mean(), axis=1))


def _random_scene(with_nan_point):
    rng = np.random.default_rng(3)
    m, n = 40, 3000
    vis = rng.random((m, n)) < 0.15
    M = (rng.uniform(1, 1000, size=(m, 2, n)) * vis[:, None, :]).reshape(2 * m, n).astype(np.float32)
    K = np.array([[700, 0, 480], [0, 700, 360], [0, 0, 1]])
    Ns = np.repeat(np.linalg.inv(K)[None], m, 0).astype(np.float32)
    Ps = np.zeros((m, 3, 4), dtype=np.float32)
    Ps[:, :, :3] = np.eye(3) + 0.05 * rng.standard_normal((m, 3, 3))
    Ps[:, :, 3] = 0.2 * rng.standard_normal((m, 3))
    X = rng.standard_normal((4, n)).astype(np.float32)
    X[2] = 2 + 3 * rng.random(n)
    X[3] = 0.5 + rng.random(n)
    X[2, ::11] *= -1  # behind the cameras
    if with_nan_point:
        X[:, 5] = 0.0  # 0 / 0: NaN depth on every edge of point 5
    return M, Ns, Ps, X


@pytest.mark.parametrize("with_nan_point", [True, False])
def test_depth_metrics_match_dense_restatement_random_scene(device, with_nan_point):
    M, Ns, Ps_norm, X = _random_scene(with_nan_point)
    margin = 1e-4
    conf = DictConf(dataset__calibrated=False)
    data = _scene(M, Ns, None, device)
    idx = data.x.indices.cpu().numpy()
    vis = np.zeros((40, 3000), dtype=bool)
    vis[idx[0], idx[1]] = True
    Ps = np.linalg.inv(Ns.astype(np.float64)) @ Ps_norm.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref, depth_ref, bound = _dense_depth_metrics(Ps, X.astype(np.float64), vis, margin)
    assert vis[:, 5].sum() >= 2 and np.isnan(ref["point_depth_mean"]) == with_nan_point
    finite = depth_ref[vis][~np.isnan(depth_ref[vis])]
    assert np.abs(finite - margin).min() > 1e-3 and (finite < margin).any()  # no flag hangs on rounding
    pred = _pred(Ps_norm, X, device)
    outputs = evaluation.prepare_predictions(data, pred, conf, False)
    got = evaluation.compute_errors(outputs, conf, False)
    for k in DEPTH_KEYS:
        print(k, got[k], ref[k])
    _check_depth_metrics(got, ref, bound[vis])
    depth, first = _edge_depths(outputs["_device"], margin)
    np.testing.assert_array_equal(np.isnan(depth), np.isnan(depth_ref[idx[0], idx[1]]))
    ok = ~np.isnan(depth)
    assert (np.abs(depth - depth_ref[idx[0], idx[1]])[ok] <= bound[idx[0], idx[1]][ok]).all()
    depth2, second = _edge_depths(outputs["_device"], margin)
    assert depth.tobytes() == depth2.tobytes()
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    got2 = evaluation.compute_errors(outputs, conf, False)
    assert all(np.array_equal(got[k], got2[k], equal_nan=True) for k in got)


def test_depth_stats_hand_built_csr(device):
    """Camera 0: 300 edges (more than a workgroup of 256 and several waves), camera 1: none,
    camera 2: exactly one, camera 3: 50; points 300 and 301 unseen; point 0 seen by cameras 0 and
    2, so the point order is not the edge order (perm is not the identity).  Only the LAST edge of
    camera 0 has a negative depth."""
    m, n = 4, 302
    cam = np.concatenate([np.zeros(300), [2], np.full(50, 3)]).astype(np.int32)
    pt = np.concatenate([np.arange(300), [0], np.arange(1, 51)]).astype(np.int32)
    E = cam.shape[0]
    cam_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=m))]).astype(np.int32)
    pt_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n))]).astype(np.int32)
    perm = np.argsort(pt, kind="stable").astype(np.int32)
    assert not np.array_equal(perm, np.arange(E))
    P = np.zeros((m, 12), dtype=np.float32)
    P[:, 10] = 1.0  # depth = X_z / w
    X = np.zeros((4, n), dtype=np.float32)
    X[2], X[3] = 4.0, 2.0
    X[2, 299] = -2.0
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    depth = torch.empty(E, dtype=torch.float32, device=device)
    cam_neg, pt_neg, stats = _native.depth_stats(t(cam), t(pt), t(cam_ptr), t(pt_ptr), t(perm), t(P), t(X), 1e-4,
                                                 depth)
    want = np.full(E, 2.0, dtype=np.float32)
    want[299] = -1.0
    assert np.array_equal(depth.cpu().numpy(), want)
    assert cam_neg.cpu().tolist() == [1, 0, 0, 0]
    assert np.array_equal(np.nonzero(pt_neg.cpu().numpy())[0], [299])
    assert stats.cpu().tolist() == [1.0, 3.0, 300.0, 2.0 * (E - 1) - 1.0, -1.0, 2.0]
    # identity perm: edges already in point order (one camera)
    one = _native.depth_stats(t(cam[:300]), t(pt[:300]), t(np.array([0, 300], dtype=np.int32)),
                              t(np.minimum(np.arange(n + 1), 300).astype(np.int32)), None, t(P[:1]), t(X), 1e-4)
    assert one[0].cpu().tolist() == [1] and one[1].sum().item() == 1 and one[2].cpu().tolist()[:3] == [1.0, 1.0, 300.0]


def test_depth_stats_no_edges(device):
    e = torch.empty(0, dtype=torch.int32, device=device)
    z = lambda k: torch.zeros(k, dtype=torch.int32, device=device)  # noqa: E731
    cam_neg, pt_neg, stats = _native.depth_stats(e, e, z(3), z(4), None, torch.ones((2, 12), device=device),
                                                 torch.ones((4, 3), device=device), 1e-4)
    assert cam_neg.cpu().tolist() == [0, 0] and pt_neg.cpu().tolist() == [0, 0, 0]
    s = stats.cpu().numpy()
    assert s[:3].tolist() == [0.0, 0.0, 0.0] and np.isnan(s[3:]).all()


def test_epoch_evaluation_end_to_end_with_ba(device):
    f = golden("net_small.npz")
    s = golden("scene_config1.npz")
    sc = synthetic.config1()
    y = (sc.K[None] @ sc.Ps_gt().astype(np.float64)).astype(np.float32)
    data = _scene(s["M"], s["Ns"], y, device, "config1")
    net = gasfm_amd.GraphAttnSfMNet(gasfm_amd.conf.small_conf(2))
    net.load_state_dict({k[3:]: torch.from_numpy(f[k]).float() for k in f.files if k.startswith("sd/")})
    with torch.no_grad():
        pred = net.to(device)(data)
    conf = DictConf(dataset__calibrated=True, ba__repeat=True)
    outputs = evaluation.prepare_predictions(data, pred, conf, True)
    errors = evaluation.compute_errors(outputs, conf, True)
    for k in sorted(errors):
        print(k, errors[k])
    # the reference's dummy has neither ba_time nor the two camera-centre spreads (evaluation.py:368-432)
    dummy = set(evaluation.get_dummy_errors(conf, True))
    assert set(errors) == dummy | {"ba_time", "cam_centers_std", "cam_centers_gt_std"}
    assert all(np.isfinite(v) for v in errors.values()), errors
    assert errors["repro_ba"] <= errors["our_repro"]
    for k in ("Rs_ba", "ts_ba", "Xs_ba", "Ps_ba", "Rs_ba_fixed", "ts_ba_fixed", "Xs_ba_fixed", "Ks", "scene_name"):
        assert k in outputs, k
    assert outputs["Xs_ba"].shape == (4, 200) and outputs["Ps_ba"].shape == (10, 3, 4)
    assert "xs" not in outputs  # nothing needed the dense array
    xs = outputs["xs"]
    M = s["M"]
    assert np.array_equal(xs, M.reshape(10, 2, 200).transpose(0, 2, 1)) and "xs" in outputs
