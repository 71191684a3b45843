"""Generate tests/golden/eval_errors.npz from the REFERENCE's own evaluation (build container only).

    python tests/golden/make_golden_eval.py

Imports code/evaluation.py in place (tests/golden/refimport.py; PyCeres stubbed as in
make_golden_repro.py) and runs ``prepare_predictions`` + ``compute_errors`` with
``dataset.calibrated = False`` and ``bundle_adjustment = False`` (the calibrated branch solves its
alignment with cvxpy, which is absent offline; nothing of this project stands in for it).

Depth set (``d_*``): the config-1 scene with make_golden_repro's predictions (cameras near
identity) and every third point camera 0 does not see mirrored behind the cameras.  Saved: the
inputs (fp32 values, handed to the reference as float64), the reference's whole compute_errors dict (``d_err_<key>``) and (Ps @ pts3D_pred)[:, 2, :]
at the edges.  The script asserts that some but not all views and points have a negative depth
and that no visible depth is within 1e-3 of the margin (fp32 rounding cannot flip a flag).

Geometry set (``g_*``): config 1 has random pixels and identical ground-truth cameras, so a DLT
on it is degenerate; this set uses synthetic.ba_scene (cameras on a circle, true projections
+ 0.3 px noise).  Ps_norm = K^-1 Ps_gt plus small noise, points near their true positions, all
fp32 values; the reference is handed them as float64 so its own numpy work is fp64.  Saved: its
pts3D_triangulated, triangulated_repro, our_repro, decompose_camera_matrix of the prediction and
of the ground truth, and tranlsation_rotation_errors on those (unaligned) poses.

``dummy_<calibrated><ba><repeat>``: the key lists of the reference's get_dummy_errors.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import refimport  # noqa: E402
from gasfm_amd import synthetic  # noqa: E402  (input generation only)
from make_golden_repro import predictions  # noqa: E402

MARGIN = 1e-4


def conf_dict(calibrated, repeat=True):
    return {"dataset": {"calibrated": calibrated},
            "model": {"view_head": {"enabled": True}, "scenepoint_head": {"enabled": True}},
            "eval": {"calc_reprojerr_with_gtposes_for_depth_pred": False},
            "loss": {"infinity_pts_margin": MARGIN},
            "ba": {"repeat": repeat, "triangulation": False, "print_out": False}}


def depth_set(ref, evaluation, out):
    sc = synthetic.config1()
    # fp32 values handed over as float64, so the reference's numpy work (its DLT too) is fp64
    M, Ns = torch.from_numpy(sc.dense_M()).double(), torch.from_numpy(sc.Ns()).double()
    data = ref.SceneData.SceneData(M, Ns, torch.from_numpy(sc.Ps_gt()).double(), "synthetic_config1",
                                   calibrated=True)
    m, n = data.x.shape[0], data.x.shape[1]
    cam, pt = data.x.indices[0].numpy(), data.x.indices[1].numpy()
    Ps_norm, pts3D = predictions(m, n)
    unseen0 = np.setdiff1d(np.arange(n), pt[cam == 0])
    flipped = unseen0[::3]
    pts3D[2, flipped] *= -1  # behind the (near-identity) cameras
    conf = refimport.DictConf(conf_dict(False))
    outputs = evaluation.prepare_predictions(data, {"Ps_norm": Ps_norm.double(), "pts3D": pts3D.double()}, conf,
                                             False)
    errors = evaluation.compute_errors(outputs, conf, False)
    depth = (outputs["Ps"] @ outputs["pts3D_pred"])[:, 2, :][cam, pt]
    neg = depth < MARGIN
    assert 0 < errors["fraction_views_neg_depth_for_any_point"] < 1, errors
    assert np.setdiff1d(np.arange(n), pt[neg]).size > 0 and neg.any()
    assert np.abs(depth - MARGIN).min() > 1e-3, np.abs(depth - MARGIN).min()
    print("depth set:", {k: float(v) for k, v in errors.items()}, "min |depth - margin|",
          np.abs(depth - MARGIN).min())
    out.update(d_M=data.M.numpy().astype(np.float32), d_Ns=Ns.numpy().astype(np.float32), d_Ps_norm=Ps_norm.numpy(), d_pts3D=pts3D.numpy(), d_cam=cam,
               d_pt=pt, d_depth=depth, d_margin=np.float64(MARGIN), d_flipped=flipped)
    for k, v in errors.items():
        out["d_err_" + k] = np.float64(v)


def geometry_set(ref, evaluation, geo_utils, out):
    sc = synthetic.ba_scene(8, 60, 3, noise_px=0.3, seed=5)
    m, n = sc["xs"].shape[:2]
    rng = np.random.default_rng(6)
    M = sc["xs"].transpose(0, 2, 1).reshape(2 * m, n).astype(np.float32)
    Ns = np.linalg.inv(sc["Ks"]).astype(np.float32)
    Rt = np.concatenate([sc["Rs"].transpose(0, 2, 1), -(sc["Rs"].transpose(0, 2, 1) @ sc["ts"][:, :, None])], 2)
    y = (sc["Ks"] @ Rt).astype(np.float32)
    Ps_norm = (Rt + 2e-3 * rng.standard_normal(Rt.shape)).astype(np.float32)
    w = 0.5 + rng.random(n)
    X = sc["Xs"].T + 5e-3 * rng.standard_normal((3, n))
    pts3D = np.concatenate([X * w, w[None]]).astype(np.float32)
    f64 = lambda a: torch.from_numpy(a.astype(np.float64))  # noqa: E731
    data = ref.SceneData.SceneData(f64(M), f64(Ns), f64(y), "ba_scene", calibrated=True)
    conf = refimport.DictConf(conf_dict(False))
    pred = {"Ps_norm": f64(Ps_norm), "pts3D": f64(pts3D)}
    outputs = evaluation.prepare_predictions(data, pred, conf, False)
    errors = evaluation.compute_errors(outputs, conf, False)
    Ks = data.Ns_invT.transpose(1, 2).numpy()
    Rs_gt, ts_gt = geo_utils.decompose_camera_matrix(data.y.numpy(), Ks, inverse_direction_camera2global=True)
    Rs, ts = geo_utils.decompose_camera_matrix(outputs["Ps_norm"], inverse_direction_camera2global=True)
    R_err, t_err = geo_utils.tranlsation_rotation_errors(Rs, ts, Rs_gt, ts_gt)
    tri = outputs["pts3D_triangulated"]
    assert tri is not None and np.isfinite(tri).all()
    print("geometry set: our_repro", errors["our_repro"], "triangulated_repro", errors["triangulated_repro"],
          "R_err", R_err.mean(), "t_err", t_err.mean())
    cam, pt = data.x.indices[0].numpy(), data.x.indices[1].numpy()
    xs = geo_utils.M_to_xs(data.M.numpy())
    tri_edge = geo_utils.reprojection_error_with_points(outputs["Ps"], tri.T, xs)[cam, pt]
    out.update(g_M=M, g_Ns=Ns, g_y=y, g_Ps_norm=Ps_norm, g_pts3D=pts3D, g_cam=cam, g_pt=pt,
               g_pts3D_triangulated=tri, g_triangulated_edge_errors=tri_edge,
               g_triangulated_repro=np.float64(errors["triangulated_repro"]),
               g_our_repro=np.float64(errors["our_repro"]), g_Rs=Rs, g_ts=ts, g_Rs_gt=Rs_gt, g_ts_gt=ts_gt,
               g_R_err=R_err, g_t_err=t_err)


def main():
    sys.modules["PyCeres"] = types.ModuleType("PyCeres")
    ref = refimport.load()
    evaluation = importlib.import_module("evaluation")
    geo_utils = importlib.import_module("utils.geo_utils")
    out = {}
    depth_set(ref, evaluation, out)
    geometry_set(ref, evaluation, geo_utils, out)
    for cal in (0, 1):
        for ba in (0, 1):
            for rep in (0, 1):
                keys = evaluation.get_dummy_errors(refimport.DictConf(conf_dict(bool(cal), bool(rep))), bool(ba))
                out[f"dummy_{cal}{ba}{rep}"] = np.array(list(keys))
    path = os.path.join(HERE, "eval_errors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
