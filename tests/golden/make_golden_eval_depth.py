"""Generate tests/golden/eval_depth.npz from the REFERENCE's own depth-head evaluation (build container only).

    python tests/golden/make_golden_eval_depth.py

Imports code/evaluation.py in place (tests/golden/refimport.py) and runs, on the CPU, with the depth
head on and ``eval.calc_reprojerr_with_gtposes_for_depth_pred`` on:

  compute_core_errors                    after np.random.seed(NP_SEED)      -> ``core_*``
  prepare_predictions + compute_errors   after np.random.seed(NP_SEED + 1)  -> ``full_*``

Scene: the calibrated scene of make_golden_depth.py (m = 6, n = 60, ragged tracks of 2 to 5 views),
built with ``store_depth_targets=True``.  Predicted depths: the ground truth x (1 + 5 % noise) x 3.7,
so the rescale by s_gt / s_pred matters.

The pairing the reference draws is recorded by wrapping
general_utils.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern for the duration of
each call: the source edge id rides as a fourth column of ``values`` on the way in and is stripped on
the way out; ``src[e']`` is the edge whose backprojected point lands at edge e'.

Recorded: the inputs (M, Ns, Ks = Ns_invT^T, y, dense depths, indices, predicted depths); per run
``src``, the reference's scalars (``<run>_err_<key>``) and their key order; for the full run the
per-edge ``errors`` and ``reproj_depths`` (before the division by s_gt) at the visible entries, s_pred
and s_gt; and the key lists of get_dummy_errors for the depth confs (``dummy_<depth><flag><explicit>``).
Data only.
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
from make_golden_depth import make_scene  # noqa: E402
from gasfm_amd.scene_device import _axis_angle_to_matrix  # noqa: E402

NP_SEED, NOISE, FACTOR = 5, 0.05, 3.7


def conf_dict(depth=True, flag=True, explicit=False, calibrated=True):
    return {"dataset": {"calibrated": calibrated},
            "model": {"view_head": {"enabled": explicit}, "scenepoint_head": {"enabled": explicit},
                      "depth_head": {"enabled": depth}},
            "eval": {"calc_reprojerr_with_gtposes_for_depth_pred": flag},
            "loss": {"infinity_pts_margin": 1e-4},
            "ba": {"repeat": False, "triangulation": False, "print_out": False}}


class Recorder:
    """Wraps the reference's shuffle: src per destination edge, in the order of ``indices`` (cam-major)."""

    def __init__(self, general_utils, edge_of):
        self.gu, self.edge_of, self.src = general_utils, edge_of, None
        self.orig = general_utils.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern

    def __enter__(self):
        def wrapped(values, indices, shuffle_axis=0):
            ids = np.array([self.edge_of[(int(c), int(p))] for c, p in indices.T], dtype=np.float64)
            vals, idx = self.orig(np.concatenate([values, ids[:, None]], 1), indices, shuffle_axis)
            src = np.full(len(self.edge_of), -1, dtype=np.int32)
            for (c, p), s in zip(idx.T, vals[:, 3]):
                src[self.edge_of[(int(c), int(p))]] = int(s)
            self.src = src
            return vals[:, :3], idx

        self.gu.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern = wrapped
        return self

    def __exit__(self, *exc):
        self.gu.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern = self.orig
        return False


def main():
    sys.modules["PyCeres"] = types.ModuleType("PyCeres")
    ref = refimport.load()
    ref.SceneData.axis_angle_to_matrix = _axis_angle_to_matrix
    evaluation = importlib.import_module("evaluation")
    general_utils = importlib.import_module("utils.general_utils")
    M, Ns, Ps, vis = make_scene()
    data = ref.SceneData.SceneData(M, Ns, Ps, "synthetic_depth", calibrated=True, store_depth_targets=True)
    idx = data.x.indices
    E = idx.shape[1]
    edge_of = {(int(c), int(p)): e for e, (c, p) in enumerate(idx.T.tolist())}
    rng = np.random.default_rng(17)
    d_gt = data.depths[idx[0], idx[1]]
    d_pred = (d_gt.double() * torch.from_numpy((1 + NOISE * rng.standard_normal(E)) * FACTOR)).float()
    depths = ref.sparse_utils.SparseMat(d_pred[:, None], idx, data.x.cam_per_pts, data.x.pts_per_cam,
                                        (data.x.shape[0], data.x.shape[1], 1))
    pred = {"depths": depths}
    conf = refimport.DictConf(conf_dict())
    out = {"M": data.M, "Ns": data.Ns, "Ks": data.Ns_invT.transpose(1, 2), "y": data.y, "depths": data.depths,
           "indices": idx, "d_pred": d_pred, "params": np.array([NP_SEED, NOISE, FACTOR])}

    with Recorder(general_utils, edge_of) as rec:
        np.random.seed(NP_SEED)
        core = evaluation.compute_core_errors(data, pred, conf)
    out["core_src"] = rec.src
    with Recorder(general_utils, edge_of) as rec:
        np.random.seed(NP_SEED + 1)
        outputs = evaluation.prepare_predictions(data, pred, conf, False)
        full = evaluation.compute_errors(outputs, conf, False)
    out["full_src"] = rec.src
    assert not np.array_equal(out["core_src"], out["full_src"])
    for src in (out["core_src"], out["full_src"]):
        assert (src >= 0).all() and (src != np.arange(E)).all() and np.array_equal(np.sort(src), np.arange(E))
        assert np.array_equal(idx[1].numpy()[src], idx[1].numpy())
    # the per-edge values of the full run: the same call compute_errors makes, with the recorded pairing
    geo = importlib.import_module("utils.geo_utils")
    fixed = rec.src

    def replay(values, indices, shuffle_axis=0):
        order = np.array([edge_of[(int(c), int(p))] for c, p in indices.T])
        by_edge = np.empty_like(values)
        by_edge[order] = values
        return by_edge[fixed][order], indices  # position of edge e' receives the value of src[e']

    general_utils.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern = replay
    try:
        errs, rdep = geo.reprojection_error_backproj_random_view_pairs(
            outputs["Ks"], outputs["Ps_gt"], outputs["depths_pred_dense"] / outputs["s_pred"] * outputs["s_gt"],
            outputs["xs"], visible_points=None, calc_reproj_depths=True)
    finally:
        general_utils.shuffle_coo_matrix_along_axis_while_preserving_sparsity_pattern = rec.orig
    c, p = idx[0].numpy(), idx[1].numpy()
    assert np.nanmean(errs) == full["repro_backproj_rnd_gt_2view"], (np.nanmean(errs), full)
    assert (rdep[c, p] / outputs["s_gt"]).mean() == full["repro_backproj_depth_norm_mean_rnd_gt_2view"]
    out.update(full_errors=errs[c, p], full_reproj_depths=rdep[c, p], s_pred=outputs["s_pred"], s_gt=outputs["s_gt"])
    for tag, d in (("core", core), ("full", full)):
        out[f"{tag}_keys"] = np.array(list(d))
        for k, v in d.items():
            out[f"{tag}_err_{k}"] = np.float64(v)
        print(tag, {k: float(v) for k, v in d.items()})
    for depth in (0, 1):
        for flag in (0, 1):
            for explicit in (0, 1):
                keys = evaluation.get_dummy_errors(
                    refimport.DictConf(conf_dict(bool(depth), bool(flag), bool(explicit))), False)
                out[f"dummy_{depth}{flag}{explicit}"] = np.array(list(keys), dtype=str)
    path = os.path.join(HERE, "eval_depth.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
