"""Host-side parts of the scene evaluation (gasfm_amd/evaluation.py): get_dummy_errors' key sets
against the reference's (tests/golden/eval_errors.npz, make_golden_eval.py), the scale /
translation fit of align_cameras, and ba._Edges built from an edge list.

The alignment has no reference fixture (the reference solves it with cvxpy, absent offline), so it
is held to what defines it: (a) an exact similarity transform is recovered; (b) with noise the
returned (c, t) is a stationary point of  sum_i || g_i - (c p_i + t) ||  (convex: the minimum) and
no worse than the closed-form least-squares fit.
"""
import numpy as np
import torch

from conftest import golden
from gasfm_amd import ba, evaluation, synthetic


class DictConf:
    def __init__(self, **kw):
        self.d = {"model.view_head.enabled": True, "model.scenepoint_head.enabled": True,
                  "eval.calc_reprojerr_with_gtposes_for_depth_pred": False, "loss.infinity_pts_margin": 1e-4,
                  "ba.triangulation": False, "ba.print_out": False}
        self.d.update({k.replace("__", "."): v for k, v in kw.items()})

    def _get(self, key, *default, **kw):
        if key in self.d:
            return self.d[key]
        if default or "default" in kw:
            return default[0] if default else kw["default"]
        raise KeyError(key)

    get_bool = get_float = get_int = get_string = _get


def test_dummy_errors_keys_match_reference():
    f = golden("eval_errors.npz")
    for cal in (0, 1):
        for use_ba in (0, 1):
            for rep in (0, 1):
                conf = DictConf(dataset__calibrated=bool(cal), ba__repeat=bool(rep))
                got = evaluation.get_dummy_errors(conf, bool(use_ba))
                assert list(got) == [str(k) for k in f[f"dummy_{cal}{use_ba}{rep}"]], (cal, use_ba, rep)
                assert all(np.isnan(v) for v in got.values())


def _poses(m, seed):
    rng = np.random.default_rng(seed)
    Rs = ba.rodrigues_to_matrix(torch.from_numpy(rng.standard_normal((m, 3)))).numpy()
    return rng, Rs, 3.0 * rng.standard_normal((m, 3))


def _similarity(rng):
    R0 = ba.rodrigues_to_matrix(torch.from_numpy(rng.standard_normal(3))).numpy()
    return R0, 2.5, np.array([0.7, -1.3, 2.1])


def test_alignment_exact_similarity():
    rng, Rs_gt, ts_gt = _poses(12, 0)
    R0, c0, t0 = _similarity(rng)
    # gt = similarity(pred):  R_gt = R0 R_pred,  C_gt = c0 R0 C_pred + t0
    Rs_pred = R0.T[None] @ Rs_gt
    ts_pred = (ts_gt - t0) @ R0 / c0
    Rs_fixed, ts_fixed, sim = evaluation.align_cameras(Rs_pred, Rs_gt, ts_pred, ts_gt, return_alignment=True)
    R_err, t_err = evaluation.translation_rotation_errors(Rs_fixed, ts_fixed, Rs_gt, ts_gt)
    spread = np.linalg.norm(ts_gt - ts_gt.mean(0), axis=1).mean()
    assert t_err.max() <= 1e-6 * spread and R_err.max() <= 1e-4
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = c0 * R0, t0
    np.testing.assert_allclose(sim, want, atol=1e-6, rtol=0)
    # without return_alignment: the two arrays only
    assert len(evaluation.align_cameras(Rs_pred, Rs_gt, ts_pred, ts_gt)) == 2


def test_alignment_noisy_stationary():
    for m, seed in ((10, 1), (200, 2)):
        rng, Rs_gt, g = _poses(m, seed)
        R0, c0, t0 = _similarity(rng)
        p = (g - t0) @ R0 / c0 + 0.2 * rng.standard_normal((m, 3))
        p[0] += 5.0  # an outlier: the unsquared norms and least squares disagree
        Rs_pred = R0.T[None] @ Rs_gt
        Rs_fixed, ts_fixed, sim = evaluation.align_cameras(Rs_pred, Rs_gt, p, g, return_alignment=True)
        assert not np.array_equal(sim, np.eye(4))
        R_opt = Rs_fixed[0] @ Rs_pred[0].T
        c = np.cbrt(np.linalg.det(sim[:3, :3]))
        t = sim[:3, 3]
        q = p @ R_opt.T
        np.testing.assert_allclose(ts_fixed, c * q + t, atol=1e-12)
        res = g - (c * q + t)
        u = res / np.linalg.norm(res, axis=1, keepdims=True)
        grad = -np.concatenate([[(u * q).sum()], u.sum(0)])
        S = np.linalg.norm(g - g.mean(0), axis=1).sum()
        assert np.linalg.norm(grad) <= 1e-8 * S, (np.linalg.norm(grad), S)
        c_ls, t_ls = evaluation.least_squares_scale_translation(g, q)
        f = np.linalg.norm(res, axis=1).sum()
        f_ls = np.linalg.norm(g - (c_ls * q + t_ls), axis=1).sum()
        assert f <= f_ls and f < f_ls * (1 - 1e-6)


def test_alignment_failure_returns_predictions_unchanged(capsys):
    rng, Rs, ts = _poses(5, 3)
    bad = ts.copy()
    bad[2, 1] = np.nan
    R, t, sim = evaluation.align_cameras(Rs, Rs, bad, ts, return_alignment=True)
    assert np.array_equal(sim, np.eye(4)) and np.array_equal(R, Rs) and np.array_equal(t, bad, equal_nan=True)
    Rn = Rs.copy()
    Rn[0, 0, 0] = np.nan
    R, t, sim = evaluation.align_cameras(Rn, Rs, ts, ts, return_alignment=True)
    assert np.array_equal(sim, np.eye(4)) and np.array_equal(t, ts)
    assert "alignment failed" in capsys.readouterr().out


def test_edges_from_list_equal_edges_from_dense():
    sc = synthetic.ba_scene(7, 60, 3, noise_px=0.3, seed=11)
    xs = torch.from_numpy(sc["xs"])
    xs[:, 7] = 0.0      # a point nobody sees
    xs[1:, 9] = 0.0     # seen once: not a valid point
    a = ba._Edges(xs)
    c, p = torch.nonzero(ba.valid_points(xs), as_tuple=True)
    assert a.cidx.shape[0] > 100
    b = ba._Edges.from_edges(c.to(torch.int32), p.to(torch.int32), xs[c, p].float().double(), 7, 60)
    for name in ("cidx", "pidx", "pt_ptr", "perm", "c32", "vis"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and torch.equal(x, y), name
    assert (a.m, a.n) == (b.m, b.n) and b.obs.dtype == a.obs.dtype
    torch.testing.assert_close(b.obs, a.obs, rtol=1e-7, atol=0)  # through fp32, as the scene's pixels are
