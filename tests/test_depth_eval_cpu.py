"""Depth-head evaluation without a GPU: the torch restatements of gasfm_amd/depth_eval against the
reference's own results (tests/golden/eval_depth.npz, make_golden_eval_depth.py), the pairing's
properties, the header as the binding reads it, and the confs that still raise.

Bars against the reference.  U = 2^-24.

* Per edge, with the reference's pairing and the reference's own fp32 rescaled depths
  ``(d / s_pred) * s_gt`` handed in (scale 1): the fp64 restatement matches an independent fp64 numpy
  restatement of geo_utils.py:393-464 (``np_2view`` below) to 1e-9 relative.  The reference itself does
  not meet 1e-9 against fp64: decompose_camera_matrix computes ``np.linalg.inv(Ks) @ Ps`` on float32
  arrays, so its R^T and camera centres are float32 results, and its reprojected depth applies the same
  float32 ``inv(Ks)``.  ``np_2view(ref_steps=True)`` repeats exactly these float32 steps; STEP = the
  largest per-edge change they cause (measured: 7.0e-5 px on errors of 1 to 60 px, 2.3e-7 on depths of
  about 4).  Against the recorded ``errors`` / ``reproj_depths`` the bar is 2 STEP + 1e-9 |value| (2: a
  float32 LAPACK inverse need not round alike everywhere); it is the reference's own rounding and
  does not depend on the code under test.
* The scalars go through evaluation.py, which computes the scales itself in fp64.  The reference's
  fp32 steps are: s_pred, s_gt = torch.mean in fp32; d / s_pred and (.) * s_gt in fp32; the
  normalised depths, their quantiles (np.quantile's lerp on a float32 array) and their means
  (numpy's pairwise float32 sum, <= ceil(log2 E) + 1 = 9 roundings at E = 190) in fp32.  The scale
  errors EPS_P, EPS_G are taken from the fixture (the recorded fp32 means against the fp64 means of
  the recorded inputs), so
    depth_*_norm_*      relative  EPS + 12 U   (1 division + 3 lerp + 9 mean, rounded up to 12)
    depth_pred_err_mean absolute  (EPS_P + EPS_G + 4 U) max|normalised depth| + 12 U |value|
    2-view values       a depth moves by EPS_D = EPS_P + EPS_G + 2 U relative; its effect on each edge's
                        error / reprojected depth is the derivative with respect to a common factor on
                        the depths, taken by central differences of an independent fp64 numpy
                        restatement in this file; means use the mean derivative, min / max / quantiles the
                        largest; the normalised reprojected depths add EPS_G + U relative; all add
                        2 STEP.
"""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import REPO, golden
from gasfm_amd import _abi, _native, depth_eval, evaluation
from gasfm_amd.build import DEPTH_EVAL_HEADER, LIB
from gasfm_amd.depth_eval import _binding

U = 2.0 ** -24
TRACK_LENGTHS = (1, 2, 3, 63, 64, 65, 130, 1000)


class DictConf:
    def __init__(self, depth=True, flag=True, explicit=False, calibrated=True):
        self.d = {"dataset.calibrated": calibrated, "model.view_head.enabled": explicit,
                  "model.scenepoint_head.enabled": explicit, "model.depth_head.enabled": depth,
                  "eval.calc_reprojerr_with_gtposes_for_depth_pred": flag, "loss.infinity_pts_margin": 1e-4,
                  "ba.repeat": False, "ba.triangulation": False, "ba.print_out": False}

    def _get(self, key, *default, **kw):
        if key in self.d:
            return self.d[key]
        if default or "default" in kw:
            return default[0] if default else kw["default"]
        raise KeyError(key)

    get_bool = get_float = get_int = get_string = _get


def fixture_scene(f, device="cpu", dense_targets=True):
    """The fixture's scene as this project's SceneData, with the reference's Ks (Ns_invT^T)."""
    t = lambda k: torch.from_numpy(np.ascontiguousarray(f[k]))  # noqa: E731
    data = gasfm_amd.SceneData(t("M"), t("Ns"), t("y"), "synthetic_depth")
    assert np.array_equal(data.x.indices.numpy(), f["indices"])
    data.Ns_invT = t("Ks").transpose(1, 2).contiguous()
    c, p = f["indices"]
    data.depths = t("depths") if dense_targets else torch.from_numpy(f["depths"][c, p].copy())
    return data.to(device) if device != "cpu" else data


def np_2view(f, depth, src, ref_steps=False):
    """Independent fp64 numpy restatement of geo_utils.py:393-464 on the edges: (err, reproj_depth).
    ``ref_steps``: with the reference's float32 ``np.linalg.inv(Ks) @ Ps`` for the backprojection and
    its float32 ``inv(Ks)`` applied to Ps X for the reprojected depth."""
    c, p = f["indices"]
    K, P = f["Ks"].astype(np.float64), f["y"].astype(np.float64)
    Rt = np.linalg.inv(K) @ P
    if ref_steps:
        Kinv32 = np.linalg.inv(f["Ks"])
        assert Kinv32.dtype == np.float32
        Rt_exact, Rt = Rt, (Kinv32 @ f["y"]).astype(np.float64)
    xy = np.stack([f["M"][2 * c, p], f["M"][2 * c + 1, p]], 1).astype(np.float64)
    cs = c[src]
    xn = np.einsum("eij,ej->ei", np.linalg.inv(K)[cs], np.concatenate([xy[src], np.ones((len(c), 1))], 1))
    loc = np.concatenate([xn[:, :2] / xn[:, 2:], np.ones((len(c), 1))], 1) * depth[src][:, None]
    X = np.einsum("eji,ej->ei", Rt[cs][:, :, :3], loc - Rt[cs][:, :, 3])
    if ref_steps:
        Rt = Rt_exact
    q = np.einsum("eij,ej->ei", Rt[c][:, :, :3], X) + Rt[c][:, :, 3]
    y = np.einsum("eij,ej->ei", K[c], q)
    if ref_steps:
        q = np.einsum("eij,ej->ei", Kinv32.astype(np.float64)[c], y)
    return np.linalg.norm(xy - y[:, :2] / y[:, 2:], axis=1), q[:, 2]


def ref_depths(f):
    """The depths the reference backprojects with: its own fp32 steps (evaluation.py:243, 282)."""
    return (f["d_pred"] / f["s_pred"]) * f["s_gt"]


def scale_errors(f):
    c, p = f["indices"]
    sp, sg = f["d_pred"].astype(np.float64).mean(), f["depths"][c, p].astype(np.float64).mean()
    return abs(float(f["s_pred"]) - sp) / sp, abs(float(f["s_gt"]) - sg) / sg


def sensitivities(f, src):
    """|d err / d ln k|, |d rdepth / d ln k| per edge for a common factor k on the depths."""
    d, h = ref_depths(f).astype(np.float64), 1e-6
    (e1, r1), (e0, r0) = np_2view(f, d * (1 + h), src), np_2view(f, d * (1 - h), src)
    return np.abs(e1 - e0) / (2 * h), np.abs(r1 - r0) / (2 * h)


def step_errors(f, src):
    """STEP of the module docstring: (on the errors, on the reprojected depths)."""
    d = ref_depths(f).astype(np.float64)
    (e1, r1), (e0, r0) = np_2view(f, d, src, ref_steps=True), np_2view(f, d, src)
    return np.abs(e1 - e0).max(), np.abs(r1 - r0).max()


# ------------------------------------------------------------------ restatements against the reference
def test_numpy_restatement_is_the_reference():
    f = golden("eval_depth.npz")
    step_e, step_r = step_errors(f, f["full_src"])
    print("STEP", step_e, step_r)
    assert 0 < step_e < 1e-3 and 0 < step_r < 1e-5  # float32 roundings of O(1) camera entries, not more
    err, rd = np_2view(f, ref_depths(f).astype(np.float64), f["full_src"])
    assert (np.abs(err - f["full_errors"]) <= 2 * step_e + 1e-9 * f["full_errors"]).all()
    assert (np.abs(rd - f["full_reproj_depths"]) <= 2 * step_r + 1e-9 * f["full_reproj_depths"]).all()


def test_2view_restatement_matches_reference_per_edge():
    f = golden("eval_depth.npz")
    data = fixture_scene(f)
    (cam, pt), _, _, _, _ = evaluation._edge_tensors(data)
    xy = evaluation._pixel_measurements(data)
    tab = evaluation._camera_table(data, torch.float64, torch.device("cpu"))
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (6, depth_eval.CAMTAB_FLOATS)
    assert evaluation._camera_table(data, torch.float64, torch.device("cpu")) is tab  # cached per scene
    d = torch.from_numpy(ref_depths(f))
    assert d.dtype == torch.float32
    err, rd, tot = depth_eval.backproj_2view_torch(cam, pt, xy, d, torch.ones(()), torch.from_numpy(f["full_src"]), tab)
    assert err.dtype == torch.float64
    want_e, want_r = np_2view(f, ref_depths(f).astype(np.float64), f["full_src"])
    np.testing.assert_allclose(err.numpy(), want_e, rtol=1e-9)
    np.testing.assert_allclose(rd.numpy(), want_r, rtol=1e-9)
    step_e, step_r = step_errors(f, f["full_src"])
    assert (np.abs(err.numpy() - f["full_errors"]) <= 2 * step_e + 1e-9 * f["full_errors"]).all()
    assert (np.abs(rd.numpy() - f["full_reproj_depths"]) <= 2 * step_r + 1e-9 * f["full_reproj_depths"]).all()
    ref_mean = float(f["full_err_repro_backproj_rnd_gt_2view"])
    assert abs(float(tot[0] / tot[1]) - ref_mean) <= 2 * step_e + 1e-9 * ref_mean
    assert int(tot[1]) == cam.shape[0]
    # an in-place edit of y rebuilds the table
    data.y.mul_(1.0)
    assert evaluation._camera_table(data, torch.float64, torch.device("cpu")) is not tab


def test_2view_restatement_refuses_to_follow_bad_sources():
    f = golden("eval_depth.npz")
    data = fixture_scene(f)
    (cam, pt), _, _, _, _ = evaluation._edge_tensors(data)
    xy = evaluation._pixel_measurements(data)
    tab = evaluation._camera_table(data, torch.float64, torch.device("cpu"))
    E = cam.shape[0]
    src = torch.from_numpy(f["full_src"].copy())
    other = int(np.nonzero((f["indices"][1] != f["indices"][1][3]) & (np.arange(E) != int(src[5])))[0][0])
    src[0], src[1], src[2], src[3] = -1, E, -7, other  # 3: an edge of another track
    d = torch.from_numpy(ref_depths(f)).clone()
    d[int(src[5])] = float("nan")
    err, rd, tot = depth_eval.backproj_2view_torch(cam, pt, xy, d, torch.ones(()), src, tab)
    bad = [0, 1, 2, 3, 5]
    assert torch.isnan(err[bad]).all() and torch.isnan(rd[bad]).all()
    assert int(tot[1]) == E - len(bad) and int(torch.isnan(err).sum()) == len(bad)
    np.testing.assert_allclose(float(tot[0]), float(err[~torch.isnan(err)].sum()), rtol=1e-12)
    # pt None: the pairing is trusted, edge 3 follows its source
    err2, _, _ = depth_eval.backproj_2view_torch(cam, None, xy, d, torch.ones(()), src, tab)
    assert not torch.isnan(err2[3])


def check_scalars(f, got, tag, src, kernel_err=0.0, kernel_rd=0.0, kernel_rel=0.0):
    """``kernel_*``: what a float32 path may add (tests/test_gpu_depth_eval.py): absolute per-edge bars on
    the error and the reprojected depth, and a relative one on the normalised depths."""
    eps_p, eps_g = scale_errors(f)
    eps_p, eps_g = eps_p + kernel_rel, eps_g + kernel_rel
    step_extra = (kernel_err, kernel_rd)
    eps_d = eps_p + eps_g + 2 * U
    s_err, s_rd = sensitivities(f, src)
    step_e, step_r = (a + b / 2 for a, b in zip(step_errors(f, src), step_extra))
    s_gt = float(f["s_gt"])
    ref = {str(k): float(f[f"{tag}_err_{k}"]) for k in f[f"{tag}_keys"]}
    assert list(got) == list(ref)
    a_max = (f["d_pred"] / f["s_pred"]).max()
    for k, r in ref.items():
        if k.startswith("depth_pred_norm"):
            bar = (eps_p + 12 * U) * abs(r)
        elif k.startswith("depth_gt_norm"):
            bar = (eps_g + 12 * U) * abs(r)
        elif k == "depth_pred_err_mean":
            bar = (eps_p + eps_g + 4 * U) * a_max + 12 * U * abs(r)
        elif k == "repro_backproj_rnd_gt_2view":
            bar = s_err.mean() * eps_d + 2 * step_e + 1e-9 * abs(r)
        elif "depth_norm_mean" in k:
            bar = (s_rd.mean() * eps_d + 2 * step_r) / s_gt + (eps_g + U) * abs(r) + 1e-9 * abs(r)
        else:
            bar = (s_rd.max() * eps_d + 2 * step_r) / s_gt + (eps_g + U) * abs(r) + 1e-9 * abs(r)
        print(f"{k}: got {got[k]!r} ref {r!r} diff {abs(got[k] - r):.3e} bar {bar:.3e}")
        assert abs(got[k] - r) <= bar, (k, got[k], r, bar)


@pytest.mark.parametrize("dense_targets", [True, False])
def test_evaluation_scalars_match_reference(dense_targets):
    f = golden("eval_depth.npz")
    data = fixture_scene(f, dense_targets=dense_targets)
    conf = DictConf()
    E = f["indices"].shape[1]
    vals = torch.from_numpy(f["d_pred"]).double()
    depths = gasfm_amd.scene.SparseMat(vals[:, None], data.x.indices, data.x.cam_per_pts, data.x.pts_per_cam, (6, 60, 1))
    core = evaluation.compute_core_errors(data, {"depths": depths}, conf, pairing=f["core_src"])
    check_scalars(f, core, "core", f["core_src"])
    # a plain [E] tensor instead of the SparseMat, no Ps_norm / pts3D: a depth-only model
    outputs = evaluation.prepare_predictions(data, {"depths": vals}, conf, False)
    assert outputs["Ps_gt"].shape == (6, 3, 4) and "Ps" not in outputs
    eps_p, eps_g = scale_errors(f)
    np.testing.assert_allclose(outputs["s_pred"], float(f["s_pred"]), rtol=eps_p + 1e-12)
    np.testing.assert_allclose(outputs["s_gt"], float(f["s_gt"]), rtol=eps_g + U)  # targets are fp32 here
    full = evaluation.compute_errors(outputs, conf, False, pairing=f["full_src"])
    check_scalars(f, full, "full", f["full_src"])
    # the dense arrays of the reference appear on first access only
    assert "depths_pred_dense" not in outputs and "depths_gt_dense" not in outputs
    c, p = f["indices"]
    dense = outputs["depths_pred_dense"]
    assert dense.shape == (6, 60) and np.array_equal(dense[c, p], f["d_pred"].astype(np.float64))
    assert np.count_nonzero(dense) == E
    assert np.array_equal(outputs["depths_gt_dense"][c, p], f["depths"][c, p])
    if dense_targets:
        assert np.array_equal(outputs["depths_gt_dense"], f["depths"], equal_nan=True)


def test_random_pairing_is_seeded_and_stays_in_the_tracks():
    f = golden("eval_depth.npz")
    data = fixture_scene(f)
    conf = DictConf()
    pred = {"depths": torch.from_numpy(f["d_pred"])}
    torch.manual_seed(3)
    a = evaluation.compute_core_errors(data, pred, conf)
    torch.manual_seed(3)
    b = evaluation.compute_core_errors(data, pred, conf)
    c = evaluation.compute_core_errors(data, pred, conf)
    assert a == b and a != c and list(a) == ["repro_backproj_rnd_gt_2view"]
    # 5 % depth noise at ~4 units from a 700 px camera: tens of pixels, like the reference's draws
    assert 5 < a["repro_backproj_rnd_gt_2view"] < 100


def test_dummy_errors_keys_match_reference():
    f = golden("eval_depth.npz")
    for depth in (0, 1):
        for flag in (0, 1):
            for explicit in (0, 1):
                got = evaluation.get_dummy_errors(DictConf(bool(depth), bool(flag), bool(explicit)), False)
                assert list(got) == [str(k) for k in f[f"dummy_{depth}{flag}{explicit}"]], (depth, flag, explicit)
                assert all(np.isnan(v) for v in got.values())


def test_confs_that_still_raise():
    f = golden("eval_depth.npz")
    data = fixture_scene(f)
    pred = {"depths": torch.from_numpy(f["d_pred"])}
    with pytest.raises(ValueError, match="calibrated"):
        evaluation.compute_core_errors(data, pred, DictConf(calibrated=False))
    with pytest.raises(ValueError, match="calibrated"):
        evaluation.prepare_predictions(data, pred, DictConf(calibrated=False), False)
    for fn in (lambda c: evaluation.compute_core_errors(data, pred, c),
               lambda c: evaluation.prepare_predictions(data, pred, c, False)):
        with pytest.raises(NotImplementedError):
            fn(DictConf(depth=False, explicit=True))
    # no flag, no explicit heads, no depth head: nothing to compute, nothing raised
    assert evaluation.compute_core_errors(data, pred, DictConf(depth=False, flag=False)) == {}
    with pytest.raises(ValueError, match="pairing"):
        evaluation.compute_core_errors(data, pred, DictConf(), pairing=f["full_src"][:-1])


# ------------------------------------------------------------------ depth statistics restatement
def test_depth_norm_stats_restatement():
    rng = np.random.default_rng(0)
    dp = torch.from_numpy(rng.uniform(0.5, 9.0, 1000).astype(np.float32))
    dg = torch.from_numpy(rng.uniform(0.5, 4.0, 1000).astype(np.float32))
    scales, st = depth_eval.depth_norm_stats(dp, dg)
    assert scales.dtype == torch.float32 and st.dtype == torch.float64
    assert scales[0].item() == np.float32(dp.double().mean().item()) and scales[1].item() == np.float32(
        dg.double().mean().item())
    a, b = (dp / scales[0]).numpy(), (dg / scales[1]).numpy()
    want = [a.astype(np.float64).sum(), a.min(), a.max(), b.astype(np.float64).sum(), b.min(), b.max(),
            np.abs(a - b).astype(np.float64).sum()]
    np.testing.assert_allclose(st.numpy(), want, rtol=1e-13)
    dp[7] = float("nan")
    _, st = depth_eval.depth_norm_stats(dp, dg)
    assert torch.isnan(st[[0, 1, 2, 6]]).all() and not torch.isnan(st[3:6]).any()
    _, st = depth_eval.depth_norm_stats(dg, None)
    assert torch.isnan(st[3:]).all() and not torch.isnan(st[:3]).any()
    scales, st = depth_eval.depth_norm_stats(dg[:0], None)
    assert torch.isnan(scales).all() and torch.isnan(st).all()


def test_quantiles_follow_numpy():
    rng = np.random.default_rng(1)
    for E in (1, 2, 5, 190, 1001):
        x = rng.standard_normal(E)
        got = evaluation._quantiles(torch.from_numpy(x)).numpy()
        np.testing.assert_allclose(got, np.quantile(x, 0.01 * np.array([10, 25, 50, 75, 90])), rtol=1e-14, atol=1e-15)
    x[3] = np.nan
    assert np.isnan(evaluation._quantiles(torch.from_numpy(x)).numpy()).all()
    assert np.isnan(evaluation._quantiles(torch.zeros(0)).numpy()).all()


# ------------------------------------------------------------------ pairing
def track_graph(lengths=TRACK_LENGTHS, seed=0, identity=False):
    """(pt_ptr [n + 1], perm [E] or None, E): one track per length plus an empty one, the tracks' edges
    scattered over the edge ids by a random permutation."""
    L = np.array(list(lengths[:3]) + [0] + list(lengths[3:]))
    ptr = np.concatenate([[0], np.cumsum(L)]).astype(np.int32)
    E = int(ptr[-1])
    perm = None if identity else np.random.default_rng(seed).permutation(E).astype(np.int32)
    return ptr, perm, E


def check_pairing(ptr, perm, src, bad):
    E = int(ptr[-1])
    edge = np.arange(E) if perm is None else perm
    track_of = np.empty(E, dtype=np.int64)
    track_of[edge] = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    L = np.diff(ptr)[track_of]
    assert int(bad) == int((np.diff(ptr) == 1).sum())
    assert (src[L == 1] == -1).all()
    multi = np.nonzero(L >= 2)[0]
    s = src[multi]
    assert (s >= 0).all() and (s < E).all()
    assert np.array_equal(track_of[s], track_of[multi])  # stays within the track
    assert (s != multi).all()
    assert np.array_equal(np.sort(s), multi)  # a permutation of the edges of the tracks with L >= 2
    for t in np.nonzero(np.diff(ptr) >= 2)[0]:  # one cycle of length L
        members = edge[ptr[t]:ptr[t + 1]]
        e, steps = members[0], 0
        while True:
            e, steps = src[e], steps + 1
            if e == members[0]:
                break
            assert steps <= len(members)
        assert steps == len(members), (t, steps, len(members))


def test_pairing_restatement_properties():
    ptr, perm, E = track_graph()
    assert E % 64 != 0 and E % 256 != 0
    t = torch.from_numpy
    torch.manual_seed(0)
    key = depth_eval.draw_keys(E, torch.device("cpu"))
    assert key.dtype == torch.int32 and key.shape == (E,)
    src, bad = depth_eval.track_cycle(t(ptr), t(perm), key)
    assert src.dtype == torch.int32 and bad.dtype == torch.int32
    check_pairing(ptr, perm, src.numpy(), bad.item())
    src2, _ = depth_eval.track_cycle(t(ptr), t(perm), key)
    assert torch.equal(src, src2)
    torch.manual_seed(1)
    src3, bad3 = depth_eval.track_cycle(t(ptr), t(perm), depth_eval.draw_keys(E, torch.device("cpu")))
    check_pairing(ptr, perm, src3.numpy(), bad3.item())
    assert not torch.equal(src, src3)
    # ties break by edge id: equal keys order a track by its edge ids
    src4, _ = depth_eval.track_cycle(t(ptr), t(perm), torch.zeros(E, dtype=torch.int32))
    members = np.sort(perm[ptr[-2]:ptr[-1]])
    assert np.array_equal(src4.numpy()[members], np.roll(members, 1))
    # perm None: the CSR positions are the edge ids
    ptr_i, _, _ = track_graph(identity=True)
    src5, bad5 = depth_eval.track_cycle(t(ptr_i), None, key)
    check_pairing(ptr_i, None, src5.numpy(), bad5.item())


def test_pairing_is_uniform_over_the_two_3_cycles():
    """4096 tracks of length 3: each of the two cycles is drawn with probability 1/2, so its count is
    binomial(4096, 1/2): sigma = 32, and 6 sigma = 192 is missed about 2e-9 of the time."""
    n = 4096
    ptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int32)
    torch.manual_seed(11)
    src, bad = depth_eval.track_cycle(ptr, None, depth_eval.draw_keys(3 * n, torch.device("cpu")))
    assert bad.item() == 0
    first = src.numpy()[0::3] - np.arange(0, 3 * n, 3)
    assert set(np.unique(first)) == {1, 2}
    count = int((first == 1).sum())
    print("cycle counts", count, n - count)
    assert abs(count - 2048) <= 192


# ------------------------------------------------------------------ header, binding
def test_header_parses_and_library_exports_it():
    with open(DEPTH_EVAL_HEADER) as fh:
        fns, consts, structs = _abi.parse(fh.read())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert fns == {"gasfm_track_cycle": (i32, [vp, vp, vp, i64, i64, vp, vp, vp]),
                   "gasfm_backproj_2view_part_rows": (i32, [i64]),
                   "gasfm_backproj_2view": (i32, 6 * [vp] + [i64, vp, i32] + 4 * [vp]),
                   "gasfm_depth_norm_stats_ws_doubles": (i64, [i64]),
                   "gasfm_depth_norm_stats": (i32, [vp, vp, i64, vp, vp, vp, vp])}
    assert consts == {"GASFM_CAMTAB_FLOATS": 32} and structs == {}
    assert fns == _binding.functions and depth_eval.CAMTAB_FLOATS == 32
    assert len(_abi.functions) == 164 and not any(k in _abi.functions for k in fns)  # gasfm.h is left alone
    if not os.path.exists(LIB):
        return
    L = ctypes.CDLL(LIB)
    for name in fns:
        assert hasattr(L, name), f"{name} is declared but not exported by libgasfm.so"
    B = _binding.lib()
    assert B is _native.lib() and B.gasfm_backproj_2view.argtypes == fns["gasfm_backproj_2view"][1]
    # host-side argument checks and size queries need no device
    assert B.gasfm_backproj_2view_part_rows(0) == 1 and B.gasfm_backproj_2view_part_rows(257) == 2
    assert B.gasfm_backproj_2view_part_rows(10 ** 7) == 1024
    assert B.gasfm_depth_norm_stats_ws_doubles(257) == 9 * 2
    assert B.gasfm_track_cycle(None, None, None, -1, 0, None, None, None) == _native.GASFM_ERR_INVALID
    assert B.gasfm_track_cycle(None, None, None, 5, 3, None, None, None) == _native.GASFM_ERR_INVALID
    assert B.gasfm_backproj_2view(*[None] * 6, 5, None, 2, None, None, None, None) == _native.GASFM_ERR_INVALID
    assert b"gasfm_backproj_2view" in B.gasfm_last_error()
    assert B.gasfm_depth_norm_stats(None, None, 5, None, None, None, None) == _native.GASFM_ERR_INVALID


def test_call_sites_pass_the_declared_number_of_arguments():
    """The AST count of test_abi_cpu.py, over gasfm_amd/depth_eval/ and the new header."""
    bad, seen = [], set()
    for path in sorted(glob.glob(os.path.join(REPO, "gasfm_amd", "depth_eval", "*.py"))):
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr.startswith("gasfm_")):
                continue
            name, where = node.func.attr, f"{os.path.basename(path)}:{node.lineno}"
            assert name in _binding.functions, f"{where}: {name} is not declared in gasfm_depth_eval.h"
            assert not any(isinstance(a, ast.Starred) for a in node.args), f"{where}: starred call"
            seen.add(name)
            want = len(_binding.functions[name][1])
            if len(node.args) != want or node.keywords:
                bad.append(f"{where}: {name} passes {len(node.args)} arguments, the header declares {want}")
    assert not bad, "\n".join(bad)
    assert seen == set(_binding.functions)  # the walk sees every wrapper
