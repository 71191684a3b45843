"""Per-edge depth targets without a GPU: the torch restatements of the three kernels of
csrc/depth_targets.hip (scene_device.depth_targets_torch / depth_gather_torch / depth_rescale_torch,
the path CPU tensors take) against the reference's dense depths (tests/golden/depth_targets.npz,
make_golden_depth.py), the new C signatures, and the error contracts.  The helpers here (the fixture
views, the fp64 evaluations and the bounds) are shared with tests/test_gpu_depth_targets.py.

Bounds, u = 2^-24, derived and not measured:

targets   d = a . X, a 4-term dot product in fp32, in any order, fused or not: against the fp64 value
          of the same float32 inputs |dd| <= 4u S, S = sum_i |a_i| |X_i| (n u holds for an n-term dot
          product without higher-order terms); against the fixture 6u S, since the reference rounds
          its own dot product and its X may sit on neighbouring floats.
rescale   d' = d / z_old * z_new, h = (u_px, v_px, 1), q_i = N_i . h, z_old = q_2, z_new = r . q
          (r = the third row of R).  With g3 = 3u / (1 - 3u) and S_i = |N_i0||u_px| + |N_i1||v_px| + |N_i2|:
            |dq_i| <= g3 S_i                                      (a 3-term dot product)
            |dz_new| <= g3 sum_i |r_i||q^_i| + sum_i |r_i||dq_i|   (a 3-term dot product of rounded q^)
                     <= g3 (2 + g3) sum_i |r_i| S_i =: B_new
          and the division and the multiplication each add a factor (1 + e), |e| <= u.  With
          rho_old = g3 S_2 / |z_old| and rho_new = B_new / |z_new| the computed value lies within
            |dd'| <= |d'| ((1 + rho_new) (1 + u)^2 / (1 - rho_old) - 1)
          of the fp64 value of the same inputs.  Twice that against the fixture: both sides round.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO, golden
from gasfm_amd import _native, scene_device as sd

U = 2.0 ** -24
NEW_SYMBOLS = ("gasfm_depth_part_slots", "gasfm_depth_targets", "gasfm_depth_gather", "gasfm_depth_rescale")


# ------------------------------------------------------------------ shared helpers
def fixture():
    f = golden("depth_targets.npz")
    return {k: torch.from_numpy(f[k]) for k in f.files}


def edges_of(M):
    """(cam, pt) int64 of a dense M in the scene's camera-major order (get_M_valid_points)."""
    from gasfm_amd.scene import get_M_valid_points
    cam, pt = torch.nonzero(get_M_valid_points(M), as_tuple=True)
    return cam, pt


def cam_ptr_of(cam, m):
    ptr = torch.zeros(m + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(cam, minlength=m), 0)
    return ptr


def sample_case(f, views):
    """SceneData.sample_data of the fixture's scene for the given (ascending) views, dense: (view_idx,
    keep, sampled M, cam', pt', the dense depths read at the sampled edges)."""
    views = torch.as_tensor(views, dtype=torch.int64)
    rows = torch.stack([2 * views, 2 * views + 1], 1).view(-1)
    Ms = f["M"][rows]
    from gasfm_amd.scene import get_M_valid_points
    keep = torch.nonzero(get_M_valid_points(Ms).any(0)).view(-1)
    Ms = Ms[:, keep].contiguous()
    cam, pt = edges_of(Ms)
    return views, keep, Ms, cam, pt, f["depths"][views][:, keep][cam, pt]


def parent_arrays(f):
    """(cam_ptr, pt, per-edge depths) of the fixture's full scene."""
    cam, pt = f["indices"][0], f["indices"][1]
    return cam_ptr_of(cam, f["M"].shape[0] // 2), pt.contiguous(), f["depths"][cam, pt].contiguous()


def targets_fp64(a, X, cam, pt):
    """(fp64 a . X per edge, S = sum |a_i||X_i|)."""
    p = a[cam].double() * X[pt].double()
    return p.sum(1), p.abs().sum(1)


def rescale_fp64(d, cam, pt, M, Ns, R):
    """(fp64 d / z_old * z_new of the float32 inputs, the bound of the module docstring, z_new / z_old)."""
    g3 = 3 * U / (1 - 3 * U)
    h = torch.stack([M[2 * cam, pt], M[2 * cam + 1, pt], torch.ones(cam.shape[0])], 1).double()
    N, r = Ns[cam].double(), R[cam].double()[:, 2, :]
    q = (N * h[:, None, :]).sum(2)
    S = (N.abs() * h.abs()[:, None, :]).sum(2)
    z_old, z_new = q[:, 2], (r * q).sum(1)
    exact = d.double() / z_old * z_new
    rho_old = g3 * S[:, 2] / z_old.abs()
    rho_new = g3 * (2 + g3) * (r.abs() * S).sum(1) / z_new.abs()
    return exact, exact.abs() * ((1 + rho_new) * (1 + U) ** 2 / (1 - rho_old) - 1), z_new / z_old


def assert_within(got, ref, bound, what):
    err = (got.double().cpu() - ref.double()).abs()
    worst = (err / bound).max().item() if err.numel() else 0.0
    print(f"{what}: max |err| {err.max().item() if err.numel() else 0.0:.3e}, max err / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: err / bound up to {worst:.3f}"


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gasfm.h")).read(), flags=re.S)


# ------------------------------------------------------------------ restatements against the fixture
VIEW_CASES = {
    "fixture sample, camera 5's row empty": [2, 3, 4, 5],
    "parent row of length 1 (camera 5), non-adjacent": [0, 2, 5],
    "points 50-53 dropped (camera 4 missing)": [0, 1, 2, 3],
    "non-adjacent pair": [1, 4],
    "all views": [0, 1, 2, 3, 4, 5],
}


def test_fixture_scene_has_the_cases_the_gather_tests_need():
    f = fixture()
    cam = f["indices"][0]
    assert int((cam == 5).sum()) == 1  # a parent row of length 1
    v, keep, Ms, c, p, _ = sample_case(f, [2, 3, 4, 5])
    assert torch.equal(Ms, f["s_M"]) and torch.equal(torch.stack([c, p]), f["s_indices"])
    assert int((c == 3).sum()) == 0  # camera 5 sampled, all of its points dropped
    assert 54 not in keep.tolist() and f["M"].shape[1] - keep.shape[0] > 2
    v, keep, _, c, p, _ = sample_case(f, [0, 2, 5])
    assert int((c == 2).sum()) == 1 and 54 in keep.tolist()
    assert not set(range(50, 54)) & set(sample_case(f, [0, 1, 2, 3])[1].tolist())
    e = f["depths"][f["indices"][0], f["indices"][1]]
    assert bool(torch.isfinite(e).all()) and bool((e > 0).all())  # the reference's asserts


@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_gather_restatement_equals_dense_indexing(name):
    f = fixture()
    views, keep, _, cam, pt, want = sample_case(f, VIEW_CASES[name])
    d, missing = sd.depth_gather_torch(*parent_arrays(f), views, keep, cam, pt)
    assert int(missing) == 0 and torch.equal(d, want)
    if name.startswith("fixture"):
        assert torch.equal(d, f["s_depths"][cam, pt])
    # every hit position: the first and the last element of a parent row are among them
    pcam_ptr, ppt, _ = parent_arrays(f)
    first = {int(ppt[pcam_ptr[c]]) for c in views.tolist()}
    last = {int(ppt[pcam_ptr[c + 1] - 1]) for c in views.tolist()}
    hit = set(keep[pt].tolist())
    assert name != "all views" or (first <= hit and last <= hit)


def test_gather_restatement_counts_edges_without_a_parent():
    f = fixture()
    views, keep, _, cam, pt, _ = sample_case(f, [2, 3, 4, 5])
    keep = keep.clone()
    keep[pt[0]] = 59  # no camera sees point 59
    d, missing = sd.depth_gather_torch(*parent_arrays(f), views, keep, cam, pt)
    assert int(missing) == int((pt == pt[0]).sum()) and bool(torch.isnan(d[pt == pt[0]]).all())
    d, missing = sd.depth_gather_torch(*parent_arrays(f), views, keep, cam[:0], pt[:0])
    assert d.shape == (0,) and int(missing) == 0


def test_targets_restatement_within_bounds():
    f = fixture()
    a = sd.depth_rows(f["Ns"], f["Ps_gt"])
    X = f["X"].t().contiguous()
    cam, pt = f["indices"][0], f["indices"][1]
    assert bool((X[pt.unique(), 3] == 1).all()) and bool(torch.isnan(X[58:]).all())
    d, bad = sd.depth_targets_torch(a, X, cam, pt)
    exact, S = targets_fp64(a, X, cam, pt)
    assert int(bad) == 0
    assert_within(d, exact, 4 * U * S, "targets restatement vs fp64")
    assert_within(d, f["depths"][cam, pt], 6 * U * S, "targets restatement vs the reference")
    assert torch.equal(sd.depth_targets_from_points(a, X, cam, pt), d)


def test_rescale_restatement_within_bounds():
    f = fixture()
    cam, pt = f["s_indices"][0], f["s_indices"][1]
    assert torch.equal(f["a_indices"], f["s_indices"])
    d = f["s_depths"][cam, pt]
    Ns = f["Ns"][f["s_views"]]
    got = sd.depth_rescale_torch(d, cam, pt, f["s_M"], Ns, f["R_aug"])
    exact, bound, _ = rescale_fp64(d, cam, pt, f["s_M"], Ns, f["R_aug"])
    assert_within(got, exact, bound, "rescale restatement vs fp64")
    assert_within(got, f["a_depths"][cam, pt], 2 * bound, "rescale restatement vs the reference")


# ------------------------------------------------------------------ C ABI
def test_new_signatures_match_the_header():
    scalars = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    text = header_text()
    for name in NEW_SYMBOLS:
        m = re.search(r"([\w \t\*]+?)\b" + name + r"\s*\(([^;{]*?)\)\s*;", text)
        assert m, f"{name} is not declared in include/gasfm.h"
        restype, argtypes = _native._SIGS[name]
        assert scalars[m.group(1).split()[-1]] is restype
        params = [p.strip() for p in m.group(2).split(",")]
        want = [ctypes.c_void_p if "*" in p else scalars[[w for w in p.split() if w != "const"][0]] for p in params]
        assert want == argtypes, name
        assert hasattr(_native.lib(), name)


def test_empty_edge_list_returns_before_any_pointer():
    """E = 0 is GASFM_OK with null pointers (no HIP call: this needs no device); a negative size is
    the invalid-argument status."""
    L = _native.lib()
    assert L.gasfm_depth_part_slots(0) == 0
    assert L.gasfm_depth_targets(None, 3, None, 5, None, None, 1, 0, None, None, None, None) == _native.GASFM_OK
    assert L.gasfm_depth_gather(None, None, 1, None, 3, 0, None, None, 2, 4, None, None, 1, 0, None, None, None,
                                None) == _native.GASFM_OK
    assert L.gasfm_depth_rescale(None, None, None, 1, 0, None, 5, 3, 5, None, None, None, None) == _native.GASFM_OK
    assert L.gasfm_depth_targets(None, -1, None, 5, None, None, 1, 0, None, None, None, None) \
        == _native.GASFM_ERR_INVALID
    assert b"gasfm_depth_targets" in L.gasfm_last_error()
    slots = [L.gasfm_depth_part_slots(E) for E in (1, 256, 257, 1 << 40)]
    assert slots[0] == slots[1] == 4 and slots[2] == 8 and slots[3] % 4 == 0


# ------------------------------------------------------------------ error contracts
def test_uncalibrated_scene_is_not_implemented():
    f = fixture()
    b = {"cam": f["indices"][0], "pt": f["indices"][1]}
    with pytest.raises(NotImplementedError, match="uncalibrated"):
        sd._scene_depths(f["M"], f["Ns"], f["Ps_gt"], b, False, "s", None)
    with pytest.raises(ValueError, match="Ps_gt"):
        sd._scene_depths(f["M"], f["Ns"], None, b, True, "s", None)


def test_point_behind_a_camera_is_a_value_error():
    f = fixture()
    a = sd.depth_rows(f["Ns"], f["Ps_gt"])
    X = f["X"].t().contiguous()
    cam, pt = f["indices"][0], f["indices"][1]
    X[7, :3] = 2 * X[7, :3] + 9 * torch.tensor([1.0, 0.0, 0.0])  # beyond camera 0, which looks back along x
    n_bad = int(sd.depth_targets_torch(a, X, cam, pt)[1])
    assert n_bad >= 1
    with pytest.raises(ValueError, match=f"{n_bad} of {cam.shape[0]} depth targets"):
        sd.depth_targets_from_points(a, X, cam, pt, "s")
    X[7] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        sd.depth_targets_from_points(a, X, cam, pt, "s")


def test_adopted_depths_shapes():
    f = fixture()
    cam, pt = f["indices"][0], f["indices"][1]
    b = {"cam": cam, "pt": pt}
    e = f["depths"][cam, pt]
    assert torch.equal(sd._scene_depths(f["M"], f["Ns"], None, b, True, "s", e), e)
    assert torch.equal(sd._scene_depths(f["M"], f["Ns"], None, b, True, "s", f["depths"]), e)
    with pytest.raises(ValueError, match="edges"):
        sd._scene_depths(f["M"], f["Ns"], None, b, True, "s", e[:-1])
    with pytest.raises(ValueError, match=r"\[m, n\]"):
        sd._scene_depths(f["M"], f["Ns"], None, b, True, "s", f["depths"][:, :-1])


def _scene(cam, pt, m, n, **kw):
    x = types.SimpleNamespace(indices=torch.stack([cam, pt]), shape=(m, n, 2),
                              pts_per_cam=torch.bincount(cam, minlength=m).unsqueeze(1))
    return types.SimpleNamespace(x=x, scene_name="s", **kw)


def test_carry_depths_contracts():
    """sample_data_device / apply_rotational_homography_aug_device hand the targets on through
    _carry_depths: gathered (a host scene's dense depths once), the edge count checked, rescaled."""
    f = fixture()
    views, keep, Ms, cam, pt, want = sample_case(f, [2, 3, 4, 5])
    parent = _scene(f["indices"][0], f["indices"][1], 6, 60, store_depth_targets=True, depths=f["depths"])
    arrays = sd._per_edge_depths(parent, torch.device("cpu"))
    assert torch.equal(arrays[2], parent_arrays(f)[2]) and torch.equal(arrays[0], parent_arrays(f)[0])
    assert sd._per_edge_depths(parent, torch.device("cpu")) is arrays  # once per scene
    E = torch.tensor(cam.shape[0])
    src = sd._DepthSource(*arrays, views, keep, E)
    out = sd._carry_depths(_scene(cam, pt, 4, keep.shape[0]), parent, src, None, None, None)
    assert out.store_depth_targets and torch.equal(out.depths, want)
    Ns = f["Ns"][views]
    out = sd._carry_depths(_scene(cam, pt, 4, keep.shape[0]), parent, src, Ms, Ns, f["R_aug"])
    assert torch.equal(out.depths, sd.depth_rescale_torch(want, cam, pt, Ms, Ns, f["R_aug"]))
    # a built scene with per-edge targets entering the augmentation: taken as they are
    built = _scene(cam, pt, 4, keep.shape[0], store_depth_targets=True, depths=want)
    assert torch.equal(sd._carry_depths(_scene(cam, pt, 4, keep.shape[0]), built, None, None, None, None).depths, want)
    with pytest.raises(ValueError, match="changed the observed entries"):
        sd._carry_depths(_scene(cam[1:], pt[1:], 4, keep.shape[0]), built, None, None, None, None)
    with pytest.raises(ValueError, match="changed the observed entries"):
        sd._carry_depths(_scene(cam[1:], pt[1:], 4, keep.shape[0]), parent, src, None, None, None)
    bad_keep = keep.clone()
    bad_keep[pt[0]] = 59
    with pytest.raises(ValueError, match="no edge in the parent"):
        sd._carry_depths(_scene(cam, pt, 4, keep.shape[0]), parent,
                         sd._DepthSource(*arrays, views, bad_keep, E), None, None, None)
    # without the flag nothing is attached
    plain = _scene(cam, pt, 4, keep.shape[0])
    assert sd._carry_depths(plain, _scene(cam, pt, 4, keep.shape[0]), None, None, None, None) is plain
    assert not hasattr(plain, "depths")
