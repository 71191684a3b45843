"""The depth branch over a union batch (gasfm_amd/depth_batch/, static_batch) on the CPU.

The fp64 torch restatements of the segmented DirectDepthLoss, depth scales and 2-view error, run on a
handmade union, equal the single-scene restatements per scene to 1e-12 (the same formulas on the
same numbers in another grouping: a few fp64 roundings on values of order 1 to 100): the fp64
per-edge loss of tests/test_losses_cpu.py with autograd for the gradients, depth_norm_stats_torch and
backproj_2view_torch.  Pairing over the union restricted to a scene is exactly the scene's own pairing.
StaticBatch.fill_torch puts depths / camtab at the scenes' offsets with the pad defaults, and the new
header, its binding and the library agree.
"""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from conftest import REPO
from gasfm_amd import _abi, _native, depth_batch, depth_eval, evaluation, static_batch, synthetic
from gasfm_amd.build import DEPTH_BATCH_HEADER, LIB
from gasfm_amd.depth_batch import _binding
from gasfm_amd.scene import SceneData

from test_losses_cpu import depth_loss_edges

TOL = 1e-12


# ------------------------------------------------------------------ DirectDepthLoss
def _loss_union(sizes, weights, seed=0):
    """(a, b, eoff, weight) fp64: scenes of ``sizes`` edges; the depths of a weight-0 scene are NaN."""
    g = torch.Generator().manual_seed(seed)
    E = sum(sizes)
    a = 0.5 + 2.0 * torch.rand(E, generator=g, dtype=torch.float64)
    b = 1.0 + 3.0 * torch.rand(E, generator=g, dtype=torch.float64)
    eoff = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    for s, w in enumerate(weights):
        if w == 0:
            a[eoff[s]:eoff[s + 1]] = float("nan")
            b[eoff[s]:eoff[s + 1]] = float("nan")
    return a, b, eoff, torch.tensor(weights, dtype=torch.float64)


@pytest.mark.parametrize("cost_fcn", ["L1", "L2"])
@pytest.mark.parametrize("sizes,weights", [((1, 5, 300, 40), (1.0, 0.5, 1.0, 0.0)), ((7, 0, 33), (1.0, 0.0, 2.0))])
def test_segmented_loss_restatement_equals_the_scenes(cost_fcn, sizes, weights):
    a, b, eoff, weight = _loss_union(sizes, weights)
    l2 = cost_fcn == "L2"
    loss, sums, tot = depth_batch.depth_loss_seg_fwd(a, b, eoff, weight, l2)  # CPU fp64: the restatement
    dloss = torch.tensor(0.75, dtype=torch.float64)
    da = depth_batch.depth_loss_seg_bwd(a, b, eoff, weight, sums, tot, l2, dloss)
    ref, ref_da = 0.0, torch.zeros_like(a)
    for s, w in enumerate(weights):
        e0, e1 = int(eoff[s]), int(eoff[s + 1])
        if w == 0:
            continue
        x = a[e0:e1].clone().requires_grad_(True)
        ls = depth_loss_edges(x, b[e0:e1], cost_fcn)
        (0.75 * w * ls).backward()
        ref = ref + w * float(ls.detach())
        ref_da[e0:e1] = x.grad
        assert abs(float(sums[s, 0]) - float(a[e0:e1].sum())) <= TOL * float(a[e0:e1].sum())
    assert abs(float(loss) - ref) <= TOL * max(1.0, abs(ref))
    assert not torch.isnan(da).any() and not torch.isnan(loss).any()
    assert float((da - ref_da).abs().max()) <= TOL
    for s, w in enumerate(weights):
        if w == 0:
            assert float(da[eoff[s]:eoff[s + 1]].abs().sum()) == 0.0 and float(tot[s].abs().sum()) == 0.0
    if sizes[0] == 1:  # a one-edge scene: u is exactly 0
        assert float(tot[0, 0]) == 0.0 and float(da[0]) == 0.0


def test_weighted_empty_scene_is_nan():
    a, b, eoff, weight = _loss_union((4, 0), (1.0, 1.0))
    loss, _, _ = depth_batch.depth_loss_seg_fwd(a, b, eoff, weight, True)
    assert torch.isnan(loss).all()


# ------------------------------------------------------------------ scenes for the 2-view error and the fill
@pytest.fixture(scope="module")
def scenes():
    out = []
    g = torch.Generator().manual_seed(3)
    for i in range(2):
        sc = synthetic.windowed_scene(12 + 2 * i, 1500, mean_extra=4, seed=50 + i)
        d = SceneData(torch.from_numpy(sc.dense_M()), torch.from_numpy(sc.Ns()), torch.from_numpy(sc.Ps_gt()), f"s{i}")
        d.depths = (1.0 + 3.0 * torch.rand(d.x.indices.shape[1], generator=g, dtype=torch.float64)).float()
        out.append(d)
    return out


def _scene_inputs(d):
    (cam, pt), _, _, pt_ptr, perm = evaluation._edge_tensors(d)
    return cam, pt, evaluation._pixel_measurements(d).double(), pt_ptr, perm, \
        evaluation._camera_table(d, torch.float64, torch.device("cpu"))


def _union(scenes):
    parts = [_scene_inputs(d) for d in scenes]
    Es = [p[0].shape[0] for p in parts]
    ms = [p[5].shape[0] for p in parts]
    ns = [p[3].shape[0] - 1 for p in parts]
    eo, mo, no = (np.concatenate([[0], np.cumsum(v)]) for v in (Es, ms, ns))
    cam = torch.cat([p[0] + int(mo[i]) for i, p in enumerate(parts)])
    pt = torch.cat([p[1] + int(no[i]) for i, p in enumerate(parts)])
    xy = torch.cat([p[2] for p in parts])
    ptr = torch.cat([p[3][:-1] + int(eo[i]) for i, p in enumerate(parts)] + [torch.tensor([int(eo[-1])], dtype=torch.int32)])
    perm = torch.cat([(torch.arange(Es[i], dtype=torch.int32) if p[4] is None else p[4]) + int(eo[i])
                      for i, p in enumerate(parts)])
    tab = torch.cat([p[5] for p in parts])
    return parts, (cam, pt, xy, ptr, perm, tab), torch.tensor(eo, dtype=torch.int32)


def test_union_pairing_scales_and_2view_equal_the_scenes(scenes):
    parts, (cam, pt, xy, ptr, perm, tab), eoff = _union(scenes)
    E = cam.shape[0]
    g = torch.Generator().manual_seed(5)
    dg = torch.cat([d.depths.double() for d in scenes])
    dp = dg * (1 + 0.05 * torch.randn(E, generator=g, dtype=torch.float64)) * 3.7
    dp[int(eoff[1]):] *= 0.4  # the scenes' scale factors differ
    torch.manual_seed(6)
    keys = depth_eval.draw_keys(E, torch.device("cpu"))
    src, bad = depth_eval.track_cycle_torch(ptr, perm, keys)
    scales = depth_batch.depth_scales_seg(dp, dg, eoff)
    tot, err, rdepth = depth_batch.backproj_2view_seg(cam, pt, xy, dp, scales, src, eoff, tab, per_edge=True)
    n_bad = 0
    for s, p in enumerate(parts):
        e0, e1 = int(eoff[s]), int(eoff[s + 1])
        # the pairing identity: ranking is by (key, edge id), union edge ids are the scene's own + e0
        src_s, bad_s = depth_eval.track_cycle_torch(p[3], p[4], keys[e0:e1])
        n_bad += int(bad_s)
        sliced = torch.where(src[e0:e1] >= 0, src[e0:e1] - e0, src[e0:e1])
        assert torch.equal(sliced, src_s)
        sc_s, _ = depth_eval.depth_norm_stats_torch(dp[e0:e1], dg[e0:e1], stats=False)
        assert float((scales[s] - sc_s).abs().max()) <= TOL * float(sc_s.abs().max())
        e_s, r_s, t_s = depth_eval.backproj_2view_torch(p[0], p[1], p[2], dp[e0:e1], sc_s[1] / sc_s[0], src_s, p[5])
        assert int(tot[s, 1]) == int(t_s[1]) > 0
        assert abs(float(tot[s, 0]) - float(t_s[0])) <= TOL * float(t_s[0])
        assert torch.equal(torch.isnan(err[e0:e1]), torch.isnan(e_s))
        ok = ~torch.isnan(e_s)
        assert float((err[e0:e1] - e_s)[ok].abs().max()) <= TOL * float(e_s[ok].max())
        assert float((rdepth[e0:e1] - r_s)[ok].abs().max()) <= TOL * float(r_s[ok].abs().max())
    assert int(bad) == n_bad
    # a source of another scene (another track) or out of range is not followed
    wrong = src.clone()
    wrong[0], wrong[1] = int(eoff[1]), E
    tot2 = depth_batch.backproj_2view_seg(cam, pt, xy, dp, scales, wrong, eoff, tab)
    assert int(tot2[0, 1]) == int(tot[0, 1]) - 2 and int(tot2[1, 1]) == int(tot[1, 1])


# ------------------------------------------------------------------ StaticBatch
def test_fill_torch_places_depths_and_cameras(scenes, monkeypatch):
    monkeypatch.setattr(static_batch, "S2G_PIECES", 64)
    st = static_batch.BatchStats(scenes)
    assert st.expressible() is None
    caps = static_batch.Caps.for_batch(st)
    sb = static_batch.StaticBatch(caps, torch.device("cpu"))
    assert sb.depths is None and sb.camtab is None and sb.pair_keys is None  # other buckets keep their footprint
    sb.fill(scenes, st)
    assert sb.depths is None
    sb.enable_depth()
    assert tuple(sb.depths.shape) == (caps.E,) and tuple(sb.camtab.shape) == (caps.M, depth_eval.CAMTAB_FLOATS)
    assert sb.pair_keys.dtype == torch.int32 and tuple(sb.pair_keys.shape) == (caps.E,)
    torch.manual_seed(1)
    sb.fill(scenes, st)
    mo, no, eo = sb.offsets
    for s, d in enumerate(scenes):
        assert torch.equal(sb.depths[eo[s]:eo[s + 1]], d.depths)
        assert torch.equal(sb.camtab[mo[s]:mo[s + 1]], evaluation._camera_table(d, torch.float32, torch.device("cpu")))
    assert (sb.depths[st.E:] == 1.0).all() and sb.two_view_ready
    pad = sb.camtab[st.M:]
    eye = torch.eye(3)
    assert torch.equal(pad[:, :12].view(-1, 3, 4)[:, :, :3], eye.expand(len(pad), 3, 3))
    assert (pad[:, :12].view(-1, 3, 4)[:, :, 3] == 0).all() and (pad[:, 30:] == 0).all()
    assert torch.equal(pad[:, 12:21].view(-1, 3, 3), eye.expand(len(pad), 3, 3))
    assert torch.equal(pad[:, 21:30].view(-1, 3, 3), eye.expand(len(pad), 3, 3))
    torch.manual_seed(1)
    assert torch.equal(sb.pair_keys, depth_eval.draw_keys(caps.E, torch.device("cpu")))
    keys = sb.pair_keys.clone()
    sb.fill(scenes, st)
    assert not torch.equal(sb.pair_keys, keys)  # every fill draws fresh keys
    # split hands out per-scene depths as SparseMat views
    vals = torch.arange(caps.E, dtype=torch.float32)[:, None]
    parts = sb.split({"depths": static_batch.SparseMat(vals, sb.indices, sb.cam_per_pts, sb.pts_per_cam,
                                                       (caps.M, caps.N, 1))})
    for s, d in enumerate(scenes):
        dep = parts[s]["depths"]
        assert set(parts[s]) == {"depths"} and dep.indices is d.x.indices
        assert torch.equal(dep.values[:, 0], torch.arange(eo[s], eo[s + 1], dtype=torch.float32))
    # the bucket on the CPU runs the restatements: the loss equals the sum of the scenes'
    g = torch.Generator().manual_seed(2)
    a = 0.5 + torch.rand(caps.E, generator=g)
    a[st.E:] = float("nan")
    loss, _, _ = depth_batch.depth_loss_seg_fwd(a, sb.depths, sb.eoff, sb.weight, True)
    ref = sum(float(depth_loss_edges(a[eo[s]:eo[s + 1]].double(), d.depths.double(), "L2")) for s, d in enumerate(scenes))
    assert abs(float(loss) - ref) <= 1e-5 * ref
    # a scene without depths, and one without y, are named
    d0 = scenes[0]
    keep = d0.depths
    try:
        d0.depths = None
        with pytest.raises(ValueError, match="'s0' carries no depths"):
            sb.fill(scenes, st)
    finally:
        d0.depths = keep


def test_trainer_refuses_scenes_without_depths_or_cameras(scenes):
    from gasfm_amd.loss import DirectDepthLoss, ESFMLoss
    trainer = static_batch.StaticTrainer.__new__(static_batch.StaticTrainer)
    trainer.depth, trainer.two_view_error = True, True

    class Scene:
        scene_name = "bare"
        depths = torch.ones(3)
        y = None

    with pytest.raises(ValueError, match="'bare' carries no ground-truth cameras"):
        trainer._check_depth_scenes([scenes[0], Scene()])
    Scene.depths = None
    with pytest.raises(ValueError, match="'bare' carries no depths"):
        trainer._check_depth_scenes([Scene()])
    trainer._check_depth_scenes(scenes)
    assert DirectDepthLoss is not ESFMLoss


# ------------------------------------------------------------------ header, binding
def test_header_parses_and_library_exports_it():
    with open(DEPTH_BATCH_HEADER) as fh:
        fns, consts, structs = _abi.parse(fh.read())
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert fns == {"gasfm_depth_seg_part_rows": (i32, [i32]),
                   "gasfm_depth_loss_seg_sums": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, vp]),
                   "gasfm_depth_loss_seg_fwd": (i32, [vp, vp, vp, i32, i64, vp, vp, i32, vp, vp, vp, vp]),
                   "gasfm_depth_loss_seg_bwd": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, i32, vp, vp, vp]),
                   "gasfm_depth_scales_seg": (i32, [vp, vp, vp, i32, i64, vp, vp, vp]),
                   "gasfm_backproj_2view_seg": (i32, 7 * [vp] + [i32, i64, vp, i32] + 5 * [vp])}
    assert consts == {"GASFM_DEPTH_SEG_G": 32} and structs == {}
    assert fns == _binding.functions and depth_batch.SEG_G == 32
    assert len(_abi.functions) == 164 and not any(k in _abi.functions for k in fns)  # gasfm.h is left alone
    if not os.path.exists(LIB):
        return
    L = ctypes.CDLL(LIB)
    for name in fns:
        assert hasattr(L, name), f"{name} is declared but not exported by libgasfm.so"
    B = _binding.lib()
    assert B is _native.lib() and B.gasfm_backproj_2view_seg.argtypes == fns["gasfm_backproj_2view_seg"][1]
    # host-side argument checks and size queries need no device
    assert B.gasfm_depth_seg_part_rows(3) == 3 * 32
    bad = _native.GASFM_ERR_INVALID
    assert B.gasfm_depth_loss_seg_sums(None, None, None, 0, 5, None, None, None, None) == bad  # S = 0
    assert B.gasfm_depth_loss_seg_sums(None, None, None, 257, 5, None, None, None, None) == bad  # S > 256
    assert B.gasfm_depth_loss_seg_fwd(None, None, None, 2, 5, None, None, 1, None, None, None, None) == bad
    assert b"gasfm_depth_loss_seg_fwd" in B.gasfm_last_error()
    assert B.gasfm_depth_loss_seg_bwd(None, None, None, 2, -1, None, None, None, 1, None, None, None) == bad
    assert B.gasfm_depth_scales_seg(None, None, None, 2, 5, None, None, None) == bad
    assert B.gasfm_backproj_2view_seg(*[None] * 7, 2, 5, None, 2, None, None, None, None, None) == bad


def test_call_sites_pass_the_declared_number_of_arguments():
    """The AST count of test_abi_cpu.py, over gasfm_amd/depth_batch/ and the new header."""
    bad, seen = [], set()
    for path in sorted(glob.glob(os.path.join(REPO, "gasfm_amd", "depth_batch", "*.py"))):
        with open(path) as fh:
            tree = ast.parse(fh.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr.startswith("gasfm_")):
                continue
            name, where = node.func.attr, f"{os.path.basename(path)}:{node.lineno}"
            assert name in _binding.functions, f"{where}: {name} is not declared in gasfm_depth_batch.h"
            assert not any(isinstance(a, ast.Starred) for a in node.args), f"{where}: starred call"
            seen.add(name)
            want = len(_binding.functions[name][1])
            if len(node.args) != want or node.keywords:
                bad.append(f"{where}: {name} passes {len(node.args)} arguments, the header declares {want}")
    assert not bad, "\n".join(bad)
    assert seen == set(_binding.functions)  # the walk sees every wrapper
