"""The depth-evaluation kernels (csrc/depth_eval.hip) against their torch restatements, and the
depth-head evaluation end to end against the reference's scalars (tests/golden/eval_depth.npz).

Tolerances.  U = 2^-24.

* gasfm_track_cycle: integers; equal to the restatement.
* gasfm_backproj_2view: the error passes through two 3x3 products with a cancellation (camera frame to
  world and back), a division by q_z and a norm; no clean bound comes out of the operation count.
  As the issue prescribes, the float32 torch restatement is measured against its fp64 self on the CPU on
  the same float32 inputs, and the kernel gets 8 x that maximum (operation order and FMA contraction
  differ).  Measured on the CPU: fixture scene 9.7e-5 px (err, on errors of about 25 px), 3.6e-7 (depth, of
  about 4); handmade scene with the long tracks 1.3e-4 px, 4.8e-7.  The tests recompute the maxima and print them.
* gasfm_depth_norm_stats: the sums are accumulated in fp64 from float32 terms, so they are held at
  U x the fp64 sum of the absolute values; min and max are exact; scales are the fp64 means rounded once.
* End to end: the CPU suite's bars (tests/test_depth_eval_cpu.py), plus the 8 x bar above for the kernel
  and 4 U relative on the normalised depths (float32 mean, division and their use).
"""
import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import golden
from gasfm_amd import _native, depth_eval, evaluation, synthetic
from gasfm_amd.depth_eval import _binding
from test_depth_eval_cpu import (TRACK_LENGTHS, DictConf, check_pairing, check_scalars, fixture_scene, ref_depths,
                                 track_graph)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD, SENTINEL = 64, -12345.0


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ------------------------------------------------------------------ pairing
@pytest.mark.parametrize("identity", [False, True])
def test_track_cycle_equals_restatement(device, identity):
    ptr, perm, E = track_graph(identity=identity)
    assert E % 64 != 0 and E % 256 != 0 and set(TRACK_LENGTHS) <= set(np.diff(ptr).tolist())
    torch.manual_seed(5)
    key = depth_eval.draw_keys(E, device)
    assert key.is_cuda and key.dtype == torch.int32
    perm_d = None if perm is None else _t(perm, device)
    src, bad = depth_eval.track_cycle(_t(ptr, device), perm_d, key)
    want, want_bad = depth_eval.track_cycle_torch(torch.from_numpy(ptr), None if perm is None else torch.from_numpy(perm),
                                                  key.cpu())
    assert torch.equal(src.cpu(), want) and bad.item() == want_bad.item() == 1
    check_pairing(ptr, perm, src.cpu().numpy(), bad.item())
    src2, bad2 = depth_eval.track_cycle(_t(ptr, device), perm_d, key)
    assert src.cpu().numpy().tobytes() == src2.cpu().numpy().tobytes() and bad2.item() == 1
    # equal keys: ties break by edge id
    zero = torch.zeros(E, dtype=torch.int32, device=device)
    src3, _ = depth_eval.track_cycle(_t(ptr, device), perm_d, zero)
    assert torch.equal(src3.cpu(), depth_eval.track_cycle_torch(
        torch.from_numpy(ptr), None if perm is None else torch.from_numpy(perm), zero.cpu())[0])


def test_track_cycle_no_edges(device):
    ptr = torch.zeros(4, dtype=torch.int32, device=device)
    src, bad = depth_eval.track_cycle(ptr, None, torch.zeros(0, dtype=torch.int32, device=device))
    assert src.shape == (0,) and bad.item() == 0


# ------------------------------------------------------------------ 2-view error
def _long_track_scene():
    """m = 1000 cameras on a circle, one point per length of TRACK_LENGTHS seen by the first L cameras:
    (cam, pt, xy, d, camtab64 source K and y, pt_ptr, perm), edges cam-major."""
    rng = np.random.default_rng(2)
    m, n = 1000, len(TRACK_LENGTHS)
    ang = np.linspace(0, 2 * np.pi, m, endpoint=False)
    C = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), 0.3 * rng.standard_normal(m)], 1)
    R = np.stack([synthetic.rotation_look_at(c) for c in C])  # camera-to-world, as make_golden_depth.py
    K = np.repeat(synthetic.K_DEFAULT[None], m, 0)
    Rt = np.concatenate([R.transpose(0, 2, 1), -(R.transpose(0, 2, 1) @ C[:, :, None])], 2)
    y = (K @ Rt).astype(np.float32)
    X = rng.uniform(-1, 1, size=(n, 3))
    cam = np.concatenate([np.arange(L) for L in TRACK_LENGTHS])
    pt = np.concatenate([np.full(L, j) for j, L in enumerate(TRACK_LENGTHS)])
    order = np.lexsort((pt, cam))
    cam, pt = cam[order].astype(np.int32), pt[order].astype(np.int32)
    q = np.einsum("eij,ej->ei", Rt[cam], np.concatenate([X[pt], np.ones((len(pt), 1))], 1))
    pix = np.einsum("eij,ej->ei", K[cam], q)
    xy = (pix[:, :2] / pix[:, 2:]).astype(np.float32)
    d = (q[:, 2] * (1 + 0.05 * rng.standard_normal(len(pt))) * 3.7).astype(np.float32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n))]).astype(np.int32)
    perm = np.argsort(pt, kind="stable").astype(np.int32)
    return cam, pt, xy, d, K.astype(np.float32), y, ptr, perm


def _fixture_inputs(f):
    data = fixture_scene(f)
    (cam, pt), _, _, pt_ptr, perm = evaluation._edge_tensors(data)
    xy = evaluation._pixel_measurements(data)
    return (cam.numpy(), pt.numpy(), xy.numpy(), ref_depths(f), f["Ks"], f["y"], pt_ptr.numpy(),
            None if perm is None else perm.numpy())


def _measured_fp32_error(cam, pt, xy, d, scale, src, tab64):
    """max |float32 restatement - fp64 restatement| on the CPU, on the same float32 inputs: (err, depth)."""
    a = depth_eval.backproj_2view_torch(cam, pt, xy, d, scale, src, tab64.float())
    b = depth_eval.backproj_2view_torch(cam, pt, xy, d, scale, src, tab64.float().double())
    ok = ~torch.isnan(b[0])
    return (float((a[0].double() - b[0])[ok].abs().max()), float((a[1].double() - b[1])[ok].abs().max())), b


@pytest.mark.parametrize("scene", ["fixture", "long_tracks"])
def test_backproj_2view_against_fp64_restatement(device, scene):
    cam, pt, xy, d, K, y, ptr, perm = _fixture_inputs(golden("eval_depth.npz")) if scene == "fixture" \
        else _long_track_scene()
    E = cam.shape[0]
    c = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    torch.manual_seed(1)
    src, _ = depth_eval.track_cycle_torch(c(ptr), c(perm), depth_eval.draw_keys(E, torch.device("cpu")))
    src = src.clone()
    d = c(d).clone()
    if scene == "long_tracks":
        assert (src[c(pt) == 0] == -1).all()  # the track of length 1
        d[int(src[700])] = float("nan")  # a NaN depth: NaN at the edge that takes it
        src[900] = E  # out of range: not followed
    scale = torch.tensor(0.27 if scene == "long_tracks" else 1.0)
    tab = depth_eval.camera_table(_t(K, device), _t(y, device))  # m-sized fp64 work on the device
    assert tab.is_cuda and tab.dtype == torch.float32
    host_tab = depth_eval.camera_table(c(K), c(y), torch.float64)
    assert torch.allclose(tab.cpu().double(), host_tab, rtol=2 * U, atol=1e-9)
    tab64 = tab.cpu().double()  # the same float32 table the kernel reads
    (m_err, m_rd), (ref_err, ref_rd, ref_tot) = _measured_fp32_error(c(cam), c(pt), c(xy), d, scale, src, tab64)
    print(f"{scene}: measured fp32 restatement error {m_err:.3e} px, depth {m_rd:.3e}")
    dev = lambda a: a.to(device)  # noqa: E731
    args = (dev(c(cam)), dev(c(pt)), dev(c(xy)), dev(d), dev(scale), dev(src), tab)
    buf = torch.full((2, E + 2 * GUARD), SENTINEL, dtype=torch.float32, device=device)
    err, rd = buf[0, GUARD:GUARD + E], buf[1, GUARD:GUARD + E]
    part = _binding.backproj_2view(*args, err, rd)
    tot = _native.colsum(part).cpu().double()
    b = buf.cpu()
    assert (b[:, :GUARD] == SENTINEL).all() and (b[:, GUARD + E:] == SENTINEL).all()  # guard words untouched
    got_err, got_rd = b[0, GUARD:GUARD + E].double(), b[1, GUARD:GUARD + E].double()
    nan = torch.isnan(ref_err)
    assert torch.equal(torch.isnan(got_err), nan) and torch.equal(torch.isnan(got_rd), nan)
    if scene == "long_tracks":
        assert int(nan.sum()) == 3 and nan[900] and nan[int((src == int(src[700])).nonzero()[0])]
    else:
        assert not nan.any()
    k_err, k_rd = float((got_err - ref_err)[~nan].abs().max()), float((got_rd - ref_rd)[~nan].abs().max())
    print(f"{scene}: kernel error {k_err:.3e} px (bar {8 * m_err:.3e}), depth {k_rd:.3e} (bar {8 * m_rd:.3e})")
    assert k_err <= 8 * m_err and k_rd <= 8 * m_rd
    assert int(tot[1]) == int((~nan).sum()) == int(ref_tot[1])
    # the float32 sum: a thread's few terms, 6 steps across the wave, 4 waves, then the partial rows
    chain = -(-E // (256 * part.shape[0])) + 6 + 4 + part.shape[0]
    assert abs(float(tot[0]) - float(ref_tot[0])) <= int(tot[1]) * 8 * m_err + chain * U * float(ref_tot[0])
    # either optional output NULL: the other one and the partials keep their bits
    only_err, only_rd = torch.empty(E, device=device), torch.empty(E, device=device)
    p1 = _binding.backproj_2view(*args, only_err, None)
    p2 = _binding.backproj_2view(*args, None, only_rd)
    p3 = _binding.backproj_2view(*args, None, None)
    same = lambda x, z: x.cpu().numpy().tobytes() == z.cpu().numpy().tobytes()  # noqa: E731
    assert same(only_err, err) and same(only_rd, rd) and same(p1, part) and same(p2, part) and same(p3, part)
    # pt NULL: the pairing is trusted; here it is a valid one, so nothing changes
    p4 = _binding.backproj_2view(args[0], None, *args[2:], None, None)
    assert same(p4, part)
    # the dispatcher: kernel + colsum
    tot2, err2, rd2 = depth_eval.backproj_2view(*args, per_edge=True)
    assert same(err2, err) and same(rd2, rd) and same(tot2, _native.colsum(part))


def test_backproj_2view_no_edges(device):
    e = torch.empty(0, dtype=torch.int32, device=device)
    z = torch.empty(0, device=device)
    part = _binding.backproj_2view(e, e, torch.empty((0, 2), device=device), z, torch.ones((), device=device), e,
                                   torch.zeros((2, 32), device=device))
    assert part.cpu().tolist() == [[0.0, 0.0]]


# ------------------------------------------------------------------ depth statistics
def test_depth_norm_stats(device):
    rng = np.random.default_rng(4)
    E = 300007  # more than 1024 workgroup rows of 256: the grid-stride loop runs twice for some threads
    dp = torch.from_numpy(rng.uniform(0.5, 40.0, E).astype(np.float32))
    dg = torch.from_numpy(rng.uniform(0.5, 9.0, E).astype(np.float32))
    scales, st = depth_eval.depth_norm_stats(dp.to(device), dg.to(device))
    assert scales.is_cuda and scales.dtype == torch.float32 and st.dtype == torch.float64
    s = scales.cpu()
    assert s[0].item() == np.float32(dp.double().mean().item()) and s[1].item() == np.float32(dg.double().mean().item())
    a, b = (dp / s[0]).double(), (dg / s[1]).double()  # float32 divisions, as the kernel's
    diff = ((dp / s[0]) - (dg / s[1])).abs().double()
    st = st.cpu()
    for i, v in ((0, a), (3, b), (6, diff)):
        assert abs(st[i].item() - v.sum().item()) <= U * v.abs().sum().item(), i
    assert st[1].item() == a.min().item() and st[2].item() == a.max().item()
    assert st[4].item() == b.min().item() and st[5].item() == b.max().item()
    scales2, st2 = depth_eval.depth_norm_stats(dp.to(device), dg.to(device))
    assert scales2.cpu().numpy().tobytes() == s.numpy().tobytes() and st2.cpu().numpy().tobytes() == st.numpy().tobytes()
    # scales alone; targets missing; NaN; nothing
    only, none = depth_eval.depth_norm_stats(dp.to(device), dg.to(device), stats=False)
    assert none is None and torch.equal(only.cpu(), s)
    s3, st3 = depth_eval.depth_norm_stats(dp.to(device), None)
    assert s3[0].item() == s[0].item() and torch.isnan(s3[1]) and torch.isnan(st3[3:]).all()
    assert torch.equal(st3[:3].cpu(), st[:3])
    dp[E // 2] = float("nan")
    s4, st4 = depth_eval.depth_norm_stats(dp.to(device), dg.to(device))
    assert torch.isnan(s4[0]) and not torch.isnan(s4[1])
    assert torch.isnan(st4[[0, 1, 2, 6]]).all() and torch.equal(st4[3:6].cpu(), st[3:6])
    s5, st5 = depth_eval.depth_norm_stats(dp[:0].to(device), dg[:0].to(device))
    assert torch.isnan(s5).all() and torch.isnan(st5).all()


# ------------------------------------------------------------------ end to end
def test_evaluation_matches_reference_on_the_device(device):
    f = golden("eval_depth.npz")
    data = fixture_scene(f, device)
    conf = DictConf()
    # the kernel's bars: 8 x the float32 restatement's own error on this scene (module docstring)
    cam, pt, xy, d, K, y, _, _ = _fixture_inputs(f)
    c = torch.from_numpy
    tab64 = depth_eval.camera_table(c(K), c(y), torch.float64)
    bars = {}
    for tag in ("core", "full"):
        (m_err, m_rd), _ = _measured_fp32_error(c(cam), c(pt), c(xy), c(d), torch.ones(()), c(f[f"{tag}_src"]), tab64)
        bars[tag] = dict(kernel_err=8 * m_err, kernel_rd=8 * m_rd, kernel_rel=4 * U)
    vals = _t(f["d_pred"], device)
    depths = gasfm_amd.scene.SparseMat(vals[:, None], data.x.indices, data.x.cam_per_pts, data.x.pts_per_cam, (6, 60, 1))
    core = evaluation.compute_core_errors(data, {"depths": depths}, conf, pairing=f["core_src"])
    check_scalars(f, core, "core", f["core_src"], **bars["core"])
    # a depth-only model: no Ps_norm / pts3D in the predictions
    outputs = evaluation.prepare_predictions(data, {"depths": depths}, conf, False)
    assert outputs["_device"]["depths_pred"].is_cuda and outputs["_device"]["camtab"].dtype == torch.float32
    full = evaluation.compute_errors(outputs, conf, False, pairing=f["full_src"])
    check_scalars(f, full, "full", f["full_src"], **bars["full"])
    again = evaluation.compute_errors(outputs, conf, False, pairing=f["full_src"])
    assert all(np.array_equal(full[k], again[k]) for k in full)
    # a random pairing: seeded, within the tracks (the kernel refuses nothing: no NaN, all E counted)
    torch.manual_seed(9)
    r1 = evaluation.compute_core_errors(data, {"depths": depths}, conf)
    torch.manual_seed(9)
    r2 = evaluation.compute_core_errors(data, {"depths": depths}, conf)
    assert r1 == r2 and 5 < r1["repro_backproj_rnd_gt_2view"] < 100
    assert outputs["depths_pred_dense"].shape == (6, 60)


def test_captured_pipeline_replays_bitwise(device):
    """scales -> pairing -> 2-view error -> colsum in one torch.cuda.graph; the keys are an input."""
    cam, pt, xy, d, K, y, ptr, perm = _long_track_scene()
    E = cam.shape[0]
    rng = np.random.default_rng(8)
    dg = _t((d / 3.7 * (1 + 0.01 * rng.standard_normal(E))).astype(np.float32), device)
    cam, pt, xy, d, ptr, perm = (_t(a, device) for a in (cam, pt, xy, d, ptr, perm))
    tab = depth_eval.camera_table(_t(K, device), _t(y, device))
    torch.manual_seed(2)
    key = depth_eval.draw_keys(E, device)

    def pipeline():
        scales, _ = depth_eval.depth_norm_stats(d, dg, stats=False)
        src, bad = depth_eval.track_cycle(ptr, perm, key)
        tot, err, rd = depth_eval.backproj_2view(cam, None, xy, d, scales[1] / scales[0], src, tab, per_edge=True)
        return scales, src, bad, tot, err, rd

    eager = [t.clone() for t in pipeline()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipeline()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = pipeline()
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert eager[2].item() == 1 and int(eager[3][1].item()) == E - 1  # the length-1 track is left out
