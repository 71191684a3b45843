"""A batch of scenes through SetOfSetNet as one union-graph forward on the MI355X: the ordered
per-range column sums (csrc/colsum_ranges.hip), the fused per-scene layer against the fp64 composite
run scene by scene, and ``forward_batch`` against the per-scene loop."""
import numpy as np
import pytest
import torch

import gasfm_amd
from conftest import check_grad
from gasfm_amd import _native, setofset
from gasfm_amd.batch import SceneBatch, forward_batch
from gasfm_amd.conf import dpesfm_conf
from gasfm_amd.graph_step import CapturedStep
from gasfm_amd.loss import ESFMLoss
from oracle.weights import deterministic_state_dict
from test_gpu_batch import _scenes
from test_gpu_setofset import OUT_ATOL, OUT_RTOL, SCENE_EDGES, hand_scene, layer_pair

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ colsum_ranges
ISSUE_PTR = [0, 0, 1, 2, 19, 19, 4115]   # empty first, single row, empty middle, long last range
BLOCK = 256                              # threads of a workgroup
UNROLL = 8                               # rows a row lane keeps in flight


def row_lanes(cols):
    """Row lanes of the kernel's 256 threads for a (<= 32-column chunk of a) cols-wide matrix read
    contiguously: float4 column groups when cols % 4 == 0, else one column per thread."""
    c = min(cols, 32)
    return BLOCK // (c // 4 if cols % 4 == 0 else c)


def split_ptr(cols):
    """Ranges one shorter than, equal to and one longer than a workgroup's batch of UNROLL * lanes rows
    (where the unrolled loop hands over to the row-by-row tail), and the same around one row per lane."""
    rl = row_lanes(cols)
    lens = [UNROLL * rl - 1, UNROLL * rl, UNROLL * rl + 1, rl - 1, rl, rl + 1]
    return [sum(lens[:i]) for i in range(len(lens) + 1)]


def layouts(rows, cols, device):
    """(name, A) with A [rows, cols] fp32: contiguous, row stride cols + 4 and cols + 1, base offset
    by one float (not 16-byte aligned)."""
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + cols)
    base = torch.randn(rows, cols, generator=g).to(device)
    out = [("contiguous", base)]
    for pad in (4, 1):
        buf = torch.full((rows, cols + pad), float("nan"), device=device)
        buf[:, :cols] = base
        out.append((f"ld=cols+{pad}", buf[:, :cols]))
    flat = torch.full((rows * cols + 1,), float("nan"), device=device)
    flat[1:] = base.reshape(-1)
    out.append(("unaligned", flat[1:].view(rows, cols)))
    assert out[3][1].data_ptr() % 16 == 4 and out[1][1].stride(0) == cols + 4
    return out


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("ranges", ["issue", "split"])
@pytest.mark.parametrize("cols", [1, 2, 3, 32, 256])
def test_colsum_ranges_matches_an_fp64_loop(device, cols, ranges, weighted):
    ptr = ISSUE_PTR if ranges == "issue" else split_ptr(cols)
    rows, n, G = ptr[-1], len(ptr) - 1, 2
    row_ptr = torch.tensor(ptr, dtype=torch.int32, device=device)
    w = None
    if weighted:
        w = torch.randn(rows, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(device)
    for name, A in layouts(rows, cols, device):
        WA = A.double() if w is None else A.double() * w[:, None]
        ref = torch.stack([WA[a:b].sum(0) for a, b in zip(ptr[:-1], ptr[1:])])
        mag = torch.stack([WA[a:b].abs().sum(0) for a, b in zip(ptr[:-1], ptr[1:])])
        buf = torch.full((n + 2 * G, cols), -7.5, dtype=torch.float64, device=device)   # sentinel rows around out
        got = _native.colsum_ranges(A, row_ptr, w, out=buf[G:G + n])
        err, bound = (got - ref).abs(), 1e-12 * mag
        print(f"cols={cols} {ranges} {name}: max err {float(err.max()):.3e}, bound there "
              f"{float(bound.flatten()[err.argmax()]):.3e}")
        assert bool((err <= bound).all()), (name, float((err - bound).max()))
        assert bool((buf[:G] == -7.5).all()) and bool((buf[G + n:] == -7.5).all()), name
        for s, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
            if a == b:
                assert not got[s].any(), (name, s)
        again = _native.colsum_ranges(A, row_ptr, w)
        assert torch.equal(again, got), name


def test_colsum_ranges_rejects_bad_arguments(device):
    A = torch.zeros(4, 8, device=device)
    ptr = torch.tensor([0, 4], dtype=torch.int32, device=device)
    with pytest.raises(ValueError):
        _native.colsum_ranges(A, ptr.long())
    with pytest.raises(ValueError):
        _native.colsum_ranges(A, ptr, w=torch.zeros(4, device=device))
    with pytest.raises(ValueError):
        _native.colsum_ranges(A.double(), ptr)
    with pytest.raises(ValueError):
        _native.colsum_ranges(A, ptr, out=torch.zeros(2, 8, dtype=torch.float64, device=device))
    none = _native.colsum_ranges(A, ptr[:1])
    assert tuple(none.shape) == (0, 8)


# ------------------------------------------------------------------ one layer on a union
_UNION = {}


def hand_union(device):
    """Three hand_scene patterns with different seeds and, second, a scene without edges: the scenes on
    the device, their union and its EdgeIndex (built once)."""
    if not _UNION:
        empty = gasfm_amd.SceneData.from_sparse(np.zeros(0, np.int64), np.zeros(0, np.int64),
                                                np.zeros((0, 2), np.float32), 3, 5, max_piece=4)
        datas = [hand_scene(SCENE_EDGES[0], seed=0), empty, hand_scene(SCENE_EDGES[1], seed=1),
                 hand_scene(SCENE_EDGES[0], seed=2)]
        datas = [d.to(device) for d in datas]
        batch = SceneBatch(datas, max_piece=4)
        _UNION["datas"], _UNION["batch"] = datas, batch
        _UNION["edges"] = setofset.scene_edge_index(batch, device)
        _UNION["scene_edges"] = [setofset.scene_edge_index(d, device) for d in datas]
    return _UNION


def test_hand_union_has_the_edge_cases(device):
    u = hand_union(device)
    e, b = u["edges"], u["batch"]
    assert b.edge_off == [0, 1025, 1025, 2048, 3073] and b.cam_off == [0, 7, 10, 17, 24]
    pp, pc = e.plans["proj2scenepoint"], e.plans["proj2view"]
    assert pp.n_combine > 0 and pc.n_combine > 0 and pp.perm is not None and pc.perm is None
    assert setofset._union(e).B == 4 and setofset.fusable(torch.zeros(3073, 32, device=device), 32, 32, e)


def union_run(layer, X, edges, center, relu, R, C):
    """The fused layer on the whole union."""
    for p in layer.parameters():
        p.grad = None
    X = X.clone().requires_grad_(True)
    R = None if R is None else R.clone().requires_grad_(True)
    Y = layer(X, edges, center=center, relu=relu, residual=R, composite=False)
    (Y * C).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in layer.named_parameters()}
    grads["X"] = X.grad
    if R is not None:
        grads["R"] = R.grad
    return Y.detach(), grads


def loop_run(layer, X, scene_edges, off, center, relu, R, C):
    """The composite layer scene by scene on each scene's own edges; one backward of the summed loss."""
    for p in layer.parameters():
        p.grad = None
    X = X.clone().requires_grad_(True)
    R = None if R is None else R.clone().requires_grad_(True)
    Y = torch.cat([layer(X[a:b], e, center=center, relu=relu, residual=None if R is None else R[a:b], composite=True)
                   for e, a, b in zip(scene_edges, off[:-1], off[1:])])
    (Y * C).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in layer.named_parameters()}
    grads["X"] = X.grad
    if R is not None:
        grads["R"] = R.grad
    return Y.detach(), grads


@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("act", [False, True], ids=["plain", "center_relu"])
@pytest.mark.parametrize("d_in,d_out", [(2, 256), (256, 256), (256, 128), (32, 32)])
def test_union_layer_matches_fp64_per_scene(device, d_in, d_out, act, skip):
    u = hand_union(device)
    edges, off = u["edges"], u["batch"].edge_off
    E = off[-1]
    layer, _ = layer_pair(d_in, d_out, device, seed=d_in + d_out)
    torch.manual_seed(1)
    X = torch.randn(E, d_in, device=device)
    R = torch.randn(E, d_out, device=device) if skip else None
    C = torch.randn(E, d_out, device=device)
    with _native.dispatch_record() as rec:
        Y, g = union_run(layer, X, edges, act, act, R, C)
    assert rec.counts["sos_edge_fwd"] == 1 and rec.counts["sos_edge_dx"] == 1 and rec.counts["sos_edge_dw"] == 1
    Y32, g32 = loop_run(layer, X, u["scene_edges"], off, act, act, R, C)
    l64 = layer.double()
    Y64, g64 = loop_run(l64, X.double(), u["scene_edges"], off, act, act, None if R is None else R.double(), C.double())
    layer.float()
    torch.testing.assert_close(Y.double(), Y64, atol=OUT_ATOL, rtol=OUT_RTOL)
    for k in g64:
        check_grad(g[k], g64[k].cpu().numpy(), f"{d_in}->{d_out} {k}", ref32=g32[k].double().cpu().numpy())


def test_skip_projection_centring_is_per_scene(device):
    """The skip ProjLayer's centring of a block with a width change, on the fused path of a union,
    against the composite block scene by scene (fp64)."""
    u = hand_union(device)
    edges, off = u["edges"], u["batch"].edge_off
    conf = dpesfm_conf(num_features=32, add_skipconn_for_residual_blocks=True)
    torch.manual_seed(4)
    blk = setofset.SetOfSetBlock(2, 32, conf).to(device)
    X = torch.randn(off[-1], 2, device=device)
    C = torch.randn(off[-1], 32, device=device)

    def run(b, x, c, union):
        for p in b.parameters():
            p.grad = None
        if union:
            Y = b(x, edges, composite=False)
        else:
            Y = torch.cat([b(x[a0:a1], e, composite=True) for e, a0, a1 in zip(u["scene_edges"], off[:-1], off[1:])])
        (Y * c).sum().backward()
        return Y.detach(), {k: p.grad.detach().clone() for k, p in b.named_parameters()}

    Y, g = run(blk, X, C, True)
    Y32, g32 = run(blk, X, C, False)
    Y64, g64 = run(blk.double(), X.double(), C.double(), False)
    torch.testing.assert_close(Y.double(), Y64, atol=OUT_ATOL, rtol=OUT_RTOL)
    for k in g64:
        check_grad(g[k], g64[k].cpu().numpy(), k, ref32=g32[k].double().cpu().numpy())


# ------------------------------------------------------------------ the model on sampled scenes
CONFS = {
    "shipped": dict(),
    "depth": dict(num_features=32, depth_head={"enabled": True, "n_feat": 32, "n_hidden_layers": 2}),
}
_CASES = {}
_DATAS = []


def sampled_scenes(device):
    if not _DATAS:
        _DATAS.extend(_scenes(device))
    return _DATAS


def loss_conf(name):
    conf = dpesfm_conf(**CONFS[name])
    conf.put("loss", {"infinity_pts_margin": 1e-4, "pts_grad_equalization_pre_perspective_divide": True,
                      "normalize_grad_wrt_valid_projections_only": True, "hinge_loss": True,
                      "hinge_loss_weight": 1.0})
    return conf


def model_case(device, name):
    """forward + summed ESFMLoss (+ a linear term on the depths) + one backward, five ways, computed
    once: the union twice, the fused per-scene loop, the fp32 and fp64 composite per-scene loops.  The
    loss kernels are fp32: the fp64 run hands them its predictions rounded to fp32."""
    if name in _CASES:
        return _CASES[name]
    datas = sampled_scenes(device)
    conf = loss_conf(name)
    net = gasfm_amd.SetOfSetNet(conf)
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.to(device)
    lossf = ESFMLoss(conf)
    gen = torch.Generator().manual_seed(11)
    cD = [torch.randn(d.x.values.shape[0], 1, generator=gen).to(device) for d in datas]
    vals32 = [d.x.values for d in datas]

    def run(dtype, composite, union):
        net.to(dtype)
        net.composite = composite
        for d, v in zip(datas, vals32):
            d.x.values = v.to(dtype)
        for p in net.parameters():
            p.grad = None
        preds = forward_batch(net, datas) if union else [net(d) for d in datas]
        loss = 0
        for p, d, c in zip(preds, datas, cD):
            loss = loss + lossf({k: p[k].float() for k in ("Ps_norm", "pts3D")}, d)
            if "depths" in p:
                loss = loss + (p["depths"].values * c.to(dtype)).sum()
        loss.backward()
        outs = [{k: (v.values if k == "depths" else v).detach().clone() for k, v in p.items()} for p in preds]
        return outs, {k: p.grad.detach().clone() for k, p in net.named_parameters()}, float(loss.detach())

    case = {"c64": run(torch.float64, True, False), "c32": run(torch.float32, True, False),
            "loop": run(torch.float32, False, False)}
    with _native.dispatch_record() as rec:
        case["u1"] = run(torch.float32, False, True)
    case["u2"] = run(torch.float32, False, True)
    case["fused_layers"] = rec.counts["sos_edge_fwd"]
    net.composite = False
    case["net"], case["datas"] = net, datas
    _CASES[name] = case
    return case


@pytest.mark.parametrize("name", list(CONFS))
def test_forward_batch_matches_the_per_scene_loop(device, name):
    case = model_case(device, name)
    (o, g, loss), (o_loop, _, loss_loop) = case["u1"], case["loop"]
    assert case["fused_layers"] == 3                      # one edge kernel per layer for the whole batch
    assert len(o) == len(o_loop) == 3
    for i, (a, b) in enumerate(zip(o, o_loop)):
        assert set(a) == set(b) and ("depths" in a) == (name == "depth")
        for k in b:
            assert a[k].shape == b[k].shape
            np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-4, atol=1e-5,
                                       err_msg=f"{name} scene {i} {k}")
    np.testing.assert_allclose(loss, loss_loop, rtol=1e-4)
    (_, g64, _), (_, g32, _) = case["c64"], case["c32"]
    for k in g64:
        check_grad(g[k], g64[k].cpu().numpy(), f"{name} {k}", ref32=g32[k].double().cpu().numpy())


def test_split_depths_carry_each_scenes_indices(device):
    case = model_case(device, "depth")
    net, datas = case["net"], case["datas"]
    with torch.no_grad():
        preds = forward_batch(net, datas)
    for p, d in zip(preds, datas):
        dep = p["depths"]
        assert dep.values.shape == (d.x.values.shape[0], 1) and torch.equal(dep.indices, d.x.indices)
        assert list(dep.shape) == [d.x.shape[0], d.x.shape[1], 1]


def test_two_union_runs_are_bitwise_equal(device):
    case = model_case(device, "shipped")
    (o1, g1, _), (o2, g2, _) = case["u1"], case["u2"]
    assert all(torch.equal(a[k], b[k]) for a, b in zip(o1, o2) for k in a)
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])]


def test_net_on_a_scene_batch_is_forward_batch(device):
    case = model_case(device, "shipped")
    net, datas = case["net"], case["datas"]
    with torch.no_grad():
        batch = SceneBatch(datas)
        direct = batch.split(net(batch))
    for a, b in zip(direct, case["u1"][0]):
        assert all(torch.equal(a[k], b[k]) for k in b)


def test_a_nan_in_one_scene_stays_in_that_scene(device):
    case = model_case(device, "shipped")
    net, datas = case["net"], case["datas"]
    clean = case["u1"][0]
    keep = datas[1].x.values
    try:
        bad = keep.clone()
        bad[bad.shape[0] // 2, 1] = float("nan")
        datas[1].x.values = bad
        with torch.no_grad():
            preds = forward_batch(net, datas)
    finally:
        datas[1].x.values = keep
    for i in (0, 2):
        for k in ("Ps_norm", "pts3D"):
            assert bool(torch.isfinite(preds[i][k]).all()), (i, k)
            assert torch.equal(preds[i][k], clean[i][k]), (i, k)
    assert bool(preds[1]["Ps_norm"].isnan().any())


def test_captured_step_over_a_fixed_union(device):
    case = model_case(device, "shipped")
    net, datas = case["net"], case["datas"]
    batch = SceneBatch(datas)
    torch.manual_seed(6)
    cP = [torch.randn(d.x.shape[0], 3, 4, device=device) for d in datas]
    cX = [torch.randn(4, d.x.shape[1], device=device) for d in datas]

    def fwd_bwd():
        preds = batch.split(net(batch))
        loss = sum((p["Ps_norm"] * a).sum() + (p["pts3D"] * b).sum() for p, a, b in zip(preds, cP, cX))
        loss.backward()
        return loss

    for p in net.parameters():
        p.grad = None
    fwd_bwd()
    eager = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    step = CapturedStep(fwd_bwd, list(net.parameters()))
    assert step.fallback_reason is None and step.captured
    step()
    torch.cuda.synchronize()
    bad = [k for k, p in net.named_parameters() if not torch.equal(p.grad, eager[k])]
    assert not bad, bad


def test_union_of_one_scene_matches_the_plain_forward(device):
    case = model_case(device, "shipped")
    net, datas = case["net"], case["datas"]
    with torch.no_grad():
        one = forward_batch(net, datas[:1])[0]
        plain = net(datas[0])
    for k in plain:
        np.testing.assert_allclose(one[k].cpu().numpy(), plain[k].cpu().numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
