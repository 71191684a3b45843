"""The 32 -> 128 edge epilogue kernels (csrc/edge_wide.hip), WideEpilogueFn and the wide route of a depth
conf's last block, at the smallest sizes at which each mechanism can go wrong.

References: the fp64 restatements of tests/edge_wide_ref.py (held to autograd of the unfused arithmetic by
tests/test_edge_wide_cpu.py).  Bars, all the project's own (tests/test_gpu_edge_block_edges.py): per-edge
outputs, dP / dP0 |d| <= 1e-5 + 1e-4 |ref|; parameter gradients normwise 1e-5 ||ref|| + 1e-6; per-node sums
(dSv, dSp, dSg) atol = rtol = 1e-4; model level: conftest.check_grad; captured step: the bars of
tests/test_gpu_depth_batch.py's trainer test.

  forward      E = 1 .. 33 (every remainder of the 16-edge tile, in the 32-wide row layout (lane>>3) + 8u, the
               128-wide one (lane>>5) + 2u and the MFMA C layout), 47 .. 49, 63 .. 65 (idle waves of the
               4-wave workgroup), 127 .. 129 (2 and 3 workgroups), and one size above a single pass of the
               kernel's own grid (edge_wide.part_shape(0): workgroups x edges per pass, + 17: `t += nw` and the
               prefetch of a second tile run).  Each size runs with P0 and contiguous Sv, and without P0
               with Sv as a column slice of an [m, 256] block.  Outputs in NaN-guarded exact-size buffers,
               inputs end in NaN rows, index arrays in indices of a NaN guard row of Sp / Sv.
  backward     hand_graph()'s camera plans whole and in pieces of 256 and of 7: item lengths 1, 15 .. 17,
               31 .. 33, 48, 300 and 0; partial buffers pre-filled NaN / 1e30 / NaN in three calls.
  rowsum       items of 0 .. 200 rows, perm given and None on a sorted plan, ldX = 136, part None.
  contracts    every refusal before a launch; E = 0 / n_items = 0.
  model        the whole block: route on against route off and against the fp64 net on the unfused route.
  captured     StaticTrainer's depth step takes the wide route, matches the eager union step, replays bitwise.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import gasfm_amd
from gasfm_amd import _native, edge_wide, model, static_batch, synthetic
from gasfm_amd.attention import AttnPlan, bwd_combine
from gasfm_amd.edge_block import PROJ_SCALE, WideEpilogueFn
from gasfm_amd.loss import DirectDepthLoss

import edge_wide_ref as ref
from conftest import check_grad
from test_gpu_edge_block import normwise
from test_gpu_edge_seam import GUARD, PIECES, cam_plan, hand_graph, point_plan

pytestmark = pytest.mark.gpu

SWEEP_E = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 127, 128, 129]
TAIL = 16
SENTINEL = 0x7FC5A5A5  # a NaN payload no arithmetic produces
NAMES = ("P", "P0", "Sp", "Sv", "Sg", "Wp", "bp", "Wsk", "bsk", "law", "lab", "lbw", "lbb")


def close(got, want, msg=""):
    got, want = got.detach().double().cpu(), want.double()
    bad = (got - want).abs() > 1e-5 + 1e-4 * want.abs()
    assert not bool(bad.any()), f"{msg}: {int(bad.sum())} elements, max |d| {float((got - want).abs().max()):.3e}"


def guarded(rows, cols, dev):
    """(buffer, view of its rows GUARD .. GUARD + rows - 1), every word the sentinel NaN."""
    buf = torch.full(((rows + 2 * GUARD) * cols,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    buf = buf.view(rows + 2 * GUARD, cols)
    return buf, buf[GUARD:GUARD + rows]


def guards_untouched(buf, rows, name):
    w = buf.view(torch.int32)
    assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + rows:] == SENTINEL).all()), f"{name}: guard rows written"
    assert bool(torch.isfinite(buf[GUARD:GUARD + rows]).all()), f"{name}: a live row is not finite"


def nan_tailed(t, dev, dtype=torch.float32):
    """t on the device as the first rows of a buffer that ends in TAIL NaN rows."""
    buf = torch.full((t.shape[0] + TAIL,) + tuple(t.shape[1:]), float("nan"), dtype=dtype, device=dev)
    buf[:t.shape[0]] = t.to(dtype)
    return buf[:t.shape[0]]


def tailed_index(idx, guard_row, dev):
    buf = torch.full((idx.shape[0] + TAIL,), guard_row, dtype=torch.int32, device=dev)
    buf[:idx.shape[0]] = idx.to(torch.int32)
    return buf[:idx.shape[0]]


def device_inputs(c, with_p0, dev, sv_slice=False):
    """c's inputs on the device: per-edge arrays NaN-tailed, Sp / Sv with a NaN guard row the index tails
    point at; sv_slice: Sv as columns 128 .. 255 of an [m + 1, 256] block."""
    f = lambda t: t.float().to(dev).contiguous()  # noqa: E731
    d = types.SimpleNamespace(P=nan_tailed(c.P, dev), P0=nan_tailed(c.P0, dev) if with_p0 else None,
                              cam=tailed_index(c.cam, c.m, dev), pt=tailed_index(c.pt, c.n, dev))
    d.Sp = torch.cat([c.Sp.float(), torch.full((1, ref.WO), float("nan"))]).to(dev)
    sv = torch.cat([c.Sv.float(), torch.full((1, ref.WO), float("nan"))]).to(dev)
    if sv_slice:
        block = torch.full((c.m + 1, 2 * ref.WO), float("nan"), device=dev)
        block[:, ref.WO:] = sv
        sv = block[:, ref.WO:]
    d.Sv, d.Sg = sv, f(c.Sg)
    d.Wp = f(c.Wp if with_p0 else c.Wp[:, :32])
    for k in ("bp", "Wsk", "bsk", "law", "lab", "lbw", "lbb"):
        setattr(d, k, f(getattr(c, k)))
    return d


def run_fwd(c, with_p0, dev, sv_slice):
    d = device_inputs(c, with_p0, dev, sv_slice)
    buf, out = guarded(c.E, ref.WO, dev)
    edge_wide.epilogue_fwd(d.P, d.P0, d.cam, d.pt, d.law, d.lab, d.lbw, d.lbb, ref.EPS, d.Wp, d.bp, d.Wsk, d.bsk,
                                   d.Sp, d.Sv, d.Sg, PROJ_SCALE, out)
    torch.cuda.synchronize()
    guards_untouched(buf, c.E, f"P' E={c.E}")
    return out


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("E", SWEEP_E)
def test_forward_sweep(device, E):
    c = ref.case(E)
    close(run_fwd(c, True, device, False), ref.fwd_ref(E, True), f"P' E={E} with P0")
    close(run_fwd(c, False, device, True), ref.fwd_ref(E, False), f"P' E={E} without P0, Sv a column slice")


def test_forward_above_one_pass(device):
    wg, per = edge_wide.part_shape(0, 1 << 30)
    assert wg >= 1 and per == 64
    E = wg * per + 17  # a second pass of the tile loop: one whole tile and a one-row tile
    c = ref.make_case(E, 9900)
    out = run_fwd(c, True, device, False)
    close(out, ref.fwd_of(c, True), f"P' E={E}")
    again = run_fwd(c, True, device, False)
    assert torch.equal(out, again)


# ------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def hand_case():
    g = hand_graph()
    c = ref.make_case(g.E, 9700, cam=g.cam, pt=g.pt, m=g.m, n=g.n)
    return c, {p0: ref.bwd_of(c, p0) for p0 in (True, False)}


def split_part(tot, ldWp):
    W = ref.WO
    o1 = W * ldWp
    o2 = o1 + W * 32
    o3 = o2 + W
    return dict(Wp=tot[:o1].view(W, ldWp), Wsk=tot[o1:o2].view(W, 32), bsk=tot[o2:o3], law=tot[o3:o3 + 32],
                lab=tot[o3 + 32:o3 + 64], lbw=tot[o3 + 64:o3 + 96], lbb=tot[o3 + 96:o3 + 128])


@pytest.mark.parametrize("with_p0", [True, False])
@pytest.mark.parametrize("max_piece", PIECES)
def test_backward_kernel_hand_graph(device, max_piece, with_p0):
    (c, refs), g = hand_case(), hand_graph()
    want = refs[with_p0]
    plan = cam_plan("hand", max_piece).to(device)
    d = device_inputs(c, with_p0, device)
    dPo = nan_tailed(c.dPo, device)
    ldWp = d.Wp.shape[1]
    rows, cols = edge_wide.part_shape(1, c.E, plan.n_items, ldWp)
    assert rows == min(-(-plan.n_items // 4), rows) and cols == 128 * ldWp + 128 * 32 + 128 + 128
    results = []
    for fill in (float("nan"), 1e30, float("nan")):
        bP, dP = guarded(c.E, 32, device)
        b0, dP0 = guarded(c.E, 2, device) if with_p0 else (None, None)
        bS, dSv = guarded(c.m, ref.WO, device)
        part = torch.full((rows, cols), fill, device=device)
        part_dsv = torch.full((max(plan.n_part_rows, 1), ref.WO), fill, device=device)
        edge_wide.epilogue_bwd(plan.items, plan.n_items, dPo, d.P, d.P0, d.law, d.lab, d.lbw, d.lbb, ref.EPS,
                                       d.Wp, d.Wsk, PROJ_SCALE, dP, dP0, dSv, part_dsv if plan.n_slots else None, part)
        bwd_combine(plan, part_dsv, ref.WO, dSv)
        tot = _native.colsum(part)
        torch.cuda.synchronize()
        guards_untouched(bP, c.E, "dP")
        guards_untouched(bS, c.m, "dSv")
        if with_p0:
            guards_untouched(b0, c.E, "dP0")
        assert bool(torch.isfinite(tot).all()), "a promised partial row was not written"
        results.append((dP.clone(), None if dP0 is None else dP0.clone(), dSv.clone(), tot))
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert (a is None and b is None) or torch.equal(a, b)
    dP, dP0, dSv, tot = results[0]
    close(dP, want["P"], "dP")
    last = int(g.deg[11]) % 16 or 16  # the last tile of the last camera with edges (300 = 18 tiles + 12 rows)
    e1 = int(np.cumsum(g.deg)[11])
    close(dP[e1 - last:e1], want["P"][e1 - last:e1], "dP, last tile")
    if with_p0:
        close(dP0, want["P0"], "dP0")
    torch.testing.assert_close(dSv.double().cpu(), want["Sv"], atol=1e-4, rtol=1e-4)
    for k, v in split_part(tot, ldWp).items():
        normwise(v, want[k], msg=f"d{k} pieces {max_piece}")


def _edges(c, plan_c, plan_p, dev):
    return types.SimpleNamespace(cam=c.cam.to(torch.int32).to(dev), pt=c.pt.to(torch.int32).to(dev), m=c.m, n=c.n,
                                 plans={"proj2view": plan_c, "proj2scenepoint": plan_p})


def run_fn(c, with_p0, edges, dev):
    lv = {k: getattr(c, k).float().to(dev).requires_grad_(True) for k in NAMES}
    if not with_p0:
        lv["P0"] = None
        lv["Wp"] = c.Wp[:, :32].float().contiguous().to(dev).requires_grad_(True)
    lv["Sg"] = c.Sg.float().view(1, -1).to(dev).requires_grad_(True)
    out = WideEpilogueFn.apply(*(lv[k] for k in NAMES), ref.EPS, edges)
    (out * c.dPo.float().to(dev)).sum().backward()
    return out, {k: v.grad for k, v in lv.items() if v is not None}


@pytest.mark.parametrize("with_p0", [True, False])
@pytest.mark.parametrize("max_piece", PIECES)
def test_wide_epilogue_fn_hand_graph(device, max_piece, with_p0):
    c, refs = hand_case()
    want = refs[with_p0]
    edges = _edges(c, cam_plan("hand", max_piece).to(device), point_plan("hand").to(device), device)
    out, grads = run_fn(c, with_p0, edges, device)
    close(out, ref.fwd_of(c, with_p0), "P'")
    close(grads["P"], want["P"], "dP")
    if with_p0:
        close(grads["P0"], want["P0"], "dP0")
    for k in ("Sv", "Sp", "Sg"):
        torch.testing.assert_close(grads[k].double().cpu().reshape(want[k].shape), want[k], atol=1e-4, rtol=1e-4)
    for k in ("Wp", "bp", "Wsk", "bsk", "law", "lab", "lbw", "lbb"):
        normwise(grads[k], want[k], msg=f"d{k} pieces {max_piece}")


# ------------------------------------------------------------------------------ the 128-wide segment row sum
ROWSUM_LEN = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 200, 0, 64]


@pytest.mark.parametrize("sorted_plan", [True, False])
@pytest.mark.parametrize("max_piece", [4096, 16])
def test_segment_rowsum_w(device, sorted_plan, max_piece):
    g = torch.Generator().manual_seed(31)
    tgt = torch.repeat_interleave(torch.arange(len(ROWSUM_LEN)), torch.tensor(ROWSUM_LEN))
    if not sorted_plan:
        tgt = tgt[torch.randperm(tgt.numel(), generator=g)]
    E, N = tgt.numel(), len(ROWSUM_LEN)
    plan = AttnPlan.from_targets(tgt, N, max_piece=max_piece).to(device)
    assert (plan.perm is None) == sorted_plan and (plan.n_slots == 0) == (max_piece == 4096)
    X64 = torch.randn(E, ref.WO, generator=g, dtype=torch.float64)
    block = torch.full((E + TAIL, 136), float("nan"), device=device)
    block[:E, :ref.WO] = X64.float().to(device)
    X = block[:E, :ref.WO]
    assert X.stride(0) == 136
    want = PROJ_SCALE * torch.zeros(N, ref.WO, dtype=torch.float64).index_add(0, tgt, X64)
    outs = []
    for fill in (float("nan"), 1e30):
        buf, out = guarded(N, ref.WO, device)
        part = torch.full((plan.n_part_rows, ref.WO), fill, device=device) if plan.n_slots else None
        edge_wide.segment_rowsum_w(plan.items, plan.n_items, plan.perm, X, PROJ_SCALE, out, part)
        if part is not None:
            bwd_combine(plan, part, ref.WO, out)
        torch.cuda.synchronize()
        guards_untouched(buf, N, "rowsum out")
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    torch.testing.assert_close(outs[0].double().cpu(), want, atol=1e-4, rtol=1e-4)
    assert float(outs[0][0].abs().max()) == 0.0 and float(outs[0][11].abs().max()) == 0.0  # empty segments


# ------------------------------------------------------------------------------ contracts
def _raw(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_entry_point_contracts(device):
    c = ref.case(17)
    d = device_inputs(c, True, device)
    L = edge_wide.lib()
    buf, out = guarded(c.E, ref.WO, device)
    stream = _native._stream(out)

    def fwd(**kw):
        a = dict(P=_raw(d.P), P0=_raw(d.P0), cam=_raw(d.cam), pt=_raw(d.pt), E=c.E, law=_raw(d.law), lab=_raw(d.lab),
                 lbw=_raw(d.lbw), lbb=_raw(d.lbb), ldWp=34, Wp=_raw(d.Wp), bp=_raw(d.bp), Wsk=_raw(d.Wsk),
                 bsk=_raw(d.bsk), Sp=_raw(d.Sp), Sv=_raw(d.Sv), ldSv=128, Sg=_raw(d.Sg), out=_raw(out))
        a.update(kw)
        return L.gasfm_edge_wide_epilogue_fwd(a["P"], a["P0"], a["cam"], a["pt"], a["E"], a["law"], a["lab"], a["lbw"],
                                              a["lbb"], ref.EPS, a["Wp"], a["ldWp"], a["bp"], a["Wsk"], a["bsk"],
                                              a["Sp"], a["Sv"], a["ldSv"], a["Sg"], PROJ_SCALE, a["out"], stream)

    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)  # noqa: E731
    bad = [dict(E=-1), dict(law=None), dict(lbb=None), dict(P0=None), dict(ldWp=32), dict(ldSv=64), dict(ldSv=130),
           dict(P=off4(d.P)), dict(Sp=off4(d.Sp)), dict(out=off4(out)), dict(law=off4(d.law))]
    bad += [{k: None} for k in ("P", "cam", "pt", "Wp", "bp", "Wsk", "bsk", "Sp", "Sv", "Sg", "out")]
    for kw in bad:
        assert fwd(**kw) == _native.GASFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == SENTINEL).all()), "a refused call launched"
    assert fwd(E=0, P=None, out=None, cam=None, pt=None, Sp=None) == _native.GASFM_OK
    assert fwd() == _native.GASFM_OK

    plan = AttnPlan.from_targets(c.cam.sort().values, c.m).to(device)
    dPo = c.dPo.float().to(device)
    rows, cols = edge_wide.part_shape(1, c.E, plan.n_items, 34)
    bP, dP = guarded(c.E, 32, device)
    dP0, dSv = torch.empty(c.E, 2, device=device), torch.empty(c.m, ref.WO, device=device)
    part = torch.empty(rows, cols, device=device)

    def bwd(**kw):
        a = dict(items=_raw(plan.items), n=plan.n_items, dPo=_raw(dPo), P=_raw(d.P), P0=_raw(d.P0), law=_raw(d.law),
                 lab=_raw(d.lab), lbw=_raw(d.lbw), lbb=_raw(d.lbb), Wp=_raw(d.Wp), ldWp=34, Wsk=_raw(d.Wsk), dP=_raw(dP),
                 dP0=_raw(dP0), dSv=_raw(dSv), part=_raw(part))
        a.update(kw)
        return L.gasfm_edge_wide_epilogue_bwd(a["items"], a["n"], a["dPo"], a["P"], a["P0"], a["law"], a["lab"],
                                              a["lbw"], a["lbb"], ref.EPS, a["Wp"], a["ldWp"], a["Wsk"], PROJ_SCALE,
                                              a["dP"], a["dP0"], a["dSv"], None, a["part"], stream)

    bad = [dict(lab=None), dict(lbw=None), dict(dP0=None), dict(ldWp=32), dict(P0=None), dict(dPo=off4(dPo)),
           dict(dP=off4(dP))]
    bad += [{k: None} for k in ("items", "dPo", "P", "Wp", "Wsk", "dP", "dSv", "part")]
    for kw in bad:
        assert bwd(**kw) == _native.GASFM_ERR_INVALID, kw
    torch.cuda.synchronize()
    assert bool((bP.view(torch.int32) == SENTINEL).all()), "a refused call launched"
    assert bwd(n=0, items=None, dPo=None, dP=None) == _native.GASFM_OK
    assert edge_wide.part_shape(1, 0, 0, 34)[0] == 0 and edge_wide.part_shape(0, 0)[0] == 0

    X = torch.zeros(4, 128, device=device)
    one = AttnPlan.from_targets(torch.zeros(4, dtype=torch.int64), 1).to(device)
    o = torch.zeros(1, 128, device=device)
    rs = lambda **kw: L.gasfm_segment_rowsum_w(kw.get("items", _raw(one.items)), kw.get("n", one.n_items), None,  # noqa: E731
                                               kw.get("X", _raw(X)), kw.get("ldX", 128), 1.0, kw.get("out", _raw(o)),
                                               None, stream)
    for kw in (dict(items=None), dict(X=None), dict(out=None), dict(ldX=64), dict(ldX=130), dict(X=off4(X))):
        assert rs(**kw) == _native.GASFM_ERR_INVALID, kw
    assert rs(n=0, items=None, X=None, out=None) == _native.GASFM_OK and rs() == _native.GASFM_OK


@pytest.mark.parametrize("with_p0", [True, False])
def test_fn_without_edges(device, with_p0):
    c = ref.make_case(0, 5)
    empty = torch.zeros(0, dtype=torch.int64)
    edges = _edges(c, AttnPlan.from_targets(empty, c.m).to(device), AttnPlan.from_targets(empty, c.n).to(device), device)
    out, grads = run_fn(c, with_p0, edges, device)
    assert tuple(out.shape) == (0, ref.WO) and tuple(grads["P"].shape) == (0, 32)
    for k, v in grads.items():
        assert float(v.abs().sum()) == 0.0 and v.shape == (c.Wp[:, :32] if k == "Wp" and not with_p0 else
                                                           c.Sg.view(1, -1) if k == "Sg" else getattr(c, k)).shape, k


# ------------------------------------------------------------------------------ the whole block at model level
def _depth_conf():
    return gasfm_amd.conf.learning_conf(depth_head={"enabled": True, "n_feat": 128, "n_hidden_layers": 2},
                                        view_head={"enabled": False, "n_hidden_layers": 2, "rot_representation": "quat"},
                                        scenepoint_head={"enabled": False, "n_hidden_layers": 2})


def _oracle_depths(sd, sc, coef, dtype):
    """The depth conf's forward as the oracle's composition of the same state dict (its blocks are the
    unfused arithmetic; the package's own attention runs in fp32 on the device only): depths [E, 1] and
    every parameter gradient of sum(depths * coef)."""
    from oracle import gasfm_ref, scenes
    g = scenes.graph_from_edges(sc.cam, sc.pt, sc.m, sc.n)
    sdt = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    P0 = gasfm_ref._lin(sdt, "embed.post_embed_lin", torch.from_numpy(sc.normalized_values()).to(dtype))
    P, prev = P0, (None, None, None)
    for b in range(1 + max(int(k.split(".")[1]) for k in sdt if k.startswith("equivariant_blocks."))):
        P, prev = gasfm_ref._block(sdt, f"equivariant_blocks.{b}", P, P0, g, prev, 4)
    d = gasfm_ref._mlp(sdt, "depth_head", P)
    (d * coef.to(dtype)).sum().backward()
    return d.detach().double(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy()
                                 for k, v in sdt.items()}


def test_model_wide_route(device, monkeypatch):
    from oracle.weights import deterministic_state_dict
    sc = synthetic.windowed_scene(8, 80, mean_extra=3, seed=11)
    net = gasfm_amd.GraphAttnSfMNet(_depth_conf())
    sd = deterministic_state_dict(net.state_dict())
    net.load_state_dict(sd)
    net = net.to(device)
    data = gasfm_amd.SceneData.from_synthetic(sc).to(device)
    coef = torch.randn(sc.num_edges, 1, generator=torch.Generator().manual_seed(2), dtype=torch.float64)

    def run():
        net.zero_grad(set_to_none=True)
        depths = net(data)["depths"].values
        (depths * coef.float().to(device)).sum().backward()
        return depths.detach().double().cpu(), {k: (p.grad if p.grad is not None else torch.zeros_like(p)).double().cpu()
                                                for k, p in net.named_parameters()}

    last = net.equivariant_blocks[-1]
    assert last.fusable_wide() and not last.fusable()
    d_on, g_on = run()
    assert last.last_route == "wide" and net.last_routes[-1] == "wide" and set(net.last_routes[1:-1]) == {"fused"}
    assert net.last_carry is None or net.last_carry.pending() == []
    monkeypatch.setattr(model, "EDGE_WIDE", False)
    d_off, g_off = run()
    assert last.last_route == "unfused" and net.last_routes[-1] == "unfused"
    d64, g64 = _oracle_depths(sd, sc, coef, torch.float64)
    d32, g32 = _oracle_depths(sd, sc, coef, torch.float32)
    assert tuple(d_on.shape) == tuple(d64.shape) == (sc.num_edges, 1) and set(g64) == set(g_on)
    print(f"depths: on - off {float((d_on - d_off).abs().max()):.3e}, on - fp64 {float((d_on - d64).abs().max()):.3e}, "
          f"off - fp64 {float((d_off - d64).abs().max()):.3e}, |fp64| {float(d64.abs().max()):.3e}")
    check_grad(d_on, d_off.numpy(), "depths on / off")
    check_grad(d_on, d64.numpy(), "depths on / fp64", ref32=d32.numpy())
    check_grad(d_off, d64.numpy(), "depths off / fp64", ref32=d32.numpy())
    for k in g64:
        check_grad(g_on[k], g64[k], f"{k} on / fp64", ref32=g32[k])
        check_grad(g_off[k], g64[k], f"{k} off / fp64", ref32=g32[k])
        check_grad(g_on[k], g_off[k].numpy(), f"{k} on / off", ref32=g32[k] - g64[k] + g_off[k].numpy())


# ------------------------------------------------------------------------------ the captured step
def test_static_trainer_takes_the_wide_route(device, monkeypatch):
    from test_gpu_depth_batch import _check_step_grads, _eager_union, _train_scenes, depth_conf
    monkeypatch.setattr(static_batch, "S2G_PIECES", 128)  # as that module's tests: ~1-2k valid points per scene
    monkeypatch.setattr(static_batch, "MAX_WASTE", 10.0)
    torch.manual_seed(5)
    conf = depth_conf("L2")
    net = gasfm_amd.GraphAttnSfMNet(conf).to(device)
    lossf = DirectDepthLoss(conf)
    datas = _train_scenes(device, (12, 15), seed=3)
    loss_ref, g_ref = _eager_union(net, lossf, datas)
    assert net.equivariant_blocks[-1].last_route == "wide"
    trainer = static_batch.StaticTrainer(net, lossf, two_view_error=True)
    seen = []
    for k in range(2):
        net.equivariant_blocks[-1].last_route = None
        torch.manual_seed(7)  # the same fill both times: the 2-view pairing keys are drawn when the bucket is filled
        loss, errs = trainer.step(datas)
        assert trainer.captures == 1 and trainer.fallbacks == [] and trainer.eager_steps == 0
        assert next(iter(trainer.buckets.values()))[1].captured
        if k == 0:
            assert net.equivariant_blocks[-1].last_route == "wide"  # set while the step was captured
        assert abs(float(loss) - loss_ref) <= 1e-4 * abs(loss_ref)
        _check_step_grads(net, g_ref, f"step {k}")
        seen.append((float(loss), list(errs), [None if p.grad is None else p.grad.clone() for p in net.parameters()]))
    assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1]
    for a, b in zip(seen[0][2], seen[1][2]):
        assert (a is None and b is None) or torch.equal(a, b)
