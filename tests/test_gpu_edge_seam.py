"""The camera-item edge kernels at the ABI and through their Functions, on hand-made camera plans.

gasfm_edge_cam_fwd / gasfm_edge_cam_pbwd (csrc/edge_cam.hip) and the forward seams
gasfm_edge_seam_fwd / gasfm_edge0_seam_fwd (csrc/edge_seam.hip) against an fp64 torch restatement
of what they compute (block b's edge epilogue, layers.py:245-261 and 214-220 for block 0; block
b+1's LayerNorm + ReLU and both convs' lin_l, layers.py:232-234; the camera-direction GATv2
attention, oracle/pyg_gatv2.py), on two graphs built for the kernels' item loops:

  hand_graph()    13 cameras with 0, 0, 1, 15, 16, 17, 0, 31, 32, 33, 48, 300 and 0 edges: an empty
                  work item first, in a run, between non-empty ones and last; item lengths on both
                  sides of the 16-row tile; camera 11 whole (max_piece 4096), in two pieces (256:
                  one combine level) and in 43 (7: both combine levels, every other non-empty
                  camera but 2 split as well); points 310..319 without an edge.
  stride_graph()  9000 cameras with c % 5 edges: more complete items (slot < 0) than an MI355X
                  holds waves (256 CUs x 32), so every wave takes its next item `it += nw` whatever
                  the kernels' occupancy, and one item in five is empty.

Forward outputs are written into NaN-filled buffers with guard rows on both sides (a store to a
row outside the item's own shows as a finite guard row or as a wrong neighbouring row), with pos
given and without, and with Sv / XR as the two halves of one [m, 64] block (row stride 64).

Tolerances (fp32 vs fp64, those of test_gpu_edge_cam.py / test_gpu_edge_block.py): per-edge rows,
aggregates and statistics |d| <= 1e-5 + 1e-4 |ref|; per-node sums (dXR, dSv, dSp: up to 300
edges) atol = rtol = 1e-4; sums over every edge within 1e-4 of their largest element (close_sum).
Block 0's 2-wide LayerNorm is ill-conditioned where x0 ~ x1: its forward is bounded by
1e-5 + 1e-4 |ref| + 4 |fp32 torch - fp64| elementwise and its gradients normwise by
max(1e-5 ||ref|| + 1e-6, 4 ||fp32 torch - fp64||), as test_block0_edge_body_fwd_bwd.

SeamFn returns block b's input gradient through its token input (dP' = the gradient of its output
P', which block b's own EdgeCamFn folds into dP): the token's gradient is compared with the fp64
gradient of P'.  Block b's LayerNorm gradients are that EdgeCamFn's (test_edge_cam_fn_bwd with the
token gradient).  Seam0Fn is chained behind Block0PrologueFn, which turns its aux gradient into
block 0's dP and LN_a gradients.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gasfm_amd import _native, attention, edge_block
from gasfm_amd.attention import AttnPlan
from gasfm_amd.edge_block import PROJ_SCALE, Block0PrologueFn, EdgeCamFn, Seam0Fn, SeamFn
from oracle.pyg_gatv2 import gatv2_segment_reference
from test_gpu_edge_cam import close, close_sum

gpu = pytest.mark.gpu

EPS = 1e-5
SLOPE = 0.2
GUARD = 3  # NaN rows on either side of every output the kernels write
HAND_DEG = [0, 0, 1, 15, 16, 17, 0, 31, 32, 33, 48, 300, 0]
HAND_EMPTY = [0, 1, 6, 12]
PIECES = [4096, 256, 7]


def _graph(name, deg, n, pts_of):
    """Camera-major edges (as M2sparse emits them): camera c's points are pts_of(c, deg[c]), sorted."""
    m = len(deg)
    cam = np.repeat(np.arange(m), deg).astype(np.int64)
    pt = np.concatenate([np.asarray(sorted(pts_of(c, d)), dtype=np.int64) for c, d in enumerate(deg)])
    assert len(set(zip(cam.tolist(), pt.tolist()))) == cam.size  # one edge per (camera, point)
    return types.SimpleNamespace(name=name, m=m, n=n, E=int(cam.size), deg=np.asarray(deg),
                                 cam=torch.from_numpy(cam), pt=torch.from_numpy(pt))


@functools.lru_cache(maxsize=None)
def hand_graph():
    return _graph("hand", HAND_DEG, 320, lambda c, d: [(7 * c + 3 * j) % 310 for j in range(d)])


@functools.lru_cache(maxsize=None)
def stride_graph():
    return _graph("stride", [c % 5 for c in range(9000)], 64, lambda c, d: [(c + 13 * j) % 64 for j in range(d)])


GRAPHS = {"hand": hand_graph, "stride": stride_graph}


@functools.lru_cache(maxsize=None)
def cam_plan(gname, max_piece, all_partial=False):
    g = GRAPHS[gname]()
    return AttnPlan.from_targets(g.cam, g.m, max_piece=max_piece, all_partial=all_partial)


@functools.lru_cache(maxsize=None)
def point_plan(gname):
    g = GRAPHS[gname]()
    return AttnPlan.from_targets(g.pt, g.n)


def _items_of(plan, c):
    it = plan.items.numpy()
    return it[it[:, 0] == c]


def test_hand_graph_plans():
    """The camera plans of hand_graph() hold the items the GPU tests rely on (host only)."""
    g = hand_graph()
    assert g.E == 493 and g.m == 13 and g.n == 320
    p = cam_plan("hand", 4096)
    assert p.perm is None and p.n_items == 13 and p.n_slots == 0
    it = p.items.numpy()
    assert np.array_equal(it[:, 0], np.arange(13)) and np.all(it[:, 3] == -1)
    for c in HAND_EMPTY:
        assert it[c, 1] == it[c, 2]
    assert np.array_equal(it[:, 2] - it[:, 1], HAND_DEG)
    p = cam_plan("hand", 256)
    assert len(_items_of(p, 11)) == 2 and p.n_combine == 1 and p.n_l1 == 0 and p.n_slots == 2
    p = cam_plan("hand", 7)
    assert len(_items_of(p, 11)) == 43 and 43 > attention.L1_THRESHOLD and p.n_l1 > 0
    for c in HAND_EMPTY:
        w = _items_of(p, c)
        assert w.shape[0] == 1 and w[0, 1] == w[0, 2] and w[0, 3] == -1
    w = _items_of(p, 2)
    assert w.shape[0] == 1 and w[0, 2] - w[0, 1] == 1 and w[0, 3] == -1
    assert np.all(np.diff(p.items.numpy()[:, 0]) >= 0)  # items in camera order: empty first / in a run / last
    pp = point_plan("hand")
    assert pp.perm is not None and pp.pos is not None
    assert not pp.segment_lengths()[310:].any()
    pa = cam_plan("hand", 256, True)
    assert pa.all_partial and np.all(pa.items.numpy()[:, 3] >= 0)
    # the stride graph: one complete item per camera, more of them than the device holds waves
    ps = cam_plan("stride", 4096)
    assert stride_graph().E == 18000 and ps.n_items > 8192 and ps.n_slots == 0
    it = ps.items.numpy()
    assert np.all(it[:, 3] == -1) and int((it[:, 1] == it[:, 2]).sum()) == 1800


# ------------------------------------------------------------------------------ inputs, reference
@functools.lru_cache(maxsize=None)
def leaves(gname, entry, ln, with_p0):
    """fp32 CPU inputs of one entry point (cam: EdgeCamFn, seam: SeamFn, seam0: Seam0Fn) with the
    next block's LayerNorm (ln) and block b's P0 skip input (with_p0; seam only)."""
    g = GRAPHS[gname]()
    E, m, n = g.E, g.m, g.n
    gen = torch.Generator().manual_seed(1000 + 97 * len(gname) + 7 * len(entry) + 2 * ln + with_p0)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc
    t = dict(Wpt=r(32, 32, sc=0.2), bpt=r(32, sc=0.1), Wc=r(32, 32, sc=0.2), bc=r(32, sc=0.1), XR=r(m, 32),
             att=r(1, 4, 8, sc=0.35), bias=r(32, sc=0.1), Wpn=r(32, 34, sc=0.2), P0n=r(E, 2))
    if ln:
        t.update(lw=1 + 0.3 * r(32), lb=0.2 * r(32))
    if entry == "cam":
        t.update(P=r(E, 32))
        return t
    t.update(Sp=r(n, 32), Sv=r(m, 32), Sg=r(1, 32), bp=r(32, sc=0.1))
    if entry == "seam":
        t.update(P=r(E, 32), Wp=r(32, 34 if with_p0 else 32, sc=0.2), elw=1 + 0.3 * r(32), elb=0.2 * r(32))
        if with_p0:
            t.update(P0=r(E, 2))
    else:
        P = r(E, 2)
        P[::7, 1] = P[::7, 0]  # x0 == x1 rows of the 2-wide LayerNorm (rstd = 1 / sqrt(eps))
        t.update(P=P, Wp=r(32, 2), Wsk=r(32, 2), bsk=r(32, sc=0.1), law=1 + 0.1 * r(2), lab=0.1 * r(2),
                 lbw=1 + 0.1 * r(2), lbb=0.1 * r(2), W0=r(8, 2), b0=r(8, sc=0.1))
    return t


def ref_forward(entry, t, g):
    """Plain torch in t's dtype: P' (section "What the seam computes"), the next block's prologue on
    it and the camera attention.  Returns P', x = relu(LN(P')) (or P'), XLp, out, seg_max, seg_sum."""
    cam, pt = g.cam, g.pt
    if entry == "cam":
        Pn = t["P"]
    elif entry == "seam":
        ph = F.relu(F.layer_norm(t["P"], (32,), t["elw"], t["elb"], EPS))
        y = ph @ t["Wp"][:, :32].T + t["bp"] + t["Sg"] + t["Sp"][pt] + t["Sv"][cam]
        if "P0" in t:
            y = y + t["P0"] @ t["Wp"][:, 32:34].T
        Pn = t["P"] + PROJ_SCALE * y
    else:
        pa = F.relu(F.layer_norm(t["P"], (2,), t["law"], t["lab"], EPS))
        pb = F.relu(F.layer_norm(t["P"], (2,), t["lbw"], t["lbb"], EPS))
        Pn = pb @ t["Wsk"].T + t["bsk"] + PROJ_SCALE * (pa @ t["Wp"].T + t["bp"] + t["Sg"] + t["Sp"][pt] + t["Sv"][cam])
    x = F.relu(F.layer_norm(Pn, (32,), t["lw"], t["lb"], EPS)) if "lw" in t else Pn
    xlp = x @ t["Wpt"].T + t["bpt"]
    xlc = x @ t["Wc"].T + t["bc"]
    out, smax, ssum = gatv2_segment_reference(xlc.view(-1, 4, 8), t["XR"].view(-1, 4, 8), t["att"].view(4, 8),
                                              t["bias"], cam, g.m, SLOPE)
    return dict(Pout=Pn, x=x, XLp=xlp, out=out, smax=smax, ssum=ssum)


@functools.lru_cache(maxsize=None)
def forward_reference(gname, entry, ln, with_p0):
    """(fp64 reference, fp32 torch evaluation for block 0's bound else None), computed once."""
    g, t = GRAPHS[gname](), leaves(gname, entry, ln, with_p0)
    with torch.no_grad():
        r64 = ref_forward(entry, {k: v.double() for k, v in t.items()}, g)
        r32 = ref_forward(entry, t, g) if entry == "seam0" else None
    return r64, r32


def close32(got, r64, r32, msg=""):
    """test_block0_edge_body_fwd_bwd's elementwise bound: 1e-5 + 1e-4 |ref| + 4 |fp32 torch - fp64|."""
    got, r64, r32 = (np.asarray(x.detach().double().cpu()) for x in (got, r64, r32))
    bound = 1e-5 + 1e-4 * np.abs(r64) + 4 * np.abs(r32 - r64)
    over = np.abs(got - r64) - bound
    assert np.all(over <= 0), f"{msg}: {float(over.max()):.3e} over the bound"


# ------------------------------------------------------------------------------ forward at the ABI
def _nan_rows(rows, cols, dev):
    buf = torch.full((rows + 2 * GUARD, cols), float("nan"), device=dev)
    return buf, buf[GUARD:GUARD + rows]


def _guards_untouched(buf, rows, name):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + rows:]).all()), \
        f"{name}: a guard row was written"


def run_forward(entry, d, g, plan, pos, strided, dev, plan_partial=None, shard=None):
    """One forward of an entry point at the ABI through edge_block._cam_attention_fwd, as the
    Functions' forward does, every kernel output in a NaN-filled buffer with guard rows.  Returns
    Pout (None for cam), XLp, out, smax, ssum."""
    E, m = g.E, g.m
    Pout_b, Pout = _nan_rows(E, 32, dev)
    XLp_b, XLp = _nan_rows(E, 32, dev)
    Sv, XR = d.get("Sv"), d["XR"]
    if strided:  # the two halves of one [m, 64] block, as the gathered [SV | XR] rows
        blk = torch.zeros((m, 64), device=dev)
        blk[:, 32:] = XR
        XR = blk[:, 32:]
        if Sv is not None:
            blk[:, :32] = Sv
            Sv = blk[:, :32]
        assert XR.stride(0) == 64
    attf = d["att"].reshape(-1).contiguous()
    lw, lb = d.get("lw"), d.get("lb")
    pt32 = g.pt.int().to(dev)
    launches = []

    def launch(items, n_items, finalize, out, smax, ssum, part):
        own, o, s1, s2, p = {}, None, None, None, None
        if out is not None:
            own["out"], o = _nan_rows(m, 32, dev)
            own["smax"], s1 = _nan_rows(m, 4, dev)
            own["ssum"], s2 = _nan_rows(m, 4, dev)
        if part is not None:
            own["part"], p = _nan_rows(part.shape[0], part.shape[1], dev)
        tail = (lw, lb, EPS, d["Wpt"], d["bpt"], d["Wc"], d["bc"], XLp, pos, XR, attf,
                d["bias"] if finalize else None, SLOPE, items, n_items, finalize, o, s1, s2, p)
        if entry == "cam":
            _native.edge_cam_fwd(d["P"], *tail)
        elif entry == "seam":
            _native.edge_seam_fwd(d["P"], d.get("P0"), pt32, d["elw"], d["elb"], EPS, d["Wp"], d["bp"], d["Sp"], Sv,
                                  d["Sg"].reshape(-1), PROJ_SCALE, Pout, *tail)
        else:
            _native.edge0_seam_fwd(d["P"], pt32, d["law"], d["lab"], d["lbw"], d["lbb"], EPS, d["Wp"], d["bp"],
                                   d["Wsk"], d["bsk"], d["Sp"], Sv, d["Sg"].reshape(-1), PROJ_SCALE, Pout, *tail)
        for k, dst in (("out", out), ("smax", smax), ("ssum", ssum), ("part", part)):
            if dst is not None:
                _guards_untouched(own[k], dst.shape[0], k)
                dst.copy_(own[k][GUARD:GUARD + dst.shape[0]])
        launches.append(1)

    out, smax, ssum = edge_block._cam_attention_fwd(launch, d["bias"], plan, 4, 32, plan_partial, shard, dev)
    assert len(launches) == 1
    _guards_untouched(XLp_b, E, "XLp")
    assert not bool(torch.isnan(XLp).any()), "XLp: a row was not written"
    if entry != "cam":
        _guards_untouched(Pout_b, E, "Pout")
        assert not bool(torch.isnan(Pout).any()), "Pout: a row was not written"
    for k, v in (("out", out), ("seg_max", smax), ("seg_sum", ssum)):
        assert not bool(torch.isnan(v).any()), f"{k}: a row was not written"
    return dict(Pout=Pout if entry != "cam" else None, XLp=XLp, out=out, smax=smax, ssum=ssum)


def check_forward(entry, res, gname, ln, with_p0, pos, dev):
    g = GRAPHS[gname]()
    r64, r32 = forward_reference(gname, entry, ln, with_p0)
    bias = leaves(gname, entry, ln, with_p0)["bias"].to(dev)
    full_c = torch.from_numpy(g.deg > 0)
    full = full_c.to(dev)
    got = dict(res, XLp=res["XLp"] if pos is None else res["XLp"][pos.long()])  # row pos[e] holds edge e
    for k in ("Pout", "XLp", "out", "ssum", "smax"):
        if got[k] is None:
            continue
        a, b = got[k], r64[k]
        if k == "smax":  # an empty camera's maximum is -inf on both sides
            a, b = a[full], b[full_c]
        if r32 is None:
            close(a, b, msg=k)
        else:
            close32(a, b, r32[k][full_c] if k == "smax" else r32[k], msg=k)
    empty = ~full
    n_empty = int(empty.sum())
    assert n_empty > 0
    assert torch.equal(res["out"][empty], bias.expand(n_empty, 32)), "an empty camera's row is not the bias"
    assert not bool(res["ssum"][empty].any()), "an empty camera's seg_sum is not 0"


def _device_leaves(gname, entry, ln, with_p0, dev):
    return {k: v.to(dev) for k, v in leaves(gname, entry, ln, with_p0).items()}


FWD_CONFIGS = [("cam", True, False), ("cam", False, False),
               ("seam", True, True), ("seam", True, False), ("seam", False, True), ("seam", False, False),
               ("seam0", True, False)]
_cfg_id = lambda c: f"{c[0]}-{'ln' if c[1] else 'raw'}{'-p0' if c[2] else ''}"


@gpu
@pytest.mark.parametrize("strided", [False, True], ids=["rows32", "rows64"])
@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("max_piece", PIECES)
@pytest.mark.parametrize("cfg", FWD_CONFIGS, ids=_cfg_id)
def test_forward_hand_graph(device, cfg, max_piece, with_pos, strided):
    """edge_cam_fwd / edge_seam_fwd / edge0_seam_fwd on hand_graph(): Pout, XLp, the camera
    aggregates and the softmax statistics against fp64; empty cameras' rows exactly the bias with
    seg_sum 0; guard rows untouched and every row inside written; two launches bitwise equal."""
    entry, ln, with_p0 = cfg
    g = hand_graph()
    d = _device_leaves("hand", entry, ln, with_p0, device)
    plan = cam_plan("hand", max_piece).to(device)
    pos = point_plan("hand").pos.to(device) if with_pos else None
    res = run_forward(entry, d, g, plan, pos, strided, device)
    check_forward(entry, res, "hand", ln, with_p0, pos, device)
    again = run_forward(entry, d, g, plan, pos, strided, device)
    for k, v in res.items():
        assert v is None or torch.equal(v, again[k]), f"{k}: two launches differ"


@gpu
@pytest.mark.parametrize("max_piece", PIECES)
@pytest.mark.parametrize("cfg", [("cam", True, False), ("seam", True, True), ("seam", False, False),
                                 ("seam0", True, False)], ids=_cfg_id)
def test_forward_partial_rows_hand_graph(device, cfg, max_piece):
    """finalize = 0: every item (the empty ones too) writes a packed partial row of an all-partial
    plan, merged as one rank's share of a point-sharded scene; same bounds against fp64."""
    from gasfm_amd.distributed import ShardContext
    entry, ln, with_p0 = cfg
    g = hand_graph()
    d = _device_leaves("hand", entry, ln, with_p0, device)
    plan = cam_plan("hand", max_piece).to(device)
    partial = cam_plan("hand", max_piece, True).to(device)
    pos = point_plan("hand").pos.to(device)
    shard = ShardContext(0, 1, emulate=True)  # one rank: the gathered partial rows are its own
    res = run_forward(entry, d, g, plan, pos, False, device, plan_partial=partial, shard=shard)
    check_forward(entry, res, "hand", ln, with_p0, pos, device)
    again = run_forward(entry, d, g, plan, pos, False, device, plan_partial=partial, shard=shard)
    for k, v in res.items():
        assert v is None or torch.equal(v, again[k]), f"{k}: two launches differ"


@gpu
@pytest.mark.parametrize("cfg", [("cam", True, False), ("seam", True, True), ("seam0", True, False)], ids=_cfg_id)
def test_forward_stride_graph(device, cfg):
    """More complete items than resident waves: the kernels' `it += nw` loop over items that write
    their camera directly, one in five of them empty."""
    entry, ln, with_p0 = cfg
    g = stride_graph()
    d = _device_leaves("stride", entry, ln, with_p0, device)
    plan = cam_plan("stride", 4096).to(device)
    assert plan.n_items > 8192 and plan.n_slots == 0
    pos = point_plan("stride").pos.to(device)
    res = run_forward(entry, d, g, plan, pos, False, device)
    check_forward(entry, res, "stride", ln, with_p0, pos, device)
    again = run_forward(entry, d, g, plan, pos, False, device)
    for k, v in res.items():
        assert v is None or torch.equal(v, again[k]), f"{k}: two launches differ"


# ------------------------------------------------------------------------------ backward
def _cotangents(g, dres):
    gen = torch.Generator().manual_seed(77)
    c = dict(XLp=torch.randn(g.E, 32, generator=gen), out=torch.randn(g.m, 32, generator=gen))
    if dres:
        c["dres"] = torch.randn(g.E, 32, generator=gen)
    return c


def ref_backward(entry, gname, ln, with_p0, dres, dtype):
    """Autograd of the reference in dtype: gradients by leaf name, plus "Pout" (the gradient of P')."""
    g = GRAPHS[gname]()
    t = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in leaves(gname, entry, ln, with_p0).items()}
    cot = {k: v.to(dtype) for k, v in _cotangents(g, dres).items()}
    r = ref_forward(entry, t, g)
    if entry != "cam":
        r["Pout"].retain_grad()
    L = (r["XLp"] * cot["XLp"]).sum() + (r["out"] * cot["out"]).sum()
    if dres:  # the next block's output P' + (Wp [x | P0] + ...) / 4 as seen from its prologue
        L = L + (cot["dres"] * (r["Pout"] + PROJ_SCALE * (r["x"] @ t["Wpn"][:, :32].T
                                                          + t["P0n"] @ t["Wpn"][:, 32:].T))).sum()
    L.backward()
    grads = {k: v.grad for k, v in t.items()}
    grads["Pout"] = r["Pout"].grad if entry != "cam" else None
    return grads


def run_backward(entry, gname, max_piece, ln, with_p0, dres, dwp, dev):
    """Forward + backward of the entry's Function; returns {leaf name: gradient or None}, with
    "Pout": the token input's gradient (seam) and the epilogue-kernel call count left to the caller."""
    from gasfm_amd.model import EdgeIndex
    g = GRAPHS[gname]()
    d = {k: v.to(dev).requires_grad_(True) for k, v in leaves(gname, entry, ln, with_p0).items()}
    cot = {k: v.to(dev) for k, v in _cotangents(g, dres).items()}
    pc, pp = cam_plan(gname, max_piece).to(dev), point_plan(gname).to(dev)
    edges = EdgeIndex(g.cam.int().to(dev), g.pt.int().to(dev), g.m, g.n, {"proj2view": pc, "proj2scenepoint": pp})
    lw, lb = d.get("lw"), d.get("lb")
    cam_args = (lw, lb, d["Wpt"], d["bpt"], d["Wc"], d["bc"], d["Wpn"], EPS, pp.pos, d["XR"], d["att"], d["bias"], pc,
                4, SLOPE, None, None, d["P0n"] if dwp else None, dwp)
    token = None
    if entry == "cam":
        XLp, out, token_n = EdgeCamFn.apply(d["P"], *cam_args)
    elif entry == "seam":
        token = torch.zeros((g.E, 32), device=dev, requires_grad=True)  # never read; its gradient is dP'
        _, XLp, out, token_n = SeamFn.apply(d["P"], d.get("P0"), token, d["Sp"], d["Sv"], d["Sg"], d["Wp"], d["bp"],
                                            d["elw"], d["elb"], EPS, edges, dwp, *cam_args)
    else:
        _, tok0 = Block0PrologueFn.apply(d["P"], d["law"], d["lab"], d["W0"], d["b0"], EPS)
        _, XLp, out, token_n = Seam0Fn.apply(d["P"], tok0, d["Sp"], d["Sv"], d["Sg"], d["Wp"], d["bp"], d["law"],
                                             d["lab"], d["lbw"], d["lbb"], d["Wsk"], d["bsk"], EPS, edges, *cam_args)
    outs, gs = [XLp, out], [cot["XLp"], cot["out"]]
    if dres:
        outs.append(token_n)
        gs.append(cot["dres"])
    torch.autograd.backward(outs, gs)
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in d.items()}
    grads["Pout"] = token.grad if token is not None else None
    return grads


NEXT_SUMS = ("Wpt", "bpt", "Wc", "bc", "att", "bias", "lw", "lb")  # sums over every edge: close_sum


def _check_exact(entry, got, again, g):
    empty = torch.from_numpy(g.deg == 0).to(got["XR"].device)
    assert not bool(got["XR"][empty].any()), "dXR of an empty camera is not 0"
    if entry != "cam":
        assert not bool(got["Sv"][empty].any()), "dSv of an empty camera is not 0"
        unseen = torch.ones(g.n, dtype=torch.bool)
        unseen[g.pt] = False
        unseen = unseen.to(got["Sp"].device)
        if g.name == "hand":
            assert bool(unseen[310:].all())
        if bool(unseen.any()):
            assert not bool(got["Sp"][unseen].any()), "dSp of a point without edges is not 0"
    for k, v in got.items():
        if v is not None:
            assert not bool(torch.isnan(v).any()), f"d{k} holds a NaN"
            assert torch.equal(v, again[k]), f"d{k}: two backward passes differ"
        else:
            assert again[k] is None


def _check_cam_side(got, ref, ln, dres, dwp):
    close(got["XR"], ref["XR"], atol=1e-4, msg="dXR")
    for k in NEXT_SUMS:
        if k in ref:
            close_sum(got[k], ref[k], msg="d" + k)
    if dwp and dres and ln:
        close_sum(got["Wpn"], ref["Wpn"], msg="dWp (folded epilogue weight gradient)")
    else:
        assert got["Wpn"] is None


# (next block's LayerNorm, token gradient dRes, dwp); without the LayerNorm (the final update's raw
# features) the model has neither a residual nor a lin_proj gradient to fold
BWD_MODES = [(True, True, True), (True, True, False), (True, False, True), (True, False, False),
             (False, False, True), (False, False, False)]
_mode_id = lambda mo: f"{'ln' if mo[0] else 'raw'}-{'dres' if mo[1] else 'nores'}-{'dwp' if mo[2] else 'nodwp'}"


@gpu
@pytest.mark.parametrize("mode", BWD_MODES, ids=_mode_id)
@pytest.mark.parametrize("max_piece", PIECES)
def test_edge_cam_fn_bwd_hand_graph(device, max_piece, mode):
    """EdgeCamFn (edge_cam_fwd + edge_cam_pbwd) on hand_graph() against fp64 autograd."""
    ln, dres, dwp = mode
    g = hand_graph()
    got = run_backward("cam", "hand", max_piece, ln, False, dres, dwp, device)
    again = run_backward("cam", "hand", max_piece, ln, False, dres, dwp, device)
    ref = ref_backward("cam", "hand", ln, False, dres, torch.float64)
    close(got["P"], ref["P"], msg="dP")
    _check_cam_side(got, ref, ln, dres, dwp)
    _check_exact("cam", got, again, g)


def _count_epilogue_bwd(monkeypatch):
    calls = []
    orig = _native.edge_epilogue_bwd
    monkeypatch.setattr(_native, "edge_epilogue_bwd", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


def _check_seam(got, ref, with_p0, ln, dres, dwp):
    close(got["Pout"], ref["Pout"], msg="dP' (the token's gradient)")
    if with_p0:
        close(got["P0"], ref["P0"], msg="dP0")
    for k in ("Sv", "Sp"):
        close(got[k], ref[k], atol=1e-4, msg="d" + k)
    close_sum(got["Sg"], ref["Sg"], msg="dSg")
    close_sum(got["bp"], ref["bp"], msg="dbp")
    if dwp:  # wp_by_cam: block b's own EdgeCamFn returns its lin_proj gradient
        assert got["Wp"] is None
    else:
        close_sum(got["Wp"], ref["Wp"], msg="dWp")
    _check_cam_side(got, ref, ln, dres, dwp)


@gpu
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("with_p0", [True, False], ids=["p0", "nop0"])
@pytest.mark.parametrize("mode", BWD_MODES, ids=_mode_id)
@pytest.mark.parametrize("max_piece", PIECES)
def test_seam_fn_bwd_hand_graph(device, monkeypatch, max_piece, mode, with_p0, fold):
    """SeamFn on hand_graph() against fp64 autograd, with block b's epilogue backward folded into
    edge_cam_pbwd (EPI_FOLD with wp_by_cam: no edge_epilogue_bwd launch) and on its own."""
    ln, dres, dwp = mode
    g = hand_graph()
    monkeypatch.setattr(edge_block, "EPI_FOLD", fold)
    calls = _count_epilogue_bwd(monkeypatch)
    got = run_backward("seam", "hand", max_piece, ln, with_p0, dres, dwp, device)
    # folded: wp_by_cam, and the kernel's LN and RES forms together (block with both or the final update)
    folded = fold and dwp and ln == dres
    assert len(calls) == (0 if folded else 1), (len(calls), folded)
    again = run_backward("seam", "hand", max_piece, ln, with_p0, dres, dwp, device)
    ref = ref_backward("seam", "hand", ln, with_p0, dres, torch.float64)
    _check_seam(got, ref, with_p0, ln, dres, dwp)
    _check_exact("seam", got, again, g)


@gpu
@pytest.mark.parametrize("dwp", [True, False], ids=["dwp", "nodwp"])
@pytest.mark.parametrize("dres", [True, False], ids=["dres", "nores"])
@pytest.mark.parametrize("max_piece", PIECES)
def test_seam0_fn_bwd_hand_graph(device, max_piece, dres, dwp):
    """Block0PrologueFn + Seam0Fn on hand_graph() (with x0 == x1 rows) against fp64 autograd, at
    test_block0_edge_body_fwd_bwd's bounds relative to the fp32 torch evaluation's own error."""
    g = hand_graph()
    got = run_backward("seam0", "hand", max_piece, True, False, dres, dwp, device)
    again = run_backward("seam0", "hand", max_piece, True, False, dres, dwp, device)
    ref = ref_backward("seam0", "hand", True, False, dres, torch.float64)
    r32 = ref_backward("seam0", "hand", True, False, dres, torch.float32)
    nrm = lambda a, b: float((a.detach().double().cpu() - b.double()).norm())
    e_got, e_32 = nrm(got["P"], ref["P"]), nrm(r32["P"], ref["P"])
    assert e_got <= 4 * e_32 + 1e-5 * float(ref["P"].norm()), ("dP", e_got, e_32)
    names = ["law", "lab", "lbw", "lbb", "Wp", "bp", "Wsk", "bsk", "Sp", "Sv", "Sg", "XR", *NEXT_SUMS]
    if dwp and dres:
        names.append("Wpn")
    else:
        assert got["Wpn"] is None
    for k in names:
        e_got, e_32 = nrm(got[k], ref[k]), nrm(r32[k], ref[k])
        assert e_got <= max(1e-5 * float(ref[k].norm()) + 1e-6, 4 * e_32), ("d" + k, e_got, e_32)
    _check_exact("seam0", got, again, g)


@gpu
def test_seam_fn_bwd_stride_graph(device, monkeypatch):
    """SeamFn forward + backward over more complete items than resident waves, with the token
    gradient, the lin_proj gradient and the folded epilogue (edge_cam_pbwd's EPI and DWP forms)."""
    g = stride_graph()
    monkeypatch.setattr(edge_block, "EPI_FOLD", True)
    calls = _count_epilogue_bwd(monkeypatch)
    got = run_backward("seam", "stride", 4096, True, True, True, True, device)
    assert not calls
    again = run_backward("seam", "stride", 4096, True, True, True, True, device)
    ref = ref_backward("seam", "stride", True, True, True, torch.float64)
    _check_seam(got, ref, True, True, True, True)
    _check_exact("seam", got, again, g)
