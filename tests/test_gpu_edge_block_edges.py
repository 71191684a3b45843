"""Edges of the per-edge block kernels (csrc/edge_block.hip, csrc/edge_block0.hip, segment_rowsum):
16-row tile remainders, idle waves and workgroups, the XCD tile ranges of the epilogue forward, the
grid-stride loops, the split operands production passes, exact-size buffers, recycled partial rows
and the entry points' contracts.

References are the fp64 torch restatements of test_gpu_edge_block.py, callable with eps and the
variant flags (pro_ref, epi_ref, pbwd_ref, e0_* below; pbwd_ref is the closed form, checked against
autograd of pro_ref / epi_ref by the one test here that needs no GPU).  Bars, all the project's own:
per-edge outputs, dP / dP0 / aux |d| <= 1e-5 + 1e-4 |ref| (test_gpu_edge_block.py); parameter
gradients normwise 1e-5 ||ref|| + 1e-6; per-node sums (dSv, dSp) atol = rtol = 1e-4
(test_gpu_edge_seam.py); block-0 rows with x0 == x1: 1e-5 + 1e-4 |ref| + 4 |fp32 torch - fp64|
(close32).  dP meets its bar a second time over the last tile's rows alone.  Every fp64-compared
case with E <= 1000 has its LayerNorm beta moved off the ReLU edge (relu_edge.off_relu_edge); the
loop cases (E > 1000) move the few elements of P whose pre-activation lies within the margin instead
(_nudge_off_edge); block 0's P has |x0 - x1| >= 3 (_p0_rows says why not 0.1): x_hat ~ +-1.

Which (E, variant) reaches which mechanism -- what a removed case would uncover:

  remainder      A wave owns a 16-row tile; E % 16 = 1 .. 15 and 0 all run (E = 1 .. 33).  Rows past E
                 re-read row 0 of the tile (load_rows32, pb_issue, issue, the npos / ncam / npt clamps)
                 and are masked later in three layouts: the row layout (lane>>3) + 8u (a remainder
                 that is no multiple of 8 cuts a lane group), the XL row layout (lane>>4) + 4u and the
                 MFMA C layout 4 (lane>>4) + r (no multiple of 4).  A dropped mask adds a finite
                 duplicate of row 0 to dW / db / dgamma / dbeta: only fp64 sees it (section A).  The
                 epilogue forward's cam / pt use index 0 in the last live row, so a clamped dead row is
                 not told apart by its index.
  idle waves     A workgroup is 4 waves = 64 rows.  E < 16: three idle waves, E <= 48: one or two,
                 E = 47 .. 49, 63 .. 65: the edges; their accW must be 0 inside wg_reduce<40> / <20>.
  workgroups     E = 65, 127 .. 129: 2 and 3 workgroups (several partial rows, a last workgroup with
                 one live row); E = 448 / 449 / 465 / 513 / 577: 28, 29, 30, 33, 37 tiles = 7, 8, 8, 9,
                 10 workgroups of edge_epilogue_fwd: nx goes 1 -> 8 at 8 workgroups (E = 449), with
                 ntiles % 8 != 0 (29, 30, 33, 37) and gridDim.x % 8 != 0 (9, 10): t_lo / t_hi / blk_x.
                 A gap is a skipped row: section C's sentinel outputs show it at 449.
  loop,          E = 140 001 (8751 tiles > 256 CUs x 32 waves), 270 001 / 40 001 (block 0: kMaxGrid
  prefetch       = 1024 workgroups of 256 / 32 edges), stride_graph() (9000 items) and a 9000-segment
                 point plan: the only sizes at which `t += nw`, issue(t + nw) and the `w = wn` /
                 `wn = wnn` item pipelines run; in guarded, poisoned buffers, run twice (section C).
  split          W2 / b2 halves, pos, ldY = 72, dXLc with ldC = 32 and 64, Wp [32, 34] read with its
  operands       row stride by the prologue backward, Sv as [:, :32] of an [m, 64] block, RES / LN on
                 and off, P0 None (p0p aliases P): the full cross product at E = 1, 5, 17, 63, 65, 130,
                 the production variant (LN + RES + split W + dXLc) over the whole sweep.
  Functions      EdgePrologueFn + EdgeEpilogueFn at E = 1, 17, 65 (one workgroup and two): the Python
                 slicing of `tot`, dSv / dSp / dSg through the plans, P0 given and None.
  block 0        edge0_prologue_fwd / _rows: 256 edges per workgroup (E = 255 .. 257); epilogue
                 forward: 8 lanes per edge, 32 edges per workgroup (E = 1 .. 9, 31 .. 33, 257); epilogue
                 backward: 4 groups of 8 rows per step, item lengths 1, 15 .. 17, 31 .. 33, 48, 300
                 (hand_graph(), whole and in pieces of 256 and 7) and 1, 0, 9.
  segment_rowsum ldX = 40, perm None on a sorted plan, part None without slots, items of 0 .. 200 rows.
  exact-size     Section C: outputs are rows GUARD .. GUARD+E-1 of a buffer holding one NaN bit
  buffers        pattern (guards and the pad columns of ldY = 72 must keep it, live rows must be
                 finite), inputs end in 16 NaN rows, index arrays in 16 out-of-table indices that point
                 at a NaN guard row of Sp / Sv.
  partial rows   Section C: part / part_w / part_dsv / part_dsp pre-filled NaN, 1e30, NaN in three
                 successive calls; the reduced gradients bitwise equal and finite.  torch.empty in
                 production, and param_colsum sums every promised row.
  contracts      Section D: every GASFM_REQUIRE of these entry points refuses before a launch; E = 0 /
                 n_items = 0 return OK without looking at a pointer, and the Functions give empty
                 tensors and zero parameter gradients.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gasfm_amd import _native
from gasfm_amd.attention import AttnPlan, bwd_combine
from gasfm_amd.edge_block import (PROJ_SCALE, Block0EpilogueFn, Block0PrologueFn, EdgeEpilogueFn, EdgePrologueFn)
from relu_edge import RELU_MARGIN, off_relu_edge
from test_gpu_edge_block import normwise
from test_gpu_edge_seam import GUARD, PIECES, cam_plan, close32, hand_graph, point_plan, stride_graph

gpu = pytest.mark.gpu

EPS = 1e-5
SWEEP_E = list(range(1, 34)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 448, 449, 465, 513, 577]
CROSS_E = [1, 5, 17, 63, 65, 130]
FN_E = [1, 17, 65]
KERNEL_E = [21, 65, 449]
E0_PRO_E = [1, 2, 63, 64, 65, 255, 256, 257]
E0_EPI_E = list(range(1, 10)) + [31, 32, 33, 257]
BIG_E, BIG_E0_PRO, BIG_E0_EPI = 140_001, 270_001, 40_001
M_TAB, N_TAB = 5, 7
TAIL = 16  # NaN rows behind every per-edge input of section C
PART_GUARD = 2
SENTINEL = 0x7FC5A5A5  # a NaN payload no arithmetic produces
NPART = 64 * 32 + 64 + 64  # [dW | db | dgamma | dbeta] of edge_prologue_bwd


# ------------------------------------------------------------------------------ fp64 references (CPU only)
def _ln_relu(P, g, b, eps):
    return F.relu(F.layer_norm(P, P.shape[1:], g, b, eps))


def pro_ref(P, lnw, lnb, W, b, eps=EPS):
    """XL = W relu(LN(P)) + b; lnw None: W P + b."""
    return (P if lnw is None else _ln_relu(P, lnw, lnb, eps)) @ W.T + b


def epi_ref(P, P0, cam, pt, lnw, lnb, Wp, bp, Sp, Sv, Sg, eps=EPS):
    """P' = P + (Wp [relu(LN(P)) | P0] + bp + Sp[pt] + Sv[cam] + Sg) / 4; P0 None: Wp is [32, 32]."""
    ph = _ln_relu(P, lnw, lnb, eps)
    x = ph if P0 is None else torch.cat([ph, P0], 1)
    return P + PROJ_SCALE * (x @ Wp.T + bp + Sp[pt] + Sv[cam] + Sg.reshape(-1))


def pbwd_ref(P, lnw, lnb, W, Wp, dXL, dRes, eps=EPS):
    """edge_prologue_bwd in closed form: dP = LN_bwd(mask (W^T dXL + scale Wp[:, :32]^T dRes)) + dRes,
    dW = dXL^T relu(LN(P)), db, dgamma, dbeta; lnw None: no LayerNorm, dRes None: no residual."""
    dy = dXL @ W
    if dRes is not None:
        dy = dy + PROJ_SCALE * dRes @ Wp[:, :32]
    if lnw is None:
        ph, dP, dg, dbt = P, dy, torch.zeros(32, dtype=P.dtype), torch.zeros(32, dtype=P.dtype)
    else:
        mean = P.mean(1, keepdim=True)
        rstd = ((P - mean).pow(2).mean(1, keepdim=True) + eps).rsqrt()
        xh = (P - mean) * rstd
        pre = xh * lnw + lnb
        ph, dy = pre.clamp_min(0), dy * (pre > 0)
        dg, dbt = (dy * xh).sum(0), dy.sum(0)
        gv = dy * lnw
        dP = rstd * (gv - gv.mean(1, keepdim=True) - xh * (gv * xh).mean(1, keepdim=True))
    if dRes is not None:
        dP = dP + dRes
    return dict(dP=dP, dW=dXL.T @ ph, db=dXL.sum(0), dgamma=dg, dbeta=dbt)


def _nudge_off_edge(P, g, b, eps):
    """P with the few elements whose pre-activation LN(P) g + b lies within RELU_MARGIN of 0 moved by
    0.01 (the loop cases: too many rows for a per-column shift of beta to clear)."""
    for _ in range(50):
        pre = F.layer_norm(P, P.shape[1:], g, b, eps)
        bad = pre.abs() < RELU_MARGIN
        if not bool(bad.any()):
            return P
        P = P + 0.01 * bad
    raise AssertionError("pre-activations stay on the ReLU edge")


def _r(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale + shift


@functools.lru_cache(maxsize=None)
def case32(E):
    """fp64 inputs of the 32-wide kernels at E edges, shared and never modified: cam / pt random
    indices into M_TAB / N_TAB rows, index 0 in the last row; pos a random permutation."""
    g = torch.Generator().manual_seed(7000 + E)
    c = types.SimpleNamespace(E=E, m=M_TAB, n=N_TAB)
    c.P, c.P0 = _r(g, E, 32, scale=1.5, shift=0.2), _r(g, E, 2)
    c.lnw, c.lnb = _r(g, 32, scale=0.3, shift=1), _r(g, 32, scale=0.2)
    if E <= 1000:
        c.lnb = off_relu_edge(c.P, c.lnw, c.lnb, EPS)
    else:
        c.P = _nudge_off_edge(c.P, c.lnw, c.lnb, EPS)
    c.W, c.b = _r(g, 64, 32, scale=1 / 6), _r(g, 64, scale=0.1)
    c.Wp, c.bp = _r(g, 32, 34, scale=0.2), _r(g, 32, scale=0.1)
    c.Sp, c.Sv, c.Sg = _r(g, N_TAB, 32), _r(g, M_TAB, 32), _r(g, 32)
    c.cam = torch.randint(0, M_TAB, (E,), generator=g)
    c.pt = torch.randint(0, N_TAB, (E,), generator=g)
    c.cam[-1] = c.pt[-1] = 0
    c.pos = torch.randperm(E, generator=g)
    c.dXL, c.dRes = _r(g, E, 64), _r(g, E, 32)
    return c


@functools.lru_cache(maxsize=None)
def pro_fwd_ref(E, ln):
    c = case32(E)
    return pro_ref(c.P, c.lnw if ln else None, c.lnb, c.W, c.b)


@functools.lru_cache(maxsize=None)
def epi_fwd_ref(E, with_p0):
    c = case32(E)
    Wp = c.Wp if with_p0 else c.Wp[:, :32]
    return epi_ref(c.P, c.P0 if with_p0 else None, c.cam, c.pt, c.lnw, c.lnb, Wp, c.bp, c.Sp, c.Sv, c.Sg)


@functools.lru_cache(maxsize=None)
def pro_bwd_ref(E, ln, res):
    c = case32(E)
    return pbwd_ref(c.P, c.lnw if ln else None, c.lnb, c.W, c.Wp, c.dXL, c.dRes if res else None)


def _camera_major(E, m, g):
    """Sorted camera ids of E edges over m cameras (camera 1 empty when m > 2): the order the camera
    items of edge_epilogue_bwd / edge0_epilogue_bwd index edges in."""
    cam = torch.randint(0, m, (E,), generator=g)
    if m > 2:
        cam[cam == 1] = 2
    return cam.sort().values


@functools.lru_cache(maxsize=None)
def fn_case(E, with_p0):
    """case32(E) on a camera-major graph with its plans (pieces of 16: split cameras from E = 65 on),
    and the fp64 gradients of every leaf of EdgePrologueFn + EdgeEpilogueFn by plain autograd."""
    c = case32(E)
    g = torch.Generator().manual_seed(7500 + E)
    f = types.SimpleNamespace(c=c, cam=_camera_major(E, M_TAB, g), pt=c.pt, G1=_r(g, E, 64), G2=_r(g, E, 32))
    f.plan_c = AttnPlan.from_targets(f.cam, M_TAB, max_piece=16)
    f.plan_p = AttnPlan.from_targets(f.pt, N_TAB, max_piece=16)
    f.names = ("P", "P0", "lnw", "lnb", "W", "b", "Wp", "bp", "Sp", "Sv", "Sg")
    f.leaves = dict(P=c.P, P0=c.P0 if with_p0 else None, lnw=c.lnw, lnb=c.lnb, W=c.W, b=c.b,
                    Wp=c.Wp if with_p0 else c.Wp[:, :32].contiguous(), bp=c.bp, Sp=c.Sp, Sv=c.Sv, Sg=c.Sg.view(1, 32))
    r = {k: v.clone().requires_grad_(True) for k, v in f.leaves.items() if v is not None}
    f.XL = pro_ref(r["P"], r["lnw"], r["lnb"], r["W"], r["b"])
    f.Pn = epi_ref(r["P"], r.get("P0"), f.cam, f.pt, r["lnw"], r["lnb"], r["Wp"], r["bp"], r["Sp"], r["Sv"], r["Sg"])
    ((f.XL * f.G1).sum() + (f.Pn * f.G2).sum()).backward()
    f.grads = {k: v.grad for k, v in r.items()}
    f.XL, f.Pn = f.XL.detach(), f.Pn.detach()
    return f


# block 0
E0_SEP = 3.0


def _p0_rows(g, E, equal_rows=False):
    """[E, 2] with |x0 - x1| >= E0_SEP (x_hat ~ +-1: the 2-wide LayerNorm well conditioned).  3 and not 0.1:
    the LayerNorm backward cancels to ~eps rstd^3 |g|, with an fp32 rounding of ~1e-7 rstd |g| left over;
    at a separation of 0.1 (rstd up to 20) fp32 torch itself misses the 1e-5 + 1e-4 |ref| bar of aux / dP
    by 7.8e-5 on hand_graph() and 8.6e-4 on stride_graph(), at 2 it passes, at 3 with room.  equal_rows:
    every 7th row x0 == x1 exactly (rstd = 1 / sqrt(eps))."""
    x0 = _r(g, E)
    d = _r(g, E)
    P = torch.stack([x0, x0 + torch.where(d >= 0, E0_SEP + d, -E0_SEP + d)], 1)
    if equal_rows:
        P[::7, 1] = P[::7, 0]
    return P


def e0_pro_ref(P, law, lab, W0, b0, eps=EPS):
    return _ln_relu(P, law, lab, eps) @ W0.T + b0


def e0_epi_ref(P, cam, pt, law, lab, lbw, lbb, Wp, bp, Wsk, bsk, Sp, Sv, Sg, eps=EPS):
    pa, pb = _ln_relu(P, law, lab, eps), _ln_relu(P, lbw, lbb, eps)
    return pb @ Wsk.T + bsk + PROJ_SCALE * (pa @ Wp.T + bp + Sp[pt] + Sv[cam] + Sg.reshape(-1))


@functools.lru_cache(maxsize=None)
def case0(E, equal_rows=False, m=M_TAB, n=N_TAB):
    """fp64 inputs of the block-0 kernels at E edges (cam / pt as case32)."""
    g = torch.Generator().manual_seed(8000 + E + 3 * equal_rows)
    c = types.SimpleNamespace(E=E, m=m, n=n)
    c.P = _p0_rows(g, E, equal_rows)
    c.law, c.lab, c.lbw, c.lbb = _r(g, 2, scale=0.1, shift=1), _r(g, 2, scale=0.1), _r(g, 2, scale=0.1, shift=1), \
        _r(g, 2, scale=0.1)
    if E <= 1000:
        c.lab, c.lbb = off_relu_edge(c.P, c.law, c.lab, EPS), off_relu_edge(c.P, c.lbw, c.lbb, EPS)
    c.W0, c.b0 = _r(g, 8, 2), _r(g, 8, scale=0.1)
    c.Wp, c.bp, c.Wsk, c.bsk = _r(g, 32, 2), _r(g, 32, scale=0.1), _r(g, 32, 2), _r(g, 32, scale=0.1)
    c.Sp, c.Sv, c.Sg = _r(g, n, 32), _r(g, m, 32), _r(g, 32)
    c.cam = torch.randint(0, m, (E,), generator=g)
    c.pt = torch.randint(0, n, (E,), generator=g)
    c.cam[-1] = c.pt[-1] = 0
    c.perm = torch.randperm(E, generator=g)
    c.pos = torch.empty(E, dtype=torch.int64)
    c.pos[c.perm] = torch.arange(E)
    c.dXL, c.dPo = _r(g, E, 8), _r(g, E, 32)
    return c


def e0_bwd_ref(c, cam, m):
    """fp64 results of edge0_epilogue_bwd + edge0_prologue_bwd on c's inputs with camera ids cam:
    aux = (scale Wp^T dP', LN_b branch's dP), dSv, the two partial rows' column blocks, dP."""
    lv = {k: getattr(c, k).clone().requires_grad_(True)
          for k in ("P", "law", "lab", "lbw", "lbb", "W0", "b0", "Wp", "Wsk", "bsk")}
    pa, pb = _ln_relu(lv["P"], lv["law"], lv["lab"], EPS), _ln_relu(lv["P"], lv["lbw"], lv["lbb"], EPS)
    XL = pa @ lv["W0"].T + lv["b0"]
    Pn = pb @ lv["Wsk"].T + lv["bsk"] + PROJ_SCALE * (pa @ lv["Wp"].T)
    ((XL * c.dXL).sum() + (Pn * c.dPo).sum()).backward()
    Pb = c.P.clone().requires_grad_(True)
    ((_ln_relu(Pb, c.lbw, c.lbb, EPS) @ c.Wsk.T) * c.dPo).sum().backward()
    r = {k: v.grad for k, v in lv.items()}
    r["aux"] = torch.cat([PROJ_SCALE * c.dPo @ c.Wp, Pb.grad], 1)
    r["dSv"] = torch.zeros(m, 32, dtype=torch.float64).index_add(0, cam, c.dPo) * PROJ_SCALE
    return r


def all_case_builders():
    """Every cached fp64 case of sections A and B, built (each asserts its ReLU margin); needs no GPU."""
    n = 0
    for E in SWEEP_E + [130]:
        case32(E), pro_fwd_ref(E, True), epi_fwd_ref(E, True), pro_bwd_ref(E, True, True)
        n += 1
    for E in FN_E:
        fn_case(E, True), fn_case(E, False)
    for E in sorted(set(E0_PRO_E + E0_EPI_E)):
        case0(E)
        n += 1
    return n


def test_references_match_autograd():
    """The closed-form pbwd_ref against plain autograd of pro_ref and the epilogue's Wp product, for the
    four <LN, RES> forms at E = 1, 17, 65, in fp64; and the builders run without a device."""
    for E in FN_E:
        c = case32(E)
        assert c.cam[-1] == 0 and c.pt[-1] == 0 and sorted(c.pos.tolist()) == list(range(E))
        for ln in (True, False):
            for res in (True, False):
                lv = {k: getattr(c, k).clone().requires_grad_(True) for k in ("P", "lnw", "lnb", "W", "b")}
                lnw = lv["lnw"] if ln else None
                loss = (pro_ref(lv["P"], lnw, lv["lnb"], lv["W"], lv["b"]) * c.dXL).sum()
                if res:
                    ph = _ln_relu(lv["P"], lnw, lv["lnb"], EPS) if ln else lv["P"]
                    loss = loss + ((lv["P"] + PROJ_SCALE * ph @ c.Wp[:, :32].T) * c.dRes).sum()
                loss.backward()
                ref = pro_bwd_ref(E, ln, res)
                pairs = [("dP", "P"), ("dW", "W"), ("db", "b")] + ([("dgamma", "lnw"), ("dbeta", "lnb")] if ln else [])
                for k, leaf in pairs:
                    torch.testing.assert_close(ref[k], lv[leaf].grad, rtol=1e-10, atol=1e-10, msg=f"{k} E={E}")
        f = fn_case(E, True)
        assert set(f.grads) == set(f.names) and f.plan_c.perm is None
        torch.testing.assert_close(f.XL, pro_fwd_ref(E, True), rtol=1e-12, atol=1e-12)
        c0 = case0(E)
        assert float((c0.P[:, 0] - c0.P[:, 1]).abs().min()) >= E0_SEP
        r0 = e0_bwd_ref(c0, c0.cam, c0.m)
        assert r0["aux"].shape == (E, 4) and r0["dSv"].shape == (c0.m, 32)
    big = _nudge_off_edge(_r(torch.Generator().manual_seed(1), 5000, 32), case32(1).lnw, case32(1).lnb, EPS)
    assert float(F.layer_norm(big, (32,), case32(1).lnw, case32(1).lnb, EPS).abs().min()) >= RELU_MARGIN


# ------------------------------------------------------------------------------ buffers
def _bits(t):
    return t.view(torch.int32)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


class Bufs:
    """The tensors of one kernel call.  Plain: exact-size, torch.empty outputs and partials (what
    production passes).  guard: every per-edge input is the first E rows of an (E + 16)-row buffer
    ending in NaN rows (index arrays: in ``tail``), every output rows GUARD .. GUARD+E-1 of a buffer
    holding SENTINEL, every partial pre-filled with ``fill`` and followed by two guard rows."""

    def __init__(self, dev, guard=False, fill=float("nan")):
        self.dev, self.guard, self.fill = dev, guard, fill
        self.outs, self.parts = {}, {}

    def rows(self, t, ld=None, tail=None):
        """Per-edge input [E, w] (row stride ld) or index array [E] (int32, ending in 16 x tail)."""
        if t.dim() == 1:
            t = t.int()
            if self.guard:
                return torch.cat([t, torch.full((TAIL,), tail, dtype=torch.int32)]).to(self.dev)[:t.numel()]
            return t.to(self.dev)
        E, w = t.shape
        big = torch.full((E + (TAIL if self.guard else 0), ld or w), float("nan"), device=self.dev)
        big[:E, :w] = t.float().to(self.dev)
        return big[:E, :w]

    def table(self, t, ld=None):
        """Node table [rows, 32] (row stride ld) with one NaN row behind it, which the index tails hit."""
        rows = t.shape[0]
        big = torch.full((rows + 1, ld or 32), float("nan"), device=self.dev)
        big[:rows, :32] = t.float().to(self.dev)
        return big[:rows, :32]

    def out(self, name, E, cols, ld=None):
        ld = ld or cols
        if self.guard:
            buf = _sentinel((E + 2 * GUARD, ld), self.dev)
            view = buf[GUARD:GUARD + E, :cols]
        else:
            buf = torch.empty((E, ld), device=self.dev)
            view = buf[:, :cols]
        self.outs[name] = (buf, view)
        return view

    def part(self, name, rows, cols):
        if self.guard:
            buf = torch.full((rows + PART_GUARD, cols), self.fill, device=self.dev)
            before = _bits(buf[rows:]).clone()
        else:
            buf, before = torch.empty((rows, cols), device=self.dev), None
        self.parts[name] = (buf, rows, before)
        return buf[:rows]

    def verify(self, unwritten=()):
        """Guards and pad columns keep the pattern, every live element was written and is finite.
        unwritten: outputs whose rows the call writes only in part (dSv of an item-less camera...)."""
        if not self.guard:
            return
        for name, (buf, view) in self.outs.items():
            E, cols = view.shape
            live = torch.zeros(buf.shape, dtype=torch.bool, device=self.dev)
            live[GUARD:GUARD + E, :cols] = True
            assert bool((_bits(buf)[~live] == SENTINEL).all()), f"{name}: written outside its {E} x {cols} rows"
            if name not in unwritten:
                assert not bool((_bits(view) == SENTINEL).any()), f"{name}: elements not written"
                assert bool(torch.isfinite(view).all()), f"{name}: not finite"
        for name, (buf, rows, before) in self.parts.items():
            assert torch.equal(_bits(buf[rows:]), before), f"{name}: written past row {rows}"


def _dev(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


def close(got, ref, msg=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.numpy(), atol=1e-5, rtol=1e-4, err_msg=msg)


def close_node(got, ref, msg=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.numpy(), atol=1e-4, rtol=1e-4, err_msg=msg)


# ------------------------------------------------------------------------------ kernel runners
def run_pro_fwd(dev, c, ln=True, with_pos=False, split=False, ld=64, b=None):
    """gasfm_edge_prologue_fwd; returns Y [E, 64] as written (point half at row pos[e] with pos)."""
    b = b or Bufs(dev)
    W, bias = _dev(c.W, dev), _dev(c.b, dev)
    Y = b.out("Y", c.E, 64, ld)
    _native.edge_prologue_fwd(b.rows(c.P), _dev(c.lnw, dev) if ln else None, _dev(c.lnb, dev) if ln else None, EPS,
                              W[:32] if split else W, bias[:32] if split else bias, Y,
                              b.rows(c.pos, tail=c.E) if with_pos else None,
                              W[32:] if split else None, bias[32:] if split else None)
    b.verify()
    return dict(Y=Y)


def run_epi_fwd(dev, c, with_p0=True, strided=False, b=None):
    b = b or Bufs(dev)
    Wp = _dev(c.Wp if with_p0 else c.Wp[:, :32], dev)
    out = b.out("Pn", c.E, 32)
    Sv = b.table(c.Sv, 64 if strided else None)
    assert Sv.stride(0) == (64 if strided else 32)
    _native.edge_epilogue_fwd(b.rows(c.P), b.rows(c.P0) if with_p0 else None, b.rows(c.cam, tail=c.m),
                              b.rows(c.pt, tail=c.n), _dev(c.lnw, dev), _dev(c.lnb, dev), EPS, Wp, _dev(c.bp, dev),
                              b.table(c.Sp), Sv, _dev(c.Sg, dev), PROJ_SCALE, out)
    b.verify()
    return dict(Pn=out)


def run_pro_bwd(dev, c, ln=True, res=True, split=False, dxl="whole", wp_cols=34, b=None):
    """gasfm_edge_prologue_bwd; dxl: "whole" [E, 64], or the point half plus dXLc with ldC = 32 ("c32") or
    64 ("c64").  Returns dP and the column sums of the partial rows."""
    b = b or Bufs(dev)
    E = c.E
    W = _dev(c.W, dev)
    if dxl == "whole":
        dXL, dXLc = b.rows(c.dXL), None
    else:
        dXL, dXLc = b.rows(c.dXL[:, :32]), b.rows(c.dXL[:, 32:], ld=32 if dxl == "c32" else 64)
        assert dXL.stride(0) == 32 and dXLc.stride(0) == (32 if dxl == "c32" else 64)
    rows = _native.edge_part_floats(0, E) // NPART
    assert 1 <= rows <= -(-E // 64)
    part = b.part("part", rows, NPART)
    dP = b.out("dP", E, 32)
    Wp = _dev(c.Wp if wp_cols == 34 else c.Wp[:, :32], dev) if res else None
    _native.edge_prologue_bwd(dXL, b.rows(c.P), b.rows(c.dRes) if res else None, _dev(c.lnw, dev) if ln else None,
                              _dev(c.lnb, dev) if ln else None, EPS, W[:32] if split else W, Wp, PROJ_SCALE, dP, part,
                              W[32:] if split else None, dXLc=dXLc)
    b.verify()
    return dict(dP=dP, tot=_native.colsum(part))


def check_pro_bwd(res, ref, E, msg):
    tot = res["tot"]
    close(res["dP"], ref["dP"], f"dP {msg}")
    lo = 16 * ((E - 1) // 16)
    close(res["dP"][lo:], ref["dP"][lo:], f"dP rows {lo}..{E - 1} {msg}")
    for k, a in (("dW", tot[:2048].view(64, 32)), ("db", tot[2048:2112]), ("dgamma", tot[2112:2144]),
                 ("dbeta", tot[2144:])):
        assert bool(torch.isfinite(a).all()), f"{k} {msg}"
        normwise(a, ref[k], msg=f"{k} {msg}")


def _item_graph(E, seed):
    g = torch.Generator().manual_seed(seed)
    cam = _camera_major(E, M_TAB, g)
    return cam, AttnPlan.from_targets(cam, M_TAB, max_piece=16)


def run_epi_bwd(dev, c, cam, plan, with_p0=True, b=None):
    """gasfm_edge_epilogue_bwd on the camera items of plan; returns dSv (combined), dP0, dWp."""
    b = b or Bufs(dev)
    pc = plan.to(dev)
    Wp = _dev(c.Wp if with_p0 else c.Wp[:, :32], dev)
    dSv = b.out("dSv", pc.num_targets, 32)
    dP0 = b.out("dP0", c.E, 2) if with_p0 else None
    part_dsv = b.part("part_dsv", max(pc.n_part_rows, 1), 32)
    wg = _native.edge_part_floats(1, c.E, pc.n_items) // (32 * 34)
    part_w = b.part("part_w", wg, 32 * Wp.shape[1])
    _native.edge_epilogue_bwd(pc.items, pc.n_items, b.rows(c.dRes), b.rows(c.P), b.rows(c.P0) if with_p0 else None,
                              _dev(c.lnw, dev), _dev(c.lnb, dev), EPS, Wp, PROJ_SCALE, dSv, part_dsv, dP0, part_w)
    split = set(pc.combine[:, 0].tolist()) if pc.n_combine else set()
    b.verify(unwritten=("dSv",) if split else ())
    bwd_combine(pc, part_dsv, 32, dSv)
    assert bool(torch.isfinite(dSv).all()), "dSv not finite"
    res = dict(dSv=dSv.clone(), dWp=_native.colsum(part_w).view(32, -1))
    if with_p0:
        res["dP0"] = dP0
    return res


def epi_bwd_ref(c, cam, m, with_p0):
    ph = _ln_relu(c.P, c.lnw, c.lnb, EPS)
    d = PROJ_SCALE * c.dRes
    x = torch.cat([ph, c.P0], 1) if with_p0 else ph
    return dict(dSv=torch.zeros(m, 32, dtype=torch.float64).index_add(0, cam, d), dWp=d.T @ x, dP0=d @ c.Wp[:, 32:])


def run_rowsum(dev, X, plan, ld=32, b=None):
    """gasfm_segment_rowsum of X [E, 32] (row stride ld) over plan, combined; part None without slots."""
    b = b or Bufs(dev)
    pp = plan.to(dev)
    out = b.out("dSp", pp.num_targets, 32)
    part = b.part("part_dsp", pp.n_part_rows, 32) if pp.n_slots else None
    _native.segment_rowsum(pp.items, pp.n_items, pp.perm, b.rows(X, ld=ld), PROJ_SCALE, out, part)
    b.verify(unwritten=("dSp",) if pp.n_combine else ())
    if part is not None:
        bwd_combine(pp, part, 32, out)
    assert bool(torch.isfinite(out).all()), "dSp not finite"
    return dict(dSp=out.clone())


def _e0_params(c, dev, *names):
    return [_dev(getattr(c, k), dev) for k in names]


def run_e0_pro_fwd(dev, c, form="pos", b=None):
    """form: "plain" (no pos), "pos" (gasfm_edge0_prologue_fwd scattering through pos), "rows" (_fwd_rows)."""
    b = b or Bufs(dev)
    XL = b.out("XL0", c.E, 8)
    args = (b.rows(c.P), *_e0_params(c, dev, "law", "lab"), EPS, *_e0_params(c, dev, "W0", "b0"), XL)
    if form == "rows":
        _native.edge0_prologue_fwd_rows(*args, b.rows(c.perm, tail=c.E))
    else:
        _native.edge0_prologue_fwd(*args, b.rows(c.pos, tail=c.E) if form == "pos" else None)
    b.verify()
    return dict(XL0=XL)


def run_e0_epi_fwd(dev, c, strided=False, b=None):
    b = b or Bufs(dev)
    out = b.out("Pn", c.E, 32)
    _native.edge0_epilogue_fwd(b.rows(c.P), b.rows(c.cam, tail=c.m), b.rows(c.pt, tail=c.n),
                               *_e0_params(c, dev, "law", "lab", "lbw", "lbb"), EPS,
                               *_e0_params(c, dev, "Wp", "bp", "Wsk", "bsk"), b.table(c.Sp),
                               b.table(c.Sv, 64 if strided else None), _dev(c.Sg, dev), PROJ_SCALE, out)
    b.verify()
    return dict(Pn=out)


def run_e0_epi_bwd(dev, c, plan, b=None):
    """gasfm_edge0_epilogue_bwd; returns aux, dSv (combined) and the partial rows' column sums."""
    b = b or Bufs(dev)
    pc = plan.to(dev)
    dSv = b.out("dSv", pc.num_targets, 32)
    aux = b.out("aux", c.E, 4)
    part_dsv = b.part("part_dsv", max(pc.n_part_rows, 1), 32)
    part = b.part("part", _native.edge0_part_rows(1, c.E, pc.n_items), 164)
    _native.edge0_epilogue_bwd(pc.items, pc.n_items, b.rows(c.dPo), b.rows(c.P),
                               *_e0_params(c, dev, "law", "lab", "lbw", "lbb"), EPS, *_e0_params(c, dev, "Wp", "Wsk"),
                               PROJ_SCALE, dSv, part_dsv, aux, part)
    b.verify(unwritten=("dSv",) if pc.n_combine else ())
    bwd_combine(pc, part_dsv, 32, dSv)
    assert bool(torch.isfinite(dSv).all()), "dSv not finite"
    return dict(aux=aux, dSv=dSv.clone(), tot=_native.colsum(part))


def run_e0_pro_bwd(dev, c, aux, b=None):
    """gasfm_edge0_prologue_bwd (aux: fp64 [E, 4] or None); returns dP and the partial rows' column sums."""
    b = b or Bufs(dev)
    dP = b.out("dP", c.E, 2)
    part = b.part("part", _native.edge0_part_rows(0, c.E), 28)
    _native.edge0_prologue_bwd(b.rows(c.dXL), b.rows(c.P), b.rows(aux) if aux is not None else None,
                               *_e0_params(c, dev, "law", "lab"), EPS, _dev(c.W0, dev), dP, part)
    b.verify()
    return dict(dP=dP, tot=_native.colsum(part))


def check_e0_bwd(epi, pro, ref, msg):
    close(epi["aux"], ref["aux"], f"aux {msg}")
    close_node(epi["dSv"], ref["dSv"], f"dSv {msg}")
    t = epi["tot"]
    for k, a in (("Wp", t[:64].view(32, 2)), ("Wsk", t[64:128].view(32, 2)), ("bsk", t[128:160]), ("lbw", t[160:162]),
                 ("lbb", t[162:164])):
        normwise(a, ref[k], msg=f"d{k} {msg}")
    close(pro["dP"], ref["P"], f"dP {msg}")
    t = pro["tot"]
    for k, a in (("W0", t[:16].view(8, 2)), ("b0", t[16:24]), ("law", t[24:26]), ("lab", t[26:28])):
        normwise(a, ref[k], msg=f"d{k} {msg}")


# ------------------------------------------------------------------------------ A. remainder sweep (32-wide)
@gpu
@pytest.mark.parametrize("E", SWEEP_E)
def test_a_prologue_fwd_sweep(device, E):
    c = case32(E)
    pos = c.pos.to(device)
    for ln in (True, False):
        ref = pro_fwd_ref(E, ln)
        for with_pos in (False, True):
            for split in (False, True):
                for ld in (64, 72):
                    Y = run_pro_fwd(device, c, ln, with_pos, split, ld)["Y"]
                    msg = f"E={E} ln={ln} pos={with_pos} split={split} ldY={ld}"
                    close(Y[pos, :32] if with_pos else Y[:, :32], ref[:, :32], "point half " + msg)
                    close(Y[:, 32:], ref[:, 32:], "camera half " + msg)


@gpu
@pytest.mark.parametrize("E", SWEEP_E)
def test_a_epilogue_fwd_sweep(device, E):
    c = case32(E)
    for with_p0 in (True, False):
        for strided in (False, True):
            out = run_epi_fwd(device, c, with_p0, strided)["Pn"]
            close(out, epi_fwd_ref(E, with_p0), f"E={E} p0={with_p0} strided Sv={strided}")


@gpu
@pytest.mark.parametrize("E", SWEEP_E)
def test_a_prologue_bwd_production_sweep(device, E):
    """LN + RES + split W + dXLc (ldC = 32) + Wp [32, 34]: what EdgeCamFn's item-less backward passes."""
    res = run_pro_bwd(device, case32(E), True, True, True, "c32", 34)
    check_pro_bwd(res, pro_bwd_ref(E, True, True), E, f"E={E}")


@gpu
@pytest.mark.parametrize("E", CROSS_E)
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("res", [True, False])
def test_a_prologue_bwd_cross(device, E, ln, res):
    c, ref = case32(E), pro_bwd_ref(E, ln, res)
    for split in (False, True):
        for dxl in ("whole", "c32", "c64"):
            for wp_cols in ((34, 32) if res else (34,)):
                got = run_pro_bwd(device, c, ln, res, split, dxl, wp_cols)
                check_pro_bwd(got, ref, E, f"E={E} ln={ln} res={res} split={split} dXL={dxl} Wp cols={wp_cols}")
                if not ln:
                    assert int(torch.count_nonzero(got["tot"][2112:])) == 0, "dgamma / dbeta without LayerNorm"


@gpu
@pytest.mark.parametrize("E", FN_E)
@pytest.mark.parametrize("with_p0", [True, False])
def test_a_functions(device, E, with_p0):
    """EdgePrologueFn + EdgeEpilogueFn: the gradient of every leaf."""
    from gasfm_amd.model import EdgeIndex
    f = fn_case(E, with_p0)
    plans = {"proj2view": f.plan_c.to(device), "proj2scenepoint": f.plan_p.to(device)}
    edges = EdgeIndex(f.cam.int().to(device), f.pt.int().to(device), M_TAB, N_TAB, plans)
    d = {k: v.float().to(device).requires_grad_(True) for k, v in f.leaves.items() if v is not None}
    XL, tok = EdgePrologueFn.apply(d["P"], d["lnw"], d["lnb"], d["W"], d["b"], d["Wp"], EPS)
    Pn = EdgeEpilogueFn.apply(d["P"], d.get("P0"), tok, d["Sp"], d["Sv"], d["Sg"], d["Wp"], d["bp"], d["lnw"],
                              d["lnb"], EPS, edges)
    ((XL * f.G1.float().to(device)).sum() + (Pn * f.G2.float().to(device)).sum()).backward()
    close(XL, f.XL, "XL")
    close(Pn, f.Pn, "P'")
    for k in d:
        assert d[k].grad is not None and bool(torch.isfinite(d[k].grad).all()), k
        if k in ("P", "P0"):
            close(d[k].grad, f.grads[k], f"d{k}")
        elif k in ("Sp", "Sv"):
            close_node(d[k].grad, f.grads[k], f"d{k}")
        else:
            normwise(d[k].grad, f.grads[k], msg=f"d{k}")


# ------------------------------------------------------------------------------ B. block 0, segment_rowsum
@gpu
@pytest.mark.parametrize("E", E0_PRO_E)
def test_b_edge0_prologue_fwd(device, E):
    c = case0(E)
    h = e0_pro_ref(c.P, c.law, c.lab, c.W0, c.b0)
    plain = run_e0_pro_fwd(device, c, "plain")["XL0"]
    close(plain, h, f"E={E} without pos")
    scat, rows = run_e0_pro_fwd(device, c, "pos")["XL0"], run_e0_pro_fwd(device, c, "rows")["XL0"]
    close(rows, torch.cat([h[c.perm, :4], h[:, 4:]], 1), f"E={E} rows")
    assert torch.equal(scat, rows), "scatter and row forms differ"
    p = [_dev(t, device) for t in (c.P, c.law, c.lab, c.W0, c.b0)]
    XL_f, _ = Block0PrologueFn.apply(*p, EPS, c.pos.int().to(device), c.perm.int().to(device))
    assert torch.equal(XL_f, rows), "Block0PrologueFn differs"
    XL_f, _ = Block0PrologueFn.apply(*p, EPS)
    assert torch.equal(XL_f, plain)


@gpu
@pytest.mark.parametrize("E", E0_EPI_E)
def test_b_edge0_epilogue_fwd(device, E):
    c = case0(E)
    ref = e0_epi_ref(c.P, c.cam, c.pt, c.law, c.lab, c.lbw, c.lbb, c.Wp, c.bp, c.Wsk, c.bsk, c.Sp, c.Sv, c.Sg)
    for strided in (False, True):
        close(run_e0_epi_fwd(device, c, strided)["Pn"], ref, f"E={E} strided Sv={strided}")


@gpu
def test_b_edge0_equal_rows(device):
    """x0 == x1 rows (rstd = 1 / sqrt(eps)) through both block-0 forwards, at the close32 bound."""
    c = case0(65, True)
    args_p = (c.P, c.law, c.lab, c.W0, c.b0)
    args_e = (c.P, c.cam, c.pt, c.law, c.lab, c.lbw, c.lbb, c.Wp, c.bp, c.Wsk, c.bsk, c.Sp, c.Sv, c.Sg)
    f32 = lambda ts: [t.float() if t.is_floating_point() else t for t in ts]  # noqa: E731
    close32(run_e0_pro_fwd(device, c, "plain")["XL0"], e0_pro_ref(*args_p), e0_pro_ref(*f32(args_p)), "XL0")
    close32(run_e0_epi_fwd(device, c)["Pn"], e0_epi_ref(*args_e), e0_epi_ref(*f32(args_e)), "P'")


@functools.lru_cache(maxsize=None)
def _e0_item_case(gname, max_piece):
    """(case0 inputs, camera ids, camera plan, fp64 results) on hand_graph() or the (1, 0, 9) graph."""
    if gname == "hand":
        g = hand_graph()
        cam, m, plan = g.cam, g.m, cam_plan("hand", max_piece)
    else:
        cam, m = torch.tensor([0] + [2] * 9), 3
        plan = AttnPlan.from_targets(cam, m, max_piece=max_piece)
    c = case0(int(cam.numel()), False, m, N_TAB)
    return c, cam, plan, e0_bwd_ref(c, cam, m)


@gpu
@pytest.mark.parametrize("gname,max_piece", [("hand", p) for p in PIECES] + [("deg109", 4096)])
def test_b_edge0_bwd_items(device, gname, max_piece):
    c, cam, plan, ref = _e0_item_case(gname, max_piece)
    epi = run_e0_epi_bwd(device, c, plan)
    pro = run_e0_pro_bwd(device, c, epi["aux"].double().cpu())
    check_e0_bwd(epi, pro, ref, f"{gname} max_piece={max_piece}")


@gpu
@pytest.mark.parametrize("gname,max_piece", [("hand", p) for p in PIECES])
@pytest.mark.parametrize("with_p0", [True, False])
def test_b_epilogue_bwd_items(device, gname, max_piece, with_p0):
    """gasfm_edge_epilogue_bwd on hand_graph()'s camera items: dSv, dP0 and dWp (P0 None: Wp [32, 32])."""
    g = hand_graph()
    c = case32(g.E)
    got = run_epi_bwd(device, c, g.cam, cam_plan("hand", max_piece), with_p0)
    ref = epi_bwd_ref(c, g.cam, g.m, with_p0)
    close_node(got["dSv"], ref["dSv"], "dSv")
    normwise(got["dWp"], ref["dWp"], msg="dWp")
    if with_p0:
        close(got["dP0"], ref["dP0"], "dP0")


LENS = [0, 1, 31, 32, 33, 64, 65, 200, 0, 3]


@functools.lru_cache(maxsize=None)
def _rowsum_case(kind):
    """(X fp64 [E, 32], targets, plan) of a segment_rowsum variant."""
    rng = np.random.default_rng(2)
    if kind in ("lens", "lens-sorted", "lens-noslots"):
        dst = np.repeat(np.arange(len(LENS)), LENS)
        if kind == "lens":
            dst = rng.permutation(dst)
        n, piece = len(LENS), (16 if kind != "lens-noslots" else 4096)
    else:  # 9000 segments of c % 5 rows: more items than resident waves, two-deep item pipeline wraps
        dst, n, piece = stride_graph().cam.numpy(), 9000, 4096
        if kind == "9000-perm":
            dst = rng.permutation(dst)
    dst = torch.from_numpy(np.ascontiguousarray(dst))
    plan = AttnPlan.from_targets(dst, n, max_piece=piece)
    X = _r(torch.Generator().manual_seed(len(kind)), dst.numel(), 32)
    return X, dst, plan


def _rowsum_ref(X, dst, n):
    return torch.zeros(n, 32, dtype=torch.float64).index_add(0, dst, X) * PROJ_SCALE


@gpu
@pytest.mark.parametrize("kind", ["lens", "lens-sorted", "lens-noslots", "9000-sorted", "9000-perm"])
@pytest.mark.parametrize("ld", [32, 40])
def test_b_segment_rowsum(device, kind, ld):
    X, dst, plan = _rowsum_case(kind)
    assert (plan.perm is None) == (kind in ("lens-sorted", "lens-noslots", "9000-sorted"))
    assert (plan.n_slots == 0) == (kind not in ("lens", "lens-sorted"))
    if kind.startswith("9000"):
        assert plan.n_items > 8192  # an MI355X holds at most 256 CUs x 32 waves
    got = run_rowsum(device, X, plan, ld)["dSp"]
    close(got, _rowsum_ref(X, dst, plan.num_targets), kind)


# ------------------------------------------------------------------------------ C. guards, poison, loops
def _c_pro_fwd(dev, E, b):
    return run_pro_fwd(dev, case32(E), True, True, True, 72, b)


def _c_pro_fwd_plain(dev, E, b):
    return run_pro_fwd(dev, case32(E), False, False, False, 64, b)


def _c_epi_fwd(dev, E, b):
    return run_epi_fwd(dev, case32(E), True, True, b)


def _c_epi_fwd_nop0(dev, E, b):
    return run_epi_fwd(dev, case32(E), False, False, b)


def _c_pro_bwd(dev, E, b):
    return run_pro_bwd(dev, case32(E), True, True, True, "c64", 34, b)


def _c_pro_bwd_plain(dev, E, b):
    return run_pro_bwd(dev, case32(E), False, False, False, "whole", 34, b)


def _c_epi_bwd(dev, E, b, with_p0=True):
    cam, plan = _item_graph(E, 9100 + E)
    return run_epi_bwd(dev, case32(E), cam, plan, with_p0, b)


def _c_epi_bwd_nop0(dev, E, b):
    return _c_epi_bwd(dev, E, b, False)


def _c_rowsum(dev, E, b):
    c = case32(E)
    return run_rowsum(dev, c.dRes, AttnPlan.from_targets(c.pt, N_TAB, max_piece=16), 40, b)


def _c_e0_pro_fwd(dev, E, b):
    return run_e0_pro_fwd(dev, case0(E), "pos", b)


def _c_e0_pro_fwd_rows(dev, E, b):
    return run_e0_pro_fwd(dev, case0(E), "rows", b)


def _c_e0_epi_fwd(dev, E, b):
    return run_e0_epi_fwd(dev, case0(E), True, b)


def _c_e0_epi_bwd(dev, E, b):
    return run_e0_epi_bwd(dev, case0(E), _item_graph(E, 9200 + E)[1], b)


def _c_e0_pro_bwd(dev, E, b):
    c = case0(E)
    return run_e0_pro_bwd(dev, c, _r(torch.Generator().manual_seed(E), E, 4), b)


KERNELS = {"prologue_fwd": _c_pro_fwd, "prologue_fwd-plain": _c_pro_fwd_plain, "epilogue_fwd": _c_epi_fwd,
           "epilogue_fwd-nop0": _c_epi_fwd_nop0, "epilogue_bwd": _c_epi_bwd, "epilogue_bwd-nop0": _c_epi_bwd_nop0,
           "prologue_bwd": _c_pro_bwd, "prologue_bwd-plain": _c_pro_bwd_plain, "segment_rowsum": _c_rowsum,
           "edge0_prologue_fwd": _c_e0_pro_fwd, "edge0_prologue_fwd_rows": _c_e0_pro_fwd_rows,
           "edge0_epilogue_fwd": _c_e0_epi_fwd, "edge0_epilogue_bwd": _c_e0_epi_bwd,
           "edge0_prologue_bwd": _c_e0_pro_bwd}


def _guarded_equals_plain(run, dev, E):
    """Three guarded calls with the partials holding NaN, 1e30, NaN, then the plain exact-size call: every
    result bitwise the same and finite.  Returns the results."""
    first = None
    for fill in (float("nan"), 1e30, float("nan"), None):
        res = run(dev, E, Bufs(dev, fill is not None, fill))
        res = {k: v.clone() for k, v in res.items()}
        first = first or res
        for k, v in res.items():
            assert bool(torch.isfinite(v).all()), f"{k} not finite (partials held {fill})"
            assert torch.equal(_bits(v), _bits(first[k])), \
                f"{k}: " + ("differs from the exact-size run" if fill is None else "depends on what its buffers held")
    return first


@gpu
@pytest.mark.parametrize("E", KERNEL_E)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_c_guarded_poisoned(device, kernel, E):
    _guarded_equals_plain(KERNELS[kernel], device, E)


@gpu
def test_c_loop_prologue_fwd(device):
    E = BIG_E
    Y = _guarded_equals_plain(_c_pro_fwd, device, E)["Y"]
    ref, pos = pro_fwd_ref(E, True), case32(E).pos.to(device)
    close(Y[pos, :32], ref[:, :32], "point half")
    close(Y[:, 32:], ref[:, 32:], "camera half")


@gpu
def test_c_loop_epilogue_fwd(device):
    close(_guarded_equals_plain(_c_epi_fwd, device, BIG_E)["Pn"], epi_fwd_ref(BIG_E, True))


@gpu
def test_c_loop_prologue_bwd(device):
    got = _guarded_equals_plain(_c_pro_bwd, device, BIG_E)
    check_pro_bwd(got, pro_bwd_ref(BIG_E, True, True), BIG_E, f"E={BIG_E}")


@gpu
@pytest.mark.parametrize("with_p0", [True, False])
def test_c_loop_epilogue_bwd(device, with_p0):
    """stride_graph(): 9000 camera items, one in five empty."""
    g = stride_graph()
    c = case32(g.E)
    got = _guarded_equals_plain(lambda dev, E, b: run_epi_bwd(dev, c, g.cam, cam_plan("stride", 4096), with_p0, b),
                                device, g.E)
    ref = epi_bwd_ref(c, g.cam, g.m, with_p0)
    close_node(got["dSv"], ref["dSv"], "dSv")
    normwise(got["dWp"], ref["dWp"], msg="dWp")
    if with_p0:
        close(got["dP0"], ref["dP0"], "dP0")


@gpu
def test_c_loop_segment_rowsum(device):
    X, dst, plan = _rowsum_case("9000-perm")
    got = _guarded_equals_plain(lambda dev, E, b: run_rowsum(dev, X, plan, 40, b), device, X.shape[0])
    close(got["dSp"], _rowsum_ref(X, dst, 9000))


@gpu
def test_c_loop_edge0_prologue(device):
    """270 001 edges: more than kMaxGrid workgroups of 256, forward (both forms) and backward."""
    E = BIG_E0_PRO
    c = case0(E)
    h = e0_pro_ref(c.P, c.law, c.lab, c.W0, c.b0)
    rows = _guarded_equals_plain(_c_e0_pro_fwd_rows, device, E)["XL0"]
    close(rows, torch.cat([h[c.perm, :4], h[:, 4:]], 1))
    assert torch.equal(_guarded_equals_plain(_c_e0_pro_fwd, device, E)["XL0"], rows)
    aux = _r(torch.Generator().manual_seed(E), E, 4)
    got = _guarded_equals_plain(_c_e0_pro_bwd, device, E)
    lv = {k: getattr(c, k).clone().requires_grad_(True) for k in ("P", "law", "lab", "W0", "b0")}
    pa = _ln_relu(lv["P"], lv["law"], lv["lab"], EPS)
    (((pa @ lv["W0"].T + lv["b0"]) * c.dXL).sum() + (pa * aux[:, :2]).sum()).backward()
    close(got["dP"], lv["P"].grad + aux[:, 2:], "dP")
    t = got["tot"]
    for k, a in (("W0", t[:16].view(8, 2)), ("b0", t[16:24]), ("law", t[24:26]), ("lab", t[26:28])):
        normwise(a, lv[k].grad, msg=f"d{k}")


@gpu
def test_c_loop_edge0_epilogue(device):
    """40 001 edges: more than kMaxGrid workgroups of 32 (forward); stride_graph()'s 9000 items (backward)."""
    E = BIG_E0_EPI
    c = case0(E)
    ref = e0_epi_ref(c.P, c.cam, c.pt, c.law, c.lab, c.lbw, c.lbb, c.Wp, c.bp, c.Wsk, c.bsk, c.Sp, c.Sv, c.Sg)
    close(_guarded_equals_plain(_c_e0_epi_fwd, device, E)["Pn"], ref)
    g = stride_graph()
    c = case0(g.E, False, g.m, N_TAB)
    epi = _guarded_equals_plain(lambda dev, E, b: run_e0_epi_bwd(dev, c, cam_plan("stride", 4096), b), device, g.E)
    pro = run_e0_pro_bwd(device, c, epi["aux"].double().cpu())
    check_e0_bwd(epi, pro, e0_bwd_ref(c, g.cam, g.m), "stride graph")


# ------------------------------------------------------------------------------ D. contracts
def _misaligned(t, dev):
    """t's values, contiguous, starting 4 bytes into their buffer."""
    flat = torch.zeros(t.numel() + 4, device=dev)
    v = flat.as_strided(tuple(t.shape), tuple(t.contiguous().stride()), 1)
    v.copy_(t.float().to(dev))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@gpu
@pytest.mark.parametrize("E", [21, 65])
def test_d_refusals(device, E):
    """Each violation raises before any launch: no output or partial of the call changes.  Buffers are
    sized so that a launch, were the refusal missing, would stay inside them."""
    dev, c = device, case32(E)
    P, P0, dXL, dRes = (_dev(t, dev) for t in (c.P, c.P0, c.dXL, c.dRes))
    lnw, lnb, W, bias, Wp34, bp = (_dev(t, dev) for t in (c.lnw, c.lnb, c.W, c.b, c.Wp, c.bp))
    Wp32 = _dev(c.Wp[:, :32], dev)
    Sp, Sv, Sg = (_dev(t, dev) for t in (c.Sp, c.Sv, c.Sg))
    cam, pt = c.cam.int().to(dev), c.pt.int().to(dev)
    _, plan = _item_graph(E, 9100 + E)
    plan = plan.to(dev)
    outs = {k: _sentinel((E + TAIL, w), dev) for k, w in (("Y", 72), ("Pn", 32), ("dP", 32), ("dP0", 2), ("dSv", 32),
                                                          ("dSp", 32))}
    parts = {k: _sentinel(shape, dev) for k, shape in (("part", (-(-E // 64) + 1, NPART)), ("part_w", (8, 32 * 34)),
                                                       ("part_dsv", (64, 32)))}
    Y, Pn, dP, dP0 = outs["Y"][:E, :64], outs["Pn"][:E], outs["dP"][:E], outs["dP0"][:E]
    pro_fwd = lambda **kw: _native.edge_prologue_fwd(**dict(dict(  # noqa: E731
        P=P, ln_w=lnw, ln_b=lnb, eps=EPS, W=W, b=bias, Y=Y, pos=None, W2=None, b2=None), **kw))
    epi_fwd = lambda **kw: _native.edge_epilogue_fwd(**dict(dict(  # noqa: E731
        P=P, P0=P0, cam=cam, pt=pt, ln_w=lnw, ln_b=lnb, eps=EPS, Wp=Wp34, bp=bp, Sp=Sp, Sv=Sv, Sg=Sg, scale=PROJ_SCALE,
        out=Pn), **kw))
    epi_bwd = lambda **kw: _native.edge_epilogue_bwd(**dict(dict(  # noqa: E731
        items=plan.items, n_items=plan.n_items, dPo=dRes, P=P, P0=P0, ln_w=lnw, ln_b=lnb, eps=EPS, Wp=Wp34,
        scale=PROJ_SCALE, dSv=outs["dSv"][:M_TAB], part_dsv=parts["part_dsv"], dP0=dP0, part_w=parts["part_w"]), **kw))
    pro_bwd = lambda **kw: _native.edge_prologue_bwd(**dict(dict(  # noqa: E731
        dXL=dXL, P=P, dRes=dRes, ln_w=lnw, ln_b=lnb, eps=EPS, W=W, Wp=Wp34, scale=PROJ_SCALE, dP=dP,
        part=parts["part"], W2=None, dXLc=None), **kw))
    y_flat = outs["Y"].view(-1)
    refused = [
        ("ldY", lambda: pro_fwd(Y=y_flat.as_strided((E, 64), (60, 1)))),
        ("ldY", lambda: pro_fwd(Y=y_flat.as_strided((E, 64), (66, 1)))),
        ("aligned", lambda: pro_fwd(P=_misaligned(c.P, dev))),
        ("bad args", lambda: pro_fwd(W=W[:32], b=bias[:32], W2=W[32:])),
        ("bad args", lambda: pro_fwd(W=W[:32], b=bias[:32], b2=bias[32:])),
        ("aligned", lambda: epi_fwd(P=_misaligned(c.P, dev))),
        ("ldWp", lambda: epi_fwd(Wp=Wp32)),
        ("ldWp", lambda: epi_fwd(P0=None)),
        ("aligned", lambda: epi_bwd(P=_misaligned(c.P, dev))),
        ("aligned", lambda: epi_bwd(dPo=_misaligned(c.dRes, dev))),
        ("ldWp", lambda: epi_bwd(Wp=Wp32)),
        ("ldWp", lambda: epi_bwd(P0=None, dP0=None)),
        ("aligned", lambda: pro_bwd(P=_misaligned(c.P, dev))),
        ("aligned", lambda: pro_bwd(dRes=_misaligned(c.dRes, dev))),
        ("dRes needs Wp", lambda: pro_bwd(Wp=None)),
        ("dXLc", lambda: pro_bwd(dXL=dXL[:, :32].contiguous(), dXLc=dXL.view(-1).as_strided((E, 32), (30, 1), 32))),
        ("alignment", lambda: _native.segment_rowsum(plan.items, plan.n_items, None, _misaligned(c.dRes, dev),
                                                     PROJ_SCALE, outs["dSp"][:M_TAB], parts["part_dsv"])),
    ]
    for match, call in refused:
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + list(parts.items()):
        assert bool((_bits(t) == SENTINEL).all()), f"{k} written by a refused call"


@gpu
def test_d_empty(device):
    """E = 0 / n_items = 0: every entry point returns OK before it looks at a pointer (none is passed), and
    the four Functions give empty outputs and zero gradients."""
    import ctypes
    from gasfm_amd.model import EdgeIndex
    L, nul, eps, sc = _native.lib(), None, ctypes.c_float(EPS), ctypes.c_float(PROJ_SCALE)
    before = L.gasfm_last_error()
    assert L.gasfm_edge_prologue_fwd(nul, 0, nul, nul, eps, *[nul] * 5, 64, nul, nul) == 0
    assert L.gasfm_edge_epilogue_fwd(*[nul] * 4, 0, nul, nul, eps, nul, 34, *[nul] * 3, 32, nul, sc, nul, nul) == 0
    assert L.gasfm_edge_epilogue_bwd(nul, 0, *[nul] * 5, eps, nul, 34, sc, *[nul] * 5) == 0
    assert L.gasfm_edge_prologue_bwd(nul, 64, nul, nul, 0, nul, nul, eps, nul, nul, nul, 34, sc, *[nul] * 3, 0, nul) == 0
    assert L.gasfm_segment_rowsum(nul, 0, nul, nul, 32, sc, nul, nul, nul) == 0
    assert L.gasfm_edge0_prologue_fwd(nul, 0, nul, nul, eps, *[nul] * 5) == 0
    assert L.gasfm_edge0_prologue_fwd_rows(nul, 0, nul, nul, eps, *[nul] * 5) == 0
    assert L.gasfm_edge0_epilogue_fwd(*[nul] * 3, 0, *[nul] * 4, eps, *[nul] * 6, 32, nul, sc, nul, nul) == 0
    assert L.gasfm_edge0_epilogue_bwd(nul, 0, *[nul] * 6, eps, nul, nul, sc, *[nul] * 5) == 0
    assert L.gasfm_edge0_prologue_bwd(*[nul] * 3, 0, nul, nul, eps, *[nul] * 4) == 0
    # n_items = 0 with real outputs: untouched
    dSv, part = _sentinel((4, 32), device), _sentinel((4, 32 * 34), device)
    one = torch.zeros(1, 32, device=device)
    items = torch.zeros(1, 4, dtype=torch.int32, device=device)
    _native.segment_rowsum(items, 0, None, one, PROJ_SCALE, dSv, part)
    _native.edge_epilogue_bwd(items, 0, one, one, None, one[0], one[0], EPS, one.expand(32, 32).contiguous(), PROJ_SCALE,
                              dSv, part, None, part)
    torch.cuda.synchronize()
    assert bool((_bits(dSv) == SENTINEL).all() and (_bits(part) == SENTINEL).all())
    assert L.gasfm_last_error() == before
    # the Functions
    empty = torch.zeros(0, dtype=torch.int64)
    plans = {"proj2view": AttnPlan.from_targets(empty, M_TAB).to(device),
             "proj2scenepoint": AttnPlan.from_targets(empty, N_TAB).to(device)}
    edges = EdgeIndex(empty.int().to(device), empty.int().to(device), M_TAB, N_TAB, plans)
    c = case32(1)
    for with_p0 in (True, False):
        lv = dict(P=c.P[:0], lnw=c.lnw, lnb=c.lnb, W=c.W, b=c.b, Wp=c.Wp if with_p0 else c.Wp[:, :32], bp=c.bp, Sp=c.Sp,
                  Sv=c.Sv, Sg=c.Sg.view(1, 32))
        if with_p0:
            lv["P0"] = c.P0[:0]
        d = {k: _dev(v, device).requires_grad_(True) for k, v in lv.items()}
        XL, tok = EdgePrologueFn.apply(d["P"], d["lnw"], d["lnb"], d["W"], d["b"], d["Wp"], EPS)
        Pn = EdgeEpilogueFn.apply(d["P"], d.get("P0"), tok, d["Sp"], d["Sv"], d["Sg"], d["Wp"], d["bp"], d["lnw"],
                                  d["lnb"], EPS, edges)
        assert XL.shape == (0, 64) and Pn.shape == (0, 32)
        (XL.sum() + Pn.sum()).backward()
        for k, t in d.items():
            assert t.grad is not None and t.grad.shape == t.shape and int(torch.count_nonzero(t.grad)) == 0, k
    c = case0(1)
    lv = {k: getattr(c, k) for k in ("law", "lab", "lbw", "lbb", "W0", "b0", "Wp", "bp", "Wsk", "bsk", "Sp", "Sv")}
    lv.update(P=c.P[:0], Sg=c.Sg.view(1, 32))
    d = {k: _dev(v, device).requires_grad_(True) for k, v in lv.items()}
    XL, tok = Block0PrologueFn.apply(d["P"], d["law"], d["lab"], d["W0"], d["b0"], EPS)
    Pn = Block0EpilogueFn.apply(d["P"], tok, d["Sp"], d["Sv"], d["Sg"], d["Wp"], d["bp"], d["law"], d["lab"], d["lbw"],
                                d["lbb"], d["Wsk"], d["bsk"], EPS, edges)
    assert XL.shape == (0, 8) and Pn.shape == (0, 32)
    (XL.sum() + Pn.sum()).backward()
    for k, t in d.items():
        assert t.grad is not None and t.grad.shape == t.shape and int(torch.count_nonzero(t.grad)) == 0, k
