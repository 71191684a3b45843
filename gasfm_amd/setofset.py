"""``SetOfSetNet`` (the DPESFM baseline) for MI355X: same constructor, forward and state_dict as the
reference's models/SetOfSet.py + models/layers.py:87-147, 959-984.

One ``SetOfSetLayer(d_in, d_out)`` on the [E, d_in] edge features X of a scene is

    mp[p], mc[c], mg = means of X over the edges of point p / of camera c / over all E edges
    S = lin_scenepoint(mp), V = lin_view(mc), g = lin_global(mg)
    Y[e] = (lin_proj(X[e]) + S[pt[e]] + V[cam[e]] + g) / 4

The reference builds a torch sparse tensor and ``.coalesce()``s it in every layer; on the
camera-major edge order of M2sparse that is the identity, so the layers here work on the edge rows
directly with the scene's camera / point plans (attention.AttnPlan).

Two paths, one module tree:
  * composite: plain torch ops (index_add segment sums), any device, dtype and width: the CPU
    path, the tests' fp64 oracle and tools/setofset_bench.py's baseline;
  * fused (fp32 CUDA tensors, d_in == 2 or a multiple of 32 up to 256, d_out a multiple of 32 up
    to 256): csrc/setofset.hip through ``SetOfSetLayerFn``.  The layer's forward is two segment-mean
    launches (X read twice), node-sized linears and ONE edge kernel whose epilogue gathers S and
    V (+ b + g folded into V), centres, adds the skip and applies the ReLU.  The centring vector is
    not a pass over [E, d_out]: mean_e Y = (mg W^T + (sum_p deg_p S[p] + sum_c deg_c V'[c]) / E) / 4,
    accumulated in fp64 from node-sized quantities.  The backward saves X and the layer's own
    output (the next layer's X; its sign is the ReLU mask) and nothing else of size [E, d].

A union of B scenes (batch.SceneBatch, ``batch.forward_batch``) runs on both paths with the global
mean, the global row g and the centring vector taken per scene: the scenes' cameras, points and
edges are contiguous row ranges, so these are [B, d] matrices of per-range column sums
(csrc/colsum_ranges.hip on the fused path, index_add on the composite), gathered by the scene of
each camera / edge.
"""
import torch
import torch.nn.functional as F
from torch.nn import Linear, Module, ModuleList

from . import _native, dense
from . import depth_head as depth_head_op
from .model import BaseNet, EmbeddingLayer, ProjLayer, get_linear_layers, scene_edge_index


# ------------------------------------------------------------------ scene-side quantities
class _Degrees:
    """Per-point / per-camera edge counts of a scene (float32 and float64), cached on its EdgeIndex.
    For a union of B scenes (B is not None) also the scenes' row ranges: int32 row pointers ptrc /
    ptrp / ptre, the scene of every camera / point / edge row soc / sop / soe, Es = max(E_s, 1) and
    deg / E_s per camera and point (wc, wp).  A batch.SceneBatch union builds them once from its host
    offset lists; a static_batch.StaticBatch bucket supplies them as per-step device tables."""

    # what a shape-stable union (static_batch.StaticBatch) hands over under plans["_scene_tables"]
    TABLES = ("ptrc", "ptrp", "ptre", "ptr_all_c", "Es", "degc", "invc", "wc", "degp", "invp", "wp", "soc", "sop", "soe")

    def __init__(self, edges):
        pp, pc = edges.plans["proj2scenepoint"], edges.plans["proj2view"]
        self.E = int(edges.cam.shape[0])
        tables = edges.plans.get("_scene_tables")
        if tables is not None:
            # a padded bucket: its contents change with every fill and a replayed graph reads nothing
            # from the host, so the bucket owns these as static device buffers that every fill
            # rewrites (gasfm_sos_union_tables); they are adopted, not rebuilt -- degrees included
            self.B = int(tables.B)
            for name in self.TABLES:
                setattr(self, name, getattr(tables, name))
            return
        for name, plan in (("p", pp), ("c", pc)):
            deg = (plan.seg_ptr[1:] - plan.seg_ptr[:-1]).to(torch.float64)
            setattr(self, "deg" + name, deg)
            setattr(self, "inv" + name, torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg)))
        # a union of B scenes (batch.SceneBatch): every scene's cameras, points and edges are a
        # contiguous row range.  Built once from the batch's host lists; the layers read device
        # tensors only, so a step over a fixed union captures
        self.B = None
        off = edges.plans.get("_scene_off")
        if off is None:
            if "_scene_of_cam" in edges.plans:
                raise TypeError("SetOfSetNet: this union carries no per-scene row ranges (only batch.SceneBatch "
                                "unions are supported)")
            return
        dev = edges.cam.device
        self.B = len(off[0]) - 1
        if any(len(o) != self.B + 1 for o in off):
            raise ValueError("SetOfSetNet: the union's cam / pt / edge offsets differ in length")
        ptrs = torch.tensor([list(o) for o in off], dtype=torch.int32, device=dev)           # one copy to the device
        ar = torch.arange(self.B, device=dev)
        for name, ptr, o in zip(("c", "p", "e"), ptrs, off):
            setattr(self, "ptr" + name, ptr)                                                   # int32 row pointers
            cnt = (ptr[1:] - ptr[:-1]).long()
            setattr(self, "so" + name, torch.repeat_interleave(ar, cnt, output_size=o[-1]))   # scene of row
        self.ptr_all_c = self.ptrc[::self.B].contiguous()                                      # [0, M]: all cameras
        self.Es = (self.ptre[1:] - self.ptre[:-1]).clamp(min=1).double()                       # max(E_s, 1)
        self.wc, self.wp = self.degc / self.Es[self.soc], self.degp / self.Es[self.sop]      # deg / E_s per node


def _degrees(edges):
    d = edges.__dict__.get("_sos_degrees")
    if d is None:
        d = edges.__dict__["_sos_degrees"] = _Degrees(edges)
    return d


def _union(edges):
    """The _Degrees of a union of scenes (per-scene global mean and centring); None for one scene."""
    if "_scene_of_cam" not in edges.plans:
        return None
    return _degrees(edges)


def _scene_means(X, u):
    """[B, d] means of the rows of X over each scene's edge rows (index_add; any dtype, any device)."""
    tot = torch.zeros((u.B, X.shape[1]), dtype=X.dtype, device=X.device).index_add(0, u.soe, X)
    return tot / u.Es.to(X.dtype)[:, None]


def _composite_means(X, edges):
    """(mp [n, d], mc [m, d], mg [1, d]) with index_add segment sums; empty segments give zero rows.
    For a union of B scenes mg is [B, d]: one mean per scene."""
    cam, pt = edges.cam.long(), edges.pt.long()
    E = X.shape[0]
    ones = torch.ones(E, dtype=X.dtype, device=X.device)
    degp = torch.zeros(edges.n, dtype=X.dtype, device=X.device).index_add(0, pt, ones).clamp(min=1)
    degc = torch.zeros(edges.m, dtype=X.dtype, device=X.device).index_add(0, cam, ones).clamp(min=1)
    mp = torch.zeros((edges.n, X.shape[1]), dtype=X.dtype, device=X.device).index_add(0, pt, X) / degp[:, None]
    mc = torch.zeros((edges.m, X.shape[1]), dtype=X.dtype, device=X.device).index_add(0, cam, X) / degc[:, None]
    u = _union(edges)
    mg = X.sum(0, keepdim=True) / max(E, 1) if u is None else _scene_means(X, u)
    return mp, mc, mg


def _center_rows(Y, edges):
    """Y minus its mean over the edge rows, per scene for a union (torch ops)."""
    if not Y.shape[0]:
        return Y
    u = _union(edges)
    if u is None:
        return Y - Y.mean(dim=0, keepdim=True)
    return Y - _scene_means(Y, u)[u.soe]


def fusable(X, d_in, d_out, edges):
    """The fused kernels take this layer: fp32 CUDA rows of a covered width over plain plans (one
    scene, or a union with its per-scene row ranges: a batch.SceneBatch's host offsets or a
    static_batch.StaticBatch's device tables)."""
    if not (X.is_cuda and X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] == d_in):
        return False
    pp, pc = edges.plans["proj2scenepoint"], edges.plans["proj2view"]
    if pp.all_partial or pc.all_partial or "_shard" in edges.plans:
        return False
    if "_scene_of_cam" in edges.plans and "_scene_off" not in edges.plans and "_scene_tables" not in edges.plans:
        return False
    if pc.perm is not None or (pp.perm is not None and pp.perm.dtype != torch.int32):
        return False
    return _native.sos_width_ok(d_in, d_out)


def segment_means(X, edges):
    """Fused per-point and per-camera means of X ([n, d], [m, d]); X is read once per direction."""
    return (_native.sos_segment_sum(edges.plans["proj2scenepoint"], X, mean=True),
            _native.sos_segment_sum(edges.plans["proj2view"], X, mean=True))


class SegmentMeansFn(torch.autograd.Function):
    """(mp, mc) of X for the final global update; the backward is the gather-only edge kernel."""

    @staticmethod
    def forward(ctx, X, edges):
        X = X.contiguous()
        ctx.edges = edges
        ctx.shape = X.shape
        return segment_means(X, edges)

    @staticmethod
    def backward(ctx, dmp, dmc):
        edges = ctx.edges
        dg = _degrees(edges)
        E, d = ctx.shape
        Bp = (dmp.double() * dg.invp[:, None]).float().contiguous()
        Ac = (dmc.double() * dg.invc[:, None]).float().contiguous()
        return _native.sos_edge_dx(None, None, None, edges.cam, edges.pt, Ac, Bp, E, d), None


class SetOfSetLayerFn(torch.autograd.Function):
    """One SetOfSetLayer with what follows it in the block (centring, skip add, ReLU) fused."""

    @staticmethod
    def forward(ctx, X, Wp, bp, Wsp, bsp, Wv, bv, Wg, bg, R, edges, center, relu):
        X = X.contiguous()
        dg = _degrees(edges)
        ctx.union = dg.B is not None
        if ctx.union:
            return SetOfSetLayerFn._forward_union(ctx, X, Wp, bp, Wsp, bsp, Wv, bv, Wg, bg, R, edges, center, relu, dg)
        E = max(dg.E, 1)
        mp, mc = segment_means(X, edges)
        mg = (dg.degc @ mc.double()) / E                       # [d_in], fp64, fixed order (camera rows)
        S = torch.addmm(bsp, mp, Wsp.t())
        g = (mg.float() @ Wg.t() + bg) + bp                    # the global row and lin_proj's bias
        Vb = torch.addmm(bv + g, mc, Wv.t())                   # V' = V + b + g: one gathered row per edge
        cm = None
        if center:
            cm = (0.25 * (Wp.double() @ mg + (dg.degp @ S.double() + dg.degc @ Vb.double()) / E)).float()
        Rc = None if R is None else R.contiguous()
        Y = _native.sos_edge_fwd(X, Wp.contiguous(), edges.cam, edges.pt, S, Vb, cm, Rc, relu)
        ctx.save_for_backward(X, Y if relu else None, Wp, Wsp, Wv, Wg, mp, mc, mg)
        ctx.edges, ctx.center, ctx.has_R = edges, center, R is not None
        return Y

    @staticmethod
    def _forward_union(ctx, X, Wp, bp, Wsp, bsp, Wv, bv, Wg, bg, R, edges, center, relu, dg):
        """A union of B scenes: the global mean, the global row and the centring vector are one row
        per scene ([B, .], fp64, from the ordered per-range column sums).  Every camera belongs to
        one scene, so both the global row and the centring vector are folded into its gathered row
        V'[c] and the edge kernel runs as for one scene, with no centring vector of its own."""
        mp, mc = segment_means(X, edges)
        inv_E = 1.0 / dg.Es[:, None]
        MG = _native.colsum_ranges(mc, dg.ptrc, dg.degc) * inv_E             # [B, d_in]
        S = torch.addmm(bsp, mp, Wsp.t())
        G = (MG.float() @ Wg.t() + bg) + bp                                    # [B, d_out]
        Vb = torch.addmm(bv, mc, Wv.t()) + G[dg.soc]
        if center:  # 4 cm_s = Wp mg_s + (sum_p deg_p S[p] + sum_c deg_c V'[c]) / E_s; Y = (.. + V') / 4
            cm4 = MG @ Wp.double().t() + (_native.colsum_ranges(S, dg.ptrp, dg.degp)
                                          + _native.colsum_ranges(Vb, dg.ptrc, dg.degc)) * inv_E
            Vb = (Vb.double() - cm4[dg.soc]).float()
        Rc = None if R is None else R.contiguous()
        Y = _native.sos_edge_fwd(X, Wp.contiguous(), edges.cam, edges.pt, S, Vb, None, Rc, relu)
        ctx.save_for_backward(X, Y if relu else None, Wp, Wsp, Wv, Wg, mp, mc, MG)
        ctx.edges, ctx.center, ctx.has_R = edges, center, R is not None
        return Y

    @staticmethod
    def _backward_union(ctx, dY):
        X, Ym, Wp, Wsp, Wv, Wg, mp, mc, MG = ctx.saved_tensors
        edges, dg = ctx.edges, _degrees(ctx.edges)
        dY = dY.contiguous()
        pp, pc = edges.plans["proj2scenepoint"], edges.plans["proj2view"]
        dS32 = _native.sos_segment_sum(pp, dY, 0.25, mask=Ym)
        dV32 = _native.sos_segment_sum(pc, dY, 0.25, mask=Ym)
        U = None
        if ctx.center:  # u_s = -sum_{c in s} dV32[c]: the gradient of 4 cm_s, through its node-sized inputs
            U = -_native.colsum_ranges(dV32, dg.ptrc)                          # [B, d_out]
            dS32 = (dS32.double() + dg.wp[:, None] * U[dg.sop]).float()
            dV32 = (dV32.double() + dg.wc[:, None] * U[dg.soc]).float()
        DG = _native.colsum_ranges(dV32, dg.ptrc)                              # [B, d_out]: the global rows' gradient
        dgrow32 = _native.colsum_ranges(dV32, dg.ptr_all_c)[0].float()         # sum_s DG[s]: the shared biases
        dWsp, dbsp = dS32.t() @ mp, _native.colsum(dS32)
        dWv, dbv = dV32.t() @ mc, dgrow32.clone()
        dWg, dbg = (DG.t() @ MG).float(), dgrow32.clone()
        dMG = DG @ Wg.double()
        if U is not None:
            dMG = dMG + U @ Wp.double()
        dX = None
        if ctx.needs_input_grad[0]:
            dmp = dS32 @ Wsp
            dmc = (dV32 @ Wv).double() + dg.wc[:, None] * dMG[dg.soc]          # mg_s = sum_{c in s} deg_c mc[c] / E_s
            Bp = (dmp.double() * dg.invp[:, None]).float()
            Ac = (dmc * dg.invc[:, None]).float()
            dX = _native.sos_edge_dx(dY, Ym, Wp.contiguous(), edges.cam, edges.pt, Ac, Bp, X.shape[0], X.shape[1])
        dWp = _native.sos_edge_dw(dY, Ym, X)
        if U is not None:
            dWp = (dWp.double() + U.t() @ MG).float()
        dR = None
        if ctx.has_R and ctx.needs_input_grad[9]:
            dR = dY if Ym is None else dY * (Ym > 0)
        return dX, dWp, dgrow32, dWsp, dbsp, dWv, dbv, dWg, dbg, dR, None, None, None

    @staticmethod
    def backward(ctx, dY):
        if ctx.union:
            return SetOfSetLayerFn._backward_union(ctx, dY)
        X, Ym, Wp, Wsp, Wv, Wg, mp, mc, mg = ctx.saved_tensors
        edges, dg = ctx.edges, _degrees(ctx.edges)
        E = max(dg.E, 1)
        dY = dY.contiguous()
        pp, pc = edges.plans["proj2scenepoint"], edges.plans["proj2view"]
        # dT = mask . dY / 4: its segment sums; node-sized from here on.  Column sums over the node
        # rows go through the ordered colsum kernel (torch's reductions did not replay bitwise
        # from a captured graph), elementwise work in fp64
        dS32 = _native.sos_segment_sum(pp, dY, 0.25, mask=Ym)
        dV32 = _native.sos_segment_sum(pc, dY, 0.25, mask=Ym)
        dWp_extra = dmg = None
        if ctx.center:
            # cmean's gradient is -sum_e mask . dY; u = that / 4 through cmean's node-sized inputs
            u = -_native.colsum(dV32).double()
            dS32 = (dS32.double() + (dg.degp / E)[:, None] * u).float()
            dV32 = (dV32.double() + (dg.degc / E)[:, None] * u).float()
            dWp_extra = torch.outer(u, mg)
            dmg = u @ Wp.double()
        dgrow32 = _native.colsum(dV32)                         # db of lin_proj == the global row's gradient
        dgrow = dgrow32.double()
        dWsp, dbsp = dS32.t() @ mp, _native.colsum(dS32)
        dWv, dbv = dV32.t() @ mc, dgrow32.clone()       # one tensor per parameter: .grad adopts it
        dWg, dbg = torch.outer(dgrow, mg).float(), dgrow32.clone()
        dmg_t = dgrow @ Wg.double()
        dmg = dmg_t if dmg is None else dmg + dmg_t
        dX = None
        if ctx.needs_input_grad[0]:
            dmp = dS32 @ Wsp
            dmc = (dV32 @ Wv).double() + (dg.degc / E)[:, None] * dmg  # mg = sum_c deg_c mc[c] / E
            Bp = (dmp.double() * dg.invp[:, None]).float()
            Ac = (dmc * dg.invc[:, None]).float()
            dX = _native.sos_edge_dx(dY, Ym, Wp.contiguous(), edges.cam, edges.pt, Ac, Bp, X.shape[0], X.shape[1])
        dWp = _native.sos_edge_dw(dY, Ym, X)
        if dWp_extra is not None:
            dWp = (dWp.double() + dWp_extra).float()
        dR = None
        if ctx.has_R and ctx.needs_input_grad[9]:
            dR = dY if Ym is None else dY * (Ym > 0)
        return dX, dWp, dgrow32, dWsp, dbsp, dWv, dbv, dWg, dbg, dR, None, None, None


class SceneCenterFn(torch.autograd.Function):
    """X minus each scene's mean over its (contiguous) edge rows, for a union on the fused path: the
    skip ProjLayer's centring.  The means are the ordered per-range column sums; centring is its own
    adjoint, so the backward is the same operation on dY."""

    @staticmethod
    def _center(X, dg):
        mean = _native.colsum_ranges(X, dg.ptre) / dg.Es[:, None]
        return X - mean.float()[dg.soe]

    @staticmethod
    def forward(ctx, X, edges):
        ctx.edges = edges
        return SceneCenterFn._center(X.contiguous(), _degrees(edges))

    @staticmethod
    def backward(ctx, dY):
        return SceneCenterFn._center(dY.contiguous(), _degrees(ctx.edges)), None


# ------------------------------------------------------------------ modules (reference key names)
class SetOfSetGlobalFeatureUpdate(Module):
    """layers.py:100-126."""

    def __init__(self, d_in, d_out, output_global=True):
        super().__init__()
        self.lin_scenepoint = Linear(d_in, d_out)
        self.lin_view = Linear(d_in, d_out)
        self.output_global = output_global
        if output_global:
            self.lin_global = Linear(d_in, d_out)

    def forward(self, X, edges):
        """The final update (output_global False) on raw tensors: (S [n, d_out], V [m, d_out])."""
        if fusable(X, X.shape[1], 32, edges):
            mp, mc = SegmentMeansFn.apply(X, edges)
        else:
            mp, mc, _ = _composite_means(X, edges)
        return dense.linear(mp, self.lin_scenepoint), dense.linear(mc, self.lin_view)


class SetOfSetProjectionFeatureUpdate(Module):
    """layers.py:129-147."""

    def __init__(self, d_in, d_out):
        super().__init__()
        self.lin_proj = Linear(d_in, d_out)


class SetOfSetLayer(Module):
    """layers.py:87-97, with the block's centring / skip add / ReLU that follow it."""

    def __init__(self, d_in, d_out):
        super().__init__()
        self.d_in, self.d_out = d_in, d_out
        self.global_feature_update = SetOfSetGlobalFeatureUpdate(d_in, d_out)
        self.projection_feature_update = SetOfSetProjectionFeatureUpdate(d_in, d_out)

    def forward(self, X, edges, center=False, relu=False, residual=None, composite=False):
        gfu, lp = self.global_feature_update, self.projection_feature_update.lin_proj
        if not composite and fusable(X, self.d_in, self.d_out, edges):
            return SetOfSetLayerFn.apply(X, lp.weight, lp.bias, gfu.lin_scenepoint.weight, gfu.lin_scenepoint.bias,
                                         gfu.lin_view.weight, gfu.lin_view.bias, gfu.lin_global.weight,
                                         gfu.lin_global.bias, residual, edges, center, relu)
        mp, mc, mg = _composite_means(X, edges)
        S, V, g = gfu.lin_scenepoint(mp), gfu.lin_view(mc), gfu.lin_global(mg)
        u = _union(edges)
        if u is not None:  # one global row per scene
            g = g[u.soe]
        Y = (lp(X) + S[edges.pt.long()] + V[edges.cam.long()] + g) / 4
        if center:
            Y = _center_rows(Y, edges)
        if residual is not None:
            Y = residual + Y
        return F.relu(Y) if relu else Y


class SetOfSetBlock(Module):
    """SetOfSet.py:7-46."""

    def __init__(self, d_in, d_out, conf):
        super().__init__()
        self.block_size = conf.get_int("model.block_size")
        self.proj_feat_normalization = conf.get_bool("model.proj_feat_normalization")
        self.add_skipconn_for_residual_blocks = conf.get_bool("model.add_skipconn_for_residual_blocks")
        self.layers = ModuleList([SetOfSetLayer(d_in, d_out)]
                                 + [SetOfSetLayer(d_out, d_out) for _ in range(1, self.block_size)])
        if self.add_skipconn_for_residual_blocks:
            self.skip_projection = None if d_in == d_out else ProjLayer(d_in, d_out)

    def forward(self, X, edges, composite=False):
        skip = None
        if self.add_skipconn_for_residual_blocks:
            skip = X
            if self.skip_projection is not None:
                skip = dense.linear(X, self.skip_projection.lin_proj)
                if self.proj_feat_normalization and skip.shape[0]:
                    if not composite and skip.is_cuda and skip.dtype == torch.float32 and _union(edges) is not None:
                        skip = SceneCenterFn.apply(skip, edges)
                    else:
                        skip = _center_rows(skip, edges)
        xl = X
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            if i < last:
                xl = layer(xl, edges, center=self.proj_feat_normalization, relu=True, composite=composite)
            else:  # the skip add and the block's final ReLU in the last layer's epilogue
                xl = layer(xl, edges, center=False, relu=True, residual=skip, composite=composite)
        return xl


class SetOfSetNet(BaseNet):
    """SetOfSet.py:49-142."""

    def __init__(self, conf, batchnorm=False):
        super().__init__(conf)
        num_blocks = conf.get_int("model.num_blocks")
        num_feats = conf.get_int("model.num_features")
        pos_emb_n_freq = conf.get_int("model.pos_emb_n_freq")
        self.depth_head_enabled = conf.get_bool("model.depth_head.enabled", default=False)
        self.view_head_enabled = conf.get_bool("model.view_head.enabled", default=False)
        self.scenepoint_head_enabled = conf.get_bool("model.scenepoint_head.enabled", default=False)
        self.batchnorm = batchnorm
        n_feat_depth = conf.get_int("model.depth_head.n_feat") if self.depth_head_enabled else None
        self.embed = EmbeddingLayer(pos_emb_n_freq, 2)  # raises for pos_emb_n_freq > 0
        self.equivariant_blocks = ModuleList()
        for i in range(num_blocks):
            self.equivariant_blocks.append(SetOfSetBlock(
                self.embed.d_out if i == 0 else num_feats,
                n_feat_depth if self.depth_head_enabled and i == num_blocks - 1 else num_feats, conf))
        if self.view_head_enabled or self.scenepoint_head_enabled:
            if not self.view_head_enabled:
                raise NotImplementedError("Final feature aggregation for only view features or scenepoint features "
                                          "alone is not implemented.")
            self.final_global_update = SetOfSetGlobalFeatureUpdate(num_feats, num_feats, output_global=False)
        if self.batchnorm:
            raise NotImplementedError()
        if self.depth_head_enabled:
            nh = conf.get_int("model.depth_head.n_hidden_layers")
            self.depth_head = get_linear_layers((1 + nh) * [n_feat_depth] + [1], norm=False)
        if self.view_head_enabled:
            nh = conf.get_int("model.view_head.n_hidden_layers")
            self.view_head = get_linear_layers((1 + nh) * [num_feats] + [self.out_channels], norm=False)
        if self.scenepoint_head_enabled:
            nh = conf.get_int("model.scenepoint_head.n_hidden_layers")
            self.scenepoint_head = get_linear_layers((1 + nh) * [num_feats] + [3], norm=False)

    # False: every layer on the fused kernels where they apply; True: the torch-op composite path
    composite = False

    def edge_index_for(self, data, device):
        tables = getattr(data, "sos_tables", None)
        if tables is not None:  # a static_batch.StaticBatch: its per-scene tables, made on first use
            tables()
        return scene_edge_index(data, device)

    def forward(self, data):
        values = data.x.values
        edges = self.edge_index_for(data, values.device)
        x = self.embed(values)
        for blk in self.equivariant_blocks:
            x = blk(x, edges, composite=self.composite)
        pred = {}
        if self.depth_head_enabled:
            from .scene import SparseMat
            sx = data.x
            d = depth_head_op.apply(self.depth_head, x) if depth_head_op.fusable(self.depth_head, x) \
                else self.depth_head(x)
            pred["depths"] = SparseMat(d, sx.indices, sx.cam_per_pts, sx.pts_per_cam, [sx.shape[0], sx.shape[1], 1])
        if self.view_head_enabled or self.scenepoint_head_enabled:
            if self.composite:
                mp, mc, _ = _composite_means(x, edges)
                fgu = self.final_global_update
                n_in, m_in = fgu.lin_scenepoint(mp), fgu.lin_view(mc)
            else:
                n_in, m_in = self.final_global_update(x, edges)
            n_in, m_in = F.relu(n_in), F.relu(m_in)
        if self.view_head_enabled:
            pred.update(self.extract_view_outputs(dense.sequential(self.view_head, m_in)))
        if self.scenepoint_head_enabled:
            pred.update(self.extract_scenepoint_outputs(dense.sequential(self.scenepoint_head, n_in).T))
        return pred
