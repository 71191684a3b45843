"""``GraphAttnSfMNet`` for MI355X — same constructor, forward signature and state_dict.

The module tree reproduces the reference's parameter names exactly (886 keys
for the 12-block learning conf; code/models/graph_attn_sfm.py:8-115,
code/models/layers.py), so ``load_state_dict`` of a reference checkpoint
works and ``main.py``'s pretrained-key whitelist (main.py:168-190) holds.

The forward is re-designed around the scene's ``AttnPlan``s instead of the
reference's concatenate-then-PyG sequence:
  * no ``to_torch_hybrid_sparse_coo().coalesce()`` per layer (layers.py:823,922):
    edges stay in M2sparse's cam-major order and the point direction uses the
    plan's CSC permutation;
  * GATv2 lin_l runs on the E edge rows only and lin_r on the N target rows only
    (PyG runs both on all E+N rows), and block 0's zero target features become
    the lin_r bias (no E+N zero tensor);
  * edge-softmax + aggregation (+ backward) is the fused HIP kernel;
  * no host syncs (the reference asserts index equality on the host every block,
    sparse_utils.py:298-300, dataset_utils.py:557).
Dense per-node projections (view 1024 / global 2048 widths) run on MFMA through
torch (hipBLASLt).
"""
import copy
import os

import torch
import torch.nn.functional as F
from torch.nn import Identity, LayerNorm, Linear, Module, ModuleList, ReLU, Sequential

from . import _native, dense, edge_block, edge_ops, point_block, view_block
from . import depth_head as depth_head_op
from .attention import AttnPlan, GatAttentionFn, gat_attention
from .edge_block import (Block0PrologueFn, CamArgs, DualAttentionFn, EdgeCamFn, EdgePrologueFn, Epilogue0Args,
                         EpilogueArgs, PendingEpilogue, WideEpilogueFn, materialize)
from .gatv2 import GATv2Conv, zero_target_rows


# Edge prologue with the camera attention fused in (edge_block.EdgeCamFn, csrc/edge_cam.hip) for the
# 32-wide blocks; GASFM_EDGE_CAM=0 selects the separate prologue + DualAttentionFn kernels (A/B).
EDGE_CAM = os.environ.get("GASFM_EDGE_CAM", "1") != "0"
# A 32-wide block's edge epilogue is left pending (edge_block.PendingEpilogue) and run in one kernel
# with the next block's prologue + camera attention (SeamFn, gasfm_edge_seam_fwd); 0: separately.
EDGE_SEAM = os.environ.get("GASFM_EDGE_SEAM", "1") != "0"
# Block 0's (2-wide) epilogue likewise inside block 1's prologue kernel (Seam0Fn, gasfm_edge0_seam_fwd).
EDGE_SEAM0 = os.environ.get("GASFM_EDGE_SEAM0", "1") != "0"
# A depth conf's last block (32-wide features in, 128-wide out: lin_proj [128, 34], LayerNorm'd skip
# projection [128, 32]) on the fused edge kernels (forward_fused_wide, csrc/edge_wide.hip);
# GASFM_EDGE_WIDE=0: the unfused aten route.
EDGE_WIDE = os.environ.get("GASFM_EDGE_WIDE", "1") != "0"
# A block's whole global-node chain (its tail and every consumer of g) as one GlobalChainFn
# (csrc/global_chain.hip, round 4); GASFM_GLOBAL_CHAIN=0: the GlobalLinearFn / GlobalHubFn path.
GLOBAL_CHAIN = os.environ.get("GASFM_GLOBAL_CHAIN", "1") != "0"


def replicated_to_local(x, shard):
    if shard is None:
        return x
    from .distributed import AllReduceGrad
    return AllReduceGrad.apply(x, shard)


def replicated_to_local_n(shard, *xs):
    """Several replicated tensors consumed locally: one gradient all-reduce for all of them."""
    if shard is None:
        return xs
    from .distributed import AllReduceGradN
    return AllReduceGradN.apply(shard, *xs)


def _cam_sharded(shard):
    return shard is not None and shard.cams is not None


class BlockCarry:
    """What the fused hubs of one forward hand on, one field per hand-off; None: not set.  (The
    carry itself is None on the CPU and for stateless features: no hubs run.)

    field      producer (in block b)               consumer
    XRp        point hub                           block b+1's point attention (its target rows)
    pts_skip   point hub                           block b+1's point tail (its state skip)
    SA         point hub                           block b's edge epilogue (point term)
    XLs2g      point hub                           block b's points->global conv (its lin_l rows)
    XRc        view hub, or the block exchange     block b+1's camera attention (its target rows), via
                                                   block b's _edge_terms (the shard boundary's wrap)
    view_skip  view hub                            block b+1's view tail (its state skip)
    SV         view hub, or the block exchange     block b's edge epilogue (camera term)
    XLv2g      view hub                            block b's views->global conv (its lin_l rows)
    exch       view hub (camera-sharded)           block b's global convs: the BlockExchange
    rows_own   view hub (camera-sharded)           block b's global convs: this rank's (SV, XR) rows
    SG         global chain (or global hub)        block b's edge epilogue (global term)
    pre_glob   global chain (or global hub)        block b+1's global convs: (XRv, XRp, state skip)
    """
    __slots__ = ("XRp", "pts_skip", "SA", "XLs2g", "XRc", "view_skip", "SV", "XLv2g", "exch", "rows_own", "SG",
                 "pre_glob")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)

    def take(self, name):
        """The field's value; the field is cleared."""
        value = getattr(self, name)
        setattr(self, name, None)
        return value

    def pending(self):
        """Names of the fields still set (none after a whole forward)."""
        return [name for name in self.__slots__ if getattr(self, name) is not None]


def _edge_terms(pfu, pts, view, glob, plans, carry):
    """A block's epilogue terms (sp, sv, sg): the hubs' where they ran (carry), folded over the scenes
    of a SceneBatch.  sv / sg (replicated, read by the local edges) get their gradients summed over
    ranks by ONE all-reduce -- together with the next block's camera target rows XRc when the view
    hub left them in carry (their gradient, from that block's camera attention on the local edges,
    is partial too): an XRc taken from the carry is wrapped, and that block runs no all-reduce."""
    hub = (carry.take("SA"), carry.take("SV"), carry.take("SG")) if carry is not None else ()
    sp, sv, sg = pfu.node_terms(pts, view, glob, *hub)
    if carry is None or carry.XRc is None:
        sv, sg = replicated_to_local_n(plans.get("_shard"), sv, sg)
    else:
        sv, sg, carry.XRc = replicated_to_local_n(plans.get("_shard"), sv, sg, carry.XRc)
    return (sp, *_fold_global(sv, sg, plans))


class _LazySharded:
    """ShardedAttentionFn, imported on first use (keeps torch.distributed out of the 1-GPU import path)."""

    @staticmethod
    def apply(*args):
        from .distributed import ShardedAttentionFn as F_
        return F_.apply(*args)


ShardedAttentionFn = _LazySharded

GRAPH_NAMES = ("proj2view", "proj2scenepoint", "view2global", "scenepoint2global")


def get_linear_layers(feats, init_activation=False, final_activation=False, norm=True):
    """Same layer sequence (and Sequential indices) as layers.py:10-44."""
    assert len(feats) >= 2
    seq = []
    if init_activation:
        seq += ([LayerNorm(feats[0])] if norm else []) + [ReLU(inplace=True)]
    for a, b in zip(feats[:-2], feats[1:-1]):
        seq.append(Linear(a, b))
        seq += ([LayerNorm(b)] if norm else []) + [ReLU(inplace=True)]
    seq.append(Linear(feats[-2], feats[-1]))
    if final_activation:
        seq += ([LayerNorm(feats[-1])] if norm else []) + [ReLU(inplace=True)]
    return Sequential(*seq)


def _norm_relu_proj(width_state, width_proj):
    seq = [LayerNorm(width_state), ReLU(inplace=True)]
    if width_proj != width_state:
        seq.append(Linear(width_state, width_proj))
    return Sequential(*seq)


def _agg_width(n_feat_in, n_heads, explicit):
    if explicit is not None:
        assert explicit % n_heads == 0
        return explicit
    w = n_feat_in
    if w % n_heads:
        w += n_heads - w % n_heads
    return w


class _NodeAggregation(Module):
    """Shared body of Proj2View (layers.py:266-361) and Proj2ScenePoint (363-458)."""

    _state_key = _proj_key = None

    def __init__(self, n_feat_proj_in, n_feat_out, n_heads, stateful=True, use_norm_pre_mlp=True,
                 n_feat_agg=None, n_hidden_layers=0):
        super().__init__()
        self.n_feat_proj_in = n_feat_proj_in
        self.n_feat_out = n_feat_out
        self.stateful = stateful
        self.use_norm_pre_mlp = use_norm_pre_mlp
        self.n_feat_agg = _agg_width(n_feat_proj_in, n_heads, n_feat_agg)
        if stateful:
            setattr(self, self._state_key, _norm_relu_proj(n_feat_out, n_feat_proj_in))
        self.graph_conv = GATv2Conv(n_feat_proj_in, self.n_feat_agg // n_heads, heads=n_heads, add_self_loops=False)
        if self.n_feat_agg != n_feat_out:
            setattr(self, self._proj_key, Linear(self.n_feat_agg, n_feat_out))
        if use_norm_pre_mlp:
            self.norm_pre_mlp = LayerNorm(n_feat_out)
        self.mlp = get_linear_layers((2 + n_hidden_layers) * [n_feat_out], norm=False)

    def forward_plan(self, proj_feats, plan, prev, plan_partial=None, shard=None):
        """proj_feats [E, F_in] (edge order) -> node features [N, n_feat_out]."""
        assert self.stateful == (prev is not None)
        if shard is not None and plan_partial is not None:
            XR = replicated_to_local(self.target_rows(prev, plan.num_targets), shard)
            XL = dense.linear(proj_feats, self.graph_conv.lin_l)
            c = self.graph_conv
            x = ShardedAttentionFn.apply(XL, XR, c.att, c.bias, plan, plan_partial, c.heads, c.negative_slope, shard)
            return self.tail(x, prev)
        x_agg = dense.sequential(getattr(self, self._state_key), prev) if prev is not None else None
        return self.tail(self.graph_conv.attend(proj_feats, x_agg, plan), prev)

    def target_rows(self, prev, num_targets):
        """XR = lin_r(x_agg) of the destination nodes (lin_r(0) broadcast when stateless)."""
        conv = self.graph_conv
        if prev is None:
            return zero_target_rows(conv.lin_r, num_targets, conv.lin_r.weight)
        return dense.linear(dense.sequential(getattr(self, self._state_key), prev), conv.lin_r)

    def tail(self, x, prev, exch=None):
        """Everything after the GATv2 aggregation: proj, state skip, LN+ReLU, MLP, skip.  exch: the
        camera-sharded block exchange (the view tail's backward writes into its send block)."""
        if point_block.tail_fusable(self, x, prev):
            return point_block.tail(self, x, prev)
        if view_block.tail_fusable(self, x, prev):
            return view_block.tail(self, x, prev, exch)
        if self.n_feat_agg != self.n_feat_out:
            x = dense.linear(x, getattr(self, self._proj_key))
        if prev is not None:
            x = prev + x
        if self.use_norm_pre_mlp and len(self.mlp) == 1:
            return dense.ln_relu_linear(x, self.norm_pre_mlp, self.mlp[0], residual=True)
        skip = x
        if self.use_norm_pre_mlp:
            x = F.relu(dense.layer_norm(x, self.norm_pre_mlp))
        return skip + dense.sequential(self.mlp, x)


class Proj2View(_NodeAggregation):
    _state_key, _proj_key = "norm_and_proj_view2proj", "proj_proj2view"

    def __init__(self, n_feat_proj_in, n_feat_view_out, n_heads, stateful=True, use_norm_pre_mlp=True,
                 n_feat_proj2view_agg=None, n_hidden_layers_view_update=0):
        super().__init__(n_feat_proj_in, n_feat_view_out, n_heads, stateful, use_norm_pre_mlp,
                         n_feat_proj2view_agg, n_hidden_layers_view_update)


class Proj2ScenePoint(_NodeAggregation):
    _state_key, _proj_key = "norm_and_proj_scenepoint2proj", "proj_proj2scenepoint"

    def __init__(self, n_feat_proj_in, n_feat_scenepoint_out, n_heads, stateful=True, use_norm_pre_mlp=True,
                 n_feat_proj2scenepoint_agg=None, n_hidden_layers_scenepoint_update=0):
        super().__init__(n_feat_proj_in, n_feat_scenepoint_out, n_heads, stateful, use_norm_pre_mlp,
                         n_feat_proj2scenepoint_agg, n_hidden_layers_scenepoint_update)


class ViewAndScenePoint2Global(Module):
    """layers.py:460-603: GATv2 over valid views -> 1 and valid points -> 1, then MLP."""

    def __init__(self, n_feat_scenepoint_in, n_feat_view_in, n_feat_global_out, n_heads, stateful=True,
                 use_norm_pre_mlp=True, n_feat_scenepoint2global_agg=None, n_feat_view2global_agg=None,
                 n_hidden_layers_global_update=0):
        super().__init__()
        self.n_feat_global_out = n_feat_global_out
        self.stateful = stateful
        self.use_norm_pre_mlp = use_norm_pre_mlp
        self.n_feat_scenepoint2global_agg = _agg_width(n_feat_scenepoint_in, n_heads, n_feat_scenepoint2global_agg)
        self.n_feat_view2global_agg = _agg_width(n_feat_view_in, n_heads, n_feat_view2global_agg)
        if stateful:
            self.norm_and_proj_global2view = _norm_relu_proj(n_feat_global_out, n_feat_view_in)
        self.graph_conv_view2global = GATv2Conv(n_feat_view_in, self.n_feat_view2global_agg // n_heads,
                                                heads=n_heads, add_self_loops=False)
        if stateful:
            self.norm_and_proj_global2scenepoint = _norm_relu_proj(n_feat_global_out, n_feat_scenepoint_in)
        self.graph_conv_scenepoint2global = GATv2Conv(n_feat_scenepoint_in,
                                                      self.n_feat_scenepoint2global_agg // n_heads,
                                                      heads=n_heads, add_self_loops=False)
        cat_w = self.n_feat_view2global_agg + self.n_feat_scenepoint2global_agg
        if cat_w != n_feat_global_out:
            self.proj_view_and_scenepoint2global = Linear(cat_w, n_feat_global_out)
        if use_norm_pre_mlp:
            self.norm_pre_mlp = LayerNorm(n_feat_global_out)
        self.mlp = get_linear_layers((2 + n_hidden_layers_global_update) * [n_feat_global_out], norm=False)

    def forward_plan(self, view, pts, plan_v2g, plan_s2g, prev, plan_s2g_partial=None, shard=None,
                     plan_v2g_partial=None, chain=None, carry=None):
        """Returns (g, rows).  carry (BlockCarry): its pre_glob, XLv2g, XLs2g (the convs' lin_l(view) /
        lin_l(pts)) and exch are taken where the hubs set them.
        Camera-sharded (shard.cams): view holds this rank's camera rows and both attentions
        exchange partial states in one all-gather (distributed.ShardedGlobalAttentionFn); with exch
        the view hub's rows_own leave in it too (ShardedGlobalExchangeFn) and rows is the gathered
        [m, 32] (SV, XRc), else None.
        chain: dense.chain_params of this update and the consumers of its output; the tail then runs
        as one GlobalChainFn and g is its (g, SG[, XRv, XRp]) tuple."""
        assert self.stateful == (prev is not None)
        cv, c = self.graph_conv_view2global, self.graph_conv_scenepoint2global
        pre_glob = XLv = XLp = exch = None
        if carry is not None:
            pre_glob, XLv, XLp, exch = (carry.take(k) for k in ("pre_glob", "XLv2g", "XLs2g", "exch"))
        if pre_glob is not None:
            XRv, XRp, prev = pre_glob
        else:
            xv = dense.sequential(self.norm_and_proj_global2view, prev) if prev is not None else None
            xp = dense.sequential(self.norm_and_proj_global2scenepoint, prev) if prev is not None else None
            XRv, XRp = _target_row(cv, xv, view, plan_v2g.num_targets), _target_row(c, xp, pts, plan_s2g.num_targets)
        XLv = XLv if XLv is not None else dense.linear(view, cv.lin_l)
        XLp = XLp if XLp is not None else dense.linear(pts, c.lin_l)
        rows = None
        if exch is not None:  # camera-sharded, from the view hub
            from .distributed import ShardedGlobalExchangeFn
            x, *rows = ShardedGlobalExchangeFn.apply(
                XLv, XRv, cv.att, cv._bias(XLv), XLp, XRp, c.att, c.bias, *carry.take("rows_own"),
                (plan_v2g, plan_s2g), c.heads, c.negative_slope, shard, exch, pre_glob is not None)
        elif _cam_sharded(shard):
            from .distributed import ShardedGlobalAttentionFn
            x = ShardedGlobalAttentionFn.apply(
                XLv, XRv, cv.att, cv._bias(XLv), XLp, XRp, c.att, c.bias,
                (plan_v2g, plan_v2g_partial, plan_s2g, plan_s2g_partial), c.heads, c.negative_slope, shard)
        elif shard is None and XLv.is_cuda and plan_v2g.num_targets == 1 and plan_s2g.num_targets == 1 \
                and cv.heads == c.heads and cv.negative_slope == c.negative_slope:
            from .attention import GlobalPairFn
            x = GlobalPairFn.apply(XLv, XRv, cv.att, cv._bias(XLv), XLp, XRp, c.att, c._bias(XLp), plan_v2g, plan_s2g,
                                   c.heads, c.negative_slope)
        else:
            v2g = gat_attention(XLv, XRv, cv.att, cv._bias(XLv), plan_v2g, cv.heads, cv.negative_slope)
            if shard is None:
                s2g = gat_attention(XLp, XRp, c.att, c._bias(XLp), plan_s2g, c.heads, c.negative_slope)
            else:  # points are sharded, the global target is replicated
                s2g = ShardedAttentionFn.apply(XLp, replicated_to_local(XRp, shard), c.att, c.bias, plan_s2g,
                                               plan_s2g_partial, c.heads, c.negative_slope, shard)
            x = torch.cat([v2g, s2g], dim=1)
        return self._global_tail(x, prev, chain), rows

    def _global_tail(self, x, prev, chain=None):
        if chain is not None:
            out = dense.global_chain(x, prev, chain, getattr(self, "_proj_bf16", False))
            if out is not None:
                return out
        if hasattr(self, "proj_view_and_scenepoint2global"):
            x = dense.linear_res(x, self.proj_view_and_scenepoint2global, prev)
        elif prev is not None:
            x = prev + x
        if self.use_norm_pre_mlp and len(self.mlp) == 1:
            return dense.ln_relu_linear(x, self.norm_pre_mlp, self.mlp[0], residual=True)
        skip = x
        if self.use_norm_pre_mlp:
            x = F.relu(dense.layer_norm(x, self.norm_pre_mlp))
        return skip + dense.sequential(self.mlp, x)


def _target_row(conv, x_tgt, ref, n=1):
    """XR of a one-target GATv2 conv (n targets for a SceneBatch): lin_r(x_tgt), or lin_r(0) (== its
    bias) for the reference's zero target features when stateless (dataset_utils.py:569-571)."""
    if x_tgt is None:
        return zero_target_rows(conv.lin_r, n, ref)
    return dense.linear(x_tgt, conv.lin_r)


class FoldGlobalFn(torch.autograd.Function):
    """Sv'[c] = Sv[c] + Sg[scene(c)] in one kernel each way (csrc/static_batch.hip): the backward's
    per-scene sums run in camera order without atomics (torch's index_select backward is an
    atomic index_add after a fill)."""

    @staticmethod
    def forward(ctx, sv, sg, soc):
        ctx.save_for_backward(soc)
        ctx.S = sg.shape[0]
        return _native.fold_scene_rows_fwd(sv, sg, soc)

    @staticmethod
    def backward(ctx, dout):
        (soc,) = ctx.saved_tensors
        dout = dout if dout.stride(1) == 1 else dout.contiguous()
        return dout, _native.fold_scene_rows_bwd(dout, soc, ctx.S), None


_ZERO_ROWS = {}


def _zero_row(width, device):
    """A cached [1, width] zero row (read-only): the folded global term Sg' without a fill launch."""
    key = (width, str(device))
    z = _ZERO_ROWS.get(key)
    if z is None:
        z = _ZERO_ROWS[key] = torch.zeros((1, width), dtype=torch.float32, device=device)
    return z


def _fold_global(sv, sg, plans):
    """SceneBatch (batch.py): the per-edge global term of scene s, Sg[s], added to the per-camera
    term of its cameras (every camera belongs to one scene), so the edge kernels see one scene:
    Sv'[c] = Sv[c] + Sg[scene(c)], Sg' = 0."""
    soc = plans.get("_scene_of_cam")
    if soc is None or sg is None or sg.shape[0] == 1:
        return sv, sg
    if (sv.is_cuda and sv.dtype == torch.float32 and sg.dtype == torch.float32 and sv.dim() == 2
            and sv.stride(1) == 1 and sg.stride(1) == 1 and sg.shape[1] == sv.shape[1] and soc.dtype == torch.int64):
        return FoldGlobalFn.apply(sv, sg, soc), _zero_row(sg.shape[1], sg.device)
    return sv + sg.index_select(0, soc), torch.zeros((1, sg.shape[1]), dtype=sg.dtype, device=sg.device)


class _Global2Node(Module):
    """Global2View / Global2ScenePoint (layers.py:605-720); disabled in every GASFM conf."""

    _node_norm = _node_lin = None

    def __init__(self, n_feat_global_in, n_feat_node, n_hidden_layers=0, use_norm=True):
        super().__init__()
        self.use_norm = use_norm
        self.n_hidden_layers = n_hidden_layers
        if use_norm:
            setattr(self, self._node_norm, LayerNorm(n_feat_node))
            self.global_norm_layer = LayerNorm(n_feat_global_in)
        setattr(self, self._node_lin, Linear(n_feat_node, n_feat_node))
        self.lin_global = Linear(n_feat_global_in, n_feat_node, bias=False)
        if n_hidden_layers > 0:
            self.mlp = get_linear_layers(n_hidden_layers * [n_feat_node] + [n_feat_node], norm=False)

    def forward(self, glob, prev):
        x, g = prev, glob
        if self.use_norm:
            x = F.relu(getattr(self, self._node_norm)(x))
            g = F.relu(self.global_norm_layer(g))
        x = getattr(self, self._node_lin)(x) + self.lin_global(g)
        if self.n_hidden_layers > 0:
            x = self.mlp(F.relu(x))
        return prev + x


class Global2View(_Global2Node):
    _node_norm, _node_lin = "view_norm_layer", "lin_view"

    def __init__(self, n_feat_global_in, n_feat_view_in_out, n_hidden_layers_view_update=0,
                 use_norm_global2view_update=True):
        super().__init__(n_feat_global_in, n_feat_view_in_out, n_hidden_layers_view_update,
                         use_norm_global2view_update)


class Global2ScenePoint(_Global2Node):
    _node_norm, _node_lin = "scenepoint_norm_layer", "lin_scenepoint"

    def __init__(self, n_feat_global_in, n_feat_scenepoint_in_out, n_hidden_layers_scenepoint_update=0,
                 use_norm_global2scenepoint_update=True):
        super().__init__(n_feat_global_in, n_feat_scenepoint_in_out, n_hidden_layers_scenepoint_update,
                         use_norm_global2scenepoint_update)


class GraphAttnSfMGlobalFeatureUpdate(Module):
    """layers.py:723-870."""

    def __init__(self, n_feat_proj_in, n_feat_scenepoint_out, n_feat_view_out, n_feat_proj2scenepoint_agg=None,
                 n_feat_proj2view_agg=None, n_feat_global_out=None, n_feat_scenepoint2global_agg=None,
                 n_feat_view2global_agg=None, output_global=True, n_heads=1, stateful=True,
                 global2view_and_global2scenepoint_enabled=True, n_hidden_layers_scenepoint_update=0,
                 n_hidden_layers_view_update=0, n_hidden_layers_global_update=0):
        super().__init__()
        self.n_feat_proj_in = n_feat_proj_in
        self.output_global = output_global
        self.global2view_and_global2scenepoint_enabled = global2view_and_global2scenepoint_enabled
        self.proj2view = Proj2View(n_feat_proj_in, n_feat_view_out, n_heads, stateful, True, n_feat_proj2view_agg,
                                   n_hidden_layers_view_update)
        self.proj2scenepoint = Proj2ScenePoint(n_feat_proj_in, n_feat_scenepoint_out, n_heads, stateful, True,
                                               n_feat_proj2scenepoint_agg, n_hidden_layers_scenepoint_update)
        if output_global or global2view_and_global2scenepoint_enabled:
            assert n_feat_global_out is not None and n_feat_global_out % n_heads == 0
            self.view_and_scenepoint2global = ViewAndScenePoint2Global(
                n_feat_scenepoint_out, n_feat_view_out, n_feat_global_out, n_heads, stateful, True,
                n_feat_scenepoint2global_agg, n_feat_view2global_agg, n_hidden_layers_global_update)
        if global2view_and_global2scenepoint_enabled:
            self.global2view = Global2View(n_feat_global_out, n_feat_view_out, n_hidden_layers_view_update)
            self.global2scenepoint = Global2ScenePoint(n_feat_global_out, n_feat_scenepoint_out,
                                                       n_hidden_layers_scenepoint_update)

    def fusable(self):
        """Edge side expressible with the fused 32-wide kernels (every GASFM conf, blocks >= 1)."""
        ok = True
        for m in (self.proj2scenepoint, self.proj2view):
            c = m.graph_conv
            ok &= c.in_channels == 32 and c.heads * c.out_channels == 32 and c.lin_l.bias is not None
            ok &= c.bias is not None
        return bool(ok)

    def fusable0(self):
        """Block-0 shape: 2-wide inputs, H*C = 4 per direction (every GASFM conf)."""
        ok = True
        for m in (self.proj2scenepoint, self.proj2view):
            c = m.graph_conv
            ok &= c.in_channels == 2 and c.heads * c.out_channels == 4 and c.lin_l.bias is not None
            ok &= c.bias is not None
        return bool(ok)

    def lin_l_pair(self):
        """(point lin_l weight, bias), (camera lin_l weight, bias): XL = [point | camera]."""
        a, b = self.proj2scenepoint.graph_conv.lin_l, self.proj2view.graph_conv.lin_l
        return (a.weight, a.bias), (b.weight, b.bias)

    def lin_l_stack(self):
        a, b = self.proj2scenepoint.graph_conv.lin_l, self.proj2view.graph_conv.lin_l
        return torch.cat([a.weight, b.weight], 0), torch.cat([a.bias, b.bias], 0)

    def prologue(self, P, plans, ln=None, Wp=None):
        """(XL, token) of EdgePrologueFn on P, where the fused prologue + camera attention does not
        apply.  ln / Wp: the block's LayerNorm and lin_proj weight; none for the final update."""
        (W, b), (W2, b2) = self.lin_l_pair()
        ln_w, ln_b, eps = (ln.weight, ln.bias, ln.eps) if ln is not None else (None, None, 1e-5)
        return EdgePrologueFn.apply(P, ln_w, ln_b, W, b, Wp, eps, plans["proj2scenepoint"].pos, W2, b2)

    def forward_fused(self, XL, plans, prev_pt=None, prev_view=None, prev_glob=None, carry=None, pfu=None, nxt=None,
                      attend=None):
        """Node side of the update given XL = [lin_l_point(P_hat) | lin_l_camera(P_hat)] [E, 64]
        (point half in point-segment order when the point plan has pos), or attend(XRp, XRc) ->
        (point aggregates, camera aggregates) (the fused prologue + camera attention, EdgeCamAttend).
        carry: the forward's BlockCarry (its docstring lists what travels); pfu / nxt: this block's
        projection-feature update and the next block's (or the final) GraphAttnSfMGlobalFeatureUpdate,
        whose Proj2ScenePoint and Proj2View are the hubs' next-block consumers (None: no next consumer)."""
        sp, sv = self.proj2scenepoint, self.proj2view
        pp, pc = plans["proj2scenepoint"], plans["proj2view"]
        shard = plans.get("_shard")
        if carry is not None and carry.XRp is not None:
            XRp, prev_pt = carry.take("XRp"), carry.take("pts_skip")
        else:
            XRp = sp.target_rows(prev_pt, pp.num_targets)
        cams = _cam_sharded(shard)
        if carry is not None and carry.XRc is not None:  # wrapped for the shard boundary by _edge_terms
            XRc, prev_view = carry.take("XRc"), carry.take("view_skip")
        else:
            if cams and prev_view is not None:
                raise RuntimeError("camera-sharded execution needs the fused view hubs (stateful block without carry)")
            XRc = replicated_to_local(sv.target_rows(prev_view, pc.num_targets), shard)
        cp, cc = sp.graph_conv, sv.graph_conv
        hubs = carry is not None and self.output_global and nxt is not None
        vsg = self.view_and_scenepoint2global if hubs else None
        hp = point_block.hub_params(pfu, vsg.graph_conv_scenepoint2global, nxt.proj2scenepoint) if hubs else None
        if attend is not None:
            agg_p, agg_c = attend(XRp, XRc)
        else:
            agg_p, agg_c = DualAttentionFn.apply(XL, XRp, XRc, cp.att, cc.att, cp.bias, cc.bias, pp, pc, cp.heads,
                                                 cp.negative_slope, plans.get("_partial", {}).get("proj2view"), shard,
                                                 pp.pos is not None)
        exch = None
        if cams:  # this rank's camera rows only from here on (distributed.py, camera sharding)
            from .distributed import BlockExchange, own_rows
            if hubs and self._exchange_ok(vsg):
                cvg, csg = vsg.graph_conv_view2global, vsg.graph_conv_scenepoint2global
                exch = BlockExchange(shard, cvg.att.numel(), csg.att.numel(), csg.heads, agg_c.device)
            agg_c = own_rows(agg_c, shard, exch)
        view = sv.tail(agg_c, prev_view, exch=exch)
        if hubs:
            hv = view_block.hub_params(pfu, vsg.graph_conv_view2global, nxt.proj2view)
            if hv is not None and view_block._rows_ok(view, view.shape[1]):
                skip, SV, XLv, XRn = view_block.hub(view, hv, getattr(self, "_proj_bf16", False), packed=cams,
                                                    out=exch.rows_out() if exch is not None else None)
                if exch is not None:  # SV and XR of every rank travel with the global convs' partial rows
                    carry.exch, carry.rows_own = exch, (SV, XRn)
                else:
                    if cams:  # every rank's edges read all cameras' SV and XR: one all-gather
                        from .distributed import gather_rows
                        SV, XRn = gather_rows(shard, SV, XRn)
                    carry.XRc, carry.SV = XRn, SV
                carry.view_skip, carry.XLv2g = skip, XLv
            elif cams:
                raise RuntimeError("camera-sharded execution needs the fused view hub shapes")
        if hp is not None and point_block.FUSED_TAIL_HUB and point_block.tail_fusable(sp, agg_p, prev_pt):
            # the point tail and hub as one forward launch (round 6, PointTailHubFn)
            pts, carry.pts_skip, carry.SA, carry.XLs2g, carry.XRp = point_block.tail_hub(sp, agg_p, prev_pt, hp)
        else:
            pts = sp.tail(agg_p, prev_pt)
            if hp is not None and point_block._rows_ok(pts, point_block.P_W):
                carry.pts_skip, carry.SA, carry.XLs2g, carry.XRp = point_block.hub(pts, hp)
        return self._finish(pts, view, plans, prev_glob, carry, pfu, nxt)

    def _exchange_ok(self, vsg):
        """The merged block exchange applies: both global convs on the fused kernels' shapes (H = 4,
        C in {256, 16}, global_attn.hip) and the fused view hub's 32-wide SV / XR."""
        cvg, csg = vsg.graph_conv_view2global, vsg.graph_conv_scenepoint2global
        return (cvg.heads == 4 and csg.heads == 4 and cvg.att.numel() in (64, 1024) and csg.att.numel() in (64, 1024)
                and cvg.negative_slope == csg.negative_slope and cvg.bias is not None and csg.bias is not None)

    def cam_fusable(self, plans):
        """The fused prologue + camera attention (EdgeCamFn) applies: both convs H = 4, C = 8, and
        the camera plan over the camera-major edges themselves (no permutation)."""
        cp, cc = self.proj2scenepoint.graph_conv, self.proj2view.graph_conv
        return (EDGE_CAM and cc.heads == 4 and cc.out_channels == 8 and cp.heads == 4 and cp.out_channels == 8
                and plans["proj2view"].perm is None)

    def forward_plan(self, P_hat, plans, prev_pt=None, prev_view=None, prev_glob=None):
        shard = plans.get("_shard")
        pts = self.proj2scenepoint.forward_plan(P_hat, plans["proj2scenepoint"], prev_pt)
        view = self.proj2view.forward_plan(P_hat, plans["proj2view"], prev_view,
                                           plans.get("_partial", {}).get("proj2view"), shard)
        return self._finish(pts, view, plans, prev_glob)

    def _finish(self, pts, view, plans, prev_glob, carry=None, pfu=None, nxt=None):
        glob = None
        if self.output_global or self.global2view_and_global2scenepoint_enabled:
            chain = None
            nv = nxt.view_and_scenepoint2global if nxt is not None and nxt.output_global else None
            if GLOBAL_CHAIN and carry is not None and pfu is not None and self.output_global:
                chain = dense.chain_params(self.view_and_scenepoint2global, pfu, nv)
            part = plans.get("_partial", {})
            glob, rows = self.view_and_scenepoint2global.forward_plan(
                view, pts, plans["view2global"], plans["scenepoint2global"], prev_glob, part.get("scenepoint2global"),
                plans.get("_shard"), part.get("view2global"), chain, carry)
            if rows is not None:
                carry.SV, carry.XRc = rows
            if isinstance(glob, tuple):  # GlobalChainFn: (g, SG[, XRv, XRp]), g with its consumers' rows
                glob, carry.SG, *xr = glob
                carry.pre_glob = (*xr, glob) if xr else None
            elif carry is not None and nv is not None and dense._gvec_ok(glob, glob.shape[1]):
                hg = dense.global_hub_params(pfu, nv)
                if hg is not None:
                    skip, carry.SG, XRv, XRp = dense.GlobalHubFn.apply(glob, *hg)
                    carry.pre_glob = (XRv, XRp, skip)
        if self.global2view_and_global2scenepoint_enabled:
            pts = self.global2scenepoint(glob, pts)
            view = self.global2view(glob, view)
        return pts, view, glob


class EdgeCamAttend:
    """attend callback of gfu.forward_fused: EdgeCamFn on P (lin_l of both convs, the camera
    attention; XLp written in point order) then the point attention on XLp.  The call sets .P, the
    block's input rows (P, or the output of a PendingEpilogue P), and .token, the prologue's (see
    EdgePrologueFn).  dwp: EdgeCamFn's, it returns the block's lin_proj gradient (P0: its skip input)."""

    def __init__(self, gfu, P, ln_w, ln_b, eps, Wp, plans, P0=None, dwp=False):
        (Wpt, bpt), (Wc, bc) = gfu.lin_l_pair()
        self.P, self.token, self.pp, self.cp = P, None, plans["proj2scenepoint"], gfu.proj2scenepoint.graph_conv
        cc = gfu.proj2view.graph_conv
        self.cam = CamArgs(ln_w=ln_w, ln_b=ln_b, Wpt=Wpt, bpt=bpt, Wc=Wc, bc=bc, Wp=Wp, eps=eps, pos=self.pp.pos,
                           XR=None, att=cc.att, bias=cc.bias, plan=plans["proj2view"], heads=cc.heads,
                           slope=cc.negative_slope, plan_partial=plans.get("_partial", {}).get("proj2view"),
                           shard=plans.get("_shard"), P0=P0, dwp=dwp)

    def __call__(self, XRp, XRc):
        pp, cp, cam = self.pp, self.cp, self.cam._replace(XR=XRc)
        if isinstance(self.P, PendingEpilogue) and self.P.block0 and cam.ln_w is None:
            self.P = self.P.materialize()  # the block-0 seam is built for a LayerNorm prologue only
        if isinstance(self.P, PendingEpilogue):  # the previous block's epilogue in the same kernel
            self.P, XLp, agg_c, self.token = self.P.seam(cam)
        else:
            XLp, agg_c, self.token = EdgeCamFn.apply(self.P, *cam)
        agg_p = GatAttentionFn.apply(XLp, XRp, cp.att, cp.bias, pp, cp.heads, cp.negative_slope,
                                     pp.pos is not None)[0]
        return agg_p, agg_c


class GraphAttnSfMProjectionFeatureUpdate(Module):
    """layers.py:873-956: Δ_e = (lin_proj(x_e) + Wp·p̂[pt_e] + Wv·v̂[cam_e] + Wg·ĝ) / 4."""

    def __init__(self, n_feat_proj_in, n_feat_scenepoint_in, n_feat_view_in, n_feat_global_in, n_feat_proj_out,
                 n_hidden_layers_proj_update=0, normalize_global_features=True):
        super().__init__()
        self.n_feat_proj_out = n_feat_proj_out
        self.n_hidden_layers_proj_update = n_hidden_layers_proj_update
        self.normalize_global_features = normalize_global_features
        if normalize_global_features:
            self.scenepoint_norm_layer = LayerNorm(n_feat_scenepoint_in)
            self.view_norm_layer = LayerNorm(n_feat_view_in)
            self.global_norm_layer = LayerNorm(n_feat_global_in)
        self.lin_proj = Linear(n_feat_proj_in, n_feat_proj_out)
        self.lin_scenepoint = Linear(n_feat_scenepoint_in, n_feat_proj_out, bias=False)
        self.lin_view = Linear(n_feat_view_in, n_feat_proj_out, bias=False)
        self.lin_global = Linear(n_feat_global_in, n_feat_proj_out, bias=False)
        if n_hidden_layers_proj_update > 0:
            self.mlp = get_linear_layers(n_hidden_layers_proj_update * [n_feat_proj_out] + [n_feat_proj_out],
                                         norm=False)

    def node_terms(self, pts, view, glob, sp=None, sv=None, sg=None):
        """sp / sv / sg: the point / view / global terms when the hubs already computed them."""
        if self.normalize_global_features:
            return (sp if sp is not None else dense.ln_relu_linear(pts, self.scenepoint_norm_layer, self.lin_scenepoint),
                    sv if sv is not None else dense.ln_relu_linear(view, self.view_norm_layer, self.lin_view),
                    sg if sg is not None else dense.ln_relu_linear(glob, self.global_norm_layer, self.lin_global))
        return dense.linear(pts, self.lin_scenepoint), dense.linear(view, self.lin_view), \
            dense.linear(glob, self.lin_global)


class ProjLayer(Module):
    def __init__(self, n_feat_proj_in, n_feat_proj_out):
        super().__init__()
        self.lin_proj = Linear(n_feat_proj_in, n_feat_proj_out)


class GraphAttnSfMLayer(Module):
    """layers.py:148-263."""

    def __init__(self, n_feat_proj_in, n_feat_proj_out, n_feat_scenepoint_hidden, n_feat_view_hidden,
                 n_feat_global_hidden, n_feat_proj2scenepoint_agg=None, n_feat_proj2view_agg=None,
                 n_feat_scenepoint2global_agg=None, n_feat_view2global_agg=None, use_norm_proj_update=True,
                 add_residual_skipconn_proj_update=True, n_feat_skipconn_init_projfeat_in=None, n_heads=1,
                 stateful=True, global2view_and_global2scenepoint_enabled=True, n_hidden_layers_scenepoint_update=0,
                 n_hidden_layers_view_update=0, n_hidden_layers_global_update=0, n_hidden_layers_proj_update=0):
        super().__init__()
        self.use_norm_proj_update = use_norm_proj_update
        self.add_residual_skipconn_proj_update = add_residual_skipconn_proj_update
        self.add_skipconn_from_init_projfeat = n_feat_skipconn_init_projfeat_in is not None
        n_skip_in = n_feat_skipconn_init_projfeat_in or 0
        if use_norm_proj_update:
            self.prev_projfeat_norm_layer = LayerNorm(n_feat_proj_in)
        self.global_feature_update = GraphAttnSfMGlobalFeatureUpdate(
            n_feat_proj_in, n_feat_scenepoint_hidden, n_feat_view_hidden, n_feat_proj2scenepoint_agg,
            n_feat_proj2view_agg, n_feat_global_hidden, n_feat_scenepoint2global_agg, n_feat_view2global_agg,
            True, n_heads, stateful, global2view_and_global2scenepoint_enabled, n_hidden_layers_scenepoint_update,
            n_hidden_layers_view_update, n_hidden_layers_global_update)
        self.projection_feature_update = GraphAttnSfMProjectionFeatureUpdate(
            n_feat_proj_in + n_skip_in, n_feat_scenepoint_hidden, n_feat_view_hidden, n_feat_global_hidden,
            n_feat_proj_out, n_hidden_layers_proj_update, True)
        self.skip_projection = None
        if add_residual_skipconn_proj_update and n_feat_proj_in != n_feat_proj_out:
            if use_norm_proj_update:
                self.residual_skipconn_proj_norm_layer = LayerNorm(n_feat_proj_in)
            self.skip_projection = ProjLayer(n_feat_proj_in, n_feat_proj_out)

    last_route = None  # the route the last forward_plan took: "fused", "fused0", "wide" or "unfused"

    def fusable(self):
        pfu = self.projection_feature_update
        w = pfu.lin_proj.weight
        return (self.use_norm_proj_update and self.add_residual_skipconn_proj_update and self.skip_projection is None
                and pfu.n_hidden_layers_proj_update == 0 and pfu.normalize_global_features
                and w.shape[0] == 32 and w.shape[1] in (32, 34)
                and (w.shape[1] == 34) == self.add_skipconn_from_init_projfeat
                and self.prev_projfeat_norm_layer.normalized_shape == (32,)
                and self.global_feature_update.fusable())

    def fusable0(self):
        pfu = self.projection_feature_update
        w = pfu.lin_proj.weight
        return (self.use_norm_proj_update and self.add_residual_skipconn_proj_update
                and self.skip_projection is not None and not self.add_skipconn_from_init_projfeat
                and pfu.n_hidden_layers_proj_update == 0 and pfu.normalize_global_features
                and tuple(w.shape) == (32, 2) and tuple(self.skip_projection.lin_proj.weight.shape) == (32, 2)
                and self.prev_projfeat_norm_layer.normalized_shape == (2,)
                and self.global_feature_update.fusable0())

    def fusable_wide(self):
        """The 32 -> 128 last block of a depth conf: LayerNorm and residual on, the LayerNorm'd skip
        projection [128, 32], lin_proj [128, 34] (init-feature skip) or [128, 32], no hidden layers."""
        pfu = self.projection_feature_update
        w = pfu.lin_proj.weight
        if not (self.use_norm_proj_update and self.add_residual_skipconn_proj_update
                and self.skip_projection is not None):
            return False
        la, lb, sk = self.prev_projfeat_norm_layer, self.residual_skipconn_proj_norm_layer, self.skip_projection.lin_proj
        return (pfu.n_hidden_layers_proj_update == 0 and pfu.normalize_global_features
                and tuple(w.shape) in ((128, 34), (128, 32))
                and (w.shape[1] == 34) == self.add_skipconn_from_init_projfeat
                and tuple(sk.weight.shape) == (128, 32) and sk.bias is not None and pfu.lin_proj.bias is not None
                and la.normalized_shape == (32,) and lb.normalized_shape == (32,) and la.eps == lb.eps
                and la.weight is not None and lb.weight is not None and la.bias is not None and lb.bias is not None
                and self.global_feature_update.fusable())

    def forward_fused_wide(self, P, plans, edges, prev_pt, prev_view, prev_glob, P0, carry=None):
        """The 32 -> 128 last block with the fused HIP edge kernels: the attention half as forward_fused
        (EdgeCamFn without the lin_proj gradient or a token gradient; a PendingEpilogue P runs in its
        kernel, SeamFn), then edge_block.WideEpilogueFn.  Returns the materialised P' [E, 128]."""
        la, lb = self.prev_projfeat_norm_layer, self.residual_skipconn_proj_norm_layer
        gfu, pfu = self.global_feature_update, self.projection_feature_update
        P0e = P0 if self.add_skipconn_from_init_projfeat else None
        if gfu.cam_fusable(plans):
            attend = EdgeCamAttend(gfu, P, la.weight, la.bias, la.eps, None, plans)
            pts, view, glob = gfu.forward_fused(None, plans, prev_pt, prev_view, prev_glob, carry, attend=attend)
            P = attend.P
        else:
            P = materialize(P)
            XL, _ = gfu.prologue(P, plans, la)
            pts, view, glob = gfu.forward_fused(XL, plans, prev_pt, prev_view, prev_glob, carry)
        sp, sv, sg = _edge_terms(pfu, pts, view, glob, plans, carry)
        sk = self.skip_projection.lin_proj
        Pn = WideEpilogueFn.apply(P, P0e, sp, sv, sg, pfu.lin_proj.weight, pfu.lin_proj.bias, sk.weight, sk.bias,
                                  la.weight, la.bias, lb.weight, lb.bias, la.eps, edges)
        return Pn, pts, view, glob

    def forward_fused0(self, P, plans, edges, carry=None, nxt=None):
        """Block 0 (2-wide inputs, projected residual) with the block-0 HIP edge kernels."""
        la, lb = self.prev_projfeat_norm_layer, self.residual_skipconn_proj_norm_layer
        gfu, pfu = self.global_feature_update, self.projection_feature_update
        W, b = gfu.lin_l_stack()
        pp = plans["proj2scenepoint"]
        perm = pp.perm if pp.pos is not None and pp.src_rows == pp.num_edges else None
        XL, token = Block0PrologueFn.apply(P.contiguous(), la.weight, la.bias, W, b, la.eps, pp.pos, perm)
        pts, view, glob = gfu.forward_fused(XL, plans, carry=carry, pfu=pfu, nxt=nxt)
        sp, sv, sg = _edge_terms(pfu, pts, view, glob, plans, carry)
        sk = self.skip_projection.lin_proj
        epi = PendingEpilogue(Epilogue0Args(P.contiguous(), token, sp, sv, sg, pfu.lin_proj.weight, pfu.lin_proj.bias,
                                            la.weight, la.bias, lb.weight, lb.bias, sk.weight, sk.bias, la.eps, edges))
        # left pending, it runs with block 1's prologue (edge_block.Seam0Fn)
        return (epi if EDGE_SEAM and EDGE_SEAM0 and epi.seam_ok() else epi.materialize()), pts, view, glob

    def forward_fused(self, P, plans, edges, prev_pt, prev_view, prev_glob, P0, carry=None, nxt=None):
        """Blocks >= 1 with the fused HIP edge kernels (see gasfm_amd/edge_block.py).  P may be the
        previous block's PendingEpilogue; with EDGE_SEAM this block's own epilogue is returned
        pending as well (the caller's next consumer runs or materializes it)."""
        ln = self.prev_projfeat_norm_layer
        gfu, pfu = self.global_feature_update, self.projection_feature_update
        P0e = P0 if self.add_skipconn_from_init_projfeat else None
        dwp = False
        if gfu.cam_fusable(plans):
            # the block's lin_proj gradient from its edge_cam_pbwd (edge_block.EPI_FOLD)
            dwp = edge_block.EPI_FOLD and ln.weight is not None
            attend = EdgeCamAttend(gfu, P, ln.weight, ln.bias, ln.eps, pfu.lin_proj.weight, plans,
                                   P0e if dwp else None, dwp)
            pts, view, glob = gfu.forward_fused(None, plans, prev_pt, prev_view, prev_glob, carry, pfu, nxt, attend)
            P, token = attend.P, attend.token
        else:
            P = materialize(P)
            XL, token = gfu.prologue(P, plans, ln, pfu.lin_proj.weight)
            pts, view, glob = gfu.forward_fused(XL, plans, prev_pt, prev_view, prev_glob, carry, pfu, nxt)
        sp, sv, sg = _edge_terms(pfu, pts, view, glob, plans, carry)
        epi = PendingEpilogue(EpilogueArgs(P, P0e, token, sp, sv, sg, pfu.lin_proj.weight, pfu.lin_proj.bias, ln.weight,
                                           ln.bias, ln.eps, edges, dwp))
        return (epi if EDGE_SEAM and epi.seam_ok() else epi.materialize()), pts, view, glob

    def forward_plan(self, P, plans, edges, prev_pt=None, prev_view=None, prev_glob=None, P0=None, carry=None,
                     nxt=None):
        """P [E, F_in] edge features (cam-major) -> (P' [E, F_out], pts, view, glob).

        carry / nxt: see GraphAttnSfMGlobalFeatureUpdate.forward_fused (fused CUDA path only).  On
        the fused path P and P' may be PendingEpilogue handles (edge_block.SeamFn)."""
        if (isinstance(P, PendingEpilogue) or P.is_cuda) and self.fusable():
            self.last_route = "fused"
            return self.forward_fused(P, plans, edges, prev_pt, prev_view, prev_glob, P0, carry, nxt)
        if EDGE_WIDE and plans.get("_shard") is None and self.fusable_wide() \
                and (isinstance(P, PendingEpilogue)
                     or (P.is_cuda and P.dtype == torch.float32 and P.dim() == 2 and P.shape[1] == 32)):
            self.last_route = "wide"
            return self.forward_fused_wide(P, plans, edges, prev_pt, prev_view, prev_glob, P0, carry)
        P = materialize(P)
        if P.is_cuda and prev_pt is None and prev_view is None and prev_glob is None and self.fusable0():
            self.last_route = "fused0"
            return self.forward_fused0(P, plans, edges, carry, nxt)
        self.last_route = "unfused"
        if carry is not None and carry.pending():
            raise RuntimeError("point hub outputs pending for a block on the unfused path")
        if self.use_norm_proj_update:
            P_hat = edge_ops.layer_norm_relu(P, self.prev_projfeat_norm_layer)
        else:
            P_hat = F.relu(P)
        pts, view, glob = self.global_feature_update.forward_plan(P_hat, plans, prev_pt, prev_view, prev_glob)
        pfu = self.projection_feature_update
        x_cat = torch.cat([P_hat, P0], dim=1) if self.add_skipconn_from_init_projfeat else P_hat
        sp, sv, sg = pfu.node_terms(pts, view, glob)
        shard = plans.get("_shard")
        sv, sg = replicated_to_local_n(shard, sv, sg)
        sv, sg = _fold_global(sv, sg, plans)
        delta = edge_ops.projection_update(x_cat, pfu.lin_proj, sp, sv, sg, edges)
        if pfu.n_hidden_layers_proj_update > 0:
            delta = pfu.mlp(F.relu(delta))
        if not self.add_residual_skipconn_proj_update:
            return delta, pts, view, glob
        skip = P
        if self.skip_projection is not None:
            if self.use_norm_proj_update:
                skip = edge_ops.layer_norm_relu(skip, self.residual_skipconn_proj_norm_layer)
            skip = dense.linear(skip, self.skip_projection.lin_proj)  # as edge_ops.projection_update
        return skip + delta, pts, view, glob


class EmbeddingLayer(Module):
    """layers.py:992-1015 with pos_emb_n_freq = 0 (every GASFM conf, e.g. learning conf :60)."""

    def __init__(self, pos_emb_n_freq, in_dim, post_embed_proj_dim=None):
        super().__init__()
        if pos_emb_n_freq > 0:
            raise NotImplementedError("positional embedding (pos_emb_n_freq > 0) is off in all GASFM confs")
        self.embed, self.d_out = Identity(), in_dim
        self.post_embed_lin = None
        if post_embed_proj_dim is not None:
            d = self.d_out if post_embed_proj_dim == -1 else post_embed_proj_dim
            self.post_embed_lin = Linear(self.d_out, d)
            self.d_out = d

    def forward(self, values):
        x = self.embed(values)
        return self.post_embed_lin(x) if self.post_embed_lin is not None else x


class EdgeIndex:
    """int32 camera / point id of every edge (cam-major order), on the model's device."""

    def __init__(self, cam, pt, m, n, plans):
        self.cam, self.pt, self.m, self.n = cam, pt, m, n
        self.plans = plans


def _plan_from_wrapper(name, w, device):
    """Plan for a reference-style wrapper (no .plan attribute): built once, cached on it."""
    cache = w.__dict__.setdefault("_gasfm_plans", {})
    key = str(device)
    if key not in cache:
        vi = w.valid_indices.cpu()
        if name in ("proj2view", "proj2scenepoint"):
            plan = AttnPlan.from_targets(vi[w.non_agg_dim], w.n_agg_nodes)
        else:
            src = vi[w.agg_dim]
            rows = (w.m, w.n)[w.agg_dim]
            plan = AttnPlan.from_targets(torch.zeros_like(src), 1, src=src, src_rows=rows,
                                         max_piece=8 if name == "view2global" else max(256, -(-src.numel() // 1024)))
        plan = plan.to(device)
        plan.tag = name
        cache[key] = plan
    return cache[key]


def scene_plans(data, device):
    plans = {}
    for name in GRAPH_NAMES:
        w = data.graph_wrappers[name]
        plan = getattr(w, "plan", None)
        if plan is None:
            plan = _plan_from_wrapper(name, w, device)
        elif plan.device != device:
            raise ValueError(f"graph '{name}' plan is on {plan.device}; move the scene with data.to({device})")
        plans[name] = plan
    return plans


class Embed2Fn(torch.autograd.Function):
    """P = values W^T + b for the Linear(2, 2) input embedding (layers.py:992-1015,
    graph_attn_sfm.py:53) in one streaming kernel each way (csrc/embed.hip) instead of a
    hipBLASLt tile sweep and a split-K batched GEMM over E rows."""

    @staticmethod
    def forward(ctx, x, W, b):
        x = x.contiguous()
        y = torch.empty_like(x)
        _native.embed2_fwd(x, W.contiguous(), b.contiguous(), y)
        ctx.save_for_backward(x, W)
        ctx.defer = _native.defer_token(W, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dW, db = _native.embed2_bwd(x, dy, ctx.defer)
        return (dy @ W if ctx.needs_input_grad[0] else None), dW, db


def _embed(values, lin):
    if (values.is_cuda and values.dtype == torch.float32 and values.dim() == 2 and values.shape[1] == 2
            and lin.in_features == 2 and lin.out_features == 2 and lin.bias is not None):
        return Embed2Fn.apply(values, lin.weight, lin.bias)
    return dense.linear(values, lin)


class FanOutFn(torch.autograd.Function):
    """x -> n identical views; the backward sums the consumers' gradients in one kernel
    (gasfm_sum_n) where autograd would run n - 1 full-size adds."""

    @staticmethod
    def forward(ctx, x, n):
        # a consumer that sends no gradient stays None (not a zero-filled [E, 2] tensor summed in)
        ctx.set_materialize_grads(False)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g.contiguous() for g in gs if g is not None]
        if not gs:
            return None, None
        return (gs[0] if len(gs) == 1 else _native.sum_n(gs)), None


# Bumped by every parameter / submodule registration in the process (GraphAttnSfMNet._param_list's
# cache key): a parameter replaced deep in the tree (module.weight = Parameter(...)) re-lists them.
_TREE_VERSION = [0]


def _bump_tree_version(*args):
    _TREE_VERSION[0] += 1


torch.nn.modules.module.register_module_parameter_registration_hook(_bump_tree_version)
torch.nn.modules.module.register_module_module_registration_hook(_bump_tree_version)


class BaseNet(Module):
    """baseNet.py:8-92: the output format of a conf and the decoding of the head outputs, shared by
    GraphAttnSfMNet and setofset.SetOfSetNet."""

    def __init__(self, conf):
        super().__init__()
        self.calibrated = conf.get_bool("dataset.calibrated")
        self.normalize_output = conf.get_string("model.view_head.normalize_output", default=None)
        self.rot_representation = conf.get_string("model.view_head.rot_representation", default="quat")
        self.soft_sign = torch.nn.Softsign()
        if self.calibrated and self.rot_representation == "6d":
            self.out_channels = 9
        elif self.calibrated and self.rot_representation == "quat":
            self.out_channels = 7
        elif self.calibrated and self.rot_representation == "svd":
            self.out_channels = 12
        elif not self.calibrated:
            self.out_channels = 12
        else:
            raise ValueError("Illegal output format")

    @staticmethod
    def extract_scenepoint_outputs(n_out):
        """[3, n] head output -> {"pts3D": [4, n]} (ones-padded)."""
        return {"pts3D": torch.cat([n_out, torch.ones(1, n_out.shape[1], dtype=n_out.dtype, device=n_out.device)])}

    def extract_view_outputs(self, x):
        if not self.calibrated:
            Ps = x.reshape(-1, 3, 4)
            if self.normalize_output == "Chirality":
                Ps = Ps * (torch.sign(Ps[:, 0:3, 0:3].det()) / Ps[:, 2, 0:3].norm(dim=1)).reshape(-1, 1, 1)
            elif self.normalize_output == "Differentiable Chirality":
                Ps = Ps * (self.soft_sign(Ps[:, 0:3, 0:3].det() * 10e3) / Ps[:, 2, 0:3].norm(dim=1)).reshape(-1, 1, 1)
            elif self.normalize_output == "Frobenius":
                Ps = Ps / Ps.norm(dim=(1, 2), p="fro", keepdim=True)
            return {"Ps_norm": Ps}
        if self.rot_representation == "6d":
            R = rotation_6d_to_matrix(x[:, :6])
        elif self.rot_representation == "svd":
            R = project_to_rot(x[:, :9].reshape(-1, 3, 3))
        elif x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 7:
            return {"Ps_norm": QuatPoseFn.apply(x)}
        else:
            R = quaternion_to_matrix(x[:, :4])
        return {"Ps_norm": torch.cat((R, x[:, -3:].unsqueeze(-1)), dim=-1)}


def require_gasfm(net, what):
    """The batched, captured-trainer and sharded paths are built around GraphAttnSfMNet's blocks."""
    if not isinstance(net, GraphAttnSfMNet):
        raise TypeError(f"{what} supports GraphAttnSfMNet only, got {type(net).__name__}")


def scene_edge_index(data, device):
    """The EdgeIndex (int32 camera / point ids, the four plans) of a scene on device, cached on its
    SparseMat; accepts the reference's SceneData and this package's (host- or device-built)."""
    x = data.x
    cache = x.__dict__.setdefault("_gasfm_edges", {})
    key = (str(device), x.indices.data_ptr())
    if key not in cache:
        cache.clear()
        idx = x.indices.to(device)
        plans = scene_plans(data, device)
        soc = getattr(data, "scene_of_cam", None)
        if soc is not None:  # a SceneBatch (batch.py): one global row per scene
            plans["_scene_of_cam"] = soc.to(device)
            off = tuple(getattr(data, k, None) for k in ("cam_off", "pt_off", "edge_off"))
            if all(o is not None for o in off):  # the scenes' row ranges (host lists): setofset's per-scene means
                plans["_scene_off"] = off
        cache[key] = EdgeIndex(idx[0].to(torch.int32).contiguous(), idx[1].to(torch.int32).contiguous(),
                               x.shape[0], x.shape[1], plans)
    return cache[key]


class GraphAttnSfMNet(BaseNet):
    """graph_attn_sfm.py:8-185 (BaseNet: baseNet.py:8-92)."""

    def __init__(self, conf, batchnorm=False):
        super().__init__(conf)
        g = lambda k, **kw: conf.get_int("model." + k, **kw)
        num_layers, n_heads = g("num_layers"), g("n_heads")
        n_feat_proj, n_feat_sp = g("n_feat_proj"), g("n_feat_scenepoint")
        n_feat_view, n_feat_glob = g("n_feat_view"), g("n_feat_global")
        aggs = dict(n_feat_proj2scenepoint_agg=g("n_feat_proj2scenepoint_agg", default=None),
                    n_feat_proj2view_agg=g("n_feat_proj2view_agg", default=None),
                    n_feat_scenepoint2global_agg=g("n_feat_scenepoint2global_agg", default=None),
                    n_feat_view2global_agg=g("n_feat_view2global_agg", default=None))
        hid = dict(n_hidden_layers_scenepoint_update=g("n_hidden_layers_scenepoint_update"),
                   n_hidden_layers_view_update=g("n_hidden_layers_view_update"),
                   n_hidden_layers_global_update=g("n_hidden_layers_global_update"))
        n_hidden_proj = g("n_hidden_layers_proj_update")
        pos_emb_n_freq = g("pos_emb_n_freq")
        use_norm = conf.get_bool("model.use_norm_proj_update")
        add_res = conf.get_bool("model.add_residual_skipconn_proj_update")
        self.add_skipconn_from_init_projfeat = conf.get_bool("model.add_skipconn_from_init_projfeat")
        self.stateful_global_features = conf.get_bool("model.stateful_global_features")
        g2v = conf.get_bool("model.global2view_and_global2scenepoint_enabled")
        self.depth_head_enabled = conf.get_bool("model.depth_head.enabled", default=False)
        self.view_head_enabled = conf.get_bool("model.view_head.enabled", default=False)
        self.scenepoint_head_enabled = conf.get_bool("model.scenepoint_head.enabled", default=False)
        self.batchnorm = batchnorm
        if batchnorm:
            raise NotImplementedError()
        n_feat_depth = conf.get_int("model.depth_head.n_feat") if self.depth_head_enabled else None
        # not a reference key: "bf16" runs the m x 1024 x 1024 camera-side GEMMs on the bf16 MFMA
        # kernel (BASELINE config 5); parameters and every other op stay fp32
        self._projection_precision = conf.get_string("model.projection_precision", default="fp32")

        self.embed = EmbeddingLayer(pos_emb_n_freq, 2, post_embed_proj_dim=-1)
        d_emb = self.embed.d_out
        self.n_feat_skipconn_init_projfeat_in = d_emb if self.add_skipconn_from_init_projfeat else 0
        self.equivariant_blocks = ModuleList()
        for i in range(num_layers):
            last = i == num_layers - 1
            self.equivariant_blocks.append(GraphAttnSfMLayer(
                d_emb if i == 0 else n_feat_proj,
                n_feat_depth if (self.depth_head_enabled and last) else n_feat_proj,
                n_feat_sp, n_feat_view, n_feat_glob, **aggs,
                use_norm_proj_update=use_norm, add_residual_skipconn_proj_update=add_res,
                n_feat_skipconn_init_projfeat_in=(self.n_feat_skipconn_init_projfeat_in
                                                  if i > 0 and self.add_skipconn_from_init_projfeat else None),
                n_heads=n_heads, stateful=False if i == 0 else self.stateful_global_features,
                global2view_and_global2scenepoint_enabled=g2v, **hid,
                n_hidden_layers_proj_update=n_hidden_proj))
        if self.view_head_enabled or self.scenepoint_head_enabled:
            if not self.view_head_enabled:
                raise NotImplementedError("final aggregation for scenepoint features alone")
            self.final_global_update = GraphAttnSfMGlobalFeatureUpdate(
                n_feat_depth if self.depth_head_enabled else n_feat_proj, n_feat_sp, n_feat_view, **aggs,
                n_feat_global_out=n_feat_glob, output_global=False, n_heads=n_heads,
                stateful=self.stateful_global_features, global2view_and_global2scenepoint_enabled=g2v, **hid)
        if self.depth_head_enabled:
            nh = conf.get_int("model.depth_head.n_hidden_layers")
            self.depth_head = get_linear_layers((1 + nh) * [n_feat_depth] + [1], norm=False)
        if self.view_head_enabled:
            nh = conf.get_int("model.view_head.n_hidden_layers")
            self.view_head = get_linear_layers((1 + nh) * [n_feat_view] + [self.out_channels], norm=False)
        if self.scenepoint_head_enabled:
            nh = conf.get_int("model.scenepoint_head.n_hidden_layers")
            self.scenepoint_head = get_linear_layers((1 + nh) * [n_feat_sp] + [3], norm=False)

        self.set_projection_precision(self._projection_precision)

    def set_projection_precision(self, precision):
        """"fp32" (default: the reference's precision) or "bf16": the camera-side D x D products
        (Proj2View's MLP, graph_conv_view2global.lin_l; layers.py:292-320, 352-358, 506-511) in
        bf16 on MFMA with fp32 accumulation, forward and backward, and the global node's chain
        (layers.py:497-533, 594-603, 928-935) on bf16 weight shadows (BASELINE config 5; call
        refresh_weight_shadows() after each optimizer step when the step is a captured graph)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError(f"projection precision {precision!r}: expected 'fp32' or 'bf16'")
        self._projection_precision = precision
        for mod in self.modules():
            mod._proj_bf16 = precision == "bf16"
        return self

    @staticmethod
    def refresh_weight_shadows():
        """Re-round the bf16 weight shadows (set_projection_precision("bf16")) from their weights:
        after an optimizer step whose forward/backward is replayed from a captured graph (an eager
        forward re-rounds a changed weight by itself)."""
        dense.refresh_weight_shadows()

    # ------------------------------------------------------------------ forward
    def edge_index_for(self, data, device):
        return scene_edge_index(data, device)

    last_carry = None  # the last forward's BlockCarry: the tests read that nothing stays pending in it
    last_routes = ()  # the route each block of the last forward took (GraphAttnSfMLayer.last_route)

    def forward_features(self, values, edges):
        """Block stack + final update on raw tensors; returns (P, pts, view) after the final update."""
        plans = edges.plans
        lin = self.embed.post_embed_lin
        P = _embed(values, lin) if lin is not None else self.embed(values)
        nb = len(self.equivariant_blocks)
        p0s = [P if self.add_skipconn_from_init_projfeat else None] * nb
        if self.add_skipconn_from_init_projfeat and P.is_cuda and P.requires_grad and torch.is_grad_enabled():
            # the embedded input feeds block 0 and every block's projection update (layers.py:245-251):
            # its gradient is summed in one pass instead of autograd's nb full-size adds
            views = FanOutFn.apply(P.contiguous(), nb + 1)
            P, p0s = views[0], list(views[1:])
        pts = view = glob = None
        sf = self.stateful_global_features
        heads = self.view_head_enabled or self.scenepoint_head_enabled
        fgu = self.final_global_update if heads else None
        final_fused = fgu is not None and values.is_cuda and fgu.fusable() and self.equivariant_blocks[-1].fusable()
        # nxt, the consumers of each block's hub outputs: the next block's (or the fused final update's)
        # Proj2ScenePoint / Proj2View; carry hands them forward
        carry = self.last_carry = BlockCarry() if (values.is_cuda and sf) else None
        blocks = list(self.equivariant_blocks)
        for i, blk in enumerate(blocks):
            if i + 1 < len(blocks):
                nxt = blocks[i + 1].global_feature_update if blocks[i + 1].fusable() else None
            else:
                nxt = fgu if final_fused else None
            prev = (pts, view, glob) if sf else (None, None, None)
            P, pts, view, glob = blk.forward_plan(P, plans, edges, *prev, P0=p0s[i], carry=carry, nxt=nxt)
        self.last_routes = tuple(blk.last_route for blk in blocks)
        if heads:
            args = (pts, view, glob) if sf else (None, None, None)
            pend = isinstance(P, PendingEpilogue)
            if (pend or P.is_cuda) and fgu.fusable() and fgu.cam_fusable(plans) and (pend or P.shape[1] == 32):
                # raw (un-normalised) projection features (graph_attn_sfm.py:141-148): no LN prologue;
                # a pending last-block epilogue runs in the same kernel (SeamFn)
                attend = EdgeCamAttend(fgu, P if pend else P.contiguous(), None, None, 1e-5, None, plans)
                pts, view, _ = fgu.forward_fused(None, plans, *args, carry=carry, attend=attend)
                P = attend.P
            else:
                P = materialize(P)
                if P.is_cuda and P.shape[1] == 32 and fgu.fusable():
                    pts, view, _ = fgu.forward_fused(fgu.prologue(P.contiguous(), plans)[0], plans, *args, carry=carry)
                else:
                    pts, view, _ = fgu.forward_plan(P, plans, *args)
        return materialize(P), pts, view

    # Weight-gradient column sums of the backward pass run as one batched launch at its end
    # (_native.param_colsum) when every parameter's .grad is unset at forward time (the usual
    # zero_grad(set_to_none=True) loop); gradient accumulation into existing .grad tensors
    # takes the immediate path.  False disables the batching.
    batch_weight_grads = True

    def _apply(self, *args, **kwargs):
        # .to() / .cuda() / .float() may replace Parameter objects without a registration hook
        # (torch.__future__.set_overwrite_module_params_on_conversion): re-list them afterwards
        out = super()._apply(*args, **kwargs)
        _bump_tree_version()
        return out

    def _param_list(self):
        """The parameters as a list, rebuilt only after a parameter or module was registered anywhere
        (torch's global registration hooks bump _TREE_VERSION): self.parameters() walks ~180 modules
        through nested generators, ~1.5 ms per eager step."""
        cache = self.__dict__.get("_plist_cache")
        if cache is None or cache[0] != _TREE_VERSION[0]:
            cache = (_TREE_VERSION[0], list(self.parameters()))
            self.__dict__["_plist_cache"] = cache
        return cache[1]

    def forward(self, data, shard=None, partial_plans=None):
        from . import _native
        values = data.x.values
        device = values.device
        edges = self.edge_index_for(data, device)
        if shard is not None:
            edges = copy.copy(edges)
            edges.plans = dict(edges.plans, _shard=shard, _partial=partial_plans)
        defer = (self.batch_weight_grads and values.is_cuda and torch.is_grad_enabled()
                 and all(p.grad is None for p in self._param_list()))
        with _native.deferring_param_grads(defer):
            return self._forward_outputs(data, values, edges, device)

    def _forward_outputs(self, data, values, edges, device):
        P, pts, view = self.forward_features(values, edges)
        pred = {}
        if self.depth_head_enabled:
            from .scene import SparseMat
            x = data.x
            # the fused 128-128-128-1 head (csrc/depth_head.hip) where it applies, else the Sequential as is
            d = depth_head_op.apply(self.depth_head, P) if depth_head_op.fusable(self.depth_head, P) \
                else self.depth_head(P)
            pred["depths"] = SparseMat(d, x.indices, x.cam_per_pts, x.pts_per_cam, [x.shape[0], x.shape[1], 1])
        if self.view_head_enabled:
            out = self.extract_view_outputs(dense.sequential(self.view_head, F.relu(view)))
            shard = edges.plans.get("_shard")
            if _cam_sharded(shard):  # this rank's camera rows -> all cameras (one all-gather)
                from .distributed import gather_rows
                out = {k: gather_rows(shard, v)[0] for k, v in out.items()}
            pred.update(out)
        if self.scenepoint_head_enabled and point_block.head_fusable(self.scenepoint_head, pts):
            pred["pts3D"] = point_block.head(self.scenepoint_head, pts)
        elif self.scenepoint_head_enabled:
            n_out = dense.sequential(self.scenepoint_head, F.relu(pts)).T
            pred["pts3D"] = torch.cat([n_out, torch.ones(1, n_out.shape[1], dtype=n_out.dtype, device=device)])
        return pred


class QuatPoseFn(torch.autograd.Function):
    """x [m, 7] -> [R(q) | t] [m, 3, 4] in one HIP kernel each way (csrc/pose_head.hip)."""

    @staticmethod
    def forward(ctx, x):
        from . import _native
        P = torch.empty((x.shape[0], 3, 4), dtype=torch.float32, device=x.device)
        _native.pose_fwd(x, P)
        ctx.save_for_backward(x)
        return P

    @staticmethod
    def backward(ctx, dP):
        from . import _native
        (x,) = ctx.saved_tensors
        dx = torch.empty((x.shape[0], 7), dtype=torch.float32, device=x.device)
        _native.pose_bwd(x, dP.contiguous(), dx)
        return dx


def rotation_6d_to_matrix(d6):
    """pytorch3d.transforms.rotation_6d_to_matrix (baseNet.py:43; published formula: Gram-Schmidt of
    the two 3-vectors, rows b1, b2, b1 x b2)."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = F.normalize(a1, dim=-1)
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


def project_to_rot(m):
    """geo_utils.project_to_rot (code/utils/geo_utils.py:25-31): the nearest rotation U diag(1, 1, det) V^T."""
    u, _, v = torch.svd(m)
    vt = v.transpose(1, 2)
    det = torch.det(u @ vt).view(-1, 1, 1)
    return u @ torch.cat((vt[:, :2, :], vt[:, -1:, :] * det), 1)


def quaternion_to_matrix(q):
    """Real-part-first quaternion -> rotation (the pytorch3d formula baseNet.py:48 calls)."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))
